// de_fast.hip — SECOND translation unit of libdigitalearth_hip.so: render_kernel_v6 compiled with -DDE_FAST_MATH semantics (de_math.h: the hardware's
// transcendental units and shorter polynomials instead of the arithmetic contract's fixed sequences), selected per context by DE_FLAG_FAST_MATH.
// Opt-in and NOT bit-reproducible against the CPU oracle (what bit-exactness costs, priced — profiles/r5_fast_math.md).
// Device code of the two units never meets (no relocatable device code); on the host side the kernel and its init kernel get their own names
// so that the two units' launch stubs stay apart.
#define DE_FAST_MATH 1
#define v6_kernel v6_kernel_fast_math
#define v6_init_kernel v6_init_kernel_fast_math
#include "de_stages.h"
#include "render_kernel_v6.hip"

// launched by de_launch.h: launch_v6 (the control words and RenderArgs are initialised there, by the contract unit's v6_init_kernel)
hipError_t de_fast_launch_v6(const bs::Args& A, const FrameConsts* fc, dim3 grid, dim3 block, hipStream_t stream, bool clamp, bool tail) {
    if (tail) {
        if (clamp) hipLaunchKernelGGL((v6_kernel<true, false, true>), grid, block, 0, stream, A, fc);
        else hipLaunchKernelGGL((v6_kernel<false, false, true>), grid, block, 0, stream, A, fc);
    } else {
        if (clamp) hipLaunchKernelGGL((v6_kernel<true, false, false>), grid, block, 0, stream, A, fc);
        else hipLaunchKernelGGL((v6_kernel<false, false, false>), grid, block, 0, stream, A, fc);
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ debug math
// aux_kernels.hip's math_kernel once more, in THIS unit: the same function numbers on the DE_FAST_MATH half of de_math.h (de_debug_math_fast; de_sqrt
// and the plain quotient are the compiler's IEEE sequences in both units).  For tests/test_gpu_fast_math_leaves.py.
__global__ void math_kernel_fast_math(int fn, const float* a, const float* b, float* out, size_t n) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    float x = a[k], y = b ? b[k] : 0.0f, r;
    switch (fn) {
        case 0: r = de_exp(x); break;
        case 1: r = de_log(x); break;
        case 2: r = de_sin(x); break;
        case 3: r = de_cos(x); break;
        case 4: r = de_atan2(x, y); break;
        case 5: r = de_asin(x); break;
        case 6: r = de_pow(x, y); break;
        case 7: r = x / y; break;
        case 8: r = de_sqrt(x); break;
        case 9: r = de_sqrt_nr(x); break;
        case 10: r = de_div_rc_ng(x, y, 1.0f / y); break;      // DE_DIVC_NG(x, c) with c given at run time: x * RN(1 / c)
        case 11: r = x * de_rcp_nr(y); break;
        case 12: r = de_log_unit(x); break;
        case 13: r = de_rcp_nr(x); break;
        case 14: r = de_exp_nonpos(x); break;
        case 15: { float s, c; de_sincos(x, &s, &c); r = s; break; }      // de_sincos's two outputs (the contract's math_kernel has no 15 / 16: de_sin / de_cos ARE its de_sincos)
        case 16: { float s, c; de_sincos(x, &s, &c); r = c; break; }
        default: r = 0.0f;
    }
    out[k] = r;
}

// launched by de_api.hip: de_debug_math_fast (device pointers, n > 0)
hipError_t de_fast_launch_math(int fn, const float* a, const float* b, float* out, size_t n, hipStream_t stream) {
    hipLaunchKernelGGL(math_kernel_fast_math, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, fn, a, b, out, n);
    return hipGetLastError();
}
