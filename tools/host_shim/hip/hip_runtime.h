/* hip/hip_runtime.h as a HOST build of the kernels' sources sees it (tools/local_exposure_host_check.py puts this directory on the include path, and
 * nothing else does): csrc/de_math.h includes <hip/hip_runtime.h>, and a sanitizer build with a plain C++ compiler has no HIP.  Only what de_math.h and
 * local_exposure_kernels.hip use: the qualifiers as nothing, the two vector types, and the two hardware estimates that de_math.h's refined square root
 * and reciprocal start from (not used by the code under test; plain divisions here). */
#ifndef DE_HOST_SHIM_HIP_RUNTIME_H
#define DE_HOST_SHIM_HIP_RUNTIME_H
#include <math.h>
#include <stdint.h>

#define __device__
#define __forceinline__ inline

struct float2 { float x, y; };
struct float4 { float x, y, z, w; };
static inline float2 make_float2(float x, float y) { float2 v; v.x = x; v.y = y; return v; }
static inline float4 make_float4(float x, float y, float z, float w) { float4 v; v.x = x; v.y = y; v.z = z; v.w = w; return v; }
static inline float __builtin_amdgcn_rsqf(float x) { return 1.0f / sqrtf(x); }
static inline float __builtin_amdgcn_rcpf(float x) { return 1.0f / x; }
#endif
