// ibl_tables.h — the host side of the IBL output (include/digital_earth_ibl.h), plain C++ with no HIP in it: the geometry of the chains,
// the settings' check, and the three things the header has the host compute in double and round once — a level's GGX sample table, the texel solid
// angles, the DDS front.  tools/ibl_host_check.cpp compiles it with ibl_body.h under the sanitizers.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#define IBL_MAX_LEVELS 11            // log2(1024) + 1
#define IBL_SH_EDGE 64
#define IBL_DDS_HEADER 148
#define IBL_MAX_PAYLOAD (1ull << 27)
#define IBL_PIXEL_HALF 1
#define IBL_PIXEL_FLOAT 2

// One kept sample of a specular level (the header's THE SAMPLE TABLE): 8 words, read by every lane at once.
struct IblSample { float hx, hy, hz, coef, frac; int32_t l0, l1, pad; };

static inline int ibl_log2(int v) { int n = 0; while ((1 << n) < v) ++n; return n; }
// texels of one face of levels 0 ... m - 1 of a chain of edge E
static inline size_t ibl_texels_before(int E, int m) { size_t s = 0; for (int q = 0; q < m; ++q) s += (size_t)(E >> q) * (size_t)(E >> q); return s; }
// floats in front of level m of a level-major chain, [level][6][e][e][3]
static inline size_t ibl_level_offset(int E, int m) { return ibl_texels_before(E, m) * 18; }
static inline size_t ibl_payload_bytes(int E, int L, int pixel_type) { return ibl_texels_before(E, L) * 6 * (pixel_type == IBL_PIXEL_HALF ? 8u : 16u); }

// nullptr: the settings are in range; else what is wrong (struct_bytes is the caller's to compare)
static inline const char* ibl_settings_fault(int edge, int levels, int samples, int supersample, float lod_bias, int pixel_type) {
    if (edge < 8 || edge > 1024 || (edge & (edge - 1)) != 0) return "de_ibl.edge must be a power of two in 8 ... 1024";
    if (levels < 2 || levels > ibl_log2(edge) + 1) return "de_ibl.levels must lie in 2 ... log2(edge) + 1";
    if (samples < 8 || samples > 1024 || (samples & (samples - 1)) != 0) return "de_ibl.samples must be a power of two in 8 ... 1024";
    if (supersample < 1 || supersample > 4) return "de_ibl.supersample must lie in 1 ... 4";
    if (!(lod_bias >= -1e30f && lod_bias <= 1e30f)) return "de_ibl.lod_bias must be finite";      // NaN fails both
    if (pixel_type != IBL_PIXEL_HALF && pixel_type != IBL_PIXEL_FLOAT) return "de_ibl.pixel_type must be DE_EXR_PIXEL_HALF or DE_EXR_PIXEL_FLOAT";
    if (ibl_payload_bytes(edge, levels, pixel_type) > IBL_MAX_PAYLOAD) return "de_ibl: the DDS payload must not exceed 2^27 bytes";
    return nullptr;
}

// The kept samples of specular level l (1 ... L - 1) of a bake with K samples, chain edge E and lod_bias, in table order.
static inline void ibl_build_samples(int E, int L, int K, int l, float lod_bias, std::vector<IblSample>* out) {
    const double pi = 3.14159265358979323846;
    const int M = ibl_log2(E) + 1;
    const double rho = (double)l / (double)(L - 1), alpha = rho * rho, a2 = alpha * alpha;
    const double omega_p = 4.0 * pi / (6.0 * (double)E * (double)E);
    double W = 0.0;
    out->clear();
    for (int k = 0; k < K; ++k) {
        uint32_t bits = (uint32_t)k, rev = 0;
        for (int b = 0; b < 32; ++b) { rev = (rev << 1) | (bits & 1u); bits >>= 1; }
        const double xi1 = ((double)k + 0.5) / (double)K, xi2 = (double)rev / 4294967296.0;
        const double c2 = (1.0 - xi1) / (1.0 + (a2 - 1.0) * xi1), ct = sqrt(c2), st = sqrt(1.0 - c2), phi = 2.0 * pi * xi2;
        const double w = 2.0 * c2 - 1.0;
        if (!(w > 0.0)) continue;
        const double d = c2 * (a2 - 1.0) + 1.0, D = a2 / (pi * d * d), pdf = D / 4.0, omega_s = 1.0 / ((double)K * pdf);
        double lod = 0.5 * log2(omega_s / omega_p);
        if (!(lod > 0.0)) lod = 0.0;
        lod += (double)lod_bias;
        if (!(lod > 0.0)) lod = 0.0;
        if (lod > (double)(M - 1)) lod = (double)(M - 1);
        IblSample s;
        s.l0 = (int32_t)floor(lod);
        s.frac = (float)(lod - (double)s.l0);
        if (s.l0 >= M - 1) { s.l0 = M - 1; s.frac = 0.0f; }
        s.l1 = s.l0 + 1 < M - 1 ? s.l0 + 1 : M - 1;
        s.pad = 0;
        W += w;
        s.hx = (float)(st * cos(phi)); s.hy = (float)(st * sin(phi)); s.hz = (float)ct; s.coef = (float)(w / W);
        out->push_back(s);
    }
}

// The solid angles of the texels of a face of edge es, [j][i], by the corner formula.
static inline void ibl_build_omega(int es, std::vector<float>* out) {
    auto A = [](double x, double y) { return atan2(x * y, sqrt(x * x + y * y + 1.0)); };
    out->resize((size_t)es * (size_t)es);
    for (int j = 0; j < es; ++j)
        for (int i = 0; i < es; ++i) {
            const double x0 = 2.0 * (double)i / (double)es - 1.0, x1 = 2.0 * (double)(i + 1) / (double)es - 1.0;
            const double y0 = 2.0 * (double)j / (double)es - 1.0, y1 = 2.0 * (double)(j + 1) / (double)es - 1.0;
            (*out)[(size_t)j * (size_t)es + (size_t)i] = (float)(A(x1, y1) - A(x0, y1) - A(x1, y0) + A(x0, y0));
        }
}

// The 148 bytes in front of the payload.
static inline void ibl_dds_header(int E, int L, int pixel_type, uint8_t* out) {
    uint32_t w[IBL_DDS_HEADER / 4];
    memset(w, 0, sizeof w);
    const uint32_t bpp = pixel_type == IBL_PIXEL_HALF ? 8u : 16u;
    w[0] = 0x20534444u;                       // "DDS "
    w[1] = 124u; w[2] = 0x0002100Fu;          // size; CAPS | HEIGHT | WIDTH | PITCH | PIXELFORMAT | MIPMAPCOUNT
    w[3] = (uint32_t)E; w[4] = (uint32_t)E; w[5] = (uint32_t)E * bpp; w[6] = 0u; w[7] = (uint32_t)L;
    w[19] = 32u; w[20] = 0x4u; w[21] = 0x30315844u;      // the pixel format: its size, DDPF_FOURCC, "DX10"
    w[27] = 0x00401008u;                      // COMPLEX | TEXTURE | MIPMAP
    w[28] = 0x0000FE00u;                      // CUBEMAP and all six faces
    w[32] = pixel_type == IBL_PIXEL_HALF ? 10u : 2u;     // DXGI_FORMAT_R16G16B16A16_FLOAT, _R32G32B32A32_FLOAT
    w[33] = 3u; w[34] = 0x4u; w[35] = 1u; w[36] = 0u;    // TEXTURE2D, TEXTURECUBE, one cube, alpha mode unknown
    for (int k = 0; k < IBL_DDS_HEADER / 4; ++k) { out[4 * k] = (uint8_t)w[k]; out[4 * k + 1] = (uint8_t)(w[k] >> 8); out[4 * k + 2] = (uint8_t)(w[k] >> 16); out[4 * k + 3] = (uint8_t)(w[k] >> 24); }
}
