// display_source.h — what the display launch is about to read, stated once for every stage that runs ahead of it (the meter, the bloom, the history
// blend, local exposure): the buffer, its divisor, and how a group of four pixels and a luminance are taken from it.  Device code only; the includer
// brings DE_DEV, the vector types and <stdint.h> (de_kernels.h, or a host build of one kernel file alone: tools/host_shim, tools/*_host_check.cpp).
#pragma once

struct DisplaySrc {
    const float* hdr;           // [H][W][3]: DisplayArgs::hdr
    const int32_t* tile_spp;    // [H/8][W/8] when the display divides every tile by its own count (display_kernel<true>), else null
    int samples;                // DisplayArgs::samples
    int W, H;
};

// Twelve floats = 4 pixels of a row.  VEC: the buffer is 16-byte aligned (the context's own always are; a bound buffer or a display source may not be).
template <bool VEC>
DE_DEV void src_load4(const float* p, float* px) {
    if (VEC) {
        const float4 v0 = reinterpret_cast<const float4*>(p)[0], v1 = reinterpret_cast<const float4*>(p)[1], v2 = reinterpret_cast<const float4*>(p)[2];
        px[0] = v0.x; px[1] = v0.y; px[2] = v0.z; px[3] = v0.w; px[4] = v1.x; px[5] = v1.y; px[6] = v1.z; px[7] = v1.w;
        px[8] = v2.x; px[9] = v2.y; px[10] = v2.z; px[11] = v2.w;
    } else {
        for (int k = 0; k < 12; ++k) px[k] = p[k];
    }
}

// display_pixel's own sample count for pixel (i, j) (a group of 4 pixels lies in one 8x8 tile)
DE_DEV float src_samples(const DisplaySrc& s, int i, int j) {
    return s.tile_spp ? (float)s.tile_spp[(j >> 3) * (s.W >> 3) + (i >> 3)] : (float)s.samples;
}

// Rec.709 luminance of a mean, in the meter's association: every stage that thresholds or weighs by luminance sees the meter's value.  No vignette:
// the scene is metered, not the lens.
DE_DEV float src_luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
