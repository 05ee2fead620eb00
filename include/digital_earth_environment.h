/* digital_earth_environment.h — the scene-linear panorama of libdigitalearth_hip.so: an HDR environment map as one OpenEXR file (same library,
 * ABI 6, additions only).
 *
 * The panorama of include/digital_earth_panorama.h resamples six cube faces BEHIND the display transform: tone-mapped, 0 ... 1.  The EXR output of
 * include/digital_earth_exr.h delivers scene-linear radiance, of the pinhole rectangle.  This header joins them: a SECOND set of six face slots
 * that hold the frame IN FRONT of the display, the same resampling arithmetic over them, and the unchanged EXR coder behind it.  The face cameras,
 * the apron, the projection, the size, the supersample and the basis are de_set_panorama's; the pixel type, the compression, the chunk size and
 * the scale are de_set_exr's.  A context that never calls de_environment_capture allocates and runs nothing new.
 *
 * THE LINEAR SLOTS.  Six slots of N x N x 3 float32 in the layout the display slots have, index (u N + v) 3 + c, v = 0 at the bottom.  The capture
 * kernel divides the sums ([N][N][3], rows v) by the frame's count — inside an adaptive frame by the 8 x 8 tile's own count —, one IEEE float32
 * division per channel, and transposes through an LDS tile.  The value of linear face k is therefore de_fetch_hdr() / (float)spp of face k's render,
 * bit for bit, in de_fetch_image's orientation.
 *
 * THE FILE.  While the panorama stage is on and all six linear slots are held, de_render_to_exr, de_fetch_exr, de_fetch_exr_view and
 * de_fetch_exr_begin / _end deliver ONE OpenEXR file of panorama.width x panorama.height, and de_exr_capacity answers for that size: the slots
 * resampled by the arithmetic of digital_earth_panorama.h, every rounded operation unchanged, into a row-major image that the EXR layout reads
 * with a divisor of 1 (x / 1.0f == x), top row first.  pixel_type, compression, chunk_bytes and scale are read at the fetch; `source` is read at the
 * CAPTURE, the slots are what they are.  With the stage on and fewer than six linear slots the EXR calls answer DE_ERR_STATE as they did before
 * this header existed; with the stage off nothing changes.  AOV channels (include/digital_earth_exr_aovs.h) do not exist in this mode: with
 * de_set_exr_aovs != 0 the calls answer DE_ERR_STATE.  The size limit is the EXR output's, width height 3 bps <= 2^27 (4096 x 2048 fits at half
 * and at float): DE_ERR_INVALID beyond it.  de_set_panorama answers DE_ERR_STATE while an EXR fetch begun with the stage on is in flight.
 *
 * HALF clamps at +-65504 (digital_earth_exr.h).  Where the sun's disc exceeds that in the mean's units the answer is de_exr.scale or
 * DE_EXR_PIXEL_FLOAT, not another clamp.
 */
#ifndef DIGITAL_EARTH_ENVIRONMENT_H
#define DIGITAL_EARTH_ENVIRONMENT_H
#include "digital_earth_panorama.h"
#include "digital_earth_exr.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The scene-linear twin of de_panorama_capture: the frame as it stands, in FRONT of the display, into linear slot `face`.  The slots are allocated
 * by the first call that succeeds.  What is captured is decided by de_exr.source at this moment:
 *   DE_EXR_SOURCE_MEAN        what de_fetch_exr reads with the stage off: the context's sums, the display source or the reduced frame, each channel
 *                             divided in float32 by the frame's count, inside an adaptive frame by the tile's own;
 *   DE_EXR_SOURCE_DENOISED    the image de_fetch_denoised_hdr hands out, with its refusals and its side effects;
 *   DE_EXR_SOURCE_HISTORY, _BLOOM, _LOCAL_EXPOSURE    DE_ERR_STATE: the history belongs to another face's camera, and the pyramids of the bloom
 *                             and of local exposure end at the face's border.
 * A vignette and auto-exposure do NOT refuse: they live behind the display.  DE_ERR_STATE while the panorama stage is off; DE_ERR_INVALID for a
 * face outside 0 ... 5.  A refused call changes nothing.  The library does not check the camera of a capture. */
int de_environment_capture(de_ctx* ctx, int face);
/* Bit k of *mask: linear slot k holds a face.  de_set_panorama clears this mask together with its own; de_reset keeps it. */
int de_environment_captured(de_ctx* ctx, uint32_t* mask);
/* Linear slot `face` as (N, N, 3) float32 in de_fetch_image's layout — a linear cube map face.  DE_ERR_STATE if that face is not held. */
int de_fetch_environment_face(de_ctx* ctx, int face, float* out);
/* The resampling and the EXR conversion once on six host-given linear faces, faces[6][n][n][3] as de_debug_panorama takes them (any n in
 * 4 ... 16384), with `panorama` as de_set_panorama and `exr` as de_set_exr take them (`on` and `source` are not read).  The file goes to `out`
 * (out_bytes of room), its length to *len — also when out_bytes is too small (DE_ERR_INVALID).  Buffers and tables of its own; the context's
 * settings and slots are untouched.  Every argument and setting refusal answers before the context is read. */
int de_debug_environment_exr(de_ctx* ctx, const float* faces, int n, const de_panorama* panorama, const de_exr* exr, void* out, uint64_t out_bytes, uint64_t* len);

#ifdef __cplusplus
}
#endif
#endif /* DIGITAL_EARTH_ENVIRONMENT_H */
