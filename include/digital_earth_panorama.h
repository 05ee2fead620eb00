/* digital_earth_panorama.h — opt-in panorama output of libdigitalearth_hip.so (same library, ABI 6, additions only).
 *
 * The camera of include/digital_earth.h casts through a tangent plane of half-extent `fov`: a pinhole rectangle, no 180° view.  With W = H = N,
 * aspect_scale = 1 and fov = 1 the same camera is an exact 90° cube face, so a 360° frame is six ordinary renders and ONE resampling stage behind
 * the display, in the place output scaling has (include/digital_earth_output_scale.h): while the stage below is on and its six face slots are
 * filled, everything that hands out the DISPLAYED image — de_render_to_image, de_fetch_image*, de_output_size, de_render_to_pixels and the
 * de_fetch_pixels* calls, the HDR pixels, the video frames, the JPEG and the PNG calls — delivers `width` x `height`: the six captured faces
 * resampled on the GPU to an equirectangular frame or a fisheye dome master, and, for the packed and coded outputs, converted from that image by
 * their unchanged kernels.  The render kernels, de_params and everything ahead of the display know nothing of it.  While the stage is off, the
 * default, every call returns exactly the bytes it returned before this header existed.  Layouts are unchanged: floats (width, height, 3) with
 * the pixels of a column contiguous, index (i height + j) 3 + c, j = 0 at the bottom (v up, as the display writes).
 *
 * FACES.  The panorama's frame is basis[9] = r, u, f: its right, up and forward in world space.  Face 0 ... 5 = +r, -r, +u, -u, +f, -f:
 *     face   look   up            Every face is rendered with aspect_scale = 1 and fov = fl32(N / (N - 2 apron)): the inner N - 2 apron
 *     +r      r      u            pixels span exactly 90° and `apron` more pixels on every side lie beyond the cube's edge, so every
 *     -r     -r      u            bilinear tap of a direction that belongs to a face comes from that face's own render — the kernel never
 *     +u      u     -f            reads across a cube edge.  de_panorama_face_camera returns these cameras; the host sets one, resets,
 *     -u     -u      f            accumulates and calls de_panorama_capture, six times (Renderer.render_panorama).  The library does not
 *     +f      f      u            check the camera of a capture.
 *     -f     -f      u
 * Per face the library computes, in double from the float32 basis and rounded ONCE to float32, the axes the renderer derives for that camera,
 * du = normalize(look x up), dv = normalize(du x look), and from them four numbers m00 m01 m10 m11 = e1.du, e2.du, e1.dv, e2.dv, where e1, e2 are
 * the two basis vectors OTHER than the face's axis, in r, u, f order (for an exactly orthonormal basis each is 0 or +-1).
 *
 * THE KERNEL, all float32, every operation rounded on its own (no fma but inside de_sincos; no hardware transcendental): the arithmetic contract
 * of digital_earth.h.  Output pixel (i, j) takes S x S sub-positions, S = supersample; sub-position (a, b) has the sub-indices ki = i S + a and
 * kj = j S + b, that is x = i + (a + 0.5) / S, y = j + (b + 0.5) / S.
 *   direction, as components (cr, cu, cf) along r, u, f:
 *     DE_PANO_EQUIRECT   lon = (x / width - 0.5) 2 pi, lat = (y / height - 0.5) pi: four tables sin lon, cos lon [width S] and sin lat, cos lat
 *                        [height S], entry k at ((k + 0.5) / (n S) - 0.5) times 2 pi or pi, computed in double on the host and rounded once.
 *                        cr = cos lat * sin lon, cu = sin lat, cf = cos lat * cos lon.
 *     DE_PANO_FISHEYE    px = (float)(2 ki + 1) / (float)(width S) - 1, py likewise with kj and height (IEEE division);
 *                        rho = sqrt(px px + py py) correctly rounded; rho > 1: the sub-position's value is 0 in every channel;
 *                        theta = rho * fl32(aperture_deg pi / 360); (st, ct) = de_sincos(theta);
 *                        cr = st * (px / rho), cu = st * (py / rho), cf = ct; rho = 0 gives (0, 0, 1).
 *   face: the component of largest magnitude; ties go to r, then u, then f (|cr| >= |cu| and |cr| >= |cf|: r; else |cu| >= |cf|: u; else f);
 *     a negative component is the face's second half.  p, q = the OTHER two components, in r, u, f order, each divided by that magnitude (IEEE).
 *   in-face coordinates: fu = p * m00 + q * m01, fv = p * m10 + q * m11.
 *   pixel coordinates: X = (fu + fov) * fl32(N / (2 fov)) - 0.5, Y likewise — the exact inverse of the camera's cast at pixel centres,
 *     fu = 2 fov (X + 0.5) / N - fov.  The camera's cast also subtracts 1e-5 from fu and fv (8e-5 of a pixel at N = 16, less above): that offset
 *     is DROPPED here.
 *   taps: X and Y clamped to [0, N - 1] (NaN gives 0); i0 = min(floor(X), N - 2), ax = X - i0, the same along v; four taps of the face's slot.
 *   value, per channel: along u first, t0 = c00 + ax * (c10 - c00), t1 = c01 + ax * (c11 - c01) (c10: tap (i0 + 1, j0)); then t0 + ay * (t1 - t0).
 *   average: the sub-positions in the order a ascending inside b ascending (k = 1 ... S^2), as a running mean m_1 = v_1,
 *     m_k = m_(k-1) + (v_k - m_(k-1)) * fl32(1 / k).  (A sum of nine equal values times fl32(1 / 9) does not give the value back: 0.3 fails.  The
 *     running mean of equal values is that value.)  Hence a constant face gives exactly that constant at every S: black and a clipped 1.0 survive
 *     and DE_PIXELS_TRUNCATE still gives 255.
 * tests/panorama_ref.py restates all of this in numpy, and the GPU equals it bit for bit.
 *
 * EXR sits in front of the display, where these slots do not reach: the scene-linear panorama is include/digital_earth_environment.h's, a second set
 * of slots captured in front of the display (de_environment_capture).  Until all six of THOSE are held the EXR calls answer DE_ERR_STATE while the
 * stage is on.
 */
#ifndef DIGITAL_EARTH_PANORAMA_H
#define DIGITAL_EARTH_PANORAMA_H
#include "digital_earth.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DE_PANO_EQUIRECT 0   /* longitude along the width (-180° ... 180°, 0 at f, positive towards r), latitude along the height */
#define DE_PANO_FISHEYE 1    /* equidistant ("dome master"): the angle from f grows linearly with the radius, aperture_deg across the circle */
#define DE_PANO_FACES 6

typedef struct de_panorama {
    uint32_t struct_bytes;               /* sizeof(de_panorama) of the caller; checked like de_output_scale's */
    int32_t on;                          /* 0 (default): the stage is off */
    int32_t projection;                  /* DE_PANO_*; default DE_PANO_EQUIRECT */
    int32_t width, height;               /* the output size: width a multiple of 16, height of 8, width * height <= 2^28; DE_PANO_FISHEYE: width == height */
    float aperture_deg;                  /* DE_PANO_FISHEYE only (not read otherwise): (0, 360]; default 180 */
    int32_t apron;                       /* face pixels beyond 90° on every side: 1 ... N / 4; default 1 */
    int32_t supersample;                 /* S: 1 ... 4; default 2 */
    float basis[9];                      /* r, u, f in world space; orthonormal within 1e-4 (every |length^2 - 1| and every |dot|) */
} de_panorama;

/* Set the stage; on first use the context allocates six face slots of N x N x 3 float32 and the output.  Every call that succeeds CLEARS the six
 * slots (de_reset does not: the host resets between faces).  DE_ERR_INVALID: a mismatched struct_bytes, a field outside the table above, a basis
 * that is not orthonormal, or a context with W != H (a face camera is square; the settings are checked whether or not `on` is set).  DE_ERR_STATE:
 * `on` is set while output scaling is enabled (the two stages produce the shown image and a context has one; de_set_output_scale answers the same
 * while this stage is on), or a lagged fetch of the float image, the pixels, the video frames, the JPEG or the PNG output is in flight.  A refused call changes nothing. */
int de_set_panorama(de_ctx* ctx, const de_panorama* settings);
/* The current settings (before any de_set_panorama: off, DE_PANO_EQUIRECT, 0 x 0, 180, 1, 2, the identity basis). */
int de_get_panorama(de_ctx* ctx, de_panorama* out);
/* Host-only: the camera of face 0 ... 5 under the current settings, for a camera at pos[3].  look_at[k] = fl32(pos[k] + L look[k]) with
 * L = max(1, |pos|) in double (a unit step would vanish in float32 at planetary distances), up[3] = the table's up, *fov = fl32(N / (N - 2 apron)).
 * DE_ERR_INVALID for a face out of range or W != H. */
int de_panorama_face_camera(de_ctx* ctx, int face, const float* pos, float* look_at, float* up, float* fov);
/* Run de_render_to_image's chain as it stands — denoiser, manual exposure, display transform (SDR or HDR), look — and copy the displayed image,
 * ahead of any pack, into the slot of `face`.  DE_ERR_STATE while the stage is off, or while anything is on that would print the face's border into
 * the picture: vignette_strength != 0, auto-exposure, bloom, local exposure, history.  Otherwise de_render_to_image's own errors. */
int de_panorama_capture(de_ctx* ctx, int face);
/* Bit k of *mask: slot k holds a face.  The delivering calls answer DE_ERR_STATE while the stage is on with fewer than six; with six they run the
 * resampling kernel alone — the frame as it stands is not displayed, the shown image is a function of the slots. */
int de_panorama_captured(de_ctx* ctx, uint32_t* mask);

#ifdef __cplusplus
}
#endif
#endif /* DIGITAL_EARTH_PANORAMA_H */
