"""Headless `EarthViewer` / `Camera` — earth_viewer.py:23-318 without the GGUI window.

The reference's viewer is an interactive ti.ui window (WASD/mouse camera, sliders, 'i'/'o' config.txt save/load,
'p' screenshot).  A headless MI355X node has no window, so the class keeps the reference's names, camera math and
config-file format, and replaces the event loop by `render(spp)`:

    v = EarthViewer(config="config - florida.txt")   # or EarthViewer() for the default camera
    img = v.render(spp=256)                           # accumulate() x spp -> fetch_image()
    v.save("florida.png")
"""
import math
import os

import numpy as np

from . import luts, png16
from .renderer import Renderer

SCREEN_RES = (1920, 1080)      # earth_viewer.py:12
TARGET_FPS = 30                # earth_viewer.py:13
UP_DIR = (0, 1, 0)             # earth_viewer.py:14
planet_r = 6371e3              # lib/volume_rendering_models.py:34


def np_normalize(v):           # lib/math_utils.py:78-80
    return v / np.sqrt(np.sum(v ** 2))


def np_rotate_matrix(axis, theta):
    """lib/math_utils.py:83-102 — rotation matrix for a counter-clockwise rotation about `axis` by `theta` radians
    (Euler-Rodrigues formula).  The reference credits https://stackoverflow.com/a/6802723 for this helper; it is kept
    because SURVEY §8(f)-1 asks for the reference's Camera math."""
    axis = np_normalize(axis)
    a = math.cos(theta / 2.0)
    b, c, d = -axis * math.sin(theta / 2.0)
    aa, bb, cc, dd = a * a, b * b, c * c, d * d
    bc, ad, ac, ab, bd, cd = b * c, a * d, a * c, a * b, b * d, c * d
    return np.array([[aa + bb - cc - dd, 2 * (bc + ad), 2 * (bd - ac), 0],
                     [2 * (bc - ad), aa + cc - bb - dd, 2 * (cd + ab), 0],
                     [2 * (bd + ac), 2 * (cd - ab), aa + dd - bb - cc, 0],
                     [0, 0, 0, 1]])


class Config:
    """The 10-line preset the reference writes with 'i' and reads with 'o' (earth_viewer.py:100-126, 203-236):
    position, look_at, up (3 floats each), fov, aspect_scale, exposure, selected_crf, gamma, sun_angle, sun_path_rot."""

    def __init__(self, position, look_at, up, fov, aspect_scale, exposure, selected_crf, gamma, sun_angle, sun_path_rot):
        self.position = np.array(position, dtype=np.float64)
        self.look_at = np.array(look_at, dtype=np.float64)
        self.up = np.array(up, dtype=np.float64)
        self.fov, self.aspect_scale, self.exposure = float(fov), float(aspect_scale), float(exposure)
        self.selected_crf, self.gamma = int(selected_crf), float(gamma)
        self.sun_angle, self.sun_path_rot = float(sun_angle), float(sun_path_rot)

    def apply(self, renderer):
        renderer.set_camera_pos(*self.position)
        renderer.set_look_at(*self.look_at)
        renderer.set_up(*self.up)
        renderer.set_fov(self.fov)
        renderer.set_aspect_scale(self.aspect_scale)
        renderer.set_exposure(self.exposure)
        renderer.set_crf(self.selected_crf)
        renderer.set_gamma(self.gamma)
        renderer.set_sun_angle(self.sun_angle)
        renderer.set_sun_path_rot(self.sun_path_rot)

    def write(self, path):
        with open(path, "w") as f:
            for v in (self.position, self.look_at, self.up):
                f.write("%s %s %s\n" % (str(v[0]), str(v[1]), str(v[2])))
            f.write("\n".join(str(x) for x in (self.fov, self.aspect_scale, self.exposure, self.selected_crf, self.gamma,
                                               self.sun_angle)) + "\n")
            f.write(str(self.sun_path_rot))


def load_config(path):
    if not os.path.exists(path):
        alt = os.path.join(luts.CONFIG_DIR, path)
        if os.path.exists(alt):
            path = alt
    with open(path) as f:
        pos = [float(x) for x in f.readline().split()]
        look = [float(x) for x in f.readline().split()]
        up = [float(x) for x in f.readline().split()]
        fov = float(f.readline())
        aspect_scale = float(f.readline())
        exposure = float(f.readline())
        crf = int(f.readline())
        gamma = float(f.readline())
        sun_angle = float(f.readline())
        sun_path_rot = float(f.readline())
    return Config(pos, look, up, fov, aspect_scale, exposure, crf, gamma, sun_angle, sun_path_rot)


class Camera:
    """earth_viewer.py:23-163.  The window argument is kept for signature parity and may be None; movement that the
    reference reads from keys / the mouse is exposed as methods."""

    def __init__(self, window=None, up=UP_DIR):
        self._window = window
        self._lookat_pos = np.array((0.0, 0.0, 0.0))
        self._camera_pos = np.array((-15000000., 0.0, 15000000.))          # :27
        self._up = np_normalize(np.array(up, dtype=np.float64))
        self._last_mouse_pos = None
        self._moved = False

    @property
    def mouse_exclusive_owner(self):
        return True

    def set_up(self, new_up):
        self._up = new_up

    @property
    def position(self):
        return self._camera_pos

    @property
    def look_at(self):
        return self._lookat_pos

    @property
    def target_dir(self):
        return np_normalize(self.look_at - self.position)

    def _compute_cam_r(self):
        return np.sqrt(np.sum(self._camera_pos ** 2))

    def _compute_left_dir(self, tgtdir):                                   # :157-161
        cos = np.dot(self._up, tgtdir)
        if abs(cos) > 0.999:
            return np.array([-1.0, 0.0, 0.0])
        return np.cross(self._up, tgtdir)

    def rotate(self, dx, dy, scale=3):
        """_update_by_mouse (:43-67) for a cursor displacement (dx, dy)."""
        out_dir = self._lookat_pos - self._camera_pos
        leftdir = self._compute_left_dir(np_normalize(out_dir))
        rotx = np_rotate_matrix(self._up, dx * scale)
        roty = np_rotate_matrix(leftdir, dy * scale)
        out_dir_homo = np.array(list(out_dir) + [0.0])
        new_out_dir = np.matmul(np.matmul(roty, rotx), out_dir_homo)[:3]
        self._lookat_pos = self._camera_pos + new_out_dir
        self._moved = True
        return True

    def move(self, direction, elapsed_time, shift=False):
        """_update_by_wasd (:72-144) for a summed key direction vector."""
        d = np.array(direction, dtype=np.float64) * 0.05
        speed = 30.0 * max(min(self._compute_cam_r() - planet_r, planet_r * 0.5), 0.0)
        if shift:
            speed *= 3.0
        cam_step = d * speed * elapsed_time
        self._lookat_pos += cam_step
        self._camera_pos += cam_step
        if self._compute_cam_r() < planet_r * 1.000:
            self._lookat_pos -= cam_step * 2
            self._camera_pos -= cam_step * 2
        self._moved = True
        return True

    def update_camera(self, elapsed_time):
        """earth_viewer.py:146-155: True when the camera changed since the last call.  No input devices on a headless node:
        changes come from rotate() / move() / load()."""
        moved, self._moved = self._moved, False
        return moved

    def load(self, cfg):
        self._camera_pos = cfg.position.copy()
        self._lookat_pos = cfg.look_at.copy()
        self._up = cfg.up.copy()
        self._moved = True


def _rgb_picture(px):
    """(H, W, 3 | 4) uint8 rows top-down -> the image writer's RGB picture.  The writer's own unpacker reads the bytes (RGBA8 as RGBX: the alpha byte is
    dropped, so the file is the one an RGB array gives whatever the channel count); no numpy pass over the pixels."""
    from PIL import Image
    h, w, ch = px.shape
    return Image.frombytes("RGB", (w, h), np.ascontiguousarray(px).tobytes(), "raw", "RGBX" if ch == 4 else "RGB", 0, 1)


class EarthViewer:
    """earth_viewer.py:166-318, headless."""

    def __init__(self, config=None, screen_res=SCREEN_RES, history=None, local_exposure=None, output_res=None, output_filter="lanczos3", hdr_output=None, look=None, look_strength=1.0, exr_aovs=(), panorama=None, ibl_bc6h=None, **renderer_kwargs):
        """history: None / False (off), True (Renderer.set_history's defaults) or a dict of its keywords — the picture then survives camera moves
        in frame()'s loop instead of restarting at one sample per pixel.  local_exposure: the same for Renderer.set_local_exposure — every frame is
        dodged and burned on the GPU ahead of the display transform.  output_res: None, or the (width, height) at which frames are delivered and
        saved while screen_res is rendered (Renderer.set_output_scale with `output_filter`): a supersampled still, or a window larger than the render.
        hdr_output: None / False, True (Renderer.set_hdr_output's defaults: 1000-nit Rec.2020 PQ) or a dict of its keywords — frames are then the HDR
        signal, frame(hdr_pixels=True) hands out 10 / 16-bit pixels and save() writes a 16-bit PNG that names its colour space.
        look: None, the path of a 3D .cube file or a digital_earth_amd.cube.Cube — every frame is graded through it on the GPU behind the display
        transform, mixed with the ungraded frame by look_strength (Renderer.set_look; a shaper or trilinear interpolation: call that directly).
        exr_aovs: names of channel groups ("depth", "normal", "albedo", "coverage", "transmittance", "variance", "samples", or "all") that
        save("x.exr"), frame(exr=True) and record("f%05d.exr") write beside B, G, R (Renderer.set_exr's aovs).
        panorama: None / False, True (Renderer.set_panorama's defaults: a 4 N x 2 N equirectangular frame) or a dict of its keywords — screen_res must
        be square, (N, N), and the vignette is turned off (it would print every face's border); frame(panorama=True) then renders the six cube faces around the camera and hands out the 360° frame, and save() and
        record() write it through the writers as they are.
        ibl_bc6h: None / False, True (Renderer.set_ibl_bc6h's defaults: quality 0) or a dict of its keywords — save("x.dds") and
        frame(panorama=True, ibl=True) then deliver the IBL cube map as BC6H_UF16 blocks (Renderer.fetch_ibl_bc6h_dds) instead of half floats."""
        self.window = None
        self.camera = Camera(self.window, up=UP_DIR)
        self.renderer = Renderer(image_res=screen_res, up=UP_DIR, **renderer_kwargs)
        self.renderer.set_camera_pos(*self.camera.position)
        self.renderer.copy_textures()
        if history:
            self.renderer.set_history(True, **(history if isinstance(history, dict) else {}))
        if local_exposure:
            self.renderer.set_local_exposure(True, **(local_exposure if isinstance(local_exposure, dict) else {}))
        if output_res is not None:
            self.renderer.set_output_scale(tuple(output_res), filter=output_filter)
        if hdr_output:
            self.renderer.set_hdr_output(True, **(hdr_output if isinstance(hdr_output, dict) else {}))
        if look is not None:
            self.renderer.set_look(look, strength=look_strength)
        if exr_aovs:
            self.renderer.set_exr(aovs=exr_aovs)
        if panorama:
            self.renderer.vignette_strength = 0.0      # a vignette would darken every face's border: a capture under one is refused
            self.renderer.set_panorama(**(panorama if isinstance(panorama, dict) else {}))
        if ibl_bc6h:
            self.renderer.set_ibl_bc6h(True, **(ibl_bc6h if isinstance(ibl_bc6h, dict) else {}))
        self.config = None
        if config is not None:
            self.load_config(config)
        self._image = None
        self._pixels = None                     # the picture of the last frame(pixels=True)
        self._held_hdr = None                   # Renderer.hdr_output when the picture held was taken: what save() labels it with
        self._hdr_in_flight = {False: [], True: []}      # the same per lagged fetch in flight (float ring, pixel ring), oldest first
        self._sliders = None

    def load_config(self, path_or_config):
        cfg = path_or_config if isinstance(path_or_config, Config) else load_config(path_or_config)
        self.config = cfg
        self.camera.load(cfg)
        self.camera.update_camera(0.0)          # the renderer gets the camera right here
        cfg.apply(self.renderer)
        self._sliders = None                    # 'o' re-reads the slider values from the file (:213-236)
        self.renderer.reset_framebuffer()

    def save_config(self, path):
        r = self.renderer
        Config(self.camera.position, self.camera.look_at, self.camera._up, r.fov[None], r.aspect_scale[None], r.exposure[None],
               r.selected_crf[None], r.gamma[None], r.sun_angle[None], r.sun_path_rot[None]).write(path)

    def render(self, spp=1, chunk=64):
        """The body of the reference loop (:241-243): accumulate() spp times, then fetch_image()."""
        left = int(spp)
        while left > 0:
            n = min(left, chunk)
            self.renderer.accumulate(n)
            left -= n
        self._image = self.renderer.fetch_image()
        self._pixels, self._held_hdr = None, self.renderer.hdr_output
        return self._image

    def render_to_noise(self, threshold, max_spp, min_spp=16, round_spp=16, floor=None):
        """Adaptive sampling (Renderer.render_adaptive): a NEW frame in which every 8x8 tile is rendered until its noise converges — its standard error
        below `threshold` times the luminance, floored at `floor` (default Renderer's ADAPTIVE_FLOOR) — or until `max_spp`.  Returns the image;
        self.last_adaptive holds dict(rounds, pixel_samples, mean_spp)."""
        r = self.renderer
        r.reset_framebuffer()
        kw = {} if floor is None else {"floor": floor}
        self.last_adaptive = r.render_adaptive(threshold, max_spp, min_spp=min_spp, round_spp=round_spp, **kw)
        self._image = r.fetch_image()
        self._pixels, self._held_hdr = None, r.hdr_output
        return self._image

    def frame(self, spp=1, copy=True, pipelined=False, pixels=False, **sliders):
        """ONE iteration of the reference's window loop (earth_viewer.py:203-317), with the GUI sliders passed as keywords
        (sun_angle, sun_path_rot, fov, aspect_scale, exposure, selected_crf, gamma):
          1. a moved camera is pushed to the renderer and marks the framebuffer for reset          (:206-213)
          2. accumulate() x spp, fetch_image() — with the parameters of the PREVIOUS iteration     (:241-243)
          3. slider changes: sun angle / sun path rotation / fov / aspect scale mark the framebuffer for reset;
             exposure, camera response and gamma do not (display-only)                            (:268-305)
          4. the scalars are written to the renderer, then the reset happens                       (:308-317)
        Returns the displayed image of step 2 (copy=False: a read-only view that the next frame() overwrites — what a canvas needs).
        pipelined=True (or 2: two frames of lag): the display and the host copy of this frame are only enqueued (Renderer.fetch_image(lag=...)) and the
        image RETURNED is the previous iteration's (None in the first): the next iteration's accumulate() renders while this frame is shown — the same images, one
        iteration later, at a fraction of the frame time; finish() returns the last one.
        pixels=True: the iteration returns the packed 8-bit picture instead of the float field — (H, W, channels) uint8, rows top-down, converted on the
        GPU in the format of Renderer.set_pixels() (Renderer.fetch_pixels) — with the same copy / pipelined rules; finish(pixels=True) ends that loop.
        hdr_pixels=True (a keyword beside the sliders, none of them): the iteration returns the packed HDR pixels of Renderer.fetch_hdr_pixels() — uint32
        (H, W) or uint16 (H, W, 3) — always a copy, never pipelined: these pixels have no ring.  The HDR display output must be on.
        video=True (a keyword beside the sliders too): the iteration returns one video frame in the format of Renderer.set_video() — a flat
        uint8 array, Renderer.fetch_video — under the same copy / pipelined rules as pixels=True, through the video ring; finish(video=True)
        ends that loop.  It goes with neither pixels=True nor hdr_pixels=True, and the picture save() holds is left as it was.
        jpeg=True (a keyword beside the sliders too): the iteration returns one complete JPEG file in the settings of Renderer.set_jpeg() — bytes, or a
        memoryview with copy=False; Renderer.fetch_jpeg — under the same rules as video=True, through the JPEG ring; finish(jpeg=True) ends that
        loop.  It goes with none of pixels=True, hdr_pixels=True and video=True.
        png=True (a keyword beside the sliders too): the same for one complete PNG file in the settings of Renderer.set_png() — Renderer.fetch_png,
        through the PNG ring; finish_png() ends that loop.  It goes with none of the others.
        exr=True (a keyword beside the sliders too): the same for one complete OpenEXR file of the scene-linear frame in the settings of
        Renderer.set_exr() — Renderer.fetch_exr, through the EXR ring; finish_exr() ends that loop.  It goes with none of the others.
        rgbe=True (a keyword beside the sliders too): the same for one complete Radiance .hdr file (RGBE) of the scene-linear frame in the settings
        of Renderer.set_rgbe() — Renderer.fetch_rgbe, through the RGBE ring; finish_rgbe() ends that loop.  It goes with none of the others; with
        panorama=True it is the 360° environment map, as exr=True.
        panorama=True (a keyword beside the sliders too; the viewer was made with panorama=...): step 2 is Renderer.render_panorama(spp) — the six
        cube faces around the camera, `spp` each, never accumulated over iterations — and what is handed out (the float field, or with pixels /
        hdr_pixels / video / jpeg / png = True that output, pipelined or not) is the 360° frame at Renderer.output_size() — so
        record(path, n, panorama=True) writes a 360° Y4M, Motion-JPEG or PNG sequence through the writers as they are.  With exr=True step 2 is
        Renderer.render_environment(spp) instead — the same six renders captured in FRONT of the display — and the file handed out, through the EXR
        ring when pipelined, is the scene-linear 360° frame, an HDR environment map: record("env/%05d.exr", n, panorama=True) writes a sequence.
        ibl=True with panorama=True (it goes with no other output and not with pipelined): step 2 is Renderer.render_environment(spp) and
        Renderer.build_ibl() behind it, and what is handed out is Renderer.fetch_ibl_dds(): the GGX-prefiltered cube map as one DDS file, in the
        settings of Renderer.set_ibl(); Renderer.fetch_ibl_sh() holds the irradiance's SH coefficients of the same bake."""
        r = self.renderer
        hdr_pixels = bool(sliders.pop("hdr_pixels", False))
        video = bool(sliders.pop("video", False))
        jpeg = bool(sliders.pop("jpeg", False))
        png = bool(sliders.pop("png", False))
        exr = bool(sliders.pop("exr", False))
        rgbe = bool(sliders.pop("rgbe", False))
        panorama = bool(sliders.pop("panorama", False))
        ibl = bool(sliders.pop("ibl", False))
        if ibl and (not panorama or pipelined or pixels or hdr_pixels or video or jpeg or png or exr or rgbe):
            raise ValueError("ibl=True needs panorama=True and goes with no other output and not with pipelined")
        if rgbe and (pixels or hdr_pixels or video or jpeg or png or exr):
            raise ValueError("rgbe=True goes with none of pixels=True, hdr_pixels=True, video=True, jpeg=True, png=True and exr=True")
        if exr and (pixels or hdr_pixels or video or jpeg or png):
            raise ValueError("exr=True goes with none of pixels=True, hdr_pixels=True, video=True, jpeg=True and png=True")
        if png and (pixels or hdr_pixels or video or jpeg):
            raise ValueError("png=True goes with none of pixels=True, hdr_pixels=True, video=True and jpeg=True")
        if jpeg and (pixels or hdr_pixels or video):
            raise ValueError("jpeg=True goes with none of pixels=True, hdr_pixels=True and video=True")
        if hdr_pixels and (pixels or pipelined):
            raise ValueError("hdr_pixels=True goes with neither pixels=True nor pipelined")
        if video and (pixels or hdr_pixels):
            raise ValueError("video=True goes with neither pixels=True nor hdr_pixels=True")
        should_reset = False
        if self.camera.update_camera(0.0):
            r.set_camera_pos(*self.camera.position)
            r.set_look_at(*self.camera.look_at)
            r.set_up(*self.camera._up)
            should_reset = True
        if panorama and (exr or rgbe or ibl):
            r.render_environment(int(spp))      # the same six renders, captured in front of the display (include/digital_earth_environment.h)
        elif panorama:
            r.render_panorama(int(spp))         # six faces around the camera, `spp` each; the camera is put back and the frame left empty
        else:
            r.accumulate(int(spp))              # == accumulate() x spp, bit for bit
        frame = None
        if ibl:
            r.build_ibl()
            frame = r.fetch_ibl_bc6h_dds() if r.ibl_bc6h["on"] else r.fetch_ibl_dds()
        elif rgbe:
            frame = r.fetch_rgbe(copy=copy, lag=int(pipelined))
        elif exr:
            frame = r.fetch_exr(copy=copy, lag=int(pipelined))
        elif png:
            frame = r.fetch_png(copy=copy, lag=int(pipelined))
        elif jpeg:
            frame = r.fetch_jpeg(copy=copy, lag=int(pipelined))
        elif video:
            frame = r.fetch_video(copy=copy, lag=int(pipelined))
        elif hdr_pixels:
            self._pixels, self._image = r.fetch_hdr_pixels(), None
        elif pixels:
            self._pixels, self._image = r.fetch_pixels(copy=copy, lag=int(pipelined)), None
        else:
            self._image = r.fetch_image(copy=copy, lag=int(pipelined))
            self._pixels = None
        # The settings this picture was displayed with (read before the sliders below).  A pipelined iteration returns an EARLIER iteration's picture:
        # the settings travel through a queue of their own, one entry per fetch in flight, so that save() labels each picture as it was taken.
        shown = self._pixels if (pixels or hdr_pixels) else self._image
        if video or jpeg or png or exr or rgbe or ibl:
            pass                                # no picture of save()'s changed hands
        elif pipelined:
            self._hdr_in_flight[bool(pixels)].append(r.hdr_output)
            if shown is not None:
                self._held_hdr = self._hdr_in_flight[bool(pixels)].pop(0)
        else:
            self._held_hdr = r.hdr_output
        if self._sliders is None:               # current_* of earth_viewer.py:191-199, read once when the loop starts
            self._sliders = {"sun_angle": r.sun_angle[None], "sun_path_rot": r.sun_path_rot[None], "fov": r.fov[None],
                             "aspect_scale": r.aspect_scale[None], "exposure": r.exposure[None],
                             "selected_crf": r.selected_crf[None], "gamma": r.gamma[None]}
        cur = self._sliders
        for k, v in sliders.items():
            if k not in cur:
                raise TypeError("unknown slider %r" % k)
            if v != cur[k]:
                if k in ("sun_angle", "sun_path_rot", "fov", "aspect_scale"):
                    should_reset = True
                cur[k] = v
        r.sun_angle[None] = cur["sun_angle"]; r.sun_path_rot[None] = cur["sun_path_rot"]
        r.fov[None] = cur["fov"]; r.aspect_scale[None] = cur["aspect_scale"]
        r.exposure[None] = cur["exposure"]; r.gamma[None] = cur["gamma"]; r.selected_crf[None] = cur["selected_crf"]
        if should_reset:
            r.reset_framebuffer()
        if video or jpeg or png or exr or rgbe or ibl:
            return frame
        return self._pixels if (pixels or hdr_pixels) else self._image

    def _record_jpeg(self, path, n, spp, fps, sliders_per_frame):
        """record()'s Motion-JPEG side: frame(jpeg=True) through the pipelined JPEG ring into an AVI (.avi) or the bare concatenation (.mjpeg)."""
        from . import mjpeg
        r = self.renderer
        size = r.jpeg()["size"]
        w = mjpeg.AVIWriter(path, size[0], size[1], fps=fps) if path.endswith(".avi") else mjpeg.MJPEGWriter(path)
        try:
            for i in range(n):
                now = {k: (v[i] if hasattr(v, "__len__") else v) for k, v in sliders_per_frame.items()}
                got = self.frame(spp=spp, copy=False, pipelined=1, jpeg=True, **now)
                if got is not None:
                    w.write(got)
                del got
            for got in r.fetch_pending_jpeg(all_images=True):
                w.write(got)
        finally:
            w.close()
        return w.frames

    def _record_png(self, path, n, spp, sliders_per_frame, exr=False, rgbe=False):
        """record()'s lossless side: frame(png=True) through the pipelined PNG ring into the numbered files path % 0, path % 1, ...; exr=True: the
        scene-linear side, frame(exr=True) through the EXR ring; rgbe=True: frame(rgbe=True) through the RGBE ring."""
        r = self.renderer
        written = 0
        which = {"rgbe": True} if rgbe else {"exr": True} if exr else {"png": True}

        def write(got):
            nonlocal written
            with open(path % written, "wb") as f:
                f.write(got)
            written += 1
        for i in range(n):
            now = {k: (v[i] if hasattr(v, "__len__") else v) for k, v in sliders_per_frame.items()}
            got = self.frame(spp=spp, copy=False, pipelined=1, **which, **now)
            if got is not None:
                write(got)
            del got
        for got in (r.fetch_pending_rgbe if rgbe else r.fetch_pending_exr if exr else r.fetch_pending_png)(all_images=True):
            write(got)
        return written

    def record(self, path, frames, spp=1, fps=(TARGET_FPS, 1), **sliders_per_frame):
        """Write `frames` iterations of frame(video=True) to `path` as a Y4M file (digital_earth_amd/y4m.py) that every player opens, through the
        pipelined video ring: the GPU renders frame k + 1 while frame k is packed, copied and written.  The video output must be planar — "i420" or
        "i010" (Renderer.set_video; ValueError otherwise, before anything is rendered or written).  Every slider keyword is either a value, held
        for the whole recording, or a sequence of one value per frame (a sun angle per frame is a time-lapse); move the camera between calls, or
        record in several calls.  Returns the number of frames written.
        A path ending in `.avi` writes a Motion-JPEG AVI instead (digital_earth_amd/mjpeg.py) and one ending in `.mjpeg` the concatenated JPEG files,
        both from frame(jpeg=True) through the pipelined JPEG ring, in the settings of Renderer.set_jpeg().
        A path ending in `.png` is a pattern with one integer field ("frames/%05d.png"): a numbered lossless sequence, one complete PNG file per
        frame from frame(png=True) through the pipelined PNG ring, in the settings of Renderer.set_png() (frames count from 0; `fps` is not used).
        A path ending in `.exr` is such a pattern too ("frames/%05d.exr"): one complete OpenEXR file of the scene-linear frame per iteration, from
        frame(exr=True) through the pipelined EXR ring, in the settings of Renderer.set_exr().
        A path ending in `.hdr` is such a pattern too ("frames/%05d.hdr"): one complete Radiance RGBE file per iteration, from frame(rgbe=True)
        through the pipelined RGBE ring, in the settings of Renderer.set_rgbe() (the defaults if that was never called)."""
        from . import y4m
        r = self.renderer
        n = int(frames)
        for k, v in sliders_per_frame.items():
            if hasattr(v, "__len__") and len(v) != n:
                raise ValueError("slider %r has %d values for %d frames" % (k, len(v), n))
        if path.endswith((".avi", ".mjpeg")):
            return self._record_jpeg(path, n, spp, fps, sliders_per_frame)
        if path.endswith((".png", ".exr", ".hdr")):
            suffix = path[-4:]
            try:
                numbered = path % 0 != path % 1
            except (TypeError, ValueError):
                numbered = False
            if not numbered:
                raise ValueError("a %s recording needs a pattern with one integer field, such as frames/%%05d%s" % (suffix, suffix))
            return self._record_png(path, n, spp, sliders_per_frame, exr=suffix == ".exr", rgbe=suffix == ".hdr")
        fmt = r.video()
        w = y4m.Y4MWriter(path, fmt["size"][0], fmt["size"][1], fps=fps, format=fmt["format"], range=fmt["range"], siting=fmt["siting"])
        try:
            for i in range(n):
                now = {k: (v[i] if hasattr(v, "__len__") else v) for k, v in sliders_per_frame.items()}
                got = self.frame(spp=spp, copy=False, pipelined=1, video=True, **now)
                if got is not None:
                    w.write(got)
                del got
            for got in r.fetch_pending(all_images=True, video=True):
                w.write(got)
        finally:
            w.close()
        return w.frames

    def finish_png(self, copy=True):
        """End a pipelined frame(png=True) loop: the file of its last iteration (None when nothing is in flight).  A method of its own, as
        Renderer.fetch_pending_jpeg is: finish()'s signature is pinned."""
        return self.renderer.fetch_pending_png(copy=copy)

    def finish_exr(self, copy=True):
        """End a pipelined frame(exr=True) loop: the file of its last iteration (None when nothing is in flight)."""
        return self.renderer.fetch_pending_exr(copy=copy)

    def finish_rgbe(self, copy=True):
        """End a pipelined frame(rgbe=True) loop: the file of its last iteration (None when nothing is in flight)."""
        return self.renderer.fetch_pending_rgbe(copy=copy)

    def finish(self, copy=True, pixels=False, video=False, jpeg=False):
        """End a pipelined loop: the image of the last frame() iteration (None when nothing is in flight); pixels=True: of a frame(pixels=True) loop;
        video=True: the frame of a frame(video=True) loop; jpeg=True: the file of a frame(jpeg=True) loop.  (A frame(png=True) loop ends in finish_png().)"""
        if jpeg:
            return self.renderer.fetch_pending_jpeg(copy=copy)
        if video:
            return self.renderer.fetch_pending(copy=copy, video=True)
        img = self.renderer.fetch_pending(copy=copy, pixels=pixels)
        queue = self._hdr_in_flight[bool(pixels)]
        if img is not None and queue:
            self._held_hdr = queue[-1]          # the newest fetch's picture is the one handed out
        del queue[:]
        if img is not None:
            if pixels:
                self._pixels = img
            else:
                self._image = img
        return img

    def close(self):
        """Release the renderer.  A zero-copy image kept from frame(copy=False) is copied first: it lives in the renderer's staging buffer."""
        if self._image is not None and getattr(self._image, "_owner", None) is not None:
            self._image = np.array(self._image)
        if self._pixels is not None and getattr(self._pixels, "_owner", None) is not None:
            self._pixels = np.array(self._pixels)
        self.renderer.close()

    def save(self, path):
        """'p' screenshot (:244-250): writes the displayed image, at the output size when output_res is set; `.npy` keeps the float (W, H, 3) array.  Every other format gets packed 8-bit pixels
        converted on the GPU in the renderer's current mode (Renderer.set_pixels; truncation by default: the reference's to_vec3u, byte for byte) and
        handed to the image writer as they are, rows top-down — no clip, cast, transpose or flip on the host.  What is written is the picture this
        viewer last showed, never a new display of the context: the image held goes through the pack kernel as it is (Renderer.debug_pixels), and
        after frame(pixels=True) the picture held is written.  A slider, bloom or exposure changed since then does not reach the file.
        A picture taken while the HDR display output was on (render, frame, frame(hdr_pixels=True)) is written, for every format but `.npy`, as a
        16-bit RGB PNG with a cICP chunk naming the gamut and the transfer it was TAKEN with (colour primaries 1 / 12 / 9, transfer 8 / 16 / 18 for
        linear / PQ / HLG, RGB, full range; digital_earth_amd/png16.py).  Here too nothing is displayed again and no setting or dither phase of the
        renderer is touched: "rgb16" pixels are written as they are, "rgb10a2" codes widened to 16 bits by bit replication, and a float signal held
        from render() / frame() is quantised on the host by rounding (png16.to_rgb16) — the setting's mode and dither belong to fetch_hdr_pixels().
        Under the P3-D65 and Rec.2020 gamuts the label names the container, not a colorimetric picture: see Renderer.set_hdr_output.
        `.jpg` / `.jpeg` with a float image held (render, frame) and the HDR output off: the file is the GPU encoder's (Renderer.debug_jpeg on the
        image held, in the settings of Renderer.set_jpeg) — no host encoder; with packed pixels held the image writer encodes them as before.
        `.png` once Renderer.set_png() has been called: the same picture under the same rules — the pixels held, or the image held through the pack
        kernel at the phase it was shown with — filtered and deflated by the GPU's encoder (Renderer.debug_png, in the filter and chunk size of
        set_png); a picture taken with the HDR output on is the 16-bit file with the cICP chunk of the setting it was taken with.  Without
        set_png() the file is written the way it was before, byte for byte.
        `.exr`: not a picture held but the scene-linear frame of the CURRENT accumulation, as one OpenEXR file converted and deflated on the GPU
        (Renderer.fetch_exr) in the settings of Renderer.set_exr(), or the defaults (half, ZIP, the mean) if that was never called; a sample is
        rendered first if the frame holds none.  digital_earth_amd.exr.read opens it again.  Behind frame(panorama=True, exr=True) or
        Renderer.render_environment() the file is whatever fetch_exr() delivers then: the scene-linear panorama.
        `.hdr` once Renderer.set_rgbe() has been called: the same scene-linear frame as one Radiance RGBE file, converted and run-length coded on the
        GPU (Renderer.fetch_rgbe) in the settings of set_rgbe(); digital_earth_amd.rgbe.read opens it again.  Without set_rgbe() the extension is
        what it was before: one the image writer does not know.
        `.dds` while a panorama with all six linear faces is held (frame(panorama=True, exr / rgbe / ibl = True), Renderer.render_environment()): the
        IBL bake of those faces in the settings of Renderer.set_ibl() (Renderer.build_ibl, fetch_ibl_dds), a GGX-prefiltered cube map with the DX10
        header; digital_earth_amd.dds.read opens it again.  Otherwise the extension is one the image writer does not know."""
        r = self.renderer
        if path.endswith(".dds") and r.panorama["on"] and len(r.environment["captured"]) == 6:
            r.build_ibl()
            with open(path, "wb") as f:
                f.write(r.fetch_ibl_bc6h_dds() if r.ibl_bc6h["on"] else r.fetch_ibl_dds())
            return
        if path.endswith(".hdr") and r.rgbe_is_set:
            if r.current_spp == 0 and not (r.panorama["on"] and len(r.environment["captured"]) == 6):
                self.render(1)
            with open(path, "wb") as f:
                f.write(r.fetch_rgbe())
            return
        if path.endswith(".exr"):
            if r.current_spp == 0 and not (r.panorama["on"] and len(r.environment["captured"]) == 6):      # the panorama is made of its slots, not of the frame
                self.render(1)
            with open(path, "wb") as f:
                f.write(r.fetch_exr())
            return
        if self._image is None and self._pixels is None:
            self.render(1)
        if path.endswith(".npy"):
            np.save(path, self._image if self._image is not None else r.fetch_image())
            return
        hdr = self._held_hdr
        gpu_png = path.endswith(".png") and r.png_is_set
        if gpu_png:
            fmt = r.png()
            if hdr is not None:
                held = self._pixels if self._pixels is not None else np.asarray(self._image, dtype=np.float32)
                data = r.debug_png(np.ascontiguousarray(png16.to_rgb16(held)), filter=fmt["filter"], chunk_bytes=fmt["chunk_bytes"],
                                   cicp=png16.cicp_of(hdr["gamut"], hdr["transfer"]))
            else:
                px = self._pixels
                if px is None:
                    pf = r.pixels()
                    px = r.debug_pixels(self._image, channels=pf["channels"], mode=pf["mode"], seed=pf["seed"], phase=pf["last_phase"])
                data = r.debug_png(px, filter=fmt["filter"], chunk_bytes=fmt["chunk_bytes"])
            with open(path, "wb") as f:
                f.write(data)
            return
        if hdr is not None:
            held = self._pixels if self._pixels is not None else np.asarray(self._image, dtype=np.float32)
            png16.write_png16(path, png16.to_rgb16(held), png16.cicp_of(hdr["gamut"], hdr["transfer"]))
            return
        if path.endswith((".jpg", ".jpeg")) and self._image is not None:      # the GPU's encoder on the image held, in the settings of set_jpeg()
            fmt = r.jpeg()
            with open(path, "wb") as f:
                f.write(r.debug_jpeg(self._image, quality=fmt["quality"], restart=fmt["restart"]))
            return
        px = self._pixels
        if px is None:
            fmt = r.pixels()
            px = r.debug_pixels(self._image, channels=fmt["channels"], mode=fmt["mode"], seed=fmt["seed"], phase=fmt["last_phase"])
        _rgb_picture(px).save(path)

    def start(self, spp=64, out="screenshot/earth.png", noise=None, denoise=False, auto_exposure=False):
        """Reference entry point (main.py:4).  Headless: render one frame and save it.  noise=None: `spp` samples per pixel; noise = a threshold:
        adaptive sampling up to `spp` per pixel (render_to_noise).  denoise=True: the saved image is the denoised one (Renderer.set_denoise, turned on
        before the frame starts so that it has the per-pixel variance).  auto_exposure=True: the saved image is exposed by the GPU meter
        (Renderer.set_auto_exposure, default settings) instead of the configuration's hand-set exposure."""
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        if auto_exposure:
            self.renderer.set_auto_exposure(True)
        if denoise:
            self.renderer.set_denoise(True)
            self.renderer.reset_framebuffer()
        if noise is not None:
            self.render_to_noise(float(noise), int(spp))
        else:
            self.render(spp)
        self.save(out)
        return out
