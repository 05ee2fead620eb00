"""`Renderer` — the host-side operator API of the reference (renderer.py:15-401), bound to the gfx950 library.

Method and attribute names, argument meaning and call order are the reference's:

    r = Renderer(image_res=(1920, 1080), up=(0, 1, 0))      # renderer.py:17
    r.set_camera_pos(x, y, z); r.set_look_at(...)            # :225-266
    r.copy_textures()                                        # :136
    r.accumulate()                                           # :371   (1 sample per pixel, current_spp += 1)
    img = r.fetch_image()                                    # :382   (W, H, 3) float32 in [0, 1]
    r.fov[None] = 0.2                                        # scalar fields keep Taichi's [None] indexing

All device work happens in libdigitalearth_hip.so through ctypes (digital_earth_amd/_native.py).  There is no
Taichi and no CPU implementation in this package.
"""
import ctypes
import weakref
import os

import numpy as np

from . import _native, luts, textures as tex
from ._native import DeParams, DeCounters, DeAdaptive, DeDenoise, DeAutoExposure, DeMetering, DeBloom, DeHistory, DePixels, DeOutputScale, DePanorama, DeLocalExposure, DeHdrOutput, DeVideo, DeLook, DeJpeg, DePng, DeExr, DeRgbe, DeIbl, DeIblBc6h, DigitalEarthError, check

# Default luminance floor of the adaptive noise test (accumulate_adaptive), in HDR units (per-pixel mean of the color_buffer sums).  Measured on the MI355X
# with tools/adaptive_price.py --luminance (the four BASELINE views at a quarter of their size, 64 spp; profiles/adaptive.md): the Rec.709 luminance of the
# pixels that show the Earth or its atmosphere has its 10th percentile at 0.018 / 0.013 / 0.0027 / 0.0085 (default camera, florida, sunset hurricane,
# Apollo 11; median 0.011) and its median at 0.033 / 0.022 / 0.016 / 0.024.  0.01 sits at about the dark tenth of the lit pixels: darker pixels (night
# side, deep shadow, space) are held to an absolute standard error of threshold x 0.01 instead of a relative one that would never be reached near zero.
ADAPTIVE_FLOOR = 0.01


class _ScalarField:
    """Stand-in for a 0-d ti.field: `field[None]` reads, `field[None] = v` writes (earth_viewer.py:191-199,308-314)."""

    def __init__(self, owner, name, cast):
        # a weak reference: the Renderer must be freed (and with it its device memory: up to tens of GB of pipeline queues) the
        # moment the last user reference goes, not at the garbage collector's next cycle sweep
        self._owner, self._name, self._cast = weakref.proxy(owner), name, cast

    def __getitem__(self, key):
        return self._cast(getattr(self._owner._params, self._name))

    def __setitem__(self, key, value):
        setattr(self._owner._params, self._name, self._cast(value))
        self._owner._push_params()


class _VectorField:
    def __init__(self, owner, name):
        self._owner, self._name = weakref.proxy(owner), name

    def __getitem__(self, key):
        return np.array(list(getattr(self._owner._params, self._name)), dtype=np.float32)

    def __setitem__(self, key, value):
        arr = getattr(self._owner._params, self._name)
        for i in range(3):
            arr[i] = float(value[i])
        self._owner._push_params()


class _StagingView(np.ndarray):
    """fetch_image(copy=False): a read-only window on the library's pinned staging buffer.  Overwritten by the next fetch_* call of its
    Renderer; holds a reference to that Renderer so that garbage collection cannot free the buffer under it."""
    _owner = None

    def __array_finalize__(self, obj):
        self._owner = getattr(obj, "_owner", None)


class _FetchRing:
    """One output's fetches (csrc/de_fetch.h is the native side): synchronous, into a fresh array or as a view of the library's staging buffer, and
    lagged through the output's ring of four.  Holds what the lag protocol needs: the fetches in flight, what `capture` answered at the newest begin
    (the setters that would change it are refused while fetches are in flight: it holds for every one of them) and a weak reference to the last view
    handed out, so that close() can refuse while it is referenced.  `array(ptr, captured)` is the output's shape rule, a method of the Renderer
    (_staging_view, _pixel_view, _vd_view): the array over the library's buffer at `ptr`, or a fresh one of that shape (ptr None).  The Renderer
    and its method are passed in, not kept: no reference cycle."""

    def __init__(self, lib, stem, fetch, ctype, capture, name, busy):
        self._begin, self._end, self._view, self._fetch = (getattr(lib, n) for n in (stem + "_begin", stem + "_end", stem + "_view", fetch))
        self._sized = len(self._fetch.argtypes) == 3      # de_fetch_pixels / de_fetch_video take the size of `out`
        self._ctype, self._capture, self.name, self._busy = ctype, capture, name, busy
        self.in_flight, self.captured, self.view_ref = 0, None, None

    def view(self, r, array, ptr, captured):
        view = array(ptr, captured).view(_StagingView)
        view.flags.writeable = False
        view._owner = r                            # the memory belongs to the context: the view keeps its Renderer alive ...
        self.view_ref = weakref.ref(view)          # ... and close() refuses while the view is
        return view

    def fetch(self, r, array, copy, lag):
        if not r._textures_copied:
            r.copy_textures()
        if lag not in (0, 1, 2, 3):
            raise ValueError("lag must be 0 ... 3")
        captured = self._capture(r)
        if lag:
            check(self._begin(r._h))
            self.in_flight += 1
            self.captured = captured
            return None if self.in_flight <= lag else self.end(r, array, copy)
        if self.in_flight:
            raise RuntimeError(self._busy)
        if not copy:
            ptr = ctypes.POINTER(self._ctype)()
            check(self._view(r._h, ctypes.byref(ptr)))
            return self.view(r, array, ptr, captured)
        out = array(None, captured)
        check(self._fetch(r._h, out.ctypes.data, *((ctypes.c_uint64(out.nbytes),) if self._sized else ())))
        return out

    def end(self, r, array, copy):
        ptr = ctypes.POINTER(self._ctype)()
        self.in_flight -= 1
        check(self._end(r._h, ctypes.byref(ptr)))
        view = self.view(r, array, ptr, self.captured)
        return np.array(view) if copy else view

    def referenced(self):
        return self.view_ref is not None and self.view_ref() is not None


class _CodedFetch:
    """One coded output's fetches (fetch_jpeg, fetch_png, fetch_exr, fetch_rgbe; csrc/de_fetch.h's CodedOut is the native side): a whole file whose length the device
    decides, as bytes or as a view of the library's pinned buffer, synchronous or lagged through the output's ring of four.  Parametrised by the
    output: its library functions, its noun, and the names of its two attributes of the Renderer — the lagged fetches in flight (`_jp_in_flight`,
    `_pn_in_flight`) and a weak reference to the last view handed out (close() refuses while it is referenced).  The Renderer is passed in, not kept."""

    def __init__(self, lib, stem, noun, prefix):
        self._view, self._begin, self._end = (getattr(lib, "de_fetch_%s_%s" % (stem, n)) for n in ("view", "begin", "end"))
        self._render_to = getattr(lib, "de_render_to_" + stem)
        self.stem, self._noun, self._counter, self._ref = stem, noun, prefix + "_in_flight", prefix + "_view_ref"

    def in_flight(self, r, change=0):
        setattr(r, self._counter, getattr(r, self._counter) + change)
        return getattr(r, self._counter)

    def referenced(self, r):
        ref = getattr(r, self._ref)
        return ref is not None and ref() is not None

    def view(self, r, ptr, n, copy):
        if copy:
            return ctypes.string_at(ptr, n)
        view = np.ctypeslib.as_array(ptr, shape=(n,)).view(_StagingView)
        view.flags.writeable = False
        view._owner = r
        setattr(r, self._ref, weakref.ref(view))
        return memoryview(view)

    def end(self, r, copy):
        ptr, n = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64()
        self.in_flight(r, -1)
        check(self._end(r._h, ctypes.byref(ptr), ctypes.byref(n)))
        return self.view(r, ptr, int(n.value), copy)

    def fetch(self, r, copy, lag):
        if not r._textures_copied:
            r.copy_textures()
        if lag not in (0, 1, 2, 3):
            raise ValueError("lag must be 0 ... 3")
        if lag:
            check(self._begin(r._h))
            return None if self.in_flight(r, +1) <= lag else self.end(r, copy)
        if self.in_flight(r):
            raise RuntimeError("lagged %s fetches are in flight: fetch_pending_%s() first" % (self._noun, self.stem))
        ptr, n = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64()
        check(self._view(r._h, ctypes.byref(ptr), ctypes.byref(n)))
        return self.view(r, ptr, int(n.value), copy)

    def pending(self, r, copy, all_images):
        imgs = []
        while self.in_flight(r) > 0:
            imgs.append(self.end(r, copy or all_images))
        return imgs if all_images else (imgs[-1] if imgs else None)

    def render_to(self, r):
        if not r._textures_copied:
            r.copy_textures()
        p, n = ctypes.c_void_p(), ctypes.c_void_p()
        check(self._render_to(r._h, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value


class Renderer:
    """GPU implementation of the reference `Renderer` (renderer.py:15-401).

    Extra keyword arguments (no reference counterpart):
      device          HIP device index (one context = one GPU)
      texture_source  "auto": image files from `texture_dir` when present, else synthetic stand-ins;
                      "files": image files only (FileNotFoundError like the reference when absent);
                      "synthetic": procedural maps generated on the GPU (the reference ships no maps, README.md:31-32);
                      "constant": 1x1 maps (BASELINE cfg1: flat albedo, no topography, no clouds)
      texture_quality 0/1/2 — lib/textures.py:1 (resolutions of the tier are used for synthetic maps too)
      texture_size    override (w, h) for every synthetic map, or {slot: (w, h)} per map (tests)
      cloud_heavy     synthetic cloud variant of BASELINE cfg4
      seed            base seed of the per-sample RNG streams
    """

    def __init__(self, image_res, up, device=0, texture_source="auto", texture_dir=None,
                 texture_quality=tex.TEXTURE_QUALITY, texture_size=None, cloud_heavy=False, seed=0,
                 synth_seed=tex.SYNTH_SEED):
        self._lib = _native.load()
        self.image_res = (int(image_res[0]), int(image_res[1]))
        self.aspect_ratio = image_res[0] / image_res[1]                  # renderer.py:19
        self.current_spp = 0                                             # :23
        self.seed = int(seed)
        self.tile_rank, self.tile_world = 0, 1
        self._h = ctypes.c_void_p()
        self._image_ring = _FetchRing(self._lib, "de_fetch_image", "de_fetch_image", ctypes.c_float, lambda r: None, "fetch_image",
                                      "lagged fetches are in flight: fetch_pending() first")
        self._pixel_ring = _FetchRing(self._lib, "de_fetch_pixels", "de_fetch_pixels", ctypes.c_uint8, lambda r: r.pixels()["channels"], "fetch_pixels",
                                      "lagged pixel fetches are in flight: fetch_pending(pixels=True) first")
        self._vd_ring = _FetchRing(self._lib, "de_fetch_videoframe", "de_fetch_video", ctypes.c_uint8, Renderer._vd_bytes, "fetch_video",
                                   "lagged video fetches are in flight: fetch_pending(video=True) first")
        self._jp_coded, self._pn_coded = _CodedFetch(self._lib, "jpeg", "JPEG", "_jp"), _CodedFetch(self._lib, "png", "PNG", "_pn")
        self._jp_in_flight, self._jp_view_ref = 0, None      # the lagged fetch_jpeg() calls; the last view handed out
        self._pn_in_flight, self._pn_view_ref, self._png_set = 0, None, False      # the same for fetch_png(); set_png() has been called
        self._ex_coded, self._ex_in_flight, self._ex_view_ref = _CodedFetch(self._lib, "exr", "EXR", "_ex"), 0, None      # the same for fetch_exr()
        self._rg_coded, self._rg_in_flight, self._rg_view_ref, self._rgbe_set = _CodedFetch(self._lib, "rgbe", "RGBE", "_rg"), 0, None, False      # the same for fetch_rgbe(); set_rgbe() has been called
        check(self._lib.de_create(int(device), self.image_res[0], self.image_res[1], ctypes.byref(self._h)))
        _native.apply_env_tuning(self._h)      # experiment overrides (DE_KERNEL, DE_V6_* ...): read HERE, not in the library
        self._params = DeParams()
        check(self._lib.de_get_params(self._h, ctypes.byref(self._params)))   # reference defaults, renderer.py:20-22,49-58

        self.fov = _ScalarField(self, "fov", float)                      # :27
        self.aspect_scale = _ScalarField(self, "aspect_scale", float)    # :28
        self.exposure = _ScalarField(self, "exposure", float)            # :30
        self.selected_crf = _ScalarField(self, "selected_crf", int)      # :31
        self.gamma = _ScalarField(self, "gamma", float)                  # :33
        self.sun_angle = _ScalarField(self, "sun_angle", float)          # :36
        self.sun_path_rot = _ScalarField(self, "sun_path_rot", float)    # :37
        self.camera_pos = _VectorField(self, "camera_pos")               # :39
        self.look_at = _VectorField(self, "look_at")                     # :40
        self.up = _VectorField(self, "up")                               # :41

        self.set_up(*up)                                                 # :49
        self.set_fov(np.radians(27.) * 0.5)                              # :50
        self.set_aspect_scale(1.0)
        self.set_exposure(2.5)
        self.set_gamma(1.0)
        self.set_crf(0)
        self.set_sun_angle(np.radians(60.0))
        self.set_sun_path_rot(np.radians(-45.0))

        # textures (renderer.py:60-94): staged here, sent to the device by copy_textures()
        self._texture_plan = self._plan_textures(texture_source, texture_dir, texture_quality, texture_size,
                                                 cloud_heavy, synth_seed)
        self._textures_copied = False
        self._bound = None           # (tensor, stream) kept alive while the context points at them (parallel.DistributedFrame)
        self._adaptive = None        # the current adaptive frame's outputs after its last round (accumulate_adaptive); None in a uniform frame

        # LUTs (renderer.py:96-134)
        self.crf_names = []
        crf_array = self.load_crfs()
        self.crf_lut_res = (1024, len(self.crf_names))
        self._luts = (luts.load_cie(), luts.load_srgb2spec(), luts.load_o3(), crf_array)
        self.set_crf_count(self.crf_lut_res[1])

    # ------------------------------------------------------------------ lifetime
    def close(self):
        """de_destroy.  Fails (DigitalEarthError, DE_ERR_STATE) while another Renderer still borrows this one's maps, and (RuntimeError)
        while a zero-copy image of fetch_image(copy=False) is still referenced: that array IS the context's pinned staging buffer."""
        if getattr(self, "_h", None):
            for ring in (self._image_ring, self._pixel_ring, self._vd_ring):
                if ring.referenced():
                    raise RuntimeError("a %s(copy=False) view of this Renderer is still referenced: drop it (or copy it) before close()" % ring.name)
            for coded in (self._jp_coded, self._pn_coded, self._ex_coded, self._rg_coded):
                if coded.referenced(self):
                    raise RuntimeError("a fetch_%s(copy=False) view of this Renderer is still referenced: drop it (or copy it) before close()" % coded.stem)
            check(self._lib.de_destroy(self._h))
            self._h = ctypes.c_void_p()
            self._lender = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ attributes kept from the reference
    @property
    def vignette_strength(self):
        return self._params.vignette_strength

    @vignette_strength.setter
    def vignette_strength(self, v):
        self._params.vignette_strength = float(v)
        self._push_params()

    @property
    def vignette_radius(self):
        return self._params.vignette_radius

    @vignette_radius.setter
    def vignette_radius(self, v):
        self._params.vignette_radius = float(v)
        self._push_params()

    @property
    def vignette_center(self):
        return [self._params.vignette_center[0], self._params.vignette_center[1]]

    @vignette_center.setter
    def vignette_center(self, v):
        self._params.vignette_center[0], self._params.vignette_center[1] = float(v[0]), float(v[1])
        self._push_params()

    @property
    def land_height_scale(self):
        return self._params.land_height_scale

    @land_height_scale.setter
    def land_height_scale(self, v):
        self._params.land_height_scale = float(v)
        self._push_params()

    @property
    def color_buffer(self):
        """HDR accumulation as a (W, H, 3) float32 array (renderer.py:25,330)."""
        return self.fetch_hdr()

    def _push_params(self):
        check(self._lib.de_set_params(self._h, ctypes.byref(self._params)))

    # ------------------------------------------------------------------ textures
    def _plan_textures(self, source, texture_dir, quality, size, cloud_heavy, synth_seed):
        table = tex.texture_table(quality)
        if source in ("auto", "files"):
            d = texture_dir or tex.find_texture_dir()
            have = d is not None and all(os.path.exists(os.path.join(d, table[s][0])) for s in table)
            if have:
                return [("file", s, os.path.join(d, table[s][0])) for s in range(7)]
            if source == "files":
                raise FileNotFoundError("texture files %s not found in %r (the reference expects them under textures/, "
                                        "README.md:31-32)" % ([table[s][0] for s in table], d))
            source = "synthetic"
        if source == "synthetic":
            plan = []
            for s in range(7):
                w, h = (size[s] if isinstance(size, dict) else size) if size is not None else table[s][1]
                plan.append(("synthetic", s, (int(w), int(h), int(synth_seed), 1 if cloud_heavy else 0)))
            return plan
        if source == "constant":
            return [("array", s, tex.constant_texels(s, (128, 128, 128) if s == tex.ALBEDO else 0)) for s in range(7)]
        raise ValueError("texture_source must be auto, files, synthetic or constant")

    def set_texture(self, slot, texels):
        """Replace one map by a uint8 array [height][width][channels] (row 0 = south)."""
        self._texture_plan[slot] = ("array", slot, np.ascontiguousarray(texels, dtype=np.uint8))
        if self._textures_copied:
            self._copy_one(self._texture_plan[slot])

    def _copy_one(self, item):
        kind, slot, arg = item
        if kind == "synthetic":
            w, h, seed, variant = arg
            check(self._lib.de_generate_texture(self._h, slot, w, h, seed, variant))
            return
        arr = tex.load_image_texels(arg, tex.SLOT_CHANNELS[slot]) if kind == "file" else arg
        h, w, ch = arr.shape
        check(self._lib.de_upload_texture(self._h, slot, arr.ctypes.data, w, h, ch))

    def copy_textures(self):
        """renderer.py:136-145 — the nine copy_* upload kernels (7 maps + CIE + CRF)."""
        for item in self._texture_plan:
            self._copy_one(item)
        cie, s2s, o3, crf = self._luts
        check(self._lib.de_upload_luts(self._h, cie.ctypes.data, s2s.ctypes.data, o3.ctypes.data, crf.ctypes.data,
                                       crf.shape[1]))
        self._textures_copied = True

    def copy_texture(self, slot):
        """Send ONE map of this renderer's own texture plan to the device.  After share_textures_from() this makes the renderer the owner
        of that map while it keeps borrowing the others (a second view of the same Earth under another cloud cover: BASELINE cfg4's
        cloud-heavy variant differs from the default in the cloud map alone)."""
        self._copy_one(self._texture_plan[slot])
        self._own_slots = getattr(self, "_own_slots", set()) | {int(slot)}

    def share_textures_from(self, other):
        """Use `other`'s device-resident maps and LUTs (same GPU) instead of uploading / generating copies: a second
        frame in flight costs no second 9 GB.  Keeps a reference to `other` so it outlives this renderer."""
        if not other._textures_copied:
            other.copy_textures()
        check(self._lib.de_share_textures(self._h, other._h))
        self._lender = other
        self._own_slots = set()
        self._textures_copied = True

    def trim_textures(self):
        """Free the as-uploaded copies of the maps (2.1 GB at quality 2); the kernels keep their packed copies."""
        if not self._textures_copied:
            self.copy_textures()
        check(self._lib.de_trim_textures(self._h))

    def download_texture(self, slot):
        """The map as uploaded.  A borrower (share_textures_from) holds no as-uploaded copy: the owner's is returned."""
        if getattr(self, "_lender", None) is not None and int(slot) not in getattr(self, "_own_slots", ()):
            return self._lender.download_texture(slot)
        w, h, ch = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(self._lib.de_texture_info(self._h, slot, ctypes.byref(w), ctypes.byref(h), ctypes.byref(ch)))
        out = np.zeros((h.value, w.value, ch.value), dtype=np.uint8)
        check(self._lib.de_download_texture(self._h, slot, out.ctypes.data, out.nbytes))
        return out

    def load_crfs(self):
        """renderer.py:147-167 — (1024, n, 3) float32; fills self.crf_names (Neutral.rf first, then sorted: Q10)."""
        names, arr = luts.load_crfs()
        self.crf_names = list(names)
        return arr

    # ------------------------------------------------------------------ setters, renderer.py:224-266
    def set_camera_pos(self, x, y, z):
        self._params.camera_pos[0], self._params.camera_pos[1], self._params.camera_pos[2] = float(x), float(y), float(z)
        self._push_params()

    def set_up(self, x, y, z):
        v = np.array([x, y, z], dtype=np.float32)
        # ti.Vector.normalized() in f32 (taichi/lang/matrix.py): invlen = 1 / norm; invlen * v — checked against the value the
        # reference's set_up kernel stores (tests/golden/ref_frames_*.npz, tests/test_gpu_ref_fixtures.py)
        v = (np.float32(1.0) / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])) * v
        self._params.up[0], self._params.up[1], self._params.up[2] = float(v[0]), float(v[1]), float(v[2])
        self._push_params()

    def set_look_at(self, x, y, z):
        self._params.look_at[0], self._params.look_at[1], self._params.look_at[2] = float(x), float(y), float(z)
        self._push_params()

    def set_fov(self, fov):
        self._params.fov = float(fov)
        self._push_params()

    def set_aspect_scale(self, scale):
        self._params.aspect_scale = float(scale)
        self._push_params()

    def set_exposure(self, exposure):
        self._params.exposure = float(exposure)
        self._push_params()

    def set_gamma(self, gam):
        self._params.gamma = float(gam)
        self._push_params()

    def set_crf(self, index):
        self._params.selected_crf = int(index)
        self._push_params()

    def set_crf_count(self, num):
        self._crf_count = int(num)       # the device takes the count from the uploaded CRF array (renderer.py:257)

    def set_sun_angle(self, ang):
        self._params.sun_angle = float(ang)
        self._push_params()

    def set_sun_path_rot(self, ang):
        self._params.sun_path_rot = float(ang)
        self._push_params()

    # extensions of the scalar state (include/digital_earth.h: de_params.flags)
    def set_fixed_wavelength(self, nm):
        """BASELINE cfg1: trace a single wavelength instead of sampling one per path (None to disable)."""
        if nm is None:
            self._params.flags &= ~_native.DE_FLAG_FIXED_WAVELENGTH
        else:
            self._params.flags |= _native.DE_FLAG_FIXED_WAVELENGTH
            self._params.fixed_wavelength = float(nm)
        self._push_params()

    def set_flag(self, flag, on):
        if on:
            self._params.flags |= flag
        else:
            self._params.flags &= ~flag
        self._push_params()

    def set_integrator(self, name):
        """'path_tracer' (pathtracer.py:316, what the reference runs) or 'ray_marcher' (pathtracer.py:544)."""
        if name not in ("path_tracer", "ray_marcher"):
            raise ValueError(name)
        self.set_flag(_native.DE_FLAG_RAY_MARCHER, name == "ray_marcher")

    def set_display_transform(self, name):
        """'opendrt' (what the reference runs: OpenDRT + camera response + gamma, renderer.py:357-362) or 'agx'
        (the alternative kept behind a comment at renderer.py:356, lib/AgX.py)."""
        if name not in ("opendrt", "agx"):
            raise ValueError(name)
        self.set_flag(_native.DE_FLAG_AGX, name == "agx")

    def set_fast_math(self, on=True):
        """OPT-IN (DE_FLAG_FAST_MATH): path_tracer on the hardware's transcendental units instead of the arithmetic contract's fixed sequences.
        Faster (profiles/r5_fast_math.md) and no longer bit-reproducible against the CPU oracle: a sample whose collision test lands on the other
        side follows a different path, so images agree with the contract's statistically, not sample by sample."""
        self.set_flag(_native.DE_FLAG_FAST_MATH, bool(on))

    def set_topo_res_override(self, res):
        self._params.topo_res_override = int(res)
        self._push_params()

    def set_tile_partition(self, rank, world):
        """Multi-GPU: this context renders only the 8x8 tiles (tx, ty) with (tx + ty) % world == rank."""
        if not (0 <= rank < world):
            raise ValueError("rank %d not in [0, %d)" % (rank, world))
        self.tile_rank, self.tile_world = int(rank), int(world)

    def set_sample_partition(self, rank, world):
        """Multi-GPU, the other split: this context renders, of the frame's sample indices, those = rank (mod world) of every
        pixel it owns; accumulate(spp) still advances the frame's sample counter by spp.  The ranks' buffers are then partial sums of every
        pixel: assemble them with reduce_ordered / parallel.reduce_hdr_ordered (rank-ordered additions), not with a plain sum-reduce."""
        if not (0 <= rank < world):
            raise ValueError("rank %d not in [0, %d)" % (rank, world))
        check(self._lib.de_set_sample_partition(self._h, int(rank), int(world)))
        self.sample_rank, self.sample_world = int(rank), int(world)

    # ------------------------------------------------------------------ frame loop, renderer.py:367-384
    def reset_framebuffer(self):
        self.current_spp = 0
        check(self._lib.de_reset(self._h))
        self._adaptive = None

    def accumulate(self, spp=1):
        """renderer.py:371-380, `spp` times in one launch (the reference's accumulate() is spp = 1)."""
        if not self._textures_copied:
            self.copy_textures()
        check(self._lib.de_accumulate(self._h, int(spp), self.seed, self.tile_rank, self.tile_world))
        self.current_spp += int(spp)

    # ------------------------------------------------------------------ adaptive sampling (include/digital_earth.h: de_accumulate_adaptive)
    def accumulate_adaptive(self, threshold, max_spp, min_spp=16, round_spp=16, floor=ADAPTIVE_FLOOR):
        """One round of an adaptive frame: every 8x8 tile still active gets `round_spp` more samples (never past `max_spp`), then the tiles whose
        noise has converged leave.  A tile stays while some pixel's standard error, in some channel, exceeds `threshold` times the pixel's luminance
        floored at `floor` (HDR units); it stops at `max_spp` at the latest.  A tile that stopped at n samples holds the bits of a uniform n-spp frame.
        The first call after reset_framebuffer() starts the frame; threshold, spp settings, floor and seed stay fixed until the next reset.
        Returns the number of tiles still active (0: the frame is finished; further calls render nothing).  current_spp follows the largest tile
        count; tile_spp() has every tile's."""
        if not self._textures_copied:
            self.copy_textures()
        if self.tile_world > 1:
            raise DigitalEarthError(_native.DE_ERR_STATE, "an adaptive frame covers the whole image: no tile partition")
        W, H = self.image_res
        counts = np.empty((H // 8, W // 8), dtype=np.int32)
        io = DeAdaptive()
        io.struct_bytes = ctypes.sizeof(DeAdaptive)
        io.threshold, io.floor = float(threshold), float(floor)
        io.min_spp, io.max_spp, io.round_spp = int(min_spp), int(max_spp), int(round_spp)
        io.tile_spp = counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        check(self._lib.de_accumulate_adaptive(self._h, ctypes.c_uint64(self.seed), ctypes.byref(io)))
        self._adaptive = dict(active_tiles=int(io.active_tiles), rounds=int(io.rounds), pixel_samples=int(io.pixel_samples), tile_spp=counts)
        spp = ctypes.c_int()
        check(self._lib.de_current_spp(self._h, ctypes.byref(spp)))
        self.current_spp = int(spp.value)
        return int(io.active_tiles)

    def render_adaptive(self, threshold, max_spp, min_spp=16, round_spp=16, floor=ADAPTIVE_FLOOR):
        """accumulate_adaptive() until no tile is active.  Returns dict(rounds, pixel_samples, mean_spp) — mean_spp = pixel_samples / (W H)."""
        while self.accumulate_adaptive(threshold, max_spp, min_spp=min_spp, round_spp=round_spp, floor=floor) > 0:
            pass
        a = self._adaptive
        return dict(rounds=a["rounds"], pixel_samples=a["pixel_samples"], mean_spp=a["pixel_samples"] / float(self.image_res[0] * self.image_res[1]))

    def tile_spp(self):
        """Samples per 8x8 tile, int32 (W/8, H/8) in fetch_image's (u, v) orientation: the adaptive frame's counts after its last round, or
        current_spp everywhere in a uniform frame."""
        W, H = self.image_res
        if getattr(self, "_adaptive", None) is None:
            return np.full((W // 8, H // 8), self.current_spp, dtype=np.int32)
        return np.ascontiguousarray(self._adaptive["tile_spp"].T)

    def adaptive_moments(self):
        """Per-pixel sums of squares of the last adaptive frame, (W, H, 3) float32 (include/digital_earth_debug.h)."""
        out = np.empty((self.image_res[0], self.image_res[1], 3), dtype=np.float32)
        check(self._lib.de_debug_adaptive_moments(self._h, out.ctypes.data))
        return out

    # ------------------------------------------------------------------ denoiser (include/digital_earth_denoise.h)
    def set_denoise(self, on=True, levels=5, sigma_luminance=4.0):
        """Turn the denoiser of the display path on (or off).  While it is on, fetch_image (every mode, lag included) returns the denoised image: an
        edge-avoiding a-trous filter of the HDR mean guided by noise-free first-hit features, with the per-pixel variance when the frame tracked its
        sums of squares from its first sample (turn it on before accumulating) and the 7x7 spatial variance otherwise.  fetch_hdr() is unchanged."""
        if not on:
            check(self._lib.de_set_denoise(self._h, None))
            return
        d = DeDenoise()
        d.struct_bytes = ctypes.sizeof(DeDenoise)
        d.levels, d.sigma_luminance = int(levels), float(sigma_luminance)
        check(self._lib.de_set_denoise(self._h, ctypes.byref(d)))

    def denoise(self):
        """The denoiser's settings, dict(levels, sigma_luminance), or None while it is off."""
        d = DeDenoise()
        check(self._lib.de_get_denoise(self._h, ctypes.byref(d)))
        return None if d.levels == 0 else dict(levels=int(d.levels), sigma_luminance=float(d.sigma_luminance))

    def fetch_denoised_hdr(self):
        """The filtered HDR mean, (W, H, 3) float32 in fetch_hdr's layout (a mean, not a sum).  The denoiser must be on."""
        if not self._textures_copied:
            self.copy_textures()
        out = np.empty((self.image_res[0], self.image_res[1], 3), dtype=np.float32)
        check(self._lib.de_fetch_denoised_hdr(self._h, out.ctypes.data))
        return out

    def fetch_guides(self):
        """The denoiser's guides, (W, H, 9) float32: coverage, distance (m), normal xyz, albedo rgb, cloud transmittance."""
        if not self._textures_copied:
            self.copy_textures()
        out = np.empty((self.image_res[0], self.image_res[1], 9), dtype=np.float32)
        check(self._lib.de_fetch_guides(self._h, out.ctypes.data))
        return out

    def debug_denoise(self, mean, var, guides, levels=5, sigma_luminance=4.0):
        """The filter's levels on given inputs (include/digital_earth_debug.h: de_debug_denoise): mean (W, H, 3), var (W, H), guides (W, H, 9).
        Returns (W, H, 4): filtered rgb and the carried variance."""
        W, H = self.image_res
        mean = np.ascontiguousarray(mean, dtype=np.float32).reshape(W, H, 3)
        var = np.ascontiguousarray(var, dtype=np.float32).reshape(W, H)
        guides = np.ascontiguousarray(guides, dtype=np.float32).reshape(W, H, 9)
        out = np.empty((W, H, 4), dtype=np.float32)
        check(self._lib.de_debug_denoise(self._h, mean.ctypes.data, var.ctypes.data, guides.ctypes.data, int(levels), float(sigma_luminance), out.ctypes.data))
        return out

    # ------------------------------------------------------------------ auto-exposure (include/digital_earth_exposure.h)
    def set_auto_exposure(self, on=True, key=0.18, compensation=0.0, ev_range=(-8.0, 16.0), percentiles=(0.10, 0.95), adapt=1.0, region=None):
        """Turn the metered exposure of the display path on (or off).  While it is on, every fetch_image (lag included) first meters what it shows on the
        GPU — a histogram of log2 luminance, 8 bins per octave; the mean of the pixels between the two `percentiles` is mapped to `key`, plus `compensation`
        EV, clamped to `ev_range` — and displays with that exposure instead of the manual one, which is kept (set_exposure, exposure[None]) and comes
        back when the feature is turned off.  adapt < 1 eases towards the target from display to display: ev += adapt (target - ev).  region =
        (x0, y0, x1, y1), half-open in pixels: meter that rectangle only.  Every call restarts the adaptation; reset_framebuffer() does not."""
        if not on:
            check(self._lib.de_set_auto_exposure(self._h, None))
            return
        s = DeAutoExposure()
        s.struct_bytes = ctypes.sizeof(DeAutoExposure)
        s.key, s.compensation, s.adapt = float(key), float(compensation), float(adapt)
        s.ev_min, s.ev_max = float(ev_range[0]), float(ev_range[1])
        s.low_fraction, s.high_fraction = float(percentiles[0]), float(percentiles[1])
        if region is not None:
            if len(region) != 4:
                raise ValueError("region is (x0, y0, x1, y1)")
            s.region[:] = [int(v) for v in region]
        check(self._lib.de_set_auto_exposure(self._h, ctypes.byref(s)))

    def auto_exposure(self):
        """The auto-exposure settings as a dict (set_auto_exposure's keywords), or None while it is off."""
        s = DeAutoExposure()
        check(self._lib.de_get_auto_exposure(self._h, ctypes.byref(s)))
        if s.key == 0.0:
            return None
        region = tuple(int(v) for v in s.region)
        return dict(key=float(s.key), compensation=float(s.compensation), ev_range=(float(s.ev_min), float(s.ev_max)),
                    percentiles=(float(s.low_fraction), float(s.high_fraction)), adapt=float(s.adapt), region=region if any(region) else None)

    def metering(self):
        """What the newest display metered (waits for it): dict(ev, ev_target, mean_log2, valid, metered, below, clipped, histogram) — histogram a
        numpy uint32 array of 256 bins, bin k = octave (k >> 3) - 24, sub-bin k & 7.  Auto-exposure must be on and a fetch_image issued since."""
        m = DeMetering()
        m.struct_bytes = ctypes.sizeof(DeMetering)
        check(self._lib.de_get_metering(self._h, ctypes.byref(m)))
        return dict(ev=float(np.float32(m.ev)), ev_target=float(np.float32(m.ev_target)), mean_log2=float(np.float32(m.mean_log2)), valid=bool(m.valid),
                    metered=int(m.metered), below=int(m.below), clipped=int(m.clipped), histogram=np.array(m.histogram, dtype=np.uint32))

    # ------------------------------------------------------------------ bloom (include/digital_earth_bloom.h)
    def set_bloom(self, on=True, intensity=0.05, threshold=0.0, knee=0.5, clamp=0.0, spread=0.7, levels=6):
        """Turn the bloom of the display path on (or off).  While it is on, every fetch_image (lag included) first takes the fraction `intensity` of
        the light above `threshold` (luminance of the HDR mean; soft `knee`; at most `clamp` per pixel, 0 = no bound) from every pixel and gives it
        back through a wide, normalised point-spread function — a pyramid of `levels` levels, `spread` the weight of each coarser one — on the GPU;
        energy is conserved.  threshold = 0 is plain veiling glare.  fetch_hdr() is unchanged; auto-exposure meters the image before the bloom."""
        if not on:
            check(self._lib.de_set_bloom(self._h, None))
            return
        s = DeBloom()
        s.struct_bytes = ctypes.sizeof(DeBloom)
        s.intensity, s.threshold, s.knee, s.clamp, s.spread, s.levels = float(intensity), float(threshold), float(knee), float(clamp), float(spread), int(levels)
        check(self._lib.de_set_bloom(self._h, ctypes.byref(s)))

    def bloom(self):
        """The bloom settings as a dict (set_bloom's keywords), or None while it is off."""
        s = DeBloom()
        check(self._lib.de_get_bloom(self._h, ctypes.byref(s)))
        if s.levels == 0:
            return None
        return dict(intensity=float(s.intensity), threshold=float(s.threshold), knee=float(s.knee), clamp=float(s.clamp), spread=float(s.spread), levels=int(s.levels))

    def fetch_bloom_hdr(self):
        """The composited HDR mean that the display transform is given, (W, H, 3) float32 in fetch_hdr's layout (a mean, not a sum).  Bloom must be on."""
        if self.denoise() is not None and not self._textures_copied:
            self.copy_textures()
        out = np.empty((self.image_res[0], self.image_res[1], 3), dtype=np.float32)
        check(self._lib.de_fetch_bloom_hdr(self._h, out.ctypes.data))
        return out

    # ------------------------------------------------------------------ history reprojection (include/digital_earth_history.h)
    MAX_HISTORY = 32.0          # samples: the largest weight a reprojected pixel may carry
    DEPTH_TOLERANCE = 0.02      # a history tap is refused when its land distance is off by more than this fraction

    def set_history(self, enabled=True, max_history=MAX_HISTORY, depth_tolerance=DEPTH_TOLERANCE):
        """Turn history reprojection on (or off).  While it is on, every fetch_image (lag included) keeps what it showed, and after a
        reset_framebuffer() — a camera move — the next images blend, pixel by pixel, the new frame's mean with the previous picture reprojected into the
        new camera, weighted by sample counts (at most `max_history` samples for the old picture; taps whose land distance differs by more than
        `depth_tolerance` are refused).  A change of the sun, the terrain scale, a map or the integrator drops the history; exposure, gamma and the camera
        response keep it.  fetch_hdr() is unchanged; auto-exposure and bloom see the blended image.  Every call drops the history."""
        if not enabled:
            check(self._lib.de_set_history(self._h, None))
            return
        s = DeHistory()
        s.struct_bytes = ctypes.sizeof(DeHistory)
        s.max_history, s.depth_tolerance = float(max_history), float(depth_tolerance)
        check(self._lib.de_set_history(self._h, ctypes.byref(s)))

    def history(self):
        """The history settings as a dict (set_history's keywords), or None while it is off."""
        s = DeHistory()
        check(self._lib.de_get_history(self._h, ctypes.byref(s)))
        if s.max_history == 0.0:
            return None
        return dict(max_history=float(s.max_history), depth_tolerance=float(s.depth_tolerance))

    def fetch_history_hdr(self):
        """The blended HDR mean that the display transform is given and its weight in samples, (W, H, 4) float32 in fetch_hdr's layout.  History
        reprojection must be on.  Counts as a display: the next reset_framebuffer() keeps this picture."""
        if not self._textures_copied:
            self.copy_textures()
        out = np.empty((self.image_res[0], self.image_res[1], 4), dtype=np.float32)
        check(self._lib.de_fetch_history_hdr(self._h, out.ctypes.data))
        return out

    def debug_history(self, mean, n, dist, params, hist_c=None, hist_d=None, hist_params=None, max_history=MAX_HISTORY, depth_tolerance=DEPTH_TOLERANCE):
        """The blend once on given arrays (include/digital_earth_debug.h: de_debug_history): mean (W, H, 3), n (W, H) int32, dist (W, H), params the
        current DeParams; hist_c (W, H, 4), hist_d (W, H) and hist_params the history (None: no history yet).  Returns (W, H, 4)."""
        W, H = self.image_res
        mean = np.ascontiguousarray(mean, dtype=np.float32).reshape(W, H, 3)
        n = np.ascontiguousarray(n, dtype=np.int32).reshape(W, H)
        dist = np.ascontiguousarray(dist, dtype=np.float32).reshape(W, H)
        hc = hd = hp = None
        if hist_c is not None:
            hist_c = np.ascontiguousarray(hist_c, dtype=np.float32).reshape(W, H, 4)
            hist_d = np.ascontiguousarray(hist_d, dtype=np.float32).reshape(W, H)
            hc, hd, hp = hist_c.ctypes.data, hist_d.ctypes.data, ctypes.byref(hist_params)
        out = np.empty((W, H, 4), dtype=np.float32)
        check(self._lib.de_debug_history(self._h, mean.ctypes.data, n.ctypes.data, dist.ctypes.data, ctypes.byref(params), hc, hd, hp,
                                         float(max_history), float(depth_tolerance), out.ctypes.data))
        return out

    # ------------------------------------------------------------------ local exposure (include/digital_earth_local_exposure.h)
    def _local_exposure_settings(self, highlights, shadows, sigma, max_ev, key, levels):
        s = DeLocalExposure()
        s.struct_bytes = ctypes.sizeof(DeLocalExposure)
        s.on = 1
        s.highlights, s.shadows, s.sigma, s.max_ev, s.key, s.levels = float(highlights), float(shadows), float(sigma), float(max_ev), float(key), int(levels)
        return s

    def set_local_exposure(self, on=True, highlights=0.5, shadows=0.25, sigma=1.0, max_ev=2.0, key=0.18, levels=6):
        """Turn the local exposure of the display path on (or off): an edge-aware dodge and burn.  While it is on, every fetch_image / fetch_pixels (lag
        included) first multiplies every pixel of the HDR mean by 2^ev on the GPU, ev = -strength (B - mid) clamped to +-`max_ev` stops: B a smooth base
        of log2 luminance that stops at edges (a pyramid of `levels` levels, `sigma` stops wide in range), mid the scene luminance that the exposure in
        use (the metered one under auto-exposure) maps to `key`, strength `highlights` above mid and `shadows` below.  Detail and chroma are kept: the
        gain depends on the base only.  It runs last, behind the meter and the bloom.  fetch_hdr() is unchanged."""
        if not on:
            check(self._lib.de_set_local_exposure(self._h, None))
            return
        check(self._lib.de_set_local_exposure(self._h, ctypes.byref(self._local_exposure_settings(highlights, shadows, sigma, max_ev, key, levels))))

    @property
    def local_exposure(self):
        """The local exposure settings as a dict (set_local_exposure's keywords), or None while it is off."""
        s = DeLocalExposure()
        check(self._lib.de_get_local_exposure(self._h, ctypes.byref(s)))
        if not s.on:
            return None
        return dict(highlights=float(s.highlights), shadows=float(s.shadows), sigma=float(s.sigma), max_ev=float(s.max_ev), key=float(s.key), levels=int(s.levels))

    def fetch_local_exposure_hdr(self):
        """The dodged HDR mean that the display transform is given, (W, H, 3) float32 in fetch_hdr's layout (a mean, not a sum): the display chain up to
        and including this stage.  Local exposure must be on.  Under auto-exposure it counts as a display for the meter's adaptation."""
        if not self._textures_copied:
            self.copy_textures()
        out = np.empty((self.image_res[0], self.image_res[1], 3), dtype=np.float32)
        check(self._lib.de_fetch_local_exposure_hdr(self._h, out.ctypes.data))
        return out

    def debug_local_exposure(self, mean, exposure_scale, highlights=0.5, shadows=0.25, sigma=1.0, max_ev=2.0, key=0.18, levels=6):
        """The stage once on a given (W, H, 3) float32 mean of this renderer's size, the anchor taken from `exposure_scale` = 2^exposure
        (include/digital_earth_local_exposure.h: de_debug_local_exposure).  Returns (W, H, 3); the renderer's settings and frame are not touched."""
        W, H = self.image_res
        mean = np.ascontiguousarray(mean, dtype=np.float32).reshape(W, H, 3)
        out = np.empty((W, H, 3), dtype=np.float32)
        s = self._local_exposure_settings(highlights, shadows, sigma, max_ev, key, levels)
        check(self._lib.de_debug_local_exposure(self._h, mean.ctypes.data, ctypes.c_float(float(exposure_scale)), ctypes.byref(s), out.ctypes.data))
        return out

    # ------------------------------------------------------------------ output scaling (include/digital_earth_output_scale.h)
    SCALE_FILTERS = ("box", "triangle", "mitchell", "lanczos3")

    def _output_scale_settings(self, size, filter, on):
        if filter not in self.SCALE_FILTERS:
            raise ValueError("filter must be one of %s" % (self.SCALE_FILTERS,))
        s = DeOutputScale()
        s.struct_bytes = ctypes.sizeof(DeOutputScale)
        s.enabled = 1 if on else 0
        s.width, s.height = (0, 0) if size is None else (int(size[0]), int(size[1]))      # 0, 0: the source's own size
        s.filter = self.SCALE_FILTERS.index(filter)
        return s

    def set_output_scale(self, size=None, filter="lanczos3", on=True):
        """Deliver the displayed image at `size` = (width, height) instead of image_res: while this is on, fetch_image, fetch_pixels (lag included) and
        render_to_image_device hand out the image of the unchanged display transform resampled on the GPU by a separable polyphase filter — "box",
        "triangle", "mitchell" or "lanczos3", antialiased when it shrinks — and the pixels packed from it.  Render 3840 x 2160 and deliver 1920 x 1080
        (a quarter of the bytes cross the link), or render at half size while the camera moves.  width a multiple of 16, height of 8, each within
        [1/8, 8] of image_res; size=None is image_res (the identity, bit for bit).  Black and clipped white survive exactly.  Everything ahead of the
        display runs at image_res; fetch_hdr() is unchanged.  Refused (DE_ERR_STATE) while lagged fetches are in flight; a view from a fetch with
        copy=False does not outlive a change of size.  on=False: every fetch returns the bytes it returned before."""
        check(self._lib.de_set_output_scale(self._h, ctypes.byref(self._output_scale_settings(size, filter, on))))

    def output_scale(self):
        """The output scaling as a dict (set_output_scale's keywords; size is image_res until one is set)."""
        s = DeOutputScale()
        check(self._lib.de_get_output_scale(self._h, ctypes.byref(s)))
        return dict(size=(int(s.width), int(s.height)), filter=self.SCALE_FILTERS[s.filter], on=bool(s.enabled))

    def output_size(self):
        """(width, height) of what fetch_image and fetch_pixels deliver now: image_res while the output scaling is off."""
        w, h = ctypes.c_int(), ctypes.c_int()
        check(self._lib.de_output_size(self._h, ctypes.byref(w), ctypes.byref(h)))
        return int(w.value), int(h.value)

    def debug_output_scale(self, image, size, filter="lanczos3"):
        """The stage once on a given (W, H, 3) float32 image (include/digital_earth_debug.h: de_debug_output_scale), W a multiple of 16 and H of 8 but
        free of this renderer's size; returns (width, height, 3) float32.  The renderer's own setting is not touched."""
        image = np.ascontiguousarray(image, dtype=np.float32)
        if image.ndim != 3 or image.shape[2] != 3:
            raise ValueError("image must have shape (W, H, 3)")
        W, H = image.shape[:2]
        s = self._output_scale_settings(size, filter, True)
        ow, oh = (W, H) if size is None else (int(size[0]), int(size[1]))
        out = np.empty((max(ow, 0), max(oh, 0), 3), dtype=np.float32)
        check(self._lib.de_debug_output_scale(self._h, image.ctypes.data, W, H, ctypes.byref(s), out.ctypes.data))
        return out

    def debug_output_scale_weights(self, n_src, n_dst, filter):
        """The table of one axis exactly as the kernels read it (de_debug_output_scale_weights): (first, weights) — first (n_dst,) int32, the first
        source index of every output sample, unclamped; weights (n_dst, taps) float32."""
        if filter not in self.SCALE_FILTERS:
            raise ValueError("filter must be one of %s" % (self.SCALE_FILTERS,))
        f, taps = self.SCALE_FILTERS.index(filter), ctypes.c_int()
        check(self._lib.de_debug_output_scale_weights(self._h, int(n_src), int(n_dst), f, None, None, ctypes.byref(taps)))
        first, w = np.empty(int(n_dst), np.int32), np.empty((int(n_dst), int(taps.value)), np.float32)
        check(self._lib.de_debug_output_scale_weights(self._h, int(n_src), int(n_dst), f, first.ctypes.data, w.ctypes.data, ctypes.byref(taps)))
        return first, w

    # ------------------------------------------------------------------ panorama output (include/digital_earth_panorama.h)
    PANORAMA_PROJECTIONS = ("equirect", "fisheye")
    PANORAMA_FACES = ("+r", "-r", "+u", "-u", "+f", "-f")

    def _panorama_settings(self, size, projection, aperture, apron, supersample, basis, on):
        if projection not in self.PANORAMA_PROJECTIONS:
            raise ValueError("projection must be one of %s" % (self.PANORAMA_PROJECTIONS,))
        s = DePanorama()
        s.struct_bytes = ctypes.sizeof(DePanorama)
        s.on = 1 if on else 0
        s.projection = self.PANORAMA_PROJECTIONS.index(projection)
        s.width, s.height = int(size[0]), int(size[1])
        s.aperture_deg, s.apron, s.supersample = float(aperture), int(apron), int(supersample)
        b = np.asarray(np.eye(3) if basis is None else basis, dtype=np.float32).reshape(9)
        for k in range(9):
            s.basis[k] = float(b[k])
        return s

    def camera_basis(self):
        """The current camera's right, up and forward as a (3, 3) float64 array, rows r, u, f: forward = look_at - camera_pos, right = forward x up,
        up = right x forward, each normalised — the axes the renderer casts with."""
        pos, at, up = (np.array([v[0], v[1], v[2]], dtype=np.float64) for v in (self._params.camera_pos, self._params.look_at, self._params.up))
        f = at - pos
        f /= np.linalg.norm(f)
        r = np.cross(f, up)
        r /= np.linalg.norm(r)
        u = np.cross(r, f)
        return np.stack([r, u / np.linalg.norm(u), f])

    def set_panorama(self, size=None, projection="equirect", aperture=180.0, apron=1, supersample=2, basis=None, on=True):
        """Deliver a 360° frame instead of the pinhole rectangle: while this is on and six cube faces are captured (render_panorama), fetch_image,
        fetch_pixels, fetch_hdr_pixels, fetch_video, fetch_jpeg, fetch_png and render_to_image_device hand out `size` = (width, height): the faces
        resampled on the GPU to an "equirect" frame (a VR player, a video site, an environment map; size=None: (4 N, 2 N)) or a "fisheye" dome master
        of `aperture` degrees (width == height; size=None: (2 N, 2 N)).  The renderer must be square, image_res = (N, N).  apron: face pixels rendered
        beyond 90° on every side (1 ... N / 4) so that no bilinear tap crosses a cube edge; supersample: S x S sub-positions per output pixel
        (1 ... 4).  basis: the panorama's right, up and forward, (3, 3) rows r, u, f, orthonormal; None: the world axes — render_panorama(basis=None)
        sets the current camera's.  Every call clears the captured faces, the linear ones too.  Refused (DE_ERR_STATE) while output scaling is on or
        lagged fetches are in flight (of the EXR output: those of a scene-linear panorama).  The scene-linear side is
        include/digital_earth_environment.h's: while this is on fetch_exr is refused until six LINEAR faces are captured (render_environment), and
        then hands out the HDR environment map.  on=False: every fetch returns the bytes it returned before."""
        N = self.image_res[0]
        if size is None:
            size = (2 * N, 2 * N) if projection == "fisheye" else (4 * N, 2 * N)
        check(self._lib.de_set_panorama(self._h, ctypes.byref(self._panorama_settings(size, projection, aperture, apron, supersample, basis, on))))

    @property
    def panorama(self):
        """The panorama settings as a dict (set_panorama's keywords) plus captured, the tuple of the faces (0 ... 5 = +r, -r, +u, -u, +f, -f) held."""
        s, mask = DePanorama(), ctypes.c_uint32()
        check(self._lib.de_get_panorama(self._h, ctypes.byref(s)))
        check(self._lib.de_panorama_captured(self._h, ctypes.byref(mask)))
        return dict(size=(int(s.width), int(s.height)), projection=self.PANORAMA_PROJECTIONS[s.projection], aperture=float(s.aperture_deg), apron=int(s.apron),
                    supersample=int(s.supersample), basis=np.array(list(s.basis), dtype=np.float32).reshape(3, 3), on=bool(s.on),
                    captured=tuple(k for k in range(6) if mask.value >> k & 1))

    def panorama_face_camera(self, face):
        """The camera of cube face `face` under the current settings, at the current camera position: dict(look_at, up, fov) — set these with
        aspect_scale = 1, reset, accumulate, capture_panorama_face(face)."""
        pos, at, up, fov = (ctypes.c_float * 3)(*[float(v) for v in self._params.camera_pos]), (ctypes.c_float * 3)(), (ctypes.c_float * 3)(), ctypes.c_float()
        check(self._lib.de_panorama_face_camera(self._h, int(face), pos, at, up, ctypes.byref(fov)))
        return dict(look_at=tuple(float(v) for v in at), up=tuple(float(v) for v in up), fov=float(fov.value))

    def capture_panorama_face(self, face):
        """Display the frame as it stands and keep the image as cube face `face` (de_panorama_capture).  Refused (DE_ERR_STATE) under a vignette,
        auto-exposure, bloom, local exposure or history: each would print the face's border into the picture."""
        if not self._textures_copied:
            self.copy_textures()
        check(self._lib.de_panorama_capture(self._h, int(face)))

    def render_panorama(self, spp, basis=None):
        """The six faces of the panorama, `spp` samples per pixel each: for every face set its camera, reset, accumulate and capture; then put the
        caller's camera, fov and aspect scale back (and reset: the frame left is the last face's).  basis=None: the current camera's right, up and
        forward become the panorama's frame; otherwise (3, 3) rows r, u, f.  The settings are those of set_panorama(), which must be on."""
        self._render_faces(spp, basis, (self.capture_panorama_face,))

    def _render_faces(self, spp, basis, captures):
        """render_panorama's and render_environment's loop: every face rendered once and handed to each of `captures`."""
        held = self.panorama
        if not held["on"]:
            raise RuntimeError("the panorama is off: set_panorama() first")
        b = self.camera_basis() if basis is None else np.asarray(basis, dtype=np.float64).reshape(3, 3)
        if not np.array_equal(b.astype(np.float32), held["basis"]):      # a new frame is a new setting (refused while lagged fetches are in flight); the same one keeps its slots, overwritten below
            self.set_panorama(held["size"], held["projection"], held["aperture"], held["apron"], held["supersample"], b, True)
        p = self._params
        keep = (tuple(p.look_at), tuple(p.up), float(p.fov), float(p.aspect_scale))
        try:
            for face in range(6):
                cam = self.panorama_face_camera(face)
                p.look_at[0], p.look_at[1], p.look_at[2] = cam["look_at"]
                p.up[0], p.up[1], p.up[2] = cam["up"]
                p.fov, p.aspect_scale = cam["fov"], 1.0
                self._push_params()
                self.reset_framebuffer()
                self.accumulate(int(spp))
                for capture in captures:
                    capture(face)
        finally:
            (p.look_at[0], p.look_at[1], p.look_at[2]), (p.up[0], p.up[1], p.up[2]), p.fov, p.aspect_scale = keep[0], keep[1], keep[2], keep[3]
            self._push_params()
            self.reset_framebuffer()

    def debug_panorama(self, faces, size, projection="equirect", aperture=180.0, apron=1, supersample=2, basis=None):
        """The kernel once on given faces, (6, n, n, 3) float32, face k as fetch_image() returns the render of face k's camera (de_debug_panorama);
        any n >= 4, free of this renderer's size; returns (width, height, 3) float32.  The renderer's own setting and faces are not touched."""
        faces = np.ascontiguousarray(faces, dtype=np.float32)
        if faces.ndim != 4 or faces.shape[0] != 6 or faces.shape[1] != faces.shape[2] or faces.shape[3] != 3:
            raise ValueError("faces must have shape (6, n, n, 3)")
        s = self._panorama_settings(size, projection, aperture, apron, supersample, basis, True)
        out = np.empty((max(int(size[0]), 0), max(int(size[1]), 0), 3), dtype=np.float32)
        check(self._lib.de_debug_panorama(self._h, faces.ctypes.data, int(faces.shape[1]), ctypes.byref(s), out.ctypes.data))
        return out

    # ------------------------------------------------------------------ scene-linear panorama (include/digital_earth_environment.h)
    def capture_environment_face(self, face):
        """Keep the frame as it stands, in FRONT of the display, as LINEAR cube face `face` (de_environment_capture): what fetch_exr() would write
        with the panorama off — the mean, or with set_exr(source="denoised") the filtered mean; the other sources are refused (DE_ERR_STATE), a
        vignette and auto-exposure are not.  The panorama must be on."""
        if not self._textures_copied:
            self.copy_textures()
        check(self._lib.de_environment_capture(self._h, int(face)))

    def fetch_environment_face(self, face):
        """Linear face `face` as (N, N, 3) float32 in fetch_image's orientation: fetch_hdr() / spp of that face's render — one face of a linear
        cube map.  DE_ERR_STATE if it is not held."""
        N = self.image_res[0]
        out = np.empty((N, N, 3), dtype=np.float32)
        check(self._lib.de_fetch_environment_face(self._h, int(face), out.ctypes.data))
        return out

    @property
    def environment(self):
        """dict(captured=...): the tuple of the LINEAR faces (0 ... 5 = +r, -r, +u, -u, +f, -f) held.  With all six and the panorama on, fetch_exr()
        hands out the environment map at panorama["size"]."""
        mask = ctypes.c_uint32()
        check(self._lib.de_environment_captured(self._h, ctypes.byref(mask)))
        return dict(captured=tuple(k for k in range(6) if mask.value >> k & 1))

    def render_environment(self, spp, basis=None, display=False):
        """render_panorama's six renders, each captured LINEARLY (capture_environment_face): afterwards fetch_exr() — and save("x.exr"),
        frame(panorama=True, exr=True) — deliver one OpenEXR file of the scene-linear 360° frame, an HDR environment map, in the settings of
        set_exr().  display=True: every face is captured through the display too (capture_panorama_face), so that fetch_image, fetch_png, ... hand
        out the tone-mapped panorama of the same renders."""
        self._render_faces(spp, basis, (self.capture_environment_face, self.capture_panorama_face) if display else (self.capture_environment_face,))

    def debug_environment_exr(self, faces, size, projection="equirect", aperture=180.0, apron=1, supersample=2, basis=None,
                              pixel_type="half", compression="zip", chunk_bytes=None, scale=1.0):
        """The resampling and the EXR conversion once on given LINEAR faces, (6, n, n, 3) float32 as debug_panorama takes them
        (de_debug_environment_exr); returns the file as bytes.  The renderer's own settings and faces are not touched."""
        faces = np.ascontiguousarray(faces, dtype=np.float32)
        if faces.ndim != 4 or faces.shape[0] != 6 or faces.shape[1] != faces.shape[2] or faces.shape[3] != 3:
            raise ValueError("faces must have shape (6, n, n, 3)")
        p = self._panorama_settings(size, projection, aperture, apron, supersample, basis, True)
        s = self._ex_settings("mean", pixel_type, compression, chunk_bytes, scale)
        return self._coded_debug(self._lib.de_debug_exr_framing, (ctypes.byref(s), int(size[0]), int(size[1])), lambda out, n_bytes, n: self._lib.de_debug_environment_exr(
            self._h, faces.ctypes.data, int(faces.shape[1]), ctypes.byref(p), ctypes.byref(s), out, n_bytes, n))

    def _coded_debug(self, framing, shape, call):
        """The tail of every debug conversion whose length the library decides.  framing(*shape, out, out_bytes, len, capacity) is the format's
        de_debug_*_framing with its settings and shape: it answers the capacity.  call(out, out_bytes, len) converts into a buffer of that capacity
        filled, as 64 bytes behind it are, with a sentinel; nothing may be written behind *len.  Returns the file as bytes."""
        cap, n = ctypes.c_uint64(), ctypes.c_uint64()
        check(framing(*shape, None, 0, None, ctypes.byref(cap)))
        size = int(cap.value) + 64
        out = ctypes.create_string_buffer(b"\xA5" * size, size)
        check(call(out, ctypes.c_uint64(int(cap.value)), ctypes.byref(n)))
        if out.raw[int(n.value):] != b"\xA5" * (size - int(n.value)):
            raise RuntimeError("%s: the encoder wrote behind the file's length" % framing.__name__.replace("_framing", ""))
        return out.raw[:int(n.value)]

    def _staging_view(self, ptr, _=None):
        ow, oh = self.output_size()
        return np.empty((ow, oh, 3), dtype=np.float32) if ptr is None else np.ctypeslib.as_array(ptr, shape=(ow, oh, 3))

    def fetch_image(self, copy=True, lag=0):
        """renderer.py:382-384 — display transform of the accumulation; (W, H, 3) float32 in [0, 1].  copy=False returns a read-only
        view of the library's pinned staging buffer, valid until the next fetch_* call on this renderer (what a window loop needs: it
        hands the image to the canvas before it renders again) — no 24.9 MB host copy, no fresh pages.

        lag=1, 2 or 3: the window loop PIPELINED (de_fetch_image_begin / _end).  The display transform and the device-to-host copy of the frame as it
        stands are only ENQUEUED; the call returns the image of the lag-th PREVIOUS call (None until there is one), so the caller's next
        accumulate() renders while this frame is displayed and copied.  A lone one-sample launch takes ~10 ms (its longest path), so lag=1 runs
        at ~5.1 ms per 1080p frame, lag=2 at ~4.1 ms, lag=3 at ~3.5 ms (the floor, launches back to back without any fetch, is 2.9 ms).  Every image equals what the synchronous loop returns for the same frame, bit for bit,
        `lag` calls later; fetch_pending() hands out the rest.  A view (copy=False) stays valid until the next fetch_image call."""
        return self._image_ring.fetch(self, self._staging_view, copy, lag)

    def fetch_pending(self, copy=True, all_images=False, pixels=False, video=False):
        """End the pipelined window loop: wait for the fetches still in flight and return the newest image (None when there is none);
        all_images=True: the list of all of them, oldest first (copies).  pixels=True: the same for the lagged fetch_pixels() calls, which have a
        ring of their own; the float fetches are left alone, as the pixel fetches are without it.  video=True: the same for the lagged
        fetch_video() calls and their ring.  (The lagged fetch_jpeg() calls end in fetch_pending_jpeg().)"""
        if video and pixels:
            raise ValueError("pixels=True and video=True name two rings: one call each")
        ring, array = (self._vd_ring, self._vd_view) if video else (self._pixel_ring, self._pixel_view) if pixels else (self._image_ring, self._staging_view)
        imgs = []
        while ring.in_flight > 0:
            imgs.append(ring.end(self, array, copy or all_images))
        if all_images:
            return imgs
        return imgs[-1] if imgs else None

    # ------------------------------------------------------------------ 8-bit pixel output (include/digital_earth_pixels.h)
    PIXEL_MODES = ("truncate", "round", "dither")

    def set_pixels(self, channels=4, mode="truncate", seed=0, animate=False):
        """The format of fetch_pixels(): 3 (RGB8) or 4 (RGBA8, alpha 255) channels; mode "truncate" (to_vec3u: what screenshots have always held),
        "round", or "dither" (a two-LSB triangular dither from a hash of `seed`, the pixel and the channel, fading out at 0 and 255 so that black
        and clipped white stay exact).  animate=False: a frame always gives the same bytes; True: the pattern changes with every conversion.  Every
        call resets the phase counter; refused (DE_ERR_STATE) while lagged pixel fetches are in flight.  fetch_image() is not affected."""
        if mode not in self.PIXEL_MODES:
            raise ValueError("mode must be one of %s" % (self.PIXEL_MODES,))
        s = DePixels()
        s.struct_bytes = ctypes.sizeof(DePixels)
        s.channels, s.mode, s.seed, s.animate = int(channels), self.PIXEL_MODES.index(mode), int(seed) & 0xffffffff, 1 if animate else 0
        check(self._lib.de_set_pixels(self._h, ctypes.byref(s)))

    def pixels(self):
        """The pixel format as a dict (set_pixels' keywords) plus last_phase, the dither phase of the newest conversion."""
        s, phase = DePixels(), ctypes.c_uint32()
        check(self._lib.de_get_pixels(self._h, ctypes.byref(s), ctypes.byref(phase)))
        return dict(channels=int(s.channels), mode=self.PIXEL_MODES[s.mode], seed=int(s.seed), animate=bool(s.animate), last_phase=int(phase.value))

    def _pixel_view(self, ptr, channels):
        ow, oh = self.output_size()
        return np.empty((oh, ow, channels), dtype=np.uint8) if ptr is None else np.ctypeslib.as_array(ptr, shape=(oh, ow, channels))

    def fetch_pixels(self, copy=True, lag=0):
        """The displayed image as packed 8-bit pixels, converted on the GPU behind the display transform: (H, W, channels) uint8, rows top-down — what
        a canvas, an image writer or an encoder takes as it is — in the format of set_pixels().  A quarter or a third of fetch_image()'s bytes cross the
        link and the host converts nothing.  copy=False: a read-only view of the library's pinned pixel staging buffer, valid until the next
        fetch_pixels call.  lag=1, 2 or 3: pipelined like fetch_image(lag=...), through a ring of its own — the call returns the pixels of the
        lag-th previous call (None until there is one); fetch_pending(pixels=True) hands out the rest."""
        return self._pixel_ring.fetch(self, self._pixel_view, copy, lag)

    def debug_pixels(self, image, channels=4, mode="truncate", seed=0, phase=0):
        """The conversion once on a given (W, H, 3) float32 image (include/digital_earth_debug.h: de_debug_pixels), W a multiple of 16 and H of 8 but
        free of this renderer's size; returns (H, W, channels) uint8.  The renderer's own pixels and phase counter are not touched."""
        image = np.ascontiguousarray(image, dtype=np.float32)
        if image.ndim != 3 or image.shape[2] != 3:
            raise ValueError("image must have shape (W, H, 3)")
        W, H = image.shape[:2]
        s = DePixels()
        s.struct_bytes = ctypes.sizeof(DePixels)
        s.channels, s.mode, s.seed, s.animate = int(channels), self.PIXEL_MODES.index(mode), int(seed) & 0xffffffff, 0
        out = np.empty((H, W, int(channels) if channels in (3, 4) else 4), dtype=np.uint8)
        check(self._lib.de_debug_pixels(self._h, image.ctypes.data, W, H, ctypes.byref(s), ctypes.c_uint32(int(phase) & 0xffffffff), out.ctypes.data))
        return out

    # ------------------------------------------------------------------ video frame output (include/digital_earth_video.h)
    VIDEO_FORMATS = ("nv12", "i420", "p010", "i010")
    VIDEO_MATRICES = ("bt709", "bt601", "bt2020")
    VIDEO_RANGES = ("limited", "full")
    VIDEO_SITINGS = ("left", "center", "topleft")

    def _vd_settings(self, format, matrix, range, siting, mode, seed, animate):
        for value, names, what in ((format, self.VIDEO_FORMATS, "format"), (matrix, self.VIDEO_MATRICES, "matrix"), (range, self.VIDEO_RANGES, "range"),
                                   (siting, self.VIDEO_SITINGS, "siting"), (mode, self.PIXEL_MODES, "mode")):
            if value not in names:
                raise ValueError("%s must be one of %s" % (what, names))
        s = DeVideo()
        s.struct_bytes = ctypes.sizeof(DeVideo)
        s.format, s.matrix, s.range, s.siting = self.VIDEO_FORMATS.index(format), self.VIDEO_MATRICES.index(matrix), self.VIDEO_RANGES.index(range), self.VIDEO_SITINGS.index(siting)
        s.mode, s.seed, s.animate = self.PIXEL_MODES.index(mode), int(seed) & 0xffffffff, 1 if animate else 0
        return s

    def set_video(self, format="nv12", matrix="bt709", range="limited", siting="left", mode="round", seed=0, animate=False):
        """The format of fetch_video(): Y'CbCr 4:2:0 planes packed on the GPU behind the display transform (and behind output scaling).
        format "nv12" / "i420" (8 bits) or "p010" / "i010" (10 bits in uint16 words: high bits / low bits, i010 = yuv420p10le); matrix "bt709",
        "bt601" or "bt2020" (non-constant luminance); range "limited" (16-235 / 16-240, scaled by 4 at 10 bits) or "full"; chroma siting "left"
        (MPEG-2 / H.264), "center" (JPEG) or "topleft" (BT.2020 / HDR); mode, seed and animate as set_pixels, rounding by default.  Every call resets
        the phase counter; refused (DE_ERR_STATE) while lagged video fetches are in flight.  No other fetch is affected.  With set_hdr_output(True,
        transfer="pq", gamut="rec2020") ahead of it, format="i010", matrix="bt2020", siting="topleft" is the HDR10 frame (set_hdr_output's known
        limit on that gamut carries over)."""
        check(self._lib.de_set_video(self._h, ctypes.byref(self._vd_settings(format, matrix, range, siting, mode, seed, animate))))

    def video(self):
        """The video format as a dict (set_video's keywords) plus last_phase, size = (width, height), frame_bytes, and the byte offsets and row
        strides of the Y, Cb and Cr samples (plane_offsets, plane_strides)."""
        s, phase = DeVideo(), ctypes.c_uint32()
        check(self._lib.de_get_video(self._h, ctypes.byref(s), ctypes.byref(phase)))
        n, off, stride = ctypes.c_uint64(), (ctypes.c_uint64 * 3)(), (ctypes.c_uint64 * 3)()
        check(self._lib.de_videoframe_bytes(self._h, ctypes.byref(n), off, stride))
        return dict(format=self.VIDEO_FORMATS[s.format], matrix=self.VIDEO_MATRICES[s.matrix], range=self.VIDEO_RANGES[s.range], siting=self.VIDEO_SITINGS[s.siting],
                    mode=self.PIXEL_MODES[s.mode], seed=int(s.seed), animate=bool(s.animate), last_phase=int(phase.value), size=self.output_size(),
                    frame_bytes=int(n.value), plane_offsets=tuple(int(x) for x in off), plane_strides=tuple(int(x) for x in stride))

    def _vd_bytes(self):
        n = ctypes.c_uint64()
        check(self._lib.de_videoframe_bytes(self._h, ctypes.byref(n), None, None))
        return int(n.value)

    def _vd_view(self, ptr, nbytes):
        return np.empty(nbytes, dtype=np.uint8) if ptr is None else np.ctypeslib.as_array(ptr, shape=(nbytes,))

    def fetch_video(self, copy=True, lag=0):
        """The displayed image as one video frame in the format of set_video(): a flat uint8 array of video()["frame_bytes"] bytes, the
        planes one after the other, rows top-down — what an encoder or a raw-video pipe takes as it is; split_video() views it as planes.  1.5 (8-bit)
        or 3 (10-bit) bytes per pixel cross the link.  copy=False: a read-only view of the library's pinned video staging buffer, valid until the next
        fetch_video call.  lag=1, 2 or 3: pipelined like fetch_pixels(lag=...), through a ring of its own — the call returns the frame of the
        lag-th previous call (None until there is one); fetch_pending(video=True) hands out the rest."""
        return self._vd_ring.fetch(self, self._vd_view, copy, lag)

    def split_video(self, frame, size=None, format=None):
        """A frame as numpy views, no copy: (Y, Cb, Cr) for "i420" / "i010", (Y, CbCr) with CbCr of shape (H / 2, W / 2, 2) for "nv12" / "p010"; uint8
        or, for the 10-bit formats, uint16.  size = (width, height) and format default to this renderer's current output size and video format."""
        if size is None:
            size = self.output_size()
        if format is None:
            format = self.video()["format"]
        W, H = int(size[0]), int(size[1])
        if format not in self.VIDEO_FORMATS:
            raise ValueError("format must be one of %s" % (self.VIDEO_FORMATS,))
        if W <= 0 or H <= 0 or W % 2 or H % 2:
            raise ValueError("a 4:2:0 frame has an even width and height")
        flat = np.asarray(frame).reshape(-1).view(np.uint8)
        if format in ("p010", "i010"):
            flat = flat.view(np.uint16)
        if flat.size != W * H * 3 // 2:
            raise ValueError("the frame does not hold %d x %d samples of %s" % (W, H, format))
        y = flat[:W * H].reshape(H, W)
        if format in ("nv12", "p010"):
            return y, flat[W * H:].reshape(H // 2, W // 2, 2)
        n = (W // 2) * (H // 2)
        return y, flat[W * H:W * H + n].reshape(H // 2, W // 2), flat[W * H + n:].reshape(H // 2, W // 2)

    def render_to_video(self):
        """Run the display and the video pack and leave the frame on the device (de_render_to_video); returns its address."""
        if not self._textures_copied:
            self.copy_textures()
        p = ctypes.c_void_p()
        check(self._lib.de_render_to_video(self._h, ctypes.byref(p)))
        return p.value

    def debug_video(self, image, format="nv12", matrix="bt709", range="limited", siting="left", mode="round", seed=0, phase=0):
        """The conversion once on a given (W, H, 3) float32 image (de_debug_video), W and H even but free of this renderer's size; returns the frame as
        a flat uint8 array (split_video(frame, (W, H), format) views it).  The renderer's own settings, frame and phase counter are not touched."""
        image = np.ascontiguousarray(image, dtype=np.float32)
        if image.ndim != 3 or image.shape[2] != 3:
            raise ValueError("image must have shape (W, H, 3)")
        W, H = image.shape[:2]
        s = self._vd_settings(format, matrix, range, siting, mode, seed, False)
        out = np.empty(max(W * H // 2, 1) * 3 * (2 if format in ("p010", "i010") else 1), dtype=np.uint8)
        check(self._lib.de_debug_video(self._h, image.ctypes.data, W, H, ctypes.byref(s), ctypes.c_uint32(int(phase) & 0xffffffff), out.ctypes.data))
        return out

    # ------------------------------------------------------------------ JPEG output (include/digital_earth_jpeg.h)
    def _jp_settings(self, quality, restart):
        s = DeJpeg()
        s.struct_bytes = ctypes.sizeof(DeJpeg)
        s.quality, s.restart_mcus = int(quality), _native.JPEG_DEFAULT_RESTART if restart is None else int(restart)
        return s

    def set_jpeg(self, quality=90, restart=None):
        """The settings of fetch_jpeg(): a baseline JFIF file (4:2:0, the typical Huffman tables) encoded on the GPU behind the display transform (and
        behind the look and output scaling).  quality 1 ... 100 on the IJG scale; restart: MCUs (16 x 16 pixels) per restart interval, 1 ... 65535 —
        the encoder's unit of parallelism; None: the measured default (profiles/jpeg.md).  Refused (DE_ERR_STATE) while lagged JPEG fetches are in
        flight.  No other fetch is affected."""
        check(self._lib.de_set_jpeg(self._h, ctypes.byref(self._jp_settings(quality, restart))))

    def jpeg(self):
        """The JPEG settings as a dict (set_jpeg's keywords, restart as a number) plus size = (width, height) and capacity, the upper bound of any
        frame's length at these settings."""
        s, n = DeJpeg(), ctypes.c_uint64()
        check(self._lib.de_get_jpeg(self._h, ctypes.byref(s)))
        check(self._lib.de_jpeg_capacity(self._h, ctypes.byref(n)))
        return dict(quality=int(s.quality), restart=int(s.restart_mcus), size=self.output_size(), capacity=int(n.value))

    def fetch_jpeg(self, copy=True, lag=0):
        """The displayed image as one complete JPEG file: `bytes` that open(path, "wb").write() or a socket takes as they are.  Only the file's own
        bytes cross the link.  copy=False: a read-only memoryview of the library's pinned buffer, valid until the next fetch_jpeg call (lag = 0) or
        until the ring comes round (lag > 0).  lag=1, 2 or 3: pipelined like fetch_video(lag=...), through a ring of its own — the call returns the
        file of the lag-th previous call (None until there is one); fetch_pending_jpeg() hands out the rest."""
        return self._jp_coded.fetch(self, copy, lag)

    def fetch_pending_jpeg(self, copy=True, all_images=False):
        """fetch_pending() for the lagged fetch_jpeg() calls and their ring: wait for the JPEG fetches still in flight and return the newest file
        (None when there is none) — bytes, or a memoryview with copy=False; all_images=True: the list of all of them, oldest first (bytes)."""
        return self._jp_coded.pending(self, copy, all_images)

    def render_to_jpeg(self):
        """Run the display and the encoder and leave the stream on the device (de_render_to_jpeg); returns (address of the stream, address of its
        uint64 length).  Nothing is waited for."""
        return self._jp_coded.render_to(self)

    def debug_jpeg(self, image, quality=90, restart=None):
        """The encoder once on a given (W, H, 3) float32 image (de_debug_jpeg), W and H even but free of this renderer's size; returns the file as
        bytes.  The renderer's own settings and streams are not touched."""
        image = np.ascontiguousarray(image, dtype=np.float32)
        if image.ndim != 3 or image.shape[2] != 3:
            raise ValueError("image must have shape (W, H, 3)")
        W, H = image.shape[:2]
        s = self._jp_settings(quality, restart)
        return self._coded_debug(self._lib.de_debug_jpeg_framing, (ctypes.byref(s), W, H), lambda out, size, n: self._lib.de_debug_jpeg(
            self._h, image.ctypes.data, W, H, ctypes.byref(s), out, size, n))

    # ------------------------------------------------------------------ PNG output (include/digital_earth_png.h)
    def _pn_settings(self, source, filter, chunk_bytes):
        if source not in _native.PNG_SOURCES:
            raise ValueError("source must be one of %s" % (_native.PNG_SOURCES,))
        if filter not in _native.PNG_FILTERS:
            raise ValueError("filter must be one of %s" % (_native.PNG_FILTERS,))
        s = DePng()
        s.struct_bytes = ctypes.sizeof(DePng)
        s.source, s.filter = _native.PNG_SOURCES.index(source), _native.PNG_FILTERS.index(filter)
        s.chunk_bytes = _native.PNG_DEFAULT_CHUNK if chunk_bytes is None else int(chunk_bytes)
        return s

    def set_png(self, source="pixels", filter="adaptive", chunk_bytes=None):
        """The settings of fetch_png(): one complete, lossless PNG file filtered and deflated on the GPU behind the packed outputs.  source "pixels":
        the 8-bit pixels of set_pixels() (RGB or RGBA); "hdr_pixels": the 16-bit RGB pixels of set_hdr_output(pixel_format="rgb16"), with a cICP
        chunk.  filter: "adaptive" (per row, the lowest sum of absolute values) or a fixed "none" / "sub" / "up" / "average" / "paeth".  chunk_bytes:
        filtered bytes per independent deflate chunk, 1024 ... 65535 — the encoder's unit of parallelism; None: the default.  Refused (DE_ERR_STATE)
        while lagged PNG fetches are in flight.  No other fetch is affected."""
        check(self._lib.de_set_png(self._h, ctypes.byref(self._pn_settings(source, filter, chunk_bytes))))
        self._png_set = True

    def png(self):
        """The PNG settings as a dict (set_png's keywords) plus size = (width, height) and capacity, the proven bound of any frame's length."""
        s, n = DePng(), ctypes.c_uint64()
        check(self._lib.de_get_png(self._h, ctypes.byref(s)))
        check(self._lib.de_png_capacity(self._h, ctypes.byref(n)))
        return dict(source=_native.PNG_SOURCES[s.source], filter=_native.PNG_FILTERS[s.filter], chunk_bytes=int(s.chunk_bytes),
                    size=self.output_size(), capacity=int(n.value))

    @property
    def png_is_set(self):
        """True once set_png() has been called: EarthViewer.save("x.png") then writes the GPU's file."""
        return self._png_set

    def fetch_png(self, copy=True, lag=0):
        """The displayed image as one complete PNG file: `bytes` that open(path, "wb").write() takes as they are.  Only the file's own bytes cross
        the link.  copy=False: a read-only memoryview of the library's pinned buffer, valid until the next fetch_png call (lag = 0) or until the
        ring comes round (lag > 0).  lag=1, 2 or 3: pipelined like fetch_jpeg(lag=...), through a ring of its own — the call returns the file of
        the lag-th previous call (None until there is one); fetch_pending_png() hands out the rest."""
        return self._pn_coded.fetch(self, copy, lag)

    def fetch_pending_png(self, copy=True, all_images=False):
        """fetch_pending() for the lagged fetch_png() calls and their ring: wait for the PNG fetches still in flight and return the newest file
        (None when there is none) — bytes, or a memoryview with copy=False; all_images=True: the list of all of them, oldest first (bytes)."""
        return self._pn_coded.pending(self, copy, all_images)

    def render_to_png(self):
        """Run the display, the pack and the encoder and leave the file on the device (de_render_to_png); returns (address of the file, address of
        its uint64 length).  Nothing is waited for."""
        return self._pn_coded.render_to(self)

    def debug_png(self, pixels, filter="adaptive", chunk_bytes=None, cicp=None):
        """The encoder once on given packed pixels (de_debug_png): (H, W, 3 | 4) uint8 or (H, W, 3) uint16, rows top-down, of any size; returns the
        file as bytes.  The renderer's own settings and streams are not touched.  cicp: four code points for a 16-bit file other than the call's
        own (1, 8, 0, 1) — the front is the host's part (de_debug_png_framing), so the host exchanges it."""
        pixels = np.ascontiguousarray(pixels)
        if pixels.ndim != 3 or not ((pixels.dtype == np.uint8 and pixels.shape[2] in (3, 4)) or (pixels.dtype == np.uint16 and pixels.shape[2] == 3)):
            raise ValueError("pixels must be (H, W, 3 | 4) uint8 or (H, W, 3) uint16")
        H, W, ch = pixels.shape
        depth = 8 * pixels.dtype.itemsize
        s = self._pn_settings("pixels", filter, chunk_bytes)
        data = self._coded_debug(self._lib.de_debug_png_framing, (ctypes.byref(s), W, H, ch, depth, None), lambda out, size, n: self._lib.de_debug_png(
            self._h, pixels.ctypes.data, W, H, ch, depth, ctypes.byref(s), out, size, n))
        if cicp is not None and depth == 16:
            front, m = ctypes.create_string_buffer(64), ctypes.c_uint64()
            check(self._lib.de_debug_png_framing(ctypes.byref(s), W, H, ch, depth, bytes(bytearray(cicp)), front, ctypes.c_uint64(64), ctypes.byref(m), None))
            data = front.raw[:int(m.value)] + data[int(m.value):]
        return data

    # ------------------------------------------------------------------ OpenEXR output (include/digital_earth_exr.h)
    def _ex_settings(self, source, pixel_type, compression, chunk_bytes, scale):
        if source not in _native.EXR_SOURCES:
            raise ValueError("source must be one of %s" % (_native.EXR_SOURCES,))
        if pixel_type not in _native.EXR_PIXEL_TYPES:
            raise ValueError("pixel_type must be one of %s" % (tuple(_native.EXR_PIXEL_TYPES),))
        if compression not in _native.EXR_COMPRESSIONS:
            raise ValueError("compression must be one of %s" % (tuple(_native.EXR_COMPRESSIONS),))
        s = DeExr()
        s.struct_bytes = ctypes.sizeof(DeExr)
        s.source, s.pixel_type, s.compression = _native.EXR_SOURCES.index(source), _native.EXR_PIXEL_TYPES[pixel_type], _native.EXR_COMPRESSIONS[compression]
        s.chunk_bytes = _native.EXR_DEFAULT_CHUNK if chunk_bytes is None else int(chunk_bytes)
        s.scale = float(scale)
        return s

    @staticmethod
    def _ex_aov_mask(aovs):
        """Names of AOV groups (or "all", or one name) -> the DE_EXR_AOV_* mask."""
        if isinstance(aovs, str):
            aovs = (aovs,)
        mask = 0
        for name in aovs or ():
            if name == "all":
                mask |= _native.EXR_AOV_ALL
            elif name in _native.EXR_AOVS:
                mask |= _native.EXR_AOVS[name]
            else:
                raise ValueError("aovs must be names of %s, or \"all\"" % (tuple(_native.EXR_AOVS),))
        return mask

    def set_exr(self, source="mean", pixel_type="half", compression="zip", chunk_bytes=None, scale=1.0, aovs=()):
        """The settings of fetch_exr(): one complete OpenEXR scan-line file of the SCENE-LINEAR frame, converted and deflated on the GPU in front of
        the display transform.  source "mean": the sums divided by the sample count (per tile inside an adaptive frame); "denoised" / "history" /
        "bloom" / "local_exposure": the image fetch_denoised_hdr() / fetch_history_hdr() / fetch_bloom_hdr() / fetch_local_exposure_hdr() hand
        out, refused as those are while the stage is off.  pixel_type "half" (clamped to +-65504, nearest even) or "float"; compression "zip"
        (16 lines per block), "zips" (one) or "none"; chunk_bytes: predicted bytes per independent deflate chunk, 1024 ... 65535 (None: the
        default); scale: finite, > 0, multiplied into every sample.  The file is always the context's size: output scaling and the look do not
        apply.  Refused (DE_ERR_STATE) while lagged EXR fetches are in flight.  No other fetch is affected.
        aovs: names of channel groups written beside B, G, R in the same file (include/digital_earth_exr_aovs.h) — "depth" (Z, metres,
        always float), "normal" (N.X, N.Y, N.Z), "albedo" (albedo.R, .G, .B), "coverage", "transmittance", "variance" (variance.R, .G, .B of the
        mean, always float: needs the denoiser on since before the frame's first sample, or an adaptive frame), "samples" (always float) — or "all".
        () : none, the three-channel file.  digital_earth_amd.exr.read returns them in info["channels"].  A refused call changes nothing."""
        s, mask = self._ex_settings(source, pixel_type, compression, chunk_bytes, scale), self._ex_aov_mask(aovs)
        W, H = self.image_res
        if mask:      # what de_set_exr_aovs could refuse behind the new settings, first (without AOVs a frame past the limit is refused at the fetch, as before)
            check(self._lib.de_debug_exr_aov_framing(ctypes.byref(s), mask, int(W), int(H), None, 0, None, None))
        check(self._lib.de_set_exr_aovs(self._h, 0))      # refuses while fetches are in flight, as de_set_exr does; the mask goes on behind the settings it is checked against
        check(self._lib.de_set_exr(self._h, ctypes.byref(s)))
        check(self._lib.de_set_exr_aovs(self._h, mask))

    def exr_aovs(self):
        """The names of the AOV channel groups in force (set_exr's aovs), in the order of their bits."""
        mask = ctypes.c_uint32()
        check(self._lib.de_get_exr_aovs(self._h, ctypes.byref(mask)))
        return tuple(name for name, bit in _native.EXR_AOVS.items() if mask.value & bit)

    def exr(self):
        """The EXR settings as a dict (set_exr's keywords) plus size = (width, height) and capacity, the proven bound of any frame's length — of the
        panorama's size while fetch_exr() delivers the scene-linear panorama (render_environment)."""
        s, n = DeExr(), ctypes.c_uint64()
        check(self._lib.de_get_exr(self._h, ctypes.byref(s)))
        check(self._lib.de_exr_capacity(self._h, ctypes.byref(n)))
        name = lambda table, v: next(k for k, x in table.items() if x == v)
        return dict(source=_native.EXR_SOURCES[s.source], pixel_type=name(_native.EXR_PIXEL_TYPES, s.pixel_type),
                    compression=name(_native.EXR_COMPRESSIONS, s.compression), chunk_bytes=int(s.chunk_bytes), scale=float(s.scale),
                    size=self._exr_size(), capacity=int(n.value))

    def _exr_size(self):
        p = self.panorama
        return p["size"] if p["on"] and len(self.environment["captured"]) == 6 else self.image_res

    def fetch_exr(self, copy=True, lag=0):
        """The scene-linear frame as one complete OpenEXR file: `bytes` that open(path, "wb").write() takes as they are (digital_earth_amd.exr.read
        opens them again).  Only the file's own bytes cross the link.  copy=False: a read-only memoryview of the library's pinned buffer, valid
        until the next fetch_exr call (lag = 0) or until the ring comes round (lag > 0).  lag=1, 2 or 3: pipelined like fetch_png(lag=...), through
        a ring of its own — the call returns the file of the lag-th previous call (None until there is one); fetch_pending_exr() hands out the rest."""
        return self._ex_coded.fetch(self, copy, lag)

    def fetch_pending_exr(self, copy=True, all_images=False):
        """fetch_pending() for the lagged fetch_exr() calls and their ring: wait for the EXR fetches still in flight and return the newest file
        (None when there is none) — bytes, or a memoryview with copy=False; all_images=True: the list of all of them, oldest first (bytes)."""
        return self._ex_coded.pending(self, copy, all_images)

    def render_to_exr(self):
        """Run the stages up to the source's and the encoder and leave the file on the device (de_render_to_exr); returns (address of the file,
        address of its uint64 length).  Nothing is waited for."""
        return self._ex_coded.render_to(self)

    def debug_exr(self, image, pixel_type="half", compression="zip", chunk_bytes=None, scale=1.0):
        """The encoder once on a given (H, W, 3) float32 image in R, G, B order, rows top-down, of any size (de_debug_exr); returns the file as
        bytes.  The renderer's own settings and streams are not touched."""
        image = np.ascontiguousarray(image, dtype=np.float32)
        if image.ndim != 3 or image.shape[2] != 3:
            raise ValueError("image must have shape (H, W, 3)")
        H, W = image.shape[:2]
        s = self._ex_settings("mean", pixel_type, compression, chunk_bytes, scale)
        return self._coded_debug(self._lib.de_debug_exr_framing, (ctypes.byref(s), W, H), lambda out, size, n: self._lib.de_debug_exr(
            self._h, image.ctypes.data, W, H, ctypes.byref(s), out, size, n))

    def debug_exr_aovs(self, image, guides=None, s2=None, counts=None, aovs=(), pixel_type="half", compression="zip", chunk_bytes=None, scale=1.0):
        """The encoder with AOV channels once on given arrays, rows top-down, of any size (de_debug_exr_aovs): image (H, W, 3) is read as the sums,
        guides (H, W, 9) in fetch_guides' order, s2 (H, W, 3), counts (H, W) the divisor per pixel (None: 1).  An array no selected channel reads
        may be None.  aovs: names as for set_exr, or the mask itself.  Returns the file as bytes."""
        image = np.ascontiguousarray(image, dtype=np.float32)
        if image.ndim != 3 or image.shape[2] != 3:
            raise ValueError("image must have shape (H, W, 3)")
        H, W = image.shape[:2]
        keep = []

        def arg(a, shape, what):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.shape != shape:
                raise ValueError("%s must have shape %s" % (what, shape))
            keep.append(a)
            return a.ctypes.data
        mask = int(aovs) if isinstance(aovs, (int, np.integer)) else self._ex_aov_mask(aovs)
        s = self._ex_settings("mean", pixel_type, compression, chunk_bytes, scale)
        arrays = (arg(guides, (H, W, 9), "guides"), arg(s2, (H, W, 3), "s2"), arg(counts, (H, W), "counts"))
        return self._coded_debug(self._lib.de_debug_exr_aov_framing, (ctypes.byref(s), mask, W, H), lambda out, size, n: self._lib.de_debug_exr_aovs(
            self._h, image.ctypes.data, *arrays, W, H, ctypes.byref(s), mask, out, size, n))

    # ------------------------------------------------------------------ Radiance HDR output (include/digital_earth_rgbe.h)
    def _rg_settings(self, source, rle, rounding, scale):
        if source not in _native.EXR_SOURCES:
            raise ValueError("source must be one of %s" % (_native.EXR_SOURCES,))
        if rounding not in _native.RGBE_ROUNDINGS:
            raise ValueError("rounding must be one of %s" % (tuple(_native.RGBE_ROUNDINGS),))
        s = DeRgbe()
        s.struct_bytes = ctypes.sizeof(DeRgbe)
        s.source, s.rle, s.rounding, s.scale = _native.EXR_SOURCES.index(source), 1 if rle else 0, _native.RGBE_ROUNDINGS[rounding], float(scale)
        return s

    def set_rgbe(self, source="mean", rle=True, rounding="trunc", scale=1.0):
        """The settings of fetch_rgbe(): one complete Radiance picture file (.hdr, RGBE) of the SCENE-LINEAR frame, converted and run-length coded
        on the GPU in front of the display transform — the format environment maps are traded in.  source: as set_exr's, with its refusals.
        rle: new-style run-length coded rows (where the format allows them: 8 <= W <= 32767), else flat rows.  rounding "trunc" is Radiance's own
        float2rgbe and suits decoders that add half a step (digital_earth_amd.rgbe.read(half_step=True)); "round" suits those that do not.
        scale: finite, > 0, multiplied into every sample and written as EXPOSURE.  The file is always the context's size: output scaling and the
        look do not apply.  Refused (DE_ERR_STATE) while lagged RGBE fetches are in flight.  No other fetch is affected."""
        s = self._rg_settings(source, rle, rounding, scale)
        check(self._lib.de_set_rgbe(self._h, ctypes.byref(s)))
        self._rgbe_set = True

    @property
    def rgbe_is_set(self):
        """True once set_rgbe() has been called: EarthViewer.save("x.hdr") then writes the GPU's file."""
        return self._rgbe_set

    def rgbe(self):
        """The RGBE settings as a dict (set_rgbe's keywords) plus size = (width, height) and capacity, the proven bound of any frame's length — of
        the panorama's size while fetch_rgbe() delivers the scene-linear panorama (render_environment)."""
        s, n = DeRgbe(), ctypes.c_uint64()
        check(self._lib.de_get_rgbe(self._h, ctypes.byref(s)))
        check(self._lib.de_rgbe_capacity(self._h, ctypes.byref(n)))
        return dict(source=_native.EXR_SOURCES[s.source], rle=bool(s.rle), rounding=next(k for k, x in _native.RGBE_ROUNDINGS.items() if x == s.rounding),
                    scale=float(s.scale), size=self._exr_size(), capacity=int(n.value))

    def fetch_rgbe(self, copy=True, lag=0):
        """The scene-linear frame as one complete Radiance .hdr file: `bytes` that open(path, "wb").write() takes as they are
        (digital_earth_amd.rgbe.read opens them again).  Only the file's own bytes cross the link.  copy=False, lag: as fetch_exr's, through a ring
        of its own; fetch_pending_rgbe() hands out the rest.  Behind render_environment() with the panorama on: the 360° environment map."""
        return self._rg_coded.fetch(self, copy, lag)

    def fetch_pending_rgbe(self, copy=True, all_images=False):
        """fetch_pending() for the lagged fetch_rgbe() calls and their ring."""
        return self._rg_coded.pending(self, copy, all_images)

    def render_to_rgbe(self):
        """Run the stages up to the source's and the encoder and leave the file on the device (de_render_to_rgbe); returns (address of the file,
        address of its uint64 length).  Nothing is waited for."""
        return self._rg_coded.render_to(self)

    def debug_rgbe(self, image, rle=True, rounding="trunc", scale=1.0):
        """The encoder once on a given (H, W, 3) float32 image in R, G, B order, rows top-down, of any size (de_debug_rgbe); returns the file as
        bytes.  The renderer's own settings and streams are not touched."""
        image = np.ascontiguousarray(image, dtype=np.float32)
        if image.ndim != 3 or image.shape[2] != 3:
            raise ValueError("image must have shape (H, W, 3)")
        H, W = image.shape[:2]
        s = self._rg_settings("mean", rle, rounding, scale)
        return self._coded_debug(self._lib.de_debug_rgbe_framing, (ctypes.byref(s), W, H), lambda out, size, n: self._lib.de_debug_rgbe(
            self._h, image.ctypes.data, W, H, ctypes.byref(s), out, size, n))

    def debug_environment_rgbe(self, faces, size, projection="equirect", aperture=180.0, apron=1, supersample=2, basis=None, rle=True, rounding="trunc", scale=1.0):
        """The resampling and the RGBE conversion once on given LINEAR faces, (6, n, n, 3) float32 as debug_panorama takes them
        (de_debug_environment_rgbe); returns the file as bytes.  The renderer's own settings and faces are not touched."""
        faces = np.ascontiguousarray(faces, dtype=np.float32)
        if faces.ndim != 4 or faces.shape[0] != 6 or faces.shape[1] != faces.shape[2] or faces.shape[3] != 3:
            raise ValueError("faces must have shape (6, n, n, 3)")
        p = self._panorama_settings(size, projection, aperture, apron, supersample, basis, True)
        s = self._rg_settings("mean", rle, rounding, scale)
        return self._coded_debug(self._lib.de_debug_rgbe_framing, (ctypes.byref(s), int(size[0]), int(size[1])), lambda out, n_bytes, n: self._lib.de_debug_environment_rgbe(
            self._h, faces.ctypes.data, int(faces.shape[1]), ctypes.byref(p), ctypes.byref(s), out, n_bytes, n))

    # ------------------------------------------------------------------ IBL output (include/digital_earth_ibl.h)
    def _ibl_settings(self, edge, levels, samples, supersample, lod_bias, pixel_type):
        if pixel_type not in _native.EXR_PIXEL_TYPES:
            raise ValueError("pixel_type must be one of %s" % (tuple(_native.EXR_PIXEL_TYPES),))
        s = DeIbl()
        s.struct_bytes = ctypes.sizeof(DeIbl)
        s.edge, s.levels, s.samples, s.supersample = int(edge), int(levels), int(samples), int(supersample)
        s.lod_bias, s.pixel_type = float(lod_bias), _native.EXR_PIXEL_TYPES[pixel_type]
        return s

    def set_ibl(self, edge=128, levels=6, samples=256, supersample=2, lod_bias=0.0, pixel_type="half"):
        """The settings of build_ibl(): a cube map of `edge` (a power of two, 8 ... 1024) with `levels` GGX-prefiltered levels (level l: edge >> l,
        roughness l / (levels - 1)), `samples` per texel (a power of two, 8 ... 1024), the base level's `supersample` (1 ... 4), a bias on every
        sample's source level of detail, and the DDS file's pixel type, "half" or "float".  Drops the product of an earlier build_ibl()."""
        s = self._ibl_settings(edge, levels, samples, supersample, lod_bias, pixel_type)
        check(self._lib.de_set_ibl(self._h, ctypes.byref(s)))

    @property
    def ibl(self):
        """The IBL settings as a dict (set_ibl's keywords) plus file_bytes, the DDS file's length."""
        s, n = DeIbl(), ctypes.c_uint64()
        check(self._lib.de_get_ibl(self._h, ctypes.byref(s)))
        check(self._lib.de_ibl_file_bytes(self._h, ctypes.byref(n)))
        return dict(edge=int(s.edge), levels=int(s.levels), samples=int(s.samples), supersample=int(s.supersample), lod_bias=float(s.lod_bias),
                    pixel_type=next(k for k, x in _native.EXR_PIXEL_TYPES.items() if x == s.pixel_type), file_bytes=int(n.value))

    def build_ibl(self):
        """Bake the six linear faces as they stand (behind render_environment(), the panorama on) into the cube map, its GGX-prefiltered levels, the SH
        coefficients of the irradiance and the DDS payload, on the GPU (de_ibl_build).  The fetch_ibl_* calls hand the product out."""
        check(self._lib.de_ibl_build(self._h))

    def fetch_ibl_sh(self):
        """The irradiance's spherical-harmonic coefficients, (3, 9) float32: rows R, G, B; l = 0 ... 2, the cosine lobe applied."""
        out = np.empty((3, 9), dtype=np.float32)
        check(self._lib.de_fetch_ibl_sh(self._h, out.ctypes.data))
        return out

    def fetch_ibl_face(self, level, face):
        """Face 0 ... 5 (+r, -r, +u, -u, +f, -f: the DDS order) of specular level `level` as (e, e, 3) float32, e = edge >> level, rows top first."""
        e = self.ibl["edge"] >> max(0, min(int(level), 30))
        out = np.empty((max(e, 1), max(e, 1), 3), dtype=np.float32)
        check(self._lib.de_fetch_ibl_face(self._h, int(level), int(face), out.ctypes.data))
        return out

    def fetch_ibl_dds(self):
        """The whole product as one DDS cube map file with the DX10 header (`bytes`): digital_earth_amd.dds.read opens it again."""
        n = self.ibl["file_bytes"]
        out = ctypes.create_string_buffer(n)
        check(self._lib.de_fetch_ibl_dds(self._h, out, ctypes.c_uint64(n)))
        return out.raw

    def debug_ibl(self, faces, apron=1, basis=None, edge=16, levels=5, samples=8, supersample=1, lod_bias=0.0, pixel_type="half"):
        """The bake once on given LINEAR faces, (6, n, n, 3) float32 as debug_panorama takes them (de_debug_ibl).  Returns (sh (3, 9), levels, dds):
        levels[l] is (6, e, e, 3) float32.  The renderer's own settings, faces and product are not touched."""
        faces = np.ascontiguousarray(faces, dtype=np.float32)
        if faces.ndim != 4 or faces.shape[0] != 6 or faces.shape[1] != faces.shape[2] or faces.shape[3] != 3:
            raise ValueError("faces must have shape (6, n, n, 3)")
        p = self._panorama_settings((16, 8), "equirect", 180.0, apron, 1, basis, True)
        s = self._ibl_settings(edge, levels, samples, supersample, lod_bias, pixel_type)
        edges = [max(int(edge) >> l, 0) for l in range(max(int(levels), 0))]
        flat = np.empty(max(sum(18 * e * e for e in edges), 1), dtype=np.float32)
        n = 148 + sum(6 * e * e for e in edges) * (8 if pixel_type == "half" else 16)
        sh, dds = np.empty((3, 9), dtype=np.float32), ctypes.create_string_buffer(n)
        check(self._lib.de_debug_ibl(self._h, faces.ctypes.data, int(faces.shape[1]), ctypes.byref(p), ctypes.byref(s), sh.ctypes.data, flat.ctypes.data, dds, ctypes.c_uint64(n)))
        out, at = [], 0
        for e in edges:
            out.append(flat[at:at + 18 * e * e].reshape(6, e, e, 3).copy())
            at += 18 * e * e
        return sh, out, dds.raw

    # ------------------------------------------------------------------ IBL output, BC6H-compressed (include/digital_earth_ibl_bc6h.h)
    @staticmethod
    def _ibl_bc6h_settings(on, quality):
        s = DeIblBc6h()
        s.struct_bytes, s.on, s.quality = ctypes.sizeof(DeIblBc6h), 1 if on else 0, int(quality)
        return s

    def set_ibl_bc6h(self, on=True, quality=0):
        """The BC6H stage of the IBL output: with it on, fetch_ibl_bc6h_dds() delivers the cube chain as BC6H_UF16 blocks, 1 byte per texel.  quality
        0: mode 11 alone; 1: the 32 two-region partitions as well.  Every other fetch is unchanged.  Drops the blocks of an earlier fetch."""
        s = self._ibl_bc6h_settings(on, quality)
        check(self._lib.de_set_ibl_bc6h(self._h, ctypes.byref(s)))

    @property
    def ibl_bc6h(self):
        """The BC6H stage's settings as a dict (set_ibl_bc6h's keywords) plus file_bytes, the compressed file's length under the IBL settings."""
        s, n = DeIblBc6h(), ctypes.c_uint64()
        check(self._lib.de_get_ibl_bc6h(self._h, ctypes.byref(s)))
        check(self._lib.de_ibl_bc6h_file_bytes(self._h, ctypes.byref(n)))
        return dict(on=bool(s.on), quality=int(s.quality), file_bytes=int(n.value))

    def fetch_ibl_bc6h_dds(self):
        """The product of build_ibl() as one DDS cube map file of BC6H_UF16 blocks (`bytes`): digital_earth_amd.bc6h.read opens it again."""
        n = self.ibl_bc6h["file_bytes"]
        out = ctypes.create_string_buffer(n)
        check(self._lib.de_fetch_ibl_bc6h_dds(self._h, out, ctypes.c_uint64(n)))
        return out.raw

    def debug_bc6h_encode(self, image, quality=0):
        """The encoder alone on an (h, w, 3) float32 image, any h, w >= 1 (de_debug_bc6h_encode): ceil(w / 4) ceil(h / 4) blocks as `bytes`, rows of
        blocks top first.  The renderer's own settings and product are not touched."""
        image = np.ascontiguousarray(image, dtype=np.float32)
        if image.ndim != 3 or image.shape[2] != 3:
            raise ValueError("image must have shape (h, w, 3)")
        s = self._ibl_bc6h_settings(True, quality)
        n = 16 * ((image.shape[1] + 3) // 4) * ((image.shape[0] + 3) // 4)
        out = ctypes.create_string_buffer(max(n, 1))
        check(self._lib.de_debug_bc6h_encode(self._h, image.ctypes.data, int(image.shape[1]), int(image.shape[0]), ctypes.byref(s), out, ctypes.c_uint64(n)))
        return out.raw[:n]

    def debug_ibl_bc6h(self, faces, quality=0, apron=1, basis=None, edge=16, levels=5, samples=8, supersample=1, lod_bias=0.0):
        """debug_ibl() with the compressed file out (de_debug_ibl_bc6h).  Returns (sh (3, 9), levels, half_levels, dds): levels[l] is (6, e, e, 3)
        float32, half_levels[l] the same texels as uint16 half integers 0 ... 0x7BFF — what the blocks of dds encode."""
        faces = np.ascontiguousarray(faces, dtype=np.float32)
        if faces.ndim != 4 or faces.shape[0] != 6 or faces.shape[1] != faces.shape[2] or faces.shape[3] != 3:
            raise ValueError("faces must have shape (6, n, n, 3)")
        p = self._panorama_settings((16, 8), "equirect", 180.0, apron, 1, basis, True)
        s = self._ibl_settings(edge, levels, samples, supersample, lod_bias, "half")
        b = self._ibl_bc6h_settings(True, quality)
        edges = [max(int(edge) >> l, 0) for l in range(max(int(levels), 0))]
        total = max(sum(18 * e * e for e in edges), 1)
        flat, halves = np.empty(total, dtype=np.float32), np.empty(total, dtype=np.uint16)
        n = 148 + 96 * sum(max(1, e // 4) ** 2 for e in edges)
        sh, dds = np.empty((3, 9), dtype=np.float32), ctypes.create_string_buffer(n)
        check(self._lib.de_debug_ibl_bc6h(self._h, faces.ctypes.data, int(faces.shape[1]), ctypes.byref(p), ctypes.byref(s), ctypes.byref(b), sh.ctypes.data, flat.ctypes.data,
                                          halves.ctypes.data, dds, ctypes.c_uint64(n)))
        out, out_half, at = [], [], 0
        for e in edges:
            out.append(flat[at:at + 18 * e * e].reshape(6, e, e, 3).copy())
            out_half.append(halves[at:at + 18 * e * e].reshape(6, e, e, 3).copy())
            at += 18 * e * e
        return sh, out, out_half, dds.raw

    # ------------------------------------------------------------------ look LUTs (include/digital_earth_look.h)
    LOOK_INTERPOLATIONS = ("trilinear", "tetrahedral")

    @staticmethod
    def _look_table(item, kind, what):
        """A path or a Cube -> the Cube, of the kind the slot takes."""
        from . import cube as cube_mod
        if item is None:
            return None
        c = item if isinstance(item, cube_mod.Cube) else cube_mod.read_cube(os.fspath(item))
        if c.kind != kind:
            raise ValueError("%s takes a %s table, not a %s one" % (what, kind.upper(), c.kind.upper()))
        return c

    def _look_settings(self, cube, shaper, strength, interpolation, enabled):
        """(DeLook, 1D table or None, 3D table or None); the arrays must outlive the call they are passed to."""
        if interpolation not in self.LOOK_INTERPOLATIONS:
            raise ValueError("interpolation must be one of %s" % (self.LOOK_INTERPOLATIONS,))
        s = DeLook()
        s.struct_bytes = ctypes.sizeof(DeLook)
        s.enabled, s.interpolation, s.strength = 1 if enabled else 0, self.LOOK_INTERPOLATIONS.index(interpolation), float(strength)
        t1 = t3 = None
        if shaper is not None:
            s.size_1d, s.min_1d, s.max_1d = shaper.size, (ctypes.c_float * 3)(*shaper.domain_min), (ctypes.c_float * 3)(*shaper.domain_max)
            t1 = np.ascontiguousarray(np.frombuffer(shaper.table, dtype=np.float32))
        if cube is not None:
            s.size_3d, s.min_3d, s.max_3d = cube.size, (ctypes.c_float * 3)(*cube.domain_min), (ctypes.c_float * 3)(*cube.domain_max)
            t3 = np.ascontiguousarray(np.frombuffer(cube.table, dtype=np.float32))
        return s, t1, t3

    def set_look(self, cube=None, shaper=None, strength=1.0, interpolation="tetrahedral", enabled=True):
        """Grade the displayed image through lookup tables on the GPU, directly behind the display transform: `cube` is a 3D table, `shaper` a 1D
        table applied ahead of it; each is the path of a .cube file, a digital_earth_amd.cube.Cube or None (no such table).  The graded pixel is
        mixed with the ungraded one by `strength` in [0, 1] and clamped to [0, 1]; interpolation "tetrahedral" or "trilinear" is the 3D table's.
        Every fetch of the displayed image — fetch_image, fetch_pixels, fetch_hdr_pixels, fetch_video, their views and rings,
        render_to_image_device, behind output scaling too — delivers the graded image; fetch_hdr() and the intermediate fetches do not change.
        The tables act on whatever signal the display wrote: load one made for that signal (an SDR look for the SDR picture, a PQ one under
        set_hdr_output(transfer="pq")).  With neither `cube` nor `shaper` the tables of the previous call are kept: set_look(enabled=False)
        turns the stage off, set_look() turns it on again, set_look(strength=0.5) changes the mix.  May be called while lagged fetches are in flight."""
        if cube is None and shaper is None:
            cube, shaper = getattr(self, "_look_held", (None, None))
            if cube is None and shaper is None and enabled:
                raise ValueError("set_look needs a cube or a shaper")
        else:
            cube, shaper = self._look_table(cube, "3d", "cube"), self._look_table(shaper, "1d", "shaper")
        s, t1, t3 = self._look_settings(cube, shaper, strength, interpolation, enabled)
        check(self._lib.de_set_look(self._h, ctypes.byref(s), t1.ctypes.data if t1 is not None else None, t3.ctypes.data if t3 is not None else None))
        self._look_held = (cube, shaper)

    def look(self):
        """The look as a dict — enabled, strength, interpolation, and per table its size and domain (cube_size, cube_domain, shaper_size,
        shaper_domain; size 0 and domain None without that table) — or None while the stage is off."""
        s = DeLook()
        check(self._lib.de_get_look(self._h, ctypes.byref(s)))
        if not s.enabled:
            return None
        return dict(enabled=True, strength=float(s.strength), interpolation=self.LOOK_INTERPOLATIONS[s.interpolation],
                    cube_size=int(s.size_3d), cube_domain=(tuple(s.min_3d), tuple(s.max_3d)) if s.size_3d else None,
                    shaper_size=int(s.size_1d), shaper_domain=(tuple(s.min_1d), tuple(s.max_1d)) if s.size_1d else None)

    def debug_look(self, rgb, cube=None, shaper=None, strength=1.0, interpolation="tetrahedral"):
        """The look kernel once on (..., 3) float32 pixels (de_debug_look), with tables given as to set_look; returns the graded pixels in the same
        shape.  The renderer's own look is not touched."""
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        if rgb.ndim < 1 or rgb.shape[-1] != 3:
            raise ValueError("rgb must have shape (..., 3)")
        s, t1, t3 = self._look_settings(self._look_table(cube, "3d", "cube"), self._look_table(shaper, "1d", "shaper"), strength, interpolation, True)
        out = np.empty_like(rgb)
        check(self._lib.de_debug_look(self._h, rgb.ctypes.data, ctypes.c_uint64(rgb.size // 3), ctypes.byref(s),
                                      t1.ctypes.data if t1 is not None else None, t3.ctypes.data if t3 is not None else None, out.ctypes.data))
        return out

    # ------------------------------------------------------------------ HDR display output (include/digital_earth_hdr_output.h)
    HDR_GAMUTS =("rec709", "p3d65", "rec2020")
    HDR_TRANSFERS = ("linear", "pq", "hlg")
    HDR_PIXEL_FORMATS = ("rgb10a2", "rgb16")

    def _hdr_output_settings(self, on, peak_nits, gamut, transfer, pixel_format, mode, seed, animate):
        for value, names, what in ((gamut, self.HDR_GAMUTS, "gamut"), (transfer, self.HDR_TRANSFERS, "transfer"), (pixel_format, self.HDR_PIXEL_FORMATS, "pixel_format"),
                                   (mode, self.PIXEL_MODES, "mode")):
            if value not in names:
                raise ValueError("%s must be one of %s" % (what, names))
        s = DeHdrOutput()
        s.struct_bytes = ctypes.sizeof(DeHdrOutput)
        s.on, s.peak_nits = 1 if on else 0, float(peak_nits)
        s.gamut, s.transfer, s.pixel_format = self.HDR_GAMUTS.index(gamut), self.HDR_TRANSFERS.index(transfer), self.HDR_PIXEL_FORMATS.index(pixel_format)
        s.mode, s.seed, s.animate = self.PIXEL_MODES.index(mode), int(seed) & 0xffffffff, 1 if animate else 0
        return s

    def set_hdr_output(self, on=True, peak_nits=1000.0, gamut="rec2020", transfer="pq", pixel_format="rgb10a2", mode="truncate", seed=0, animate=False):
        """Turn the HDR display output on (or off).  While it is on, the display transform is OpenDRT in its general form instead of the 100-nit sRGB
        picture: rendered for a display of `peak_nits` (100 ... 10000) in the `gamut` "rec709", "p3d65" or "rec2020" and encoded by the `transfer`
        "linear" (1.0 = the peak), "pq" (ST 2084) or "hlg".  The camera response curve, gamma and the sRGB OETF are NOT applied in this mode: an SDR film
        curve and an SDR encoding.  fetch_image() then returns that signal as floats in [0, 1], output scaling resamples it, fetch_pixels() keeps working on
        it (8 bits of PQ: legal but coarse), and fetch_hdr_pixels() packs it to `pixel_format` "rgb10a2" or "rgb16" in `mode` "truncate", "round" or
        "dither" (set_pixels' modes, seed and animate).  Everything ahead of the display — adaptive counts, the denoiser, history, auto-exposure, bloom,
        local exposure — is inherited.  Refused (DE_ERR_STATE at the next display) together with the AgX display transform.
        KNOWN LIMIT, kept from the reference: only gamut="rec709" is colorimetrically meaningful.  The reference's two gamut products multiply by the
        transposed matrices, which cancels for Rec.709 only; under "p3d65" and "rec2020" — the default — every neutral comes out strongly green (0.18
        grey gives the signal (0.256, 0.383, 0.339) at 1000-nit Rec.2020 PQ).  This method reproduces the reference; pass gamut="rec709" for a
        picture meant for a panel.  Whether 1000-nit PQ at the
        default exposure looks right on a panel has not been judged: the defaults are starting values.  fetch_hdr() is unchanged."""
        check(self._lib.de_set_hdr_output(self._h, ctypes.byref(self._hdr_output_settings(on, peak_nits, gamut, transfer, pixel_format, mode, seed, animate))))

    @property
    def hdr_output(self):
        """The HDR display output as a dict (set_hdr_output's keywords) plus last_phase, or None while it is off."""
        s, phase = DeHdrOutput(), ctypes.c_uint32()
        check(self._lib.de_get_hdr_output(self._h, ctypes.byref(s), ctypes.byref(phase)))
        if not s.on:
            return None
        return dict(on=True, peak_nits=float(s.peak_nits), gamut=self.HDR_GAMUTS[s.gamut], transfer=self.HDR_TRANSFERS[s.transfer],
                    pixel_format=self.HDR_PIXEL_FORMATS[s.pixel_format], mode=self.PIXEL_MODES[s.mode], seed=int(s.seed), animate=bool(s.animate),
                    last_phase=int(phase.value))

    def fetch_hdr_pixels(self):
        """The displayed HDR signal as packed pixels of the output size, converted on the GPU, rows top-down: uint32 (H, W) for "rgb10a2" (R in bits
        0-9, G in 10-19, B in 20-29, alpha 3 in 30-31) or uint16 (H, W, 3) for "rgb16".  The HDR display output must be on."""
        if not self._textures_copied:
            self.copy_textures()
        s = DeHdrOutput()
        check(self._lib.de_get_hdr_output(self._h, ctypes.byref(s), None))
        ow, oh = self.output_size()
        out = np.empty((oh, ow, 3), dtype=np.uint16) if s.pixel_format == 1 else np.empty((oh, ow), dtype=np.uint32)
        check(self._lib.de_fetch_hdr_pixels(self._h, out.ctypes.data, ctypes.c_uint64(out.nbytes)))
        return out

    def render_to_hdr_pixels_device(self):
        """Run the display and the HDR pack and leave the pixels on the device (de_render_to_hdr_pixels); returns their address."""
        if not self._textures_copied:
            self.copy_textures()
        p = ctypes.c_void_p()
        check(self._lib.de_render_to_hdr_pixels(self._h, ctypes.byref(p)))
        return p.value

    def debug_hdr_transform(self, rgb, peak_nits=1000.0, gamut="rec2020", transfer="pq"):
        """The HDR display transform alone on (..., 3) float32 scene-linear Rec.709 colours, already exposed (de_debug_hdr_transform); returns the
        signal in the same shape.  The renderer's own setting is not touched."""
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        if rgb.ndim < 1 or rgb.shape[-1] != 3:
            raise ValueError("rgb must have shape (..., 3)")
        out = np.empty_like(rgb)
        s = self._hdr_output_settings(True, peak_nits, gamut, transfer, "rgb10a2", "truncate", 0, False)
        check(self._lib.de_debug_hdr_transform(self._h, rgb.ctypes.data, ctypes.c_uint64(rgb.size // 3), ctypes.byref(s), out.ctypes.data))
        return out

    def fetch_hdr(self):
        out = np.empty((self.image_res[0], self.image_res[1], 3), dtype=np.float32)
        check(self._lib.de_fetch_hdr(self._h, out.ctypes.data))
        return out

    # ------------------------------------------------------------------ measurement / plumbing
    def synchronize(self):
        check(self._lib.de_synchronize(self._h))

    def last_accumulate_ms(self):
        ms = ctypes.c_float()
        check(self._lib.de_last_accumulate_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def enable_counters(self, on=True):
        check(self._lib.de_enable_counters(self._h, 1 if on else 0))

    def set_kernel_variant(self, variant):
        """4 = automatic (default): a call of at least 4096 paths runs the per-CU stage scheduler (render_kernel_v6: one persistent launch, + a small
        tail launch for big calls), smaller calls and counting launches the wave-level state machine; 2 / 6 = that kernel for every call.  1, 3, 5
        (per-lane loops, wavefront pipeline, HBM-queue scheduler) exist in the legacy library only.  Identical results, bit for bit."""
        check(self._lib.de_set_kernel_variant(self._h, int(variant)))

    def set_memory_budget(self, n_bytes):
        """Bytes the context may hold in pipeline queues / cold records / chunk pools (0 = automatic); include/digital_earth.h."""
        check(self._lib.de_set_memory_budget(self._h, ctypes.c_uint64(int(n_bytes))))

    def memory_use(self):
        n = ctypes.c_uint64()
        check(self._lib.de_get_memory_use(self._h, ctypes.byref(n)))
        return int(n.value)

    def last_call_info(self):
        """What the last accumulate() ran: dict(variant, pipes, depths, launches, kernel) — include/digital_earth.h."""
        v = [ctypes.c_int() for _ in range(4)]
        check(self._lib.de_last_call_info(self._h, *[ctypes.byref(x) for x in v]))
        variant, pipes, depths, launches = (int(x.value) for x in v)
        name = {0: "ray marcher", 1: "per-lane loops", 2: "state machine", 5: "persistent stage scheduler", 6: "per-CU stage scheduler",
                3: "pipeline x%d, %d rounds%s" % (pipes, depths, " + state machine" if depths < 25 else "")}.get(variant, "?")
        return dict(variant=variant, pipes=pipes, depths=depths, launches=launches, kernel=name)

    def last_launch_phases(self):
        """(launch_ms, drain_ms) of the last render_kernel_v6 launch, from the kernel's own clock: the drain is the time between the
        first wave that found no work item left and the last wave's exit (include/digital_earth.h)."""
        ms = (ctypes.c_float * 2)()
        check(self._lib.de_last_launch_phases(self._h, ms))
        return float(ms[0]), float(ms[1])

    def tuning(self):
        """The context's de_tuning (include/digital_earth.h) as a ctypes struct; change fields and pass it to set_tuning."""
        t = _native.DeTuning()
        check(self._lib.de_get_tuning(self._h, ctypes.byref(t)))
        return t

    def set_tuning(self, t):
        check(self._lib.de_set_tuning(self._h, ctypes.byref(t)))

    def v5_stats(self, n=24):
        """Statistics block of the persistent stage scheduler (legacy library, kernel variant 5 with DE_V5_STATS=1); include/digital_earth_legacy.h."""
        if not hasattr(self._lib, "de_debug_v5_stats"):
            raise RuntimeError("de_debug_v5_stats lives in the legacy library (DE_LIB_PATH=.../libdigitalearth_hip_legacy.so)")
        out = (ctypes.c_uint64 * n)()
        check(self._lib.de_debug_v5_stats(self._h, out, n))
        return [int(x) for x in out]

    def v6_stats(self, n=48):
        """Statistics block of the per-CU stage scheduler (kernel variant 6 with DE_V6_STATS=1); include/digital_earth.h."""
        out = (ctypes.c_uint64 * n)()
        check(self._lib.de_debug_v6_stats(self._h, out, n))
        return [int(x) for x in out]

    def counters(self):
        c = DeCounters()
        check(self._lib.de_get_counters(self._h, ctypes.byref(c)))
        return c.as_dict()

    def sched_stats(self, n=48):
        """Raw scheduler statistics of render_kernel_v2 (counters must be enabled); see tools/sched_stats.py."""
        out = (ctypes.c_uint64 * n)()
        check(self._lib.de_debug_sched_stats(self._h, out, n))
        return [int(x) for x in out]

    def hdr_device_pointer(self):
        p, n = ctypes.c_void_p(), ctypes.c_uint64()
        check(self._lib.de_hdr_device_ptr(self._h, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def bind_hdr(self, device_ptr, n_floats):
        """Accumulate into caller-owned device memory (e.g. a torch tensor) instead of the library's buffer."""
        check(self._lib.de_bind_hdr(self._h, ctypes.c_void_p(device_ptr), int(n_floats)))

    def unbind(self):
        """Back to the library's own HDR buffer and stream (undoes bind_hdr / set_stream)."""
        check(self._lib.de_bind_hdr(self._h, None, 0))
        check(self._lib.de_use_own_stream(self._h))
        self._bound = None

    # in-library collective (include/digital_earth.h: de_comm_*, de_reduce)
    def comm_unique_id(self):
        buf = ctypes.create_string_buffer(128)
        check(self._lib.de_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, unique_id, rank, world):
        if len(unique_id) != 128:
            raise ValueError("the RCCL unique id is 128 bytes")
        check(self._lib.de_comm_init(self._h, ctypes.c_char_p(bytes(unique_id)), int(rank), int(world)))

    def comm_destroy(self):
        check(self._lib.de_comm_destroy(self._h))

    def reduce(self, root=0, comm=None):
        """Sum the HDR buffers of all ranks onto `root` (RCCL, in place, on the context's stream)."""
        check(self._lib.de_reduce(self._h, ctypes.c_void_p(comm) if comm else None, int(root)))

    def reduce_progressive(self, root=0, comm=None):
        """Out-of-place sum onto `root`: this rank keeps accumulating; the root displays the assembled frame (progressive mode)."""
        check(self._lib.de_reduce_progressive(self._h, ctypes.c_void_p(comm) if comm else None, int(root)))

    def reduce_ordered(self, root=0, comm=None, out_of_place=False):
        """Sample partition: gather the ranks' HDR buffers on `root` and add them in rank order (in place, or into the assembled buffer
        the display reads: progressive mode)."""
        check(self._lib.de_reduce_ordered(self._h, ctypes.c_void_p(comm) if comm else None, int(root), 1 if out_of_place else 0))

    def last_reduce_ms(self):
        ms = ctypes.c_float()
        check(self._lib.de_last_reduce_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def debug_ordered_sum(self, parts, root=0, out_of_place=False):
        """The root's half of reduce_ordered on ONE GPU (include/digital_earth_debug.h): `parts` = per-rank partial sums as (W, H, 3) arrays; part `root`
        is loaded into the accumulation buffer, the others where ncclRecv would put them; the library's own launch adds them in rank order.
        Returns the assembled frame as (W, H, 3)."""
        W, H = self.image_res
        dev = np.ascontiguousarray(np.stack([np.asarray(p, dtype=np.float32).transpose(1, 0, 2) for p in parts]))      # device layout [H][W][3]
        if dev.shape != (len(parts), H, W, 3):
            raise ValueError("every part must have shape (W, H, 3)")
        out = np.empty((H, W, 3), dtype=np.float32)
        check(self._lib.de_debug_ordered_sum(self._h, dev.ctypes.data, len(parts), int(root), 1 if out_of_place else 0, out.ctypes.data))
        return np.ascontiguousarray(out.transpose(1, 0, 2))

    def debug_standin_reduce(self, extra_copies=0):
        """A one-GPU stand-in for the frame's collective, enqueued where reduce() goes (include/digital_earth_debug.h); last_reduce_ms() then
        reports its queue-to-finish latency."""
        check(self._lib.de_debug_standin_reduce(self._h, int(extra_copies)))

    def set_display_source(self, device_ptr):
        """Display / fetch from another [H][W][3] f32 device buffer (None: the accumulation buffer again)."""
        check(self._lib.de_set_display_source(self._h, ctypes.c_void_p(device_ptr) if device_ptr else None))

    def set_launch_slots(self, n_slots, n_big=None):
        """Launches in flight: n_slots for small launches, n_big for big ones (1 = serial)."""
        check(self._lib.de_set_launch_slots(self._h, int(n_slots), int(n_big if n_big is not None else min(n_slots, 3))))

    def set_wave_budget(self, waves_per_cu):
        check(self._lib.de_set_wave_budget(self._h, int(waves_per_cu)))

    def render_to_image_device(self):
        """Run the display transform and leave the image on the device, (W, H, 3) float32 — (width, height, 3) of output_size() while the output scaling
        is on; returns its address."""
        if not self._textures_copied:
            self.copy_textures()
        p = ctypes.c_void_p()
        check(self._lib.de_render_to_image(self._h, ctypes.byref(p)))
        return p.value

    def set_stream(self, hip_stream_handle):
        """Use the caller's HIP stream as the context stream; 0 / None is HIP's null stream (torch's default stream)."""
        check(self._lib.de_set_stream(self._h, ctypes.c_void_p(hip_stream_handle or None)))

    def flush(self):
        """Make the context stream wait (on the device) for every accumulate() issued so far — before the caller enqueues
        work of its own on that stream (parallel.reduce_hdr on the bound tensor)."""
        check(self._lib.de_flush(self._h))

    def upload_hdr(self, hdr, spp):
        """Load an accumulation state ((W, H, 3) float32 sums, sample count) — resume of a progressive render."""
        hdr = np.ascontiguousarray(hdr, dtype=np.float32)
        if hdr.shape != (self.image_res[0], self.image_res[1], 3):
            raise ValueError("hdr must have shape (W, H, 3)")
        check(self._lib.de_upload_hdr(self._h, hdr.ctypes.data, int(spp)))
        self.current_spp = int(spp)

    def save_checkpoint(self, path):
        """Persist the progressive state — HDR sums, sample count, RNG base seed and the scalar parameters — so that a long
        render (BASELINE cfg5: 1024 spp) can be resumed.  The reference keeps this state in memory only (renderer.py:23,25).
        An adaptive frame (accumulate_adaptive) has no checkpoint: its state is a sample count per tile."""
        if getattr(self, "_adaptive", None) is not None:
            raise RuntimeError("an adaptive frame cannot be checkpointed: finish it, or reset_framebuffer()")
        np.savez(path, hdr=self.fetch_hdr(), spp=np.int64(self.current_spp), seed=np.uint64(self.seed),
                 params=np.frombuffer(bytes(self._params), dtype=np.uint8), image_res=np.array(self.image_res))

    def load_checkpoint(self, path):
        """Resume from save_checkpoint(): the next accumulate() continues with sample index `spp`, bit-identically."""
        z = np.load(path)
        if tuple(int(x) for x in z["image_res"]) != self.image_res:
            raise ValueError("checkpoint is %s, renderer is %s" % (tuple(z["image_res"]), self.image_res))
        ctypes.memmove(ctypes.byref(self._params), z["params"].tobytes(), ctypes.sizeof(self._params))
        self._push_params()
        self.seed = int(z["seed"])
        self.upload_hdr(z["hdr"], int(z["spp"]))

    def set_current_spp(self, spp):
        self.current_spp = int(spp)
        check(self._lib.de_set_current_spp(self._h, int(spp)))

    def debug_samples(self, sample_index):
        """Per pixel [H][W]: radiance, wavelength, RNG draws, vertices of sample `sample_index` (not accumulated)."""
        if not self._textures_copied:
            self.copy_textures()
        out = np.empty((self.image_res[1], self.image_res[0], 4), dtype=np.float32)
        check(self._lib.de_debug_samples(self._h, self.seed, int(sample_index), out.ctypes.data))
        return out

    def debug_math(self, fn, a, b=None, fast=False):
        """Function `fn` of include/digital_earth_debug.h on the device; fast=True: the DE_FLAG_FAST_MATH kernel's definitions."""
        a = np.ascontiguousarray(a, dtype=np.float32)
        out = np.empty_like(a)
        bp = None
        if b is not None:
            b = np.ascontiguousarray(b, dtype=np.float32)
            bp = b.ctypes.data
        call = self._lib.de_debug_math_fast if fast else self._lib.de_debug_math
        check(call(self._h, int(fn), a.ctypes.data, bp, out.ctypes.data, a.size))
        return out

    @staticmethod
    def to_vec3u(c):                                                     # renderer.py:386-393
        return (np.clip(np.asarray(c, dtype=np.float32), 0.0, 1.0) * 255).astype(np.uint8)

    @staticmethod
    def to_vec3(c):                                                      # renderer.py:395-401
        return np.asarray(c, dtype=np.float32) / 255.0
