"""The HDR display output's C ABI without a GPU: include/digital_earth_hdr_output.h compiles as pedantic C99 alone and together with the debug header,
the struct mirror matches field by field, the five entry points it declares are bound and exported, the binder's header keeps its 40 entry points at
ABI 6, arguments are refused where the header says so, the host constants equal the restatement's, the Python signatures have the documented defaults,
and the build tracks the new sources."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from digital_earth_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"de_set_hdr_output", "de_get_hdr_output", "de_render_to_hdr_pixels", "de_fetch_hdr_pixels", "de_debug_hdr_transform"}
CTYPE = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "float": ctypes.c_float}
HEADER = "digital_earth_hdr_output.h"


def _header(name=HEADER):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name=HEADER):
    text = re.sub(r"/\*.*?\*/", "", _header(name), flags=re.S)
    return set(re.findall(r"\b(de_[a-z0-9_]+)\s*\(", text))


def _fields():
    body = re.search(r"typedef struct de_hdr_output \{(.*?)\} de_hdr_output;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        m = re.match(r"\s*(uint32_t|int32_t|float)\s+(\w+)\s*$", decl.strip(), re.S)
        if not m:
            assert not decl.strip(), decl
            continue
        out.append((m.group(2), CTYPE[m.group(1)]))
    return out


def _settings(**kw):
    s = _native.DeHdrOutput()
    s.struct_bytes, s.on, s.peak_nits, s.gamut, s.transfer, s.pixel_format, s.mode, s.seed, s.animate = ctypes.sizeof(s), 1, 1000.0, 2, 1, 0, 0, 0, 0
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _lib():
    from digital_earth_amd import build
    build.build()
    return ctypes.CDLL(build.OUT)


def test_struct_matches_header():
    want = _fields()
    assert [n for n, _ in want] == ["struct_bytes", "on", "peak_nits", "gamut", "transfer", "pixel_format", "mode", "seed", "animate"]
    assert [n for n, _ in _native.DeHdrOutput._fields_] == [n for n, _ in want]
    for (n, a), (_, b) in zip(_native.DeHdrOutput._fields_, want):
        assert a is b, n
    assert ctypes.sizeof(_native.DeHdrOutput) == 36
    defs = dict(re.findall(r"#define\s+(DE_HDR_\w+)\s+(\d+)", _header()))
    assert defs == {"DE_HDR_GAMUT_REC709": "0", "DE_HDR_GAMUT_P3D65": "1", "DE_HDR_GAMUT_REC2020": "2", "DE_HDR_TRANSFER_LINEAR": "0", "DE_HDR_TRANSFER_PQ": "1",
                    "DE_HDR_TRANSFER_HLG": "2", "DE_HDR_PIXELS_RGB10A2": "0", "DE_HDR_PIXELS_RGB16": "1"}
    text = _header()
    assert "Out of scope" in text and "_begin / _end" in text                      # the header says that these pixels have no pinned ring
    assert "camera response" in text and "sRGB OETF" in text and "NOT applied" in text


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_header_compiles_as_pedantic_c99(tmp_path):
    inc = os.path.join(ROOT, "include")
    for first, second in ((HEADER, "digital_earth_debug.h"), ("digital_earth_debug.h", HEADER)):
        src = tmp_path / "t.c"
        src.write_text('#include "%s"\n#include "%s"\n' % (first, second) +
                       'int main(void) { de_hdr_output s; s.struct_bytes = sizeof s; (void)de_debug_hdr_consts; (void)de_debug_hdr_transform;'
                       ' return s.struct_bytes != 36 || DE_HDR_TRANSFER_HLG != 2 || DE_PIXELS_DITHER != 2; }\n')
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, "-c", str(src), "-o", str(tmp_path / "t.o")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    src.write_text('#include "%s"\nint main(void) { de_hdr_output s; s.struct_bytes = sizeof s; return s.struct_bytes != 36; }\n' % HEADER)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, str(src), "-o", str(tmp_path / "t")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


def test_symbols_declared_bound_and_exported():
    assert _declared() == set(_native.HDR_OUTPUT_SYMBOLS) == NAMES
    others = (set(_native.SYMBOLS) | set(_native.DEBUG_SYMBOLS) | set(_native.DENOISE_SYMBOLS) | set(_native.EXPOSURE_SYMBOLS) | set(_native.BLOOM_SYMBOLS)
              | set(_native.HISTORY_SYMBOLS) | set(_native.PIXELS_SYMBOLS) | set(_native.LOCAL_EXPOSURE_SYMBOLS) | set(_native.OUTPUT_SCALE_SYMBOLS) | set(_native.LEGACY_SYMBOLS))
    assert not NAMES & others
    assert len(_declared("digital_earth.h")) == 40 and not (NAMES | {"de_debug_hdr_consts"}) & _declared("digital_earth.h")      # the binder's own list is unchanged
    assert re.search(r"#define\s+DE_ABI_VERSION\s+6\b", _header("digital_earth.h"))
    for name in ("de_set_hdr_output", "de_get_hdr_output"):
        res, args = _native.HDR_OUTPUT_SYMBOLS[name]
        assert res is ctypes.c_int and args[1]._type_ is _native.DeHdrOutput
    assert _native.HDR_OUTPUT_SYMBOLS["de_get_hdr_output"][1][2]._type_ is ctypes.c_uint32
    assert _native.HDR_OUTPUT_SYMBOLS["de_fetch_hdr_pixels"][1][2] is ctypes.c_uint64
    res, args = _native.HDR_OUTPUT_SYMBOLS["de_debug_hdr_transform"]
    assert res is ctypes.c_int and len(args) == 5 and args[2] is ctypes.c_uint64 and args[3]._type_ is _native.DeHdrOutput
    assert "de_debug_hdr_consts" in _declared("digital_earth_debug.h") and "de_debug_hdr_consts" in _native.DEBUG_SYMBOLS
    assert "HDR_OUTPUT_SYMBOLS" in inspect.getsource(_native.load)
    lib = _lib()
    for name in NAMES | {"de_debug_hdr_consts"}:
        assert hasattr(lib, name), name
    lib.de_abi_version.restype = ctypes.c_int
    assert lib.de_abi_version() == 6 == _native.ABI_VERSION


def test_arguments_are_refused_without_a_device():
    """The checks that come before any device work: null arguments, struct_bytes, peak_nits, the enums — through the host-only constants entry point,
    which validates with de_set_hdr_output's own check, and through the entry points' null checks."""
    lib = _lib()
    consts = lib.de_debug_hdr_consts
    consts.restype, consts.argtypes = _native.DEBUG_SYMBOLS["de_debug_hdr_consts"]
    ctx = None                    # the hook is host only: its context is not read and may be NULL (include/digital_earth_debug.h)
    out = np.zeros(19, np.float32)
    assert consts(ctx, ctypes.byref(_settings()), out.ctypes.data) == 0
    nan, inf = float("nan"), float("inf")
    for kw in (dict(struct_bytes=32), dict(struct_bytes=40), dict(peak_nits=99.0), dict(peak_nits=10001.0), dict(peak_nits=nan), dict(peak_nits=inf), dict(peak_nits=-1000.0),
               dict(gamut=-1), dict(gamut=3), dict(transfer=-1), dict(transfer=3), dict(pixel_format=-1), dict(pixel_format=2), dict(mode=-1), dict(mode=3)):
        assert consts(ctx, ctypes.byref(_settings(**kw)), out.ctypes.data) == _native.DE_ERR_INVALID, kw
        assert consts(ctx, ctypes.byref(_settings(on=0, **kw)), out.ctypes.data) == _native.DE_ERR_INVALID, kw      # checked whether `on` is set or not
    for kw in (dict(peak_nits=100.0), dict(peak_nits=10000.0), dict(gamut=0, transfer=2, pixel_format=1, mode=2, seed=0xffffffff, animate=1)):
        assert consts(ctx, ctypes.byref(_settings(**kw)), out.ctypes.data) == 0, kw
    assert consts(ctx, None, out.ctypes.data) == 0                                # no settings: the SDR display's own six constants (below)
    assert consts(ctx, ctypes.byref(_settings()), None) == _native.DE_ERR_INVALID
    for name, args in (("de_set_hdr_output", (None, None)), ("de_get_hdr_output", (None, None, None)), ("de_render_to_hdr_pixels", (None, None)),
                       ("de_fetch_hdr_pixels", (None, None, 0)), ("de_debug_hdr_transform", (None, None, 0, None, None))):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _native.HDR_OUTPUT_SYMBOLS[name]
        assert fn(*args) == _native.DE_ERR_INVALID, name
    lib.de_last_error.restype = ctypes.c_char_p
    assert consts(ctx, ctypes.byref(_settings(peak_nits=50.0)), out.ctypes.data) == _native.DE_ERR_INVALID and b"peak_nits" in lib.de_last_error()


def test_host_constants_equal_the_restatement():
    """hdr_output_consts of csrc/de_host_consts.h against tests/hdr_output_ref.py: both evaluate the same double expressions; the roundings to f32 may
    differ by the last bit where the two libms' pow / log10 do."""
    import hdr_output_ref as ho
    lib = _lib()
    consts = lib.de_debug_hdr_consts
    consts.restype, consts.argtypes = _native.DEBUG_SYMBOLS["de_debug_hdr_consts"]
    for peak in (100.0, 600.0, 1000.0, 4000.0, 10000.0):
        for g, gamut in enumerate(ho.GAMUTS):
            for t, transfer in enumerate(ho.TRANSFERS):
                out = np.zeros(19, np.float32)
                assert consts(None, ctypes.byref(_settings(peak_nits=peak, gamut=g, transfer=t)), out.ctypes.data) == 0
                want = ho.constants_vector(ho.constants(peak, gamut, transfer))
                assert (np.abs(out.astype(np.float64) - want) <= np.spacing(np.abs(want))).all(), (peak, gamut, transfer, out, want)
    out = np.zeros(19, np.float32)
    assert consts(None, ctypes.byref(_settings(peak_nits=100.0, gamut=0, transfer=0)), out.ctypes.data) == 0
    assert out[2] == np.float32(0.005) and out[3] == 1.0 and out[4] == 1.0      # fl, ds, clamp_max of today's display


def test_host_constants_at_100_nits_equal_todays_opendrt_consts():
    """The library's two host functions side by side: hdr_output_consts(100, any gamut, linear) and opendrt_consts — what setup_kernel hands to
    FrameConsts today, reported by the hook when it is given no settings — agree in every bit of m, s, fl, ds, clamp_max and dch_s."""
    lib = _lib()
    consts = lib.de_debug_hdr_consts
    consts.restype, consts.argtypes = _native.DEBUG_SYMBOLS["de_debug_hdr_consts"]
    today = np.full(19, 7.0, np.float32)
    assert consts(None, None, today.ctypes.data) == 0
    assert (today[6:] == 0).all() and today[2] == np.float32(0.005) and today[3] == 1.0 and today[4] == 1.0 and today[0] > 1.0 and today[1] > 0.0
    for g in range(3):
        out = np.zeros(19, np.float32)
        assert consts(None, ctypes.byref(_settings(peak_nits=100.0, gamut=g, transfer=0)), out.ctypes.data) == 0
        assert (out[:6].view(np.uint32) == today[:6].view(np.uint32)).all(), (g, out[:6], today[:6])
    out = np.zeros(19, np.float32)
    assert consts(None, ctypes.byref(_settings(peak_nits=1000.0, gamut=0, transfer=0)), out.ctypes.data) == 0
    assert (out[:2] != today[:2]).all()                                           # and another peak gives another tonescale


def test_python_api_without_a_device():
    from digital_earth_amd.renderer import Renderer
    from digital_earth_amd.earth_viewer import EarthViewer
    import hdr_output_ref as ho
    sig = inspect.signature(Renderer.set_hdr_output).parameters
    assert list(sig)[1:] == ["on", "peak_nits", "gamut", "transfer", "pixel_format", "mode", "seed", "animate"]
    assert ho.DEFAULTS == {k: v.default for k, v in sig.items() if k != "self"}
    assert Renderer.HDR_GAMUTS == ho.GAMUTS and Renderer.HDR_TRANSFERS == ho.TRANSFERS and Renderer.HDR_PIXEL_FORMATS == ho.FORMATS and Renderer.PIXEL_MODES == ho.MODES
    assert isinstance(Renderer.hdr_output, property)
    assert list(inspect.signature(Renderer.fetch_hdr_pixels).parameters) == ["self"]
    sig = inspect.signature(Renderer.debug_hdr_transform).parameters
    assert list(sig)[1:] == ["rgb", "peak_nits", "gamut", "transfer"]
    init = inspect.signature(EarthViewer.__init__).parameters
    assert init["hdr_output"].default is None and list(init).index("hdr_output") > list(init).index("output_filter") and init["renderer_kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    assert "hdr_pixels" in inspect.getsource(EarthViewer.frame) and "png16" in inspect.getsource(EarthViewer.save)


def test_build_tracks_the_new_sources():
    from digital_earth_amd import build
    assert "hdr_output_kernels.hip" in build.DEPS
    assert any(d.endswith("digital_earth_hdr_output.h") for d in build.DEPS)
    ctx = open(os.path.join(build.CSRC, "de_context.h")).read()
    assert ctx.index('#include "hdr_output_kernels.hip"') > ctx.index('#include "aux_kernels.hip"')      # behind the helpers it shares
    src = open(os.path.join(build.CSRC, "hdr_output_kernels.hip")).read()
    for name in ("hdr_display_kernel", "hdr_pack_kernel", "hdr_transform_kernel", "de_pow", "de_log", "de_sqrt"):
        assert name in src
    assert "FrameConsts" in open(os.path.join(build.CSRC, "de_kernels.h")).read() and "hdr" not in re.search(r"struct FrameConsts \{.*?\n\};", open(os.path.join(build.CSRC, "de_kernels.h")).read(), re.S).group(0).lower().replace("hdr buffer", "")
