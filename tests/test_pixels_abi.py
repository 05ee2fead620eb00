"""The pixel-output C ABI without a GPU: include/digital_earth_pixels.h compiles as pedantic C99 together with the debug header, the struct mirror matches
field by field, every entry point it declares is bound and exported, the binder's header keeps its 40 entry points at ABI 6, the Python signatures
have the documented defaults, and the build tracks the new sources."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

from digital_earth_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"de_set_pixels", "de_get_pixels", "de_render_to_pixels", "de_fetch_pixels", "de_fetch_pixels_view", "de_fetch_pixels_begin", "de_fetch_pixels_end"}
CTYPE = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "float": ctypes.c_float}


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", _header(name), flags=re.S)
    return set(re.findall(r"\b(de_[a-z0-9_]+)\s*\(", text))


def _fields(struct):
    """[(name, ctype)] of a struct of the header: `type a, b;` declarations."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _header("digital_earth_pixels.h"), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        m = re.match(r"\s*(uint32_t|int32_t|float)\s+(.+?)\s*$", decl.strip(), re.S)
        if not m:
            assert not decl.strip(), decl
            continue
        for item in m.group(2).split(","):
            out.append((re.match(r"\s*(\w+)\s*$", item).group(1), CTYPE[m.group(1)]))
    return out


def test_pixels_struct_matches_header():
    want = _fields("de_pixels")
    assert [n for n, _ in want] == ["struct_bytes", "channels", "mode", "seed", "animate"]
    assert [n for n, _ in _native.DePixels._fields_] == [n for n, _ in want]
    for (n, a), (_, b) in zip(_native.DePixels._fields_, want):
        assert a is b, n
    assert ctypes.sizeof(_native.DePixels) == 20
    modes = dict(re.findall(r"#define\s+DE_PIXELS_(\w+)\s+(\d+)", _header("digital_earth_pixels.h")))
    assert modes == {"TRUNCATE": "0", "ROUND": "1", "DITHER": "2"}


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_pixels_header_compiles_as_pedantic_c99(tmp_path):
    for first, second in (("digital_earth_pixels.h", "digital_earth_debug.h"), ("digital_earth_debug.h", "digital_earth_pixels.h")):
        src = tmp_path / "t.c"
        src.write_text('#include "%s"\n#include "%s"\n' % (first, second) +
                       'int main(void) { de_pixels p; p.struct_bytes = sizeof p; (void)de_debug_pixels; return p.struct_bytes != 20 || DE_PIXELS_DITHER != 2; }\n')
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    src.write_text('#include "digital_earth_pixels.h"\nint main(void) { de_pixels p; p.struct_bytes = sizeof p; return p.struct_bytes != 20; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


def test_pixels_symbols_declared_bound_and_exported():
    assert _declared("digital_earth_pixels.h") == set(_native.PIXELS_SYMBOLS) == NAMES
    assert not set(_native.PIXELS_SYMBOLS) & (set(_native.SYMBOLS) | set(_native.DEBUG_SYMBOLS) | set(_native.DENOISE_SYMBOLS) | set(_native.EXPOSURE_SYMBOLS)
                                              | set(_native.BLOOM_SYMBOLS) | set(_native.HISTORY_SYMBOLS) | set(_native.LEGACY_SYMBOLS))
    assert len(_declared("digital_earth.h")) == 40 and not NAMES & _declared("digital_earth.h")
    assert re.search(r"#define\s+DE_ABI_VERSION\s+6\b", _header("digital_earth.h"))
    for name in ("de_set_pixels", "de_get_pixels"):
        res, args = _native.PIXELS_SYMBOLS[name]
        assert res is ctypes.c_int and args[1]._type_ is _native.DePixels
    assert _native.PIXELS_SYMBOLS["de_get_pixels"][1][2]._type_ is ctypes.c_uint32
    assert _native.PIXELS_SYMBOLS["de_fetch_pixels"][1][2] is ctypes.c_uint64
    for name in ("de_fetch_pixels_view", "de_fetch_pixels_end"):
        assert _native.PIXELS_SYMBOLS[name][1][1]._type_._type_ is ctypes.c_uint8
    assert "de_debug_pixels" in _declared("digital_earth_debug.h") and "de_debug_pixels" in _native.DEBUG_SYMBOLS
    res, args = _native.DEBUG_SYMBOLS["de_debug_pixels"]
    assert res is ctypes.c_int and len(args) == 7 and args[4]._type_ is _native.DePixels and args[5] is ctypes.c_uint32
    assert "PIXELS_SYMBOLS" in inspect.getsource(_native.load)
    from digital_earth_amd import build
    build.build()
    lib = ctypes.CDLL(build.OUT)
    for name in NAMES | {"de_debug_pixels"}:
        assert hasattr(lib, name), name
    lib.de_abi_version.restype = ctypes.c_int
    assert lib.de_abi_version() == 6 == _native.ABI_VERSION


def test_pixels_python_api_without_a_device():
    from digital_earth_amd.renderer import Renderer
    from digital_earth_amd.earth_viewer import EarthViewer
    sig = inspect.signature(Renderer.set_pixels).parameters
    assert list(sig)[1:] == ["channels", "mode", "seed", "animate"]
    assert sig["channels"].default == 4 and sig["mode"].default == "truncate" and sig["seed"].default == 0 and sig["animate"].default is False
    assert Renderer.PIXEL_MODES == ("truncate", "round", "dither")
    sig = inspect.signature(Renderer.fetch_pixels).parameters
    assert list(sig)[1:] == ["copy", "lag"] and sig["copy"].default is True and sig["lag"].default == 0
    for name in ("pixels", "debug_pixels"):
        assert callable(getattr(Renderer, name))
    # fetch_pending keeps its first keywords and their defaults; the pixel ring is an addition behind them
    sig = inspect.signature(Renderer.fetch_pending).parameters
    assert list(sig)[1:3] == ["copy", "all_images"] and sig["copy"].default is True and sig["all_images"].default is False and sig["pixels"].default is False
    # frame(..., pixels=False, **sliders): a keyword of its own, ahead of the sliders and none of them
    sig = inspect.signature(EarthViewer.frame).parameters
    assert list(sig)[1:] == ["spp", "copy", "pipelined", "pixels", "sliders"]
    assert sig["pixels"].default is False and sig["sliders"].kind is inspect.Parameter.VAR_KEYWORD
    assert "pixels" not in ("sun_angle", "sun_path_rot", "fov", "aspect_scale", "exposure", "selected_crf", "gamma")
    import pixels_ref
    assert pixels_ref.DEFAULTS == {k: v.default for k, v in inspect.signature(Renderer.set_pixels).parameters.items() if k != "self"}
    assert pixels_ref.MODES == Renderer.PIXEL_MODES


def test_build_tracks_the_new_sources():
    from digital_earth_amd import build
    assert "pixels_kernels.hip" in build.DEPS
    assert any(d.endswith("digital_earth_pixels.h") for d in build.DEPS)
    ctx = open(os.path.join(build.CSRC, "de_context.h")).read()
    assert ctx.index('#include "pixels_kernels.hip"') > ctx.index('#include "history_kernels.hip"')      # in the product library's one translation unit, after the history
