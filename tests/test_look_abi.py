"""The look-LUT C ABI without a GPU: include/digital_earth_look.h compiles as pedantic C99, the struct mirror matches field by field with size and
offsets, every entry point it declares is bound and exported, its table is disjoint from every other, the enums and limits have their values, the
Python signatures have the documented defaults, and the build tracks the new sources."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

from digital_earth_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"de_set_look", "de_get_look", "de_debug_look"}
CTYPE = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "float": ctypes.c_float}
FIELDS = [("struct_bytes", ctypes.c_uint32, 1), ("enabled", ctypes.c_int32, 1), ("interpolation", ctypes.c_int32, 1), ("strength", ctypes.c_float, 1),
          ("size_1d", ctypes.c_int32, 1), ("min_1d", ctypes.c_float, 3), ("max_1d", ctypes.c_float, 3),
          ("size_3d", ctypes.c_int32, 1), ("min_3d", ctypes.c_float, 3), ("max_3d", ctypes.c_float, 3)]


def _header(name="digital_earth_look.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name="digital_earth_look.h"):
    text = re.sub(r"/\*.*?\*/", "", _header(name), flags=re.S)
    return set(re.findall(r"\b(de_[a-z0-9_]+)\s*\(", text))


def _fields():
    """(name, ctype, count) of every member of de_look, in the header's order; `float a[3], b[3]` declares two arrays."""
    body = re.search(r"typedef struct de_look \{(.*?)\} de_look;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        m = re.match(r"\s*(uint32_t|int32_t|float)\s+(.+?)\s*$", decl.strip(), re.S)
        if not m:
            assert not decl.strip(), decl
            continue
        for item in m.group(2).split(","):
            name, count = re.match(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*$", item).groups()
            out.append((name, CTYPE[m.group(1)], int(count or 1)))
    return out


def test_look_struct_and_constants_match_header():
    assert _fields() == FIELDS
    assert [n for n, _ in _native.DeLook._fields_] == [n for n, _, _ in FIELDS]
    offset = 0
    for (name, ctype), (_, want, count) in zip(_native.DeLook._fields_, FIELDS):
        assert (ctype is want) if count == 1 else (ctype._type_ is want and ctype._length_ == count), name
        assert getattr(_native.DeLook, name).offset == offset, name
        offset += 4 * count
    assert ctypes.sizeof(_native.DeLook) == offset == 72
    consts = dict(re.findall(r"#define\s+DE_LOOK_(\w+)\s+(\d+)", _header()))
    assert consts == {"TRILINEAR": "0", "TETRAHEDRAL": "1", "MAX_1D": "65536", "MAX_3D": "65"}
    from digital_earth_amd.renderer import Renderer
    from digital_earth_amd import cube
    assert Renderer.LOOK_INTERPOLATIONS == ("trilinear", "tetrahedral")
    assert (cube.MAX_1D, cube.MAX_3D) == (65536, 65)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_look_header_compiles_as_pedantic_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "digital_earth_look.h"\n#include "digital_earth_debug.h"\n'
                   'int main(void) { de_look p; p.struct_bytes = sizeof p; (void)de_set_look; (void)de_get_look; (void)de_debug_look;\n'
                   '  return p.struct_bytes != 72 || DE_LOOK_TETRAHEDRAL != 1 || DE_LOOK_MAX_3D != 65 || sizeof p.max_3d != 12; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_look_symbols_declared_bound_and_exported():
    assert _declared() == set(_native.LOOK_SYMBOLS) == NAMES
    others = (set(_native.SYMBOLS) | set(_native.DEBUG_SYMBOLS) | set(_native.DENOISE_SYMBOLS) | set(_native.EXPOSURE_SYMBOLS) | set(_native.BLOOM_SYMBOLS)
              | set(_native.HISTORY_SYMBOLS) | set(_native.PIXELS_SYMBOLS) | set(_native.LOCAL_EXPOSURE_SYMBOLS) | set(_native.OUTPUT_SCALE_SYMBOLS)
              | set(_native.HDR_OUTPUT_SYMBOLS) | set(_native.VIDEO_SYMBOLS) | set(_native.LEGACY_SYMBOLS))
    assert not NAMES & others
    assert len(_declared("digital_earth.h")) == 40 and not NAMES & _declared("digital_earth.h") and not NAMES & _declared("digital_earth_debug.h")
    assert re.search(r"#define\s+DE_ABI_VERSION\s+6\b", _header("digital_earth.h"))
    L, P = _native.LOOK_SYMBOLS, ctypes.c_void_p
    assert all(res is ctypes.c_int for res, _ in L.values())
    args = L["de_set_look"][1]
    assert len(args) == 4 and args[0] is P and args[1]._type_ is _native.DeLook and args[2] is P and args[3] is P
    args = L["de_get_look"][1]
    assert len(args) == 2 and args[0] is P and args[1]._type_ is _native.DeLook
    args = L["de_debug_look"][1]
    assert len(args) == 7 and args[1] is P and args[2] is ctypes.c_uint64 and args[3]._type_ is _native.DeLook and args[4:] == [P, P, P]
    assert "LOOK_SYMBOLS" in inspect.getsource(_native.load)
    from digital_earth_amd import build
    build.build()
    lib = ctypes.CDLL(build.OUT)
    for name in NAMES:
        assert hasattr(lib, name), name
    lib.de_abi_version.restype = ctypes.c_int
    assert lib.de_abi_version() == 6 == _native.ABI_VERSION


def test_look_python_api_without_a_device():
    from digital_earth_amd.renderer import Renderer
    from digital_earth_amd.earth_viewer import EarthViewer
    import look_ref
    sig = inspect.signature(Renderer.set_look).parameters
    assert list(sig)[1:] == ["cube", "shaper", "strength", "interpolation", "enabled"]
    assert {k: v.default for k, v in sig.items() if k != "self"} == look_ref.DEFAULTS
    sig = inspect.signature(Renderer.debug_look).parameters
    assert list(sig)[1:] == ["rgb", "cube", "shaper", "strength", "interpolation"] and sig["strength"].default == 1.0 and sig["interpolation"].default == "tetrahedral"
    assert callable(Renderer.look) and look_ref.INTERPOLATIONS == Renderer.LOOK_INTERPOLATIONS
    init = inspect.signature(EarthViewer.__init__).parameters
    names = list(init)
    assert init["look"].default is None and init["look_strength"].default == 1.0
    assert names.index("look") == names.index("hdr_output") + 1 and names.index("look_strength") == names.index("look") + 1      # behind every earlier keyword
    assert names[-1] == "renderer_kwargs" and init["renderer_kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    # the pinned signatures are as they were
    assert list(inspect.signature(EarthViewer.frame).parameters)[1:] == ["spp", "copy", "pipelined", "pixels", "sliders"]
    assert list(inspect.signature(EarthViewer.record).parameters)[1:] == ["path", "frames", "spp", "fps", "sliders_per_frame"]
    assert list(inspect.signature(Renderer.fetch_pending).parameters)[1:] == ["copy", "all_images", "pixels", "video"]
    # a table of the wrong kind is refused before anything reaches the library
    from digital_earth_amd import cube
    with pytest.raises(ValueError):
        Renderer._look_table(cube.identity(4, "1d"), "3d", "cube")
    with pytest.raises(ValueError):
        Renderer._look_table(cube.identity(4), "1d", "shaper")
    assert Renderer._look_table(None, "3d", "cube") is None


def test_build_tracks_the_new_sources():
    from digital_earth_amd import build
    assert "look_kernels.hip" in build.DEPS
    assert any(d.endswith("digital_earth_look.h") for d in build.DEPS)
    ctx = open(os.path.join(build.CSRC, "de_context.h")).read()
    assert '#include "look_kernels.hip"' in ctx and '#include "../../include/digital_earth_look.h"' in ctx      # in the product library's one translation unit
    kernel = open(os.path.join(build.CSRC, "look_kernels.hip")).read()
    assert "DE_LOOK_STANDALONE" in kernel and "look_apply_kernel" in kernel and os.path.exists(os.path.join(ROOT, "tools", "look_host_check.cpp"))
    api = open(os.path.join(build.CSRC, "de_api.hip")).read()
    render = api[api.index("int de_render_to_image("):api.index("int de_fetch_image(")]
    assert render.index("hipEventRecord(c->ev_main") < render.index("lk_launch(") < render.index("run_output_scale(")      # behind ev_main, ahead of the scaler
