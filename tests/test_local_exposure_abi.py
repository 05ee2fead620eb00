"""The local exposure C ABI without a GPU: include/digital_earth_local_exposure.h compiles as pedantic C99, the struct mirror matches field by field in
size and offsets, the four entry points it declares are bound and exported, the binder's header keeps its 40 entry points at ABI 6, the Python
signatures have the documented defaults, out-of-range settings are refused ahead of any device call, and the build tracks the new sources."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

from digital_earth_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"de_set_local_exposure", "de_get_local_exposure", "de_fetch_local_exposure_hdr", "de_debug_local_exposure"}
FIELDS = ["struct_bytes", "on", "highlights", "shadows", "sigma", "max_ev", "key", "levels"]
CTYPE = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "float": ctypes.c_float}


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", _header(name), flags=re.S)
    return set(re.findall(r"\b(de_[a-z0-9_]+)\s*\(", text))


def _fields():
    """[(name, ctype)] of de_local_exposure in the header: `type a;` declarations."""
    body = re.search(r"typedef struct de_local_exposure \{(.*?)\} de_local_exposure;", _header("digital_earth_local_exposure.h"), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        m = re.match(r"\s*(uint32_t|int32_t|float)\s+(\w+)\s*$", decl.strip(), re.S)
        if not m:
            assert not decl.strip(), decl
            continue
        out.append((m.group(2), CTYPE[m.group(1)]))
    return out


def test_struct_matches_header():
    want = _fields()
    assert [n for n, _ in want] == FIELDS
    assert [n for n, _ in _native.DeLocalExposure._fields_] == FIELDS
    for (n, a), (_, b) in zip(_native.DeLocalExposure._fields_, want):
        assert a is b, n
    assert ctypes.sizeof(_native.DeLocalExposure) == 32


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_header_compiles_as_pedantic_c99_with_the_mirrors_size_and_offsets(tmp_path):
    src = tmp_path / "t.c"
    checks = " || ".join("offsetof(de_local_exposure, %s) != %d" % (n, getattr(_native.DeLocalExposure, n).offset) for n in FIELDS)
    src.write_text('#include <stddef.h>\n#include "digital_earth_local_exposure.h"\n#include "digital_earth_debug.h"\n'
                   'int main(void) { de_local_exposure s; s.struct_bytes = sizeof s; return s.struct_bytes != %d || %s; }\n'
                   % (ctypes.sizeof(_native.DeLocalExposure), checks))
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


def test_symbols_declared_bound_and_exported():
    assert _declared("digital_earth_local_exposure.h") == set(_native.LOCAL_EXPOSURE_SYMBOLS) == NAMES
    assert not set(_native.LOCAL_EXPOSURE_SYMBOLS) & (set(_native.SYMBOLS) | set(_native.DEBUG_SYMBOLS) | set(_native.DENOISE_SYMBOLS) | set(_native.EXPOSURE_SYMBOLS)
                                                      | set(_native.BLOOM_SYMBOLS) | set(_native.HISTORY_SYMBOLS) | set(_native.PIXELS_SYMBOLS) | set(_native.LEGACY_SYMBOLS))
    assert len(_declared("digital_earth.h")) == 40 and not NAMES & _declared("digital_earth.h")      # the binder's own list is unchanged
    assert not NAMES & _declared("digital_earth_debug.h")
    assert re.search(r"#define\s+DE_ABI_VERSION\s+6\b", _header("digital_earth.h"))
    for name in ("de_set_local_exposure", "de_get_local_exposure"):
        res, args = _native.LOCAL_EXPOSURE_SYMBOLS[name]
        assert res is ctypes.c_int and args[1]._type_ is _native.DeLocalExposure
    assert len(_native.LOCAL_EXPOSURE_SYMBOLS["de_fetch_local_exposure_hdr"][1]) == 2
    res, args = _native.LOCAL_EXPOSURE_SYMBOLS["de_debug_local_exposure"]
    assert res is ctypes.c_int and args[2] is ctypes.c_float and args[3]._type_ is _native.DeLocalExposure and len(args) == 5
    assert "LOCAL_EXPOSURE_SYMBOLS" in inspect.getsource(_native.load)
    from digital_earth_amd import build
    build.build()
    lib = ctypes.CDLL(build.OUT)
    for name in NAMES:
        assert hasattr(lib, name), name
    lib.de_abi_version.restype = ctypes.c_int
    assert lib.de_abi_version() == 6 == _native.ABI_VERSION


def test_python_api_without_a_device():
    from digital_earth_amd.renderer import Renderer
    from digital_earth_amd.earth_viewer import EarthViewer
    import local_exposure_ref
    sig = inspect.signature(Renderer.set_local_exposure).parameters
    assert list(sig)[1:] == ["on", "highlights", "shadows", "sigma", "max_ev", "key", "levels"]
    assert sig["on"].default is True
    assert {k: v.default for k, v in sig.items() if k not in ("self", "on")} == dict(highlights=0.5, shadows=0.25, sigma=1.0, max_ev=2.0, key=0.18, levels=6)
    assert local_exposure_ref.DEFAULTS == {k: v.default for k, v in sig.items() if k not in ("self", "on")}
    dbg = inspect.signature(Renderer.debug_local_exposure).parameters
    assert list(dbg)[1:3] == ["mean", "exposure_scale"] and {k: dbg[k].default for k in list(dbg)[3:]} == local_exposure_ref.DEFAULTS
    assert isinstance(Renderer.local_exposure, property)
    assert callable(Renderer.fetch_local_exposure_hdr)
    init = inspect.signature(EarthViewer.__init__).parameters
    assert init["local_exposure"].default is None and list(init).index("local_exposure") == list(init).index("history") + 1
    assert "local_exposure" not in inspect.signature(EarthViewer.start).parameters
    assert "local_exposure" not in inspect.signature(EarthViewer.frame).parameters


def test_range_refusals_come_before_any_device_call():
    """The library answers a bad setting with DE_ERR_INVALID from its argument checks: no device is needed to see that (a null context is refused the
    same way), and the checks' bounds are the header's."""
    from digital_earth_amd import build
    build.build()
    lib = ctypes.CDLL(build.OUT)
    lib.de_set_local_exposure.restype = ctypes.c_int
    lib.de_set_local_exposure.argtypes = [ctypes.c_void_p, ctypes.POINTER(_native.DeLocalExposure)]
    s = _native.DeLocalExposure()
    s.struct_bytes = ctypes.sizeof(s)
    assert lib.de_set_local_exposure(None, ctypes.byref(s)) == _native.DE_ERR_INVALID
    lib.de_debug_local_exposure.restype = ctypes.c_int
    lib.de_debug_local_exposure.argtypes = _native.LOCAL_EXPOSURE_SYMBOLS["de_debug_local_exposure"][1]
    assert lib.de_debug_local_exposure(None, None, 1.0, ctypes.byref(s), None) == _native.DE_ERR_INVALID
    src = open(os.path.join(build.CSRC, "de_display.h")).read()      # the stages' host code
    check = src[src.index("int lx_settings_check("):src.index("int lx_run(")]
    for text in ("s->highlights >= 0.0f", "s->highlights <= 1.0f", "s->shadows >= 0.0f", "s->shadows <= 1.0f", "s->sigma > 0.0f", "s->max_ev >= 0.0f", "s->key > 0.0f",
                 "s->levels < 1 || s->levels > LX_MAX_LEVELS", "sizeof(de_local_exposure)"):
        assert text in check, text
    assert check.count("DE_ERR_INVALID") == 4


def test_build_tracks_the_new_sources():
    from digital_earth_amd import build
    assert "local_exposure_kernels.hip" in build.DEPS
    assert any(d.endswith("digital_earth_local_exposure.h") for d in build.DEPS)
    ctx = open(os.path.join(build.CSRC, "de_context.h")).read()
    assert ctx.index('#include "local_exposure_kernels.hip"') > ctx.index('#include "bloom_kernels.hip"')      # in the product library's one translation unit
    assert "de_display.h" in build.DEPS
    # last ahead of the display launch: last in the chain (de_display.h), which de_render_to_image runs to its end before it launches the display
    chain = open(os.path.join(build.CSRC, "de_display.h")).read()
    chain = chain[chain.index("int display_chain("):]
    assert chain.index("run_bloom(") < chain.index("run_local_exposure(") < chain.rindex("return DE_OK;")
    assert chain.count("run_") == chain[:chain.index("run_local_exposure(")].count("run_") + 1      # no stage runs after it
    api = open(os.path.join(build.CSRC, "de_api.hip")).read()
    body = api[api.index("int de_render_to_image("):api.index("int de_fetch_image(")]
    assert "run_bloom(" not in body and "run_local_exposure(" not in body
    assert body.index("display_chain(c, STOP_IMAGE") < body.index("display_kernel<true>")
