"""The history-reprojection C ABI without a GPU: include/digital_earth_history.h compiles as pedantic C99 together with the debug header, the struct
mirror matches field by field, every entry point it declares is bound and exported, the binder's header keeps its 40 entry points at ABI 6, the Python
signatures have the documented defaults, and the build tracks the new sources."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

from digital_earth_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"de_set_history", "de_get_history", "de_fetch_history_hdr"}
CTYPE = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "float": ctypes.c_float}


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", _header(name), flags=re.S)
    return set(re.findall(r"\b(de_[a-z0-9_]+)\s*\(", text))


def _fields(struct):
    """[(name, ctype)] of a struct of the header: `type a, b;` declarations."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _header("digital_earth_history.h"), re.S).group(1)
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


def test_history_struct_matches_header():
    want = _fields("de_history")
    assert [n for n, _ in want] == ["struct_bytes", "max_history", "depth_tolerance"]
    assert [n for n, _ in _native.DeHistory._fields_] == [n for n, _ in want]
    for (n, a), (_, b) in zip(_native.DeHistory._fields_, want):
        assert a is b, n
    assert ctypes.sizeof(_native.DeHistory) == 12


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_history_header_compiles_as_pedantic_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "digital_earth_history.h"\n#include "digital_earth_debug.h"\n'
                   'int main(void) { de_history s; s.struct_bytes = sizeof s; (void)de_debug_history; return s.struct_bytes != 12; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_history_symbols_declared_bound_and_exported():
    assert _declared("digital_earth_history.h") == set(_native.HISTORY_SYMBOLS) == NAMES
    assert not set(_native.HISTORY_SYMBOLS) & (set(_native.SYMBOLS) | set(_native.DEBUG_SYMBOLS) | set(_native.DENOISE_SYMBOLS) | set(_native.EXPOSURE_SYMBOLS)
                                               | set(_native.BLOOM_SYMBOLS) | set(_native.LEGACY_SYMBOLS))
    # digital_earth.h is unchanged: its 40 entry points, none of them new, at ABI 6
    assert len(_declared("digital_earth.h")) == 40 and not (NAMES | {"de_debug_history"}) & _declared("digital_earth.h")
    assert re.search(r"#define\s+DE_ABI_VERSION\s+6\b", _header("digital_earth.h"))
    for name in ("de_set_history", "de_get_history"):
        res, args = _native.HISTORY_SYMBOLS[name]
        assert res is ctypes.c_int and args[1]._type_ is _native.DeHistory
    assert _native.HISTORY_SYMBOLS["de_fetch_history_hdr"][0] is ctypes.c_int and len(_native.HISTORY_SYMBOLS["de_fetch_history_hdr"][1]) == 2
    assert "de_debug_history" in _declared("digital_earth_debug.h") and "de_debug_history" in _native.DEBUG_SYMBOLS
    res, args = _native.DEBUG_SYMBOLS["de_debug_history"]
    assert res is ctypes.c_int and len(args) == 11 and args[4]._type_ is _native.DeParams and args[7]._type_ is _native.DeParams
    assert args[8] is ctypes.c_float and args[9] is ctypes.c_float
    assert "HISTORY_SYMBOLS" in inspect.getsource(_native.load)
    from digital_earth_amd import build
    build.build()
    lib = ctypes.CDLL(build.OUT)
    for name in NAMES | {"de_debug_history"}:
        assert hasattr(lib, name), name
    lib.de_abi_version.restype = ctypes.c_int
    assert lib.de_abi_version() == 6 == _native.ABI_VERSION


def test_history_python_api_without_a_device():
    from digital_earth_amd.renderer import Renderer
    from digital_earth_amd.earth_viewer import EarthViewer
    sig = inspect.signature(Renderer.set_history).parameters
    assert list(sig)[1:] == ["enabled", "max_history", "depth_tolerance"]
    assert sig["enabled"].default is True and sig["max_history"].default == 32.0 == Renderer.MAX_HISTORY
    assert sig["depth_tolerance"].default == 0.02 == Renderer.DEPTH_TOLERANCE
    for name in ("history", "fetch_history_hdr", "debug_history"):
        assert callable(getattr(Renderer, name))
    assert inspect.signature(EarthViewer.__init__).parameters["history"].default is None
    import history_ref
    assert history_ref.DEFAULTS == {k: v.default for k, v in sig.items() if k not in ("self", "enabled")}


def test_build_tracks_the_new_sources():
    from digital_earth_amd import build
    assert "history_kernels.hip" in build.DEPS
    assert any(d.endswith("digital_earth_history.h") for d in build.DEPS)
    ctx = open(os.path.join(build.CSRC, "de_context.h")).read()
    assert ctx.index('#include "history_kernels.hip"') > ctx.index('#include "bloom_kernels.hip"')      # in the product library's one translation unit
