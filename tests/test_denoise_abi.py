"""The denoiser's C ABI without a GPU: include/digital_earth_denoise.h compiles as pedantic C99, its struct mirror matches field by field, every entry point it
declares (and the debug hook) is bound and exported, the binder's header keeps its 40 entry points, and the Python signatures have the documented defaults."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

from digital_earth_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", _header(name), flags=re.S)
    return set(re.findall(r"\b(de_[a-z0-9_]+)\s*\(", text))


def test_denoise_struct_matches_header():
    body = re.search(r"typedef struct de_denoise \{(.*?)\} de_denoise;", _header("digital_earth_denoise.h"), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "float": ctypes.c_float}
    want = []
    for decl in body.split(";"):
        m = re.match(r"\s*(uint32_t|int32_t|float)\s+(\w+)\s*$", decl.strip())
        if m:
            want.append((m.group(2), ctype[m.group(1)]))
    assert [n for n, _ in _native.DeDenoise._fields_] == [n for n, _ in want] == ["struct_bytes", "levels", "sigma_luminance"]
    for (n, a), (_, b) in zip(_native.DeDenoise._fields_, want):
        assert a == b, n
    assert ctypes.sizeof(_native.DeDenoise) == 12


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_denoise_header_compiles_as_pedantic_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "digital_earth_denoise.h"\n#include "digital_earth_debug.h"\nint main(void) { de_denoise d; d.struct_bytes = sizeof d; return d.struct_bytes != 12; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_denoise_symbols_declared_bound_and_exported():
    assert _declared("digital_earth_denoise.h") == set(_native.DENOISE_SYMBOLS) == {"de_set_denoise", "de_get_denoise", "de_fetch_denoised_hdr", "de_fetch_guides"}
    assert not set(_native.DENOISE_SYMBOLS) & (set(_native.SYMBOLS) | set(_native.DEBUG_SYMBOLS))
    assert "de_debug_denoise" in _declared("digital_earth_debug.h") and "de_debug_denoise" in _native.DEBUG_SYMBOLS
    assert len(_declared("digital_earth.h")) == 40
    res, args = _native.DENOISE_SYMBOLS["de_set_denoise"]
    assert res is ctypes.c_int and args[1]._type_ is _native.DeDenoise
    from digital_earth_amd import build
    build.build()
    lib = ctypes.CDLL(build.OUT)
    for name in list(_native.DENOISE_SYMBOLS) + ["de_debug_denoise"]:
        assert hasattr(lib, name), name
    lib.de_abi_version.restype = ctypes.c_int
    assert lib.de_abi_version() == 6 == _native.ABI_VERSION


def test_denoise_python_api_without_a_device():
    from digital_earth_amd.renderer import Renderer
    from digital_earth_amd.earth_viewer import EarthViewer
    sig = inspect.signature(Renderer.set_denoise)
    assert list(sig.parameters)[1:] == ["on", "levels", "sigma_luminance"]
    assert sig.parameters["on"].default is True and sig.parameters["levels"].default == 5 and sig.parameters["sigma_luminance"].default == 4.0
    for name in ("fetch_denoised_hdr", "fetch_guides", "denoise"):
        assert callable(getattr(Renderer, name))
    st = inspect.signature(EarthViewer.start).parameters
    assert st["denoise"].default is False and st["noise"].default is None


def test_build_tracks_the_new_sources():
    from digital_earth_amd import build
    assert "denoise_kernels.hip" in build.DEPS
    assert any(d.endswith("digital_earth_denoise.h") for d in build.DEPS)
