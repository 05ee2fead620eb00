"""The bloom C ABI without a GPU: include/digital_earth_bloom.h compiles as pedantic C99 together with the debug header, the struct mirror matches field
by field, every entry point it declares is bound and exported, the binder's header keeps its 40 entry points at ABI 6, the Python signatures have the
documented defaults, and the build tracks the new sources."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

from digital_earth_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"de_set_bloom", "de_get_bloom", "de_fetch_bloom_hdr"}
CTYPE = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "float": ctypes.c_float}


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", _header(name), flags=re.S)
    return set(re.findall(r"\b(de_[a-z0-9_]+)\s*\(", text))


def _fields(struct):
    """[(name, ctype)] of a struct of the header: `type a, b;` declarations."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _header("digital_earth_bloom.h"), re.S).group(1)
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


def test_bloom_struct_matches_header():
    want = _fields("de_bloom")
    assert [n for n, _ in want] == ["struct_bytes", "intensity", "threshold", "knee", "clamp", "spread", "levels"]
    assert [n for n, _ in _native.DeBloom._fields_] == [n for n, _ in want]
    for (n, a), (_, b) in zip(_native.DeBloom._fields_, want):
        assert a is b, n
    assert ctypes.sizeof(_native.DeBloom) == 28


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_bloom_header_compiles_as_pedantic_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "digital_earth_bloom.h"\n#include "digital_earth_debug.h"\n'
                   'int main(void) { de_bloom b; b.struct_bytes = sizeof b; return b.struct_bytes != 28; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


def test_bloom_symbols_declared_bound_and_exported():
    assert _declared("digital_earth_bloom.h") == set(_native.BLOOM_SYMBOLS) == NAMES
    assert not set(_native.BLOOM_SYMBOLS) & (set(_native.SYMBOLS) | set(_native.DEBUG_SYMBOLS) | set(_native.DENOISE_SYMBOLS) | set(_native.EXPOSURE_SYMBOLS)
                                             | set(_native.LEGACY_SYMBOLS))
    assert len(_declared("digital_earth.h")) == 40 and not NAMES & _declared("digital_earth.h")
    assert re.search(r"#define\s+DE_ABI_VERSION\s+6\b", _header("digital_earth.h"))
    for name in ("de_set_bloom", "de_get_bloom"):
        res, args = _native.BLOOM_SYMBOLS[name]
        assert res is ctypes.c_int and args[1]._type_ is _native.DeBloom
    assert _native.BLOOM_SYMBOLS["de_fetch_bloom_hdr"][0] is ctypes.c_int and len(_native.BLOOM_SYMBOLS["de_fetch_bloom_hdr"][1]) == 2
    assert "BLOOM_SYMBOLS" in inspect.getsource(_native.load)
    from digital_earth_amd import build
    build.build()
    lib = ctypes.CDLL(build.OUT)
    for name in NAMES:
        assert hasattr(lib, name), name
    lib.de_abi_version.restype = ctypes.c_int
    assert lib.de_abi_version() == 6 == _native.ABI_VERSION


def test_bloom_python_api_without_a_device():
    from digital_earth_amd.renderer import Renderer
    from digital_earth_amd.earth_viewer import EarthViewer
    sig = inspect.signature(Renderer.set_bloom).parameters
    assert list(sig)[1:] == ["on", "intensity", "threshold", "knee", "clamp", "spread", "levels"]
    assert sig["on"].default is True and sig["intensity"].default == 0.05 and sig["threshold"].default == 0.0 and sig["knee"].default == 0.5
    assert sig["clamp"].default == 0.0 and sig["spread"].default == 0.7 and sig["levels"].default == 6
    for name in ("bloom", "fetch_bloom_hdr"):
        assert callable(getattr(Renderer, name))
    # bloom is a persistent renderer setting: the viewer's entry points keep their signatures
    assert "bloom" not in inspect.signature(EarthViewer.start).parameters
    assert "bloom" not in inspect.signature(EarthViewer.frame).parameters
    import bloom_ref
    assert bloom_ref.DEFAULTS == {k: v.default for k, v in sig.items() if k not in ("self", "on")}


def test_build_tracks_the_new_sources():
    from digital_earth_amd import build
    assert "bloom_kernels.hip" in build.DEPS
    assert any(d.endswith("digital_earth_bloom.h") for d in build.DEPS)
    ctx = open(os.path.join(build.CSRC, "de_context.h")).read()
    assert ctx.index('#include "bloom_kernels.hip"') > ctx.index('#include "exposure_kernels.hip"')      # in the product library's one translation unit, after the meter
