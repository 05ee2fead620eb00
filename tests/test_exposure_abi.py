"""The auto-exposure C ABI without a GPU: include/digital_earth_exposure.h compiles as pedantic C99 together with the debug header, both struct mirrors match
field by field, every entry point it declares is bound and exported, the binder's header keeps its 40 entry points at ABI 6, the Python signatures have the
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
NAMES = {"de_set_auto_exposure", "de_get_auto_exposure", "de_get_metering"}
CTYPE = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "float": ctypes.c_float, "uint64_t": ctypes.c_uint64}


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", _header(name), flags=re.S)
    return set(re.findall(r"\b(de_[a-z0-9_]+)\s*\(", text))


def _fields(struct):
    """[(name, ctype)] of a struct of the header: `type a, b;` and `type a[n];` declarations."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _header("digital_earth_exposure.h"), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        m = re.match(r"\s*(uint32_t|int32_t|float|uint64_t)\s+(.+?)\s*$", decl.strip(), re.S)
        if not m:
            assert not decl.strip(), decl
            continue
        for item in m.group(2).split(","):
            a = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", item)
            t = CTYPE[m.group(1)]
            out.append((a.group(1), t * int(a.group(2)) if a.group(2) else t))
    return out


def _same(mirror, want):
    assert [n for n, _ in mirror._fields_] == [n for n, _ in want]
    for (n, a), (_, b) in zip(mirror._fields_, want):
        if hasattr(a, "_length_"):
            assert a._length_ == b._length_ and a._type_ is b._type_, n
        else:
            assert a is b, n


def test_auto_exposure_struct_matches_header():
    want = _fields("de_auto_exposure")
    assert [n for n, _ in want] == ["struct_bytes", "key", "compensation", "ev_min", "ev_max", "low_fraction", "high_fraction", "adapt", "region"]
    _same(_native.DeAutoExposure, want)
    assert ctypes.sizeof(_native.DeAutoExposure) == 48


def test_metering_struct_matches_header():
    want = _fields("de_metering")
    assert [n for n, _ in want] == ["struct_bytes", "ev", "ev_target", "mean_log2", "valid", "metered", "below", "clipped", "histogram"]
    _same(_native.DeMetering, want)
    assert ctypes.sizeof(_native.DeMetering) == 1072 and _native.DeMetering.metered.offset == 24 and _native.DeMetering.histogram.offset == 48


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_exposure_header_compiles_as_pedantic_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "digital_earth_exposure.h"\n#include "digital_earth_debug.h"\n'
                   'int main(void) { de_auto_exposure a; de_metering m; a.struct_bytes = sizeof a; m.struct_bytes = sizeof m; return a.struct_bytes != 48 || m.struct_bytes != 1072; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


def test_exposure_symbols_declared_bound_and_exported():
    assert _declared("digital_earth_exposure.h") == set(_native.EXPOSURE_SYMBOLS) == NAMES
    assert not set(_native.EXPOSURE_SYMBOLS) & (set(_native.SYMBOLS) | set(_native.DEBUG_SYMBOLS) | set(_native.DENOISE_SYMBOLS) | set(_native.LEGACY_SYMBOLS))
    assert len(_declared("digital_earth.h")) == 40 and not NAMES & _declared("digital_earth.h")
    assert re.search(r"#define\s+DE_ABI_VERSION\s+6\b", _header("digital_earth.h"))
    res, args = _native.EXPOSURE_SYMBOLS["de_set_auto_exposure"]
    assert res is ctypes.c_int and args[1]._type_ is _native.DeAutoExposure
    assert _native.EXPOSURE_SYMBOLS["de_get_metering"][1][1]._type_ is _native.DeMetering
    assert "EXPOSURE_SYMBOLS" in inspect.getsource(_native.load)
    from digital_earth_amd import build
    build.build()
    lib = ctypes.CDLL(build.OUT)
    for name in NAMES:
        assert hasattr(lib, name), name
    lib.de_abi_version.restype = ctypes.c_int
    assert lib.de_abi_version() == 6 == _native.ABI_VERSION


def test_exposure_python_api_without_a_device():
    from digital_earth_amd.renderer import Renderer
    from digital_earth_amd.earth_viewer import EarthViewer
    sig = inspect.signature(Renderer.set_auto_exposure).parameters
    assert list(sig)[1:] == ["on", "key", "compensation", "ev_range", "percentiles", "adapt", "region"]
    assert sig["on"].default is True and sig["key"].default == 0.18 and sig["compensation"].default == 0.0
    assert sig["ev_range"].default == (-8.0, 16.0) and sig["percentiles"].default == (0.10, 0.95) and sig["adapt"].default == 1.0 and sig["region"].default is None
    for name in ("auto_exposure", "metering"):
        assert callable(getattr(Renderer, name))
    st = inspect.signature(EarthViewer.start).parameters
    assert list(st)[1:] == ["spp", "out", "noise", "denoise", "auto_exposure"]
    assert st["auto_exposure"].default is False and st["denoise"].default is False and st["noise"].default is None
    assert "auto_exposure" not in inspect.signature(EarthViewer.frame).parameters


def test_build_tracks_the_new_sources():
    from digital_earth_amd import build
    assert "exposure_kernels.hip" in build.DEPS
    assert any(d.endswith("digital_earth_exposure.h") for d in build.DEPS)
    ctx = open(os.path.join(build.CSRC, "de_context.h")).read()
    assert '#include "exposure_kernels.hip"' in ctx      # built into the product library's one translation unit, like denoise_kernels.hip
