"""The Radiance HDR output's ABI without a GPU (include/digital_earth_rgbe.h): the header against the ctypes mirror, the struct's size, the
host-only entry point de_debug_rgbe_framing against the restatement's front and capacity with every refusal de_set_rgbe makes, and the plain
leaves under the sanitizers (tools/rgbe_host_check.cpp, a program of its own)."""
import ctypes
import os
import re

import pytest

import rgbe_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "digital_earth_rgbe.h")).read()
ERR_INVALID = -1


@pytest.fixture(scope="module")
def native():
    from digital_earth_amd import _native
    return _native


@pytest.fixture(scope="module")
def lib(native):
    return native.load()


def _settings(native, source=0, rle=1, rounding=0, scale=1.0, struct_bytes=None):
    s = native.DeRgbe()
    s.struct_bytes = ctypes.sizeof(native.DeRgbe) if struct_bytes is None else struct_bytes
    s.source, s.rle, s.rounding, s.scale = source, rle, rounding, scale
    return s


def test_header_declares_what_the_mirror_binds(native):
    body = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    declared = dict(re.findall(r"^int (de_\w+)\(([^;]*)\);", body, flags=re.M))
    assert set(declared) == set(native.RGBE_SYMBOLS)
    for name, (res, args) in native.RGBE_SYMBOLS.items():
        assert res is ctypes.c_int and len(args) == declared[name].count(",") + 1, name
    defines = dict(re.findall(r"^#define (DE_RGBE_\w+) (\d+)", HEADER, flags=re.M))
    assert int(defines["DE_RGBE_ROUND_TRUNC"]) == native.RGBE_ROUNDINGS["trunc"] == gr.ROUNDINGS["trunc"]
    assert int(defines["DE_RGBE_ROUND_NEAREST"]) == native.RGBE_ROUNDINGS["round"] == gr.ROUNDINGS["round"]
    assert "digital_earth_rgbe.h" not in open(os.path.join(ROOT, "include", "digital_earth.h")).read()      # the binder's header stays as it is
    assert native.ABI_VERSION == 6


def test_struct_size_and_fields(native):
    fields = re.search(r"typedef struct de_rgbe \{(.*?)\} de_rgbe;", HEADER, flags=re.S).group(1)
    names = re.findall(r"^\s*(?:u?int32_t|float) (\w+);", fields, flags=re.M)
    assert names == [f[0] for f in native.DeRgbe._fields_] == ["struct_bytes", "source", "rle", "rounding", "scale"]
    assert ctypes.sizeof(native.DeRgbe) == 20


@pytest.mark.parametrize("shape", [(1, 1), (7, 3), (8, 1100), (1920, 1080), (4096, 2048), (32767, 1), (32768, 1)])
@pytest.mark.parametrize("rle", [1, 0])
@pytest.mark.parametrize("scale", [1.0, 0.25, 1.0 / 3.0])
def test_framing_equals_the_restatement(native, lib, shape, rle, scale):
    W, H = shape
    s = _settings(native, rle=rle, scale=scale)
    want = gr.front(W, H, scale)
    size = len(want) + 5
    out, n, cap = ctypes.create_string_buffer(b"\xA5" * size, size), ctypes.c_uint64(), ctypes.c_uint64()
    assert lib.de_debug_rgbe_framing(ctypes.byref(s), W, H, out, ctypes.c_uint64(size), ctypes.byref(n), ctypes.byref(cap)) == 0
    assert n.value == len(want) and out.raw == want + b"\xA5" * 5      # nothing behind it
    assert cap.value == gr.capacity(W, H, rle, scale)
    assert (b"EXPOSURE=" in out.raw) == (scale != 1.0)
    assert lib.de_debug_rgbe_framing(ctypes.byref(s), W, H, None, ctypes.c_uint64(0), ctypes.byref(n), ctypes.byref(cap)) == 0      # sizes alone


def test_framing_refuses_what_set_rgbe_refuses(native, lib):
    out, n, cap = ctypes.create_string_buffer(b"\xA5" * 400, 400), ctypes.c_uint64(7), ctypes.c_uint64(7)

    def call(s, W=16, H=8, buf=out, size=400):
        return lib.de_debug_rgbe_framing(ctypes.byref(s) if s is not None else None, W, H, buf, ctypes.c_uint64(size), ctypes.byref(n), ctypes.byref(cap))
    assert call(_settings(native)) == 0 and n.value == len(gr.front(16, 8))
    n.value = cap.value = 7
    out.raw = b"\xA5" * 400
    bad = [_settings(native, struct_bytes=16), _settings(native, struct_bytes=24), _settings(native, source=-1), _settings(native, source=5),
           _settings(native, rle=2), _settings(native, rle=-1), _settings(native, rounding=2), _settings(native, rounding=-1),
           _settings(native, scale=0.0), _settings(native, scale=-1.0), _settings(native, scale=float("inf")), _settings(native, scale=float("nan"))]
    for s in bad:
        assert call(s) == ERR_INVALID
    assert call(None) == ERR_INVALID
    for kw in (dict(W=0), dict(H=0), dict(W=-1), dict(W=1 << 13, H=(1 << 12) + 1)):      # the last: one row past 2^27 flat bytes
        assert call(_settings(native), **kw) == ERR_INVALID
    assert n.value == 7 and cap.value == 7 and out.raw == b"\xA5" * 400                   # a refused call writes nothing
    assert call(_settings(native), W=1 << 13, H=1 << 12, buf=None, size=0) == 0            # exactly 2^27
    assert call(_settings(native), W=3840, H=2160, buf=None, size=0) == 0 and cap.value == gr.capacity(3840, 2160)
    n.value = 7
    assert call(_settings(native), size=10) == ERR_INVALID and n.value == len(gr.front(16, 8)) and out.raw == b"\xA5" * 400      # too small an `out`: the length, nothing written
    for ok in (_settings(native, source=4, rle=0, rounding=1, scale=1e-3), _settings(native, scale=3e38)):
        assert call(ok) == 0


def _cxx():
    import shutil
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    raise AssertionError("no host C++ compiler found (the library's own build needs one too)")


def test_host_leaves_under_the_sanitizers(tmp_path):
    """tools/rgbe_host_check.cpp: the sample, the front, the geometry and the run-length coder's three rounds, on the CPU."""
    import subprocess
    exe = str(tmp_path / "rgbe_host_check")
    subprocess.check_call([_cxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "rgbe_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    assert "no sanitizer report" in out.stdout and "coder" in out.stdout, out.stdout
