"""The OpenEXR output's ABI without a GPU (include/digital_earth_exr.h): the header against the ctypes mirror, the struct's size and defaults, and
the host-only entry point de_debug_exr_framing against the restatement's front and capacity, with every refusal de_set_exr makes."""
import ctypes
import os
import re

import pytest

import exr_ref as xr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "digital_earth_exr.h")).read()
ERR_INVALID = -1


@pytest.fixture(scope="module")
def native():
    from digital_earth_amd import _native
    return _native


@pytest.fixture(scope="module")
def lib(native):
    return native.load()


def _settings(native, source=0, pixel_type=1, compression=3, chunk_bytes=32768, scale=1.0, struct_bytes=None):
    s = native.DeExr()
    s.struct_bytes = ctypes.sizeof(native.DeExr) if struct_bytes is None else struct_bytes
    s.source, s.pixel_type, s.compression, s.chunk_bytes, s.scale = source, pixel_type, compression, chunk_bytes, scale
    return s


def test_header_declares_what_the_mirror_binds(native):
    body = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    declared = dict(re.findall(r"^int (de_\w+)\(([^;]*)\);", body, flags=re.M))
    assert set(declared) == set(native.EXR_SYMBOLS)
    for name, (res, args) in native.EXR_SYMBOLS.items():
        assert res is ctypes.c_int and len(args) == declared[name].count(",") + 1, name
    defines = dict(re.findall(r"^#define (DE_EXR_\w+) (\d+)", HEADER, flags=re.M))
    assert int(defines["DE_EXR_DEFAULT_CHUNK"]) == native.EXR_DEFAULT_CHUNK == xr.DEFAULT_CHUNK
    for i, name in enumerate(native.EXR_SOURCES):
        assert int(defines["DE_EXR_SOURCE_" + name.upper()]) == i
    for name, v in native.EXR_PIXEL_TYPES.items():
        assert int(defines["DE_EXR_PIXEL_" + name.upper()]) == v == xr.PIXEL_TYPES[name]
    for name, v in native.EXR_COMPRESSIONS.items():
        assert int(defines["DE_EXR_COMPRESSION_" + name.upper()]) == v == xr.COMPRESSIONS[name]
    assert "digital_earth_exr.h" not in open(os.path.join(ROOT, "include", "digital_earth.h")).read()      # the binder's header stays as it is
    assert "unmeasured" in HEADER.lower()                                                                   # the default chunk says what it is


def test_struct_size_and_fields(native):
    fields = re.search(r"typedef struct de_exr \{(.*?)\} de_exr;", HEADER, flags=re.S).group(1)
    names = re.findall(r"^\s*(?:u?int32_t|float) (\w+);", fields, flags=re.M)
    assert names == [f[0] for f in native.DeExr._fields_] == ["struct_bytes", "source", "pixel_type", "compression", "chunk_bytes", "scale"]
    assert ctypes.sizeof(native.DeExr) == 24


@pytest.mark.parametrize("shape", [(1, 1), (3, 17), (700, 33), (8, 1100), (1920, 1080), (3840, 2160)])
@pytest.mark.parametrize("pixel_type", ["half", "float"])
@pytest.mark.parametrize("compression", ["none", "zips", "zip"])
def test_framing_equals_the_restatement(native, lib, shape, pixel_type, compression):
    W, H = shape
    s = _settings(native, pixel_type=xr.PIXEL_TYPES[pixel_type], compression=xr.COMPRESSIONS[compression], chunk_bytes=4096)
    nb = (H + xr.LINES[compression] - 1) // xr.LINES[compression]
    size = xr.FRONT_FIXED + 8 * nb + 5
    out, n, cap = ctypes.create_string_buffer(b"\xA5" * size, size), ctypes.c_uint64(), ctypes.c_uint64()
    assert lib.de_debug_exr_framing(ctypes.byref(s), W, H, out, ctypes.c_uint64(size), ctypes.byref(n), ctypes.byref(cap)) == 0
    assert n.value == xr.FRONT_FIXED + 8 * nb
    assert out.raw == xr.front(W, H, pixel_type, compression) + b"\0" * (8 * nb) + b"\xA5" * 5      # the table zeroed, nothing behind it
    assert cap.value == xr.capacity(W, H, pixel_type, compression)
    assert lib.de_debug_exr_framing(ctypes.byref(s), W, H, None, ctypes.c_uint64(0), ctypes.byref(n), ctypes.byref(cap)) == 0      # sizes alone


def test_framing_refuses_what_set_exr_refuses(native, lib):
    out, n, cap = ctypes.create_string_buffer(b"\xA5" * 400, 400), ctypes.c_uint64(7), ctypes.c_uint64(7)

    def call(s, W=16, H=8, buf=out, size=400):
        return lib.de_debug_exr_framing(ctypes.byref(s) if s is not None else None, W, H, buf, ctypes.c_uint64(size), ctypes.byref(n), ctypes.byref(cap))
    assert call(_settings(native)) == 0 and n.value == 313 + 8
    n.value = cap.value = 7
    out.raw = b"\xA5" * 400
    bad = [_settings(native, struct_bytes=20), _settings(native, struct_bytes=28), _settings(native, source=-1), _settings(native, source=5),
           _settings(native, pixel_type=0), _settings(native, pixel_type=3), _settings(native, compression=1), _settings(native, compression=4),
           _settings(native, compression=-1), _settings(native, chunk_bytes=1023), _settings(native, chunk_bytes=65536),
           _settings(native, scale=0.0), _settings(native, scale=-1.0), _settings(native, scale=float("inf")), _settings(native, scale=float("nan"))]
    for s in bad:
        assert call(s) == ERR_INVALID
    assert call(None) == ERR_INVALID
    for kw in (dict(W=0), dict(H=0), dict(W=-1), dict(W=1 << 13, H=(1 << 12) + 1)):      # the last: one row past 2^27 raw bytes at HALF
        assert call(_settings(native), **kw) == ERR_INVALID
    assert call(_settings(native, pixel_type=2), W=3840, H=2160, buf=None, size=0) == 0 and cap.value == xr.capacity(3840, 2160, "float", "zip")      # 4K at float32 fits
    assert call(_settings(native, pixel_type=2), W=1 << 12, H=(1 << 11) + 683) == ERR_INVALID
    n.value = cap.value = 7
    assert call(_settings(native), size=320) == ERR_INVALID and n.value == 321 and out.raw == b"\xA5" * 400      # too small an `out`: the length, nothing written
    for ok in (_settings(native, chunk_bytes=1024), _settings(native, chunk_bytes=65535), _settings(native, source=4, pixel_type=2, compression=0, scale=1e-3)):
        assert call(ok) == 0


def _cxx():
    import shutil
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    raise AssertionError("no host C++ compiler found (the library's own build needs one too)")


def test_host_leaves_under_the_sanitizers(tmp_path):
    """tools/exr_host_check.cpp: the front, the geometry, the conversion, the reorder / predictor and the compaction from `alt`, on the CPU."""
    import subprocess
    exe = str(tmp_path / "exr_host_check")
    subprocess.check_call([_cxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "exr_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    assert "no sanitizer report" in out.stdout and "conversion" in out.stdout, out.stdout
