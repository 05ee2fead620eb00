"""The PNG output's ABI without a GPU (include/digital_earth_png.h): the header against the ctypes mirror, the struct's size, and the host-only
entry point de_debug_png_framing against the restatement's front and capacity, with every refusal de_set_png makes."""
import ctypes
import os
import re

import pytest

import png_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "digital_earth_png.h")).read()
ERR_INVALID = -1


@pytest.fixture(scope="module")
def native():
    from digital_earth_amd import _native
    return _native


@pytest.fixture(scope="module")
def lib(native):
    return native.load()


def _settings(native, source=0, filter=5, chunk_bytes=16384, struct_bytes=None):
    s = native.DePng()
    s.struct_bytes = ctypes.sizeof(native.DePng) if struct_bytes is None else struct_bytes
    s.source, s.filter, s.chunk_bytes = source, filter, chunk_bytes
    return s


def test_header_declares_what_the_mirror_binds(native):
    body = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    declared = dict(re.findall(r"^int (de_\w+)\(([^;]*)\);", body, flags=re.M))
    assert set(declared) == set(native.PNG_SYMBOLS)
    for name, (res, args) in native.PNG_SYMBOLS.items():
        assert res is ctypes.c_int and len(args) == declared[name].count(",") + 1, name
    defines = dict(re.findall(r"^#define (DE_PNG_\w+) (\d+)", HEADER, flags=re.M))
    assert int(defines["DE_PNG_DEFAULT_CHUNK"]) == native.PNG_DEFAULT_CHUNK == pr.DEFAULT_CHUNK
    for i, name in enumerate(native.PNG_SOURCES):
        assert int(defines["DE_PNG_SOURCE_" + name.upper()]) == i
    for i, name in enumerate(native.PNG_FILTERS):
        assert int(defines["DE_PNG_FILTER_" + name.upper()]) == i
    assert tuple(native.PNG_FILTERS) == pr.FILTERS
    assert "digital_earth_png.h" not in open(os.path.join(ROOT, "include", "digital_earth.h")).read()      # the binder's header stays as it is


def test_struct_size_and_fields(native):
    fields = re.search(r"typedef struct de_png \{(.*?)\} de_png;", HEADER, flags=re.S).group(1)
    names = re.findall(r"^\s*u?int32_t (\w+);", fields, flags=re.M)
    assert names == [f[0] for f in native.DePng._fields_] == ["struct_bytes", "source", "filter", "chunk_bytes"]
    assert ctypes.sizeof(native.DePng) == 16


@pytest.mark.parametrize("shape", [(1, 1, 3, 8), (7, 5, 4, 8), (33, 17, 3, 16), (1920, 1080, 3, 8), (1920, 1080, 3, 16)])
@pytest.mark.parametrize("chunk", [1024, 16384, 65535])
def test_framing_equals_the_restatement(native, lib, shape, chunk):
    W, H, ch, depth = shape
    s = _settings(native, chunk_bytes=chunk)
    out, n, cap = ctypes.create_string_buffer(b"\xA5" * 64, 64), ctypes.c_uint64(), ctypes.c_uint64()
    cicp = bytes((9, 16, 0, 1))
    assert lib.de_debug_png_framing(ctypes.byref(s), W, H, ch, depth, cicp, out, ctypes.c_uint64(64), ctypes.byref(n), ctypes.byref(cap)) == 0
    want = pr.front(W, H, ch, depth, (9, 16, 0, 1))
    assert n.value == len(want) == (49 if depth == 16 else 33) and out.raw[:n.value] == want and out.raw[n.value:] == b"\xA5" * (64 - n.value)
    assert cap.value == pr.capacity(W, H, ch, depth, chunk)
    if depth == 16:                                                 # no code points given: linear Rec.709, what de_debug_png writes
        assert lib.de_debug_png_framing(ctypes.byref(s), W, H, ch, depth, None, out, ctypes.c_uint64(64), ctypes.byref(n), None) == 0
        assert out.raw[:n.value] == pr.front(W, H, ch, depth)
    assert lib.de_debug_png_framing(ctypes.byref(s), W, H, ch, depth, None, None, ctypes.c_uint64(0), ctypes.byref(n), ctypes.byref(cap)) == 0      # sizes alone


def test_framing_refuses_what_set_png_refuses(native, lib):
    out, n, cap = ctypes.create_string_buffer(b"\xA5" * 64, 64), ctypes.c_uint64(7), ctypes.c_uint64(7)

    def call(s, W=16, H=8, ch=3, depth=8, buf=out, size=64):
        return lib.de_debug_png_framing(ctypes.byref(s) if s is not None else None, W, H, ch, depth, None, buf, ctypes.c_uint64(size), ctypes.byref(n), ctypes.byref(cap))
    assert call(_settings(native)) == 0
    n.value = cap.value = 7
    out.raw = b"\xA5" * 64
    bad = [_settings(native, struct_bytes=12), _settings(native, struct_bytes=20), _settings(native, source=-1), _settings(native, source=2),
           _settings(native, filter=-1), _settings(native, filter=6), _settings(native, chunk_bytes=1023), _settings(native, chunk_bytes=65536),
           _settings(native, chunk_bytes=0)]
    for s in bad:
        assert call(s) == ERR_INVALID
    assert call(None) == ERR_INVALID
    for kw in (dict(W=0), dict(H=0), dict(W=-1), dict(ch=2), dict(ch=5), dict(ch=4, depth=16), dict(depth=10), dict(W=1 << 14, H=1 << 12)):
        assert call(_settings(native), **kw) == ERR_INVALID
    assert n.value == 7 and cap.value == 7 and out.raw == b"\xA5" * 64          # a refused call changes nothing
    assert call(_settings(native), size=32) == ERR_INVALID and n.value == 33 and out.raw == b"\xA5" * 64      # too small an `out`: the length, nothing written
    for ok in (_settings(native, chunk_bytes=1024), _settings(native, chunk_bytes=65535), _settings(native, source=1, filter=0)):
        assert call(ok) == 0
