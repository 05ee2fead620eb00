"""The EXR AOV channels' ABI without a GPU (include/digital_earth_exr_aovs.h): the header against the ctypes mirror, the host-only
entry point de_debug_exr_aov_framing against the restatement (tests/exr_aov_ref.py) for all 128 masks and both pixel types — the channel order
against Python's sorted() —, the capacity, the limit, the refusals, and the host leaves under the sanitizers."""
import ctypes
import os
import re
import struct

import pytest

import exr_aov_ref as xa
import exr_ref as xr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "digital_earth_exr_aovs.h")).read()
ERR_INVALID = -1


@pytest.fixture(scope="module")
def native():
    from digital_earth_amd import _native
    return _native


@pytest.fixture(scope="module")
def lib(native):
    return native.load()


def _settings(native, pixel_type="half", compression="zip", chunk_bytes=4096):
    s = native.DeExr()
    s.struct_bytes = ctypes.sizeof(native.DeExr)
    s.source, s.pixel_type, s.compression, s.chunk_bytes, s.scale = 0, xr.PIXEL_TYPES[pixel_type], xr.COMPRESSIONS[compression], chunk_bytes, 1.0
    return s


def _framing(lib, s, mask, W, H, size=None):
    n, cap = ctypes.c_uint64(7), ctypes.c_uint64(7)
    if size is None:
        return lib.de_debug_exr_aov_framing(ctypes.byref(s), mask, W, H, None, ctypes.c_uint64(0), ctypes.byref(n), ctypes.byref(cap)), n.value, cap.value, b""
    out = ctypes.create_string_buffer(b"\xA5" * size, size)
    rc = lib.de_debug_exr_aov_framing(ctypes.byref(s), mask, W, H, out, ctypes.c_uint64(size), ctypes.byref(n), ctypes.byref(cap))
    return rc, n.value, cap.value, out.raw


def test_header_declares_what_the_mirror_binds_and_de_exr_is_still_24_bytes(native, lib):
    body = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    declared = dict(re.findall(r"^int (de_\w+)\(([^;]*)\);", body, flags=re.M))
    assert set(declared) == set(native.EXR_AOV_SYMBOLS) == {"de_set_exr_aovs", "de_get_exr_aovs", "de_debug_exr_aovs", "de_debug_exr_aov_framing"}
    for name, (res, args) in native.EXR_AOV_SYMBOLS.items():
        assert res is ctypes.c_int and len(args) == declared[name].count(",") + 1, name
        assert getattr(lib, name) is not None                      # exported
    defines = {k: int(v) for k, v in re.findall(r"^#define (DE_EXR_AOV_\w+) (\d+)", HEADER, flags=re.M)}
    assert {k[len("DE_EXR_AOV_"):].lower(): v for k, v in defines.items() if k != "DE_EXR_AOV_ALL"} == native.EXR_AOVS == xa.BITS
    assert defines["DE_EXR_AOV_ALL"] == native.EXR_AOV_ALL == xa.ALL == sum(xa.BITS.values())
    assert ctypes.sizeof(native.DeExr) == 24
    assert "digital_earth_exr_aovs.h" not in open(os.path.join(ROOT, "include", "digital_earth.h")).read()      # the binder's header stays as it is
    exr_header = open(os.path.join(ROOT, "include", "digital_earth_exr.h")).read()
    assert "extra layers" not in exr_header and "digital_earth_exr_aovs.h" in exr_header


def _chlist_names(front):
    """The names and types of the `channels` attribute of a front, in file order, parsed apart from the reference."""
    at = front.index(b"channels\0chlist\0") + 16
    size, = struct.unpack_from("<i", front, at)
    value, at, out = front[at + 4:at + 4 + size], 0, []
    while value[at] != 0:
        end = value.index(b"\0", at)
        out.append((value[at:end], struct.unpack_from("<i", value, end + 1)[0]))
        at = end + 1 + 16
    assert at + 1 == len(value)
    return out


@pytest.mark.parametrize("pixel_type", ["half", "float"])
def test_front_order_and_capacity_for_all_128_masks(native, lib, pixel_type):
    W, H = 37, 17
    for mask in range(128):
        for compression in (("zip", "zips", "none") if mask in (0, 3, 127) else ("zip",)):
            s = _settings(native, pixel_type, compression)
            want = xa.front(W, H, pixel_type, compression, mask)
            nb = (H + xr.LINES[compression] - 1) // xr.LINES[compression]
            size = len(want) + 8 * nb + 5
            rc, n, cap, out = _framing(lib, s, mask, W, H, size)
            assert rc == 0 and n == len(want) + 8 * nb, mask
            assert out == want + b"\0" * (8 * nb) + b"\xA5" * 5, mask      # the table zeroed, nothing behind it
            got = _chlist_names(out)
            assert [g[0] for g in got] == sorted(g[0] for g in got), mask      # Python's byte-wise sort of the encoded names
            assert got == [(nm.encode(), xr.PIXEL_TYPES[t]) for nm, t in xa.channel_list(mask, pixel_type)], mask
            pixel = sum(4 if t == 2 else 2 for _, t in got)
            assert cap == len(want) + 8 * nb + 8 * nb + H * W * pixel == xa.capacity(W, H, pixel_type, compression, mask), mask
            if mask == 0:
                assert want == xr.front(W, H, pixel_type, compression) and len(want) == 313
                assert cap == xr.capacity(W, H, pixel_type, compression)
    assert [n for n, _ in xa.channel_list(127)] == ["B", "G", "N.X", "N.Y", "N.Z", "R", "Z", "albedo.B", "albedo.G", "albedo.R", "coverage", "samples",
                                                    "transmittance", "variance.B", "variance.G", "variance.R"]
    assert xa.pixel_bytes(127, "half") == 42 and xa.pixel_bytes(127, "float") == 64 and len(xa.front(1, 1, "half", "zip", 127)) == 626


def test_mask_0_is_the_three_channel_entry_point(native, lib):
    for shape in ((1, 1), (700, 33), (1920, 1080)):
        s = _settings(native, "float", "zips")
        nb = shape[1]
        size = 313 + 8 * nb
        rc, n, cap, out = _framing(lib, s, 0, shape[0], shape[1], size)
        old, n0, cap0 = ctypes.create_string_buffer(size), ctypes.c_uint64(), ctypes.c_uint64()
        assert lib.de_debug_exr_framing(ctypes.byref(s), shape[0], shape[1], old, ctypes.c_uint64(size), ctypes.byref(n0), ctypes.byref(cap0)) == 0
        assert rc == 0 and (n, cap, out) == (n0.value, cap0.value, old.raw)


def test_refusals_and_the_limit(native, lib):
    s = _settings(native)
    for mask in (128, 256, 1 << 31, 127 | 128):
        assert _framing(lib, s, mask, 16, 8)[0] == ERR_INVALID       # an unknown bit
    assert _framing(lib, s, 127, 0, 8)[0] == ERR_INVALID and _framing(lib, s, 127, 16, -1)[0] == ERR_INVALID
    bad = _settings(native); bad.chunk_bytes = 100
    assert _framing(lib, bad, 1, 16, 8)[0] == ERR_INVALID
    assert lib.de_debug_exr_aov_framing(None, 1, 16, 8, None, ctypes.c_uint64(0), None, None) == ERR_INVALID
    rc, n, cap, out = _framing(lib, s, 127, 16, 8, size=600)         # too small an `out`: the length, nothing written
    assert rc == ERR_INVALID and n == 626 + 8 and out == b"\xA5" * 600
    # the limit, as the reference alone says it: everything on, 1920 x 1080 and 3840 x 2160 at HALF and FLOAT
    said = {}
    for W, H in ((1920, 1080), (3840, 2160)):
        for pixel_type in ("half", "float"):
            fits = xa.within_limit(W, H, 127, pixel_type)
            said[(W, H, pixel_type)] = fits
            rc, n, cap, _ = _framing(lib, _settings(native, pixel_type), 127, W, H)
            assert (rc == 0) == fits and (not fits or cap == xa.capacity(W, H, pixel_type, "zip", 127)), (W, H, pixel_type)
    assert said == {(1920, 1080, "half"): True, (1920, 1080, "float"): True, (3840, 2160, "half"): False, (3840, 2160, "float"): False}
    assert 1920 * 1080 * 64 < xa.MAX_RAW < 1920 * 1093 * 64      # FLOAT at 1080p is just under the limit
    assert _framing(lib, _settings(native, "float"), 127, 2048, 1024)[0] == 0 and _framing(lib, _settings(native, "float"), 127, 2048, 1025)[0] == ERR_INVALID
    assert _framing(lib, _settings(native, "float"), 0, 3840, 2160)[0] == 0      # the three-channel file's own limit is unchanged


def _cxx():
    import shutil
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    raise AssertionError("no host C++ compiler found (the library's own build needs one too)")


def test_host_leaves_under_the_sanitizers(tmp_path):
    """tools/exr_aov_host_check.cpp: the channel sort, the front, the offsets and the capacity for all masks, and the AOV layout leaf for every thread."""
    import subprocess
    exe = str(tmp_path / "exr_aov_host_check")
    subprocess.check_call([_cxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "exr_aov_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    assert "no sanitizer report" in out.stdout and "128 masks" in out.stdout, out.stdout
