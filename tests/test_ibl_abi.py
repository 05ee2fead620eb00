"""The IBL output's ABI without a GPU (include/digital_earth_ibl.h): the header as pedantic C99, declared = bound = exported, the struct, every refusal
of de_set_ibl and de_debug_ibl before the context is read, digital_earth_amd/dds.py's round trip and refusals, the build list, and the kernels'
bodies under the sanitizers (tools/ibl_host_check.cpp, a program of its own)."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ibl_ref as ir
from digital_earth_amd import _native, dds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "digital_earth_ibl.h")).read()
NAMES = {"de_set_ibl", "de_get_ibl", "de_ibl_build", "de_fetch_ibl_sh", "de_fetch_ibl_face", "de_ibl_file_bytes", "de_fetch_ibl_dds", "de_debug_ibl"}


def _lib():
    from digital_earth_amd import build
    build.build()
    return ctypes.CDLL(build.OUT)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_header_compiles_as_pedantic_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "digital_earth_ibl.h"\nint main(void) { de_ibl s; s.struct_bytes = sizeof s; (void)de_ibl_build; (void)de_debug_ibl; return s.struct_bytes != 28; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_declared_bound_and_exported():
    body = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    declared = dict(re.findall(r"^int (de_\w+)\(([^;]*)\);", body, flags=re.M))
    assert set(declared) == set(_native.IBL_SYMBOLS) == NAMES
    for name, (res, args) in _native.IBL_SYMBOLS.items():
        assert res is ctypes.c_int and len(args) == declared[name].count(",") + 1, name
    others = [getattr(_native, n) for n in dir(_native) if n.endswith("_SYMBOLS") and n != "IBL_SYMBOLS"]
    assert not any(NAMES & set(o) for o in others)
    assert "digital_earth_ibl.h" not in open(os.path.join(ROOT, "include", "digital_earth.h")).read()      # the binder's header stays as it is
    assert "IBL_SYMBOLS" in inspect.getsource(_native.load) and _native.ABI_VERSION == 6
    lib = _lib()
    for name in NAMES:
        assert hasattr(lib, name), name


def test_struct_size_and_fields():
    fields = re.search(r"typedef struct de_ibl \{(.*?)\} de_ibl;", HEADER, flags=re.S).group(1)
    names = re.findall(r"^\s*(?:u?int32_t|float) (\w+);", fields, flags=re.M)
    assert names == [f[0] for f in _native.DeIbl._fields_] == ir.FIELDS
    assert ctypes.sizeof(_native.DeIbl) == ir.STRUCT_BYTES == 28


def test_the_build_tracks_the_new_sources_and_the_python_api():
    from digital_earth_amd import build
    from digital_earth_amd.renderer import Renderer
    from digital_earth_amd.earth_viewer import EarthViewer
    for name in ("ibl_kernels.hip", "ibl_body.h", "ibl_tables.h", os.path.join("..", "..", "include", "digital_earth_ibl.h")):
        assert name in build.DEPS and os.path.exists(os.path.join(build.CSRC, name)), name
    sig = inspect.signature(Renderer.set_ibl).parameters
    assert list(sig)[1:] == ["edge", "levels", "samples", "supersample", "lod_bias", "pixel_type"]
    assert {k: sig[k].default for k in ir.DEFAULTS} == ir.DEFAULTS
    assert isinstance(Renderer.ibl, property)
    for name in ("build_ibl", "fetch_ibl_sh", "fetch_ibl_face", "fetch_ibl_dds", "debug_ibl"):
        assert callable(getattr(Renderer, name))
    assert list(inspect.signature(Renderer.fetch_ibl_face).parameters)[1:] == ["level", "face"]
    assert "build_ibl" in inspect.getsource(EarthViewer.frame) and '".dds"' in inspect.getsource(EarthViewer.save)


def _ibl(**kw):
    s = _native.DeIbl()
    s.struct_bytes, s.edge, s.levels, s.samples, s.supersample, s.lod_bias, s.pixel_type = ctypes.sizeof(s), 16, 5, 8, 1, 0.0, 1
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _pano(**kw):
    s = _native.DePanorama()
    s.struct_bytes, s.on, s.projection, s.width, s.height, s.aperture_deg, s.apron, s.supersample = ctypes.sizeof(s), 1, 0, 64, 32, 180.0, 1, 2
    for k in range(9):
        s.basis[k] = float(np.eye(3).reshape(9)[k])
    for k, v in kw.items():
        setattr(s, k, v)
    return s


BAD_IBL = [dict(struct_bytes=24), dict(struct_bytes=32), dict(edge=4), dict(edge=2048), dict(edge=24), dict(edge=0), dict(edge=-16), dict(levels=1), dict(levels=6),
           dict(edge=1024, levels=12), dict(samples=4), dict(samples=2048), dict(samples=12), dict(supersample=0), dict(supersample=5), dict(lod_bias=float("nan")),
           dict(lod_bias=float("inf")), dict(pixel_type=0), dict(pixel_type=3)]


def test_every_refusal_answers_before_the_context_is_read():
    """A context pointer that a refused call never dereferences: de_set_ibl and de_debug_ibl check their arguments and settings first."""
    lib = _lib()
    for name in ("de_set_ibl", "de_debug_ibl"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _native.IBL_SYMBOLS[name]
    ctx = ctypes.c_void_p(1)
    for kw in BAD_IBL:
        assert lib.de_set_ibl(ctx, ctypes.byref(_ibl(**kw))) == _native.DE_ERR_INVALID, kw
    assert lib.de_set_ibl(ctx, None) == _native.DE_ERR_INVALID and lib.de_set_ibl(None, ctypes.byref(_ibl())) == _native.DE_ERR_INVALID
    faces = np.zeros((6, 16, 16, 3), np.float32)
    sh = np.full(27, 7.0, np.float32)
    room = 148 + 6 * (256 + 64 + 16 + 4 + 1) * 8
    out = ctypes.create_string_buffer(b"\xA5" * room, room)

    def call(c=ctx, f=faces.ctypes.data, n=16, p=None, s=None, o=out, size=room):
        return lib.de_debug_ibl(c, f, n, ctypes.byref(p or _pano()), ctypes.byref(s or _ibl()), sh.ctypes.data, None, o, ctypes.c_uint64(size))
    for kw in BAD_IBL:
        assert call(s=_ibl(**kw)) == _native.DE_ERR_INVALID, kw
    for kw in (dict(struct_bytes=64), dict(projection=2), dict(width=40), dict(apron=0), dict(apron=5), dict(supersample=0)):
        assert call(p=_pano(**kw)) == _native.DE_ERR_INVALID, kw
    bad_basis = _pano()
    bad_basis.basis[0] = 2.0
    assert call(p=bad_basis) == _native.DE_ERR_INVALID
    assert call(c=None) == _native.DE_ERR_INVALID and call(f=None) == _native.DE_ERR_INVALID and call(n=3) == _native.DE_ERR_INVALID and call(n=16385) == _native.DE_ERR_INVALID
    assert call(size=room - 1) == _native.DE_ERR_INVALID                                            # too small a `dds`
    assert call(s=_ibl(pixel_type=2)) == _native.DE_ERR_INVALID                                     # float needs twice the room
    assert out.raw == b"\xA5" * room and (sh == 7.0).all()                                          # a refused call writes nothing
    # the payload limit: with E <= 1024 the largest payload is 32 bytes short of 2^27, so no setting inside the ranges reaches the refusal
    assert 6 * sum((1024 >> l) ** 2 for l in range(11)) * 16 == (1 << 27) - 32


def test_dds_round_trip_and_refusals():
    rng = np.random.default_rng(5)
    levels = [(rng.random((6, 8 >> l, 8 >> l, 3)) * 100).astype(np.float32) for l in range(3)]
    levels[0][2, 1, 3] = [70000.0, -70000.0, np.nan]
    for pixel_type, bpp in (("half", 8), ("float", 16)):
        data = dds.write(levels, pixel_type)
        assert len(data) == 148 + 6 * (64 + 16 + 4) * bpp and data[:4] == b"DDS " and data[84:88] == b"DX10"
        back, info = dds.read(data)
        assert info == dict(edge=8, levels=3, pixel_type=pixel_type)
        for l in range(3):
            assert (back[l][..., 3] == 1).all()
            if pixel_type == "float":
                assert np.array_equal(back[l][..., :3].view(np.uint32), levels[l].view(np.uint32))
            else:
                want = np.where(np.isnan(levels[l]), 0, np.clip(levels[l], -65504, 65504)).astype(np.float16).astype(np.float32)
                assert np.array_equal(back[l][..., :3], want)
        assert np.frombuffer(data, np.uint16 if pixel_type == "half" else np.uint32, 3, 148 + (2 * (64 + 16 + 4) + 8 + 3) * bpp).tolist() == \
            ([0x7BFF, 0xFBFF, 0] if pixel_type == "half" else [0x4788B800, 0xC788B800, 0x7FC00000])
        # the order: face-major, each face followed by its levels
        first = np.frombuffer(data, np.float16 if pixel_type == "half" else np.float32, 4, 148 + 64 * bpp).astype(np.float32)
        assert np.array_equal(first[:3], back[1][0, 0, 0, :3])
    good = dds.write(levels, "half")
    words = lambda k, v: good[:4 * k] + int(v).to_bytes(4, "little") + good[4 * k + 4:]
    for bad, what in ((good[:100], "shorter"), (b"XXXX" + good[4:], "magic"), (words(1, 100), "sizes"), (words(21, 0x31545844), "DX10"), (words(32, 28), "DXGI format"),
                      (words(34, 0), "cube"), (words(35, 2), "cube"), (words(28, 0x200), "cube"), (words(3, 16), "power of two"), (words(7, 5), "mipMapCount"),
                      (good + b"\0", "bytes"), (good[:-1], "bytes")):
        with pytest.raises(dds.DdsError, match=what):
            dds.read(bad)
    with pytest.raises(dds.DdsError):
        dds.write(levels[:1] + levels[:1], "half")
    with pytest.raises(dds.DdsError):
        dds.write(levels, "rgbe")


def _cxx():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    raise AssertionError("no host C++ compiler found (the library's own build needs one too)")


def test_host_bodies_under_the_sanitizers(tmp_path):
    """tools/ibl_host_check.cpp: every thread of every kernel's launch shape on heap blocks of exactly their sizes, on the CPU."""
    exe = str(tmp_path / "ibl_host_check")
    subprocess.check_call([_cxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "ibl_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    assert "no sanitizer report" in out.stdout and "kept samples" in out.stdout, out.stdout
