"""The BC6H stage's ABI without a GPU (include/digital_earth_ibl_bc6h.h): the header as pedantic C99, declared = bound = exported, the struct, every
refusal before the context is read, what must not have changed, bc6h.py's file round trip and refusals, the C tables against bc6h.py's, and the
encoder's body under the sanitizers (tools/bc6h_host_check.cpp, a program of its own)."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bc6h_ref as br
from digital_earth_amd import _native, bc6h, dds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "digital_earth_ibl_bc6h.h")).read()
NAMES = {"de_set_ibl_bc6h", "de_get_ibl_bc6h", "de_ibl_bc6h_file_bytes", "de_fetch_ibl_bc6h_dds", "de_debug_bc6h_encode", "de_debug_ibl_bc6h"}


def _lib():
    from digital_earth_amd import build
    build.build()
    return ctypes.CDLL(build.OUT)


def test_pillow_is_here():
    import PIL.Image      # noqa: F401 — tests/test_bc6h_ref.py's importorskip must not fire where this suite is built
    from PIL import DdsImagePlugin      # noqa: F401


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_header_compiles_as_pedantic_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "digital_earth_ibl_bc6h.h"\nint main(void) { de_ibl_bc6h s; de_ibl i; s.struct_bytes = sizeof s; i.struct_bytes = sizeof i; (void)de_fetch_ibl_bc6h_dds; '
                   '(void)de_debug_bc6h_encode; (void)de_debug_ibl_bc6h; return s.struct_bytes != 12 || i.struct_bytes != 28; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_declared_bound_exported_and_what_stays():
    body = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    declared = dict(re.findall(r"^int (de_\w+)\(([^;]*)\);", body, flags=re.M))
    assert set(declared) == set(_native.IBL_BC6H_SYMBOLS) == NAMES
    for name, (res, args) in _native.IBL_BC6H_SYMBOLS.items():
        assert res is ctypes.c_int and len(args) == declared[name].count(",") + 1, name
    others = [getattr(_native, n) for n in dir(_native) if n.endswith("_SYMBOLS") and n != "IBL_BC6H_SYMBOLS"]
    assert not any(NAMES & set(o) for o in others)
    main_header = open(os.path.join(ROOT, "include", "digital_earth.h")).read()
    assert "bc6h" not in main_header.lower() and "#define DE_ABI_VERSION 6" in main_header
    assert "IBL_BC6H_SYMBOLS" in inspect.getsource(_native.load) and _native.ABI_VERSION == 6
    assert '#include "digital_earth_ibl.h"' in HEADER
    assert set(_native.IBL_SYMBOLS) == {"de_set_ibl", "de_get_ibl", "de_ibl_build", "de_fetch_ibl_sh", "de_fetch_ibl_face", "de_ibl_file_bytes", "de_fetch_ibl_dds", "de_debug_ibl"}
    assert ctypes.sizeof(_native.DeIbl) == 28
    lib = _lib()
    for name in NAMES:
        assert hasattr(lib, name), name


def test_struct_size_and_fields():
    fields = re.search(r"typedef struct de_ibl_bc6h \{(.*?)\} de_ibl_bc6h;", HEADER, flags=re.S).group(1)
    names = re.findall(r"^\s*(?:u?int32_t|float) (\w+);", fields, flags=re.M)
    assert names == [f[0] for f in _native.DeIblBc6h._fields_] == br.FIELDS
    assert ctypes.sizeof(_native.DeIblBc6h) == br.STRUCT_BYTES == 12


def test_the_build_tracks_the_new_sources_and_the_python_api():
    from digital_earth_amd import build
    from digital_earth_amd.renderer import Renderer
    from digital_earth_amd.earth_viewer import EarthViewer
    for name in ("bc6h_kernels.hip", "bc6h_body.h", "bc6h_tables.h", os.path.join("..", "..", "include", "digital_earth_ibl_bc6h.h")):
        assert name in build.DEPS and os.path.exists(os.path.join(build.CSRC, name)), name
    assert list(inspect.signature(Renderer.set_ibl).parameters)[1:] == ["edge", "levels", "samples", "supersample", "lod_bias", "pixel_type"]
    sig = inspect.signature(Renderer.set_ibl_bc6h).parameters
    assert list(sig)[1:] == ["on", "quality"] and sig["on"].default is True and sig["quality"].default == 0
    assert isinstance(Renderer.ibl_bc6h, property)
    for name in ("fetch_ibl_bc6h_dds", "debug_bc6h_encode", "debug_ibl_bc6h"):
        assert callable(getattr(Renderer, name))
    assert "ibl_bc6h" in inspect.signature(EarthViewer.__init__).parameters
    assert "fetch_ibl_bc6h_dds" in inspect.getsource(EarthViewer.frame) and "fetch_ibl_bc6h_dds" in inspect.getsource(EarthViewer.save)


def _bc(**kw):
    s = _native.DeIblBc6h()
    s.struct_bytes, s.on, s.quality = ctypes.sizeof(s), 1, 0
    for k, v in kw.items():
        setattr(s, k, v)
    return s


BAD = [dict(struct_bytes=8), dict(struct_bytes=16), dict(on=2), dict(on=-1), dict(quality=2), dict(quality=-1)]


def test_every_refusal_answers_before_the_context_is_read():
    """A context pointer that a refused call never dereferences."""
    from test_ibl_abi import BAD_IBL, _ibl, _pano
    lib = _lib()
    for name in NAMES:
        getattr(lib, name).restype, getattr(lib, name).argtypes = _native.IBL_BC6H_SYMBOLS[name]
    ctx = ctypes.c_void_p(1)
    for kw in BAD:
        assert lib.de_set_ibl_bc6h(ctx, ctypes.byref(_bc(**kw))) == _native.DE_ERR_INVALID, kw
    assert lib.de_set_ibl_bc6h(ctx, None) == _native.DE_ERR_INVALID and lib.de_set_ibl_bc6h(None, ctypes.byref(_bc())) == _native.DE_ERR_INVALID
    assert lib.de_get_ibl_bc6h(None, ctypes.byref(_bc())) == _native.DE_ERR_INVALID and lib.de_ibl_bc6h_file_bytes(ctx, None) == _native.DE_ERR_INVALID
    assert lib.de_fetch_ibl_bc6h_dds(ctx, None, 0) == _native.DE_ERR_INVALID
    image = np.zeros((7, 5, 3), np.float32)
    out = ctypes.create_string_buffer(b"\xA5" * 64, 64)

    def enc(c=ctx, i=image.ctypes.data, w=5, h=7, s=None, o=out, n=64):
        return lib.de_debug_bc6h_encode(c, i, w, h, ctypes.byref(s or _bc()), o, ctypes.c_uint64(n))
    for kw in BAD:
        assert enc(s=_bc(**kw)) == _native.DE_ERR_INVALID, kw
    for kw in (dict(c=None), dict(i=None), dict(o=None), dict(w=0), dict(h=0), dict(w=16385), dict(h=-4), dict(n=63)):
        assert enc(**kw) == _native.DE_ERR_INVALID, kw
    faces = np.zeros((6, 16, 16, 3), np.float32)
    room = 148 + 96 * (16 + 4 + 1 + 1 + 1)
    big = ctypes.create_string_buffer(b"\xA5" * room, room)

    def bake(c=ctx, f=faces.ctypes.data, n=16, p=None, s=None, b=None, size=room):
        return lib.de_debug_ibl_bc6h(c, f, n, ctypes.byref(p or _pano()), ctypes.byref(s or _ibl()), ctypes.byref(b or _bc()), None, None, None, big, ctypes.c_uint64(size))
    for kw in BAD:
        assert bake(b=_bc(**kw)) == _native.DE_ERR_INVALID, kw
    for kw in BAD_IBL:
        assert bake(s=_ibl(**kw)) == _native.DE_ERR_INVALID, kw
    assert bake(p=_pano(apron=0)) == _native.DE_ERR_INVALID and bake(c=None) == _native.DE_ERR_INVALID and bake(f=None) == _native.DE_ERR_INVALID and bake(n=3) == _native.DE_ERR_INVALID
    assert bake(size=room - 1) == _native.DE_ERR_INVALID
    assert out.raw == b"\xA5" * 64 and big.raw == b"\xA5" * room                     # a refused call writes nothing


def test_file_round_trip_and_refusals():
    rng = np.random.default_rng(5)
    levels = [(rng.random((6, 8 >> l, 8 >> l, 3)) * 4).astype(np.float32) for l in range(4)]
    levels[0][2, 1, 3] = [70000.0, -70000.0, np.nan]
    for quality in (0, 1):
        data = bc6h.write(levels, quality)
        assert len(data) == bc6h.file_bytes(8, 4) == 148 + 6 * 16 * (4 + 1 + 1 + 1) and data[:4] == b"DDS " and data[84:88] == b"DX10"
        w = np.frombuffer(data, np.uint32, 37)
        assert w[2] == 0x000A1007 and w[5] == 64 and w[32] == 95 and w[7] == 4 and w[3] == w[4] == 8
        same = [k for k in range(37) if w[k] == np.frombuffer(dds.header(8, 4), np.uint32)[k]]
        assert sorted(set(range(37)) - set(same)) == [2, 32]      # today's header but for flags and format (and the linear size, which at E = 8 equals the half file's pitch)
        back, info = bc6h.read(data)
        assert info == dict(edge=8, levels=4)
        at = 148
        for face in range(6):                                                         # face-major, each face followed by its levels
            for l in range(4):
                e = 8 >> l
                n = 16 * bc6h.level_blocks(e)
                assert data[at:at + n] == br.encode(levels[l][face], quality)
                assert np.array_equal(back[l][face], bc6h.decode_blocks(data[at:at + n], e, e))
                at += n
        assert back[0][2, 1, 3].tolist()[1:] == [0, 0]
        assert bc6h.write([bc6h.to_half(v) for v in levels], quality) == data       # half integers in give the same file
    good = bc6h.write(levels, 0)
    words = lambda k, v: good[:4 * k] + int(v).to_bytes(4, "little") + good[4 * k + 4:]
    for bad, what in ((good[:100], "shorter"), (b"XXXX" + good[4:], "magic"), (words(1, 100), "sizes"), (words(21, 0x31545844), "DX10"), (words(32, 10), "DXGI format"),
                      (words(34, 0), "cube"), (words(35, 2), "cube"), (words(28, 0x200), "cube"), (words(3, 16), "power of two"), (words(7, 5), "mipMapCount"),
                      (words(2, 0x0002100F), "LINEARSIZE"), (words(5, 128), "LINEARSIZE"), (good + b"\0", "bytes"), (good[:-1], "bytes")):
        with pytest.raises(dds.DdsError, match=what):
            bc6h.read(bad)
    with pytest.raises(dds.DdsError, match="DXGI format"):
        dds.read(good)                                                                # dds.read's refusals stay
    with pytest.raises(dds.DdsError):
        bc6h.write(levels[:1] + levels[:1], 0)
    with pytest.raises(ValueError):
        bc6h.write(levels, 2)


def _cxx():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    raise AssertionError("no host C++ compiler found (the library's own build needs one too)")


def test_host_body_under_the_sanitizers_and_the_c_tables(tmp_path):
    """tools/bc6h_host_check.cpp: every thread of both launch shapes on heap blocks of exactly their sizes, on the CPU; and the tables it prints
    (csrc/bc6h_tables.h) against bc6h.py's, which were written on their own."""
    exe = str(tmp_path / "bc6h_host_check")
    subprocess.check_call([_cxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "bc6h_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    assert "no sanitizer report" in out.stdout and "297 blocks" in out.stdout, out.stdout
    seen = 0
    for line in out.stdout.splitlines():
        m = re.match(r"mode (\d+) value (\d+) count (\d+) precision (\d+) delta (\d+) (\d+) (\d+) regions (\d+) layout (.*)", line)
        if m:
            mode = int(m.group(1))
            assert bc6h.MODES[mode] == (int(m.group(2)), int(m.group(3)), int(m.group(4)), (int(m.group(5)), int(m.group(6)), int(m.group(7))), int(m.group(8)))
            assert m.group(9).split() == ["%s%d" % (n, k) for n, k in bc6h.layout_bits(mode) if n != "M"], mode
            seen += 1
        m = re.match(r"partition (\d+) anchor (\d+) regions ([01]{16})", line)
        if m:
            assert bc6h.ANCHORS[int(m.group(1))] == int(m.group(2)) and bc6h.PARTITIONS[int(m.group(1))] == m.group(3)
            seen += 1
    assert seen == 14 + 32
