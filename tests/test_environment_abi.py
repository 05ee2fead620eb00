"""The scene-linear panorama's C ABI without a GPU (include/digital_earth_environment.h): the header compiles as pedantic C99 together
with the panorama's and the EXR output's in either order, every entry point it declares is bound and exported and no other table holds it, the
binder's header keeps its 40 entry points at ABI 6 and the panorama header its five, the Python signatures are the documented ones,
de_debug_environment_exr answers every refusal of its arguments and of both settings before the context is read, and the build tracks the new sources."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from digital_earth_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"de_environment_capture", "de_environment_captured", "de_fetch_environment_face", "de_debug_environment_exr"}
H = "digital_earth_environment.h"


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", _header(name), flags=re.S)
    return set(re.findall(r"\b(de_[a-z0-9_]+)\s*\(", text))


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_environment_header_compiles_as_pedantic_c99(tmp_path):
    for order in ((H, "digital_earth_panorama.h", "digital_earth_exr.h"), ("digital_earth_exr.h", "digital_earth_panorama.h", H), ("digital_earth_debug.h", H), (H, "digital_earth_debug.h")):
        src = tmp_path / "t.c"
        src.write_text("".join('#include "%s"\n' % h for h in order) +
                       "int main(void) { de_panorama p; de_exr e; p.struct_bytes = sizeof p; e.struct_bytes = sizeof e; (void)de_environment_capture; (void)de_debug_environment_exr;\n"
                       "  return p.struct_bytes != 68 || e.struct_bytes != 24; }\n")
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def _lib():
    from digital_earth_amd import build
    build.build()
    return ctypes.CDLL(build.OUT)


def test_environment_symbols_declared_bound_and_exported():
    assert _declared(H) == set(_native.ENVIRONMENT_SYMBOLS) == NAMES
    others = [getattr(_native, n) for n in dir(_native) if n.endswith("_SYMBOLS") and n != "ENVIRONMENT_SYMBOLS"]
    assert len(others) >= 17 and not any(NAMES & set(o) for o in others)
    assert len(_declared("digital_earth.h")) == 40 and not NAMES & _declared("digital_earth.h")
    assert len(_declared("digital_earth_panorama.h")) == 5 and not NAMES & _declared("digital_earth_debug.h")
    assert re.search(r"#define\s+DE_ABI_VERSION\s+6\b", _header("digital_earth.h"))
    assert ctypes.sizeof(_native.DePanorama) == 68 and ctypes.sizeof(_native.DeExr) == 24
    res, args = _native.ENVIRONMENT_SYMBOLS["de_environment_capture"]
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.c_int]
    res, args = _native.ENVIRONMENT_SYMBOLS["de_fetch_environment_face"]
    assert res is ctypes.c_int and len(args) == 3 and args[1] is ctypes.c_int
    res, args = _native.ENVIRONMENT_SYMBOLS["de_debug_environment_exr"]
    assert res is ctypes.c_int and len(args) == 8 and args[2] is ctypes.c_int and args[3]._type_ is _native.DePanorama and args[4]._type_ is _native.DeExr and args[6] is ctypes.c_uint64
    assert "ENVIRONMENT_SYMBOLS" in inspect.getsource(_native.load)
    lib = _lib()
    for name in NAMES:
        assert hasattr(lib, name), name
    lib.de_abi_version.restype = ctypes.c_int
    assert lib.de_abi_version() == 6 == _native.ABI_VERSION


def test_environment_python_api_without_a_device():
    from digital_earth_amd.renderer import Renderer
    from digital_earth_amd.earth_viewer import EarthViewer
    sig = lambda f: inspect.signature(f).parameters
    assert list(sig(Renderer.capture_environment_face))[1:] == ["face"] and list(sig(Renderer.fetch_environment_face))[1:] == ["face"]
    assert isinstance(Renderer.environment, property) and isinstance(Renderer.panorama, property)
    env = sig(Renderer.render_environment)
    assert list(env)[1:] == ["spp", "basis", "display"] and env["basis"].default is None and env["display"].default is False
    dbg = sig(Renderer.debug_environment_exr)
    assert list(dbg)[1:] == ["faces", "size", "projection", "aperture", "apron", "supersample", "basis", "pixel_type", "compression", "chunk_bytes", "scale"]
    assert [dbg[k].default for k in ("projection", "aperture", "apron", "supersample", "basis", "pixel_type", "compression", "chunk_bytes", "scale")] == \
        ["equirect", 180.0, 1, 2, None, "half", "zip", None, 1.0]
    # what the panorama's tests pin stays
    assert list(sig(Renderer.render_panorama))[1:] == ["spp", "basis"]
    assert list(sig(Renderer.fetch_exr))[1:] == ["copy", "lag"]
    assert list(sig(EarthViewer.frame))[1:] == ["spp", "copy", "pipelined", "pixels", "sliders"]
    # one loop, two callers
    for f in (Renderer.render_panorama, Renderer.render_environment):
        assert "_render_faces" in inspect.getsource(f) and "accumulate" not in inspect.getsource(f).split('"""')[2]
    assert "render_environment" in inspect.getsource(EarthViewer.frame) and "does not go with exr" not in inspect.getsource(EarthViewer.frame)


def test_every_refusal_answers_before_the_context_is_read():
    """de_debug_environment_exr checks its arguments, the panorama settings (against the faces' size), the EXR settings and the EXR size limit at the
    panorama's size before it reads the context: held without a GPU, with a context pointer that a refused call never dereferences."""
    lib = _lib()
    fn = lib.de_debug_environment_exr
    fn.restype, fn.argtypes = _native.ENVIRONMENT_SYMBOLS["de_debug_environment_exr"]
    ctx = ctypes.c_void_p(1)
    faces = np.zeros((6, 16, 16, 3), np.float32)
    out, n = ctypes.create_string_buffer(b"\xA5" * 64, 64), ctypes.c_uint64(77)

    def pano(**kw):
        s = _native.DePanorama()
        s.struct_bytes, s.on, s.projection, s.width, s.height, s.aperture_deg, s.apron, s.supersample = ctypes.sizeof(s), 1, 0, 64, 32, 180.0, 1, 2
        for k in range(9):
            s.basis[k] = float(np.eye(3).reshape(9)[k])
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def exr(**kw):
        s = _native.DeExr()
        s.struct_bytes, s.source, s.pixel_type, s.compression, s.chunk_bytes, s.scale = ctypes.sizeof(s), 0, 1, 3, 32768, 1.0
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def call(c=ctx, f=faces.ctypes.data, size=16, p=None, e=None, o=out, room=64, length=n):
        return fn(c, f, size, ctypes.byref(p or pano()), ctypes.byref(e or exr()), o, ctypes.c_uint64(room), ctypes.byref(length) if length is not None else None)
    for kw in (dict(struct_bytes=64), dict(projection=2), dict(width=40), dict(height=12), dict(width=0), dict(projection=1), dict(projection=1, width=32, height=32, aperture_deg=0.0),
               dict(apron=0), dict(apron=5), dict(supersample=0), dict(supersample=5)):
        assert call(p=pano(**kw)) == _native.DE_ERR_INVALID, kw
    for kw in (dict(struct_bytes=20), dict(source=5), dict(pixel_type=0), dict(compression=1), dict(chunk_bytes=1023), dict(chunk_bytes=65536), dict(scale=0.0),
               dict(scale=float("inf")), dict(scale=float("nan"))):
        assert call(e=exr(**kw)) == _native.DE_ERR_INVALID, kw
    # the EXR size limit at the PANORAMA's size, width height 3 bps <= 2^27: 4096 x 2048 fits at half and at float (no refusal to show without a device),
    # 6144 x 2048 only at half, 8192 x 4096 at neither
    assert call(p=pano(width=6144, height=2048), e=exr(pixel_type=2)) == _native.DE_ERR_INVALID
    assert call(p=pano(width=8192, height=4096)) == _native.DE_ERR_INVALID
    assert 4096 * 2048 * 3 * 4 <= 1 << 27 < 6144 * 2048 * 3 * 4 and 6144 * 2048 * 3 * 2 <= 1 << 27 < 8192 * 4096 * 3 * 2
    assert call(size=3) == _native.DE_ERR_INVALID and call(size=16385) == _native.DE_ERR_INVALID
    assert call(c=None) == _native.DE_ERR_INVALID and call(f=None) == _native.DE_ERR_INVALID and call(o=None) == _native.DE_ERR_INVALID and call(length=None) == _native.DE_ERR_INVALID
    assert fn(ctx, faces.ctypes.data, 16, None, ctypes.byref(exr()), out, ctypes.c_uint64(64), ctypes.byref(n)) == _native.DE_ERR_INVALID
    assert fn(ctx, faces.ctypes.data, 16, ctypes.byref(pano()), None, out, ctypes.c_uint64(64), ctypes.byref(n)) == _native.DE_ERR_INVALID
    assert out.raw == b"\xA5" * 64 and n.value == 77                  # a refused call changes nothing
    for name in ("de_environment_capture", "de_environment_captured", "de_fetch_environment_face"):      # a null context is an argument, not a crash
        f = getattr(lib, name)
        f.restype, f.argtypes = _native.ENVIRONMENT_SYMBOLS[name]
    assert lib.de_environment_capture(None, 0) == _native.DE_ERR_INVALID and lib.de_environment_captured(None, None) == _native.DE_ERR_INVALID
    assert lib.de_fetch_environment_face(None, 0, None) == _native.DE_ERR_INVALID


def test_build_tracks_the_new_sources():
    from digital_earth_amd import build
    for name in ("environment_kernels.hip", "environment_body.h", "panorama_body.h"):
        assert name in build.DEPS
    assert any(d.endswith(H) for d in build.DEPS)
    ctx = open(os.path.join(build.CSRC, "de_context.h")).read()
    assert ctx.index('#include "environment_kernels.hip"') > ctx.index('#include "panorama_kernels.hip"')      # its leaves and tables are that file's
    body = open(os.path.join(build.CSRC, "panorama_body.h")).read()
    assert body.count("DE_DEV void pano_pixel_mean(") == 1 and body.count("mean[ch] + (v[ch] - mean[ch]) * w") == 1      # one running mean, two stores
    assert "pano_pixel_mean(" in body.split("DE_DEV void pano_pixel(")[1] and "pano_pixel_mean(" in body.split("DE_DEV void pano_pixel_rows(")[1]
    env = open(os.path.join(build.CSRC, "environment_body.h")).read()
    assert "hip" not in env.split("#pragma once")[1]                 # the capture's two phases need nothing of the device
    for tool in ("environment_host_check.cpp", "environment_host_check.py", "panorama_host_check.cpp"):
        assert os.path.exists(os.path.join(ROOT, "tools", tool))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no C++ compiler")
def test_the_host_builds_of_both_bodies_equal_numpy(tmp_path):
    """tools/environment_host_check.cpp and the rows side of tools/panorama_host_check.cpp WITHOUT the sanitizers (tools/*_host_check.py run them with):
    the capture's two phases give sums / count transposed, per frame and per tile, on 2 x 2 tiles with the last partial; the row-major store gives the
    restatement's image transposed, on 3 x 2 tiles with the tables staged as the kernel stages them."""
    import panorama_ref as ref
    F = np.float32
    flags = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fno-fast-math"]
    exe = str(tmp_path / "capture")
    subprocess.check_call(flags + [os.path.join(ROOT, "tools", "environment_host_check.cpp"), "-o", exe])
    rng = np.random.default_rng(5)
    N = 48
    sums = (rng.random((N, N, 3), dtype=F) * F(1e4) - F(100.0)).astype(F)
    counts = rng.integers(1, 40, (N // 8, N // 8)).astype(np.int32)
    for per_tile in (False, True):
        with open(str(tmp_path / "in.bin"), "wb") as fh:
            fh.write(np.array([N, 3, int(per_tile)], np.int32).tobytes() + sums.tobytes() + (counts.tobytes() if per_tile else b""))
        subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
        got = np.fromfile(str(tmp_path / "out.bin"), F).reshape(N, N, 3)
        div = np.repeat(np.repeat(counts, 8, axis=0), 8, axis=1).astype(F)[..., None] if per_tile else F(3)
        want = np.ascontiguousarray((sums / div).astype(F).transpose(1, 0, 2))
        assert (got.view(np.uint32) == want.view(np.uint32)).all(), per_tile
    exe = str(tmp_path / "rows")
    subprocess.check_call(flags + [os.path.join(ROOT, "tools", "panorama_host_check.cpp"), "-o", exe])
    faces = (rng.random((6, 16, 16, 3), dtype=F) * F(1e4) - F(100.0)).astype(F)
    for size, projection, aperture, S in (((96, 40), "equirect", 180.0, 4), ((48, 48), "fisheye", 90.0, 3)):
        fov, scale, half, m = ref.consts(16, 4, aperture, None)
        tabs = ref.tables(size[0], S, 2.0 * np.pi) + ref.tables(size[1], S, np.pi)
        with open(str(tmp_path / "in.bin"), "wb") as fh:
            fh.write(np.array([16, size[0], size[1], S, int(projection == "fisheye")], np.int32).tobytes())
            fh.write(np.array([fov, scale, half], F).tobytes() + np.ascontiguousarray(m, F).tobytes())
            for t in tabs:
                fh.write(np.ascontiguousarray(t, F).tobytes())
            fh.write(faces.tobytes())
        subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), "rows"])
        got = np.ascontiguousarray(np.fromfile(str(tmp_path / "out.bin"), F).reshape(size[1], size[0], 3).transpose(1, 0, 2))
        want = ref.panorama(faces, size, projection, aperture, 4, S)
        assert (got.view(np.uint32) == want.view(np.uint32)).all(), (size, projection)
