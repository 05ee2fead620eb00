"""The panorama C ABI without a GPU: include/digital_earth_panorama.h compiles as pedantic C99 together with the debug header in either order, the
struct mirror matches field by field, every entry point it declares is bound and exported, the binder's header keeps its 40 entry points at ABI 6, the
Python signatures have the documented defaults, every refusal of the settings answers its code before the context is read, and the build tracks the
new sources."""
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
NAMES = {"de_set_panorama", "de_get_panorama", "de_panorama_face_camera", "de_panorama_capture", "de_panorama_captured"}
DEBUG_NAMES = {"de_debug_panorama"}
CTYPE = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "float": ctypes.c_float}
H = "digital_earth_panorama.h"


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", _header(name), flags=re.S)
    return set(re.findall(r"\b(de_[a-z0-9_]+)\s*\(", text))


def _fields():
    body = re.search(r"typedef struct de_panorama \{(.*?)\} de_panorama;", _header(H), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        m = re.match(r"\s*(uint32_t|int32_t|float)\s+(.+?)\s*$", decl.strip(), re.S)
        if not m:
            assert not decl.strip(), decl
            continue
        for item in m.group(2).split(","):
            name, count = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", item).groups()
            out.append((name, CTYPE[m.group(1)] * int(count) if count else CTYPE[m.group(1)]))
    return out


def test_panorama_struct_matches_header():
    import panorama_ref
    want = _fields()
    assert [n for n, _ in want] == ["struct_bytes", "on", "projection", "width", "height", "aperture_deg", "apron", "supersample", "basis"]
    assert [n for n, _ in _native.DePanorama._fields_] == [n for n, _ in want]
    for (n, a), (_, b) in zip(_native.DePanorama._fields_, want):
        assert a is b, n
    assert ctypes.sizeof(_native.DePanorama) == 68 == panorama_ref.STRUCT_BYTES
    defs = dict(re.findall(r"#define\s+DE_PANO_(\w+)\s+(\d+)", _header(H)))
    assert defs == {"EQUIRECT": "0", "FISHEYE": "1", "FACES": "6"}


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_panorama_header_compiles_as_pedantic_c99(tmp_path):
    for first, second in ((H, "digital_earth_debug.h"), ("digital_earth_debug.h", H)):
        src = tmp_path / "t.c"
        src.write_text('#include "%s"\n#include "%s"\n' % (first, second) +
                       'int main(void) { de_panorama s; s.struct_bytes = sizeof s; (void)de_debug_panorama; return s.struct_bytes != 68 || DE_PANO_FISHEYE != 1; }\n')
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def _lib():
    from digital_earth_amd import build
    build.build()
    return ctypes.CDLL(build.OUT)


def test_panorama_symbols_declared_bound_and_exported():
    assert _declared(H) == set(_native.PANORAMA_SYMBOLS) == NAMES
    others = [getattr(_native, n) for n in dir(_native) if n.endswith("_SYMBOLS") and n != "PANORAMA_SYMBOLS"]
    assert not any(set(_native.PANORAMA_SYMBOLS) & set(o) for o in others)
    assert len(_declared("digital_earth.h")) == 40 and not (NAMES | DEBUG_NAMES) & _declared("digital_earth.h")
    assert re.search(r"#define\s+DE_ABI_VERSION\s+6\b", _header("digital_earth.h"))
    for name in ("de_set_panorama", "de_get_panorama"):
        res, args = _native.PANORAMA_SYMBOLS[name]
        assert res is ctypes.c_int and len(args) == 2 and args[1]._type_ is _native.DePanorama
    assert len(_native.PANORAMA_SYMBOLS["de_panorama_face_camera"][1]) == 6
    assert DEBUG_NAMES <= _declared("digital_earth_debug.h") and DEBUG_NAMES <= set(_native.DEBUG_SYMBOLS)
    res, args = _native.DEBUG_SYMBOLS["de_debug_panorama"]
    assert res is ctypes.c_int and len(args) == 5 and args[2] is ctypes.c_int and args[3]._type_ is _native.DePanorama
    assert "PANORAMA_SYMBOLS" in inspect.getsource(_native.load)
    lib = _lib()
    for name in NAMES | DEBUG_NAMES:
        assert hasattr(lib, name), name
    lib.de_abi_version.restype = ctypes.c_int
    assert lib.de_abi_version() == 6 == _native.ABI_VERSION


def test_panorama_python_api_without_a_device():
    from digital_earth_amd.renderer import Renderer
    from digital_earth_amd.earth_viewer import EarthViewer
    import panorama_ref
    sig = inspect.signature(Renderer.set_panorama).parameters
    assert list(sig)[1:] == ["size", "projection", "aperture", "apron", "supersample", "basis", "on"]
    assert panorama_ref.DEFAULTS == {k: v.default for k, v in sig.items() if k != "self"}
    assert Renderer.PANORAMA_PROJECTIONS == panorama_ref.PROJECTIONS and len(Renderer.PANORAMA_FACES) == 6
    assert list(inspect.signature(Renderer.debug_panorama).parameters)[1:] == ["faces", "size", "projection", "aperture", "apron", "supersample", "basis"]
    assert list(inspect.signature(Renderer.render_panorama).parameters)[1:] == ["spp", "basis"] and inspect.signature(Renderer.render_panorama).parameters["basis"].default is None
    assert isinstance(Renderer.panorama, property)
    for name in ("panorama_face_camera", "capture_panorama_face", "camera_basis"):
        assert callable(getattr(Renderer, name))
    init = inspect.signature(EarthViewer.__init__).parameters
    assert init["panorama"].default is None and list(init).index("panorama") > list(init).index("exr_aovs") and init["renderer_kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    assert list(inspect.signature(EarthViewer.frame).parameters)[1:] == ["spp", "copy", "pipelined", "pixels", "sliders"]      # panorama travels beside the sliders
    assert "panorama" in inspect.getsource(EarthViewer.frame)


def test_every_refusal_of_the_settings_answers_before_the_context_is_read():
    """de_debug_panorama checks its arguments and the settings — de_set_panorama's own check, against the faces' size — before it reads the context:
    the refusals are held without a GPU.  (Those that need a context's state are tests/test_gpu_panorama.py's.)"""
    lib = _lib()
    fn = lib.de_debug_panorama
    fn.restype, fn.argtypes = _native.DEBUG_SYMBOLS["de_debug_panorama"]
    ctx = ctypes.c_void_p(1)      # never dereferenced by a refused call, only checked for NULL
    faces, out = np.zeros((6, 16, 16, 3), np.float32), np.full((64, 32, 3), 7.0, np.float32)

    def settings(**kw):
        s = _native.DePanorama()
        s.struct_bytes, s.on, s.projection, s.width, s.height, s.aperture_deg, s.apron, s.supersample = ctypes.sizeof(s), 1, 0, 64, 32, 180.0, 1, 2
        basis = kw.pop("basis", np.eye(3))
        for k in range(9):
            s.basis[k] = float(np.asarray(basis).reshape(9)[k])
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    skew = np.eye(3); skew[0, 1] = 2e-4
    long_ = np.eye(3); long_[2, 2] = 1.0002
    bad = (dict(struct_bytes=64), dict(struct_bytes=72), dict(projection=2), dict(projection=-1), dict(width=40), dict(height=12), dict(width=0), dict(height=-8),
           dict(width=1 << 15, height=1 << 14), dict(projection=1), dict(projection=1, width=32, height=32, aperture_deg=0.0),
           dict(projection=1, width=32, height=32, aperture_deg=360.5), dict(projection=1, width=32, height=32, aperture_deg=float("nan")),
           dict(apron=0), dict(apron=5), dict(supersample=0), dict(supersample=5), dict(basis=skew), dict(basis=long_), dict(basis=np.zeros((3, 3))),
           dict(basis=np.full((3, 3), np.nan)))
    for kw in bad:
        assert fn(ctx, faces.ctypes.data, 16, ctypes.byref(settings(**kw)), out.ctypes.data) == _native.DE_ERR_INVALID, kw
    assert fn(ctx, faces.ctypes.data, 3, ctypes.byref(settings()), out.ctypes.data) == _native.DE_ERR_INVALID      # faces below 4 pixels a side
    assert fn(ctx, None, 16, ctypes.byref(settings()), out.ctypes.data) == _native.DE_ERR_INVALID
    assert fn(None, faces.ctypes.data, 16, ctypes.byref(settings()), out.ctypes.data) == _native.DE_ERR_INVALID
    assert fn(ctx, faces.ctypes.data, 16, None, out.ctypes.data) == _native.DE_ERR_INVALID
    assert (out == 7.0).all()                                      # a refused call changes nothing
    near = np.eye(3); near[0, 1] = 5e-5                            # inside the tolerance: not refused by the check (the next line would reach the device)
    import panorama_ref
    assert np.isfinite(panorama_ref.consts(16, 1, 180.0, near)[3]).all()


def test_build_tracks_the_new_sources():
    from digital_earth_amd import build
    assert "panorama_kernels.hip" in build.DEPS and "panorama_body.h" in build.DEPS
    assert any(d.endswith(H) for d in build.DEPS)
    ctx = open(os.path.join(build.CSRC, "de_context.h")).read()
    assert ctx.index('#include "panorama_kernels.hip"') > ctx.index('#include "output_scale_kernels.hip"')      # in the product library's one translation unit
    body = open(os.path.join(build.CSRC, "panorama_body.h")).read()
    assert "hip" not in body.split("#pragma once")[1]              # the per-pixel body needs nothing of the device
    assert os.path.exists(os.path.join(ROOT, "tools", "panorama_host_check.cpp"))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no C++ compiler")
def test_the_host_build_of_the_body_equals_the_restatement(tmp_path):
    """tools/panorama_host_check.cpp WITHOUT the sanitizers (tools/panorama_host_check.py runs it with them): the body the kernel runs, built for the
    host, equals the restatement bit for bit on one case per projection."""
    import panorama_ref as ref
    exe = str(tmp_path / "host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fno-fast-math", os.path.join(ROOT, "tools", "panorama_host_check.cpp"), "-o", exe])
    F = np.float32
    faces = np.random.default_rng(3).random((6, 16, 16, 3), dtype=F)
    for size, projection, aperture, S in (((48, 24), "equirect", 180.0, 3), ((32, 32), "fisheye", 360.0, 2)):
        fov, scale, half, m = ref.consts(16, 4, aperture, None)
        tabs = ref.tables(size[0], S, 2.0 * np.pi) + ref.tables(size[1], S, np.pi)
        with open(str(tmp_path / "in.bin"), "wb") as fh:
            fh.write(np.array([16, size[0], size[1], S, int(projection == "fisheye")], np.int32).tobytes())
            fh.write(np.array([fov, scale, half], F).tobytes() + np.ascontiguousarray(m, F).tobytes())
            for t in tabs:
                fh.write(np.ascontiguousarray(t, F).tobytes())
            fh.write(faces.tobytes())
        subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
        got = np.fromfile(str(tmp_path / "out.bin"), F).reshape(size[0], size[1], 3)
        want = ref.panorama(faces, size, projection, aperture, 4, S)
        assert (got.view(np.uint32) == want.view(np.uint32)).all(), (size, projection)
