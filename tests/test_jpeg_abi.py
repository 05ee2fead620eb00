"""The JPEG-output C ABI without a GPU: include/digital_earth_jpeg.h compiles as pedantic C99, the struct mirror matches, every entry point it declares
is bound and exported, its table is disjoint from every other, the Python signatures have the documented defaults, the build tracks the new sources —
and the host's part of the encoder (de_debug_jpeg_framing needs no device): every refusal of the settings, the framing byte for byte the reference's,
and a capacity that bounds the reference's longest stream.  (The two DE_ERR_STATE refusals need a context: tests/test_gpu_jpeg.py.)"""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

import jpeg_cases as jc
import jpeg_ref as jr
from digital_earth_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"de_set_jpeg", "de_get_jpeg", "de_jpeg_capacity", "de_render_to_jpeg", "de_fetch_jpeg", "de_fetch_jpeg_view", "de_fetch_jpeg_begin",
         "de_fetch_jpeg_end", "de_debug_jpeg", "de_debug_jpeg_framing"}
ERR_INVALID = -1


def _header(name="digital_earth_jpeg.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name="digital_earth_jpeg.h"):
    text = re.sub(r"/\*.*?\*/", "", _header(name), flags=re.S)
    return set(re.findall(r"\b(de_[a-z0-9_]+)\s*\(", text))


@pytest.fixture(scope="module")
def lib():
    from digital_earth_amd import build
    build.build()
    L = ctypes.CDLL(build.OUT)
    L.de_debug_jpeg_framing.restype, L.de_debug_jpeg_framing.argtypes = _native.JPEG_SYMBOLS["de_debug_jpeg_framing"]
    L.de_last_error.restype = ctypes.c_char_p
    return L


def _settings(quality=90, restart=8, struct_bytes=None):
    s = _native.DeJpeg()
    s.struct_bytes = ctypes.sizeof(_native.DeJpeg) if struct_bytes is None else struct_bytes
    s.quality, s.restart_mcus = quality, restart
    return s


def test_struct_defaults_and_header():
    body = re.search(r"typedef struct de_jpeg \{(.*?)\} de_jpeg;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(m.group(2), m.group(1)) for m in re.finditer(r"(uint32_t|int32_t)\s+(\w+)\s*;", body)]
    assert fields == [("struct_bytes", "uint32_t"), ("quality", "int32_t"), ("restart_mcus", "int32_t")]
    assert [n for n, _ in _native.DeJpeg._fields_] == [n for n, _ in fields]
    assert [t for _, t in _native.DeJpeg._fields_] == [ctypes.c_uint32, ctypes.c_int32, ctypes.c_int32] and ctypes.sizeof(_native.DeJpeg) == 12
    default = int(re.search(r"#define\s+DE_JPEG_DEFAULT_RESTART\s+(\d+)", _header()).group(1))
    assert default == _native.JPEG_DEFAULT_RESTART == jr.DEFAULT_RESTART and default in (1, 2, 4, 8, 16)
    assert re.search(r"#define\s+DE_ERR_INTERNAL\s+\(-6\)", _header()) and _native.DE_ERR_INTERNAL == -6
    ctx = open(os.path.join(ROOT, "digital_earth_amd", "csrc", "de_context.h")).read()
    assert "de_jpeg jp = {(uint32_t)sizeof(de_jpeg), 90, DE_JPEG_DEFAULT_RESTART};" in ctx      # what de_get_jpeg answers before any de_set_jpeg
    assert "profiles/jpeg.md" in _header()                                                      # the header says where the default was measured
    from digital_earth_amd.renderer import Renderer
    from digital_earth_amd.earth_viewer import EarthViewer
    sig = inspect.signature(Renderer.set_jpeg).parameters
    assert list(sig)[1:] == ["quality", "restart"] and {k: v.default for k, v in sig.items() if k != "self"} == jr.DEFAULTS
    sig = inspect.signature(Renderer.fetch_jpeg).parameters
    assert list(sig)[1:] == ["copy", "lag"] and sig["copy"].default is True and sig["lag"].default == 0
    for name in ("jpeg", "render_to_jpeg", "debug_jpeg"):
        assert callable(getattr(Renderer, name))
    assert list(inspect.signature(Renderer.fetch_pending).parameters)[1:] == ["copy", "all_images", "pixels", "video"]      # pinned: the JPEG ring ends in a method of its own
    sig = inspect.signature(Renderer.fetch_pending_jpeg).parameters
    assert list(sig)[1:] == ["copy", "all_images"] and sig["copy"].default is True and sig["all_images"].default is False
    assert list(inspect.signature(EarthViewer.frame).parameters)[1:] == ["spp", "copy", "pipelined", "pixels", "sliders"]      # jpeg travels beside the sliders
    assert list(inspect.signature(EarthViewer.finish).parameters)[1:] == ["copy", "pixels", "video", "jpeg"]


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_header_compiles_as_pedantic_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "digital_earth_jpeg.h"\n'
                   'int main(void) { de_jpeg p; p.struct_bytes = sizeof p; (void)de_debug_jpeg; return p.struct_bytes != 12 || DE_ERR_INTERNAL != -6; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_symbols_declared_bound_and_exported(lib):
    assert _declared() == set(_native.JPEG_SYMBOLS) == NAMES
    others = (set(_native.SYMBOLS) | set(_native.DEBUG_SYMBOLS) | set(_native.DENOISE_SYMBOLS) | set(_native.EXPOSURE_SYMBOLS) | set(_native.BLOOM_SYMBOLS)
              | set(_native.HISTORY_SYMBOLS) | set(_native.PIXELS_SYMBOLS) | set(_native.LOCAL_EXPOSURE_SYMBOLS) | set(_native.OUTPUT_SCALE_SYMBOLS)
              | set(_native.HDR_OUTPUT_SYMBOLS) | set(_native.VIDEO_SYMBOLS) | set(_native.LOOK_SYMBOLS) | set(_native.LEGACY_SYMBOLS))
    assert not NAMES & others
    assert len(_declared("digital_earth.h")) == 40 and not NAMES & _declared("digital_earth.h")
    assert re.search(r"#define\s+DE_ABI_VERSION\s+6\b", _header("digital_earth.h"))
    J, P, u64p = _native.JPEG_SYMBOLS, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)
    assert all(res is ctypes.c_int for res, _ in J.values())
    assert J["de_set_jpeg"][1][1]._type_ is _native.DeJpeg and J["de_get_jpeg"][1][1]._type_ is _native.DeJpeg
    assert J["de_fetch_jpeg"][1] == [P, P, ctypes.c_uint64, u64p] and J["de_fetch_jpeg_begin"][1] == [P]
    assert J["de_fetch_jpeg_view"][1][2] is u64p and J["de_fetch_jpeg_end"][1][2] is u64p and len(J["de_debug_jpeg"][1]) == 8
    assert "JPEG_SYMBOLS" in inspect.getsource(_native.load)
    for name in NAMES:
        assert hasattr(lib, name), name
    lib.de_abi_version.restype = ctypes.c_int
    assert lib.de_abi_version() == 6 == _native.ABI_VERSION


def test_build_tracks_the_new_sources():
    from digital_earth_amd import build
    assert "jpeg_kernels.hip" in build.DEPS and "jpeg_tables.h" in build.DEPS
    assert any(d.endswith("digital_earth_jpeg.h") for d in build.DEPS)
    ctx = open(os.path.join(build.CSRC, "de_context.h")).read()
    assert ctx.index('#include "jpeg_kernels.hip"') > ctx.index('#include "videoframe_kernels.hip"')      # it packs its planes with that kernel
    kernel = open(os.path.join(build.CSRC, "jpeg_kernels.hip")).read()
    assert "DE_JPEG_STANDALONE" in kernel and os.path.exists(os.path.join(ROOT, "tools", "jpeg_host_check.cpp"))
    assert "asm" not in kernel and "atomic" not in kernel.split("#ifndef DE_JPEG_STANDALONE")[1]
    video = open(os.path.join(build.CSRC, "videoframe_kernels.hip")).read()
    assert "jpeg" not in video.lower()                                                                   # reused unchanged


def test_every_refusal_of_the_settings(lib):
    n, cap = ctypes.c_uint64(77), ctypes.c_uint64(77)
    buf = ctypes.create_string_buffer(b"\xA5" * 1024, 1024)

    def call(s, W=64, H=32, out=buf, out_bytes=1024):
        return lib.de_debug_jpeg_framing(ctypes.byref(s) if s is not None else None, W, H, out, out_bytes, ctypes.byref(n), ctypes.byref(cap))
    assert call(_settings()) == 0 and n.value == jr.FRAMING_BYTES
    for bad in (_settings(quality=0), _settings(quality=101), _settings(quality=-5), _settings(restart=0), _settings(restart=65536), _settings(restart=-1),
                _settings(struct_bytes=8), _settings(struct_bytes=16)):
        buf.raw = b"\xA5" * 1024
        assert call(bad) == ERR_INVALID and lib.de_last_error()
        assert buf.raw == b"\xA5" * 1024                         # a refused call writes nothing
    assert call(None) == ERR_INVALID
    for W, H in ((63, 32), (64, 31), (0, 32), (64, -2)):         # an odd or empty size
        assert call(_settings(), W, H) == ERR_INVALID
    buf.raw = b"\xA5" * 1024
    assert call(_settings(), out_bytes=jr.FRAMING_BYTES - 1) == ERR_INVALID and buf.raw == b"\xA5" * 1024 and n.value == jr.FRAMING_BYTES      # *len is set either way
    assert call(_settings(quality=1, restart=1)) == 0 and call(_settings(quality=100, restart=65535)) == 0      # the ends of both ranges


def test_framing_equals_the_reference_and_capacity_bounds_it(lib):
    n, cap = ctypes.c_uint64(), ctypes.c_uint64()
    buf = ctypes.create_string_buffer(1024)
    for quality in (1, 25, 49, 50, 51, 75, 90, 100):
        for (W, H, restart) in jc.SIZES + [(1920, 1080, 8), (1920, 1080, 120)]:
            assert lib.de_debug_jpeg_framing(ctypes.byref(_settings(quality, restart)), W, H, buf, 1024, ctypes.byref(n), ctypes.byref(cap)) == 0
            assert buf.raw[:n.value] == jr.framing(W, H, quality, restart), (quality, W, H, restart)
            assert cap.value == jr.capacity(W, H, restart)
    longest = 0
    for (W, H, restart) in jc.SIZES:
        assert lib.de_debug_jpeg_framing(ctypes.byref(_settings(100, restart)), W, H, None, 0, None, ctypes.byref(cap)) == 0
        for name in jc.INPUTS:
            data = jc.reference(name, W, H, restart)[0]
            longest = max(longest, len(data))
            assert cap.value >= len(data)
    assert longest > 4000                                        # noise at quality 100 was among them
