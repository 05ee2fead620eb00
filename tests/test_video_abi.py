"""The video-output C ABI without a GPU: include/digital_earth_video.h compiles as pedantic C99, the struct mirror matches field by field, every entry
point it declares is bound and exported, its table is disjoint from every other, the enums have their values, the Python signatures have the documented
defaults, and the build tracks the new sources."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

from digital_earth_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"de_set_video", "de_get_video", "de_videoframe_bytes", "de_render_to_video", "de_fetch_video", "de_fetch_videoframe_view", "de_fetch_videoframe_begin",
         "de_fetch_videoframe_end", "de_debug_video"}
CTYPE = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "float": ctypes.c_float}


def _header(name="digital_earth_video.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name="digital_earth_video.h"):
    text = re.sub(r"/\*.*?\*/", "", _header(name), flags=re.S)
    return set(re.findall(r"\b(de_[a-z0-9_]+)\s*\(", text))


def _fields(struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        m = re.match(r"\s*(uint32_t|int32_t|float)\s+(.+?)\s*$", decl.strip(), re.S)
        if not m:
            assert not decl.strip(), decl
            continue
        for item in m.group(2).split(","):
            out.append((re.match(r"\s*(\w+)\s*$", item).group(1), CTYPE[m.group(1)]))
    return out


def test_video_struct_and_enums_match_header():
    want = _fields("de_video")
    assert [n for n, _ in want] == ["struct_bytes", "format", "matrix", "range", "siting", "mode", "seed", "animate"]
    assert [n for n, _ in _native.DeVideo._fields_] == [n for n, _ in want]
    for (n, a), (_, b) in zip(_native.DeVideo._fields_, want):
        assert a is b, n
    assert ctypes.sizeof(_native.DeVideo) == 32
    for i, (n, _) in enumerate(_native.DeVideo._fields_):
        assert getattr(_native.DeVideo, n).offset == 4 * i
    enums = dict(re.findall(r"#define\s+DE_VIDEO_(\w+)\s+(\d+)", _header()))
    assert enums == {"NV12": "0", "I420": "1", "P010": "2", "I010": "3", "MATRIX_BT709": "0", "MATRIX_BT601": "1", "MATRIX_BT2020": "2",
                     "RANGE_LIMITED": "0", "RANGE_FULL": "1", "SITING_LEFT": "0", "SITING_CENTER": "1", "SITING_TOPLEFT": "2"}
    from digital_earth_amd.renderer import Renderer
    assert Renderer.VIDEO_FORMATS == ("nv12", "i420", "p010", "i010") and Renderer.VIDEO_MATRICES == ("bt709", "bt601", "bt2020")
    assert Renderer.VIDEO_RANGES == ("limited", "full") and Renderer.VIDEO_SITINGS == ("left", "center", "topleft")


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_video_header_compiles_as_pedantic_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "digital_earth_video.h"\n#include "digital_earth_debug.h"\n'
                   'int main(void) { de_video p; p.struct_bytes = sizeof p; (void)de_debug_video; return p.struct_bytes != 32 || DE_VIDEO_I010 != 3 || DE_PIXELS_ROUND != 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_video_symbols_declared_bound_and_exported():
    assert _declared() == set(_native.VIDEO_SYMBOLS) == NAMES
    others = (set(_native.SYMBOLS) | set(_native.DEBUG_SYMBOLS) | set(_native.DENOISE_SYMBOLS) | set(_native.EXPOSURE_SYMBOLS) | set(_native.BLOOM_SYMBOLS)
              | set(_native.HISTORY_SYMBOLS) | set(_native.PIXELS_SYMBOLS) | set(_native.LOCAL_EXPOSURE_SYMBOLS) | set(_native.OUTPUT_SCALE_SYMBOLS)
              | set(_native.HDR_OUTPUT_SYMBOLS) | set(_native.LEGACY_SYMBOLS))
    assert not NAMES & others
    assert len(_declared("digital_earth.h")) == 40 and not NAMES & _declared("digital_earth.h")
    assert re.search(r"#define\s+DE_ABI_VERSION\s+6\b", _header("digital_earth.h"))
    V, P, u8pp = _native.VIDEO_SYMBOLS, ctypes.c_void_p, ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8))
    assert all(res is ctypes.c_int for res, _ in V.values())
    assert V["de_set_video"][1][0] is P and V["de_set_video"][1][1]._type_ is _native.DeVideo and len(V["de_set_video"][1]) == 2
    assert V["de_get_video"][1][1]._type_ is _native.DeVideo and V["de_get_video"][1][2]._type_ is ctypes.c_uint32 and len(V["de_get_video"][1]) == 3
    assert [a._type_ for a in V["de_videoframe_bytes"][1][1:]] == [ctypes.c_uint64] * 3
    assert V["de_render_to_video"][1] == [P, ctypes.POINTER(ctypes.c_void_p)]
    assert V["de_fetch_video"][1] == [P, P, ctypes.c_uint64]
    assert V["de_fetch_videoframe_view"][1] == [P, u8pp] and V["de_fetch_videoframe_end"][1] == [P, u8pp] and V["de_fetch_videoframe_begin"][1] == [P]
    args = V["de_debug_video"][1]
    assert len(args) == 7 and args[2] is ctypes.c_int and args[3] is ctypes.c_int and args[4]._type_ is _native.DeVideo and args[5] is ctypes.c_uint32
    assert "VIDEO_SYMBOLS" in inspect.getsource(_native.load)
    from digital_earth_amd import build
    build.build()
    lib = ctypes.CDLL(build.OUT)
    for name in NAMES:
        assert hasattr(lib, name), name
    lib.de_abi_version.restype = ctypes.c_int
    assert lib.de_abi_version() == 6 == _native.ABI_VERSION


def test_video_python_api_without_a_device():
    from digital_earth_amd.renderer import Renderer
    from digital_earth_amd.earth_viewer import EarthViewer
    import video_ref
    sig = inspect.signature(Renderer.set_video).parameters
    assert list(sig)[1:] == ["format", "matrix", "range", "siting", "mode", "seed", "animate"]
    assert {k: v.default for k, v in sig.items() if k != "self"} == video_ref.DEFAULTS
    sig = inspect.signature(Renderer.fetch_video).parameters
    assert list(sig)[1:] == ["copy", "lag"] and sig["copy"].default is True and sig["lag"].default == 0
    for name in ("video", "split_video", "render_to_video", "debug_video"):
        assert callable(getattr(Renderer, name))
    sig = inspect.signature(Renderer.fetch_pending).parameters      # the earlier keywords keep their places and defaults
    assert list(sig)[1:4] == ["copy", "all_images", "pixels"] and sig["pixels"].default is False and sig["video"].default is False
    sig = inspect.signature(EarthViewer.frame).parameters           # video travels beside the sliders, like hdr_pixels: the signature is unchanged
    assert list(sig)[1:] == ["spp", "copy", "pipelined", "pixels", "sliders"]
    sig = inspect.signature(EarthViewer.record).parameters
    assert list(sig)[1:] == ["path", "frames", "spp", "fps", "sliders_per_frame"] and sig["sliders_per_frame"].kind is inspect.Parameter.VAR_KEYWORD
    assert (video_ref.FORMATS, video_ref.MATRICES, video_ref.RANGES, video_ref.SITINGS) == (Renderer.VIDEO_FORMATS, Renderer.VIDEO_MATRICES, Renderer.VIDEO_RANGES, Renderer.VIDEO_SITINGS)


def test_build_tracks_the_new_sources():
    from digital_earth_amd import build
    assert "videoframe_kernels.hip" in build.DEPS
    assert any(d.endswith("digital_earth_video.h") for d in build.DEPS)
    ctx = open(os.path.join(build.CSRC, "de_context.h")).read()
    assert ctx.index('#include "videoframe_kernels.hip"') > ctx.index('#include "pixels_kernels.hip"')      # in the product library's one translation unit: it uses the pixel pack's hash
    kernel = open(os.path.join(build.CSRC, "videoframe_kernels.hip")).read()
    assert "DE_VIDEO_STANDALONE" in kernel and os.path.exists(os.path.join(ROOT, "tools", "video_host_check.cpp"))
