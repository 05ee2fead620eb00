"""The output-scaling C ABI without a GPU: include/digital_earth_output_scale.h compiles as pedantic C99 together with the debug header in either order,
the struct mirror matches field by field, every entry point it declares is bound and exported, the binder's header keeps its 40 entry points at ABI 6,
the Python signatures have the documented defaults, and the build tracks the new sources."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

from digital_earth_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"de_set_output_scale", "de_get_output_scale", "de_output_size"}
DEBUG_NAMES = {"de_debug_output_scale", "de_debug_output_scale_weights"}
CTYPE = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "float": ctypes.c_float}


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", _header(name), flags=re.S)
    return set(re.findall(r"\b(de_[a-z0-9_]+)\s*\(", text))


def _fields(struct):
    """[(name, ctype)] of a struct of the header: `type a, b;` declarations."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _header("digital_earth_output_scale.h"), re.S).group(1)
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


def test_output_scale_struct_matches_header():
    want = _fields("de_output_scale")
    assert [n for n, _ in want] == ["struct_bytes", "enabled", "width", "height", "filter"]
    assert [n for n, _ in _native.DeOutputScale._fields_] == [n for n, _ in want]
    for (n, a), (_, b) in zip(_native.DeOutputScale._fields_, want):
        assert a is b, n
    assert ctypes.sizeof(_native.DeOutputScale) == 20
    filters = dict(re.findall(r"#define\s+DE_SCALE_(\w+)\s+(\d+)", _header("digital_earth_output_scale.h")))
    assert filters == {"BOX": "0", "TRIANGLE": "1", "MITCHELL": "2", "LANCZOS3": "3"}


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_output_scale_header_compiles_as_pedantic_c99(tmp_path):
    for first, second in (("digital_earth_output_scale.h", "digital_earth_debug.h"), ("digital_earth_debug.h", "digital_earth_output_scale.h")):
        src = tmp_path / "t.c"
        src.write_text('#include "%s"\n#include "%s"\n' % (first, second) +
                       'int main(void) { de_output_scale s; s.struct_bytes = sizeof s; (void)de_debug_output_scale; (void)de_debug_output_scale_weights;'
                       ' return s.struct_bytes != 20 || DE_SCALE_LANCZOS3 != 3; }\n')
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    src.write_text('#include "digital_earth_output_scale.h"\nint main(void) { de_output_scale s; s.struct_bytes = sizeof s; return s.struct_bytes != 20; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


def test_output_scale_symbols_declared_bound_and_exported():
    assert _declared("digital_earth_output_scale.h") == set(_native.OUTPUT_SCALE_SYMBOLS) == NAMES
    assert not set(_native.OUTPUT_SCALE_SYMBOLS) & (set(_native.SYMBOLS) | set(_native.DEBUG_SYMBOLS) | set(_native.DENOISE_SYMBOLS) | set(_native.EXPOSURE_SYMBOLS)
                                                    | set(_native.BLOOM_SYMBOLS) | set(_native.HISTORY_SYMBOLS) | set(_native.PIXELS_SYMBOLS)
                                                    | set(_native.LOCAL_EXPOSURE_SYMBOLS) | set(_native.LEGACY_SYMBOLS))
    assert len(_declared("digital_earth.h")) == 40 and not (NAMES | DEBUG_NAMES) & _declared("digital_earth.h")
    assert re.search(r"#define\s+DE_ABI_VERSION\s+6\b", _header("digital_earth.h"))
    for name in ("de_set_output_scale", "de_get_output_scale"):
        res, args = _native.OUTPUT_SCALE_SYMBOLS[name]
        assert res is ctypes.c_int and len(args) == 2 and args[1]._type_ is _native.DeOutputScale
    res, args = _native.OUTPUT_SCALE_SYMBOLS["de_output_size"]
    assert res is ctypes.c_int and len(args) == 3 and args[1]._type_ is ctypes.c_int and args[2]._type_ is ctypes.c_int
    assert DEBUG_NAMES <= _declared("digital_earth_debug.h") and DEBUG_NAMES <= set(_native.DEBUG_SYMBOLS)
    res, args = _native.DEBUG_SYMBOLS["de_debug_output_scale"]
    assert res is ctypes.c_int and len(args) == 6 and args[2] is ctypes.c_int and args[3] is ctypes.c_int and args[4]._type_ is _native.DeOutputScale
    res, args = _native.DEBUG_SYMBOLS["de_debug_output_scale_weights"]
    assert res is ctypes.c_int and len(args) == 7 and args[1:4] == [ctypes.c_int] * 3 and args[6]._type_ is ctypes.c_int
    assert "OUTPUT_SCALE_SYMBOLS" in inspect.getsource(_native.load)
    from digital_earth_amd import build
    build.build()
    lib = ctypes.CDLL(build.OUT)
    for name in NAMES | DEBUG_NAMES:
        assert hasattr(lib, name), name
    lib.de_abi_version.restype = ctypes.c_int
    assert lib.de_abi_version() == 6 == _native.ABI_VERSION


def test_output_scale_python_api_without_a_device():
    from digital_earth_amd.renderer import Renderer
    from digital_earth_amd.earth_viewer import EarthViewer
    import output_scale_ref
    sig = inspect.signature(Renderer.set_output_scale).parameters
    assert list(sig)[1:] == ["size", "filter", "on"]
    assert sig["size"].default is None and sig["filter"].default == "lanczos3" and sig["on"].default is True
    assert output_scale_ref.DEFAULTS == {k: v.default for k, v in sig.items() if k != "self"}
    assert Renderer.SCALE_FILTERS == ("box", "triangle", "mitchell", "lanczos3") == output_scale_ref.FILTERS
    sig = inspect.signature(Renderer.debug_output_scale).parameters
    assert list(sig)[1:] == ["image", "size", "filter"] and sig["filter"].default == "lanczos3"
    assert list(inspect.signature(Renderer.debug_output_scale_weights).parameters)[1:] == ["n_src", "n_dst", "filter"]
    for name in ("output_scale", "output_size"):
        assert callable(getattr(Renderer, name))
    init = inspect.signature(EarthViewer.__init__).parameters
    assert init["output_res"].default is None and init["output_filter"].default == "lanczos3"
    assert list(init).index("output_res") > list(init).index("local_exposure") and init["renderer_kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    # the calls that hand out the displayed image size themselves from output_size(), not from image_res
    for fn in (Renderer.fetch_image, Renderer._staging_view, Renderer.fetch_pixels, Renderer._pixel_view):
        src = inspect.getsource(fn)
        assert "image_res" not in src.split('"""')[-1] and ("output_size()" in src or "_staging_view" in src or "_pixel_view" in src), fn.__name__


def test_the_weights_entry_point_needs_no_device():
    """de_debug_output_scale_weights builds its table on the host: the library's tables can be held to the restatement's without a GPU.  Where both run
    on one libm they are the same bits."""
    import numpy as np
    import output_scale_ref as ref
    from digital_earth_amd import build
    build.build()
    lib = ctypes.CDLL(build.OUT)
    fn = lib.de_debug_output_scale_weights
    fn.restype, fn.argtypes = _native.DEBUG_SYMBOLS["de_debug_output_scale_weights"]
    ctx = ctypes.c_void_p(1)      # never dereferenced by this entry point, only checked for NULL
    for n_src, n_dst in ((40, 24), (8, 32), (64, 8), (120, 72)):
        for f, name in enumerate(ref.FILTERS):
            taps = ctypes.c_int()
            assert fn(ctx, n_src, n_dst, f, None, None, ctypes.byref(taps)) == 0
            first, w = np.empty(n_dst, np.int32), np.empty((n_dst, taps.value), np.float32)
            assert fn(ctx, n_src, n_dst, f, first.ctypes.data, w.ctypes.data, ctypes.byref(taps)) == 0
            want_first, want_w = ref.weights(n_src, n_dst, name)
            assert (first == want_first).all() and w.shape == want_w.shape
            assert (ref.row_sums(w) == np.float32(1.0)).all()
            assert np.abs(w.astype(np.float64) - want_w).max() <= taps.value * np.spacing(np.float32(1.0))
    assert fn(ctx, 8, 72, 0, None, None, ctypes.byref(taps)) == _native.DE_ERR_INVALID
    assert fn(None, 8, 32, 0, None, None, ctypes.byref(taps)) == _native.DE_ERR_INVALID


def test_build_tracks_the_new_sources():
    from digital_earth_amd import build
    assert "output_scale_kernels.hip" in build.DEPS
    assert any(d.endswith("digital_earth_output_scale.h") for d in build.DEPS)
    ctx = open(os.path.join(build.CSRC, "de_context.h")).read()
    assert ctx.index('#include "output_scale_kernels.hip"') > ctx.index('#include "pixels_kernels.hip"')      # in the product library's one translation unit, after the pack kernel
    assert "#ifndef DE_OUTPUT_SCALE_STANDALONE" in open(os.path.join(build.CSRC, "output_scale_kernels.hip")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "output_scale_host_check.cpp"))
