"""What the packed outputs share is stated once (csrc/pack.h): the dither's hash lives in one file under csrc/, and every pack includes
that file.  No GPU: the sources are read, as the *_abi.py tests read them."""
import os
import re

from digital_earth_amd import build


def _sources():
    for root, _, names in os.walk(build.CSRC):
        for name in names:
            yield os.path.join(root, name)


def test_the_hash_is_stated_in_exactly_one_file():
    holders = [os.path.relpath(p, build.CSRC) for p in _sources() if "0x7feb352d" in open(p, errors="replace").read().lower()]
    assert holders == ["pack.h"]
    assert "pack.h" in build.DEPS and "hdr_pack.h" in build.DEPS      # a change to either rebuilds the library


def test_every_pack_includes_it():
    for name in ("pixels_kernels.hip", "hdr_pack.h", "videoframe_kernels.hip"):
        assert re.search(r'^#include "pack\.h"', open(os.path.join(build.CSRC, name)).read(), re.M), name
    # the HDR pack's halves are a file of their own, which the kernel's file includes
    hdr = open(os.path.join(build.CSRC, "hdr_output_kernels.hip")).read()
    assert re.search(r'^#include "hdr_pack\.h"', hdr, re.M) and "hdr_pack_kernel" in hdr
