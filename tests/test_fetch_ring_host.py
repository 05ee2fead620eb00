"""The ring arithmetic of the lagged fetches (the top of csrc/de_fetch.h: the counters, the cell index, refuse-the-fifth and refuse-when-empty) on the
host: tools/fetch_ring_host_check.cpp, a stand-alone program that includes that part of the header alone, built with the host compiler under the address
and undefined-behaviour sanitizers.  It walks every legal interleaving of begins and ends across the wrap of the 32-bit counters.  Needs no GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cxx():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    raise AssertionError("no host C++ compiler found (the library's own build needs one too)")


def test_ring_arithmetic_across_the_counter_wrap(tmp_path):
    exe = str(tmp_path / "fetch_ring_host_check")
    subprocess.check_call([_cxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "fetch_ring_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    assert "no sanitizer report" in out.stdout and "interleavings" in out.stdout, out.stdout


def test_the_library_uses_the_arithmetic_the_program_checks():
    """One statement: the ring's begin and end go through the four functions, and nothing else in the host code forms a cell index or compares the counters."""
    src = open(os.path.join(ROOT, "digital_earth_amd", "csrc", "de_fetch.h")).read()
    head, body = src.split("#ifndef DE_FETCH_STANDALONE")
    for fn in ("ring_in_flight", "ring_full", "ring_empty", "ring_cell"):
        assert ("inline" in head and fn + "(" in head) and fn + "(" in body, fn
    assert "hip" not in head.split("#pragma once")[1].lower().replace("no hip", "")      # the checked part makes no HIP call
    ctx = open(os.path.join(ROOT, "digital_earth_amd", "csrc", "de_context.h")).read()
    assert "#define DE_FETCH_RING 4" in ctx      # the program's DEPTH
    for name in ("de_api.hip", "de_display.h", "de_launch.h"):
        text = open(os.path.join(ROOT, "digital_earth_amd", "csrc", name)).read()
        assert ".begun" not in text and ".ended" not in text and "% (unsigned)DE_FETCH_RING" not in text, name
