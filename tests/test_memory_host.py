"""The one owner of a context's memory (csrc/de_memory.h: Dev<T>, Pinned<T>) on the host: tools/memory_host_check.cpp, a stand-alone program that includes
that header alone over counting stand-ins for the four HIP allocation calls, built with the host compiler under the address and undefined-behaviour
sanitizers.  And the source statement that goes with it: nothing else under csrc/ allocates or frees.  Needs no GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "digital_earth_amd", "csrc")


def _cxx():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    raise AssertionError("no host C++ compiler found (the library's own build needs one too)")


def test_owner_type_frees_each_block_once(tmp_path):
    exe = str(tmp_path / "memory_host_check")
    subprocess.check_call([_cxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "memory_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    assert "no sanitizer report" in out.stdout and "0 alive at exit" in out.stdout, out.stdout


def test_the_library_allocates_through_the_type_the_program_checks():
    """One statement: outside de_memory.h no file under csrc/ (legacy/ included) calls the four allocation functions, and de_destroy keeps no list of
    buffers: the members free themselves."""
    seen = 0
    for folder, _, names in os.walk(CSRC):
        for name in names:
            if name == "de_memory.h":
                continue
            text = open(os.path.join(folder, name), encoding="utf-8").read()
            seen += 1
            for call in ("hipMalloc(", "hipFree(", "hipHostMalloc(", "hipHostFree("):
                assert call not in text, (name, call)
    assert seen >= 30      # the walk saw the sources (csrc/ holds 34 files besides de_memory.h)
    owner = open(os.path.join(CSRC, "de_memory.h")).read()
    for call in ("hipMalloc(", "hipFree(", "hipHostMalloc(", "hipHostFree("):
        assert owner.count(call) == 1, call
    assert "de_ctx" not in owner      # the type knows nothing of the context: the stand-alone program includes the header as it is
    api = open(os.path.join(CSRC, "de_api.hip")).read()
    assert "ptrs[]" not in api and "legacy_destroy" not in api
    assert '"de_memory.h"' in open(os.path.join(ROOT, "digital_earth_amd", "build.py")).read()      # a change of the header rebuilds the library
