"""The queue logic of dg_search_batched, without a GPU.

tests/host/batch_core_test.cpp drives dingo-store_amd/csrc/dg_batch_core.h
with a fake flush: 32 threads, thousands of calls with mixed k and mixed
compatibility keys, calls at max_batch that bypass, one injected flush
failure that only its members may see, disable under traffic, and every
caller must receive exactly its own rows.  This test compiles the program
plain and runs it; tests/host/Makefile also builds it with
-fsanitize=thread and -fsanitize=address,undefined as stand-alone binaries.
The header-symbol test for the new entry points is
test_abi_cpu.py::test_all_header_symbols_exported.
"""
import os
import re
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "batch_core_test.cpp")
CORE = os.path.join(REPO, "dingo-store_amd", "csrc", "dg_batch_core.h")


def _cxx():
    for c in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        p = shutil.which(c)
        if p:
            return p
    raise AssertionError("no C++ compiler found")


def test_batch_core_program(tmp_path):
    exe = str(tmp_path / "batch_core_test")
    r = subprocess.run(
        [_cxx(), "-std=c++17", "-O2", "-Wall", "-pthread", SRC, "-o", exe],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("OK"), r.stdout[-2000:]
    # batches did form and the failure was injected
    m = re.search(r"phase A: (\d+) calls, (\d+) ok, (\d+) failed, "
                  r"(\d+) bypassed, (\d+) after disable; (\d+) flushes", r.stdout)
    assert m, r.stdout
    calls, ok, failed, bypassed, after, flushes = map(int, m.groups())
    assert calls == 32 * 150 and failed >= 1 and bypassed >= 1 and after >= 1
    assert flushes < ok + failed


def test_batch_core_is_free_of_hip():
    """The core must stay buildable without ROCm: no HIP or library
    header, no dg_index."""
    src = open(CORE).read()
    includes = re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", src)
    assert includes and all("/" not in i and not i.startswith("dg_")
                            for i in includes), includes
    assert "hip" not in " ".join(includes)
