"""gfa::Scratch, the owner of a call's device work buffers, needs no device to be checked.

tests/csrc/scratch_host_test.cpp compiles galois_amd/csrc/gfa_scratch.h with g++ against an allocator of its own (malloc / free
that log every call and can refuse the k-th one) and checks: n = 0, 1, 5, 8 buffers are freed exactly once each, last taken
first, on the guard's stream, also when the scope is left by an early return; a refused allocation at every position k < n leaves
a null pointer and frees only the k earlier buffers; a ninth buffer is refused with hipErrorInvalidValue without a call of the
allocator.  Once plain, once under AddressSanitizer and UBSan, where a leak or a double free ends the run."""
import os
import subprocess

import pytest


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_scratch_guard_frees_each_buffer_once_in_reverse_order(tmp_path, repo_root, sanitize):
    exe = str(tmp_path / "scratch_host_test")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__"] + flags + ["-I", os.path.join(rocm, "include"),
                    "-I", os.path.join(repo_root, "galois_amd", "csrc"),
                    os.path.join(repo_root, "tests", "csrc", "scratch_host_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "scratch guard ok" in r.stdout, r.stdout + r.stderr
