"""The part of the shift registers that needs no device.

galois_amd/csrc/gfa_lfsr.h holds the register clocks (one thread per register) and the jump-ahead (a team of threads per register)
as the kernels run them, as __host__ __device__ templates; tests/csrc/lfsr_host_test.cpp compiles them with g++ (polydiv::Solo) and
checks them against a schoolbook transcription of the reference's four step loops and a schoolbook x^e mod P: orders {1, 2, 63, 64,
65, 130}, steps {1, n-1, n, n+1, 3n+1}, forward and backward, a_n = 0, Galois states that only shift, jumps by {0, 1, n, 2^40 + 3},
the Fibonacci <-> Galois conversion and the one-word GF(2) clock -- once plain, once under AddressSanitizer and UBSan."""
import os
import subprocess

import pytest


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_lfsr_header_agrees_with_the_schoolbook_loops_on_the_host(tmp_path, repo_root, sanitize):
    exe = str(tmp_path / "lfsr_host_test")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wno-unknown-pragmas"] + flags + ["-I", os.path.join(repo_root, "galois_amd", "csrc"),
                    os.path.join(repo_root, "tests", "csrc", "lfsr_host_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "lfsr host model ok" in r.stdout, r.stdout + r.stderr
    for name in ("GF(5)", "GF(4294967291)", "GF(4294967291^2)"):
        # per order and kind: 3, 4 or 5 step counts x 2 directions (27 x 2 x 2 = 108) and one a_n = 0 case (12); 6 states that only
        # shift.  4 exponents x 2 kinds x 6 orders jumps, one conversion per order.
        assert f"{name}: 126 step cases, 48 jump cases, 6 conversion cases" in r.stdout
    assert "GF(2) words: 60 cases" in r.stdout  # 5 orders x 2 kinds x 6 step counts


REF_TESTS = "/root/reference/tests/test_fibonacci_lfsr.py"


@pytest.mark.skipif(not os.path.exists(REF_TESTS), reason="the reference checkout is not on this machine")
def test_sage_lfsr_fixture_regenerates_identically(tmp_path, repo_root):
    """tests/golden/sage_lfsr.npz is the reference's own data: read again out of its test file it comes out array for array as committed."""
    import importlib.util

    import numpy as np

    golden = os.path.join(repo_root, "tests", "golden")
    spec = importlib.util.spec_from_file_location("generate_lfsr_golden", os.path.join(golden, "generate_lfsr_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fresh, committed = np.load(gen.pack(str(tmp_path))), np.load(os.path.join(golden, "sage_lfsr.npz"))
    assert sorted(fresh.keys()) == sorted(committed.keys()) and len(fresh.keys()) == 8 * 4 + 1
    for k in fresh.keys():
        assert fresh[k].dtype == committed[k].dtype and fresh[k].shape == committed[k].shape and np.array_equal(fresh[k], committed[k]), k
