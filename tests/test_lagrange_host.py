"""The part of Lagrange interpolation that needs no device.

galois_amd/csrc/gfa_lagrange.h holds the weights, the duplicate flag and the sweeps of the interpolation kernel as
__host__ __device__ templates; tests/csrc/lagrange_host_test.cpp compiles them with g++ and checks them against a schoolbook
elimination of the Vandermonde system over GF(2), GF(3), GF(5), GF(4) and GF(4294967291): every k from 1 to min(q, 9) and k = q,
teams with fewer threads than points, a repeated x in the first, middle and last position, all-zero and constant y, x with and
without 0 -- once plain, once under AddressSanitizer and UBSan."""
import os
import subprocess

import pytest


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_lagrange_header_agrees_with_a_schoolbook_vandermonde_solve_on_the_host(tmp_path, repo_root, sanitize):
    exe = str(tmp_path / "lagrange_host_test")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wno-unknown-pragmas"] + flags + ["-I", os.path.join(repo_root, "galois_amd", "csrc"),
                    os.path.join(repo_root, "tests", "csrc", "lagrange_host_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "lagrange host model ok" in r.stdout, r.stdout + r.stderr
    # per k and per choice of x (with 0, without): 3 kinds of y + a repeated x in min(k, 3) places for k >= 2; 9 team runs each
    for name, ks in (("GF(2)", [1, 2]), ("GF(3)", [1, 2, 3]), ("GF(5)", [1, 2, 3, 4, 5]), ("GF(4)", [1, 2, 3, 4]),
                     ("GF(4294967291)", list(range(1, 10)) + [33])):
        cases = sum(2 * (3 + (min(k, 3) if k >= 2 else 0)) for k in ks)
        assert f"{name}: {cases} lagrange cases, {9 * cases} runs" in r.stdout, r.stdout
