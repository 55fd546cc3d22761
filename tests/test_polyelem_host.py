"""The part of the primitive / normal element feature that needs no device.

galois_amd/csrc/gfa_polyelem.h holds the per-candidate routines of the kernels as __host__ __device__ templates;
tests/csrc/polyelem_host_test.cpp compiles them with g++ and checks them on every residue of GF(2^m) up to m = 10, GF(3^m) up to
m = 5, GF(5^m) up to m = 4 and GF(4)[x] at degrees 2 and 3 against an elimination of the conjugate matrix and the multiplicative
order found by stepping, with the cofactor matrices fed whole and in slabs, and the bit-packed path at m = 63 .. 129 -- once
plain, once under AddressSanitizer and UBSan."""
import os
import subprocess

import pytest


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_polyelem_header_agrees_with_rank_and_order_on_the_host(tmp_path, repo_root, sanitize):
    exe = str(tmp_path / "polyelem_host_test")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wno-unknown-pragmas"] + flags + ["-I", os.path.join(repo_root, "galois_amd", "csrc"),
                    os.path.join(repo_root, "tests", "csrc", "polyelem_host_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "polyelem host model ok" in r.stdout, r.stdout + r.stderr
    # the counts q^m prod (1 - q^(-deg P_i)) of the eleven recorded fields, and phi(q^m - 1)
    for line in ("GF(2), m = 2: 1 factors of x^m - 1, 2 normal, 2 primitive", "GF(2), m = 3: 2 factors of x^m - 1, 3 normal, 6 primitive",
                 "GF(2), m = 4: 1 factors of x^m - 1, 8 normal, 8 primitive", "GF(2), m = 5: 2 factors of x^m - 1, 15 normal, 30 primitive",
                 "GF(2), m = 6: 2 factors of x^m - 1, 24 normal, 36 primitive", "GF(3), m = 2: 2 factors of x^m - 1, 4 normal, 4 primitive",
                 "GF(3), m = 3: 1 factors of x^m - 1, 18 normal, 12 primitive", "GF(3), m = 4: 3 factors of x^m - 1, 32 normal, 32 primitive",
                 "GF(5), m = 2: 2 factors of x^m - 1, 16 normal, 8 primitive", "GF(5), m = 3: 2 factors of x^m - 1, 96 normal, 60 primitive",
                 "GF(5), m = 4: 4 factors of x^m - 1, 256 normal, 192 primitive", "GF(4), m = 2: 1 factors of x^m - 1, 12 normal, 8 primitive",
                 "GF(4), m = 3: 3 factors of x^m - 1, 27 normal, 36 primitive", "GF(2), m = 129, W = 4: 11 factors"):
        assert line in r.stdout, line
