"""The parts of the irreducibility / primitivity feature that need no device.

galois_amd/csrc/gfa_polytest.h holds the per-candidate routines of the kernels as __host__ __device__ templates;
tests/csrc/polytest_host_test.cpp compiles them with g++ and checks them against a sieve of every monic polynomial over GF(2) up
to degree 12, GF(3) up to degree 6, GF(5) and GF(4) up to degree 4, and against the order of x found by stepping -- once plain,
once under AddressSanitizer and UBSan.  The host enumerator of fixed-term candidates is checked on its own."""
import math
import os
import subprocess

import pytest


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_polytest_header_agrees_with_a_sieve_on_the_host(tmp_path, repo_root, sanitize):
    exe = str(tmp_path / "polytest_host_test")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wno-unknown-pragmas"] + flags + ["-I", os.path.join(repo_root, "galois_amd", "csrc"),
                    os.path.join(repo_root, "tests", "csrc", "polytest_host_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "polytest host model ok" in r.stdout, r.stdout + r.stderr
    assert "GF(2): degrees 1..12, 747 irreducible" in r.stdout  # sum over d <= 12 of the necklace counts


def _digits(v, q):
    out = []
    while v:
        v, d = divmod(v, q)
        out.append(d)
    return out  # ascending


@pytest.mark.parametrize("q, m, t", [(2, 8, 3), (2, 8, 5), (3, 5, 3), (5, 4, 2)])
@pytest.mark.parametrize("reverse", [False, True])
def test_fixed_term_candidates_are_enumerated_in_order(q, m, t, reverse):
    from galois_amd._polysearch import _fixed_term_ints

    ints = list(_fixed_term_ints(q, m, t, reverse))
    assert len(ints) == math.comb(m - 1, t - 2) * (q - 1) ** (t - 1)
    if reverse:
        ints = ints[::-1]
    assert all(a < b for a, b in zip(ints, ints[1:]))  # strictly increasing: lexicographic order, no duplicates
    for v in ints:
        d = _digits(v, q)
        assert len(d) == m + 1 and d[m] == 1 and d[0] != 0 and sum(1 for c in d if c) == t


def test_fixed_term_candidates_with_one_term():
    from galois_amd._polysearch import _fixed_term_ints

    assert list(_fixed_term_ints(3, 4, 1)) == [81]
