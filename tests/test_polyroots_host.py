"""The part of the root search that needs no device.

galois_amd/csrc/gfa_polyroots.h holds the slot rule, the rank sort and the repeated synthetic division of the finishing kernel as
__host__ __device__ templates; tests/csrc/polyroots_host_test.cpp compiles them with g++ and checks them against a schoolbook count
of the factors (x - r) over GF(2), GF(3), GF(5), GF(4) and GF(4294967291): multiplicities p - 1, p, p + 1 and 2 p, a row whose
capacity is exactly full (and claims beyond it), rows without roots and the zero row -- once plain, once under AddressSanitizer
and UBSan."""
import os
import subprocess

import pytest


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_polyroots_header_agrees_with_a_schoolbook_count_of_linear_factors_on_the_host(tmp_path, repo_root, sanitize):
    exe = str(tmp_path / "polyroots_host_test")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wno-unknown-pragmas"] + flags + ["-I", os.path.join(repo_root, "galois_amd", "csrc"),
                    os.path.join(repo_root, "tests", "csrc", "polyroots_host_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "polyroots host model ok" in r.stdout, r.stdout + r.stderr
    # 5 multiplicities x (2 rows per leading root, up to 4 of them, + the pure power) + 3 full rows + 4 rows without roots
    for name, cases in (("GF(2)", 32), ("GF(3)", 42), ("GF(5)", 52), ("GF(4)", 52), ("GF(4294967291)", 52)):
        assert f"{name}: {cases} root cases" in r.stdout, r.stdout
