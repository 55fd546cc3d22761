"""The part of polynomial division and modular powers that needs no device.

galois_amd/csrc/gfa_polydiv.h holds the blocked synthetic division and the square-and-multiply chain of the kernels as
__host__ __device__ templates; tests/csrc/polydiv_host_test.cpp compiles them with g++ and checks them against a schoolbook loop and
against repeated multiply-and-reduce, for every combination of quotient length in {1, K-1, K, K+1, 2K+3} and divisor length in
{1, 2, K, K+1, 3K+5} on sparse operands -- once plain, once under AddressSanitizer and UBSan."""
import os
import subprocess

import pytest


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_polydiv_header_agrees_with_schoolbook_division_on_the_host(tmp_path, repo_root, sanitize):
    exe = str(tmp_path / "polydiv_host_test")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wno-unknown-pragmas"] + flags + ["-I", os.path.join(repo_root, "galois_amd", "csrc"),
                    os.path.join(repo_root, "tests", "csrc", "polydiv_host_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "polydiv host model ok" in r.stdout, r.stdout + r.stderr
    for name in ("GF(3)", "GF(5)", "GF(4294967291)", "GF(4)", "GF(4294967291^2)"):
        assert f"{name}: 100 division cases" in r.stdout and f"{name}: 115 power cases" in r.stdout  # 5 x 5 shapes x 4 operand patterns
