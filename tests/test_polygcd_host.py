"""The part of the polynomial gcd that needs no device.

galois_amd/csrc/gfa_polygcd.h holds Euclid's algorithm and its extended form as the kernel runs them, as __host__ __device__
templates; tests/csrc/polygcd_host_test.cpp compiles them with g++ (polydiv::Solo) and checks them against a schoolbook Euclid: every
degree pair of {0, 1, 63, 64, 65, 130}^2, zero operands, b | a, a = b, deg a < deg b, and remainder sequences built backwards from
quotients of 1, 64, 65 and 66 coefficients -- once plain, once under AddressSanitizer and UBSan."""
import os
import subprocess

import pytest


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_polygcd_header_agrees_with_schoolbook_euclid_on_the_host(tmp_path, repo_root, sanitize):
    exe = str(tmp_path / "polygcd_host_test")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wno-unknown-pragmas"] + flags + ["-I", os.path.join(repo_root, "galois_amd", "csrc"),
                    os.path.join(repo_root, "tests", "csrc", "polygcd_host_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "polygcd host model ok" in r.stdout, r.stdout + r.stderr
    for name in ("GF(5)", "GF(4294967291)", "GF(4294967291^2)"):
        # 36 degree pairs x 3 operand patterns, 16 with a zero operand, 20 with a planted divisor, 10 with chosen quotients
        assert f"{name}: 154 euclid cases" in r.stdout
