"""The part of the elimination entry points that needs no device: which kernels a gfa_row_reduce call runs and which shapes are refused.

galois_amd/csrc/gfa_elim_plan.h holds the decision gfa_linalg.hip takes (one workgroup per matrix, two kernels per column, or a refusal) on
plain integers; tests/csrc/elim_plan_host_test.cpp compiles it with g++ and sweeps rows and columns around 256, 4096, 2^24 and the tallest
matrix the two-kernel grid holds, m * n around 131072 (including products past 32 bits) and batches around 32 and 65535 against the rules
restated in 128-bit arithmetic -- once plain, once under AddressSanitizer and UBSan.  The program prints the route of every call of the
sweep; tests/elim_plan.py, the Python mirror the GPU tests assert their routes with, must give the same lines."""
import os
import re
import subprocess

import pytest

from tests import elim_plan as P

ROUTE = re.compile(r"^row_reduce batch=(\d+) m=(\d+) n=(\d+) -> [A-Z_]+$")
PLU = re.compile(r"^plu m=(\d+) n=(\d+) -> (yes|no)$")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_elim_plan_header_on_the_host_and_its_python_mirror(tmp_path, repo_root, sanitize):
    exe = str(tmp_path / "elim_plan_host_test")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", os.path.join(repo_root, "galois_amd", "csrc"),
                    os.path.join(repo_root, "tests", "csrc", "elim_plan_host_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "elim plan host model ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()[:-1]
    assert len(lines) > 100_000
    seen = set()
    for line in lines:
        g = ROUTE.match(line)
        if g:
            b, m, n = map(int, g.groups())
            assert P.describe_route(b, m, n) == line
            seen.add((P.elim_route(b, m, n), b <= P.GJ_WIDE_MAX_BATCH, m <= P.GJ_MAX_ROWS, m * n >= P.GJ_WIDE_MIN_ELEMS, m * n >= 2**32))
        else:
            g = PLU.match(line)
            assert g, line
            assert P.describe_plu(int(g.group(1)), int(g.group(2))) == line
    # the sweep reaches every route on both sides of every threshold, with and without a product past 32 bits
    for key in [(P.ONE_WORKGROUP, True, True, False, False), (P.ONE_WORKGROUP, False, True, True, False), (P.ONE_WORKGROUP, False, True, True, True),
                (P.TWO_KERNELS, True, True, True, False), (P.TWO_KERNELS, True, True, True, True), (P.TWO_KERNELS, True, False, False, False),
                (P.TWO_KERNELS, True, False, True, True), (P.UNSUPPORTED, False, False, False, False), (P.UNSUPPORTED, False, False, True, True),
                (P.UNSUPPORTED, True, False, True, True)]:
        assert key in seen, key


def test_routes_of_the_shapes_the_gpu_tests_name():
    """The thresholds spelled out on the shapes of tests/test_gpu_elimination_routes.py: a change of the planner that moves them shows here
    first."""
    r = P.elim_route
    assert (r(1, 300, 40), r(1, 40, 300), r(1, 300, 300), r(1, 362, 362), r(1, 363, 362)) == (P.ONE_WORKGROUP,) * 4 + (P.TWO_KERNELS,)
    assert (257 * 510, 257 * 511) == (131070, 131327) and (r(1, 257, 510), r(1, 257, 511)) == (P.ONE_WORKGROUP, P.TWO_KERNELS)
    assert (r(1, 256, 511), r(1, 256, 512), r(1, 1, 131071), r(1, 1, 131072)) == (P.ONE_WORKGROUP, P.TWO_KERNELS, P.ONE_WORKGROUP, P.TWO_KERNELS)
    assert (r(32, 257, 511), r(33, 257, 511), r(5, 257, 511)) == (P.TWO_KERNELS, P.ONE_WORKGROUP, P.TWO_KERNELS)
    assert (r(1, 255, 510), r(1, 256, 512)) == (P.ONE_WORKGROUP, P.TWO_KERNELS)  # [A | I] of the inverse at n = 255, 256
    assert (r(1, 4096, 8), r(1, 4097, 8), r(32, 4097, 8), r(33, 4097, 8), r(33, 4096, 8), r(1, 4097, 32)) == (
        P.ONE_WORKGROUP, P.TWO_KERNELS, P.TWO_KERNELS, P.UNSUPPORTED, P.ONE_WORKGROUP, P.TWO_KERNELS)
    assert (r(1, 2097120, 1), r(1, 2097121, 1), r(1, 1, 2**24), r(1, 1, 2**24 + 1)) == (P.TWO_KERNELS, P.UNSUPPORTED, P.TWO_KERNELS, P.UNSUPPORTED)
    assert (r(65539, 3, 4), r(65539, 3, 6), r(1, 420, 428), r(1, 412, 420), r(1, 256, 520)) == (P.ONE_WORKGROUP, P.ONE_WORKGROUP) + (P.TWO_KERNELS,) * 3
    assert (P.plu_supported(4096, 4), P.plu_supported(4097, 4), P.plu_supported(300, 300), P.plu_supported(4096, 2**24 + 1)) == (True, False, True, False)
