"""The part of the folds and scans that needs no device: how a call is cut into segments and which kernels run.

galois_amd/csrc/gfa_reduce_plan.h holds the arithmetic gfa_reduce.hip plans a call with (segments per row, segment length, first-phase
kernel, joining kernel), on plain integers with the CU count as a parameter; tests/csrc/reduce_plan_host_test.cpp compiles it with g++ and
sweeps CU counts {1, 64, 256, 304}, row counts up to 2^31 - 1 and lengths around every threshold up to 2^40: the segments cover the folded
columns exactly once with none empty, 1 <= nseg <= 4096, scan segments are multiples of 256, the 64-bit bounds of the integer-sum and
log-sum forms hold wherever they are chosen, and rows x segments fits the launch grid for every row count the entry points accept -- once
plain, once under AddressSanitizer and UBSan.  The program prints the plan of a fixed list of calls; tests/fold_plan.py, the Python mirror
the GPU tests take their shapes from, must give the same lines."""
import os
import re
import subprocess

import pytest

from tests import fold_plan as P

LINE = re.compile(r"^(reduce|accumulate) op=(\d) cus=(\d+) rows=(\d+) cols=(\d+) size=(\d) p=(\d+) m=(\d+) lut=([01]) -> ")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_reduce_plan_header_on_the_host_and_its_python_mirror(tmp_path, repo_root, sanitize):
    exe = str(tmp_path / "reduce_plan_host_test")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", os.path.join(repo_root, "galois_amd", "csrc"),
                    os.path.join(repo_root, "tests", "csrc", "reduce_plan_host_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "reduce plan host model ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()[:-1]
    assert len(lines) > 10_000
    seen = set()
    for line in lines:
        g = LINE.match(line)
        assert g, line
        kind, (op, cus, rows, cols, size, p, m, lut) = g.group(1), map(int, g.groups()[1:])
        pl = P.plan(kind, op, rows, cols, size, p, m, p**m, bool(lut), cus)
        assert P.describe(pl, size, p, m, bool(lut), cus) == line
        covered = P.segments(pl)
        assert covered[0][0] == (1 if op in (P.SUB, P.DIV) else 0) and covered[-1][1] == cols
        assert all(a[1] == b[0] for a, b in zip(covered, covered[1:])) and all(lo < hi for lo, hi in covered) or cols == 1
        seen.add((pl.form, pl.join, min(pl.c, 2), pl.nseg > 1))
    # the list reaches every first-phase form with every join
    for form in (P.GENERIC, P.STREAM_XOR, P.STREAM_SUM, P.STREAM_LOG, P.STREAM_TAB):
        for join in (("thread", 0, False), ("thread", 0, True), ("block", 0, True), ("carries", 1, True), ("carries", 2, True)):
            assert (form, join[0], join[1], join[2]) in seen, (form, join)
    assert (None, "row", 0, False) in seen


def test_fold_plan_of_the_shapes_the_gpu_tests_name():
    """The routes that the shapes of tests/test_gpu_folds.py take at 256 CUs, spelled out: a change of the planner that moves them shows
    here first."""
    gf256 = dict(elem_size=1, p=2, m=8, q=256, lookup=True, cus=256)
    gf243 = dict(elem_size=1, p=3, m=5, q=243, lookup=True, cus=256)
    r = lambda op, rows, cols, f=gf256: P.plan_reduce(op, rows, cols, **f)
    a = lambda op, rows, cols, f=gf256: P.plan_accumulate(op, rows, cols, **f)
    assert (r(P.ADD, 5, 8192).nseg, r(P.ADD, 5, 8193).nseg, r(P.ADD, 5, 8193).join) == (1, 3, "thread")
    assert (r(P.SUB, 5, 8193).nseg, r(P.SUB, 5, 8194).nseg, r(P.DIV, 5, 8194).seg_len) == (1, 3, 2731)
    assert (r(P.ADD, 3, 40003).nseg, r(P.ADD, 3, 40003).join, r(P.ADD, 3, 40003).seg_len) == (10, "block", 4001)
    assert (r(P.ADD, 3, 40003, gf243).form, r(P.ADD, 3, 40003, gf243).nseg) == (P.STREAM_TAB, 10)
    # sums of a byte table field of degree > 1 plan with 2 workgroups per CU (GF(2^8) too, though its sums are xors), everything else with 8
    gf65521 = dict(elem_size=2, p=65521, m=1, q=65521, lookup=False, cus=256)
    assert (r(P.ADD, 1025, 9001, gf65521).nseg, r(P.MUL, 1025, 9001).nseg, r(P.ADD, 257, 9001, gf243).nseg, r(P.ADD, 257, 9001).nseg) == (2, 2, 2, 2)
    assert (r(P.ADD, 2048, 9001, gf65521).nseg, r(P.ADD, 512, 9001, gf243).nseg, r(P.ADD, 512, 9001).nseg, r(P.MUL, 512, 9001, gf243).nseg) == (1, 1, 1, 3)
    assert (r(P.MUL, 1, 8 * 4096).join, r(P.MUL, 1, 8 * 4096 + 1).join, r(P.MUL, 1, 8 * 4096 + 1).nseg) == ("thread", "block", 9)
    assert (a(P.ADD, 2, 65535).join, a(P.ADD, 2, 65536).nseg, a(P.ADD, 2, 65536).seg_len, a(P.SUB, 2, 65536).join, a(P.SUB, 2, 65537).nseg) == ("row", 8, 8192, "row", 8)
    assert (a(P.ADD, 3, 70001).nseg, a(P.ADD, 3, 70001).seg_len, P.segments(a(P.ADD, 3, 70001))[-1]) == (8, 8960, (62720, 70001))
    assert (a(P.MUL, 1, 2_200_001).nseg, a(P.MUL, 1, 2_200_001).c, a(P.MUL, 1, 2_200_001).form) == (261, 2, P.STREAM_LOG)
    assert a(P.ADD, 512, 70001).join == "row" and a(P.ADD, 511, 70001).join == "carries"
