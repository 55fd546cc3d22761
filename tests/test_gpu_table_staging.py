"""How the table kernels bring their tables into LDS (stage_table_lds, gfa_internal.h): every lane of a workgroup loads a batch of
four 16-byte units and then writes them, batch after batch, the last batch cut off at the end of the image.  What can go wrong
is a unit that lands in the wrong place or not at all -- a whole 16 KiB quarter of the 64 KiB table of the uint8 kernels, the
part of a batch behind the end of a LOG | EXP | ZECH image -- and that shows only for operands that READ those entries: random
data at small sizes can miss them.  So the operands here run over every pair of field elements (uint8 kernels: every byte of
the table is read) or every field element on both sides (uint16 kernels: every entry of LOG, and of EXP / ZECH whatever the
permutation reaches).  Expected values come from numpy (GF(2^8), bit-serial) or the oracle, never from the library.

The tab8 cases run again in a fresh process per forced kernel (non-temporal stores, claimed blocks), as in test_gpu_tab8_order.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import galois_amd as ga
from galois_amd import _lib as L
from oracle import gf_oracle as O

pytestmark = pytest.mark.gpu

BLOCK = 1024 * 16  # elements per workgroup and round of the uint8 table kernels (TAB8_THREADS lanes x one 16-byte vector)


def gf256_mul(a, b):
    """Bit-serial product in GF(2)[x] / (x^8 + x^4 + x^3 + x^2 + 1)."""
    a, b = a.astype(np.uint16), b.astype(np.uint16)
    r = np.zeros_like(a)
    for k in range(8):
        r ^= a * ((b >> k) & 1)
        a = (a << 1) ^ (((a >> 7) & 1) * 0x11D)
    return r.astype(np.uint8)


def gf256_inverses():
    """v^-1 = v^254 by bit-serial products (entry 0 is 0 and never used)."""
    v = np.arange(256, dtype=np.uint8)
    inv = np.ones(256, dtype=np.uint8)
    for _ in range(254):
        inv = gf256_mul(inv, v)
    return inv


def binary(GF, op, a, b, out, err=None):
    st = torch.cuda.current_stream().cuda_stream
    L.check(L.lib().gfa_binary(GF._handle, op, a.data_ptr(), 1, b.data_ptr(), 1, out.data_ptr(), a.numel(), L.U8, st,
                               err.data_ptr() if err is not None else None), "gfa_binary")


def run_u8(GF, op, ah, bh):
    """op over two host arrays through gfa_binary; checks that nothing behind the n results was written."""
    n = ah.size
    a, b = torch.from_numpy(ah).cuda(), torch.from_numpy(bh).cuda()
    out = torch.full((n + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    binary(GF, op, a, b, out[:n], err=err)
    got = out.cpu().numpy()
    assert (got[n:] == 0xEE).all(), "wrote past the end"
    assert int(err.item()) == 0
    return got[:n]


def test_tab8_every_table_byte_gf256_mul_div():
    GF = ga.GF(2**8)
    v = np.arange(256, dtype=np.uint8)
    a, b = np.repeat(v, 256), np.tile(v, 256)  # entry (a << 8) | b of the table for every a, b: n = 65536
    got, want = run_u8(GF, L.OP_MUL, a, b), gf256_mul(a, b)
    assert np.array_equal(got, want), f"first difference at table entry {int(np.flatnonzero(got != want)[0])}"
    a, b = np.repeat(v, 255), np.tile(v[1:], 256)  # every entry with b != 0
    got, want = run_u8(GF, L.OP_DIV, a, b), gf256_mul(a, gf256_inverses()[b])
    assert np.array_equal(got, want), f"first difference at index {int(np.flatnonzero(got != want)[0])}"


def test_tab8_every_table_byte_gf243_add_sub():
    GF = ga.GF(3**5)
    F = O.OracleField(GF.characteristic, GF.degree, int(GF.irreducible_poly), int(GF.primitive_element), lookup=True)
    v = np.arange(243, dtype=np.uint8)
    a, b = np.repeat(v, 243), np.tile(v, 243)  # n = 59049 = 16 * 3690 + 9: whole vectors and a tail
    for op, oop in ((L.OP_ADD, O.ADD), (L.OP_SUB, O.SUB)):
        got, want = run_u8(GF, op, a, b), F.ufunc_u8(oop, a, b)
        assert np.array_equal(got, want), f"op {op}: first difference at index {int(np.flatnonzero(got != want)[0])}"


@pytest.mark.parametrize("n", [5, 16, 17, 31, BLOCK + 16])
def test_tab8_lanes_and_workgroups_without_operands_stage_their_share(n):
    """Fewer vectors than lanes (n = 5: none at all, the sub-16 tail reads the table), and a second workgroup with ONE vector:
    all four quarters of the table must be there although most lanes, or most of a workgroup, loaded no operand."""
    GF = ga.GF(2**8)
    rng = np.random.default_rng(n)
    a = np.array([0, 64, 128, 192, 255], dtype=np.uint8)[np.arange(n) % 5]  # one value per 16 KiB quarter of the table (and the last row)
    if n > 31:
        a = a[rng.permutation(n)]
    b = rng.integers(0, 256, n, dtype=np.uint8)
    assert np.array_equal(run_u8(GF, L.OP_MUL, a, b), gf256_mul(a, b))
    bnz = np.where(b == 0, 1, b).astype(np.uint8)
    assert np.array_equal(run_u8(GF, L.OP_DIV, a, bnz), gf256_mul(a, gf256_inverses()[bnz]))


FORCED = {"nt_stores": {"GFA_TAB8_NT_MIN_LOG": "0", "GFA_TAB8_CLAIM_MIN_LOG": "62"},
          "claimed_blocks": {"GFA_TAB8_CLAIM_MIN_LOG": "0"}}


@pytest.mark.parametrize("kernel", sorted(FORCED))
def test_forced_kernel(kernel, repo_root):
    env = dict(os.environ, **FORCED[kernel])
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-k", "tab8",
                        os.path.abspath(__file__)],
                       cwd=repo_root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "7 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


# ---- uint16 storage: LOG | EXP | ZECH images of run-time size (mid_kernel, mid_powv_kernel) ----
# order -> (lanes per workgroup, k): n = 8 * lanes * k + 9 elements, at least the 2^17 from which these kernels are used.
#   GF(257):  LOG + EXP = 264 + 528 entries = 99 units of 16 bytes, fewer than the 512 lanes: one batch, most lanes load nothing
#   GF(3^7):  q = 2187, qa = 2192: 822 units for products, 1096 with ZECH: two and three units for some lanes, one batch
#   GF(2^15): the largest field of these kernels, LOG + EXP = 2 x 32768 entries = 8192 units on 1024 lanes: two whole batches
#             (sums are xors there, so ZECH is never staged)
#   GF(3^9):  q = 19683, qa = 19688 on 1024 lanes: 4922 units for products (a second batch of one unit, for 826 lanes only), 7383
#             with ZECH (a second batch of three units, a fourth for 215 lanes): the batch that is cut off inside
#   GF(163^2): q = 26569, the largest extension field of odd characteristic whose three tables fit: LOG | EXP | ZECH = 3 x 26576
#             entries = 155.7 KiB = 9966 units on 1024 lanes, the largest image there is: two whole batches and a third of 1774
#             units (two units for 750 lanes, one for the rest); 6644 units for products
MID = {257: (512, 33), 3**7: (512, 33), 2**15: (1024, 17), 3**9: (1024, 17), 163**2: (1024, 17)}


def mid_operands(q, need_nonzero_b=False):
    lanes, k = MID[q]
    n = 8 * lanes * k + 9
    a = np.resize(np.arange(q, dtype=np.uint64), n)
    b = a[np.random.default_rng(q).permutation(n)]
    if need_nonzero_b:
        b = np.where(b == 0, 1, b)
    return a, b


def mid_field(q):
    GF = ga.GF(q)
    p, m = GF.characteristic, GF.degree
    F = O.OracleField(p, m, int(GF.irreducible_poly) if m > 1 else None, GF._primitive_element_int, lookup=True)
    return GF, F


def first_diff(got, want):
    d = np.flatnonzero(got != want)
    return f"{d.size} differ, first at {int(d[0])}: got {int(got[d[0]])}, want {int(want[d[0]])}" if d.size else ""


@pytest.mark.parametrize("q", sorted(MID))
def test_mid_every_element_mul_div_reciprocal_power(q):
    GF, F = mid_field(q)
    a, b = mid_operands(q, need_nonzero_b=True)
    ga_, gb_ = GF(a.astype(np.uint16), dtype=np.uint16), GF(b.astype(np.uint16), dtype=np.uint16)
    for name, got, want in (("mul", ga_ * gb_, F.mul(a, b)), ("div", ga_ / gb_, F.div(a, b)),
                            ("reciprocal", np.reciprocal(gb_), F.recip(b)), ("power", ga_**5, F.pow(a, np.full(a.size, 5)))):
        got = got.numpy().astype(np.uint64)
        assert np.array_equal(got, want), f"GF({q}) {name}: {first_diff(got, want)}"


@pytest.mark.parametrize("q", [3**7, 3**9, 163**2])
def test_mid_every_element_add_with_zech(q):
    GF, F = mid_field(q)
    a, b = mid_operands(q)
    got = (GF(a.astype(np.uint16), dtype=np.uint16) + GF(b.astype(np.uint16), dtype=np.uint16)).numpy().astype(np.uint64)
    want = F.add(a, b)
    assert np.array_equal(got, want), f"GF({q}) add: {first_diff(got, want)}"


def test_mid_power_with_an_exponent_array_gf3_7():
    q = 3**7
    GF, F = mid_field(q)
    a, _ = mid_operands(q)
    e = np.random.default_rng(77).integers(-3000, 3000, a.size)
    e[a == 0] = np.abs(e[a == 0])  # 0 ** negative raises
    got = (GF(a.astype(np.uint16), dtype=np.uint16) ** e).numpy().astype(np.uint64)
    want = F.pow(a, e)
    assert np.array_equal(got, want), f"GF({q}) power: {first_diff(got, want)}"
