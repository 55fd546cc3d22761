"""The 64 KiB-table kernel behind every binary op of a field of order <= 256 on uint8 (launch_tab8_binary): array sizes at
every boundary of its block schedule, division by zero in the last block and in the sub-16 tail, another table, in-place use,
back-to-back launches, two streams, and graph replay.  Expected values are a few lines of numpy here -- a bit-serial product
for GF(2^8)/0x11D, the oracle's 243 x 243 addition table indexed with the operands for GF(3^5) -- never the library.

launch_tab8_binary chooses among three kernels by array size: static striding with ordinary stores (below 2^26 elements), the
same with non-temporal stores (2^26 .. 2^28) and claimed blocks (from 2^28).  The sizes here reach only the first on their own,
so test_forced_kernel runs this whole file again in a fresh process per kernel, with GFA_TAB8_NT_MIN_LOG / GFA_TAB8_CLAIM_MIN_LOG
(read once per process) moving the bounds to 1 element: every case below then runs on the non-temporal kernel and on the claim
kernel too -- DIV instantiations, in-place use, streams and graph replay included."""
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

BLOCK = 1024 * 16  # elements per block: one 16-byte vector per lane of a 1024-thread workgroup (TAB8_THREADS)


def grid():
    """The library's grid for a full device: two 64 KiB-LDS workgroups per CU (tab8_grid)."""
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count


def sizes():
    G, B = grid(), BLOCK
    return [1, 15, 16, 17, B - 1, B, B + 1, G * B - 16, G * B, G * B + 16 + 3, 3 * G * B + 5]


def gf256_mul(a, b):
    """Bit-serial product in GF(2)[x] / (x^8 + x^4 + x^3 + x^2 + 1)."""
    a, b = a.astype(np.uint16), b.astype(np.uint16)
    r = np.zeros_like(a)
    for k in range(8):
        r ^= a * ((b >> k) & 1)
        a = (a << 1) ^ (((a >> 7) & 1) * 0x11D)
    return r.astype(np.uint8)


_GF256_INV = None


def gf256_div(a, b):
    """a * b^-1 with b^-1 = b^254 by bit-serial products; b must have no zero."""
    global _GF256_INV
    if _GF256_INV is None:
        v = np.arange(256, dtype=np.uint8)
        inv = np.ones(256, dtype=np.uint8)
        for _ in range(254):
            inv = gf256_mul(inv, v)
        _GF256_INV = inv
    return gf256_mul(a, _GF256_INV[b])


def binary(GF, op, a, b, out, stream=None, err=None):
    st = (stream or torch.cuda.current_stream()).cuda_stream
    L.check(L.lib().gfa_binary(GF._handle, op, a.data_ptr(), 1, b.data_ptr(), 1, out.data_ptr(), a.numel(), L.U8, st,
                               err.data_ptr() if err is not None else None), "gfa_binary")


@pytest.fixture(scope="module")
def big():
    """Random operands of the largest size, 3 G B + 5, and their product: computed once, shared, never modified."""
    n = sizes()[-1]
    rng = np.random.default_rng(7)
    a, b = rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8)
    z = gf256_mul(a, b)
    for v in (a, b, z):
        v.setflags(write=False)
    return a, b, z


def test_gf256_mul_at_every_schedule_boundary(big):
    GF = ga.GF(2**8)
    A, B_, Z = big
    for n in sizes():
        # the first n elements of the shared operands, in fresh (16-byte-aligned) tensors
        a, b = torch.from_numpy(A[:n].copy()).cuda(), torch.from_numpy(B_[:n].copy()).cuda()
        out = torch.full((n + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        binary(GF, L.OP_MUL, a, b, out[:n])
        got = out.cpu().numpy()
        assert np.array_equal(got[:n], Z[:n]), f"n = {n}"
        assert (got[n:] == 0xEE).all(), f"n = {n}: wrote past the end"
        a.fill_(255), b.fill_(255)
        binary(GF, L.OP_MUL, a, b, out[:n])
        got = out.cpu().numpy()
        assert (got[:n] == gf256_mul(np.array([255], np.uint8), np.array([255], np.uint8))[0]).all() and (got[n:] == 0xEE).all(), f"n = {n}"


def test_division_by_zero_in_the_last_block_and_in_the_tail(big):
    GF = ga.GF(2**8)
    A, B_, _ = big
    n = sizes()[-1]  # 3 G B + 5: the last whole vector is the last block's, elements n - 5 .. n - 1 are the tail
    bnz = np.where(B_ == 0, 1, B_).astype(np.uint8)
    a, out = torch.from_numpy(A.copy()).cuda(), torch.empty(n, dtype=torch.uint8, device="cuda")
    want = gf256_div(A, bnz)
    for zero_at, raises in [(None, False), ((n // 16) * 16 - 7, True), (n - 2, True)]:
        bh = bnz.copy()
        if zero_at is not None:
            bh[zero_at] = 0
        b = torch.from_numpy(bh).cuda()
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        binary(GF, L.OP_DIV, a, b, out, err=err)
        assert bool(int(err.item()) & L.DEVERR_ZERO_DIVISION) == raises, f"zero at {zero_at}"
        if not raises:
            assert np.array_equal(out.cpu().numpy(), want)


def test_another_table_gf243_add():
    GF = ga.GF(3**5)
    F = O.OracleField(GF.characteristic, GF.degree, int(GF.irreducible_poly), int(GF.primitive_element), lookup=True)
    v = np.arange(243, dtype=np.uint8)
    table = F.ufunc_u8(O.ADD, np.repeat(v, 243), np.tile(v, 243)).reshape(243, 243)
    n = sizes()[-1]
    rng = np.random.default_rng(8)
    ah, bh = rng.integers(0, 243, n, dtype=np.uint8), rng.integers(0, 243, n, dtype=np.uint8)
    a, b = torch.from_numpy(ah).cuda(), torch.from_numpy(bh).cuda()
    out = torch.empty_like(a)
    binary(GF, L.OP_ADD, a, b, out)
    assert np.array_equal(out.cpu().numpy(), table[ah, bh])


def test_in_place(big):
    GF = ga.GF(2**8)
    A, B_, Z = big
    for alias in ("a", "b"):
        a, b = torch.from_numpy(A.copy()).cuda(), torch.from_numpy(B_.copy()).cuda()
        out = a if alias == "a" else b
        binary(GF, L.OP_MUL, a, b, out)
        assert np.array_equal(out.cpu().numpy(), Z), f"out is {alias}"


_GF256_TABLE = None


def gf256_mul_fast(a, b):
    """The same bit-serial product, taken once over all 256 x 256 pairs and then indexed: for the many-launch tests."""
    global _GF256_TABLE
    if _GF256_TABLE is None:
        v = np.arange(256, dtype=np.uint8)
        _GF256_TABLE = gf256_mul(np.repeat(v, 256), np.tile(v, 256)).reshape(256, 256)
    return _GF256_TABLE[a, b]


def _operands(count, n, seed):
    """`count` different operand pairs from one random pair: launch i gets (a ^ i, b ^ (3 i + 1))."""
    rng = np.random.default_rng(seed)
    a0, b0 = rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8)
    hs = [(a0 ^ np.uint8(i), b0 ^ np.uint8((3 * i + 1) & 255)) for i in range(count)]
    ds = [(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), torch.empty(n, dtype=torch.uint8, device="cuda")) for a, b in hs]
    return hs, ds


def test_back_to_back_launches_on_one_stream():
    GF = ga.GF(2**8)
    n = grid() * BLOCK + 16 + 3  # more blocks than workgroups, a partial block and a tail
    hs, ds = _operands(64, n, 9)
    for a, b, o in ds:
        binary(GF, L.OP_MUL, a, b, o)
    torch.cuda.synchronize()
    for i, ((ah, bh), (_, _, o)) in enumerate(zip(hs, ds)):
        assert np.array_equal(o.cpu().numpy(), gf256_mul_fast(ah, bh)), f"launch {i}"


def test_two_streams_concurrently():
    GF = ga.GF(2**8)
    n = grid() * BLOCK + 16 + 3
    hs, ds = _operands(64, n, 10)
    torch.cuda.synchronize()
    s = [torch.cuda.Stream(), torch.cuda.Stream()]
    for i, (a, b, o) in enumerate(ds):  # alternate, so that launches of both streams are in flight together
        binary(GF, L.OP_MUL, a, b, o, stream=s[i & 1])
    torch.cuda.synchronize()
    for i, ((ah, bh), (_, _, o)) in enumerate(zip(hs, ds)):
        assert np.array_equal(o.cpu().numpy(), gf256_mul_fast(ah, bh)), f"launch {i} (stream {i & 1})"


def test_graph_replay_on_rewritten_operands():
    GF = ga.GF(2**8)
    n = grid() * BLOCK + 16 + 3
    (_, ds) = _operands(1, n, 11)
    a, b, o1 = ds[0]
    o2 = torch.empty_like(o1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        binary(GF, L.OP_MUL, a, b, o1, stream=side)  # warm-up outside the capture: table upload, attributes
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            binary(GF, L.OP_MUL, a, b, o1, stream=side)   # o1 = a * b
            binary(GF, L.OP_MUL, o1, b, o2, stream=side)  # o2 = a * b * b
    rng = np.random.default_rng(12)
    for replay in range(20):
        ah, bh = rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8)
        a.copy_(torch.from_numpy(ah).cuda()), b.copy_(torch.from_numpy(bh).cuda())
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        if replay >= 17:
            z = gf256_mul_fast(ah, bh)
            assert np.array_equal(o1.cpu().numpy(), z), f"replay {replay}, first launch"
            assert np.array_equal(o2.cpu().numpy(), gf256_mul_fast(z, bh)), f"replay {replay}, second launch"


FORCED = {"nt_stores": {"GFA_TAB8_NT_MIN_LOG": "0", "GFA_TAB8_CLAIM_MIN_LOG": "62"},
          "claimed_blocks": {"GFA_TAB8_CLAIM_MIN_LOG": "0"}}


@pytest.mark.parametrize("kernel", sorted(FORCED))
def test_forced_kernel(kernel, repo_root):
    env = dict(os.environ, **FORCED[kernel])
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-k", "not forced_kernel",
                        os.path.abspath(__file__)],
                       cwd=repo_root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "7 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
