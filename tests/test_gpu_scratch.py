"""No call leaves a work buffer behind: every site that takes device memory through gfa::Scratch (galois_amd/csrc/gfa_scratch.h)
is called twice with the smallest input that reaches it, and gfa_debug_scratch_in_use() -- the bytes currently taken from the
library's stream-ordered pool -- reads the same after the second call as after the first; the second result equals the first.

site -> case
  gfa_charpoly.hip        launch_charpoly_ft (five buffers)            charpoly: three 5 x 5 matrices over GF(7)
  gfa_linalg.hip          launch_row_reduce_wide_ft (state, factor)    row_reduce_wide: 256 x 512 over GF(2^8) (m n >= 131072)
  gfa_dlog.hip            dlog_run (lb)                                log_base: GF(2^31 - 1), base=
  gfa_conv_crt.hip        run_crt_set                                  convolve_crt: 2048 x 2048 terms over GF(31)
  gfa_conv_crt.hip        run_planes                                   convolve_planes: 1024 x 1024 terms over GF(2^8)
  gfa_rs.hip              gfa_rs_decode (rem)                          rs_decode: RS(255, 223)
  gfa_rs.hip              gfa_debug_rs_bm_selftest (d_seq/d_len/d_out) rs_bm_selftest: 1000 sequences
  gfa_rs_wide.hip         polydiv_t (scratch)                          rs_wide_message: non-systematic RS(1023, 1003) over GF(2^10)
  gfa_rs_wide.hip         rs_wide_decode (tmp)                         rs_wide_in_place: out is recv through the C-ABI
  gfa_elementwise.hip     launch_tab8_claim (counter)                  tab8_claim: 2^28 bytes over GF(2^8)
  gfa_elementwise_mid.hip big16_inv_launch<3> (tab)                    big16_pow_table: y ** 12345, GF(3^10), uint16, 2^19 elements
  gfa_elementwise_mid.hip big16_launch (idx, two-kernel branch)        big16_two_kernel: x * y, GF(3^10), uint16, 2^22 elements
  gfa_elementwise_mid.hip big16_power_each (idx)                       big16_power_each: an exponent per element, GF(3^10)
  gfa_elementwise_mid.hip big16_run_wide_t (wa)                        big16_wide: x * y, GF(3^10) held as uint32
  gfa_elementwise_packed.hip pow24_run (tab)                           pow24: y ** 12345, GF(3^11), uint32, 8 q elements
  gfa_polytest.hip        gfa_poly_classify (dev, list)                poly_classify: three quartics over GF(7), primitivity asked
  gfa_polydiv.hip         launch_div (ws)                              poly_div_global: a divisor one longer than the LDS window
  gfa_polydiv.hip         gfa_poly_powmod (exps)                       poly_powmod: x^12345 mod a quadratic over GF(31)
  gfa_matmul_mfma.hip     run_mfma                                     matmul_prime: 128^3 over GF(31)
  gfa_matmul_mfma.hip     run_mfma_limbs                               matmul_limbs: 512^3 over GF(65537)
  gfa_matmul_mfma.hip     run_mfma_bits                                matmul_bits: 256^3 over GF(2^8) (2^24 multiply-adds: the default
                                                                       GFA_MFMA_BITS_MIN_LOG, which is read once per process)
  gfa_matmul_mfma.hip     run_mfma_digits                              matmul_digits: 256^3 over GF(3^2)
The two sites of gfa_dist.hip need a communicator: tests/test_gpu_multi.py runs them."""
import ctypes

import numpy as np
import pytest
import torch

import galois_amd as ga
from galois_amd import _lib as L
from galois_amd import _polydiv as PD
from galois_amd import _polysearch as PS

pytestmark = pytest.mark.gpu


def _same(x, y) -> bool:
    if isinstance(x, (tuple, list)):
        return len(x) == len(y) and all(_same(a, b) for a, b in zip(x, y))
    if isinstance(x, ga.FieldArray):
        return torch.equal(x._t, y._t)
    if isinstance(x, torch.Tensor):
        return torch.equal(x, y)
    if isinstance(x, np.ndarray):
        return np.array_equal(x, y)
    return bool(x == y)


def _device_random(GF, shape, low, np_dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.randint(low, GF.order, (shape,), generator=g, device="cuda", dtype=torch.uint8 if GF.order <= 256 else torch.int64)
    return GF(t, dtype=np_dtype)


def _charpoly():
    A = ga.GF(7).Random((3, 5, 5), seed=1)
    return lambda: ga.linalg.characteristic_poly_batched(A)


def _row_reduce_wide():
    A = ga.GF(2**8).Random((256, 512), seed=2)
    return lambda: A.row_reduce()


def _log_base():
    GF = ga.GF(2**31 - 1)
    x = GF.Random(1000, low=1, seed=3)
    base = GF(GF._primitive_element_int)
    return lambda: x.log(base=base)


def _convolve(order, n):
    GF = ga.GF(order)
    a, b = GF.Random(n, seed=4), GF.Random(n, seed=5)
    return lambda: np.convolve(a, b)


def _rs_decode():
    rs = ga.ReedSolomon(255, 223)
    R = rs.encode(np.random.default_rng(6).integers(0, 256, (16, 223))).numpy().copy()
    R[:, 5] ^= 1
    return lambda: rs.decode(R, output="codeword", errors=True)


def _rs_bm_selftest():
    GF = ga.GF(2**8)

    def run():
        bad = ctypes.c_int64(-1)
        L.check(L.lib().gfa_debug_rs_bm_selftest(GF._handle, 1000, 7, ctypes.byref(bad), torch.cuda.current_stream().cuda_stream),
                "gfa_debug_rs_bm_selftest")
        return bad.value
    return run


def _wide_received(rs, rows):
    k = rs.k
    R = rs.encode(np.random.default_rng(8).integers(0, 1024, (rows, k))).numpy().astype(np.int64)
    R[:, 3] = (R[:, 3] + 1) % 1024
    return R


def _rs_wide_message():
    rs = ga.ReedSolomon(1023, 1003, field=ga.GF(2**10), systematic=False)
    R = _wide_received(rs, 4)
    return lambda: rs.decode(R, errors=True)


def _rs_wide_in_place():
    rs = ga.ReedSolomon(1023, 1003, field=ga.GF(2**10))
    recv = torch.from_numpy(_wide_received(rs, 4).astype(np.int16)).cuda()

    def run():
        buf = recv.clone()
        nerr = torch.empty(4, dtype=torch.int64, device="cuda")
        L.check(L.lib().gfa_rs_decode(rs._handle, buf.data_ptr(), None, 1023, buf.data_ptr(), nerr.data_ptr(), 4, L.U16,
                                      torch.cuda.current_stream().cuda_stream), "gfa_rs_decode")
        return buf, nerr
    return run


def _tab8_claim():
    GF = ga.GF(2**8)
    a, b = _device_random(GF, 1 << 28, 0, np.uint8, 9), _device_random(GF, 1 << 28, 0, np.uint8, 10)
    return lambda: a * b


def _big16(op, n, np_dtype):
    GF = ga.GF(3**10)
    x, y = _device_random(GF, n, 0, np_dtype, 11), _device_random(GF, n, 1, np_dtype, 12)
    if op == "mul":
        return lambda: x * y
    if op == "pow":
        return lambda: y ** 12345
    ks = np.random.default_rng(13).integers(-(2**40), 2**40, n)
    return lambda: y ** ks


def _pow24():
    GF = ga.GF(3**11)
    y = _device_random(GF, 8 * 3**11 + 8, 1, np.uint32, 14)
    return lambda: y ** 12345


def _poly_classify():
    GF = ga.GF(7)
    t = GF.Random((3, 5), low=1, seed=15)._t.contiguous()
    return lambda: PS._classify(GF, t, True)


def _poly_div_global():
    GF = ga.GF(31)
    nb = PD.divmod_lds_max_divisor(GF) + 1
    a, b = GF.Random((2, nb + 2), low=1, seed=16)._t.contiguous(), GF.Random(nb, low=1, seed=17)._t.contiguous()
    return lambda: PD._divmod_t(GF, a, b, True, True)


def _poly_powmod():
    GF = ga.GF(31)
    a, c = GF.Random((2, 4), low=1, seed=18)._t.contiguous(), GF([1, 3, 5])._t.contiguous()
    return lambda: PD._powmod_t(GF, a, 12345, c)


def _matmul(order, n):
    GF = ga.GF(order)
    A, B = GF.Random((n, n), seed=19), GF.Random((n, n), seed=20)
    return lambda: A @ B


CASES = {
    "charpoly": _charpoly,
    "row_reduce_wide": _row_reduce_wide,
    "log_base": _log_base,
    "convolve_crt": lambda: _convolve(31, 2048),
    "convolve_planes": lambda: _convolve(2**8, 1024),
    "rs_decode": _rs_decode,
    "rs_bm_selftest": _rs_bm_selftest,
    "rs_wide_message": _rs_wide_message,
    "rs_wide_in_place": _rs_wide_in_place,
    "tab8_claim": _tab8_claim,
    "big16_pow_table": lambda: _big16("pow", 1 << 19, np.uint16),
    "big16_two_kernel": lambda: _big16("mul", 1 << 22, np.uint16),
    "big16_power_each": lambda: _big16("pow_each", 1 << 19, np.uint16),
    "big16_wide": lambda: _big16("mul", 1 << 19, np.uint32),
    "pow24": _pow24,
    "poly_classify": _poly_classify,
    "poly_div_global": _poly_div_global,
    "poly_powmod": _poly_powmod,
    "matmul_prime": lambda: _matmul(31, 128),
    "matmul_limbs": lambda: _matmul(65537, 512),
    "matmul_bits": lambda: _matmul(2**8, 256),
    "matmul_digits": lambda: _matmul(3**2, 256),
}


@pytest.mark.parametrize("case", list(CASES))
def test_a_second_call_leaves_the_pool_as_the_first_left_it(case):
    call = CASES[case]()
    in_use = L.lib().gfa_debug_scratch_in_use
    first = call()  # warm-up: tables, kernel attributes, the pool itself
    torch.cuda.synchronize()
    before = in_use()
    second = call()
    torch.cuda.synchronize()
    assert _same(first, second), f"{case}: the second call computed something else"
    after = in_use()
    print(f"{case}: pool bytes in use {before} -> {after}")
    assert before >= 0, "the pool's hipMemPoolAttrUsedMemCurrent cannot be read"
    assert after == before, f"{case}: {after - before} bytes stayed allocated in the work-buffer pool"
