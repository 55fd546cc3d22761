"""divmod / // / % / ** / three-argument pow of Poly, poly_divmod_batched / poly_powmod_batched and the entry points gfa_poly_divmod /
gfa_poly_powmod (galois_amd/csrc/gfa_polydiv.hip): the reference's Sage vectors and live answers (tests/golden/sage_polydiv.npz),
division checked by uniqueness (a == q b + r with r shorter than b, through the product and sum kernels) at every shape at which the
blocked kernel takes another path, the fused power against the multiply-then-reduce loop and against Fermat / Rabin identities,
the C contract and the Python error paths.  Everything is exact."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import galois_amd as ga
from galois_amd import _lib as L
from galois_amd import _numtheory as nt
from galois_amd import _polydiv as PD
from galois_amd import _polysearch as PS
from tests import helpers as H

pytestmark = pytest.mark.gpu

K, THREADS = PD.BLOCK, PD.DIV_THREADS
GOLDEN = os.path.join(H.GOLDEN, "sage_polydiv.npz")
TAGS = sorted(k.split("/")[1] for k in np.load(GOLDEN).keys() if k.startswith("sage/") and k.endswith("/properties"))


@functools.lru_cache(maxsize=None)
def _golden():
    d = np.load(GOLDEN)
    return {k: d[k] for k in d.keys()}


def _sage_field(tag):
    props = json.loads(str(_golden()[f"sage/{tag}/properties"]))
    p, m = props["characteristic"], props["degree"]
    if m == 1:
        return ga.GF(p, primitive_element=int(props["primitive_element"]))
    return ga.GF(p, m, irreducible_poly=[int(c) for c in props["irreducible_poly"]], primitive_element=int(props["primitive_element"]))


def _coeffs(poly):
    return [int(v) for v in poly.coeffs.numpy()]


def _poly(GF, c):
    return ga.Poly(GF(np.array([int(v) for v in c], dtype=object)))


def _lists(key):
    """The polynomials stored under `key` as lists of Python integers."""
    g = _golden()
    flat, ends = [int(v) for v in g[key]], np.cumsum(g[key + "_len"])
    return [flat[e - n:e] for e, n in zip(ends, g[key + "_len"])]


def _is(poly, GF, c):
    return isinstance(poly, ga.Poly) and poly.field is GF and _coeffs(poly) == [int(v) for v in c]


# ---- 1. the reference's vectors -----------------------------------------------------------------------------------------------------
def test_all_sage_folders_present():
    assert len(TAGS) == 16
    assert {"GF_2", "GF_2e8", "GF_2e8_283_19", "GF_7e3", "GF_2147483647", "GF_2e32", "GF_2e100", "GF_109987e4", "GF_36893488147419103183"} <= set(TAGS)


@pytest.mark.parametrize("tag", TAGS)
def test_sage_divmod(tag):
    GF = _sage_field(tag)
    X, Y, Q, R = (_lists(f"sage/{tag}/divmod_{k}") for k in "XYQR")
    assert len(X) == 23
    for x, y, q, r in zip(X, Y, Q, R):
        f, g = _poly(GF, x), _poly(GF, y)
        got_q, got_r = divmod(f, g)
        assert _is(got_q, GF, q) and _is(got_r, GF, r), f"{tag}: divmod({x}, {y})"
        assert _is(f // g, GF, q) and _is(f % g, GF, r), f"{tag}: {x} // or % {y}"


@pytest.mark.parametrize("tag", TAGS)
def test_sage_powers(tag):
    GF = _sage_field(tag)
    g = _golden()
    X, M, Z = (_lists(f"sage/{tag}/modpow_{k}") for k in "XMZ")
    E = [int(e) for e in g[f"sage/{tag}/modpow_E"]]
    assert len(X) == 20
    for x, e, m, z in zip(X, E, M, Z):
        assert _is(pow(_poly(GF, x), e, _poly(GF, m)), GF, z), f"{tag}: pow({x}, {e}, {m})"
    X, Y, Z = _lists(f"sage/{tag}/power_X"), [int(e) for e in g[f"sage/{tag}/power_Y"]], _lists(f"sage/{tag}/power_Z")
    assert len(X) == 5 and len(Y) == 4 and len(Z) == 20
    for i, x in enumerate(X):
        for j, e in enumerate(Y):
            assert _is(_poly(GF, x) ** e, GF, Z[4 * i + j]), f"{tag}: {x} ** {e}"


@pytest.mark.parametrize("order", [2**8, 7**3, 2**100])
def test_live_answers_for_long_exponents(order):
    g = _golden()
    tag = {2**8: "GF_2e8", 7**3: "GF_7e3", 2**100: "GF_2e100"}[order]
    p, m = nt.factors(order)[0][0], nt.factors(order)[1][0]
    GF = ga.GF(p, m, irreducible_poly=[int(c) for c in g[f"live/{tag}/irreducible_poly"]], primitive_element=int(g[f"live/{tag}/primitive_element"]))
    assert GF.order == order
    f, c = _poly(GF, g[f"live/{tag}/f"]), _poly(GF, g[f"live/{tag}/g"])
    exps = [int(e) for e in g["live/exponents"]]
    assert exps == [2**64, 2**64 + 1234, 2**70 + 105030405]
    for k, e in enumerate(exps):
        assert _is(pow(f, e, c), GF, g[f"live/{tag}/z{k}"]), f"{tag}: exponent {e}"


# ---- 2. division beyond the fixtures, by uniqueness --------------------------------------------------------------------------------
def _wrap(GF, t):
    return GF._wrap(t.contiguous(), PS._storage(GF)[0])


def _sparse(GF, shape, seed, keep=0.5):
    """Random elements with about half of them zeroed, as a storage tensor."""
    t = GF.Random(shape, seed=seed)._t
    mask = (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) < keep).to(t.device)
    return torch.where(mask, t, torch.zeros_like(t)).contiguous()


def _divisor(GF, nb, seed):
    b = _sparse(GF, (nb,), seed, keep=0.4)  # zero interior coefficients
    b[0] = GF.Random(1, low=1, seed=seed + 1)._t[0]
    return b


def _dividends(GF, batch, na, seed):
    a = _sparse(GF, (batch, na), seed)
    if batch > 1:
        a[1] = 0  # a zero row
    if batch > 2:
        a[2, :(na + 1) // 2] = 0  # leading zeros: zero quotient coefficients
    return a


def _assert_is_the_division(GF, a, b, q, r):
    """a == q b + r row by row, with two kernel calls: the quotients, spaced na apart in one long polynomial, times b."""
    batch, na = a.shape
    nb = b.numel()
    nq = na - nb + 1
    assert tuple(q.shape) == (batch, nq) and tuple(r.shape) == (batch, nb - 1) and q.dtype == a.dtype and r.dtype == a.dtype
    qpad = torch.zeros_like(a)
    qpad[:, nb - 1:] = q
    prod = np.convolve(_wrap(GF, qpad.reshape(-1)), _wrap(GF, b))
    assert prod.size == batch * na + nb - 1
    rpad = torch.zeros_like(a)
    rpad[:, nq:] = r
    back = _wrap(GF, prod._t[nb - 1:].reshape(batch, na)) + _wrap(GF, rpad)
    assert torch.equal(back._t, a)


def _division_case(GF, batch, nq, nb, seed):
    na = nq + nb - 1
    a, b = _dividends(GF, batch, na, seed), _divisor(GF, nb, seed + 7)
    keep_a, keep_b = a.clone(), b.clone()
    Q, R = ga.poly_divmod_batched(_wrap(GF, a), _wrap(GF, b))
    assert type(Q) is GF and type(R) is GF
    q = Q._t
    r = R._t if nb > 1 else R._t[:, :0]  # a constant divisor: one zero column
    if nb == 1:
        assert tuple(R.shape) == (batch, 1) and not bool(R._t.any())
    _assert_is_the_division(GF, a, b, q, r)
    assert torch.equal(a, keep_a) and torch.equal(b, keep_b)  # the inputs are not modified
    # quotient-only and remainder-only calls equal the pair
    q_only, none = PD._divmod_t(GF, a, b, True, False)
    assert none is None and torch.equal(q_only, q)
    none, r_only = PD._divmod_t(GF, a, b, False, True)
    assert none is None and torch.equal(r_only, r)
    return a, b, q, r


FIELDS = {
    "GF(2)": lambda: ga.GF(2), "GF(31)": lambda: ga.GF(31), "GF(3191)": lambda: ga.GF(3191), "GF(2147483647)": lambda: ga.GF(2147483647),
    "GF(2^61-1)": lambda: ga.GF(2**61 - 1), "Goldilocks": lambda: ga.GF(H.GOLDILOCKS), "GF(2^8)": lambda: ga.GF(2**8),
    "GF(2^8) calculate": lambda: ga.GF(2**8), "GF(2^32)": lambda: ga.GF(2**32), "GF(7^3)": lambda: ga.GF(7**3), "GF(3^7)": lambda: ga.GF(3**7),
    "GF(7^7)": lambda: ga.GF(7**7), "GF(7^8)": lambda: ga.GF(7**8), "GF(3^13)": lambda: ga.GF(3**13),  # the last two: digit vectors
}
DIVISION_FIELDS = [n for n in FIELDS if n != "GF(3^13)"]  # (its products in the check are the slowest; it is covered at fewer shapes below)


class _mode:
    """The field in the named mode for the length of a test ("GF(2^8) calculate" pins explicit arithmetic)."""

    def __init__(self, name):
        self.GF = FIELDS[name]()
        self.calculate = name.endswith("calculate")

    def __enter__(self):
        if self.calculate:
            self.GF.compile("jit-calculate")
        return self.GF

    def __exit__(self, *exc):
        if self.calculate:
            self.GF.compile("auto")


@pytest.mark.parametrize("name", DIVISION_FIELDS)
def test_division_is_the_unique_one_at_every_block_shape(name):
    with _mode(name) as GF:
        seed = 100
        for nq in (1, K - 1, K, K + 1, 2 * K + 1):
            for deg in (0, 1, K - 1, K, K + 1, 4 * THREADS + 3):
                a, b, q, r = _division_case(GF, 257, nq, deg + 1, seed)
                # prefixes of the batch give the same rows
                for batch in (1, 3):
                    Q, R = ga.poly_divmod_batched(_wrap(GF, a[:batch]), _wrap(GF, b))
                    assert torch.equal(Q._t, q[:batch]) and (deg == 0 or torch.equal(R._t, r[:batch]))
                seed += 1


@pytest.mark.parametrize("name", DIVISION_FIELDS)
def test_division_at_the_lds_boundary(name):
    """The longest divisor whose window is held in LDS, and one coefficient more (the work copy in global memory)."""
    with _mode(name) as GF:
        nb = PD.divmod_lds_max_divisor(GF)
        assert nb == (8128 if PD._elem_bytes(GF) == 4 else 4032)
        for n, nq in ((nb, K + 1), (nb + 1, K + 1), (nb + 1, 1)):
            _division_case(GF, 3, nq, n, 900 + nq + n)


@pytest.mark.parametrize("name", ["GF(31)", "GF(2^8)", "GF(2^32)", "GF(7^3)", "Goldilocks", "GF(3^13)"])
def test_poly_operators_agree_with_the_batched_form(name):
    with _mode(name) as GF:
        for nq, nb in ((1, 1), (K + 1, 2), (3, K + 1), (2 * K + 1, K)):
            a, b, q, r = _division_case(GF, 3, nq, nb, 40 + nq)
            g = ga.Poly(_wrap(GF, b))
            for k in range(3):
                f = ga.Poly(_wrap(GF, a[k]))
                fq, fr = divmod(f, g)
                assert fq == ga.Poly(_wrap(GF, q[k])) and fr == (ga.Poly(_wrap(GF, r[k])) if nb > 1 else ga.Poly(GF([0])))
                assert f // g == fq and f % g == fr and fq * g + fr == f
                assert fr.degree < g.degree or _coeffs(fr) == [0]


def test_short_dividends_and_reflected_operands():
    GF = ga.GF(31)
    f, g = ga.Poly(GF([3, 0, 5])), ga.Poly(GF([1, 2, 0, 30]))
    assert divmod(f, g) == (ga.Poly(GF([0])), f) and f // g == ga.Poly(GF([0])) and f % g == f  # deg a < deg b: (0, a)
    assert divmod(ga.Poly(GF([0])), g) == (ga.Poly(GF([0])), ga.Poly(GF([0])))
    assert divmod(f, ga.Poly(GF([2]))) == (ga.Poly(GF([3, 0, 5]) / GF(2)), ga.Poly(GF([0])))  # a constant divisor: (a / b0, 0)
    s = GF(7)
    assert divmod(s, ga.Poly(GF([2]))) == (ga.Poly(GF([7]) / GF(2)), ga.Poly(GF([0])))
    assert s // g == ga.Poly(GF([0])) and s % g == ga.Poly(GF([7])) and g % s == ga.Poly(GF([0])) and g // s == ga.Poly(g.coeffs / s)
    Q, R = ga.poly_divmod_batched(GF([[0, 3, 0, 5], [0, 0, 0, 1]]), g)  # rows shorter than the divisor once trimmed, and as given
    assert Q.numpy().tolist() == [[0], [0]] and R.numpy().tolist() == [[3, 0, 5], [0, 0, 1]]
    Q, R = ga.poly_divmod_batched(GF([[3, 0, 5]]), GF([0, 0, 1, 2, 0, 30]))  # a 1-D divisor with leading zeros is trimmed
    assert Q.numpy().tolist() == [[0]] and R.numpy().tolist() == [[3, 0, 5]]


# ---- 3. powers ------------------------------------------------------------------------------------------------------------------
def _loop_power(f, e, c):
    """The Python multiply-then-% loop, right to left (the fused kernel walks the exponent from the left)."""
    acc, sq = ga.Poly(f.field([1])), f % c
    while e:
        if e & 1:
            acc = (acc * sq) % c
        e >>= 1
        if e:
            sq = (sq * sq) % c
    return acc % c


POWER_FIELDS = ["GF(31)", "GF(2^8)", "GF(2^8) calculate", "Goldilocks", "GF(7^7)", "GF(7^8)", "GF(3^13)"]


@pytest.mark.parametrize("degrees", ["1, 2, K, K + 1", "cap", "cap + 1"])
@pytest.mark.parametrize("name", POWER_FIELDS)
def test_fused_power_equals_the_multiply_then_reduce_loop(name, degrees):
    """Degrees up to the cap run the fused kernel, cap + 1 the fallback; exponents 0, 1, 2, 2^20 + 3 and 2^64 + 1234 at each."""
    with _mode(name) as GF:
        cap = PD.powmod_max_degree(GF)
        assert cap == (7654 if PD._elem_bytes(GF) == 4 else 3814)
        for d in {"1, 2, K, K + 1": (1, 2, K, K + 1), "cap": (cap,), "cap + 1": (cap + 1,)}[degrees]:
            seed = 7 + 3 * d
            c = ga.Poly(_wrap(GF, _divisor(GF, d + 1, seed)))
            f = ga.Poly(_wrap(GF, _sparse(GF, (d + 3,), seed + 1)))  # longer than the modulus: reduced first
            for e in (0, 1, 2, 2**20 + 3, 2**64 + 1234):
                if d >= cap and e > 2 and name not in ("GF(31)", "Goldilocks"):
                    continue  # the long chains at the cap run on one field per element width
                got = pow(f, e, c)
                assert got.field is GF and got == (_loop_power(f, e, c) if e else ga.Poly(GF([1]))), f"degree {d}, exponent {e}"


@pytest.mark.parametrize("name", POWER_FIELDS)
def test_power_identities(name):
    with _mode(name) as GF:
        c = ga.Poly(_wrap(GF, _divisor(GF, 2 * K + 6, 21)))
        f = ga.Poly(_wrap(GF, _sparse(GF, (2 * K,), 22)))
        e1, e2 = 2**64 + 1234, 2**20 + 3
        assert pow(f, e1 + e2, c) == (pow(f, e1, c) * pow(f, e2, c)) % c
        assert pow(f, 3, c) == (f * f * f) % c and f**3 == f * f * f and f**0 == ga.Poly(GF([1])) and f**1 == f
        assert pow(f, 5, ga.Poly(GF([3]))) == ga.Poly(GF([0]))  # modulo a unit
        assert pow(ga.Poly(GF([0])), 0, c) == ga.Poly(GF([1]))  # pow_jit: 0^0 = 1
        # the batched form equals the row-by-row form, and prefixes of a batch give the same rows
        a = _dividends(GF, 257, 2 * K + 9, 23)
        Z = ga.poly_powmod_batched(_wrap(GF, a), e2, c)
        assert type(Z) is GF and tuple(Z.shape) == (257, c.degree)
        for k in (0, 1, 2, 256):
            z = pow(ga.Poly(_wrap(GF, a[k])), e2, c)
            assert z == ga.Poly(_wrap(GF, Z._t[k]))
        assert not bool(Z._t[1].any())  # the zero row
        assert torch.equal(ga.poly_powmod_batched(_wrap(GF, a[:3]), e2, c.coeffs)._t, Z._t[:3])
        ones = ga.poly_powmod_batched(_wrap(GF, a[:3]), 0, c)
        assert ones.numpy().tolist() == [[0] * (c.degree - 1) + [1]] * 3


@pytest.mark.parametrize("q, m", [(2, 64), (3, 20), (31, 5), (2**8, 3), (7**3, 4), (2**61 - 1, 2)])
def test_frobenius_fixes_x_modulo_an_irreducible_polynomial(q, m):
    GF = ga.GF(q)
    f = ga.irreducible_poly(q, m)
    x = ga.Poly(GF([1, 0]))
    assert pow(x, q**m, f) == x
    assert pow(x, q, f) != x  # m > 1: x is not in the ground field


@pytest.mark.parametrize("q, m", [(2, 16), (3, 8), (2**8, 2), (31, 3)])
def test_order_of_x_modulo_a_primitive_polynomial(q, m):
    """Cross-check with the independent Rabin / order kernel behind primitive_polys."""
    GF = ga.GF(q)
    f = next(ga.primitive_polys(q, m))
    x, one = ga.Poly(GF([1, 0])), ga.Poly(GF([1]))
    n = q**m - 1
    assert pow(x, n, f) == one
    for r in nt.factors(n)[0]:
        assert pow(x, n // r, f) != one, f"x has order dividing (q^m - 1) / {r}"
    g = next(h for h in ga.irreducible_polys(q, m) if not h.is_primitive() and _coeffs(h)[-1] != 0)
    assert pow(x, n, g) == one and any(pow(x, n // r, g) == one for r in nt.factors(n)[0])


# ---- 4. the C entry points' contract ------------------------------------------------------------------------------------------------
def _p(t):
    return t.data_ptr() if t is not None else None


def _divmod(GF, a, batch, na, b, nb, q, r, dtype):
    return L.lib().gfa_poly_divmod(GF._handle, _p(a), batch, na, _p(b), nb, _p(q), _p(r), dtype, torch.cuda.current_stream().cuda_stream)


def _powmod(GF, a, batch, na, e, c, nc, out, dtype, limbs=None):
    arr, n = PD._exp_limbs(e) if e is not None else (None, 1)
    return L.lib().gfa_poly_powmod(GF._handle, _p(a), batch, na, arr, n if limbs is None else limbs, _p(c), nc, _p(out), dtype,
                                   torch.cuda.current_stream().cuda_stream)


def test_divmod_entry_point_contract():
    GF = ga.GF(7)
    dev = torch.device("cuda")
    a = torch.tensor([[0, 3, 1, 4, 1, 5], [2, 6, 5, 3, 5, 6]], dtype=torch.uint8, device=dev)
    b = torch.tensor([3, 0, 2], dtype=torch.uint8, device=dev)
    q = torch.full((2, 4), 0x55, dtype=torch.uint8, device=dev)
    r = torch.full((2, 2), 0x55, dtype=torch.uint8, device=dev)
    assert _divmod(GF, a, 2, 6, b, 3, q, r, L.U8) == L.OK
    # by hand over GF(7): 1/3 = 5
    assert q.cpu().tolist() == [[0, 1, 5, 3], [3, 2, 2, 2]] and r.cpu().tolist() == [[5, 6], [1, 2]]
    for k in range(2):  # a == q b + r
        f, g = ga.Poly(GF(a[k].cpu().numpy())), ga.Poly(GF(b.cpu().numpy()))
        assert ga.Poly(GF(q[k].cpu().numpy())) * g + ga.Poly(GF(r[k].cpu().numpy())) == f
    # either output may be NULL; the other is written as before and the NULL one's buffer is left alone
    q2, r2 = torch.full_like(q, 0x55), torch.full_like(r, 0x55)
    assert _divmod(GF, a, 2, 6, b, 3, q2, None, L.U8) == L.OK and torch.equal(q2, q)
    assert _divmod(GF, a, 2, 6, b, 3, None, r2, L.U8) == L.OK and torch.equal(r2, r)
    assert _divmod(GF, a, 2, 6, b, 3, None, None, L.U8) == L.OK
    # nb == 1: r_out is not touched
    r2.fill_(0x55)
    assert _divmod(GF, a, 2, 6, b, 1, torch.empty((2, 6), dtype=torch.uint8, device=dev), r2, L.U8) == L.OK
    assert r2.cpu().tolist() == [[0x55, 0x55]] * 2
    q6 = torch.empty((2, 6), dtype=torch.uint8, device=dev)
    assert _divmod(GF, a, 2, 6, b, 1, q6, None, L.U8) == L.OK and q6.cpu().tolist() == [[0, 1, 5, 6, 5, 4], [3, 2, 4, 1, 4, 2]]
    # another storage width and a non-default stream
    s = torch.cuda.Stream()
    q4, r4 = torch.zeros((2, 4), dtype=torch.int64, device=dev), torch.zeros((2, 2), dtype=torch.int64, device=dev)
    a64, b64 = a.to(torch.int64), b.to(torch.int64)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        assert L.lib().gfa_poly_divmod(GF._handle, _p(a64), 2, 6, _p(b64), 3, _p(q4), _p(r4), L.U64, s.cuda_stream) == L.OK
    s.synchronize()
    assert torch.equal(q4, q.to(torch.int64)) and torch.equal(r4, r.to(torch.int64))
    # a zero leading coefficient is a caller error: the call ends and stays inside its buffers
    z = torch.tensor([0, 0, 2], dtype=torch.uint8, device=dev)
    assert _divmod(GF, a, 2, 6, z, 3, q2, r2, L.U8) == L.OK
    torch.cuda.synchronize()
    # batch == 0 touches nothing, whatever the pointers
    q2.fill_(0x55)
    assert _divmod(GF, None, 0, 6, None, 3, None, None, L.U8) == L.OK and _divmod(GF, a, 0, 6, b, 3, q2, r2, L.U8) == L.OK
    assert q2.cpu().tolist() == [[0x55] * 4] * 2
    # rejected calls
    assert _divmod(GF, None, 2, 6, b, 3, q2, r2, L.U8) == L.ERR_INVALID and _divmod(GF, a, 2, 6, None, 3, q2, r2, L.U8) == L.ERR_INVALID
    assert _divmod(GF, a, 2, 6, b, 0, q2, r2, L.U8) == L.ERR_INVALID and _divmod(GF, a, 2, 6, b, 7, q2, r2, L.U8) == L.ERR_INVALID
    assert _divmod(GF, a, -1, 6, b, 3, q2, r2, L.U8) == L.ERR_INVALID and _divmod(GF, a, 2, 6, b, 3, q2, r2, 9) == L.ERR_INVALID
    assert _divmod(ga.GF(65537), a, 2, 6, b, 3, q2, r2, L.U8) == L.ERR_INVALID and "dtype" in L.last_error()
    assert _divmod(GF, a, 2**31, 6, b, 3, q2, r2, L.U8) == L.ERR_UNSUPPORTED
    assert q2.cpu().tolist() == [[0x55] * 4] * 2


def test_powmod_entry_point_contract():
    GF = ga.GF(7)
    dev = torch.device("cuda")
    a = torch.tensor([[1, 0], [0, 0], [3, 5]], dtype=torch.uint8, device=dev)
    c = torch.tensor([1, 0, 0, 2], dtype=torch.uint8, device=dev)  # x^3 + 2
    out = torch.full((3, 3), 0x55, dtype=torch.uint8, device=dev)
    assert _powmod(GF, a, 3, 2, 4, c, 4, out, L.U8) == L.OK
    # x^4 = -2 x = 5 x;  (3 x + 5)^4 = 4 x^4 + x^3 + 6 x^2 + 2 x + 2 = 6 x^2 + (4 * 5 + 2) x + (5 + 2) = 6 x^2 + x
    assert out.cpu().tolist() == [[0, 5, 0], [0, 0, 0], [6, 1, 0]]
    assert _powmod(GF, a, 3, 2, 0, c, 4, out, L.U8) == L.OK and out.cpu().tolist() == [[0, 0, 1]] * 3  # e == 0: 1, also for the zero row
    assert _powmod(GF, a, 3, 2, 1, c, 4, out, L.U8) == L.OK and out.cpu().tolist() == [[0, 1, 0], [0, 0, 0], [0, 3, 5]]
    long_row = torch.tensor([[1, 0, 0, 0, 0, 3]], dtype=torch.uint8, device=dev)  # x^5 + 3 = x^2 (x^3 + 2) - 2 x^2 + 3
    assert _powmod(GF, long_row, 1, 6, 1, c, 4, out[:1], L.U8) == L.OK and out[:1].cpu().tolist() == [[5, 0, 3]]
    # an exponent with an empty high word; a modulus of degree 1: evaluation at the root
    arr = (ctypes.c_uint64 * 3)(4, 0, 0)
    assert L.lib().gfa_poly_powmod(GF._handle, _p(a), 3, 2, arr, 3, _p(c), 4, _p(out), L.U8, torch.cuda.current_stream().cuda_stream) == L.OK
    assert out.cpu().tolist() == [[0, 5, 0], [0, 0, 0], [6, 1, 0]]
    lin = torch.tensor([1, 4], dtype=torch.uint8, device=dev)  # x + 4: root 3
    o1 = torch.zeros((3, 1), dtype=torch.uint8, device=dev)
    assert _powmod(GF, a, 3, 2, 5, lin, 2, o1, L.U8) == L.OK and o1.cpu().tolist() == [[pow(3, 5, 7)], [0], [pow(14, 5, 7)]]
    # batch == 0 touches nothing
    out.fill_(0x55)
    assert _powmod(GF, None, 0, 2, 4, None, 4, None, L.U8) == L.OK and _powmod(GF, a, 0, 2, 4, c, 4, out, L.U8) == L.OK
    # rejected calls
    assert _powmod(GF, None, 3, 2, 4, c, 4, out, L.U8) == L.ERR_INVALID and _powmod(GF, a, 3, 2, 4, None, 4, out, L.U8) == L.ERR_INVALID
    assert _powmod(GF, a, 3, 2, 4, c, 4, None, L.U8) == L.ERR_INVALID and _powmod(GF, a, 3, 2, None, c, 4, out, L.U8) == L.ERR_INVALID
    assert _powmod(GF, a, 3, 2, 4, c, 1, out, L.U8) == L.ERR_INVALID and _powmod(GF, a, 3, 2, 4, c, 4, out, 9) == L.ERR_INVALID
    assert _powmod(GF, a, -1, 2, 4, c, 4, out, L.U8) == L.ERR_INVALID and _powmod(GF, a, 3, 2, 4, c, 4, out, L.U8, limbs=0) == L.ERR_INVALID
    assert _powmod(ga.GF(65537), a, 3, 2, 4, c, 4, out, L.U8) == L.ERR_INVALID and "dtype" in L.last_error()
    assert _powmod(GF, a, 2**31, 2, 4, c, 4, out, L.U8) == L.ERR_UNSUPPORTED
    assert out.cpu().tolist() == [[0x55] * 3] * 3


@pytest.mark.parametrize("name", ["GF(31)", "GF(2^8)", "GF(2^8) calculate", "GF(2^32)", "GF(7^3)", "GF(7^7)", "GF(2^61-1)", "Goldilocks", "GF(2147483647)"])
def test_powmod_cap_is_named_and_agrees_with_the_python_side(name):
    with _mode(name) as GF:
        cap = PD.powmod_max_degree(GF)
        np_dtype, tdt = PS._storage(GF)
        dtype = {1: L.U8, 2: L.U16, 4: L.U32, 8: L.U64}[torch.empty(0, dtype=tdt).element_size()]
        a = torch.ones((1, 1), dtype=tdt, device="cuda")
        c = torch.zeros(cap + 2, dtype=tdt, device="cuda")
        c[0] = 1
        out = torch.zeros((1, cap + 1), dtype=tdt, device="cuda")
        assert _powmod(GF, a, 1, 1, 3, c, cap + 2, out, dtype) == L.ERR_UNSUPPORTED
        assert str(cap) in L.last_error() and str(cap + 1) in L.last_error()
        assert _powmod(GF, a, 1, 1, 3, c[:cap + 1].contiguous(), cap + 1, out, dtype) == L.OK  # 1^3 modulo x^cap
        assert out[0, :cap].cpu().tolist() == [0] * (cap - 1) + [1]


# ---- 5. the Python error paths ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [31, 2**100])
def test_python_error_paths(order):
    GF = ga.GF(order)
    f, g, zero = ga.Poly(GF([1, 2, 3])), ga.Poly(GF([1, 5])), ga.Poly(GF([0]))
    for op in (lambda: divmod(f, zero), lambda: f // zero, lambda: f % zero, lambda: pow(f, 2, zero), lambda: GF(3) % zero):
        with pytest.raises(ZeroDivisionError):
            op()
    with pytest.raises(NotImplementedError, match="true division is not supported"):
        f / g
    with pytest.raises(NotImplementedError, match="true division is not supported"):
        GF(3) / g
    with pytest.raises(TypeError):
        f ** 2.0
    with pytest.raises(TypeError):
        pow(f, "2", g)
    with pytest.raises(ValueError, match="Can only exponentiate polynomials to non-negative integers, not -1"):
        f ** -1
    with pytest.raises(TypeError):
        f % ga.Poly(ga.GF(7)([1, 2]))
    with pytest.raises(TypeError):
        divmod(f, 3)
    assert f**0 == ga.Poly(GF([1])) and pow(f, 0, g) == ga.Poly(GF([1])) and pow(f, 7, ga.Poly(GF([4]))) == zero
    with pytest.raises(ZeroDivisionError):
        ga.poly_divmod_batched(GF([[1, 2, 3]]), zero)
    with pytest.raises(ZeroDivisionError):
        ga.poly_powmod_batched(GF([[1, 2, 3]]), 2, GF([0, 0]))
    with pytest.raises(ValueError):
        ga.poly_divmod_batched(GF([1, 2, 3]), g)
    with pytest.raises(TypeError):
        ga.poly_divmod_batched(GF([[1, 2, 3]]), [1, 5])
    with pytest.raises(ValueError):
        ga.poly_powmod_batched(GF([[1, 2, 3]]), -2, g)
    with pytest.raises(TypeError):
        ga.poly_powmod_batched(GF([[1, 2, 3]]), 2.5, g)


def test_batched_forms_over_a_field_of_order_above_2_64():
    GF = ga.GF(2**100)
    f = [[1, 2**99 + 5, 0, 7, 2**64], [0, 0, 3, 1, 2], [0, 0, 0, 0, 0]]
    g = ga.Poly(GF(np.array([2**80 + 1, 0, 9], dtype=object)))
    A = GF(np.array(f, dtype=object))
    Q, R = ga.poly_divmod_batched(A, g)
    assert tuple(Q.shape) == (3, 3) and tuple(R.shape) == (3, 2)
    Z = ga.poly_powmod_batched(A, 2**64 + 3, g)
    assert tuple(Z.shape) == (3, 2)
    for k in range(3):
        fk = _poly(GF, f[k])
        q, r = divmod(fk, g)
        assert q == ga.Poly(Q[k]) and r == ga.Poly(R[k]) and q * g + r == fk
        assert pow(fk, 2**64 + 3, g) == ga.Poly(Z[k])


def test_remainders_are_reed_solomon_parity_symbols():
    """Cross-check with the independent code kernel: systematic parity = (message x^(n-k)) mod g over GF(2^8)."""
    GF = ga.GF(2**8)
    rs = ga.ReedSolomon(255, 223)
    msg = GF.Random((300, 223), seed=3)
    msg[1] = GF.Zeros(223)
    a = torch.zeros((300, 255), dtype=torch.uint8, device=msg._t.device)
    a[:, :223] = msg._t
    g = GF(rs.generator_poly.coeffs)
    Q, R = ga.poly_divmod_batched(GF._wrap(a, np.uint8), g)
    assert torch.equal(R._t, rs.encode(msg, output="parity")._t) and tuple(Q.shape) == (300, 223)
