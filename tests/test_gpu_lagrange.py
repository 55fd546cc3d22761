"""lagrange_poly, lagrange_poly_batched, crt and the entry point gfa_poly_lagrange (galois_amd/csrc/gfa_lagrange.hip): the reference's
Sage vectors (tests/golden/sage_lagrange.npz), and for the sizes without a vector the completeness check -- a polynomial of degree
< k is determined by its k values, so k coefficients whose evaluation BY THE CPU ORACLE at the k abscissae gives the k ordinates
are the right ones -- over one field per arithmetic policy, at every size where the kernel changes its shape.  Everything is exact."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import galois_amd as ga
from galois_amd import _lagrange as LG
from galois_amd import _lib as L
from oracle import gf_oracle as O
from tests import helpers as H

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(H.GOLDEN, "sage_lagrange.npz")
_PROPS = {k.split("/")[1]: json.loads(str(v)) for k, v in np.load(GOLDEN).items() if k.endswith("/properties")}
TAGS = sorted(_PROPS)
PACK_THREADS = 256  # LG_PACK_THREADS: rows of up to this many points share a workgroup of this many threads
P33 = 2**32 + 15  # a prime above 2^32 (Montgomery policy)


@functools.lru_cache(maxsize=None)
def _golden():
    d = np.load(GOLDEN)
    return {k: d[k] for k in d.keys()}


def _lists(key):
    """The entries of a packed list of lists; None for an entry stored with length -1."""
    g = _golden()
    flat, out, at = [int(v) for v in g[key]], [], 0
    for n in g[key + "_len"]:
        out.append(None if n < 0 else flat[at:at + n])
        at += max(int(n), 0)
    return out


def _sage_field(tag):
    props = _PROPS[tag]
    p, m = props["characteristic"], props["degree"]
    if m == 1:
        return ga.GF(p, primitive_element=int(props["primitive_element"]))
    return ga.GF(p, m, irreducible_poly=[int(c) for c in props["irreducible_poly"]], primitive_element=int(props["primitive_element"]))


def _arr(GF, a):
    return GF(np.array(a, dtype=object))


def _poly(GF, c):
    return ga.Poly(_arr(GF, [int(v) for v in c]))


def _ints(a):
    return np.array(a.numpy(), dtype=object).astype(np.uint64)


class _calculate:
    """The field pinned to explicit arithmetic for the length of a test (GF(2^8) then runs on Bin, GF(7^3) on ExtP<3>)."""

    def __init__(self, GF, on):
        self.GF, self.on = GF, on

    def __enter__(self):
        if self.on:
            self.GF.compile("jit-calculate")
        return self.GF

    def __exit__(self, *exc):
        if self.on:
            self.GF.compile("auto")


@functools.lru_cache(maxsize=None)
def _oracle(order):
    GF = ga.GF(order)
    m = GF.degree
    return O.OracleField(GF.characteristic, m, int(GF.irreducible_poly) if m > 1 else None, GF._primitive_element_int)


def _points(order, batch, k, seed):
    """(x, y) as uint64 (batch, k): every row of x distinct, holding 0 and q - 1 where there is room; y random."""
    rng = np.random.default_rng(seed)
    if order <= 2**20:
        x = np.stack([rng.permutation(order)[:k] for _ in range(batch)]).astype(np.uint64)
    else:
        while True:
            x = rng.integers(0, order, (batch, k), dtype=np.uint64)
            if k >= 2:
                x[:, 0], x[:, k - 1] = 0, order - 1
            s = np.sort(x, axis=1)
            if not (s[:, 1:] == s[:, :-1]).any():
                break
    y = rng.integers(0, order, (batch, k), dtype=np.uint64)
    return x, y


def _complete(order, x, y, coeffs):
    """Row by row: k coefficients that the oracle evaluates to y at x."""
    F = _oracle(order)
    c = _ints(coeffs)
    assert c.shape == y.shape, f"{c.shape} coefficients for {y.shape} ordinates"
    for r in range(y.shape[0]):
        got = F.poly_eval(c[r], x[r if x.shape[0] > 1 else 0])
        assert np.array_equal(got, y[r]), f"GF({order}), k = {y.shape[1]}, row {r} of {y.shape[0]}: L(x) != y at {np.flatnonzero(got != y[r])[:8]}"
    return True


def _interpolate_checked(order, batch, k, seed, method=None, calculate=False):
    with _calculate(ga.GF(order), calculate) as GF:
        x, y = _points(order, batch, k, seed)
        C = ga.lagrange_poly_batched(_arr(GF, x), _arr(GF, y), method=method)
        assert type(C) is GF and tuple(C.shape) == (batch, k)
        _complete(order, x, y, C)
        return x, y, C


# ---- 1. the reference's vectors ---------------------------------------------------------------------------------------------------------
def test_all_sage_folders_present():
    assert len(TAGS) == 16 and sum(_PROPS[t]["order"] >= 2**64 for t in TAGS) == 3
    for t in TAGS:
        assert len(_lists(f"sage/{t}/LX")) == len(_lists(f"sage/{t}/LY")) == len(_lists(f"sage/{t}/LZ")) == 3
        assert len(_lists(f"sage/{t}/CZ")) == 20 and int(_golden()[f"sage/{t}/CN"].sum()) == len(_lists(f"sage/{t}/CX")) == len(_lists(f"sage/{t}/CY"))
    assert any(z is None for t in TAGS for z in _lists(f"sage/{t}/CZ"))


@pytest.mark.parametrize("tag", TAGS)
def test_sage_lagrange_poly(tag):
    GF = _sage_field(tag)
    for x, y, z in zip(_lists(f"sage/{tag}/LX"), _lists(f"sage/{tag}/LY"), _lists(f"sage/{tag}/LZ")):
        poly = ga.lagrange_poly(_arr(GF, x), _arr(GF, y))
        assert type(poly) is ga.Poly and poly.field is GF and type(poly.coeffs) is GF
        assert poly == _poly(GF, z), f"{tag}: through {x}, {y}"
        if not GF._limbed:  # and the whole-array route gives the same polynomial
            assert ga.lagrange_poly(_arr(GF, x), _arr(GF, y), method="arrays") == poly


def _crt_params():
    out = []
    for tag in TAGS:  # fields of order >= 2^64: host loops on limb kernels, a few systems at a time keep a case at a few seconds
        step = 5 if _PROPS[tag]["order"] >= 2**64 else 20
        out += [(tag, lo, lo + step) for lo in range(0, 20, step)]
    return out


@pytest.mark.parametrize("tag,lo,hi", _crt_params())
def test_sage_crt(tag, lo, hi):
    GF = _sage_field(tag)
    n = [int(v) for v in _golden()[f"sage/{tag}/CN"]]
    X, Y, Z = _lists(f"sage/{tag}/CX"), _lists(f"sage/{tag}/CY"), _lists(f"sage/{tag}/CZ")
    ends = np.cumsum(n)
    for i in range(lo, hi):
        a = [_poly(GF, c) for c in X[ends[i] - n[i]:ends[i]]]
        m = [_poly(GF, c) for c in Y[ends[i] - n[i]:ends[i]]]
        if Z[i] is None:
            with pytest.raises(ValueError):
                ga.crt(a, m)
        else:
            z = ga.crt(a, m)
            assert isinstance(z, ga.Poly) and z.field is GF and type(z.coeffs) is GF
            assert z == _poly(GF, Z[i]), f"{tag}: system {i}"


# ---- 2. completeness over one field per policy ------------------------------------------------------------------------------------------
# (order, pinned to explicit arithmetic): Lut and Bin on GF(2^8), Lut on GF(3^5) and GF(7^3), Prime32, Bin on 32 bits, Prime64,
# Goldilocks, ExtP<3>
POLICIES = [(2**8, False), (2**8, True), (3**5, False), (7**3, False), (65537, False), (2**31 - 1, False), (2**32, False), (P33, False),
            (H.GOLDILOCKS, False), (7**3, True)]


@pytest.mark.parametrize("order,calculate", POLICIES, ids=lambda v: str(v))
def test_every_policy_interpolates_at_the_wavefront_edges(order, calculate):
    for k in (1, 2, 63, 64, 65):
        _interpolate_checked(order, 3, k, 1000 + k, calculate=calculate)


def _team(k):
    t = 1
    while t < k:
        t *= 2
    return t


# either side of every step of the team size (a power of two up to PACK_THREADS), of the packing limit, and of one coefficient
# per thread (1024)
SHAPE_KS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 128, 129, 255, 256, 257, 1023, 1024, 1025]


@pytest.mark.parametrize("k", SHAPE_KS)
def test_team_sizes_and_partly_filled_workgroups(k):
    rows = PACK_THREADS // _team(k) if k <= PACK_THREADS else 1
    for batch in sorted({1, max(rows - 1, 1), rows + 1}):
        _interpolate_checked(65537, batch, k, 2000 + k, method="kernel")
    _interpolate_checked(H.GOLDILOCKS, rows + 1, k, 3000 + k, method="kernel")  # 64-bit elements in LDS


@pytest.mark.parametrize("order", [5, 2**8])
def test_all_elements_of_the_field_as_abscissae(order):
    x, y, C = _interpolate_checked(order, 2, order, 7)
    assert sorted(int(v) for v in x[0]) == list(range(order))


@pytest.mark.parametrize("order", [65537, H.GOLDILOCKS], ids=["32-bit", "64-bit"])
def test_largest_point_count_the_kernel_serves(order):
    GF = ga.GF(order)
    cap = ga.lagrange_max_points(GF)
    assert cap == (6399 if order == 65537 else 3199)
    _interpolate_checked(order, 1, cap, 11, method="kernel")
    x, y = _points(order, 1, cap + 1, 12)
    with pytest.raises(NotImplementedError, match=str(cap)):
        ga.lagrange_poly_batched(_arr(GF, x), _arr(GF, y), method="kernel")


def test_one_point_above_the_cap_takes_the_whole_array_route():
    GF = ga.GF(H.GOLDILOCKS)
    k = ga.lagrange_max_points(GF) + 1
    x, y = _points(H.GOLDILOCKS, 1, k, 13)
    poly = ga.lagrange_poly(_arr(GF, x[0]), _arr(GF, y[0]))
    c = _ints(poly.coeffs)
    assert c.size <= k
    assert np.array_equal(_oracle(H.GOLDILOCKS).poly_eval(c, x[0]), y[0])


@pytest.mark.parametrize("order", [2**8, 65537, P33])
def test_the_routes_agree(order):
    GF = ga.GF(order)
    for k in (1, 5, 65):
        x, y = _points(order, 4, k, 17 + k)
        X, Y = _arr(GF, x), _arr(GF, y)
        want = ga.lagrange_poly_batched(X, Y, method="kernel")
        _complete(order, x, y, want)
        assert np.array_equal(ga.lagrange_poly_batched(X, Y, method="arrays"), want)
        assert np.array_equal(ga.lagrange_poly_batched(X[0], Y, method="arrays"), ga.lagrange_poly_batched(X[0], Y, method="kernel"))


# ---- 3. the batched form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [2**8, 65537, H.GOLDILOCKS])
def test_batched_rows_are_lagrange_poly_of_each_row(order):
    GF = ga.GF(order)
    batch, k = 5, 7
    x, y = _points(order, batch, k, 23)
    X, Y = _arr(GF, x), _arr(GF, y)
    own, shared = ga.lagrange_poly_batched(X, Y), ga.lagrange_poly_batched(X[0], Y)
    assert tuple(own.shape) == tuple(shared.shape) == (batch, k)
    for r in range(batch):
        assert ga.Poly(own[r]) == ga.lagrange_poly(X[r], Y[r])
        assert ga.Poly(shared[r]) == ga.lagrange_poly(X[0], Y[r])
    _complete(order, x[:1], y, shared)


@pytest.mark.parametrize("order", [2**8, 65537, P33])
def test_matmul_route_equals_the_direct_route_at_as_many_rows_as_points(order):
    GF = ga.GF(order)
    k = 9
    for batch in (k - 1, k, k + 1):
        x, y = _points(order, batch, k, 29 + batch)
        X, Y = _arr(GF, x[0]), _arr(GF, y)
        direct = ga.lagrange_poly_batched(X, Y, method="kernel")
        _complete(order, x[:1], y, direct)
        assert np.array_equal(ga.lagrange_poly_batched(X, Y, method="matmul"), direct)
        assert np.array_equal(ga.lagrange_poly_batched(X, Y), direct)


def test_default_route_either_side_of_the_measured_matmul_rule():
    GF = ga.GF(65537)
    k = 16
    assert LG.MATMUL_MIN_ROWS_PER_POINT * k <= 2**16 - 1 and 2**16 * k * k == LG.MATMUL_MIN_WORK
    rng = np.random.default_rng(37)
    x = np.sort(rng.permutation(65537)[:k]).astype(np.uint64)[None, :]
    for batch, route in ((2**16 - 1, "kernel"), (2**16, "matmul")):
        assert LG._route(GF, True, batch, k) == route and LG._route(GF, False, batch, k) == "kernel"
        y = rng.integers(0, 65537, (batch, k), dtype=np.uint64)
        X, Y = GF(x[0]), GF(y)
        C = ga.lagrange_poly_batched(X, Y)
        assert np.array_equal(C, ga.lagrange_poly_batched(X, Y, method="kernel" if route == "matmul" else "matmul"))
        rows = [0, 1, batch // 2, batch - 1]
        _complete(65537, x, y[rows], C[rows])


def test_repeated_x_in_a_middle_row():
    GF = ga.GF(65537)
    batch, k = 5, 6
    x, y = _points(65537, batch, k, 31)
    x[2, 4] = x[2, 1]
    dev = torch.device("cuda")
    xt, yt = torch.tensor(x.astype(np.int64), dtype=torch.int32, device=dev), torch.tensor(y.astype(np.int64), dtype=torch.int32, device=dev)
    coeffs, status = LG._lagrange_t(GF, xt, yt)
    assert status.cpu().tolist() == [0, 0, 1, 0, 0]
    c = coeffs.cpu().numpy().astype(np.uint64)
    assert not c[2].any()
    keep = [0, 1, 3, 4]
    _complete(65537, x[keep], y[keep], _arr(GF, c[keep]))
    for method in (None, "kernel", "arrays"):
        with pytest.raises(ValueError, match="row 2"):
            ga.lagrange_poly_batched(_arr(GF, x), _arr(GF, y), method=method)
    for method in ("kernel", "matmul", "arrays"):  # a shared x with a repeat spoils every row: the first is named
        with pytest.raises(ValueError, match="row 0"):
            ga.lagrange_poly_batched(_arr(GF, x[2]), _arr(GF, y), method=method)
    for method in (None, "arrays"):
        with pytest.raises(ValueError, match="unique"):
            ga.lagrange_poly(_arr(GF, x[2]), _arr(GF, y[2]), method=method)


@pytest.mark.parametrize("order", [2**8, 65537, 2**100])
def test_zero_and_constant_ordinates(order):
    GF = ga.GF(order)
    k = 6
    x = _arr(GF, [3, 0, 7, 1, 200, 50])
    assert ga.lagrange_poly(x, GF.Zeros(k)) == _poly(GF, [0])
    const = ga.lagrange_poly(x, _arr(GF, [77] * k))
    assert const.degree == 0 and const == _poly(GF, [77])
    line = ga.lagrange_poly(x[:2], x[:2] + _arr(GF, [2, 2]))  # through (3, 3 + 2) and (0, 2): x + 2
    assert line == _poly(GF, [1, 2])
    rows = ga.lagrange_poly_batched(x, np.concatenate([GF.Zeros((1, k)), _arr(GF, [[77] * k])], axis=0))
    assert [int(v) for v in rows.numpy().ravel()] == [0] * (2 * k - 1) + [77]
    assert ga.lagrange_poly(GF.Zeros(0), GF.Zeros(0)) == _poly(GF, [0])


# ---- 4. crt ------------------------------------------------------------------------------------------------------------------------------
def test_crt_of_polynomials_over_gf7():
    GF = ga.GF(7)
    truth = _poly(GF, [3, 0, 6, 2, 1, 5, 4])
    m = [_poly(GF, [1, 2, 0, 3]), _poly(GF, [2, 0, 1, 1, 6]), _poly(GF, [1, 0, 0, 3, 0, 1])]
    a = [truth % mi for mi in m]
    x = ga.crt(a, m)
    assert isinstance(x, ga.Poly) and x.field is GF
    assert all(x % mi == ai for mi, ai in zip(m, a))
    if ga.lcm(*m).degree > truth.degree:
        assert x == truth


def test_crt_of_integers():
    assert ga.crt([0, 3, 4], [3, 4, 5]) == 39
    assert ga.crt((np.int64(2), 3), (5, np.int64(7))) == 17
    x = ga.crt([2, 8], [6, 9])  # gcd 3 and 2 = 8 (mod 3): solvable modulo lcm = 18
    assert x == 8 and x % 6 == 2 and x % 9 == 8
    with pytest.raises(ValueError):
        ga.crt([0, 3, 4], [3, 4, 6])
    big = ga.crt([12345678901234567890, 5], [2**89 - 1, 2**61 - 1])
    assert big % (2**89 - 1) == 12345678901234567890 and big % (2**61 - 1) == 5 and 0 <= big < (2**89 - 1) * (2**61 - 1)


@pytest.mark.parametrize("order", [7, 2**8, 65537, 2**100])
def test_crt_with_linear_moduli_is_interpolation_and_agrees_with_the_fold(order):
    GF = ga.GF(order)
    roots, values = [3, 0, 5, 1, 6], [4, 4, 1, 0, 2]
    m = [ga.Poly(np.concatenate([GF.Ones(1), -_arr(GF, [r])])) for r in roots]
    a = [_poly(GF, [v]) for v in values]
    x = ga.crt(a, m)
    assert x == LG._crt_fold(a, m) and x == ga.lagrange_poly(_arr(GF, roots), _arr(GF, values))
    assert [int(v) for v in x(_arr(GF, roots)).numpy()] == values
    # a repeated modulus is no interpolation problem: the fold decides (equal residues: solvable; different: not)
    assert ga.crt(a + [a[0]], m + [m[0]]) == x
    with pytest.raises(ValueError):
        ga.crt(a + [_poly(GF, [int(values[0]) ^ 1])], m + [m[0]])
    # a modulus that is not monic is left to the fold as well
    two = m[:1] + [_poly(GF, [1, 1, 1])]
    y = ga.crt(a[:2], two)
    assert y % two[0] == a[0] and y % two[1] == a[1]


def test_lagrange_poly_exceptions():
    GF = ga.GF(251)
    x, y = GF([0, 1, 2, 3]), GF([100, 101, 102, 103])
    with pytest.raises(TypeError):
        ga.lagrange_poly(x.numpy(), y)
    with pytest.raises(TypeError):
        ga.lagrange_poly(x, y.numpy())
    with pytest.raises(TypeError):
        ga.lagrange_poly(x, ga.GF(2**8)(y.numpy()))
    with pytest.raises(ValueError):
        ga.lagrange_poly(x.reshape((2, 2)), y)
    with pytest.raises(ValueError):
        ga.lagrange_poly(x, y.reshape((2, 2)))
    with pytest.raises(ValueError):
        ga.lagrange_poly(x, np.append(y, 104))
    with pytest.raises(ValueError):
        ga.lagrange_poly(GF([0, 1, 2, 0]), y)
    with pytest.raises(ValueError):
        ga.lagrange_poly(x, y, method="fast")
    with pytest.raises(TypeError):
        ga.lagrange_poly_batched(x, y.numpy().reshape(1, 4))
    with pytest.raises(ValueError):
        ga.lagrange_poly_batched(x, y)
    with pytest.raises(ValueError):
        ga.lagrange_poly_batched(x[:3], y.reshape(1, 4))
    with pytest.raises(ValueError):
        ga.lagrange_poly_batched(x.reshape(2, 2), y.reshape(1, 4))
    assert tuple(ga.lagrange_poly_batched(x, GF.Zeros((0, 4))).shape) == (0, 4)


def test_crt_exceptions():
    with pytest.raises(TypeError):
        ga.crt(np.array([0, 3, 4]), [3, 4, 5])
    with pytest.raises(TypeError):
        ga.crt([0, 3, 4], np.array([3, 4, 5]))
    with pytest.raises(TypeError):
        ga.crt([0, 3.0, 4], [3, 4, 5])
    with pytest.raises(TypeError):
        ga.crt([0, 3, 4], [3, 4.0, 5])
    with pytest.raises(ValueError):
        ga.crt([0, 3, 4], [3, 4, 5, 7])
    with pytest.raises(ValueError):
        ga.crt([0, 3, 4], [3, 4, 6])
    a = [ga.Poly([1, 1]), ga.Poly([1, 1, 1])]
    m = [ga.Poly([1, 0, 1]), ga.Poly([1, 1, 0, 1])]
    with pytest.raises(TypeError):
        ga.crt(np.array(a, dtype=object), m)
    with pytest.raises(TypeError):
        ga.crt(a, np.array(m, dtype=object))
    with pytest.raises(TypeError):
        ga.crt([a[0].coeffs, a[1]], m)
    with pytest.raises(TypeError):
        ga.crt(a, [m[0].coeffs, m[1]])
    with pytest.raises(ValueError):
        ga.crt(a + [ga.Poly([1, 1, 1])], m)
    with pytest.raises(ValueError):
        ga.crt(a, m + [ga.Poly([1, 1, 0, 1])])
    with pytest.raises(ValueError):  # a remainder of its modulus's degree
        ga.crt([ga.Poly([1, 1, 1]), a[1]], m)


# ---- 5. the C contract -------------------------------------------------------------------------------------------------------------------
def _call(GF, x, y, batch, npts, x_rows, c, s, dtype, handle=True):
    p = lambda t: t.data_ptr() if t is not None else None
    return L.lib().gfa_poly_lagrange(GF._handle if handle else None, p(x), p(y), batch, npts, x_rows, p(c), p(s), dtype, torch.cuda.current_stream().cuda_stream)


def test_lagrange_entry_point_contract():
    GF = ga.GF(7)
    dev = torch.device("cuda")
    x = torch.tensor([[0, 1, 2], [3, 5, 6]], dtype=torch.uint8, device=dev)
    y = torch.tensor([[1, 3, 0], [4, 4, 4]], dtype=torch.uint8, device=dev)  # x^2 + x + 1 at 0, 1, 2 over GF(7); the constant 4
    want = [1, 1, 1, 0, 0, 4]
    fill = lambda dt, n: torch.full((n,), 0x55, dtype=dt, device=dev)
    c, s = fill(torch.uint8, 6), fill(torch.int32, 2)
    assert _call(GF, x, y, 2, 3, 2, c, s, L.U8) == L.OK
    assert c.cpu().tolist() == want and s.cpu().tolist() == [0, 0]
    # shared abscissae: row 0 of x for both rows
    c1, s1 = fill(torch.uint8, 6), fill(torch.int32, 2)
    assert _call(GF, x, y, 2, 3, 1, c1, s1, L.U8) == L.OK
    assert c1.cpu().tolist() == [1, 1, 1, 0, 0, 4] and s1.cpu().tolist() == [0, 0]
    # another storage width on a non-default stream gives the same
    x64, y64, c64, s64 = x.to(torch.int64), y.to(torch.int64), fill(torch.int64, 6), fill(torch.int32, 2)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        assert L.lib().gfa_poly_lagrange(GF._handle, x64.data_ptr(), y64.data_ptr(), 2, 3, 2, c64.data_ptr(), s64.data_ptr(), L.U64, stream.cuda_stream) == L.OK
    stream.synchronize()
    assert c64.cpu().tolist() == want and s64.cpu().tolist() == [0, 0]
    # batch == 0 touches nothing, whatever the pointers
    assert _call(GF, None, None, 0, 3, 0, None, None, L.U8) == L.OK and _call(GF, None, None, 0, 3, 1, None, None, L.U8) == L.OK
    # rejected calls: no points, negative batch, x_rows that is neither, missing pointers, a dtype that cannot hold the field
    c2, s2 = fill(torch.uint8, 6), fill(torch.int32, 2)
    assert _call(GF, x, y, 2, 0, 2, c2, s2, L.U8) == L.ERR_INVALID and _call(GF, x, y, -1, 3, 1, c2, s2, L.U8) == L.ERR_INVALID
    assert _call(GF, x, y, 2, 3, 3, c2, s2, L.U8) == L.ERR_INVALID and _call(GF, x, y, 2, 3, 0, c2, s2, L.U8) == L.ERR_INVALID
    assert _call(GF, None, y, 2, 3, 2, c2, s2, L.U8) == L.ERR_INVALID and _call(GF, x, None, 2, 3, 2, c2, s2, L.U8) == L.ERR_INVALID
    assert _call(GF, x, y, 2, 3, 2, None, s2, L.U8) == L.ERR_INVALID and _call(GF, x, y, 2, 3, 2, c2, None, L.U8) == L.ERR_INVALID
    assert _call(GF, x, y, 2, 3, 2, c2, s2, 9) == L.ERR_INVALID
    assert _call(ga.GF(65537), x, y, 2, 3, 2, c2, s2, L.U8) == L.ERR_INVALID and "dtype" in L.last_error()
    # not served: more than 2^31 - 1 rows, rows above the LDS cap (named in the message), no field handle
    assert _call(GF, x, y, 2**31, 3, 1, c2, s2, L.U8) == L.ERR_UNSUPPORTED
    assert ga.lagrange_max_points(GF) == 6399
    assert _call(GF, x, y, 2, 6400, 2, c2, s2, L.U8) == L.ERR_UNSUPPORTED and "6399" in L.last_error()
    gold = ga.GF(H.GOLDILOCKS)
    assert _call(gold, x64, y64, 2, 3200, 2, c64, s64, L.U64) == L.ERR_UNSUPPORTED and "3199" in L.last_error()
    wide = ga.GF(2**100)
    assert wide._limbed and wide._handle is None
    assert _call(wide, x64, y64, 2, 3, 2, c64, s64, L.U64) == L.ERR_UNSUPPORTED and "2^64" in L.last_error()
    assert _call(GF, x, y, 2, 3, 2, c2, s2, L.U8, handle=False) == L.ERR_UNSUPPORTED
    assert c2.cpu().tolist() == [0x55] * 6 and s2.cpu().tolist() == [0x55] * 2 and c64.cpu().tolist() == want
    # no sticky error: the next call works
    assert _call(GF, x, y, 2, 3, 2, c2, s2, L.U8) == L.OK and c2.cpu().tolist() == want and s2.cpu().tolist() == [0, 0]
