"""Poly.roots, Poly.Roots, poly_roots_batched and the entry points gfa_poly_roots / gfa_poly_root_multiplicity
(galois_amd/csrc/gfa_polyroots.hip): the reference's Sage vectors (tests/golden/sage_polyroots.npz) on every route, the edges of the
search's candidate range, polynomials constructed from chosen roots, and the C contract.  Everything is exact."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import galois_amd as ga
from galois_amd import _lib as L
from galois_amd import _polyroots as PR
from tests import helpers as H

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(H.GOLDEN, "sage_polyroots.npz")
_PROPS = {k.split("/")[1]: json.loads(str(v)) for k, v in np.load(GOLDEN).items() if k.endswith("/properties")}
TAGS = sorted(_PROPS)
DTYPE = {1: L.U8, 2: L.U16, 4: L.U32, 8: L.U64}


@functools.lru_cache(maxsize=None)
def _golden():
    d = np.load(GOLDEN)
    return {k: d[k] for k in d.keys()}


def _lists(key):
    g = _golden()
    flat, ends = [int(v) for v in g[key]], np.cumsum(g[key + "_len"])
    return [flat[e - n:e] for e, n in zip(ends, g[key + "_len"])]


@functools.lru_cache(maxsize=None)
def _sage_cases(tag):
    """[(coefficients, roots, multiplicities)] of a folder."""
    X, R = _lists(f"sage/{tag}/X"), _lists(f"sage/{tag}/R")
    M, out, at = [int(v) for v in _golden()[f"sage/{tag}/M"]], [], 0
    for f, r in zip(X, R):
        out.append((f, r, M[at:at + len(r)]))
        at += len(r)
    return out


def _sage_field(tag):
    props = _PROPS[tag]
    p, m = props["characteristic"], props["degree"]
    if m == 1:
        return ga.GF(p, primitive_element=int(props["primitive_element"]))
    return ga.GF(p, m, irreducible_poly=[int(c) for c in props["irreducible_poly"]], primitive_element=int(props["primitive_element"]))


def _poly(GF, c):
    return ga.Poly(GF(np.array([int(v) for v in c], dtype=object)))


def _ints(a):
    return [int(v) for v in a.numpy().ravel()]


@functools.lru_cache(maxsize=None)
def _quadratic(order):
    """A quadratic without roots: the lexicographically last irreducible one (in characteristic 2 the first q, x^2 + c, are squares)."""
    return ga.irreducible_poly(order, 2, method="max")


def _roots_are(f, roots, mult, method=None):
    """f.roots() with and without multiplicities gives exactly these."""
    GF = f.field
    r = f.roots(method=method)
    rm, m = f.roots(multiplicity=True, method=method)
    return (type(r) is GF and type(rm) is GF and r.ndim == 1 and _ints(r) == list(roots) and _ints(rm) == list(roots) and isinstance(m, np.ndarray)
            and np.issubdtype(m.dtype, np.integer) and m.tolist() == list(mult))


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


# ---- 1. the reference's vectors ---------------------------------------------------------------------------------------------------------
def _fixture_params():
    out = []
    for tag in TAGS:
        order = _PROPS[tag]["order"]
        if order >= 2**64:  # host loops on limb kernels: one polynomial at a time keeps a case at a few seconds
            out += [(tag, method, lo, lo + 1) for method in (None, "split") for lo in range(20)]
        else:
            out += [(tag, method, 0, 20) for method in ((None, "search", "split") if order <= 2**16 else (None, "split"))]
    return out


def test_all_sage_folders_present():
    assert len(TAGS) == 16 and sum(_PROPS[t]["order"] >= 2**64 for t in TAGS) == 3 and sum(_PROPS[t]["order"] <= 2**16 for t in TAGS) == 11
    assert all(len(_sage_cases(t)) == 20 for t in TAGS)


@pytest.mark.parametrize("tag,method,lo,hi", _fixture_params(), ids=lambda v: "default" if v is None else str(v))
def test_sage_roots(tag, method, lo, hi):
    GF = _sage_field(tag)
    for f, roots, mult in _sage_cases(tag)[lo:hi]:
        assert _roots_are(_poly(GF, f), roots, mult, method), f"{tag}: roots of {f}"


# ---- 2. the search: candidate range, many hits, full rows, 64-bit indices ---------------------------------------------------------------
@pytest.mark.parametrize("order", [2, 3, 7**3, 3191, 2**8, 2**16, 65537])
def test_search_finds_roots_at_the_edges_of_the_candidate_range(order):
    """The first and the last candidate, and both sides of a wavefront's (64) and a workgroup's (256, and 1024 = 4 chains) boundary."""
    GF = ga.GF(order)
    roots = sorted({r for r in (0, 1, 63, 64, 255, 256, 1023, 1024, order - 2, order - 1) if 0 <= r < order})
    f = ga.Poly.Roots(roots, field=GF) * _quadratic(order)
    assert f.degree == len(roots) + 2
    assert _roots_are(f, roots, [1] * len(roots), "search")
    assert _roots_are(f, roots, [1] * len(roots))


@pytest.mark.parametrize("roots", [list(range(64)), list(range(1, 200))], ids=["a whole wavefront", "199 of 256"])
def test_many_hits_in_one_wavefront(roots):
    GF = ga.GF(2**8)
    f = ga.Poly.Roots(roots, field=GF)
    assert _roots_are(f, roots, [1] * len(roots), "search")
    assert _roots_are(f, roots, [1] * len(roots), "split")


@pytest.mark.parametrize("order", [7**3, 2**8])
def test_capacity_exactly_full(order):
    """x^q - x: q roots in q slots."""
    GF = ga.GF(order)
    c = [0] * (order + 1)
    c[0], c[order - 1] = 1, int(-GF(1))
    f = _poly(GF, c)
    assert _roots_are(f, range(order), [1] * order, "search")
    x = ga.Poly(GF([1, 0]))
    assert _roots_are(f * x, range(order), [2] + [1] * (order - 1), "search")  # a slot to spare, and a double root at 0


@pytest.mark.parametrize("order,roots", [(2**31 - 1, [1, 2**30, 2**31 - 2]), (2**32, [2**31 - 1, 2**31, 2**32 - 1])], ids=["GF(2^31-1)", "GF(2^32)"])
def test_search_indexes_candidates_with_64_bits(order, roots):
    GF = ga.GF(order)
    f = ga.Poly.Roots(roots, field=GF)
    assert _roots_are(f, roots, [1, 1, 1], "search")


# ---- 3. multiplicities -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["search", "split"])
def test_multiplicities_of_the_documented_examples(method):
    f = ga.Poly.Roots([1, 0], [7, 3])
    assert f.field is ga.GF(2) and f.degree == 10 and _roots_are(f, [0, 1], [3, 7], method)
    GF = ga.GF(3**5)
    f = ga.Poly.Roots([18, 227, 153], [5, 7, 3], field=GF)
    assert f.degree == 15 and _roots_are(f, [18, 153, 227], [5, 3, 7], method)


@pytest.mark.parametrize("method", ["search", "split"])
def test_multiplicities_around_the_characteristic(method):
    GF = ga.GF(5)
    f = ga.Poly.Roots([1, 2, 4], [5, 6, 10], field=GF) * _quadratic(5)  # p, p + 1 and 2 p
    assert f.degree == 23 and _roots_are(f, [1, 2, 4], [5, 6, 10], method)
    assert _roots_are(ga.Poly.Roots([3], [4], field=GF), [3], [4], method)  # p - 1, and nothing left of the quotient


@pytest.mark.parametrize("order", [H.GOLDILOCKS, 2**61 - 1])
def test_multiplicities_over_fields_too_large_to_search(order):
    """Goldilocks and Prime64: the split route, multiplicities from the finishing kernel."""
    GF = ga.GF(order)
    roots, mult = [3, order // 3, order - 2], [2, 1, 3]
    f = ga.Poly.Roots(roots, mult, field=GF) * _poly(GF, [5])
    assert _roots_are(f, roots, mult)
    assert PR._root_multiplicity(f, GF(np.array([order - 2, 4, 3], dtype=object))).tolist() == [3, 0, 2]
    with pytest.raises(NotImplementedError, match="2\\^42"):
        f.roots(method="search")


# ---- 4. the two routes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["GF(2^8)", "GF(2^8) calculate", "GF(7^3)", "GF(7^3) calculate", "GF(3191)", "GF(2^16)", "GF(2^20)"])
def test_routes_agree_on_constructed_products(name):
    order = {"GF(2^8)": 2**8, "GF(7^3)": 7**3, "GF(3191)": 3191, "GF(2^16)": 2**16, "GF(2^20)": 2**20}[name.split(" ")[0]]
    rng = np.random.default_rng(order)
    cofactor = _quadratic(order)
    with _calculate(ga.GF(order), name.endswith("calculate")) as GF:
        for k in (1, 2, 5, 12):
            roots = sorted(int(r) for r in rng.choice(order, size=k, replace=False))
            mult = [int(m) for m in rng.integers(1, 4, size=k)]
            f = ga.Poly.Roots(roots, mult, field=GF) * cofactor * _poly(GF, [int(rng.integers(1, order))])
            assert _roots_are(f, roots, mult, "search"), f"{name}: search, {k} roots"
            assert _roots_are(f, roots, mult, "split"), f"{name}: split, {k} roots"
        assert _roots_are(cofactor, [], [], "search") and _roots_are(cofactor, [], [], "split")


def test_default_route_follows_the_work_constant():
    assert PR.SEARCH_MAX_WORK & (PR.SEARCH_MAX_WORK - 1) == 0  # a power of two
    GF = ga.GF(2**8)
    assert PR._search_serves(GF, 11) and 2**8 * 10 <= PR.SEARCH_MAX_WORK  # (the fixtures' default route over GF(2^8) is the search)
    assert not PR._search_serves(ga.GF(2**100), 3) and not PR._search_serves(GF, ga.roots_max_terms(GF) + 1)
    assert ga.roots_max_terms(GF) == 150 * 1024 // 4 // 4 and ga.roots_max_terms(ga.GF(2**32)) == 150 * 1024 // 8 // 4


# ---- 5. stacks and the C entry points ---------------------------------------------------------------------------------------------------
def _stack_rows(GF, order):
    """Six rows of five coefficients with different degrees, and what their roots are: a full row, a double root behind leading zeros,
    a constant, the zero row, a row without roots, a cubic with one root."""
    quad = _quadratic(order)
    full = sorted({0, 1, order - 1, order // 2, 2})[:4]
    a = order - 2
    polys = [ga.Poly.Roots(full, field=GF), ga.Poly.Roots([a], [2], field=GF) * _poly(GF, [order - 1]), _poly(GF, [3 % order or 1]), None, quad,
             ga.Poly.Roots([1], field=GF) * quad]
    rows = [[0] * (5 - (p.degree + 1)) + _ints(p.coeffs) if p is not None else [0] * 5 for p in polys]
    expected = [(full, [1] * 4), ([a], [2]), ([], []), None, ([], []), ([1], [1])]
    return rows, expected


def _expected_arrays(expected, cap):
    roots = [(e[0] if e else []) + [0] * (cap - len(e[0] if e else [])) for e in expected]
    mult = [(e[1] if e else []) + [0] * (cap - len(e[1] if e else [])) for e in expected]
    counts = [len(e[0]) if e is not None else -1 for e in expected]
    return roots, counts, mult


@pytest.mark.parametrize("name", ["GF(5)", "GF(2^8)", "GF(2^8) calculate", "GF(7^3)", "GF(7^3) calculate", "GF(65537)", "GF(2^20)"])
def test_stack_of_rows_in_every_storage_width(name):
    order = {"GF(5)": 5, "GF(2^8)": 2**8, "GF(7^3)": 7**3, "GF(65537)": 65537, "GF(2^20)": 2**20}[name.split(" ")[0]]
    with _calculate(ga.GF(order), name.endswith("calculate")) as GF:
        rows, expected = _stack_rows(GF, order)
        want_r, want_n, want_m = _expected_arrays(expected, 4)
        assert len(GF.dtypes) >= 2
        for dt in GF.dtypes:
            A = GF(np.array(rows, dtype=object), dtype=dt)
            keep = A._t.clone()
            R, N, M = ga.poly_roots_batched(A, multiplicity=True)
            assert type(R) is GF and R.dtype == A.dtype and tuple(R.shape) == (6, 4) and N.dtype == np.int64 and M.dtype == np.int32
            assert R.numpy().tolist() == want_r and N.tolist() == want_n and M.tolist() == want_m, f"{name} {dt}"
            R2, N2 = ga.poly_roots_batched(A)
            assert torch.equal(R2._t, R._t) and N2.tolist() == want_n and torch.equal(A._t, keep)
            # the entry point itself, on buffers with sentinels behind them, with and without mult_out
            t = A._t
            fill = 0x55
            for with_mult in (True, False):
                r_out = torch.full((6 * 4 + 8,), fill, dtype=t.dtype, device=t.device)
                m_out = torch.full((6 * 4 + 8,), fill, dtype=torch.int32, device=t.device)
                n_out = torch.full((6 + 2,), fill, dtype=torch.int64, device=t.device)
                rc = L.lib().gfa_poly_roots(GF._handle, t.data_ptr(), 6, 5, r_out.data_ptr(), m_out.data_ptr() if with_mult else None, n_out.data_ptr(),
                                            DTYPE[t.element_size()], torch.cuda.current_stream().cuda_stream)
                assert rc == L.OK, L.last_error()
                assert torch.equal(r_out[:24].reshape(6, 4), R._t) and r_out[24:].cpu().tolist() == [fill] * 8
                assert n_out.cpu().tolist() == want_n + [fill] * 2
                assert m_out.cpu().tolist() == ([v for row in want_m for v in row] if with_mult else [fill] * 24) + [fill] * 8
            # a single row
            R1, N1, M1 = ga.poly_roots_batched(A[1:2], multiplicity=True)
            assert R1.numpy().tolist() == want_r[1:2] and N1.tolist() == want_n[1:2] and M1.tolist() == want_m[1:2]


def test_a_thousand_short_rows():
    GF = ga.GF(2**8)
    rng = np.random.default_rng(1000)
    abc = rng.integers(0, 256, size=(1000, 3))
    abc[:50, 1] = abc[:50, 0]  # double roots
    abc[50:60, 2] = abc[50:60, 1] = abc[50:60, 0]  # triple roots
    a, b, c = (GF(abc[:, k].astype(np.uint8)) for k in range(3))
    # (x - a)(x - b)(x - c) in characteristic 2
    A = GF.Zeros((1000, 4))
    A[:, 0] = GF.Ones(1000)
    A[:, 1] = a + b + c
    A[:, 2] = a * b + a * c + b * c
    A[:, 3] = a * b * c
    R, N, M = ga.poly_roots_batched(A, multiplicity=True)
    want_r, want_n, want_m = np.zeros((1000, 3), dtype=np.int64), np.zeros(1000, dtype=np.int64), np.zeros((1000, 3), dtype=np.int64)
    for k in range(1000):
        values, counts = np.unique(abc[k], return_counts=True)
        want_n[k] = len(values)
        want_r[k, :len(values)], want_m[k, :len(values)] = values, counts
    assert np.array_equal(R.numpy().astype(np.int64), want_r) and np.array_equal(N, want_n) and np.array_equal(M, want_m)
    assert want_n.min() == 1 and want_n.max() == 3


def test_batched_form_over_a_field_of_order_above_2_64_and_its_argument_checks():
    GF = ga.GF(2**100)
    f = ga.Poly.Roots([2**99 + 1, 7], [2, 1], field=GF)
    A = GF(np.array([_ints(f.coeffs), [0, 0, 0, 5], [0, 0, 0, 0]], dtype=object))
    R, N, M = ga.poly_roots_batched(A, multiplicity=True)
    assert type(R) is GF and tuple(R.shape) == (3, 3) and N.tolist() == [2, 0, -1]
    assert [int(v) for v in R.numpy().ravel()] == [7, 2**99 + 1, 0, 0, 0, 0, 0, 0, 0] and M.tolist() == [[1, 2, 0], [0, 0, 0], [0, 0, 0]]
    small = ga.GF(7)
    with pytest.raises(TypeError):
        ga.poly_roots_batched([[1, 2]])
    with pytest.raises(ValueError):
        ga.poly_roots_batched(small([1, 2]))
    with pytest.raises(TypeError):
        ga.poly_roots_batched(small([[1, 2]]), multiplicity=1)
    R, N = ga.poly_roots_batched(small([[3], [0]]))  # constants only: no room for roots
    assert tuple(R.shape) == (2, 0) and N.tolist() == [0, -1]


def _call_roots(GF, c, batch, ncoef, r, m, n, dtype, handle=True):
    p = lambda t: t.data_ptr() if t is not None else None
    return L.lib().gfa_poly_roots(GF._handle if handle else None, p(c), batch, ncoef, p(r), p(m), p(n), dtype, torch.cuda.current_stream().cuda_stream)


def test_roots_entry_point_contract():
    GF = ga.GF(7)
    dev = torch.device("cuda")
    c = torch.tensor([[1, 0, 6], [0, 1, 4]], dtype=torch.uint8, device=dev)  # x^2 - 1 and x - 3
    fill = lambda dt, n: torch.full((n,), 0x55, dtype=dt, device=dev)
    r, m, n = fill(torch.uint8, 4), fill(torch.int32, 4), fill(torch.int64, 2)
    assert _call_roots(GF, c, 2, 3, r, m, n, L.U8) == L.OK
    assert r.cpu().tolist() == [1, 6, 3, 0] and m.cpu().tolist() == [1, 1, 1, 0] and n.cpu().tolist() == [2, 1]
    # another storage width on a non-default stream gives the same
    c64, r64, n64 = c.to(torch.int64), fill(torch.int64, 4), fill(torch.int64, 2)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        assert L.lib().gfa_poly_roots(GF._handle, c64.data_ptr(), 2, 3, r64.data_ptr(), None, n64.data_ptr(), L.U64, stream.cuda_stream) == L.OK
    stream.synchronize()
    assert r64.cpu().tolist() == [1, 6, 3, 0] and n64.cpu().tolist() == [2, 1]
    # batch == 0 touches nothing, whatever the pointers
    assert _call_roots(GF, None, 0, 3, None, None, None, L.U8) == L.OK
    # rejected calls: rows without room for a root, negative batch, missing pointers, a dtype that cannot hold the field
    r2, n2 = fill(torch.uint8, 4), fill(torch.int64, 2)
    assert _call_roots(GF, c, 2, 1, r2, None, n2, L.U8) == L.ERR_INVALID and _call_roots(GF, c, -1, 3, r2, None, n2, L.U8) == L.ERR_INVALID
    assert _call_roots(GF, None, 2, 3, r2, None, n2, L.U8) == L.ERR_INVALID and _call_roots(GF, c, 2, 3, None, None, n2, L.U8) == L.ERR_INVALID
    assert _call_roots(GF, c, 2, 3, r2, None, None, L.U8) == L.ERR_INVALID and _call_roots(GF, c, 2, 3, r2, None, n2, 9) == L.ERR_INVALID
    assert _call_roots(ga.GF(65537), c, 2, 3, r2, None, n2, L.U8) == L.ERR_INVALID and "dtype" in L.last_error()
    # not served: more than 2^31 - 1 rows or coefficients, rows above the LDS cap, a search of more than 2^42 steps, no field handle
    assert _call_roots(GF, c, 2**31, 3, r2, None, n2, L.U8) == L.ERR_UNSUPPORTED and _call_roots(GF, c, 2, 2**31, r2, None, n2, L.U8) == L.ERR_UNSUPPORTED
    assert _call_roots(GF, c, 2, ga.roots_max_terms(GF) + 1, r2, None, n2, L.U8) == L.ERR_UNSUPPORTED and "9600" in L.last_error()
    big = ga.GF(2**61 - 1)
    assert _call_roots(big, c64, 2, 3, r64, None, n64, L.U64) == L.ERR_UNSUPPORTED and "2^42" in L.last_error()
    wide = ga.GF(2**100)
    assert wide._limbed and wide._handle is None
    assert _call_roots(wide, c64, 2, 3, r64, None, n64, L.U64) == L.ERR_UNSUPPORTED and "2^64" in L.last_error()
    assert _call_roots(GF, c, 2, 3, r2, None, n2, L.U8, handle=False) == L.ERR_UNSUPPORTED
    assert r2.cpu().tolist() == [0x55] * 4 and n2.cpu().tolist() == [0x55] * 2 and r64.cpu().tolist() == [1, 6, 3, 0]
    # no sticky error: the next call works
    assert _call_roots(GF, c, 2, 3, r2, None, n2, L.U8) == L.OK and r2.cpu().tolist() == [1, 6, 3, 0]


def test_root_multiplicity_entry_point_on_given_elements():
    GF = ga.GF(7)
    dev = torch.device("cuda")
    c = torch.tensor([[1, 5, 1], [0, 0, 0], [0, 0, 2]], dtype=torch.uint8, device=dev)  # (x - 1)^2, zero, a constant
    given = torch.tensor([[1, 1, 3, 0], [1, 2, 3, 4], [0, 1, 2, 3]], dtype=torch.uint8, device=dev)  # unsorted, repeated
    m = torch.full((12 + 4,), 0x55, dtype=torch.int32, device=dev)
    call = lambda f, nroots, out: L.lib().gfa_poly_root_multiplicity(f, c.data_ptr(), 3, 3, given.data_ptr(), nroots, out, L.U8, torch.cuda.current_stream().cuda_stream)
    assert call(GF._handle, 4, m.data_ptr()) == L.OK
    assert m.cpu().tolist() == [2, 2, 0, 0] + [0] * 8 + [0x55] * 4
    assert call(GF._handle, 0, None) == L.OK and call(GF._handle, 4, None) == L.ERR_INVALID and call(None, 4, m.data_ptr()) == L.ERR_UNSUPPORTED
    f = ga.Poly(GF([1, 5, 1]))
    assert PR._root_multiplicity(f, GF([3, 1])).tolist() == [0, 2] and PR._root_multiplicity(f, GF([1])[:0]).tolist() == []


# ---- 6. Poly.Roots ---------------------------------------------------------------------------------------------------------------------
def test_roots_constructor_exceptions():
    GF = ga.GF(2**8)
    roots, multiplicities = [134, 212], [1, 2]
    with pytest.raises(TypeError):
        ga.Poly.Roots(134, field=GF)
    with pytest.raises(TypeError, match="'field' must be a FieldArray subclass"):
        ga.Poly.Roots(roots, field="invalid-type")
    with pytest.raises(TypeError, match="'multiplicities' must be an instance of"):
        ga.Poly.Roots(roots, multiplicities=134, field=GF)
    with pytest.raises(ValueError, match="must have the same length, not 2 and 3"):
        ga.Poly.Roots(roots, multiplicities=multiplicities + [1], field=GF)


@pytest.mark.parametrize("order", [2, 5, 2**8, 3**5, 3191, 2**31 - 1, 2**32, 2**100])
def test_roots_constructor(order):
    GF = ga.GF(order)
    ab = GF.Random(2, seed=order)
    neg = -ab
    a, b = _ints(ab)
    coeffs = [1, _ints(neg[0:1] + neg[1:2])[0], _ints(neg[0:1] * neg[1:2])[0]]  # (x - a)(x - b) = x^2 + (-a + -b) x + (-a)(-b), as the reference's test
    for p in (ga.Poly.Roots([a, b], field=GF), ga.Poly.Roots(ab)):
        assert isinstance(p, ga.Poly) and p.field is GF and p.degree == 2 and _ints(p.coeffs) == coeffs
        assert int(p) == sum(c * order**d for d, c in zip((2, 1, 0), coeffs))
        assert _ints(p(ab)) == [0, 0]
    coeffs = [1, _ints(neg[0:1] + neg[0:1])[0], _ints(neg[0:1] * neg[0:1])[0]]
    for p in (ga.Poly.Roots([a], multiplicities=[2], field=GF), ga.Poly.Roots(ab[0:1], multiplicities=(2,))):
        assert p.field is GF and p.degree == 2 and _ints(p.coeffs) == coeffs


def test_roots_constructor_field_override_and_defaults():
    p = ga.Poly.Roots(ga.GF2([1, 0]))
    assert p.field is ga.GF2 and _ints(p.coeffs) == [1, 1, 0]
    GF = ga.GF(2**8)
    p = ga.Poly.Roots(ga.GF2([1, 0]), field=GF)
    assert p.field is GF and _ints(p.coeffs) == [1, 1, 0]
    p = ga.Poly.Roots([0, 0, 1])  # GF(2) by default; a repeated entry is a repeated root
    assert p.field is ga.GF2 and _ints(p.coeffs) == [1, 1, 0, 0] and _ints(p(ga.GF2([0, 0, 1]))) == [0, 0, 0]
    assert _ints(ga.Poly.Roots([], field=GF).coeffs) == [1] and _ints(ga.Poly.Roots([5], [0], field=GF).coeffs) == [1]
    assert _ints(ga.Poly.Roots([-3], field=ga.GF(7)).coeffs) == [1, 3]  # "-3" is the negative of the element 3: x - (-3)


# ---- 7. error cases --------------------------------------------------------------------------------------------------------------------
def test_roots_error_cases():
    GF = ga.GF(31)
    f = ga.Poly(GF([1, 0, 30]))
    with pytest.raises(TypeError, match="'multiplicity' must be an instance of"):
        f.roots(multiplicity=1)
    with pytest.raises(ValueError, match="'method' must be in"):
        f.roots(method="chien")
    with pytest.raises(ValueError, match="zero polynomial"):
        ga.Poly(GF([0])).roots()
    for method in (None, "search", "split"):
        r = ga.Poly(GF([4])).roots(method=method)
        assert type(r) is GF and tuple(r.shape) == (0,)
        r, m = ga.Poly(GF([4])).roots(multiplicity=True, method=method)
        assert type(r) is GF and tuple(r.shape) == (0,) and isinstance(m, np.ndarray) and m.shape == (0,)
    wide = ga.GF(2**100)
    with pytest.raises(NotImplementedError, match="2\\^64"):
        ga.Poly(wide([1, 5])).roots(method="search")
    assert _roots_are(ga.Poly(GF([3, 0, 28])), [1, 30], [1, 1])  # not monic
    assert _roots_are(ga.Poly(wide([2, 6])), [3], [1])  # 2 x + 6 = 2 (x + 3), characteristic 2
