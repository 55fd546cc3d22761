"""Poly.is_irreducible() / is_primitive(), the batched forms, irreducible_poly / irreducible_polys / primitive_polys and
gfa_poly_classify (galois_amd/csrc/gfa_polytest.hip): the reference's complete tables, its Sage vectors and its live answers
(tests/golden/reference_polytest.npz), exhaustive sweeps against the closed-form counts, the word and degree boundaries of the
two kernel regimes, the cases that separate Rabin's two conditions, cross-checks against independent kernels and the C entry
point's contract.  Everything is exact."""
import functools
import itertools
import json
import os

import numpy as np
import pytest
import torch

import galois_amd as ga
from galois_amd import _lib as L
from galois_amd import _numtheory as nt
from galois_amd import _polysearch as PS
from tests import helpers as H

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _golden():
    d = np.load(os.path.join(H.GOLDEN, "reference_polytest.npz"))
    return {k: d[k] for k in d.keys()}


def _coeffs(poly):
    return [int(v) for v in poly.coeffs.numpy()]


def _rows(a):
    return [[int(v) for v in r] for r in a]


def _terms(row):
    return sum(1 for c in row if c)


TABLES = [(int(q), int(m)) for q, m in np.load(os.path.join(H.GOLDEN, "reference_polytest.npz"))["tables"]]


# ---- 1. the reference's complete tables: search order, terms=, method= -------------------------------------------------------
@pytest.mark.parametrize("q, m", TABLES)
@pytest.mark.parametrize("kind", ["irr", "prim"])
def test_searches_reproduce_the_reference_tables(q, m, kind):
    table = _rows(_golden()[f"{kind}/{q}_{m}"])
    polys = ga.irreducible_polys if kind == "irr" else ga.primitive_polys
    got = list(polys(q, m))
    assert all(isinstance(f, ga.Poly) and f.field is ga.GF(q) for f in got)
    assert [_coeffs(f) for f in got] == table
    assert [_coeffs(f) for f in polys(q, m, reverse=True)] == table[::-1]
    if kind == "irr":
        assert _coeffs(ga.irreducible_poly(q, m)) == table[0]
        assert _coeffs(ga.irreducible_poly(q, m, method="min")) == table[0]
        assert _coeffs(ga.irreducible_poly(q, m, method="max")) == table[-1]
    min_terms = min(_terms(r) for r in table)
    for k in range(1, m + 2):
        sub = [r for r in table if _terms(r) == k]
        assert [_coeffs(f) for f in polys(q, m, terms=k)] == sub, f"terms={k}"
        if kind == "irr":
            if sub:
                assert _coeffs(ga.irreducible_poly(q, m, terms=k)) == sub[0]
                assert _coeffs(ga.irreducible_poly(q, m, terms=k, method="max")) == sub[-1]
            else:
                with pytest.raises(RuntimeError, match=f"No monic irreducible polynomial of degree {m} over GF\\({q}\\) with {k} terms exists"):
                    ga.irreducible_poly(q, m, terms=k)
    assert [_coeffs(f) for f in polys(q, m, terms="min")] == [r for r in table if _terms(r) == min_terms]
    if kind == "irr":
        assert _coeffs(ga.irreducible_poly(q, m, terms="min")) == [r for r in table if _terms(r) == min_terms][0]


def test_argument_checks_follow_the_reference():
    with pytest.raises(TypeError):
        ga.irreducible_poly(2.0, 3)
    with pytest.raises(TypeError):
        ga.irreducible_polys(2, 3, terms=2.0)
    with pytest.raises(TypeError):
        ga.primitive_polys(2, 3, reverse=1)
    with pytest.raises(ValueError, match="must be a prime power, not 6"):
        ga.irreducible_poly(6, 3)
    with pytest.raises(ValueError, match="must be at least 1, not 0. There are no irreducible polynomials with degree 0"):
        ga.irreducible_poly(2, 0)
    with pytest.raises(ValueError, match="must be at least 0, not -1"):
        ga.primitive_polys(2, -1)
    with pytest.raises(ValueError, match="must be at least 1 and at most 4, not 5"):
        ga.irreducible_poly(2, 3, terms=5)
    with pytest.raises(ValueError, match="must be 'min', not 'max'"):
        ga.irreducible_polys(2, 3, terms="max")
    with pytest.raises(ValueError, match="must be in \\['min', 'max', 'random'\\]"):
        ga.irreducible_poly(2, 3, method="first")
    assert list(ga.irreducible_polys(3, 0)) == [] and list(ga.primitive_polys(3, 0)) == []


def test_poly_int_degrees_and_int():
    GF = ga.GF(3)
    f = ga.Poly.Int(3**4 + 2 * 3 + 1, field=GF)
    assert _coeffs(f) == [1, 0, 0, 2, 1] and int(f) == 88
    assert _coeffs(ga.Poly.Int(0b100011011)) == [1, 0, 0, 0, 1, 1, 0, 1, 1] and ga.Poly.Int(5).field is ga.GF(2)
    g = ga.Poly.Degrees([8, 4, 3, 1, 0])
    assert int(g) == 0b100011011 and g.is_irreducible() and not g.is_primitive()  # the AES polynomial (_primitive.py:62-68)
    assert _coeffs(ga.Poly.Degrees([3, 1, 0], [1, 2, 2], field=GF)) == [1, 0, 2, 2]
    assert int(ga.Poly.Int(0)) == 0 and not ga.Poly.Int(0).is_irreducible() and not ga.Poly.Int(1).is_primitive()
    assert not ga.Poly([2], field=GF).is_irreducible() and not ga.Poly([2], field=GF).is_primitive()  # degree 0
    assert ga.Poly([1, 0], field=GF).is_irreducible() and not ga.Poly([1, 0], field=GF).is_primitive()  # x
    assert ga.Poly([2, 0, 2], field=GF).is_irreducible() == ga.Poly([1, 0, 1], field=GF).is_irreducible() is True  # non-monic


# ---- 2. Sage vectors ---------------------------------------------------------------------------------------------------------
def _sage_tags():
    return sorted(k.split("/")[1] for k in _golden() if k.startswith("sage/") and k.endswith("/properties"))


def _sage_field(tag):
    props = json.loads(str(_golden()[f"sage/{tag}/properties"]))
    p, m = props["characteristic"], props["degree"]
    if m == 1:
        return ga.GF(p, primitive_element=int(props["primitive_element"]))
    return ga.GF(p, m, irreducible_poly=H.poly_coeffs_to_int(props["irreducible_poly"], p), primitive_element=int(props["primitive_element"]))


def test_sage_folders_present():
    assert len(_sage_tags()) == 11
    assert {"GF_2e8", "GF_2e8_283_19", "GF_7e3", "GF_31", "GF_3191"} <= set(_sage_tags())


@pytest.mark.parametrize("tag", _sage_tags())
def test_sage_vectors(tag):
    g = _golden()
    GF = _sage_field(tag)
    for kind, method, batched in (("irr", "is_irreducible", ga.is_irreducible_batched), ("prim", "is_primitive", ga.is_primitive_batched)):
        by_degree = {}
        for name, expect in ((f"{kind}_IS", True), (f"{kind}_IS_NOT", False)):
            lens, flat = g[f"sage/{tag}/{name}_len"], [int(v) for v in g[f"sage/{tag}/{name}"]]
            assert len(lens) == 10
            ends = np.cumsum(lens)
            for i, n in enumerate(lens):
                c = flat[ends[i] - n:ends[i]]
                f = ga.Poly(GF(np.array(c, dtype=object)))
                assert getattr(f, method)() is expect, f"{tag}: {method} of {c}"
                by_degree.setdefault(f.degree, []).append((_coeffs(f), expect))
        for degree, cases in by_degree.items():
            if degree == 0:
                continue
            got = batched(GF(np.array([c for c, _ in cases], dtype=object)))
            assert got.dtype == np.bool_ and got.tolist() == [e for _, e in cases], f"{tag}: batched {method}, degree {degree}"


# ---- 3. exhaustive sweeps against the closed forms -------------------------------------------------------------------------
def _mobius(n):
    ps, es = nt.factors(n) if n > 1 else ([], [])
    return 0 if any(e > 1 for e in es) else (-1) ** len(ps)


def _count_irreducible(q, m):
    return sum(_mobius(d) * q ** (m // d) for d in range(1, m + 1) if m % d == 0) // m


def _count_primitive(q, m):
    n = q**m - 1
    phi = n
    for r in nt.factors(n)[0]:
        phi = phi // r * (r - 1)
    return phi // m


@functools.lru_cache(maxsize=None)
def _sweep(q, m):
    """Every monic polynomial of degree m over GF(q): (the candidates, irreducible flags, primitive flags), computed once."""
    GF = ga.GF(q)
    cand = GF._wrap(PS._range_tensor(GF, m, 0, q**m), PS._storage(GF)[0])
    return cand, ga.is_irreducible_batched(cand), ga.is_primitive_batched(cand)


@pytest.mark.parametrize("q, m, n_irr, n_prim", [(2, 16, 4080, 2048), (2, 20, 52377, 24000), (3, 10, 5880, 2640), (7, 5, 3360, 1120),
                                                 (2**8, 2, 32640, 16384), (31, 3, 9920, 2640)])
def test_exhaustive_sweeps_match_the_closed_form_counts(q, m, n_irr, n_prim):
    assert (_count_irreducible(q, m), _count_primitive(q, m)) == (n_irr, n_prim)
    cand, irr, prim = _sweep(q, m)
    assert cand.shape == (q**m, m + 1)
    rows = cand.numpy()
    for i in (0, 1, q, q**m - 1):  # the candidates are the integers q^m + i in radix q
        assert H.poly_coeffs_to_int(rows[i], q) == q**m + i
    assert int(irr.sum()) == n_irr and int(prim.sum()) == n_prim
    assert not np.any(prim & ~irr)


def test_prefixes_of_a_sweep_give_the_same_flags():
    cand, irr, prim = _sweep(2, 16)
    for n in (1, 63, 64, 65, 257):
        assert np.array_equal(ga.is_irreducible_batched(cand[:n]), irr[:n])
        assert np.array_equal(ga.is_primitive_batched(cand[:n]), prim[:n])


# ---- 4. word and degree boundaries -----------------------------------------------------------------------------------------
def _conway_product(p, m):
    """A product of Conway polynomials over GF(p) of total degree m (two factors when the shipped table allows it)."""
    GF = ga.GF(p)
    have = [d for d in range(1, 101) if d == 1 or (p, d) in nt._load_conway()]
    a = max(d for d in have if d <= m - 1)
    parts = [a]
    while sum(parts) < m:
        parts.append(max(d for d in have if d <= m - sum(parts)))
    f = ga.Poly.Int(nt.conway_poly(p, parts[0]), field=GF)
    for d in parts[1:]:
        f = f * ga.Poly.Int(nt.conway_poly(p, d), field=GF)
    assert f.degree == m
    return f


@pytest.mark.parametrize("m", [63, 64, 65, 127, 128, 129, 255])
def test_gf2_word_boundaries(m):
    g = _golden()
    degrees = [int(d) for d in g[f"live/min_irr_{m}"]]
    f = ga.Poly.Degrees(degrees)
    assert f.degree == m and f.is_irreducible()
    if m <= 128:
        assert f.is_primitive() is bool(g[f"live/min_irr_{m}_primitive"]) is True
    assert ga.irreducible_poly(2, m, terms="min") == f  # the reference's answer, found by the search
    h = _conway_product(2, m)
    assert not h.is_irreducible()
    if m == 127:  # 2^127 - 1 is prime: every irreducible polynomial is primitive
        assert not h.is_primitive()
        for t in (3, 5):
            cand = ga.GF(2)._wrap(PS._ints_to_tensor(ga.GF(2), m, list(itertools.islice(PS._fixed_term_ints(2, m, t), 200))), np.uint8)
            assert np.array_equal(ga.is_primitive_batched(cand), ga.is_irreducible_batched(cand))


def test_gf2_live_searches():
    g = _golden()
    assert [int(f) for f in ga.irreducible_polys(2, 24, terms=3)] == [int(v) for v in g["live/irr_2_24_terms3"]]
    assert next(ga.primitive_polys(2, 61, terms="min")) == ga.Poly.Degrees([int(d) for d in g["live/prim_2_61_min"]])


def test_extension_field_live_searches():
    g = _golden()
    assert _coeffs(ga.irreducible_poly(2**8, 3)) == [int(v) for v in g["live/irr_256_3"]]
    assert _coeffs(next(ga.primitive_polys(2**8, 2, reverse=True))) == [int(v) for v in g["live/prim_256_2_max"]]


@pytest.mark.parametrize("m", range(2, 33))
def test_gf3_every_degree(m):
    GF = ga.GF(3)
    f = ga.Poly.Int(nt.conway_poly(3, m), field=GF)
    assert f.degree == m and f.is_irreducible() and f.is_primitive()
    h = _conway_product(3, m)
    assert not h.is_irreducible() and not h.is_primitive()


def test_degrees_beyond_the_kernels_raise():
    with pytest.raises(NotImplementedError, match="255"):
        ga.Poly.Degrees([256, 1, 0]).is_irreducible()
    with pytest.raises(NotImplementedError, match="32"):
        ga.Poly.Degrees([33, 1, 0], field=ga.GF(3)).is_primitive()
    with pytest.raises(NotImplementedError):
        ga.irreducible_poly(2, 256)
    with pytest.raises(NotImplementedError):
        next(ga.primitive_polys(3, 33))


# ---- 5. the two conditions of Rabin's test -----------------------------------------------------------------------------------
def test_rabin_conditions_are_both_needed():
    """Over GF(5) at degree 12: a product of DISTINCT irreducibles whose degrees divide 12 satisfies x^(5^12) = x (mod f), so only
    the gcd step rejects it; a square, or a product with a factor degree that does not divide 12, fails that congruence."""
    GF = ga.GF(5)
    g = _golden()
    pool = {d: [ga.Poly(GF(r)) for r in g[f"irr/5_{d}"]] for d in (1, 2, 3, 4)}
    pool[6] = list(itertools.islice(ga.irreducible_polys(5, 6), 3))
    pool[5] = [ga.irreducible_poly(5, 5)]
    pool[7] = [ga.irreducible_poly(5, 7)]
    assert all(f.degree == d and f.is_irreducible() for d, fs in pool.items() for f in fs)

    def product(picks):
        f = None
        for d, i in picks:
            f = pool[d][i] if f is None else f * pool[d][i]
        assert f.degree == 12
        return f

    only_gcd = [[(6, 0), (6, 1)], [(6, 1), (6, 2)], [(4, 0), (4, 1), (3, 0), (1, 0)], [(3, 0), (3, 1), (3, 2), (2, 0), (1, 1)],
                [(4, 0), (4, 1), (4, 2)], [(6, 0), (4, 0), (2, 0)], [(6, 0), (3, 0), (2, 1), (1, 2)], [(4, 3), (3, 3), (2, 2), (1, 0), (1, 1), (1, 2)]]
    congruence = [[(6, 0), (6, 0)], [(5, 0), (7, 0)], [(4, 0), (4, 0), (4, 0)], [(5, 0), (5, 0), (2, 0)]]
    polys = [product(p) for p in only_gcd + congruence]
    for f in polys:
        assert not f.is_irreducible() and not f.is_primitive()
    stack = GF(np.array([_coeffs(f) for f in polys] + [_coeffs(ga.irreducible_poly(5, 12))]))
    assert ga.is_irreducible_batched(stack).tolist() == [False] * len(polys) + [True]


# ---- 6. cross-check with minimal polynomials and multiplicative orders ------------------------------------------------------
@pytest.mark.parametrize("p, m", [(3, 8), (2, 16)])
def test_minimal_polynomials_are_irreducible_and_primitive_by_order(p, m):
    GF = ga.GF(p**m)
    b = GF.Random(64, low=1, seed=11)
    orders = [int(v) for v in np.atleast_1d(b.multiplicative_order())]
    seen = set()
    for i in range(64):
        f = b[i].minimal_poly()
        assert f.field is GF.prime_subfield and f.is_irreducible()
        assert f.is_primitive() is (orders[i] == p**f.degree - 1)
        seen.add(f.is_primitive())
    assert seen == {True, False}


# ---- 7. method="random" -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q, m", [(2**8, 3), (65537, 2)])
def test_random_search(q, m):
    f = ga.irreducible_poly(q, m, method="random")
    assert f.field is ga.GF(q) and f.degree == m and _coeffs(f)[0] == 1 and f.is_irreducible()
    h = ga.irreducible_poly(q, m, terms=m + 1, method="random")
    assert h.degree == m and _terms(_coeffs(h)) == m + 1 and h.is_irreducible()
    k = ga.irreducible_poly(q, m, terms="min", method="random")
    assert k.degree == m and _terms(_coeffs(k)) == 2 and k.is_irreducible()  # x^m + c exists for both fields


# ---- 8. the C entry point's contract ----------------------------------------------------------------------------------------
def _call(GF, coeffs, batch, degree, dtype, flags, exps=None, n_exps=0, limbs=0, stream=None):
    return L.lib().gfa_poly_classify(GF._handle, coeffs.data_ptr() if coeffs is not None else None, batch, degree, dtype, exps, n_exps, limbs,
                                     flags.data_ptr() if flags is not None else None,
                                     torch.cuda.current_stream().cuda_stream if stream is None else stream)


def test_entry_point_contract():
    GF = ga.GF(7)
    dev = torch.device("cuda")
    n_exps, limbs, exps = PS._cofactor_exponents(7, 3)
    rows = torch.tensor([[1, 0, 1, 1], [0, 5, 1, 1], [1, 6, 0, 4], [3, 4, 0, 5], [1, 1, 0, 2], [0, 0, 0, 0], [1, 0, 0, 6]], dtype=torch.uint8, device=dev)
    keep = rows.clone()
    flags = torch.full((7,), 0x55, dtype=torch.uint8, device=dev)
    assert _call(GF, rows, 7, 3, L.U8, flags, exps, n_exps, limbs) == L.OK
    got = flags.cpu().tolist()
    assert torch.equal(rows, keep)  # the input is not modified
    assert got[1] == 0x80 and got[5] == 0x80  # not of the stated degree; the neighbours are classified as usual
    solo = torch.zeros(1, dtype=torch.uint8, device=dev)
    for i in (0, 2, 3, 4, 6):
        assert _call(GF, rows[i:i + 1].contiguous(), 1, 3, L.U8, solo, exps, n_exps, limbs) == L.OK
        assert int(solo.item()) == got[i]
    # GF(7) is not among the reference's tables: the expected flags come from the host routines of _numtheory
    expect = [int(nt.is_irreducible(r, 7)) | (2 * int(nt.is_primitive_poly(r, 7))) for r in ([1, 0, 1, 1], [1, 6, 0, 4], [1, 1, 0, 2], [1, 0, 0, 6])]
    assert [got[0], got[2], got[4], got[6]] == expect
    assert got[3] == got[2]  # 3 x^3 + 4 x^2 + 5 = 3 (x^3 + 6 x^2 + 4): a non-monic row is classified as its monic multiple
    # irreducibility only: bit 1 stays clear
    assert _call(GF, rows, 7, 3, L.U8, flags) == L.OK
    assert flags.cpu().tolist() == [v & 0x81 for v in got]
    # another storage width and a non-default stream give the same flags
    wide = rows.to(torch.int32)
    s = torch.cuda.Stream()
    f2 = torch.zeros(7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        assert _call(GF, wide, 7, 3, L.U32, f2, exps, n_exps, limbs, stream=s.cuda_stream) == L.OK
    s.synchronize()
    assert f2.cpu().tolist() == got
    # batch == 0 touches nothing, whatever the pointers
    flags.fill_(0x55)
    assert _call(GF, None, 0, 3, L.U8, None) == L.OK
    assert _call(GF, rows, 0, 3, L.U8, flags) == L.OK
    assert flags.cpu().tolist() == [0x55] * 7
    # rejected calls
    big = ga.GF(65537)
    r16 = torch.zeros((1, 4), dtype=torch.uint8, device=dev)
    assert _call(big, r16, 1, 3, L.U8, flags) == L.ERR_INVALID and "dtype" in L.last_error()
    assert _call(GF, rows, -1, 3, L.U8, flags) == L.ERR_INVALID
    assert _call(GF, rows, 7, 0, L.U8, flags) == L.ERR_INVALID
    assert _call(GF, rows, 7, 3, L.U8, None) == L.ERR_INVALID
    assert _call(GF, None, 7, 3, L.U8, flags) == L.ERR_INVALID
    assert _call(GF, rows, 7, 3, L.U8, flags, None, 2, 1) == L.ERR_INVALID
    assert _call(GF, rows, 7, 3, 9, flags) == L.ERR_INVALID
    assert _call(GF, rows, 1, 33, L.U8, flags) == L.ERR_UNSUPPORTED and "32" in L.last_error()
    assert _call(ga.GF(2), rows, 1, 256, L.U8, flags) == L.ERR_UNSUPPORTED and "255" in L.last_error()
    assert flags.cpu().tolist() == [0x55] * 7


def test_degree_one():
    """Every polynomial of degree 1 is irreducible; x + a is primitive iff -a generates the multiplicative group (over GF(2): x + 1)."""
    assert ga.is_irreducible_batched(ga.GF(2)([[1, 0], [1, 1]])).tolist() == [True, True]
    assert ga.is_primitive_batched(ga.GF(2)([[1, 0], [1, 1]])).tolist() == [False, True]
    GF = ga.GF(31)
    stack = GF(np.stack([np.ones(31, dtype=np.int64), np.arange(31)], axis=1))
    assert ga.is_irreducible_batched(stack).all()
    assert ga.is_primitive_batched(stack).tolist() == [a != 0 and nt.is_primitive_root((-a) % 31, 31) for a in range(31)]


def test_fields_of_order_2_64_and_above_raise():
    GF = ga.GF(36893488147419103183, primitive_element=3)
    f = ga.Poly(GF(np.array([1, 0, 5], dtype=object)))
    with pytest.raises(NotImplementedError, match="2\\^64"):
        f.is_irreducible()
    with pytest.raises(NotImplementedError, match="2\\^64"):
        f.is_primitive()
    with pytest.raises(NotImplementedError, match="2\\^64"):
        ga.is_irreducible_batched(GF(np.array([[1, 0, 5]], dtype=object)))


@pytest.mark.parametrize("order, degree", [(2**61 - 1, 3), (2**64 - 2**32 + 1, 2), (2**40, 3), (7**8, 2), (5**9, 3), (3**13, 2),
                                           (3**16, 2), (3**12, 4)])
def test_every_arithmetic_kind(order, degree):
    """Prime64, Goldilocks, Bin, digit-vector extension fields of degrees 8, 9, 13 and 16, and a table field: the first and the last irreducible polynomial are found,
    their products with each other are rejected, and a primitive polynomial's reciprocal is primitive too."""
    GF = ga.GF(order)  # (over GF(2^40) degree 3: x^2 + c is a square, and the first x^2 + x + c lies 2^40 candidates away)
    lo, hi = ga.irreducible_poly(order, degree), ga.irreducible_poly(order, degree, method="max")
    assert lo.degree == hi.degree == degree and lo.is_irreducible() and hi.is_irreducible() and lo != hi
    assert not (lo * hi).is_irreducible() and not (lo * lo).is_irreducible()
    assert not ga.Poly.Int(order**degree, field=GF).is_irreducible()  # x^degree
    # f irreducible with a root r: the reciprocal polynomial has the root 1 / r, of the same order
    rev = ga.Poly(np.flip(lo.coeffs))
    assert rev.degree == degree and rev.is_irreducible() and rev.is_primitive() is lo.is_primitive()
    # x^2 - a is irreducible iff a is a non-square: a = g (a generator) is one for odd q, and every element is a square for even q
    g_elem = GF(GF._primitive_element_int)
    quad = ga.Poly(np.concatenate([GF.Ones(1), GF.Zeros(1), (-g_elem).reshape(1)]))
    assert quad.is_irreducible() is (order % 2 == 1)


@pytest.mark.parametrize("p", [2147483629, 4294967291], ids=["below_2e31", "below_2e32"])
def test_quadratic_extensions_of_large_primes(p):
    """GF(p^2) for the largest primes below 2^31 and below 2^32 (order < 2^64, digit-vector arithmetic; above 2^31 the unreduced
    64-bit middle coefficient of a product would overflow).  Known answers from Euler's criterion and from multiplicative orders,
    both computed by the element-wise kernels: x^2 - c is irreducible iff c^((q-1)/2) != 1, x^3 - c iff c^((q-1)/3) != 1
    (3 | q - 1), x - b is primitive iff b has order q - 1; scaling a row by a unit changes nothing."""
    a = next(v for v in range(2, 100) if pow(v, (p - 1) // 2, p) != 1)
    GF = ga.GF(p, 2, irreducible_poly=[1, 0, p - a], primitive_element=p, verify=False)
    q = p * p
    assert not GF._limbed and GF.order == q < 2**64
    c = GF.Random(64, low=1, seed=5)
    neg = [int(v) for v in (-c).numpy()]
    unit = GF.Random(64, low=1, seed=6)
    for d in (2, 3):
        expect = [int(v) != 1 for v in np.power(c, (q - 1) // d).numpy()]
        assert True in expect and False in expect
        host = [[1] + [0] * (d - 1) + [v] for v in neg]
        rows = GF(np.array(host, dtype=object))
        assert ga.is_irreducible_batched(rows).tolist() == expect
        cols = [[int(v) for v in (unit * GF(np.array([r[j] for r in host], dtype=object))).numpy()] for j in range(d + 1)]  # every row times its own unit
        scaled = GF(np.array(cols, dtype=object).T.copy())
        assert ga.is_irreducible_batched(scaled).tolist() == expect
        f = ga.Poly(rows[0])
        assert f.is_irreducible() is expect[0]
    orders = [int(v) for v in c.multiplicative_order()]
    lin = GF(np.array([[1, v] for v in neg], dtype=object))
    assert ga.is_irreducible_batched(lin).all()
    assert ga.is_primitive_batched(lin).tolist() == [o == q - 1 for o in orders]
    # products of two linear factors, and of an irreducible quadratic with a linear factor
    quad = [i for i in range(64) if int(np.power(c[i], (q - 1) // 2)) != 1][0]
    f2 = ga.Poly(GF(np.array([1, 0, neg[quad]], dtype=object)))
    l0, l1 = ga.Poly(lin[0]), ga.Poly(lin[1])
    assert f2.is_irreducible() and not (l0 * l1).is_irreducible() and not (f2 * l0).is_irreducible() and not (f2 * f2).is_irreducible()
