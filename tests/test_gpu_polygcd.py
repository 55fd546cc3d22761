"""gcd / egcd / lcm / prod of Poly, poly_gcd_batched / poly_egcd_batched and the entry point gfa_poly_gcd
(galois_amd/csrc/gfa_polygcd.hip): the reference's Sage vectors (tests/golden/sage_polygcd.npz), the reference's Euclid restated on
the division, product and difference operators that existed before the kernel, planted common divisors, and the C contract.
Everything is exact."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import galois_amd as ga
from galois_amd import _lib as L
from galois_amd import _polygcd as PG
from galois_amd import _polysearch as PS
from tests import helpers as H

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(H.GOLDEN, "sage_polygcd.npz")
TAGS = sorted(k.split("/")[1] for k in np.load(GOLDEN).keys() if k.startswith("sage/") and k.endswith("/properties"))
DEGREES = [0, 1, 63, 64, 65, 130]  # the host test's set: around the division's block of 64


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
    g = _golden()
    flat, ends = [int(v) for v in g[key]], np.cumsum(g[key + "_len"])
    return [flat[e - n:e] for e, n in zip(ends, g[key + "_len"])]


def _is(poly, GF, c):
    return isinstance(poly, ga.Poly) and poly.field is GF and _coeffs(poly) == [int(v) for v in c]


def _groups(key):
    """The argument lists of the lcm / prod cases."""
    flat, out, at = _lists(key), [], 0
    for n in _golden()[key + "_count"]:
        out.append(flat[at:at + int(n)])
        at += int(n)
    return out


# ---- 1. the reference's vectors -----------------------------------------------------------------------------------------------------
def test_all_sage_folders_present():
    assert len(TAGS) == 16
    assert {"GF_2", "GF_2e8", "GF_7e3", "GF_2147483647", "GF_2e32", "GF_2e100", "GF_109987e4", "GF_36893488147419103183"} <= set(TAGS)
    with_square_free = [t for t in TAGS if len(_golden()[f"sage/{t}/sqfree_Z"])]
    assert len(with_square_free) == 11 and {"GF_2", "GF_2e8", "GF_7e3", "GF_3191"} <= set(with_square_free)
    assert sum(ga.GF(json.loads(str(_golden()[f"sage/{t}/properties"]))["order"])._limbed for t in ("GF_2e100", "GF_36893488147419103183")) == 2


@pytest.mark.parametrize("tag", TAGS)
def test_sage_egcd(tag):
    GF = _sage_field(tag)
    X, Y, D, S, T = (_lists(f"sage/{tag}/egcd_{k}") for k in "XYDST")
    assert len(X) == 20
    for x, y, d, s, t in zip(X, Y, D, S, T):
        a, b = _poly(GF, x), _poly(GF, y)
        got = ga.egcd(a, b)
        assert _is(got[0], GF, d) and _is(got[1], GF, s) and _is(got[2], GF, t), f"{tag}: egcd({x}, {y})"
        assert _is(ga.gcd(a, b), GF, d), f"{tag}: gcd({x}, {y})"


@pytest.mark.parametrize("tag", TAGS)
def test_sage_lcm_prod_and_square_freeness(tag):
    GF = _sage_field(tag)
    for name, fn in (("lcm", ga.lcm), ("prod", ga.prod)):
        X, Z = _groups(f"sage/{tag}/{name}_X"), _lists(f"sage/{tag}/{name}_Z")
        assert len(X) == len(Z) >= 1
        for xs, z in zip(X, Z):
            assert _is(fn(*[_poly(GF, x) for x in xs]), GF, z), f"{tag}: {name}{xs}"
    X, Z = _lists(f"sage/{tag}/sqfree_X"), [bool(z) for z in _golden()[f"sage/{tag}/sqfree_Z"]]
    assert len(X) == len(Z)  # (the reference has no such vectors for its five largest fields: see test_all_sage_folders_present)
    for x, z in zip(X, Z):
        assert _poly(GF, x).is_square_free() is z, f"{tag}: is_square_free({x})"


# ---- 2. the reference's Euclid on the operators that existed before the kernel ------------------------------------------------------
def _euclid_by_operators(a, b):
    """_functions.py:40-57, word for word, on // * - of Poly."""
    GF = a.field
    zero, one = ga.Poly(GF([0])), ga.Poly(GF([1]))
    r2, r1 = a, b
    s2, s1 = one, zero
    t2, t1 = zero, one
    while r1 != zero:
        q = r2 // r1
        r2, r1 = r1, r2 - q * r1
        s2, s1 = s1, s2 - q * s1
        t2, t1 = t1, t2 - q * t1
    c = ga.Poly(r2.coeffs[:1])
    if int(r2.coeffs[0]) > 1:
        r2, s2, t2 = r2 // c, s2 // c, t2 // c
    return r2, s2, t2


FIELDS = {
    "GF(2)": lambda: ga.GF(2), "GF(7)": lambda: ga.GF(7), "GF(2^8)": lambda: ga.GF(2**8), "GF(2^8) calculate": lambda: ga.GF(2**8),
    "GF(3^5)": lambda: ga.GF(3**5), "GF(65537)": lambda: ga.GF(65537), "GF(2147483647)": lambda: ga.GF(2**31 - 1),
    "Goldilocks": lambda: ga.GF(H.GOLDILOCKS), "GF(2^32)": lambda: ga.GF(2**32), "GF(7^3)": lambda: ga.GF(7**3),
    "GF(109987^4)": lambda: _sage_field("GF_109987e4"),
}


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


def _random_poly(GF, degree, seed):
    c = GF.Random(degree + 1, seed=seed)
    c[0] = GF.Random(low=1, seed=seed + 1)
    return ga.Poly(c)


def _stack(GF, polys, width):
    """The polynomials as right-aligned rows of a (len, width) array."""
    if GF._limbed:
        out = GF.Zeros((len(polys), width))
        for k, p in enumerate(polys):
            out[k, width - p.coeffs.size:] = p.coeffs
        return out
    np_dtype, tdt = PS._storage(GF)
    t = torch.zeros((len(polys), width), dtype=tdt, device="cuda")
    for k, p in enumerate(polys):
        t[k, width - p.coeffs.size:] = p.coeffs._t
    return GF._wrap(t, np_dtype)


def _rows_are(M, polys, width):
    return tuple(M.shape) == (len(polys), width) and torch.equal(M._t, _stack(type(M), polys, width)._t)


@functools.lru_cache(maxsize=None)
def _cases(name):
    """(pairs, their egcd by the operators), computed once per field and shared by the two tests below."""
    GF = FIELDS[name]()
    zero = ga.Poly(GF([0]))
    pairs = [(_random_poly(GF, da, 10 * i), _random_poly(GF, db, 10 * i + 5)) for i, (da, db) in enumerate((da, db) for da in DEGREES for db in DEGREES)]
    a65, b64 = pairs[DEGREES.index(65) * 6 + DEGREES.index(64)]
    # rows of other true degrees: zero operands, b | a, a = b, and sequences whose degrees drop by 64 and by 2
    u, low = _random_poly(GF, 64, 991), _random_poly(GF, 1, 992)
    pairs += [(zero, b64), (a65, zero), (zero, zero), (b64 * _random_poly(GF, 60, 990), b64), (b64, b64), (u * a65 + low, a65),
              (a65 * _random_poly(GF, 2, 993) + low, a65)]
    return pairs, [_euclid_by_operators(a, b) for a, b in pairs]


@pytest.mark.parametrize("name", list(FIELDS))
def test_egcd_equals_the_loop_over_the_operators(name):
    with _mode(name) as GF:
        pairs, expected = _cases(name)
        assert len(pairs) == 36 + 7
        for (a, b), (d, s, t) in zip(pairs, expected):
            got = ga.egcd(a, b)
            assert got[0] == d and got[1] == s and got[2] == t, f"egcd at degrees {a.degree}, {b.degree}"
            if not GF._limbed:  # (no kernel there: gcd is the same loop without the cofactors)
                assert ga.gcd(a, b) == d
                assert a * s + b * t == d


@pytest.mark.parametrize("name", list(FIELDS))
def test_batched_forms_equal_the_loop_over_the_operators(name):
    with _mode(name) as GF:
        pairs, expected = _cases(name)
        # the whole list as one stack: the rows have different true degrees
        width = 132
        A, B = _stack(GF, [a for a, _ in pairs], width), _stack(GF, [b for _, b in pairs], width - 1)
        keep_a, keep_b = A._t.clone(), B._t.clone()
        G, S, T = ga.poly_egcd_batched(A, B)
        assert type(G) is GF and type(S) is GF and type(T) is GF
        assert _rows_are(G, [e[0] for e in expected], width) and _rows_are(S, [e[1] for e in expected], width) and _rows_are(T, [e[2] for e in expected], width)
        assert torch.equal(ga.poly_gcd_batched(A, B)._t, G._t)
        assert torch.equal(A._t, keep_a) and torch.equal(B._t, keep_b)  # the inputs are not modified
        # one b for every row, as a Poly and as a 1-D array
        b64 = pairs[DEGREES.index(65) * 6 + DEGREES.index(64)][1]
        rows = pairs[36:] if GF._limbed else pairs[30:]  # (every row is a loop over the operators where there is no kernel)
        shared = [_euclid_by_operators(a, b64) for a, _ in rows]
        A30 = _stack(GF, [a for a, _ in rows], width)
        G, S, T = ga.poly_egcd_batched(A30, b64)
        assert _rows_are(G, [e[0] for e in shared], width) and _rows_are(S, [e[1] for e in shared], width) and _rows_are(T, [e[2] for e in shared], width)
        assert torch.equal(ga.poly_gcd_batched(A30, b64.coeffs)._t, G._t)


@pytest.mark.parametrize("name", ["GF(2^8)", "GF(65537)"])
@pytest.mark.parametrize("extended", [False, True], ids=["gcd", "egcd"])
def test_the_lds_cap_and_the_loop_above_it(name, extended):
    """na + nb == gcd_max_terms runs in the kernel, one coefficient more in the loop over the operators, with the same answer.  The
    divisor is short (the loop above the cap costs a launch per step); the dividend fills LDS."""
    with _mode(name) as GF:
        cap = ga.gcd_max_terms(GF, extended)
        assert cap == (150 * 1024 - 8) // 4 // (3 if extended else 1)
        nb = 4
        na = cap - nb
        g, v = _random_poly(GF, 1, 5), _random_poly(GF, 2, 6)
        b = g * v
        a = g * _random_poly(GF, na - 2, 7)
        assert a.coeffs.size == na and b.coeffs.size == nb
        A, A1 = _stack(GF, [a], na), _stack(GF, [a], na + 1)
        assert PG._served(GF, na, nb, extended) and not PG._served(GF, na + 1, nb, extended)
        at, bt = A._t, b.coeffs._t.reshape(1, -1)
        dtype = {1: L.U8, 2: L.U16, 4: L.U32, 8: L.U64}[at.element_size()]
        if extended:
            G, S, T = ga.poly_egcd_batched(A, b)
            G1, S1, T1 = ga.poly_egcd_batched(A1, b)
            assert torch.equal(S1._t[:, 1:], S._t) and torch.equal(T1._t[:, 1:], T._t) and not bool(S1._t[:, 0].any()) and not bool(T1._t[:, 0].any())
            assert a * ga.Poly(S[0]) + b * ga.Poly(T[0]) == ga.Poly(G[0])
        else:
            G, G1 = ga.poly_gcd_batched(A, b), ga.poly_gcd_batched(A1, b)
        assert torch.equal(G1._t[:, 1:], G._t) and not bool(G1._t[:, 0].any())
        d = ga.Poly(G[0])
        assert d.degree >= 1 and d.is_monic and (d % g) == ga.Poly(GF([0])) and (a % d) == ga.Poly(GF([0])) and (b % d) == ga.Poly(GF([0]))
        assert ga.gcd(a, b) == d


# ---- 3. planted common divisors -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [7, 2**8, 65537, 7**3])
def test_planted_gcd(order):
    GF = ga.GF(order)
    irr = []
    for degree, count in ((2, 4), (3, 4)):
        for p in ga.irreducible_polys(order, degree):
            irr.append(p)
            if len(irr) % 4 == 0:
                break
    assert len(irr) == 8 and all(p.is_irreducible() for p in irr)
    u, v = ga.prod(irr[0], irr[2], irr[4], irr[6]) ** 3, ga.prod(irr[1], irr[3], irr[5], irr[7]) ** 2  # coprime, degrees 30 and 20
    for k, dg in enumerate([0, 1, 64, 200]):
        g = _random_poly(GF, dg, 40 + k)
        monic = g // ga.Poly(g.coeffs[:1])
        a, b = g * u, g * v
        d, s, t = ga.egcd(a, b)
        assert d == monic and ga.gcd(a, b) == monic and ga.gcd(b, a) == monic, f"deg g = {dg}"
        assert s * a + t * b == d
        assert ga.lcm(a, b) == monic * (u * v)  # u and v are monic
    assert ga.gcd(u, v) == ga.Poly(GF([1]))


def test_polymorphism_and_error_paths():
    GF = ga.GF(7)
    f, g = ga.Poly(GF([1, 0, 6])), ga.Poly(GF([1, 6]))
    assert ga.gcd(12, 18) == 6 and ga.egcd(12, 18) == (6, -1, 1) and ga.lcm(4, 6, 10) == 60 and ga.prod(2, 3, 4) == 24
    assert ga.gcd(np.int64(12), 18) == 6
    assert ga.factors(12) == ([2, 3], [2, 1])
    with pytest.raises(TypeError, match="must both be either int or galois.Poly"):
        ga.gcd(f, 3)
    with pytest.raises(TypeError, match="must both be either int or galois.Poly"):
        ga.egcd(3, g)
    with pytest.raises(TypeError, match="All arguments must be either int or galois.Poly"):
        ga.lcm(f, 3)
    with pytest.raises(TypeError, match="All arguments must be either int or galois.Poly"):
        ga.prod(f, 3.0)
    with pytest.raises(ValueError, match="At least one argument must be provided"):
        ga.lcm()
    with pytest.raises(ValueError, match="At least one argument must be provided"):
        ga.prod()
    other = ga.Poly(ga.GF(5)([1, 2]))
    with pytest.raises(ValueError, match="must be over the same Galois field"):
        ga.gcd(f, other)
    with pytest.raises(ValueError, match="must be over the same Galois field"):
        ga.egcd(f, other)
    with pytest.raises(ValueError, match="All polynomial arguments must be over the same field"):
        ga.lcm(f, other)
    with pytest.raises(ValueError, match="All polynomial arguments must be over the same field"):
        ga.prod(f, other)
    zero, one = ga.Poly(GF([0])), ga.Poly(GF([1]))
    assert ga.egcd(zero, zero) == (zero, one, zero) and ga.gcd(ga.Poly(GF([3, 0])), zero) == ga.Poly(GF([1, 0]))
    assert ga.egcd(ga.Poly(GF([3])), zero) == (one, ga.Poly(GF([5])), zero)
    with pytest.raises(TypeError):
        ga.poly_gcd_batched([[1, 2]], g)
    with pytest.raises(ValueError):
        ga.poly_gcd_batched(GF([1, 2]), g)
    with pytest.raises(TypeError):
        ga.poly_gcd_batched(GF([[1, 2]]), other)
    with pytest.raises(ValueError):
        ga.poly_egcd_batched(GF([[1, 2], [3, 4], [5, 6]]), GF([[1, 2], [3, 4]]))


def test_batched_forms_over_a_field_of_order_above_2_64():
    GF = ga.GF(2**100)
    g = _poly(GF, [1, 2**99 + 5, 3])
    u, v = _poly(GF, [2**64 + 1, 0, 7, 1]), _poly(GF, [5, 2**80])
    A = GF(np.array([_coeffs(g * u), [0, 0, 0, 0, 0, 0], [0, 0, 0, 1, 2, 3]], dtype=object))
    B = GF(np.array([[0] + _coeffs(g * v), [0, 0, 0, 2, 9], [0, 0, 0, 0, 0]], dtype=object))
    G, S, T = ga.poly_egcd_batched(A, B)
    assert tuple(G.shape) == tuple(S.shape) == tuple(T.shape) == (3, 6)
    assert torch.equal(ga.poly_gcd_batched(A, B)._t, G._t)
    for k in range(3):
        a, b = ga.Poly(A[k]), ga.Poly(B[k])
        d, s, t = _euclid_by_operators(a, b)
        assert ga.Poly(G[k]) == d and ga.Poly(S[k]) == s and ga.Poly(T[k]) == t and ga.egcd(a, b) == (d, s, t)
    assert ga.Poly(G[0]) == g


# ---- 4. the C entry point's contract ------------------------------------------------------------------------------------------------
def _p(t):
    return t.data_ptr() if t is not None else None


def _gcd(GF, a, batch, na, b, b_rows, nb, g, s, t, deg, dtype, handle=True):
    return L.lib().gfa_poly_gcd(GF._handle if handle else None, _p(a), batch, na, _p(b), b_rows, nb, _p(g), _p(s), _p(t), _p(deg), dtype,
                                torch.cuda.current_stream().cuda_stream)


def test_gcd_entry_point_contract():
    GF = ga.GF(7)
    dev = torch.device("cuda")
    u8 = lambda rows: torch.tensor(rows, dtype=torch.uint8, device=dev)
    a = u8([[1, 0, 6], [0, 0, 3], [0, 0, 0], [1, 1, 1]])
    b = u8([[1, 6], [0, 0], [0, 0], [2, 1]])
    fill = lambda: torch.full((4, 3), 0x55, dtype=torch.uint8, device=dev)
    g, s, t = fill(), fill(), fill()
    deg = torch.full((4,), 77, dtype=torch.int32, device=dev)
    assert _gcd(GF, a, 4, 3, b, 4, 2, g, s, t, deg, L.U8) == L.OK
    # by hand over GF(7): x^2 - 1 and x - 1; 3 and 0 (1/3 = 5); 0 and 0; x^2 + x + 1 = (4 x + 2)(2 x + 1) + 6 with 1/6 = 6
    assert g.cpu().tolist() == [[0, 1, 6], [0, 0, 1], [0, 0, 0], [0, 0, 1]]
    assert s.cpu().tolist() == [[0, 0, 0], [0, 0, 5], [0, 0, 1], [0, 0, 6]]
    assert t.cpu().tolist() == [[0, 0, 1], [0, 0, 0], [0, 0, 0], [0, 4, 2]]
    assert deg.cpu().tolist() == [1, 0, -1, 0]
    # s and t, and deg, may be NULL: the others are written as before
    g2, deg2 = fill(), torch.full_like(deg, 77)
    assert _gcd(GF, a, 4, 3, b, 4, 2, g2, None, None, deg2, L.U8) == L.OK and torch.equal(g2, g) and torch.equal(deg2, deg)
    g2 = fill()
    assert _gcd(GF, a, 4, 3, b, 4, 2, g2, None, None, None, L.U8) == L.OK and torch.equal(g2, g)
    g2, s2, t2 = fill(), fill(), fill()
    assert _gcd(GF, a, 4, 3, b, 4, 2, g2, s2, t2, None, L.U8) == L.OK and torch.equal(g2, g) and torch.equal(s2, s) and torch.equal(t2, t)
    # one b for all rows, the longer operand second, another storage width and a non-default stream
    b1 = torch.tensor([[0, 1, 0, 6]], dtype=torch.int64, device=dev)  # x^2 - 1
    a64 = a.to(torch.int64)
    g4, d4 = torch.zeros((4, 4), dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        assert L.lib().gfa_poly_gcd(GF._handle, _p(a64), 4, 3, _p(b1), 1, 4, _p(g4), None, None, _p(d4), L.U64, stream.cuda_stream) == L.OK
    stream.synchronize()
    assert g4.cpu().tolist() == [[0, 1, 0, 6], [0, 0, 0, 1], [0, 1, 0, 6], [0, 0, 0, 1]] and d4.cpu().tolist() == [2, 0, 2, 0]
    # batch == 0 touches nothing, whatever the pointers
    g2 = fill()
    assert _gcd(GF, None, 0, 3, None, 1, 2, None, None, None, None, L.U8) == L.OK and _gcd(GF, a, 0, 3, b, 0, 2, g2, None, None, None, L.U8) == L.OK
    # rejected calls: b_rows outside {1, batch}, s without t, missing pointers, empty rows, a dtype that cannot hold the field
    assert _gcd(GF, a, 4, 3, b, 2, 2, g2, None, None, None, L.U8) == L.ERR_INVALID and "b_rows" in L.last_error()
    assert _gcd(GF, a, 4, 3, b, 0, 2, g2, None, None, None, L.U8) == L.ERR_INVALID and _gcd(GF, a, 4, 3, b, 5, 2, g2, None, None, None, L.U8) == L.ERR_INVALID
    assert _gcd(GF, a, 4, 3, b, 4, 2, g2, s2, None, None, L.U8) == L.ERR_INVALID and _gcd(GF, a, 4, 3, b, 4, 2, g2, None, t2, None, L.U8) == L.ERR_INVALID
    assert _gcd(GF, None, 4, 3, b, 4, 2, g2, None, None, None, L.U8) == L.ERR_INVALID and _gcd(GF, a, 4, 3, None, 4, 2, g2, None, None, None, L.U8) == L.ERR_INVALID
    assert _gcd(GF, a, 4, 3, b, 4, 2, None, None, None, None, L.U8) == L.ERR_INVALID
    assert _gcd(GF, a, 4, 0, b, 4, 2, g2, None, None, None, L.U8) == L.ERR_INVALID and _gcd(GF, a, 4, 3, b, 4, 0, g2, None, None, None, L.U8) == L.ERR_INVALID
    assert _gcd(GF, a, -1, 3, b, 1, 2, g2, None, None, None, L.U8) == L.ERR_INVALID and _gcd(GF, a, 4, 3, b, 4, 2, g2, None, None, None, 9) == L.ERR_INVALID
    assert _gcd(ga.GF(65537), a, 4, 3, b, 4, 2, g2, None, None, None, L.U8) == L.ERR_INVALID and "dtype" in L.last_error()
    # fields of order >= 2^64 have no handle of this kind
    wide = ga.GF(2**100)
    assert wide._limbed and wide._handle is None
    assert _gcd(wide, a, 4, 3, b, 4, 2, g2, None, None, None, L.U64) == L.ERR_UNSUPPORTED and "2^64" in L.last_error()
    assert g2.cpu().tolist() == [[0x55] * 3] * 4


@pytest.mark.parametrize("name", ["GF(7)", "GF(2^8)", "GF(2^8) calculate", "GF(2^32)", "GF(7^3)", "Goldilocks", "GF(2147483647)"])
@pytest.mark.parametrize("extended", [False, True], ids=["gcd", "egcd"])
def test_gcd_cap_is_named_and_leaves_no_sticky_error(name, extended):
    with _mode(name) as GF:
        cap = ga.gcd_max_terms(GF, extended)
        np_dtype, tdt = PS._storage(GF)
        dtype = {1: L.U8, 2: L.U16, 4: L.U32, 8: L.U64}[torch.empty(0, dtype=tdt).element_size()]
        na, nb = cap - 1, 2
        a = torch.zeros((1, na), dtype=tdt, device="cuda")
        a[0, 0], a[0, -1] = 1, 1  # x^(na - 1) + 1
        b = torch.ones((1, nb), dtype=tdt, device="cuda")  # x + 1
        out = [torch.zeros((1, na), dtype=tdt, device="cuda") for _ in range(3)]
        deg = torch.zeros(1, dtype=torch.int32, device="cuda")
        s, t = (out[1], out[2]) if extended else (None, None)
        assert _gcd(GF, a, 1, na, b, 1, nb, out[0], s, t, deg, dtype) == L.ERR_UNSUPPORTED  # cap + 1 terms: one too many
        assert str(cap) in L.last_error() and str(cap + 1) in L.last_error()
        torch.cuda.synchronize()  # nothing was launched and no HIP error stays behind
        assert _gcd(GF, a, 1, na - 1, b, 1, nb, out[0], s, t, deg, dtype) == L.OK  # the first na - 1 columns: x^(na - 2), cap terms
        torch.cuda.synchronize()
        assert int(deg.item()) == 0 and out[0][0, :na - 1].cpu().tolist() == [0] * (na - 2) + [1]
