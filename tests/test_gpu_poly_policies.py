"""Every entry point of the batched polynomial kernels (gfa_polydiv.hip, gfa_polygcd.hip, gfa_polyroots.hip, gfa_lagrange.hip,
gfa_lfsr.hip, gfa_polytest.hip, gfa_polyelem.hip) once for each explicit-arithmetic extension degree: GF(3^M), M = 2 .. 16, which the
policy dispatch of gfa_poly_launch.h serves with ExtP<M>.  The other tests of these kernels reach degrees 3, 4, 7, 8 and 13 only.

The shapes are the smallest that still run the kernels (3 rows, 5 .. 9 coefficients, 4 points, an exponent above 2^64) and every
answer is checked by an identity on operations these kernels have no part in: products, sums and differences of Poly, evaluation,
element-wise arithmetic and matrix products of field arrays.  Everything is exact."""
import functools
import random

import numpy as np
import pytest

import galois_amd as ga
from galois_amd import _lagrange as LG
from galois_amd import _lfsr as LF
from galois_amd import _polydiv as PD
from galois_amd import _polyelem as PE
from galois_amd import _polygcd as PG
from galois_amd import _polyroots as PR
from galois_amd import _polysearch as PS

pytestmark = pytest.mark.gpu

DEGREES = list(range(2, 17))
BIG = 2**64 + 13  # an exponent of two words


@functools.lru_cache(maxsize=None)
def _field(M):
    return ga.GF(3**M)


class _explicit:
    """GF(3^M) on explicit arithmetic for the length of a test: up to 3^12 the field has tables and is pinned to "jit-calculate",
    above it there are none.  Either way the kernels get a digit-vector descriptor of degree M (64-bit elements)."""

    def __init__(self, M):
        self.M, self.GF, self.pinned = M, _field(M), 3**M <= 2**20

    def __enter__(self):
        if self.pinned:
            self.GF.compile("jit-calculate")
        assert self.GF.characteristic == 3 and self.GF.degree == self.M and PD._elem_bytes(self.GF) == 8
        return self.GF

    def __exit__(self, *exc):
        if self.pinned:
            self.GF.compile("auto")


def _poly(GF, ints):
    return ga.Poly(GF([int(v) for v in ints]))


def _ints(a):
    return [int(v) for v in a.numpy().reshape(-1)]


def _random_poly(GF, rng, ncoef, monic=False):
    return _poly(GF, [1 if monic else rng.randrange(1, GF.order)] + [rng.randrange(GF.order) for _ in range(ncoef - 1)])


def _stack(polys, width):
    return np.stack([p.coefficients(width) for p in polys])


def _neg(GF, v):
    return int((-GF([int(v)]))[0])


def _linear(GF, r):
    """x - r"""
    return _poly(GF, [1, _neg(GF, r)])


def _product(polys):
    out = polys[0]
    for p in polys[1:]:
        out = out * p
    return out


# ---- the residue ring GF(q)[x] / (c), c monic, on products of Poly and one matrix product per reduction -------------------------------
def _high_powers(c):
    """(d - 1, d): x^(2 d - 2), .., x^d modulo the monic c of degree d, a row of d coefficients each, highest degree first."""
    GF, d = c.field, c.degree
    x, rows, p = ga.Poly.Identity(GF), [], ga.Poly(-c.coeffs[1:])  # x^d = -(c - x^d)
    for _ in range(d - 1):
        rows.append(p.coefficients(d))
        p = p * x
        if p.degree == d:
            p = p - ga.Poly(p.coeffs[:1]) * c
    return np.stack(rows[::-1])


def _reduce(t, c, R):
    """t modulo c for deg t <= 2 deg c - 2: its low coefficients plus its high ones times R = _high_powers(c)."""
    d, co = c.degree, t.coeffs
    n = co.size
    if n <= d:
        return t
    high = co[:n - d].reshape(1, n - d) @ R[d - 1 - (n - d):]
    return ga.Poly(co[n - d:] + high[0])


def _power(a, e, c, R):
    """a^e modulo c by repeated multiply-and-reduce, the exponent's bits from the top."""
    a = _reduce(a, c, R)
    r = a
    for bit in bin(e)[3:]:
        r = _reduce(r * r, c, R)
        if bit == "1":
            r = _reduce(r * a, c, R)
    return r


# ---- gfa_poly_divmod, gfa_poly_powmod --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", DEGREES)
def test_divmod_and_powmod(M):
    with _explicit(M) as GF:
        rng = random.Random(100 + M)
        rows = [_random_poly(GF, rng, 9) for _ in range(3)]
        b = _random_poly(GF, rng, 5)
        Q, R = PD.poly_divmod_batched(_stack(rows, 9), b)
        assert tuple(Q.shape) == (3, 5) and tuple(R.shape) == (3, 4)
        for k, a in enumerate(rows):
            q, r = ga.Poly(Q[k]), ga.Poly(R[k])
            assert q * b + r == a and r.degree < b.degree, f"GF(3^{M}) row {k}"

        bases = [_random_poly(GF, rng, 7) for _ in range(3)]
        c = _random_poly(GF, rng, 5, monic=True)
        out = PD.poly_powmod_batched(_stack(bases, 7), BIG, c)
        assert tuple(out.shape) == (3, 4)
        hp = _high_powers(c)
        for k, a in enumerate(bases):
            assert ga.Poly(out[k]) == _power(a, BIG, c, hp), f"GF(3^{M}) row {k}"


# ---- gfa_poly_gcd ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", DEGREES)
def test_gcd_and_egcd(M):
    with _explicit(M) as GF:
        rng = random.Random(200 + M)
        common = [_random_poly(GF, rng, 3) for _ in range(3)]  # planted: the gcds have degree 2 at least
        A = [d * _random_poly(GF, rng, 7) for d in common]
        B = [d * _random_poly(GF, rng, 5) for d in common]
        assert PG._served(GF, 9, 7, True)
        G = PG.poly_gcd_batched(_stack(A, 9), _stack(B, 7))
        G2, S, T = PG.poly_egcd_batched(_stack(A, 9), _stack(B, 7))
        assert tuple(G.shape) == (3, 9) and _ints(G) == _ints(G2)
        for k, (a, b) in enumerate(zip(A, B)):
            g, s, t = ga.Poly(G[k]), ga.Poly(S[k]), ga.Poly(T[k])
            assert a * s + b * t == g and int(g.coeffs[0]) == 1 and g.degree >= 2, f"GF(3^{M}) row {k}"
            # g divides both: the quotients are certificates, checked by a product
            assert (a // g) * g == a and (b // g) * g == b, f"GF(3^{M}) row {k}"


# ---- gfa_poly_roots, gfa_poly_root_multiplicity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", DEGREES)
def test_roots_and_multiplicities(M):
    with _explicit(M) as GF:
        rng = random.Random(300 + M)
        r = sorted(rng.sample(range(GF.order), 4))
        lin = [_linear(GF, v) for v in r]
        quadratic = _poly(GF, [1, 0, _neg(GF, GF.primitive_element)])  # x^2 - g, g no square (q is odd): no root
        rows = [_product(lin), lin[0] * lin[0] * quadratic, lin[1] * lin[2] * lin[2] * lin[2]]
        known = [{r[0]: 1, r[1]: 1, r[2]: 1, r[3]: 1}, {r[0]: 2}, {r[1]: 1, r[2]: 3}]
        A = _stack(rows, 5)
        assert GF.order * 4 * 3 <= PR.SEARCH_MAX_WORK and PR._search_serves(GF, 5)  # (the work cap of the entry point is 2^42)
        roots, counts, mult = PR.poly_roots_batched(A, multiplicity=True)
        assert tuple(roots.shape) == (3, 4) and tuple(mult.shape) == (3, 4)
        for k, f in enumerate(rows):
            n = int(counts[k])
            assert n == len(known[k]), f"GF(3^{M}) row {k}"
            assert _ints(f(roots[k, :n])) == [0] * n, f"GF(3^{M}) row {k}"
            assert _ints(roots[k]) == sorted(known[k]) + [0] * (4 - n), f"GF(3^{M}) row {k}"
            assert [int(v) for v in mult[k]] == [known[k][v] for v in sorted(known[k])] + [0] * (4 - n), f"GF(3^{M}) row {k}"
        # the multiplicities of given elements: the four roots of the first row in every row
        given = GF([r, r, r])
        got = PR._mult_t(GF, A._t.contiguous(), given._t.contiguous()).cpu().numpy()
        assert [[int(v) for v in row] for row in got] == [[known[k].get(v, 0) for v in r] for k in range(3)]


# ---- gfa_poly_lagrange -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", DEGREES)
def test_lagrange(M):
    with _explicit(M) as GF:
        rng = random.Random(400 + M)
        X = GF([rng.sample(range(GF.order), 4) for _ in range(3)])
        Y = GF([[rng.randrange(GF.order) for _ in range(4)] for _ in range(3)])
        own = LG.lagrange_poly_batched(X, Y, method="kernel")
        shared = LG.lagrange_poly_batched(X[0], Y, method="kernel")
        assert tuple(own.shape) == (3, 4) and tuple(shared.shape) == (3, 4)
        for k in range(3):
            assert _ints(ga.Poly(own[k])(X[k])) == _ints(Y[k]), f"GF(3^{M}) row {k}"
            assert _ints(ga.Poly(shared[k])(X[0])) == _ints(Y[k]), f"GF(3^{M}) row {k}, shared abscissae"


# ---- gfa_lfsr_step, gfa_lfsr_jump --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", DEGREES)
def test_lfsr_step_and_jump(M):
    with _explicit(M) as GF:
        rng = random.Random(500 + M)
        n = 5
        feedback = _poly(GF, [rng.randrange(1, GF.order)] + [rng.randrange(GF.order) for _ in range(n - 1)] + [1])
        states = GF([[rng.randrange(GF.order) for _ in range(n)] for _ in range(3)])
        for cls in (LF.FLFSR, LF.GLFSR):
            reg = cls(feedback, state=states[0])
            kind = LF._KINDS[reg._type]
            assert n <= LF.lfsr_max_order(GF) and n <= LF._step_max_order(GF)
            # seven clocks of three registers against the loops on whole arrays
            Y, S = LF.lfsr_step_batched(reg, states, 7)
            for k in range(3):
                y, s = LF._host_step(kind, True, reg.taps, states[k], 7)
                assert _ints(Y[k]) == _ints(y) and _ints(S[k]) == _ints(s), f"GF(3^{M}) {reg._type} row {k}"
            # a jump of 7 is 7 single clocks; a jump of BIG + 7 is a jump of BIG and 7 single clocks
            reg.jump(7)
            assert _ints(reg.state) == _ints(S[0]), f"GF(3^{M}) {reg._type}"
            reg.reset()
            reg.jump(BIG)
            far = reg.state
            reg.reset()
            reg.jump(BIG + 7)
            assert _ints(reg.state) == _ints(LF._host_step(kind, True, reg.taps, far, 7)[1]), f"GF(3^{M}) {reg._type}"
            if cls is LF.GLFSR:  # one clock multiplies S_0 + S_1 x + .. by x modulo the characteristic polynomial
                c = reg.characteristic_poly
                hp = _high_powers(c)
                ahead = _reduce(_power(ga.Poly.Identity(GF), BIG, c, hp) * ga.Poly(np.flip(states[0], axis=0)), c, hp)
                assert _ints(far) == _ints(ahead.coefficients(n, order="asc")), f"GF(3^{M}) galois, BIG clocks"


# ---- gfa_poly_classify, gfa_poly_element_classify ----------------------------------------------------------------------------------------
def _artin_schreier(GF, seed):
    """(c1, c0), non-zero: x^3 - x - c is irreducible over GF(3^M) when the trace of c down to GF(3) is not zero (c1), and has three
    roots in the field when it is (c0)."""
    cand = GF.Random(64, low=1, seed=seed)
    t, trace = cand, cand
    for _ in range(GF.degree - 1):
        t = t * t * t
        trace = trace + t
    tr, c = _ints(trace), _ints(cand)
    assert set(tr) <= {0, 1, 2}
    return next(v for v, s in zip(c, tr) if s != 0), next(v for v, s in zip(c, tr) if s == 0)


@pytest.mark.parametrize("M", DEGREES)
def test_classify_polynomials_and_elements(M):
    with _explicit(M) as GF:
        rng = random.Random(600 + M)
        g = int(GF.primitive_element)
        quadratic = _poly(GF, [1, 0, _neg(GF, g)])  # x^2 - g: irreducible, g is no square
        r = rng.sample(range(1, GF.order), 2)
        two = [quadratic, _linear(GF, r[0]) * _linear(GF, r[1]), _poly(GF, [1, 0, 0])]
        assert PS.is_irreducible_batched(_stack(two, 3)).tolist() == [True, False, False], f"GF(3^{M}) degree 2"

        c1, c0 = _artin_schreier(GF, 700 + M)
        cubic = _poly(GF, [1, 0, 2, _neg(GF, c1)])
        split = _poly(GF, [1, 0, 2, _neg(GF, c0)])
        three = [cubic, split, _linear(GF, r[0]) * quadratic]
        assert PS.is_irreducible_batched(_stack(three, 4)).tolist() == [True, False, False], f"GF(3^{M}) degree 3"
        roots, counts = PR.poly_roots_batched(_stack([cubic, split], 4))
        assert counts.tolist() == [0, 3] and _ints(split(roots[1])) == [0, 0, 0]

        # modulo the cubic, a root w has the conjugates w, w + k, w + 2 k (k the trace of c1): they sum to zero, so w is not normal,
        # nor is 1; the conjugates w^2, w^2 + 2 k w + k^2, w^2 + k w + k^2 of w^2 have determinant -k^3, not zero: normal
        residues = GF([[1, 0, 0], [0, 1, 0], [0, 0, 1]])
        assert PE.is_normal_element_batched(residues, cubic).tolist() == [True, False, False], f"GF(3^{M})"
