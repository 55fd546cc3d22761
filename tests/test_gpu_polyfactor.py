"""Poly.is_monic / Random / is_square_free / square_free_factors / distinct_degree_factors / equal_degree_factors / factors
(galois_amd/_polyfactor.py over gfa_poly_gcd, gfa_poly_divmod and gfa_poly_powmod): the reference's live answers and the products
constructed from its irreducible polynomials (tests/golden/sage_polygcd.npz), reconstruction of random inputs from their factors,
the reference's exception cases, and the characteristic-2 product the reference's own splitting cannot finish quickly.  Everything
is exact."""
import functools
import os
import time

import numpy as np
import pytest

import galois_amd as ga
from galois_amd import _numtheory as nt
from tests import helpers as H

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(H.GOLDEN, "sage_polygcd.npz")
LIVE = sorted({k.split("/")[1] for k in np.load(GOLDEN).keys() if k.startswith("live/")})
BUILT = sorted({k.split("/")[1] for k in np.load(GOLDEN).keys() if k.startswith("built/")})


@functools.lru_cache(maxsize=None)
def _golden():
    d = np.load(GOLDEN)
    return {k: d[k] for k in d.keys()}


def _field(key):
    """The field of a fixture entry "live/GF_7e3" or "built/GF_2e8", with the reference's parameters."""
    g = _golden()
    base, _, exp = key.split("/")[1][3:].partition("e")
    order = int(base) ** int(exp or 1)
    (p,), (m,) = nt.factors(order)
    alpha = int(g[f"{key}/primitive_element"])
    if m == 1:
        return ga.GF(p, primitive_element=alpha)
    return ga.GF(p, m, irreducible_poly=[int(c) for c in g[f"{key}/irreducible_poly"]], primitive_element=alpha)


def _coeffs(poly):
    return [int(v) for v in poly.coeffs.numpy()]


def _poly(GF, c):
    return ga.Poly(GF(np.array([int(v) for v in c], dtype=object)))


def _lists(key):
    g = _golden()
    flat, ends = [int(v) for v in g[key]], np.cumsum(g[key + "_len"])
    return [flat[e - n:e] for e, n in zip(ends, g[key + "_len"])]


def _same(polys, GF, lists):
    return len(polys) == len(lists) and all(isinstance(p, ga.Poly) and p.field is GF and _coeffs(p) == c for p, c in zip(polys, lists))


def _product(GF, polys, mult):
    out = ga.Poly(GF([1]))
    for p, e in zip(polys, mult):
        out = out * p**e
    return out


# ---- 1. the fixtures ----------------------------------------------------------------------------------------------------------------
def test_fixture_fields():
    assert LIVE == sorted(["GF_2", "GF_3", "GF_5", "GF_2e2", "GF_3e2", "GF_5e2", "GF_7e3", "GF_3191", "GF_2147483647"])
    assert BUILT == ["GF_2e32", "GF_2e8"]


@pytest.mark.parametrize("tag", LIVE)
def test_live_reference_factorisations(tag):
    g, key = _golden(), f"live/{tag}"
    GF = _field(key)
    f = _poly(GF, g[f"{key}/f"])
    assert f.is_monic and not f.is_square_free()  # it holds the square of a cubic
    factors, mult = f.factors()
    assert _same(factors, GF, _lists(f"{key}/factors")) and mult == [int(e) for e in g[f"{key}/factors_mult"]]
    assert ga.factors(f) == (factors, mult)
    sf, sf_mult = f.square_free_factors()
    assert _same(sf, GF, _lists(f"{key}/sf")) and sf_mult == [int(e) for e in g[f"{key}/sf_mult"]]
    assert sf[0].is_square_free()
    ddf, degrees = sf[0].distinct_degree_factors()
    assert _same(ddf, GF, _lists(f"{key}/ddf")) and degrees == [int(e) for e in g[f"{key}/ddf_deg"]]
    for k, (p, d) in enumerate(zip(ddf, degrees)):
        assert _same(p.equal_degree_factors(d), GF, _lists(f"{key}/edf{k}")), f"{tag}: equal_degree_factors({d}) of factor {k}"


@pytest.mark.parametrize("tag", BUILT)
def test_products_of_the_references_irreducible_polynomials(tag):
    g, key = _golden(), f"built/{tag}"
    GF = _field(key)
    f = _poly(GF, g[f"{key}/f"])
    expected, mult = _lists(f"{key}/factors"), [int(e) for e in g[f"{key}/factors_mult"]]
    assert max(mult) >= 2 and max(np.bincount([len(c) for c in expected])) >= 3
    factors, got_mult = f.factors()
    assert _same(factors, GF, expected) and got_mult == mult
    assert all(p.is_irreducible() for p in factors) and _product(GF, factors, got_mult) == f


# ---- 2. reconstruction --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [2, 5, 2**8])
def test_random_polynomials_are_the_product_of_their_irreducible_factors(order):
    GF = ga.GF(order)
    for seed, degree in enumerate([30, 29, 17, 8, 1]):
        f = ga.Poly.Random(degree, seed=seed, field=GF)
        assert f.degree == degree and f == ga.Poly.Random(degree, seed=seed, field=GF)  # seeded: reproducible
        f = f // ga.Poly(f.coeffs[:1])
        assert f.is_monic
        factors, mult = f.factors()
        assert _product(GF, factors, mult) == f, f"seed {seed}"
        assert all(p.is_irreducible() and p.is_monic for p in factors)
        assert [int(p) for p in factors] == sorted(int(p) for p in factors) and len(set(int(p) for p in factors)) == len(factors)
        assert f.factors() == (factors, mult)  # the random choices inside are seeded too
        assert f.is_square_free() is (max(mult) == 1)


def test_random_and_is_monic():
    GF = ga.GF(7)
    rng = np.random.default_rng(5)
    f, g = ga.Poly.Random(6, seed=rng, field=GF), ga.Poly.Random(6, seed=rng, field=GF)
    assert f.degree == 6 and g.degree == 6 and f != g and f.field is GF
    assert ga.Poly.Random(4).field is ga.GF(2) and ga.Poly.Random(0, seed=1, field=GF).degree == 0
    assert ga.Poly(GF([1, 3])).is_monic and not ga.Poly(GF([2, 3])).is_monic and not ga.Poly(GF([0])).is_monic
    with pytest.raises(TypeError):
        ga.Poly.Random(2.0, field=GF)
    with pytest.raises(TypeError):
        ga.Poly.Random(2, seed=1.5, field=GF)
    with pytest.raises(ValueError):
        ga.Poly.Random(-1, field=GF)
    with pytest.raises(ValueError):
        ga.Poly.Random(2, seed=-1, field=GF)


# ---- 3. the reference's exception cases (tests/polys/test_factors.py) ------------------------------------------------------------------
def test_exceptions():
    GF = ga.GF(5)
    a, b, c = ga.Poly(GF([1, 0])), ga.Poly(GF([1, 0, 2, 4])), ga.Poly(GF([1, 4, 1]))
    assert a.is_irreducible() and b.is_irreducible() and c.is_irreducible()
    f = a * b * c**3
    assert f.square_free_factors() == ([a * b, c], [1, 3]) and f.factors() == ([a, c, b], [1, 3, 1])
    non_monic, constant = ga.Poly(GF([2, 0, 2, 4])), ga.Poly(GF([2]))
    for method in ("factors", "square_free_factors", "distinct_degree_factors"):
        with pytest.raises(ValueError, match="must be monic"):
            getattr(non_monic, method)()
        with pytest.raises(ValueError, match="must be non-constant"):
            getattr(constant, method)()
    with pytest.raises(ValueError, match="must be monic"):
        non_monic.equal_degree_factors(1)
    with pytest.raises(ValueError, match="must be non-constant"):
        constant.equal_degree_factors(1)
    with pytest.raises(ValueError, match="must be square-free"):
        f.distinct_degree_factors()
    with pytest.raises(ValueError, match="must be square-free"):
        (c**2).equal_degree_factors(2)
    with pytest.raises(ValueError, match="must divide the degree of the polynomial, 2 does not divide 3"):
        b.equal_degree_factors(2)
    with pytest.raises(TypeError):
        b.equal_degree_factors(3.0)
    assert constant.is_square_free() and non_monic.is_square_free() is (non_monic // constant).is_square_free()
    # the examples of the reference's documentation
    a2, b2 = ga.Poly([1, 0]), ga.Poly([1, 1])
    assert (a2 * b2).equal_degree_factors(1) == [a2, b2]
    c2, d2, e2 = ga.Poly([1, 1, 1]), ga.Poly([1, 0, 1, 1]), ga.Poly([1, 1, 0, 1])
    assert (a2 * b2 * c2 * d2 * e2).distinct_degree_factors() == ([a2 * b2, c2, d2 * e2], [1, 2, 3])
    p, q = ga.Poly(GF([1, 0, 2, 1])), ga.Poly(GF([1, 4, 4, 4]))
    assert (p * q).equal_degree_factors(3) == [p, q]


# ---- 4. characteristic 2 ----------------------------------------------------------------------------------------------------------
def test_equal_degree_splitting_in_characteristic_two_is_quick():
    """Four irreducible quadratics and three cubics over GF(2^8): the reference's g = h^((q^d - 1) / 2) - 1 splits this only when h is 1
    modulo a factor; the trace polynomial splits on every draw with probability about 1/2 per pair of factors."""
    GF = ga.GF(2**8)
    quadratics, cubics = [], []
    for p in ga.irreducible_polys(2**8, 2):
        quadratics.append(p)
        if len(quadratics) == 4:
            break
    for p in ga.irreducible_polys(2**8, 3, reverse=True):
        cubics.append(p)
        if len(cubics) == 3:
            break
    f = ga.prod(*quadratics) * ga.prod(*cubics)
    assert f.degree == 17
    f.factors()  # (loads the kernels)
    t0 = time.perf_counter()
    factors, mult = f.factors()
    seconds = time.perf_counter() - t0
    assert factors == sorted(quadratics + cubics, key=int) and mult == [1] * 7
    assert (ga.prod(*quadratics)).equal_degree_factors(2) == sorted(quadratics, key=int)
    assert seconds < 3.0, f"{seconds:.2f} s"
