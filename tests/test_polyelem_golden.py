"""The primitive / normal element functions against the reference's own data (tests/golden/reference_elements.npz): the 22
recorded lists of every primitive and every normal element of GF(p^m) for (p, m) = (2, 2..6), (3, 2..4), (5, 2..4) on the field's
irreducible polynomial, live answers of the reference for every residue over GF(4), GF(8) and GF(9), and the argument checks of
its exception tests (tests/fields/test_normal_elements.py:14-77, test_primitive_elements.py:14-78; without the string forms and
the Poly.Random() defaults, which do not exist here).  Everything is exact."""
import functools
import os

import numpy as np
import pytest

import galois_amd as ga
from tests import helpers as H

pytestmark = pytest.mark.gpu

_FILE = os.path.join(H.GOLDEN, "reference_elements.npz")
TABLES = [(int(p), int(m)) for p, m in np.load(_FILE)["tables"]]
LIVE = [(int(q), int(m)) for q, m in np.load(_FILE)["live"]]
KINDS = {
    "primitive": (ga.is_primitive_element, ga.primitive_element, ga.primitive_elements, ga.is_primitive_element_batched),
    "normal": (ga.is_normal_element, ga.normal_element, ga.normal_elements, ga.is_normal_element_batched),
}


@functools.lru_cache(maxsize=None)
def _golden():
    d = np.load(_FILE)
    return {k: d[k] for k in d.keys()}


def _field_poly(p, m):
    return ga.Poly.Int(int(ga.GF(p**m).irreducible_poly), field=ga.GF(p))


@pytest.mark.parametrize("p, m", TABLES)
@pytest.mark.parametrize("kind", ["primitive", "normal"])
def test_enumerations_and_searches_reproduce_the_recorded_lists(p, m, kind):
    table = [int(v) for v in _golden()[f"{kind}/{p}_{m}"]]
    is_one, one, every, _ = KINDS[kind]
    f = _field_poly(p, m)
    got = every(f)
    assert isinstance(got, list) and all(isinstance(g, ga.Poly) and g.field is ga.GF(p) and g.degree < m for g in got)
    assert [int(g) for g in got] == table
    assert got[0] == ga.Poly.Int(table[0], field=ga.GF(p))  # trimmed like any other Poly
    assert int(one(f)) == table[0] and int(one(f, method="min")) == table[0] and int(one(f, method="max")) == table[-1]
    assert all(int(one(f, method="random")) in table for _ in range(3))
    assert every(ga.GF(p**m).irreducible_poly) == got  # what the class property of the field hands out is accepted as it is
    members = set(table)
    for v in range(p**m):
        assert is_one(v, f) is (v in members), v
    assert is_one(ga.Poly.Int(table[-1], field=ga.GF(p)), f) is True
    coeffs = [int(c) for c in ga.Poly.Int(table[0], field=ga.GF(p)).coeffs.numpy()]
    assert is_one(coeffs, f) is True and is_one(ga.GF(p)(coeffs), f) is True


@pytest.mark.parametrize("p, m", TABLES)
def test_class_properties_agree_with_the_recorded_lists(p, m):
    GF = ga.GF(p**m)
    prim = GF.primitive_elements
    assert type(prim) is GF and prim.ndim == 1 and [int(v) for v in prim.numpy()] == [int(v) for v in _golden()[f"primitive/{p}_{m}"]]
    norm = GF.normal_elements
    assert type(norm) is GF and norm.ndim == 1 and [int(v) for v in norm.numpy()] == [int(v) for v in _golden()[f"normal/{p}_{m}"]]
    one = GF.normal_element
    assert type(one) is GF and one.ndim == 0 and int(one) == int(_golden()[f"normal/{p}_{m}"][0])
    norm[0] = 0  # a copy: the cached array is not touched
    assert int(GF.normal_elements[0]) == int(_golden()[f"normal/{p}_{m}"][0])
    assert np.all(prim.multiplicative_order() == p**m - 1)


def test_class_properties_of_prime_fields():
    GF = ga.GF(31)
    assert GF.normal_element is None
    assert type(GF.normal_elements) is GF and GF.normal_elements.size == 0
    roots = [v for v in range(1, 31) if len({pow(v, k, 31) for k in range(30)}) == 30]
    assert [int(v) for v in GF.primitive_elements.numpy()] == roots
    assert [int(v) for v in ga.GF(2).primitive_elements.numpy()] == [1]


@pytest.mark.parametrize("q, m", LIVE)
def test_batched_forms_reproduce_the_reference_on_every_residue(q, m):
    g = _golden()
    GF = ga.GF(q)
    f = ga.Poly(GF([int(c) for c in g[f"live/{q}_{m}/poly"]]))
    assert f.degree == m and f == ga.irreducible_poly(q, m)  # the first of this project's search order
    v = np.arange(q**m)
    elements = GF(np.stack([(v // q**(m - 1 - j)) % q for j in range(m)], axis=1))
    for kind in ("primitive", "normal"):
        got = KINDS[kind][3](elements, f)
        assert isinstance(got, np.ndarray) and got.dtype == bool and got.shape == (q**m,)
        assert got.tolist() == [bool(b) for b in g[f"live/{q}_{m}/{kind}"]], kind
        assert [int(e) for e in KINDS[kind][2](f)] == [int(i) for i in np.nonzero(g[f"live/{q}_{m}/{kind}"][q:])[0] + q]
    # a non-monic modulus defines the same residue ring
    scaled = ga.Poly(f.coeffs * GF(2))
    assert ga.is_normal_element_batched(elements, scaled).tolist() == [bool(b) for b in g[f"live/{q}_{m}/normal"]]


@pytest.mark.parametrize("kind", ["primitive", "normal"])
def test_argument_checks(kind):
    is_one, one, every, batched = KINDS[kind]
    GF2 = ga.GF(2)
    p = _field_poly(2, 8)
    with pytest.raises(TypeError):
        one(p.coeffs)
    with pytest.raises(ValueError, match="degree greater than 1"):
        one(ga.Poly([1]))
    with pytest.raises(ValueError, match="degree greater than 1"):
        one(ga.Poly([1, 1]))
    with pytest.raises(ValueError, match="is reducible over GF\\(2\\)"):
        one(ga.Poly([1, 1, 1]) * ga.Poly([1, 0, 1]))
    with pytest.raises(ValueError, match="'method' must be in"):
        one(p, method="invalid")
    with pytest.raises(ValueError, match="must be irreducible"):
        one(ga.Poly([1, 0, 0, 0, 0]))
    with pytest.raises(TypeError):
        every(float(int(p)))
    with pytest.raises(ValueError, match="degree greater than 1"):
        every(ga.Poly([1]))
    with pytest.raises(ValueError, match="must be irreducible"):
        every(ga.Poly([1, 1, 1]) * ga.Poly([1, 0, 1]))
    e = ga.Poly([1, 0, 1, 1])
    f = ga.Poly([1, 0, 0, 0, 1, 1, 1, 0, 1])
    with pytest.raises(TypeError):
        is_one(float(int(e)), f)
    with pytest.raises(TypeError):
        is_one(e, f.coeffs)
    with pytest.raises(ValueError, match="over the same field"):
        is_one(e, ga.Poly([1, 0, 0, 0, 1, 1, 1, 0, 1], field=ga.GF(3)))
    with pytest.raises(ValueError, match="degree less than"):
        is_one(f, f)
    with pytest.raises(ValueError, match="must be irreducible"):
        is_one(e, ga.Poly([1, 0, 0, 0, 0]))
    with pytest.raises(TypeError):
        batched([[1, 0, 1]], f)
    with pytest.raises(ValueError, match="over the same field"):
        batched(ga.GF(3)([[1, 0, 1, 0, 0, 0, 0, 0]]), f)
    with pytest.raises(ValueError, match="8 coefficients"):
        batched(GF2([[1, 0, 1]]), f)
    assert batched(GF2(np.zeros((0, 8), dtype=np.uint8)), f).shape == (0,)


def test_limits_raise_not_implemented():
    GF = ga.GF(36893488147419103183, primitive_element=3)
    f = ga.Poly(GF(np.array([1, 0, 5], dtype=object)))
    for fn in (ga.is_primitive_element_batched, ga.is_normal_element_batched):
        with pytest.raises(NotImplementedError, match="2\\^64"):
            fn(GF(np.array([[1, 2]], dtype=object)), f)
    g = ga.Poly.Degrees([33, 0], field=ga.GF(3))
    with pytest.raises(NotImplementedError, match="up to 32"):
        ga.is_normal_element_batched(ga.GF(3).Zeros((1, 33)), g)
    h = ga.Poly.Degrees([256, 0])
    with pytest.raises(NotImplementedError, match="255"):
        ga.is_primitive_element_batched(ga.GF(2).Zeros((1, 256)), h)
