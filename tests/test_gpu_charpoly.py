"""FieldArray.characteristic_poly() / minimal_poly() and gfa_charpoly (galois_amd/csrc/gfa_charpoly.hip): the reference's Sage
vectors (tests/golden/sage_charpoly.npz), known answers from conjugated companion matrices at sizes that cross the kernel's
internal boundaries and its two launch regimes, degenerate structure, cross-checks against independent kernels (det, @,
matrix Horner) and the C entry point's contract.  Everything is exact."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import galois_amd as ga
from galois_amd import _lib as L
from tests import helpers as H

pytestmark = pytest.mark.gpu

GOLDILOCKS = 2**64 - 2**32 + 1


@functools.lru_cache(maxsize=None)
def _golden():
    d = np.load(os.path.join(H.GOLDEN, "sage_charpoly.npz"))
    return {k: d[k] for k in d.keys()}


def _tags(wide):
    out = []
    for k, v in _golden().items():
        if k.endswith("/properties") and (wide or json.loads(str(v))["order"] < 2**64):
            out.append(k.split("/")[0])
    return sorted(out)


def _field(tag):
    props = json.loads(str(_golden()[f"{tag}/properties"]))
    p, m = props["characteristic"], props["degree"]
    if m == 1:
        return ga.GF(p, primitive_element=int(props["primitive_element"]))
    return ga.GF(p, m, irreducible_poly=H.poly_coeffs_to_int(props["irreducible_poly"], p),
                 primitive_element=int(props["primitive_element"]))


def _ints(a):
    return [int(v) for v in np.asarray(a).ravel()]


def _mk(GF, host, dtype=None):
    """Host integers (any dtype, any nesting) -> device array over GF."""
    host = np.array(host, dtype=object)
    if GF.dtypes == [np.object_]:
        return GF(host)
    dt = GF.dtypes[-1] if dtype is None else dtype
    return GF(host.astype(np.uint64).astype(dt), dtype=dt)


def _coeffs(poly):
    return _ints(poly.coeffs.numpy())


# ---- 1. Sage matrix vectors --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", _tags(wide=False))
def test_sage_matrix_vectors(tag):
    g = _golden()
    GF = _field(tag)
    rng = np.random.default_rng(5)
    assert int(g[f"{tag}/cpm_count"]) == 5
    for i in range(5):
        X, Z = g[f"{tag}/cpm{i}_X"], _ints(g[f"{tag}/cpm{i}_Z"])
        assert X.shape == (i + 2, i + 2)
        dt = GF.dtypes[int(rng.integers(0, len(GF.dtypes)))]  # the reference tests draw a random legal dtype too
        A = _mk(GF, X, dt)
        poly = A.characteristic_poly()
        assert isinstance(poly, ga.Poly) and poly.field is GF
        assert _coeffs(poly) == Z, f"{tag} case {i}"
        stack = _mk(GF, np.stack([X, X.T, X]), dt)  # det(xI - A) = det(xI - A^T)
        got = ga.linalg.characteristic_poly_batched(stack)
        assert type(got) is GF and got.shape == (3, i + 3)
        assert [_ints(r) for r in got.numpy()] == [Z, Z, Z], f"{tag} case {i} (batched)"


# ---- 2. Sage element vectors -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", _tags(wide=True))
def test_sage_element_vectors(tag):
    g = _golden()
    GF = _field(tag)
    sub = GF.prime_subfield
    seen_subfield_element = False
    for key, method in (("cpe", "characteristic_poly"), ("mpe", "minimal_poly")):
        X, Zl, Zf = _ints(g[f"{tag}/{key}_X"]), g[f"{tag}/{key}_Zlen"], _ints(g[f"{tag}/{key}_Z"])
        ends = np.cumsum(Zl)
        for i, x in enumerate(X):
            Z = Zf[ends[i] - Zl[i]:ends[i]]
            poly = getattr(GF(x), method)()
            assert poly.field is (GF if GF.is_prime_field else sub)
            assert _coeffs(poly) == Z, f"{tag} {method}({x})"
            seen_subfield_element |= key == "mpe" and len(Z) - 1 < GF.degree
    if GF.degree > 1 and len(X) == GF.order:
        assert seen_subfield_element  # a folder of all elements holds the proper subfields: deg m_a < m is exercised


@pytest.mark.parametrize("p, m, d", [(2, 32, 1), (2, 32, 16), (2, 100, 4), (2, 100, 50), (109987, 4, 2),
                                     (109987, 4, 1)])
def test_subfield_elements_of_sampled_fields(p, m, d):
    """alpha^((q - 1) / (p^d - 1)) has order p^d - 1, so it generates GF(p^d): its minimal polynomial has degree exactly d,
    annihilates it, and the characteristic polynomial is its (m / d)-th power.  (The Sage folders of GF(2^32) and of the
    two-limb fields hold 20 random elements, none of them in a proper subfield.)"""
    GF = _field({32: "GF_2e32", 100: "GF_2e100", 4: "GF_109987e4"}[m])
    b = GF(GF._primitive_element_int) ** ((p**m - 1) // (p**d - 1))
    mp, cp = b.minimal_poly(), b.characteristic_poly()
    assert mp.field is GF.prime_subfield and cp.field is GF.prime_subfield
    assert mp.degree == d and cp.degree == m and _coeffs(mp)[0] == 1
    assert int(ga.Poly(_mk(GF, _coeffs(mp)))(b)) == 0
    power = mp
    for _ in range(m // d - 1):
        power = power * mp
    assert cp == power


# ---- 3. known answers: conjugated companion matrices -------------------------------------------------------------------
_KA_FIELDS = {
    "gf2": lambda: ga.GF(2),
    "gf3": lambda: ga.GF(3),
    "gf2e8_lookup": lambda: ga.GF(2**8),
    "gf65537": lambda: ga.GF(65537),
    "gf2e16": lambda: ga.GF(2**16),
    "gf2147483647": lambda: ga.GF(2147483647),
    "goldilocks": lambda: ga.GF(GOLDILOCKS),
    "gf251e3": lambda: ga.GF(251**3),
}


def _companion(GF, f):
    """Companion matrix (host integers) of the monic polynomial f, coefficients highest degree first."""
    n = len(f) - 1
    C = np.zeros((n, n), dtype=object)
    for i in range(1, n):
        C[i, i - 1] = 1
    C[:, n - 1] = _ints((-_mk(GF, f[1:][::-1])).numpy())
    return C


def _unit_lu(GF, n, seed):
    """S = L U from random unit lower and unit upper triangular factors: always invertible."""
    R = GF.Random((2, n, n), seed=seed).numpy().astype(object)
    eye = np.eye(n, dtype=object)
    return _mk(GF, np.tril(R[0], -1) + eye) @ _mk(GF, np.triu(R[1], 1) + eye)


@functools.lru_cache(maxsize=None)
def _conjugated_companion(name, n):
    GF = _KA_FIELDS[name]()
    f = [1] + _ints(GF.Random(n, seed=1000 + n).numpy())
    S = _unit_lu(GF, n, seed=2000 + n)
    B = S @ _mk(GF, _companion(GF, f)) @ np.linalg.inv(S)
    return GF, f, B


@pytest.mark.parametrize("n", [1, 2, 3, 17, 255, 256, 257])
@pytest.mark.parametrize("name", list(_KA_FIELDS))
def test_conjugated_companion(name, n):
    if name == "gf2e8_lookup":
        assert ga.GF(2**8).ufunc_mode == "jit-lookup"
    GF, f, B = _conjugated_companion(name, n)
    assert _coeffs(B.characteristic_poly()) == f
    assert _coeffs(B.T.characteristic_poly()) == f


@pytest.mark.parametrize("name", ["gf2", "gf2e8_lookup", "goldilocks"])
def test_both_regimes_agree_at_384(name):
    GF, f, B = _conjugated_companion(name, 384)
    Bt = B.T
    one = B.characteristic_poly()  # batch 1, 384^2 >= 131072: the chip-wide kernels
    assert _coeffs(one) == f
    assert _coeffs(Bt.characteristic_poly()) == f
    pair = ga.linalg.characteristic_poly_batched(np.stack([B, Bt]))  # still chip-wide, two matrices per launch
    assert [_ints(r) for r in pair.numpy()] == [f, f]
    stack = np.stack([B, Bt] * 16 + [B])  # 33 matrices: one workgroup each
    got = ga.linalg.characteristic_poly_batched(stack)
    assert got.shape == (33, 385)
    want = one.coeffs.numpy()
    for r in got.numpy():
        assert np.array_equal(r, want)


# ---- 4. degenerate structure -------------------------------------------------------------------------------------------
def _poly_from_roots(GF, roots):
    out = ga.Poly(_mk(GF, [1]))
    for r in roots:
        out = out * ga.Poly(np.concatenate([_mk(GF, [1]), (-_mk(GF, [r]))]))
    return out


@pytest.mark.parametrize("name", ["gf2", "gf2e8_lookup", "gf31"])
def test_degenerate_structure(name):
    GF = ga.GF(31) if name == "gf31" else _KA_FIELDS[name]()
    n = 40
    rng = np.random.default_rng(11)
    x_n = [1] + [0] * n
    R = GF.Random((n, n), seed=7).numpy().astype(object)

    assert _coeffs(_mk(GF, np.zeros((n, n), dtype=object)).characteristic_poly()) == x_n
    assert GF.Identity(n).characteristic_poly() == _poly_from_roots(GF, [1] * n)
    shift = np.zeros((n, n), dtype=object)
    for i in range(1, n):
        shift[i, i - 1] = 1
    assert _coeffs(_mk(GF, shift).characteristic_poly()) == x_n
    strictly_lower = np.tril(R, -1)  # nilpotent, and dense below the diagonal: every step eliminates
    assert _coeffs(_mk(GF, strictly_lower).characteristic_poly()) == x_n

    # three companion blocks, conjugated by a random permutation matrix
    polys, blocks = [], np.zeros((n, n), dtype=object)
    at = 0
    for k, size in enumerate((7, 13, 20)):
        f = [1] + _ints(GF.Random(size, seed=20 + k).numpy())
        polys.append(ga.Poly(_mk(GF, f)))
        blocks[at:at + size, at:at + size] = _companion(GF, f)
        at += size
    perm = rng.permutation(n)
    assert _mk(GF, blocks[perm][:, perm]).characteristic_poly() == polys[0] * polys[1] * polys[2]

    upper = np.triu(R)
    assert _mk(GF, upper).characteristic_poly() == _poly_from_roots(GF, [upper[i, i] for i in range(n)])

    # first column zero below the diagonal: (x - a00) * charpoly of the trailing block, a conjugated companion of g
    g = [1] + _ints(GF.Random(n - 1, seed=31).numpy())
    S = _unit_lu(GF, n - 1, seed=32)
    tail = (S @ _mk(GF, _companion(GF, g)) @ np.linalg.inv(S)).numpy()
    first = R.copy()
    first[1:, 0] = 0
    first[1:, 1:] = tail
    assert _mk(GF, first).characteristic_poly() == _poly_from_roots(GF, [first[0, 0]]) * ga.Poly(_mk(GF, g))


# ---- 5. cross-checks with independent kernels --------------------------------------------------------------------------
@pytest.mark.parametrize("order", [3**5, 7340033])
def test_cross_checks(order):
    GF = ga.GF(order)
    n = 64
    A = GF.Random((n, n), seed=3)
    poly = A.characteristic_poly()
    c = poly.coeffs
    assert poly.degree == n and int(c[0]) == 1
    assert int(c[1]) == int(-np.trace(A)), "x^(n-1) coefficient = -trace"
    assert int(c[n]) == int(np.linalg.det(-A)), "constant coefficient = det(-A)"
    assert not poly(A, elementwise=False).numpy().any(), "Cayley-Hamilton"
    P = _unit_lu(GF, n, seed=4)
    assert (P @ A @ np.linalg.inv(P)).characteristic_poly() == poly


# ---- 6. contract ---------------------------------------------------------------------------------------------------------
def _call(GF, a, out, batch, n, dtype):
    return L.lib().gfa_charpoly(GF._handle, a.data_ptr() if a is not None else None, out.data_ptr() if out is not None else None,
                                batch, n, dtype, torch.cuda.current_stream().cuda_stream)


def test_input_is_not_modified():
    GF = ga.GF(2**8)
    for shape in [(17, 17), (384, 384)]:  # both regimes
        A = GF.Random(shape, seed=9)
        before = A.numpy().copy()
        A.characteristic_poly()
        assert np.array_equal(A.numpy(), before)
    S = GF.Random((5, 9, 9), seed=10)
    before = S.numpy().copy()
    ga.linalg.characteristic_poly_batched(S)
    assert np.array_equal(S.numpy(), before)


def test_c_entry_point_edges():
    GF = ga.GF(65537)
    dev = torch.device("cuda")
    assert _call(GF, None, None, 0, 5, L.U32) == L.OK  # batch == 0 touches nothing
    out = torch.full((3, 1), 7, dtype=torch.int32, device=dev)
    assert _call(GF, None, out, 3, 0, L.U32) == L.OK  # n == 0: the single coefficient 1 per matrix
    assert out.cpu().tolist() == [[1], [1], [1]]
    a = torch.zeros((2, 2), dtype=torch.int32, device=dev)
    out = torch.zeros(8, dtype=torch.int32, device=dev)
    assert _call(GF, a, out, 1, 2, L.U8) == L.ERR_INVALID  # uint8 / uint16 cannot hold GF(65537)
    assert _call(GF, a, out, 1, 2, L.U16) == L.ERR_INVALID
    assert _call(GF, a, out, 1, 4097, L.U32) == L.ERR_UNSUPPORTED
    assert _call(GF, a, out, -1, 2, L.U32) == L.ERR_INVALID
    assert _call(GF, a, None, 1, 2, L.U32) == L.ERR_INVALID
    assert _call(GF, a, out, 1, 2, L.U32) == L.OK
    assert out.cpu().tolist()[:3] == [1, 0, 0]


def test_shapes_and_unsupported_forms():
    GF = ga.GF(31)
    for bad in [GF.Random((3, 4), seed=1), GF.Random(5, seed=1), GF.Random((2, 3, 3), seed=1)]:
        with pytest.raises(ValueError):
            bad.characteristic_poly()
    for bad in [GF.Random(5, seed=1), GF.Random((2, 3, 3), seed=1), GF.Random((3, 4), seed=1)]:
        with pytest.raises(ValueError):
            bad.minimal_poly()
    with pytest.raises(NotImplementedError, match="factor"):
        GF.Random((3, 3), seed=1).minimal_poly()
    with pytest.raises(ValueError):
        ga.linalg.characteristic_poly_batched(GF.Random((3, 3), seed=1))
    # the limits are named: matrices over two-limb fields, elements of fields above 2^128
    W = ga.GF(36893488147419103183, primitive_element=3)
    with pytest.raises(NotImplementedError, match="2\\^64"):
        W.Random((3, 3), seed=1).characteristic_poly()
    Big = ga.GF(2**521 - 1, primitive_element=3, verify=False)
    for method in ("characteristic_poly", "minimal_poly"):
        with pytest.raises(NotImplementedError, match="2\\^128"):
            getattr(Big(5), method)()


def test_non_default_stream():
    GF = ga.GF(2147483647)
    for n in (33, 384):  # both regimes
        A = GF.Random((n, n), seed=n)
        want = _coeffs(A.characteristic_poly())
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            got = _coeffs(A.characteristic_poly())
        s.synchronize()
        assert got == want
