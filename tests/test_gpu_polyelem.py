"""gfa_poly_element_classify (galois_amd/csrc/gfa_polyelem.hip) at its boundaries, against an independent route through kernels
that were there before it: the conjugates g^(q^k) from m - 1 poly_powmod_batched calls with exponent q and the rank of the stacked
conjugate matrices from linalg.row_reduce_batched (normality, the reference's definition), poly_powmod_batched with every
cofactor exponent (primitivity).  Where q^m - 1 is out of the host's reach only normality is tested: it needs no integer
factoring.  Everything is exact."""
import functools
import random

import numpy as np
import pytest
import torch

import galois_amd as ga
from galois_amd import _lib as L
from galois_amd import _numtheory as nt
from galois_amd import _polyelem as PE
from galois_amd import _polysearch as PS
from tests import helpers as H

pytestmark = pytest.mark.gpu

# A prime above 2^32 (64-bit elements in the kernels) with p = 1 mod 31 and mod 4: x^31 - a and x^32 - a are then irreducible for
# suitable a, so irreducible_poly(p, m) finds its lexicographically first polynomial among the first few candidates.  For a prime
# without that (2^32 + 15, say) every x^m + c is reducible and the search has 2^32 candidates to reject before x^m + x + c.
# x^31 - 1 also splits into 31 linear factors here: 31 matrices, six to a slab.
P33 = 2**32 + 1113


@functools.lru_cache(maxsize=None)
def _modulus(q, m):
    return ga.irreducible_poly(q, m)


def _elements(GF, m, batch, seed):
    """(batch, m) residues, highest degree first: the zero row, the row `1`, x (m > 1), constants, then random rows."""
    q = GF.order
    rng = random.Random(seed)
    rows = [[0] * m, [0] * (m - 1) + [1], ([0] * (m - 2) + [1, 0]) if m > 1 else [q - 1], [0] * (m - 1) + [q - 1]]
    while len(rows) < batch:
        rows.append([rng.randrange(q) for _ in range(m)])
    rows[-1] = [q - 1] * m
    return GF(np.array(rows, dtype=object))


def _conjugates(elements, f):
    q = type(elements).order
    out = [elements]
    for _ in range(f.degree - 1):
        out.append(ga.poly_powmod_batched(out[-1], q, f))
    return out


def _normal_by_rank(elements, f):
    GF = type(elements)
    conj = _conjugates(elements, f)
    stack = GF._wrap(torch.stack([c._t for c in conj], dim=1).contiguous(), elements._np_dtype)
    _, ranks = ga.linalg.row_reduce_batched(stack)
    return np.asarray(ranks) == f.degree


def _primitive_by_powers(elements, f):
    GF = type(elements)
    n = GF.order**f.degree - 1
    nonzero = (elements._t != 0).any(dim=1).cpu().numpy()
    ok = nonzero.copy()
    for r in (nt.factors(n)[0] if n > 1 else []):  # GF(2), m = 1: the group is trivial
        h = ga.poly_powmod_batched(elements, n // r, f)._t
        is_one = ((h[:, -1] == 1) & (h[:, :-1] == 0).all(dim=1)).cpu().numpy()
        ok &= ~is_one
    return ok


def _check(GF, m, batch, seed, primitive):
    f = _modulus(GF.order, m)
    el = _elements(GF, m, batch, seed)
    keep = el._t.clone()
    normal = ga.is_normal_element_batched(el, f)
    expect = _normal_by_rank(el, f)
    assert normal.tolist() == expect.tolist()
    assert not normal[0] and (m == 1 or not normal[1])  # the zero row; 1 spans only GF(q)
    if primitive:
        got = ga.is_primitive_element_batched(el, f)
        assert got.tolist() == _primitive_by_powers(el, f).tolist()
        assert not got[0]
    assert torch.equal(el._t, keep)
    return f, el, normal


# ---- m = 1: the residues are the constants --------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [2, 3, 251, 2**8, 65537])
def test_degree_one(q):
    GF = ga.GF(q)
    f, el, normal = _check(GF, 1, 70, 1, True)
    values = [int(v) for v in el.numpy().ravel()]
    assert normal.tolist() == [v != 0 for v in values]
    x_plus_one = ga.Poly(GF([1, 1]))  # modulo x + 1 a constant is itself
    orders = GF([v if v else 1 for v in values]).multiplicative_order()
    assert ga.is_primitive_element_batched(el, x_plus_one).tolist() == [v != 0 and int(o) == q - 1 for v, o in zip(values, orders)]


# ---- the general path at its degree limits, every arithmetic kind ----------------------------------------------------------------
@pytest.mark.parametrize("m", [2, 31, 32])
@pytest.mark.parametrize("q", [3, 251, 65537, P33, 2**8, 3**5, 7**2])
def test_general_path(q, m):
    primitive = m == 2 or q == 3  # (q - 1)(q + 1), and 3^31 - 1, 3^32 - 1: factored at once; the others are not tried
    _check(ga.GF(q), m, 131, 7 * m + q % 1000, primitive)


# A power chain of full length needs no factoring: g^(q^m) = g, so the single "cofactor exponent" q^m flags every residue but 0
# and 1, and q^m - 1 flags none.  Both run the r / t columns over m log2(q) squarings at the degree limit, for every arithmetic
# kind: prime below and above 2^32, Goldilocks, tables, binary and digit-vector extension fields.  The large fields are taken
# at the degrees where some x^m - a is irreducible (31 | q - 1, or q = 1 mod 4 for m = 32), so that irreducible_poly finds its
# first polynomial at once: GF(2^25) and GF(1117^2) have 31 | q - 1; over GF(2^k) every x^32 + c is a 32nd power.  (GF(5^9) would
# do for the digit vectors of nine entries, at 8 s and 10 s a case: left out.)
P2 = 1117  # = 1 mod 31; GF(P2^2) has more than 2^20 elements: digit-vector arithmetic, no tables


@pytest.mark.parametrize("q, m", [(251, 31), (251, 32), (P33, 31), (P33, 32), (H.GOLDILOCKS, 32), (2**8, 31), (2**8, 32), (3**5, 31),
                                  (3**5, 32), (2**25, 31), (P2**2, 31), (P2**2, 32)])
def test_general_path_power_chains_at_the_degree_limit(q, m):
    if q == P2**2:
        a = next(v for v in range(2, 100) if pow(v, (P2 - 1) // 2, P2) != 1)
        GF = ga.GF(P2, 2, irreducible_poly=[1, 0, P2 - a], primitive_element=P2, verify=False)  # GF(p)[x] / (x^2 - a)
        assert GF.order == q and not GF._limbed
    else:
        GF = ga.GF(q)
    if q == P2**2:  # the searches build the default field of an order: a binomial over this one, checked by Rabin's test;
        # the constant from outside GF(p), whose elements are all squares in GF(p^2)
        f = next(g for g in (ga.Poly(GF([1] + [0] * (m - 1) + [c])) for c in range(P2 + 1, P2 + 40)) if g.is_irreducible())
    else:
        f = _modulus(q, m)
    consts = PE._constants(f)
    el = _elements(GF, m, 131, m + 5)
    t = el._t.contiguous()
    assert t.dtype == consts.f_t.dtype
    constant01 = ((t[:, :-1] == 0).all(dim=1) & ((t[:, -1] == 0) | (t[:, -1] == 1))).cpu().tolist()
    assert constant01[:2] == [True, True] and sum(constant01) == 2
    flags = torch.full((131,), 0x55, dtype=torch.uint8, device=t.device)
    for e, expect in ((q**m, [0 if c else PE.PRIMITIVE for c in constant01]), (q**m - 1, [0] * 131)):
        exps, limbs = _limbs(e)
        assert _call(GF._handle, t, consts.f_t, m, el._gfa_dtype(), exps, 1, limbs, None, 0, flags) == L.OK
        assert flags.cpu().tolist() == expect


def _limbs(e):
    import ctypes

    n = (e.bit_length() + 63) // 64
    return (ctypes.c_uint64 * n)(*[(e >> (64 * k)) & (2**64 - 1) for k in range(n)]), n


# ---- the storage width of the arguments: the entry point reads residues, modulus and matrices through one type ------------------
@pytest.mark.parametrize("first", ["default", "wide"])
@pytest.mark.parametrize("q", [2, 3, 65537])
def test_storage_widths_of_the_arguments_do_not_matter(q, first):
    """f and the elements in the field's default storage and in int64, in every combination, and with the per-field constants
    first built from either form of f."""
    GF = ga.GF(q)
    m = 4 if q < 100 else 2
    f = _modulus(q, m)
    f_wide = ga.Poly(f.coeffs.astype(np.int64))
    assert f_wide.coeffs._t.dtype == torch.int64 and f.coeffs._t.dtype != torch.int64 and int(f_wide) == int(f)
    if q < 100:
        v = np.arange(q**m)
        el = GF(np.stack([(v // q**(m - 1 - j)) % q for j in range(m)], axis=1))  # every residue, by its integer
    else:
        el = _elements(GF, m, 131, 9)
    el_wide = el.astype(np.int64)
    assert el_wide._t.dtype == torch.int64 and el._t.dtype != torch.int64
    expect = {False: _normal_by_rank(el, f).tolist(), True: _primitive_by_powers(el, f).tolist()}
    PE._CONSTANTS.clear()
    for poly in ((f, f_wide) if first == "default" else (f_wide, f)):
        for primitive, batched, is_one, one, every in ((False, ga.is_normal_element_batched, ga.is_normal_element, ga.normal_element, ga.normal_elements),
                                                       (True, ga.is_primitive_element_batched, ga.is_primitive_element, ga.primitive_element, ga.primitive_elements)):
            for e in (el, el_wide):
                assert batched(e, poly).tolist() == expect[primitive]
                for k in (0, 1, 5, el.shape[0] - 1):
                    assert is_one(e[k], poly) is expect[primitive][k] and is_one(ga.Poly(e[k]), poly) is expect[primitive][k]
            if q < 100:
                members = [k for k in range(q, q**m) if expect[primitive][k]]
                assert [int(g) for g in every(poly)] == members
                assert int(one(poly)) == members[0] and int(one(poly, method="max")) == members[-1]
                assert int(one(poly, method="random")) in members
                assert all(is_one(k, poly) is expect[primitive][k] for k in range(q**m))
            else:
                g = one(poly)
                assert is_one(g, f) and is_one(g, f_wide) and one(poly, method="random").degree < m
    assert PE._constants(f) is PE._constants(f_wide) and PE._constants(f).f_t.dtype == f.coeffs._t.dtype
    assert PE._constants(f).mats.dtype == f.coeffs._t.dtype
    PE._CONSTANTS.clear()


# ---- more matrices than one slab of LDS holds -----------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [97, H.GOLDILOCKS])
def test_slab_path(q):
    """p = 1 mod 32: x^32 - 1 splits into 32 linear factors, 32 matrices of 1024 elements -- 128 KiB, and 256 KiB on 64-bit
    elements, where a pass holds 5."""
    GF = ga.GF(q)
    f, el, normal = _check(GF, 32, 131, 3, False)
    assert PE._constants(f).mats.shape == (32, 32, 32)
    assert normal.any() and not normal.all()
    # w^q - lambda w has no component in the eigenspace of lambda = the root of the LAST factor: only the last matrix sends it to
    # zero, so only the last slab can tell (97, 32-bit elements: 13 matrices to a pass, the third; Goldilocks: 5, the seventh)
    consts = PE._constants(f)
    xm1 = ga.Poly(GF(np.array([1] + [0] * 31 + [q - 1], dtype=object)))
    last = xm1.factors()[0][31]
    assert last.degree == 1
    k = int(np.nonzero(normal)[0][0])
    w = el[k:k + 1]  # normal: a component in every eigenspace
    vec = ga.poly_powmod_batched(w, q, f) + w * last.coeffs[1]
    assert ga.is_normal_element_batched(vec, f).tolist() == [False] and _normal_by_rank(vec, f).tolist() == [False]
    flags = torch.zeros(1, dtype=torch.uint8, device=vec._t.device)
    t = vec._t.contiguous()
    for n_mats, expect in ((31, PE.NORMAL), (32, 0)):
        assert _call(GF._handle, t, consts.f_t, 32, el._gfa_dtype(), None, 0, 0, consts.mats, n_mats, flags) == L.OK
        assert int(flags.item()) == expect


# ---- p | m: x^m - 1 = (x - 1)^m, one matrix, normal <=> trace != 0 ---------------------------------------------------------------
@pytest.mark.parametrize("q, m", [(2, 64), (2, 128), (3, 27)])
def test_characteristic_divides_degree(q, m):
    GF = ga.GF(q)
    f, el, normal = _check(GF, m, 300, m, False)
    assert PE._constants(f).mats.shape[0] == 1
    trace = functools.reduce(lambda a, b: a + b, _conjugates(el, f))
    assert (trace._t[:, :-1] == 0).all()  # the trace lies in GF(q)
    assert normal.tolist() == (trace._t[:, -1] != 0).cpu().tolist()
    assert normal.any() and not normal.all()


@pytest.mark.parametrize("q, m", [(2, 8), (3, 3), (3, 9), (5, 5), (4, 4)])
def test_characteristic_divides_degree_counts(q, m):
    assert len(ga.normal_elements(_modulus(q, m))) == q**m - q**(m - 1)


# ---- GF(2), bit-packed: word boundaries, one to four words ------------------------------------------------------------------------
@pytest.mark.parametrize("m", [63, 64, 65, 127, 128, 129, 192, 193, 255])
def test_packed_path_normality(m):
    f, el, normal = _check(ga.GF(2), m, 300, m, False)
    assert normal.any() and not normal.all()


@pytest.mark.parametrize("m", [89, 127])
def test_packed_path_primitivity_mersenne(m):
    """2^m - 1 is prime: every residue other than 0 and 1 generates."""
    GF = ga.GF(2)
    el = _elements(GF, m, 300, m)
    got = ga.is_primitive_element_batched(el, _modulus(2, m))
    constant = (el._t[:, :-1] == 0).all(dim=1).cpu().tolist()  # 0 and 1
    assert constant[:2] == [True, True] and sum(constant) < 8
    assert got.tolist() == [not c for c in constant]


@pytest.mark.parametrize("m", [64, 128])
def test_packed_path_primitivity_fermat(m):
    """2^m - 1 is the product of the Fermat numbers below it: the host factors it at once."""
    assert max(nt.factors(2**m - 1)[0]) == (67280421310721 if m == 128 else 6700417)
    f, el, _ = _check(ga.GF(2), m, 300, m + 1, True)
    # elements of the subfield GF(2^(m/2)) are not primitive; x^(2^(m/2) + 1) lies in it
    sub = ga.poly_powmod_batched(el, 2**(m // 2) + 1, f)
    assert not ga.is_primitive_element_batched(sub, f).any()


# ---- the C entry point's contract --------------------------------------------------------------------------------------------------
def _call(handle, el, f_t, m, dtype, exps, n_exps, limbs, mats, n_mats, flags, stream=None, batch=None):
    return L.lib().gfa_poly_element_classify(handle, el.data_ptr() if el is not None else None, el.shape[0] if batch is None else batch,
                                             f_t.data_ptr() if f_t is not None else None, m, dtype, exps, n_exps, limbs,
                                             mats.data_ptr() if mats is not None else None, n_mats,
                                             flags.data_ptr() if flags is not None else None,
                                             torch.cuda.current_stream().cuda_stream if stream is None else stream)


def test_entry_point_contract():
    GF = ga.GF(7)
    m = 3
    f = _modulus(7, m)
    consts = PE._constants(f)
    el = _elements(GF, m, 70, 11)
    t, f_t, mats = el._t.contiguous(), consts.f_t, consts.mats
    keep = (t.clone(), f_t.clone(), mats.clone())
    n_exps, limbs, exps = PS._cofactor_exponents(7, m)
    normal = _normal_by_rank(el, f).astype(np.uint8)
    prim = _primitive_by_powers(el, f).astype(np.uint8)
    assert normal.any() and prim.any() and (normal != prim).any()
    flags = torch.full((70,), 0x55, dtype=torch.uint8, device=t.device)
    h = GF._handle
    assert _call(h, t, f_t, m, L.U8, exps, n_exps, limbs, mats, mats.shape[0], flags) == L.OK
    assert flags.cpu().tolist() == (prim + 2 * normal).tolist()
    for kept, now in zip(keep, (t, f_t, mats)):
        assert torch.equal(kept, now)  # the inputs are not modified
    # a test that is not asked for leaves its bit 0
    assert _call(h, t, f_t, m, L.U8, None, 0, 0, mats, mats.shape[0], flags) == L.OK
    assert flags.cpu().tolist() == (2 * normal).tolist()
    assert _call(h, t, f_t, m, L.U8, exps, n_exps, limbs, None, 0, flags) == L.OK
    assert flags.cpu().tolist() == prim.tolist()
    assert _call(h, t, f_t, m, L.U8, None, 0, 0, None, 0, flags) == L.OK
    assert flags.cpu().tolist() == [0] * 70
    # another storage width and a non-default stream give the same flags
    s = torch.cuda.Stream()
    f2 = torch.zeros(70, dtype=torch.uint8, device=t.device)
    wide = (t.to(torch.int32), f_t.to(torch.int32), mats.to(torch.int32))
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        assert _call(h, wide[0], wide[1], m, L.U32, exps, n_exps, limbs, wide[2], mats.shape[0], f2, stream=s.cuda_stream) == L.OK
    s.synchronize()
    assert f2.cpu().tolist() == (prim + 2 * normal).tolist()
    # batch == 0 touches nothing, whatever the pointers
    flags.fill_(0x55)
    assert _call(h, None, None, m, L.U8, None, 0, 0, None, 0, None, batch=0) == L.OK
    assert _call(h, t, f_t, m, L.U8, exps, n_exps, limbs, mats, mats.shape[0], flags, batch=0) == L.OK
    # rejected calls
    assert _call(h, t, f_t, m, L.U8, exps, n_exps, limbs, mats, mats.shape[0], None) == L.ERR_INVALID
    assert _call(h, None, f_t, m, L.U8, exps, n_exps, limbs, mats, mats.shape[0], flags, batch=70) == L.ERR_INVALID
    assert _call(h, t, None, m, L.U8, exps, n_exps, limbs, mats, mats.shape[0], flags) == L.ERR_INVALID
    assert _call(h, t, f_t, 0, L.U8, exps, n_exps, limbs, mats, mats.shape[0], flags) == L.ERR_INVALID
    assert _call(h, t, f_t, m, L.U8, None, 2, 1, mats, mats.shape[0], flags) == L.ERR_INVALID
    assert _call(h, t, f_t, m, L.U8, exps, n_exps, limbs, mats, -1, flags) == L.ERR_INVALID
    assert _call(h, t, f_t, m, L.U8, exps, n_exps, limbs, mats, mats.shape[0], flags, batch=-1) == L.ERR_INVALID
    assert _call(h, t, f_t, m, 9, exps, n_exps, limbs, mats, mats.shape[0], flags) == L.ERR_INVALID
    assert _call(ga.GF(65537)._handle, t, f_t, m, L.U8, None, 0, 0, None, 0, flags) == L.ERR_INVALID and "dtype" in L.last_error()
    assert _call(h, t, f_t, 33, L.U8, None, 0, 0, None, 0, flags, batch=1) == L.ERR_UNSUPPORTED and "32" in L.last_error()
    assert _call(ga.GF(2)._handle, t, f_t, 256, L.U8, None, 0, 0, None, 0, flags, batch=1) == L.ERR_UNSUPPORTED and "255" in L.last_error()
    limbed = ga.GF(36893488147419103183, primitive_element=3)
    assert limbed._handle is None
    assert _call(None, t, f_t, m, L.U8, None, 0, 0, None, 0, flags) == L.ERR_UNSUPPORTED and "2^64" in L.last_error()
    assert flags.cpu().tolist() == [0x55] * 70


def test_values_outside_the_field_and_a_reducible_modulus_stay_inside_the_buffers():
    """The call ends and writes flags only, whatever the buffers hold: stored values that are no field elements count as 0 (a
    table field would index past its tables otherwise), and a reducible modulus gives flags without meaning."""
    GF = ga.GF(3**5)
    m = 4
    f = _modulus(3**5, m)
    consts = PE._constants(f)
    el = _elements(GF, m, 70, 5)
    n_exps, limbs, exps = PS._cofactor_exponents(3**5, m)
    t = el._t.contiguous().clone()
    expect = torch.zeros(70, dtype=torch.uint8, device=t.device)
    guard = torch.full((72,), 0x55, dtype=torch.uint8, device=t.device)
    bad = t.clone()
    bad[5, 2] = 250  # 243 .. 255 are no elements of GF(3^5)
    as_zero = t.clone()
    as_zero[5, 2] = 0
    assert _call(GF._handle, as_zero, consts.f_t, m, L.U8, exps, n_exps, limbs, consts.mats, consts.mats.shape[0], expect) == L.OK
    assert _call(GF._handle, bad, consts.f_t, m, L.U8, exps, n_exps, limbs, consts.mats, consts.mats.shape[0], guard[1:71]) == L.OK
    assert guard[1:71].cpu().tolist() == expect.cpu().tolist() and int(guard[0]) == 0x55 and int(guard[71]) == 0x55
    reducible = torch.tensor([1, 0, 0, 0, 0], dtype=torch.uint8, device=t.device)  # x^4
    assert _call(GF._handle, t, reducible, m, L.U8, exps, n_exps, limbs, consts.mats, consts.mats.shape[0], guard[1:71]) == L.OK
    torch.cuda.synchronize()
    assert int(guard[0]) == 0x55 and int(guard[71]) == 0x55


# ---- exhaustive sweeps of about 2^16 residues --------------------------------------------------------------------------------------
def _normal_count(q, m):
    f = ga.Poly(ga.GF(q)(np.array([1] + [0] * (m - 1) + [ga.GF(q).characteristic - 1], dtype=object)))
    n = q**m
    for p in f.factors()[0]:
        n = n // q**p.degree * (q**p.degree - 1)
    return n


def _euler_phi(n):
    for r in nt.factors(n)[0]:
        n = n // r * (r - 1)
    return n


@pytest.mark.parametrize("q, m", [(2, 16), (2**8, 2)])
def test_exhaustive_sweep(q, m):
    GF = ga.GF(q)
    f = _modulus(q, m)
    rng = random.Random(q + m)
    sample = sorted(rng.sample(range(q**m), 200))
    el = GF(np.array([[(v // q**(m - 1 - j)) % q for j in range(m)] for v in sample], dtype=object))
    for primitive, every, count, by_route in ((False, ga.normal_elements, _normal_count(q, m), _normal_by_rank),
                                              (True, ga.primitive_elements, _euler_phi(q**m - 1), _primitive_by_powers)):
        got = every(f)
        ints = PE._all_integers(f, primitive, q)  # the same sweep as integers: the list holds one Poly for each, in this order
        assert len(got) == len(ints) == count and ints == sorted(set(ints)) and ints[0] >= q
        for k in [0, 1, len(got) - 1] + rng.sample(range(len(got)), 40):
            assert int(got[k]) == ints[k] and got[k] == ga.Poly.Int(ints[k], field=GF)
        members = set(ints)
        assert [v in members for v in sample] == by_route(el, f).tolist()


def test_class_properties_of_gf_2_16():
    GF = ga.GF(2**16)
    norm, prim = GF.normal_elements, GF.primitive_elements
    assert norm.size == 2**15 and prim.size == _euler_phi(2**16 - 1)
    assert int(GF.normal_element) == int(norm[0])
    assert np.all(GF(np.array(random.Random(1).sample([int(v) for v in prim.numpy()], 64), dtype=object)).multiplicative_order() == 2**16 - 1)
    # normal over GF(2) with p | m: exactly the elements of trace 1
    assert np.all(norm.field_trace() == 1)
