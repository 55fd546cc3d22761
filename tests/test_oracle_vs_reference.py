"""Pins oracle/gf_oracle.c (and the host-side field factory / number theory) against the reference itself.

Every value the reference contributes goes through ref(key, thunk).  `tests/golden/generate_golden.py reference_live` runs this
module with GOLDEN_RECORD_REFERENCE=1 next to the reference (imported in place, oracle/ref_shim): the thunks run, every assertion is
checked live, and the values are written to tests/golden/reference_live.json.  Otherwise the thunks never run and the values are read
back from that fixture, so the suite needs nothing outside the repository.  Arrays of more than 1024 elements are recorded as their
length and SHA-256 over the decimal values."""
import hashlib
import json
import os
import sys
import warnings

import numpy as np
import pytest

from oracle import gf_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RECORDING = os.environ.get("GOLDEN_RECORD_REFERENCE") == "1"
if RECORDING:
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "oracle", "ref_shim"))
    import load_reference  # noqa: E402

    _REC = {}
else:
    with open(os.path.join(GOLDEN, "reference_live.json")) as _f:
        _REC = json.load(_f)


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    if RECORDING:
        with open(os.path.join(os.environ.get("GOLDEN_OUT", GOLDEN), "reference_live.json"), "w") as f:
            json.dump(_REC, f, sort_keys=True, separators=(",", ":"))


def _ints(x):
    return [int(v) for v in np.asarray(x).ravel()]


def _digest(vals):
    return {"n": len(vals), "sha256": hashlib.sha256(",".join(map(str, vals)).encode()).hexdigest()}


def _store(v):
    if isinstance(v, dict):
        return {k: _store(e) for k, e in v.items()}
    if isinstance(v, (list, tuple)):
        return [_store(e) for e in v]
    if v is None or isinstance(v, (bool, str)):
        return v
    if isinstance(v, (np.bool_, np.integer, int)):
        return v.item() if isinstance(v, np.generic) else v
    vals = _ints(v)
    return _digest(vals) if len(vals) > 1024 else vals


def ref(key, thunk):
    """The reference's value for `key`: computed now (recording run) or read back from tests/golden/reference_live.json."""
    if RECORDING:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _REC[key] = _store(thunk())
    return _REC[key]


def _ref_field(order, **kw):
    """The reference's field (recording run only; None otherwise, where no thunk that uses it runs)."""
    if not RECORDING:
        return None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return load_reference.ref_field(order, **kw)


def _pair(order, lookup=False, **kw):
    GF = _ref_field(order, **kw)
    c, d, irr, prim = ref(f"field/{order}/{sorted(kw.items())}", lambda: [GF.characteristic, GF.degree,
                                                                          int(GF.irreducible_poly) if GF.degree > 1 else None,
                                                                          int(GF.primitive_element)])
    F = O.OracleField(c, d, irr, prim, lookup=lookup)
    return GF, F


def _eq(x, rec):
    vals = _ints(x)
    return _digest(vals) == rec if isinstance(rec, dict) else vals == rec


def _ref_tables(GF):
    GF.compile("jit-lookup")
    t = [GF._EXP, GF._LOG, GF._ZECH_LOG, int(GF._ZECH_E)]
    GF.compile("python-calculate")
    return t


@pytest.mark.parametrize("order,kw", [(2, {}), (4, {}), (2**8, {}), (5, {}), (31, {}), (3191, {}), (3**4, {}), (7**3, {}),
                                      (3**5, {}), (65537, {}), (2**8, dict(irreducible_poly=283, primitive_element=19)),
                                      (7**3, dict(irreducible_poly=643, primitive_element=244)), (2147483647, {}),
                                      (2**32, {}), (7340033, {}), (2**64 - 2**32 + 1, {}), (251**3, {})])
def test_elementwise_against_reference(order, kw):
    rng = np.random.default_rng(order % 9973)
    n = 120
    for lookup in ([False, True] if 2 < order <= 2**16 else [False]):
        GF, F = _pair(order, lookup, **kw)
        k = f"elementwise/{order}/{sorted(kw.items())}/{lookup}/"
        a = [int(rng.integers(0, 2**62)) * 3 % order for _ in range(n)]
        b = [int(rng.integers(0, 2**62)) * 5 % order for _ in range(n)]
        a[:3] = [0, 0, 0]
        b[1:4] = [0, 0, 0]
        oa, ob = np.array(a, dtype=object), np.array(b, dtype=object)
        assert (_eq(F.add(oa, ob), ref(k + "add", lambda: GF(a) + GF(b))) and _eq(F.sub(oa, ob), ref(k + "sub", lambda: GF(a) - GF(b)))
                and _eq(F.mul(oa, ob), ref(k + "mul", lambda: GF(a) * GF(b))))
        assert _eq(F.neg(oa), ref(k + "neg", lambda: -GF(a)))
        bnz = [v or 1 for v in b]
        assert _eq(F.div(oa, np.array(bnz, dtype=object)), ref(k + "div", lambda: GF(a) / GF(bnz)))
        assert _eq(F.recip(np.array(bnz, dtype=object)), ref(k + "recip", lambda: GF(bnz) ** -1))
        e = rng.integers(-20, 40, n)
        anz = [v or 1 for v in a]
        assert _eq(F.pow(np.array(anz, dtype=object), e), ref(k + "pow", lambda: GF(anz) ** e))
        if lookup:
            E, Lg, Z, ze = F.tables()
            rE, rLg, rZ, rze = ref(k + "tables", lambda: _ref_tables(GF))
            assert _eq(E, rE) and _eq(Lg, rLg) and _eq(Z, rZ)
            assert ze == rze


@pytest.mark.parametrize("order,n", [(769, 4), (65537, 256), (7340033, 64), (31, 30), (31, 15), (2**8, 255), (3**5, 22),
                                     (2**64 - 2**32 + 1, 32), (5**3, 124)])
def test_fft_against_reference(order, n):
    rng = np.random.default_rng(n)
    GF, F = _pair(order, lookup=order <= 2**16 and order != 31)
    x = [int(v) for v in rng.integers(0, min(order, 2**62), n)]
    assert _eq(F.ntt(x), ref(f"fft/{order}/{n}/forward", lambda: np.fft.fft(GF(x))))
    assert _eq(F.ntt(x, inverse=True), ref(f"fft/{order}/{n}/inverse", lambda: np.fft.ifft(GF(x))))


@pytest.mark.parametrize("order,n,k,c,shorten", [(16, 15, 9, 1, 0), (16, 15, 9, 1, 3), (16, 15, 11, 3, 0), (81, 16, 10, 1, 0),
                                                 (27, 26, 20, 1, 0), (27, 13, 7, 1, 2), (256, 255, 223, 1, 0),
                                                 (31, 30, 22, 1, 0)])
def test_reed_solomon_against_reference(order, n, k, c, shorten):
    galois = load_reference.load() if RECORDING else None
    rng = np.random.default_rng(n * 100 + k)
    kw = dict(irreducible_poly=ref("matlab_primitive_poly/2/8", lambda: int(galois.matlab_primitive_poly(2, 8)))) if order == 256 else {}
    GF, F = _pair(order, lookup=True, **kw)
    rs = galois.ReedSolomon(n, k, field=GF, c=c) if RECORDING else None
    key = f"rs/{order}/{n}/{k}/{c}/{shorten}/"
    R = O.OracleRS(F, n, k, c=c, alpha=ref(key + "alpha", lambda: int(rs.alpha)))
    assert (_eq(R.generator_poly, ref(key + "generator_poly", lambda: rs.generator_poly.coeffs)) and _eq(R.G, ref(key + "G", lambda: rs.G))
            and _eq(R.H, ref(key + "H", lambda: rs.H)))
    ks, ns, N = k - shorten, n - shorten, 6
    M = rng.integers(0, order, (N, ks))
    C = R.encode(M)
    assert _eq(C, ref(key + "encode", lambda: rs.encode(GF(M))))
    t = (n - k) // 2
    Rx = np.asarray(C).astype(np.int64).copy()
    E = np.zeros((N, ns), dtype=bool)
    for i in range(N):
        ne = min([0, t, t + 1, t // 2, 1, t + 3][i], ns)
        pos = rng.choice(ns, ne, replace=False)
        Rx[i, pos] = (Rx[i, pos] + rng.integers(1, order, ne)) % order
        if i >= 3:
            nu = min([2, n - k, n - k + 1][i % 3], ns)
            E[i, rng.choice(ns, nu, replace=False)] = True
    dref, nref = ref(key + "decode", lambda: rs.decode(GF(Rx), erasures=E, output="codeword", errors=True))
    dmine, nmine = R.decode(Rx, erasures=E)
    assert np.asarray(nmine).shape == (N,) and _eq(nmine, nref) and _eq(dmine, dref)
    assert np.asarray(R.detect(Rx)).shape == (N,) and _eq(R.detect(Rx), ref(key + "detect", lambda: rs.detect(GF(Rx))))


# ---- the "next" rows: BCH decoding, linear algebra, polynomial evaluation and logarithms, live against the reference ----
@pytest.mark.parametrize("p,n,k,d,c,shorten", [(2, 15, 7, None, 1, 0), (2, 31, None, 7, 1, 5), (2, 63, 45, None, 1, 0), (3, 26, 14, None, 1, 0),
                                                (3, 13, None, 5, 3, 2), (2, 15, None, 7, 3, 0)])
def test_bch_against_reference(p, n, k, d, c, shorten):
    key = f"bch/{p}/{n}/{k}/{d}/{c}/{shorten}/"
    galois = GFp = ext = bch = None
    if RECORDING:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            galois = load_reference.load()
            GFp = load_reference.ref_field(p)
            m = galois.ilog(n, p) + 1
            ext = load_reference.ref_field(p**m, irreducible_poly=galois.matlab_primitive_poly(p, m))
            bch = galois.BCH(n, k, d, field=GFp, extension_field=ext, c=c)
    m, irr, prim = ref(key + "extension_field", lambda: [ext.degree, int(ext.irreducible_poly), int(ext.primitive_element)])
    alpha, bk, bd, bt = ref(key + "code", lambda: [int(bch.alpha), bch.k, bch.d, bch.t])
    Fe = O.OracleField(p, m, irr, prim, lookup=True)
    B = O.OracleBCH(Fe, n, k, d=d, alpha=alpha, c=c)
    assert (B.k, B.d) == (bk, bd)
    assert B.generator_poly == ref(key + "generator_poly", lambda: [int(v) for v in bch.generator_poly.coeffs])
    assert _eq(B.G, ref(key + "G", lambda: bch.G)) and _eq(B.H, ref(key + "H", lambda: bch.H))
    rng = np.random.default_rng(n * 7 + c)
    ks, ns, t = bk - shorten, n - shorten, bt
    for trial in range(8):
        msg = rng.integers(0, p, ks)
        cw = np.array(ref(f"{key}{trial}/encode", lambda: bch.encode(GFp(msg))), dtype=np.int64)
        assert _eq(B.encode(msg)[0], _ints(cw))
        r = cw.copy()
        ne = int(rng.integers(0, t + 2))
        pos = rng.choice(ns, min(ne, ns), replace=False)
        r[pos] = (r[pos] + rng.integers(1, p, pos.size)) % p
        er = np.zeros(ns, dtype=bool)
        if trial % 3 == 2:
            er[rng.choice(ns, int(rng.integers(0, bd)), replace=False)] = True
        odec, onerr = B.decode(r, er if er.any() else None)

        def decode():
            try:
                return bch.decode(GFp(r), erasures=er if er.any() else None, output="codeword", errors=True)
            except (ValueError, OverflowError):
                return "rejected"

        got = ref(f"{key}{trial}/decode", decode)
        if got == "rejected":
            assert ((odec < 0) | (odec >= p)).any()  # the reference rejects symbols outside GF(p)
            continue
        dec, nerr = got
        assert int(nerr) == int(onerr[0]) and _eq(odec[0], dec)
        assert ref(f"{key}{trial}/detect", lambda: bool(bch.detect(GFp(r)))) == bool(B.detect(r)[0])


@pytest.mark.parametrize("order", [2, 5, 31, 2**8, 3**3, 65537, 2147483647, 2**64 - 2**32 + 1])
def test_linear_algebra_against_reference(order):
    GF, F = _pair(order)
    rng = np.random.default_rng(order % 1009)

    def rnd(shape):
        return np.array([int(rng.integers(0, 2**62)) % order for _ in range(int(np.prod(shape)))], dtype=object).reshape(shape)

    def inv_or_singular(gA):
        try:
            return np.linalg.inv(gA)
        except np.linalg.LinAlgError:
            return "singular"

    def lu_or_none(gA):
        try:
            return gA.lu_decompose()
        except ValueError:
            return "no LU"

    for m, n in [(1, 1), (3, 3), (4, 6), (6, 4), (5, 5)]:
        A = rnd((m, n))
        if m == 5:
            A[2] = A[0]  # rank-deficient
            A[:, 1] = 0
        key = f"linalg/{order}/{m}x{n}/"
        gA = GF(A) if RECORDING else None
        assert _eq(F.row_reduce(A)[0], ref(key + "row_reduce", lambda: gA.row_reduce()))
        P, Lm, U, _ = F.plu_decompose(A)
        rp, rl, ru = ref(key + "plu_decompose", lambda: gA.plu_decompose())
        assert _eq(P, rp) and _eq(Lm, rl) and _eq(U, ru)
        B = rnd((n, 3))
        assert _eq(F.matmul(A, B), ref(key + "matmul", lambda: gA @ GF(B)))
        assert F.matrix_rank(A) == ref(key + "matrix_rank", lambda: int(np.linalg.matrix_rank(gA)))
        for op in ("row_space", "column_space", "left_null_space", "null_space"):
            want = ref(key + op, lambda: getattr(gA, op)())
            got = getattr(F, op)(A)
            assert len(want) == got.size and _eq(got, want), op
        if m == n:
            assert F.det(A) == ref(key + "det", lambda: int(np.linalg.det(gA)))
            inv = ref(key + "inv", lambda: inv_or_singular(gA))
            if inv == "singular":
                with pytest.raises(np.linalg.LinAlgError):
                    F.inv(A)
            else:
                assert _eq(F.inv(A), inv)
                b = rnd((n,))
                assert _eq(F.solve(A, b), ref(key + "solve", lambda: np.linalg.solve(gA, GF(b))))
            lu = ref(key + "lu_decompose", lambda: lu_or_none(gA))
            if lu == "no LU":
                with pytest.raises(ValueError):
                    F.lu_decompose(A)
            else:
                rl2, ru2 = lu
                l2, u2 = F.lu_decompose(A)
                assert _eq(l2, rl2) and _eq(u2, ru2)


@pytest.mark.parametrize("order", [31, 2**8, 3**4, 65537])
def test_poly_evaluate_and_log_against_reference(order):
    GF, F = _pair(order, lookup=True)
    rng = np.random.default_rng(order)
    coeffs = rng.integers(0, order, 9)
    coeffs[0] = 1
    x = rng.integers(0, order, 40)
    assert _eq(F.poly_eval(coeffs, x), ref(f"poly_evaluate/{order}", lambda: load_reference.load().Poly(coeffs, field=GF)(GF(x))))
    xs = rng.integers(1, order, 40)
    _, LOG, _, _ = F.tables()
    assert _eq(LOG[xs], ref(f"log/{order}", lambda: np.log(GF(xs))))


FACTORY_ORDERS = [2, 3, 5, 7, 31, 251, 257, 509, 3191, 8191, 32749, 65521, 65537, 7340033, 2147483647, 4294967291, 2**61 - 1,
                  2**64 - 2**32 + 1, 18446744073709551557, 2**2, 2**3, 2**4, 2**8, 2**9, 2**10, 2**12, 2**13, 2**14, 2**15, 2**16, 2**17,
                  2**20, 2**24, 2**31, 2**32, 3**2, 3**4, 3**5, 3**7, 3**9, 3**10, 5**3, 5**5, 7**3, 7**5, 11**4, 13**4, 127**2, 251**2,
                  251**3, 31**5, 2**100, 36893488147419103183, 109987**4]


@pytest.mark.parametrize("order", FACTORY_ORDERS)
def test_field_factory_matches_the_reference(order):
    """galois_amd.GF(order) against galois.GF(order) of the reference: name, characteristic / degree / order, default
    irreducible polynomial (Conway table), default primitive element, is_primitive_poly, the dtype list and the array-free parts
    of `properties` -- the host side of SURVEY.md 8(a1) / (a3) for every size class the device kernels distinguish."""
    import galois_amd as ga

    R = _ref_field(order)
    r = ref(f"factory/{order}", lambda: dict(
        name=R.name, characteristic=R.characteristic, degree=R.degree, order=R.order, irreducible_poly=int(R.irreducible_poly),
        primitive_element=int(R.primitive_element), is_primitive_poly=bool(R.is_primitive_poly), is_prime_field=R.is_prime_field,
        is_extension_field=R.is_extension_field, dtypes=[np.dtype(d).name for d in R.dtypes], irreducible_poly_str=str(R.irreducible_poly)))
    G = ga.GF(order)
    assert (G.name, G.characteristic, G.degree, G.order) == (r["name"], r["characteristic"], r["degree"], r["order"])
    assert int(G.irreducible_poly) == r["irreducible_poly"]
    assert int(G.primitive_element) == r["primitive_element"]
    assert bool(G.is_primitive_poly) == r["is_primitive_poly"]
    assert G.is_prime_field == r["is_prime_field"] and G.is_extension_field == r["is_extension_field"]
    assert [np.dtype(d) for d in G.dtypes] == [np.dtype(d) for d in r["dtypes"]]
    assert str(G.irreducible_poly) == r["irreducible_poly_str"]


def test_number_theory_matches_the_reference():
    """galois_amd/_numtheory.py (what the field factory and galois.ntt's modulus choice stand on) against the reference's functions
    of the same names: primality, factorisation, primitive roots, irreducibility / primitivity of polynomials, the MATLAB
    default polynomials and the Conway table."""
    from galois_amd import _numtheory as nt

    galois = load_reference.load() if RECORDING else None
    rng = np.random.default_rng(7)
    numbers = [1, 2, 3, 4, 31, 255, 256, 257, 65535, 65536, 65537, 7340033, 2**31 - 1, 2**32 - 1, 2**32 + 1, 4294967291, 2**61 - 1,
               2**64 - 2**32 + 1, 2**64 - 2**32, 3**20, 2**63, 1000003 * 999983] + [int(v) for v in rng.integers(2, 2**40, 40)]
    for n in numbers:
        assert nt.is_prime(n) == ref(f"is_prime/{n}", lambda: bool(galois.is_prime(n))), n
        if n > 1:
            f, e = ref(f"factors/{n}", lambda: galois.factors(n))
            assert nt.factors(n) == (f, e), n
    for p in (2, 3, 5, 7, 31, 257, 769, 7681, 12289, 65537, 7340033, 469762049, 2**31 - 1, 2**61 - 1, 2**64 - 2**32 + 1):
        assert nt.primitive_root(p) == ref(f"primitive_root/{p}", lambda: int(galois.primitive_root(p))), p
    for p, m in ((2, 2), (2, 8), (2, 16), (2, 32), (3, 5), (3, 10), (5, 4), (7, 3), (127, 2), (251, 3), (2, 100), (109987, 4)):
        assert nt.conway_poly(p, m) == ref(f"conway_poly/{p}/{m}", lambda: int(galois.conway_poly(p, m))), (p, m)
    for p, m in ((2, 2), (2, 3), (2, 4), (2, 7), (2, 8), (2, 16)):  # (odd p: the reference's polynomial search needs its JIT arrays)
        assert nt.matlab_primitive_poly(p, m) == ref(f"matlab_primitive_poly/{p}/{m}", lambda: int(galois.matlab_primitive_poly(p, m))), (p, m)
    for val in (0x11B, 0x11D, 0x11C, 0x1002D, 0x10001, 0b111, 0b1011, 0b1111, 0x100008299):  # over GF(2)
        coeffs = nt.poly_from_int(val, 2)
        assert nt.is_irreducible(coeffs, 2) == ref(f"is_irreducible/2/{val}", lambda: bool(galois.Poly.Int(val).is_irreducible())), hex(val)
        if nt.is_irreducible(coeffs, 2):
            assert nt.is_primitive_poly(coeffs, 2) == ref(f"is_primitive/2/{val}", lambda: bool(galois.Poly.Int(val).is_primitive())), hex(val)


@pytest.mark.parametrize("x,size", [([1, 2, 3, 4], None), ([1, 2, 3, 4], 8), ([0, 0, 0, 0], None), ([100, 200, 300], 4), ([65536] * 16, None),
                                    ([12288] * 8, 1024), ([7340032, 5], 1 << 20), (list(range(30)), 32), ([2**31, 1, 2, 3], None)])
def test_default_ntt_modulus_matches_the_reference(x, size):
    """galois.ntt(x, size) without a modulus: the field the reference's result lives in against galois_amd._ntt._default_modulus."""
    from galois_amd._ntt import _default_modulus

    galois = load_reference.load() if RECORDING else None
    n = size or len(x)
    want = _default_modulus(max(x), n)
    if n <= 64:  # run the reference's transform itself for the small cases
        assert ref(f"ntt_characteristic/{x}/{size}", lambda: int(type(galois.ntt(x, size=size)).characteristic)) == want
    m = int(np.ceil(max(x) / n))
    while not ref(f"is_prime/{m * n + 1}", lambda: bool(galois.is_prime(m * n + 1))):
        m += 1
    assert want == m * n + 1
