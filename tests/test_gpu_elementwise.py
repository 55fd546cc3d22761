"""Parity of the element-wise HIP kernels (through the C-ABI, via the FieldArray API) against the golden fixtures and
the oracle.  Bit-exact."""
import json

import numpy as np
import pytest

import galois_amd as ga
from oracle import gf_oracle as O
from tests import helpers as H

pytestmark = pytest.mark.gpu


def field_from_props(props):
    p, m = props["characteristic"], props["degree"]
    if m == 1:
        return ga.GF(p, primitive_element=int(props["primitive_element"]))
    return ga.GF(p, m, irreducible_poly=[int(c) for c in props["irreducible_poly"]],
                 primitive_element=int(props["primitive_element"]))


@pytest.mark.parametrize("tag", H.SAGE_FIELDS)
@pytest.mark.parametrize("mode", ["jit-lookup", "jit-calculate"])
def test_sage_vectors(tag, mode):
    """The reference's own Sage-generated arithmetic tables (tests/fields/test_arithmetic.py:17-199)."""
    props, d = H.load_sage_field(tag)
    GF = field_from_props(props)
    if mode not in GF.ufunc_modes:
        pytest.skip(f"{mode} is not legal for {GF.name}")
    GF.compile(mode)
    try:
        rng = np.random.default_rng(1)
        for dtype in [GF.dtypes[0], GF.dtypes[int(rng.integers(0, len(GF.dtypes)))], GF.dtypes[-1]]:
            for op, fn in [("add", np.add), ("subtract", np.subtract), ("multiply", np.multiply), ("divide", np.true_divide)]:
                x = GF(d[f"{op}_X"].astype(np.int64), dtype=dtype)
                y = GF(d[f"{op}_Y"].astype(np.int64), dtype=dtype)
                z = fn(x.reshape(-1, 1), y.reshape(1, -1))
                assert type(z) is GF and z.dtype == np.dtype(dtype)
                H.assert_equal_ints(z.numpy(), d[f"{op}_Z"], f"{tag} {op} {dtype}")
            x = GF(d["additive_inverse_X"].astype(np.int64), dtype=dtype)
            H.assert_equal_ints((-x).numpy(), d["additive_inverse_Z"])
            x = GF(d["multiplicative_inverse_X"].astype(np.int64), dtype=dtype)
            H.assert_equal_ints(np.reciprocal(x).numpy(), d["multiplicative_inverse_Z"])
            H.assert_equal_ints((x**-1).numpy(), d["multiplicative_inverse_Z"])
            x = GF(d["power_X"].astype(np.int64), dtype=dtype)
            z = x.reshape(-1, 1) ** d["power_Y"].astype(np.int64).reshape(1, -1)
            assert z.dtype == np.dtype(dtype)
            H.assert_equal_ints(z.numpy(), d["power_Z"], f"{tag} power")
            x = GF(d["scalar_multiply_X"].astype(np.int64), dtype=dtype)
            z = x.reshape(-1, 1) * d["scalar_multiply_Y"].astype(np.int64).reshape(1, -1)
            H.assert_equal_ints(z.numpy(), d["scalar_multiply_Z"], f"{tag} scalar multiply")
    finally:
        GF.compile("auto")


@pytest.mark.parametrize("tag", ["gf256", "gf31", "gf65537", "gf7340033", "goldilocks", "gf2e32", "gf3e5", "gf251e3"])
def test_reference_outputs(tag):
    d = H.reference_outputs()
    meta = json.loads(str(d[f"ew/{tag}/meta"]))
    p, m = meta["p"], meta["m"]
    GF = ga.GF(p, m, irreducible_poly=meta["irr"], primitive_element=meta["alpha"]) if m > 1 else ga.GF(p, primitive_element=meta["alpha"])
    for mode in GF.ufunc_modes:
        GF.compile(mode)
        a, b, e = d[f"ew/{tag}/a"], d[f"ew/{tag}/b"], d[f"ew/{tag}/e"]
        conv = (lambda v: np.array([int(t) for t in v], dtype=object)) if GF.order > 2**63 else (lambda v: v.astype(np.int64))
        ga_, gb_ = GF(conv(a)), GF(conv(b))
        gbnz, ganz = GF(conv(np.where(b == 0, 1, b))), GF(conv(np.where(a == 0, 1, a)))
        H.assert_equal_ints((ga_ + gb_).numpy(), d[f"ew/{tag}/add"], "add")
        H.assert_equal_ints((ga_ - gb_).numpy(), d[f"ew/{tag}/sub"], "sub")
        H.assert_equal_ints((ga_ * gb_).numpy(), d[f"ew/{tag}/mul"], "mul")
        H.assert_equal_ints((-ga_).numpy(), d[f"ew/{tag}/neg"], "neg")
        H.assert_equal_ints((ga_ / gbnz).numpy(), d[f"ew/{tag}/div"], "div")
        H.assert_equal_ints((gbnz**-1).numpy(), d[f"ew/{tag}/recip"], "recip")
        H.assert_equal_ints((ganz**e).numpy(), d[f"ew/{tag}/pow"], "pow")
        H.assert_equal_ints((ga_ * 7).numpy(), d[f"ew/{tag}/smul"], "smul")
        H.assert_equal_ints((7 * ga_).numpy(), d[f"ew/{tag}/smul"], "rsmul")
    GF.compile("auto")


@pytest.mark.parametrize("tag", ["gf3e7", "gf2e10", "gf2e13", "gf5e5", "gf8191", "gf2e14", "gf3e9", "gf2e15", "gf32749", "gf2e16", "gf3e10",
                                 "gf65521", "gf251e2"])
def test_reference_outputs_for_table_fields_through_the_lds_kernels(tag):
    """Outputs of the reference itself for fields of 257 .. 65536 elements (tests/golden/reference_table_fields.npz), repeated to
    2^19 elements on uint16 storage so that the LDS-table kernels (not the generic ones) produce them, in every mode."""
    d = H.reference_table_fields()
    meta = json.loads(str(d[f"ew/{tag}/meta"]))
    p, m = meta["p"], meta["m"]
    GF = ga.GF(p, m, irreducible_poly=meta["irr"], primitive_element=meta["alpha"]) if m > 1 else ga.GF(p, primitive_element=meta["alpha"])
    reps = 2048
    a, b, e = d[f"ew/{tag}/a"], d[f"ew/{tag}/b"], d[f"ew/{tag}/e"]
    big = lambda v: np.tile(np.asarray(v), reps)
    mk = lambda v: GF(big(v).astype(np.uint16), dtype=np.uint16)
    try:
        for mode in list(GF.ufunc_modes) + ["auto"]:
            GF.compile(mode)
            ga_, gb_ = mk(a), mk(b)
            gbnz, ganz = mk(np.where(b == 0, 1, b)), mk(np.where(a == 0, 1, a))
            H.assert_equal_ints((ga_ + gb_).numpy(), big(d[f"ew/{tag}/add"]), "add")
            H.assert_equal_ints((ga_ - gb_).numpy(), big(d[f"ew/{tag}/sub"]), "sub")
            H.assert_equal_ints((ga_ * gb_).numpy(), big(d[f"ew/{tag}/mul"]), "mul")
            H.assert_equal_ints((-ga_).numpy(), big(d[f"ew/{tag}/neg"]), "neg")
            H.assert_equal_ints((ga_ / gbnz).numpy(), big(d[f"ew/{tag}/div"]), "div")
            H.assert_equal_ints(np.reciprocal(gbnz).numpy(), big(d[f"ew/{tag}/recip"]), "recip")
            H.assert_equal_ints((ganz ** big(e)).numpy(), big(d[f"ew/{tag}/pow"]), "pow")
            H.assert_equal_ints((ga_ ** 12345).numpy(), big(d[f"ew/{tag}/pow12345"]), "pow12345")
            H.assert_equal_ints((ganz ** -7).numpy(), big(d[f"ew/{tag}/pow_minus7"]), "pow_minus7")
    finally:
        GF.compile("auto")


def test_gf256_full_size_1e8_bit_exact():
    """BASELINE.json configs[1] at full size: 1e8 uint8 elements, every output byte compared with the oracle."""
    n = 100_000_000
    GF = ga.GF(2**8)
    F = O.OracleField(2, 8, 285, 2, lookup=True)
    x = np.random.default_rng(1).integers(0, 256, n, dtype=np.uint8)
    y = np.random.default_rng(2).integers(0, 256, n, dtype=np.uint8)
    gx, gy = GF(x), GF(y)
    assert np.array_equal((gx * gy).numpy(), F.ufunc_u8(O.MUL, x, y))
    ynz = np.random.default_rng(2).integers(1, 256, n, dtype=np.uint8)
    gynz = GF(ynz)
    r = np.reciprocal(gynz)
    assert np.array_equal(r.numpy(), F.ufunc_u8(O.RECIP, ynz))
    # size-independent properties: (x*y)/y == x ; x*y + x*z == x*(y+z)
    assert np.array_equal(((gx * gynz) / gynz).numpy(), x)
    z = GF(np.random.default_rng(3).integers(0, 256, n, dtype=np.uint8))
    assert np.array_equal((gx * gy + gx * z).numpy(), (gx * (gy + z)).numpy())
    with pytest.raises(ZeroDivisionError):
        np.reciprocal(gy)  # contains zeros
    with pytest.raises(ZeroDivisionError):
        gx / gy


def test_gf256_calculate_mode_and_wide_dtypes_large():
    n = 5_000_003  # odd size: exercises the vector tail
    GF = ga.GF(2**8)
    F = O.OracleField(2, 8, 285, 2, lookup=True)
    x = np.random.default_rng(11).integers(0, 256, n, dtype=np.uint8)
    y = np.random.default_rng(12).integers(1, 256, n, dtype=np.uint8)
    want_mul, want_div = F.ufunc_u8(O.MUL, x, y), F.ufunc_u8(O.DIV, x, y)
    try:
        for mode in ["jit-lookup", "jit-calculate"]:
            GF.compile(mode)
            for dtype in [np.uint8, np.int64, np.uint16]:
                gx, gy = GF(x.astype(dtype)), GF(y.astype(dtype))
                assert np.array_equal((gx * gy).numpy(), want_mul.astype(dtype)), (mode, dtype)
                assert np.array_equal((gx / gy).numpy(), want_div.astype(dtype)), (mode, dtype)
            # unaligned views (offset by one element) take the scalar path
            gx, gy = GF(x)[1:], GF(y)[1:]
            assert np.array_equal((gx * gy).numpy(), want_mul[1:])
    finally:
        GF.compile("auto")


def test_gf31_config_c1_1e6():
    """BASELINE.json configs[0]: GF(31) add / mul on 1e6 elements."""
    GF = ga.GF(31)
    F = O.OracleField(31, 1, None, 3)
    x = np.random.default_rng(1).integers(0, 31, 1_000_000, dtype=np.uint8)
    y = np.random.default_rng(2).integers(0, 31, 1_000_000, dtype=np.uint8)
    for mode in GF.ufunc_modes:
        GF.compile(mode)
        assert np.array_equal((GF(x) + GF(y)).numpy(), F.add(x, y).astype(np.uint8))
        assert np.array_equal((GF(x) * GF(y)).numpy(), F.mul(x, y).astype(np.uint8))
    GF.compile("auto")


@pytest.mark.parametrize("order", [65537, 7340033, 2147483647, 2**64 - 2**32 + 1, 2**32, 2**16, 3**5, 251**3,
                                   18446744073709551557, 4294967291])
def test_large_random_against_oracle(order):
    GF = ga.GF(order)
    p, m = GF.characteristic, GF.degree
    F = O.OracleField(p, m, int(GF.irreducible_poly) if m > 1 else None, GF._primitive_element_int, lookup=order <= 2**16)
    rng = np.random.default_rng(order % 7919)
    n = 200_001
    if order <= 2**63:
        a, b = rng.integers(0, order, n, dtype=np.uint64), rng.integers(1, order, n, dtype=np.uint64)
    else:
        a = (rng.integers(0, 2**63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)) % np.uint64(order)
        b = (rng.integers(0, 2**63, n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)) % np.uint64(order)
        b[b == 0] = 1
    a[:3] = 0
    mk = (lambda v: GF(np.array([int(t) for t in v], dtype=object))) if GF.dtypes == [np.object_] else (lambda v: GF(v.astype(GF.dtypes[-1])))
    ga_, gb_ = mk(a), mk(b)
    for mode in GF.ufunc_modes:
        GF.compile(mode)
        H.assert_equal_ints((ga_ + gb_).numpy().astype(np.uint64), F.add(a, b))
        H.assert_equal_ints((ga_ - gb_).numpy().astype(np.uint64), F.sub(a, b))
        H.assert_equal_ints((ga_ * gb_).numpy().astype(np.uint64), F.mul(a, b))
        H.assert_equal_ints((ga_ / gb_).numpy().astype(np.uint64), F.div(a, b))
        H.assert_equal_ints(np.reciprocal(gb_).numpy().astype(np.uint64), F.recip(b))
        e = rng.integers(-1000, 1000, n)
        H.assert_equal_ints((gb_**e).numpy().astype(np.uint64), F.pow(b, e))
        H.assert_equal_ints((ga_**3).numpy().astype(np.uint64), F.pow(a, np.full(n, 3)))
        H.assert_equal_ints(np.square(ga_).numpy().astype(np.uint64), F.mul(a, a))
    GF.compile("auto")


@pytest.mark.parametrize("order", [65537, 2147483647, 4294967291, 2**64 - 2**32 + 1, 18446744073709551557, 2**32, 251**3])
def test_power_with_one_exponent_per_element_edges(order):
    """np.power with an exponent array on the calculate-mode kernels (ew_intarg_kernel: eight powers per lane share one inversion
    for the negative exponents among them): zero bases under zero / positive exponents, exponents far beyond q - 1 on both
    sides, lengths around the eight-per-lane rounds, and 0 ** negative anywhere in the array raising as the reference does
    (_lookup.py:262-263, _calculate.py:447-489)."""
    GF = ga.GF(order)
    p, m = GF.characteristic, GF.degree
    F = O.OracleField(p, m, int(GF.irreducible_poly) if m > 1 else None, GF._primitive_element_int, lookup=False)
    rng = np.random.default_rng(order % 1013)
    mk = (lambda v: GF(np.array([int(t) for t in v], dtype=object))) if GF.dtypes == [np.object_] else (lambda v: GF(v.astype(GF.dtypes[-1])))
    for n in (1, 7, 8, 9, 1000, 65536 * 8 + 5, 1_500_003):
        if order <= 2**63:
            a = rng.integers(0, order, n, dtype=np.uint64)
        else:
            a = (rng.integers(0, 2**63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)) % np.uint64(order)
        e = rng.integers(-60, 1200, n)
        big = rng.random(n) < 0.02
        e[big] = rng.integers(-(2**62), 2**62, int(big.sum()))
        zero = rng.random(n) < 0.05
        a[zero] = 0
        e[zero] = np.abs(e[zero]) * (rng.random(int(zero.sum())) < 0.5)  # zero bases: exponent 0 or positive
        e[a == 0] = np.abs(e[a == 0])  # (zeros the generator drew by itself)
        H.assert_equal_ints((mk(a) ** e).numpy().astype(np.uint64), F.pow(a, e), f"n={n}")
    a = np.arange(1, 2001, dtype=np.uint64) % np.uint64(min(order, 2**63))
    a[1234] = 0
    e = np.full(2000, 5)
    e[1234] = -3
    with pytest.raises(ZeroDivisionError):
        mk(a) ** e
    e[1234] = 0
    assert int((mk(a) ** e).numpy()[1234]) == 1


def test_reductions_and_outer():
    for order in [2**8, 31, 3**5, 65537]:
        GF = ga.GF(order)
        p, m = GF.characteristic, GF.degree
        F = O.OracleField(p, m, int(GF.irreducible_poly) if m > 1 else None, GF._primitive_element_int)
        rng = np.random.default_rng(5)
        a = rng.integers(1, order, (37, 1000)).astype(GF.dtypes[-1])
        g = GF(a)
        for mode in GF.ufunc_modes:
            GF.compile(mode)
            for ufunc, fold in [(np.add, F.add), (np.multiply, F.mul), (np.subtract, F.sub), (np.true_divide, F.div)]:
                want = a[:, 0].astype(np.uint64)
                for j in range(1, a.shape[1]):
                    want = fold(want, a[:, j].astype(np.uint64))
                got = ufunc.reduce(g, axis=1)
                assert type(got) is GF and got.shape == (37,)
                H.assert_equal_ints(got.numpy().astype(np.uint64), want, f"{order} {ufunc.__name__} reduce")
            big = GF(rng.integers(1, order, 3_000_000).astype(GF.dtypes[0]))
            want = 0
            bh = big.numpy().astype(np.uint64)
            # tree-vs-fold: add is associative, fold with the oracle in chunks
            acc = bh[:1000].copy()
            for s in range(1000, 3_000_000, 1000):
                acc = F.add(acc, bh[s:s + 1000])
            tot = np.uint64(0)
            for v in acc:
                tot = F.add([tot], [v])[0]
            assert int(np.add.reduce(big).numpy()) == int(tot)
            for ufunc, fold in [(np.add, F.add), (np.multiply, F.mul), (np.subtract, F.sub), (np.true_divide, F.div)]:
                sub = a[:5, :700]
                want = np.empty(sub.shape, dtype=np.uint64)
                want[:, 0] = sub[:, 0]
                for j in range(1, sub.shape[1]):
                    want[:, j] = fold(want[:, j - 1], sub[:, j].astype(np.uint64))
                got = ufunc.accumulate(GF(sub), axis=1)
                H.assert_equal_ints(got.numpy().astype(np.uint64), want, f"{order} {ufunc.__name__} accumulate")
                got0 = ufunc.accumulate(GF(np.ascontiguousarray(sub.T)), axis=0)
                H.assert_equal_ints(got0.numpy().astype(np.uint64), want.T, f"{order} {ufunc.__name__} accumulate axis 0")
            out = np.multiply.outer(GF(a[0, :50]), GF(a[1, :60]))
            assert out.shape == (50, 60)
            H.assert_equal_ints(out.numpy().astype(np.uint64), F.mul(a[0, :50, None].astype(np.uint64), a[1, None, :60].astype(np.uint64)))
        GF.compile("auto")
        with pytest.raises(ValueError):
            np.negative.reduce(g)
        with pytest.raises(ValueError):
            np.power.reduce(g)
        with pytest.raises(ValueError):
            np.reciprocal.accumulate(g)


def test_api_semantics_and_errors():
    GF = ga.GF(2**8)
    x = GF([1, 2, 3, 0], dtype=np.int32)
    y = GF([5, 6, 7, 9])
    assert (x * y).dtype == np.int32 and (y * x).dtype == np.uint8  # dtype of `self` is kept (_ufunc.py:675)
    assert np.array_equal(np.asarray(x + y), [4, 4, 4, 9])
    assert repr(GF([1, 2])) == "GF([1, 2], order=2^8)"
    for bad in (lambda: x + 1, lambda: 1 + x, lambda: x - 1, lambda: x / 2, lambda: np.add(x, np.array([1, 2, 3, 4]))):
        with pytest.raises(TypeError):
            bad()
    with pytest.raises(TypeError):
        x ** y
    with pytest.raises(TypeError):
        x * 1.5
    with pytest.raises(ZeroDivisionError):
        x ** -1
    with pytest.raises(ZeroDivisionError):
        y / x
    assert int((GF(0) ** 0)) == 1  # 0**0 == 1 (_lookup.py:262-263)
    with pytest.raises(ValueError):
        GF([256])
    with pytest.raises(ValueError):
        GF([-1])
    with pytest.raises(TypeError):
        GF([1.0])
    with pytest.raises(TypeError):
        GF([1], dtype=np.int8)
    with pytest.raises(TypeError):
        x.astype(np.float32)
    with pytest.raises(NotImplementedError):
        np.sin(x)
    q, r = divmod(y, GF([1, 2, 3, 4]))
    assert np.array_equal(r.numpy(), [0, 0, 0, 0]) and np.array_equal((y % y).numpy(), [0, 0, 0, 0])
    # empty and 0-D arrays
    e = GF(np.array([], dtype=np.uint8))
    assert (e * e).shape == (0,) and np.reciprocal(e).shape == (0,)
    s = GF(7)
    assert s.shape == () and int(s * s) == int(GF([7])[0] * GF([7])[0])
    z = GF.Zeros((3, 4)); o = GF.Ones((3, 4)); assert np.array_equal((z + o).numpy(), np.ones((3, 4)))
    r1 = GF.Random((5, 6), seed=3)
    assert np.array_equal(r1.numpy(), np.random.default_rng(3).integers(0, 256, (5, 6), dtype=np.uint8))
    x[0] = 200
    assert int(x[0]) == 200
    with pytest.raises(ValueError):
        x[0] = 300
    # zero-copy adoption of a torch tensor
    import torch
    t = torch.arange(0, 256, dtype=torch.uint8, device="cuda")
    v = GF(t, copy=False)
    assert v.torch().data_ptr() == t.data_ptr()
    with pytest.raises(ValueError):
        ga.GF(31)(t)


def test_mixed_storage_widths_keep_large_unsigned_values():
    """uint32 / uint16 arrays sit in same-width signed torch storage: widening to int64 must not sign-extend."""
    GF = ga.GF(2**32)
    a = np.array([2**31, 2**32 - 1, 5, 2**31 + 12345], dtype=np.uint32)
    x32, x64 = GF(a, dtype=np.uint32), GF(a.astype(np.int64), dtype=np.int64)
    assert np.array_equal(x32.astype(np.int64).numpy(), a.astype(np.int64))
    assert np.array_equal((x64 + x32).numpy(), np.zeros(4, dtype=np.int64))
    assert np.array_equal((x64 * x32).numpy(), (x64 * x64).numpy())
    assert np.array_equal(x64 == x32, np.ones(4, dtype=bool))
    G16 = ga.GF(2**16)
    b = np.array([2**15, 2**16 - 1, 7], dtype=np.uint16)
    assert np.array_equal((G16(b.astype(np.int32), dtype=np.int32) * G16(b)).numpy(), (G16(b) * G16(b)).numpy().astype(np.int32))


@pytest.mark.parametrize("order", [3**5, 2**8, 7**3, 251**3, 2**32, 31, 2**16])
def test_vector_and_Vector(order):
    """FieldArray.vector / FieldArray.Vector (_fields/_array.py:383-491): base-p digits, degree m-1 first, and back."""
    GF = ga.GF(order)
    p, m = GF.characteristic, GF.degree
    rng = np.random.default_rng(order % 1000)
    x = rng.integers(0, order, (5, 7), dtype=np.uint64)
    x[0, :3] = [0, order - 1, p % order]
    v = GF([[int(e) for e in r] for r in x]).vector()
    assert type(v) is GF.prime_subfield and v.shape == (5, 7, m)
    want = np.zeros((5, 7, m), dtype=np.uint64)
    y = x.copy()
    for i in range(m - 1, -1, -1):  # the reference's own loop (_fields/_array.py:485-489)
        want[..., i] = y % p
        y //= p
    assert np.array_equal(v.numpy().astype(np.uint64), want)
    back = GF.Vector(v)
    assert type(back) is GF and np.array_equal(back.numpy().astype(np.uint64), x)
    assert np.array_equal(GF.Vector(want.astype(np.int64).tolist()).numpy().astype(np.uint64), x)
    with pytest.raises(ValueError):
        GF.Vector(np.zeros((2, m + 1), dtype=np.int64))
    # addition in GF(p^m) is digit-wise addition in GF(p)
    a, b = GF.Random(100, seed=1), GF.Random(100, seed=2)
    assert np.array_equal((a + b).vector().numpy(), (a.vector() + b.vector()).numpy())


def test_gf256_arrays_beyond_the_infinity_cache():
    """2^28 + 12345 elements: the table kernel switches to claimed blocks (and the generic kernels to flat launches); the
    whole result is compared with the oracle, and a zero divisor anywhere still raises."""
    GF = ga.GF(2**8)
    F = O.OracleField(2, 8, 285, 2, lookup=True)
    n = (1 << 28) + 12345
    rng = np.random.default_rng(123)
    a = rng.integers(0, 256, n, dtype=np.uint8)
    b = rng.integers(1, 256, n, dtype=np.uint8)
    ga_, gb_ = GF(a), GF(b)
    assert np.array_equal((ga_ * gb_).numpy(), F.ufunc_u8(O.MUL, a, b))
    assert np.array_equal((ga_ / gb_).numpy(), F.ufunc_u8(O.DIV, a, b))
    assert np.array_equal((ga_ + gb_).numpy(), a ^ b)
    # unary table kernel: sliced launches above 2^28 elements
    inv = np.reciprocal(gb_).numpy()
    assert np.array_equal(inv, F.ufunc_u8(O.DIV, np.ones(n, dtype=np.uint8), b))
    assert np.array_equal((-ga_).numpy(), a)
    b[n - 7] = 0
    with pytest.raises(ZeroDivisionError):
        ga_ / GF(b)
    with pytest.raises(ZeroDivisionError):
        np.reciprocal(GF(b))


@pytest.mark.parametrize("order", [2**8, 31, 65537, 3**5, 2**32])
def test_reduceat_and_at(order):
    """ufunc.reduceat / ufunc.at (tests/fields/test_numpy_ufuncs.py TestReduceAt / TestAt) against sequential oracle folds."""
    GF = ga.GF(order)
    F = O.OracleField(GF.characteristic, GF.degree, int(GF.irreducible_poly) if GF.degree > 1 else None, int(GF.primitive_element))
    rng = np.random.default_rng(order % 97)
    a = rng.integers(1, order, 50, dtype=np.uint64)
    idx = np.array([0, 7, 7, 20, 3, 49, 10])  # increasing, repeated and decreasing entries
    ends = list(idx[1:]) + [50]
    for ufn, op in ((np.add, F.add), (np.subtract, F.sub), (np.multiply, F.mul), (np.true_divide, F.div)):
        got = ufn.reduceat(GF(a), idx).numpy().astype(np.uint64)
        want = []
        for s0, e0 in zip(idx, ends):
            seg = a[s0:e0] if e0 > s0 else a[s0:s0 + 1]
            acc = seg[0]
            for v in seg[1:]:
                acc = op([acc], [v])[0]
            want.append(acc)
        assert np.array_equal(got, np.array(want, dtype=np.uint64)), ufn.__name__
    m2 = rng.integers(0, order, (4, 50), dtype=np.uint64)
    got = np.add.reduceat(GF(m2), [0, 10, 25], axis=1).numpy().astype(np.uint64)
    for r in range(4):
        for j, (s0, e0) in enumerate(((0, 10), (10, 25), (25, 50))):
            acc = m2[r, s0]
            for v in m2[r, s0 + 1:e0]:
                acc = F.add([acc], [v])[0]
            assert got[r, j] == acc
    # at: repeated indices accumulate in order
    x = GF(a.copy())
    ii = np.array([3, 3, 5, 3, 49, 0, 5])
    vv = rng.integers(1, order, ii.size, dtype=np.uint64)
    np.add.at(x, ii, GF(vv))
    want = a.copy()
    for i, v in zip(ii, vv):
        want[i] = F.add([want[i]], [v])[0]
    assert np.array_equal(x.numpy().astype(np.uint64), want)
    np.multiply.at(x, ii, GF(vv))
    for i, v in zip(ii, vv):
        want[i] = F.mul([want[i]], [v])[0]
    assert np.array_equal(x.numpy().astype(np.uint64), want)
    np.negative.at(x, [1, 1, 2])
    want[2] = F.neg([want[2]])[0]
    assert np.array_equal(x.numpy().astype(np.uint64), want)
    np.power.at(x, [4, 4], 3)
    want[4] = F.pow([want[4]], [9])[0]
    assert np.array_equal(x.numpy().astype(np.uint64), want)
    np.subtract.at(x, [6], GF(vv[:1]))
    want[6] = F.sub([want[6]], [vv[0]])[0]
    assert np.array_equal(x.numpy().astype(np.uint64), want)


def test_library_calls_are_graph_capturable():
    """After a warm-up call (plans, tables and scratch exist) the hot-path entry points are plain kernel launches on the
    caller's stream, so they can be captured into a HIP graph and replayed on new data."""
    import torch

    GF = ga.GF(2**8)
    P = ga.GF(7340033)
    rs = ga.ReedSolomon(255, 223)
    rng = np.random.default_rng(21)
    x, y = GF(rng.integers(0, 256, 1 << 20)), GF(rng.integers(1, 256, 1 << 20))
    v = P(rng.integers(0, 7340033, (4, 1 << 12)))
    m = GF(rng.integers(0, 256, (2048, 223)))
    from galois_amd._ntt import fft_batched

    def work():
        z = x * y
        w = z + x  # (division would not capture through the Python front end: its ZeroDivisionError check reads the device
        #             error word back; the C-ABI call itself is capturable)
        V = fft_batched(v)
        c = rs.encode(m)
        return z, w, V, c

    work()  # warm-up: builds plans / uploads tables outside the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        work()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            z, w, V, c = work()
    # replay on NEW input data written into the captured buffers
    x2, m2 = rng.integers(0, 256, 1 << 20), rng.integers(0, 256, (2048, 223))
    v2 = rng.integers(0, 7340033, (4, 1 << 12))
    x._t.copy_(torch.from_numpy(x2.astype(np.uint8)).cuda())
    m._t.copy_(torch.from_numpy(m2.astype(np.uint8)).cuda())
    v._t.copy_(torch.from_numpy(v2.astype(np.int32)).cuda())
    g.replay()
    torch.cuda.synchronize()
    F = O.OracleField(2, 8, 285, 2, lookup=True)
    assert np.array_equal(z.numpy(), F.ufunc_u8(O.MUL, x2.astype(np.uint8), y.numpy()))
    assert np.array_equal(w.numpy(), z.numpy() ^ x2.astype(np.uint8))
    FP = O.OracleField(7340033, 1, None, P._primitive_element_int)
    assert np.array_equal(V.numpy()[1].astype(np.uint32), FP.ntt_u32_pow2(v2[1].astype(np.uint32), P._root_of_unity_int(1 << 12)))
    assert np.array_equal(c.numpy(), O.OracleRS(F, 255, 223).encode_u8(m2.astype(np.uint8)))


def test_torch_adoption_range_checks_in_every_storage_width():
    """Range checks happen on the tensor as given (its own width and signedness), before any narrowing: fields whose
    2- or 4-byte storage needs the top bit, and out-of-field values that would wrap into the field."""
    import torch

    G16, G65521, G32, G8, G7 = ga.GF(2**16), ga.GF(65521), ga.GF(2**32), ga.GF(2**8), ga.GF(7)
    a = G16(torch.tensor([5, 7, 65535, 32768], dtype=torch.uint16))
    assert [int(v) for v in a.numpy()] == [5, 7, 65535, 32768]
    assert [int(v) for v in (a * a).numpy()] == [int(v) for v in (G16([5, 7, 65535, 32768]) * G16([5, 7, 65535, 32768])).numpy()]
    b = G65521(torch.tensor([5, 65520, 40000], dtype=torch.uint16))
    assert [int(v) for v in (b + b).numpy()] == [10, 65519, 80000 - 65521]
    with pytest.raises(ValueError):
        G65521(torch.tensor([65521], dtype=torch.uint16))
    c = G32(torch.tensor([5, 2**32 - 1, 2**31], dtype=torch.uint32))
    assert [int(v) for v in c.numpy()] == [5, 2**32 - 1, 2**31]
    with pytest.raises(ValueError):
        G8(torch.tensor([261, 300]), dtype=np.uint8)  # would wrap to [5, 44]
    with pytest.raises(ValueError):
        G7(torch.tensor([6, -1], dtype=torch.int8))
    with pytest.raises(ValueError):
        G16(torch.tensor([65536], dtype=torch.int32))
    assert int(G16(torch.tensor([65535], dtype=torch.int32))[0]) == 65535


def test_out_keyword_writes_in_place_and_unsupported_keywords_raise():
    GF = ga.GF(2**8)
    x = GF.Random(1000, seed=1); y = GF.Random(1000, low=1, seed=2)
    want = (x * y).numpy()
    out = GF.Zeros(1000)
    ptr = out.torch().data_ptr()
    r = np.multiply(x, y, out=out)
    assert r is out and out.torch().data_ptr() == ptr and np.array_equal(out.numpy(), want)
    # aliasing an input (x *= y style) and the other element-wise kernels
    x2 = x.copy(); p2 = x2.torch().data_ptr()
    np.multiply(x2, y, out=x2)
    assert x2.torch().data_ptr() == p2 and np.array_equal(x2.numpy(), want)
    o2 = GF.Zeros(1000)
    np.reciprocal(y, out=o2); assert np.array_equal(o2.numpy(), (y ** -1).numpy())
    np.power(x, 3, out=o2); assert np.array_equal(o2.numpy(), (x * x * x).numpy())
    np.divide(x, y, out=(o2,)); assert np.array_equal(o2.numpy(), (x / y).numpy())
    # a wider target: computed, then stored
    wide = GF.Zeros(1000, dtype=np.int32)
    np.add(x, y, out=wide); assert wide.dtype == np.int32 and np.array_equal(wide.numpy(), (x + y).numpy())
    with pytest.raises(ValueError):
        np.add(x, y, out=GF.Zeros(999))
    with pytest.raises(TypeError):
        np.add(x, y, out=np.zeros(1000, dtype=np.uint8))
    # where= / initial=: tests/test_gpu_ufunc_kwargs.py
    assert np.array_equal(np.add(x, y, where=np.arange(1000) % 2 == 0).numpy()[::2], (x + y).numpy()[::2])
    assert int(np.add.reduce(x, initial=GF(3))) == int(np.add.reduce(x) + GF(3))
    # casting= is overridden by the reference too, dtype= only names an intermediate type: accepted, no effect on values
    assert np.array_equal(np.add(x, y, casting="safe").numpy(), (x + y).numpy())
    assert np.array_equal(np.add(x, y, dtype=np.int64).numpy(), (x + y).numpy())


def test_numpy_functions_stay_in_the_field_or_raise():
    """np.sum / prod / cumsum / cumprod / trace / diff reach the device reductions (the reference gets there through
    ndarray.__array_function__ -> ufunc methods); data-movement functions return field arrays; the rest raises."""
    GF = ga.GF(7)
    a = GF([3, 5, 6, 1])
    assert int(np.sum(a)) == (3 + 5 + 6 + 1) % 7 and type(np.sum(a)) is GF
    assert int(np.prod(a)) == (3 * 5 * 6 * 1) % 7
    assert np.array_equal(np.cumsum(a).numpy(), np.cumsum([3, 5, 6, 1]) % 7)
    assert np.array_equal(np.cumprod(a).numpy(), np.cumprod([3, 5, 6, 1]) % 7)
    assert np.array_equal(np.diff(a).numpy(), np.diff([3, 5, 6, 1]) % 7)
    m = GF(np.arange(12).reshape(3, 4) % 7)
    assert np.array_equal(np.sum(m, axis=0).numpy(), (np.arange(12).reshape(3, 4) % 7).sum(axis=0) % 7)
    assert np.array_equal(np.sum(m, axis=1, keepdims=True).numpy(), (np.arange(12).reshape(3, 4) % 7).sum(axis=1, keepdims=True) % 7)
    sq = GF(np.arange(9).reshape(3, 3) % 7)
    assert int(np.trace(sq)) == int(np.trace(np.arange(9).reshape(3, 3) % 7)) % 7
    c = np.concatenate([a, a])
    assert type(c) is GF and np.array_equal(c.numpy(), [3, 5, 6, 1, 3, 5, 6, 1])
    assert type(np.stack([a, a])) is GF and np.stack([a, a]).shape == (2, 4)
    assert type(np.broadcast_to(a, (2, 4))) is GF
    assert np.array_equal(np.flip(a).numpy(), [1, 6, 5, 3]) and np.array_equal(np.roll(a, 1).numpy(), [1, 3, 5, 6])
    assert np.array_equal(np.transpose(m).numpy(), (np.arange(12).reshape(3, 4) % 7).T)
    assert type(np.reshape(m, (4, 3))) is GF and np.array_equal(np.tile(a, 2).numpy(), np.tile([3, 5, 6, 1], 2))
    assert np.array_equal(np.where(np.array([True, False, True, False]), a, GF([0, 0, 0, 0])).numpy(), [3, 0, 6, 0])
    assert np.array_equal(np.diag(sq).numpy(), np.diag(np.arange(9).reshape(3, 3) % 7))
    assert np.count_nonzero(GF([0, 1, 0, 2])) == 2 and np.array_equal(a, GF([3, 5, 6, 1]))
    with pytest.raises(TypeError):
        np.concatenate([a, ga.GF(5)([1, 2])])
    for f in (np.around, np.gradient, np.cross, np.median, np.mean):
        with pytest.raises(NotImplementedError):
            f(a) if f is not np.cross else f(a, a)


@pytest.mark.parametrize("order,dt", [(7, np.uint8), (4294967291, np.uint32), (2**61 - 1, np.int64), (2**64 - 2**32 + 1, None)])
def test_ordering_and_editing_functions_follow_numpy_on_the_integer_values(order, dt):
    """np.sort / argsort / unique / append / insert / delete / take(axis=-1): the reference serves them through its ndarray
    subclass (they are not in _UNSUPPORTED_FUNCTIONS, _domains/_function.py:405-461), i.e. by integer value -- which for
    uint32 / uint64 storage must be the UNSIGNED order although the device tensors are signed."""
    GF = ga.GF(order)
    rng = np.random.default_rng(5)
    vals = [int(v) % order for v in rng.integers(0, 2**63, 40)] + [0, order - 1, order - 1, 1, order // 2 + 1]
    h = np.array(vals, dtype=object).reshape(5, 9)
    x = GF(h if dt is None else h.astype(dt))
    ints = lambda a: np.array([int(v) for v in np.asarray(a.numpy()).ravel()], dtype=object).reshape(a.shape)
    assert np.array_equal(ints(np.sort(x)), np.sort(h, axis=-1)) and type(np.sort(x)) is GF
    assert np.array_equal(ints(np.sort(x, axis=0)), np.sort(h, axis=0))
    assert np.array_equal(ints(np.sort(x, axis=None)), np.sort(h, axis=None))
    assert np.array_equal(np.argsort(x, axis=1, kind="stable"), np.argsort(h, axis=1, kind="stable"))
    u, inv, cnt = np.unique(x, return_inverse=True, return_counts=True)
    hu, hinv, hcnt = np.unique(h.astype(object), return_inverse=True, return_counts=True)
    assert np.array_equal(ints(u), hu) and np.array_equal(inv.reshape(-1), hinv.reshape(-1)) and np.array_equal(cnt, hcnt)
    row = GF(h[0] if dt is None else h[0].astype(dt))
    assert np.array_equal(ints(np.append(x, row)), np.append(h, h[0]))
    assert np.array_equal(ints(np.append(x, row.reshape(1, 9), axis=0)), np.append(h, h[:1], axis=0))
    assert np.array_equal(ints(np.delete(x, [1, 3], axis=0)), np.delete(h, [1, 3], axis=0))
    assert np.array_equal(ints(np.delete(x, 4)), np.delete(h, 4))
    assert np.array_equal(ints(np.insert(x, 2, row, axis=0)), np.insert(h, 2, h[0], axis=0))
    assert np.array_equal(ints(np.insert(row, [1, 5], GF([1, 2]) if dt is None else GF(np.array([1, 2], dtype=dt)))), np.insert(h[0], [1, 5], [1, 2]))
    # NumPy's pairing rules: a scalar position takes EVERY value; values[i] goes with obj[i] also when obj is unsorted
    mk = lambda v: GF(v) if dt is None else GF(np.array(v, dtype=dt))
    assert np.array_equal(ints(np.insert(row, 1, mk([1, 2, 3]))), np.insert(h[0], 1, [1, 2, 3]))
    assert np.array_equal(ints(np.insert(row, [5, 1], mk([1, 2]))), np.insert(h[0], [5, 1], [1, 2]))
    assert np.array_equal(ints(np.insert(row, [3, 3, 0], mk([1, 2, 3]))), np.insert(h[0], [3, 3, 0], [1, 2, 3]))
    assert np.array_equal(ints(np.insert(x, [4, 1], mk([[1], [2]]), axis=0)), np.insert(h, [4, 1], [[1], [2]], axis=0))
    assert np.array_equal(ints(np.insert(x, 3, mk([1, 2, 3, 4, 5]), axis=1)), np.insert(h, 3, [1, 2, 3, 4, 5], axis=1))
    # a size-1 index SEQUENCE takes NumPy's scalar path too: all values go in at that index
    assert np.array_equal(ints(np.insert(row, [2], mk([6, 5, 4]))), np.insert(h[0], [2], [6, 5, 4]))
    assert np.array_equal(ints(np.insert(x, [1], mk([[1, 2, 3, 4, 5, 6, 0, 1, 2], [6, 5, 4, 3, 2, 1, 0, 6, 5]]), axis=0)),
                          np.insert(h, [1], [[1, 2, 3, 4, 5, 6, 0, 1, 2], [6, 5, 4, 3, 2, 1, 0, 6, 5]], axis=0))
    assert np.array_equal(ints(np.insert(x, [3], mk([[1], [2], [3], [4], [5]]), axis=1)), np.insert(h, [3], [[1], [2], [3], [4], [5]], axis=1))
    assert np.array_equal(ints(np.take(x, [0, 8, 3], axis=-1)), np.take(h, [0, 8, 3], axis=-1))
    assert np.array_equal(ints(np.take(x, [[0, 1], [2, 3]], axis=-2)), np.take(h, [[0, 1], [2, 3]], axis=-2))


def test_out_argument_that_overlaps_an_operand_or_feeds_a_composite():
    """np.sqrt is several kernels that re-read their input: with out=x the first kernel must not overwrite x.  A target that
    partially overlaps an operand (views of one buffer) is computed through a fresh buffer, as NumPy's overlap handling does."""
    GF = ga.GF(7340033)
    rng = np.random.default_rng(9)
    r = GF(rng.integers(1, 7340033, 5000, dtype=np.uint32))
    x = r * r
    want = np.sqrt(x).numpy()
    y = x.copy()
    res = np.sqrt(y, out=y)
    assert res is y and np.array_equal(y.numpy(), want)
    a = GF(rng.integers(0, 7340033, 4096, dtype=np.uint32))
    h = a.numpy().astype(np.int64)
    np.add(a[:-1], a[1:], out=a[1:])
    assert np.array_equal(a.numpy()[1:].astype(np.int64), (h[:-1] + h[1:]) % 7340033) and int(a[0]) == h[0]
    b = GF(h.astype(np.uint32))
    np.multiply(b[1:], b[1:], out=b[1:])  # the SAME view as operand and target: written in place
    assert np.array_equal(b.numpy()[1:].astype(np.int64), (h[1:] * h[1:]) % 7340033)


def _big_case(q, dt, n, seed, mode="jit-calculate", GF=None, lookup=False):
    GF = GF or ga.GF(q)
    F = O.OracleField(GF.characteristic, GF.degree, int(GF.irreducible_poly) if GF.degree > 1 else None, int(GF.primitive_element),
                      lookup=lookup)
    if mode in GF.ufunc_modes:
        GF.compile(mode)
    rng = np.random.default_rng(seed)
    if q > 2**63:
        a = (rng.integers(0, 2**63, n, dtype=np.uint64) * 2 + 1) % np.uint64(q)
        b = (rng.integers(0, 2**63, n, dtype=np.uint64) * 2 + 1) % np.uint64(q)
    else:
        a = rng.integers(0, q, n, dtype=np.uint64)
        b = rng.integers(0, q, n, dtype=np.uint64)
    for arr in (a, b):
        arr[:6] = [0, 1, q - 1, q - 2, 2, q // 2]
    bnz = np.where(b == 0, np.uint64(1), b)
    mk = (lambda v: GF._wrap(__import__("torch").from_numpy(v.view(np.int64)).cuda(), np.object_)) if dt is None else (lambda v: GF(v.astype(dt), dtype=dt))
    u = lambda x: x._t.cpu().numpy().view(np.uint64) if dt is None else x.numpy().astype(np.uint64)
    return GF, F, a, b, bnz, mk, u


@pytest.mark.parametrize("q,dt", [(65537, np.uint32), (7340033, np.uint32), (65521, np.uint16), (251, np.uint8), (2**61 - 1, None),
                                  (2**64 - 2**32 + 1, None)])
def test_prime_field_reciprocal_and_division_on_large_arrays(q, dt):
    """Large odd-length arrays take the 16-elements-per-lane Montgomery-trick inversion (one exponentiation per 16 elements,
    vectors nth apart); zeros inside a batch must not disturb their neighbours and must raise."""
    n = 1_200_003
    GF, F, a, b, bnz, mk, u = _big_case(q, dt, n, 11)
    try:
        A, Bnz = mk(a), mk(bnz)
        assert np.array_equal(u(np.reciprocal(Bnz)), F.recip(bnz))
        assert np.array_equal(u(A / Bnz), F.div(a, bnz))
        assert np.array_equal(u(A / mk(bnz[:1])[0]), F.div(a, np.full(n, bnz[0], dtype=np.uint64)))  # scalar divisor
        with pytest.raises(ZeroDivisionError):
            np.reciprocal(mk(b))
        with pytest.raises(ZeroDivisionError):
            A / mk(b)
    finally:
        GF.compile("auto")


@pytest.mark.parametrize("q,dt", [(2**8, np.uint8), (2**3, np.uint8), (2**10, np.uint16), (2**12, np.uint16), (2**16, np.uint16), (2**5, np.uint16),
                                  (2**20, np.uint32), (2**32, np.uint32), (2**8, np.int64), (2**17, np.uint32), (2**18, np.uint32),
                                  (2**21, np.uint32), (2**22, np.uint32), (2**24, np.uint32), (2**27, np.uint32), (2**31, np.uint32),
                                  (2**16, np.uint32), (2**32, np.int64)])
def test_binary_field_calculate_mode_products_on_large_arrays(q, dt):
    """Packed shift-and-xor products (four uint8 / two uint16 elements per register), the branch-free 32-bit product, the
    integer-multiply carry-less product with folds through the field polynomial (17 <= m <= 32 where the polynomial is sparse
    enough: 9 or 16 multiplies), tails, scalar operands and misaligned views, against the oracle."""
    n = 1_000_003
    GF, F, a, b, bnz, mk, u = _big_case(q, dt, n, 12)
    try:
        A, B = mk(a), mk(b)
        want = F.mul(a, b)
        assert np.array_equal(u(A * B), want)
        assert np.array_equal(u(A * B[3]), F.mul(a, np.full(n, b[3], dtype=np.uint64)))
        assert np.array_equal(u(A[5] * B), F.mul(np.full(n, a[5], dtype=np.uint64), b))
        assert np.array_equal(u(A[1:] * B[1:]), want[1:])                     # views that are not 16-byte aligned
        assert np.array_equal(u(A[:1000] / mk(bnz)[:1000]), F.div(a[:1000], bnz[:1000]))
        e = np.random.default_rng(5).integers(-20, 300, 2000)
        anz = np.where(a[:2000] == 0, np.uint64(1), a[:2000])
        assert np.array_equal(u(mk(anz) ** e), F.pow(anz, e))
    finally:
        GF.compile("auto")


@pytest.mark.parametrize("q", [7**2, 251**2, 2147483647**2, 46351**2, 3**4, 5**4, 13**4, 3**5, 3**6, 11**6, 7**3, 251**3, 31**5,
                               3**7, 7**7, 251**7, 3**8, 5**8, 251**8])
def test_extension_fields_of_every_templated_degree(q):
    """GF(p^m), 2 <= m <= 6, calculate mode: the per-degree kernels (digits in registers, unreduced 64-bit accumulation -- the
    largest p for m = 2 sits at the accumulation bound 3 p^2 < 2^64) against the oracle."""
    p, m = ga._numtheory.prime_power(q)
    # p = 3 (mod 4): x^2 + 1 is irreducible (no Conway polynomial is shipped for these two characteristics)
    GF0 = ga.GF(p, m, irreducible_poly=[1, 0, 1]) if q in (2147483647**2, 46351**2) else ga.GF(q)
    dt = GF0.dtypes[0] if GF0.dtypes != [np.object_] else None
    n = 50_003
    GF, F, a, b, bnz, mk, u = _big_case(q, dt, n, 13, GF=GF0)
    try:
        A, B = mk(a), mk(b)
        assert np.array_equal(u(A + B), F.add(a, b))
        assert np.array_equal(u(A - B), F.sub(a, b))
        assert np.array_equal(u(-A), F.neg(a))
        assert np.array_equal(u(A * B), F.mul(a, b))
        assert np.array_equal(u(A[:3000] / mk(bnz)[:3000]), F.div(a[:3000], bnz[:3000]))
        e = np.random.default_rng(6).integers(-20, 300, 3000)
        anz = np.where(a[:3000] == 0, np.uint64(1), a[:3000])
        assert np.array_equal(u(mk(anz) ** e), F.pow(anz, e))
        assert np.array_equal(u(A * 12345), F.mul(a, np.full(n, 12345 % GF.characteristic, dtype=np.uint64)))
    finally:
        GF.compile("auto")


@pytest.mark.parametrize("q", [3**7, 2**10, 2**13, 5**5, 3191, 8191, 257, 2**9, 17**3, 89**2])
@pytest.mark.parametrize("mode", ["jit-lookup", "auto"])
def test_mid_size_fields_with_tables_in_lds(q, mode):
    """256 < q <= 8192 on uint16 storage: EXP / LOG / Zech held in LDS as 16-bit entries (gfa_elementwise_mid.hip).  Every
    operation, scalar operands on either side, tails, misaligned views (which fall back to the generic kernels), zeros
    among the operands and the ZeroDivisionError paths, against the oracle; `auto` routes only division / reciprocal /
    power of the calculated fields there."""
    n = 400_003
    GF, F, a, b, bnz, mk, u = _big_case(q, np.uint16, n, 21, mode=mode, lookup=True)
    a[100:140] = 0
    b[120:160] = 0
    a[1000:1040] = b[1000:1040]                       # a - a = 0, a + (-a)
    bnz = np.where(b == 0, np.uint64(1), b)
    full = lambda v: np.full(n, v, dtype=np.uint64)
    try:
        A, B, Bnz = mk(a), mk(b), mk(bnz)
        assert np.array_equal(u(A + B), F.add(a, b))
        assert np.array_equal(u(A - B), F.sub(a, b))
        assert np.array_equal(u(A + (-A)), np.zeros(n, dtype=np.uint64))
        assert np.array_equal(u(-A), F.neg(a))
        assert np.array_equal(u(A * B), F.mul(a, b))
        assert np.array_equal(u(A / Bnz), F.div(a, bnz))
        assert np.array_equal(u(np.reciprocal(Bnz)), F.recip(bnz))
        for k in (5, 7):                                 # one operand a scalar (k = 5: value q // 2, k = 7 random)
            assert np.array_equal(u(A * B[k]), F.mul(a, full(b[k])))
            assert np.array_equal(u(A[k] - B), F.sub(full(a[k]), b))
            assert np.array_equal(u(A + B[k]), F.add(a, full(b[k])))
            assert np.array_equal(u(A[k] / Bnz), F.div(full(a[k]), bnz))
            assert np.array_equal(u(A / Bnz[k]), F.div(a, full(bnz[k])))
        assert np.array_equal(u(A[0] * B), np.zeros(n, dtype=np.uint64))
        assert np.array_equal(u(A[3:] * B[3:]), F.mul(a[3:], b[3:]))       # not 16-byte aligned: generic kernels
        assert np.array_equal(u(A[8:] / Bnz[8:]), F.div(a[8:], bnz[8:]))   # aligned view, odd tail
        for e in (0, 1, 2, 3, -1, -7, 12345, q - 1, q - 2, -(q - 1), 2**40 + 3, -(2**40) - 3):
            assert np.array_equal(u(Bnz ** e), F.pow(bnz, np.full(n, e, dtype=np.int64))), e
        assert np.array_equal(u(A ** 3), F.pow(a, np.full(n, 3, dtype=np.int64)))
        assert np.array_equal(u(A ** 0), np.ones(n, dtype=np.uint64))
        # one exponent per element: small, huge, negative, zero, multiples of q - 1
        e = np.random.default_rng(22).integers(-2**62, 2**62, n)
        e[:n // 2] = np.random.default_rng(23).integers(-300, 300, n // 2)
        e[5:12] = [0, q - 1, -(q - 1), 2 * (q - 1), -2**63, 2**63 - 1, 1]
        assert np.array_equal(u(Bnz ** e), F.pow(bnz, e))
        ez = np.abs(e)
        assert np.array_equal(u(A ** ez), F.pow(a, ez))             # zeros in the base: 0 ** 0 = 1, 0 ** k = 0
        with pytest.raises(ZeroDivisionError):
            A / B
        with pytest.raises(ZeroDivisionError):
            np.reciprocal(B)
        with pytest.raises(ZeroDivisionError):
            A ** -2
        with pytest.raises(ZeroDivisionError):
            A ** e
    finally:
        GF.compile("auto")


@pytest.mark.parametrize("q,n", [(2**16, 600_011), (2**16, 17_000_003), (3**10, 4_300_003), (65521, 4_194_304), (2**14, 600_011), (3**10, 600_011), (65521, 600_011), (8209, 524_288),
                                 (251**2, 700_001), (2**15, 4_200_005), (3**9, 600_011), (13**4, 600_011), (32771, 600_011), (32749, 600_011)])
@pytest.mark.parametrize("mode", ["jit-lookup", "auto"])
def test_fields_up_to_2e16_with_log_and_exp_staged_in_turn(q, n, mode):
    """8192 < q <= 65536 on uint16 storage.  Up to 32768 elements LOG and a q-entry EXP are both resident in LDS (indices reduced
    below q - 1; ZECH too while 6q bytes fit); above, products / quotients / reciprocals / powers go through LOG, then EXP, staged
    in LDS in two phases per tile (big16_kernel).  Both tile shapes, tails of n & 7 elements, scalar operands, zeros,
    ZeroDivisionError."""
    GF, F, a, b, bnz, mk, u = _big_case(q, np.uint16, n, 31, mode=mode, lookup=True)
    a[100:140] = 0
    b[120:160] = 0
    bnz = np.where(b == 0, np.uint64(1), b)
    full = lambda v: np.full(n, v, dtype=np.uint64)
    try:
        A, B, Bnz = mk(a), mk(b), mk(bnz)
        assert np.array_equal(u(A * B), F.mul(a, b))
        assert np.array_equal(u(A / Bnz), F.div(a, bnz))
        assert np.array_equal(u(np.reciprocal(Bnz)), F.recip(bnz))
        assert np.array_equal(u(A + B), F.add(a, b))
        assert np.array_equal(u(A - B), F.sub(a, b))
        assert np.array_equal(u(-A), F.neg(a))
        if n >= 2_000_000:  # (from 2^22 elements: the two streaming passes through an index array, big16_index_kernel / big16_exp_kernel)
            for e in (12345, -3):
                assert np.array_equal(u(Bnz ** e), F.pow(bnz, np.full(n, e, dtype=np.int64))), e
            assert np.array_equal(u(A * B[7]), F.mul(a, full(b[7])))
            assert np.array_equal(u(A[9] / Bnz), F.div(full(a[9]), bnz))
        if n < 2_000_000:
            for k in (5, 7):
                assert np.array_equal(u(A * B[k]), F.mul(a, full(b[k])))
                assert np.array_equal(u(A[k] - B), F.sub(full(a[k]), b))
                assert np.array_equal(u(A[k] / Bnz), F.div(full(a[k]), bnz))
                assert np.array_equal(u(A / Bnz[k]), F.div(a, full(bnz[k])))
            assert np.array_equal(u(A[8:] / Bnz[8:]), F.div(a[8:], bnz[8:]))
            assert np.array_equal(u(A[3:] / Bnz[3:]), F.div(a[3:], bnz[3:]))   # not 16-byte aligned: generic kernels
            for e in (0, 1, 3, -1, 12345, q - 1, q - 2, -(q - 1), 2**40 + 3, -(2**40) - 3):
                assert np.array_equal(u(Bnz ** e), F.pow(bnz, np.full(n, e, dtype=np.int64))), e
            assert np.array_equal(u(A ** 3), F.pow(a, np.full(n, 3, dtype=np.int64)))
            assert np.array_equal(u(A ** 0), np.ones(n, dtype=np.uint64))
            C = A.copy()
            np.multiply(C, B, out=C)                                            # in place
            assert np.array_equal(u(C), F.mul(a, b))
            C = A.copy()
            np.subtract(C, B, out=C)
            assert np.array_equal(u(C), F.sub(a, b))
            e = np.random.default_rng(32).integers(-2**62, 2**62, n)
            e[:n // 2] = np.random.default_rng(33).integers(-300, 300, n // 2)
            e[5:12] = [0, q - 1, -(q - 1), 2 * (q - 1), -2**63, 2**63 - 1, 1]
            assert np.array_equal(u(Bnz ** e), F.pow(bnz, e))
            assert np.array_equal(u(A ** np.abs(e)), F.pow(a, np.abs(e)))
        with pytest.raises(ZeroDivisionError):
            A / B
        with pytest.raises(ZeroDivisionError):
            np.reciprocal(B)
        with pytest.raises(ZeroDivisionError):
            A ** -2
    finally:
        GF.compile("auto")


@pytest.mark.parametrize("q", [2**8, 31, 3**5, 251, 2**3, 5**3, 2])
def test_uint8_power_with_one_exponent_is_a_256_entry_map(q):
    """x ** k on uint8 storage, one exponent for the whole array (lookup mode): the 256 possible results are computed once on the
    device and applied by the streaming table kernel.  Every exponent class, zeros present and absent, tails, against the oracle."""
    n = 300_007
    GF, F, a, b, bnz, mk, u = _big_case(q, np.uint8, n, 41, mode="jit-lookup", lookup=True)
    a[:6] = [0, 1, q - 1, max(q - 2, 0), min(2, q - 1), q // 2]
    anz = np.where(a == 0, np.uint64(1), a)
    try:
        A, Anz = mk(a), mk(anz)
        for e in (0, 1, 2, 3, 7, q - 1, q - 2, 12345, 2**40 + 3, 2**63 - 1):
            assert np.array_equal(u(A ** e), F.pow(a, np.full(n, e, dtype=np.int64))), e
        for e in (-1, -2, -(q - 1), -12345, -(2**40) - 3, -2**63):
            assert np.array_equal(u(Anz ** e), F.pow(anz, np.full(n, e, dtype=np.int64))), e
            with pytest.raises(ZeroDivisionError):
                A ** e
        assert np.array_equal(u(A[16:5000] ** 5), F.pow(a[16:5000], np.full(4984, 5, dtype=np.int64)))
        assert np.array_equal(u(A[3:5000] ** 5), F.pow(a[3:5000], np.full(4997, 5, dtype=np.int64)))   # misaligned: generic kernel
    finally:
        GF.compile("auto")


@pytest.mark.parametrize("q", [2**16, 3**10])
def test_staged_table_kernels_repeat_identically_over_many_tiles_per_workgroup(q):
    """Arrays large enough that every workgroup of the staged-table kernels walks several tiles (re-staging LOG / ZECH / EXP each
    time), every operation repeated with other kernels in between.  The first pipelined version passed single runs and produced
    intermittent wrong words under exactly this pattern: its 16-byte buffer stores carried the vector index in the SCALAR offset,
    and on gfx950 such a store followed at once by a VALU write of its data registers stores corrupted words (the compiler
    inserts the wait states only for the immediate-offset form).  The stores now use the VGPR offset; this test keeps watch."""
    n = 17_000_003
    GF, F, a, b, bnz, mk, u = _big_case(q, np.uint16, n, 51, mode="jit-lookup", lookup=True)
    try:
        A, B, Bnz = mk(a), mk(b), mk(bnz)
        e = np.full(n, 12345, dtype=np.int64)
        want = {"mul": F.mul(a, b), "div": F.div(a, bnz), "recip": F.recip(bnz), "pow": F.pow(bnz, e)}
        ops = {"mul": lambda: A * B, "div": lambda: A / Bnz, "recip": lambda: np.reciprocal(Bnz), "pow": lambda: Bnz ** 12345}
        if q % 2:
            want.update({"add": F.add(a, b), "sub": F.sub(a, b), "neg": F.neg(a)})
            ops.update({"add": lambda: A + B, "sub": lambda: A - B, "neg": lambda: -A})
        for mode in ("jit-lookup", "auto"):
            GF.compile(mode)
            for rep in range(6):
                for name, fn in ops.items():
                    junk = A + B if q % 2 == 0 else A * B           # a different kernel in between
                    got = u(fn())
                    assert np.array_equal(got, want[name]), (mode, rep, name, int((got != want[name]).sum()))
    finally:
        GF.compile("auto")


@pytest.mark.parametrize("q", [2**8, 3**5, 251, 31, 2**4])
@pytest.mark.parametrize("dt", [np.uint16, np.uint32, np.int64])
def test_small_fields_in_wide_storage(q, dt):
    """Fields of at most 256 elements held in uint16 / uint32 / int64 arrays (the reference's dtype=int) on large arrays: every binary
    operation, scalar operands, tails, views, in place, ZeroDivisionError, against the oracle.  (A variant of the 64 KiB LDS
    table kernel for these storage widths was measured at the same 0.63 of the roofline as the generic kernel with its tables in
    L1 -- 24 bytes per element of traffic leave the gathers idle either way -- and was not kept.)"""
    if np.dtype(dt) not in [np.dtype(d) for d in ga.GF(q).dtypes]:
        pytest.skip("dtype not offered for this field")
    n = 700_003
    GF, F, a, b, bnz, mk, u = _big_case(q, dt, n, 61, mode="jit-lookup", lookup=True)
    full = lambda v: np.full(n, v, dtype=np.uint64)
    try:
        A, B, Bnz = mk(a), mk(b), mk(bnz)
        assert np.array_equal(u(A + B), F.add(a, b))
        assert np.array_equal(u(A - B), F.sub(a, b))
        assert np.array_equal(u(A * B), F.mul(a, b))
        assert np.array_equal(u(A / Bnz), F.div(a, bnz))
        assert np.array_equal(u(A * B[7]), F.mul(a, full(b[7])))
        assert np.array_equal(u(A[7] - B), F.sub(full(a[7]), b))
        assert np.array_equal(u(A[7] / Bnz), F.div(full(a[7]), bnz))
        step = 16 // np.dtype(dt).itemsize
        assert np.array_equal(u(A[step:] * B[step:]), F.mul(a[step:], b[step:]))   # aligned view
        assert np.array_equal(u(A[1:] * B[1:]), F.mul(a[1:], b[1:]))               # misaligned: generic kernel
        C = A.copy()
        np.multiply(C, B, out=C)
        assert np.array_equal(u(C), F.mul(a, b))
        with pytest.raises(ZeroDivisionError):
            A / B
    finally:
        GF.compile("auto")


@pytest.mark.parametrize("q", [3**7, 2**12, 7919, 2**15, 3**9])
@pytest.mark.parametrize("dt", [np.uint32, np.int64])
def test_table_fields_up_to_2e15_in_uint32_and_int64_storage(q, dt):
    """256 < q <= 32768 held in uint32 / int64 arrays (the reference documentation's dtype=int, _domains/_array.py:445-451): the
    LDS-table kernels of gfa_elementwise_mid.hip unpack 4 / 2 elements per 16-byte vector instead of 8; every operation, scalar
    operands, tails, aligned and misaligned views, in place, ZeroDivisionError, against the oracle."""
    if np.dtype(dt) not in [np.dtype(d) for d in ga.GF(q).dtypes]:
        pytest.skip("dtype not offered for this field")
    n = 600_011
    GF, F, a, b, bnz, mk, u = _big_case(q, dt, n, 77, mode="jit-lookup", lookup=True)
    full = lambda v: np.full(n, v, dtype=np.uint64)
    try:
        A, B, Bnz = mk(a), mk(b), mk(bnz)
        assert A.dtype == np.dtype(dt)
        assert np.array_equal(u(A + B), F.add(a, b))
        assert np.array_equal(u(A - B), F.sub(a, b))
        assert np.array_equal(u(A * B), F.mul(a, b))
        assert np.array_equal(u(A / Bnz), F.div(a, bnz))
        assert np.array_equal(u(-A), F.sub(full(0), a))
        assert np.array_equal(u(np.reciprocal(Bnz)), F.div(full(1), bnz))
        assert np.array_equal(u(A ** 5), F.pow(a, np.full(n, 5, dtype=np.int64)))
        assert np.array_equal(u(Bnz ** -3), F.pow(bnz, np.full(n, -3, dtype=np.int64)))
        assert np.array_equal(u(A * B[7]), F.mul(a, full(b[7])))
        assert np.array_equal(u(A[7] - B), F.sub(full(a[7]), b))
        assert np.array_equal(u(A[7] / Bnz), F.div(full(a[7]), bnz))
        step = 16 // np.dtype(dt).itemsize
        assert np.array_equal(u(A[step:] * B[step:]), F.mul(a[step:], b[step:]))   # aligned view
        assert np.array_equal(u(A[1:] / Bnz[1:]), F.div(a[1:], bnz[1:]))           # misaligned: generic kernel
        C = A.copy()
        np.multiply(C, B, out=C)
        assert np.array_equal(u(C), F.mul(a, b))
        assert (A * B).dtype == np.dtype(dt)
        with pytest.raises(ZeroDivisionError):
            A / B
    finally:
        GF.compile("auto")


@pytest.mark.parametrize("order", [65521, 3**10, 2**16])
@pytest.mark.parametrize("dt", [np.uint32, np.int64])
def test_wide_storage_of_fields_between_2e15_and_2e16_elements(order, dt):
    """r05 (VERDICT r04 missing #6): uint32 / int64 arrays of lookup-mode fields with 32768 < q <= 65536 -- the reference's dtype
    list offers them (_fields/_ufunc.py:97-111) -- take the staged LDS-table kernels through a 16-bit work buffer.  Against the
    oracle's lookup-mode scalars on every element; an array length that leaves a tail of 5 and a broadcast scalar operand."""
    GF = ga.GF(order, compile="jit-lookup")
    F = O.OracleField(GF.characteristic, GF.degree, int(GF.irreducible_poly) if GF.degree > 1 else None, int(GF.primitive_element), lookup=True)
    n = (1 << 19) + 5
    rng = np.random.default_rng(order)
    a = rng.integers(0, order, n, dtype=np.uint64)
    b = rng.integers(1, order, n, dtype=np.uint64)
    a[:4] = (0, order - 1, 1, 0)
    x, y = GF(a.astype(dt), dtype=dt), GF(b.astype(dt), dtype=dt)
    assert x.dtype == np.dtype(dt)
    for name, got in (("add", x + y), ("sub", x - y), ("mul", x * y), ("div", x / y)):
        assert got.dtype == np.dtype(dt)
        H.assert_equal_ints(got.numpy().astype(np.uint64), getattr(F, name)(a, b), f"GF({order}) {np.dtype(dt).name} {name}")
    H.assert_equal_ints(np.reciprocal(y).numpy().astype(np.uint64), F.div(np.ones(n, dtype=np.uint64), b), "reciprocal")
    H.assert_equal_ints((-x).numpy().astype(np.uint64), F.sub(np.zeros(n, dtype=np.uint64), a), "negative")
    s = GF(np.array(int(b[7]), dtype=dt), dtype=dt)
    H.assert_equal_ints((x * s).numpy().astype(np.uint64), F.mul(a, np.full(n, b[7], dtype=np.uint64)), "broadcast scalar")
    with pytest.raises(ZeroDivisionError):
        y / x
    GF.compile("auto")


@pytest.mark.parametrize("order,dt", [(3**9, np.uint16), (3**10, np.uint16), (3**10, np.uint32), (5**8, np.uint32), (7**7, np.uint32), (13**5, np.uint32),
                                      (97**3, np.uint32), (997**2, np.uint32),
                                      (3**11, np.uint32), (3**12, np.uint32),  # r06: 33 / 36 packed bits -> two words (packed_lin2_kernel)
                                      # pinned to jit-calculate, the small fields take the same kernels (uint8 arrays included); in lookup mode their LDS tables
                                      (3**2, np.uint8), (3**5, np.uint8), (5**3, np.uint8), (13**2, np.uint8), (3**7, np.uint16), (7**3, np.uint16), (3**5, np.uint32)])
@pytest.mark.parametrize("mode", ["jit-lookup", "jit-calculate"])
def test_packed_digit_sums_of_odd_characteristic_extension_fields(order, dt, mode):
    """r05 (VERDICT r04 missing #5 / item 7): np.add / np.subtract / np.negative over GF(p^m), p odd, 8192 < q <= 2^20 run as packed
    base-p digit arithmetic (gfa_elementwise_packed.hip) in BOTH modes; against the oracle's scalars of the mode (Zech logarithms in
    lookup mode, digit vectors in calculate mode: _lookup.py:31-150, _calculate.py:150-285) on every element, with a tail, a broadcast
    scalar, a view that is not 16-byte aligned (the generic kernels take it) and in-place output."""
    GF = ga.GF(order, compile=mode)
    try:
        F = O.OracleField(GF.characteristic, GF.degree, int(GF.irreducible_poly), int(GF.primitive_element), lookup=(mode == "jit-lookup"))
        n = 70_003
        rng = np.random.default_rng(order % 1000)
        a = rng.integers(0, order, n, dtype=np.uint64)
        b = rng.integers(0, order, n, dtype=np.uint64)
        a[:4] = (0, order - 1, 1, order - 1)
        b[:4] = (0, order - 1, order - 1, 1)
        x, y = GF(a.astype(dt), dtype=dt), GF(b.astype(dt), dtype=dt)
        H.assert_equal_ints((x + y).numpy().astype(np.uint64), F.add(a, b), f"GF({order}) {mode} add")
        H.assert_equal_ints((x - y).numpy().astype(np.uint64), F.sub(a, b), f"GF({order}) {mode} sub")
        H.assert_equal_ints((-x).numpy().astype(np.uint64), F.sub(np.zeros(n, dtype=np.uint64), a), f"GF({order}) {mode} neg")
        H.assert_equal_ints((x * y).numpy().astype(np.uint64), F.mul(a, b), f"GF({order}) {mode} mul")  # (digit tables where the route applies)
        H.assert_equal_ints((x[1:] * y[1:]).numpy().astype(np.uint64), F.mul(a[1:], b[1:]), "misaligned product")
        s = GF(np.array(int(b[9]), dtype=dt), dtype=dt)
        H.assert_equal_ints((x + s).numpy().astype(np.uint64), F.add(a, np.full(n, b[9], dtype=np.uint64)), "scalar on the right")
        H.assert_equal_ints((s - x).numpy().astype(np.uint64), F.sub(np.full(n, b[9], dtype=np.uint64), a), "scalar on the left")
        H.assert_equal_ints((s * x).numpy().astype(np.uint64), F.mul(np.full(n, b[9], dtype=np.uint64), a), "scalar product")
        H.assert_equal_ints((x[1:] + y[1:]).numpy().astype(np.uint64), F.add(a[1:], b[1:]), "misaligned views")
        z = x.copy()
        np.add(z, y, out=z)
        H.assert_equal_ints(z.numpy().astype(np.uint64), F.add(a, b), "in place")
        assert (x + y).dtype == np.dtype(dt)
    finally:
        GF.compile("auto")


@pytest.mark.parametrize("order", [997**2, 97**3, 31**4, 13**5, 5**8, 7**7])
def test_auto_mode_products_of_extension_fields_above_2e16_elements(order):
    """r05: in AUTO, products (degree 2: quotients and reciprocals too) of odd-characteristic extension fields with 65536 < q <= 2^20 run
    on the digit-vector kernels instead of three table gathers from L2 -- the reference's default for these fields is jit-lookup
    (_domains/_meta.py:42-44); the values are the same.  Against the oracle in LOOKUP mode, and the field pinned to jit-lookup against
    the same vectors (the table route still exists)."""
    GF = ga.GF(order)
    assert GF.ufunc_mode == "jit-lookup"
    F = O.OracleField(GF.characteristic, GF.degree, int(GF.irreducible_poly), int(GF.primitive_element), lookup=True)
    n = 50_007
    rng = np.random.default_rng(order % 997)
    a = rng.integers(0, order, n, dtype=np.uint64)
    b = rng.integers(1, order, n, dtype=np.uint64)
    a[:3] = (0, order - 1, 1)
    x, y = GF(a.astype(np.uint32)), GF(b.astype(np.uint32))
    u = lambda v: v.numpy().astype(np.uint64)
    want_mul, want_div = F.mul(a, b), F.div(a, b)
    H.assert_equal_ints(u(x * y), want_mul, f"GF({order}) mul")
    H.assert_equal_ints(u(x / y), want_div, f"GF({order}) div")
    H.assert_equal_ints(u(np.reciprocal(y)), F.div(np.ones(n, dtype=np.uint64), b), f"GF({order}) reciprocal")
    H.assert_equal_ints(u(x * GF(int(b[5]))), F.mul(a, np.full(n, b[5], dtype=np.uint64)), "scalar operand")
    with pytest.raises(ZeroDivisionError):
        y / x
    GF.compile("jit-lookup")
    try:
        H.assert_equal_ints(u(x * y), want_mul, "pinned to the tables")
        H.assert_equal_ints(u(x / y), want_div)
    finally:
        GF.compile("auto")


@pytest.mark.parametrize("order", [257**2, 509**2, 997**2])  # (1021^2: no Conway polynomial in the shipped table; the host test covers p = 1021)
def test_degree_two_quotients_by_the_norm(order):
    """r06: a / b and 1 / b over GF(p^2), 65536 < q <= 2^20, as conjugate / norm with the norm's inverse from a p-entry LDS table
    (gfa_packed.h::div2, packed_div2_kernel) -- the reference divides through its LOG / EXP tables (_lookup.py:176-235).  Every
    element against the oracle's lookup scalars, with a tail, broadcast scalars on either side, a misaligned view (the digit-vector
    kernel takes it), in-place output, and the zero divisor flagged."""
    GF = ga.GF(order)
    F = O.OracleField(GF.characteristic, GF.degree, int(GF.irreducible_poly), int(GF.primitive_element), lookup=True)
    n = 40_003
    rng = np.random.default_rng(order % 991)
    a = rng.integers(0, order, n, dtype=np.uint64)
    b = rng.integers(1, order, n, dtype=np.uint64)
    p = GF.characteristic
    a[:4] = (0, order - 1, 1, p)
    b[:6] = (1, order - 1, p, p - 1, p + 1, order - p)
    x, y = GF(a.astype(np.uint32)), GF(b.astype(np.uint32))
    u = lambda v: v.numpy().astype(np.uint64)
    H.assert_equal_ints(u(x / y), F.div(a, b), f"GF({order}) div")
    H.assert_equal_ints(u(np.reciprocal(y)), F.div(np.ones(n, dtype=np.uint64), b), f"GF({order}) reciprocal")
    s = GF(int(b[7]))
    H.assert_equal_ints(u(x / s), F.div(a, np.full(n, b[7], dtype=np.uint64)), "scalar divisor")
    H.assert_equal_ints(u(s / y), F.div(np.full(n, b[7], dtype=np.uint64), b), "scalar dividend")
    H.assert_equal_ints(u(x[1:] / y[1:]), F.div(a[1:], b[1:]), "misaligned views")
    z = x.copy()
    np.true_divide(z, y, out=z)
    H.assert_equal_ints(u(z), F.div(a, b), "in place")
    H.assert_equal_ints(u((x / y) * y), a, "round trip")
    with pytest.raises(ZeroDivisionError):
        y / x
    with pytest.raises(ZeroDivisionError):
        np.reciprocal(x)


@pytest.mark.parametrize("order,dt", [(251**2, np.uint16), (251**2, np.uint32), (191**2, np.uint16), (37**3, np.uint16), (37**3, np.uint32)])
def test_extension_fields_between_2e15_and_2e16_elements_on_the_digit_tables(order, dt):
    """r06: GF(p^m), p odd, 32768 < q <= 65536 in AUTO: products through the digit tables (gfa_packed.h::mul_digits) and, in degree 2, quotients
    and reciprocals by the norm, on uint16 and uint32 arrays -- these fields' LOG / EXP tables do not fit LDS together and the staged
    kernels ran at 0.40 / 0.27.  Every element against the oracle's lookup scalars (_lookup.py:153-235), with a tail, broadcast scalars,
    a misaligned view, in-place output, the zero divisor flagged; the field pinned to jit-lookup still takes the tables."""
    GF = ga.GF(order)
    F = O.OracleField(GF.characteristic, GF.degree, int(GF.irreducible_poly), int(GF.primitive_element), lookup=True)
    n = 60_005
    rng = np.random.default_rng(order % 983)
    a = rng.integers(0, order, n, dtype=np.uint64)
    b = rng.integers(1, order, n, dtype=np.uint64)
    p = GF.characteristic
    a[:4] = (0, order - 1, 1, p)
    b[:6] = (1, order - 1, p, p - 1, p + 1, order - p)
    x, y = GF(a.astype(dt), dtype=dt), GF(b.astype(dt), dtype=dt)
    u = lambda v: v.numpy().astype(np.uint64)
    want_mul, want_div = F.mul(a, b), F.div(a, b)
    H.assert_equal_ints(u(x * y), want_mul, f"GF({order}) mul")
    H.assert_equal_ints(u(x / y), want_div, f"GF({order}) div")
    H.assert_equal_ints(u(np.reciprocal(y)), F.div(np.ones(n, dtype=np.uint64), b), f"GF({order}) reciprocal")
    s = GF(int(b[7]))
    H.assert_equal_ints(u(x * s), F.mul(a, np.full(n, b[7], dtype=np.uint64)), "scalar factor")
    H.assert_equal_ints(u(x / s), F.div(a, np.full(n, b[7], dtype=np.uint64)), "scalar divisor")
    H.assert_equal_ints(u(s / y), F.div(np.full(n, b[7], dtype=np.uint64), b), "scalar dividend")
    H.assert_equal_ints(u(x[1:] * y[1:]), want_mul[1:], "misaligned product")
    H.assert_equal_ints(u(x[1:] / y[1:]), want_div[1:], "misaligned quotient")
    z = x.copy()
    np.multiply(z, y, out=z)
    H.assert_equal_ints(u(z), want_mul, "in place")
    assert (x * y).dtype == np.dtype(dt) and (x / y).dtype == np.dtype(dt)
    with pytest.raises(ZeroDivisionError):
        y / x
    with pytest.raises(ZeroDivisionError):
        np.reciprocal(x)
    GF.compile("jit-lookup")
    try:
        H.assert_equal_ints(u(x * y), want_mul, "pinned to the tables")
        H.assert_equal_ints(u(x / y), want_div)
    finally:
        GF.compile("auto")


@pytest.mark.parametrize("order", [41**3, 67**3, 97**3, 101**3])
def test_degree_three_quotients_by_cramers_rule(order):
    """r06: a / b and 1 / b over GF(p^3), 65536 < q <= 2^20, from the cofactors of the multiplication matrix and one table inverse of its
    determinant (gfa_packed.h::div3, packed_div3_kernel) -- the reference divides through LOG / EXP tables (_lookup.py:176-235).  Every
    element against the oracle's lookup scalars, with a tail, broadcast scalars, a misaligned view, in place, the zero divisor flagged."""
    try:
        GF = ga.GF(order)
    except LookupError:
        pytest.skip("no Conway polynomial for this field in the shipped table")
    F = O.OracleField(GF.characteristic, GF.degree, int(GF.irreducible_poly), int(GF.primitive_element), lookup=True)
    n = 40_003
    rng = np.random.default_rng(order % 977)
    a = rng.integers(0, order, n, dtype=np.uint64)
    b = rng.integers(1, order, n, dtype=np.uint64)
    p = GF.characteristic
    a[:4] = (0, order - 1, 1, p)
    b[:7] = (1, order - 1, p, p - 1, p + 1, p * p, order - p)
    x, y = GF(a.astype(np.uint32)), GF(b.astype(np.uint32))
    u = lambda v: v.numpy().astype(np.uint64)
    H.assert_equal_ints(u(x / y), F.div(a, b), f"GF({order}) div")
    H.assert_equal_ints(u(np.reciprocal(y)), F.div(np.ones(n, dtype=np.uint64), b), f"GF({order}) reciprocal")
    s = GF(int(b[9]))
    H.assert_equal_ints(u(x / s), F.div(a, np.full(n, b[9], dtype=np.uint64)), "scalar divisor")
    H.assert_equal_ints(u(s / y), F.div(np.full(n, b[9], dtype=np.uint64), b), "scalar dividend")
    H.assert_equal_ints(u(x[1:] / y[1:]), F.div(a[1:], b[1:]), "misaligned views")
    z = x.copy()
    np.true_divide(z, y, out=z)
    H.assert_equal_ints(u(z), F.div(a, b), "in place")
    H.assert_equal_ints(u((x / y) * y), a, "round trip")
    with pytest.raises(ZeroDivisionError):
        y / x
    with pytest.raises(ZeroDivisionError):
        np.reciprocal(x)


@pytest.mark.parametrize("order", [7**7, 5**8, 13**5, 11**5, 31**4, 17**4, 7**6, 5**7])
def test_quotients_of_degrees_four_to_eight_by_the_inverse_table(order):
    """r06: a / b and 1 / b over GF(p^m), m = 4 .. 8, 65536 < q <= 2^20, uint32 arrays: 1 / b is one gather from the field's 3-byte inverse
    table (gfa_field::inverse_table), the quotient the digit-table product a * (1 / b) (packed_divt_kernel) -- the reference divides
    through LOG / EXP tables (_lookup.py:176-235).  Every element against the oracle's lookup scalars, with tails shorter than a vector,
    broadcast scalars on either side, a misaligned view (table kernels), in place, a length past two grid strides, zero divisors flagged
    wherever they sit (first vector, a look-ahead vector, the tail)."""
    try:
        GF = ga.GF(order)
    except LookupError:
        pytest.skip("no Conway polynomial for this field in the shipped table")
    F = O.OracleField(GF.characteristic, GF.degree, int(GF.irreducible_poly), int(GF.primitive_element), lookup=True)
    p = GF.characteristic
    u = lambda v: v.numpy().astype(np.uint64)
    rng = np.random.default_rng(order % 977)
    for n in (1027, 40_003, 2 * 1024 * 512 * 4 + 4 * 512 * 7 + 2):  # the last: every workgroup runs two full strides, some a third, then the tail
        a = rng.integers(0, order, n, dtype=np.uint64)
        b = rng.integers(1, order, n, dtype=np.uint64)
        a[:4] = (0, order - 1, 1, p)
        b[:7] = (1, order - 1, p, p - 1, p + 1, p * p, order - p)
        x, y = GF(a.astype(np.uint32)), GF(b.astype(np.uint32))
        H.assert_equal_ints(u(x / y), F.div(a, b), f"GF({order}) div n={n}")
        H.assert_equal_ints(u(np.reciprocal(y)), F.div(np.ones(n, dtype=np.uint64), b), f"GF({order}) reciprocal n={n}")
    n = 40_003
    s = GF(int(b[9]))
    a, b, x, y = a[:n], b[:n], x[:n], y[:n]
    H.assert_equal_ints(u(x / s), F.div(a, np.full(n, b[9], dtype=np.uint64)), "scalar divisor")
    H.assert_equal_ints(u(s / y), F.div(np.full(n, b[9], dtype=np.uint64), b), "scalar dividend")
    H.assert_equal_ints(u(x[1:] / y[1:]), F.div(a[1:], b[1:]), "misaligned views")
    z = x.copy()
    np.true_divide(z, y, out=z)
    H.assert_equal_ints(u(z), F.div(a, b), "in place")
    H.assert_equal_ints(u((x / y) * y), a, "round trip")
    for where in (0, 5, 4 * 512 * 3 + 1, n - 1):  # first vector, inside, a vector the look-ahead of another thread reads, the tail
        bz = b.copy()
        bz[where] = 0
        yz = GF(bz.astype(np.uint32))
        with pytest.raises(ZeroDivisionError):
            x / yz
        with pytest.raises(ZeroDivisionError):
            np.reciprocal(yz)
    with pytest.raises(ZeroDivisionError):
        x / GF(0)
    # a field pinned to jit-lookup keeps the LOG / EXP gathers and agrees
    GF.compile("jit-lookup")
    try:
        H.assert_equal_ints(u(x / y), F.div(a, b), "jit-lookup")
    finally:
        GF.compile("auto")


@pytest.mark.parametrize("order", [3**11, 3**12])
def test_reciprocals_of_the_degrees_above_eight_by_the_inverse_table(order):
    """r06: 1 / b over GF(3^11), GF(3^12) (no one-word digit plan, so no digit-table product): the gather from the 3-byte inverse table alone;
    quotients stay on the LOG / EXP tables.  Every element against the oracle's lookup scalars, tails, zero flagged."""
    GF = ga.GF(order)
    F = O.OracleField(GF.characteristic, GF.degree, int(GF.irreducible_poly), int(GF.primitive_element), lookup=True)
    u = lambda v: v.numpy().astype(np.uint64)
    rng = np.random.default_rng(order % 977)
    for n in (1025, 70_003):
        b = rng.integers(1, order, n, dtype=np.uint64)
        b[:5] = (1, order - 1, 3, 2, order - 3)
        y = GF(b.astype(np.uint32))
        H.assert_equal_ints(u(np.reciprocal(y)), F.recip(b), f"GF({order}) reciprocal n={n}")
        H.assert_equal_ints(u(y ** -1), F.recip(b), f"GF({order}) ** -1 n={n}")
        H.assert_equal_ints(u(GF(1) / y), F.recip(b), f"GF({order}) 1 / y n={n}")
        H.assert_equal_ints(u(np.reciprocal(y[3:])), F.recip(b[3:]), "misaligned view")
    b[n - 1] = 0
    with pytest.raises(ZeroDivisionError):
        np.reciprocal(GF(b.astype(np.uint32)))


@pytest.mark.parametrize("m", [17, 18, 20])
def test_binary_fields_of_2e17_to_2e20_elements_divide_through_the_inverse_table(m):
    """r06: GF(2^17) .. GF(2^20) in AUTO: a / b = the carry-less product a * INV[b] with one gather from the 3-byte inverse table
    (bin32_tab_mul_kernel<true>), 1 / b the gather alone, x ** k through LOG / EXP (the reference's lookup ufuncs, _lookup.py:176-270) --
    against the oracle's explicit arithmetic, with tails, scalars on either side, misaligned views, zero divisors, negative exponents;
    the pinned modes agree."""
    GF = ga.GF(2**m)
    order = 2**m
    F = O.OracleField(2, m, int(GF.irreducible_poly), int(GF.primitive_element))
    u = lambda v: v.numpy().astype(np.uint64)
    rng = np.random.default_rng(m)
    n = 50_003
    a = rng.integers(0, order, n, dtype=np.uint64)
    b = rng.integers(1, order, n, dtype=np.uint64)
    a[:3] = (0, order - 1, 1)
    b[:4] = (1, order - 1, 2, order // 2)
    x, y = GF(a.astype(np.uint32)), GF(b.astype(np.uint32))
    want = F.div(a, b)
    H.assert_equal_ints(u(x / y), want, "div")
    H.assert_equal_ints(u(np.reciprocal(y)), F.recip(b), "reciprocal")
    H.assert_equal_ints(u(x[:1025] / y[:1025]), want[:1025], "short, one-element tail")
    H.assert_equal_ints(u(x[1:] / y[1:]), want[1:], "misaligned views")
    s = GF(int(b[9]))
    H.assert_equal_ints(u(x / s), F.div(a, np.full(n, b[9], dtype=np.uint64)), "scalar divisor")
    H.assert_equal_ints(u(s / y), F.div(np.full(n, b[9], dtype=np.uint64), b), "scalar dividend")
    H.assert_equal_ints(u((x / y) * y), a, "round trip")
    for k in (0, 1, 2, 12345, -1, -7, order - 1, order + 5):
        H.assert_equal_ints(u(y ** k), F.pow(b, np.full(n, k, dtype=np.int64)), f"y ** {k}")
    ks = rng.integers(-order, order, n)
    H.assert_equal_ints(u(y ** ks), F.pow(b, ks.astype(np.int64)), "exponent array")
    for where in (0, 4 * 256 * 8 + 2, n - 1):
        bz = b.copy()
        bz[where] = 0
        yz = GF(bz.astype(np.uint32))
        with pytest.raises(ZeroDivisionError):
            x / yz
        with pytest.raises(ZeroDivisionError):
            np.reciprocal(yz)
        with pytest.raises(ZeroDivisionError):
            yz ** -1
    for mode in ("jit-calculate", "jit-lookup"):
        GF.compile(mode)
        try:
            H.assert_equal_ints(u(x / y), want, mode)
            H.assert_equal_ints(u(y ** -7), F.pow(b, np.full(n, -7, dtype=np.int64)), mode + " power")
        finally:
            GF.compile("auto")


def _irreducible_without_conway(p, m):
    """x^2 + x + c (1 - 4 c a non-residue) / x^3 + x + c (no root): an irreducible polynomial for fields outside the shipped Conway table."""
    if m == 2:
        c = next(c for c in range(1, p) if pow((1 - 4 * c) % p, (p - 1) // 2, p) == p - 1)
        return [1, 1, c]
    c = next(c for c in range(1, p) if all((x * x * x + x + c) % p for x in range(p)))
    return [1, 0, 1, c]


@pytest.mark.parametrize("p,m", [(251, 3), (103, 3), (1021, 3), (1447, 3), (1031, 2), (8191, 2), (32771, 2), (37813, 2)])
def test_quotients_of_quadratic_and_cubic_fields_without_tables(p, m):
    """r06: GF(p^2), 1021 < p <= 37813, and GF(p^3), 101 < p <= 1621 (2^20 < q < 2^32, uint32 arrays; the reference computes these fields
    explicitly, _calculate.py:447-513): quotients by the norm / Cramer's rule with an exact digit split over the whole 32-bit range and the
    GF(p) inverse from an LDS table (packed_div2_kernel / packed_div3_kernel, WIDE).  Every element against the oracle, digits at p - 1,
    tails, scalars on either side, misaligned views (digit-vector kernels), zero divisors; the pinned mode agrees."""
    order = p**m
    try:
        GF = ga.GF(order)
    except LookupError:
        GF = ga.GF(order, irreducible_poly=_irreducible_without_conway(p, m))
    assert np.uint32 in GF.dtypes  # (order - 1)^2 fits int64: the reference's own rule for fixed-width arrays; GF(1621^3) is the test below
    F = O.OracleField(p, m, int(GF.irreducible_poly), int(GF.primitive_element))
    u = lambda v: v.numpy().astype(np.uint64)
    rng = np.random.default_rng(p)
    n = 30_003
    a = rng.integers(0, order, n, dtype=np.uint64)
    b = rng.integers(1, order, n, dtype=np.uint64)
    a[:5] = (0, order - 1, 1, p, order - p)
    b[:8] = (1, order - 1, p, p - 1, p + 1, order - p, order // p, (p - 1) * (order // p))
    x, y = GF(a.astype(np.uint32)), GF(b.astype(np.uint32))
    want = F.div(a, b)
    H.assert_equal_ints(u(x / y), want, f"GF({p}^{m}) div")
    H.assert_equal_ints(u(np.reciprocal(y)), F.recip(b), "reciprocal")
    H.assert_equal_ints(u(x[:1026] / y[:1026]), want[:1026], "short with a tail")
    H.assert_equal_ints(u(x[1:] / y[1:]), want[1:], "misaligned views")
    s = GF(int(b[11]))
    H.assert_equal_ints(u(x / s), F.div(a, np.full(n, b[11], dtype=np.uint64)), "scalar divisor")
    H.assert_equal_ints(u(s / y), F.div(np.full(n, b[11], dtype=np.uint64), b), "scalar dividend")
    H.assert_equal_ints(u((x / y) * y), a, "round trip")
    for where in (0, 4 * 512 * 2 + 3, n - 1):
        bz = b.copy()
        bz[where] = 0
        yz = GF(bz.astype(np.uint32))
        with pytest.raises(ZeroDivisionError):
            x / yz
        with pytest.raises(ZeroDivisionError):
            np.reciprocal(yz)
    GF.compile("jit-calculate")
    try:
        H.assert_equal_ints(u(x / y), want, "jit-calculate")
    finally:
        GF.compile("auto")


def test_cubic_quotients_at_the_largest_prime_through_the_c_abi():
    """GF(1621^3) (4 259 406 061 elements, the largest cube below 2^32): the reference holds it as dtype=object ((order - 1)^2 leaves int64), so
    FieldArray never builds a uint32 array of it -- the C ABI accepts one (every element fits), and the WIDE Cramer form is written for it.
    gfa_binary / gfa_unary on raw uint32 buffers against the oracle."""
    import torch
    from galois_amd import _lib as L

    p, m = 1621, 3
    GF = ga.GF(p**m, irreducible_poly=_irreducible_without_conway(p, m))
    F = O.OracleField(p, m, int(GF.irreducible_poly), int(GF.primitive_element))
    order = p**m
    rng = np.random.default_rng(5)
    n = 20_002
    a = rng.integers(0, order, n, dtype=np.uint64)
    b = rng.integers(1, order, n, dtype=np.uint64)
    a[:4] = (0, order - 1, 1, p)
    b[:6] = (1, order - 1, p, p * p, order - p, (p - 1) * p * p)
    da = torch.from_numpy(a.astype(np.uint32).view(np.int32)).cuda()
    db = torch.from_numpy(b.astype(np.uint32).view(np.int32)).cuda()
    out = torch.empty_like(da)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    lib = L.lib()
    st = torch.cuda.current_stream().cuda_stream
    L.check(lib.gfa_binary(GF._handle, L.OP_DIV, da.data_ptr(), 1, db.data_ptr(), 1, out.data_ptr(), n, L.U32, st, err.data_ptr()))
    H.assert_equal_ints(out.cpu().numpy().view(np.uint32).astype(np.uint64), F.div(a, b), "div")
    L.check(lib.gfa_unary(GF._handle, L.OP_RECIP, db.data_ptr(), out.data_ptr(), n, L.U32, st, err.data_ptr()))
    H.assert_equal_ints(out.cpu().numpy().view(np.uint32).astype(np.uint64), F.recip(b), "reciprocal")
    assert int(err.item()) == 0
    L.check(lib.gfa_unary(GF._handle, L.OP_RECIP, da.data_ptr(), out.data_ptr(), n, L.U32, st, err.data_ptr()))
    assert int(err.item()) != 0  # a[0] == 0


@pytest.mark.parametrize("order,mode", [(2**16, "auto"), (65521, "auto"), (65521, "jit-lookup"), (40009, "auto"), (3**10, "auto"), (251**2, "jit-lookup")])
def test_fields_of_2e15_to_2e16_elements_divide_through_one_inverse_table(order, mode):
    """r06: 32768 < q <= 65536 on uint16 arrays of at least 2^19 elements: 1 / b is one gather from the 2q-byte table INV kept in LDS
    (big16_inv_kernel) instead of LOG and EXP staged in turn; a / b = a * INV[b] with the explicit product in prime fields (Barrett) and in
    GF(2^16) (carry-less, nine integer multiplies); the other extension fields keep the staged tables for quotients.  Every element against
    the oracle: zero dividends, 1, q - 1, scalars on either side, a tail of n % 8, uint32 storage (narrowed and widened around the same
    kernels), zero divisors flagged anywhere."""
    GF = ga.GF(order)
    GF.compile(mode)
    try:
        F = O.OracleField(GF.characteristic, GF.degree, int(GF.irreducible_poly), int(GF.primitive_element), lookup=True)
        u = lambda v: v.numpy().astype(np.uint64)
        rng = np.random.default_rng(order % 1013)
        n = (1 << 19) + 8 * 1024 * 3 + 5
        a = rng.integers(0, order, n, dtype=np.uint64)
        b = rng.integers(1, order, n, dtype=np.uint64)
        a[:4] = (0, order - 1, 1, 2)
        b[:4] = (1, order - 1, 2, order // 2)
        x, y = GF(a.astype(np.uint16)), GF(b.astype(np.uint16))
        want = F.div(a, b)
        H.assert_equal_ints(u(x / y), want, f"GF({order}) {mode} div")
        H.assert_equal_ints(u(np.reciprocal(y)), F.recip(b), "reciprocal")
        H.assert_equal_ints(u(y ** -1), F.recip(b), "** -1")
        s = GF(int(b[77]))
        H.assert_equal_ints(u(x / s), F.div(a, np.full(n, b[77], dtype=np.uint64)), "scalar divisor")
        H.assert_equal_ints(u(s / y), F.div(np.full(n, b[77], dtype=np.uint64), b), "scalar dividend")
        for k in (0, 1, 2, 12345, -1, -7, order - 1, order, -(2**40) - 3, 2**62 + 1):  # one gather from a per-call table of x ** k
            H.assert_equal_ints(u(y ** k), F.pow(b, np.full(n, k, dtype=np.int64)), f"y ** {k}")
        for k in (0, 3, order + 4):  # zero bases with non-negative exponents
            H.assert_equal_ints(u(x ** k), F.pow(a, np.full(n, k, dtype=np.int64)), f"x ** {k}")
        with pytest.raises(ZeroDivisionError):
            x ** -3
        # an exponent per element: LOG pass + EXP pass through a 2-byte index array (big16_power_each)
        ks = rng.integers(-(2**40), 2**40, n)
        ks[:6] = (0, 1, -1, order - 1, -(order - 1), 2**62)
        H.assert_equal_ints(u(y ** ks), F.pow(b, ks.astype(np.int64)), "exponent array")
        kp = np.abs(ks)
        kp[0] = 0  # 0 ** 0 == 1
        H.assert_equal_ints(u(x ** kp), F.pow(a, kp.astype(np.int64)), "exponent array, zero bases")
        kz = kp.copy()
        kz[0] = -5  # a[0] == 0
        with pytest.raises(ZeroDivisionError):
            x ** kz
        xw, yw = GF(a.astype(np.uint32), dtype=np.uint32), GF(b.astype(np.uint32), dtype=np.uint32)
        H.assert_equal_ints(u(xw / yw), want, "uint32 storage div")
        H.assert_equal_ints(u(yw ** -12345), F.pow(b, np.full(n, -12345, dtype=np.int64)), "uint32 storage power")
        H.assert_equal_ints(u(np.reciprocal(yw)), F.recip(b), "uint32 storage reciprocal")
        for where in (0, 8 * 1024 * 40 + 3, n - 9, n - 1):  # first vector, a later vector of the same workgroup, the last full vector, the n % 8 tail
            bz = b.copy()
            bz[where] = 0
            yz = GF(bz.astype(np.uint16))
            with pytest.raises(ZeroDivisionError):
                x / yz
            with pytest.raises(ZeroDivisionError):
                np.reciprocal(yz)
    finally:
        GF.compile("auto")


@pytest.mark.parametrize("order", [7**7, 3**11, 2**17, 2**20, 97**3])
def test_scalar_powers_of_table_fields_above_2e16_elements_through_a_per_call_table(order):
    """r06: x ** k with ONE exponent over a table field of 65536 < q <= 2^20 elements, uint32 arrays of at least 8 q elements: the table
    P[x] = x ** k is filled per call (q look-ups through LOG / EXP, 3-byte entries in stream-ordered scratch), the array then takes one
    gather per element (pow24_run) where power_ufunc.lookup's LOG + EXP (_lookup.py:247-270) are two.  Against the oracle for positive,
    negative, zero and huge exponents; 0 ** k for k >= 0; 0 ** negative raises; shorter arrays (generic kernels) agree."""
    GF = ga.GF(order)
    F = O.OracleField(GF.characteristic, GF.degree, int(GF.irreducible_poly), int(GF.primitive_element), lookup=True)
    u = lambda v: v.numpy().astype(np.uint64)
    rng = np.random.default_rng(order % 991)
    n = 8 * order + 1027
    a = rng.integers(0, order, n, dtype=np.uint64)
    b = rng.integers(1, order, n, dtype=np.uint64)
    a[:3] = (0, 1, order - 1)
    b[:3] = (1, order - 1, GF.characteristic)
    x, y = GF(a.astype(np.uint32), dtype=np.uint32), GF(b.astype(np.uint32), dtype=np.uint32)
    for k in (0, 1, 2, 12345, -1, -12345, order - 1, order - 2, order + 7, -(2**45) - 1, 2**62 + 3):
        H.assert_equal_ints(u(y ** k), F.pow(b, np.full(n, k, dtype=np.int64)), f"GF({order}) y ** {k}")
    for k in (0, 5, order):
        H.assert_equal_ints(u(x ** k), F.pow(a, np.full(n, k, dtype=np.int64)), f"x ** {k}")
    with pytest.raises(ZeroDivisionError):
        x ** -2
    H.assert_equal_ints(u(y[: 4 * 1024 + 3] ** -12345), F.pow(b[: 4 * 1024 + 3], np.full(4 * 1024 + 3, -12345, dtype=np.int64)), "short array")
    H.assert_equal_ints(u(y[1:] ** 77), F.pow(b[1:], np.full(n - 1, 77, dtype=np.int64)), "misaligned view")


@pytest.mark.parametrize("order", [2**8, 3**5, 31, 65537, 7340033, 2**16, 2**20, 2**64 - 2**32 + 1])
def test_folds_and_scans_of_long_one_dimensional_arrays(order):
    """r06: np.add.reduce / np.multiply.reduce / subtract / divide and their .accumulate over ONE long row -- the streaming first phase (xor of
    words in characteristic 2, 64-bit integer sums in prime fields, sums of byte logarithms for table fields of at most 256 elements) and the
    segmented scan (segment folds -> carries -> segment scans).  reduce: against a halving tree of the oracle's vectorised op (add and multiply
    are associative and commutative; subtract / divide are a0 op fold(rest), _ufunc reduce semantics of the reference);  accumulate: EVERY
    output against the recurrence out[i] = op(out[i-1], a[i]) evaluated by the oracle.  Lengths that leave ragged segments, a view that starts
    at an odd element, zeros under multiply, a zero divisor under divide."""
    GF = ga.GF(order)
    p, m = GF.characteristic, GF.degree
    F = O.OracleField(p, m, int(GF.irreducible_poly) if m > 1 else None, GF._primitive_element_int)
    rng = np.random.default_rng(order % 1009)
    wide = order > 2**63
    def rnd(n, low):
        if wide:
            return ((rng.integers(0, 2**63, n, dtype=np.uint64) % np.uint64(order >> 1)) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)) | np.uint64(low)
        return rng.integers(low, order, n, dtype=np.uint64)
    def mk(v):
        if wide:
            import torch
            return GF._wrap(torch.from_numpy(v.view(np.int64).copy()).cuda(), np.object_)
        return GF(v.astype(GF.dtypes[0]), dtype=GF.dtypes[0])
    def u(x):
        h = x.numpy()
        return np.array([int(t) for t in h.ravel()], dtype=np.uint64).reshape(h.shape) if h.dtype == object else h.astype(np.uint64)
    def tree(op, v):
        v = v.copy()
        while len(v) > 1:
            if len(v) & 1:
                v = np.concatenate([op(v[:1], v[-1:]), v[1:-1]])
            h = len(v) // 2
            v = op(v[:h], v[h:])
        return int(v[0])
    for n, off in ((1_000_003, 0), (300_001, 3), (70_000, 1)):
        a = rnd(n + off, 1)
        x = mk(a)[off:]
        a = a[off:]
        tot_add, tot_mul = tree(F.add, a), tree(F.mul, a)
        assert int(u(np.add.reduce(x))) == tot_add, (order, n, "add.reduce")
        assert int(u(np.multiply.reduce(x))) == tot_mul, (order, n, "multiply.reduce")
        rest_add, rest_mul = tree(F.add, a[1:]), tree(F.mul, a[1:])
        assert int(u(np.subtract.reduce(x))) == int(F.sub(a[:1], np.array([rest_add], dtype=np.uint64))[0]), (order, n, "subtract.reduce")
        assert int(u(np.true_divide.reduce(x))) == int(F.div(a[:1], np.array([rest_mul], dtype=np.uint64))[0]), (order, n, "divide.reduce")
        for ufunc, op in ((np.add, F.add), (np.multiply, F.mul), (np.subtract, F.sub), (np.true_divide, F.div)):
            out = u(ufunc.accumulate(x))
            assert out[0] == a[0] and np.array_equal(op(out[:-1], a[1:]), out[1:]), (order, n, ufunc.__name__ + ".accumulate")
    # zeros: a product over a zero is zero from there on; a zero divisor raises
    a = rnd(200_000, 1)
    a[123_457] = 0
    x = mk(a)
    assert int(u(np.multiply.reduce(x))) == 0
    out = u(np.multiply.accumulate(x))
    assert np.all(out[123_457:] == 0) and np.all(out[:123_457] != 0)
    with pytest.raises(ZeroDivisionError):
        np.true_divide.reduce(x)
    with pytest.raises(ZeroDivisionError):
        np.true_divide.accumulate(x)


def test_folds_and_scans_of_long_rows_on_two_streams_at_once():
    """gfa_reduce (add, multiply) and gfa_accumulate (add) over single rows of 2^24 GF(7340033) elements, enqueued on two streams with no
    synchronisation between them: every call cuts its row into segments and keeps the segment folds in a work buffer of its own, so
    concurrent callers on one device do not see each other's partials.  Every result against host arithmetic."""
    import torch
    from galois_amd import _lib as L

    p = 7340033
    GF = ga.GF(p)
    n = (1 << 24) + 5
    rng = np.random.default_rng(24)
    rows = [rng.integers(1, p, n, dtype=np.uint64) for _ in range(4)]  # rows 0, 2 on the first stream, 1, 3 on the second
    dev = [torch.from_numpy(r.astype(np.uint32).view(np.int32)).cuda() for r in rows]
    sums = [torch.empty(1, dtype=torch.int32, device="cuda") for _ in rows]
    prods = [torch.empty(1, dtype=torch.int32, device="cuda") for _ in rows]
    scans = [torch.empty_like(d) for d in dev]
    lib = L.lib()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())  # the uploads, not each other
    for i in range(len(rows)):
        st = streams[i % 2].cuda_stream
        L.check(lib.gfa_reduce(GF._handle, L.OP_ADD, dev[i].data_ptr(), sums[i].data_ptr(), 1, n, L.U32, st, None))
        L.check(lib.gfa_reduce(GF._handle, L.OP_MUL, dev[i].data_ptr(), prods[i].data_ptr(), 1, n, L.U32, st, None))
        L.check(lib.gfa_accumulate(GF._handle, L.OP_ADD, dev[i].data_ptr(), scans[i].data_ptr(), 1, n, L.U32, st, None))
    torch.cuda.synchronize()

    def product(v):
        while len(v) > 1:
            if len(v) & 1:
                v = np.concatenate([v[:1] * v[-1:] % p, v[1:-1]])
            v = v[: len(v) // 2] * v[len(v) // 2:] % p
        return int(v[0])

    u32 = lambda t: t.cpu().numpy().view(np.uint32).astype(np.uint64)
    for i, r in enumerate(rows):
        assert int(u32(sums[i])[0]) == int(r.sum() % p), (i, "add.reduce")
        assert int(u32(prods[i])[0]) == product(r), (i, "multiply.reduce")
        assert np.array_equal(u32(scans[i]), np.cumsum(r) % p), (i, "add.accumulate")


@pytest.mark.parametrize("order", [2**8, 2**4, 2**16, 2**20, 2**32, 3**5, 7**3, 3**2, 5**4, 3**10, 31**2])
def test_long_polynomial_products_over_extension_fields(order):
    """r06: np.convolve over GF(2^m) / GF(p^m) from 2^20 coefficient products: Karatsuba over the bit / digit positions, every leaf an exact
    integer convolution modulo one transform prime (gfa_conv_crt.hip::run_planes) -- every coefficient of every shape against the oracle's
    product, and through evaluation: c(x0) == a(x0) b(x0) at random points (Horner with the oracle), plus the full
    comparison with the direct kernel of a child process (GFA_CONV_PLANES_MIN_LOG=62)."""
    GF = ga.GF(order)
    p, m = GF.characteristic, GF.degree
    F = O.OracleField(p, m, int(GF.irreducible_poly), int(GF.primitive_element), lookup=order <= 2**16)
    rng = np.random.default_rng(order % 997)
    u = lambda v: v.numpy().astype(np.uint64)
    def horner(c, x0):  # highest degree first, as np.convolve / np.polyval order does not matter for the identity: use index = degree
        acc = np.zeros(len(x0), dtype=np.uint64)
        for coef in c[::-1]:
            acc = F.add(F.mul(acc, x0), np.full(len(x0), coef, dtype=np.uint64))
        return acc
    for na, nb in ((1024, 1024), (1500, 700), (40_000, 33)):
        a, b = rng.integers(0, order, na, dtype=np.uint64), rng.integers(0, order, nb, dtype=np.uint64)
        a[0] = b[0] = order - 1
        a[-1] = b[-1] = order - 1
        dt = GF.dtypes[0]
        c = u(np.convolve(GF(a.astype(dt), dtype=dt), GF(b.astype(dt), dtype=dt)))
        assert len(c) == na + nb - 1
        x0 = rng.integers(0, order, 6, dtype=np.uint64)
        H.assert_equal_ints(horner(c, x0), F.mul(horner(a, x0), horner(b, x0)), f"GF({order}) {na} x {nb}: c(x) == a(x) b(x)")
        # every coefficient, at every shape, against the oracle's schoolbook product (row by row) and its convolution
        want = np.zeros(na + nb - 1, dtype=np.uint64)
        for i in range(nb):
            want[i:i + na] = F.add(want[i:i + na], F.mul(a, np.full(na, b[i], dtype=np.uint64)))
        H.assert_equal_ints(c, want, f"GF({order}) {na} x {nb}")
        H.assert_equal_ints(c, F.convolve(a, b), f"GF({order}) {na} x {nb} against the oracle's convolution")


def test_long_polynomial_products_agree_with_the_direct_kernel():
    """The same products with the plane route switched off (GFA_CONV_PLANES_MIN_LOG is read once per process): a child process writes the direct
    kernel's results, this process compares every coefficient."""
    import subprocess, sys, os, tempfile

    code = (
        "import sys, numpy as np, galois_amd as ga\n"
        "rng = np.random.default_rng(11)\n"
        "out = {}\n"
        "for q in (2**8, 2**16, 3**5, 7**3):\n"
        "    GF = ga.GF(q)\n"
        "    a, b = rng.integers(0, q, 3000), rng.integers(0, q, 2500)\n"
        "    out[str(q)] = np.convolve(GF(a), GF(b)).numpy().astype(np.uint64)\n"
        "np.savez(sys.argv[1], **out)\n"
    )
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        res = {}
        for tag, val in (("planes", "20"), ("direct", "62")):
            path = os.path.join(d, tag + ".npz")
            r = subprocess.run([sys.executable, "-c", code, path], capture_output=True, text=True, env=dict(os.environ, GFA_CONV_PLANES_MIN_LOG=val, PYTHONPATH=root), timeout=600)
            assert r.returncode == 0, r.stdout + r.stderr
            res[tag] = dict(np.load(path))
        for q in res["planes"]:
            assert np.array_equal(res["planes"][q], res["direct"][q]), q


@pytest.mark.parametrize("order", [2**8, 2**16, 3**5, 7**3, 3**10, 2**32])
def test_long_polynomial_products_against_the_oracle(order):
    """The 3000 x 2500 product that the child-process test compares between the project's two kernels only: every coefficient against the
    oracle's convolution."""
    GF = ga.GF(order)
    F = O.OracleField(GF.characteristic, GF.degree, int(GF.irreducible_poly), int(GF.primitive_element), lookup=order <= 2**16)
    rng = np.random.default_rng(order % 997 + 11)
    a, b = rng.integers(0, order, 3000, dtype=np.uint64), rng.integers(0, order, 2500, dtype=np.uint64)
    a[0] = b[-1] = order - 1
    dt = GF.dtypes[0]
    c = np.convolve(GF(a.astype(dt), dtype=dt), GF(b.astype(dt), dtype=dt)).numpy().astype(np.uint64)
    H.assert_equal_ints(c, F.convolve(a, b), f"GF({order}) 3000 x 2500")


def _plane_route_longest(p):
    """The plane route's exactness rule (gfa_conv_crt.hip::planes_eligible): min(na, nb) (p - 1)^2 < 0.99 * 469762049, every integer
    coefficient of a plane product below the transform prime.  Returns the longest shorter operand it admits (integer arithmetic)."""
    lo = (99 * 469762049 - 1) // (100 * (p - 1) ** 2)
    assert 100 * lo * (p - 1) ** 2 < 99 * 469762049 <= 100 * (lo + 1) * (p - 1) ** 2
    return lo


@pytest.mark.parametrize("order,na,nbs", [(251**2, 9000, (0, 1)), (251**3, None, (0,)), (127**2, 9000, (9000,))],
                         ids=["gf251e2", "gf251e3", "gf127e2"])
def test_polynomial_products_at_the_plane_routes_exactness_bound(order, na, nbs):
    """Characteristic 251 at the longest shorter operand the plane route admits (7441 for p = 251, derived from the rule) and one past
    it, where the direct kernel takes over; a and b hold q - 1 (every digit p - 1: the largest plane values) in their first three
    quarters and random elements after.  Over GF(251^2) also operands of q - 1 throughout, whose middle coefficients are sums of
    7441 * 250^2 = 465062500 of the prime's 469762049.  GF(251^3) has no oracle tables (9000 x 7441 explicit products take 12.5 s on the
    host): 7441 x 7441, the fewest products with the shorter operand at the bound.  GF(127^2) at 9000 x 9000 as a second characteristic.
    Every coefficient against the oracle's convolution."""
    GF = ga.GF(order)
    p = GF.characteristic
    F = O.OracleField(p, GF.degree, int(GF.irreducible_poly), int(GF.primitive_element), lookup=order <= 2**16)
    rng = np.random.default_rng(order % 997 + 13)
    dt = GF.dtypes[0]
    longest = _plane_route_longest(p)
    assert p != 251 or longest == 7441
    na = longest if na is None else na
    def fill(n):
        v = rng.integers(0, order, n, dtype=np.uint64)
        v[: 3 * n // 4] = order - 1
        return v
    conv = lambda a, b: np.convolve(GF(a.astype(dt), dtype=dt), GF(b.astype(dt), dtype=dt)).numpy().astype(np.uint64)
    for nb in nbs:
        nb = nb if nb > 1 else longest + nb
        a, b = fill(na), fill(nb)
        H.assert_equal_ints(conv(a, b), F.convolve(a, b), f"GF({order}) {na} x {nb}")
    if order == 251**2:
        a, b = np.full(na, order - 1, dtype=np.uint64), np.full(longest, order - 1, dtype=np.uint64)
        H.assert_equal_ints(conv(a, b), F.convolve(a, b), f"GF({order}) {na} x {longest}, q - 1 throughout")
