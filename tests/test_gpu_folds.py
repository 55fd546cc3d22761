"""ufunc.reduce / accumulate / reduceat of gfa_reduce.hip on every route a call can take: segments per row x first-phase kernel x joining
kernel x storage width x row count, every entry of every row against the oracle.

A call is cut into a route by integer arithmetic (galois_amd/csrc/gfa_reduce_plan.h); tests/fold_plan.py mirrors it (kept honest on the CPU
by tests/test_reduce_plan_host.py).  Every case here takes its shapes from that mirror and the CU count of the device it runs on, and
asserts before launching that the shape lands on the route its name claims; test_every_route_is_visited closes the list.

Expected values: add / multiply -- a halving tree of the oracle's vectorised op along axis 1 of the whole array; subtract / divide --
a0 op tree(rest) (the reference's left folds); accumulate -- EVERY output by the recurrence out[:, 0] == a[:, 0],
out[:, 1:] == op(out[:, :-1], a[:, 1:]); prime fields below 2^32 also against NumPy's integer sums."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import galois_amd as ga
from galois_amd import _lib as L
from oracle import gf_oracle as O
from tests import fold_plan as P

pytestmark = pytest.mark.gpu

GOLDILOCKS = 2**64 - 2**32 + 1
UFUNCS = {"add": np.add, "subtract": np.subtract, "multiply": np.multiply, "divide": np.true_divide}


# ---- fields, storage widths, arithmetic modes ----------------------------------------------------------------------------------
class FieldCase:
    """One field in one storage dtype and one arithmetic mode.  dtype None: the field's first dtype; "u32": 4-byte storage of a field whose
    NumPy dtype would be object (GF(4294967291): the largest prime the 32-bit integer-sum form can meet)."""

    def __init__(self, order, dtype=None, mode="auto"):
        self.order, self.dtype, self.mode = order, dtype, mode
        self.id = f"gf{order}-{dtype or 'first'}-{mode.replace('jit-', '')}"

    @functools.cached_property
    def GF(self):
        return ga.GF(self.order)

    @functools.cached_property
    def F(self):
        GF = self.GF
        p, m = GF.characteristic, GF.degree
        return O.OracleField(p, m, int(GF.irreducible_poly) if m > 1 else None, GF._primitive_element_int, lookup=m > 1 and self.order <= 2**16)

    @property
    def np_dtype(self):
        if self.dtype == "u32":
            return np.dtype(np.uint32)
        return np.dtype(self.GF.dtypes[0] if self.dtype is None else self.dtype)

    @property
    def elem_size(self):
        return 8 if self.np_dtype == np.dtype(object) else self.np_dtype.itemsize

    @contextlib.contextmanager
    def compiled(self):
        self.GF.compile(self.mode)
        try:
            yield self.GF
        finally:
            self.GF.compile("auto")

    def lookup(self):
        return L.lib().gfa_field_get_mode(self.GF._handle) == L.MODE_LOOKUP

    def mk(self, v):
        """uint64 host values -> a device array of the field in this case's storage."""
        GF, dt = self.GF, self.np_dtype
        if dt == np.dtype(object):
            return GF._wrap(torch.from_numpy(np.ascontiguousarray(v).view(np.int64).copy()).cuda(), np.object_)
        if self.dtype == "u32":
            return GF._wrap(torch.from_numpy(v.astype(np.uint32).view(np.int32)).cuda(), np.uint32)
        return GF(v.astype(dt), dtype=dt)

    def rnd(self, rng, shape, low):
        q = self.order
        if q > 2**63:
            n = int(np.prod(shape))
            v = (rng.integers(0, 2**63, n, dtype=np.uint64) % np.uint64(q >> 1)) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
            return (v | np.uint64(low)).reshape(shape)
        return rng.integers(low, q, shape, dtype=np.uint64)

    def plan(self, kind, op, n_outer, n_inner):
        GF = self.GF
        return P.plan(kind, P.OPS[op], n_outer, n_inner, self.elem_size, GF.characteristic, GF.degree, self.order, self.lookup(), cus())


def _all_widths(order, modes=("auto",)):
    return [FieldCase(order, np.dtype(d).name, mode) for mode in modes for d in ga.GF(order).dtypes]


FIELD_CASES = (
    [FieldCase(2, "uint8")]
    + _all_widths(2**8, ("jit-lookup", "jit-calculate"))
    + [FieldCase(2**16, "uint16"), FieldCase(2**20, "uint32"), FieldCase(2**40)]
    + _all_widths(3) + _all_widths(31)
    + [FieldCase(65521, "uint16"), FieldCase(4294967291, "u32")]
    + [FieldCase(q, d) for q in (3**2, 7**2, 3**5) for d in ("uint8", "uint32")]
    + [FieldCase(3**10, None, "jit-calculate"), FieldCase(3**10, None, "jit-lookup"), FieldCase(GOLDILOCKS)]
)
# the scan of one row of more than 256 segments: GF(2^8) in bytes, GF(65521), GF(3^5) in bytes and Goldilocks (xor, integer-sum, sum-table
# and generic folds; log-sum and generic products), and one more case per remaining width of the xor and integer-sum forms
LONG_SCAN_CASES = [FieldCase(2**8, "uint8"), FieldCase(65521, "uint16"), FieldCase(3**5, "uint8"), FieldCase(GOLDILOCKS),
                   FieldCase(2**8, "uint16"), FieldCase(2**8, "uint32"), FieldCase(2**8, "int64"), FieldCase(31, "uint8"), FieldCase(31, "uint32")]
PROBE_CASES = [FieldCase(2, "uint8"), FieldCase(2**8, "uint8"), FieldCase(2**8, "int64"), FieldCase(2**8, "uint16", "jit-calculate"),
               FieldCase(3, "uint8"), FieldCase(31, "uint16"), FieldCase(3**2, "uint8"), FieldCase(3**5, "uint32"), FieldCase(65521, "uint16"),
               FieldCase(3**10, None, "jit-calculate"), FieldCase(GOLDILOCKS)]
ids = lambda cases: [c.id for c in cases]


@functools.lru_cache(None)
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count  # what the library's num_cus() reads


def host(x):
    """Every element of a device array as uint64, read from its storage."""
    h = x._t.cpu().numpy()
    return h.view(np.dtype(f"u{h.dtype.itemsize}")).astype(np.uint64)


# ---- expected values -----------------------------------------------------------------------------------------------------------
def tree(op, v, ident):
    """Halving tree of a commutative, associative oracle op along axis 1."""
    if v.shape[1] == 0:
        return np.full(v.shape[0], ident, dtype=np.uint64)
    while v.shape[1] > 1:
        if v.shape[1] & 1:
            v = np.concatenate([op(v[:, :1], v[:, -1:]), v[:, 1:-1]], axis=1)
        h = v.shape[1] // 2
        v = op(v[:, :h], v[:, h:])
    return v[:, 0].copy()


def expected_reduce(F, op, a):
    if op == "add":
        return tree(F.add, a, 0)
    if op == "multiply":
        return tree(F.mul, a, 1)
    if op == "subtract":
        return F.sub(a[:, 0], tree(F.add, a[:, 1:], 0))
    return F.div(a[:, 0], tree(F.mul, a[:, 1:], 1))


def check_scan(F, op, a, out, what):
    """out[:, 0] == a[:, 0] and out[:, i] == op(out[:, i - 1], a[:, i]) at every i.  Under divide the elements a[:, 1:] are non-zero, and then
    out[i] == out[i - 1] / a[i] exactly when out[i] * a[i] == out[i - 1]: the same recurrence, asked with the oracle's product (its
    division of 2^40-element fields takes seconds per array)."""
    f = {"add": F.add, "subtract": F.sub, "multiply": F.mul}.get(op)
    assert out.shape == a.shape and (F.q >= 2**64 or not (out >= F.q).any()), what
    assert np.array_equal(out[:, 0], a[:, 0]), what
    if a.shape[1] > 1:
        if op == "divide":
            assert a[:, 1:].all(), what
            bad = np.argwhere(F.mul(out[:, 1:], a[:, 1:]) != out[:, :-1])
        else:
            bad = np.argwhere(f(out[:, :-1], a[:, 1:]) != out[:, 1:])
        assert bad.size == 0, (what, "first wrong entry (row, column - 1)", bad[0].tolist(), len(bad))
    if op == "add" and F.m == 1 and F.p < 2**32:  # NumPy's integer sums (columns * p < 2^64)
        assert np.array_equal(out, np.cumsum(a, axis=1, dtype=np.uint64) % np.uint64(F.p)), what


def join_class(pl):
    if pl.nseg == 1:
        return "one segment"
    if pl.join == "carries":
        return "carries c=1" if pl.c == 1 else "carries c>=2"
    if pl.n_outer > 1:
        return pl.join + " join, several rows"
    return pl.join + " join, one row"


def form_name(pl, fc, op):
    form = pl.form
    if form is None:
        return "whole-row scan"
    if form == P.GENERIC:
        return "generic multiply" if op in ("multiply", "divide") else "generic add"
    if form in (P.STREAM_XOR, P.STREAM_SUM):
        return f"stream {form} at {fc.elem_size} bytes"
    return f"stream {form}"


def route(fc, kind, op, n_outer, n_inner, expect=None):
    """The plan of a call; `expect` (nseg, join) is what the case's name claims."""
    pl = fc.plan(kind, op, n_outer, n_inner)
    if expect is not None:
        assert (pl.nseg, pl.join) == expect, (fc.id, kind, op, n_outer, n_inner, pl)
    return pl


def run_reduce(fc, x, a, op, expect=None, what=""):
    rows, n = a.shape
    route(fc, "reduce", op, rows, n, expect)
    got = UFUNCS[op].reduce(x, axis=x.ndim - 1)
    assert type(got) is fc.GF
    got = host(got).reshape(-1)
    want = expected_reduce(fc.F, op, a)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (fc.id, op + ".reduce", a.shape, what, "rows", bad[:8].tolist())
    if op == "add" and fc.F.m == 1 and fc.F.p < 2**32:
        assert np.array_equal(got, a.sum(axis=1, dtype=np.uint64) % np.uint64(fc.F.p))


def run_scan(fc, x, a, op, expect=None, what=""):
    rows, n = a.shape
    route(fc, "accumulate", op, rows, n, expect)
    got = UFUNCS[op].accumulate(x, axis=x.ndim - 1)
    assert type(got) is fc.GF and got.dtype == x.dtype
    check_scan(fc.F, op, a, host(got).reshape(a.shape), (fc.id, op + ".accumulate", a.shape, what))


def variants(fc, rng, rows, n, low):
    """(device array, host values, name): a rows x n array; the view [:, 1:] of an array one column wider (rows of another pitch, made
    contiguous by the front end); the 1-D view [3:] of n + 3 elements (a row that starts 3 elements past an aligned address)."""
    a = fc.rnd(rng, (rows, n), low)
    yield fc.mk(a), a, "array"
    w = fc.rnd(rng, (rows, n + 1), low)
    yield fc.mk(w)[:, 1:], w[:, 1:], "column view"
    v = fc.rnd(rng, (n + 3,), low)
    yield fc.mk(v)[3:], v[None, 3:], "offset view"


def left(op):
    return op in ("subtract", "divide")


SEG_MIN, SPLIT_ABOVE, BLOCK_ABOVE = 4096, 8192, 8   # gfa_reduce: a segment's least length, the longest unsplit row, the per-thread join's most segments
SCAN_FROM, SCAN_SEG = 65536, 8192                   # gfa_accumulate: the shortest split row and its segment length there

# (rows, columns, {False: (nseg, join) of add / multiply, True: of subtract / divide, which fold columns - 1}): the shapes the two route
# tests below run over every FIELD_CASES entry, and test_every_route_is_visited plans once more -- one table, so that a shape or a field
# taken out of the tests leaves the closing check with it
REDUCE_SHAPES = [
    (5, SPLIT_ABOVE, {False: (1, "thread"), True: (1, "thread")}),
    (5, SPLIT_ABOVE + 1, {False: (3, "thread"), True: (1, "thread")}),
    (5, SPLIT_ABOVE + 2, {False: (3, "thread"), True: (3, "thread")}),
    (3, 9 * SEG_MIN + 3139, {False: (10, "block"), True: (10, "block")}),  # 40 003
    (1, BLOCK_ABOVE * SEG_MIN, {False: (8, "thread"), True: (8, "thread")}),
    (1, BLOCK_ABOVE * SEG_MIN + 1, {False: (9, "block"), True: (8, "thread")}),
    (1, BLOCK_ABOVE * SEG_MIN + 2, {False: (9, "block"), True: (9, "block")}),
]
_WHOLE, _SPLIT = (1, "row"), (SCAN_FROM // SCAN_SEG, "carries")
SCAN_SHAPES = [
    (2, SCAN_FROM - 1, {False: _WHOLE, True: _WHOLE}),
    (2, SCAN_FROM, {False: _SPLIT, True: _WHOLE}),
    (2, SCAN_FROM + 1, {False: _SPLIT, True: _SPLIT}),
    (3, 70_001, {False: _SPLIT, True: _SPLIT}),
]


# ---- reduce --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fc", FIELD_CASES, ids=ids(FIELD_CASES))
def test_reduce_on_every_segment_route(fc):
    """Thresholds (8192 | 8193 columns, 8194 for subtract / divide, which fold n - 1), the block finaliser with several rows and a ragged last
    segment, 8 against 9 segments of one row, short rows in great number; each 2-D shape once more as a column view and as an offset 1-D view."""
    rng = np.random.default_rng(fc.order % 1009 + fc.elem_size)
    with fc.compiled():
        for rows, n, expect in REDUCE_SHAPES:
            pl = fc.plan("reduce", "add", rows, n)
            if pl.nseg == 10:
                assert n % pl.seg_len != 0 and P.segments(pl)[-1][1] - P.segments(pl)[-1][0] < pl.seg_len  # a ragged last segment
            for low, ops in ((0, ("add", "subtract")), (1, ("multiply", "divide"))):
                for x, a, what in variants(fc, rng, rows, n, low):
                    for op in ops:
                        run_reduce(fc, x, a, op, expect[left(op)] if a.shape[0] == rows else None, what)
        for rows, n in ((100_000, 3), (4096, 1)):  # n_inner == 1 under subtract / divide: a0, and nothing raised
            for low, ops in ((0, ("add", "subtract")), (1, ("multiply", "divide"))):
                a = fc.rnd(rng, (rows, n), low)
                x = fc.mk(a)
                for op in ops:
                    run_reduce(fc, x, a, op, (1, "thread"))
                    run_scan(fc, x, a, op, (1, "row"))
        z = np.zeros((4096, 1), dtype=np.uint64)  # a0 == 0 with nothing to divide by
        assert not host(np.true_divide.reduce(fc.mk(z), axis=1)).any() and not host(np.true_divide.accumulate(fc.mk(z), axis=1)).any()


@pytest.mark.parametrize("fc", [FieldCase(2**8, "uint8"), FieldCase(65521, "uint16")], ids=["gf256", "gf65521"])
def test_reduce_where_the_row_count_limits_the_segments(fc):
    """Just more rows than half the workgroups the planner wants: 2 segments per row although the length would give 3."""
    rng = np.random.default_rng(5)
    with fc.compiled():
        for op, low in (("add", 0), ("multiply", 1)):
            tab = P.table_sum(P.OPS[op], fc.elem_size, fc.GF.degree, fc.order, fc.lookup())
            rows, n = cus() * (2 if tab else 8) // 2 + 1, 2 * SEG_MIN + 809  # 9001
            assert (n + SEG_MIN - 1) // SEG_MIN == 3 and rows * n <= 10_000_000
            a = fc.rnd(rng, (rows, n), low)
            run_reduce(fc, fc.mk(a), a, op, (2, "thread"))


# ---- accumulate ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fc", FIELD_CASES, ids=ids(FIELD_CASES))
def test_accumulate_on_every_segment_route(fc):
    """65535 | 65536 columns (65537 for subtract / divide), several rows with a ragged last segment; the views as in the reduce test."""
    rng = np.random.default_rng(fc.order % 1013 + fc.elem_size)
    with fc.compiled():
        pl = fc.plan("accumulate", "add", 3, 70_001)
        assert pl.seg_len % 256 == 0 and 70_001 % pl.seg_len != 0 and pl.c == 1
        for rows, n, expect in SCAN_SHAPES:
            for low, ops in ((0, ("add", "subtract")), (1, ("multiply", "divide"))):
                for x, a, what in variants(fc, rng, rows, n, low):
                    for op in ops:
                        run_scan(fc, x, a, op, expect[left(op)] if a.shape[0] == rows else None, what)


def long_scan_length(fc):
    """The shortest of a ladder of odd lengths at which one row is cut into more than 256 segments (2 200 001 at 256 CUs: 261 segments)."""
    for n in range(2_000_001, 4_000_002, 50_000):
        if fc.plan("accumulate", "add", 1, n).c >= 2 and fc.plan("accumulate", "divide", 1, n).c >= 2:
            return n
    raise AssertionError("no length of the ladder gives more than 256 segments on this device")


@pytest.mark.parametrize("fc", LONG_SCAN_CASES, ids=ids(LONG_SCAN_CASES))
def test_accumulate_of_one_row_in_more_than_256_segments(fc):
    """accumulate_carries_kernel with two runs per thread, under all four ops."""
    rng = np.random.default_rng(fc.order % 1019 + fc.elem_size)
    with fc.compiled():
        n = long_scan_length(fc)
        assert cus() != 256 or (n, fc.plan("accumulate", "add", 1, n).nseg) == (2_200_001, 261)
        for low, ops in ((0, ("add", "subtract")), (1, ("multiply", "divide"))):
            a = fc.rnd(rng, (1, n), low)
            x = fc.mk(a[0])
            for op in ops:
                pl = route(fc, "accumulate", op, 1, n)
                assert pl.join == "carries" and pl.c >= 2
                run_scan(fc, x, a, op)
                run_reduce(fc, x, a, op)


# ---- adversarial values ----------------------------------------------------------------------------------------------------------
def probe_columns(pl):
    segs = P.segments(pl)
    n, s = pl.n_inner, pl.seg_len
    cols = [0, 1, 2, 15, 16, 17, s - 1, s, s + 1, segs[-1][0], segs[-1][1] - 1] + list(range(n - 17, n))
    assert all(0 <= c < n for c in cols)
    return cols


@pytest.mark.parametrize("fc", PROBE_CASES, ids=ids(PROBE_CASES))
def test_one_marked_element_on_every_boundary(fc):
    """An array of identities with ONE marked element per row (1 under add, the primitive element under multiply), on the columns where the
    kernels change hands: the ends of the 16-byte head and tail, both sides of the first segment boundary, the ends of the last segment, the
    last 17 columns.  A dropped element gives the identity, a doubled one 2 x mark / mark^2 (0 / 1 only in characteristic 2 / GF(2), where a
    doubled element is a dropped one's twin): every row must give exactly the mark, every scan the step function."""
    alpha = fc.GF._primitive_element_int
    with fc.compiled():
        for n, want_join in ((3 * SEG_MIN + 3, "thread"), (9 * SEG_MIN + 3139, "block"), (70_001, "carries")):
            for op, ident, mark in (("add", 0, 1), ("multiply", 1, alpha)):
                kind = "accumulate" if want_join == "carries" else "reduce"
                rows = 28  # len(probe_columns): the row count enters the plan, so the columns come from the plan of that row count
                pl = route(fc, kind, op, rows, n)
                assert pl.join == want_join and pl.nseg > 1, pl
                cols = probe_columns(pl)
                assert len(cols) == rows
                a = np.full((rows, n), ident, dtype=np.uint64)
                a[np.arange(rows), cols] = mark
                x = fc.mk(a)
                if kind == "reduce":
                    got = host(UFUNCS[op].reduce(x, axis=1))
                    assert np.array_equal(got, np.full(rows, mark, dtype=np.uint64)), (fc.id, op, n, [c for c, g in zip(cols, got) if g != mark])
                step = np.where(np.arange(n)[None, :] >= np.array(cols)[:, None], mark, ident).astype(np.uint64)
                if kind == "accumulate" or n < 20_000:
                    got = host(UFUNCS[op].accumulate(x, axis=1))
                    bad = np.argwhere(got != step)
                    assert bad.size == 0, (fc.id, op + ".accumulate", n, "first wrong (row, column)", bad[0].tolist(), "marked column", cols[bad[0][0]])


@pytest.mark.parametrize("fc", [FieldCase(4294967291, "u32"), FieldCase(65521, "uint16")], ids=["gf4294967291", "gf65521"])
def test_sums_of_the_largest_element(fc):
    """Every element p - 1: the largest 64-bit integer sums the prime-field form can meet, against Python integers."""
    p = fc.order
    with fc.compiled():
        for rows, n in ((3, 70_001), (1, 2_200_001)):
            pl = route(fc, "reduce", "add", rows, n)
            assert pl.form == P.STREAM_SUM and pl.join == "block"
            a = np.full((rows, n), p - 1, dtype=np.uint64)
            x = fc.mk(a if rows > 1 else a[0])
            assert host(np.add.reduce(x, axis=x.ndim - 1)).reshape(-1).tolist() == [n * (p - 1) % p] * rows
            assert host(np.subtract.reduce(x, axis=x.ndim - 1)).reshape(-1).tolist() == [(p - 1 - (n - 1) * (p - 1)) % p] * rows
            pl = route(fc, "accumulate", "add", rows, n)
            assert pl.form == P.STREAM_SUM and pl.join == "carries"
            want = (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(p - 1)) % np.uint64(p)  # n (p - 1) < 2^64
            assert np.array_equal(host(np.add.accumulate(x, axis=x.ndim - 1)).reshape(rows, n), np.broadcast_to(want, (rows, n)))


@pytest.mark.parametrize("fc", [FieldCase(2**8, "uint8"), FieldCase(31, "uint8")], ids=["gf256", "gf31"])
def test_products_of_the_element_with_the_largest_logarithm(fc):
    """Every element alpha^(q - 2): the largest sums of byte logarithms, against the oracle's power."""
    q, F = fc.order, fc.F
    v = int(F.pow(np.array([fc.GF._primitive_element_int], dtype=np.uint64), np.array([q - 2], dtype=np.int64))[0])
    with fc.compiled():
        assert L.lib().gfa_field_get_mode(fc.GF._handle) == L.MODE_LOOKUP
        for rows, n in ((3, 70_001), (1, 2_200_001)):
            pl = route(fc, "reduce", "multiply", rows, n)
            assert pl.form == P.STREAM_LOG and pl.join == "block"
            a = np.full((rows, n), v, dtype=np.uint64)
            x = fc.mk(a if rows > 1 else a[0])
            assert host(np.multiply.reduce(x, axis=x.ndim - 1)).reshape(-1).tolist() == [int(F.pow(np.array([v], dtype=np.uint64), np.array([n], dtype=np.int64))[0])] * rows
            assert route(fc, "accumulate", "multiply", rows, n).form == P.STREAM_LOG
            want = F.pow(np.full(n, v, dtype=np.uint64), np.arange(1, n + 1, dtype=np.int64))
            assert np.array_equal(host(np.multiply.accumulate(x, axis=x.ndim - 1)).reshape(rows, n), np.broadcast_to(want, (rows, n)))


ZERO_CASES = [FieldCase(2, "uint8"), FieldCase(2**8, "uint8"), FieldCase(2**8, "uint32"), FieldCase(31, "uint8"), FieldCase(3**5, "uint8"), FieldCase(65521, "uint16"),
              FieldCase(3**10, None, "jit-calculate"), FieldCase(GOLDILOCKS)]


@pytest.mark.parametrize("fc", ZERO_CASES, ids=ids(ZERO_CASES))
def test_a_zero_in_one_row_of_three(fc):
    """A zero at (1, j): multiply.accumulate is zero in row 1 from j on and leaves rows 0 and 2 alone; divide raises exactly when j > 0; a zero
    in column 0 alone gives an all-zero row."""
    rng = np.random.default_rng(fc.order % 1021)
    n = 70_001
    with fc.compiled():
        seg_len = route(fc, "accumulate", "multiply", 3, n).seg_len
        assert 0 < seg_len < n
        base = fc.rnd(rng, (3, n), 1)
        clean = host(np.multiply.accumulate(fc.mk(base), axis=1))
        check_scan(fc.F, "multiply", base, clean, (fc.id, "no zero"))
        clean_div_scan, clean_div = host(np.true_divide.accumulate(fc.mk(base), axis=1)), host(np.true_divide.reduce(fc.mk(base), axis=1))
        for j in (0, 1, seg_len, n - 1):
            a = base.copy()
            a[1, j] = 0
            x = fc.mk(a)
            out = host(np.multiply.accumulate(x, axis=1))
            assert not out[1, j:].any() and np.array_equal(out[1, :j], clean[1, :j]) and np.array_equal(out[[0, 2]], clean[[0, 2]]), (fc.id, j)
            red = host(np.multiply.reduce(x, axis=1))
            assert red[1] == 0 and np.array_equal(red[[0, 2]], clean[[0, 2], -1]), (fc.id, j)
            if j == 0:
                out, red = host(np.true_divide.accumulate(x, axis=1)), host(np.true_divide.reduce(x, axis=1))
                assert not out[1].any() and np.array_equal(out[[0, 2]], clean_div_scan[[0, 2]]) and red[1] == 0 and np.array_equal(red[[0, 2]], clean_div[[0, 2]])
            else:
                with pytest.raises(ZeroDivisionError):
                    np.true_divide.accumulate(x, axis=1)
                with pytest.raises(ZeroDivisionError):
                    np.true_divide.reduce(x, axis=1)


@pytest.mark.parametrize("fc", [FieldCase(2**8, "uint8"), FieldCase(65521, "uint16"), FieldCase(31, "uint32")], ids=["gf256", "gf65521", "gf31"])
def test_an_empty_axis(fc):
    """NumPy's rule, as the fields of order >= 2^64 follow it: identities for add / multiply, ValueError for subtract / divide, an empty scan."""
    GF = fc.GF
    e = fc.mk(np.arange(1, 16, dtype=np.uint64).reshape(3, 5))[:, :0]
    assert e.shape == (3, 0)
    assert host(np.add.reduce(e, axis=1)).tolist() == [0, 0, 0] and host(np.multiply.reduce(e, axis=1)).tolist() == [1, 1, 1]
    assert type(np.add.reduce(e, axis=1)) is GF and np.add.reduce(e, axis=1).dtype == e.dtype
    assert np.add.reduce(e, axis=1, keepdims=True).shape == (3, 1) and np.add.reduce(e, axis=0).shape == (0,)
    assert int(np.sum(e[0])) == 0 and int(np.prod(e[0])) == 1
    for uf in UFUNCS.values():
        assert uf.accumulate(e, axis=1).shape == (3, 0)
    for uf in (np.subtract, np.true_divide):
        with pytest.raises(ValueError):
            uf.reduce(e, axis=1)


# ---- reduceat --------------------------------------------------------------------------------------------------------------------
def left_fold(F, op, a, starts, ends):
    """Sequential left folds of a[..., starts[i]:ends[i]] (an empty or reversed slice yields a[..., starts[i]]), the segments along the last
    axis, all segments stepping together."""
    f = {"add": F.add, "subtract": F.sub, "multiply": F.mul, "divide": F.div}[op]
    starts = np.asarray(starts)
    ends = np.maximum(np.asarray(ends), starts + 1)
    acc = a[..., starts].copy()
    for k in range(1, int((ends - starts).max())):
        live = np.flatnonzero(starts + k < ends)
        acc[..., live] = f(acc[..., live], a[..., starts[live] + k])
    return acc


REDUCEAT_CASES = [FieldCase(q) for q in (2, 2**8, 31, 3**5, 65537, 2**32, GOLDILOCKS)]


@pytest.mark.parametrize("fc", REDUCEAT_CASES, ids=ids(REDUCEAT_CASES))
def test_reduceat_over_segments_longer_than_a_workgroup(fc):
    """Segment lengths 1, 63, 64, 65, 128, 129, 1000 (one, two, three and sixteen trips of reduce_ragged_kernel's 64-lane loop, full and ragged),
    a repeated index and a decreasing pair; all four ops; 1-D, and 3 x 5000 along both axes; zeros under divide."""
    rng = np.random.default_rng(fc.order % 1031)
    F, n = fc.F, 5000
    idx = np.array([0, 1, 64, 128, 193, 321, 450, 1450, 1450, 3000, 2000, 4000])
    ends = np.r_[idx[1:], n]
    assert [int(e - s) for s, e in zip(idx, ends)][:7] == [1, 63, 64, 65, 128, 129, 1000] and (np.diff(idx) == 0).any() and (np.diff(idx) < 0).any()
    with fc.compiled():
        for shape, axis, ix in (((n,), 0, idx), ((3, n), 1, idx), ((3, n), 0, np.array([0, 2, 1, 1]))):
            any_value, nonzero = fc.rnd(rng, shape, 0), fc.rnd(rng, shape, 1)
            any_value.flat[70] = 0  # a zero under add / subtract / multiply
            for op, uf in UFUNCS.items():
                a = nonzero if op == "divide" else any_value
                moved = np.moveaxis(a, axis, -1)
                want = left_fold(F, op, moved, ix, np.r_[ix[1:], moved.shape[-1]])
                got = uf.reduceat(fc.mk(a), ix, axis=axis)
                assert type(got) is fc.GF and got.shape == tuple(len(ix) if d == axis else s for d, s in enumerate(shape))
                got = np.moveaxis(host(got), axis, -1)
                assert np.array_equal(got, want), (fc.id, op, shape, axis, np.argwhere(got != want)[:4].tolist())
        if fc.order > 2:
            # divide: a zero that leads a segment gives 0 and raises nothing; a zero further in raises
            base = fc.rnd(rng, (n,), 1)
            z = base.copy()
            z[[0, 64, 1450]] = 0  # first elements of segments (index 1450 twice: an empty slice and a long segment)
            got = host(np.true_divide.reduceat(fc.mk(z), idx))
            lead = np.isin(idx, [0, 64, 1450])
            assert not got[lead].any() and np.array_equal(got[~lead], left_fold(F, "divide", base, idx, ends)[~lead])
            for j in (65, 127, 1449, n - 1):
                z = base.copy()
                z[j] = 0
                with pytest.raises(ZeroDivisionError):
                    np.true_divide.reduceat(fc.mk(z), idx)


# ---- the C entry points ----------------------------------------------------------------------------------------------------------
def test_c_entry_points_on_several_segmented_rows():
    """gfa_reduce / gfa_accumulate on a 3 x 70 001 row-major buffer, called as a C host would: segments with n_outer > 1 without the front end."""
    fc = FieldCase(65521, "uint16")
    GF, F, lib = fc.GF, fc.F, L.lib()
    rng = np.random.default_rng(70)
    rows, n = 3, 70_001
    st = torch.cuda.current_stream().cuda_stream
    for op, code, low in (("add", L.OP_ADD, 0), ("subtract", L.OP_SUB, 0), ("multiply", L.OP_MUL, 1), ("divide", L.OP_DIV, 1)):
        assert route(fc, "reduce", op, rows, n).nseg > 8 and route(fc, "accumulate", op, rows, n, (8, "carries"))
        a = fc.rnd(rng, (rows, n), low)
        dev = torch.from_numpy(a.astype(np.uint16).view(np.int16)).cuda()
        red, scan = torch.full((rows,), -1, dtype=torch.int16, device="cuda"), torch.empty_like(dev)
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        L.check(lib.gfa_reduce(GF._handle, code, dev.data_ptr(), red.data_ptr(), rows, n, L.U16, st, err.data_ptr()))
        L.check(lib.gfa_accumulate(GF._handle, code, dev.data_ptr(), scan.data_ptr(), rows, n, L.U16, st, err.data_ptr()))
        torch.cuda.synchronize()
        assert int(err.item()) == 0
        assert np.array_equal(red.cpu().numpy().view(np.uint16).astype(np.uint64), expected_reduce(F, op, a)), op
        check_scan(F, op, a, scan.cpu().numpy().view(np.uint16).astype(np.uint64), op)


def test_c_entry_points_argument_contract():
    """The return codes the entry points document: no rows is OK and writes nothing; an empty row is invalid for gfa_reduce and OK for
    gfa_accumulate; a dtype too narrow for the field is invalid; more rows than a launch grid can express is invalid (before anything is read)."""
    lib = L.lib()
    GF = ga.GF(65521)
    st = torch.cuda.current_stream().cuda_stream
    dev = torch.arange(1, 13, dtype=torch.int16, device="cuda")
    out = torch.full((12,), 77, dtype=torch.int16, device="cuda")
    for fn in (lib.gfa_reduce, lib.gfa_accumulate):
        assert fn(GF._handle, L.OP_ADD, dev.data_ptr(), out.data_ptr(), 0, 4, L.U16, st, None) == L.OK
        assert fn(GF._handle, L.OP_ADD, dev.data_ptr(), out.data_ptr(), 3, 4, L.U8, st, None) == L.ERR_INVALID  # 65521 does not fit a byte
        assert fn(GF._handle, L.OP_ADD, dev.data_ptr(), out.data_ptr(), 2**31, 1, L.U16, st, None) == L.ERR_INVALID
        assert fn(GF._handle, L.OP_ADD, dev.data_ptr(), out.data_ptr(), 2**32 + 3, 1, L.U16, st, None) == L.ERR_INVALID
        assert fn(GF._handle, L.OP_ADD, dev.data_ptr(), out.data_ptr(), -1, 4, L.U16, st, None) == L.ERR_INVALID
        assert fn(GF._handle, 7, dev.data_ptr(), out.data_ptr(), 3, 4, L.U16, st, None) == L.ERR_INVALID
    assert lib.gfa_reduce(GF._handle, L.OP_ADD, dev.data_ptr(), out.data_ptr(), 3, 0, L.U16, st, None) == L.ERR_INVALID
    assert lib.gfa_accumulate(GF._handle, L.OP_ADD, dev.data_ptr(), out.data_ptr(), 3, 0, L.U16, st, None) == L.OK
    # nothing to read or write: the buffers may be null (an empty device array has no address), and only then
    assert lib.gfa_reduce(GF._handle, L.OP_ADD, None, None, 0, 4, L.U16, st, None) == L.OK
    assert lib.gfa_accumulate(GF._handle, L.OP_ADD, None, None, 0, 4, L.U16, st, None) == L.OK
    assert lib.gfa_accumulate(GF._handle, L.OP_ADD, None, None, 3, 0, L.U16, st, None) == L.OK
    assert lib.gfa_reduce(GF._handle, L.OP_ADD, None, out.data_ptr(), 3, 4, L.U16, st, None) == L.ERR_INVALID
    assert lib.gfa_reduce(GF._handle, L.OP_ADD, dev.data_ptr(), None, 3, 4, L.U16, st, None) == L.ERR_INVALID
    assert lib.gfa_accumulate(GF._handle, L.OP_ADD, None, out.data_ptr(), 3, 4, L.U16, st, None) == L.ERR_INVALID
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [77] * 12  # none of the calls above wrote
    assert lib.gfa_reduce(GF._handle, L.OP_ADD, dev.data_ptr(), out.data_ptr(), 3, 4, L.U16, st, None) == L.OK
    torch.cuda.synchronize()
    assert out.cpu().tolist()[:4] == [10, 26, 42, 77]


# ---- the list is closed ----------------------------------------------------------------------------------------------------------
FORMS = ([f"stream 0 at {w} bytes" for w in (1, 2, 4, 8)] + [f"stream 1 at {w} bytes" for w in (1, 2, 4)] + ["stream 2", "stream 3", "generic add", "generic multiply"])
JOINS = ["one segment", "thread join, several rows", "block join, several rows", "carries c=1", "carries c>=2"]
# (form, join) -> why the planner cannot produce it.  Empty: every first-phase form meets every join; the streaming forms are chosen by field,
# width and op alone (their segment-length guards, 2^32 and 2^40 elements, lie far above any shape here), the joins by shape alone.
UNREACHED = {}


def test_every_route_is_visited():
    """The routes of REDUCE_SHAPES and SCAN_SHAPES over FIELD_CASES and of the long scan over LONG_SCAN_CASES -- the very tables that
    test_reduce_on_every_segment_route, test_accumulate_on_every_segment_route and test_accumulate_of_one_row_in_more_than_256_segments
    run and assert -- planned once more for the device at hand: their union is {first-phase form} x {join}."""
    seen = set()
    def visit(fc, kind, op, rows, n):
        pl = route(fc, kind, op, rows, n)
        seen.add((form_name(pl, fc, op), join_class(pl)))
    for fc in FIELD_CASES:
        with fc.compiled():
            for op in UFUNCS:
                for rows, n, _ in REDUCE_SHAPES:
                    visit(fc, "reduce", op, rows, n)
                for rows, n, _ in SCAN_SHAPES:
                    visit(fc, "accumulate", op, rows, n)
    for fc in LONG_SCAN_CASES:
        with fc.compiled():
            for op in UFUNCS:
                visit(fc, "accumulate", op, 1, long_scan_length(fc))
    missing = [(f, j) for f in FORMS for j in JOINS if (f, j) not in seen and (f, j) not in UNREACHED]
    assert not missing, missing
    assert not [k for k in UNREACHED if k in seen], "a route listed as unreached is reached"
