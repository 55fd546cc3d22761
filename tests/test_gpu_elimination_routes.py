"""Row reduction and PLU on every kernel route and every pass of their loops (csrc/gfa_linalg.hip: row_reduce_kernel, gj_pivot_kernel +
gj_eliminate_kernel, plu_kernel; csrc/gfa_wide.hip: wide_row_reduce_kernel, wide_plu_kernel).

tests/test_gpu_linalg.py compares these kernels with the oracle in two size bands (up to 33 rows, and 365 rows and more on the
two-kernels-per-column route).  The cases here sit between and on the thresholds, at the smallest shapes at which each path can go wrong:
more rows or columns than the 256 threads of the one-workgroup kernels (second pass of every strided loop, first hit of the pivot search in a
later pass, LDS factors beyond entry 256), both sides of m n = 131072, of 32 / 33 matrices and of 4096 / 4097 rows, per-matrix pivot state
on the two-kernel route, stacks longer than the 65535 slices of gfa_matmul, and the two-limb kernels at 300 rows.  The route of every shape is
asserted from tests/elim_plan.py (the mirror of csrc/gfa_elim_plan.h, kept honest by tests/test_elim_plan_host.py) before anything is
launched.  Every comparison is bit-exact against oracle/gf_oracle.py (two-limb fields: the scalar rules of tests/test_gpu_limb_edges.py on
oracle/wide_oracle.py), including the pivot order of P, L and U; the conditions an input must meet to reach its path (pivot offsets, ranks,
pivot columns) are computed from the oracle alone and asserted, so that a weak input fails instead of passing.  Seeds are fixed; oracle
results are computed once per field and shared."""
import zlib

import numpy as np
import pytest

import galois_amd as ga
from tests import elim_plan as EP
from tests import helpers as H
from tests import test_gpu_limb_edges as LE
from tests.test_gpu_linalg import _FIELDS, _pair, _rand

pytestmark = pytest.mark.gpu

TAGS = [f[0] for f in _FIELDS]
WIDEST = ["gf256", "gf31", "gf3e5"]  # also run in the widest storage type where the issue asks (S3, P1)
STORAGE = [(t, False) for t in TAGS] + [(t, True) for t in WIDEST]
STORAGE_IDS = [t + ("-widest" if w else "") for t, w in STORAGE]

_CACHE = {}


def _memo(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _ctx(tag):
    return _memo(("ctx", tag), lambda: _pair(tag))


def _rng(tag, salt):
    return np.random.default_rng(zlib.crc32(f"{tag}/{salt}".encode()))


def _frozen(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    a.setflags(write=False)
    return a


def _up(GF, A, widest=False):
    """Narrowest storage type of the field (what GF(x) picks), or its widest."""
    if widest:
        dt = GF.dtypes[-1]
        assert np.dtype(dt).itemsize > np.dtype(GF.dtypes[0]).itemsize
        return GF(np.asarray(A).astype(dt), dtype=dt)
    return GF(np.asarray(A))


def _rank7(F, rng, q, m, n):
    """Product of m x 7 and 7 x n factors, with row 5 zeroed."""
    A = np.array(F.matmul(_rand(rng, q, (m, 7)), _rand(rng, q, (7, n))), dtype=np.uint64)
    A[5] = 0
    return A


def _lu_factors(rng, q, n):
    """Unit lower L0 and upper U0 with a non-zero diagonal."""
    L0 = np.tril(_rand(rng, q, (n, n)), -1) + np.eye(n, dtype=np.uint64)
    U0 = np.triu(_rand(rng, q, (n, n)), 1)
    d = _rand(rng, q, n)
    d[d == 0] = 1
    U0[np.arange(n), np.arange(n)] = d
    return L0, U0


def _mat(tag, name):
    """The inputs, by name: built once per field from a seed of their own, read-only."""
    def make():
        GF, F = _ctx(tag)
        q = GF.order
        rng = _rng(tag, name)
        if name == "late300x40":  # rows 0..279 zero in columns 0..19: the first pivots are found 261 rows and more below the pivot row
            A = _rand(rng, q, (300, 40))
            A[:280, :20] = 0
        elif name in ("r40x300", "r300x300", "r257x510", "r256x520", "r420x8", "r255b", "r256b"):
            shape = {"r40x300": (40, 300), "r300x300": (300, 300), "r257x510": (257, 510), "r256x520": (256, 520), "r420x8": (420, 8),
                     "r255b": (255, 3), "r256b": (256, 3)}[name]
            A = _rand(rng, q, shape)
        elif name == "r40x300_swap":  # the first two entries of column 0 zero: an exchange at step 0
            A = _mat(tag, "r40x300").copy()
            A[0, 0] = A[1, 0] = 0
        elif name == "rank7_300x300":
            A = _rank7(F, rng, q, 300, 300)
        elif name == "M0":
            A = _rand(rng, q, (257, 511))
        elif name == "M1":
            A = _rand(rng, q, (257, 511))
            A[:, 3] = 0
        elif name == "M2":
            A = _rank7(F, rng, q, 257, 511)
        elif name == "M3":
            A = np.zeros((257, 511), dtype=np.uint64)
        elif name == "M4":
            A = _mat(tag, "M0")[::-1].copy()
        elif name in ("tall4096x8", "tall4097x8", "tall4097x32", "tall4096x4"):  # column 0 non-zero only in the last row
            m, n = (int(v) for v in name[4:].split("x"))
            A = _rand(rng, q, (m, n))
            A[:, 0] = 0
            A[m - 1, 0] = 1 + int(rng.integers(0, min(q, 2**62) - 1))
        elif name in ("inv255", "inv256"):  # a random matrix the oracle can invert; over GF(2) most random matrices are singular: then P L0 U0
            n = int(name[3:])
            A = _rand(rng, q, (n, n))
            if F.row_reduce(A)[1] != n:
                L0, U0 = _lu_factors(rng, q, n)
                A = np.array(F.matmul(L0, U0), dtype=np.uint64)[rng.permutation(n)]
        elif name == "singular255":  # row 200 = row 3 + row 7
            A = _rand(rng, q, (255, 255))
            A[200] = F.add(A[3], A[7])
        elif name in ("L0", "U0"):
            L0, U0 = _lu_factors(rng, q, 300)
            _CACHE[(tag, "L0")], _CACHE[(tag, "U0")] = _frozen(L0), _frozen(U0)
            return _CACHE[(tag, name)]
        elif name == "lu300":
            A = F.matmul(_mat(tag, "L0"), _mat(tag, "U0"))
        elif name == "L0b":  # L0 with L0[271, 270] = 0
            A = _mat(tag, "L0").copy()
            A[271, 270] = 0
        elif name == "lu300_exchanged":  # L0b U0 with rows 270 and 271 exchanged
            A = np.array(F.matmul(_mat(tag, "L0b"), _mat(tag, "U0")), dtype=np.uint64)
            A[[270, 271]] = A[[271, 270]]
        else:
            raise KeyError(name)
        return _frozen(A)
    return _memo((tag, name), make)


def _rre(tag, name, ncols=None):
    """(reduced form, pivot count) of a named input, from the oracle."""
    return _memo((tag, name, "rre", ncols), lambda: _ctx(tag)[1].row_reduce(_mat(tag, name), ncols=ncols))


def _plu(tag, name):
    return _memo((tag, name, "plu"), lambda: _ctx(tag)[1].plu_decompose(_mat(tag, name)))


def _pivot_columns(rre):
    """Pivot columns of a reduced row echelon form: the first non-zero column of each non-zero row."""
    return [int(np.flatnonzero(r)[0]) for r in rre if r.any()]


def _pivot_offsets(F, A):
    """The oracle's row_reduce (gf_oracle.OracleField.row_reduce, line for line) with its pivot search instrumented: returns the reduced
    form, the pivot count and (column, i - p) for every pivot, i the row the search found and p the pivot row."""
    A = np.array(A, dtype=np.uint64)
    m, n = A.shape
    p, found = 0, []
    for j in range(n):
        idxs = np.nonzero(A[p:, j])[0]
        if idxs.size == 0:
            continue
        i = p + int(idxs[0])
        found.append((j, i - p))
        A[[p, i], :] = A[[i, p], :]
        A[p, :] = F.div(A[p, :], np.full(n, A[p, j], dtype=np.uint64))
        idxs = [int(r) for r in np.nonzero(A[:, j])[0] if r != p]
        F._outer_sub(A, idxs, A[idxs, j].copy(), A[p, :].copy())
        p += 1
        if p == m:
            break
    return A, p, found


def _late(tag):
    """The late-pivot input with its condition checked on the oracle: at least 10 pivots found 256 rows or more below the pivot row."""
    def make():
        GF, F = _ctx(tag)
        A = _mat(tag, "late300x40")
        rre, rank, found = _pivot_offsets(F, A)
        want, want_rank = _rre(tag, "late300x40")
        assert np.array_equal(rre, want) and rank == want_rank, "the instrumented copy is the oracle's elimination"
        late = [j for j, off in found if off >= EP.GJ_THREADS]
        print(f"{tag}: late-pivot 300 x 40: rank {rank}, {len(late)} pivots at a row offset >= {EP.GJ_THREADS} (columns {late})")
        assert len(late) >= 10, (tag, found)
        return A, want, rank, late
    return _memo((tag, "late"), make)


def _oracle_det(F, plu):
    """OracleField.det on a PLU it has already computed: (-1)^N_perm prod(diag L) prod(diag U)."""
    _, L, U, nperm = plu
    d = 1
    for i in range(U.shape[0]):
        d = int(F.mul([d], [int(L[i, i])])[0])
        d = int(F.mul([d], [int(U[i, i])])[0])
    return int(F.neg([d])[0]) if nperm % 2 else d


def _check_plu(tag, name, widest=False, product=True):
    GF, F = _ctx(tag)
    A = _mat(tag, name)
    assert EP.plu_supported(*A.shape)
    P, L, U, nperm = _plu(tag, name)
    gA = _up(GF, A, widest)
    p, l, u = gA.plu_decompose()
    H.assert_equal_ints(p.numpy(), P, f"{tag} {name} P")
    H.assert_equal_ints(l.numpy(), L, f"{tag} {name} L")
    H.assert_equal_ints(u.numpy(), U, f"{tag} {name} U")
    if product:
        H.assert_equal_ints((p @ l @ u).numpy(), A, f"{tag} {name} P @ L @ U")
    return gA, (P, L, U, nperm)


# ---- row reduction, one workgroup per matrix -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_S1_late_pivots_second_pass_of_the_pivot_search(tag):
    """Late-pivot 300 x 40: each of the first pivots is the first hit of a thread's SECOND pass (row offset >= 256), and the LDS factors
    beyond entry 256 are the only non-zero ones of those columns."""
    GF, F = _ctx(tag)
    A, want, rank, _ = _late(tag)
    assert EP.elim_route(1, *A.shape) == EP.ONE_WORKGROUP
    gA = GF(A)
    H.assert_equal_ints(gA.row_reduce().numpy(), want, f"{tag} late-pivot row_reduce")
    assert np.linalg.matrix_rank(gA) == rank == F.matrix_rank(A)


@pytest.mark.parametrize("tag", TAGS)
def test_S2_wide_rows_second_pass_of_the_swap_and_scale_loop(tag):
    """40 x 300: the swap / scale loop over the columns runs two passes; the update's column tile shrinks from 256 to 1 as n - j does."""
    GF, F = _ctx(tag)
    A = _mat(tag, "r40x300")
    want, rank = _rre(tag, "r40x300")
    assert EP.elim_route(1, *A.shape) == EP.ONE_WORKGROUP
    gA = GF(A)
    H.assert_equal_ints(gA.row_reduce().numpy(), want, f"{tag} 40 x 300 row_reduce")
    assert np.linalg.matrix_rank(gA) == rank


@pytest.mark.parametrize("op", ["row_reduce", "column_space", "left_null_space", "null_space"])
@pytest.mark.parametrize("kind", ["r300x300", "rank7_300x300"])
@pytest.mark.parametrize("tag,widest", STORAGE, ids=STORAGE_IDS)
def test_S3_300_by_300(tag, widest, kind, op):
    """300 x 300, random and of rank 7: more rows AND more columns than threads.  row_reduce / matrix_rank / row_space share one oracle
    reduction; the other subspaces are a case each (their oracle reductions are the slow part)."""
    GF, F = _ctx(tag)
    A = _mat(tag, kind)
    assert EP.elim_route(1, 300, 300) == EP.ONE_WORKGROUP  # A and A.T
    if op.endswith("null_space"):  # [A | I] is 300 x 600 and past the threshold; the block below its pivots is reduced by one workgroup again
        rank = _rre(tag, kind)[1]
        assert EP.elim_route(1, 300, 600) == EP.TWO_KERNELS and (rank == 300 or EP.elim_route(1, 300 - rank, 300) == EP.ONE_WORKGROUP)
    gA = _up(GF, A, widest)
    if op == "row_reduce":
        want, rank = _rre(tag, kind)
        if kind == "rank7_300x300":
            assert rank == 7, (tag, rank)
        H.assert_equal_ints(gA.row_reduce().numpy(), want, f"{tag} {kind} row_reduce")
        assert np.linalg.matrix_rank(gA) == rank == F.matrix_rank(A)
        H.assert_equal_ints(gA.row_space().numpy(), want[:rank], f"{tag} {kind} row_space")
        return
    want = _memo((tag, kind, op), lambda: getattr(F, op)(A))
    got = getattr(gA, op)().numpy()
    if kind == "rank7_300x300":
        assert want.shape == ((7, 300) if op == "column_space" else (293, 300))
    assert got.shape == want.shape or (got.size == 0 and want.size == 0), (op, got.shape, want.shape)
    if want.size:
        H.assert_equal_ints(got, want, f"{tag} {kind} {op}")


@pytest.mark.parametrize("name,route", [("r257x510", EP.ONE_WORKGROUP), ("M0", EP.TWO_KERNELS)])
@pytest.mark.parametrize("tag", TAGS)
def test_S4_both_sides_of_131072_elements(tag, name, route):
    """257 x 510 (131070 elements) and 257 x 511 (131327): the last shape of one route and the first of the other."""
    GF, F = _ctx(tag)
    A = _mat(tag, name)
    want, rank = _rre(tag, name)
    assert EP.elim_route(1, *A.shape) == route
    gA = GF(A)
    H.assert_equal_ints(gA.row_reduce().numpy(), want, f"{tag} {A.shape} row_reduce")
    assert np.linalg.matrix_rank(gA) == rank


def _stack33(tag):
    """The mixed stack M0..M4, then 28 copies of M0 with one entry changed each."""
    def make():
        GF, F = _ctx(tag)
        q = GF.order
        rng = _rng(tag, "stack33")
        M0 = _mat(tag, "M0")
        S = np.stack([_mat(tag, f"M{k}") for k in range(5)] + [M0] * 28)
        for k in range(5, 33):
            r, c = int(rng.integers(0, 257)), int(rng.integers(0, 511))
            S[k, r, c] = (int(S[k, r, c]) + 1 + int(rng.integers(0, min(q, 2**62) - 1))) % q
            assert S[k, r, c] != M0[r, c]
        return _frozen(S)
    return _memo((tag, "stack33"), make)


@pytest.mark.parametrize("tag", TAGS)
def test_S5_batch_cap_32_and_33_matrices_agree(tag):
    """33 matrices of 257 x 511 take one workgroup each, the first 32 of them the two-kernel route: the two routes agree matrix by
    matrix."""
    GF, F = _ctx(tag)
    S = _stack33(tag)
    assert EP.elim_route(33, 257, 511) == EP.ONE_WORKGROUP and EP.elim_route(32, 257, 511) == EP.TWO_KERNELS
    r33, ranks33 = ga.linalg.row_reduce_batched(GF(S))
    r32, ranks32 = ga.linalg.row_reduce_batched(GF(S[:32]))
    assert list(ranks33[:32]) == list(ranks32)
    diff = (r33._t[:32] != r32._t).reshape(32, -1).any(dim=1).nonzero().flatten().tolist()
    assert not diff, f"{tag}: the routes differ on matrices {diff}"


@pytest.mark.parametrize("k", [0, 1, 2, 3, 4, 32])
@pytest.mark.parametrize("tag", TAGS)
def test_S5_one_workgroup_each_of_33_against_the_oracle(tag, k):
    """M0..M4 and the last matrix of the stack of 33 (one case each: an oracle reduction of 257 x 511 is the slow part)."""
    GF, F = _ctx(tag)
    S = _stack33(tag)
    assert EP.elim_route(33, 257, 511) == EP.ONE_WORKGROUP
    want, rank = _rre(tag, f"M{k}") if k < 5 else _memo((tag, "stack33 last"), lambda: F.row_reduce(S[32]))
    r33, ranks33 = ga.linalg.row_reduce_batched(GF(S))
    H.assert_equal_ints(r33[k].numpy(), want, f"{tag} matrix {k} of 33")
    assert int(ranks33[k]) == rank


@pytest.mark.parametrize("name,route", [("tall4096x8", EP.ONE_WORKGROUP), ("tall4097x8", EP.TWO_KERNELS), ("tall4097x32", EP.TWO_KERNELS)])
@pytest.mark.parametrize("tag", TAGS)
def test_S6_row_limit_of_the_lds_factors_pivot_in_the_last_row(tag, name, route):
    """4096 x 8 fills the LDS factor array of the one-workgroup kernel; 4097 rows go to the two-kernel route whatever the size (its factors
    are in global memory), 4097 x 8 below 131072 elements and 4097 x 32 above.  Column 0 is non-zero only in the last row: the last pass of
    the pivot search (the fifth of gj_pivot_kernel's 1024 threads) finds it."""
    GF, F = _ctx(tag)
    A = _mat(tag, name)
    m, n = A.shape
    assert EP.elim_route(1, m, n) == route
    assert not A[:-1, 0].any() and A[-1, 0] != 0
    assert (m - 1) // (EP.GJ_THREADS if route == EP.ONE_WORKGROUP else EP.WIDE_PIVOT_THREADS) == (15 if m == 4096 else 4)
    want, rank = _rre(tag, name)
    got = GF(A).row_reduce()
    H.assert_equal_ints(got.numpy(), want, f"{tag} {m} x {n} row_reduce")


def test_S6_refusals_past_the_row_limits():
    """More than 32 matrices of more than 4096 rows have no route; neither has a matrix of more rows than the two-kernel grid holds.  Both
    are refused on the host, before any launch."""
    GF, _ = _ctx("gf256")
    assert EP.elim_route(33, 4097, 8) == EP.UNSUPPORTED and EP.elim_route(33, 4096, 8) == EP.ONE_WORKGROUP
    with pytest.raises(NotImplementedError):
        ga.linalg.row_reduce_batched(GF(np.ones((33, 4097, 8), dtype=np.uint8)))
    assert EP.elim_route(1, EP.GJ_WIDE_MAX_ROWS + 1, 1) == EP.UNSUPPORTED
    with pytest.raises(NotImplementedError):
        GF(np.ones((EP.GJ_WIDE_MAX_ROWS + 1, 1), dtype=np.uint8)).row_reduce()


@pytest.mark.parametrize("n,route", [(255, EP.ONE_WORKGROUP), (256, EP.TWO_KERNELS)])
@pytest.mark.parametrize("tag", TAGS)
def test_S7_inverse_and_solve_across_the_route_boundary(tag, n, route):
    """[A | I] is n x 2n: 255 x 510 is the largest inverse of the one-workgroup kernel, 256 x 512 the smallest of the two-kernel route.
    solve is inv(A) @ b in the reference, and so it is in the oracle."""
    GF, F = _ctx(tag)
    A, b = _mat(tag, f"inv{n}"), _mat(tag, f"r{n}b")
    assert EP.elim_route(1, n, 2 * n) == route
    want = _memo((tag, n, "inv"), lambda: F.inv(A))
    gA = GF(A)
    Ai = np.linalg.inv(gA)
    H.assert_equal_ints(Ai.numpy(), want, f"{tag} inverse, n = {n}")
    H.assert_equal_ints((gA @ Ai).numpy(), np.eye(n, dtype=np.uint64), f"{tag} A @ inv(A), n = {n}")
    H.assert_equal_ints(np.linalg.solve(gA, GF(b)).numpy(), F.matmul(want, b), f"{tag} solve, 2-D right-hand side")
    H.assert_equal_ints(np.linalg.solve(gA, GF(b[:, 0])).numpy(), F.matmul(want, b[:, :1])[:, 0], f"{tag} solve, 1-D right-hand side")


@pytest.mark.parametrize("tag", TAGS)
def test_S7_singular_255_by_255(tag):
    GF, F = _ctx(tag)
    A = _mat(tag, "singular255")
    assert EP.elim_route(1, 255, 510) == EP.ONE_WORKGROUP
    with pytest.raises(np.linalg.LinAlgError):
        F.inv(A)
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.inv(GF(A))
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.solve(GF(A), GF(_mat(tag, "r255b")))


# ---- row reduction, two kernels per column ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_W1_mixed_stack_per_matrix_pivot_state(tag):
    """M0 (random), M1 (column 3 zero), M2 (rank 7), M3 (zero), M4 (M0 with its rows reversed) as one batch on the two-kernel route: in
    most columns some matrices have a pivot and others have none, and their pivot rows differ."""
    GF, F = _ctx(tag)
    mats = [_mat(tag, f"M{k}") for k in range(5)]
    want = [_rre(tag, f"M{k}") for k in range(5)]
    assert EP.elim_route(5, 257, 511) == EP.TWO_KERNELS
    ranks = [r for _, r in want]
    assert len(set(ranks)) >= 3 and ranks[2] == 7 and ranks[3] == 0, (tag, ranks)
    only_m0 = sorted(set(_pivot_columns(want[0][0])) - set(_pivot_columns(want[1][0])))
    print(f"{tag}: mixed stack ranks {ranks}; columns with a pivot in M0 and none in M1: {only_m0[:8]}")
    assert 3 in only_m0, (tag, only_m0)
    got, got_ranks = ga.linalg.row_reduce_batched(GF(np.stack(mats)))
    assert list(got_ranks) == ranks, (tag, list(got_ranks), ranks)
    for k in range(5):
        H.assert_equal_ints(got[k].numpy(), want[k][0], f"{tag} M{k} of the mixed stack")


@pytest.mark.parametrize("tag", TAGS)
def test_W2_full_row_rank_before_the_last_column(tag):
    """256 x 520 of full row rank: the pivot row count reaches m columns before the end, and the remaining columns find no pivot."""
    GF, F = _ctx(tag)
    A = _mat(tag, "r256x520")
    want, rank = _rre(tag, "r256x520")
    assert EP.elim_route(1, 256, 520) == EP.TWO_KERNELS
    assert rank == 256 and _pivot_columns(want)[-1] < 519, (tag, rank)
    gA = GF(A)
    H.assert_equal_ints(gA.row_reduce().numpy(), want, f"{tag} 256 x 520 row_reduce")
    assert np.linalg.matrix_rank(gA) == 256


@pytest.mark.parametrize("form", ["ncols=100", "eye=right"])
@pytest.mark.parametrize("tag", TAGS)
def test_W3_reduced_column_range_and_flipped_form(tag, form):
    GF, F = _ctx(tag)
    A = _mat(tag, "M0")
    assert EP.elim_route(1, 257, 511) == EP.TWO_KERNELS
    if form == "ncols=100":
        want, _ = _rre(tag, "M0", ncols=100)
        H.assert_equal_ints(GF(A).row_reduce(ncols=100).numpy(), want, f"{tag} ncols=100")
    else:
        want = _memo((tag, "M0 flipped"), lambda: F.row_reduce(A[::-1, ::-1])[0][::-1, ::-1])
        H.assert_equal_ints(GF(A).row_reduce(eye="right").numpy(), want, f"{tag} eye='right'")


@pytest.mark.parametrize("tag", TAGS)
def test_W4_null_spaces_of_a_tall_matrix(tag):
    """left_null_space of 420 x 8 reduces the augmented 420 x 428 over 8 columns, then the (420 - rank) x 420 block below: both on the
    two-kernel route.  null_space of the transpose is the same computation behind a transposition."""
    GF, F = _ctx(tag)
    A = _mat(tag, "r420x8")
    want = _memo((tag, "r420x8", "lns"), lambda: F.left_null_space(A))
    rank = 420 - want.shape[0]
    assert EP.elim_route(1, 420, 428) == EP.TWO_KERNELS and EP.elim_route(1, 420 - rank, 420) == EP.TWO_KERNELS and 1 <= rank <= 8
    H.assert_equal_ints(GF(A).left_null_space().numpy(), want, f"{tag} left_null_space of 420 x 8")
    H.assert_equal_ints(GF(np.ascontiguousarray(A.T)).null_space().numpy(), want, f"{tag} null_space of 8 x 420")


# ---- PLU / LU / det (plu_kernel) -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,widest", STORAGE, ids=STORAGE_IDS)
def test_P1_plu_and_det_of_300_by_300(tag, widest):
    GF, F = _ctx(tag)
    gA, plu = _check_plu(tag, "r300x300", widest)
    assert int(np.linalg.det(gA)) == _oracle_det(F, plu)


@pytest.mark.parametrize("tag", TAGS)
def test_P2_plu_of_the_late_pivot_matrix(tag):
    """m > n, and every exchange of the first columns swaps rows of L and P whose non-zero entries sit at columns >= 256 (P's ones at
    columns 280 and up): the second pass of the L / P swap loop."""
    GF, F = _ctx(tag)
    _, _, _, late = _late(tag)
    _, (P, L, U, nperm) = _check_plu(tag, "late300x40")
    moved = [int(c) for c in np.flatnonzero(P[np.arange(300), np.arange(300)] == 0)]
    assert nperm >= 10 and len(late) >= 10 and max(moved) >= 280, (tag, nperm, moved)


@pytest.mark.parametrize("tag", TAGS)
def test_P3_plu_of_40_by_300(tag):
    """A forced exchange at step 0 (the first two entries of column 0 are zero): the row swap over 300 columns runs two passes."""
    _, (P, L, U, nperm) = _check_plu(tag, "r40x300_swap")
    A = _mat(tag, "r40x300_swap")
    assert A[0, 0] == 0 and A[1, 0] == 0
    if A[2:, 0].any():
        assert nperm >= 1 and P[0, 0] == 0


@pytest.mark.parametrize("tag", TAGS)
def test_P4a_lu_returns_the_factors_it_was_built_from(tag):
    """A = L0 @ U0 (unit lower, upper with a non-zero diagonal): all m - 1 = 299 steps of the LU run, and the factorisation is unique."""
    GF, F = _ctx(tag)
    L0, U0, A = _mat(tag, "L0"), _mat(tag, "U0"), _mat(tag, "lu300")
    assert EP.plu_supported(300, 300) and U0[np.arange(300), np.arange(300)].all() and not np.triu(L0, 1).any()
    Lw, Uw = _memo((tag, "lu300", "lu"), lambda: F.lu_decompose(A))
    assert np.array_equal(Lw, L0) and np.array_equal(Uw, U0), "the oracle recovers the factors"
    lg, ug = GF(A).lu_decompose()
    H.assert_equal_ints(lg.numpy(), L0, f"{tag} L of L0 @ U0")
    H.assert_equal_ints(ug.numpy(), U0, f"{tag} U of L0 @ U0")


@pytest.mark.parametrize("tag", TAGS)
def test_P4b_lu_fails_at_step_270(tag):
    """L0[271, 270] = 0 and rows 270 and 271 of the product exchanged: steps 0..269 succeed, step 270 meets a zero pivot with a non-zero
    entry below it."""
    GF, F = _ctx(tag)
    A = _mat(tag, "lu300_exchanged")
    with pytest.raises(ValueError):
        F.lu_decompose(A)
    with pytest.raises(ValueError):
        GF(A).lu_decompose()


@pytest.mark.parametrize("tag", TAGS)
def test_P4b_plu_needs_exactly_one_exchange(tag):
    """The same matrix: plu_decompose exchanges exactly rows 270 and 271 and finds L0 (with L0[271, 270] = 0) and U0 again;
    det = -prod(diag U0)."""
    GF, F = _ctx(tag)
    U0 = _mat(tag, "U0")
    gA, (P, L, U, nperm) = _check_plu(tag, "lu300_exchanged")
    swap = np.eye(300, dtype=np.uint64)
    swap[[270, 271]] = swap[[271, 270]]
    assert nperm == 1 and np.array_equal(P, swap) and np.array_equal(U, U0) and np.array_equal(L, _mat(tag, "L0b"))
    d = 1
    for v in U0[np.arange(300), np.arange(300)]:
        d = int(F.mul([d], [int(v)])[0])
    assert int(np.linalg.det(gA)) == int(F.neg([d])[0]) == _oracle_det(F, (P, L, U, nperm))


@pytest.mark.parametrize("tag", TAGS)
def test_P5_plu_of_the_rank_7_matrix(tag):
    """Pivot-free steps from step 7 on (row 5 is zero: one before, too): L[i, i] = 1 without an elimination, det = 0."""
    GF, F = _ctx(tag)
    assert _rre(tag, "rank7_300x300")[1] == 7
    gA, (P, L, U, nperm) = _check_plu(tag, "rank7_300x300")
    assert np.count_nonzero(U[np.arange(300), np.arange(300)]) <= 7 and L[np.arange(300), np.arange(300)].all()
    assert int(np.linalg.det(gA)) == 0 == _oracle_det(F, (P, L, U, nperm))


@pytest.mark.parametrize("tag", ["gf256", "gf65537"])
def test_P6_plu_at_the_row_limit(tag):
    """4096 x 4 with the first pivot in the last row: L and P are 4096 x 4096, their rows 0 and 4095 are exchanged over 16 passes."""
    GF, F = _ctx(tag)
    assert EP.plu_supported(4096, 4) and not EP.plu_supported(4097, 4)
    _, (P, L, U, nperm) = _check_plu(tag, "tall4096x4", product=False)
    assert P[4095, 0] == 1 and nperm >= 1
    with pytest.raises(NotImplementedError):
        GF(np.ones((4097, 4), dtype=np.uint64)).plu_decompose()


# ---- stacks longer than a 65535 slice ---------------------------------------------------------------------------------------------------
N_STACK = 65539


def _col(S, r, c):
    return np.ascontiguousarray(S[:, r, c])


def _minor2(F, S, r0, r1, c0, c1):
    return F.sub(F.mul(_col(S, r0, c0), _col(S, r1, c1)), F.mul(_col(S, r0, c1), _col(S, r1, c0)))


def _det3(F, S):
    """Determinants of a stack of 3 x 3 matrices in closed form (expansion along the first row), in the oracle's vectorised arithmetic."""
    t0 = F.mul(_col(S, 0, 0), _minor2(F, S, 1, 2, 1, 2))
    t1 = F.mul(_col(S, 0, 1), _minor2(F, S, 1, 2, 0, 2))
    t2 = F.mul(_col(S, 0, 2), _minor2(F, S, 1, 2, 0, 1))
    return F.add(F.sub(t0, t1), t2)


def _matmul3(F, A, B):
    """Stack of products of 3 x 3 matrices, entry by entry in the oracle's vectorised arithmetic."""
    C = np.empty((A.shape[0], 3, 3), dtype=np.uint64)
    for i in range(3):
        for j in range(3):
            acc = F.mul(_col(A, i, 0), _col(B, 0, j))
            for k in (1, 2):
                acc = F.add(acc, F.mul(_col(A, i, k), _col(B, k, j)))
            C[:, i, j] = acc
    return C


def _ranks_3x4(F, S):
    """Ranks of a stack of 3 x 4 matrices from their minors: 3 if a 3 x 3 minor is non-zero, else 2 if a 2 x 2 minor is, else 1 if an entry is."""
    r3 = np.zeros(S.shape[0], dtype=bool)
    for skip in range(4):
        r3 |= _det3(F, S[:, :, [c for c in range(4) if c != skip]]) != 0
    r2 = np.zeros(S.shape[0], dtype=bool)
    for r0, r1 in ((0, 1), (0, 2), (1, 2)):
        for c0 in range(4):
            for c1 in range(c0 + 1, 4):
                r2 |= _minor2(F, S, r0, r1, c0, c1) != 0
    r1_ = S.reshape(S.shape[0], -1).any(axis=1)
    return np.where(r3, 3, np.where(r2, 2, np.where(r1_, 1, 0)))


def _stack3x3(tag):
    def make():
        GF, F = _ctx(tag)
        S = _rand(_rng(tag, "stack3x3"), GF.order, (N_STACK, 3, 3))
        return _frozen(S), _det3(F, S)
    return _memo((tag, "stack3x3"), make)


@pytest.mark.parametrize("tag", ["gf31", "gf256"])
def test_P7_determinants_of_65539_matrices(tag):
    GF, F = _ctx(tag)
    S, dets = _stack3x3(tag)
    assert N_STACK > 65535 and EP.plu_supported(3, 3)
    for i in (0, 65534, 65535, 65538):
        assert int(dets[i]) == F.det(S[i]), "the closed form is the oracle's determinant"
    got = ga.linalg.det_batched(GF(S)).numpy()
    bad = np.flatnonzero(got.astype(np.uint64) != dets)
    assert bad.size == 0, f"{tag}: {bad.size} determinants differ, first at {bad[:5].tolist()}"
    assert 0 < np.count_nonzero(dets == 0) < N_STACK // 8


@pytest.mark.parametrize("tag", ["gf31", "gf256"])
def test_P7_inverses_and_products_of_65539_matrices(tag):
    """inv_batched of the non-singular matrices of the stack -- fewer than 65536 of the 65539 random ones, so the first of them are repeated
    to bring the stack back to 65539 and the product A @ inv(A) past the 65535 matrices gfa_matmul launches per slice.  Every product of
    that check is the identity, so a slice written to the wrong place could go unnoticed; the product of the whole stack with itself
    rolled by one has no two results alike, and is compared with the oracle entry by entry."""
    GF, F = _ctx(tag)
    S, dets = _stack3x3(tag)
    good = np.flatnonzero(dets != 0)
    idx = np.concatenate([good, good[:N_STACK - good.size]])
    assert idx.size == N_STACK > 65535 and good.size > N_STACK // 2
    gA = GF(S[idx])
    inv = ga.linalg.inv_batched(gA)
    prod = (gA @ inv).numpy().astype(np.uint64)
    bad = np.flatnonzero((prod != np.eye(3, dtype=np.uint64)).reshape(N_STACK, -1).any(axis=1))
    assert bad.size == 0, f"{tag}: A @ inv(A) != I for {bad.size} matrices, first at {bad[:5].tolist()}"
    with pytest.raises(np.linalg.LinAlgError):
        ga.linalg.inv_batched(GF(S[np.flatnonzero(dets == 0)[:1]]))
    B = np.roll(S, 1, axis=0)
    C = (GF(S) @ GF(B)).numpy().astype(np.uint64)
    bad = np.flatnonzero((C != _matmul3(F, S, B)).reshape(N_STACK, -1).any(axis=1))
    assert bad.size == 0, f"{tag}: {bad.size} products differ, first at {bad[:5].tolist()} (a slice starts at matrix 65535)"


@pytest.mark.parametrize("tag", ["gf31", "gf256"])
def test_P7_row_reduction_of_65539_matrices(tag):
    """65539 random 3 x 4 matrices, a few of lower rank planted on both sides of index 65535: every rank against the minors in the oracle's
    arithmetic, 64 reduced forms (index 0, 65534, 65535, 65538, the planted ones, random others) against the oracle."""
    GF, F = _ctx(tag)
    rng = _rng(tag, "stack3x4")
    S = _rand(rng, GF.order, (N_STACK, 3, 4))
    planted = [7, 65534, 65535, 65536, 65538]
    S[7, 1:] = 0                      # rank 1
    S[65534, 2] = S[65534, 0]         # rank 2
    S[65535] = 0                      # rank 0
    S[65536, 1] = S[65536, 2]         # rank 2
    S[65538, :, 0] = 0                # no pivot in column 0
    assert EP.elim_route(N_STACK, 3, 4) == EP.ONE_WORKGROUP
    want_ranks = _ranks_3x4(F, S)
    assert [int(want_ranks[i]) for i in planted[:4]] == [1, 2, 0, 2]
    got, ranks = ga.linalg.row_reduce_batched(GF(S))
    bad = np.flatnonzero(ranks != want_ranks)
    assert bad.size == 0, f"{tag}: {bad.size} ranks differ, first at {bad[:5].tolist()}"
    fixed = [0] + planted
    others = [int(i) for i in rng.choice(N_STACK, 64, replace=False) if int(i) not in fixed]
    sample = sorted(fixed + others[:64 - len(fixed)])
    assert len(set(sample)) == 64 and {0, 65534, 65535, 65538} <= set(sample)
    g = got.numpy()
    for i in sample:
        want, rank = F.row_reduce(S[i])
        H.assert_equal_ints(g[i], want, f"{tag} matrix {i}")
        assert int(ranks[i]) == rank


# ---- two-limb fields (csrc/gfa_wide.hip) -----------------------------------------------------------------------------------------------
def _plu_scalar(W, rows):
    """plu_decompose_jit of the reference on the oracle's scalars (the rules of OracleField.plu_decompose): returns P (as the reference
    does: the transpose of the row permutation), L, U and the number of exchanges."""
    A = [list(map(int, r)) for r in rows]
    m, n = len(A), len(A[0])
    L = [[0] * m for _ in range(m)]
    P = [[int(i == j) for j in range(m)] for i in range(m)]
    nperm = 0
    for i in range(min(m, n)):
        if A[i][i] == 0:
            nz = [r for r in range(i, m) if A[r][i]]
            if not nz:
                L[i][i] = 1
                continue
            j = nz[0]
            P[i], P[j] = P[j], P[i]
            A[i], A[j] = A[j], A[i]
            L[i], L[j] = L[j], L[i]
            nperm += 1
        inv = W.inv(A[i][i])
        for r in range(i + 1, m):
            l = W.mul(A[r][i], inv)
            L[r][i] = l
            if l:
                A[r] = [W.sub(v, W.mul(l, t)) for v, t in zip(A[r], A[i])]
        L[i][i] = 1
    L[m - 1][m - 1] = 1
    return [[P[j][i] for j in range(m)] for i in range(m)], L, A, nperm


def _lu_scalar(W, rows):
    """lu_decompose_jit on the oracle's scalars (OracleField.lu_decompose): ValueError where a row exchange would be needed."""
    A = [list(map(int, r)) for r in rows]
    m = len(A)
    L = [[int(i == j) for j in range(m)] for i in range(m)]
    for i in range(m - 1):
        if A[i][i] == 0:
            if not any(A[r][i] for r in range(i, m)):
                L[i][i] = 1
                continue
            raise ValueError("The LU decomposition of 'A' does not exist. Use the PLU decomposition instead.")
        inv = W.inv(A[i][i])
        for r in range(i + 1, m):
            l = W.mul(A[r][i], inv)
            L[r][i] = l
            if l:
                A[r] = [W.sub(v, W.mul(l, t)) for v, t in zip(A[r], A[i])]
    return L, A


def _det_scalar(W, L, U, nperm):
    d = 1
    for i in range(len(U)):
        d = W.mul(W.mul(d, L[i][i]), U[i][i])
    return W.neg(d) if nperm % 2 else d


def _wide_rows(tag, salt, m, n):
    GF, W, f = LE._ctx(tag)
    rng = LE._rng(tag, salt)
    return GF, W, [[rng.randrange(W.q) for _ in range(n)] for _ in range(m)]


@pytest.mark.parametrize("tag", LE.LOOP_TAGS)
def test_L1_two_limb_row_reduce_of_300_by_6_with_late_pivots(tag):
    """Rows 0..279 are zero in columns 0..2: the first pivots are found in the second pass of the pivot search."""
    GF, W, a = _wide_rows(tag, "L1", 300, 6)
    for r in range(280):
        a[r][0] = a[r][1] = a[r][2] = 0
    want, rank = LE._row_reduce(W, a, 6)
    assert rank == 6 and any(a[r][0] for r in range(280, 300))
    A = GF(LE._obj2(a))
    H.assert_equal_ints(A.row_reduce().numpy(), LE._obj2(want), f"{tag} row_reduce of 300 x 6")
    assert np.linalg.matrix_rank(A) == rank


@pytest.mark.parametrize("tag", LE.LOOP_TAGS)
def test_L2_two_limb_row_reduce_of_6_by_300(tag):
    GF, W, a = _wide_rows(tag, "L2", 6, 300)
    a[0][0] = a[1][0] = 0
    want, rank = LE._row_reduce(W, a, 300)
    assert rank == 6
    H.assert_equal_ints(GF(LE._obj2(a)).row_reduce().numpy(), LE._obj2(want), f"{tag} row_reduce of 6 x 300")


@pytest.mark.parametrize("tag", LE.LOOP_TAGS)
def test_L3_two_limb_plu_lu_and_det_of_20_by_20(tag):
    """a[0][0] = a[1][0] = 0 forces an exchange; column 7 = 3 column 2 + column 5 leaves step 7 without a pivot."""
    GF, W, a = _wide_rows(tag, "L3", 20, 20)
    a[0][0] = a[1][0] = 0
    for r in a:
        r[7] = W.add(W.mul(3 % W.q, r[2]), r[5])
    P, L, U, nperm = _plu_scalar(W, a)
    assert nperm >= 1 and U[7][7] == 0 and not any(U[r][7] for r in range(7, 20)) and all(U[i][i] for i in range(7))
    A = GF(LE._obj2(a))
    p, l, u = A.plu_decompose()
    H.assert_equal_ints(p.numpy(), LE._obj2(P), f"{tag} P")
    H.assert_equal_ints(l.numpy(), LE._obj2(L), f"{tag} L")
    H.assert_equal_ints(u.numpy(), LE._obj2(U), f"{tag} U")
    H.assert_equal_ints((p @ l @ u).numpy(), LE._obj2(a), f"{tag} P @ L @ U")
    assert int(np.linalg.det(A)) == _det_scalar(W, L, U, nperm) == 0
    with pytest.raises(ValueError):
        _lu_scalar(W, a)
    with pytest.raises(ValueError):
        A.lu_decompose()
    # the same rows in pivot order have an LU, with the pivot-free step in it
    b = [[sum(P[k][i] * a[k][j] for k in range(20)) for j in range(20)] for i in range(20)]
    Lw, Uw = _lu_scalar(W, b)
    assert Uw[7][7] == 0
    lg, ug = GF(LE._obj2(b)).lu_decompose()
    H.assert_equal_ints(lg.numpy(), LE._obj2(Lw), f"{tag} LU: L")
    H.assert_equal_ints(ug.numpy(), LE._obj2(Uw), f"{tag} LU: U")
    # column 7 random again: a determinant other than zero, its sign from the exchanges
    rng = LE._rng(tag, "L3 column 7")
    c = [r[:7] + [rng.randrange(W.q)] + r[8:] for r in a]
    Pc, Lc, Uc, nc = _plu_scalar(W, c)
    d = _det_scalar(W, Lc, Uc, nc)
    assert d != 0 and nc >= 1
    assert int(np.linalg.det(GF(LE._obj2(c)))) == d


@pytest.mark.parametrize("tag", LE.LOOP_TAGS)
def test_L4_two_limb_plu_of_300_by_4(tag):
    """L and P are 300 x 300: their initialisation runs 352 passes, and the exchange of rows 0 and 280 (column 0 is zero above row 280)
    a second pass over the columns."""
    GF, W, a = _wide_rows(tag, "L4", 300, 4)
    for r in range(280):
        a[r][0] = 0
    a[280][0] = a[280][0] or 1
    P, L, U, nperm = _plu_scalar(W, a)
    assert P[280][0] == 1 and nperm >= 1
    p, l, u = GF(LE._obj2(a)).plu_decompose()
    H.assert_equal_ints(p.numpy(), LE._obj2(P), f"{tag} P")
    H.assert_equal_ints(l.numpy(), LE._obj2(L), f"{tag} L")
    H.assert_equal_ints(u.numpy(), LE._obj2(U), f"{tag} U")
