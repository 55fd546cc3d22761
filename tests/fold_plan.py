"""The route a gfa_reduce / gfa_accumulate call takes, in Python: a mirror of galois_amd/csrc/gfa_reduce_plan.h (segments per row, segment
length, first-phase kernel) and of the choice of the joining kernel in gfa_reduce.hip::launch_reduce_ft / launch_accumulate_ft.

tests/test_reduce_plan_host.py compiles the header for the host and compares its plans with this module line for line, so the mirror cannot
drift; tests/test_gpu_folds.py derives its shapes from it and asserts the route of every case before launching."""
from collections import namedtuple

ADD, SUB, MUL, DIV = 0, 1, 2, 3  # GFA_OP_*
OPS = {"add": ADD, "subtract": SUB, "multiply": MUL, "divide": DIV}
GENERIC, STREAM_XOR, STREAM_SUM, STREAM_LOG, STREAM_TAB = -1, 0, 1, 2, 3
MAX_SEGMENTS = 4096
MAX_GRID = 2**31 - 1

# nseg, seg_len: segments per row and columns per segment (seg_len 0: the whole-row scan).  form: the first-phase kernel (STREAM_* is
# reduce_stream_kernel's MODE, GENERIC reduce_segments_kernel; None when no first phase runs).  join: "thread" (reduce_finalize_kernel),
# "block" (reduce_finalize_block_kernel), "carries" (accumulate_carries_kernel + a second accumulate_kernel pass) or "row" (one
# accumulate_kernel workgroup per row).  c: runs per thread of accumulate_carries_kernel, 0 elsewhere.
Plan = namedtuple("Plan", "kind op n_outer n_inner nseg seg_len form join c")


def _is_mul(op):
    return op in (MUL, DIV)


def _col_begin(op):
    return 1 if op in (SUB, DIV) else 0


# The header's has_log8 / has_add8 (the byte LOG + EXP / sum tables are on the device) are written q <= 256 here: gfa_field::ensure_device
# uploads them for every field of at most 256 elements, in either arithmetic mode, or fails the call.
def table_sum(op, elem_size, m, q, lookup):
    return not _is_mul(op) and lookup and elem_size == 1 and q <= 256 and m > 1  # (q <= 256: the field has its byte tables)


def stream_mode(op, elem_size, p, m, q, lookup, seg_len):
    mul = _is_mul(op)
    if not mul and p == 2:
        return STREAM_XOR
    if not mul and m == 1 and elem_size <= 4 and seg_len < 2**32:
        return STREAM_SUM
    if mul and lookup and elem_size == 1 and q <= 256 and seg_len < 2**40:
        return STREAM_LOG
    if table_sum(op, elem_size, m, q, lookup):
        return STREAM_TAB
    return GENERIC


def plan_reduce(op, n_outer, n_inner, elem_size, p, m, q, lookup, cus):
    length = n_inner - _col_begin(op)
    want_blocks = cus * (2 if table_sum(op, elem_size, m, q, lookup) else 8)
    nseg = 1
    if n_outer < want_blocks and length > 8192:
        nseg = min((want_blocks + n_outer - 1) // n_outer, (length + 4095) // 4096, MAX_SEGMENTS)
    nseg = max(nseg, 1)
    seg_len = (length + nseg - 1) // nseg if length > 0 else 1
    return Plan("reduce", op, n_outer, n_inner, nseg, seg_len, stream_mode(op, elem_size, p, m, q, lookup, seg_len),
                "block" if nseg > 8 else "thread", 0)


def plan_accumulate(op, n_outer, n_inner, elem_size, p, m, q, lookup, cus):
    length = n_inner - _col_begin(op)
    want_blocks = cus * 8
    if n_outer < want_blocks // 4 and length >= 2**16:
        nseg = min((want_blocks + n_outer - 1) // n_outer, length // 8192, MAX_SEGMENTS)
        if nseg >= 2:
            seg_len = ((length + nseg - 1) // nseg + 255) // 256 * 256
            nseg = (length + seg_len - 1) // seg_len
            return Plan("accumulate", op, n_outer, n_inner, nseg, seg_len, stream_mode(op, elem_size, p, m, q, lookup, seg_len), "carries",
                        (nseg + 255) // 256)
    return Plan("accumulate", op, n_outer, n_inner, 1, 0, None, "row", 0)


def plan(kind, op, n_outer, n_inner, elem_size, p, m, q, lookup, cus):
    return (plan_reduce if kind == "reduce" else plan_accumulate)(op, n_outer, n_inner, elem_size, p, m, q, lookup, cus)


def segments(pl):
    """[(first column, one past the last column)] of every segment of a row."""
    cb = _col_begin(pl.op)
    if pl.seg_len == 0:
        return [(cb, pl.n_inner)]
    return [(cb + s * pl.seg_len, min(cb + (s + 1) * pl.seg_len, pl.n_inner)) for s in range(pl.nseg)]


def describe(pl, elem_size, p, m, lookup, cus):
    """One line per plan, the format tests/csrc/reduce_plan_host_test.cpp prints."""
    form = "none" if pl.form is None else str(pl.form)
    return (f"{pl.kind} op={pl.op} cus={cus} rows={pl.n_outer} cols={pl.n_inner} size={elem_size} p={p} m={m} lut={int(lookup)} -> "
            f"nseg={pl.nseg} seg_len={pl.seg_len} form={form} join={pl.join} c={pl.c}")
