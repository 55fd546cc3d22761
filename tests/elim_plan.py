"""The route a gfa_row_reduce call takes and the shapes gfa_plu_decompose accepts, in Python: a mirror of galois_amd/csrc/gfa_elim_plan.h.
tests/test_elim_plan_host.py compiles the header for the host and compares its routes with this module line for line, so the mirror cannot
drift; tests/test_gpu_elimination_routes.py asserts the route of every shape it names before launching it, so a later change of a threshold
fails there loudly instead of quietly turning a test of one route into a test of the other."""

GJ_THREADS = 256            # row_reduce_kernel, plu_kernel: one workgroup per matrix
GJ_MAX_ROWS = 4096          # their LDS array of column factors
GJ_MAX_DIM = 1 << 24
GJ_WIDE_MIN_ELEMS = 131072
GJ_WIDE_MAX_BATCH = 32
GJ_WIDE_ROW_TILE = 32
GJ_WIDE_MAX_ROWS = 65535 * GJ_WIDE_ROW_TILE
WIDE_PIVOT_THREADS = 1024   # gj_pivot_kernel's workgroup (not part of the route decision: the tests size their passes with it)

ONE_WORKGROUP, TWO_KERNELS, UNSUPPORTED = "ONE_WORKGROUP", "TWO_KERNELS", "UNSUPPORTED"


def elim_route(batch, m, n):
    if batch < 1 or m < 1 or n < 1 or m > GJ_MAX_DIM or n > GJ_MAX_DIM:
        return UNSUPPORTED
    if batch <= GJ_WIDE_MAX_BATCH and (m * n >= GJ_WIDE_MIN_ELEMS or m > GJ_MAX_ROWS):
        return TWO_KERNELS if m <= GJ_WIDE_MAX_ROWS else UNSUPPORTED
    return ONE_WORKGROUP if m <= GJ_MAX_ROWS else UNSUPPORTED


def plu_supported(m, n):
    return 1 <= m <= GJ_MAX_ROWS and 1 <= n <= GJ_MAX_DIM


def describe_route(batch, m, n):
    """One line per call, the format tests/csrc/elim_plan_host_test.cpp prints."""
    return f"row_reduce batch={batch} m={m} n={n} -> {elim_route(batch, m, n)}"


def describe_plu(m, n):
    return f"plu m={m} n={n} -> {'yes' if plu_supported(m, n) else 'no'}"
