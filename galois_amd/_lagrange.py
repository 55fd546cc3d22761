"""
Interpolation, and the Chinese remainder theorem.  Paths relative to /root/reference/src/galois:

  * lagrange_poly(x, y) ......... _polys/_lagrange.py:19-74 over lagrange_poly_jit (:77-133)
  * crt(remainders, moduli) ..... _polymorphic.py:386-521

The reference builds L = sum y_j prod (x - x_m) / (x_j - x_m) with a doubly nested loop of polynomial products.  Here one
gfa_poly_lagrange call (galois_amd/csrc/gfa_lagrange.hip) interpolates a whole stack of point sets: per row the weights
w_i = prod (x_i - x_m), whose zero is the test for a repeated x, c_i = y_i / w_i, and k sweeps

    A <- x A - x_s A + c_s M        M <- x M - x_s M        (M = prod_{m<s} (x - x_m), A = sum_{i<s} c_i M / (x - x_i))

after which A is L.  Three routes with identical results:

  kernel   the launch above; rows of a stack may share one x (x_rows = 1)
  matmul   shared x and many rows: the k basis polynomials once (the kernel on y = identity), then y @ basis on gfa_matmul
  arrays   fields of order >= 2^64 and point counts above the kernel's cap (lagrange_max_points): the same weights and sweeps as
           whole-array operations, one step per point and none per element

lagrange_poly_batched exposes the stack.  crt folds pairs of congruences over egcd as the reference does; when every modulus is
a monic x - r and the r are distinct the system is an interpolation problem, and it goes to the kernel.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from ._array import FieldArray, _GFA_DTYPE, _ptr, _stream
from ._poly import Poly
from ._polydiv import POW_LDS_BYTES, _elem_bytes, _is_zero
from ._polygcd import _int_egcd, poly_egcd

# Shared x: the matmul route from this many rows per point and this many sweep steps (batch * k^2) on.  Measured on an MI355X
# (tools/bench_lagrange.py, profiles/lagrange_time.txt): below either bound the single launch of the
# kernel is faster than the basis call plus a product, above both the product wins by up to 15 x.
MATMUL_MIN_ROWS_PER_POINT = 16
MATMUL_MIN_WORK = 2**24


def lagrange_max_points(field) -> int:
    """Largest number of points of a row gfa_poly_lagrange serves over the field (LG_MAX_POINTS): the kernel holds the row's points,
    weights and two pairs of polynomials in LDS, and one flag."""
    return (POW_LDS_BYTES // _elem_bytes(field) - 1) // 6


def _kernel_serves(F, k: int) -> bool:
    return not F._limbed and 1 <= k <= lagrange_max_points(F)


# ---- the three routes on 2-D arrays: X is (1, k) or (batch, k), Y is (batch, k) -----------------------------------------------------
def _lagrange_t(field, x: torch.Tensor, y: torch.Tensor):
    """(coefficients (batch, k), int32 status (batch,)) of one gfa_poly_lagrange call on contiguous storage tensors."""
    batch, k = y.shape
    coeffs = torch.empty_like(y)
    status = torch.empty(batch, dtype=torch.int32, device=y.device)
    L.check(L.lib().gfa_poly_lagrange(field._handle, _ptr(x), _ptr(y), batch, k, x.shape[0], _ptr(coeffs), _ptr(status), _GFA_DTYPE[y.element_size()],
                                      _stream()), "gfa_poly_lagrange")
    return coeffs, status


def _route_kernel(F, X: FieldArray, Y: FieldArray):
    coeffs, status = _lagrange_t(F, X._t.contiguous(), X._same_storage(Y).contiguous())
    return F._wrap(coeffs, X._np_dtype), status.cpu().numpy() != 0


def _route_matmul(F, X: FieldArray, Y: FieldArray):
    k = X.shape[1]
    basis, dup = _route_kernel(F, X, F.Identity(k, dtype=X.dtype))  # row i: the polynomial that is 1 at x_i and 0 at the others
    yk = F._wrap(X._same_storage(Y), X._np_dtype)
    return yk @ basis, np.full(Y.shape[0], bool(dup.any()))


def _route_arrays(F, X: FieldArray, Y: FieldArray):
    batch, k = Y.shape
    xr = X.shape[0]
    eye = F.Identity(k, dtype=X.dtype)
    w = None
    for m in range(k):  # w_i = prod over m != i of (x_i - x_m): the factor m = i is 0 + 1
        d = X - X[:, m:m + 1] + eye[m:m + 1]
        w = d if w is None else w * d
    rep = np.asarray(w == 0)
    dup = rep.any(axis=1)
    if dup.any():  # keep the division defined; these rows are zeroed below
        w = np.where(rep, F.Ones((xr, k), dtype=X.dtype), w)
    c = Y / w
    A = F.Zeros((batch, k), dtype=X.dtype)  # highest degree first
    M = F.Zeros((xr, k), dtype=X.dtype)
    M[:, k - 1] = 1
    za, zm = F.Zeros((batch, 1), dtype=X.dtype), F.Zeros((xr, 1), dtype=X.dtype)
    for s in range(k):
        xs = X[:, s:s + 1]
        A = np.concatenate([A[:, 1:], za], axis=1) - xs * A + c[:, s:s + 1] * M
        M = np.concatenate([M[:, 1:], zm], axis=1) - xs * M
    dup = dup if xr == batch else np.full(batch, bool(dup.any()))
    if dup.any():
        A = np.where(np.broadcast_to(dup[:, None], (batch, k)).copy(), F.Zeros((batch, k), dtype=X.dtype), A)
    return A, dup


def _route(F, shared: bool, batch: int, k: int) -> str:
    """The route lagrange_poly_batched takes by default."""
    if not _kernel_serves(F, k):
        return "arrays"
    return "matmul" if shared and batch >= MATMUL_MIN_ROWS_PER_POINT * k and batch * k * k >= MATMUL_MIN_WORK else "kernel"


def _interpolate(F, X: FieldArray, Y: FieldArray, method: str | None = None):
    """(coefficients (batch, k) highest degree first, bool np.ndarray (batch,): the row's x has a repeated entry and its
    coefficients are zero)."""
    batch, k = Y.shape
    shared = X.shape[0] == 1
    if method is None:
        method = _route(F, shared and batch > 1, batch, k)
    if method == "matmul" and not (shared and _kernel_serves(F, k)):
        raise ValueError("The matmul route needs one x for all rows and a point count the kernel serves.")
    return {"kernel": _route_kernel, "matmul": _route_matmul, "arrays": _route_arrays}[method](F, X, Y)


# ---- the public functions -------------------------------------------------------------------------------------------------------------
def _verify(x, y):
    if not isinstance(x, FieldArray):
        raise TypeError(f"Argument 'x' must be an instance of {FieldArray}, not {type(x)}.")
    if not isinstance(y, FieldArray):
        raise TypeError(f"Argument 'y' must be an instance of {FieldArray}, not {type(y)}.")
    if type(x) is not type(y):
        raise TypeError(f"Arguments 'x' and 'y' must be over the same Galois field, not {type(x)} and {type(y)}.")


def _check_method(method):
    if method not in (None, "kernel", "matmul", "arrays"):
        raise ValueError(f"Argument 'method' must be in ['kernel', 'matmul', 'arrays'], not {method!r}.")


def lagrange_poly(x: FieldArray, y: FieldArray, method: str | None = None) -> Poly:
    """galois.lagrange_poly (_polys/_lagrange.py:19-74): the polynomial L of least degree with L(x_i) = y_i.  x and y are 1-D arrays
    over the same field, of the same size, and x has no repeated entry.  `method` ("kernel" or "arrays") overrides the choice of
    the route, for tests."""
    _verify(x, y)
    _check_method(method)
    if not x.ndim == 1:
        raise ValueError(f"Argument 'x' must be 1-D, not have shape {tuple(x.shape)}.")
    if not y.ndim == 1:
        raise ValueError(f"Argument 'y' must be 1-D, not have shape {tuple(y.shape)}.")
    if not x.size == y.size:
        raise ValueError(f"Arguments 'x' and 'y' must be the same size, not {x.size} and {y.size}.")
    F = type(x)
    if x.size == 0:
        return Poly(F.Zeros(1))
    coeffs, dup = _interpolate(F, x.reshape(1, -1), y.reshape(1, -1), method)
    if dup[0]:
        raise ValueError(f"Argument 'x' must have unique entries, not {x}.")
    return Poly(coeffs[0])


def lagrange_poly_batched(x: FieldArray, y: FieldArray, method: str | None = None) -> FieldArray:
    """Device extension: the coefficients of lagrange_poly(x[r], y[r]) for every row of a (batch, k) stack `y` of ordinates, k >= 1;
    `x` is (batch, k), or 1-D of k abscissae shared by all rows.  Returns (batch, k) coefficients, highest degree first,
    right-aligned and zero-filled on the left.  One gfa_poly_lagrange call; with a shared x and a large batch (at least 16 rows
    per point and 2^24 sweep steps), the k basis polynomials from one call and one matrix product.  A row whose x has a repeated entry raises ValueError naming
    the first such row.  `method` ("kernel", "matmul" or "arrays") overrides the choice of the route, for tests."""
    _verify(x, y)
    _check_method(method)
    if not (y.ndim == 2 and y.shape[1] >= 1):
        raise ValueError(f"Argument 'y' must be 2-D with one set of ordinates per row, not have shape {tuple(y.shape)}.")
    if not (x.ndim in (1, 2) and x.shape[-1] == y.shape[1] and (x.ndim == 1 or x.shape[0] == y.shape[0])):
        raise ValueError(f"Argument 'x' must have the shape of 'y' or be 1-D of its row length, not have shapes {tuple(x.shape)} and {tuple(y.shape)}.")
    F = type(x)
    batch, k = y.shape
    if batch == 0:
        return y.copy()
    coeffs, dup = _interpolate(F, x.reshape(1, k) if x.ndim == 1 else x, y, method)
    if dup.any():
        row = int(np.flatnonzero(dup)[0])
        raise ValueError(f"Argument 'x' must have unique entries in every row, not {x if x.ndim == 1 else x[row]} in row {row}.")
    return coeffs


# ---- crt ----------------------------------------------------------------------------------------------------------------------------------
def _crt_linear(remainders, moduli):
    """The solution when every modulus is a monic x - r over one field with distinct r -- L with L(r_i) = a_i --, else None."""
    F = moduli[0].field
    if not all(p.field is F for p in list(remainders) + list(moduli)):
        return None
    if not all(m.degree == 1 and int(m.coeffs[0]) == 1 for m in moduli):
        return None
    like = moduli[0].coeffs

    def cat(parts):
        if F._limbed:
            return np.concatenate(parts)
        return F._wrap(torch.cat([like._same_storage(p) for p in parts]), like._np_dtype)

    r = -cat([m.coeffs[1:2] for m in moduli])
    a = cat([p.coeffs[-1:] for p in remainders])  # degree < 1: constants
    coeffs, dup = _interpolate(F, r.reshape(1, -1), a.reshape(1, -1))
    return None if dup[0] else Poly(coeffs[0])


def crt(remainders, moduli):
    """galois.crt (_polymorphic.py:386-521): the solution x of x = a_i (mod m_i) for integers or for polynomials, modulo the least
    common multiple of the moduli.  Moduli need not be coprime; ValueError when the congruences contradict each other."""
    def homogeneous(values):
        return all(isinstance(v, (int, np.integer)) for v in values) or all(isinstance(v, Poly) for v in values)

    if not (isinstance(remainders, (tuple, list)) and homogeneous(remainders)):
        raise TypeError(f"Argument 'remainders' must be a tuple or list of int or Poly, not {remainders}.")
    if not (isinstance(moduli, (tuple, list)) and homogeneous(moduli)):
        raise TypeError(f"Argument 'moduli' must be a tuple or list of int or Poly, not {moduli}.")
    if not len(remainders) == len(moduli) >= 2:
        raise ValueError(f"Arguments 'remainders' and 'moduli' must be the same length of at least 2, not {len(remainders)} and {len(moduli)}.")
    polys = isinstance(remainders[0], Poly)
    if polys != isinstance(moduli[0], Poly):
        raise TypeError(f"Arguments 'remainders' and 'moduli' must both hold int or both hold Poly, not {remainders} and {moduli}.")
    if polys:
        for remainder, modulus in zip(remainders, moduli):
            if not (_is_zero(remainder) or remainder.degree < modulus.degree):
                raise ValueError(f"Each remainder must have degree strictly less than its modulus. Remainder {remainder} with modulus {modulus} "
                                 "does not satisfy that condition.")
        x = _crt_linear(remainders, moduli)
        if x is not None:
            return x
        return _crt_fold(remainders, moduli)
    a1, m1 = int(remainders[0]), int(moduli[0])
    for a2, m2 in zip(remainders[1:], moduli[1:]):
        a2, m2 = int(a2), int(m2)
        d, b1, b2 = _int_egcd(m1, m2)
        if d != 1 and not (a1 % d) == (a2 % d):
            raise ValueError(f"Moduli {[m1, m2]} are not coprime and their residuals {[a1, a2]} are not equal modulo their GCD {d}, "
                             "therefore a unique solution does not exist.")
        x = ((a1 * b2 * m2) + (a2 * b1 * m1)) // d
        m1 = (m1 * m2) // d
        a1 = x % m1
    return a1


def _crt_fold(remainders, moduli) -> Poly:
    """The reference's fold: two congruences become one, through b1 m1 + b2 m2 = gcd(m1, m2)."""
    a1, m1 = remainders[0], moduli[0]
    for a2, m2 in zip(remainders[1:], moduli[1:]):
        d, b1, b2 = poly_egcd(m1, m2)
        if d.degree == 0:  # coprime (the gcd is monic)
            x = (a1 * b2 * m2) + (a2 * b1 * m1)
            m1 = m1 * m2
        else:
            if not (a1 % d) == (a2 % d):
                raise ValueError(f"Moduli {[m1, m2]} are not coprime and their residuals {[a1, a2]} are not equal modulo their GCD {d}, "
                                 "therefore a unique solution does not exist.")
            x = ((a1 * b2 * m2) + (a2 * b1 * m1)) // d
            m1 = (m1 * m2) // d
        a1 = x % m1
    return a1
