"""
Polynomial division with remainder and modular powers.  Paths relative to /root/reference/src/galois:

  * divmod(f, g), f // g, f % g ........ _polys/_poly.py:1327-1439 over divmod_jit / floordiv_jit / mod_jit (_polys/_dense.py:126-320)
  * f ** e, pow(f, e, g) ............... _polys/_poly.py:1441-1460 over pow_jit (_polys/_dense.py:323-401)

The reference divides one pair at a time.  The kernels (galois_amd/csrc/gfa_polydiv.hip) take a whole stack of dividends against
one divisor, and a whole stack of bases raised to one exponent modulo one polynomial; the Poly operators are the batch-of-one
case and poly_divmod_batched / poly_powmod_batched expose the stacks.  gfa_poly_powmod keeps its operands in LDS, which caps the
degree of the modulus (powmod_max_degree); above the cap the same square-and-multiply chain runs here, one np.convolve and one
remainder-only gfa_poly_divmod per step.  Fields of order >= 2^64 have no kernel: their division is a host loop, one quotient
term per step, on the limb ufuncs.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib as L
from ._array import FieldArray, _ptr, _stream

# the kernels' geometry (gfa_polydiv.h / gfa_polydiv.hip), for documentation and for the tests that probe its boundaries
BLOCK = 64                   # quotient coefficients per block (PD_K)
DIV_THREADS = 1024           # threads of a workgroup at most (512 for digit-vector fields of degree 11 .. 16)
DIV_LDS_BYTES = 64 * 1024    # divisor + window: 2 nb - 1 + 2 BLOCK elements; longer divisors work in global memory
POW_LDS_BYTES = 150 * 1024


def _elem_bytes(field) -> int:
    """Size of an element inside the kernels: 32 bits for prime fields below 2^32 and for fields served from tables (the rule of
    gfa_field::use_lookup), 64 bits otherwise."""
    mode = L.lib().gfa_field_get_mode(field._handle)
    has_lut = field.order <= 2**20
    if mode == L.MODE_LOOKUP:
        lookup = has_lut
    elif mode == L.MODE_CALCULATE:
        lookup = False
    else:
        lookup = has_lut and (field.order <= 256 or (field.degree > 1 and field.characteristic != 2))
    return 4 if lookup or (field.degree == 1 and field.order < 2**32) else 8


def powmod_max_degree(field) -> int:
    """Largest degree of a modulus gfa_poly_powmod serves over the field (PD_POWMOD_MAX)."""
    return (POW_LDS_BYTES // _elem_bytes(field) - 2 * BLOCK - 1) // 5


def divmod_lds_max_divisor(field) -> int:
    """Longest divisor (in coefficients) whose window gfa_poly_divmod holds in LDS."""
    return (DIV_LDS_BYTES // _elem_bytes(field) + 1 - 2 * BLOCK) // 2


def _exp_limbs(e: int):
    n = max(1, (e.bit_length() + 63) // 64)
    arr = (ctypes.c_uint64 * n)()
    for l in range(n):
        arr[l] = (e >> (64 * l)) & 0xFFFFFFFFFFFFFFFF
    return arr, n


# ---- the two kernels on contiguous storage tensors ----------------------------------------------------------------------------
def _divmod_t(field, a: torch.Tensor, b: torch.Tensor, want_q: bool, want_r: bool):
    """(quotients or None, remainders or None) of the rows of a (batch, na) by b (nb <= na coefficients, b[0] != 0), untrimmed."""
    from ._array import _GFA_DTYPE

    batch, na = a.shape
    nb = b.numel()
    q = torch.empty((batch, na - nb + 1), dtype=a.dtype, device=a.device) if want_q else None
    r = torch.empty((batch, nb - 1), dtype=a.dtype, device=a.device) if want_r else None
    L.check(L.lib().gfa_poly_divmod(field._handle, _ptr(a), batch, na, _ptr(b), nb, _ptr(q) if want_q else None,
                                    _ptr(r) if want_r and nb > 1 else None, _GFA_DTYPE[a.element_size()], _stream()), "gfa_poly_divmod")
    return q, r


def _powmod_t(field, a: torch.Tensor, e: int, c: torch.Tensor) -> torch.Tensor:
    """a_k(x)^e mod c(x) for the rows of a (batch, na); c has nc >= 2 coefficients, nc - 1 <= powmod_max_degree(field)."""
    from ._array import _GFA_DTYPE

    batch, na = a.shape
    nc = c.numel()
    out = torch.empty((batch, nc - 1), dtype=a.dtype, device=a.device)
    limbs, n = _exp_limbs(e)
    L.check(L.lib().gfa_poly_powmod(field._handle, _ptr(a), batch, na, limbs, n, _ptr(c), nc, _ptr(out), _GFA_DTYPE[a.element_size()],
                                    _stream()), "gfa_poly_powmod")
    return out


# ---- one-dimensional coefficient arrays (trimmed divisor) ----------------------------------------------------------------------
def _divmod_limbed(a: FieldArray, b: FieldArray):
    """Fields of order >= 2^64: synthetic division on the host, one quotient term per step.  Needs a.size >= b.size."""
    nq = a.size - b.size + 1
    w = a.copy()
    binv = np.reciprocal(b[0])
    for i in range(nq):
        q = w[i] * binv
        w[i] = q
        if b.size > 1:
            w[i + 1:i + b.size] = w[i + 1:i + b.size] - q * b[1:]
    return w[:nq], w[nq:]


def _divmod_1d(a: FieldArray, b: FieldArray, want_q: bool = True, want_r: bool = True):
    """Untrimmed (quotient, remainder) of a by b, a.size >= b.size, b[0] != 0; a part not asked for is None."""
    F = type(a)
    if F._limbed:
        q, r = _divmod_limbed(a, b)
        return (q if want_q else None), (r if want_r else None)
    at = a._t.contiguous().reshape(1, -1)
    q, r = _divmod_t(F, at, a._same_storage(b).contiguous(), want_q, want_r)
    wrap = lambda t: None if t is None else F._wrap(t.reshape(-1), a._np_dtype)
    return wrap(q), wrap(r)


def _is_zero(p) -> bool:
    return p.degree == 0 and not bool(torch.any(p.coeffs._t != 0))  # (a Poly is held trimmed)


def _zero(F, like: FieldArray) -> FieldArray:
    return F.Zeros(1) if F._limbed else F._wrap(torch.zeros(1, dtype=like._t.dtype, device=like._t.device), like._np_dtype)


def _one(F, like: FieldArray) -> FieldArray:
    return F.Ones(1) if F._limbed else F._wrap(torch.ones(1, dtype=like._t.dtype, device=like._t.device), like._np_dtype)


def poly_divmod(a, b, want_q: bool = True, want_r: bool = True):
    """divmod of two Poly over the same field, as divmod_jit.__call__ (_dense.py:134-172); a part not asked for is None."""
    from ._poly import Poly

    F = a.field
    if _is_zero(b):
        raise ZeroDivisionError("Cannot divide a polynomial by zero.")
    if a.degree < b.degree:
        return (Poly(_zero(F, a.coeffs)) if want_q else None), (a if want_r else None)
    q, r = _divmod_1d(a.coeffs, b.coeffs, want_q, want_r)
    if want_r and (r is None or r.size == 0):
        r = _zero(F, a.coeffs)  # a constant divisor
    return (Poly(q) if want_q else None), (Poly(r) if want_r else None)


def _pow_loop(base: FieldArray, e: int, reduce) -> FieldArray:
    """base^e, e >= 1, left to right over the bits of e; `reduce` is applied to every product."""
    r = base
    for bit in bin(e)[3:]:
        r = reduce(np.convolve(r, r))
        if bit == "1":
            r = reduce(np.convolve(r, base))
    return r


def _powmod_1d(a: FieldArray, e: int, c: FieldArray) -> FieldArray:
    """a(x)^e mod c(x), e >= 1, c trimmed with at least two coefficients: nc - 1 untrimmed coefficients."""
    F = type(a)
    if not F._limbed and c.size - 1 <= powmod_max_degree(F):
        out = _powmod_t(F, a._t.contiguous().reshape(1, -1), e, a._same_storage(c).contiguous())
        return F._wrap(out.reshape(-1), a._np_dtype)
    reduce = lambda p: p if p.size < c.size else _divmod_1d(p, c, want_q=False)[1]
    return _pow_loop(reduce(a), e, reduce)


def poly_pow(a, exponent, modulus=None):
    """Poly.__pow__ (_polys/_poly.py:1441-1460 over pow_jit)."""
    from ._poly import Poly

    if not isinstance(exponent, (int, np.integer)):
        raise TypeError(f"Argument 'exponent' must be an instance of {int}, not {type(exponent)}.")
    if not exponent >= 0:
        raise ValueError(f"Can only exponentiate polynomials to non-negative integers, not {exponent}.")
    e = int(exponent)
    F = a.field
    if modulus is not None and _is_zero(modulus):
        raise ZeroDivisionError("Cannot reduce a polynomial modulo zero.")
    if e == 0:
        return Poly(_one(F, a.coeffs))
    if modulus is None:
        return Poly(_pow_loop(a.coeffs, e, lambda p: p))
    if modulus.degree == 0:
        return Poly(_zero(F, a.coeffs))
    return Poly(_powmod_1d(a.coeffs, e, modulus.coeffs))


# ---- the batched forms ----------------------------------------------------------------------------------------------------------
def _stack_and_divisor(A, b, name: str):
    from ._poly import Poly

    if not isinstance(A, FieldArray):
        raise TypeError(f"Argument 'A' must be a FieldArray, not {type(A)}.")
    if not (A.ndim == 2 and A.shape[1] >= 1):
        raise ValueError(f"Argument 'A' must be 2-D with one polynomial per row, highest degree first, not have shape {tuple(A.shape)}.")
    F = type(A)
    if isinstance(b, Poly):
        if b.field is not F:
            raise TypeError(f"Argument {name!r} must be over {F.name}, not {b.field.name}.")
    elif isinstance(b, FieldArray) and type(b) is F and b.ndim == 1 and b.size >= 1:
        b = Poly(b)
    else:
        raise TypeError(f"Argument {name!r} must be a Poly or a non-empty 1-D array over {F.name}, not {type(b)}.")
    return F, b


def _rows(F, A: FieldArray, fn, width: int) -> FieldArray:
    """Fields without a kernel: fn(row) -> 1-D coefficients for every row, right-aligned in `width` columns."""
    if F._limbed:
        out = F.Zeros((A.shape[0], width))
    else:
        out = F._wrap(torch.zeros((A.shape[0], width), dtype=A._t.dtype, device=A._t.device), A._np_dtype)
    for k in range(A.shape[0]):
        v = fn(A[k])
        out[k, width - v.size:] = v
    return out


def poly_divmod_batched(A: FieldArray, b):
    """Device extension: divmod(Poly(row), b) for every row of a (batch, n) array of coefficients, highest degree first, in one
    call.  Returns (Q, R), untrimmed: Q has max(n - deg b, 1) columns and R has max(deg b, 1)."""
    F, b = _stack_and_divisor(A, b, "b")
    if _is_zero(b):
        raise ZeroDivisionError("Cannot divide a polynomial by zero.")
    batch, na = A.shape
    nb = b.coeffs.size
    if F._limbed:
        if na < nb:
            return _rows(F, A, lambda row: F.Zeros(1), 1), _rows(F, A, lambda row: row, nb - 1)
        return (_rows(F, A, lambda row: _divmod_limbed(row, b.coeffs)[0], na - nb + 1),
                _rows(F, A, lambda row: _divmod_limbed(row, b.coeffs)[1], max(nb - 1, 1)))
    at = A._t.contiguous()
    if na < nb:
        q = torch.zeros((batch, 1), dtype=at.dtype, device=at.device)
        r = torch.zeros((batch, nb - 1), dtype=at.dtype, device=at.device)
        r[:, nb - 1 - na:] = at
    else:
        q, r = _divmod_t(F, at, A._same_storage(b.coeffs).contiguous(), True, True)
        if nb == 1:
            r = torch.zeros((batch, 1), dtype=at.dtype, device=at.device)
    return F._wrap(q, A._np_dtype), F._wrap(r, A._np_dtype)


def poly_powmod_batched(A: FieldArray, e: int, c) -> FieldArray:
    """Device extension: pow(Poly(row), e, c) for every row of a (batch, n) array of coefficients in one call (one launch up to
    the degree powmod_max_degree).  Returns the (batch, max(deg c, 1)) untrimmed coefficients."""
    F, c = _stack_and_divisor(A, c, "c")
    if not isinstance(e, (int, np.integer)):
        raise TypeError(f"Argument 'e' must be an instance of {int}, not {type(e)}.")
    if not e >= 0:
        raise ValueError(f"Can only exponentiate polynomials to non-negative integers, not {e}.")
    if _is_zero(c):
        raise ZeroDivisionError("Cannot reduce a polynomial modulo zero.")
    e = int(e)
    batch = A.shape[0]
    d = max(c.degree, 1)
    if c.degree == 0 or e == 0:  # the reference's conventions: 0 modulo a unit, and f^0 = 1 whatever the modulus
        out = _rows(F, A, lambda row: F.Zeros(1) if e else F.Ones(1), d) if F._limbed else None
        if out is None:
            t = torch.zeros((batch, d), dtype=A._t.dtype, device=A._t.device)
            if e == 0:
                t[:, d - 1] = 1
            out = F._wrap(t, A._np_dtype)
        return out
    if F._limbed or d > powmod_max_degree(F):
        return _rows(F, A, lambda row: _powmod_1d(row, e, c.coeffs), d)
    return F._wrap(_powmod_t(F, A._t.contiguous(), e, A._same_storage(c.coeffs).contiguous()), A._np_dtype)
