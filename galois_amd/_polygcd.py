"""
Greatest common divisors of polynomials, and the functions that stand on them.  Paths relative to /root/reference/src/galois:

  * gcd(a, b), egcd(a, b), lcm(*polys), prod(*polys) ... _polys/_functions.py:10-94, polymorphic over int arguments as
                                                         _polymorphic.py:38-301 (over _math.py:12-69)

The reference's Euclid is a loop over `%` (or `//`, `*`, `-`): one remainder, and one look at `r1 != 0`, per step.  The kernel
(galois_amd/csrc/gfa_polygcd.hip) runs the whole remainder sequence of a pair in one launch, for a stack of pairs at once; gcd and
egcd are the batch-of-one case and poly_gcd_batched / poly_egcd_batched expose the stacks.  The kernel holds the remainders (and the
cofactors) in LDS, which caps na + nb (gcd_max_terms); above the cap, and over fields of order >= 2^64, which have no kernel, the
same Euclid runs here as a loop over the operators of Poly.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib as L
from ._array import FieldArray, _ptr, _stream
from ._polydiv import POW_LDS_BYTES, _elem_bytes, _is_zero, _one, _zero

GCD_SLOT_BYTES = 8  # the workgroup-reduction word in front of the coefficients (PG_SLOT_BYTES)


def gcd_max_terms(field, extended: bool = False) -> int:
    """Largest na + nb (coefficients of the two operands together) gfa_poly_gcd serves over the field (PG_MAX_TERMS): the two
    remainders fill na + nb elements of LDS, and with cofactors (`extended`) two of each width more."""
    return (POW_LDS_BYTES - GCD_SLOT_BYTES) // _elem_bytes(field) // (3 if extended else 1)


def _make_poly(F, coeffs: FieldArray):
    """A Poly from coefficients known to be trimmed (no look at the device)."""
    from ._poly import Poly

    p = object.__new__(Poly)
    p._field = F
    p._coeffs = coeffs
    return p


# ---- the kernel on contiguous storage tensors ----------------------------------------------------------------------------------
def _gcd_t(field, a: torch.Tensor, b: torch.Tensor, extended: bool):
    """(g, s, t, deg) for the rows of a (batch, na) and of b (batch, nb) or (1, nb): (batch, max(na, nb)) right-aligned coefficients
    and the int32 degrees of the gcds (-1 for zero); s and t are None unless `extended`.  na + nb <= gcd_max_terms."""
    from ._array import _GFA_DTYPE

    batch, na = a.shape
    rows, nb = b.shape
    n = max(na, nb)
    g = torch.empty((batch, n), dtype=a.dtype, device=a.device)
    s = torch.empty_like(g) if extended else None
    t = torch.empty_like(g) if extended else None
    deg = torch.empty(batch, dtype=torch.int32, device=a.device)
    L.check(L.lib().gfa_poly_gcd(field._handle, _ptr(a), batch, na, _ptr(b), rows, nb, _ptr(g), _ptr(s) if extended else None,
                                 _ptr(t) if extended else None, _ptr(deg), _GFA_DTYPE[a.element_size()], _stream()), "gfa_poly_gcd")
    return g, s, t, deg


def _served(F, na: int, nb: int, extended: bool) -> bool:
    return not F._limbed and na + nb <= gcd_max_terms(F, extended)


# ---- Euclid on the operators (fields without a kernel, operands above the cap) --------------------------------------------------
def _euclid_host(a, b, extended: bool):
    """gcd / egcd as _functions.py:17-26 / :40-57 on the operators of Poly."""
    from ._poly import Poly

    F = a.field
    r2, r1 = a, b
    if extended:
        zero, one = Poly(_zero(F, a.coeffs)), Poly(_one(F, a.coeffs))
        s2, s1, t2, t1 = one, zero, zero, one
    while not _is_zero(r1):
        if extended:
            q = r2 // r1
            r2, r1 = r1, r2 - q * r1
            s2, s1 = s1, s2 - q * s1
            t2, t1 = t1, t2 - q * t1
        else:
            r2, r1 = r1, r2 % r1
    c = Poly(r2.coeffs[:1])  # the leading coefficient
    if int(r2.coeffs[0]) > 1:
        r2 = r2 // c
        if extended:
            s2, t2 = s2 // c, t2 // c
    return (r2, s2, t2) if extended else (r2, None, None)


def _same_field(a, b):
    if a.field is not b.field:
        raise ValueError(f"Polynomials 'a' and 'b' must be over the same Galois field, not {a.field} and {b.field}.")


def _from_row(F, like: FieldArray, row: torch.Tensor, length: int):
    """The Poly whose max(length, 1) coefficients end the row."""
    return _make_poly(F, F._wrap(row[row.numel() - max(length, 1):], like._np_dtype))


def _poly_euclid(a, b, extended: bool):
    F = a.field
    na, nb = a.coeffs.size, b.coeffs.size
    if not _served(F, na, nb, extended):
        return _euclid_host(a, b, extended)
    at = a.coeffs._t.contiguous().reshape(1, -1)
    bt = a.coeffs._same_storage(b.coeffs).contiguous().reshape(1, -1)
    g, s, t, deg = _gcd_t(F, at, bt, extended)
    d = int(deg.item())
    gp = _from_row(F, a.coeffs, g[0], d + 1)
    if not extended:
        return gp, None, None
    # deg s < deg b and deg t < deg a: the columns in front are zero
    from ._poly import Poly

    return gp, Poly(F._wrap(s[0], a.coeffs._np_dtype)), Poly(F._wrap(t[0], a.coeffs._np_dtype))


def poly_gcd(a, b):
    """gcd of two Poly (_functions.py:10-26): monic, gcd(0, 0) = 0."""
    _same_field(a, b)
    return _poly_euclid(a, b, False)[0]


def poly_egcd(a, b):
    """egcd of two Poly (_functions.py:29-57): (d, s, t) with a s + b t = d."""
    _same_field(a, b)
    return _poly_euclid(a, b, True)


def _gcd_many(us: list, g) -> list:
    """gcd(u, g) for every Poly u of a list and one Poly g: one launch on the stack of the u (right-aligned rows), and the host
    reads back their degrees only."""
    F = g.field
    if not us:
        return []
    n = max(u.coeffs.size for u in us)
    if not _served(F, n, g.coeffs.size, False):
        return [poly_gcd(u, g) for u in us]
    like = g.coeffs
    U = torch.zeros((len(us), n), dtype=like._t.dtype, device=like._t.device)
    for k, u in enumerate(us):
        U[k, n - u.coeffs.size:] = like._same_storage(u.coeffs)
    G, _, _, deg = _gcd_t(F, U, like._t.contiguous().reshape(1, -1), False)
    return [_from_row(F, like, G[k], d + 1) for k, d in enumerate(deg.cpu().tolist())]


# ---- the polymorphic functions (_polymorphic.py) ----------------------------------------------------------------------------------
def _all_ints(values) -> bool:
    return all(isinstance(v, (int, np.integer)) for v in values)


def _all_polys(values) -> bool:
    from ._poly import Poly

    return all(isinstance(v, Poly) for v in values)


def gcd(a, b):
    """galois.gcd (_polymorphic.py:38-94): the greatest common divisor of two integers or of two polynomials (monic)."""
    if _all_ints((a, b)):
        return math.gcd(int(a), int(b))
    if _all_polys((a, b)):
        return poly_gcd(a, b)
    raise TypeError(f"Arguments 'a' and 'b' must both be either int or galois.Poly, not {type(a)} and {type(b)}.")


def _int_egcd(a: int, b: int):
    r2, r1, s2, s1, t2, t1 = a, b, 1, 0, 0, 1
    while r1 != 0:
        q = r2 // r1
        r2, r1 = r1, r2 - q * r1
        s2, s1 = s1, s2 - q * s1
        t2, t1 = t1, t2 - q * t1
    if r2 < 0:
        r2, s2, t2 = -r2, -s2, -t2
    return r2, s2, t2


def egcd(a, b):
    """galois.egcd (_polymorphic.py:106-172): (d, s, t) with a s + b t = d = gcd(a, b)."""
    if _all_ints((a, b)):
        return _int_egcd(int(a), int(b))
    if _all_polys((a, b)):
        return poly_egcd(a, b)
    raise TypeError(f"Arguments 'a' and 'b' must both be either int or galois.Poly, not {type(a)} and {type(b)}.")


def _one_field(values):
    field = values[0].field
    for v in values:
        if v.field is not field:
            raise ValueError(f"All polynomial arguments must be over the same field, not {[v.field for v in values]}.")
    return field


def lcm(*values):
    """galois.lcm (_polymorphic.py:184-237): the least common multiple of integers (positive) or polynomials (monic)."""
    from ._poly import Poly

    if not len(values) > 0:
        raise ValueError("At least one argument must be provided.")
    if _all_ints(values):
        return math.lcm(*[int(v) for v in values])
    if not _all_polys(values):
        raise TypeError(f"All arguments must be either int or galois.Poly, not {[type(value) for value in values]}.")
    F = _one_field(values)
    out = Poly(_one(F, values[0].coeffs))
    for v in values:
        out = (out * v) // poly_gcd(out, v)
    return out // Poly(out.coeffs[:1])


def prod(*values):
    """galois.prod (_polymorphic.py:249-301): the product of integers or of polynomials."""
    from ._poly import Poly

    if not len(values) > 0:
        raise ValueError("At least one argument must be provided.")
    if _all_ints(values):
        return math.prod(int(v) for v in values)
    if not _all_polys(values):
        raise TypeError(f"All arguments must be either int or galois.Poly, not {[type(value) for value in values]}.")
    F = _one_field(values)
    out = Poly(_one(F, values[0].coeffs))
    for v in values:
        out = out * v
    return out


# ---- the batched forms ----------------------------------------------------------------------------------------------------------
def _stacks(A, B):
    """(field, A, B as a 2-D array of one row or of A's row count)."""
    from ._poly import Poly

    if not isinstance(A, FieldArray):
        raise TypeError(f"Argument 'A' must be a FieldArray, not {type(A)}.")
    if not (A.ndim == 2 and A.shape[1] >= 1):
        raise ValueError(f"Argument 'A' must be 2-D with one polynomial per row, highest degree first, not have shape {tuple(A.shape)}.")
    F = type(A)
    if isinstance(B, Poly):
        if B.field is not F:
            raise TypeError(f"Argument 'B' must be over {F.name}, not {B.field.name}.")
        B = B.coeffs
    if not (isinstance(B, FieldArray) and type(B) is F):
        raise TypeError(f"Argument 'B' must be a Poly, a 1-D array or a 2-D stack over {F.name}, not {type(B)}.")
    if B.ndim == 1 and B.size >= 1:
        B = B.reshape((1, B.size))
    if not (B.ndim == 2 and B.shape[1] >= 1 and B.shape[0] in (1, A.shape[0])):
        raise ValueError(f"Argument 'B' must be one polynomial or one per row of 'A' ({A.shape[0]}), not have shape {tuple(B.shape)}.")
    return F, A, B


def _batched(A, B, extended: bool):
    from ._poly import Poly

    F, A, B = _stacks(A, B)
    batch, na = A.shape
    nb = B.shape[1]
    n = max(na, nb)
    if _served(F, na, nb, extended):
        g, s, t, _ = _gcd_t(F, A._t.contiguous(), A._same_storage(B).contiguous(), extended)
        wrap = lambda x: F._wrap(x, A._np_dtype)
        return (wrap(g), wrap(s), wrap(t)) if extended else (wrap(g), None, None)
    # the same Euclid on the operators, row by row
    if F._limbed:
        outs = [F.Zeros((batch, n)) for _ in range(3 if extended else 1)]
    else:
        outs = [F._wrap(torch.zeros((batch, n), dtype=A._t.dtype, device=A._t.device), A._np_dtype) for _ in range(3 if extended else 1)]
    for k in range(batch):
        res = _euclid_host(Poly(A[k]), Poly(B[k if B.shape[0] > 1 else 0]), extended)
        for out, p in zip(outs, res):
            out[k, n - p.coeffs.size:] = p.coeffs
    return (outs[0], outs[1], outs[2]) if extended else (outs[0], None, None)


def poly_gcd_batched(A: FieldArray, B) -> FieldArray:
    """Device extension: gcd(Poly(A[k]), Poly(B[k])) for every row of two (batch, n) stacks of coefficients, highest degree first
    (leading zeros allowed), in one launch; `B` may also be one Poly or 1-D array shared by all rows.  Returns the monic gcds as
    (batch, max(na, nb)) coefficients, right-aligned and zero-filled on the left."""
    return _batched(A, B, False)[0]


def poly_egcd_batched(A: FieldArray, B):
    """Device extension: egcd of every pair of rows, as poly_gcd_batched: (G, S, T), each (batch, max(na, nb)) right-aligned, with
    Poly(A[k]) Poly(S[k]) + Poly(B[k]) Poly(T[k]) = Poly(G[k])."""
    return _batched(A, B, True)
