"""
Roots of polynomials, and polynomials from their roots.  Paths relative to /root/reference/src/galois:

  * Poly.roots(multiplicity=False) ... _polys/_poly.py:706-787 over roots_jit (_polys/_dense.py:443-513) and _root_multiplicity
                                       (_polys/_poly.py:1672-1698)
  * Poly.Roots(roots, multiplicities, field) ... _polys/_poly.py:536-612

The reference evaluates the polynomial at all q elements (Chien search) and then finds the multiplicities one root at a time.
There are two routes here, with identical results:

  search   one gfa_poly_roots call (galois_amd/csrc/gfa_polyroots.hip): a kernel that makes the q candidates from its index,
           evaluates and keeps the hits, and a finishing kernel that sorts them and finds all multiplicities at once.  Its work
           is q * degree evaluation steps per polynomial.
  split    algebra on what Poly already has: g = gcd(f, x^q - x mod f) is the product of (x - r) over the distinct roots
           (pow(x, q, f) and gcd are one fused launch each), g.equal_degree_factors(1) splits it, and a root is minus the
           constant term of a factor.  Its work does not grow with q beyond the log q squarings, so it takes over where the
           search's work passes SEARCH_MAX_WORK, and it is the only route over fields of order >= 2^64.

Multiplicities of roots that are already known (_root_multiplicity, the seam the reference has under the same name) come from the
finishing kernel alone (gfa_poly_root_multiplicity), and over fields of order >= 2^64 from divmod by (x - r) while it is exact.
poly_roots_batched exposes the stack the kernels take.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from ._array import FieldArray, _GFA_DTYPE, _ptr, _stream
from ._poly import Poly
from ._polydiv import POW_LDS_BYTES, _elem_bytes, _is_zero, _one, _zero
from ._polygcd import poly_gcd

# The default route is the search while q * degree * rows stays at or below this.  Measured on an MI355X (tools/bench_polyroots.py,
# profiles/polyroots_time.txt): over q in {2^8 .. 2^32} and degrees {4, 16, 64, 256} the search was the faster route at every
# point up to q * degree = 2^32 (2^24 * 256) and the split route at every point from 2^33 ((2^31 - 1) * 4); this is the largest
# power of two below that crossover.  (Per degree the two meet near q = 2^25 .. 2^28: DESIGN.md section 4.7.)
SEARCH_MAX_WORK = 2**32


def roots_max_terms(field) -> int:
    """Largest number of coefficients of a row gfa_poly_roots and gfa_poly_root_multiplicity serve over the field (PR_MAX_TERMS):
    the finishing kernel holds the row, its roots twice and one quotient in LDS."""
    return POW_LDS_BYTES // _elem_bytes(field) // 4


# ---- the kernels on contiguous storage tensors ---------------------------------------------------------------------------------
def _roots_t(field, c: torch.Tensor, want_mult: bool):
    """(roots, counts, multiplicities or None) of the rows of c (batch, ncoef >= 2): (batch, ncoef - 1) sorted roots and int32
    multiplicities, zero-filled, and int64 counts (-1 for a zero row)."""
    batch, ncoef = c.shape
    roots = torch.empty((batch, ncoef - 1), dtype=c.dtype, device=c.device)
    counts = torch.empty(batch, dtype=torch.int64, device=c.device)
    mult = torch.empty((batch, ncoef - 1), dtype=torch.int32, device=c.device) if want_mult else None
    L.check(L.lib().gfa_poly_roots(field._handle, _ptr(c), batch, ncoef, _ptr(roots), _ptr(mult) if want_mult else None, _ptr(counts),
                                   _GFA_DTYPE[c.element_size()], _stream()), "gfa_poly_roots")
    return roots, counts, mult


def _mult_t(field, c: torch.Tensor, r: torch.Tensor) -> torch.Tensor:
    """int32 (batch, nroots): the multiplicity of r[k][j] as a root of row k of c (batch, ncoef)."""
    batch, ncoef = c.shape
    mult = torch.empty(r.shape, dtype=torch.int32, device=c.device)
    L.check(L.lib().gfa_poly_root_multiplicity(field._handle, _ptr(c), batch, ncoef, _ptr(r), r.shape[1], _ptr(mult), _GFA_DTYPE[c.element_size()],
                                               _stream()), "gfa_poly_root_multiplicity")
    return mult


def _search_serves(F, ncoef: int) -> bool:
    """Do the kernels take rows of ncoef coefficients over the field?"""
    return not F._limbed and ncoef <= roots_max_terms(F)


def _empty(F, like: FieldArray) -> FieldArray:
    return F.Zeros(0) if F._limbed else F._wrap(torch.empty(0, dtype=like._t.dtype, device=like._t.device), like._np_dtype)


def _elements(F, values: list, like: FieldArray) -> FieldArray:
    """A 1-D array of the field from Python integers, in the storage of `like`."""
    if not values:
        return _empty(F, like)
    arr = F(np.array(values, dtype=object))
    return arr if F._limbed else F._wrap(like._same_storage(arr), like._np_dtype)


# ---- multiplicities of given roots -----------------------------------------------------------------------------------------------
def _root_multiplicity(f: Poly, roots: FieldArray) -> np.ndarray:
    """The multiplicity of every element of the 1-D array `roots` as a root of the non-zero f (0 for an element that is none): all
    of them in one launch of the finishing kernel; over fields of order >= 2^64, and above the kernel's cap, by divmod."""
    F = f.field
    if roots.size == 0:
        return np.zeros(0, dtype=np.int64)
    if _search_serves(F, f.coeffs.size):
        c = f.coeffs._t.contiguous().reshape(1, -1)
        r = f.coeffs._same_storage(roots).contiguous().reshape(1, -1)
        return _mult_t(F, c, r)[0].cpu().numpy().astype(np.int64)
    out = []
    one = _one(F, f.coeffs)
    for k in range(roots.size):
        lin = Poly(np.concatenate([one, -roots[k:k + 1]]))
        m, p = 0, f
        while p.degree >= 1:
            quo, rem = divmod(p, lin)
            if not _is_zero(rem):
                break
            m, p = m + 1, quo
        out.append(m)
    return np.array(out, dtype=np.int64)


# ---- the two routes ----------------------------------------------------------------------------------------------------------------
def _roots_search(f: Poly, multiplicity: bool):
    F = f.field
    roots, counts, mult = _roots_t(F, f.coeffs._t.contiguous().reshape(1, -1), multiplicity)
    n = int(counts.item())
    r = F._wrap(roots[0, :n].contiguous(), f.coeffs._np_dtype)
    return (r, mult[0, :n].cpu().numpy().astype(np.int64)) if multiplicity else r


def _roots_split(f: Poly, multiplicity: bool):
    F = f.field
    lead = f.coeffs[:1]
    monic = f if int(lead[0]) == 1 else f // Poly(lead)
    if monic.degree == 1:
        g = monic
    else:
        x = Poly(np.concatenate([_one(F, f.coeffs), _zero(F, f.coeffs)]))
        g = poly_gcd(monic, pow(x, F.order, monic) - x)  # the product of (x - r) over the distinct roots
    if g.degree == 0:
        linear = []
    elif g.degree == 1:
        linear = [g]
    else:
        linear = g.equal_degree_factors(1)
    if linear:
        consts = F(np.array([int(p.coeffs[1]) for p in linear], dtype=object))
        values = sorted(int(v) for v in (-consts).numpy())
    else:
        values = []
    r = _elements(F, values, f.coeffs)
    return (r, _root_multiplicity(f, r)) if multiplicity else r


def poly_roots(f: Poly, multiplicity: bool = False, method: str | None = None):
    """Poly.roots (_polys/_poly.py:706-787): the distinct roots of f in its field, in increasing order; with `multiplicity` also their
    multiplicities as an integer np.ndarray.  A non-zero constant has none; of the zero polynomial every element is a root, which
    is a ValueError here.  `method` ("search" or "split") overrides the choice of the route, for tests."""
    if not isinstance(multiplicity, bool):
        raise TypeError(f"Argument 'multiplicity' must be an instance of {bool}, not {type(multiplicity)}.")
    if method not in (None, "search", "split"):
        raise ValueError(f"Argument 'method' must be in ['search', 'split'], not {method!r}.")
    F = f.field
    if _is_zero(f):
        raise ValueError("Every element of the field is a root of the zero polynomial.")
    if f.degree == 0:
        r = _empty(F, f.coeffs)
        return (r, np.zeros(0, dtype=np.int64)) if multiplicity else r
    if method is None:
        method = "search" if _search_serves(F, f.coeffs.size) and F.order * f.degree <= SEARCH_MAX_WORK else "split"
    return _roots_search(f, multiplicity) if method == "search" else _roots_split(f, multiplicity)


def poly_roots_batched(A: FieldArray, multiplicity: bool = False):
    """Device extension: the roots of Poly(A[k]) for every row of a (batch, n) stack of coefficients, highest degree first (leading
    zeros allowed).  Returns (roots, counts) or (roots, counts, multiplicities): `roots` is (batch, max(n - 1, 0)) over the field,
    row k holding its roots in increasing order and then zeros; `counts` is an int64 np.ndarray with -1 for a zero row;
    `multiplicities` is an int32 np.ndarray shaped like `roots`, 0 in the fill.  One gfa_poly_roots call where the search's work
    q * (n - 1) * batch is within SEARCH_MAX_WORK, and the split route row by row otherwise."""
    if not isinstance(A, FieldArray):
        raise TypeError(f"Argument 'A' must be a FieldArray, not {type(A)}.")
    if not (A.ndim == 2 and A.shape[1] >= 1):
        raise ValueError(f"Argument 'A' must be 2-D with one polynomial per row, highest degree first, not have shape {tuple(A.shape)}.")
    if not isinstance(multiplicity, bool):
        raise TypeError(f"Argument 'multiplicity' must be an instance of {bool}, not {type(multiplicity)}.")
    F = type(A)
    batch, n = A.shape
    cap = n - 1
    if batch and n >= 2 and _search_serves(F, n) and F.order * cap * batch <= SEARCH_MAX_WORK:
        roots, counts, mult = _roots_t(F, A._t.contiguous(), multiplicity)
        out = (F._wrap(roots, A._np_dtype), counts.cpu().numpy())
        return out + (mult.cpu().numpy(),) if multiplicity else out
    if F._limbed:
        roots = F.Zeros((batch, cap))
    else:
        roots = F._wrap(torch.zeros((batch, cap), dtype=A._t.dtype, device=A._t.device), A._np_dtype)
    counts = np.zeros(batch, dtype=np.int64)
    mult = np.zeros((batch, cap), dtype=np.int32)
    for k in range(batch):
        p = Poly(A[k])
        if _is_zero(p):
            counts[k] = -1
        elif p.degree >= 1:
            r, m = _roots_split(p, True) if multiplicity else (_roots_split(p, False), None)
            counts[k] = r.size
            if r.size:
                roots[k, :r.size] = r
            if multiplicity:
                mult[k, :r.size] = m
    return (roots, counts, mult) if multiplicity else (roots, counts)


# ---- Poly.Roots ----------------------------------------------------------------------------------------------------------------------
def Roots(cls, roots, multiplicities=None, field=None) -> Poly:
    """Poly.Roots (_polys/_poly.py:536-612): the monic polynomial prod (x - r_i)^(m_i)."""
    multiplicities = [1] * len(roots) if multiplicities is None else multiplicities
    if not isinstance(roots, (tuple, list, np.ndarray, FieldArray)):
        raise TypeError(f"Argument 'roots' must be an instance of {(tuple, list, np.ndarray, FieldArray)}, not {type(roots)}.")
    if not isinstance(multiplicities, (tuple, list, np.ndarray)):
        raise TypeError(f"Argument 'multiplicities' must be an instance of {(tuple, list, np.ndarray)}, not {type(multiplicities)}.")
    if not (field is None or (isinstance(field, type) and issubclass(field, FieldArray))):
        raise TypeError(f"Argument 'field' must be a FieldArray subclass, not {field}.")
    if isinstance(roots, FieldArray):  # _convert_coeffs (_polys/_poly.py:1650-1669)
        if field is None:
            field = type(roots)
        elif type(roots) is not field:
            roots = field(np.array([int(v) for v in roots.numpy().ravel()], dtype=object))
        r = roots.flatten()
    else:
        if field is None:
            from ._factory import GF

            field = GF(2)
        ints = [int(v) for v in np.array(roots, dtype=object).ravel()]
        r = field(np.array([abs(v) for v in ints], dtype=object))
        if any(v < 0 for v in ints):  # "-r" stands for the negative of the element r
            neg = -r
            for k, v in enumerate(ints):
                if v < 0:
                    r[k] = neg[k]
    if not r.size == len(multiplicities):
        raise ValueError(f"Arguments 'roots' and 'multiplicities' must have the same length, not {r.size} and {len(multiplicities)}.")
    one = field.Ones(1) if r.size == 0 else _one(field, r)
    poly = cls(one)
    neg = -r if r.size else r
    for k, m in enumerate(multiplicities):
        poly = poly * cls(np.concatenate([one, neg[k:k + 1]])) ** m
    return poly


def _method_roots(self, multiplicity=False, method=None):
    return poly_roots(self, multiplicity, method)


_method_roots.__doc__ = poly_roots.__doc__
Poly.roots = _method_roots
Poly.Roots = classmethod(Roots)
