"""
Primitive and normal elements of GF(q^m) = GF(q)[x] / (f(x)) for an irreducible polynomial f.  Paths relative to
/root/reference/src/galois:

  * is_primitive_element / primitive_element / primitive_elements ... _fields/_primitive_element.py:18-410
  * is_normal_element / normal_element / normal_elements ............. _fields/_normal_element.py:17-411
  * GF.primitive_elements / GF.normal_element / GF.normal_elements ... _fields/_meta.py:311-431 (the properties are on
                                                                       FieldArrayMeta, galois_amd/_array.py)

The reference tests one residue after the other: pow(Poly, k, f) for every prime divisor of q^m - 1, and m - 1 modular powers
plus a rank for normality.  Here one gfa_poly_element_classify call (galois_amd/csrc/gfa_polyelem.hip) classifies a whole chunk
of residues.  Candidates of the searches and enumerations are integer ranges turned into radix-q digits on the device, as in
galois_amd/_polysearch.py; "min" and "max" classify chunks that grow geometrically.

What the kernel needs per (field, f) is built once and kept on the device (_constants): the cofactor exponents
(q^m - 1) / r, and for normality the matrices c_i(Phi), where Phi is the matrix of the q-th power on residues (its columns
x^(q j) mod f from one poly_powmod_batched call), x^m - 1 = prod P_i^(e_i) (Poly.factors) and c_i = (x^m - 1) / P_i is
evaluated at Phi by Horner's rule with matrix products.  g is normal iff no c_i(Phi) sends its coefficient vector to zero --
GF(q^m) is a cyclic GF(q)[x]-module through Phi with annihilator x^m - 1 -- which is the reference's rank criterion without an
elimination per candidate.
"""
from __future__ import annotations

import random

import numpy as np
import torch

from . import _lib as L
from ._array import _GFA_DTYPE, FieldArray, _ptr, _stream, _to_storage
from ._poly import Poly
from ._polysearch import MAX_DEGREE, MAX_DEGREE_GF2, _cofactor_exponents, _ints_to_tensor, _range_tensor, _storage

PRIMITIVE, NORMAL = 1, 2


def _check_limits(field, degree: int, what: str):
    if field._limbed:
        raise NotImplementedError(
            f"The {what} element test is not implemented for polynomials over {field.name}: gfa_poly_element_classify serves fields "
            "of order below 2^64."
        )
    limit = MAX_DEGREE_GF2 if field.order == 2 else MAX_DEGREE
    if degree > limit:
        raise NotImplementedError(
            f"The {what} element test is not implemented for degree {degree} over {field.name}: gfa_poly_element_classify serves "
            f"degrees up to {MAX_DEGREE_GF2} over GF(2) and up to {MAX_DEGREE} over every other field."
        )


# ---- per-field constants -----------------------------------------------------------------------------------------------------
class _Constants:
    """What the kernel needs for one monic irreducible f: f itself and, built on first use, the cofactor matrices; on the device.
    The entry point reads the residues, the modulus and the matrices through ONE storage type: everything here is held in the
    field's default storage (_storage), whatever dtype the caller's polynomial came in, and _classify takes residues of that
    width only."""

    def __init__(self, f: Poly):
        field = f.field
        np_dtype, tdt = _storage(field)
        self.field = field
        self.m = f.degree
        self.f_t = _to_storage(f.coeffs._t, tdt).contiguous()
        self.f = Poly._from_trimmed(field, field._wrap(self.f_t, np_dtype))
        self._mats = None

    @property
    def exponents(self):
        return _cofactor_exponents(self.field.order, self.m)

    @property
    def mats(self) -> torch.Tensor:
        """(n_mats, m, m) storage tensor: c_i(Phi) for the distinct irreducible factors P_i of x^m - 1, row-major, acting on
        ascending coefficient vectors."""
        if self._mats is None:
            from ._polydiv import poly_powmod_batched

            field, m = self.field, self.m
            np_dtype = self.f.coeffs._np_dtype
            tdt = self.f_t.dtype
            # row j = x^j, highest degree first; one launch raises them all to the q-th power
            rows = field._wrap(torch.flip(torch.eye(m, dtype=tdt, device=self.f_t.device), dims=(1,)).contiguous(), np_dtype)
            powers = poly_powmod_batched(rows, field.order, self.f)._t  # row j = x^(q j) mod f, highest degree first
            phi = field._wrap(torch.flip(powers, dims=(1,)).T.contiguous(), np_dtype)  # column j = x^(q j), ascending rows
            minus_one = field.characteristic - 1
            xm1 = Poly(field(np.array([1] + [0] * (m - 1) + [minus_one], dtype=object))) if m > 1 else Poly(field([1, minus_one]))
            factors, _ = xm1.factors()
            mats = []
            for p in factors:
                c = xm1 // p
                mats.append(phi._same_storage(c(phi, elementwise=False)).contiguous())
            self._mats = torch.stack(mats).contiguous()
        return self._mats


_CONSTANTS: dict[tuple, _Constants] = {}
_IRREDUCIBLE: dict[tuple, bool] = {}


def _is_irreducible(f: Poly) -> bool:
    key = (f.field, int(f))
    if key not in _IRREDUCIBLE:
        if len(_IRREDUCIBLE) > 4096:
            _IRREDUCIBLE.clear()
        _IRREDUCIBLE[key] = f.is_irreducible()
    return _IRREDUCIBLE[key]


def _constants(f: Poly) -> _Constants:
    """The constants of the monic multiple of f (the residue ring is the same)."""
    field = f.field
    lead = f.coeffs[0]
    if int(lead) != 1:
        f = Poly(f.coeffs * np.reciprocal(lead))
    key = (field, int(f))
    if key not in _CONSTANTS:
        if len(_CONSTANTS) > 256:
            _CONSTANTS.clear()
        _CONSTANTS[key] = _Constants(f)
    return _CONSTANTS[key]


def _classify(consts: _Constants, t: torch.Tensor, primitive: bool, normal: bool) -> torch.Tensor:
    """Flags (uint8, on the device) of the rows of a contiguous (batch, m) storage tensor of residues."""
    field = consts.field
    batch = t.shape[0]
    flags = torch.empty(batch, dtype=torch.uint8, device=t.device)
    n_exps, limbs, exps = consts.exponents if primitive else (0, 0, None)
    mats = consts.mats if normal else None
    if t.dtype != consts.f_t.dtype or (normal and mats.dtype != t.dtype) or not t.is_contiguous():
        raise TypeError(f"residues of storage type {t.dtype} against constants of {consts.f_t.dtype}")  # (a fault of this module)
    L.check(L.lib().gfa_poly_element_classify(field._handle, _ptr(t), batch, _ptr(consts.f_t), consts.m, _GFA_DTYPE[t.element_size()],
                                              exps, n_exps, limbs, _ptr(mats) if normal else None, mats.shape[0] if normal else 0,
                                              _ptr(flags), _stream()), "gfa_poly_element_classify")
    return flags


# ---- arguments ---------------------------------------------------------------------------------------------------------------
def _verify_poly(irreducible_poly) -> Poly:
    from ._factory import GF, IrreduciblePoly

    if isinstance(irreducible_poly, IrreduciblePoly):  # what GF.irreducible_poly returns: a polynomial over the prime subfield
        return Poly.Int(int(irreducible_poly), field=GF(irreducible_poly._p))
    if not isinstance(irreducible_poly, Poly):
        raise TypeError(f"Argument 'irreducible_poly' must be an instance of {Poly}, not {type(irreducible_poly)}.")
    return irreducible_poly


def _verify_irreducible(f: Poly):
    if not _is_irreducible(f):
        raise ValueError(f"Argument 'irreducible_poly' must be irreducible, {f} is reducible over {f.field.name}.")


def _element_like(element, field) -> Poly:
    """Poly.Like(element, field=field) for the forms this package has: a Poly, an integer (Poly.Int), or coefficients."""
    if isinstance(element, Poly):
        return element
    if isinstance(element, (int, np.integer)) and not isinstance(element, bool):
        return Poly.Int(int(element), field=field)
    if isinstance(element, FieldArray):
        if type(element) is not field:
            raise ValueError(
                f"Arguments 'element' and 'irreducible_poly' must be over the same field, not {type(element).name} and {field.name}."
            )
        return Poly(element)
    if isinstance(element, (list, tuple, np.ndarray)):
        return Poly(element, field=field)
    raise TypeError(f"Argument 'element' must be a Poly, an int or a sequence of coefficients, not {type(element)}.")


def _is_element(element, irreducible_poly, primitive: bool) -> bool:
    f = _verify_poly(irreducible_poly)
    field = f.field
    element = _element_like(element, field)
    if element.field is not field:
        raise ValueError(
            f"Arguments 'element' and 'irreducible_poly' must be over the same field, not {element.field.name} and {field.name}."
        )
    if not element.degree < f.degree:
        raise ValueError(
            f"Argument 'element' must have degree less than 'irreducible_poly', not degrees {element.degree} and {f.degree}."
        )
    _verify_irreducible(f)
    _check_limits(field, f.degree, "primitive" if primitive else "normal")
    consts = _constants(f)
    t = consts.f_t.new_zeros((1, consts.m))
    c = _to_storage(element.coeffs._t, t.dtype)  # the constants' width, whatever dtype the element or f came in
    t[0, consts.m - c.numel():] = c
    flag = int(_classify(consts, t, primitive, not primitive).item())
    return bool(flag & (PRIMITIVE if primitive else NORMAL))


def is_primitive_element(element, irreducible_poly) -> bool:
    """galois.is_primitive_element (_fields/_primitive_element.py:18-134): does the residue class of `element` generate the
    multiplicative group of GF(q)[x] / (irreducible_poly)?  `element` is a Poly, an int (Poly.Int) or coefficients, highest degree
    first."""
    return _is_element(element, irreducible_poly, True)


def is_normal_element(element, irreducible_poly) -> bool:
    """galois.is_normal_element (_fields/_normal_element.py:17-140): are the conjugates g, g^q, .., g^(q^(m-1)) of the residue
    class of `element` a basis of GF(q^m) over GF(q)?"""
    return _is_element(element, irreducible_poly, False)


def _batched(elements, irreducible_poly, primitive: bool) -> np.ndarray:
    f = _verify_poly(irreducible_poly)
    if not isinstance(elements, FieldArray):
        raise TypeError(f"Argument 'elements' must be a FieldArray, not {type(elements)}.")
    field = f.field
    if type(elements) is not field:
        raise ValueError(
            f"Arguments 'elements' and 'irreducible_poly' must be over the same field, not {type(elements).name} and {field.name}."
        )
    _check_limits(field, f.degree, "primitive" if primitive else "normal")
    if not (elements.ndim == 2 and elements.shape[1] == f.degree):
        raise ValueError(
            f"Argument 'elements' must be 2-D with one residue per row, {f.degree} coefficients, highest degree first, "
            f"not have shape {tuple(elements.shape)}."
        )
    _verify_irreducible(f)
    consts = _constants(f)
    t = _to_storage(elements._t, consts.f_t.dtype).contiguous()
    flags = _classify(consts, t, primitive, not primitive).cpu().numpy()
    return (flags & (PRIMITIVE if primitive else NORMAL)) != 0


def is_primitive_element_batched(elements: FieldArray, irreducible_poly) -> np.ndarray:
    """Device extension: is_primitive_element of every row of a (batch, m) array of coefficients, highest degree first, modulo one
    irreducible polynomial of degree m, in one call.  Returns a NumPy bool array."""
    return _batched(elements, irreducible_poly, True)


def is_normal_element_batched(elements: FieldArray, irreducible_poly) -> np.ndarray:
    """Device extension: is_normal_element of every row of a (batch, m) array of coefficients."""
    return _batched(elements, irreducible_poly, False)


# ---- searches and enumerations -------------------------------------------------------------------------------------------------
def _residues(field, m: int, k0: int, n: int) -> torch.Tensor:
    """The residues with the integers k0 .. k0 + n - 1 (k0 + n <= q^m) as a contiguous (n, m) storage tensor."""
    return _range_tensor(field, m, k0, n)[:, 1:].contiguous()


def _polys_from_rows(field, rows: torch.Tensor) -> list:
    """Poly objects of the rows of a (k, m) storage tensor, none of them zero; the trim offsets come back in one copy."""
    if rows.shape[0] == 0:
        return []
    np_dtype = _storage(field)[0]
    lead = (rows != 0).to(torch.uint8).argmax(dim=1).cpu().tolist()
    return [Poly._from_trimmed(field, field._wrap(rows[k, at:], np_dtype)) for k, at in enumerate(lead)]


def _hits(consts: _Constants, primitive: bool, start: int, stop: int, reverse: bool, grow: bool):
    """Yields (k0, candidates, indices of the flagged rows) over [start, stop) in chunks, from the top when `reverse`."""
    field, m = consts.field, consts.m
    mask = PRIMITIVE if primitive else NORMAL
    total, done, chunk = stop - start, 0, 256 if grow else 1 << 20
    while done < total:
        n = min(chunk, total - done)
        k0 = stop - done - n if reverse else start + done
        cand = _residues(field, m, k0, n)
        flags = _classify(consts, cand, primitive, not primitive)
        idx = torch.nonzero(flags & mask).reshape(-1)
        yield k0, cand, (torch.flip(idx, dims=(0,)) if reverse else idx)
        done += n
        chunk = min(4 * chunk, 1 << 20)


def _verify_search(irreducible_poly, method=None) -> Poly:
    f = _verify_poly(irreducible_poly)
    if not f.degree > 1:
        raise ValueError(f"Argument 'irreducible_poly' must have degree greater than 1, not {f.degree}.")
    _verify_irreducible(f)
    if method is not None and method not in ["min", "max", "random"]:
        raise ValueError(f"Argument 'method' must be in ['min', 'max', 'random'], not {method!r}.")
    return f


def _one_element(irreducible_poly, method: str, primitive: bool) -> Poly:
    f = _verify_search(irreducible_poly, method)
    field = f.field
    q, m = field.order, f.degree
    _check_limits(field, m, "primitive" if primitive else "normal")
    consts = _constants(f)
    if method in ("min", "max"):
        for _, cand, idx in _hits(consts, primitive, q, q**m, method == "max", True):
            if idx.numel():
                return _polys_from_rows(field, cand[idx[:1]])[0]
    else:
        mask = PRIMITIVE if primitive else NORMAL
        while True:
            ints = [q**m + random.randint(q, q**m - 1) for _ in range(64)]
            cand = _ints_to_tensor(field, m, ints)[:, 1:].contiguous()
            idx = torch.nonzero(_classify(consts, cand, primitive, not primitive) & mask).reshape(-1)
            if idx.numel():
                return _polys_from_rows(field, cand[idx[:1]])[0]
    kind = "primitive" if primitive else "normal"
    raise RuntimeError(f"No {kind} elements in GF({q}^{m}) were found with irreducible polynomial {f}.")


def _all_elements(irreducible_poly, primitive: bool) -> list:
    f = _verify_search(irreducible_poly)
    field = f.field
    q, m = field.order, f.degree
    _check_limits(field, m, "primitive" if primitive else "normal")
    out = []
    for _, cand, idx in _hits(_constants(f), primitive, q, q**m, False, False):
        out.extend(_polys_from_rows(field, cand[idx]))
    return out


def _all_integers(f: Poly, primitive: bool, start: int) -> list:
    """The integers in [start, q^m) of the primitive (normal) residues modulo f, ascending: what the class properties hold."""
    field = f.field
    _check_limits(field, f.degree, "primitive" if primitive else "normal")
    out = []
    for k0, _, idx in _hits(_constants(f), primitive, start, field.order**f.degree, False, False):
        out.extend(k0 + i for i in idx.cpu().tolist())
    return out


def primitive_element(irreducible_poly, method: str = "min") -> Poly:
    """galois.primitive_element (_fields/_primitive_element.py:169-301): a primitive element of GF(q)[x] / (irreducible_poly) as a
    polynomial of degree < m -- the one with the smallest ("min") or largest ("max") integer, or a random one.  The constants
    0 .. q - 1 are skipped, as in the reference."""
    return _one_element(irreducible_poly, method, True)


def primitive_elements(irreducible_poly) -> list:
    """galois.primitive_elements (_fields/_primitive_element.py:304-410): all of them, sorted by their integers.  The reference
    takes the powers of one primitive element at the totatives of q^m - 1; here the classifier sweeps [q, q^m)."""
    return _all_elements(irreducible_poly, True)


def normal_element(irreducible_poly, method: str = "min") -> Poly:
    """galois.normal_element (_fields/_normal_element.py:188-299): a normal element of GF(q)[x] / (irreducible_poly) over GF(q)."""
    return _one_element(irreducible_poly, method, False)


def normal_elements(irreducible_poly) -> list:
    """galois.normal_elements (_fields/_normal_element.py:302-411): all of them, sorted by their integers."""
    return _all_elements(irreducible_poly, False)


# ---- the class properties (FieldArrayMeta) --------------------------------------------------------------------------------------
def _field_poly(cls) -> Poly:
    return _verify_poly(cls._irreducible_poly)


def _field_array(cls, ints: list):
    return cls(np.array(ints, dtype=object)) if ints else cls.Zeros(0)


def field_primitive_elements(cls):
    if "_primitive_elements" not in cls.__dict__:
        cls._primitive_elements = _field_array(cls, _all_integers(_field_poly(cls), True, 1))
    return cls._primitive_elements.copy()


def field_normal_element(cls):
    if "_normal_element" not in cls.__dict__:
        cls._normal_element = None if cls._degree == 1 else cls(int(normal_element(_field_poly(cls))))
    return None if cls._normal_element is None else cls._normal_element.copy()


def field_normal_elements(cls):
    if "_normal_elements" not in cls.__dict__:
        ints = [] if cls._degree == 1 else _all_integers(_field_poly(cls), False, cls._characteristic)
        cls._normal_elements = _field_array(cls, ints)
    return cls._normal_elements.copy()
