"""
galois_amd.Poly -- a small dense univariate polynomial over a device field: the part of the reference's Poly that is
array-sized work.  Paths relative to /root/reference/src/galois:

  * Poly.__call__ (element-wise and square-matrix evaluation) ... _polys/_poly.py:862-950 over evaluate_elementwise_jit /
                                                                 evaluate_matrix_jit (_polys/_dense.py:404-470)
  * + - * (polynomial and scalar), negation ..................... _polys/_dense.py:54-123 (multiply = np.convolve)
  * is_irreducible() / is_primitive(), Int / Degrees / int() .... _polys/_irreducible.py:27-124, _primitive.py:26-104,
                                                                 _poly.py:372-530 (the tests run in galois_amd/_polysearch.py)
  * divmod, //, %, ** and three-argument pow() .................. _polys/_poly.py:1327-1460 over divmod_jit / floordiv_jit /
                                                                 mod_jit / pow_jit (_polys/_dense.py:126-401; galois_amd/_polydiv.py)
  * gcd / egcd / lcm / prod, is_square_free() and the factorisations ... _polys/_functions.py:10-94 and _polys/_factor.py:15-450
                                                                 (galois_amd/_polygcd.py on gfa_poly_gcd; galois_amd/_polyfactor.py,
                                                                 which also adds Poly.Random and Poly.is_monic)
  * roots(multiplicity) and Poly.Roots .......................... _polys/_poly.py:706-787 over roots_jit (_polys/_dense.py:443-513) and
                                                                 _root_multiplicity, and _poly.py:536-612 (galois_amd/_polyroots.py on
                                                                 gfa_poly_roots / gfa_poly_root_multiplicity)
  * lagrange_poly, lagrange_poly_batched and crt ................ _polys/_lagrange.py:19-133 and _polymorphic.py:386-521
                                                                 (galois_amd/_lagrange.py on gfa_poly_lagrange)
  * reverse(), Identity, coefficients(size, order) ............... _polys/_poly.py:229-256, 618-703 (what galois_amd/_lfsr.py needs)
The sparse/binary representations stay out of scope.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from . import _numtheory as nt
from ._array import FieldArray, _ptr, _stream


class Poly:
    """Dense polynomial with coefficients in degree-descending order, held as a 1-D device field array."""

    _reflected_division = True  # FieldArray's / // % divmod hand a Poly on the right to the reflected operators below

    def __init__(self, coeffs, field=None, order: str = "desc"):
        if order not in ["desc", "asc"]:
            raise ValueError(f"Argument 'order' must be in ['desc', 'asc'], not {order!r}.")
        if isinstance(coeffs, FieldArray):
            if field is not None and type(coeffs) is not field:
                raise TypeError(f"Argument 'coeffs' is over {type(coeffs).name} but 'field' is {field.name}.")
            c = coeffs
        else:
            if field is None:
                from ._factory import GF

                field = GF(2)
            arr = np.asarray(coeffs)
            if arr.dtype != object and np.issubdtype(arr.dtype, np.integer) and arr.size and arr.min() < 0:
                arr = arr % field.characteristic if field.is_prime_field else arr  # "-1" style coefficients over GF(p)
            c = field(arr)
        if c.ndim != 1 or c.size == 0:
            raise ValueError(f"Argument 'coeffs' must be a non-empty 1-D array, not shape {tuple(c.shape)}.")
        if order == "asc":
            c = np.flip(c)
        self._field = type(c)
        self._coeffs = self._trim(c)

    @staticmethod
    def _trim(c: FieldArray) -> FieldArray:
        nz = torch.nonzero(c._t.reshape(c.size, -1).any(dim=1))  # (fields of order >= 2^64: two limbs per element)
        if nz.numel() == 0:
            return c[-1:] if c.size else c
        return c[int(nz[0].item()):]

    @classmethod
    def _from_trimmed(cls, field, coeffs: FieldArray) -> "Poly":
        """The Poly of a 1-D array over `field` whose first coefficient is non-zero (or the single coefficient 0), without the
        checks and the device round trip of _trim: for callers that make many polynomials from rows they have already measured."""
        p = object.__new__(cls)
        p._field = field
        p._coeffs = coeffs
        return p

    @classmethod
    def Int(cls, integer: int, field=None) -> "Poly":
        """Poly.Int (_polys/_poly.py:372-444): the polynomial whose coefficients are the radix-q digits of the integer."""
        if not isinstance(integer, (int, np.integer)):
            raise TypeError(f"Argument 'integer' must be an instance of {int}, not {type(integer)}.")
        if not integer >= 0:
            raise ValueError(f"Argument 'integer' must be non-negative, not {integer}.")
        if field is None:
            from ._factory import GF

            field = GF(2)
        return cls(field(np.array(nt.poly_from_int(int(integer), field.order), dtype=object)))

    @classmethod
    def Degrees(cls, degrees, coeffs=None, field=None) -> "Poly":
        """Poly.Degrees (_polys/_poly.py:447-530): the polynomial with the given non-zero degrees (coefficients default to 1)."""
        degrees = [int(d) for d in degrees]
        if any(d < 0 for d in degrees):
            raise ValueError(f"Argument 'degrees' must have non-negative values, not {degrees}.")
        if isinstance(coeffs, FieldArray):
            if field is not None and type(coeffs) is not field:
                raise TypeError(f"Argument 'coeffs' is over {type(coeffs).name} but 'field' is {field.name}.")
            field = type(coeffs)
            coeffs = coeffs.numpy()
        coeffs = [1] * len(degrees) if coeffs is None else [int(c) for c in coeffs]
        if len(coeffs) != len(degrees):
            raise ValueError(f"Arguments 'degrees' and 'coeffs' must have the same length, not {len(degrees)} and {len(coeffs)}.")
        if field is None:
            from ._factory import GF

            field = GF(2)
        dense = [0] * (max(degrees, default=0) + 1)
        for d, c in zip(degrees, coeffs):
            dense[len(dense) - 1 - d] = c
        return cls(field(np.array(dense, dtype=object)))

    @classmethod
    def Identity(cls, field=None) -> "Poly":
        """Poly.Identity (_polys/_poly.py:229-256): the polynomial x."""
        if field is None:
            from ._factory import GF

            field = GF(2)
        return cls(field([1, 0]))

    def coefficients(self, size=None, order: str = "desc") -> FieldArray:
        """Poly.coefficients (_polys/_poly.py:618-678): the coefficients in `size` >= degree + 1 entries, zeros for the higher
        degrees, highest degree first or ("asc") last."""
        if not (size is None or isinstance(size, (int, np.integer))):
            raise TypeError(f"Argument 'size' must be an instance of {int}, not {type(size)}.")
        if not isinstance(order, str):
            raise TypeError(f"Argument 'order' must be an instance of {str}, not {type(order)}.")
        n = self._coeffs.size
        size = n if size is None else int(size)
        if not size >= n:
            raise ValueError(f"Argument 'size' must be at least degree + 1 ({n}), not {size}.")
        if order not in ["desc", "asc"]:
            raise ValueError(f"Argument 'order' must be either 'desc' or 'asc', not {order!r}.")
        F = self._field
        zeros = F.Zeros(size - n) if F._limbed else F.Zeros(size - n, dtype=self._coeffs.dtype)
        coeffs = self._coeffs.copy() if size == n else np.concatenate([zeros, self._coeffs])
        return np.flip(coeffs, axis=0) if order == "asc" else coeffs

    def reverse(self) -> "Poly":
        """Poly.reverse (_polys/_poly.py:680-703): x^d f(1/x) for the degree d -- the coefficients reversed."""
        return Poly(np.flip(self._coeffs, axis=0))

    def __int__(self) -> int:
        """The integer whose radix-q digits are the coefficients (_polys/_poly.py:752-775)."""
        return nt.poly_to_int([int(v) for v in self._coeffs.numpy()], self._field.order)

    def is_irreducible(self) -> bool:
        """Poly.is_irreducible (_polys/_irreducible.py:27-124): Rabin's test, on the device (gfa_poly_classify)."""
        from ._polysearch import _poly_test

        return _poly_test(self, False)

    def is_primitive(self) -> bool:
        """Poly.is_primitive (_polys/_primitive.py:26-104): irreducible, non-zero constant term, and x of full order."""
        from ._polysearch import _poly_test

        return _poly_test(self, True)

    field = property(lambda self: self._field)
    coeffs = property(lambda self: self._coeffs)
    degree = property(lambda self: self._coeffs.size - 1)

    def __repr__(self) -> str:
        return f"Poly({self}, {self._field.name})"

    def __str__(self) -> str:
        return nt.poly_str([int(v) for v in self._coeffs.numpy()])

    def __eq__(self, other) -> bool:
        if not isinstance(other, Poly) or other._field is not self._field or other.degree != self.degree:
            return False
        return bool(np.all(self._coeffs == other._coeffs))

    # ---- evaluation --------------------------------------------------------------------------------------------------
    def __call__(self, x, elementwise: bool = True):
        F = self._field
        xa = x if isinstance(x, FieldArray) and type(x) is F else F(x)
        if F._limbed:  # order >= 2^64: two-limb kernels (gfa_wide_poly_evaluate; matrix Horner on gfa_wide_matmul)
            if elementwise:
                return self._coeffs._poly_evaluate(xa)
            if not (xa.ndim == 2 and xa.shape[0] == xa.shape[1]):
                raise ValueError(f"Argument 'x' must be a square matrix when evaluating the polynomial not element-wise, not shape {tuple(xa.shape)}.")
            eye = F.Identity(xa.shape[0])
            acc = eye * self._coeffs[0]
            for j in range(1, self._coeffs.size):
                acc = acc @ xa + eye * self._coeffs[j]
            return acc
        c = xa._same_storage(self._coeffs).contiguous()
        if elementwise:
            t = xa._t.contiguous()
            out = torch.empty_like(t)
            L.check(L.lib().gfa_poly_evaluate(F._handle, _ptr(c), c.numel(), _ptr(t), _ptr(out), t.numel(), xa._gfa_dtype(),
                                              _stream()), "gfa_poly_evaluate")
            return F._wrap(out, xa._np_dtype)
        # matrix evaluation: Horner with matrix products (evaluate_matrix_jit, _dense.py:443-470)
        if not (xa.ndim == 2 and xa.shape[0] == xa.shape[1]):
            raise ValueError(f"Argument 'x' must be a square matrix when evaluating the polynomial not element-wise, not shape {tuple(xa.shape)}.")
        eye = F.Identity(xa.shape[0], dtype=xa.dtype if xa.dtype != np.dtype(object) else None)
        cs = F._wrap(c, xa._np_dtype)
        acc = eye * cs[0]
        for j in range(1, cs.size):
            acc = acc @ xa + eye * cs[j]
        return acc

    # ---- arithmetic --------------------------------------------------------------------------------------------------
    def _coerce(self, other) -> "Poly":
        if isinstance(other, Poly):
            if other._field is not self._field:
                raise TypeError(f"Both polynomials must be over the same field, not {self._field.name} and {other._field.name}.")
            return other
        if isinstance(other, FieldArray) and type(other) is self._field and other.ndim == 0:
            return Poly(other.reshape(1))
        raise TypeError(f"Cannot combine a polynomial over {self._field.name} with {type(other)}.")

    def _aligned(self, other: "Poly"):
        a, b = self._coeffs, other._coeffs
        n = max(a.size, b.size)
        F = self._field
        if F._limbed:
            pad = lambda v: np.concatenate([F.Zeros(n - v.size), v]) if v.size < n else v
            return pad(a), pad(b)
        ta = torch.zeros(n, dtype=a._t.dtype, device=a._t.device)
        tb = torch.zeros(n, dtype=a._t.dtype, device=a._t.device)
        ta[n - a.size:] = a._t
        tb[n - b.size:] = a._same_storage(b)
        return F._wrap(ta, a._np_dtype), F._wrap(tb, a._np_dtype)

    def __add__(self, other):
        a, b = self._aligned(self._coerce(other))
        return Poly(a + b)

    __radd__ = __add__

    def __sub__(self, other):
        a, b = self._aligned(self._coerce(other))
        return Poly(a - b)

    def __rsub__(self, other):
        return self._coerce(other) - self

    def __neg__(self):
        return Poly(-self._coeffs)

    def __mul__(self, other):
        if isinstance(other, (int, np.integer)):
            return Poly(self._coeffs * int(other))  # scalar (repeated-addition) multiplication, _poly.py:1406-1416
        o = self._coerce(other)
        return Poly(np.convolve(self._coeffs, o._coeffs))

    __rmul__ = __mul__

    # division with remainder and powers (galois_amd/_polydiv.py): gfa_poly_divmod / gfa_poly_powmod
    def __divmod__(self, other):
        from ._polydiv import poly_divmod

        return poly_divmod(self, self._coerce(other))

    def __rdivmod__(self, other):
        return divmod(self._coerce(other), self)

    def __floordiv__(self, other):
        from ._polydiv import poly_divmod

        return poly_divmod(self, self._coerce(other), want_r=False)[0]

    def __rfloordiv__(self, other):
        return self._coerce(other) // self

    def __mod__(self, other):
        from ._polydiv import poly_divmod

        return poly_divmod(self, self._coerce(other), want_q=False)[1]  # the kernel writes no quotients

    def __rmod__(self, other):
        return self._coerce(other) % self

    def __truediv__(self, other):
        raise NotImplementedError(
            "Polynomial true division is not supported because fractional polynomials are not yet supported. "
            "Use floor division //, modulo %, and/or divmod() instead."
        )

    __rtruediv__ = __truediv__

    def __pow__(self, exponent, modulus=None):
        from ._polydiv import poly_pow

        return poly_pow(self, exponent, None if modulus is None else self._coerce(modulus))

    def derivative(self, k: int = 1) -> "Poly":
        """Formal derivative (_polys/_poly.py:1098-1160): coefficient of x^(j-1) is (j mod p) * a_j."""
        if not isinstance(k, (int, np.integer)) or k < 1:
            raise ValueError(f"Argument 'k' must be a positive integer, not {k}.")
        p = self
        for _ in range(int(k)):
            if p.degree == 0:
                return Poly(p._field([0]))
            c = p._coeffs[:-1]
            mult = np.arange(p.degree, 0, -1)
            p = Poly(c * mult)
        return p


def berlekamp_massey(sequence, output: str = "minimal"):
    """galois.berlekamp_massey (_lfsr.py:1560-1625): the minimal (characteristic) polynomial c(x) of a linear recurrent
    sequence, or its connection polynomial C(x) = reverse of c(x); "fibonacci" and "galois" give the register that puts the
    sequence out next (_lfsr.py:1613-1619): its state is the first deg C values reversed."""
    if not isinstance(sequence, FieldArray):
        raise TypeError(f"Argument 'sequence' must be a FieldArray, not {type(sequence)}.")
    if not isinstance(output, str):
        raise TypeError(f"Argument 'output' must be a string, not {type(output)}.")
    if not sequence.ndim == 1:
        raise ValueError(f"Argument 'sequence' must be 1-D, not {sequence.ndim}-D.")
    if output not in ["minimal", "connection", "fibonacci", "galois"]:
        raise ValueError(f"Argument 'output' must be in ['minimal', 'connection', 'fibonacci', 'galois'], not {output!r}.")
    F = type(sequence)
    t = sequence._t.contiguous()
    n = t.numel()
    out = torch.empty_like(t)
    ln = torch.empty(1, dtype=torch.int64, device=t.device)
    L.check(L.lib().gfa_berlekamp_massey(F._handle, _ptr(t), n, 1, _ptr(out), _ptr(ln), sequence._gfa_dtype(), _stream()),
            "gfa_berlekamp_massey")
    asc = out[: int(ln.item())]
    if output != "minimal":
        connection = Poly(F._wrap(torch.flip(asc, dims=(0,)).contiguous(), sequence._np_dtype))  # degree-descending C(x)
        if output == "connection":
            return connection
        from ._lfsr import FLFSR

        lfsr = FLFSR(connection, state=np.flip(sequence[0:connection.degree], axis=0))
        return lfsr if output == "fibonacci" else lfsr.to_galois_lfsr()
    return Poly(F._wrap(asc.contiguous(), sequence._np_dtype))  # c(x) = x^L C(1/x): the ascending C read as descending
