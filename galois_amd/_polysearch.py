"""
Irreducibility / primitivity tests of whole batches of polynomials and the searches built on them.  Paths relative to
/root/reference/src/galois:

  * Poly.is_irreducible / Poly.is_primitive ............ _polys/_irreducible.py:27-124, _polys/_primitive.py:26-104
  * irreducible_poly / irreducible_polys ............... _polys/_irreducible.py:127-373
  * primitive_polys (and the Poly form of primitive_poly) _polys/_primitive.py:107-354
  * search order, terms=, method= ....................... _polys/_search.py

The reference tests one candidate after the other on the host.  Here candidates are produced in chunks -- integer ranges
become radix-q digits on the device with torch integer operations, fixed-term patterns come from a host generator of
integers in lexicographic order -- and one gfa_poly_classify call (galois_amd/csrc/gfa_polytest.hip) classifies a chunk.
For "min" and "max" the chunks grow geometrically, so a hit near the start does not pay for a large sweep.
"""
from __future__ import annotations

import ctypes
import functools
import itertools
import random

import numpy as np
import torch

from . import _lib as L
from . import _numtheory as nt
from ._array import _GFA_DTYPE, _TORCH_STORAGE, FieldArray, _device, _ptr, _stream

MAX_DEGREE = 32       # fields other than GF(2)
MAX_DEGREE_GF2 = 255  # bit-packed
IRREDUCIBLE, PRIMITIVE, BAD_DEGREE = 1, 2, 0x80


def _check_limits(field, degree: int, what: str):
    if field._limbed:
        raise NotImplementedError(
            f"The {what} test is not implemented for polynomials over {field.name}: gfa_poly_classify serves fields of order below 2^64."
        )
    limit = MAX_DEGREE_GF2 if field.order == 2 else MAX_DEGREE
    if degree > limit:
        raise NotImplementedError(
            f"The {what} test is not implemented for degree {degree} over {field.name}: gfa_poly_classify serves degrees up to "
            f"{MAX_DEGREE_GF2} over GF(2) and up to {MAX_DEGREE} over every other field."
        )


@functools.lru_cache(maxsize=1024)
def _cofactor_exponents(q: int, m: int):
    """(q^m - 1) / r for the prime divisors r of q^m - 1, as little-endian 64-bit limbs for the C entry point."""
    n = q**m - 1
    if n == 1:  # GF(2), degree 1: nothing to exclude, but primitivity is still asked for (a non-null pointer says so)
        return 0, 1, (ctypes.c_uint64 * 1)()
    primes = nt.factors(n)[0]
    limbs = (n.bit_length() + 63) // 64
    arr = (ctypes.c_uint64 * (len(primes) * limbs))()
    for i, r in enumerate(primes):
        e = n // r
        for l in range(limbs):
            arr[i * limbs + l] = (e >> (64 * l)) & 0xFFFFFFFFFFFFFFFF
    return len(primes), limbs, arr


def _classify(field, t: torch.Tensor, primitive: bool) -> torch.Tensor:
    """Flags (uint8, on the device) of the rows of a contiguous (batch, degree + 1) storage tensor over `field`."""
    batch, n = t.shape
    flags = torch.empty(batch, dtype=torch.uint8, device=t.device)
    if primitive:
        n_exps, limbs, exps = _cofactor_exponents(field.order, n - 1)
    else:
        n_exps, limbs, exps = 0, 0, None
    L.check(L.lib().gfa_poly_classify(field._handle, _ptr(t), batch, n - 1, _GFA_DTYPE[t.element_size()], exps, n_exps, limbs,
                                      _ptr(flags), _stream()), "gfa_poly_classify")
    return flags


def _storage(field):
    np_dtype = field.dtypes[0]
    return np_dtype, _TORCH_STORAGE[field._itemsize(np_dtype)]


# ---- the tests on Poly objects and on stacks of coefficients ---------------------------------------------------------------
def _poly_test(poly, primitive: bool) -> bool:
    if poly.degree == 0:
        return False  # the zero polynomial and the units are neither
    field = poly.field
    _check_limits(field, poly.degree, "primitivity" if primitive else "irreducibility")
    t = poly.coeffs._t.contiguous().reshape(1, -1)
    flag = int(_classify(field, t, primitive).item())
    return bool(flag & (PRIMITIVE if primitive else IRREDUCIBLE))


def _batched(coeffs: FieldArray, primitive: bool) -> np.ndarray:
    if not isinstance(coeffs, FieldArray):
        raise TypeError(f"Argument 'coeffs' must be a FieldArray, not {type(coeffs)}.")
    if not (coeffs.ndim == 2 and coeffs.shape[1] >= 1):
        raise ValueError(f"Argument 'coeffs' must be 2-D with one polynomial per row, highest degree first, not have shape {tuple(coeffs.shape)}.")
    field = type(coeffs)
    degree = coeffs.shape[1] - 1
    _check_limits(field, degree, "primitivity" if primitive else "irreducibility")
    if degree == 0:
        return np.zeros(coeffs.shape[0], dtype=bool)
    flags = _classify(field, coeffs._t.contiguous(), primitive).cpu().numpy()
    bad = np.nonzero(flags & BAD_DEGREE)[0]
    if bad.size:
        raise ValueError(f"Row {int(bad[0])} of 'coeffs' has a zero leading coefficient: every row must have degree {degree}.")
    return (flags & (PRIMITIVE if primitive else IRREDUCIBLE)) != 0


def is_irreducible_batched(coeffs: FieldArray) -> np.ndarray:
    """Device extension: Poly.is_irreducible() of every row of a (batch, degree + 1) array of coefficients, highest degree
    first, in one call.  Returns a NumPy bool array."""
    return _batched(coeffs, False)


def is_primitive_batched(coeffs: FieldArray) -> np.ndarray:
    """Device extension: Poly.is_primitive() of every row of a (batch, degree + 1) array of coefficients."""
    return _batched(coeffs, True)


# ---- candidates -----------------------------------------------------------------------------------------------------------
def _digits(value: int, q: int, n: int) -> list[int]:
    """n radix-q digits of value, highest first."""
    out = [0] * n
    for i in range(n - 1, -1, -1):
        value, out[i] = divmod(value, q)
    return out


def _ints_to_tensor(field, degree: int, ints: list[int]) -> torch.Tensor:
    """Polynomials given as integers (radix-q digits, the reference's int(Poly)) -> (len, degree + 1) storage tensor."""
    q = field.order
    _, tdt = _storage(field)
    if q == 2:  # the digits are the bits
        nbytes = degree // 8 + 1
        raw = np.frombuffer(b"".join(int(v).to_bytes(nbytes, "big") for v in ints), dtype=np.uint8).reshape(len(ints), nbytes)
        host = np.unpackbits(raw, axis=1)[:, 8 * nbytes - degree - 1:].astype(np.int64)
    elif q ** (degree + 1) < 2**63:
        v = np.array(ints, dtype=np.int64)
        host = np.stack([(v // q**(degree - j)) % q for j in range(degree + 1)], axis=1)
    else:
        host = np.array([_digits(v, q, degree + 1) for v in ints], dtype=np.uint64).view(np.int64)
    return torch.from_numpy(np.ascontiguousarray(host)).to(_device()).to(tdt)


def _range_tensor(field, degree: int, k0: int, n: int) -> torch.Tensor:
    """The monic polynomials q^degree + k0 + i, i = 0 .. n - 1 (k0 + n <= q^degree), as a (n, degree + 1) storage tensor."""
    q = field.order
    _, tdt = _storage(field)
    if q >= 2**62:  # a digit does not fit torch's signed 64-bit arithmetic: host digits
        return _ints_to_tensor(field, degree, [q**degree + k0 + i for i in range(n)])
    low = degree  # digits taken from a 64-bit counter on the device
    while q**low > 2**62:
        low -= 1
    span = q**low
    assert low == degree or n <= span  # the counter carries into the digits above at most once
    dev = _device()
    vals = (k0 % span) + torch.arange(n, dtype=torch.int64, device=dev)
    out = torch.empty((n, degree + 1), dtype=torch.int64, device=dev)
    out[:, 0] = 1
    for j in range(low):
        out[:, degree - j] = torch.div(vals, q**j, rounding_mode="floor") % q
    if low < degree:
        carry = (vals >= span).unsqueeze(1)
        high = k0 // span
        rows = torch.tensor([_digits(high, q, degree - low), _digits(high + 1, q, degree - low)], dtype=torch.int64, device=dev)
        out[:, 1:degree - low + 1] = torch.where(carry, rows[1], rows[0])
    return out.to(tdt)


def _fixed_term_ints(q: int, degree: int, terms: int, reverse: bool = False):
    """The monic polynomials of the given degree with exactly `terms` non-zero coefficients, one of them the constant, as
    integers in increasing (reverse: decreasing) order -- the order of _deterministic_search_fixed_terms (_search.py:40-90)."""
    direction = (lambda r: reversed(r)) if reverse else (lambda r: r)
    if terms == 1:
        yield q**degree
        return

    def rec(value: int, top: int, left: int):  # `left` terms to place below x^top, the last of them the constant
        if left == 1:
            for c in direction(range(1, q)):
                yield value + c
        else:
            for d in direction(range(left - 1, top)):
                for c in direction(range(1, q)):
                    yield from rec(value + c * q**d, d, left - 1)

    yield from rec(q**degree, degree, terms - 1)


def _make_poly(field, row: torch.Tensor):
    from ._poly import Poly

    return Poly(field._wrap(row.contiguous(), _storage(field)[0]))


def _search(order: int, degree: int, terms, reverse: bool, primitive: bool):
    """All monic irreducible (primitive) polynomials of the degree, with `terms` non-zero terms when given, lexicographically."""
    from ._factory import GF

    if degree == 0:
        return  # constants are not irreducible
    field = GF(order)
    _check_limits(field, degree, "primitivity" if primitive else "irreducibility")
    mask = PRIMITIVE if primitive else IRREDUCIBLE

    def hits(cand):
        flags = _classify(field, cand, primitive).cpu().numpy()
        idx = np.nonzero(flags & mask)[0]
        return idx

    if terms is None:
        total, done, chunk = order**degree, 0, 256
        while done < total:
            n = min(chunk, total - done)
            cand = _range_tensor(field, degree, total - done - n if reverse else done, n)
            idx = hits(cand)
            for i in (idx[::-1] if reverse else idx):
                yield _make_poly(field, cand[int(i)])
            done += n
            chunk = min(4 * chunk, 1 << 20)
    else:
        gen = _fixed_term_ints(order, degree, terms, reverse)
        chunk = 64
        while True:
            ints = list(itertools.islice(gen, chunk))
            if not ints:
                break
            cand = _ints_to_tensor(field, degree, ints)
            for i in hits(cand):
                yield _make_poly(field, cand[int(i)])
            chunk = min(4 * chunk, 1 << 16)


@functools.lru_cache(maxsize=8192)
def _minimum_terms(order: int, degree: int, primitive: bool) -> int:
    """_minimum_terms (_search.py:143-171): over GF(2) an even number of terms means a root at 1, so only odd counts are tried."""
    step = 2 if order == 2 and degree > 1 else 1
    for terms in range(1, degree + 2, step):
        if next(_search(order, degree, terms, False, primitive), None) is not None:
            return terms
    kind = "primitive" if primitive else "irreducible"
    raise RuntimeError(
        f"Could not find the minimum number of terms for a degree-{degree} {kind} polynomial over GF({order}). "
        "This should never happen. Please open a GitHub issue."
    )


def _random_search(order: int, degree: int, terms, primitive: bool):
    """_random_search / _random_search_fixed_terms (_search.py:93-140), a batch of draws per call."""
    from ._factory import GF

    field = GF(order)
    _check_limits(field, degree, "primitivity" if primitive else "irreducibility")
    mask = PRIMITIVE if primitive else IRREDUCIBLE
    if terms == 1:
        ints_once = [order**degree]
    n = max(64, 8 * degree)
    while True:
        if terms is None:
            ints = [random.randint(order**degree, 2 * order**degree - 1) for _ in range(n)]
        elif terms == 1:
            ints = ints_once
        else:
            ints = []
            for _ in range(n):
                v = order**degree + random.randint(1, order - 1)
                for d in random.sample(range(1, degree), terms - 2):
                    v += random.randint(1, order - 1) * order**d
                ints.append(v)
        cand = _ints_to_tensor(field, degree, ints)
        idx = np.nonzero(_classify(field, cand, primitive).cpu().numpy() & mask)[0]
        if idx.size:
            return _make_poly(field, cand[int(idx[0])])
        if terms == 1:
            raise StopIteration


# ---- the public searches ----------------------------------------------------------------------------------------------------
def _verify(order, degree, terms, kind: str, at_least: int, method=None, reverse=None):
    for name, value, types, optional in (("order", order, int, False), ("degree", degree, int, False), ("terms", terms, (int, str), True)):
        if not (optional and value is None) and (isinstance(value, bool) and types is int or not isinstance(value, types)):
            raise TypeError(f"Argument {name!r} must be an instance of {types}, not {type(value)}.")
    if reverse is not None and not isinstance(reverse, bool):
        raise TypeError(f"Argument 'reverse' must be an instance of {bool}, not {type(reverse)}.")
    if order < 2 or len(nt.factors(order)[0]) != 1:
        raise ValueError(f"Argument 'order' must be a prime power, not {order}.")
    if not degree >= at_least:
        if at_least == 1:
            raise ValueError(f"Argument 'degree' must be at least 1, not {degree}. There are no {kind} polynomials with degree 0.")
        raise ValueError(f"Argument 'degree' must be at least 0, not {degree}.")
    if isinstance(terms, int) and not 1 <= terms <= degree + 1:
        raise ValueError(f"Argument 'terms' must be at least 1 and at most {degree + 1}, not {terms}.")
    if isinstance(terms, str) and terms not in ["min"]:
        raise ValueError(f"Argument 'terms' must be 'min', not {terms!r}.")
    if method is not None and method not in ["min", "max", "random"]:
        raise ValueError(f"Argument 'method' must be in ['min', 'max', 'random'], not {method!r}.")


def _polys(order, degree, terms, reverse, primitive: bool):
    if terms == "min":
        terms = _minimum_terms(order, degree, primitive)
    yield from _search(order, degree, terms, reverse, primitive)


def _one_poly(order, degree, terms, method, primitive: bool):
    kind = "primitive" if primitive else "irreducible"
    try:
        if method in ("min", "max"):
            return next(_polys(order, degree, terms, method == "max", primitive))
        if terms == "min":
            terms = _minimum_terms(order, degree, primitive)
        return _random_search(order, degree, terms, primitive)
    except StopIteration as e:
        terms_str = "any" if terms is None else str(terms)
        raise RuntimeError(f"No monic {kind} polynomial of degree {degree} over GF({order}) with {terms_str} terms exists.") from e


def irreducible_poly(order: int, degree: int, terms=None, method: str = "min"):
    """galois.irreducible_poly (_polys/_irreducible.py:127-256): a monic irreducible polynomial of the degree over GF(order) --
    the lexicographically first ("min"), last ("max") or a random one, optionally with a given or the minimal number of terms."""
    _verify(order, degree, terms, "irreducible", 1, method=method)
    return _one_poly(order, degree, terms, method, False)


def irreducible_polys(order: int, degree: int, terms=None, reverse: bool = False):
    """galois.irreducible_polys (_polys/_irreducible.py:259-373): iterates over all monic irreducible polynomials of the degree."""
    _verify(order, degree, terms, "irreducible", 0, reverse=reverse)
    return _polys(order, degree, terms, reverse, False)


def primitive_polys(order: int, degree: int, terms=None, reverse: bool = False):
    """galois.primitive_polys (_polys/_primitive.py:238-354): iterates over all monic primitive polynomials of the degree."""
    _verify(order, degree, terms, "primitive", 0, reverse=reverse)
    return _polys(order, degree, terms, reverse, True)
