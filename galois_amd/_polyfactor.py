"""
Factorisation of polynomials over finite fields: the methods of Poly that are loops over gcd, //, % and pow(., ., f).  Paths
relative to /root/reference/src/galois:

  * Poly.is_square_free / square_free_factors / distinct_degree_factors / equal_degree_factors / factors ... _polys/_factor.py:15-450
  * Poly.Random, Poly.is_monic ............................................................................. _polys/_poly.py:257-320, 1626

Algorithms, return orders and exceptions are the reference's.  Equal-degree splitting differs in two ways that do not show in
its result (the sorted list of the irreducible factors, which is unique):

  * characteristic 2: the reference's g = h^((q^d - 1) // 2) - 1 splits only when h = 1 modulo a factor; here g is the trace
    polynomial h + h^2 + h^4 + ... + h^(2^(m d - 1)) mod f for q = 2^m, which takes each of its two values 0 and 1 modulo half of
    the factors' residues -- m d - 1 modular squarings, each one fused gfa_poly_powmod launch over all the random h of a round;
  * the stack is used: the random h of a round are powered in one poly_powmod_batched call, and gcd(g, u) for every partial factor
    u is one gfa_poly_gcd launch (stack of u, shared g) of which the host reads back the degrees only.  The h come from a
    generator seeded with a constant, so a run is reproducible.
"""
from __future__ import annotations

import numpy as np

from . import _numtheory as nt
from ._poly import Poly
from ._polydiv import poly_powmod_batched
from ._polygcd import _gcd_many, poly_gcd

EDF_ROUND = 4      # random polynomials powered together in one round of equal-degree splitting
EDF_SEED = 0x6A09E667


def _is_one(f: Poly) -> bool:
    return f.degree == 0 and int(f.coeffs[0]) == 1


def is_monic(f: Poly) -> bool:
    """Poly.is_monic (_polys/_poly.py:1626-1650)."""
    return int(f.coeffs[0]) == 1


def Random(cls, degree: int, seed=None, field=None) -> Poly:
    """Poly.Random (_polys/_poly.py:257-320): a random polynomial of the given degree, from the reference's draws."""
    if not isinstance(degree, (int, np.integer)):
        raise TypeError(f"Argument 'degree' must be an instance of {int}, not {type(degree)}.")
    if not isinstance(seed, (type(None), int, np.integer, np.random.Generator)):
        raise TypeError(f"Argument 'seed' must be an instance of (int, np.integer, np.random.Generator), not {type(seed)}.")
    if field is None:
        from ._factory import GF

        field = GF(2)
    if not degree >= 0:
        raise ValueError(f"Argument 'degree' must be non-negative, not {degree}.")
    if seed is not None and isinstance(seed, (int, np.integer)) and not seed >= 0:
        raise ValueError(f"Argument 'seed' must be non-negative, not {seed}.")
    rng = np.random.default_rng(seed)  # one generator, so that the second draw continues the first
    coeffs = field.Random(int(degree) + 1, seed=rng)
    if int(coeffs[0]) == 0:
        coeffs[0] = field.Random(low=1, seed=rng)  # a non-zero leading coefficient
    return cls(coeffs)


def is_square_free(f: Poly) -> bool:
    """Poly.is_square_free (_factor.py:15-58)."""
    if not f.is_monic:
        f = f // Poly(f.coeffs[:1])
    if f.degree == 0:
        return True
    _, multiplicities = square_free_factors(f)
    return multiplicities == [1]


def _check(f: Poly):
    if not f.degree >= 1:
        raise ValueError(f"The polynomial must be non-constant, not {f}.")
    if not f.is_monic:
        raise ValueError(f"The polynomial must be monic, not {f}.")


def square_free_factors(f: Poly):
    """Poly.square_free_factors (_factor.py:61-159): (square-free h_j, multiplicities j) with f = prod h_j^j, by multiplicity."""
    _check(f)
    field = f.field
    p = field.characteristic
    factors_, multiplicities = [], []

    # w is the product (without multiplicity) of all factors of f that have multiplicity not divisible by p
    d = poly_gcd(f, f.derivative())
    w = f // d
    i = 1
    while not _is_one(w):
        y = poly_gcd(w, d)
        z = w // y
        if not _is_one(z) and i % p != 0:
            factors_.append(z)
            multiplicities.append(i)
        w = y
        d = d // y
        i = i + 1
    # d is now the product (with multiplicity) of the remaining factors of f, a p-th power: its p-th root has every p-th
    # coefficient, mapped by the inverse Frobenius automorphism
    if not _is_one(d):
        coeffs = d.coeffs[::p]
        if field.degree > 1:
            coeffs = coeffs ** (p ** (field.degree - 1))
        g, m = square_free_factors(Poly(coeffs))
        factors_.extend(g)
        multiplicities.extend([mi * p for mi in m])

    order = sorted(range(len(factors_)), key=lambda k: multiplicities[k])  # stable, as sorting the pairs by multiplicity
    return [factors_[k] for k in order], [multiplicities[k] for k in order]


def distinct_degree_factors(f: Poly):
    """Poly.distinct_degree_factors (_factor.py:162-269): (f_i, i) with f_i the product of the irreducible factors of degree i."""
    _check(f)
    if not f.is_square_free():
        raise ValueError(f"The polynomial must be square-free, not {f}.")
    field = f.field
    q = field.order
    n = f.degree
    x = Poly(field([1, 0]))
    factors_, degrees = [], []
    a, h = f, x
    l = 1
    while l <= n // 2 and not _is_one(a):
        h = pow(h, q, a)
        z = poly_gcd(a, h - x)
        if not _is_one(z):
            factors_.append(z)
            degrees.append(l)
            a = a // z
            h = h % a
        l += 1
    if not _is_one(a):
        factors_.append(a)
        degrees.append(a.degree)
    return factors_, degrees


def _splitters(f: Poly, degree: int, rng):
    """EDF_ROUND polynomials g = s(h) mod f for random h, each of which is 0 modulo about half of the degree-`degree` factors of f."""
    field = f.field
    q, p = field.order, field.characteristic
    n = f.degree
    H = field.Random((EDF_ROUND, n), seed=rng)  # residues modulo f
    if p == 2:
        T, G = H, H
        for _ in range(field.degree * degree - 1):
            T = poly_powmod_batched(T, 2, f)
            G = G + T
    else:
        G = poly_powmod_batched(H, (q**degree - 1) // 2, f)
        G[:, n - 1] = G[:, n - 1] - field(1)
    return [Poly(G[k]) for k in range(EDF_ROUND)]


def equal_degree_factors(f: Poly, degree: int):
    """Poly.equal_degree_factors (_factor.py:272-365): the irreducible factors of a square-free product of irreducible polynomials
    of one degree, sorted by their integer representation (Cantor-Zassenhaus)."""
    if not isinstance(degree, int):
        raise TypeError(f"Argument 'degree' must be an instance of {int}, not {type(degree)}.")
    _check(f)
    if not f.degree % degree == 0:
        raise ValueError(f"Argument 'degree' must divide the degree of the polynomial, {degree} does not divide {f.degree}.")
    if not f.is_square_free():
        raise ValueError(f"The polynomial must be square-free, not {f}.")
    r = f.degree // degree
    rng = np.random.default_rng(EDF_SEED)
    done, todo = [], [f]  # factors of the final degree, and partial factors
    if r == 1:
        done, todo = [f], []
    while todo:
        for g in _splitters(f, degree, rng):
            ds = _gcd_many(todo, g)  # one launch; the degrees decide
            nxt = []
            for u, d in zip(todo, ds):
                parts = [d, u // d] if 0 < d.degree < u.degree else [u]
                for part in parts:
                    (done if part.degree == degree else nxt).append(part)
            todo = nxt
            if not todo:
                break
    return sorted(done, key=int)


def poly_factors(f: Poly):
    """Poly.factors (_factor.py:368-450): (irreducible factors sorted by their integer representation, multiplicities)."""
    _check(f)
    factors_, multiplicities = [], []
    sf_factors, sf_multiplicities = square_free_factors(f)
    for sf_factor, sf_multiplicity in zip(sf_factors, sf_multiplicities):
        df_factors, df_degrees = distinct_degree_factors(sf_factor)
        for df_factor, df_degree in zip(df_factors, df_degrees):
            g = equal_degree_factors(df_factor, df_degree)
            factors_.extend(g)
            multiplicities.extend([sf_multiplicity] * len(g))
    order = sorted(range(len(factors_)), key=lambda k: int(factors_[k]))
    return [factors_[k] for k in order], [multiplicities[k] for k in order]


def factors(value):
    """galois.factors (_polymorphic.py:538-640): the prime factorisation of an integer, as before, or Poly.factors of a polynomial."""
    if isinstance(value, Poly):
        return value.factors()
    return nt.factors(value)


Poly.is_monic = property(is_monic)
Poly.Random = classmethod(Random)
Poly.is_square_free = is_square_free
Poly.square_free_factors = square_free_factors
Poly.distinct_degree_factors = distinct_degree_factors
Poly.equal_degree_factors = equal_degree_factors
Poly.factors = poly_factors
