"""The Sage lfsr_sequence vectors the reference records (tests/golden/sage_lfsr.npz, packed by tests/golden/generate_lfsr_golden.py):
eight registers of order 4 over GF(2), GF(3), GF(2^3) and GF(3^3), primitive and reducible characteristic polynomials, 50 outputs
each -- through FLFSR.step and, by the conversion, GLFSR.step; in one call, split as 17 + 33, and on the chunked path with C = 7."""
import functools
import os

import numpy as np
import pytest

import galois_amd as ga
from tests import helpers as H

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(H.GOLDEN, "sage_lfsr.npz")
NAMES = [str(n) for n in np.load(GOLDEN)["names"]]


@functools.lru_cache(maxsize=None)
def _case(name):
    d = np.load(GOLDEN)
    return int(d[f"lfsr/{name}/order"]), [int(v) for v in d[f"lfsr/{name}/key"]], [int(v) for v in d[f"lfsr/{name}/fill"]], [int(v) for v in d[f"lfsr/{name}/seq"]]


def _registers(name):
    """(Fibonacci register, equivalent Galois register, the 50 outputs) of a case, built as the reference's tests build them."""
    order, key, fill, seq = _case(name)
    GF = ga.GF(order)
    c = ga.Poly(np.concatenate([GF([1]), -np.flip(GF(key), axis=0)]))  # c(x) = x^n - key[n-1] x^(n-1) - ... - key[0]
    fib = ga.FLFSR(c.reverse(), state=np.flip(GF(fill), axis=0))  # the fill is the first n outputs: the state reversed
    assert fib.characteristic_poly == c and fib.order == len(key)
    return fib, fib.to_galois_lfsr(), seq


def _ints(a):
    return [int(v) for v in np.atleast_1d(a.numpy())]


def test_all_cases_present():
    assert len(NAMES) == 8 and {"gf2_primitive", "gf3_reducible", "gf2_3_primitive", "gf3_3_reducible"} <= set(NAMES)
    for name in NAMES:
        order, key, fill, seq = _case(name)
        assert order in (2, 3, 8, 27) and len(key) == len(fill) == 4 and len(seq) == 50 and seq[:4] == fill


@pytest.mark.parametrize("name", NAMES)
def test_sage_sequences_in_one_call(name):
    fib, gal, seq = _registers(name)
    for reg in (fib, gal):
        y = reg.step(50)
        assert type(y) is reg.field and _ints(y) == seq, name


@pytest.mark.parametrize("name", NAMES)
def test_sage_sequences_split_as_17_and_33(name):
    fib, gal, seq = _registers(name)
    for reg in (fib, gal):
        assert _ints(reg.step(17)) == seq[:17] and _ints(reg.step(33)) == seq[17:], name


@pytest.mark.parametrize("name", NAMES)
def test_sage_sequences_on_the_chunked_path(name):
    fib, gal, seq = _registers(name)
    for reg in (fib, gal):
        start = _ints(reg.state)
        assert _ints(reg._step_forward(50, chunk=7, chunk_from=1)) == seq, name  # seven chunks of 7 and a tail of 1
        end = _ints(reg.state)
        reg.reset()
        assert _ints(reg.state) == start
        reg.step(50)
        assert _ints(reg.state) == end, name
