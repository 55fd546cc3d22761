"""FLFSR / GLFSR, lfsr_step_batched, jump and the entry points gfa_lfsr_step / gfa_lfsr_jump (galois_amd/csrc/gfa_lfsr.hip).

Expected values come from two sources that share nothing with the kernels: the reference's four step loops written out on the
oracle's element-wise add / sub / mul / div (Python integers for the field of order >= 2^64), and the division kernel --
the T outputs of a Galois register are the quotient of G x^T by the characteristic polynomial, its new state the remainder.
Chunked (C forced to 8 and to 64), unchunked, one-word and generic paths must agree with them and so with each other.
Everything is exact."""
import ctypes

import numpy as np
import pytest
import torch

import galois_amd as ga
from galois_amd import _lfsr as LF
from galois_amd import _lib as L
from oracle import gf_oracle as O
from tests import helpers as H

pytestmark = pytest.mark.gpu

BIG_PRIME = 36893488147419103183  # 65 bits: two-limb elements, the host path
FIELDS = {
    "GF(2)": lambda: ga.GF(2), "GF(2^8)": lambda: ga.GF(2**8), "GF(3^5)": lambda: ga.GF(3**5), "GF(65537)": lambda: ga.GF(65537),
    "GF(2^31-1)": lambda: ga.GF(2**31 - 1), "Goldilocks": lambda: ga.GF(H.GOLDILOCKS), "GF(2^16) calculate": lambda: ga.GF(2**16),
    "GF(7^7)": lambda: ga.GF(7**7), "65-bit prime": lambda: ga.GF(BIG_PRIME, primitive_element=3),
}


class _mode:
    """The field in the named mode for the length of a test ("... calculate" pins explicit arithmetic)."""

    def __init__(self, name):
        self.GF = FIELDS[name]()
        self.calculate = name.endswith("calculate")

    def __enter__(self):
        if self.calculate:
            self.GF.compile("jit-calculate")
        return self.GF

    def __exit__(self, *exc):
        if self.calculate:
            self.GF.compile("auto")


class _Ops:
    """Element-wise field arithmetic on lists of Python integers, by the oracle (by Python for the 65-bit prime)."""

    def __init__(self, GF):
        self.q = GF.order
        self.F = None if GF.order >= 2**64 else O.OracleField(GF.characteristic, GF.degree, int(GF.irreducible_poly) if GF.degree > 1 else None,
                                                              GF._primitive_element_int)

    def _do(self, name, fn, a, b):
        if len(a) == 0:
            return []
        if self.F is None:
            return [fn(int(x), int(y)) for x, y in zip(a, b)]
        return [int(v) for v in getattr(self.F, name)(np.array(a, dtype=np.uint64), np.array(b, dtype=np.uint64))]

    def add(self, a, b): return self._do("add", lambda x, y: (x + y) % self.q, a, b)
    def sub(self, a, b): return self._do("sub", lambda x, y: (x - y) % self.q, a, b)
    def mul(self, a, b): return self._do("mul", lambda x, y: (x * y) % self.q, a, b)
    def div(self, a, b): return self._do("div", lambda x, y: x * pow(y, -1, self.q) % self.q, a, b)

    def total(self, v):
        acc = 0
        for x in v:  # a plain loop, in the reference's order
            acc = self.add([acc], [x])[0]
        return acc


def _model(ops, kind, forward, taps, state, steps, keep=()):
    """The reference's four loops.  Returns (outputs, final state, {t: the state after t steps, for t in keep})."""
    n, state, taps = len(taps), [int(v) for v in state], [int(v) for v in taps]
    y, kept = [], {}
    for i in range(steps):
        if kind == "fibonacci" and forward:
            f = ops.total(ops.mul(state, taps))
            y.append(state[n - 1])
            state = [f] + state[:n - 1]
        elif kind == "fibonacci":
            f, state = state[0], state[1:]
            s = ops.sub([f], [ops.total(ops.mul(state, taps[:n - 1]))])
            s = ops.div(s, [taps[n - 1]])[0]  # (times the reciprocal in the reference: the same element)
            y.append(s)
            state = state + [s]
        elif forward:
            f = state[n - 1]
            y.append(f)
            state = ops.add([0] + state[:n - 1], ops.mul([f] * n, taps))
        else:
            f = ops.div([state[0]], [taps[0]])[0]
            state = ops.sub(state[1:], ops.mul([f] * (n - 1), taps[1:])) + [f]
            y.append(f)
        if i + 1 in keep:
            kept[i + 1] = list(state)
    return y, state, kept


def _ints(a):
    return [int(v) for v in np.atleast_1d(a.numpy()).reshape(-1)]


def _arr(GF, values):
    return GF(np.array([int(v) for v in values], dtype=object))


def _random_register(GF, kind, n, rng):
    """(register, taps, state) with random taps, a_n != 0, and a state with some zeros."""
    q = GF.order
    pick = lambda: int(rng.integers(0, min(q, 2**62))) if q < 2**64 else int(rng.integers(1, 2**62)) * 4000000007 % q
    taps = [pick() if rng.random() < 0.7 else 0 for _ in range(n)]
    state = [pick() if rng.random() < 0.7 else 0 for _ in range(n)]
    an = n - 1 if kind == "fibonacci" else 0
    while taps[an] == 0:
        taps[an] = pick()
    # (Taps reads its argument as [-a_1 .. -a_n] for both kinds, as the reference's does: a Galois register's own taps are the reverse)
    reg = ga.FLFSR.Taps(_arr(GF, taps), state=_arr(GF, state)) if kind == "fibonacci" else ga.GLFSR.Taps(_arr(GF, taps[::-1]), state=_arr(GF, state))
    assert _ints(reg.taps) == taps and _ints(reg.state) == state and reg.order == n
    return reg, taps, state


CHUNKS = (8, 64)
STEPS = sorted({t for c in CHUNKS for t in (1, c - 1, c, c + 1, 2 * c + 1, 5 * c + 3)})


# ---- 1. forward steps on every path against the loops ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIELDS)
def test_forward_steps_on_every_path_equal_the_reference_loops(name):
    with _mode(name) as GF:
        ops, rng = _Ops(GF), np.random.default_rng(11)
        limbed = GF.order >= 2**64
        orders = (1, 2, 5) if limbed else (1, 2, 63, 64, 65)  # (the host path clocks one element per array operation)
        steps = [t for t in STEPS if t <= 17] if limbed else STEPS
        for n in orders:
            for kind in ("fibonacci", "galois"):
                reg, taps, state = _random_register(GF, kind, n, rng)
                all_steps = sorted(set(steps) | {max(n - 1, 1), n})  # T < n, T = n
                y, _, kept = _model(ops, kind, True, taps, state, max(all_steps), keep=all_steps)
                for T in all_steps:
                    for chunk, chunk_from in [(8, 10**9)] + ([] if limbed else [(c, 1) for c in CHUNKS]):  # unchunked, then C = 8 and 64
                        reg.reset()
                        got = reg._step_forward(T, chunk=chunk, chunk_from=chunk_from)
                        where = f"{name} {kind} n={n} T={T} chunk={chunk} from={chunk_from}"
                        assert type(got) is GF and got.ndim == (0 if T == 1 else 1), where
                        assert _ints(got) == y[:T], where
                        assert _ints(reg.state) == kept[T], where
                        assert _ints(reg.initial_state) == state, where
                # the public step(), split as 17 + 33 outputs, keeps the state between the calls
                if not limbed:
                    reg.reset()
                    assert _ints(reg.step(17)) + _ints(reg.step(33)) == y[:50], f"{name} {kind} n={n}"


@pytest.mark.parametrize("name", ["GF(2)", "GF(2^8)", "GF(65537)", "Goldilocks", "GF(7^7)"])
def test_outputs_are_the_quotient_and_the_state_the_remainder_of_a_division(name):
    with _mode(name) as GF:
        rng = np.random.default_rng(12)
        for n in (1, 2, 64, 65):
            for kind in ("fibonacci", "galois"):
                reg, _, _ = _random_register(GF, kind, n, rng)
                g = reg if kind == "galois" else reg.to_galois_lfsr()
                T = 129
                dividend = np.concatenate([np.flip(g.state, axis=0), GF.Zeros(T, dtype=g.state.dtype)]).reshape(1, -1)  # G x^T, highest degree first
                Q, R = ga.poly_divmod_batched(dividend, reg.characteristic_poly)
                for chunk_from in (10**9, 1):
                    reg.reset()
                    assert _ints(reg._step_forward(T, chunk=8, chunk_from=chunk_from)) == _ints(Q[0]), f"{name} {kind} n={n}"
                    if kind == "galois":
                        assert _ints(reg.state) == _ints(R[0])[::-1], f"{name} n={n}"


def test_shipped_chunking_and_its_overrides(monkeypatch):
    """step() as shipped chunks from CHUNK_FROM steps on, with a chunk length that follows the step count; the environment overrides both."""
    for order, n in ((2, 64), (2, 65), (65537, 16)):
        GF, word = ga.GF(order), order == 2 and n <= 64
        reg = ga.GLFSR(ga.irreducible_poly(order, n).reverse(), state=GF(np.random.default_rng(21).integers(0, order, n)))
        for T in (LF.CHUNK_FROM[word] - 1, LF.CHUNK_FROM[word], LF.CHUNK_FROM[word] + LF.CHUNK_MIN + 1):
            chunk, chunk_from = LF._chunking(T, word)
            assert chunk == LF.CHUNK_MIN and chunk_from == LF.CHUNK_FROM[word]
            want = reg._step_forward(T, chunk_from=10**12)
            state = _ints(reg.state)
            reg.reset()
            assert _ints(reg.step(T)) == _ints(want) and _ints(reg.state) == state, (order, n, T)
            reg.reset()
    assert LF._chunking(2**24, False) == (1024, 2**8) and LF._chunking(2**24, True) == (4096, 2**14) and LF._chunking(2**40, False)[0] == LF.CHUNK_MAX
    monkeypatch.setenv("GFA_LFSR_CHUNK", "7")
    monkeypatch.setenv("GFA_LFSR_CHUNK_FROM", "1")
    assert LF._chunking(2**24, True) == (7, 1) and LF._chunking(50, False, chunk=9) == (9, 1)
    assert _ints(reg.step(50)) == _ints(want)[:50]


def test_gf2_word_kernel_and_generic_kernel_agree():
    """Over GF(2) a register of 64 bits runs on one word per lane, one of 65 elements on the generic kernel.  The same taps padded with
    a_65 = 0 are the register of x c(x): a Fibonacci register then puts out its extra (oldest) element first and the same sequence
    after it; a Galois register whose extra (lowest) element is zero holds x G(x) and puts out the same sequence at once."""
    GF = ga.GF(2)
    rng = np.random.default_rng(13)
    for kind in (0, 1):
        for batch, T in ((1, 1), (3, 64), (257, 65), (300, 200)):
            taps = torch.from_numpy(rng.integers(0, 2, 64).astype(np.uint8)).cuda()
            states = torch.from_numpy(rng.integers(0, 2, (batch, 64)).astype(np.uint8)).cuda()
            extra = torch.from_numpy(rng.integers(0, 2, (batch, 1)).astype(np.uint8)).cuda()
            zero = torch.zeros(1, dtype=torch.uint8, device="cuda")
            s64, y64 = states.clone(), torch.empty((batch, T), dtype=torch.uint8, device="cuda")
            LF._step_t(GF, kind, 1, taps, s64, T, y64)
            if kind == 0:  # taps [-a_1 .. -a_65], the oldest element last
                s65, y65 = torch.cat([states, extra], dim=1).contiguous(), torch.empty((batch, T + 1), dtype=torch.uint8, device="cuda")
                LF._step_t(GF, kind, 1, torch.cat([taps, zero]), s65, T + 1, y65)
                assert torch.equal(y65[:, 1:], y64) and torch.equal(y65[:, 0], extra[:, 0]), (kind, batch, T)
            else:  # taps [-a_65 .. -a_1], the lowest element first
                s65, y65 = torch.cat([torch.zeros_like(extra), states], dim=1).contiguous(), torch.empty((batch, T), dtype=torch.uint8, device="cuda")
                LF._step_t(GF, kind, 1, torch.cat([zero, taps]), s65, T, y65)
                assert torch.equal(y65, y64) and torch.equal(s65[:, 1:], s64) and not bool(s65[:, 0].any()), (kind, batch, T)
            # without outputs the states are the same
            s64b = states.clone()
            LF._step_t(GF, kind, 1, taps, s64b, T, None)
            assert torch.equal(s64b, s64)


# ---- 2. many registers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIELDS)
def test_batched_registers_equal_single_ones(name):
    with _mode(name) as GF:
        ops, rng = _Ops(GF), np.random.default_rng(14)
        limbed = GF.order >= 2**64
        for batch in (1, 3) if limbed else (1, 3, 257):
            for kind in ("fibonacci", "galois"):
                n, T = (3, 5) if limbed else (5, 70)
                reg, taps, _ = _random_register(GF, kind, n, rng)
                rows = rng.integers(0, min(GF.order, 2**31), (batch, n))
                rows[1::4] = 0  # some registers hold nothing
                S = _arr(GF, rows.reshape(-1)).reshape(batch, n)
                Y, S2 = ga.lfsr_step_batched(reg, S, T)
                assert type(Y) is GF and tuple(Y.shape) == (batch, T) and tuple(S2.shape) == (batch, n)
                assert _ints(S) == [int(v) for v in rows.reshape(-1)]  # the input is not modified
                Yh, Sh = Y.numpy(), S2.numpy()
                for k in sorted({0, min(1, batch - 1), batch // 2, batch - 1}):
                    y, s, _ = _model(ops, kind, True, taps, [int(v) for v in rows[k]], T)
                    assert [int(v) for v in Yh[k]] == y and [int(v) for v in Sh[k]] == s, f"{name} {kind} batch={batch} row {k}"
                if batch > 1:
                    assert not Yh[1].any() and not Sh[1].any()
                # (kind, feedback polynomial) in place of the register, and all the way back
                Yb, Sb = ga.lfsr_step_batched((kind, reg.feedback_poly), S2, -T)
                assert np.array_equal(Sb.numpy(), S.numpy()) and np.array_equal(Yb.numpy()[:, ::-1], Yh), f"{name} {kind} batch={batch}"


# ---- 3. backward, jumps, conversions, Berlekamp-Massey ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIELDS)
def test_backward_steps_equal_the_loops_and_undo_forward_steps(name):
    with _mode(name) as GF:
        ops, rng = _Ops(GF), np.random.default_rng(15)
        limbed = GF.order >= 2**64
        for n in (1, 2, 5) if limbed else (1, 2, 63, 64, 65):
            for kind in ("fibonacci", "galois"):
                reg, taps, state = _random_register(GF, kind, n, rng)
                T = 7 if limbed else 70
                y, s, _ = _model(ops, kind, False, taps, state, T)
                back = reg.step(-T)
                assert _ints(back) == y and _ints(reg.state) == s, f"{name} {kind} n={n}"
                fwd = reg.step(T)
                assert _ints(fwd) == y[::-1] and _ints(reg.state) == state, f"{name} {kind} n={n}"
                assert reg.step(1) == reg.step(-1) and _ints(reg.state) == state


@pytest.mark.parametrize("name", FIELDS)
def test_jump_is_the_state_after_as_many_steps(name):
    with _mode(name) as GF:
        rng = np.random.default_rng(16)
        limbed = GF.order >= 2**64
        for n in (1, 2, 5) if limbed else (1, 2, 63, 64, 65):
            for kind in ("fibonacci", "galois"):
                reg, _, state = _random_register(GF, kind, n, rng)
                for T in (0, 1, n, 12) if limbed else (0, 1, n, 100):
                    reg.reset()
                    reg.step(T)
                    expect = _ints(reg.state)
                    reg.reset()
                    assert reg.jump(T) is None and _ints(reg.state) == expect, f"{name} {kind} n={n} T={T}"
                    assert _ints(reg.initial_state) == state
                # jump(a) then jump(b) is jump(a + b), also far beyond any step count
                a, b = (2**20 + 3, 2**21 + 7) if limbed else (2**70 + 12345, 2**131 + 7)
                reg.reset()
                reg.jump(a)
                reg.jump(b)
                expect = _ints(reg.state)
                reg.reset()
                reg.jump(a + b)
                assert _ints(reg.state) == expect, f"{name} {kind} n={n}"


def test_jump_by_2_to_the_200_equals_the_modular_power():
    GF = ga.GF(2)
    P = ga.Poly.Degrees([64, 4, 3, 1, 0])  # primitive
    state = GF(np.random.default_rng(17).integers(0, 2, 64).astype(np.uint8))
    e = 2**200 + 5
    reg = ga.GLFSR(P.reverse(), state=state)
    reg.jump(e)
    expect = (pow(ga.Poly.Identity(GF), e, P) * ga.Poly(np.flip(state, axis=0))) % P
    assert _ints(reg.state) == _ints(expect.coefficients(64, order="asc"))
    # the Fibonacci register that puts out the same sequence lands on the equivalent state
    fib = ga.GLFSR(P.reverse(), state=state).to_fibonacci_lfsr()
    fib.jump(e)
    assert _ints(fib.step(200)) == _ints(reg.step(200))
    # x has order 2^64 - 1 modulo a primitive polynomial
    reg.reset()
    reg.jump(2**64 - 1)
    assert _ints(reg.state) == _ints(state)
    with pytest.raises(ValueError):
        reg.jump(-1)
    with pytest.raises(TypeError):
        reg.jump(1.0)


@pytest.mark.parametrize("name", ["GF(2)", "GF(2^8)", "GF(3^5)", "GF(65537)", "Goldilocks", "GF(7^7)", "65-bit prime"])
def test_conversions_keep_the_sequence(name):
    with _mode(name) as GF:
        rng = np.random.default_rng(18)
        for n in (1, 4, 9):
            fib, _, _ = _random_register(GF, "fibonacci", n, rng)
            gal = fib.to_galois_lfsr()
            assert isinstance(gal, ga.GLFSR) and gal.feedback_poly == fib.feedback_poly
            back = gal.to_fibonacci_lfsr()
            assert isinstance(back, ga.FLFSR) and _ints(back.state) == _ints(fib.state)
            assert _ints(gal.state) == _ints(gal.initial_state)  # to_fibonacci_lfsr steps forward and back
            y = _ints(fib.step(3 * n + 2))
            assert _ints(gal.step(3 * n + 2)) == y and _ints(back.step(3 * n + 2)) == y
            assert y[:n] == _ints(fib.initial_state)[::-1]  # the first n outputs of a Fibonacci register are its state reversed


@pytest.mark.parametrize("name", ["GF(2)", "GF(2^8)", "GF(65537)", "GF(7^7)"])
def test_berlekamp_massey_returns_the_registers(name):
    with _mode(name) as GF:
        rng = np.random.default_rng(19)
        src, _, _ = _random_register(GF, "fibonacci", 6, rng)
        y = src.step(40)
        minimal = ga.berlekamp_massey(y)
        assert minimal == ga.berlekamp_massey(y, output="minimal")
        fib = ga.berlekamp_massey(y, output="fibonacci")
        gal = ga.berlekamp_massey(y, output="galois")
        assert isinstance(fib, ga.FLFSR) and isinstance(gal, ga.GLFSR)
        assert fib.characteristic_poly == minimal and gal.characteristic_poly == minimal
        assert fib.feedback_poly == ga.berlekamp_massey(y, output="connection")
        assert _ints(fib.step(40)) == _ints(y) and _ints(gal.step(40)) == _ints(y)
        with pytest.raises(ValueError):
            ga.berlekamp_massey(y, output="lfsr")


# ---- 4. the surface: constructors, texts, exceptions ----------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [ga.FLFSR, ga.GLFSR])
def test_exceptions(cls):
    c = ga.Poly.Int(ga.primitive_poly(7, 4), field=ga.GF(7))  # x^4 + x^2 + 3x + 5
    with pytest.raises(TypeError):
        cls(c.reverse().coeffs)
    with pytest.raises(TypeError):
        cls(c.reverse(), state=1)
    with pytest.raises(ValueError):
        f_coeffs = c.reverse().coeffs.copy()
        f_coeffs[-1] = 2  # needs to be 1
        cls(ga.Poly(f_coeffs))
    with pytest.raises(ValueError):
        cls(c.reverse(), state=[1, 2, 3, 4, 5])
    with pytest.raises(TypeError):
        cls.Taps([1, 2, 3, 4])
    lfsr = cls(c.reverse())
    with pytest.raises(TypeError):
        lfsr.reset(1)
    with pytest.raises(ValueError):
        lfsr.reset([1, 2, 3])
    with pytest.raises(TypeError):
        lfsr.step(10.0)
    with pytest.raises(TypeError):
        ga.lfsr_step_batched(lfsr, [[1, 2, 3, 4]], 3)
    with pytest.raises(ValueError):
        ga.lfsr_step_batched(lfsr, ga.GF(7)([[1, 2, 3]]), 3)
    with pytest.raises(TypeError):
        ga.lfsr_step_batched(lfsr, ga.GF(5)([[1, 2, 3, 4]]), 3)
    with pytest.raises(ValueError):
        ga.lfsr_step_batched(("lagged", c.reverse()), ga.GF(7)([[1, 2, 3, 4]]), 3)


def test_taps_texts_and_properties():
    GF = ga.GF(7)
    T = GF([1, 2, 3, 4])
    fib, gal = ga.FLFSR.Taps(T), ga.GLFSR.Taps(T)
    assert fib.characteristic_poly == ga.Poly([1, -1, -2, -3, -4], field=GF) and fib.feedback_poly == ga.Poly([-4, -3, -2, -1, 1], field=GF)
    assert gal.characteristic_poly == ga.Poly([1, -1, -2, -3, -4], field=GF) and gal.feedback_poly == ga.Poly([-4, -3, -2, -1, 1], field=GF)
    assert _ints(fib.taps) == [1, 2, 3, 4] and _ints(gal.taps) == [4, 3, 2, 1]  # (the reference's GLFSR.Taps reads [-a_1 .. -a_n] too)
    c = ga.Poly.Int(ga.primitive_poly(7, 4), field=ga.GF(7))  # x^4 + x^2 + 3x + 5
    fib, gal = ga.FLFSR(c.reverse()), ga.GLFSR(c.reverse())
    assert repr(fib) == "<Fibonacci LFSR: f(x) = 1 + x^2 + 3x^3 + 5x^4 over GF(7)>"
    assert repr(gal) == "<Galois LFSR: f(x) = 1 + x^2 + 3x^3 + 5x^4 over GF(7)>"
    assert str(fib) == ("Fibonacci LFSR:\n  field: GF(7)\n  feedback_poly: 1 + x^2 + 3x^3 + 5x^4\n  characteristic_poly: x^4 + x^2 + 3x + 5\n"
                        "  taps: [0 6 4 2]\n  order: 4\n  state: [1 1 1 1]\n  initial_state: [1 1 1 1]")
    assert str(gal) == ("Galois LFSR:\n  field: GF(7)\n  feedback_poly: 1 + x^2 + 3x^3 + 5x^4\n  characteristic_poly: x^4 + x^2 + 3x + 5\n"
                        "  taps: [2 4 6 0]\n  order: 4\n  state: [1 1 1 1]\n  initial_state: [1 1 1 1]")
    for lfsr in (fib, gal):
        assert lfsr.field is GF and lfsr.order == 4 and lfsr.feedback_poly == c.reverse() and lfsr.characteristic_poly == c
        assert lfsr.feedback_poly == lfsr.characteristic_poly.reverse()
        assert _ints(lfsr.state) == [1, 1, 1, 1] and _ints(lfsr.initial_state) == [1, 1, 1, 1]
        # `state` and `initial_state` are copies
        s = lfsr.state
        s[0] = 5
        i = lfsr.initial_state
        i[0] = 5
        assert _ints(lfsr.state) == [1, 1, 1, 1] and _ints(lfsr.initial_state) == [1, 1, 1, 1]
        y = lfsr.step(0)
        assert type(y) is GF and y.size == 0
        lfsr.step(10)
        assert _ints(lfsr.state) != [1, 1, 1, 1] and _ints(lfsr.initial_state) == [1, 1, 1, 1]
        lfsr.reset()
        assert _ints(lfsr.state) == [1, 1, 1, 1]
        lfsr.reset([1, 2, 3, 4])
        assert _ints(lfsr.state) == [1, 2, 3, 4] and _ints(lfsr.initial_state) == [1, 1, 1, 1]
        given = GF([1, 2, 3, 4])
        own = type(lfsr)(c.reverse(), state=given)
        own.step(3)
        assert _ints(given) == [1, 2, 3, 4] and _ints(own.initial_state) == [1, 2, 3, 4]


def test_poly_additions():
    GF = ga.GF(7)
    f = ga.Poly([5, 0, 3, 4], field=GF)
    assert f.reverse() == ga.Poly([4, 3, 0, 5], field=GF)
    assert ga.Poly([5, 0, 3, 0], field=GF).reverse() == ga.Poly([3, 0, 5], field=GF)
    assert ga.Poly.Identity(GF) == ga.Poly([1, 0], field=GF) and ga.Poly.Identity().field is ga.GF(2)
    assert _ints(f.coefficients()) == [5, 0, 3, 4] and _ints(f.coefficients(order="asc")) == [4, 3, 0, 5]
    assert _ints(f.coefficients(6)) == [0, 0, 5, 0, 3, 4] and _ints(f.coefficients(6, order="asc")) == [4, 3, 0, 5, 0, 0]
    with pytest.raises(ValueError):
        f.coefficients(3)
    with pytest.raises(ValueError):
        f.coefficients(order="up")
    with pytest.raises(TypeError):
        f.coefficients(4.0)


# ---- 5. the LDS cap of the jump and the C contract ------------------------------------------------------------------------------
def test_max_order_and_one_more():
    GF = ga.GF(3)
    cap = ga.lfsr_max_order(GF)
    assert cap == 7628 and ga.lfsr_max_order(ga.GF(H.GOLDILOCKS)) == 3814 and ga.lfsr_max_order(ga.GF(BIG_PRIME, primitive_element=3)) == 0
    rng = np.random.default_rng(20)
    for n in (cap, cap + 1):
        taps = rng.integers(0, 3, n)
        taps[0] = taps[-1] = 1
        reg = ga.GLFSR.Taps(GF(taps), state=GF(rng.integers(0, 3, n)))
        T = 20
        dividend = np.concatenate([np.flip(reg.state, axis=0), GF.Zeros(T, dtype=reg.state.dtype)]).reshape(1, -1)
        Q, R = ga.poly_divmod_batched(dividend, reg.characteristic_poly)
        y = reg._step_forward(T, chunk=8, chunk_from=1)  # chunked at the cap, unchunked above it
        assert _ints(y) == _ints(Q[0]) and _ints(reg.state) == _ints(R[0])[::-1], n
        reg.reset()
        reg.jump(T)  # on the kernel at the cap, through Poly above it
        assert _ints(reg.state) == _ints(R[0])[::-1], n
    P = reg._state._same_storage(reg.characteristic_poly.coeffs).contiguous()
    with pytest.raises(NotImplementedError, match=f"up to order {cap} "):
        LF._jump_t(GF, 1, P, reg._state._t.contiguous(), 5, 0, 1)


def test_registers_too_long_for_the_step_kernel_run_on_whole_arrays():
    GF = ga.GF(3)
    n = LF._step_max_order(GF) + 1
    assert n == 19168 and LF._step_max_order(ga.GF(H.GOLDILOCKS)) == 9567
    rng = np.random.default_rng(22)
    taps = rng.integers(0, 3, n)
    taps[0] = taps[-1] = 1
    state = GF(rng.integers(0, 3, n))
    gal = ga.GLFSR.Taps(GF(taps), state=state)
    T = 3
    dividend = np.concatenate([np.flip(state, axis=0), GF.Zeros(T, dtype=state.dtype)]).reshape(1, -1)
    Q, R = ga.poly_divmod_batched(dividend, gal.characteristic_poly)
    assert _ints(gal.step(T)) == _ints(Q[0]) and _ints(gal.state) == _ints(R[0])[::-1]
    assert _ints(gal.step(-T)) == _ints(Q[0])[::-1] and _ints(gal.state) == _ints(state)
    fib = ga.FLFSR.Taps(GF(taps), state=state)
    assert _ints(fib.step(T)) == _ints(state)[::-1][:T] and _ints(fib.state)[T:] == _ints(state)[:n - T]
    assert _ints(fib.step(-T)) == _ints(state)[::-1][:T][::-1] and _ints(fib.state) == _ints(state)


def test_entry_points_check_their_arguments():
    GF = ga.GF(7)
    lib = L.lib()
    taps = GF([1, 2, 3, 4])._t
    states = GF([[1, 1, 1, 1]])._t.clone()
    y = torch.empty((1, 4), dtype=states.dtype, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    step = lambda kind, direction, n, batch, steps: lib.gfa_lfsr_step(GF._handle, kind, direction, ptr(taps), n, ptr(states), batch, steps, ptr(y), L.U8, None)
    assert step(2, 1, 4, 1, 4) == L.ERR_INVALID and step(0, 0, 4, 1, 4) == L.ERR_INVALID and step(0, 1, 0, 1, 4) == L.ERR_INVALID
    assert step(0, 1, 4, -1, 4) == L.ERR_INVALID and step(0, 1, 4, 1, -1) == L.ERR_INVALID
    assert step(0, 1, 4, 0, 4) == L.OK and step(0, 1, 4, 1, 0) == L.OK
    assert lib.gfa_lfsr_step(None, 0, 1, ptr(taps), 4, ptr(states), 1, 4, ptr(y), L.U8, None) == L.ERR_UNSUPPORTED
    assert lib.gfa_lfsr_step(GF._handle, 0, 1, ptr(taps), 19168, ptr(states), 1, 4, ptr(y), L.U8, None) == L.ERR_UNSUPPORTED and "19167" in L.last_error()
    assert lib.gfa_lfsr_step(ga.GF(65537)._handle, 0, 1, ptr(taps), 4, ptr(states), 1, 4, ptr(y), L.U8, None) == L.ERR_INVALID  # dtype too narrow
    assert torch.equal(states, GF([[1, 1, 1, 1]])._t)  # nothing ran
    e = (ctypes.c_uint64 * 2)(5, 0)
    P = GF([1, 6, 5, 4, 3])._t
    out = torch.empty((2, 4), dtype=states.dtype, device="cuda")
    jump = lambda kind, n, limbs, count: lib.gfa_lfsr_jump(GF._handle, kind, ptr(P), n, ptr(states), e, limbs, 3, count, ptr(out), L.U8, None)
    assert jump(2, 4, 2, 2) == L.ERR_INVALID and jump(0, 0, 2, 2) == L.ERR_INVALID and jump(0, 4, 0, 2) == L.ERR_INVALID and jump(0, 4, 2, -1) == L.ERR_INVALID
    assert jump(0, 4, 2, 0) == L.OK
    assert lib.gfa_lfsr_jump(None, 0, ptr(P), 4, ptr(states), e, 2, 3, 2, ptr(out), L.U8, None) == L.ERR_UNSUPPORTED
    assert lib.gfa_lfsr_max_order(None) == 0
    # rows 0 and 1 are 5 and 8 clocks ahead
    assert jump(0, 4, 2, 2) == L.OK
    reg = ga.FLFSR.Taps(GF([1, 2, 3, 4]))
    assert _ints(reg.characteristic_poly.coeffs) == [1, 6, 5, 4, 3]
    reg.step(5)
    five = _ints(reg.state)
    reg.step(3)
    assert out.cpu().tolist() == [five, _ints(reg.state)]
