"""
Linear-feedback shift registers.  Paths relative to /root/reference/src/galois:

  * FLFSR, GLFSR ................ _lfsr.py:27-175, 182-716, 852-1352 over the four step loops fibonacci_lfsr_step_forward_jit /
                                  _backward_jit and galois_lfsr_step_forward_jit / _backward_jit (_lfsr.py:718-843, 1354-1477)

The reference clocks one register on one core.  gfa_lfsr_step (galois_amd/csrc/gfa_lfsr.hip) clocks a whole stack of registers with
the same taps, one lane each; lfsr_step_batched exposes the stack.  One register is not sequential either: one clock of a Galois
register multiplies its state polynomial by x modulo the characteristic polynomial, so the state any number of clocks ahead is
a modular power away (gfa_lfsr_jump; FLFSR.jump / GLFSR.jump), and a long step(T) is cut into chunks of C outputs -- one jump
to every chunk's start state, then all chunks clocked side by side; row k of the (chunks, C) output is chunk k, so the
output is the contiguous sequence already.  Backward steps and short forward steps are one unchunked gfa_lfsr_step.  Fields of
order >= 2^64 have no kernel, and a register of more than 19167 elements (9567 of 64 bits) does not fit the step kernel's LDS:
their four loops run here on whole arrays, so that the API is total.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib as L
from ._array import FieldArray, _GFA_DTYPE, _ptr, _stream
from ._poly import Poly
from ._polydiv import POW_LDS_BYTES, _elem_bytes, _exp_limbs

# One register, forward: from CHUNK_FROM steps on, the sequence is produced in chunks (gfa_lfsr_jump to the chunks' start states, then
# one gfa_lfsr_step over all chunks).  The chunk length follows the step count: C = T / CHUNKS, kept within [CHUNK_MIN, CHUNK_MAX] --
# a lane is a chunk, so there should be enough chunks to fill the device, but every chunk costs a jump of about 2 log2(T) modular
# products.  Index 0: the generic kernel; index 1: the one-word kernel of GF(2), n <= 64, whose clock is some 50 times cheaper, so
# that the jumps weigh more.  Measured on an MI355X (tools/bench_lfsr.py, profiles/lfsr_time.txt).  All are
# overridden by GFA_LFSR_CHUNK (one fixed C) and GFA_LFSR_CHUNK_FROM in the environment, and per call by the arguments of
# _LFSR._step_forward, so that tests drive both paths at tiny sizes.
CHUNK_MIN = 64
CHUNK_MAX = 4096
CHUNKS = (16384, 4096)
CHUNK_FROM = (1 << 8, 1 << 14)
JUMP_EXP_WORDS = 126  # 64-bit words of an exponent gfa_lfsr_jump takes (LS_EXP_WORDS)

_KINDS = {"fibonacci": 0, "galois": 1}


def _chunking(steps: int, word: bool, chunk=None, chunk_from=None):
    """(chunk length, step count from which chunking starts) for `steps` forward steps of one register."""
    if chunk is None:
        chunk = os.environ.get("GFA_LFSR_CHUNK")
    if chunk_from is None:
        chunk_from = os.environ.get("GFA_LFSR_CHUNK_FROM")
    chunk = min(max(steps // CHUNKS[word], CHUNK_MIN), CHUNK_MAX) if chunk is None else int(chunk)
    chunk_from = CHUNK_FROM[word] if chunk_from is None else int(chunk_from)
    if chunk < 1:
        raise ValueError(f"The chunk length must be positive, not {chunk}.")
    return chunk, chunk_from


def lfsr_max_order(field) -> int:
    """Largest order of a register gfa_lfsr_jump serves over the field (LS_JUMP_MAX; 0 for fields of order >= 2^64): the kernel
    holds the characteristic polynomial, two residues and a product in LDS.  Longer registers step unchunked."""
    if field._limbed:
        return 0
    return int(L.lib().gfa_lfsr_max_order(field._handle))


def _step_max_order(field) -> int:
    """Largest order of a register gfa_lfsr_step serves over the field (LS_STEP_MAX): taps, one register and a tile of 64 outputs in LDS."""
    return (POW_LDS_BYTES // _elem_bytes(field) - 65) // 2


# ---- the two kernels on contiguous storage tensors ------------------------------------------------------------------------------
def _step_t(field, kind: int, direction: int, taps: torch.Tensor, states: torch.Tensor, steps: int, y: torch.Tensor | None):
    """Clocks the rows of states (batch, n) IN PLACE `steps` times; y (batch, steps) or None receives the outputs."""
    batch, n = states.shape
    L.check(L.lib().gfa_lfsr_step(field._handle, kind, direction, _ptr(taps), n, _ptr(states), batch, steps, _ptr(y) if y is not None else None,
                                  _GFA_DTYPE[states.element_size()], _stream()), "gfa_lfsr_step")


def _jump_t(field, kind: int, P: torch.Tensor, state: torch.Tensor, exp0: int, stride: int, count: int) -> torch.Tensor:
    """(count, n) states: row k is `state` after exp0 + k stride forward clocks."""
    n = state.numel()
    out = torch.empty((count, n), dtype=state.dtype, device=state.device)
    limbs, n_limbs = _exp_limbs(exp0)
    L.check(L.lib().gfa_lfsr_jump(field._handle, kind, _ptr(P), n, _ptr(state), limbs, n_limbs, stride, count, _ptr(out),
                                  _GFA_DTYPE[state.element_size()], _stream()), "gfa_lfsr_jump")
    return out


# ---- fields of order >= 2^64, registers too long for LDS: the four loops on whole arrays ------------------------------------------
def _host_step(kind: int, forward: bool, taps: FieldArray, state: FieldArray, steps: int):
    """(outputs, new state) of one register; the reference's loops, a whole register per array operation."""
    F = type(state)
    n = taps.size
    if F._limbed:  # (no fold over limbs: add the products one by one)
        def total(v):
            acc = v[0]
            for j in range(1, v.size):
                acc = acc + v[j]
            return acc
    else:
        total = np.sum
    s = state.copy()
    y = F.Zeros(steps)
    tinv = None if forward else np.reciprocal(taps[n - 1] if kind == 0 else taps[0])
    for i in range(steps):
        if kind == 0 and forward:
            f = total(s * taps)
            y[i] = s[n - 1]
            if n > 1:
                s[1:] = s[:n - 1].copy()
            s[0] = f
        elif kind == 0:
            f = s[0].copy()  # (an element is a view)
            if n > 1:
                s[:n - 1] = s[1:].copy()
                f = f - total(s[:n - 1] * taps[:n - 1])
            f = f * tinv
            y[i] = f
            s[n - 1] = f
        elif forward:
            f = s[n - 1]
            y[i] = f
            new = taps * f
            if n > 1:
                new[1:] = new[1:] + s[:n - 1]
            s = new
        else:
            f = s[0] * tinv
            new = F.Zeros(n)
            if n > 1:
                new[:n - 1] = s[1:] - taps[1:] * f
            new[n - 1] = f
            s = new
            y[i] = f
    return y, s


# ---- one register or many, any field ---------------------------------------------------------------------------------------------
def _step_rows(F, kind: int, taps: FieldArray, P: Poly, states: FieldArray, steps: int, chunk=None, chunk_from=None):
    """(Y (batch, |steps|), new states (batch, n)) for the rows of `states`; steps != 0."""
    batch, n = states.shape
    count, forward = abs(steps), steps > 0
    if F._limbed or n > _step_max_order(F):
        Y = F.Zeros((batch, count)) if F._limbed else F.Zeros((batch, count), dtype=states.dtype)
        S = states.copy()
        for k in range(batch):
            Y[k], S[k] = _host_step(kind, forward, taps, states[k], count)
        return Y, S
    st = states._t.contiguous().clone()
    tt = states._same_storage(taps).contiguous()
    y = torch.empty((batch, count), dtype=st.dtype, device=st.device)
    chunk, chunk_from = _chunking(count, F.order == 2 and n <= 64, chunk, chunk_from)
    if batch == 1 and forward and count >= max(chunk_from, chunk) and n <= lfsr_max_order(F):
        full, tail = divmod(count, chunk)
        starts = _jump_t(F, kind, states._same_storage(P.coeffs).contiguous(), st[0], 0, chunk, full + 1)  # row `full`: where the tail starts
        flat = y.reshape(-1)
        _step_t(F, kind, 1, tt, starts[:full], chunk, flat[:full * chunk].reshape(full, chunk))
        st = starts[full:].clone()
        if tail:
            _step_t(F, kind, 1, tt, st, tail, flat[full * chunk:].reshape(1, tail))
    else:
        _step_t(F, kind, 1 if forward else -1, tt, st, count, y)
    return F._wrap(y, states._np_dtype), F._wrap(st, states._np_dtype)


def _asc_str(poly: Poly) -> str:
    """The polynomial with its terms in ascending degree, as the reference prints under printoptions(coeffs="asc")."""
    return " + ".join(reversed(str(poly).split(" + ")))


def _verify_isinstance(argument, types, name: str):
    if not isinstance(argument, types):
        raise TypeError(f"Argument {name!r} must be an instance of {types}, not {type(argument)}.")


class _LFSR:
    """A linear-feedback shift register base object (_lfsr.py:27-175)."""

    _type = "fibonacci"

    def __init__(self, feedback_poly: Poly, state=None):
        _verify_isinstance(feedback_poly, Poly, "feedback_poly")
        if not feedback_poly.coeffs[-1] == 1:
            raise ValueError(f"Argument 'feedback_poly' must have a 0-th degree term of 1, not {feedback_poly}.")
        self._field = feedback_poly.field
        self._feedback_poly = feedback_poly
        self._characteristic_poly = feedback_poly.reverse()
        self._order = feedback_poly.degree
        a = -self._characteristic_poly.coeffs[1:]
        # Fibonacci: T = [-a_1, -a_2, ..., -a_n]; Galois: T = [-a_n, ..., -a_2, -a_1]; c(x) = x^n + a_1 x^(n-1) + ... + a_n
        self._taps = a if self._type == "fibonacci" else np.flip(a, axis=0)
        if state is None:
            state = self.field.Ones(self.order)
        self._initial_state = self._verify_and_convert_state(state)
        self._state = self.initial_state

    @classmethod
    def Taps(cls, taps: FieldArray, state=None):
        _verify_isinstance(taps, FieldArray, "taps")
        F = type(taps)
        one = F.Ones(1) if F._limbed else F.Ones(1, dtype=taps.dtype)
        coeffs = np.concatenate([one, -taps])  # the x^0 term of f(x) (Fibonacci), the x^n term of c(x) (Galois)
        if cls._type == "fibonacci":
            feedback_poly = Poly(np.flip(coeffs, axis=0))
        else:
            feedback_poly = Poly(coeffs).reverse()
        return cls(feedback_poly, state=state)

    def _verify_and_convert_state(self, state) -> FieldArray:
        _verify_isinstance(state, (tuple, list, np.ndarray, FieldArray), "state")
        state = self.field(state)  # coerces array-likes, copies arrays
        if not (state.ndim == 1 and state.size == self.order):
            raise ValueError(
                f"Argument 'state' must have size equal to the degree of the characteristic polynomial, "
                f"not {state.size} and {self.characteristic_poly.degree}."
            )
        return state

    def reset(self, state=None):
        state = self.initial_state if state is None else state
        self._state = self._verify_and_convert_state(state)

    def step(self, steps: int = 1) -> FieldArray:
        _verify_isinstance(steps, (int, np.integer), "steps")
        steps = int(steps)
        if steps == 0:
            return self.field.Zeros(0)
        if steps > 0:
            return self._step_forward(steps)
        return self._step_backward(-steps)

    def _step_forward(self, steps: int, chunk=None, chunk_from=None) -> FieldArray:
        """`chunk` and `chunk_from` override the chunk length and CHUNK_FROM for this call."""
        assert steps > 0
        return self._run(steps, chunk, chunk_from)

    def _step_backward(self, steps: int) -> FieldArray:
        assert steps > 0
        if self.characteristic_poly.coeffs[-1] == 0:
            raise ValueError(
                "Can only step the shift register backwards if the a_n tap is non-zero, "
                f"not c(x) = {self.characteristic_poly}."
            )
        return self._run(-steps)

    def _run(self, steps: int, chunk=None, chunk_from=None) -> FieldArray:
        y, s = _step_rows(self.field, _KINDS[self._type], self._taps, self._characteristic_poly, self._state.reshape(1, -1), steps, chunk, chunk_from)
        self._state = s[0]
        return y[0, 0] if abs(steps) == 1 else y[0]

    def jump(self, steps: int) -> None:
        """Device extension: advances the state by `steps` >= 0 clocks without producing the outputs -- x^steps times the state
        polynomial modulo the characteristic polynomial, one gfa_lfsr_jump launch.  `steps` is a Python integer of any size."""
        _verify_isinstance(steps, (int, np.integer), "steps")
        steps = int(steps)
        if not steps >= 0:
            raise ValueError(f"Argument 'steps' must be non-negative, not {steps}.")
        F, n = self.field, self.order
        if not F._limbed and n <= lfsr_max_order(F) and steps.bit_length() <= 64 * JUMP_EXP_WORDS:
            s = self._state._t.contiguous()
            out = _jump_t(F, _KINDS[self._type], self._state._same_storage(self._characteristic_poly.coeffs).contiguous(), s, steps, 0, 1)
            self._state = F._wrap(out[0], self._state._np_dtype)
            return
        # no kernel: the same product through Poly, on the equivalent Galois register
        g = self if self._type == "galois" else self.to_galois_lfsr()
        P = self._characteristic_poly
        ahead = (pow(Poly.Identity(F), steps, P) * Poly(np.flip(g.state, axis=0))) % P
        state = ahead.coefficients(n, order="asc")
        self._state = state if self._type == "galois" else GLFSR(self._feedback_poly, state=state).to_fibonacci_lfsr().state

    field = property(lambda self: self._field)
    feedback_poly = property(lambda self: self._feedback_poly)
    characteristic_poly = property(lambda self: self._characteristic_poly)
    taps = property(lambda self: self._taps)
    order = property(lambda self: self._order)
    initial_state = property(lambda self: self._initial_state.copy())
    state = property(lambda self: self._state.copy())

    def __repr__(self) -> str:
        return f"<{self._type.capitalize()} LFSR: f(x) = {_asc_str(self.feedback_poly)} over {self.field.name}>"

    def __str__(self) -> str:
        string = f"{self._type.capitalize()} LFSR:"
        string += f"\n  field: {self.field.name}"
        string += f"\n  feedback_poly: {_asc_str(self.feedback_poly)}"
        string += f"\n  characteristic_poly: {self.characteristic_poly}"
        string += f"\n  taps: {self.taps}"
        string += f"\n  order: {self.order}"
        string += f"\n  state: {self.state}"
        string += f"\n  initial_state: {self.initial_state}"
        return string


class FLFSR(_LFSR):
    """A Fibonacci linear-feedback shift register (_lfsr.py:182-716): feedback polynomial f(x) = 1 + a_1 x + ... + a_n x^n, taps
    T = [-a_1, ..., -a_n], state S = [S_0, ..., S_{n-1}]; the next n outputs are the state reversed."""

    _type = "fibonacci"

    def to_galois_lfsr(self) -> "GLFSR":
        """The Galois register with the same output sequence (_lfsr.py:491-575): G_0(x) = floor(Y(x) P(x) / x^n) for Y built from
        the state and P the characteristic polynomial."""
        n = self.order
        YP = (Poly(np.flip(self.state, axis=0)) * self.characteristic_poly).coeffs
        G0 = Poly(YP[:YP.size - n]) if YP.size > n else Poly(self.field.Zeros(1))  # the quotient by x^n
        return GLFSR(self.feedback_poly, state=G0.coefficients(n, order="asc"))


class GLFSR(_LFSR):
    """A Galois linear-feedback shift register (_lfsr.py:852-1352): feedback polynomial f(x) = 1 + a_1 x + ... + a_n x^n, taps
    T = [-a_n, ..., -a_1], state S = [S_0, ..., S_{n-1}]; one clock multiplies S_0 + S_1 x + ... by x modulo c(x)."""

    _type = "galois"

    def to_fibonacci_lfsr(self) -> FLFSR:
        """The Fibonacci register with the same output sequence (_lfsr.py:1159-1211): its state is the next n outputs reversed.
        The register is stepped n clocks forward and n back, so its state is unchanged."""
        output = self.step(self.order).reshape(-1)
        self.step(-self.order)
        return FLFSR(self.feedback_poly, state=np.flip(output, axis=0))


def lfsr_step_batched(lfsr, states: FieldArray, steps: int):
    """Device extension: clocks many registers with the same taps and different states in one launch.  `lfsr` is an FLFSR or a
    GLFSR (its own state is not touched), or a pair (kind, feedback_poly) with kind "fibonacci" or "galois"; `states` is
    (batch, n).  Returns (Y, new_states): Y is (batch, |steps|) outputs in the order they are produced, negative steps clock
    backward."""
    if isinstance(lfsr, (tuple, list)) and len(lfsr) == 2:
        kind, poly = lfsr
        if kind not in _KINDS:
            raise ValueError(f"The kind of register must be in {list(_KINDS)}, not {kind!r}.")
        lfsr = (FLFSR if kind == "fibonacci" else GLFSR)(poly)
    _verify_isinstance(lfsr, _LFSR, "lfsr")
    _verify_isinstance(states, FieldArray, "states")
    _verify_isinstance(steps, (int, np.integer), "steps")
    F, steps = lfsr.field, int(steps)
    if type(states) is not F:
        raise TypeError(f"Argument 'states' must be over {F.name}, not {type(states).name}.")
    if not (states.ndim == 2 and states.shape[1] == lfsr.order):
        raise ValueError(f"Argument 'states' must be 2-D with one state of size {lfsr.order} per row, not have shape {tuple(states.shape)}.")
    if steps < 0 and lfsr.characteristic_poly.coeffs[-1] == 0:
        raise ValueError(f"Can only step the shift register backwards if the a_n tap is non-zero, not c(x) = {lfsr.characteristic_poly}.")
    if steps == 0 or states.shape[0] == 0:
        return F.Zeros((states.shape[0], abs(steps)), dtype=states.dtype), states.copy()
    return _step_rows(F, _KINDS[lfsr._type], lfsr.taps, lfsr.characteristic_poly, states, steps)
