"""Times the shift-register kernels (galois_amd/_lfsr.py, galois_amd/csrc/gfa_lfsr.hip) and what a caller could do before them:

    python tools/bench_lfsr.py [--reps 5] [--window 200] [--small] [--out profiles/lfsr_time.txt]

  * one register, T = 2^24 and 2^27 outputs, chunked (jump to every chunk's start, then all chunks side by side), over GF(2) with
    n = 31 and n = 64 (the one-word kernel), GF(2^8) with n = 16 and GF(65537) with n = 16 (the generic kernel)
  * a sweep of the chunk length C at T = 2^24, and of T with and without chunking: where CHUNKS, CHUNK_MIN, CHUNK_MAX and CHUNK_FROM of
    _lfsr.py come from
  * 2^16 registers x 2^10 steps through lfsr_step_batched
  * yardsticks, in the same run: the only device route there was before -- gfa_poly_divmod of G x^T by the characteristic
    polynomial (one workgroup), at T = 2^16 and 2^20 -- and, for the one-word kernel, a plain fill of the output array: the kernel
    writes one byte per clock, so the fill's rate is its ceiling

Results are compared for equality before anything is timed (chunked against unchunked and against the division).  Every figure is
milliseconds per call with the operands on the device, measured as tools/bench_lagrange.py does: after one warm-up call, one call
is timed to size a loop of back-to-back calls that fills about --window milliseconds; the loop runs between two device events,
--reps times, and median / min / max of (window time / calls) are reported.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import galois_amd as ga  # noqa: E402
from galois_amd import _lfsr as LF  # noqa: E402

WINDOW_MS = 200.0
LINES = []
OUT = None  # --out: rewritten after every line, so that a run cut short keeps what it measured


def say(line):
    print(line, flush=True)
    LINES.append(line)
    if OUT:
        with open(OUT, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


def _window(fn, calls):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / calls


def timed(fn, reps):
    fn()  # warm-up: code-object load, scratch pool growth
    torch.cuda.synchronize()
    calls = max(1, min(5000, int(WINDOW_MS / max(_window(fn, 1), 1e-3))))
    out = [_window(fn, calls) for _ in range(reps)]
    return float(np.median(out)), float(min(out)), float(max(out)), calls


def report(name, stats, note=""):
    med, lo, hi, calls = stats
    say(f"{name:66s} {calls:6d} {med:11.4f} {lo:11.4f} {hi:11.4f}  {note}")


def register(order, n, seed=1):
    """A Galois register over GF(order) with an irreducible characteristic polynomial."""
    GF = ga.GF(order)
    c = ga.irreducible_poly(order, n)
    rng = np.random.default_rng(seed)
    state = GF(rng.integers(1, order, n).astype(np.int64))
    return ga.GLFSR(c.reverse(), state=state)


def step(reg, T, chunk=None, chunk_from=None):
    reg.reset()
    return reg._step_forward(T, chunk=chunk, chunk_from=chunk_from)


def by_division(reg, T):
    GF = reg.field
    dividend = np.concatenate([np.flip(reg.initial_state, axis=0), GF.Zeros(T, dtype=reg.initial_state.dtype)]).reshape(1, -1)
    return ga.poly_divmod_batched(dividend, reg.characteristic_poly)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=200.0, help="milliseconds of back-to-back calls per timed window")
    ap.add_argument("--small", action="store_true", help="T up to 2^16 and 2^10 registers only (rehearsal)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    global WINDOW_MS, OUT
    WINDOW_MS, OUT = args.window, args.out
    say(f"device: {torch.cuda.get_device_name(0)}; milliseconds per call: median / min / max of {args.reps} windows of back-to-back calls "
        f"(about {WINDOW_MS:.0f} ms each) after one warm-up call; C = T / {LF.CHUNKS} within [{LF.CHUNK_MIN}, {LF.CHUNK_MAX}], "
        f"CHUNK_FROM = {LF.CHUNK_FROM} (generic kernel, one-word kernel)")
    say(f"{'case':66s} {'calls':>6s} {'median':>11s} {'min':>11s} {'max':>11s}")
    cases = [("GF(2), n = 31", 2, 31), ("GF(2), n = 64", 2, 64), ("GF(2^8), n = 16", 2**8, 16), ("GF(65537), n = 16", 65537, 16)]
    long_T = [2**14, 2**16] if args.small else [2**24, 2**27]
    check_T = 2**12 if args.small else 2**16
    for label, order, n in cases:
        reg = register(order, n)
        # equality first: chunked, unchunked and the division agree
        want = step(reg, check_T, chunk_from=10**12)
        state = reg.state
        got = step(reg, check_T, chunk=256, chunk_from=1)
        assert np.array_equal(got, want) and np.array_equal(reg.state, state), label
        Q, R = by_division(reg, check_T)
        assert np.array_equal(Q[0], want) and np.array_equal(np.flip(R[0], axis=0), state), label
        # the division route, the only one there was
        div = {}
        for T in ([check_T] if args.small else [2**16, 2**20]):
            div[T] = timed(lambda: by_division(reg, T), args.reps)
            report(f"{label}: gfa_poly_divmod of G x^T, T = 2^{T.bit_length() - 1}", div[T], f"{T / div[T][0] / 1e3:.2f} M outputs/s")
        for T in long_T:
            t = timed(lambda: step(reg, T), args.reps)
            note = f"{T / t[0] / 1e6:.2f} G outputs/s"
            if order == 2:
                y = torch.empty(T, dtype=torch.uint8, device="cuda")
                f = timed(lambda: y.fill_(1), args.reps)
                report(f"{label}: fill of 2^{T.bit_length() - 1} bytes", f, f"{T / f[0] / 1e6:.2f} GB/s")
                note += f", {f[0] / t[0]:.3f} of the fill rate"
            Td = max(div)
            note += f", {(T / t[0]) / (Td / div[Td][0]):.0f} x the division route's rate (at T = 2^{Td.bit_length() - 1})"
            report(f"{label}: step(2^{T.bit_length() - 1}), C = {LF._chunking(T, order == 2 and n <= 64)[0]}", t, note)
        # the chunk length, and where chunking starts to pay
        T = long_T[0]
        for chunk in (256, 1024, 4096, 16384, 65536):
            if chunk < T:
                report(f"{label}: T = 2^{T.bit_length() - 1}, C = {chunk}", timed(lambda: step(reg, T, chunk=chunk, chunk_from=1), args.reps))
        for T in (2**8, 2**10, 2**12, 2**14, 2**16):
            report(f"{label}: step(2^{T.bit_length() - 1}) as shipped", timed(lambda: step(reg, T), args.reps))
            u = timed(lambda: step(reg, T, chunk_from=10**12), args.reps)
            report(f"{label}: T = 2^{T.bit_length() - 1}, unchunked", u)
            for chunk in (64, 256, 1024):
                if chunk < T:
                    c = timed(lambda: step(reg, T, chunk=chunk, chunk_from=1), args.reps)
                    report(f"{label}: T = 2^{T.bit_length() - 1}, C = {chunk}", c, f"unchunked / chunked = {u[0] / c[0]:.2f}")
        # many registers
        batch, steps = (2**10, 2**8) if args.small else (2**16, 2**10)
        GF = reg.field
        S = GF(np.random.default_rng(2).integers(0, order, (batch, n)).astype(np.int64))
        Y, S2 = ga.lfsr_step_batched(reg, S, steps)
        one = type(reg)(reg.feedback_poly, state=S[batch - 1])
        assert np.array_equal(one.step(steps), Y[batch - 1]) and np.array_equal(one.state, S2[batch - 1]), label
        t = timed(lambda: ga.lfsr_step_batched(reg, S, steps), args.reps)
        report(f"{label}: {batch} registers x {steps} steps, lfsr_step_batched", t, f"{batch * steps / t[0] / 1e6:.2f} G outputs/s")


if __name__ == "__main__":
    main()
