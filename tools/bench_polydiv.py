"""Times gfa_poly_divmod and gfa_poly_powmod (galois_amd/csrc/gfa_polydiv.hip):

    python tools/bench_polydiv.py [--reps 5] [--small] [--out profiles/polydiv_time.txt]

  * remainder-only division of 2^17 rows of 255 coefficients over GF(2^8) by the RS(255, 223) generator polynomial (the rows are
    messages followed by 32 zeros, so the remainders are the parity symbols), next to the specialised gfa_rs_encode(parity_only)
    on the same messages -- the general kernel is not expected to match the one-codeword-per-lane code kernel; the two results
    are compared before anything is timed;
  * one division of a degree-4096 polynomial by a degree-2048 one over GF(2^8) and GF(65537): quadratic work on ONE compute unit;
  * pow(x, 2**255, f) for f of degree 1024 over GF(2^8) and GF(65537): the fused kernel (one launch) and the Python loop
    (np.convolve and a remainder-only gfa_poly_divmod per step) that serves moduli above the kernel's cap.
Every figure is milliseconds per call, operands already on the device: after one warm-up call, one call is timed to size a loop
of back-to-back calls that fills about --window milliseconds; the loop runs between two device events, --reps times, and
median / min / max of (window time / calls) are reported.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import galois_amd as ga  # noqa: E402
from galois_amd import _polydiv as PD  # noqa: E402

WINDOW_MS = 200.0
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


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
    say(f"{name:78s} {calls:6d} {med:11.4f} {lo:11.4f} {hi:11.4f}  {note}")


def _random_poly(GF, n, seed):
    c = GF.Random(n, seed=seed)
    c[0] = GF.Random(1, low=1, seed=seed + 1)[0]
    return ga.Poly(c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=200.0, help="milliseconds of back-to-back calls per timed window")
    ap.add_argument("--small", action="store_true", help="2^12 rows, degrees 512 / 256 and 128, exponent 2^31 (rehearsal)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    global WINDOW_MS
    WINDOW_MS = args.window
    say(f"device: {torch.cuda.get_device_name(0)}; milliseconds per call: median / min / max of {args.reps} windows of back-to-back calls "
        f"(about {WINDOW_MS:.0f} ms each) after one warm-up call")
    say(f"{'case':78s} {'calls':>6s} {'median':>11s} {'min':>11s} {'max':>11s}")

    # remainder-only division against the Reed-Solomon encoder
    GF = ga.GF(2**8)
    rs = ga.ReedSolomon(255, 223)
    rows = 1 << (12 if args.small else 17)
    msg = GF.Random((rows, 223), seed=1)
    a = torch.zeros((rows, 255), dtype=torch.uint8, device=msg._t.device)
    a[:, :223] = msg._t
    g = torch.from_numpy(rs.generator_poly.coeffs.astype(np.uint8)).to(a.device)
    parity = rs.encode(msg, output="parity")
    rem = PD._divmod_t(GF, a, g, False, True)[1]
    assert torch.equal(rem, parity._t), "the remainders are not the parity symbols"
    t_div = timed(lambda: PD._divmod_t(GF, a, g, False, True), args.reps)
    t_rs = timed(lambda: rs.encode(msg, output="parity"), args.reps)
    report(f"GF(2^8): {rows} rows of 255 % RS(255,223) generator, gfa_poly_divmod remainder only", t_div, f"{rows / t_div[0] * 1e3:.3e} rows/s")
    report(f"GF(2^8): the same {rows} messages, gfa_rs_encode(parity_only) (yardstick)", t_rs, f"{rows / t_rs[0] * 1e3:.3e} rows/s")

    na, nb = (513, 257) if args.small else (4097, 2049)
    for order in (2**8, 65537):
        F = ga.GF(order)
        f, h = _random_poly(F, na, 3), _random_poly(F, nb, 5)
        q, r = divmod(f, h)
        assert q * h + r == f
        at, bt = f.coeffs._t.reshape(1, -1).contiguous(), h.coeffs._t.contiguous()
        report(f"{F.name}: one division, degree {na - 1} / {nb - 1}, quotient and remainder (one workgroup)", timed(lambda: PD._divmod_t(F, at, bt, True, True), args.reps))

    d, e = (128, 2**31) if args.small else (1024, 2**255)
    for order in (2**8, 65537):
        F = ga.GF(order)
        c = _random_poly(F, d + 1, 7)
        x = ga.Poly(F([1, 0]))
        fused = pow(x, e, c)
        reduce = lambda p: p if p.size < c.coeffs.size else PD._divmod_1d(p, c.coeffs, want_q=False)[1]
        loop = lambda: PD._pow_loop(x.coeffs, e, reduce)
        assert ga.Poly(loop()) == fused
        xt, ct = x.coeffs._t.reshape(1, -1).contiguous(), c.coeffs._t.contiguous()
        report(f"{F.name}: pow(x, 2^{e.bit_length() - 1}, f), degree {d}, fused gfa_poly_powmod (one launch)", timed(lambda: PD._powmod_t(F, xt, e, ct), args.reps))
        report(f"{F.name}: the same power, Python loop over np.convolve and gfa_poly_divmod", timed(loop, args.reps))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
