"""Times gfa_poly_gcd (galois_amd/csrc/gfa_polygcd.hip) and the factorisation that stands on it:

    python tools/bench_polygcd.py [--reps 5] [--small] [--out profiles/polygcd_time.txt]

  * one gcd of two random polynomials of degree 64, 1024 and (LDS cap) / 2 - 1 over GF(2^8) and GF(65537): the fused kernel (one
    launch, one read-back of the degree) next to the yardstick, Euclid as a loop over the `%` operator of Poly -- one
    remainder-only gfa_poly_divmod and one look at `r1 != 0` per step, the only way to a gcd before this kernel; the two results
    are compared before anything is timed;
  * 131072 pairs of degree 32 / 24 over GF(2^8) in one call (one wave per pair);
  * factors() of one random monic polynomial of degree 64 over GF(2^8) and over GF(5).
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
from galois_amd import _polygcd as PG  # noqa: E402

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
    fn()  # warm-up: code-object load
    torch.cuda.synchronize()
    calls = max(1, min(5000, int(WINDOW_MS / max(_window(fn, 1), 1e-3))))
    out = [_window(fn, calls) for _ in range(reps)]
    return float(np.median(out)), float(min(out)), float(max(out)), calls


def report(name, stats, note=""):
    med, lo, hi, calls = stats
    say(f"{name:86s} {calls:6d} {med:11.4f} {lo:11.4f} {hi:11.4f}  {note}")


def _random_poly(GF, n, seed):
    c = GF.Random(n, seed=seed)
    c[0] = GF.Random(1, low=1, seed=seed + 1)[0]
    return ga.Poly(c)


def euclid_by_remainders(a, b):
    """gcd as _polys/_functions.py:17-26 on the `%` operator."""
    r2, r1 = a, b
    while not PD._is_zero(r1):
        r2, r1 = r1, r2 % r1
    return r2 // ga.Poly(r2.coeffs[:1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=200.0, help="milliseconds of back-to-back calls per timed window")
    ap.add_argument("--small", action="store_true", help="degrees 64 and 256 only, 2^12 pairs, degree-16 factorisations (rehearsal)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    global WINDOW_MS
    WINDOW_MS = args.window
    say(f"device: {torch.cuda.get_device_name(0)}; milliseconds per call: median / min / max of {args.reps} windows of back-to-back calls "
        f"(about {WINDOW_MS:.0f} ms each) after one warm-up call")
    say(f"{'case':86s} {'calls':>6s} {'median':>11s} {'min':>11s} {'max':>11s}")

    for order in (2**8, 65537):
        F = ga.GF(order)
        cap = ga.gcd_max_terms(F)
        for degree in (64, 256) if args.small else (64, 1024, cap // 2 - 1):
            a, b = _random_poly(F, degree + 1, 3), _random_poly(F, degree + 1, 5)
            assert PG._served(F, degree + 1, degree + 1, False)
            fused = ga.gcd(a, b)
            assert fused == euclid_by_remainders(a, b)
            note = " = (LDS cap) / 2 - 1" if degree == cap // 2 - 1 else ""
            report(f"{F.name}: gcd of two polynomials of degree {degree}{note}, fused gfa_poly_gcd (one launch)", timed(lambda: ga.gcd(a, b), args.reps))
            report(f"{F.name}: the same gcd, loop over the % operator ({degree} remainders; yardstick)", timed(lambda: euclid_by_remainders(a, b), args.reps))

    F = ga.GF(2**8)
    pairs = 1 << (12 if args.small else 17)
    A, B = F.Random((pairs, 33), seed=11), F.Random((pairs, 25), seed=12)
    G = ga.poly_gcd_batched(A, B)
    for k in (0, 1, pairs - 1):
        assert ga.Poly(G[k]) == euclid_by_remainders(ga.Poly(A[k]), ga.Poly(B[k]))
    t = timed(lambda: ga.poly_gcd_batched(A, B), args.reps)
    report(f"GF(2^8): {pairs} pairs of degree 32 / 24 in one gfa_poly_gcd call", t, f"{pairs / t[0] * 1e3:.3e} pairs/s")
    t = timed(lambda: ga.poly_egcd_batched(A, B), args.reps)
    report(f"GF(2^8): the same {pairs} pairs with cofactors (egcd)", t, f"{pairs / t[0] * 1e3:.3e} pairs/s")

    degree = 16 if args.small else 64
    for order in (2**8, 5):
        F = ga.GF(order)
        f = ga.Poly.Random(degree, seed=21, field=F)
        f = f // ga.Poly(f.coeffs[:1])
        factors, mult = f.factors()
        assert ga.prod(*[p**e for p, e in zip(factors, mult)]) == f
        report(f"{F.name}: factors() of a random monic polynomial of degree {degree} ({len(factors)} irreducible factors of degrees "
               f"{sorted(p.degree for p in factors)})", timed(lambda: f.factors(), args.reps))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
