"""Times the two routes of Poly.roots (galois_amd/_polyroots.py) and the route there was before them:

    python tools/bench_polyroots.py [--reps 5] [--small] [--yardstick-only] [--out profiles/polyroots_time.txt]

For q in {2^8, 2^16, 2^20, 2^24, 2^31 - 1, 2^32} and degree in {4, 16, 64, 256}: a product of degree / 4 distinct linear factors
(one of them squared) and an irreducible cofactor, built from a seed, and

  * search     Poly.roots(multiplicity=True, method="search"): one gfa_poly_roots call and the read-back of the count
  * split      the same with method="split": gcd(f, x^q - x), equal-degree splitting, gfa_poly_root_multiplicity
  * yardstick  for q <= 2^24 and degrees 16 and 64: what a caller could do before, f(GF.Range(0, q)) on a resident Range, a
               comparison with zero and torch.nonzero -- roots without multiplicities.  It uses nothing this feature adds, so
               --yardstick-only runs on a checkout that does not have it.

The three results are compared before anything is timed.  Searches of more than 2^42 evaluation steps are not offered by the entry
point and are left out.  Every figure is milliseconds per call, operands already on the device, measured as tools/bench_polydiv.py
does: after one warm-up call, one call is timed to size a loop of back-to-back calls that fills about --window milliseconds; the
loop runs between two device events, --reps times, and median / min / max of (window time / calls) are reported.  The last lines
give, per degree, the largest q * degree at which the search was the faster route and the smallest at which the split route was:
SEARCH_MAX_WORK is the largest power of two below that crossover.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import galois_amd as ga  # noqa: E402

WINDOW_MS = 200.0
LINES = []
ORDERS = [("2^8", 2**8), ("2^16", 2**16), ("2^20", 2**20), ("2^24", 2**24), ("2^31 - 1", 2**31 - 1), ("2^32", 2**32)]
DEGREES = [4, 16, 64, 256]
ENTRY_MAX_WORK = 2**42


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
    say(f"{name:66s} {calls:6d} {med:11.4f} {lo:11.4f} {hi:11.4f}  {note}")


def _case(GF, order, degree):
    """(f, its roots): degree / 4 distinct roots, the first of them double, times a cofactor that is a product of irreducible
    quadratics (the lexicographically last ones) and, for an odd number of places left, nothing more than a constant."""
    rng = np.random.default_rng(order % 2**32 + degree)
    k = max(1, degree // 4)
    roots = sorted({int(r) for r in rng.integers(0, order, size=4 * k)})[:k]
    linear = [ga.Poly(GF(np.array([1, int(v)], dtype=object))) for v in (-GF(np.array(roots, dtype=object))).numpy()]
    f = linear[0]
    for p in linear:
        f = f * p
    quadratics = ga.irreducible_polys(order, 2, reverse=True)
    while f.degree + 2 <= degree:
        f = f * next(quadratics)
    return f, roots


def yardstick(f, points):
    return torch.nonzero(f(points)._t == 0).reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=200.0, help="milliseconds of back-to-back calls per timed window")
    ap.add_argument("--small", action="store_true", help="q up to 2^16 and degrees 4 and 16 only (rehearsal)")
    ap.add_argument("--yardstick-only", action="store_true", help="time only the route that existed before Poly.roots")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    global WINDOW_MS
    WINDOW_MS = args.window
    say(f"device: {torch.cuda.get_device_name(0)}; milliseconds per call: median / min / max of {args.reps} windows of back-to-back calls "
        f"(about {WINDOW_MS:.0f} ms each) after one warm-up call")
    say(f"{'case':66s} {'calls':>6s} {'median':>11s} {'min':>11s} {'max':>11s}")
    orders = ORDERS[:2] if args.small else ORDERS
    degrees = DEGREES[:2] if args.small else DEGREES
    faster = {d: ([], []) for d in degrees}  # q * degree where the search / the split route won
    for label, order in orders:
        GF = ga.GF(order)
        points = GF.Range(0, order) if order <= 2**24 else None
        for degree in degrees:
            f, roots = _case(GF, order, degree)
            name = f"GF({label}), degree {degree}, {len(roots)} roots"
            if points is not None and degree in (16, 64):
                assert yardstick(f, points).cpu().tolist() == roots, name
                t_y = timed(lambda: yardstick(f, points).cpu(), args.reps)
                report(f"{name}: f(Range(0, q)) == 0, nonzero", t_y)
            else:
                t_y = None
            if args.yardstick_only:
                continue
            mult = [2] + [1] * (len(roots) - 1)
            t_s = None
            if order * degree <= ENTRY_MAX_WORK:
                r, m = f.roots(multiplicity=True, method="search")
                assert [int(v) for v in r.numpy()] == roots and m.tolist() == mult, name
                t_s = timed(lambda: f.roots(multiplicity=True, method="search"), args.reps)
                report(f"{name}: search", t_s, f"{t_y[0] / t_s[0]:.2f} x the yardstick's rate" if t_y else "")
            r, m = f.roots(multiplicity=True, method="split")
            assert [int(v) for v in r.numpy()] == roots and m.tolist() == mult, name
            t_p = timed(lambda: f.roots(multiplicity=True, method="split"), args.reps)
            report(f"{name}: split", t_p, f"search / split = {t_s[0] / t_p[0]:.3f}" if t_s else "no search: more than 2^42 steps")
            if t_s:
                faster[degree][0 if t_s[0] <= t_p[0] else 1].append(order * degree)
    if not args.yardstick_only:
        for degree, (search, split) in faster.items():
            say(f"degree {degree}: search faster up to q * degree = {max(search, default=0)}, split faster from q * degree = {min(split, default=0)} (0: never)")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
