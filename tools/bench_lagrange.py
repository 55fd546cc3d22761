"""Times the routes of lagrange_poly_batched (galois_amd/_lagrange.py) and what a caller could do before it:

    python tools/bench_lagrange.py [--reps 3] [--window 50] [--small] [--yardstick-only] [--out profiles/lagrange_time.txt]

For GF(2^8), GF(65537), GF(2^31 - 1), GF(2^64 - 2^32 + 1), k in {4, 16, 64, 256, 1024} points per row (k <= q) and batch in
{1, 2^10, 2^16} rows (where batch * k elements stay below 2^27):

  * kernel         one gfa_poly_lagrange call, every row with its own x
  * kernel shared  the same with one x for all rows (x_rows = 1)
  * matmul         shared x: the k basis polynomials from one call, then y @ basis on gfa_matmul
  * arrays         the whole-array route (fields of order >= 2^64, point counts above the cap), for batch <= 2^10 and k <= 64
  * yardstick      np.linalg.solve(np.power.outer(x, np.arange(k)), y) of ONE row -- what a caller could do before -- and that time
                   multiplied by the batch, since there is no batched solve.  It uses nothing this feature adds, so --yardstick-only
                   runs on a checkout that does not have it.

The routes are compared with each other before anything is timed.  Every figure is milliseconds per call, operands already on the
device and the status read back (the routes raise on a repeated x), measured as tools/bench_polyroots.py does: after one warm-up
call, one call is timed to size a loop of back-to-back calls that fills about --window milliseconds; the loop runs between two
device events, --reps times, and median / min / max of (window time / calls) are reported.  Then the threads of a packed workgroup
(gfa_debug_lagrange_tune) are varied for the short rows, and the last lines give the batch / k at which the matmul route overtakes
the shared-x kernel.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import galois_amd as ga  # noqa: E402

WINDOW_MS = 50.0
LINES = []
ORDERS = [("2^8", 2**8), ("65537", 65537), ("2^31 - 1", 2**31 - 1), ("2^64 - 2^32 + 1", 2**64 - 2**32 + 1)]
POINTS = [4, 16, 64, 256, 1024]
BATCHES = [1, 2**10, 2**16]
MAX_ELEMENTS = 2**27


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
    say(f"{name:58s} {calls:6d} {med:11.4f} {lo:11.4f} {hi:11.4f}  {note}")


def _points(GF, order, batch, k):
    """(x (batch, k) with distinct entries per row, y (batch, k)) on the device."""
    rng = np.random.default_rng(order % 2**32 + 7 * k + batch)
    i = np.arange(k, dtype=np.uint64)[None, :]  # distinct by construction: an image of 0 .. k - 1 per row
    if order <= 2**20:  # a * i + b mod q with a != 0 (prime q), or i ^ b
        b = rng.integers(0, order, (batch, 1), dtype=np.uint64)
        if order % 2 == 0:
            x = i ^ b
        else:
            x = (rng.integers(1, order, (batch, 1), dtype=np.uint64) * i + b) % np.uint64(order)
    else:  # b + a * i with a < 2^16 and b < q - 2^26: no wrap (random draws would repeat within some row of a large batch)
        x = rng.integers(0, order - 2**26, (batch, 1), dtype=np.uint64) + rng.integers(1, 2**16, (batch, 1), dtype=np.uint64) * i
    y = rng.integers(0, order, (batch, k), dtype=np.uint64)
    return GF(x), GF(y)


def yardstick(GF, x, y, k):
    V = np.power.outer(x, np.arange(k))  # V[i][j] = x_i^j
    return np.linalg.solve(V, y)  # coefficients, lowest degree first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--window", type=float, default=50.0, help="milliseconds of back-to-back calls per timed window")
    ap.add_argument("--small", action="store_true", help="two fields, k up to 64 and batch up to 2^10 only (rehearsal)")
    ap.add_argument("--yardstick-only", action="store_true", help="time only the route that existed before lagrange_poly")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    global WINDOW_MS, OUT
    WINDOW_MS, OUT = args.window, args.out
    say(f"device: {torch.cuda.get_device_name(0)}; milliseconds per call: median / min / max of {args.reps} windows of back-to-back calls "
        f"(about {WINDOW_MS:.0f} ms each) after one warm-up call")
    say(f"{'case':58s} {'calls':>6s} {'median':>11s} {'min':>11s} {'max':>11s}")
    orders = ORDERS[:2] if args.small else ORDERS
    points = POINTS[:3] if args.small else POINTS
    batches = BATCHES[:2] if args.small else BATCHES
    crossover = []  # (field, k, batch, shared kernel ms, matmul ms)
    for label, order in orders:
        GF = ga.GF(order)
        for k in points:
            if k > order:
                continue
            x1, y1 = _points(GF, order, 1, k)
            t_y = timed(lambda: yardstick(GF, x1[0], y1[0], k), args.reps)
            report(f"GF({label}), k = {k}: linalg.solve of one Vandermonde system", t_y)
            if args.yardstick_only:
                continue
            solved = yardstick(GF, x1[0], y1[0], k)
            assert np.array_equal(np.flip(solved), ga.lagrange_poly_batched(x1, y1, method="kernel")[0]), f"GF({label}), k = {k}: the yardstick disagrees"
            for batch in batches:
                if batch * k > MAX_ELEMENTS:
                    continue
                x, y = (x1, y1) if batch == 1 else _points(GF, order, batch, k)
                name = f"GF({label}), k = {k}, batch = {batch}"
                want = ga.lagrange_poly_batched(x, y, method="kernel")
                t_k = timed(lambda: ga.lagrange_poly_batched(x, y, method="kernel"), args.reps)
                report(f"{name}: kernel", t_k, f"{t_y[0] * batch / t_k[0]:.1f} x the yardstick's rate")
                if batch > 1 and (order < 2**32 or batch * k * k <= 2**33):  # (a 2^36-step product on 64-bit limbs takes half a minute)
                    xs = x[0]
                    shared = ga.lagrange_poly_batched(xs, y, method="kernel")
                    assert np.array_equal(ga.lagrange_poly_batched(xs, y, method="matmul"), shared), name
                    t_s = timed(lambda: ga.lagrange_poly_batched(xs, y, method="kernel"), args.reps)
                    report(f"{name}: kernel, shared x", t_s)
                    t_m = timed(lambda: ga.lagrange_poly_batched(xs, y, method="matmul"), args.reps)
                    report(f"{name}: matmul, shared x", t_m, f"kernel / matmul = {t_s[0] / t_m[0]:.2f}")
                    crossover.append((label, k, batch, t_s[0], t_m[0]))
                if batch <= 2**10 and k <= 64:
                    assert np.array_equal(ga.lagrange_poly_batched(x, y, method="arrays"), want), name
                    t_a = timed(lambda: ga.lagrange_poly_batched(x, y, method="arrays"), args.reps)
                    report(f"{name}: arrays", t_a, f"arrays / kernel = {t_a[0] / t_k[0]:.1f}")
    if not args.yardstick_only:
        from galois_amd import _lib as L

        say("threads of a workgroup that rows share (gfa_debug_lagrange_tune), batch = 2^16, own x per row:")
        for label, order in orders[1::2]:
            GF = ga.GF(order)
            for k in points[:3]:
                x, y = _points(GF, order, 2**16 if not args.small else 2**10, k)
                for threads in (64, 128, 256, 512, 1024):
                    L.lib().gfa_debug_lagrange_tune(threads)
                    t = timed(lambda: ga.lagrange_poly_batched(x, y, method="kernel"), args.reps)
                    report(f"GF({label}), k = {k}: {threads} threads, {threads // max(1, 1 << (k - 1).bit_length())} rows per workgroup", t)
                L.lib().gfa_debug_lagrange_tune(0)
        for label, k, batch, t_s, t_m in crossover:
            say(f"GF({label}), k = {k}: batch / k = {batch / k:g}: {'matmul' if t_m < t_s else 'kernel'} faster ({t_s:.4f} against {t_m:.4f} ms)")


if __name__ == "__main__":
    main()
