"""Times gfa_poly_classify (galois_amd/csrc/gfa_polytest.hip) on whole batches of candidates:

    python tools/bench_polytest.py [--reps 5] [--small]

  * every monic polynomial over GF(2) of degree 20 and over GF(3) of degree 10, irreducibility only and with primitivity;
  * 2^20 random monic candidates of degree 32 over GF(2^8) and of degree 64 over GF(2), irreducibility only;
  * what the compaction between the two launches saves: the second launch costs ("with primitivity" - "irreducibility
    only"); without compaction every wave that holds at least one irreducible row would run the primitivity powers, i.e. the
    cost of a dense batch of survivors (timed on its own, with and without primitivity) times the number of such waves over
    the number of dense waves -- printed as an estimate from the two timings and the flags;
  * for scale, the host path that existed before: _numtheory.is_irreducible, one candidate at a time, on the first 1000
    candidates of the GF(3) sweep.
Each figure is a time per CALL of gfa_poly_classify (a memset, the exponent upload and one or two launches), candidates already
on the device: after one warm-up call, one call is timed to size a loop of back-to-back calls that fills about --window
milliseconds; the loop runs between two device events, --reps times, and median / min / max of (window time / calls) are printed.
Back to back, a call costs the larger of its device time and its host enqueue time; rows/s is rows over that call time.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import galois_amd as ga  # noqa: E402
from galois_amd import _numtheory as nt  # noqa: E402
from galois_amd import _polysearch as PS  # noqa: E402


WINDOW_MS = 200.0


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


def report(name, n, stats):
    med, lo, hi, calls = stats
    print(f"{name:70s} {n:9d} {calls:6d} {med:10.4f} {lo:10.4f} {hi:10.4f} {n / med * 1e3:12.3e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=200.0, help="milliseconds of back-to-back calls per timed window")
    ap.add_argument("--small", action="store_true", help="2^16 random candidates instead of 2^20 (rehearsal)")
    args = ap.parse_args()
    global WINDOW_MS
    WINDOW_MS = args.window
    print(f"device: {torch.cuda.get_device_name(0)}; milliseconds per call: median / min / max of {args.reps} windows of back-to-back calls "
          f"(about {WINDOW_MS:.0f} ms each) after one warm-up call")
    print(f"{'case':70s} {'rows':>9s} {'calls':>6s} {'median':>10s} {'min':>10s} {'max':>10s} {'rows/s':>12s}")
    for q, m in ((2, 20), (3, 10)):
        GF = ga.GF(q)
        cand = PS._range_tensor(GF, m, 0, q**m)
        n = cand.shape[0]
        flags = PS._classify(GF, cand, True)
        n_irr, n_prim = int((flags & 1).sum()), int(((flags & 2) != 0).sum())
        t_irr = timed(lambda: PS._classify(GF, cand, False), args.reps)
        t_prim = timed(lambda: PS._classify(GF, cand, True), args.reps)
        report(f"GF({q}) degree {m} sweep, irreducibility only", n, t_irr)
        report(f"GF({q}) degree {m} sweep, with primitivity ({n_irr} -> {n_prim})", n, t_prim)
        dense = cand[(flags & 1) != 0].contiguous()
        d_irr = timed(lambda: PS._classify(GF, dense, False), args.reps)
        d_prim = timed(lambda: PS._classify(GF, dense, True), args.reps)
        report(f"GF({q}) degree {m}: the irreducible rows alone, irreducibility only", n_irr, d_irr)
        report(f"GF({q}) degree {m}: the irreducible rows alone, with primitivity", n_irr, d_prim)
        pad = torch.nn.functional.pad((flags & 1), (0, (-n) % 64)).reshape(-1, 64)
        waves_hit, waves_dense = int((pad.sum(dim=1) > 0).sum()), (n_irr + 63) // 64
        print(f"    second launch as built: {t_prim[0] - t_irr[0]:.4f} ms; ESTIMATE without compaction (no such kernel was run): {waves_hit} of "
              f"{pad.shape[0]} waves would run the powers instead of {waves_dense}, about {(d_prim[0] - d_irr[0]) * waves_hit / waves_dense:.4f} ms")
    rows = 1 << (16 if args.small else 20)
    gen = torch.Generator(device="cuda").manual_seed(1)
    for q, m in ((2**8, 32), (2, 64)):
        GF = ga.GF(q)
        cand = torch.randint(0, q, (rows, m + 1), dtype=torch.uint8, device="cuda", generator=gen)
        cand[:, 0] = 1
        flags = PS._classify(GF, cand, False)
        report(f"GF({q}) degree {m}, random monic ({int((flags & 1).sum())} irreducible)", rows, timed(lambda: PS._classify(GF, cand, False), args.reps))
    # the host path of the parent commit, for scale
    host = [nt.poly_from_int(3**10 + i, 3) for i in range(1000)]
    t0 = time.perf_counter()
    n_host = sum(nt.is_irreducible(f, 3) for f in host)
    dt = (time.perf_counter() - t0) * 1e3
    report(f"host _numtheory.is_irreducible, GF(3) degree 10 ({n_host} irreducible), whole loop", 1000, (dt, dt, dt, 1))


if __name__ == "__main__":
    main()
