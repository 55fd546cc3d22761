"""Times both routes of the routed functions of galois_amd/_integers.py, to place their crossovers:

    python tools/bench_integers.py [--reps 5] [--small] [--out profiles/integers_time.txt]

  * primes(n): the host sieve against the device sieve plus the copy of the list back, n = 2^16 .. 2^28 (PRIMES_DEVICE_FROM)
  * primes_in_range: the sieve against the primality kernel over the odd candidates, windows of 2^10 .. 2^24 integers ending at
    2^32 and at 2^40 (SIEVE_WINDOW_FACTOR: the sieve pays sqrt(stop) base primes per segment, the test pays per candidate)
  * totatives(n): the host loop against the classifier, n = 2^10 .. 2^22 (TOTATIVES_DEVICE_FROM)
  * primitive_roots: list(...) of all roots of a prime modulus on either route, and the time to the first root
  * the kernels alone, device to device: gfa_int_is_prime on 2^24 odd 64-bit candidates, gfa_int_jacobi on 2^24 pairs,
    gfa_int_unit_classify with the exponents of 2^61 - 1 on 2^20 candidates

The routes are compared for equality before anything is timed.  Figures are wall-clock milliseconds per call, the device
synchronised before the clock is read, median / min / max of --reps calls after one warm-up call.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import galois_amd as ga  # noqa: E402
from galois_amd import _integers as gi  # noqa: E402

LINES = []
OUT = None  # --out: rewritten after every line, so that a run cut short keeps what it measured


def say(line):
    print(line, flush=True)
    LINES.append(line)
    if OUT:
        with open(OUT, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out)), float(min(out)), float(max(out))


def row(what, fn, reps, items=None):
    med, lo, hi = timed(fn, reps)
    rate = f"  {items / med / 1e3:10.2f} M items/s" if items else ""
    say(f"{what:<64s} {med:10.3f} ms  [{lo:.3f}, {hi:.3f}]{rate}")
    return med


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="the small half of every sweep")
    ap.add_argument("--out")
    args = ap.parse_args()
    OUT = args.out
    reps = args.reps
    say(f"device: {torch.cuda.get_device_name(0)}; sieve segment span {ga.sieve_segment_span()}")

    say("-- primes(n): host sieve | device sieve + list")
    for k in range(16, 25 if args.small else 29, 2):
        n = 1 << k
        assert ga.primes(n, _route="host") == ga.primes(n, _route="device")
        h = row(f"primes(2^{k}) host", lambda: ga.primes(n, _route="host"), reps, n)
        d = row(f"primes(2^{k}) device", lambda: ga.primes(n, _route="device"), reps, n)
        row(f"primes_in_range(0, 2^{k}) (tensor stays on the device)", lambda: ga.primes_in_range(0, n, _route="sieve"), reps, n)
        say(f"   host / device = {h / d:.2f}")

    say("-- primes_in_range windows: sieve | primality kernel")
    for top in (1 << 32, 1 << 40):
        for k in range(10, 21 if args.small else 25, 2):
            lo = top - (1 << k)
            assert torch.equal(ga.primes_in_range(lo, top, _route="sieve"), ga.primes_in_range(lo, top, _route="test"))
            s = row(f"[{top} - 2^{k}, {top}) sieve", lambda: ga.primes_in_range(lo, top, _route="sieve"), reps, 1 << k)
            t = row(f"[{top} - 2^{k}, {top}) test", lambda: ga.primes_in_range(lo, top, _route="test"), reps, 1 << k)
            say(f"   test / sieve = {t / s:.2f}; window * {gi.SIEVE_WINDOW_FACTOR} >= isqrt(stop): {(1 << k) * gi.SIEVE_WINDOW_FACTOR >= int(top**0.5)}")

    say("-- totatives(n): host loop | classifier")
    for k in range(10, 19 if args.small else 23, 2):
        n = (1 << k) + 2  # twice an odd number
        assert ga.totatives(n, _route="host") == ga.totatives(n, _route="device")
        h = row(f"totatives(2^{k} + 2) host", lambda: ga.totatives(n, _route="host"), reps, n)
        d = row(f"totatives(2^{k} + 2) device", lambda: ga.totatives(n, _route="device"), reps, n)
        say(f"   host / device = {h / d:.2f}")

    say("-- primitive_roots(p): all of them, and the first")
    for p in (65537,) if args.small else (65537, 786433):
        assert list(ga.primitive_roots(p, _route="host")) == list(ga.primitive_roots(p, _route="device"))
        row(f"list(primitive_roots({p})) host", lambda: list(ga.primitive_roots(p, _route="host")), reps, p)
        row(f"list(primitive_roots({p})) device", lambda: list(ga.primitive_roots(p, _route="device")), reps, p)
        row(f"list(primitive_roots({p})) host chunk, then device", lambda: list(ga.primitive_roots(p)), reps, p)
    for n in (2**61 - 1, 2**64 - 59):
        row(f"primitive_root({n}) host", lambda: ga.primitive_root(n, _route="host"), reps)
        row(f"primitive_root({n}) device", lambda: ga.primitive_root(n, _route="device"), reps)

    say("-- the kernels alone")
    count = 1 << (20 if args.small else 24)
    row(f"gfa_int_is_prime, {count} odd candidates below 2^64", lambda: gi._is_prime_range(2**64 - 2 * count - 1, 2, count), reps, count)
    row(f"gfa_int_is_prime, {count} odd candidates from 2^32", lambda: gi._is_prime_range(2**32 + 1, 2, count), reps, count)
    a = torch.randint(-(2**62), 2**62, (count,), dtype=torch.int64, device="cuda")
    from galois_amd import _lib as L
    import ctypes

    out = torch.empty(count, dtype=torch.int8, device="cuda")
    n_arg = ctypes.c_uint64(2**64 - 59)
    row(f"gfa_int_jacobi, {count} pairs, n = 2^64 - 59",
        lambda: L.check(L.lib().gfa_int_jacobi(a.data_ptr(), ctypes.addressof(n_arg), count, 0, out.data_ptr(), None)), reps, count)
    n = 2**61 - 1
    exps = gi._phi_exponents(n)[1]
    small = 1 << 20
    row(f"gfa_int_unit_classify, {small} candidates, n = 2^61 - 1, {len(exps)} exponents", lambda: gi._classify_range(n, 2, 1, small, exps), reps, small)
    row(f"gfa_int_unit_classify, {count} candidates, units only, n = 510510", lambda: gi._classify_range(510510, 1, 1, count, ()), reps, count)


if __name__ == "__main__":
    main()
