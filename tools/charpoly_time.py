"""Times FieldArray.characteristic_poly() / characteristic_poly_batched next to np.linalg.det / det_batched (the existing
O(n^3) elimination) of the same input:

    python tools/charpoly_time.py [--n 1024] [--reps 3]

  * n x n over GF(65537), GF(2^8) and Goldilocks: the chip-wide regime (a few kernels per column);
  * a 4096-matrix stack of 32 x 32 over GF(2^8): one workgroup per matrix.
The ratio tells whether the similarity reduction (det-like work) or the recurrence and launch count dominate.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import galois_amd as ga  # noqa: E402
from galois_amd import linalg  # noqa: E402


def timed(fn, reps):
    fn()  # warm-up: module load, scratch pool growth
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        best = min(best, t0.elapsed_time(t1))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}; best of {args.reps} after one warm-up; milliseconds")
    print(f"{'case':44s} {'charpoly':>10s} {'det':>10s} {'ratio':>7s}")
    for name, GF in (("GF(65537)", ga.GF(65537)), ("GF(2^8)", ga.GF(2**8)), ("Goldilocks", ga.GF(2**64 - 2**32 + 1))):
        A = GF.Random((args.n, args.n), seed=1)
        cp = timed(lambda: A.characteristic_poly(), args.reps)
        dt = timed(lambda: np.linalg.det(A), args.reps)
        print(f"{name + f' {args.n} x {args.n} (chip-wide)':44s} {cp:10.3f} {dt:10.3f} {cp / dt:7.2f}")
    S = ga.GF(2**8).Random((4096, 32, 32), seed=2)
    cp = timed(lambda: linalg.characteristic_poly_batched(S), args.reps)
    dt = timed(lambda: linalg.det_batched(S), args.reps)
    print(f"{'GF(2^8) 4096 x (32 x 32) (one workgroup each)':44s} {cp:10.3f} {dt:10.3f} {cp / dt:7.2f}")


if __name__ == "__main__":
    main()
