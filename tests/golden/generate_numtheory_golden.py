"""
Generates tests/golden/sage_numtheory.json and tests/golden/reference_numtheory.json (run in the build container only):

    python tests/golden/generate_numtheory_golden.py

sage_numtheory.json: the Sage vectors the reference's own tests read, /root/reference/tests/data/{primes, kth_prime, prev_prime,
next_prime, is_prime, is_prime_power, is_perfect_power, is_square_free, is_smooth, is_powersmooth, euler_phi, carmichael_lambda,
is_cyclic, isqrt, iroot, ilog}.pkl, re-encoded as JSON: {name: {key: list}} with the pickles' own keys (X / N, B, R inputs, Z
outputs).

reference_numtheory.json: live answers of the reference, loaded through oracle/ref_shim/load_reference.py.  Data only:

    per_n/{function}        the answers for n = 1 .. 200 (index n - 1); a rejected argument is {"error": [type, message]}
    primitive_root          [[n, method, answer]] for the large moduli
    jacobi / kronecker      [[a, n, answer]] on a grid with negative a (and, for kronecker, negative and even n)
    legendre                [[a, p, answer]]
    pollard_rho / pollard_p1  [[args, answer]] on the inputs of the reference's docstrings
    errors                  [[function, args, kwargs, type, message]] for every rejected argument case
    misc                    single values quoted in the tests
"""
import json
import os
import pickle
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

SAGE = ["primes", "kth_prime", "prev_prime", "next_prime", "is_prime", "is_prime_power", "is_perfect_power", "is_square_free", "is_smooth",
        "is_powersmooth", "euler_phi", "carmichael_lambda", "is_cyclic", "isqrt", "iroot", "ilog"]

# (function, args, kwargs) that the reference rejects
REJECTED = [
    ("primes", [10.0], {}), ("kth_prime", [0], {}), ("kth_prime", [664580], {}), ("kth_prime", [3.0], {}), ("prev_prime", [1], {}),
    ("prev_prime", [2.0], {}), ("next_prime", [2.0], {}), ("random_prime", [0], {}), ("random_prime", [8.0], {}), ("random_prime", [8], {"seed": 1.0}),
    ("mersenne_exponents", [0], {}), ("mersenne_exponents", [2.0], {}), ("mersenne_primes", [0], {}),
    ("fermat_primality_test", [8], {"a": 3}), ("fermat_primality_test", [13], {"a": 12}), ("fermat_primality_test", [13], {"a": 2, "rounds": 0}),
    ("fermat_primality_test", [13.0], {}), ("miller_rabin_primality_test", [8], {}), ("miller_rabin_primality_test", [13], {"a": 1}),
    ("miller_rabin_primality_test", [13], {"rounds": 0}), ("miller_rabin_primality_test", [13], {"a": 2.0}),
    ("legendre_symbol", [3, 9], {}), ("legendre_symbol", [3, 2], {}), ("legendre_symbol", [3.0, 7], {}), ("jacobi_symbol", [3, 8], {}),
    ("jacobi_symbol", [3, 1], {}), ("jacobi_symbol", [3, -7], {}), ("jacobi_symbol", [3, 7.0], {}), ("kronecker_symbol", [3.0, 7], {}),
    ("perfect_power", [8.0], {}), ("trial_division", [1], {}), ("trial_division", [100], {"B": 2}), ("trial_division", [100.0], {}),
    ("pollard_p1", [8, 10], {}), ("pollard_p1", [15, 2], {}), ("pollard_p1", [15.0, 10], {}), ("pollard_p1", [1458757 * 1326001, 15], {}),
    ("pollard_rho", [1], {}), ("pollard_rho", [15], {"c": 0}), ("pollard_rho", [15], {"c": -2}), ("pollard_rho", [15.0], {}),
    ("divisors", [8.0], {}), ("divisor_sigma", [8.0], {}), ("is_prime", [7.0], {}), ("is_composite", [7.0], {}), ("is_prime_power", [7.0], {}),
    ("is_perfect_power", [7.0], {}), ("is_smooth", [10, 1], {}), ("is_smooth", [10.0, 2], {}), ("is_powersmooth", [10, 1], {}),
    ("is_powersmooth", [10, 2.0], {}), ("isqrt", [-1], {}), ("isqrt", [4.0], {}), ("iroot", [-1, 2], {}), ("iroot", [8, 0], {}),
    ("iroot", [8, 2.0], {}), ("ilog", [0, 2], {}), ("ilog", [8, 1], {}), ("ilog", [8.0, 2], {}), ("totatives", [0], {}), ("totatives", [8.0], {}),
    ("euler_phi", [0], {}), ("euler_phi", [8.0], {}), ("mobius", [0], {}), ("mobius", [8.0], {}), ("carmichael_lambda", [0], {}),
    ("carmichael_lambda", [8.0], {}), ("is_cyclic", [0], {}), ("is_cyclic", [8.0], {}), ("is_primitive_root", [2, 0], {}),
    ("is_primitive_root", [0, 7], {}), ("is_primitive_root", [7, 7], {}), ("is_primitive_root", [1, 1], {}), ("is_primitive_root", [2.0, 7], {}),
    ("primitive_root", [7], {"start": 0}), ("primitive_root", [7], {"start": 3, "stop": 3}), ("primitive_root", [7], {"stop": 8}),
    ("primitive_root", [7], {"method": "first"}), ("primitive_root", [8], {}), ("primitive_root", [7], {"start": 6}),
    ("primitive_root", [7.0], {}), ("primitive_root", [8], {"method": "random"}), ("primitive_roots", [7], {"start": 0}),
    ("primitive_roots", [7], {"stop": 8}), ("primitive_roots", [7], {"reverse": 1}), ("primitive_roots", [7.0], {}),
    ("are_coprime", [], {}), ("are_coprime", [3, 4.0], {}), ("is_square_free", [8.0], {}),
]

PER_N = ["totatives", "euler_phi", "mobius", "carmichael_lambda", "is_cyclic", "divisors", "divisor_sigma", "perfect_power", "trial_division"]


def _plain(v):
    """Tuples and generators as lists, bools and ints as themselves."""
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, bool):
        return v
    return int(v)


def _answer(fn, *args, **kwargs):
    try:
        out = fn(*args, **kwargs)
        if hasattr(out, "__next__"):
            out = list(out)
        return _plain(out)
    except Exception as e:  # recorded, with its type
        return {"error": [type(e).__name__, str(e)]}


def pack(out_dir: str = HERE):
    sage = {}
    for name in SAGE:
        with open(f"/root/reference/tests/data/{name}.pkl", "rb") as fh:
            sage[name] = {k: _plain(v) for k, v in pickle.load(fh).items()}
    with open(os.path.join(out_dir, "sage_numtheory.json"), "w") as fh:
        json.dump(sage, fh, separators=(",", ":"))

    from oracle.ref_shim.load_reference import load

    galois = load()
    ref = {"per_n": {}}
    for name in PER_N:
        ref["per_n"][name] = [_answer(getattr(galois, name), n) for n in range(1, 201)]
    ref["per_n"]["primitive_roots"] = [_answer(galois.primitive_roots, n) for n in range(1, 201)]
    ref["per_n"]["primitive_roots_reversed"] = [_answer(galois.primitive_roots, n, reverse=True) for n in range(1, 201)]
    ref["primitive_root"] = [[n, method, _answer(galois.primitive_root, n, method=method)]
                             for n in (2**61 - 1, 2 * 7**5, 1000000000000000035000061) for method in ("min", "max")]
    a_grid = [-1000003, -30, -7, -4, -3, -2, -1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 30, 1000003, 2**63 - 1, -(2**63), 2**70 + 7]
    ref["jacobi"] = [[a, n, _answer(galois.jacobi_symbol, a, n)] for a in a_grid for n in (3, 5, 9, 15, 21, 45, 1001, 2**32 - 5, 2**64 - 59, 2**70 + 25)]
    ref["kronecker"] = [[a, n, _answer(galois.kronecker_symbol, a, n)] for a in a_grid
                        for n in (-1001, -45, -16, -15, -8, -6, -4, -3, -2, -1, 0, 1, 2, 3, 4, 6, 8, 9, 12, 15, 16, 45, 1001, 2**64 - 59)]
    ref["legendre"] = [[a, p, _answer(galois.legendre_symbol, a, p)] for a in a_grid for p in (3, 5, 7, 13, 257, 65537, 2**61 - 1)]
    ref["pollard_rho"] = [[[n, c], _answer(galois.pollard_rho, n, c=c)] for n, c in
                          ((503**7 * 10007 * 1000003, 1), (1182640843 * 1716279751, 1), (1182640843 * 1716279751, 3), (503 * 1000003, 2), (15, 1),
                           (4, 1), (25, 1))]
    pq = 1458757 * 1326001
    ref["pollard_p1"] = [[[n, B, B2], _answer(galois.pollard_p1, n, B, B2=B2)] for n, B, B2 in
                         ((pq, 15, None), (pq, 17, None), (pq, 15, 100), (pq, 1039, None), (2133861346249, 10, None), (2133861346249, 15, None),
                          (15, 3, None))]
    ref["errors"] = []
    for name, args, kwargs in REJECTED:
        got = _answer(getattr(galois, name), *args, **kwargs)
        assert isinstance(got, dict), (name, args, kwargs, got)  # every case is one the reference rejects
        ref["errors"].append([name, args, kwargs] + got["error"])
    ref["misc"] = {
        "kth_prime(664579)": _answer(galois.kth_prime, 664579),
        "primitive_roots(18, reverse)": _answer(galois.primitive_roots, 18, reverse=True),
        "primitive_roots(4)": _answer(galois.primitive_roots, 4),
        "totatives(1)": _answer(galois.totatives, 1),
        "perfect_power": [[n, _answer(galois.perfect_power, n)] for n in (-729, -216, -64, -27, -16, -8, -4, -1, 0, 1, 2, 1000, 2**64, 3**40, 6**12)],
        "mersenne_exponents(2000)": _answer(galois.mersenne_exponents, 2000),
        "are_coprime": [[v, _answer(galois.are_coprime, *v)] for v in ([3, 4, 5], [3, 7, 9, 11], [6, 35], [-3, 5], [1], [0, 5])],
        "is_square_free": [[n, _answer(galois.is_square_free, n)] for n in (-12, -6, 0, 1, 6, 12, 2 * 3 * 5 * 7, 49)],
        "primitive_roots(2*7^5)[start, stop)": _answer(galois.primitive_roots, 2 * 7**5, start=1000, stop=1100),
    }
    with open(os.path.join(out_dir, "reference_numtheory.json"), "w") as fh:
        json.dump(ref, fh, separators=(",", ":"))
    return sage, ref


if __name__ == "__main__":
    sage, ref = pack()
    for name in ("sage_numtheory.json", "reference_numtheory.json"):
        print(name, os.path.getsize(os.path.join(HERE, name)), "bytes")
