"""
Generates tests/golden/reference_elements.npz (run in the build container only):

    python tests/golden/generate_elements_golden.py

Known answers for the primitive / normal element functions, all of them the reference's own data.  Data only.

(a) The 22 recorded lists of /root/reference/tests/fields/luts/{normal,primitive}_elements_{2,3,5}.py -- (p, m) = (2, 2..6),
    (3, 2..4), (5, 2..4), every primitive and every normal element of GF(p^m) on its Conway polynomial, from Sage.  The literal
    lists are read out of the syntax tree; nothing of the files is executed.
        tables                      the (p, m) pairs
        normal/{p}_{m}, primitive/{p}_{m}   the elements as integers (radix-p digits = coefficients), in the recorded (ascending) order
(b) Live answers of the reference (loaded through oracle/ref_shim/load_reference.py): is_normal_element and is_primitive_element
    of EVERY residue modulo irreducible_poly(q, m) -- the lexicographically first monic irreducible polynomial, which is also the
    first of this project's search order -- for (q, m) = (4, 2) (p | m: x^2 - 1 = (x - 1)^2), (4, 3) (x^3 - 1 splits completely),
    (9, 2) and (8, 2):
        live                        the (q, m) pairs
        live/{q}_{m}/poly           the m + 1 coefficients of the polynomial, highest degree first
        live/{q}_{m}/normal, live/{q}_{m}/primitive   q^m flags, indexed by the integer of the residue
"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LUTS = "/root/reference/tests/fields/luts"
TABLES = [(2, m) for m in range(2, 7)] + [(3, m) for m in range(2, 5)] + [(5, m) for m in range(2, 5)]
LIVE = [(4, 2), (4, 3), (9, 2), (8, 2)]


def _lists(path: str) -> dict:
    """name -> literal list of every top-level `NAME = [...]` of a file."""
    out = {}
    for stmt in ast.parse(open(path).read()).body:
        if isinstance(stmt, ast.Assign) and len(stmt.targets) == 1 and isinstance(stmt.targets[0], ast.Name) and isinstance(stmt.value, ast.List):
            try:
                out[stmt.targets[0].id] = ast.literal_eval(stmt.value)
            except ValueError:
                pass  # a list of names (the index of the tables), not of numbers
    return out


def _integer(coeffs, p: int) -> int:
    v = 0
    for c in coeffs:
        v = v * p + int(c)
    return v


def pack(out_dir: str = HERE) -> str:
    out = {"tables": np.array(TABLES, dtype=np.int64)}
    for kind in ("normal", "primitive"):
        for p in (2, 3, 5):
            lists = _lists(os.path.join(LUTS, f"{kind}_elements_{p}.py"))
            for q, m in TABLES:
                if q != p:
                    continue
                rows = lists[f"{kind.upper()}_ELEMENTS_{p}_{m}"]
                assert rows and all(1 <= len(r) <= m for r in rows), (kind, p, m)
                ints = [_integer(r, p) for r in rows]
                assert ints == sorted(set(ints)) and ints[-1] < p**m
                out[f"{kind}/{p}_{m}"] = np.array(ints, dtype=np.int64)

    sys.path.insert(0, os.path.join(HERE, "..", ".."))
    from oracle.ref_shim import load_reference as ref

    galois = ref.load()
    out["live"] = np.array(LIVE, dtype=np.int64)
    for q, m in LIVE:
        GF = ref.ref_field(q)
        f = galois.irreducible_poly(q, m)
        out[f"live/{q}_{m}/poly"] = np.array([int(c) for c in f.coeffs], dtype=np.uint8)
        normal, primitive = [], []
        for v in range(q**m):
            g = galois.Poly.Int(v, field=GF)
            normal.append(bool(galois.is_normal_element(g, f)))
            primitive.append(bool(galois.is_primitive_element(g, f)))
        out[f"live/{q}_{m}/normal"] = np.array(normal, dtype=np.uint8)
        out[f"live/{q}_{m}/primitive"] = np.array(primitive, dtype=np.uint8)

    target = os.path.join(out_dir, "reference_elements.npz")
    np.savez_compressed(target, **out)
    return target


if __name__ == "__main__":
    print("packed", pack(os.environ.get("GOLDEN_OUT", HERE)))
