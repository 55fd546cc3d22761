"""
Generates tests/golden/sage_lagrange.npz (run in the build container only):

    python tests/golden/generate_lagrange_golden.py

The Sage vectors /root/reference/tests/polys/data/*/lagrange_poly.pkl and crt.pkl of all 16 field folders, with the field
parameters of the matching /root/reference/tests/fields/data/*/properties.json.  Data only.  Per folder `tag`:

    sage/{tag}/properties          the JSON string
    sage/{tag}/LX, LX_len          lagrange_poly: the abscissae of the 3 cases, concatenated, and how many each case has
    sage/{tag}/LY, LY_len          the ordinates, likewise
    sage/{tag}/LZ, LZ_len          the coefficients of the interpolating polynomials (highest degree first), and their lengths
    sage/{tag}/CN                  crt: how many congruences each of the 20 cases has
    sage/{tag}/CX, CX_len          the remainders of all cases in turn, coefficients concatenated, and their lengths
    sage/{tag}/CY, CY_len          the moduli, likewise
    sage/{tag}/CZ, CZ_len          the solutions, and their lengths: -1 where the system has no solution (Z is None)

Values are unsigned integers of the smallest width that holds them, and decimal strings in the three folders of order >= 2^64.
"""
import json
import os
import pickle

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_POLYS = "/root/reference/tests/polys"
REF_FIELDS = "/root/reference/tests/fields/data"


def _tag(folder: str) -> str:
    return folder.replace("(", "_").replace(")", "").replace("^", "e").replace(", ", "_")


def _values(flat, wide: bool) -> np.ndarray:
    flat = [int(v) for v in flat]
    if wide:
        return np.array([str(v) for v in flat])
    mx = max(flat, default=0)
    for dt in (np.uint8, np.uint16, np.uint32):
        if mx <= np.iinfo(dt).max:
            return np.array(flat, dtype=dt)
    return np.array(flat, dtype=np.uint64)


def _lists(out: dict, key: str, lists, wide: bool):
    """`lists`: one sequence of values per entry, or None for an entry that is absent (length -1)."""
    lists = [None if p is None else list(np.array(p, dtype=object).ravel()) for p in lists]
    out[key + "_len"] = np.array([-1 if p is None else len(p) for p in lists], dtype=np.int32)
    out[key] = _values([v for p in lists if p is not None for v in p], wide)


def pack(out_dir: str = HERE) -> str:
    out = {}
    for folder in sorted(os.listdir(os.path.join(REF_POLYS, "data"))):
        props = json.load(open(os.path.join(REF_FIELDS, folder, "properties.json")))
        wide = props["order"] >= 2**64
        tag = _tag(folder)
        out[f"sage/{tag}/properties"] = np.array(json.dumps(props))
        d = pickle.load(open(os.path.join(REF_POLYS, "data", folder, "lagrange_poly.pkl"), "rb"))
        assert len(d["X"]) == len(d["Y"]) == len(d["Z"]) == 3
        for key in "XYZ":
            _lists(out, f"sage/{tag}/L{key}", d[key], wide)
        d = pickle.load(open(os.path.join(REF_POLYS, "data", folder, "crt.pkl"), "rb"))
        assert len(d["X"]) == len(d["Y"]) == len(d["Z"]) == 20 and all(len(a) == len(m) for a, m in zip(d["X"], d["Y"]))
        out[f"sage/{tag}/CN"] = np.array([len(a) for a in d["X"]], dtype=np.int32)
        _lists(out, f"sage/{tag}/CX", [p for case in d["X"] for p in case], wide)
        _lists(out, f"sage/{tag}/CY", [p for case in d["Y"] for p in case], wide)
        _lists(out, f"sage/{tag}/CZ", d["Z"], wide)
    target = os.path.join(out_dir, "sage_lagrange.npz")
    np.savez_compressed(target, **out)
    return target


if __name__ == "__main__":
    print("packed", pack(os.environ.get("GOLDEN_OUT", HERE)))
