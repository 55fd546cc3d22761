"""
Generates tests/golden/sage_polyroots.npz (run in the build container only):

    python tests/golden/generate_polyroots_golden.py

The Sage vectors /root/reference/tests/polys/data/*/roots.pkl of all 16 field folders -- polynomials X, their roots R in
increasing order and the multiplicities M of those roots -- with the field parameters of the matching
/root/reference/tests/fields/data/*/properties.json.  Data only.  Per folder `tag`:

    sage/{tag}/properties          the JSON string
    sage/{tag}/X, X_len            the polynomials, coefficients concatenated (highest degree first), and their lengths
    sage/{tag}/R, R_len            the roots of all polynomials in turn, and how many each has (0 for a polynomial without roots)
    sage/{tag}/M                   the multiplicities, in the order of R

Coefficients and roots are unsigned integers of the smallest width that holds them, and decimal strings in the three folders of
order >= 2^64.
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
    lists = [list(np.array(p, dtype=object).ravel()) for p in lists]
    out[key + "_len"] = np.array([len(p) for p in lists], dtype=np.int32)
    out[key] = _values([v for p in lists for v in p], wide)


def pack(out_dir: str = HERE) -> str:
    out = {}
    for folder in sorted(os.listdir(os.path.join(REF_POLYS, "data"))):
        props = json.load(open(os.path.join(REF_FIELDS, folder, "properties.json")))
        wide = props["order"] >= 2**64
        tag = _tag(folder)
        d = pickle.load(open(os.path.join(REF_POLYS, "data", folder, "roots.pkl"), "rb"))
        assert len(d["X"]) == len(d["R"]) == len(d["M"])
        out[f"sage/{tag}/properties"] = np.array(json.dumps(props))
        _lists(out, f"sage/{tag}/X", d["X"], wide)
        _lists(out, f"sage/{tag}/R", d["R"], wide)
        mult = [[int(m) for m in np.array(ms, dtype=object).ravel()] for ms in d["M"]]
        assert [len(ms) for ms in mult] == list(out[f"sage/{tag}/R_len"])
        out[f"sage/{tag}/M"] = np.array([m for ms in mult for m in ms], dtype=np.int32)
    target = os.path.join(out_dir, "sage_polyroots.npz")
    np.savez_compressed(target, **out)
    return target


if __name__ == "__main__":
    print("packed", pack(os.environ.get("GOLDEN_OUT", HERE)))
