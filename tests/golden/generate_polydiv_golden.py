"""
Generates tests/golden/sage_polydiv.npz (run in the build container only):

    python tests/golden/generate_polydiv_golden.py

Known answers for divmod / // / % / ** / three-argument pow of Poly.  Data only.

(a) The Sage vectors /root/reference/tests/polys/data/*/{divmod,modular_power,power}.pkl of all 16 field folders, with the field
    parameters of the matching /root/reference/tests/fields/data/*/properties.json.  Per folder `tag`:
        sage/{tag}/properties                    the JSON string
        sage/{tag}/divmod_{X,Y,Q,R}              23 polynomials each, coefficients concatenated (highest degree first);
        sage/{tag}/divmod_{X,Y,Q,R}_len          their lengths
        sage/{tag}/modpow_{X,M,Z}, .._len        20 cases of pow(X, E, M) = Z;  sage/{tag}/modpow_E  the exponents
        sage/{tag}/power_X, .._len               5 polynomials;  sage/{tag}/power_Y  4 exponents
        sage/{tag}/power_Z, .._len               the 5 x 4 powers X[i] ** Y[j], i-major
    Coefficients are unsigned integers of the smallest width that holds them, and decimal strings in the three folders of
    order >= 2^64.
(b) Live answers of the reference (loaded through oracle/ref_shim/load_reference.py) for pow(f, e, g) with exponents beyond
    the Sage vectors (which stop at 10), over GF(2^8), GF(7^3) and GF(2^100):
        live/exponents                           2^64, 2^64 + 1234, 2^70 + 105030405 as decimal strings
        live/{tag}/irreducible_poly, .../primitive_element   the reference's (default) field parameters
        live/{tag}/f, live/{tag}/g               the operands (decimal strings)
        live/{tag}/z{k}                          pow(f, exponents[k], g)
"""
import json
import os
import pickle
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_POLYS = "/root/reference/tests/polys"
REF_FIELDS = "/root/reference/tests/fields/data"
EXPONENTS = [2**64, 2**64 + 1234, 2**70 + 105030405]
LIVE = {  # order: (f, g), highest degree first
    2**8: ([1, 0, 200, 3, 77], [1, 0, 0, 29, 0, 1, 255, 2, 90]),
    7**3: ([2, 0, 0, 341, 6], [300, 1, 0, 0, 0, 49, 5]),
    2**100: ([1, 2**99 + 12345, 0, 3], [2**100 - 1, 0, 0, 7, 2**64 + 1, 1]),
}


def _tag(folder: str) -> str:
    return folder.replace("(", "_").replace(")", "").replace("^", "e").replace(", ", "_")


def _reference():
    sys.path.insert(0, os.path.join(HERE, "..", ".."))
    from oracle.ref_shim import load_reference

    return load_reference


def _values(flat, wide: bool) -> np.ndarray:
    flat = [int(v) for v in flat]
    if wide:
        return np.array([str(v) for v in flat])
    mx = max(flat, default=0)
    for dt in (np.uint8, np.uint16, np.uint32):
        if mx <= np.iinfo(dt).max:
            return np.array(flat, dtype=dt)
    return np.array(flat, dtype=np.uint64)


def _polys(out: dict, key: str, polys, wide: bool):
    polys = [list(np.array(p, dtype=object).ravel()) for p in polys]
    out[key + "_len"] = np.array([len(p) for p in polys], dtype=np.int32)
    out[key] = _values([v for p in polys for v in p], wide)


def pack(out_dir: str = HERE) -> str:
    out = {}
    # (a) the Sage vectors
    for folder in sorted(os.listdir(os.path.join(REF_POLYS, "data"))):
        path = os.path.join(REF_POLYS, "data", folder)
        props = json.load(open(os.path.join(REF_FIELDS, folder, "properties.json")))
        wide = props["order"] >= 2**64
        tag = _tag(folder)
        out[f"sage/{tag}/properties"] = np.array(json.dumps(props))
        d = pickle.load(open(os.path.join(path, "divmod.pkl"), "rb"))
        for k in "XYQR":
            _polys(out, f"sage/{tag}/divmod_{k}", d[k], wide)
        d = pickle.load(open(os.path.join(path, "modular_power.pkl"), "rb"))
        for k in "XMZ":
            _polys(out, f"sage/{tag}/modpow_{k}", d[k], wide)
        out[f"sage/{tag}/modpow_E"] = np.array([int(e) for e in d["E"]], dtype=np.int64)
        d = pickle.load(open(os.path.join(path, "power.pkl"), "rb"))
        _polys(out, f"sage/{tag}/power_X", d["X"], wide)
        out[f"sage/{tag}/power_Y"] = np.array([int(e) for e in d["Y"]], dtype=np.int64)
        assert all(len(z) == len(d["Y"]) for z in d["Z"]) and len(d["Z"]) == len(d["X"])
        _polys(out, f"sage/{tag}/power_Z", [z for row in d["Z"] for z in row], wide)

    # (b) live answers for long exponents
    ref = _reference()
    galois = ref.load()
    out["live/exponents"] = np.array([str(e) for e in EXPONENTS])
    for order, (f, g) in LIVE.items():
        GF = ref.ref_field(order)
        tag = _tag(GF.name)
        pf = galois.Poly(GF(np.array(f, dtype=object) if order >= 2**64 else f))
        pg = galois.Poly(GF(np.array(g, dtype=object) if order >= 2**64 else g))
        out[f"live/{tag}/irreducible_poly"] = _values([int(c) for c in GF.irreducible_poly.coeffs], True)
        out[f"live/{tag}/primitive_element"] = np.array(str(int(GF.primitive_element)))
        out[f"live/{tag}/f"] = _values(f, True)
        out[f"live/{tag}/g"] = _values(g, True)
        for k, e in enumerate(EXPONENTS):
            out[f"live/{tag}/z{k}"] = _values([int(c) for c in pow(pf, e, pg).coeffs], True)

    target = os.path.join(out_dir, "sage_polydiv.npz")
    np.savez_compressed(target, **out)
    return target


if __name__ == "__main__":
    print("packed", pack(os.environ.get("GOLDEN_OUT", HERE)))
