"""
Generates tests/golden/reference_polytest.npz (run in the build container only):

    python tests/golden/generate_polytest_golden.py

Known answers for Poly.is_irreducible / is_primitive and the polynomial searches, all of them the reference's own data.
Data only.

(a) The reference's complete tables of monic irreducible / primitive polynomials
    (/root/reference/tests/polys/luts/irreducible_polys.py, primitive_polys.py), 26 (order, degree) entries each:
        tables                  the (order, degree) pairs
        irr/{q}_{m}, prim/{q}_{m}   (count, m + 1) coefficients, highest degree first, in lexicographic order
(b) The Sage vectors /root/reference/tests/polys/data/*/{is_irreducible,is_primitive}.pkl of the folders in which they are
    not empty, with the field parameters of the matching /root/reference/tests/fields/data/*/properties.json.  Per folder `tag`
    and list in {irr_IS, irr_IS_NOT, prim_IS, prim_IS_NOT}:
        sage/{tag}/properties   the JSON string
        sage/{tag}/{list}       the coefficients of all polynomials, concatenated;  sage/{tag}/{list}_len  their lengths
(c) Live answers of the reference (loaded through oracle/ref_shim/load_reference.py), over GF(2) unless said otherwise:
        live/min_degrees                  63, 64, 65, 127, 128, 129, 255
        live/min_irr_{m}                  the non-zero degrees of irreducible_poly(2, m, terms="min")
        live/min_irr_{m}_primitive        its is_primitive(), for m <= 128
        live/irr_2_24_terms3              irreducible_polys(2, 24, terms=3) as integers
        live/prim_2_61_min                the non-zero degrees of primitive_poly(2, 61, terms="min")
        live/irr_256_3                    the coefficients of irreducible_poly(2**8, 3)
        live/prim_256_2_max               the coefficients of primitive_poly(2**8, 2, method="max")
    Searches over odd or extension fields beyond these two take minutes to hours in the reference and are left out: their
    order follows from (a).
"""
import json
import os
import pickle
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_POLYS = "/root/reference/tests/polys"
REF_FIELDS = "/root/reference/tests/fields/data"
MIN_DEGREES = [63, 64, 65, 127, 128, 129, 255]


def _tag(folder: str) -> str:
    return folder.replace("(", "_").replace(")", "").replace("^", "e").replace(", ", "_")


def _small(a) -> np.ndarray:
    a = np.array(a, dtype=object)
    shape = a.shape
    a = np.array([int(v) for v in a.ravel()], dtype=np.uint64).reshape(shape)
    mx = int(a.max()) if a.size else 0
    for dt in (np.uint8, np.uint16, np.uint32):
        if mx <= np.iinfo(dt).max:
            return a.astype(dt)
    return a


def _reference():
    sys.path.insert(0, os.path.join(HERE, "..", ".."))
    from oracle.ref_shim import load_reference

    return load_reference


def pack(out_dir: str = HERE) -> str:
    ref = _reference()
    galois = ref.load()
    out = {}

    # (a) the complete tables
    sys.path.insert(0, REF_POLYS)
    from luts.irreducible_polys import IRREDUCIBLE_POLYS
    from luts.primitive_polys import PRIMITIVE_POLYS

    out["tables"] = np.array([(q, m) for q, m, _ in IRREDUCIBLE_POLYS], dtype=np.int64)
    assert [(q, m) for q, m, _ in PRIMITIVE_POLYS] == [(q, m) for q, m, _ in IRREDUCIBLE_POLYS]
    for key, table in (("irr", IRREDUCIBLE_POLYS), ("prim", PRIMITIVE_POLYS)):
        for q, m, polys in table:
            out[f"{key}/{q}_{m}"] = _small(polys).reshape(len(polys), m + 1)

    # (b) the Sage vectors
    for folder in sorted(os.listdir(os.path.join(REF_POLYS, "data"))):
        path = os.path.join(REF_POLYS, "data", folder)
        lists = {}
        for key, name in (("irr", "is_irreducible"), ("prim", "is_primitive")):
            d = pickle.load(open(os.path.join(path, name + ".pkl"), "rb"))
            lists[f"{key}_IS"], lists[f"{key}_IS_NOT"] = d["IS"], d["IS_NOT"]
        if not any(len(v) for v in lists.values()):
            continue
        tag = _tag(folder)
        out[f"sage/{tag}/properties"] = np.array(json.dumps(json.load(open(os.path.join(REF_FIELDS, folder, "properties.json")))))
        for name, polys in lists.items():
            out[f"sage/{tag}/{name}_len"] = np.array([len(p) for p in polys], dtype=np.int32)
            out[f"sage/{tag}/{name}"] = _small([v for p in polys for v in p])

    # (c) live answers
    out["live/min_degrees"] = np.array(MIN_DEGREES, dtype=np.int64)
    for m in MIN_DEGREES:
        f = galois.irreducible_poly(2, m, terms="min")
        out[f"live/min_irr_{m}"] = np.array([int(d) for d in f.nonzero_degrees], dtype=np.int64)
        if m <= 128:
            out[f"live/min_irr_{m}_primitive"] = np.array(bool(f.is_primitive()))
    out["live/irr_2_24_terms3"] = np.array([int(f) for f in galois.irreducible_polys(2, 24, terms=3)], dtype=np.uint64)
    out["live/prim_2_61_min"] = np.array([int(d) for d in galois.primitive_poly(2, 61, terms="min").nonzero_degrees], dtype=np.int64)
    ref.ref_field(2**8)
    out["live/irr_256_3"] = _small([int(c) for c in galois.irreducible_poly(2**8, 3).coeffs])
    out["live/prim_256_2_max"] = _small([int(c) for c in galois.primitive_poly(2**8, 2, method="max").coeffs])

    target = os.path.join(out_dir, "reference_polytest.npz")
    np.savez_compressed(target, **out)
    return target


if __name__ == "__main__":
    print("packed", pack(os.environ.get("GOLDEN_OUT", HERE)))
