"""
Generates tests/golden/sage_charpoly.npz (run in the build container only):

    python tests/golden/generate_charpoly_golden.py

The Sage vectors the reference's test-suite pins FieldArray.characteristic_poly() / minimal_poly() with
(/root/reference/tests/fields/data/*/{characteristic_poly_matrix,characteristic_poly_element,minimal_poly_element}.pkl),
re-packed as one compressed .npz because the pickles cannot travel to the GPU box.  Data only.  Per folder `tag`:

    {tag}/properties        the folder's properties.json, as a JSON string
    {tag}/cpm_count         number of matrix cases (five: 2x2 .. 6x6)
    {tag}/cpm{i}_X, _Z      the matrix and the coefficients of its characteristic polynomial, highest degree first
    {tag}/cpe_X, {tag}/mpe_X                 the elements
    {tag}/cpe_Z, {tag}/mpe_Z                 their polynomials over the prime subfield, concatenated
    {tag}/cpe_Zlen, {tag}/mpe_Zlen           ... and the number of coefficients of each

Folders of order >= 2^64 store every value as a decimal string (as pack_sage_wide_fields of generate_golden.py does).
"""
import json
import os
import pickle

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_DATA = "/root/reference/tests/fields/data"


def _tag(folder: str) -> str:
    return folder.replace("(", "_").replace(")", "").replace("^", "e").replace(", ", "_")


def _small(a: np.ndarray) -> np.ndarray:
    a = np.array([int(v) for v in a.ravel()], dtype=np.uint64).reshape(a.shape)
    mx = int(a.max()) if a.size else 0
    for dt in (np.uint8, np.uint16, np.uint32):
        if mx <= np.iinfo(dt).max:
            return a.astype(dt)
    return a


def _dec(a: np.ndarray) -> np.ndarray:
    return np.array([str(int(v)) for v in a.ravel()]).reshape(a.shape)


def pack(out_dir: str = HERE) -> str:
    out = {}
    for folder in sorted(os.listdir(REF_DATA)):
        path = os.path.join(REF_DATA, folder)
        props = json.load(open(os.path.join(path, "properties.json")))
        enc = _dec if props["order"] >= 2**64 else _small
        tag = _tag(folder)
        out[f"{tag}/properties"] = np.array(json.dumps(props))
        d = pickle.load(open(os.path.join(path, "characteristic_poly_matrix.pkl"), "rb"))
        out[f"{tag}/cpm_count"] = np.array(len(d["X"]))
        for i, (x, z) in enumerate(zip(d["X"], d["Z"])):
            out[f"{tag}/cpm{i}_X"] = enc(np.array(x, dtype=object))
            out[f"{tag}/cpm{i}_Z"] = enc(np.array(z, dtype=object))
        for key, name in (("cpe", "characteristic_poly_element"), ("mpe", "minimal_poly_element")):
            d = pickle.load(open(os.path.join(path, name + ".pkl"), "rb"))
            out[f"{tag}/{key}_X"] = enc(np.array(d["X"], dtype=object))
            out[f"{tag}/{key}_Zlen"] = np.array([len(z) for z in d["Z"]], dtype=np.int32)
            out[f"{tag}/{key}_Z"] = enc(np.array([v for z in d["Z"] for v in z], dtype=object))
    target = os.path.join(out_dir, "sage_charpoly.npz")
    np.savez_compressed(target, **out)
    return target


if __name__ == "__main__":
    print("packed", pack(os.environ.get("GOLDEN_OUT", HERE)))
