"""
Generates tests/golden/sage_polygcd.npz (run in the build container only):

    python tests/golden/generate_polygcd_golden.py

Known answers for gcd / egcd / lcm / prod of Poly and for the factorisation methods.  Data only.

(a) The Sage vectors /root/reference/tests/polys/data/*/{egcd,lcm,prod,is_square_free}.pkl of all 16 field folders, with the field
    parameters of the matching /root/reference/tests/fields/data/*/properties.json.  Per folder `tag`:
        sage/{tag}/properties                    the JSON string
        sage/{tag}/egcd_{X,Y,D,S,T}, .._len      polynomials, coefficients concatenated (highest degree first), and their lengths:
                                                 egcd(X, Y) = (D, S, T)
        sage/{tag}/{lcm,prod}_X, .._len          the arguments of all cases in turn;  {lcm,prod}_X_count  how many each case has
        sage/{tag}/{lcm,prod}_Z, .._len          the answers
        sage/{tag}/sqfree_X, .._len, sqfree_Z    polynomials and whether each is square-free
    Coefficients are unsigned integers of the smallest width that holds them, and decimal strings in the three folders of
    order >= 2^64.
(b) Live answers of the reference (loaded through oracle/ref_shim/load_reference.py) for the polynomials of LIVE below: the monic
    polynomial with the pseudo-random coefficients of _fixed(order, degree), times the square of the cubic _fixed(order, 3).
        live/{tag}/irreducible_poly, .../primitive_element   the reference's (default) field parameters
        live/{tag}/f                             the polynomial
        live/{tag}/factors, .._len, factors_mult             f.factors()
        live/{tag}/sf, .._len, sf_mult                       f.square_free_factors()
        live/{tag}/ddf, .._len, ddf_deg                      sf[0].distinct_degree_factors()
        live/{tag}/edf{k}, .._len                            ddf[k].equal_degree_factors(ddf_deg[k])
(c) Constructed products over GF(2^8) and GF(2^32), where the reference's equal-degree splitting is too slow to be called
    (characteristic 2): irreducible polynomials from the reference's irreducible_polys, each confirmed by its is_irreducible(),
    multiplied with the multiplicities of BUILT below -- at least three of one degree, and a repeated one.
        built/{tag}/irreducible_poly, .../primitive_element
        built/{tag}/f                            the product
        built/{tag}/factors, .._len, factors_mult            the irreducible polynomials sorted by their integer value, and their
                                                             multiplicities: what f.factors() must return
"""
import itertools
import json
import os
import pickle
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_POLYS = "/root/reference/tests/polys"
REF_FIELDS = "/root/reference/tests/fields/data"
LIVE = [(2, 40), (3, 30), (5, 25), (4, 20), (9, 20), (25, 20), (7**3, 12), (3191, 12), (2**31 - 1, 8)]  # (order, degree)
# order: [(degree, how many irreducible polynomials of it, skipping `skip` between two, multiplicity of each, from the
# lexicographically last downwards?)] -- over GF(2^32) the first 2^32 quadratics, x^2 + c, are all squares
BUILT = {
    2**8: [(1, 1, 0, 2, False), (2, 4, 5, 1, False), (3, 3, 2, 1, False)],
    2**32: [(1, 1, 0, 3, False), (2, 3, 1, 1, True)],
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


def _fixed(order: int, degree: int) -> list:
    """The monic polynomial of the degree whose other coefficients come from a linear congruential sequence."""
    state, coeffs = 12345 + order + degree, [1]
    for _ in range(degree):
        state = (state * 6364136223846793005 + 1442695040888963407) % 2**64
        coeffs.append((state >> 33) % order)
    return coeffs


def _coeffs(poly) -> list:
    return [int(c) for c in poly.coeffs]


def pack(out_dir: str = HERE) -> str:
    out = {}
    # (a) the Sage vectors
    for folder in sorted(os.listdir(os.path.join(REF_POLYS, "data"))):
        path = os.path.join(REF_POLYS, "data", folder)
        props = json.load(open(os.path.join(REF_FIELDS, folder, "properties.json")))
        wide = props["order"] >= 2**64
        tag = _tag(folder)
        out[f"sage/{tag}/properties"] = np.array(json.dumps(props))
        d = pickle.load(open(os.path.join(path, "egcd.pkl"), "rb"))
        for k in "XYDST":
            _polys(out, f"sage/{tag}/egcd_{k}", d[k], wide)
        for name in ("lcm", "prod"):
            d = pickle.load(open(os.path.join(path, f"{name}.pkl"), "rb"))
            assert len(d["X"]) == len(d["Z"])
            out[f"sage/{tag}/{name}_X_count"] = np.array([len(case) for case in d["X"]], dtype=np.int32)
            _polys(out, f"sage/{tag}/{name}_X", [p for case in d["X"] for p in case], wide)
            _polys(out, f"sage/{tag}/{name}_Z", d["Z"], wide)
        d = pickle.load(open(os.path.join(path, "is_square_free.pkl"), "rb"))
        _polys(out, f"sage/{tag}/sqfree_X", d["X"], wide)
        out[f"sage/{tag}/sqfree_Z"] = np.array([bool(z) for z in d["Z"]])

    ref = _reference()
    galois = ref.load()

    def field_parameters(key, GF):
        out[f"{key}/irreducible_poly"] = _values(_coeffs(GF.irreducible_poly), True)
        out[f"{key}/primitive_element"] = np.array(str(int(GF.primitive_element)))

    # (b) live answers
    for order, degree in LIVE:
        GF = ref.ref_field(order)
        key = f"live/{_tag(GF.name)}"
        cubic = galois.Poly(_fixed(order, 3), field=GF)
        f = galois.Poly(_fixed(order, degree), field=GF) * cubic**2
        field_parameters(key, GF)
        out[f"{key}/f"] = _values(_coeffs(f), False)
        g, m = f.factors()
        _polys(out, f"{key}/factors", [_coeffs(p) for p in g], False)
        out[f"{key}/factors_mult"] = np.array(m, dtype=np.int32)
        sf, m = f.square_free_factors()
        _polys(out, f"{key}/sf", [_coeffs(p) for p in sf], False)
        out[f"{key}/sf_mult"] = np.array(m, dtype=np.int32)
        ddf, degs = sf[0].distinct_degree_factors()
        _polys(out, f"{key}/ddf", [_coeffs(p) for p in ddf], False)
        out[f"{key}/ddf_deg"] = np.array(degs, dtype=np.int32)
        for k, (p, dg) in enumerate(zip(ddf, degs)):
            _polys(out, f"{key}/edf{k}", [_coeffs(e) for e in p.equal_degree_factors(int(dg))], False)

    # (c) constructed products in characteristic 2
    for order, plan in BUILT.items():
        GF = ref.ref_field(order)
        key = f"built/{_tag(GF.name)}"
        field_parameters(key, GF)
        parts = []
        for degree, count, skip, mult, reverse in plan:
            polys = itertools.islice(galois.irreducible_polys(order, degree, reverse=reverse), 0, count * (skip + 1), skip + 1)
            for p in polys:
                p = galois.Poly(_coeffs(p), field=GF)
                assert p.degree == degree and p.is_irreducible()
                parts.append((p, mult))
        parts.sort(key=lambda item: int(item[0]))
        f = galois.Poly([1], field=GF)
        for p, mult in parts:
            f = f * p**mult
        out[f"{key}/f"] = _values(_coeffs(f), False)
        _polys(out, f"{key}/factors", [_coeffs(p) for p, _ in parts], False)
        out[f"{key}/factors_mult"] = np.array([mult for _, mult in parts], dtype=np.int32)

    target = os.path.join(out_dir, "sage_polygcd.npz")
    np.savez_compressed(target, **out)
    return target


if __name__ == "__main__":
    print("packed", pack(os.environ.get("GOLDEN_OUT", HERE)))
