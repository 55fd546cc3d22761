"""tests/golden/sage_lagrange.npz is the reference's own data: regenerated from its Sage pickles it must come out array for array as
committed (needs the reference checkout), every interpolating polynomial passes through its points and every crt solution leaves its
remainders -- checked on Python integers through the oracle's field arithmetic (oracle/wide_oracle.py restates the reference's
formulas for every (p, m), so all 16 folders are covered).  No GPU."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest

from oracle.wide_oracle import WideOracle
from tests import helpers as H

REF_POLYS = "/root/reference/tests/polys"
GOLDEN = os.path.join(H.GOLDEN, "sage_lagrange.npz")
TAGS = sorted(k.split("/")[1] for k in np.load(GOLDEN).keys() if k.endswith("/properties"))


@functools.lru_cache(maxsize=None)
def _golden():
    d = np.load(GOLDEN)
    return {k: d[k] for k in d.keys()}


def _lists(key):
    g = _golden()
    flat, out, at = [int(v) for v in g[key]], [], 0
    for n in g[key + "_len"]:
        out.append(None if n < 0 else flat[at:at + n])
        at += max(int(n), 0)
    return out


@pytest.mark.skipif(not os.path.isdir(REF_POLYS), reason="the reference checkout is not on this machine")
def test_sage_lagrange_fixture_regenerates_identically(tmp_path):
    spec = importlib.util.spec_from_file_location("generate_lagrange_golden", os.path.join(H.GOLDEN, "generate_lagrange_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fresh = np.load(gen.pack(str(tmp_path)))
    committed = np.load(GOLDEN)
    assert sorted(fresh.keys()) == sorted(committed.keys())
    for k in fresh.keys():
        a, b = fresh[k], committed[k]
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), k
    assert len(fresh.keys()) == 16 * 14  # properties, LX LY LZ CX CY CZ with their lengths, CN


def test_all_sage_folders_present_with_the_shape_the_device_tests_rely_on():
    assert len(TAGS) == 16
    g = _golden()
    wide = [t for t in TAGS if json.loads(str(g[f"sage/{t}/properties"]))["order"] >= 2**64]
    assert sorted(wide) == ["GF_109987e4", "GF_2e100", "GF_36893488147419103183"] and all(g[f"sage/{t}/LX"].dtype.kind == "U" for t in wide)
    unsolvable = 0
    for t in TAGS:
        assert list(g[f"sage/{t}/LX_len"]) == list(g[f"sage/{t}/LY_len"]) and len(g[f"sage/{t}/LX_len"]) == 3
        assert all(1 <= z <= x for z, x in zip(g[f"sage/{t}/LZ_len"], g[f"sage/{t}/LX_len"]))
        cn, cz = g[f"sage/{t}/CN"], g[f"sage/{t}/CZ_len"]
        assert len(cn) == len(cz) == 20 and cn.min() >= 2 and int(cn.sum()) == len(g[f"sage/{t}/CX_len"]) == len(g[f"sage/{t}/CY_len"])
        assert g[f"sage/{t}/CX_len"].min() >= 1 and g[f"sage/{t}/CY_len"].min() >= 2
        unsolvable += int((cz < 0).sum())
    assert unsolvable >= 1


@pytest.mark.parametrize("tag", TAGS)
def test_listed_polynomials_interpolate_and_listed_solutions_leave_the_remainders(tag):
    props = json.loads(str(_golden()[f"sage/{tag}/properties"]))
    p, m = props["characteristic"], props["degree"]
    K = WideOracle(p, m, [int(c) for c in props["irreducible_poly"]] if m > 1 else None)

    def horner(f, x):
        acc = 0
        for c in f:
            acc = K.add(K.mul(acc, x), c)
        return acc

    def remainder(f, d):
        """f mod d, coefficients highest degree first."""
        f, lead = list(f), K.div(1, d[0])
        for i in range(len(f) - len(d) + 1):
            q = K.mul(f[i], lead)
            for j, c in enumerate(d):
                f[i + j] = K.sub(f[i + j], K.mul(q, c))
        r = f[max(len(f) - len(d) + 1, 0):]
        while len(r) > 1 and r[0] == 0:
            r = r[1:]
        return r or [0]

    for x, y, z in zip(_lists(f"sage/{tag}/LX"), _lists(f"sage/{tag}/LY"), _lists(f"sage/{tag}/LZ")):
        assert len(set(x)) == len(x) == len(y) and len(z) <= len(x)
        assert [horner(z, xi) for xi in x] == y, f"{tag}: {z}"
    n = [int(v) for v in _golden()[f"sage/{tag}/CN"]]
    ends = np.cumsum(n)
    X, Y, Z = _lists(f"sage/{tag}/CX"), _lists(f"sage/{tag}/CY"), _lists(f"sage/{tag}/CZ")
    for i, z in enumerate(Z):
        if z is None:
            continue
        for a, mod in zip(X[ends[i] - n[i]:ends[i]], Y[ends[i] - n[i]:ends[i]]):
            assert remainder(z, mod) == remainder(a, mod), f"{tag}: system {i}"
