"""tests/golden/sage_polyroots.npz is the reference's own data: regenerated from its Sage pickles it must come out array for array as
committed (needs the reference checkout), and every listed root is a root with exactly the listed multiplicity -- checked on Python
integers through the oracle's field arithmetic (oracle/wide_oracle.py restates the reference's formulas for every (p, m), so all 16
folders are covered).  No GPU."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest

from oracle.wide_oracle import WideOracle
from tests import helpers as H

REF_POLYS = "/root/reference/tests/polys"
GOLDEN = os.path.join(H.GOLDEN, "sage_polyroots.npz")
TAGS = sorted(k.split("/")[1] for k in np.load(GOLDEN).keys() if k.endswith("/properties"))


@functools.lru_cache(maxsize=None)
def _golden():
    d = np.load(GOLDEN)
    return {k: d[k] for k in d.keys()}


def _lists(key):
    g = _golden()
    flat, ends = [int(v) for v in g[key]], np.cumsum(g[key + "_len"])
    return [flat[e - n:e] for e, n in zip(ends, g[key + "_len"])]


@pytest.mark.skipif(not os.path.isdir(REF_POLYS), reason="the reference checkout is not on this machine")
def test_sage_polyroots_fixture_regenerates_identically(tmp_path):
    spec = importlib.util.spec_from_file_location("generate_polyroots_golden", os.path.join(H.GOLDEN, "generate_polyroots_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fresh = np.load(gen.pack(str(tmp_path)))
    committed = np.load(GOLDEN)
    assert sorted(fresh.keys()) == sorted(committed.keys())
    for k in fresh.keys():
        a, b = fresh[k], committed[k]
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), k
    assert len(fresh.keys()) == 16 * 6  # properties, X and R with their lengths, M


def test_all_sage_folders_present_with_the_shape_the_device_tests_rely_on():
    assert len(TAGS) == 16
    assert {"GF_2", "GF_2e8", "GF_7e3", "GF_3191", "GF_2147483647", "GF_2e32", "GF_2e100", "GF_109987e4", "GF_36893488147419103183"} <= set(TAGS)
    g = _golden()
    wide = [t for t in TAGS if json.loads(str(g[f"sage/{t}/properties"]))["order"] >= 2**64]
    assert sorted(wide) == ["GF_109987e4", "GF_2e100", "GF_36893488147419103183"] and all(g[f"sage/{t}/X"].dtype.kind == "U" for t in wide)
    most = 0
    for t in TAGS:
        x_len, r_len, m = g[f"sage/{t}/X_len"], g[f"sage/{t}/R_len"], g[f"sage/{t}/M"]
        assert len(x_len) == len(r_len) == 20 and int(r_len.sum()) == len(m) == len(g[f"sage/{t}/R"])
        assert 1 <= x_len.min() and x_len.max() <= 11 and r_len.max() <= 4 and 3 <= int((r_len == 0).sum()) <= 10 and m.min() >= 1
        assert all(int(f[0]) != 0 for f in _lists(f"sage/{t}/X"))  # trimmed; the constants among them are not zero
        most = max(most, int(m.max()))
    assert most == 5


@pytest.mark.parametrize("tag", TAGS)
def test_listed_roots_are_roots_of_exactly_the_listed_multiplicity(tag):
    props = json.loads(str(_golden()[f"sage/{tag}/properties"]))
    p, m = props["characteristic"], props["degree"]
    K = WideOracle(p, m, [int(c) for c in props["irreducible_poly"]] if m > 1 else None)
    X, R = _lists(f"sage/{tag}/X"), _lists(f"sage/{tag}/R")
    M = [int(v) for v in _golden()[f"sage/{tag}/M"]]

    def deflate(f, r):
        """(quotient, remainder) of f by x - r."""
        w = [f[0]]
        for c in f[1:]:
            w.append(K.add(K.mul(w[-1], r), c))
        return w[:-1], w[-1]

    at = 0
    for f, roots in zip(X, R):
        assert roots == sorted(roots) and len(set(roots)) == len(roots) and all(0 <= r < K.q for r in roots)
        degree_in_roots = 0
        for r in roots:
            quo, count = f, 0
            while len(quo) >= 2:
                nxt, rem = deflate(quo, r)
                if rem != 0:
                    break
                quo, count = nxt, count + 1
            assert count == M[at] >= 1, f"{tag}: root {r} of {f}"
            degree_in_roots += count
            at += 1
        assert degree_in_roots <= len(f) - 1
        if K.q <= 343:  # and no other element is a root
            others = [x for x in range(K.q) if x not in roots]
            assert all(deflate(f, x)[1] != 0 for x in others), f"{tag}: {f}"
    assert at == len(M)
