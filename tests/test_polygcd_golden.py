"""tests/golden/sage_polygcd.npz is the reference's own data: regenerated from its Sage pickles, its live answers and its irreducible
polynomials it must come out array for array as committed (needs the reference checkout; no GPU)."""
import importlib.util
import os

import numpy as np
import pytest

from tests import helpers as H

REF_POLYS = "/root/reference/tests/polys"


@pytest.mark.skipif(not os.path.isdir(REF_POLYS), reason="the reference checkout is not on this machine")
def test_sage_polygcd_fixture_regenerates_identically(tmp_path):
    spec = importlib.util.spec_from_file_location("generate_polygcd_golden", os.path.join(H.GOLDEN, "generate_polygcd_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fresh = np.load(gen.pack(str(tmp_path)))
    committed = np.load(os.path.join(H.GOLDEN, "sage_polygcd.npz"))
    assert sorted(fresh.keys()) == sorted(committed.keys())
    for k in fresh.keys():
        a, b = fresh[k], committed[k]
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), k
    tags = {k.split("/")[1] for k in fresh.keys() if k.startswith("sage/")}
    assert len(tags) == 16
    # per Sage folder: properties, 5 egcd lists with lengths, (arguments with lengths and counts, answers with lengths) of lcm and
    # prod, the square-free polynomials with lengths and flags
    assert len([k for k in fresh.keys() if k.startswith("sage/")]) == 16 * (1 + 10 + 2 * 5 + 3)
    for tag in tags:
        assert len(fresh[f"sage/{tag}/egcd_X_len"]) == len(fresh[f"sage/{tag}/egcd_T_len"]) == 20
        for name in ("lcm", "prod"):
            assert int(fresh[f"sage/{tag}/{name}_X_count"].sum()) == len(fresh[f"sage/{tag}/{name}_X_len"])
            assert len(fresh[f"sage/{tag}/{name}_X_count"]) == len(fresh[f"sage/{tag}/{name}_Z_len"])
        assert len(fresh[f"sage/{tag}/sqfree_Z"]) == len(fresh[f"sage/{tag}/sqfree_X_len"])
    # the nine live fields and the two constructed products, each product with three factors of one degree and a repeated one
    assert len({k.split("/")[1] for k in fresh.keys() if k.startswith("live/")}) == 9
    for tag in ("GF_2e8", "GF_2e32"):
        lens, mult = fresh[f"built/{tag}/factors_len"], fresh[f"built/{tag}/factors_mult"]
        assert max(np.bincount(lens)) >= 3 and mult.max() >= 2
        assert int(((lens - 1) * mult).sum()) == len(fresh[f"built/{tag}/f"]) - 1
