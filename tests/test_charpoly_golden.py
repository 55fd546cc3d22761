"""tests/golden/sage_charpoly.npz is the reference's own data: regenerated from the Sage pickles it must come out array for
array as committed (needs the reference checkout; no GPU)."""
import importlib.util
import os

import numpy as np
import pytest

from tests import helpers as H

REF_DATA = "/root/reference/tests/fields/data"


@pytest.mark.skipif(not os.path.isdir(REF_DATA), reason="the reference checkout is not on this machine")
def test_sage_charpoly_fixture_regenerates_identically(tmp_path):
    spec = importlib.util.spec_from_file_location("generate_charpoly_golden", os.path.join(H.GOLDEN, "generate_charpoly_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fresh = np.load(gen.pack(str(tmp_path)))
    committed = np.load(os.path.join(H.GOLDEN, "sage_charpoly.npz"))
    assert sorted(fresh.keys()) == sorted(committed.keys())
    assert len(fresh.keys()) == 16 * 18  # 16 folders: properties, the count, 5 matrices (X, Z), two element sets (X, Z, lengths)
    for k in fresh.keys():
        a, b = fresh[k], committed[k]
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), k
