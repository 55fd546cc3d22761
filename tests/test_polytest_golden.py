"""tests/golden/reference_polytest.npz is the reference's own data: regenerated from its tables, its Sage pickles and its live
answers it must come out array for array as committed (needs the reference checkout; no GPU)."""
import importlib.util
import os

import numpy as np
import pytest

from tests import helpers as H

REF_POLYS = "/root/reference/tests/polys"


@pytest.mark.skipif(not os.path.isdir(REF_POLYS), reason="the reference checkout is not on this machine")
def test_reference_polytest_fixture_regenerates_identically(tmp_path):
    spec = importlib.util.spec_from_file_location("generate_polytest_golden", os.path.join(H.GOLDEN, "generate_polytest_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fresh = np.load(gen.pack(str(tmp_path)))
    committed = np.load(os.path.join(H.GOLDEN, "reference_polytest.npz"))
    assert sorted(fresh.keys()) == sorted(committed.keys())
    # the pairs and 2 x 26 tables; 11 Sage folders of properties and four lists with lengths; 7 + 5 + 1 + 4 live answers
    assert len(fresh.keys()) == 1 + 2 * 26 + 11 * 9 + 17
    for k in fresh.keys():
        a, b = fresh[k], committed[k]
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), k
