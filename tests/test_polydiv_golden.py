"""tests/golden/sage_polydiv.npz is the reference's own data: regenerated from its Sage pickles and its live answers it must come
out array for array as committed (needs the reference checkout; no GPU)."""
import importlib.util
import os

import numpy as np
import pytest

from tests import helpers as H

REF_POLYS = "/root/reference/tests/polys"


@pytest.mark.skipif(not os.path.isdir(REF_POLYS), reason="the reference checkout is not on this machine")
def test_sage_polydiv_fixture_regenerates_identically(tmp_path):
    spec = importlib.util.spec_from_file_location("generate_polydiv_golden", os.path.join(H.GOLDEN, "generate_polydiv_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fresh = np.load(gen.pack(str(tmp_path)))
    committed = np.load(os.path.join(H.GOLDEN, "sage_polydiv.npz"))
    assert sorted(fresh.keys()) == sorted(committed.keys())
    # 16 Sage folders: properties, 4 + 3 + 2 lists with lengths, 2 exponent lists; the exponents and 3 fields x (2 field parameters, f, g, 3 answers)
    assert len(fresh.keys()) == 16 * (1 + 2 * 9 + 2) + 1 + 3 * 7
    for k in fresh.keys():
        a, b = fresh[k], committed[k]
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), k
    for tag in {k.split("/")[1] for k in fresh.keys() if k.startswith("sage/")}:
        assert len(fresh[f"sage/{tag}/divmod_X_len"]) == 23 and len(fresh[f"sage/{tag}/modpow_E"]) == 20
        assert len(fresh[f"sage/{tag}/power_X_len"]) == 5 and len(fresh[f"sage/{tag}/power_Y"]) == 4 and len(fresh[f"sage/{tag}/power_Z_len"]) == 20
        assert max(int(n) for key in fresh.keys() if key.startswith(f"sage/{tag}/divmod") and key.endswith("_len") for n in fresh[key]) <= 11
