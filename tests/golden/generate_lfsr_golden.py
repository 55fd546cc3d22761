"""
Generates tests/golden/sage_lfsr.npz (run in the build container only):

    python tests/golden/generate_lfsr_golden.py

The Sage `lfsr_sequence(key, fill, 50)` vectors recorded as literals in /root/reference/tests/test_fibonacci_lfsr.py: the eight
test_step_* cases over GF(2), GF(3), GF(2^3) and GF(3^3), each with a primitive and a reducible characteristic polynomial.  The
literal lists are read out of the syntax tree; nothing of the file is executed.  /root/reference/tests/test_galois_lfsr.py
records no Sage vector (its two extension-field cases compare against powers of a primitive element), so a Galois register is
tested on the same eight sequences through the conversion.  Data only.  Per case `name` (the test's name without "test_step_"):

    lfsr/{name}/order      the field's order
    lfsr/{name}/key        Sage's key [a_n, ..., a_1] with signs as recorded: c(x) = x^n - key[n-1] x^(n-1) - ... - key[0]
    lfsr/{name}/fill       the initial fill = the first n outputs = the Fibonacci state reversed
    lfsr/{name}/seq        the 50 outputs
"""
import ast
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = "/root/reference/tests/test_fibonacci_lfsr.py"


def _int(node) -> int:
    """An integer literal, or a power of two of them (2**3)."""
    if isinstance(node, ast.BinOp) and isinstance(node.op, ast.Pow):
        return _int(node.left) ** _int(node.right)
    return int(ast.literal_eval(node))


def _gf_list(node):
    """The list inside GF([...])."""
    assert isinstance(node, ast.Call) and len(node.args) == 1 and isinstance(node.args[0], ast.List), ast.dump(node)
    return [int(v) for v in ast.literal_eval(node.args[0])]


def pack(out_dir: str = HERE) -> str:
    tree = ast.parse(open(SOURCE).read())
    out, names = {}, []
    for fn in tree.body:
        if not (isinstance(fn, ast.FunctionDef) and fn.name.startswith("test_step_") and fn.name.endswith(("_primitive", "_reducible"))):
            continue
        found = {}
        for stmt in fn.body:
            if isinstance(stmt, ast.Assign) and len(stmt.targets) == 1 and isinstance(stmt.targets[0], ast.Name):
                target = stmt.targets[0].id
                if target == "GF" and "GF" not in found:
                    found["GF"] = _int(stmt.value.args[0])
                elif target in ("key", "state", "y_truth") and target not in found and isinstance(stmt.value, ast.Call) and stmt.value.args \
                        and isinstance(stmt.value.args[0], ast.List):
                    found[target] = _gf_list(stmt.value)
        assert set(found) == {"GF", "key", "state", "y_truth"}, (fn.name, sorted(found))
        assert len(found["y_truth"]) == 50 and len(found["key"]) == len(found["state"])
        name = fn.name[len("test_step_"):]
        names.append(name)
        out[f"lfsr/{name}/order"] = np.array(found["GF"], dtype=np.int64)
        out[f"lfsr/{name}/key"] = np.array(found["key"], dtype=np.uint8)
        out[f"lfsr/{name}/fill"] = np.array(found["state"], dtype=np.uint8)
        out[f"lfsr/{name}/seq"] = np.array(found["y_truth"], dtype=np.uint8)
    assert len(names) == 8, names
    out["names"] = np.array(names)
    target = os.path.join(out_dir, "sage_lfsr.npz")
    np.savez_compressed(target, **out)
    return target


if __name__ == "__main__":
    print("packed", pack(os.environ.get("GOLDEN_OUT", HERE)))
