"""The toolbox kernels that share csrc/toolbox.hpp (csrc/ot.hip, gpr.hip, register.hip, neighbors.hip) write the bytes they
wrote before the header existed: tests/golden/toolbox_fold_bits.json was recorded from the commit it names, the inputs
are rebuilt from their seeds by the recorder's own code (tests/golden/make_toolbox_fold_golden.py, which describes the
cases), every entry runs twice, the two runs must give equal bytes and every output's sha256 must be the recorded one.
The bar is equality: these kernels sum in a fixed order, and code that only moved into a header must not move a bit."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _recorder():
    spec = importlib.util.spec_from_file_location("make_toolbox_fold_golden",
                                                  os.path.join(GOLDEN, "make_toolbox_fold_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_output_has_the_recorded_bytes():
    from spatial_alignment_amd import ops

    rec = _recorder()
    with open(rec.PATH) as f:
        want = json.load(f)["digests"]
    seen, wrong, unstable = set(), [], []
    for case, thunk in rec.entries(ops.get_ops(), "cuda:0"):
        first, second = thunk(), thunk()
        for name, t in first.items():
            key = f"{case}/{name}"
            seen.add(key)
            d = rec.digest(t)
            if d != rec.digest(second[name]):
                unstable.append(key)
            if d != want.get(key):
                wrong.append(key)
    assert not unstable, f"two runs give different bytes (case/output): {unstable}"
    assert not wrong, f"{len(wrong)} of {len(seen)} outputs differ from the recorded bytes (case/output): {wrong}"
    assert seen == set(want), sorted(set(want) ^ seen)
