"""The toolbox entry points refuse what they refused, in the words they used: tests/golden/arg_messages.json holds the
exception type and the exact ``str(exc)`` of every case of tests/golden/make_arg_messages_golden.py (which describes
them), recorded from the commit before the argument checks were gathered in ``spatial_alignment_amd/_args.py``.  No
device is needed: every case runs on CPU tensors, and one whose arguments pass every rule ends at the CPU-tensor refusal,
so an acceptance rule that moved shows as well as a message that did."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _recorder():
    spec = importlib.util.spec_from_file_location("make_arg_messages_golden",
                                                  os.path.join(GOLDEN, "make_arg_messages_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


with open(os.path.join(GOLDEN, "arg_messages.json")) as _f:
    WANT = json.load(_f)["messages"]
ENTRIES = sorted({name.split("/")[0] for name in WANT})


@pytest.fixture(scope="module")
def got():
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (torch's note on sparse CSR support)
        return _recorder().record()


def test_the_cases_are_the_recorded_ones(got):
    assert set(got) == set(WANT), sorted(set(got) ^ set(WANT))
    assert len(ENTRIES) >= 30 and len(WANT) >= 600


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_refusal_has_the_recorded_type_and_text(got, entry):
    names = [n for n in WANT if n.split("/")[0] == entry]
    wrong = {n: (got.get(n), WANT[n]) for n in names if got.get(n) != WANT[n]}
    assert not wrong, "\n".join(f"{n}:\n  now      {g}\n  recorded {w}" for n, (g, w) in wrong.items())
