"""The loss stack's calls into the library WITHOUT a GPU: every scenario of tests/golden/make_loss_call_log.py replayed over the
stand-in library must make the calls tests/golden/loss_call_log.json holds -- the same entry points in the same order with the
same settings, coefficients and accumulate flags.  The file was written by the loss code as it stood before the node classes
were merged into one protocol; it changes only when the calls are meant to."""
import importlib.util
import json
import os

import pytest

import fake_lib

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_loss_call_log", os.path.join(HERE, "golden", "make_loss_call_log.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

fake_pkg = fake_lib.fake_pkg_fixture(*gen.SOURCES)

with open(gen.OUT) as _fh:
    GOLDEN = json.load(_fh)


def test_the_file_holds_exactly_the_scenarios():
    assert list(GOLDEN) == [s.__name__ for s in gen.SCENARIOS]


@pytest.mark.parametrize("scenario", gen.SCENARIOS, ids=lambda s: s.__name__)
def test_calls_are_those_of_the_recorded_log(fake_pkg, scenario):
    got = gen.run(scenario)
    want = GOLDEN[scenario.__name__]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "call %d differs" % i
    assert len(got) == len(want), [c[0] for c in got]
