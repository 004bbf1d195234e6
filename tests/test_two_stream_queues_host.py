"""The host side of the two-stream products and of compute_solar (pylbl_amd/two_stream.py and the
sweeps of pylbl_amd/spectroscopy.py) on a recording stand-in for the engine
(tests/two_stream_queue_cases.py): which engine calls every case makes, in which order, with which
blocks and arguments, and the shapes of what it returns -- compared with
tests/golden/two_stream_queues.json, which the code wrote before its host side was moved
(tests/golden/make_two_stream_queues.py).  No GPU, no built library."""
import json
import os

import pytest

from tests import two_stream_queue_cases as cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "two_stream_queues.json")
NAMES = [case[0] for case in cases.cases()]


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    return cases.run_cases(tmp_path_factory.mktemp("two_stream_queues"))


@pytest.fixture(scope="module")
def expected():
    with open(GOLDEN) as source:
        return json.load(source)


def test_the_cases_are_those_of_the_file(records, expected):
    assert list(records) == list(expected) == NAMES and len(set(NAMES)) == len(NAMES)
    methods = {case[1] for case in cases.cases()}
    assert methods == {"compute_solar_flux", "compute_solar_flux_spectral", "compute_thermal_flux",
                       "compute_thermal_flux_linear", "compute_thermal_flux_spectral",
                       "compute_thermal_radiance", "compute_solar"}
    refused = [name for name in NAMES if isinstance(expected[name]["result"], str)]
    assert len(refused) == 3


@pytest.mark.parametrize("name", NAMES)
def test_same_engine_calls_as_before(records, expected, name):
    got, want = records[name], expected[name]
    for index, (mine, theirs) in enumerate(zip(got["log"], want["log"])):
        assert mine == theirs, f"{name}: call {index} differs:\n  now    {mine}\n  before {theirs}"
    assert len(got["log"]) == len(want["log"]), \
        f"{name}: {len(got['log'])} calls, {len(want['log'])} before; the first one more or " \
        f"missing: {(got['log'] + want['log'])[min(len(got['log']), len(want['log']))]}"
    assert got["result"] == want["result"], name
