"""The host side of Spectroscopy.compute_absorption (pylbl_amd/absorption.py) on a recording
stand-in for the engine (tests/absorption_recorder.py): which engine calls it makes, in which order
and with which arguments, for every output format, order switch and mix of mechanisms -- compared
with tests/golden/absorption_queue_log.json, which the code wrote before its host side was moved
(tests/golden/make_absorption_queue_log.py).  The queue orders were measured into place
(profiles/r03_ab_api.txt and the comments of absorption.py); three of their rules are also stated
here outright, so that a regenerated file cannot hide a change.  No GPU, no built library."""
import json
import os
import re

import pytest

from tests import absorption_recorder as recorder

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "absorption_queue_log.json")
CASES = recorder.cases()
KERNELS = recorder.KERNEL_CALLS


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    return recorder.run_cases(tmp_path_factory.mktemp("absorption_queue"))


@pytest.fixture(scope="module")
def expected():
    with open(GOLDEN) as source:
        return json.load(source)


def test_the_cases_are_those_of_the_file(records, expected):
    assert list(records) == list(expected)


@pytest.mark.parametrize("name", sorted(
    {recorder.case_id(case) for case in CASES} |
    {"uploads of {}, {} levels".format(case.gas_set, case.levels) for case in CASES}))
def test_same_engine_calls_as_before(records, expected, name):
    got, want = records[name], expected[name]
    for index, (mine, theirs) in enumerate(zip(got["log"], want["log"])):
        assert mine == theirs, f"{name}: call {index} differs:\n  now    {mine}\n  before {theirs}"
    assert len(got["log"]) == len(want["log"]), \
        f"{name}: {len(got['log'])} calls, {len(want['log'])} before; the first one more or " \
        f"missing: {(got['log'] + want['log'])[min(len(got['log']), len(want['log']))]}"
    assert got.get("result") == want.get("result"), name
    assert got.get("error") == want.get("error"), name


# ---------------------------------------------------------------------------------------------
# The rules.
def method(entry):
    return entry.split("(", 1)[0]


def argument(entry, name):
    return re.search(r"[(\s]{}=([^,)]*)".format(name), entry).group(1)


def where(log, *methods):
    return [i for i, entry in enumerate(log) if method(entry) in methods]


def line_counts(records, case):
    """{molecule handle: number of lines} from what building the case's back ends uploaded."""
    uploads = records["uploads of {}, {} levels".format(case.gas_set, case.levels)]["log"]
    return {argument(entry, "handle"): int(argument(entry, "num_lines"))
            for entry in uploads if method(entry) == "load"}


def total_cases(order):
    for case in CASES:
        settings = dict(recorder.DEFAULTS, **dict(case.settings))
        if case.call == "absorption" and case.mode == "total" and case.fail_at is None and \
                settings["total_order"] == order and settings["device_output_limit"] > 0 and \
                case.gas_set != "unknown alias":
            yield case


def test_total_heavy_last_slots_then_lines_lightest_first(records):
    """Every continuum before every cross-section before every lines call; the lines in ascending
    num_lines; only the last lines call delivers."""
    checked = 0
    for case in total_cases("heavy_last"):
        log = records[recorder.case_id(case)]["log"]
        continua = where(log, "continuum_compute", "continuum_compute_many")
        cross, lines = where(log, "xsec_compute"), where(log, "compute")
        ordered = continua + cross + lines
        assert ordered == sorted(ordered), recorder.case_id(case)
        counts = line_counts(records, case)
        sizes = [counts[argument(log[i], "molecule")] for i in lines]
        assert sizes == sorted(sizes), recorder.case_id(case)
        delivering = [i for i in lines if argument(log[i], "deliver") != "None"]
        assert delivering == lines[-1:], recorder.case_id(case)
        assert not where(log, "deferred", "finish_deferred"), recorder.case_id(case)
        checked += len(lines) > 1
    assert checked >= 6


def test_total_deferred_heaviest_first_and_finished_last(records):
    """The heaviest gas's lines call is the first lines call and is the one kept back;
    finish_deferred follows the last other call.  Where the engine could not keep it back, the
    copy of the block follows the last call instead."""
    checked = 0
    for case in total_cases("deferred"):
        log = records[recorder.case_id(case)]["log"]
        lines = where(log, "compute")
        if not lines:
            assert not where(log, "deferred", "finish_deferred"), recorder.case_id(case)
            continue
        counts = line_counts(records, case)
        sizes = [counts[argument(log[i], "molecule")] for i in lines]
        assert sizes[0] == max(sizes), recorder.case_id(case)
        assert [argument(log[i], "defer_finish") for i in lines] == \
            ["True"] + ["False"]*(len(lines) - 1), recorder.case_id(case)
        assert [argument(log[i], "deliver") != "None" for i in lines] == \
            [True] + [False]*(len(lines) - 1), recorder.case_id(case)
        assert where(log, "deferred") == [lines[0] + 1], recorder.case_id(case)
        last = where(log, *KERNELS)[-1]
        if case.deferred_answer:
            assert where(log, "finish_deferred") == [last + 1], recorder.case_id(case)
            assert not where(log, "to_host_into"), recorder.case_id(case)
        else:
            assert not where(log, "finish_deferred"), recorder.case_id(case)
            assert where(log, "to_host_into") == [last + 1], recorder.case_id(case)
        checked += 1
    assert checked >= 6


def test_failure_cancels_and_waits_before_any_block_goes_back(records):
    """The third kernel call raises: cancel_deferred, then synchronize (which raises again), are
    logged before any block is given back to the pool, and the error raised is the first one.
    compute_absorption gives no block back after a failure; a path product gives back all."""
    failing = [case for case in CASES if case.fail_at is not None]
    assert {case.call for case in failing} == {"absorption", "path"}
    for case in failing:
        record = records[recorder.case_id(case)]
        assert record["error"][0] == "StandInFailure", recorder.case_id(case)
        log = record["log"]
        failed = where(log, *KERNELS)[case.fail_at - 1]
        assert [method(entry) for entry in log[failed + 1:failed + 3]] == \
            ["cancel_deferred", "synchronize"], recorder.case_id(case)
        assert not where(log[:failed + 3], "blocks.give"), recorder.case_id(case)
        given = where(log, "blocks.give")
        if case.call == "path":
            assert len(given) == len(where(log, "blocks.take")) > 0
        else:
            assert not given, recorder.case_id(case)
        assert method(log[-1]) == "pipeline.exit"
    kept_back = [case for case in failing if dict(case.settings).get("total_order") == "deferred"]
    log = records[recorder.case_id(kept_back[0])]["log"]
    assert "deferred(answer=True)" in log and not where(log, "finish_deferred")
