"""The host path of pylbl_amd.distributed.ShardedLines.run on real gloo ranks with a stand-in
`compute` (tests/sharded_lines_recorder.py): which compute calls, zero-fills, flushes, grouped
send/recv operations and reductions every rank makes, in which order and with which shapes and
offsets, and what its Pending and run() report -- compared with tests/golden/sharded_lines_log.json,
which the code wrote before run() was split into stages (tests/golden/make_sharded_lines_log.py).
And, without processes, the properties of the gather's plan (distributed.gather_plan) over the
same grid of cases.  No GPU, no built library."""
import json
import os

import pytest

from pylbl_amd import distributed
from tests import sharded_lines_recorder as recorder

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "sharded_lines_log.json")
CASES = recorder.cases()


@pytest.fixture(scope="module")
def records():
    return recorder.run_cases()


@pytest.fixture(scope="module")
def expected():
    with open(GOLDEN) as source:
        return json.load(source)


def test_the_cases_are_those_of_the_file(records, expected):
    assert list(records) == list(expected)
    for name in records:
        assert list(records[name]) == list(expected[name]), name


@pytest.mark.parametrize("name", [recorder.case_id(case) for case in CASES])
def test_same_host_path_as_before(records, expected, name):
    for rank, want in expected[name].items():
        got = records[name][rank]
        for index, (mine, theirs) in enumerate(zip(got, want)):
            assert mine == theirs, \
                f"{name}, {rank}: entry {index} differs:\n  now    {mine}\n  before {theirs}"
        assert len(got) == len(want), \
            f"{name}, {rank}: {len(got)} entries, {len(want)} before; the first one more or " \
            f"missing: {(got + want)[min(len(got), len(want))]}"


def test_every_receiver_got_the_values_the_stand_in_computes(records):
    """Stated outright, so that a regenerated file cannot hide it: only a rank that receives
    nothing reports values that are not the expected ones."""
    results = [entry for record in records.values() for log in record.values() for entry in log
               if entry.startswith("result(")]
    assert len(results) == sum(2*len(record) for record in records.values())
    for entry in results:
        received = "x" in entry         # a shape: "5x16"
        assert entry.endswith("correct={})".format(received)), entry


# ---------------------------------------------------------------------------------------------
# The plan of the grouped gather, without torch.
def plans(case, to_self):
    """{rank: transfers} of every rank of the case's group, and the receivers."""
    world = case.world if case.members is None else len(case.members)
    plan = distributed.partition(case.levels, recorder.WEIGHTS[case.molecules], world)
    receivers = range(world) if case.dst is None else (case.dst,)
    return plan, receivers, {
        rank: distributed.gather_plan(plan, case.output, rank, receivers, to_self)
        for rank in range(world)}


def what(transfers, kind, peer=None):
    """(key, levels) of the transfers of one kind (with one peer), in issue order."""
    return [(t.key, t.levels) for t in transfers
            if t.kind == kind and (peer is None or t.peer == peer)]


@pytest.mark.parametrize("case", CASES, ids=recorder.case_id)
def test_gather_plan(case):
    plan, receivers, by_rank = plans(case, False)
    _, _, by_rank_to_self = plans(case, True)
    # ("total" in unit mode: several ranks hold rows of one level, which is why run() sums over
    # the ranks there instead of gathering; such a plan pairs up but cannot tile.)
    tiles = not (case.output == "total" and plan.mode == "units")
    keys = [None] if case.output == "total" else list(range(len(case.molecules)))
    for rank, transfers in by_rank.items():
        for transfer in transfers + by_rank_to_self[rank]:
            assert transfer.kind in ("copy", "send", "recv")
            assert len(transfer.levels) > 0
            assert transfer.levels == list(range(transfer.levels[0], transfer.levels[-1] + 1))
        # what arrives tiles the collected array exactly once; nothing arrives elsewhere
        for arriving in (what(transfers, "copy") + what(transfers, "recv"),
                         what(by_rank_to_self[rank], "recv")):
            cells = [(key, level) for key, levels in arriving for level in levels]
            if rank not in receivers:
                assert not cells
            elif tiles:
                assert sorted(cells, key=lambda cell: (keys.index(cell[0]), cell[1])) == \
                    [(key, level) for key in keys for level in range(case.levels)]
        # a rank's own blocks: copied; with the switch on, each a send directly before its recv
        assert all(t.kind == "copy" for t in transfers if t.peer == rank)
        own = [t for t in by_rank_to_self[rank] if t.peer == rank]
        assert not what(by_rank_to_self[rank], "copy")
        assert [t.kind for t in own] == ["send", "recv"]*len(what(transfers, "copy"))
        assert what(own, "send") == what(own, "recv") == what(transfers, "copy")
        assert [t for t in by_rank_to_self[rank] if t.peer != rank] == \
            [t for t in transfers if t.peer != rank]
    # every send has its recv on the peer, at the same position among the transfers of the pair
    for ranks in (by_rank, by_rank_to_self):
        for rank, transfers in ranks.items():
            for peer in ranks:
                assert what(transfers, "send", peer) == what(ranks[peer], "recv", rank), \
                    (rank, peer)


def test_gather_plan_cases_reach_both_modes_and_empty_ranks():
    modes, empty, idle_receiver = set(), 0, 0
    for case in CASES:
        plan, receivers, by_rank = plans(case, False)
        modes.add((plan.mode, case.output))
        empty += sum(1 for rank in by_rank if not plan.units[rank])
        idle_receiver += sum(1 for rank in receivers if not plan.units[rank])
    assert modes == {(mode, output) for mode in ("levels", "units") for output in ("gas", "total")}
    assert empty > 0 and idle_receiver > 0
