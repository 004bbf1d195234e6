"""The pedestal pre-pass (csrc/pedestal.h) with more runs on a level than one launch row takes and
at its fall-back cuts.  pedestal_finish launches run_sums_kernel and run_links_kernel on
dim3(min(max_runs, 65535), levels): past 65 535 runs their grid-stride loops make a second and a
third trip and run_solve_kernel runs more than 1 024 chunks of 64 runs per level.  The cases are
tests/pedestal_run_cases.py's (A wide; B dense, and cut to exactly 65 535 and 65 536 runs; E dense
through 302 bins to the window at cut_off 150, with the same two cuts; C1 and C1' with `too_long`
true at cut_off 25, F at cut_off 200, F40 with exactly 40 too_long runs; C2 with the stretch cut true; D cut by kRunCut inside one
window, at cut_off 25 and 40); tests/test_pedestal_run_cases_host.py proves on the CPU, through a
mirror of the run bookkeeping, that each is what it is taken for here, that the runs of the later
trips are visible a thousand times above the bar, and that none needs the conditioning allowance.

Every call takes three levels (10 Pa, 16 073 Pa, 101 325 Pa): three run counts under one max_runs
stride.  Which path a level took is not reported by the engine; the observable is bit equality
among the variants {relax default, relax 2, relax 7, serial}:
  * A verified fixed point does not depend on the number of sweeps.
  * Sweeps that verified once stay verified with more of them.
  * run_chain<USE_LDS, WINDOW> is one body for the chain inside run_solve_kernel (slots in HBM
    behind a ring; it starts from zero and reads `runs` and `slot_sums` alone) and for the `serial`
    variant (slots in LDS): the same additions in the same order, the same bits, whatever the
    sweeps left behind.
  * The relaxation forms a pedestal as ks - (sum of earlier pedestals), the chain from running
    differences on the slots: other roundings.  On a level with thousands of runs a spectrum that
    differs from `serial`'s in some bit is the relaxation's.
Every (case, level) is pinned to one of three pictures (Case.bits):
  "fixed"  relax default == relax 7 != serial: the relaxation verified its fixed point within the
           default sweeps, and what run_links_kernel wrote for every run -- gs, ge, begin, the
           masks -- and every history walk of run_solve_kernel went into the compared spectrum.
           The 1-atm levels of A (1 033 chunks), E (1 036 chunks, history walks of ~14 200 runs
           through 56 LDS tiles), E cut to 65 535 and 65 536 runs, D; the 16 073 Pa levels of B, E,
           F, D40 (histories of 4 500 to 6 000 runs).
  "late"   relax 7 != serial == relax default == relax 2: five sweeps leave the level unverified,
           six verify it (C1' at 16 073 Pa, 28 354 runs).
  "same"   all four equal.  Every level the mirror hands to the serial chain must show this; so do
           the 10 Pa levels (a run to the window: the pedestal comes from the fresh last slot with
           the chain's own arithmetic) and levels whose sweeps do not settle: the 1-atm levels of B
           and its cuts, where the runs of one bin span nine chunks -- more chunk boundaries than
           seven sweeps cover.  There the pre-pass is compared through the chain's result alone.
The pins are what the engine gave when the cases were written; that a "fixed" level must differ
from `serial` rests on roundings, not on a proof -- a change of either form's arithmetic that
makes them agree moves a pin, not a bound; so does a "same" on a level that settles (with
opens_run's `r % kRunCut == 0` taken out, C2's 10 Pa level regroups its rows and differs from
`serial` in the last bits; D, the case built on that cut, keeps every pin).

With run_links_kernel's later trips taken out, A, E and E cut to 65 536 runs -- one run in the
second trip -- fail and E cut to 65 535 passes; B and its cuts pass, their 1-atm levels being the
chain's, which reads none of run_links_kernel's records.  C1's third trip of run_links_kernel
is reached and, for the same reason, not checked; run_sums_kernel's third trip is (the chain
reads its sums).

`too_long` itself is checked by F40: F cut to 16 385 + 40 runs at 1 atm, so that exactly the last
40 runs look back over more than kMaxHistory runs.  A too_long run skips its walk (gs = ge = 0);
what keeps the sweeps' result from being accepted is the level's hand-over to the chain, `if
(displaced || too_long)`.  With that reduced to `if (displaced)` the level verifies under the
default and under seven sweeps -- the wrong runs lie in the last chunk or two -- on a fixed point
whose last runs lack the whole plain sum on their first slot: 1 300 x the bound, where the
unmutated library shows "same" at 1.5e-8.  C1, C1' and F reach the cut and do not check it: their
too_long runs are consecutive over dozens of chunks (F: 5 243 runs, 82 chunks), each depends on
the wrong ones before it, a chain that costs a sweep per chunk boundary, so under the same
mutation their sweeps do not settle and the chain takes the level all the same.

Not reached from inputs, and left alone: the mid-batch settle_pairs trigger of run_sums_kernel
(n_pairs > kCorePairs - 64 needs three whole-wavenumber slots inside a line's core range per row;
no physical Doppler width gives that), and run_find_kernel's look-back beyond 64 unresolved
descriptors (dispatch timing)."""
import numpy as np
import pytest

from tests import golden_io
from tests import pedestal_run_cases as cases
from tests.test_gpu_parity import REL, assert_spectrum
from tests.test_gpu_pedestal_workspace import VARIANTS, _options

pytestmark = pytest.mark.gpu

LEVELS = range(cases.LEVEL_P.size)


@pytest.fixture(scope="module")
def engine():
    from pylbl_amd.engine import Engine
    e = Engine(0)
    yield e
    _options(e, 1, 0, 0)
    e.close()


def _call(engine, handle, name, **kw):
    v0, vn, npv, cut = cases.case(name).grid
    # (the host array is recycled by the next call: keep a copy)
    return np.array(engine.compute(handle, cases.LEVEL_T, cases.LEVEL_P, cases.LEVEL_X, v0, vn, npv,
                                   cut_off=cut, **kw))


def _meets_the_oracle(oracle, name, k, plain, label):
    grid = cases.case(name).grid
    case = golden_io.Case("many runs", 0, 0, 0, 0, grid.v0, grid.vn, grid.n_per_v, grid.cut_off,
                          True, None, 0)
    assert np.isfinite(k).all(), label
    for level in LEVELS:
        k_ref = cases.reference(oracle, name, level)
        worst = float(np.max(np.abs(k[level] - k_ref) /
                             cases.plain_tolerance(k_ref, plain[level], grid, REL)))
        print(f"{label} level {level}: {worst:.3g} x the pedestal tolerance")
        assert_spectrum(k[level], k_ref, case, f"{label} level {level}", plain[level])


def test_small_then_large_then_small(engine, oracle):
    """D (a few hundred runs) first, then A on the same workspace -- more chunks than any earlier
    call of this engine, so progress, links and the rest are reserved afresh between run_find's
    launch and the others --, then D again on the large workspace: all meet the oracle."""
    small, large = "D25", "A"
    handles = {name: engine.load(cases.case(name).table) for name in (small, large)}
    try:
        _options(engine, 1, 0, 0)
        plain = {name: _call(engine, handles[name], name) for name in (small, large)}
        _options(engine, 1, 0, 1)
        first = {}
        for turn, name in enumerate((small, large, small, large)):
            k = _call(engine, handles[name], name, remove_pedestal=True)
            _meets_the_oracle(oracle, name, k, plain[name], f"{name} turn {turn}")
            assert np.array_equal(k, first.setdefault(name, k)), (name, turn)
    finally:
        _options(engine, 1, 0, 0)
        for handle in handles.values():
            engine.free(handle)


@pytest.mark.parametrize("name", cases.NAMES)
def test_many_runs(engine, oracle, name):
    """Every variant of {relax default, relax 2, relax 7, serial} on a poisoned workspace: each
    level meets the oracle at the pedestal bar with no conditioning and holds no NaN; relaxation
    and serial chain agree within 1e-7 of the plain spectrum; a second call reproduces the first
    bit for bit; and every level shows the picture of bits it is pinned to (the head of the file)."""
    case = cases.case(name)
    handle = engine.load(case.table)
    try:
        _options(engine, 1, 0, 0)
        plain = _call(engine, handle, name)
        results = {}
        for label, (scan, launches) in VARIANTS.items():
            _options(engine, scan, launches, 1)
            results[label] = _call(engine, handle, name, remove_pedestal=True)
            again = _call(engine, handle, name, remove_pedestal=True)
            _meets_the_oracle(oracle, name, results[label], plain, f"{name} {label}")
            assert np.array_equal(again, results[label]), (name, label, "second call")
        scale = np.maximum(plain, 1e-300)
        for label in VARIANTS:
            apart = np.max(np.abs(results[label] - results["serial"])/scale, axis=1)
            print(f"{name} {label} against serial, by level:", " ".join(f"{x:.3g}" for x in apart))
            assert np.max(apart) < 1.e-7, (name, label)
        for level in LEVELS:
            default, two, seven, serial = (results[label][level] for label in
                                           ("relax default", "relax 2", "relax 7", "serial"))
            picture = case.bits[level]
            where = (name, level, picture)
            assert picture == "same" or not case.fall_back[level], where
            if picture == "fixed":
                assert np.array_equal(default, seven), where
                assert not np.array_equal(seven, serial), where
                assert np.array_equal(two, seven) or np.array_equal(two, serial), where
            elif picture == "late":
                assert not np.array_equal(seven, serial), where
                assert np.array_equal(default, serial) and np.array_equal(two, serial), where
            else:
                for other in (default, two, seven):
                    assert np.array_equal(other, serial), where
    finally:
        _options(engine, 1, 0, 0)
        engine.free(handle)
