"""CPU-only checks of tests/line_scalar_cases.py, the inputs and mirrors of
tests/test_gpu_line_scalars.py: that the float64 mirror of fill_level + prepare_line is the CPU
oracle's `derived` bit for bit on every (table, level, policy) -- exp and pow included: the mirror
calls the C library the oracle is linked to, so no column needs an allowance --, that the cases
reach every branch they are meant to (counts asserted per case), that the fused and the unfused
centres of family F fall on different sides of an integer, that the slots of family S differ, and
the float64-vs-long-double scan that measures E_cpu in the units of the case file (printed;
line_scalar_cases.E_CPU_GAMMA and E_CPU_STRENGTH record it and the GPU tests take their bound from
it)."""
import numpy as np
import pytest

from tests import line_scalar_cases as lc


def test_mirror_is_the_oracle_bit_for_bit(oracle):
    calls = 0
    for case, level, policy in lc.walk():
        mine = lc.mirror64(case, level, policy)
        theirs = lc.oracle_derived(oracle, case, level, policy)
        assert mine.shape == theirs.shape == (case.table.num_lines, 8)
        different = np.argwhere(mine != theirs)
        assert different.size == 0, "%s, %s, %s: row %d column %d: %r against %r" % (
            case.name, level, policy, different[0][0], different[0][1],
            mine[tuple(different[0])], theirs[tuple(different[0])])
        calls += 1
    assert calls == 5 + 2*6 + 24 + 2 + 4 + 8 + 2


def test_refusals_of_the_mirror():
    s = lc.cases()["S"]
    for level in lc.S_REFUSED:
        with pytest.raises(lc.Refused):
            lc.level_scalars(s.table, level)
    narrow = lc.s_table((300, 400))
    with pytest.raises(lc.Refused):
        lc.level_scalars(narrow, lc.S_NO_REFERENCE_LEVEL)
    for bad in lc.B_IDS:
        case = lc._case("B inside", "B", lc.b_inside(bad), lc.GRID, (lc.B_LEVEL,))
        for policy in ("reference", "skip"):
            with pytest.raises(lc.BadRow) as caught:
                lc.mirror64(case, lc.B_LEVEL, policy)
            assert (caught.value.row, caught.value.local_iso_id) == (lc.B_IN_AT, bad)


def test_slots_of_s_differ():
    case = lc.cases()["S"]
    slots = lc.slots_of(case.table)
    assert sorted(set(slots.tolist())) == list(range(10))
    ids = case.table.local_iso_id
    assert np.all(slots[ids == 0] == 9) and np.all(slots[ids == 10] == 9)
    assert all(np.count_nonzero(ids == k) == 11 for k in lc.S_IDS)
    for level in case.levels:
        lv = lc.level_scalars(case.table, level)
        d = lv.doppler[:10]
        assert np.min(np.abs(d[:, None]/d[None, :] - 1.) + np.eye(10)) > 1.e-3
        q = lv.q_ratio[:10]
        if level[0] == 296.:
            assert np.all(q == 1.)
        else:
            assert np.min(np.abs(q[:, None]/q[None, :] - 1.) + np.eye(10)) > 1.e-3
    # The interval of each level: first knot, on a knot, inside, the last one.
    t = case.table.tips_temperature
    assert [int(np.floor(l[0])) - int(t[0]) for l in case.levels] == [196, 0, 150, 150, 399]
    assert t.size == 401


def test_extremes_are_reached():
    for name, centres in (("E low", 8), ("E high", 4)):
        case = lc.cases()[name]
        table = case.table
        assert table.num_lines == centres*30
        assert np.count_nonzero(table.n_air < 0.) == centres*12
        assert np.count_nonzero(table.gamma_self == 0.) == centres*15
        assert np.count_nonzero(table.elower == 12000.) == centres*10
        zero_width = 0
        for level in case.levels:
            derived, more = lc.mirror64(case, level, "reference", more=True)
            assert np.all(more.accepted) and np.all(derived[:, 3] > 0.)
            assert np.all(np.isfinite(derived))
            if level[2] == 1.:
                assert more.level.p_atm - more.level.p_partial == 0.
                assert np.count_nonzero(derived[:, 2] == 0.) == centres*15
                zero_width += 1
            else:
                assert np.all(derived[:, 2] > 0.)
            # y = sqrt(ln 2) gamma/alpha: the side of voigt.c:48-53 at 0.5 Pa and 25 000 cm-1.
            y = np.sqrt(np.log(2.))*derived[:, 2]/derived[:, 1]
            if name == "E high" and level[1] == 0.5:
                assert np.any(y <= 1.e-6) == (level[2] == 1.) and np.any(y > 1.e-6)
        assert zero_width == 2
    assert lc.cases()["E low"].table.nu.min() == 0.01
    assert lc.cases()["E high"].table.nu.max() > 25000.


def test_window_branches_are_reached():
    total = np.zeros(len(lc.W_BRANCHES), dtype=int)
    for (cut_off, npv, v0), counts in lc.W_COUNTS.items():
        case = lc.cases()["W cut_off %d, %d per cm-1, v0 %d" % (cut_off, npv, v0)]
        assert lc.window_branches(case, lc.W_LEVEL) == counts, case.name
        total += counts
    assert len(lc.W_COUNTS) == 24
    assert total.tolist() == [122, 20, 20, 114, 12, 40, 48, 32]
    # A centre below zero: 0.3 cm-1 shifted to -0.8 cm-1, floor -1, a window that ends at point 0.
    case = lc.cases()["W cut_off 0, 10 per cm-1, v0 0"]
    derived = lc.mirror64(case, lc.W_LEVEL, "reference")
    assert np.any((case.table.nu == 0.3) & (derived[:, 0] < 0.) & (derived[:, 0] > -1.) &
                  (derived[:, 5] == 0.))


def test_fused_and_unfused_centres_of_f_differ():
    for name, differ in lc.F_FUSED_DIFFER.items():
        case = lc.cases()[name]
        derived, more = lc.mirror64(case, lc.F_LEVEL, "reference", more=True)
        centre = derived[:, 0]
        assert np.all(np.abs(more.level.p_atm*case.table.delta_air) <= 0.6)
        integer = np.round(centre)
        below = np.nextafter(integer, 0.)
        assert np.all((centre == integer) | (centre == below))
        assert np.count_nonzero(centre == integer) == 9 and np.count_nonzero(centre == below) == 3
        fused = lc.fused_centre(case.table.nu, case.table.delta_air, more.level.p_atm)
        other_side = np.floor(fused) != np.floor(centre)
        assert np.count_nonzero(other_side) == differ
        assert np.all(centre[other_side] == integer[other_side])
        assert np.all(fused[other_side] == below[other_side])
        # ... and it shows: the window of such a line moves by n_per_v points.
        moved = lc._windows(case, fused)
        assert np.all(moved[0][other_side] != derived[other_side, 4])


def test_rows_counts_and_bad_rows():
    r0, r = lc.cases()["R0"], lc.cases()["R"]
    nu = r0.table.nu
    assert not np.all(np.diff(nu) >= 0.)
    values, counts = np.unique(nu, return_counts=True)
    assert sorted(counts[counts > 1].tolist()) == [3, 4, 5]
    for x in lc.COLUMNS[1:]:
        assert np.unique(getattr(r0.table, x)).size == nu.size
    reference = lc.mirror64(r, lc.R_LEVEL, "reference")
    assert np.all(reference[:lc.R_OUTSIDE_AT, 6] >= 0.)
    assert np.all(reference[lc.R_OUTSIDE_AT:, 6] == -1.)
    assert np.all(reference[lc.R_OUTSIDE_AT:, :6] == 0.)
    skip = lc.mirror64(r, lc.R_LEVEL, "skip")
    assert np.flatnonzero(skip[:, 6] == -1.).tolist() == [lc.R_OUTSIDE_AT]
    assert np.array_equal(np.delete(skip, lc.R_OUTSIDE_AT, axis=0),
                          lc.mirror64(r0, lc.R_LEVEL, "skip"))
    assert [lc.cases()["N %d" % n].table.num_lines for n in lc.N_LINES] == list(lc.N_LINES)
    for n in lc.N_LINES:
        case = lc.cases()["N %d" % n]
        assert lc.evals_of(lc.mirror64(case, lc.N_LEVEL, "reference")) > 0
    b = lc.cases()["B outside"]
    assert b.table.local_iso_id[list(lc.B_OUT_AT)].tolist() == list(lc.B_IDS)
    assert np.all(lc.slots_of(b.table)[list(lc.B_OUT_AT)] == -1)
    skip = lc.mirror64(b, lc.B_LEVEL, "skip")
    assert np.flatnonzero(skip[:, 6] == -1.).tolist() == list(lc.B_OUT_AT)
    reference = lc.mirror64(b, lc.B_LEVEL, "reference")
    assert np.flatnonzero(reference[:, 6] == -1.).tolist() == list(range(lc.B_OUT_AT[0], 30))
    assert lc.empty_table().num_lines == 0


def test_rounding_allowance_of_the_mirror():
    """E_cpu: the worst error of the float64 mirror against the long-double mirror, in the units
    K_g and K_s, over every call of every case."""
    worst = {}
    for case, level, policy in lc.walk():
        derived = lc.mirror64(case, level, policy)
        gamma, strength, k_g, k_s = lc.mirror_long(case, level, policy)
        per = worst.setdefault(case.family, [0., 0.])
        per[0] = max(per[0], float(np.max(lc.error_in_units(derived[:, 2], gamma, k_g),
                                          initial=0.)))
        per[1] = max(per[1], float(np.max(lc.error_in_units(derived[:, 3], strength, k_s),
                                          initial=0.)))
    print("E_cpu per family (gamma, strength):",
          {k: "%.3f, %.3f" % tuple(v) for k, v in worst.items()})
    e_gamma = max(v[0] for v in worst.values())
    e_strength = max(v[1] for v in worst.values())
    assert sorted(worst) == sorted("SEWFRNB")
    assert e_gamma <= lc.E_CPU_GAMMA <= 1.05*e_gamma, e_gamma
    assert e_strength <= lc.E_CPU_STRENGTH <= 1.05*e_strength, e_strength
    # A condition on the units, not the bound: beyond it a unit is wrong for some case.
    assert lc.E_CPU_GAMMA <= lc.E_CAP and lc.E_CPU_STRENGTH <= lc.E_CAP
    # The units matter: without them the raw relative error of the strength is far larger.
    low = lc.cases()["E low"]
    raw = 0.
    for level in low.levels:
        derived = lc.mirror64(low, level, "reference")
        _, strength, _, k_s = lc.mirror_long(low, level, "reference")
        raw = max(raw, float(np.max(lc.error_in_units(derived[:, 3], strength, np.ones_like(k_s)))))
    print("raw relative error of the strength, E low: %.3g u" % raw)
    assert raw > 100.
