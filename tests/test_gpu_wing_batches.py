"""The far-wing loop of the four-points-per-lane kernel merges up to eight batches of eight lines
before one reciprocal; how many (K) is chosen per level from bounds on the terms' range
(pylbl_amd/csrc/line_prep.h: wing_line_bounds, wing_batches).  The choice is checked on the host
through lbl_wing_batches; the spectra of cases built to land on each K -- including both sides of
a guard boundary -- are checked against the CPU oracle on the GPU."""
import math

import numpy as np
import pytest

from pylbl_amd import synthetic
from tests import golden_io
from tests.test_gpu_parity import assert_spectrum

FILL = 0x7f7f7f7f


def wing_batches(bounds):
    from ctypes import c_int32
    from pylbl_amd import engine
    lib = engine.library()
    array = (c_int32*4)(*bounds)
    return int(lib.lbl_wing_batches(array))


def bounds_of(t_lo, t_hi, b_lo, b_hi):
    """The four reduced bounds as the kernel keeps them (maxima negated)."""
    return (t_lo, -t_hi, b_lo, -b_hi)


def test_wing_batches_choice():
    # The default workload: t in [2^-6, 2^10), bl in [2^-120, 2^-60): all eight batches.
    assert wing_batches(bounds_of(-6, 10, -120, -60)) == 8
    # Upper range: 64 t_hi + 6 <= 1000 decides between 8 and 4 ...
    assert wing_batches(bounds_of(0, 15, -100, -60)) == 8
    assert wing_batches(bounds_of(0, 16, -100, -60)) == 4
    # ... and a large amplitude counts on top of it.
    assert wing_batches(bounds_of(0, 15, -10, 40)) == 4
    # Lower range: n t_lo + b_lo >= -1000 (n = 8K lines).
    assert wing_batches(bounds_of(-14, 10, -100, -60)) == 8       # -896 - 100
    assert wing_batches(bounds_of(-15, 10, -100, -60)) == 4       # -960 - 100 < -1000
    assert wing_batches(bounds_of(-28, 10, -100, -60)) == 4       # 32 lines: -896 - 100
    assert wing_batches(bounds_of(-29, 10, -100, -60)) == 2       # 32 lines: -928 - 100
    assert wing_batches(bounds_of(-60, 10, -30, -20)) == 2       # 16 lines: -960 - 30
    assert wing_batches(bounds_of(-70, 10, -30, -20)) == 1
    # No far-wing line at all, and all amplitudes zero.
    assert wing_batches((FILL, FILL, FILL, FILL)) == 1
    assert wing_batches((-6, -10, FILL, FILL)) == 8
    # Values outside every finite range (what a zero, infinite or NaN term reduces to).
    assert wing_batches(bounds_of(-4096, 10, -100, -60)) == 1
    assert wing_batches(bounds_of(-6, 4096, -100, -60)) == 1
    assert wing_batches(bounds_of(-6, 10, -4096, -60)) == 1


def ilogb(x):
    return np.frexp(x)[1] - 1


def expected_batches(oracle, table, t, p, x, v0, vn, npv, cut):
    """K as the kernel chooses it, from the oracle's per-line scalars (line_prep.h)."""
    _, extras = oracle.absorption_port(table, t, p, x, v0, vn, npv, cut_off=cut,
                                       want_derived=True)
    d = extras["derived"]
    centre, alpha, gamma, strength, first, last, status = (d[:, i] for i in range(7))
    live = (status == 1) & (last >= first)
    alpha, gamma, strength = alpha[live], gamma[live], strength[live]
    repwid = math.sqrt(math.log(2.))/alpha
    y = repwid*gamma
    xlim0 = np.where(y < 70.55, np.sqrt(np.maximum(15100. + y*(40. - y*3.6), 0.)), 0.)
    reach = np.where(xlim0 > 0., (xlim0/repwid)*(1. - 1.e-6), 0.)
    g2 = gamma*gamma
    t_lo = int(np.min(ilogb(reach*reach + g2)))
    t_hi = int(np.max(ilogb((cut + 1.)**2 + g2))) + 1
    bl = np.abs(strength*gamma/math.pi)
    bl = bl[bl > 0.]
    b_lo, b_hi = int(np.min(ilogb(bl))), int(np.max(ilogb(bl))) + 1
    return wing_batches(bounds_of(t_lo, t_hi, b_lo, b_hi))


# (label, formula, v0, vn, npv, cut, T, p [Pa], vmr, lines, K the case is built for)
CASES = [
    ("tropospheric CO2", "CO2", 600, 640, 100, 25, 288.99, 98388., 3.6e-4, 4000, 8),
    # Narrow lines at low pressure near 1 cm-1: tiny Doppler and Lorentz widths make t small.
    ("narrow lines near 1 cm-1", "H2O", 1, 3, 1000, 1, 200., 0.01, 1.e-5, 600, 2),
    # The same gas a cm-1 higher: the smallest t grows past the K = 2 / K = 4 guard.
    ("narrow lines near 2 cm-1", "H2O", 2, 4, 1000, 1, 200., 0.01, 1.e-5, 600, 2),
    ("narrow lines near 3 cm-1", "H2O", 3, 5, 1000, 1, 200., 0.01, 1.e-5, 600, 4),
    # A wide cut-off lowers K through t_max = (cut_off + 1)^2 + g2; 180 and 181 sit either side
    # of 64 log2(t_max) = 1000.
    ("cut-off 180", "CO2", 700, 706, 100, 180, 250., 50000., 4.e-4, 2500, 8),
    ("cut-off 181", "CO2", 700, 706, 100, 181, 250., 50000., 4.e-4, 2500, 4),
    ("cut-off 600", "O3", 1000, 1003, 100, 600, 250., 20000., 1.e-6, 1500, 4),
]


def case_table(label, formula, v0, vn, cut, lines):
    """Synthetic lines over the case's reach; strengths spread evenly over 11 decades
    (1e-30 ... 1e-19) in a shuffled order, so that every batch mixes them."""
    table = synthetic.line_table(formula, max(v0 - cut - 1., 0.05), vn + cut + 1.,
                                 num_lines=lines, seed=sum(map(ord, label)))
    rng = np.random.default_rng(len(label))
    table.sw = rng.permutation(10.**np.linspace(-30., -19., table.nu.size))
    return table


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_cases_reach_their_batches(oracle, case):
    label, formula, v0, vn, npv, cut, t, p, x, lines, want = case
    table = case_table(label, formula, v0, vn, cut, lines)
    assert expected_batches(oracle, table, t, p, x, v0, vn, npv, cut) == want


@pytest.fixture(scope="module")
def engine():
    from pylbl_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("prep", [0, 1], ids=["device_prep", "host_prep"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_wing_batches_against_oracle(engine, oracle, case, prep):
    label, formula, v0, vn, npv, cut, t, p, x, lines, _ = case
    table = case_table(label, formula, v0, vn, cut, lines)
    engine.set_option("points_per_lane", 4)
    engine.set_option("prep", prep)
    molecule = engine.load(table)
    try:
        got = engine.compute(molecule, np.array([t]), np.array([p]), np.array([x]), v0, vn, npv,
                             cut_off=cut)
        k_ref, _ = oracle.absorption_port(table, t, p, x, v0, vn, npv, cut_off=cut)
        spec = golden_io.Case("wing", 0, 0, 0, 0, v0, vn, npv, cut, False, None, 0)
        assert_spectrum(got[0], k_ref, spec, f"{label} prep={prep}")
    finally:
        engine.free(molecule)
        engine.set_option("points_per_lane", 0)
        engine.set_option("prep", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_kernel_uses_the_expected_batches(engine, case):
    """Which K the device chose, read from the results: capping K (engine option "wing_batches")
    at or above the level's K leaves every bit of the spectrum as it is, capping it well below
    changes the rounding.  (Dense tiles are split into work items of a bounded number of lines, so
    a wavefront of these small cases may hold only a few batches: K = 8 and K = 4 then group them
    alike, and the test caps at a quarter of K where K >= 4.)"""
    label, formula, v0, vn, npv, cut, t, p, x, lines, want = case
    table = case_table(label, formula, v0, vn, cut, lines)
    engine.set_option("points_per_lane", 4)
    molecule = engine.load(table)
    try:
        def spectrum(cap):
            engine.set_option("wing_batches", cap)
            return engine.compute(molecule, np.array([t]), np.array([p]), np.array([x]), v0, vn,
                                  npv, cut_off=cut)[0].copy()
        chosen = spectrum(8)
        assert np.array_equal(spectrum(want), chosen)
        if want > 1:
            assert not np.array_equal(spectrum(max(want//4, 1)), chosen)
    finally:
        engine.free(molecule)
        engine.set_option("wing_batches", 8)
        engine.set_option("points_per_lane", 0)
