"""lbl_path_two_stream, lbl_path_thermal_two_stream, lbl_path_thermal_two_stream_source and the two
spectral entries fed directly (rows held in torch tensors) and compared with the two-stream
*equations*, not with the mirrors of their closed forms: the reference is the long-double solver
of tests/two_stream_ode_cases.py, which builds every layer from the power series of the equations'
propagator by doubling and solves every column as one linear system in its interface fluxes.

Shapes: sweep_cases.PATHS paths of 1, 2, 9 and 17 levels (one level, the smallest with an interior
interface, just past one and two groups of eight rows in flight), both storage orders, 1, 64 and
130 columns (a lone lane, a full wavefront, two wavefronts and a partial one), an aligned and an
odd layout.  Values, per shape: a random table across the general branch (tau_c from 1e-3 to 50,
omega_c from 0.05 to 1 - 1e-6, g_c up to 0.9, a level of tau = 0, a clear level, an opaque lid,
mu0 = (1, 1e-3, 0.25)); a conservative table (omega = 1 exactly and 1 - 1e-11); for the shortwave
entry a table around the resonance guard; and one spectral case per entry with three knots.
tests/test_two_stream_ode_host.py proves on the CPU that the tables hold these and that none but
the guard's has an element in the guard: nothing is masked out here.

Bounds, none taken from the code under test.  Every flux is within
(4*E_cpu + 1e-13 + c)*scale of the reference, scale = F0 or pi*max B as in the entry's own tests:
4*E_cpu + 1e-13 is what those tests allow between the kernel and the long-double mirror, and c is
what tests/test_two_stream_ode_host.py measures between that mirror and the reference over these
very tables, recorded in two_stream_ode_cases.SOLAR_TABLES, THERMAL_TABLES and SOURCE_TABLES by the
class of the column: rounding (3e-15 and less) where every level is general, clear or exactly
conservative, 2e-9 where a level takes the conservative cut with k2 > 0, 1.3e-5 where one lies in
the resonance guard.  Which class a column counts under follows from the float64 layer inputs and
the branch criteria as the mirror states them (two_stream_ode_cases.solar_column_class): that
choice only widens the bound where the definition documents a cut, and no figure comes from the
kernels.  Because c is the mirror's own distance from the equations on the conservative and guard
tables, every flux is held to the long-double mirror as well, within (4*E_cpu + 1e-13)*scale as in
the entries' own tests, so that no kernel error can hide in c.  Nothing is NaN or inf.  Under
A = 1 the exactly conservative columns keep a net flux of 0 within the same bound."""
import numpy as np
import pytest

from tests import scatterer_cases as spectral
from tests import sweep_cases as cases
from tests import thermal_cases as tc
from tests import thermal_source_cases as tsc
from tests import two_stream_cases as ts
from tests import two_stream_ode_cases as ode
from tests.test_gpu_scatterer_shapes import longwave as run_spectral_longwave
from tests.test_gpu_scatterer_shapes import shortwave as run_spectral_shortwave
from tests.test_gpu_thermal_source_shapes import run as run_thermal
from tests.test_gpu_two_stream_shapes import run as run_solar

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
PATHS = cases.PATHS
SOLAR_NAMES = tuple(prefix + q for prefix in ("", "top_") for q in ts.QUANTITIES)
THERMAL_NAMES = tc.NAMES


@pytest.fixture(scope="module")
def engine():
    from pylbl_amd.engine import default_engine
    return default_engine(0)


def whole(inputs):
    return [(0, inputs.levels)]


def close(what, names, got, reference, scale, allowed, mirror=None, e_cpu=None):
    """Every flux finite and within allowed*scale of the reference (scale and allowed [PATHS,
    columns]: a path's levels share them), and within (4*e_cpu + 1e-13)*scale of the long-double
    mirror; the worst error over bound."""
    n = got[names[0]].shape[0]//PATHS
    worst = 0.
    if mirror is not None:
        near = close(what + ("mirror",), names, got, mirror, scale,
                     LD(4.*e_cpu + ts.FLUX_FLOOR) + LD(0.)*allowed)
        assert near <= 1.
    for name in names:
        value = got[name]
        assert np.all(np.isfinite(value)), (what, name)
        size = allowed*scale
        if not name.startswith("top_"):
            size = np.repeat(size, n, axis=0)
        error = np.abs(value.astype(LD) - reference[name])
        lit = size > 0.
        worst = max(worst, float(np.max(error[lit]/size[lit], initial=0.)))
        assert np.all(error <= size), (what, name, worst)
    print("%s: worst error / bound %.3g" % (what, worst))
    return worst


def solar_allowed(inputs, from_last, e_cpu=ts.E_CPU):
    column_class = ode.solar_column_class(inputs.layer_inputs(from_last))
    return LD(4.*e_cpu + ts.FLUX_FLOOR) + ode.column_allowance(ode.SOLAR_TABLES, ode.SOLAR_CLASSES,
                                                              column_class)


def thermal_allowed(inputs, from_last, linear, e_cpu=None):
    if e_cpu is None:
        e_cpu = tsc.E_CPU if linear else tc.E_CPU
    column_class = ode.thermal_column_class(inputs.layer_inputs(from_last))
    recorded = ode.SOURCE_TABLES if linear else ode.THERMAL_TABLES
    return LD(4.*e_cpu + tc.FLUX_FLOOR) + ode.column_allowance(recorded, ode.THERMAL_CLASSES,
                                                              column_class)


def solar_table(engine, make, depth, from_last, guard=False):
    """One table at every column count on both layouts; [(inputs, got of the aligned layout)]."""
    out = []
    for columns in ode.COLUMNS:
        inputs = make(columns, depth)
        assert (ode.guarded_elements(inputs, from_last) > 0) == guard
        reference = ode.solar_reference(inputs, from_last)
        mirror = ts.mirror(LD, inputs, from_last)
        allowed = solar_allowed(inputs, from_last)
        for layout in ode.LAYOUTS:
            got = run_solar(engine, inputs, layout, whole(inputs), from_last)
            close((inputs.name, from_last, layout), SOLAR_NAMES, got, reference,
                  reference["f0"].astype(LD), allowed, mirror, ts.E_CPU)
            if layout == ode.LAYOUTS[0]:
                out.append((inputs, got))
    return out


@pytest.mark.parametrize("depth", ode.DEPTHS)
@pytest.mark.parametrize("from_last", [False, True])
def test_shortwave_general_tables_solve_the_equations(engine, depth, from_last):
    solar_table(engine, ode.solar_general, depth, from_last)


@pytest.mark.parametrize("depth", ode.DEPTHS)
@pytest.mark.parametrize("from_last", [False, True])
def test_shortwave_conservative_tables_solve_the_equations_and_keep_the_net_flux(
        engine, depth, from_last):
    for inputs, got in solar_table(engine, ode.solar_conservative, depth, from_last):
        # Path 0 has A = 1 under mu0 = 1: where omega is 1 exactly nothing is absorbed anywhere.
        assert inputs.albedo[0] == 1. and np.any(inputs.exact)
        f0 = inputs.f0()[0, inputs.exact].astype(LD)
        allowed = solar_allowed(inputs, from_last)[0, inputs.exact]
        net = np.concatenate([
            got["top_up"][:1].astype(LD) - got["top_down"][:1].astype(LD),
            got["up"][:depth].astype(LD) - got["down"][:depth].astype(LD)])[:, inputs.exact]
        worst = float(np.max(np.abs(net)/(allowed*f0)))
        print("%s, %s: worst net flux / bound %.3g" % (inputs.name, from_last, worst))
        assert np.all(np.abs(net) <= allowed*f0), (inputs.name, worst)


@pytest.mark.parametrize("depth", ode.DEPTHS)
@pytest.mark.parametrize("from_last", [False, True])
def test_shortwave_guard_tables_stay_within_the_guard_s_recorded_error(engine, depth, from_last):
    solar_table(engine, ode.solar_guard, depth, from_last, guard=True)


@pytest.mark.parametrize("make", [ode.thermal_general, ode.thermal_conservative])
@pytest.mark.parametrize("depth", ode.DEPTHS)
@pytest.mark.parametrize("from_last", [False, True])
def test_longwave_tables_solve_the_equations_with_both_sources(engine, make, depth, from_last):
    for columns in ode.COLUMNS:
        inputs = make(columns, depth)
        layers = ode.thermal_layer(inputs.layer_inputs(from_last))
        for linear in (False, True):
            reference = ode.thermal_reference(inputs, from_last, linear, layers)
            mirror = tsc.mirror(LD, inputs, from_last) if linear else \
                tc.mirror(LD, inputs.isothermal(), from_last)
            allowed = thermal_allowed(inputs, from_last, linear)
            for layout in ode.LAYOUTS:
                got = run_thermal(engine, inputs, layout, whole(inputs), from_last,
                                  isothermal=not linear)
                close((inputs.name, from_last, layout, "linear" if linear else "isothermal"),
                      THERMAL_NAMES, got, reference, reference["scale"], allowed, mirror,
                      tsc.E_CPU if linear else tc.E_CPU)
                assert np.all(got["top_down"] == 0.), "light from space"


@pytest.mark.parametrize("from_last", [False, True])
def test_spectral_shortwave_solves_the_equations(engine, from_last):
    inputs = ode.spectral_shortwave()
    assert inputs.knots.size >= 3 and ode.guarded_elements(inputs, from_last) == 0
    reference = ode.solar_reference(inputs, from_last)
    mirror = spectral.shortwave_mirror(LD, inputs, from_last)
    allowed = solar_allowed(inputs, from_last, spectral.E_CPU_SHORTWAVE)
    for layout in ode.LAYOUTS:
        got = run_spectral_shortwave(engine, inputs, layout, whole(inputs), from_last)
        close((inputs.name, from_last, layout), SOLAR_NAMES, got, reference,
              reference["f0"].astype(LD), allowed, mirror, spectral.E_CPU_SHORTWAVE)


@pytest.mark.parametrize("from_last", [False, True])
def test_spectral_longwave_solves_the_equations_with_both_sources(engine, from_last):
    inputs = ode.spectral_longwave()
    assert inputs.knots.size >= 3
    layers = ode.thermal_layer(inputs.layer_inputs(from_last))
    for linear in (False, True):
        reference = ode.thermal_reference(inputs, from_last, linear, layers)
        mirror = spectral.longwave_mirror(LD, inputs, from_last, linear)
        allowed = thermal_allowed(inputs, from_last, linear, spectral.E_CPU_LONGWAVE)
        for layout in ode.LAYOUTS:
            got = run_spectral_longwave(engine, inputs, layout, whole(inputs), from_last, linear)
            close((inputs.name, from_last, layout, "linear" if linear else "isothermal"),
                  THERMAL_NAMES, got, reference, reference["scale"], allowed, mirror,
                  spectral.E_CPU_LONGWAVE)
