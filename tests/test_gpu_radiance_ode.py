"""The view entries run on the flux entries' own output and compared with the transfer equation:
lbl_path_thermal_two_stream, lbl_path_thermal_two_stream_source, lbl_path_two_stream and the two
spectral flux entries write their rows; lbl_path_thermal_radiance, lbl_path_thermal_radiance_source,
lbl_path_thermal_radiance_observer, lbl_path_solar_radiance and the two spectral radiance entries
read **those rows**; and the radiance is held to the long-double solver of
tests/radiance_ode_cases.py, which carries pi*I along the ray as one more state of the two-stream
equations and knows none of the closed forms of the view.  This is the hand-over no other test
covers: which interface row belongs to which level in either storage order, down[0] and direct[0]
as constants, the observer's interface, the guard's moved cosine used by both entries, and the
surface line.

Shapes: sweep_cases.PATHS paths of 1, 2, 9 and 17 levels, both storage orders, 1, 64 and 130
columns, the aligned and the odd layout; two_stream_ode_cases' general, conservative and guard
tables and its two spectral cases; mu = (1, 0.6, 0.05) and phi = (0, 90, 180), one per path; the
observer after n_p in {0, 1, L - 1, L} levels, looking down and up, with both sources.
tests/test_radiance_ode_host.py proves on the CPU what the tables hold.

Bounds, none taken from the code under test.  Every radiance is finite and within
(4*E_view + FLOOR + GAIN*(4*E_flux + FLUX_FLOOR) + c)*scale of the reference: 4*E_view + FLOOR and
4*E_flux + FLUX_FLOOR are what the entries' own tests allow between each kernel and its long-double
mirror, GAIN is what a unit of flux scale in one row moves the view by
(radiance_ode_cases.GAIN, measured on the mirrors), and c is what the long-double mirror chain
differs from the equations by in the class of the column (radiance_ode_cases.CHAIN through
two_stream_ode_cases.column_allowance).  Because c is the mirrors' own distance on the conservative
and guard tables, every radiance is also held to the long-double view mirror fed the rows the GPU
wrote, within the entry's (4*E_view + FLOOR)*scale; those rows are held to the flux reference by
tests/test_gpu_two_stream_ode.py.  No element is left out.

Without any bound: looking down with n_p = L gives the bits of the whole-view entry on the same
rows; looking up with n_p = 0 gives 0; both layouts give the same bits.  A view stopped after n_p
levels and continued from the GPU's result by the long-double mirror through the remaining levels
is the GPU's full view within the entry's bound."""
import numpy as np
import pytest

from tests import radiance_ode_cases as rad
from tests import scatterer_cases as spectral
from tests import scatterer_radiance_cases as spectral_view
from tests import solar_radiance_cases as svc
from tests import sweep_cases as cases
from tests import thermal_cases as tc
from tests import thermal_radiance_cases as rc
from tests import thermal_radiance_observer_cases as oc
from tests import thermal_radiance_source_cases as rsc
from tests import thermal_source_cases as tsc
from tests import two_stream_cases as ts
from tests import two_stream_ode_cases as ode
from tests.test_gpu_scatterer_radiance_shapes import solar as run_spectral_solar_view
from tests.test_gpu_scatterer_radiance_shapes import thermal as run_spectral_thermal_view
from tests.test_gpu_scatterer_shapes import longwave as run_spectral_longwave
from tests.test_gpu_scatterer_shapes import shortwave as run_spectral_shortwave
from tests.test_gpu_solar_radiance_shapes import run as run_solar_view
from tests.test_gpu_sweep_shapes import same_bits
from tests.test_gpu_thermal_radiance_observer_shapes import run as run_observer
from tests.test_gpu_thermal_radiance_shapes import run as run_isothermal_view
from tests.test_gpu_thermal_radiance_source_shapes import run as run_linear_view
from tests.test_gpu_thermal_source_shapes import run as run_thermal
from tests.test_gpu_two_stream_shapes import run as run_solar

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
PATHS = cases.PATHS
MU, PHI = rad.MU, rad.PHI
THERMAL_FLUXES, SOLAR_FLUXES = ("up", "down"), ("up", "direct", "diffuse")


@pytest.fixture(scope="module")
def engine():
    from pylbl_amd.engine import default_engine
    return default_engine(0)


def whole(inputs):
    return [(0, inputs.levels)]


def hold(what, value, reference, mirror, scale, allowed, near):
    """value [PATHS, columns] finite, within near*scale of the long-double view mirror fed the
    GPU's own flux rows and within allowed*scale of the reference (allowed [PATHS, columns])."""
    assert value.shape == reference.shape == mirror.shape
    assert np.all(np.isfinite(value)), what
    worst = []
    for expect, bound in ((mirror, near + LD(0.)*allowed), (reference, allowed)):
        error = np.abs(value.astype(LD) - expect)
        size = bound*scale
        lit = size > 0.
        worst.append(float(np.max(error[lit]/size[lit], initial=0.)))
        assert np.all(error <= size), (what, worst)
    print("%s: worst error / bound %.3g (mirror on the GPU's rows), %.3g (equations)" % (
        (what,) + tuple(worst)))


def allowance(e_view, floor, e_flux, flux_floor, product, recorded_classes, column_class):
    near = LD(4.*e_view + floor)
    return near, near + LD(rad.GAIN[product]*(4.*e_flux + flux_floor)) + \
        ode.column_allowance(rad.CHAIN[product], recorded_classes, column_class)


# ---------------------------------------------------------------------------------------------
# Longwave.
def thermal_table(engine, name, depth, from_last):
    for columns in ode.COLUMNS:
        inputs, reference = rad.thermal_case(name, columns, depth, from_last)
        column_class = ode.thermal_column_class(inputs.layer_inputs(from_last))
        for linear in (False, True):
            product = "linear" if linear else "isothermal"
            expect = reference[linear]
            scale = expect["scale"]
            problem = rad.thermal_problem(inputs, linear)
            e_flux = tsc.E_CPU if linear else tc.E_CPU
            view_near, view_allowed = allowance(
                rsc.E_CPU if linear else rc.E_CPU, rsc.FLOOR if linear else rc.FLOOR, e_flux,
                tc.FLUX_FLOOR, product, ode.THERMAL_CLASSES, column_class)
            near, allowed = allowance(
                oc.E_CPU_LINEAR if linear else oc.E_CPU, oc.FLOOR, e_flux, tc.FLUX_FLOOR, product,
                ode.THERMAL_CLASSES, column_class)
            run_view = run_linear_view if linear else run_isothermal_view
            base = None
            for layout in ode.LAYOUTS:
                what = (inputs.name, from_last, layout, product)
                got = run_thermal(engine, inputs, layout, whole(inputs), from_last,
                                  isothermal=not linear)
                assert np.all(got["top_down"] == 0.), "light from space"
                fluxes = rad.rows(got, THERMAL_FLUXES)
                if base is None:
                    base = fluxes
                    sweeps = rad.thermal_mirror_sweeps(problem, MU, from_last, fluxes)
                for q in THERMAL_FLUXES:
                    assert same_bits(fluxes[q], base[q]), (what, q)
                view = run_view(engine, problem, MU, layout, whole(inputs), from_last,
                                fluxes=fluxes)["radiance"]
                hold(what + ("whole view",), view, expect["down"][0], sweeps[False][0], scale,
                     view_allowed, view_near)
                seen = {}
                for up in (False, True):
                    for n in rad.observers(depth):
                        at = run_observer(engine, problem, MU, layout, whole(inputs), from_last,
                                          rad.passed(n), up, fluxes=fluxes)["radiance"]
                        seen[up, n] = at
                        hold(what + ("up" if up else "down", n), at,
                             rad.at_observer(expect["up" if up else "down"], n, up),
                             rad.at_observer(sweeps[up], n, up), scale, allowed, near)
                assert same_bits(seen[False, depth], view), (what, "n_p = L is the whole view")
                assert np.all(seen[True, 0] == 0.), (what, "looking up from space")
                # Stopped after n levels and continued by the mirror through the rest.
                for up in (False, True):
                    for n in rad.observers(depth)[:-1]:
                        onward = oc.mirror(LD, problem, MU, from_last, rad.passed(depth), up,
                                           fluxes, start=(seen[up, n], rad.passed(n)))["radiance"]
                        error = np.abs(seen[up, depth].astype(LD) - onward)
                        assert np.all(error <= near*scale), (what, "continued", up, n)


@pytest.mark.parametrize("name", sorted(rad.THERMAL_MAKERS))
@pytest.mark.parametrize("depth", ode.DEPTHS)
@pytest.mark.parametrize("from_last", [False, True])
def test_longwave_views_of_the_flux_entries_rows_solve_the_transfer_equation(
        engine, name, depth, from_last):
    thermal_table(engine, name, depth, from_last)


@pytest.mark.parametrize("from_last", [False, True])
def test_spectral_longwave_view_solves_the_transfer_equation(engine, from_last):
    columns, depth = ode.SPECTRAL_SHAPE[:2]
    inputs, reference = rad.thermal_case("spectral", columns, depth, from_last)
    expect = reference[False]
    near, allowed = allowance(
        spectral_view.E_CPU_THERMAL, spectral_view.FLOOR, spectral.E_CPU_LONGWAVE, tc.FLUX_FLOOR,
        "isothermal", ode.THERMAL_CLASSES,
        ode.thermal_column_class(inputs.layer_inputs(from_last)))
    base = None
    for layout in ode.LAYOUTS:
        got = run_spectral_longwave(engine, inputs, layout, whole(inputs), from_last, False)
        fluxes = rad.rows(got, THERMAL_FLUXES)
        if base is None:
            base = fluxes
            mirror = rad.whole_view_mirror(inputs, MU, from_last, False, fluxes)
        for q in THERMAL_FLUXES:
            assert same_bits(fluxes[q], base[q]), (layout, q)
        view = run_spectral_thermal_view(engine, inputs, MU, layout, whole(inputs), from_last,
                                         fluxes=fluxes)["radiance"]
        hold((inputs.name, from_last, layout), view, expect["down"][0], mirror, expect["scale"],
             allowed, near)


# ---------------------------------------------------------------------------------------------
# Shortwave.
def solar_table(engine, name, depth, from_last, columns=ode.COLUMNS):
    for count in columns:
        inputs, cosine, expect = rad.solar_case(name, count, depth, from_last)
        knots = rad.spectral(inputs)
        assert (ode.guarded_elements(inputs, from_last) > 0) == (name == "guard")
        near, allowed = allowance(
            spectral_view.E_CPU_SOLAR if knots else svc.E_CPU,
            spectral_view.FLOOR if knots else svc.FLOOR,
            spectral.E_CPU_SHORTWAVE if knots else ts.E_CPU, ts.FLUX_FLOOR, "solar",
            ode.SOLAR_CLASSES, ode.solar_column_class(inputs.layer_inputs(from_last)))
        chain = rad.solar_view_mirror(inputs, MU, cosine, from_last, rad.rows(
            rad.solar_flux_mirror(inputs, from_last), SOLAR_FLUXES))
        scale = svc.scale(inputs, chain)
        base = None
        for layout in ode.LAYOUTS:
            if knots:
                got = run_spectral_shortwave(engine, inputs, layout, whole(inputs), from_last)
            else:
                got = run_solar(engine, inputs, layout, whole(inputs), from_last)
            fluxes = rad.rows(got, SOLAR_FLUXES)
            if base is None:
                base = fluxes
                mirror = rad.solar_view_mirror(inputs, MU, cosine, from_last, fluxes)["radiance"]
            for q in SOLAR_FLUXES:
                assert same_bits(fluxes[q], base[q]), (layout, q)
            run_view = run_spectral_solar_view if knots else run_solar_view
            view = run_view(engine, inputs, MU, PHI, layout, whole(inputs), from_last,
                            fluxes=fluxes)["radiance"]
            hold((inputs.name, from_last, layout), view, expect["down"][0], mirror, scale, allowed,
                 near)


@pytest.mark.parametrize("name", sorted(rad.SOLAR_MAKERS))
@pytest.mark.parametrize("depth", ode.DEPTHS)
@pytest.mark.parametrize("from_last", [False, True])
def test_shortwave_view_of_the_flux_entry_s_rows_solves_the_transfer_equation(
        engine, name, depth, from_last):
    solar_table(engine, name, depth, from_last)


@pytest.mark.parametrize("from_last", [False, True])
def test_spectral_shortwave_view_solves_the_transfer_equation(engine, from_last):
    columns, depth = ode.SPECTRAL_SHAPE[:2]
    solar_table(engine, "spectral", depth, from_last, (columns,))
