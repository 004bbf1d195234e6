"""CPU-only checks of Spectroscopy.compute_thermal_radiance_at: the float64-vs-long-double scan of
the numpy mirror of tests/thermal_radiance_observer_cases.py over its case tables, observers and
directions that measures E_cpu (printed; the cases module records it and the GPU tests take their
bound from it), the looking-up level against Gauss-Legendre quadrature of the transfer integral
of the down-travelling ray, the mirror's properties (its anchors in the existing mirrors, the
composition of two views, the opaque lid), the statements of the definition, the header of the
entry (include/lbl_amd_thermal_radiance_observer.h) against its ctypes signature, the argument
checks (all raised before anything touches the GPU) and what one call queues on a stand-in
engine."""
import ctypes
import inspect
from pathlib import Path
import re

import numpy as np
import pytest

from pylbl_amd import Spectroscopy, two_stream
from pylbl_amd import engine as engine_module
from tests import abi_header, sweep_cases as cases
from tests import surface_cases as surface
from tests import thermal_cases as tc
from tests import thermal_radiance_cases as rc
from tests import thermal_radiance_observer_cases as oc
from tests import thermal_radiance_source_cases as src
from tests.test_linear_source_host import make_spectroscopy
from tests.test_thermal_radiance_host import BAD as VIEW_BAD
from tests.test_thermal_radiance_host import argument, gauss_panels, untouchable
from tests.test_thermal_radiance_source_host import declarations
from tests.test_thermal_source_host import INTERFACES, changed

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "lbl_amd_thermal_radiance_observer.h").read_text()
KERNELS = (ROOT / "pylbl_amd" / "csrc" / "thermal_radiance_observer.h").read_text()
DESIGN = (ROOT / "DESIGN.md").read_text()
F64, LD = np.float64, np.longdouble
ONES = np.ones((3, 5))


# ---------------------------------------------------------------------------------------------
# E_cpu, and what the tables hold.
@pytest.mark.parametrize("source", ["isothermal", "linear"])
def test_float64_mirror_stays_close_to_long_double(source):
    """E_cpu: the worst |float64 - long double|/scale over every case table, observer and
    direction, printed per direction."""
    worst = {False: 0., True: 0.}
    fluxes, count = {}, 0
    for inputs, mu, from_last, passed, up in oc.views(source):
        assert oc.linear(inputs) == (source == "linear")
        key = (id(inputs), from_last)
        if key not in fluxes:
            fluxes[key] = oc.flux_rows(inputs, from_last)
        error, finite = oc.worst_error(inputs, mu, from_last, passed, up, fluxes[key])
        assert finite, (inputs.name, from_last, passed, up)
        if error > worst[up]:
            print("%-20s D=%.2f from_last=%-5s n_p=%s up=%s worst |difference|/scale %.3g" % (
                inputs.name, inputs.diffusivity, from_last, passed.tolist(), up, error))
            worst[up] = error
        count += 1
    print("E_cpu (%s) = %.3g looking down, %.3g looking up, %d views" % (
        source, worst[False], worst[True], count))
    measured = max(worst.values())
    recorded = oc.E_CPU_LINEAR if source == "linear" else oc.E_CPU
    assert measured <= recorded
    assert recorded <= 2.*measured, "the cases module no longer records the value"
    # The isothermal tables stay below the project's cap; the linear ones hold
    # thermal_radiance_source_cases' mirror as the observer n_p = L looking down, which has none.
    assert oc.E_CPU <= oc.E_CPU_CAP == 1e-10
    assert oc.E_CPU_LINEAR >= src.E_CPU and oc.FLOOR == 1e-13 == rc.FLOOR


def test_case_tables_and_observers_are_those_of_the_definition():
    for source, module in (("isothermal", rc), ("linear", src)):
        tables = oc.all_cases(source)
        assert [inputs.name for inputs, _, _ in tables] == \
            [inputs.name for inputs, _, _ in module.all_cases()]
        names = {inputs.name for inputs, _, _ in tables}
        assert {"pole", "deep", "cloud at first", "cloud at last", "cloud at every"} <= names
        assert {inputs.levels_per_path for inputs, _, _ in tables} >= set(tc.DEPTHS)
        for name in ("cloud at every", "pole", "deep"):
            assert {f for inputs, _, f in tables if inputs.name == name} == {False, True}
    assert oc.interfaces(1) == [0, 1] and oc.interfaces(2) == [0, 1, 2]
    assert oc.interfaces(3) == [0, 1, 2, 3]
    assert oc.interfaces(8) == [0, 1, 4, 7, 8] and oc.interfaces(9) == [0, 1, 4, 8, 9]
    assert oc.interfaces(17) == [0, 1, 8, 16, 17]
    for depth in tc.DEPTHS:
        calls = oc.observers(depth)
        assert sorted({int(n) for passed in calls for n in passed}) == oc.interfaces(depth)
        assert len(set(calls[-1].tolist())) == min(3, depth + 1)
        assert all(passed.dtype == np.int32 and passed.shape == (3,) for passed in calls)
    assert "kThermalObserverAhead = %d;" % oc.VIEW_AHEAD in KERNELS
    assert "path_levels<kThermalObserverAhead, kVector>" in KERNELS
    a = oc.VIEW_AHEAD
    assert {1, a, a + 1, 2*a, 2*a + 1} <= set(tc.DEPTHS)


# ---------------------------------------------------------------------------------------------
# The level by independent means.
def downward_quadrature(t, mu, a, f_up, f_down):
    """int_0^t [f+(tau)(1 - a) + f-(tau)(1 + a)] exp(-(t - tau)/mu) dtau/mu in long double: what a
    ray travelling towards the surface along -mu gathers of the two-stream field between the
    level's space-side face (tau = 0) and its surface-side face (tau = t)."""
    tau, weight = gauss_panels(t)
    one = LD(1.)
    integrand = (f_up(tau)*(one - a) + f_down(tau)*(one + a))*np.exp(-(t - tau)/mu)/mu
    return np.sum(integrand*weight)


def test_exchanged_closed_forms_match_quadrature_of_the_downward_ray():
    """C of both cloudy branches with F_with and F_against in the places of up[i+1] and down[i]
    against Gauss-Legendre quadrature of the downward ray's integral over the level's own f+-
    in their P, Q (general) and N (conservative) forms, in long double, relative to |u1| + |d0|;
    and the same with the linear source's shift, whose sign follows the exchanged faces: the
    physical f+ carries +c_phys and f- carries -c_phys with c_phys = pi*(B_surface -
    B_space)/(su*t), and the exchanged call is handed c = -c_phys."""
    rng = np.random.default_rng(21)
    two = LD(2.)
    worst = shifted = 0.
    general = [(1.25, 0.8, 3.), (1.25, 0.8*(1. + 1e-9), 3.), (1.25, 0.8*(1. - 1e-9), 3.),
               (50., 1., 20.), (2., 0.5, 1e-3), (1.9, 1., 40.)]
    general += [(rng.uniform(0.05, 2.), rng.uniform(0.05, 1.), 10.**rng.uniform(-3., 1.5))
                for _ in range(40)]
    for k, mu, t in general:
        k, mu, t = LD(k), LD(mu), LD(t)
        gamma, a = LD(rng.uniform(0., 0.99)), LD(rng.uniform(0., 0.7))
        u1, d0, c = (LD(rng.uniform(-1., 1.)) for _ in range(3))
        em = -np.expm1(-t/mu)
        # The level's own solution: f+ at tau = t is u1, f- at tau = 0 is d0.
        _, p, q, _ = rc.general_c(LD, k, gamma, t, mu, a, u1, d0)
        f_up = lambda tau: p*np.exp(-k*(t - tau)) + gamma*q*np.exp(-k*tau)      # noqa: E731
        f_down = lambda tau: gamma*p*np.exp(-k*(t - tau)) + q*np.exp(-k*tau)    # noqa: E731
        closed, _, _, _ = rc.general_c(LD, k, gamma, t, mu, a, d0, u1)
        expect = downward_quadrature(t, mu, a, f_up, f_down)
        assert np.isfinite(closed)
        worst = max(worst, float(abs(closed - expect)/(abs(u1) + abs(d0))))
        # With the physical shift c: the exchanged call carries -c.
        closed = closed + (two*(a*(-c)))*em
        expect = downward_quadrature(t, mu, a, lambda tau: f_up(tau) + c,
                                     lambda tau: f_down(tau) - c)
        shifted = max(shifted, float(abs(closed - expect)/(abs(u1) + abs(d0) + abs(c))))
    for _ in range(40):
        g1, mu, t = LD(rng.uniform(0.2, 2.)), LD(rng.uniform(0.05, 1.)), LD(10.**rng.uniform(-4., 2.))
        a, u1, d0, c = (LD(rng.uniform(-1., 1.)) for _ in range(4))
        a = abs(a)*LD(0.7)
        em = -np.expm1(-t/mu)
        _, n = rc.conservative_c(LD, g1, t, mu, a, u1, d0)
        f_up = lambda tau: u1 - g1*n*(t - tau)                                  # noqa: E731
        f_down = lambda tau: d0 + g1*n*tau                                      # noqa: E731
        closed, _ = rc.conservative_c(LD, g1, t, mu, a, d0, u1)
        expect = downward_quadrature(t, mu, a, f_up, f_down)
        worst = max(worst, float(abs(closed - expect)/(abs(u1) + abs(d0))))
        closed = closed + (two*(a*(-c)))*em
        expect = downward_quadrature(t, mu, a, lambda tau: f_up(tau) + c,
                                     lambda tau: f_down(tau) - c)
        shifted = max(shifted, float(abs(closed - expect)/(abs(u1) + abs(d0) + abs(c))))
    print("worst |C exchanged - quadrature|/(|u1| + |d0|) = %.3g; with the shift, over (|u1| + "
          "|d0| + |c|), %.3g" % (worst, shifted))
    assert worst <= oc.QUADRATURE_BOUND and shifted <= oc.QUADRATURE_BOUND


def test_the_shift_of_the_exchanged_level_is_the_definitions():
    """thermal_radiance_source_cases.level, handed B_E = B_space as bb and B_X = B_surface as bt,
    forms c = (pi*(B_space - B_surface))/(su*t) and u1 = (down[i] - pi*B_space) - c, d0 =
    (up[i+1] - pi*B_surface) + c: the lines of the definition, checked on the shift alone."""
    inputs = src.with_view(tc.cloud("every"), 60)
    li = inputs.layer_inputs(False)
    here = {name: (value[2] if isinstance(value, np.ndarray) and value.ndim == 3 else value)
            for name, value in li.items()}
    order = inputs.order(False)
    b_space = src.face_planck(LD, inputs, order[:, 2], 0)
    b_surface = src.face_planck(LD, inputs, order[:, 2], 1)
    g1, g2, _, _ = rc.scalars(LD, here)
    shift, db = src.source_shift(LD, here, b_surface, b_space)       # (bt, bb) = (B_X, B_E)
    pi = LD(cases.FLUX_PI)
    with np.errstate(all="ignore"):
        expect = (pi*(b_space - b_surface))/((g1 + g2)*here["t"].astype(LD))
    cloudy = here["branch"] != tc.CLEAR
    assert np.any(cloudy) and np.array_equal(shift[cloudy], expect[cloudy])
    assert np.array_equal(db, b_space - b_surface)
    # It is the physical shift of that level, negated.
    physical, _ = src.source_shift(LD, here, b_space, b_surface)
    assert np.array_equal(shift[cloudy], -physical[cloudy]) and np.any(shift[cloudy] != 0.)


# ---------------------------------------------------------------------------------------------
# Properties in the mirror.
@pytest.mark.parametrize("source", ["isothermal", "linear"])
def test_the_whole_view_down_is_the_existing_mirror_and_no_level_is_the_start(source):
    module = src if source == "linear" else rc
    for inputs, mu, from_last in oc.all_cases(source)[::3]:
        depth = inputs.levels_per_path
        fluxes = oc.flux_rows(inputs, from_last)
        for kind in (F64, LD):
            whole = oc.mirror(kind, inputs, mu, from_last, np.full(3, depth), False, fluxes)
            expect = module.mirror(kind, inputs, mu, from_last, fluxes)
            for q in ("radiance", "brightness_temperature", "scale"):
                assert np.array_equal(whole[q], expect[q], equal_nan=True), (inputs.name, q)
            none = oc.mirror(kind, inputs, mu, from_last, np.zeros(3, dtype=int), False, fluxes)
            assert np.array_equal(none["radiance"],
                                  oc.surface_line(kind, inputs, from_last, fluxes))
            none = oc.mirror(kind, inputs, mu, from_last, np.zeros(3, dtype=int), True, fluxes)
            assert np.all(none["radiance"] == 0.)
            assert np.all(none["brightness_temperature"] == 0.)


@pytest.mark.parametrize("source", ["isothermal", "linear"])
def test_a_view_stopped_and_continued_is_the_full_view(source):
    """The radiance at interface j, handed on as the start of the levels behind it, gives the
    whole view exactly: the sweep keeps nothing but I between levels (and, with the linear
    source, a Planck value that is a function of the interface alone)."""
    for inputs, mu, from_last in oc.all_cases(source)[1::4]:
        depth = inputs.levels_per_path
        fluxes = oc.flux_rows(inputs, from_last)
        for up in (False, True):
            whole = oc.mirror(F64, inputs, mu, from_last, np.full(3, depth), up, fluxes)
            for passed in oc.observers(depth):
                first = oc.mirror(F64, inputs, mu, from_last, passed, up, fluxes)
                rest = oc.mirror(F64, inputs, mu, from_last, np.full(3, depth), up, fluxes,
                                 start=(first["radiance"], passed))
                assert np.array_equal(rest["radiance"], whole["radiance"], equal_nan=True)


def lid_problem(linear):
    """thermal_cases' shape problem of 3 levels with thermal_cases' opaque lid -- a grey absorber
    of tau_c = 3000 without scattering -- as the middle level of every path."""
    inputs = tc.shape_inputs(67, 3, 15)
    middle = np.arange(inputs.levels) % 3 == 1
    inputs.table[middle, 1:4] = (3000., 0., 0.)
    return src.with_view(inputs, 16) if linear else inputs


def test_looking_up_from_under_an_opaque_lid_gives_the_lids_planck_value():
    """Directly under the lid, looking up: exp(-3000/mu) underflows, so the isothermal level gives
    B(T_lid) whatever lies above it, to LID_BOUND of scale (measured 0: the line is 0*I + B*1).
    With the linear source the level radiates at the temperature of the face the ray leaves
    through, less dB*mu/3000 (linear_weight = 1 - A/x with A = 1 and x = 3000/mu)."""
    mu = np.array(oc.MU)
    for from_last in (False, True):
        inputs = lid_problem(False)
        order = inputs.order(from_last)
        got = oc.mirror(F64, inputs, mu, from_last, np.full(3, 2), True)
        lid = cases.planck(F64, inputs.nu[None, :], inputs.table[order[:, 1], 4][:, None])
        size = got["scale"].astype(F64)
        lit = size > 0.
        worst = float(np.max(np.abs(got["radiance"] - lid)[lit]/size[lit]))
        print("from_last=%s worst |I - B(T_lid)|/scale = %.3g" % (from_last, worst))
        assert worst <= oc.LID_BOUND
        assert np.all(lid[:, inputs.nu > 0.] > 0.)
        inputs = lid_problem(True)
        got = oc.mirror(LD, inputs, mu, from_last, np.full(3, 2), True)
        space = 1 if from_last else 0
        leave = src.face_planck(LD, inputs, order[:, 1], 1 - space)
        enter = src.face_planck(LD, inputs, order[:, 1], space)
        slack = np.abs(leave - enter)*(mu[:, None]/LD(3000.))*(LD(1.) + LD(1e-12))
        assert np.all(np.abs(got["radiance"] - leave) <= slack)
        assert np.any(np.abs(got["radiance"] - leave) > 0.25*slack)


def test_the_pitfall_problem_reads_a_real_down_row():
    """The named GPU case: its view down from between the two levels differs at order 1 from what
    a sweep with down = 0 above the cloud would give."""
    inputs = oc.pitfall()
    assert inputs.levels_per_path == 2
    fluxes = oc.flux_rows(inputs, False)
    passed = np.full(3, 1)
    good = oc.mirror(LD, inputs, oc.MU, False, passed, False, fluxes)
    wrong = dict(fluxes, down=fluxes["down"].copy())
    wrong["down"][inputs.order(False)[:, 0]] = 0.
    # The surface line reads down[L], the row of the last level: only the row above the cloud
    # is taken away.
    bad = oc.mirror(LD, inputs, oc.MU, False, passed, False, wrong)
    difference = np.abs(good["radiance"] - bad["radiance"])/good["scale"]
    assert float(difference.max()) > 1e-2


# ---------------------------------------------------------------------------------------------
# The statements of the definition.
def test_header_docstring_design_and_kernel_state_the_same_formulas():
    def squeeze(text):
        return re.sub(r"\s+", " ", re.sub(r"\n\s*(\*|//)", "\n", text))
    section = DESIGN[DESIGN.index("## 32."):]
    for text in (HEADER, KERNELS, Spectroscopy.compute_thermal_radiance_at.__doc__, section):
        text = squeeze(text)
        for formula in oc.FORMULAS[2:]:
            assert formula in text, formula
    for text in (HEADER, KERNELS, section):
        for formula in oc.FORMULAS[:2]:
            assert formula in squeeze(text), formula
    new = inspect.signature(Spectroscopy.compute_thermal_radiance_at).parameters
    old = inspect.signature(Spectroscopy.compute_thermal_radiance).parameters
    added = ["observer_interface", "looking", "interface_temperature"]
    assert list(new)[:6] == ["self", "layer_thickness", "surface_temperature"] + added
    assert new["observer_interface"].default is None and new["looking"].default == "down"
    assert new["interface_temperature"].default is None
    # Every other argument is compute_thermal_radiance's, in its order and with its defaults.
    assert [name for name in new if name not in added] == list(old)
    for name, parameter in old.items():
        assert new[name].default == parameter.default and new[name].kind == parameter.kind, name
    assert not set(added) & set(old)
    # The existing kernels are as they were: the new header only includes them.
    assert '#include "thermal_radiance.h"' in KERNELS
    assert '#include "thermal_radiance_source.h"' in KERNELS
    for name in ("thermal_radiance.h", "thermal_radiance_source.h"):
        assert "observer" not in (ROOT / "pylbl_amd" / "csrc" / name).read_text()
    assert "thermal_observer" in (ROOT / "scripts" / "checks" / "kernel_registers.sh").read_text()


# ---------------------------------------------------------------------------------------------
# The C ABI: include/lbl_amd_thermal_radiance_observer.h against
# abi.THERMAL_RADIANCE_OBSERVER_PROTOTYPES, whole.
def test_header_declares_the_entry_and_ctypes_match():
    from pylbl_amd import abi
    declared = declarations(HEADER)
    name = "lbl_path_thermal_radiance_observer"
    assert list(declared) == list(abi.THERMAL_RADIANCE_OBSERVER_PROTOTYPES) == [name]
    # lbl_path_thermal_radiance_source's arguments with the observer behind view_cosine.
    source = declarations((ROOT / "include" / "lbl_amd_thermal_radiance_source.h").read_text())
    source = source["lbl_path_thermal_radiance_source"]
    at = source.index("const double *view_cosine") + 1
    assert declared[name] == source[:at] + ["const int32_t *observer_levels",
                                            "int32_t view_up"] + source[at:]
    import __graft_entry__
    __graft_entry__.build()
    lib = abi.library()
    argtypes = abi.THERMAL_RADIANCE_OBSERVER_PROTOTYPES[name]
    assert len(argtypes) == len(declared[name])
    for argtype, parameter in zip(argtypes, declared[name]):
        abi_header.check_parameter(argtype, parameter, addresses=True)
    function = getattr(lib, name)
    assert list(function.argtypes) == list(argtypes) and function.restype is ctypes.c_int32
    for table in (abi.PROTOTYPES, abi.TWO_STREAM_PROTOTYPES, abi.THERMAL_PROTOTYPES,
                  abi.THERMAL_SOURCE_PROTOTYPES, abi.KDIST_PROTOTYPES, abi.SCATTERER_PROTOTYPES,
                  abi.THERMAL_RADIANCE_PROTOTYPES, abi.SOLAR_RADIANCE_PROTOTYPES,
                  abi.SCATTERER_RADIANCE_PROTOTYPES, abi.THERMAL_RADIANCE_SOURCE_PROTOTYPES,
                  abi.WING_PROTOTYPES, abi.RESULT_TYPES):
        assert name not in table
    assert '#include "lbl_amd.h"' in HEADER
    assert not set(declared) & set(abi_header.DECLARATIONS)
    assert callable(engine_module.Engine.path_thermal_radiance_observer)
    assert "include/lbl_amd_thermal_radiance_observer.h" in abi.__doc__


# ---------------------------------------------------------------------------------------------
# The requests.
BAD = [
    (dict(observer_interface=1.), "must be an integer"),
    (dict(observer_interface=np.array([1., 2., 3.])), "must be an integer"),
    (dict(observer_interface="1"), "must be an integer"),
    (dict(observer_interface=True), "must be an integer"),
    (dict(observer_interface=-1), r"0 \.\.\. 5"),
    (dict(observer_interface=6), r"0 \.\.\. 5"),
    (dict(observer_interface=[0, 6, 1]), r"0 \.\.\. 5"),
    (dict(observer_interface=[0, 1]), "shape"),
    (dict(observer_interface=np.zeros((3, 5), dtype=int)), "shape"),
    (dict(observer_interface=np.zeros((3, 1), dtype=int)), "shape"),
    (dict(looking="sideways"), "looking must be"),
    (dict(looking=None), "looking must be"),
    (dict(looking="Up"), "looking must be"),
    (dict(interface_temperature=np.full((3, 5), 250.)), "shape"),
    (dict(interface_temperature=np.full((3, 7), 250.)), "shape"),
    (dict(interface_temperature=changed(1, 2, np.nan)), "finite and > 0"),
    (dict(interface_temperature=changed(2, 5, 0.)), "finite and > 0"),
] + VIEW_BAD


@pytest.mark.parametrize("looking", oc.LOOKING)
@pytest.mark.parametrize("keywords, match", BAD)
def test_bad_arguments_are_refused_before_the_gpu(monkeypatch, keywords, match, looking):
    untouchable(monkeypatch)
    spec = make_spectroscopy((3, 5))
    call = dict(layer_thickness=ONES, surface_temperature=288., looking=looking)
    call.update(keywords)
    with pytest.raises(ValueError, match=match):
        spec.compute_thermal_radiance_at(**call)


def test_bands_and_instrument_exclude_each_other_and_group_is_not_offered(monkeypatch):
    untouchable(monkeypatch)
    from pylbl_amd.instrument import Instrument
    spec = make_spectroscopy((3, 5))
    instrument = Instrument.gaussian(np.array([600.2, 600.4]), 0.1)
    with pytest.raises(ValueError, match="band_edges or instrument, not both"):
        spec.compute_thermal_radiance_at(ONES, 288., 2, "up", band_edges=[600., 600.5],
                                         instrument=instrument)
    spec.group = object()
    with pytest.raises(NotImplementedError, match="compute_thermal_radiance_at"):
        spec.compute_thermal_radiance_at(ONES, 288.)


@pytest.mark.parametrize("surface_end", ["first", "last"])
@pytest.mark.parametrize("looking", oc.LOOKING)
def test_requests_map_the_interface_to_the_levels_passed(surface_end, looking):
    """All four combinations: looking down the ray passes the levels between the surface and the
    observer, looking up those between space and the observer; the surface is at interface 0
    ("first") or L."""
    spec = make_spectroscopy((3, 5))
    thickness = np.arange(1., 16.).reshape(3, 5)
    arguments = ([1., 0.5, 0.05], [1., 0.5, 0.], None, surface_end, 2., None, None, None,
                 ("brightness_temperature", "radiance"), None, None, "reference")
    plain = spec._thermal_radiance_request(thickness, [288., 270., 300.], *arguments)
    surface_at = 0 if surface_end == "first" else 5
    start_at = surface_at if looking == "down" else 5 - surface_at
    for given in (0, 1, 4, 5, np.int64(3), np.array([0, 2, 5]), [5, 0, 1], None):
        request = spec._thermal_radiance_at_request(thickness, [288., 270., 300.], given, looking,
                                                    None, *arguments)
        assert isinstance(request, two_stream._ThermalObserverRequest)
        assert isinstance(request, tuple) and request._fields[:len(plain._fields)] == plain._fields
        for name in plain._fields:
            assert np.array_equal(getattr(request, name), getattr(plain, name)), name
        assert request.edge_temperature is None and request.looking == looking
        interface = np.broadcast_to(5 - start_at if given is None else given, (3,))
        assert np.array_equal(request.observer_interface, interface)
        assert request.observer_interface.dtype == np.int64
        passed = request.observer_levels
        assert passed.dtype == np.int32 and passed.flags.c_contiguous and passed.shape == (3,)
        assert np.array_equal(passed, np.abs(interface - start_at))
        if given is None:
            assert np.all(passed == 5)
    linear = spec._thermal_radiance_at_request(thickness, [288., 270., 300.], 2, looking,
                                               INTERFACES, *arguments)
    expect = spec._thermal_radiance_linear_request(thickness, [288., 270., 300.], INTERFACES,
                                                   *arguments)
    for name in expect._fields:
        assert np.array_equal(getattr(linear, name), getattr(expect, name)), name


# ---------------------------------------------------------------------------------------------
# The queue.
def queue_of(spec, engine, limit_rows, method, **keywords):
    spec.device_output_limit = (8 << 30) if limit_rows is None else limit_rows*surface.ROW_BYTES
    engine.begin()
    engine.edge_tables, engine.view_edge_tables, engine.observer_levels = [], [], []
    result = getattr(spec, method)(**keywords)
    return list(engine.log), result


@pytest.mark.parametrize("surface_end", ["first", "last"])
@pytest.mark.parametrize("looking", oc.LOOKING)
@pytest.mark.parametrize("linear", [False, True])
def test_one_call_queues_the_flux_entry_then_one_observer_entry(tmp_path, monkeypatch, surface_end,
                                                                looking, linear):
    from pylbl_amd import spectroscopy
    monkeypatch.setattr(spectroscopy, "_XARRAY", [None])
    thickness = np.linspace(50., 300., 6).reshape(surface.SHAPE)
    both = ("radiance", "brightness_temperature")
    common = dict(layer_thickness=thickness, surface_temperature=[288., 270.],
                  view_zenith_cosine=[1., 0.4], surface=surface_end,
                  surface_emissivity=[[0.2, 0.4], [0.1, 0.3]], emissivity_wavenumber=[10., 70.],
                  diffusivity=2., quantities=both)
    source = dict(interface_temperature=surface.interfaces()) if linear else {}
    existing = "compute_thermal_radiance_linear" if linear else "compute_thermal_radiance"
    flux = "path_thermal_two_stream_source(" if linear else "path_thermal_two_stream("
    view_old = "path_thermal_radiance_source(" if linear else "path_thermal_radiance("
    view_new = "path_thermal_radiance_observer("
    surface_at = 0 if surface_end == "first" else 3
    start_at = surface_at if looking == "down" else 3 - surface_at
    with oc.recorded(tmp_path) as (spec, engine):
        # 5 blocks per level: 15 rows a path of three levels.
        for limit, runs in ((None, 1), (30, 1), (29, 2), (15, 2)):
            log, result = queue_of(spec, engine, limit, "compute_thermal_radiance_at",
                                   observer_interface=[1, 3], looking=looking, **source, **common)
            assert sum(line.startswith("compute(") for line in log) == 2*runs
            names = [line.split("(")[0] for line in log if line.startswith(
                ("surface_emissivity", "path_thermal"))]
            assert names == ["surface_emissivity"] + [flux[:-1], view_new[:-1]]*runs
            views = [line for line in log if line.startswith(view_new)]
            # Every run is handed every path's n_p; the entry picks the run's own.
            assert len(engine.observer_levels) == runs
            for passed in engine.observer_levels:
                assert passed.dtype == np.int32
                assert np.array_equal(passed, np.abs(np.array([1, 3]) - start_at))
            for view in views:
                assert argument(view, "view_up") == str(looking == "up")
                assert argument(view, "from_last") == str(surface_end == "first")
                assert ("edge_temperature" in view) == linear
                blocks = {argument(view, name) for name in
                          ("beta", "up_rows", "down_rows", "radiance_rows", "brightness_rows")}
                assert len(blocks) == 5 and argument(view, "band_start") == "None"
            for q in both:
                assert result[q].shape == (2, 160)
            assert np.array_equal(result["observer_interface"], [1, 3])
            assert result["looking"] == looking
            assert result.get("source") == ("linear_in_tau" if linear else None)
            # The flux call is the one the existing method records for the same arguments, and
            # the view entries differ by the observer alone.
            before, plain = queue_of(spec, engine, limit, existing, **source, **common)
            assert not any(line.startswith(view_new) for line in before)
            assert "observer_interface" not in plain and "looking" not in plain
            was = [line for line in before if line.startswith("path_thermal")]
            now = [line for line in log if line.startswith("path_thermal")]
            assert len(was) == len(now) == 2*runs
            for one, other in zip(was, now):
                if other.startswith(flux):
                    assert one == other
                    continue
                assert one.startswith(view_old)
                other = re.sub(r"\bview_up=[^,)]+(, )?", "", other.replace(view_new, view_old))
                assert sorted(re.findall(r"\b\w+=[^,)]+", one)) == \
                    sorted(re.findall(r"\b\w+=[^,)]+", other))
        with pytest.raises(ValueError, match="does not hold one path"):
            queue_of(spec, engine, 14, "compute_thermal_radiance_at", layer_thickness=thickness,
                     surface_temperature=288., looking=looking, **source)
        # Bands: the sweep writes a block of the call, the output receives its means.
        log, result = queue_of(spec, engine, None, "compute_thermal_radiance_at",
                               layer_thickness=thickness, surface_temperature=288.,
                               observer_interface=2, looking=looking, surface=surface_end,
                               surface_emissivity=0.3, band_edges=[20., 30., 60.], **source)
        view, = [line for line in log if line.startswith(view_new)]
        assert argument(view, "band_start") != "None" and "emissivity_rows=None" in view
        assert argument(view, "radiance_mean") != argument(view, "radiance_rows")
        assert "brightness_rows" not in view
        assert result["radiance"].shape == (2, 2)
        assert np.array_equal(result["observer_interface"], [2, 2])


def test_existing_calls_do_not_reach_the_new_entry(tmp_path):
    with oc.recorded(tmp_path) as (spec, engine):
        engine.begin()
        spec.compute_thermal_flux(np.ones(surface.SHAPE), 288.)
        spec.compute_thermal_radiance(np.ones(surface.SHAPE), 288.)
        spec.compute_thermal_radiance_linear(np.ones(surface.SHAPE), 288., surface.interfaces())
        spec.compute_radiance(np.ones(surface.SHAPE), boundary_temperature=288.)
        assert any(line.startswith("path_thermal_radiance_source") for line in engine.log)
        assert not any(line.startswith("path_thermal_radiance_observer") for line in engine.log)
    # The recorder of the linear call knows nothing of the new entry, and that call needs nothing
    # else.
    with src.recorded(tmp_path) as (spec, engine):
        assert not hasattr(engine, "path_thermal_radiance_observer")
        engine.begin()
        spec.compute_thermal_radiance_linear(np.ones(surface.SHAPE), 288., surface.interfaces())
