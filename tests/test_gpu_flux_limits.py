"""Spectroscopy.compute_flux within its limits: more paths than a launch grid's y dimension
takes, the most angles (K = 8), and the argument checks of the C ABI (lbl_path_flux), after which
the engine stays usable."""
import numpy as np
import pytest

from pylbl_amd import MemoryDatabase, Spectroscopy, synthetic
from pylbl_amd.spectroscopy import PLANCK_C1, PLANCK_C2, flux_angles

pytestmark = pytest.mark.gpu

GASES = ("H2O", "CO2", "O3")


def atmosphere(shape):
    full = synthetic.standard_atmosphere(int(np.prod(shape)))
    return synthetic.Atmos(p=full.p.reshape(shape), t=full.t.reshape(shape),
                           vmr={k: full.vmr[k].reshape(shape) for k in GASES})


def spectroscopy(shape, grid, atmos=None):
    tables = [synthetic.line_table(name, 576., 724., num_lines=3000, seed=40 + i)
              for i, name in enumerate(GASES)]
    atmos = atmosphere(shape) if atmos is None else atmos
    return Spectroscopy(atmos, grid, MemoryDatabase(tables))


def planck(nu, t):
    return (((PLANCK_C1*nu)*nu)*nu)/np.expm1((PLANCK_C2*nu)/t)


def weighted(weight, rad):
    total = weight[0]*rad[..., 0, :]
    for k in range(1, weight.size):
        total = total + weight[k]*rad[..., k, :]
    return total


def sweep_down_and_up(grid, beta, thickness, temperature, ts, es, angles):
    """Surface at level 0: (F_up, F_down) at the L + 1 interfaces, in numpy."""
    mu, weight = flux_angles(angles)
    lead, levels = beta.shape[:-2], beta.shape[-2]
    lengths = thickness[..., None]/mu
    up = np.zeros(lead + (levels + 1, grid.size))
    down = np.zeros(lead + (levels + 1, grid.size))

    def step(rad, l):
        x = lengths[..., l, :, None]*beta[..., l, None, :]
        return rad*np.exp(-x) + planck(grid, temperature[..., l, None])[..., None, :]*(-np.expm1(-x))
    rad = np.zeros(lead + (mu.size, grid.size))
    for l in range(levels - 1, -1, -1):
        rad = step(rad, l)
        down[..., l, :] = np.pi*weighted(weight, rad)
    start = es[..., None]*planck(grid, ts[..., None]) + (1. - es[..., None])*weighted(weight, rad)
    rad = np.repeat(start[..., None, :], mu.size, axis=-2)
    up[..., 0, :] = np.pi*weighted(weight, rad)
    for l in range(levels):
        rad = step(rad, l)
        up[..., l + 1, :] = np.pi*weighted(weight, rad)
    return up, down


def test_more_paths_than_the_grid_y_limit():
    """70 000 paths of two levels, a surface per path: the sweeps take several launches and the
    140 000 levels several runs.  The reference absorption comes from four Spectroscopy objects
    of 17 500 paths each (one call takes at most 65 535 levels)."""
    shape = (70000, 2)
    grid = np.arange(600., 600.64, 0.01)
    atmos = atmosphere(shape)
    spec = spectroscopy(shape, grid, atmos)
    parts = []
    for part in (slice(p, p + 17500) for p in range(0, 70000, 17500)):
        sub = synthetic.Atmos(p=atmos.p[part], t=atmos.t[part],
                              vmr={k: v[part] for k, v in atmos.vmr.items()})
        parts.append(np.asarray(spectroscopy(None, grid, sub).compute_absorption(
            "total", remove_pedestal=False)["absorption"]))
    beta = np.concatenate(parts)
    thickness = np.random.default_rng(2).uniform(0.5, 1.5, size=shape)
    thickness *= 3./np.max(np.sum(beta, axis=-2))
    ts = np.linspace(250., 310., shape[0])
    es = np.linspace(0.5, 1., shape[0])
    out = spec.compute_flux(thickness, ts, es, angles=2, remove_pedestal=False)
    up, down = sweep_down_and_up(grid, beta, thickness, spec.atmosphere.temperature, ts, es, 2)
    for q, expect in (("upward_flux", up), ("downward_flux", down)):
        got = out[q]
        ok = expect != 0.
        assert np.all(got[~ok] == 0.)
        error = np.abs(got[ok] - expect[ok])/expect[ok]
        assert error.max() <= 1.e-12, (q, error.max())
    edges = [600., 600.2, 600.45, 601.]
    bands = spec.compute_flux(thickness, ts, es, angles=2, band_edges=edges,
                              remove_pedestal=False)
    starts = np.searchsorted(grid, edges)
    for b in range(3):
        count = starts[b + 1] - starts[b]
        expect = up[..., starts[b]:starts[b + 1]].mean(axis=-1)*(count/100)
        error = np.abs(bands["upward_flux"][..., b] - expect)/expect
        assert error.max() <= 1.e-12, error.max()


def test_eight_angles():
    shape = (2, 6)
    grid = np.arange(600., 620., 0.01)
    spec = spectroscopy(shape, grid)
    beta = np.asarray(spec.compute_absorption("total", remove_pedestal=False)["absorption"])
    thickness = np.random.default_rng(5).uniform(0.5, 1.5, size=shape)
    thickness *= 8./np.max(np.sum(beta, axis=-2))
    ts, es = np.array([285., 300.]), np.array([0.95, 0.6])
    out = spec.compute_flux(thickness, ts, es, angles=8, remove_pedestal=False)
    up, down = sweep_down_and_up(grid, beta, thickness, spec.atmosphere.temperature, ts, es, 8)
    for q, expect in (("upward_flux", up), ("downward_flux", down)):
        ok = expect != 0.
        assert np.all(out[q][~ok] == 0.)
        error = np.abs(out[q][ok] - expect[ok])/expect[ok]
        assert error.max() <= 1.e-12, (q, error.max())


def test_c_abi_rejects_bad_arguments_and_stays_usable():
    from pylbl_amd import engine as engine_module
    from pylbl_amd.mt_ckd import resident_grid
    engine = engine_module.default_engine(0)
    lib = engine.lib
    paths, per_path, n, columns, angles = 2, 3, 64, 60, 2
    wavenumber = np.arange(600., 600.6, 0.01)[:columns]
    grid = resident_grid(engine, wavenumber)
    short = engine.load_grid(wavenumber[:50])
    beta = engine.blocks.take(paths*per_path, n)
    carry = engine.blocks.take(paths*angles, n)
    reflection = engine.blocks.take(paths, n)
    level = engine.blocks.take(paths*per_path, n)
    flux = engine.blocks.take(paths*per_path, 2)
    surface = engine.blocks.take(paths, 2)
    lengths = np.ones((paths*per_path, angles))
    weight = np.array([0.5, 0.5])
    temps = np.full(paths*per_path, 250.)
    ts = np.array([280., 300.])
    es = np.array([1., 0.5])
    starts = np.array([0, 10, 60], dtype=np.int64)
    UP = engine_module.PATH_FLUX_UP
    CONT, LAST = engine_module.PATH_CONTINUE, engine_module.PATH_FROM_LAST

    def pointer(array):
        return array.ctypes.data if array is not None else None

    def call(beta_p=beta.pointer, stride=n, cols=columns, grid_h=grid, n_paths=paths,
             levels=per_path, begin=0, count=paths*per_path, n_angles=angles, length=lengths,
             weights=weight, temperature=temps, surface_t=ts, surface_e=es, n_bands=0, band=None,
             carry_p=carry.pointer, reflection_p=reflection.pointer, level_p=level.pointer,
             flux_p=None, surface_p=None, flags=0):
        return lib.lbl_path_flux(
            engine.handle, beta_p, stride, cols, grid_h, n_paths, levels, begin, count, n_angles,
            pointer(length), pointer(weights), pointer(temperature), pointer(surface_t),
            pointer(surface_e), n_bands, pointer(band), carry_p, reflection_p, level_p, flux_p,
            surface_p, flags)
    try:
        engine.fill_zero(beta)
        bad = [
            dict(beta_p=None), dict(carry_p=None), dict(reflection_p=None), dict(level_p=None),
            dict(level_p=beta.pointer), dict(length=None), dict(weights=None),
            dict(temperature=None), dict(surface_t=None, flags=UP), dict(surface_e=None, flags=UP),
            dict(n_angles=0), dict(n_angles=9), dict(grid_h=-1), dict(grid_h=short),
            dict(cols=n + 1), dict(cols=0), dict(n_paths=0), dict(levels=0), dict(begin=-1),
            dict(count=0), dict(begin=1, count=paths*per_path),
            dict(begin=1, count=2),                     # inside a path without LBL_PATH_CONTINUE
            dict(begin=3, count=3, flags=CONT),         # starts a path with it
            dict(begin=0, count=2, flags=LAST),         # downward, inside a path, no CONTINUE
            dict(length=np.where(np.arange(12).reshape(6, 2) == 5, -1., 1.)),
            dict(length=np.where(np.arange(12).reshape(6, 2) == 11, np.inf, 1.)),
            dict(weights=np.array([0.5, -0.5])), dict(weights=np.array([np.nan, 1.])),
            dict(temperature=np.array([250., 0., 250., 250., 250., 250.])),
            dict(temperature=np.array([250., 250., np.nan, 250., 250., 250.])),
            dict(surface_t=np.array([0., 280.]), flags=UP),
            dict(surface_t=np.array([np.inf, 280.]), flags=UP),
            dict(surface_e=np.array([1.5, 1.]), flags=UP),
            dict(surface_e=np.array([np.nan, 1.]), flags=UP),
            dict(n_bands=2, band=None), dict(n_bands=-1),
            dict(n_bands=2, band=np.array([0, 30, 20], dtype=np.int64), flux_p=flux.pointer),
            dict(n_bands=2, band=np.array([0, 10, 61], dtype=np.int64), flux_p=flux.pointer),
            dict(n_bands=2, band=starts),                               # no flux output
            dict(n_bands=2, band=starts, flux_p=flux.pointer, flags=UP),  # no surface output
        ]
        for arguments in bad:
            assert call(**arguments) == 2, arguments        # LBL_BAD_ARGUMENT
            assert lib.lbl_last_error(engine.handle).decode().startswith("lbl_path_flux")
        # beta = 0: nothing comes down, R = 0, and every interface above the surface sees
        # eps*B(T_s).
        assert call(flags=LAST) == 0
        assert np.all(reflection.to_host()[:, :columns] == 0.)
        assert np.all(level.to_host()[:, :columns] == 0.)
        assert call(flags=UP) == 0
        got = level.to_host()[:, :columns]
        for p in range(paths):
            expect = np.pi*(es[p]*planck(wavenumber, ts[p]))
            error = np.abs(got[p*per_path:(p + 1)*per_path] - expect)/expect
            assert error.max() <= 1.e-14
            error = np.abs(reflection.to_host()[p, :columns] - expect)/expect
            assert error.max() <= 1.e-14
        # Runs that go on from the carry, the down sweep from the last level, band means.
        assert call(begin=1, count=2, flags=CONT) == 0
        assert call(begin=0, count=2, flags=LAST | CONT | UP) == 0
        assert call(n_bands=2, band=starts, flux_p=flux.pointer, surface_p=surface.pointer,
                    flags=UP) == 0
        assert call(n_angles=1, length=lengths[:, :1].copy(), weights=np.ones(1),
                    carry_p=carry.pointer) == 0
        with pytest.raises(ValueError):
            engine.path_flux(beta, columns, grid, paths, per_path, 0, lengths, weight, temps[:2],
                             carry, reflection, level)
    finally:
        engine.synchronize()
        engine.free_grid(short)
        for block in (beta, carry, reflection, level, flux, surface):
            engine.blocks.give(block)
    spec = spectroscopy((5,), np.arange(600., 601., 0.01))
    out = spec.compute_flux(np.zeros(5), 280.)
    expect = np.pi*planck(spec.grid, 280.)
    assert np.max(np.abs(out["upward_flux"] - expect)/expect) <= 1.e-14
    assert np.all(out["downward_flux"] == 0.)
