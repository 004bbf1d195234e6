"""Spectroscopy.compute_radiance within its limits: more paths than a launch grid's y dimension
takes, and the argument checks of the C ABI (Engine.path_radiance), after which the engine stays
usable."""
import numpy as np
import pytest

from pylbl_amd import MemoryDatabase, Spectroscopy, synthetic
from pylbl_amd.spectroscopy import PLANCK_C1, PLANCK_C2

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


def test_more_paths_than_the_grid_y_limit():
    """70 000 paths of two levels, downward with a boundary per path: the sweep takes several
    launches and the 140 000 levels several runs.  The reference absorption comes from four
    Spectroscopy objects of 17 500 paths each (one call takes at most 65 535 levels)."""
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
    lengths = np.random.default_rng(2).uniform(0.5, 1.5, size=shape)
    lengths *= 5./np.max(np.sum(beta, axis=-2))
    surface = np.linspace(250., 310., shape[0])
    out = spec.compute_radiance(lengths, boundary_temperature=surface,
                                direction="toward_first", remove_pedestal=False)
    t = spec.atmosphere.temperature
    rad = planck(grid, surface[:, None])
    for level in (1, 0):
        x = lengths[:, level, None]*beta[:, level, :]
        rad = rad*np.exp(-x) + planck(grid, t[:, level, None])*(-np.expm1(-x))
    error = np.abs(out["radiance"] - rad)/rad
    assert error.max() <= 1.e-12, error.max()
    edges = [600., 600.2, 600.45, 601.]
    bands = spec.compute_radiance(lengths, boundary_temperature=surface,
                                  direction="toward_first", band_edges=edges,
                                  remove_pedestal=False)
    starts = np.searchsorted(grid, edges)
    for b in range(3):
        expect = rad[:, starts[b]:starts[b + 1]].mean(axis=-1)
        error = np.abs(bands["radiance"][:, b] - expect)/expect
        assert error.max() <= 1.e-12, error.max()


def test_c_abi_rejects_bad_arguments_and_stays_usable():
    from pylbl_amd import engine as engine_module
    from pylbl_amd.mt_ckd import resident_grid
    engine = engine_module.default_engine(0)
    lib = engine.lib
    paths, per_path, n, columns = 2, 3, 64, 60
    wavenumber = np.arange(600., 600.6, 0.01)[:columns]
    grid = resident_grid(engine, wavenumber)
    short = engine.load_grid(wavenumber[:50])
    beta = engine.blocks.take(paths*per_path, n)
    carry = engine.blocks.take(paths, n)
    rad = engine.blocks.take(paths, n)
    lengths = np.ones(paths*per_path)
    temps = np.full(paths*per_path, 250.)
    tb = np.array([280., 0.])
    eb = np.array([1., 0.5])
    starts = np.array([0, 10, 60], dtype=np.int64)
    RAD, BT = engine_module.PATH_RADIANCE, engine_module.PATH_BRIGHTNESS
    CONT, LAST = engine_module.PATH_CONTINUE, engine_module.PATH_FROM_LAST
    CUM = engine_module.PATH_CUMULATIVE

    def pointer(array):
        return array.ctypes.data if array is not None else None

    def call(beta_p=beta.pointer, stride=n, cols=columns, grid_h=grid, n_paths=paths,
             levels=per_path, begin=0, count=paths*per_path, length=lengths, temperature=temps,
             boundary_t=tb, boundary_e=eb, n_bands=0, band=None, carry_p=carry.pointer,
             rad_p=rad.pointer, bt_p=None, flags=RAD):
        return lib.lbl_path_radiance(
            engine.handle, beta_p, stride, cols, grid_h, n_paths, levels, begin, count,
            pointer(length), pointer(temperature), pointer(boundary_t), pointer(boundary_e),
            n_bands, pointer(band), carry_p, rad_p, bt_p, flags)
    try:
        engine.fill_zero(beta)
        bad = [
            dict(beta_p=None), dict(carry_p=None), dict(rad_p=None), dict(length=None),
            dict(temperature=None), dict(flags=0), dict(flags=BT), dict(grid_h=-1),
            dict(grid_h=short), dict(cols=n + 1), dict(cols=0), dict(n_paths=0), dict(levels=0),
            dict(begin=-1), dict(count=0), dict(begin=1, count=paths*per_path),
            dict(begin=1, count=2),                     # inside a path without LBL_PATH_CONTINUE
            dict(begin=3, count=3, flags=RAD | CONT),   # starts a path with it
            dict(begin=0, count=2, flags=RAD | LAST),   # downward, inside a path, no CONTINUE
            dict(length=np.array([1., 1., -1., 1., 1., 1.])),
            dict(length=np.array([1., np.inf, 1., 1., 1., 1.])),
            dict(temperature=np.array([250., 0., 250., 250., 250., 250.])),
            dict(temperature=np.array([250., 250., np.nan, 250., 250., 250.])),
            dict(boundary_t=np.array([-1., 280.])), dict(boundary_t=np.array([np.inf, 280.])),
            dict(boundary_e=np.array([1.5, 1.])), dict(boundary_e=np.array([np.nan, 1.])),
            dict(n_bands=2, band=None), dict(n_bands=-1),
            dict(n_bands=2, band=np.array([0, 30, 20], dtype=np.int64)),
            dict(n_bands=2, band=np.array([0, 10, 61], dtype=np.int64)),
            dict(n_bands=2, band=starts, bt_p=rad.pointer, flags=RAD | BT),
        ]
        for arguments in bad:
            assert call(**arguments) == 2, arguments        # LBL_BAD_ARGUMENT
            assert lib.lbl_last_error(engine.handle).decode().startswith("lbl_path_radiance")
        # beta = 0: what leaves a path is its boundary term.
        assert call() == 0
        got = rad.to_host()[:, :columns]
        assert np.array_equal(got[1], np.zeros(columns))
        expect = planck(wavenumber, 280.)
        assert np.max(np.abs(got[0] - expect)/expect) <= 1.e-14
        assert call(begin=1, count=2, flags=RAD | CONT) == 0
        assert call(begin=0, count=2, flags=RAD | LAST | CONT) == 0
        assert call(boundary_t=None, boundary_e=None, flags=RAD | LAST) == 0
        assert call(n_bands=2, band=starts) == 0
        assert call(flags=RAD | CUM | LAST, rad_p=beta.pointer) == 0
        with pytest.raises(ValueError):
            engine.path_radiance(beta, columns, grid, paths, per_path, 0, lengths, temps[:2],
                                 carry, radiance=rad)
    finally:
        engine.synchronize()
        engine.free_grid(short)
        for block in (beta, carry, rad):
            engine.blocks.give(block)
    spec = spectroscopy((5,), np.arange(600., 601., 0.01))
    out = spec.compute_radiance(np.zeros(5), boundary_temperature=280.)
    expect = planck(spec.grid, 280.)
    assert np.max(np.abs(out["radiance"] - expect)/expect) <= 1.e-14
