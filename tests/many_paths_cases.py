"""What tests/test_many_paths_host.py (CPU) and tests/test_gpu_many_paths.py (GPU) share: problems
of more paths than one launch takes (kPathGridY = 65535 in the grid's y dimension), for every path
entry and for the band means behind them.

A problem is a pattern of P = 7 distinct paths of two levels on five columns, tiled to N paths.  P
does not divide 65535 (65535 % 7 = 1), so path 65535 -- the first path of the second launch, and
row 65535 of a block of per-path tables -- is another pattern path than path 0: a kernel that read
its per-path values at l.p - first_path in place of l.p - table_path, or a chunk of band means
written without its row offset, gives the values of the neighbouring pattern path.  The period of
tests/sweep_cases.py, PATHS = 3, divides 65535 and could not tell.

The mirrors of the case modules are wired to three paths.  The pattern therefore takes its paths
from three three-path problems of different seeds (PARTS), which share what a call takes once (the
grid, the solar and Rayleigh rows, the knots) and get per-path scalars from tables of nine distinct
values; the first seven of the nine paths are the pattern, and what the mirrors give per path or
per level is concatenated in the same way (part_paths, part_levels).  Every part is a problem of
the kind its mirror already stays inside; tests/test_many_paths_host.py confirms it with the
mirrors' own worst_error."""
import numpy as np

from tests import jacobian_cases as jac
from tests import linear_source_cases as linear
from tests import scatterer_cases as sc
from tests import solar_cases as solar
from tests import surface_cases as surface
from tests import sweep_cases as cases
from tests import thermal_cases as tc
from tests import thermal_radiance_cases as rc
from tests import thermal_source_cases as tsc
from tests import two_stream_cases as ts

F64, LD = np.float64, np.longdouble
GRID_Y = 65535              # kPathGridY of csrc/path.h: paths, or rows of means, per launch
P = 7                       # the period
PARTS = 3                   # three-path problems behind a pattern
N2 = GRID_Y + 7             # two launches
N3 = 2*GRID_Y + 3           # three launches: lbl_path_compute and lbl_path_thermal_radiance
LEVELS = 2                  # per path: the sweeps take a step, a cloudy level reads the next one
COLUMNS = 5                 # one workgroup in x, a one-column tail lane
LAYOUTS = ("aligned", "odd")        # the vector and the scalar kernels
BANDS = np.array([0, 2, 2, 5], dtype=np.int64)      # the middle band is empty
KNOTS = 3                   # of lbl_surface_emissivity's tables and of the spectral scatterers

# Per-path scalars of the nine paths of the parts: the first seven, the pattern's, differ.
BOUNDARY_T = (0., 288., 215., 301., 260., 245., 273., 230., 250.)      # path 0: no boundary
BOUNDARY_E = (1., 0.9, 0., 0.97, 0.5, 0.25, 0.75, 0.6, 0.4)
JACOBIAN_T = (301., 288., 215., 260., 245., 273., 230., 250., 295.)    # all behind a boundary
SURFACE_T = (270., 288., 305., 255., 295., 280., 263., 300., 275.)
SURFACE_E = (1., 0.7, 0., 0.85, 0.4, 0.15, 0.55, 0.9, 0.3)
MU0 = (1., 1e-3, 0.25, 0.5, 0.75, 0.1, 0.9, 0.6, 0.4)                  # solar_cases.MU0 and on
ALBEDO = (1., 0.3, 0., 0.8, 0.55, 0.15, 0.65, 0.9, 0.45)               # solar_cases.ALBEDO and on
VIEW_MU = (1., 0.6, 0.05, 0.8, 0.3, 0.15, 0.45, 0.7, 0.9)              # thermal_radiance_cases.MU
VIEW_EPS = (1., 0.3, 0., 0.9, 0.6, 0.15, 0.75, 0.5, 0.2)               # thermal_cases.EMISSIVITY


# ---------------------------------------------------------------------------------------------
# From the parts to the pattern, from the pattern to N paths.
def three(table, part):
    """The values of a nine-path table for the three paths of a part."""
    return np.array(table[3*part:3*part + 3], dtype=F64)


def part_paths(values):
    """[3, ...] per part -> [P, ...]."""
    values = list(values)
    assert len(values) == PARTS and all(v.shape[0] == 3 for v in values)
    return np.concatenate(values)[:P]


def part_levels(values, rows_per_level=1):
    """[3*LEVELS*rows_per_level, ...] per part -> [P*LEVELS*rows_per_level, ...]."""
    values = list(values)
    assert len(values) == PARTS and all(v.shape[0] == 3*LEVELS*rows_per_level for v in values)
    return np.concatenate(values)[:P*LEVELS*rows_per_level]


def tile_paths(values, n_paths, first_path=0, rows_per_path=1):
    """Rows of the paths first_path .. n_paths - 1 from a pattern's [P*rows_per_path, ...]."""
    path = np.arange(first_path, n_paths) % P
    index = path[:, None]*rows_per_path + np.arange(rows_per_path)
    return np.asarray(values)[index.ravel()]


def tile_levels(values, n_paths, first_path=0):
    return tile_paths(values, n_paths, first_path, LEVELS)


def pairwise_distinct(rows):
    """Whether no two rows of [rows, ...] are equal."""
    rows = np.asarray(rows).reshape(len(rows), -1)
    return all(not np.array_equal(rows[i], rows[j])
               for i in range(len(rows)) for j in range(i + 1, len(rows)))


def levels_distinct(table):
    """Whether a per-level table [P*LEVELS, ...] differs between any two paths at every level."""
    table = np.asarray(table).reshape(P, LEVELS, -1)
    return all(pairwise_distinct(table[:, level]) for level in range(LEVELS))


# ---------------------------------------------------------------------------------------------
# Runs of flat levels (first level, count) in storage order, and the cut at the launch edge.
def run_sets(n_paths, continues):
    """{name: runs}: the whole block; whole paths from path 2 on (run.first_path != 0: the later
    launch starts at path 2 + 65535); with `continues` the levels [1, 2N - 1) -- a partial first
    path in the first launch, whole paths across the launch edge, an unfinished last path --
    between the two one-level runs that start and finish them."""
    levels = n_paths*LEVELS
    sets = {"whole": [(0, levels)], "from path 2": [(2*LEVELS, levels - 2*LEVELS)]}
    if continues:
        sets["inside paths"] = [(0, 1), (1, levels - 2), (levels - 1, 1)]
    return sets


def cut_at_the_launch_edge(n_paths):
    levels = n_paths*LEVELS
    return [(0, GRID_Y*LEVELS), (GRID_Y*LEVELS, levels - GRID_Y*LEVELS)]


def first_path_of(runs):
    return min(first for first, _ in runs)//LEVELS


def launches(paths):
    """PathCall::launch: the number of launches for a run of `paths` paths."""
    return -(-paths//GRID_Y)


def mean_chunks(rows):
    """PathBands::means: the number of chunks for `rows` rows."""
    return -(-rows//GRID_Y)


# ---------------------------------------------------------------------------------------------
# The sweeps of tests/sweep_cases.py: lbl_path_compute, lbl_path_radiance_source and _surface,
# lbl_path_flux, lbl_path_jacobian, lbl_path_solar and lbl_surface_emissivity.
class SweepPattern(object):
    """Three sweep_cases.Problem on one grid and their seven pattern paths: beta [P*LEVELS,
    COLUMNS], thickness, temperature, edges [P*LEVELS(, 2)], view lengths, the per-path scalars,
    emissivity and reflection rows [P, COLUMNS], and the knot tables [P, KNOTS]."""
    def __init__(self):
        rng = np.random.default_rng(7001)
        self.parts = [cases.Problem(COLUMNS, LEVELS, seed=700 + 10*i) for i in range(PARTS)]
        self.nu = self.parts[0].nu
        self.solar = solar.solar_row(self.parts[0])
        self.knots = np.array([0.3, 0.55, 0.8])*self.nu[-1]
        for i, problem in enumerate(self.parts):
            problem.nu = self.nu
            if i > 0:
                # One level without thickness (path 0, level 1) is enough: the others differ.
                problem.thickness[1] = rng.uniform(0.5, 1.5)
            problem.boundary_t, problem.boundary_e = three(BOUNDARY_T, i), three(BOUNDARY_E, i)
            problem.jacobian_t = three(JACOBIAN_T, i)
            problem.surface_t, problem.surface_e = three(SURFACE_T, i), three(SURFACE_E, i)
            problem.mu0, problem.albedo = three(MU0, i), three(ALBEDO, i)
            problem.edges = linear.edge_table(linear.interfaces_for(problem, 710 + i))
            problem.solar_lengths, _ = solar.lengths_of(problem, problem.mu0)
            # (lengths_of's view lengths depend on the depth alone: the parts would share them)
            problem.view_lengths = rng.uniform(0.5, 2.5, size=problem.levels)
            if i == 0:
                problem.view_lengths[2] = 0.
            problem.e_rows = rng.uniform(0., 1., size=(3, COLUMNS))
            problem.d_rows = rng.uniform(0., 0.2, size=(3, COLUMNS))
            problem.albedo_rows = rng.uniform(0., 1., size=(3, COLUMNS))
            problem.knot_values = rng.uniform(0., 1., size=(3, KNOTS))
        first = self.parts[0]
        first.e_rows[1], first.e_rows[2, ::2] = 1., 0.
        first.albedo_rows[1], first.albedo_rows[2, ::2] = 1., 0.
        first.knot_values[0] = 0.625
        for name in ("boundary_t", "boundary_e", "jacobian_t", "surface_t", "surface_e", "mu0",
                     "albedo", "e_rows", "d_rows", "albedo_rows", "knot_values"):
            setattr(self, name, part_paths(getattr(p, name) for p in self.parts))
        for name in ("beta", "thickness", "temperature", "edges", "solar_lengths",
                     "view_lengths"):
            setattr(self, name, part_levels(getattr(p, name) for p in self.parts))

    def flux_lengths(self, angles):
        """(s_l/mu_k [P*LEVELS, K] as the host forms them, weights [K])."""
        both = [p.lengths(angles) for p in self.parts]
        return part_levels(x[0] for x in both), both[0][1]

    def per_path_tables(self):
        """{name: [P, ...]}: every table the kernels index by path."""
        return {name: getattr(self, name) for name in (
            "boundary_t", "boundary_e", "jacobian_t", "surface_t", "surface_e", "mu0", "albedo",
            "e_rows", "d_rows", "albedo_rows", "knot_values")}

    def per_level_tables(self):
        return {name: getattr(self, name) for name in (
            "beta", "thickness", "temperature", "edges", "solar_lengths", "view_lengths")}


_STORE = {}


def once(key, make):
    """A pattern or a mirror, formed once and left unchanged."""
    if key not in _STORE:
        _STORE[key] = make()
    return _STORE[key]


def sweep_pattern():
    return once("sweep", SweepPattern)


def path_mirror(from_last):
    """{"loop": the float64 tau in the stated order, "tau", "mag", "trans": long double; each
    [P*LEVELS, COLUMNS] after every level}."""
    def make():
        parts = sweep_pattern().parts
        loop = part_levels(cases.sweep_tau(F64, p.beta, p.thickness, LEVELS, from_last)[0]
                           for p in parts)
        both = [cases.sweep_tau(LD, p.beta, p.thickness, LEVELS, from_last) for p in parts]
        with np.errstate(under="ignore", over="ignore"):
            trans = np.exp(-loop.astype(LD))
        return {"loop": loop, "tau": part_levels(x[0] for x in both),
                "mag": part_levels(x[1] for x in both), "trans": trans}
    return once(("path", from_last), make)


def final_level(from_last):
    """The level of a path its sweep ends on."""
    return 0 if from_last else LEVELS - 1


def finals(per_level, from_last):
    """[P, ...]: the rows of each pattern path's last level in sweep order."""
    return per_level[np.arange(P)*LEVELS + final_level(from_last)]


def radiance_mirror(from_last, linear_source, rows):
    """(I, magnitude) [P*LEVELS, COLUMNS] after every level in long double: the paths start from
    eps*B(T_b) under boundary_t (path 0 has no boundary), or with `rows` from E*B(T_b) +
    (1 - E)*D of the emissivity and reflection rows under jacobian_t: a reflecting surface needs
    a boundary behind every path of the run."""
    def make():
        both = []
        for p in sweep_pattern().parts:
            start, start_mag = surface.surface_start(
                LD, p.nu, p.jacobian_t if rows else p.boundary_t,
                p.e_rows if rows else p.boundary_e,
                *((p.d_rows, np.abs(p.d_rows)) if rows else (None, None)))
            both.append(surface.restart(LD, p, p.thickness, from_last, start, start_mag,
                                        p.edges if linear_source else None))
        return part_levels(x[0] for x in both), part_levels(x[1] for x in both)
    return once(("radiance", from_last, linear_source, rows), make)


def flux_mirror(angles, surface_first):
    """test_gpu_sweep_shapes.expect_flux's references on the pattern: {name: (value, magnitude)}
    for "down" and "up" [P*LEVELS, COLUMNS], "reflection" and "surface" [P, COLUMNS]."""
    def make():
        down_last = surface_first
        w, pi = None, LD(cases.FLUX_PI)
        found = {name: [] for name in ("down", "up", "reflection", "surface")}
        for p in sweep_pattern().parts:
            lengths, weight = p.lengths(angles)
            w = weight.astype(LD)
            down = cases.sweep_flux(LD, p.nu, p.beta, lengths, weight, p.temperature, LEVELS,
                                    down_last)
            start, start_mag = cases.surface_start(LD, p.nu, p.surface_t, p.surface_e,
                                                   down.total, down.total_mag)
            up = cases.sweep_flux(LD, p.nu, p.beta, lengths, weight, p.temperature, LEVELS,
                                  not down_last, start, start_mag)
            found["down"].append((down.flux, down.flux_mag))
            found["up"].append((up.flux, up.flux_mag))
            found["reflection"].append((down.total, down.total_mag))
            found["surface"].append(tuple(
                pi*cases.flux_sum(w, np.repeat(x[:, None, :], angles, axis=1))
                for x in (start, start_mag)))
        gather = {"down": part_levels, "up": part_levels, "reflection": part_paths,
                  "surface": part_paths}
        return {name: tuple(gather[name](x[i] for x in found[name]) for i in range(2))
                for name in found}
    return once(("flux", angles, surface_first), make)


def jacobian_mirror(from_last):
    """jacobian_cases.jacobian on the seven paths at once (it takes any number of them)."""
    def make():
        pattern = sweep_pattern()
        return jac.jacobian(LD, pattern.nu, pattern.beta, pattern.thickness, pattern.temperature,
                            LEVELS, from_last, pattern.jacobian_t, pattern.boundary_e)
    return once(("jacobian", from_last), make)


def solar_mirror(from_last, view, albedo_rows):
    """test_gpu_solar_shapes.check_solar's references on the pattern: "f0", "tau" and "tv" in
    float64 as the loop leaves them, "direct" and "reflected" in long double."""
    def make():
        found = {name: [] for name in ("f0", "tau", "tv", "direct", "reflected")}
        for p in sweep_pattern().parts:
            albedo = p.albedo_rows if albedo_rows else p.albedo
            loop = solar.mirror(F64, p, p.mu0, sweep_pattern().solar, p.solar_lengths, from_last,
                                p.view_lengths if view else None, albedo)
            found["f0"].append(loop["f0"])
            found["tau"].append(loop["tau"])
            found["direct"].append(solar.direct(LD, loop["f0"], loop["tau"], LEVELS))
            if view:
                found["tv"].append(loop["tv"])
                found["reflected"].append(solar.reflected(LD, loop["f0"], albedo, loop["tau"],
                                                          loop["tv"], LEVELS, from_last))
        out = {"f0": part_paths(found["f0"]), "tau": part_levels(found["tau"]),
               "direct": part_levels(found["direct"])}
        if view:
            out["tv"] = part_levels(found["tv"])
            out["reflected"] = part_paths(found["reflected"])
        return out
    return once(("solar", from_last, view, albedo_rows), make)


def emissivity_mirror(kind):
    """lbl_surface_emissivity's rows [P, COLUMNS] of the pattern's knot tables."""
    pattern = sweep_pattern()
    return surface.emissivity(kind, pattern.knots, pattern.knot_values, pattern.nu)


# ---------------------------------------------------------------------------------------------
# The whole-path two-stream entries.
class FluxPattern(object):
    """Three Inputs of a two-stream case module and their seven pattern paths: beta and table
    [P*LEVELS, ...], the per-path scalars, and what the entry in question takes besides."""
    per_path = ()
    per_level = ("beta", "table")

    def gather(self):
        for name in self.per_path:
            setattr(self, name, part_paths(getattr(p, name) for p in self.parts))
        for name in self.per_level:
            setattr(self, name, part_levels(getattr(p, name) for p in self.parts))
        self.nu = getattr(self.parts[0], "nu", None)

    def per_path_tables(self):
        return {name: getattr(self, name) for name in self.per_path}

    def per_level_tables(self):
        return {name: getattr(self, name) for name in self.per_level}

    def mirrored(self, mirror, names, scale):
        """{name: (long-double value, scale)} of `names` and their "top_" rows from
        mirror(part) -> dict, the scale [3, COLUMNS] of a part under its key `scale`."""
        found = [mirror(p) for p in self.parts]
        top = part_paths(np.asarray(x[scale], dtype=LD) for x in found)
        out = {}
        for q in names:
            out[q] = (part_levels(x[q] for x in found), np.repeat(top, LEVELS, axis=0))
            out["top_" + q] = (part_paths(x["top_" + q] for x in found), top)
        return out


def _conservative_cloud(inputs, level, column, w_word, tau_word=None):
    """Makes `level` of a part a conservative cloud over no absorber in `column`: omega_c = 1
    (w_c = tau_c) and beta = 0 there."""
    if tau_word is not None:
        assert inputs.table[level, tau_word] > 0.
        inputs.table[level, w_word] = inputs.table[level, tau_word]
    inputs.beta[level, column] = 0.


class ShortwavePattern(FluxPattern):
    """lbl_path_two_stream (spectral: lbl_path_two_stream_spectral with KNOTS knots)."""
    per_path = ("mu0", "albedo", "albedo_rows")

    def __init__(self, spectral):
        rng = np.random.default_rng(7002)
        if spectral:
            self.parts = [sc.shortwave_inputs(COLUMNS, LEVELS, KNOTS, 800 + 10*i)
                          for i in range(PARTS)]
            self.per_level = FluxPattern.per_level + ("optics",)
        else:
            self.parts = [ts.shape_inputs(COLUMNS, LEVELS, 800 + 10*i) for i in range(PARTS)]
        first = self.parts[0]
        for i, inputs in enumerate(self.parts):
            inputs.solar, inputs.sigma = first.solar, first.sigma
            inputs.mu0, inputs.scalar_albedo = three(MU0, i), three(ALBEDO, i)
            inputs.albedo = inputs.scalar_albedo
            inputs.albedo_rows = rng.uniform(0., 1., size=(3, COLUMNS))
            if i > 0:
                # shape_inputs' level without thickness and air (path 0, level 1): once.
                inputs.table[1, 0] = rng.uniform(0.5, 1.5)
                inputs.table[1, 1] = inputs.table[1, 0]*rng.uniform(0.2e30, 1e30)
            if spectral:
                inputs.nu, inputs.knots = first.nu, first.knots
        first.albedo_rows[1], first.albedo_rows[2, ::2] = 1., 0.
        # A level that scatters and does not absorb: Rayleigh scattering alone over beta = 0.
        first.table[2, 1], first.table[2, 2:] = 0.6e30, 0.
        if spectral:
            first.optics[2] = 0.
        first.beta[2, 1] = 0.
        self.gather()
        self.solar, self.sigma = first.solar, first.sigma
        self.knots = first.knots if spectral else None
        self.spectral = spectral

    def use_albedo_rows(self, rows):
        for inputs in self.parts:
            inputs.albedo = inputs.albedo_rows if rows else inputs.scalar_albedo

    def mirror(self, from_last, albedo_rows):
        def make():
            self.use_albedo_rows(albedo_rows)
            try:
                return self.mirrored(lambda p: ts.mirror(LD, p, from_last), ts.QUANTITIES, "f0")
            finally:
                self.use_albedo_rows(False)
        return once(("shortwave", self.spectral, from_last, albedo_rows), make)

    def f0(self):
        return part_paths(p.f0() for p in self.parts)

    def worst_error(self, from_last, albedo_rows):
        self.use_albedo_rows(albedo_rows)
        try:
            return [ts.worst_error(p, from_last) for p in self.parts]
        finally:
            self.use_albedo_rows(False)

    def branches(self):
        return np.concatenate([p.layer_inputs(False)["branch"].ravel() for p in self.parts])


class LongwavePattern(FluxPattern):
    """lbl_path_thermal_two_stream ("isothermal"), lbl_path_thermal_two_stream_source ("linear")
    and lbl_path_thermal_two_stream_spectral ("spectral": either source); the isothermal parts
    are lbl_path_thermal_radiance's too, under VIEW_MU and VIEW_EPS."""
    per_path = ("surface_t", "emissivity", "emissivity_rows", "view_mu")

    def __init__(self, source):
        rng = np.random.default_rng(7003)
        seeds = [900 + 10*i for i in range(PARTS)]
        if source == "isothermal":
            self.parts = [tc.shape_inputs(COLUMNS, LEVELS, seed) for seed in seeds]
        elif source == "linear":
            self.parts = [tsc.shape_inputs(COLUMNS, LEVELS, seed) for seed in seeds]
        else:
            self.parts = [sc.longwave_inputs(COLUMNS, LEVELS, KNOTS, seed) for seed in seeds]
            self.per_level = FluxPattern.per_level + ("optics",)
        if source != "isothermal":
            self.per_level = self.per_level + ("edges",)
        first = self.parts[0]
        for i, inputs in enumerate(self.parts):
            inputs.nu = first.nu
            inputs.surface_t = three(SURFACE_T, i)
            inputs.scalar_emissivity = three(VIEW_EPS, i)
            inputs.emissivity = inputs.scalar_emissivity
            inputs.emissivity_rows = rng.uniform(0., 1., size=(3, COLUMNS))
            inputs.view_mu = three(VIEW_MU, i)
            if i > 0:
                inputs.table[1, 0] = rng.uniform(0.5, 1.5)     # shape_inputs' s_l = 0: once
            if source != "isothermal" and i > 0:
                # interfaces_for's isothermal path and its jumps once, in part 0: the rest random.
                inputs.interfaces = rng.uniform(150., 320., size=(3, LEVELS + 1))
                inputs.edges = linear.edge_table(inputs.interfaces)
                inputs.table[:, 4] = rng.uniform(150., 320., size=3*LEVELS)
            if source == "spectral":
                inputs.knots = first.knots
        first.emissivity_rows[1], first.emissivity_rows[2, ::2] = 1., 0.
        if source == "spectral":
            # A scatterer with omega_c = 1 at every knot over no absorber.
            first.optics[0, :, 0], first.optics[0, :, 1] = 0.8, 1.
            _conservative_cloud(first, 0, 1, None)
        else:
            cloudy = int(np.flatnonzero(first.table[:, 2] > 0.)[0])
            _conservative_cloud(first, cloudy, 1, 2, 1)
        self.gather()
        self.knots = first.knots if source == "spectral" else None
        self.diffusivity = first.diffusivity
        self.source = source

    def use_emissivity_rows(self, rows):
        for inputs in self.parts:
            inputs.emissivity = inputs.emissivity_rows if rows else inputs.scalar_emissivity

    def _mirror_of(self, kind, inputs, from_last, linear_source):
        if self.source == "spectral":
            return sc.longwave_mirror(kind, inputs, from_last, linear_source)
        return tsc.mirror(kind, inputs, from_last) if linear_source else \
            tc.mirror(kind, inputs, from_last)

    def mirror(self, from_last, emissivity_rows, linear_source):
        assert linear_source == (self.source == "linear") or self.source == "spectral"
        def make():
            self.use_emissivity_rows(emissivity_rows)
            try:
                return self.mirrored(lambda p: self._mirror_of(LD, p, from_last, linear_source),
                                     tc.QUANTITIES, "scale")
            finally:
                self.use_emissivity_rows(False)
        return once(("longwave", self.source, from_last, emissivity_rows, linear_source), make)

    def worst_error(self, from_last, emissivity_rows, linear_source):
        self.use_emissivity_rows(emissivity_rows)
        try:
            if self.source == "spectral":
                return [sc.longwave_worst_error(p, from_last, linear_source) for p in self.parts]
            module = tsc if linear_source else tc
            return [module.worst_error(p, from_last) for p in self.parts]
        finally:
            self.use_emissivity_rows(False)

    def branches(self):
        return np.concatenate([p.layer_inputs(False)["branch"].ravel() for p in self.parts])

    # lbl_path_thermal_radiance, on the isothermal pattern.
    def flux_rows(self, from_last):
        """{"up", "down"} [P*LEVELS, COLUMNS]: the float64 flux rows the numpy mirror of
        lbl_path_thermal_two_stream gives for the pattern (scalar emissivities)."""
        assert self.source == "isothermal"
        def make():
            found = [rc.flux_rows(p, from_last) for p in self.parts]
            return {q: part_levels(x[q] for x in found) for q in tc.QUANTITIES}
        return once(("flux rows", from_last), make)

    def view_mirror(self, from_last):
        """{"radiance": (long-double value, scale)} [P, COLUMNS]."""
        assert self.source == "isothermal"
        def make():
            found = [rc.mirror(LD, p, p.view_mu, from_last, rc.flux_rows(p, from_last))
                     for p in self.parts]
            return {"radiance": (part_paths(x["radiance"] for x in found),
                                 part_paths(x["scale"] for x in found))}
        return once(("view", from_last), make)

    def view_worst_error(self, from_last):
        return [rc.worst_error(p, p.view_mu, from_last) for p in self.parts]


def shortwave_pattern(spectral=False):
    return once(("shortwave pattern", spectral), lambda: ShortwavePattern(spectral))


def longwave_pattern(source="isothermal"):
    return once(("longwave pattern", source), lambda: LongwavePattern(source))
