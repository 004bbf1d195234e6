"""Host orchestration: the counterpart of ``Spectroscopy.compute_absorption``
(pyLBL/spectroscopy.py:144-206) for all three mechanism slots: 0 "lines", 1 "continuum"
(MT-CKD), 2 "cross_section" (ARTS-crossfit).

What is kept from the reference: constructor keywords and the KeyError for an unknown
backend name (:88-118); molecule-outer / level-inner semantics with no state carried between
units (:166-191); beta[level, 0, :] = n * k[:grid.size] with n = P x /(kb T) (:18-29,
:181-191); ``remove_pedestal`` defaulting to ``continua_backend == "mt_ckd"`` (:163-164);
the three output formats (:208-235).

What is different: all levels of a molecule go to the GPU in one batched call and the
number-density scaling happens in the kernel epilogue; xarray is optional (not installed in
this image) -- without it the atmosphere is a plain (p, t, vmr) tuple and the result a dict
of numpy arrays with the same variable names.

What is in this module: Atmosphere, MoleculeCache and Spectroscopy -- every compute_* method
with its definition, and the sweeps of compute_path, compute_radiance, compute_jacobian,
compute_flux, compute_solar and compute_kdistribution.  Which module holds the rest:
    absorption.py   the host side of compute_absorption: the gases present, the queue orders of
                    its formats, total_into, the pipeline guard;
    paths.py        the path products' argument checks, the run loop, the HBM accounting, what
                    their sweepers share and their results; its public names stay importable
                    from here;
    two_stream.py   the requests, sweeps and results of the two-stream products:
                    compute_solar_flux, compute_thermal_flux, their _linear and _spectral
                    variants and compute_thermal_radiance.
Their functions take the Spectroscopy first; those a test reaches through it are its methods.
"""
from collections import namedtuple
import os

import numpy as np

from . import absorption, errors, paths, two_stream
from .paths import (CP_DRY, DOWNWELLING, FLUX_QUANTITIES, FLUX_SURFACES,  # noqa: F401
                    JACOBIAN_LEVEL_QUANTITIES, JACOBIAN_PATH_QUANTITIES, JACOBIAN_QUANTITIES, MAX_FLUX_ANGLES,
                    KDISTRIBUTION_QUANTITIES, MAX_G_INTERVALS, g_intervals, g_quadrature_points,
                    interval_columns, quantile_table,
                    PATH_CUMULATIVE, PATH_QUANTITIES, PLANCK_C1, PLANCK_C2, R_DRY,
                    RADIANCE_DIRECTIONS, RADIANCE_QUANTITIES, SOLAR_FLUX_QUANTITIES,
                    SOLAR_QUANTITIES,
                    SOLAR_SOLID_ANGLE, SOLAR_TEMPERATURE, SOURCES,
                    SURFACE_RADIANCE_QUANTITIES, band_columns, flux_angles,
                    heating_rate, _MAX_RUN_LEVELS, _PATH_UNITS, _Pass, _Product, _cut_runs,
                    _path_layout, _run_edges, _sweep_pass)
from .plugins import continua, cross_sections, molecular_lines

kb = 1.38064852e-23  # Boltzmann constant [J K-1] (pyLBL/spectroscopy.py:15).

MECHANISMS = ["lines", "continuum", "cross_section"]


def number_density(temperature, pressure, volume_mixing_ratio):
    """Ideal-gas number density [m-3] (pyLBL/spectroscopy.py:18-29)."""
    return pressure*volume_mixing_ratio/(kb*temperature)


_STANDARD_NAME_PREFIX = "mole_fraction_of_"
_FORMULAE = {"water_vapor": "H2O", "carbon_dioxide": "CO2", "ozone": "O3",
             "nitrous_oxide": "N2O", "carbon_monoxide": "CO", "methane": "CH4",
             "oxygen": "O2", "nitrogen": "N2"}


_XARRAY = []


def _optional_xarray():
    """The xarray module, or None where it is not installed -- looked for ONCE: a failed import
    walks every entry of sys.path again (60 us per compute_absorption call, behind its last wait:
    profiles/r05_perf_api_profile.txt)."""
    if not _XARRAY:
        try:
            import xarray
            _XARRAY.append(xarray)
        except ImportError:
            _XARRAY.append(None)
    return _XARRAY[0]


class Atmosphere(object):
    """Pressure, temperature and gas mole fractions as numpy arrays.

    Accepts a (p, t, vmr) tuple/namedtuple or dict with those keys -- vmr maps a chemical
    formula to an array shaped like t -- or, when xarray is installed, a Dataset read by CF
    standard_name the way pyLBL/atmosphere.py:21-47 does.
    """
    def __init__(self, atmosphere, mapping=None):
        if hasattr(atmosphere, "data_vars"):
            self._from_dataset(atmosphere, mapping)
            return
        if isinstance(atmosphere, dict):
            p, t, vmr = atmosphere["p"], atmosphere["t"], atmosphere["vmr"]
        else:
            p, t, vmr = atmosphere.p, atmosphere.t, atmosphere.vmr
        self.pressure = np.asarray(p, dtype=np.float64)
        self.temperature = np.asarray(t, dtype=np.float64)
        self.gases = {k: np.asarray(v, dtype=np.float64) for k, v in vmr.items()}
        for name, value in self.gases.items():
            if value.shape != self.temperature.shape:
                raise ValueError(f"mole fraction of {name} is not shaped like temperature.")
        self.dims = [f"dim_{i}" for i in range(self.temperature.ndim)]

    def _from_dataset(self, dataset, mapping):
        def find(standard_name):
            for name, var in dataset.data_vars.items():
                if var.attrs.get("standard_name") == standard_name:
                    return var
            raise ValueError(f"standard name {standard_name} not found in dataset.")
        if mapping is None:
            pressure, temperature = find("air_pressure"), find("air_temperature")
            gases = {}
            for var in dataset.data_vars.values():
                name = var.attrs.get("standard_name", "")
                if name.startswith(_STANDARD_NAME_PREFIX) and name.endswith("_in_air"):
                    key = name[len(_STANDARD_NAME_PREFIX):-len("_in_air")]
                    gases[_FORMULAE.get(key, key)] = var
        else:
            pressure, temperature = dataset[mapping["play"]], dataset[mapping["tlay"]]
            gases = {k: dataset[v] for k, v in mapping["mole_fraction"].items()}
        self.pressure = np.asarray(pressure.data, dtype=np.float64)
        self.temperature = np.asarray(temperature.data, dtype=np.float64)
        self.gases = {k: np.asarray(v.data, dtype=np.float64) for k, v in gases.items()}
        self.dims = list(temperature.dims)


class MoleculeCache(object):
    """Caches the per-molecule backend objects (pyLBL/spectroscopy.py:32-69): building them
    uploads the molecule's line table and continuum coefficients to HBM once."""
    def __init__(self, name, lines_database, lines_engine, continua_engine,
                 cross_sections_engine, device):
        # `lines_database` may be the reference's own Database object, whose error classes are
        # not this package's: the conditions are told apart by name (errors.kind).
        try:
            self.gas = lines_engine(lines_database, name, device=device)
        except BaseException as error:
            if errors.kind(error) not in ("AliasNotFoundError", "IsotopologuesNotFoundError",
                                          "TipsDataNotFoundError", "TransitionsNotFoundError"):
                raise
            self.gas = None
        # Water vapour has two continua, every other gas at most one (spectroscopy.py:58-65).
        names = [name + "Foreign", name + "Self"] if name == "H2O" else [name]
        self.gas_continua = None
        if continua_engine is not None:
            try:
                self.gas_continua = [continua_engine[x](device=device) for x in names]
            except KeyError:
                self.gas_continua = None
        self.cross_section = None
        if cross_sections_engine is not None and hasattr(lines_database, "arts_crossfit"):
            try:
                self.cross_section = cross_sections_engine(
                    name, lines_database.arts_crossfit(name), device=device)
            except BaseException as error:
                if errors.kind(error) not in ("AliasNotFoundError", "CrossSectionNotFoundError"):
                    raise
                self.cross_section = None


class Spectroscopy(object):
    """Line-by-line gas optics (lines, MT-CKD continua, ARTS-crossfit cross-sections) on an
    MI355X.

    Attributes mirror pyLBL/spectroscopy.py:72-86.
    """
    def __init__(self, atmosphere, grid, database, mapping=None, lines_backend="mi355x",
                 continua_backend="mt_ckd", cross_sections_backend="arts_crossfit", device=0,
                 group=None, gather_to=0, farfield=True):
        """Args beyond the reference's (pyLBL/spectroscopy.py:88-118):
            device: GPU index of this process.
            farfield: True (default): lines far from a tile of the grid enter through one power
                   series per tile (pylbl_amd/csrc/farfield.h; truncation <= ~1.5e-11 relative,
                   asserted by tests/test_gpu_api.py at 100, 1000 and 2000 points per cm-1;
                   3-4x faster on fine grids).  False: every line at every point of its window,
                   like the reference's loop.
            group: None: this process computes every level.  True (the default process group)
                   or a torch.distributed ProcessGroup: one process per GPU, each computes a
                   contiguous block of levels (all gases and mechanisms of a level on the same
                   GPU, pylbl_amd.distributed.level_shard) and compute_absorption collects the
                   result on rank `gather_to` (None: on every rank); the other ranks get None.
        """
        self.atmosphere = Atmosphere(atmosphere, mapping=mapping)
        # A private copy: the grid's device copy is cached per array object, and the lines
        # path reads (v0, vn, n_per_v) off it on every call -- a caller editing its own array
        # afterwards must not move one mechanism's grid and leave the others behind.
        self.grid = np.array(grid, dtype=np.float64, order="C", copy=True)
        self.lines_database = database
        self.lines_backend = lines_backend
        self.lines_engine = molecular_lines[lines_backend]      # KeyError if unknown
        self.continua_backend = continua_backend
        # None switches the mechanism off; an unknown name is a KeyError (spectroscopy.py:118).
        self.continua_engine = None if continua_backend is None else continua[continua_backend]
        self.cross_sections_backend = cross_sections_backend
        self.cross_sections_engine = None if cross_sections_backend is None \
            else cross_sections[cross_sections_backend]
        self.cache = {}
        self.device = device
        self.group = group
        self.gather_to = gather_to
        self.farfield = bool(farfield)
        self.device_output_limit = 8 << 30     # bytes of spectra kept in HBM per block
        self.delivery_pieces = 4               # runs of tiles of the call that delivers its result
        # "total": in which order the gases add into the one block (absorption.queue_total).
        self.total_order = "heavy_last"
        # "gas": "each" -- every gas's lines call delivers its block piece by piece; "last" -- only
        # the last gas does, the others' blocks travel in one copy each.
        self.gas_delivery = os.environ.get("PYLBL_AMD_GAS_DELIVERY", "each")
        Output = namedtuple("Output", ["dims", "dim_sizes", "mechanisms", "units"])
        dims = list(self.atmosphere.dims) + ["mechanism", "wavenumber"]
        dim_sizes = list(self.atmosphere.temperature.shape) + [len(MECHANISMS), self.grid.size]
        self.output = Output(dims=dims, dim_sizes=dim_sizes, mechanisms=MECHANISMS,
                             units={"units": "m-1"})

    def list_molecules(self):
        return self.lines_database.molecules()

    def _molecule(self, name):
        data = self.cache.get(name)
        if data is None:
            data = MoleculeCache(name, self.lines_database, self.lines_engine,
                                 self.continua_engine, self.cross_sections_engine, self.device)
            self.cache[name] = data
        return data

    def compute_absorption(self, output_format="all", remove_pedestal=None,
                           range_policy="reference"):
        """Computes the absorption coefficient [m-1] on the grid for every level and gas of
        the atmosphere: spectral lines (slot 0), MT-CKD continua (slot 1) and ARTS-crossfit
        cross-sections (slot 2).

        Args:
            output_format: "all" (per gas, per mechanism), "gas" (per gas, mechanisms summed)
                           or anything else for the total over gases (spectroscopy.py:208-235).
            remove_pedestal: Subtract the MT-CKD "pedestal" (default: True when the continuum
                             backend is "mt_ckd", as spectroscopy.py:163-164).

        Returns:
            xarray Dataset when xarray is installed, else a dict of numpy arrays with the
            same variable names ("wavenumber", "mechanism", "<formula>_absorption" /
            "absorption").
        """
        shape = list(self.atmosphere.temperature.shape)
        levels = self.atmosphere.temperature.size
        if remove_pedestal is None:
            remove_pedestal = self.continua_backend == "mt_ckd"
        mode = output_format if output_format in ("all", "gas") else "total"
        columns = self.grid.size
        if self.group is None:
            flat = self._compute_levels(0, levels, mode, remove_pedestal, range_policy)
        else:
            # One process per GPU: this rank's block of levels, then one collection per array.
            from . import distributed
            group = None if self.group is True else self.group
            rank, world, _ = distributed._group_info(group)
            mine = distributed.level_shard(levels, rank, world)
            local = self._compute_levels(mine.start, mine.stop, mode, remove_pedestal,
                                         range_policy)
            flat = {name: distributed.gather_arrays(values, levels, self.gather_to,
                                                    group, device=self.device)
                    for name, values in local.items()}
            if any(values is None for values in flat.values()):
                return None
        tail = [len(MECHANISMS), columns] if mode == "all" else [columns]
        return self._create_output_dataset(
            {name: values.reshape(shape + tail) for name, values in flat.items()}, output_format)

    def compute_path(self, path_length, quantities=PATH_QUANTITIES, band_edges=None,
                     cumulative=None, remove_pedestal=None, range_policy="reference",
                     instrument=None):
        """Optical depth and transmittance along the paths of the atmosphere, formed on the GPU
        from the "total" absorption block without handing that block to the host.

        The path axis is the last dimension of the atmosphere: flat level i = p*L + l.  With
        beta the absorption coefficient [m-1] of compute_absorption("total", remove_pedestal,
        range_policy) and s the path lengths,
            tau_p = sum_l s_{p,l} beta_{p,l}, added as tau = tau + s*beta from l = 0 upward,
            transmittance = exp(-tau) (not clamped).

        Args:
            path_length: [m], shaped like the atmosphere's temperature, finite and >= 0: each
                         level's geometric length along its path (slant paths: times the secant).
            quantities: any of "optical_depth", "transmittance".
            band_edges: None (every grid point) or strictly increasing finite edges e_0 < ... <
                        e_B: band b holds the points e_b <= grid < e_b+1, and the result is the
                        arithmetic mean of tau or of exp(-tau) over them (NaN without points).
            cumulative: None (one result per path), "from_first" (tau over levels 0 .. l) or
                        "from_last" (tau over levels l .. L-1, summed from L-1 down).
            instrument: None, or an Instrument (pylbl_amd.instrument): the channel means of tau
                        or of exp(-tau) under its line shapes (not exp of the mean tau); NaN for
                        a channel without points or not wholly inside the grid.  Not with
                        band_edges.

        Returns:
            Like compute_absorption: an xarray Dataset when xarray is installed, else a dict of
            numpy arrays -- "optical_depth" / "transmittance" with the atmosphere's dims (without
            the last unless cumulative) and "wavenumber", "band" or "channel"; coordinates
            "wavenumber", or "band_lower", "band_upper" and "band_points", or "channel_center",
            "channel_lower", "channel_upper" and "channel_points".
        """
        request = self._path_request(path_length, quantities, band_edges, cumulative,
                                      range_policy, instrument)
        from_last = request.cumulative == "from_last"
        cumulative = request.cumulative is not None

        def sweeper(call, run):
            carry = call.take(call.paths)

            def sweep(index, beta, a, b, outputs):
                call.engine.path_compute(
                    beta, call.columns, call.paths, call.per_path, a, request.lengths[a:b], carry,
                    optical_depth=outputs.get("optical_depth"),
                    transmittance=outputs.get("transmittance"), band_start=request.starts,
                    cumulative=cumulative, from_last=from_last, asynchronous=True)
            return sweep
        if request.instrument is None:
            step, products = _sweep_pass(request.quantities, cumulative, from_last), None
        else:
            # The sweep leaves tau on the grid; both quantities are channel means of it.
            step = _sweep_pass(("optical_depth",), cumulative, from_last)
            products = [_Product(q, "optical_depth", cumulative, q == "transmittance")
                        for q in request.quantities]
        values = self._sweep_runs(request, [step], remove_pedestal, range_policy, sweeper,
                                   products=products)
        return self._create_path_dataset(values, request)

    def compute_radiance(self, path_length, boundary_temperature=None, boundary_emissivity=1.,
                         direction="toward_last", quantities=("radiance",), band_edges=None,
                         cumulative=False, remove_pedestal=None, range_policy="reference",
                         instrument=None, source="isothermal", interface_temperature=None,
                         emissivity_wavenumber=None, reflection_path_length=None):
        """Thermal emission along the paths of the atmosphere: the radiance that leaves each
        path, formed on the GPU from the "total" absorption block like compute_path's optical
        depth.  Every level is an isothermal layer at its own temperature, or with
        source="linear_in_tau" a layer whose source varies linearly in optical depth between
        the Planck values at its two interfaces.

        Paths as in compute_path: the last dimension of the atmosphere, flat level i = p*L + l.
        With beta the absorption coefficient [m-1] of compute_absorption("total",
        remove_pedestal, range_policy), s the path lengths, T_l the level temperatures and nu the
        grid [cm-1], in this order of operations (each product and sum rounded as written):
            B(nu, T) = (((C1*nu)*nu)*nu) / expm1((C2*nu)/T), 0 for nu <= 0,
                       [W m-2 sr-1 (cm-1)-1], C1 = PLANCK_C1, C2 = PLANCK_C2;
            level l, x = s_l*beta_l: t = exp(-x), a = -expm1(-x), source B(nu, T_l);
            I = eps*B(nu, T_boundary) (I = 0 without a boundary), then I = I*t + B_l*a for
            each level in sweep order;
            brightness temperature = (C2*nu) / log1p((((C1*nu)*nu)*nu) / I), 0 where I <= 0 or
            nu <= 0.
        source="linear_in_tau": the level's own temperature still sets beta, but not the
        source.  With T_i the interface temperatures, B_in = B(nu, T) at the interface the
        sweep enters level l through (l toward_last, l + 1 toward_first) and B_out at the one
        it leaves through, the update is
            w = 1 - a/x (x/2 - x^2/6 + ...; 0 at x = 0), u_in = a - w,
            I = I*t + (B_in*u_in + B_out*w),
        with w formed as 1. - a/x for |x| >= 1/16 and below that as the 8-term Horner series
            x*(1./2. - x*(1./6. - x*(1./24. - x*(1./120. - x*(1./720. - x*(1./5040.
              - x*(1./40320. - x*(1./362880.)))))))).
        An optically thick layer then radiates at the temperature of the interface the
        radiation leaves through, a thin one at the mean of the two Planck values.
        For an atmosphere whose paths start at the surface, "toward_last" with the surface as
        the boundary is the upwelling radiance at the top, "toward_first" the downwelling
        radiance at the surface.
        The boundary as a surface.  emissivity_wavenumber gives it a spectral emissivity: with
        knots k_0 < ... < k_{M-1} and the values e_0 .. e_{M-1} of a path, numpy.interp's
            for k_j <= nu < k_{j+1}:  E = e_j + (nu - k_j)*((e_{j+1} - e_j)/(k_{j+1} - k_j)),
            E = e_0 for nu <= k_0,  E = e_{M-1} for nu >= k_{M-1}
        (constant outside the knots, linear inside; each operation rounded as written, so a flat
        table e_j = c gives E = c exactly).  reflection_path_length makes it reflect: a down
        pass first sweeps the radiance against `direction`, from the far end of every path
        toward the boundary, starting from 0, with reflection_path_length as its lengths and the
        call's source model (with "linear_in_tau" the same interface temperatures, entered from
        the other side); what it leaves at the boundary is D.  The up pass is the sweep above,
        except that it starts from
            I = E*B(nu, T_boundary) + (1. - E)*D,
        E the spectral value or the scalar eps.  reflection_path_length = path_length is
        specular reflection in a plane-parallel atmosphere; 1.66 times the layer thickness is
        the diffusivity approximation of a Lambertian surface.  When the absorption of every
        level fits device_output_limit it is computed once and both passes read it; otherwise
        the up pass computes its runs again, save the one the down pass ends on.

        Args:
            path_length: [m], shaped like the atmosphere's temperature, finite and >= 0.
            boundary_temperature: None (no source behind the paths), a scalar or one per path
                         (shaped like the atmosphere without its last dimension) [K], finite and
                         > 0: the source the radiation starts from.
            boundary_emissivity: a scalar or one per path, in [0, 1]; with emissivity_wavenumber
                         [..., M] (the atmosphere's shape without its last axis, then M) or [M]
                         for every path.
            direction: "toward_last" (levels 0 .. L-1: the radiation leaves after level L-1) or
                       "toward_first" (levels L-1 .. 0).
            quantities: any of "radiance", "brightness_temperature".
            band_edges: as in compute_path: the arithmetic mean of the radiance over each band
                        (NaN without points).  Not with "brightness_temperature".
            cumulative: True: one result per level, I just after that level in sweep order.
            instrument: None, or an Instrument (pylbl_amd.instrument): the channel radiances R_c
                        under its line shapes (NaN for a channel without points or not wholly
                        inside the grid); "brightness_temperature" is then that of R_c at the
                        channel centre, (C2*nu_c)/log1p((((C1*nu_c)*nu_c)*nu_c)/R_c), 0 where
                        R_c <= 0.  Not with band_edges.
            source: "isothermal" or "linear_in_tau".
            interface_temperature: [K], the atmosphere's shape with L + 1 in place of L on the
                        last axis, finite and > 0: interface i lies between levels i-1 and i.
                        Needed with "linear_in_tau", refused without it.
            emissivity_wavenumber: None, or [M] knots [cm-1], finite and strictly ascending,
                        2 <= M <= 1024.
            reflection_path_length: None, or [m], shaped like the atmosphere's temperature,
                        finite and >= 0: the lengths of the down pass.  Needs
                        boundary_temperature.  With it "boundary_downwelling_radiance" (D per
                        path, reduced by band_edges / instrument like the radiance; not with
                        cumulative=True) may be among the quantities.

        Returns:
            Like compute_path: an xarray Dataset when xarray is installed, else a dict --
            "radiance" ("W m-2 sr-1 (cm-1)-1") / "brightness_temperature" ("K") with the
            atmosphere's dims (without the last unless cumulative) and "wavenumber", "band" or
            "channel".  With "linear_in_tau" the result carries source = "linear_in_tau" (a
            Dataset attribute, a key of the dict); likewise surface = "reflecting" with
            reflection_path_length and emissivity = "spectral" with emissivity_wavenumber.
        """
        request = self._radiance_request(
            path_length, boundary_temperature, boundary_emissivity, direction, quantities,
            band_edges, cumulative, range_policy, instrument, names=SURFACE_RADIANCE_QUANTITIES,
            source=source, interface_temperature=interface_temperature,
            emissivity_wavenumber=emissivity_wavenumber,
            reflection_path_length=reflection_path_length)
        # Behind a surface that reflects, the down pass (D into the reflection rows) comes first;
        # behind one with a spectral emissivity, the emissivity rows are filled before the up
        # pass.  With neither, the up pass alone is the plain sweep.
        reflecting = request.reflection_lengths is not None
        spectral = request.emissivity_knots is not None
        wanted = DOWNWELLING in request.quantities
        banded = request.starts is not None
        up_quantities = paths._swept_radiance(
            request, tuple(q for q in request.quantities if q != DOWNWELLING))
        down = _Pass(not request.from_last, (), (DOWNWELLING,) if wanted else ())
        up = _sweep_pass(up_quantities, request.cumulative, request.from_last)
        passes = ([down] if reflecting else []) + ([up] if up_quantities else [])

        def sweeper(call, run):
            fills = paths._FilledOnce(call)
            grid = fills.grid
            carry = call.take(call.paths)
            # D on the grid: the returned rows themselves where they are on the grid; else a
            # block of its own, which with bands is the down pass's carry (D stays in it).
            reflection = call.take(call.paths) if reflecting and (banded or not wanted) else None
            # The emissivity rows are filled before the first sweep of the up pass.
            emissivity = fills.surface_rows(request.emissivity_knots, request.boundary_emissivity)

            def sweep(index, beta, a, b, outputs):
                rows = None
                if reflecting:
                    rows = reflection if reflection is not None else outputs[DOWNWELLING]
                if passes[index] is down:
                    means = banded and wanted
                    call.engine.path_radiance(
                        beta, call.columns, grid, call.paths, call.per_path, a,
                        request.reflection_lengths[a:b], call.temperature[a:b],
                        rows if means else carry,
                        radiance=outputs[DOWNWELLING] if means else rows,
                        band_start=request.starts if means else None, cumulative=False,
                        from_last=down.from_last, asynchronous=True, **_run_edges(request, a, b))
                    return
                fills.queue()
                # (a call that uses nothing of the surface passes neither keyword)
                surface = {} if emissivity is None and rows is None else \
                    dict(emissivity_rows=emissivity, reflection=rows)
                call.engine.path_radiance(
                    beta, call.columns, grid, call.paths, call.per_path, a, request.lengths[a:b],
                    call.temperature[a:b], carry,
                    boundary_temperature=request.boundary_temperature,
                    boundary_emissivity=None if spectral else request.boundary_emissivity,
                    radiance=outputs.get("radiance"),
                    brightness_temperature=outputs.get("brightness_temperature"),
                    band_start=request.starts, cumulative=request.cumulative,
                    from_last=request.from_last, asynchronous=True,
                    **surface, **_run_edges(request, a, b))
            return sweep
        products = None
        if request.instrument is not None:
            products = [_Product(q, q, request.cumulative) for q in up_quantities] + \
                ([_Product(DOWNWELLING, DOWNWELLING, False)] if wanted else [])
        values = self._sweep_runs(request, passes, remove_pedestal, range_policy, sweeper,
                                   products=products)
        return self._create_path_dataset(paths._channel_brightness(values, request), request)

    def compute_jacobian(self, path_length, boundary_temperature=None, boundary_emissivity=1.,
                         direction="toward_last",
                         quantities=("radiance", "optical_depth_jacobian",
                                     "temperature_jacobian"),
                         band_edges=None, instrument=None, remove_pedestal=None,
                         range_policy="reference"):
        """Analytic Jacobians (weighting functions) of compute_radiance's radiance: its
        derivatives with respect to the state of every level and of the boundary, formed on the
        GPU in one more sweep over the "total" absorption block of a radiance call.

        Paths, beta, s, T_l, nu, B and the arguments as in compute_radiance.  For one path and
        one grid point, with the levels numbered k = 0 .. L-1 in sweep order (k = 0 is level 0
        for "toward_last" and level L-1 for "toward_first"), each product and sum rounded as
        written:
            x_k = s_k*beta_k, t_k = exp(-x_k), a_k = -expm1(-x_k), B_k = B(nu, T_k);
            forward, exactly compute_radiance's: I_-1 = eps*B(nu, T_b) (0 without a boundary),
            I_k = I_{k-1}*t_k + B_k*a_k; "radiance" is I_{L-1};
            trailing optical depth, summed from the observer backwards: tau'_{L-1} = 0, then
            tau'_{k-1} = tau'_k + s_k*beta_k for k = L-1 .. 0; trail_k = exp(-tau'_k),
            trail_b = exp(-tau'_{-1});
            dB(nu, T): with u = (C2*nu)/T and B = B(nu, T),
            dB = (B*(u/T))*(1. + B/(((C1*nu)*nu)*nu)), 0 for nu <= 0.
        Per level (the atmosphere's dims):
            "optical_depth_jacobian"      dI/dx_k = (B_k - I_k)*trail_k
                                          [radiance per unit optical depth];
            "log_optical_depth_jacobian"  dI/dln x_k = x_k*((B_k - I_k)*trail_k) [radiance]: the
                                          response to a fractional change of the layer's absorber
                                          amount;
            "temperature_jacobian"        dI/dT_k at fixed beta = (a_k*dB(nu, T_k))*trail_k
                                          [radiance K-1].
        Per path (without the last dim; only with boundary_temperature):
            "boundary_temperature_jacobian"  (eps*dB(nu, T_b))*trail_b [radiance K-1];
            "boundary_emissivity_jacobian"   B(nu, T_b)*trail_b [radiance].
        "temperature_jacobian" is the source-function part alone: how beta depends on T and on
        the mixing ratios is the caller's to chain, as s_k*dbeta_k/dq times
        "optical_depth_jacobian".  Jacobians of fluxes and of brightness temperature are not
        formed.

        Args:
            path_length, boundary_temperature, boundary_emissivity, direction, remove_pedestal,
            range_policy: as in compute_radiance.
            quantities: any of "radiance" and the five names above.
            band_edges: as in compute_path: the arithmetic mean of every quantity over each band
                        (the bands' weights do not depend on the state, so the mean of the
                        Jacobian is the Jacobian of the band radiance).
            instrument: None, or an Instrument: the same under its line shapes, dR_c/dq =
                        sum_j w_j dv_j/dq / sum_j w_j.  Not with band_edges.

        Returns:
            Like compute_radiance: an xarray Dataset when xarray is installed, else a dict.
        Raises ValueError where the blocks of one path (beta, the work block and one block per
        per-level quantity) exceed device_output_limit: a run holds whole paths.
        """
        request = self._radiance_request(path_length, boundary_temperature,
                                          boundary_emissivity, direction, quantities, band_edges,
                                          False, range_policy, instrument,
                                          names=JACOBIAN_QUANTITIES, caller="compute_jacobian")
        if request.boundary_temperature is None and any(
                q.startswith("boundary_") for q in request.quantities):
            raise ValueError("the boundary Jacobians need a boundary_temperature.")
        per_level = [q for q in request.quantities if q in JACOBIAN_LEVEL_QUANTITIES]
        step = _Pass(request.from_last, tuple(per_level),
                     tuple(q for q in request.quantities if q in JACOBIAN_PATH_QUANTITIES))
        # With bands the entry keeps every quantity's fine rows in the work block.
        banded = request.starts is not None
        work_blocks = max(len(per_level), 1) if banded else 1

        def sweeper(call, run):
            grid = call.grid()
            run_paths = run//call.per_path
            work = call.take(work_blocks*run +
                             (len(step.path_quantities)*run_paths if banded else 0))

            def sweep(index, beta, a, b, outputs):
                call.engine.path_jacobian(
                    beta, call.columns, grid, call.paths, call.per_path, a, request.lengths[a:b],
                    call.temperature[a:b], work,
                    boundary_temperature=request.boundary_temperature,
                    boundary_emissivity=request.boundary_emissivity, band_start=request.starts,
                    from_last=request.from_last, asynchronous=True,
                    **{q: outputs[q] for q in request.quantities})
            return sweep
        products = None if request.instrument is None else \
            [_Product(q, q, q in JACOBIAN_LEVEL_QUANTITIES) for q in request.quantities]
        values = self._sweep_runs(request, [step], remove_pedestal, range_policy, sweeper,
                                   level_blocks=1 + work_blocks, products=products,
                                   grid_outputs=True, whole_paths=True)
        return self._create_path_dataset(values, request)

    def compute_flux(self, layer_thickness, surface_temperature, surface_emissivity=1.,
                     surface="first", angles=3, quantities=("upward_flux", "downward_flux"),
                     band_edges=None, remove_pedestal=None, range_policy="reference",
                     source="isothermal", interface_temperature=None):
        """Upward and downward longwave fluxes at every layer interface, and heating rates,
        formed on the GPU from the "total" absorption block: the radiance of K angles swept
        down from space and back up from a Lambertian surface, in two passes over the block.

        Paths as in compute_path: the last dimension of the atmosphere, level l of a path an
        isothermal layer at T_l of vertical thickness s_l.  With beta the absorption coefficient
        [m-1] of compute_absorption("total", remove_pedestal, range_policy), nu the grid [cm-1]
        and B(nu, T) as in compute_radiance, each product and sum rounded as written:
            s_{l,k} = s_l/mu_k (fp64), one per level and angle;
            down: I_k = 0 at space, then for each level toward the surface, x = s_{l,k}*beta_l,
                  I_k = I_k*exp(-x) + B(nu, T_l)*(-expm1(-x)) (compute_radiance's update);
            surface: R = sum_k w_k*I_k (from k = 0) of the down sweep's I_k at the surface; the
                  up sweep starts from I_k = eps*B(nu, T_s) + (1 - eps)*R for every k;
            up: the same update, levels from the surface toward space;
            F = pi*(sum_k w_k*I_k) at an interface, from k = 0, pi = numpy.pi: F_down is 0 at
                  space, F_up at the surface comes from the starting I_k;
            band flux F_b = (band mean of F)*(n_b/n_per_v): compute_path's ordered mean times
                  the band's width in grid steps (NaN without points);
            heating rate H_l = 86400*(Fnet[i_lower] - Fnet[i_upper]) / ((rho_l*c_p)*s_l) in fp64
                  from the returned fluxes, Fnet = F_up - F_down, i_lower the interface of level
                  l nearer the surface, rho_l = p_l/(R_DRY*T_l), c_p = CP_DRY; NaN where s_l = 0
                  (see heating_rate).
        source="linear_in_tau" replaces the update of both sweeps by compute_radiance's linear
        one, I_k = I_k*exp(-x) + (B_in*u_in + B_out*w) with B at the interfaces of
        interface_temperature (shared by the angles; w per angle); the surface and the
        heating rates are formed as above.
        When the absorption of every level fits device_output_limit (two blocks of it per level:
        beta and the fluxes of a level) it is computed once and both sweeps read it.  Otherwise
        each pass computes its runs again, save the one the down pass ends on: beyond that limit
        the line cost doubles.

        Args:
            layer_thickness: [m], shaped like the atmosphere's temperature, finite and >= 0.
            surface_temperature: [K], a scalar or one per path, finite and > 0.
            surface_emissivity: a scalar or one per path, in [0, 1].
            surface: "first" (level 0 touches the surface) or "last" (level L-1 does); the other
                     end faces space, from which nothing comes in.
            angles: an int K in 1..8 (Gauss-Legendre on mu in (0, 1], see flux_angles) or a pair
                    (mu, weight) of 1..8 values, 0 < mu <= 1, weights >= 0 summing to 1 (the
                    diffusivity approximation is ([1/1.66], [1.])).
            quantities: any of "upward_flux", "downward_flux", "heating_rate" (net flux is
                        up - down).
            band_edges: as in compute_path.
            source, interface_temperature: as in compute_radiance; interface i is index i of
                        the result's "interface" dim.

        Returns:
            Like compute_path: an xarray Dataset when xarray is installed, else a dict -- the
            fluxes with the atmosphere's dims, the last replaced by "interface" (L + 1: interface
            i lies between levels i-1 and i), then "wavenumber" ("W m-2 (cm-1)-1") or "band"
            ("W m-2"); "heating_rate" with the level dim ("K day-1 (cm-1)-1" / "K day-1").
        """
        request = self._flux_request(layer_thickness, surface_temperature,
                                      surface_emissivity, surface, angles, quantities, band_edges,
                                      range_policy, source=source,
                                      interface_temperature=interface_temperature)
        angles = request.mu.size
        lengths = request.lengths[:, None]/request.mu[None, :]
        bands = request.starts is not None
        # Down from space, then up from the surface: "first" has its surface at level 0.
        passes = [_Pass(request.surface == "first", ("downward_flux",), ()),
                  _Pass(request.surface == "last", ("upward_flux",), ("surface_flux",))]

        def sweeper(call, run):
            grid = call.grid()
            carry = call.take(call.paths*angles)
            # The fluxes of a run's levels (with bands: before their means) and R, then the flux
            # at the surface: without bands those are the outputs themselves.
            level = call.take(run) if bands else None
            reflection = call.take(call.paths) if bands else None

            def sweep(index, beta, a, b, outputs):
                up = index == 1
                out = outputs["upward_flux" if up else "downward_flux"]
                call.engine.path_flux(
                    beta, call.columns, grid, call.paths, call.per_path, a, lengths[a:b],
                    request.weight, call.temperature[a:b], carry,
                    reflection if bands else outputs["surface_flux"],
                    (level if b - a == run else level.rows(b - a)) if bands else out,
                    surface_temperature=request.surface_temperature,
                    surface_emissivity=request.surface_emissivity,
                    flux=out if bands else None,
                    surface_flux=outputs["surface_flux"] if bands and up else None,
                    band_start=request.starts, up=up, from_last=passes[index].from_last,
                    asynchronous=True, **_run_edges(request, a, b))
            return sweep
        # Two blocks per level: beta and the fluxes of a level.
        values = self._sweep_runs(request, passes, remove_pedestal, range_policy, sweeper,
                                   level_blocks=2)
        return self._create_flux_dataset(self._flux_interfaces(values, request), request)

    def compute_solar(self, layer_thickness, solar_zenith_cosine, solar_irradiance=None,
                      solar_wavenumber=None, distance_factor=1., solar_path_length=None,
                      surface="first", surface_albedo=None, albedo_wavenumber=None,
                      view_path_length=None, quantities=("direct_irradiance",), band_edges=None,
                      instrument=None, remove_pedestal=None, range_policy="reference"):
        """Sunlight in an atmosphere that does not scatter: the direct solar beam at every layer
        interface, the heating by its absorption and the sunlight a Lambertian surface reflects
        to a viewer, formed on the GPU in one sweep over the "total" absorption block.  Thermal
        and solar radiation superpose without scattering: add compute_radiance's result where
        both matter.

        Paths, levels, `surface` and layer_thickness as in compute_flux: the Sun shines in from
        the end that faces space, and interface i lies between levels i-1 and i.  With beta the
        absorption coefficient [m-1] of compute_absorption("total", remove_pedestal,
        range_policy), nu the grid [cm-1], a_l the solar slant length and v_l the view length of
        level l, per path and grid point, each product and sum rounded as written:
            S(nu) = d*S_table(nu) [W m-2 (cm-1)-1], d = distance_factor; without a table
                  S = (SOLAR_SOLID_ANGLE*d)*B(nu, SOLAR_TEMPERATURE), B as in compute_radiance
                  (0 for nu <= 0); a table with knots k_0 < ... < k_{M-1} and values e_j is
                  interpolated like compute_radiance's emissivity,
                  for k_j <= nu < k_{j+1}:  E = e_j + (nu - k_j)*((e_{j+1} - e_j)/(k_{j+1} - k_j)),
                  E = e_0 for nu <= k_0,  E = e_{M-1} for nu >= k_{M-1};
            F0 = mu0*S;  tau = 0, tv = 0;  F at the interface that faces space = F0;
            for each level in order from space to the surface:
                tau = tau + a_l*beta_l;  tv = tv + v_l*beta_l;
                F at the interface below the level = F0*exp(-tau);
            reflected radiance = ((A*F0)/pi)*exp(-(tau + tv)), pi = numpy.pi, tau and tv at
                  the surface.
        Both optical depths are added in the Sun's order, from space to the surface (also the
        viewer's, whose light travels the other way): one read of beta serves both beams, and
        this order is the definition.
            band irradiance F_b = (band mean of F)*(n_b/n_per_v) as in compute_flux; band
                  radiances are means, as in compute_radiance (NaN without points);
            heating rate: paths.heating_rate of the returned irradiance as the downward flux and
                  an upward flux of zero: the absorption of the direct beam alone.  The
                  absorption of the reflected light is not included.

        Args:
            layer_thickness: [m], shaped like the atmosphere's temperature, finite and >= 0.
            solar_zenith_cosine: mu0, a scalar or one per path, in (0, 1].
            solar_irradiance: None (the blackbody above), [V] values on the grid as they are, or
                         with solar_wavenumber [M]: S at 1 au and normal incidence
                         [W m-2 (cm-1)-1], finite and >= 0.
            solar_wavenumber: None, or [M] knots [cm-1], finite and strictly ascending,
                         2 <= M <= 2**22.
            distance_factor: d, finite and > 0: (1 au / distance)**2.
            solar_path_length: None (layer_thickness/mu0, formed in fp64 on the host), or [m]
                         shaped like the atmosphere's temperature, finite and >= 0: the slant
                         lengths of the beam, e.g. spherical or refracted ones at low Sun.
            surface: "first" (level 0 touches the surface) or "last".
            surface_albedo: the Lambertian albedo A in [0, 1]: a scalar or one per path; with
                         albedo_wavenumber [..., M] or [M], 2 <= M <= 1024.
            albedo_wavenumber: None, or [M] knots [cm-1] as compute_radiance's
                         emissivity_wavenumber.
            view_path_length: [m], shaped like the atmosphere's temperature, finite and >= 0:
                         the lengths of the path from the surface to the viewer.
                         "reflected_radiance" needs it and surface_albedo; without that quantity
                         both are refused.
            quantities: any of "direct_irradiance" (at every interface), "surface_irradiance"
                         (per path: the bits of the surface interface), "reflected_radiance" (per
                         path) and "heating_rate" (per level).
            band_edges: as in compute_flux.
            instrument: None, or an Instrument: channel values of the quantities per path
                         ("surface_irradiance", "reflected_radiance") as compute_radiance's
                         radiance.  Not with band_edges or the other quantities.

        Returns:
            Like compute_flux: an xarray Dataset when xarray is installed, else a dict --
            "direct_irradiance" with the atmosphere's dims, the last replaced by "interface"
            (L + 1), then "wavenumber" ("W m-2 (cm-1)-1") or "band" ("W m-2");
            "surface_irradiance" (the same units) and "reflected_radiance"
            ("W m-2 sr-1 (cm-1)-1") without the last dim; "heating_rate" with the level dim
            ("K day-1 (cm-1)-1" / "K day-1").
        """
        request = self._solar_request(layer_thickness, solar_zenith_cosine, solar_irradiance,
                                       solar_wavenumber, distance_factor, solar_path_length,
                                       surface, surface_albedo, albedo_wavenumber,
                                       view_path_length, quantities, band_edges, instrument,
                                       range_policy)
        bands = request.starts is not None
        levels = "direct_irradiance" in request.quantities or "heating_rate" in request.quantities
        # From space to the surface: "first" has its surface at level 0.
        step = _Pass(request.surface == "first", ("direct_irradiance",) if levels else (),
                     ((paths._SPACE,) if levels else ()) +
                     tuple(q for q in request.quantities if q in paths.SOLAR_PATH_QUANTITIES))
        rows = {"direct_irradiance": "interface", paths._SPACE: "space",
                "surface_irradiance": "surface", "reflected_radiance": "reflected"}

        def sweeper(call, run):
            fills = paths._FilledOnce(call)
            carry = call.take(2*call.paths)
            solar = fills.solar_row(request)
            albedo_rows = fills.surface_rows(request.albedo_knots, request.albedo)
            fine = paths._Rows(call, step, run, bands)

            def sweep(index, beta, a, b, outputs):
                fills.queue()
                call.engine.path_solar(
                    beta, call.columns, call.paths, call.per_path, a,
                    request.solar_lengths[a:b], request.mu0, solar, carry,
                    view_lengths=None if request.view_lengths is None
                    else request.view_lengths[a:b],
                    albedo=None if albedo_rows is not None else request.albedo,
                    albedo_rows=albedo_rows, band_start=request.starts,
                    from_last=step.from_last, asynchronous=True,
                    **fine.keywords(rows, outputs, b - a))
            return sweep
        products = None if request.instrument is None else \
            [_Product(q, q, False) for q in request.quantities]
        # Two blocks per level, as compute_flux counts them: beta and the interface rows.
        values = self._sweep_runs(request, [step], remove_pedestal, range_policy, sweeper,
                                   level_blocks=2, products=products)
        return self._create_solar_dataset(self._solar_interfaces(values, request), request)

    def compute_solar_flux(self, layer_thickness, solar_zenith_cosine, solar_irradiance=None,
                           solar_wavenumber=None, distance_factor=1., surface="first",
                           surface_albedo=0., albedo_wavenumber=None, rayleigh=True,
                           rayleigh_cross_section=None, scatterer_optical_depth=None,
                           scatterer_single_scattering_albedo=None, scatterer_asymmetry=None,
                           quantities=("upward_flux", "downward_flux"), band_edges=None,
                           remove_pedestal=None, range_policy="reference"):
        """Shortwave fluxes in an atmosphere that absorbs and scatters: upward and downward
        fluxes at every layer interface, their direct and diffuse parts and heating rates, from
        a two-stream solution of every layer (delta-scaled PIFM) and the adding method, formed
        on the GPU in two sweeps over the "total" absorption block.  Rayleigh scattering by air
        and one grey scatterer per level (a cloud or aerosol layer) are included; the geometry
        is plane-parallel (there is no solar_path_length), thermal emission is not included.

        Paths, levels, `surface`, layer_thickness and the Sun S(nu) as in compute_solar.  With
        beta the absorption coefficient [m-1] of compute_absorption("total", remove_pedestal,
        range_policy) and nu the grid [cm-1], per level l, path and grid point, each product, sum
        and quotient rounded as written:
            tau_a = s_l*beta ;  tau_R = c_l*sigma(nu) ;  tau = (tau_a + tau_R) + tau_c
                  s_l = layer_thickness [m]; c_l = (p_l/(K_B*T_l))*s_l [m-2] in fp64 on the host,
                  K_B = 1.380649e-23, 0 with rayleigh=False; tau_c the scatterer's extinction
                  optical depth of the level (0 without);
            tau_s = tau_R + w_c ;  omega = tau_s/tau ;  g = h_c/tau_s  (g = 0 where tau_s == 0)
                  w_c = omega_c*tau_c and h_c = (omega_c*tau_c)*g_c, formed on the host;
            tau == 0: the layer is the identity (Rdif = Rdir = Tdp = 0, Tdif = D = 1).
        sigma(nu) [m2] is Bucholtz (1995) with lambda = 1e4/nu in um,
            sigma = 1e-4*A*lambda^-(B + C*lambda + D/lambda), formed as
            (1e-4*A)*exp(-(e*log(lambda))), e = (B + C*lambda) + D/lambda;
            lambda <= 0.5: A = 3.01577e-28, B = 3.55212, C = 1.35579, D = 0.11563;
            lambda > 0.5: A = 4.01061e-28, B = 3.99668, C = 1.10298e-3, D = 2.71393e-2;
            used as they are outside 0.2 .. 4 um; 0 for nu <= 0 (paths.rayleigh_cross_section).
        Delta scaling and PIFM coefficients (Zdunkowski, as in RRTMG_SW):
            f = g*g ; sc = 1 - omega*f ; t = sc*tau ; w = ((1 - f)*omega)/sc ; gp = g/(1 + g)
            g2 = (3*(w*(1 - gp)))/4 ; dif = 2*(1 - w) ; g1 = g2 + dif ; su = g1 + g2
            g3 = (2 - 3*(mu0*gp))/4 ; g4 = 1 - g3 ; k2 = dif*su ; D = exp(-t/mu0)
        Conservative branch, where k2*(1 + t*t) <= 1e-10:
            x = g1*t ; Rdif = x/(1 + x) ; Tdif = 1/(1 + x)
            Rdir = (x + (g3 - g1*mu0)*(-expm1(-t/mu0)))/(1 + x) ; Tdp = (1 - Rdir) - D
        General branch (Meador and Weaver 1980, scaled by exp(-k t) so that nothing overflows):
            k = sqrt(k2) ; m = mu0 ; x = k*m
            if |1 - x| < 1e-4: m = (x >= 1 ? (1 + 1e-4) : (1 - 1e-4))/k ; x = k*m
            Dm = exp(-t/m) ; E = exp(-(k*t)) ; E2 = E*E ; o1 = -expm1(-(2*(k*t)))
            den = k*(1 + E2) + g1*o1 ; q = ((1 - x)*(1 + x))*den
            Rdif = (g2*o1)/den ; Tdif = (2*(k*E))/den
            a1 = g1*g4 + g2*g3 ; a2 = g1*g3 + g2*g4
            Rdir = w*((1 - x)*(a2 + k*g3) - ((1 + x)*(a2 - k*g3))*E2 - (2*(k*(g3 - a2*m)))*(E*Dm))/q
            Ttot = Dm*(1 - w*((1 + x)*(a1 + k*g4) - ((1 - x)*(a1 - k*g4))*E2)/q) + w*((2*(k*(g4 + a1*m)))*E)/q
            Tdp = Ttot - Dm
        Adding: interface 0 faces space, level i lies between interfaces i and i + 1 in the Sun's
        order, A is the Lambertian albedo and F0 = mu0*S(nu):
            up, from the surface:  Rup[L] = Rupd[L] = A ;  for i = L-1 .. 0:
                m1 = 1/(1 - Rdif_i*Rupd[i+1])
                Rup[i] = Rdir_i + Tdif_i*((Tdp_i*Rupd[i+1] + D_i*Rup[i+1])*m1)
                Rupd[i] = Rdif_i + Tdif_i*((Tdif_i*Rupd[i+1])*m1)
            down, from space:  Tb = 1, Td = 0, Rd = 0 ;  at every interface i = 0 .. L:
                m2 = 1/(1 - Rd*Rupd[i])
                direct[i] = F0*Tb ; diffuse_down[i] = F0*((Td + (Tb*Rup[i])*Rd)*m2)
                up[i] = F0*((Tb*Rup[i] + Td*Rupd[i])*m2)
                then through level i:  m3 = 1/(1 - Rd*Rdif_i)
                Td = Tb*Tdp_i + Tdif_i*((Td + (Tb*Rd)*Rdir_i)*m3)
                Rd = Rdif_i + Tdif_i*((Tdif_i*Rd)*m3) ; Tb = Tb*D_i
            downward_flux = direct + diffuse_down
        Against the two-stream equations themselves the layer is exact to rounding, except: the
        conservative branch neglects up to its criterion (measured 4.8e-11 of F0 per layer); and
        inside the guard |1 - k*mu0| < 1e-4 the layer is solved at the moved mu0, which puts Rdir
        and Tdp off by up to 0.12*(1e-4 - |1 - k*mu0|) of F0 (measured, g_c <= 0.9): 1.2e-5 of F0
        at k*mu0 = 1 under mu0 = 1, falling linearly to 0 at the guard's edges.
        Band fluxes F_b = (band mean of F)*(n_b/n_per_v) and the heating rate, paths.heating_rate
        of the returned upward and downward fluxes, as in compute_flux.
        With g > 0 the direct irradiance is the delta-scaled beam: it contains the forward peak
        of the scattered light, so it differs from compute_solar's.
        A scatterer whose optics vary with wavenumber: compute_solar_flux_spectral.

        Args:
            layer_thickness, solar_zenith_cosine, solar_irradiance, solar_wavenumber,
            distance_factor, surface, band_edges: as in compute_solar.
            surface_albedo: the Lambertian albedo A in [0, 1]: a scalar or one per path; with
                         albedo_wavenumber [..., M] or [M], as in compute_solar.
            rayleigh: True (needs finite pressures > 0 and temperatures > 0) or False.
            rayleigh_cross_section: None (the fit above), or [V] values [m2] on the grid, finite
                         and >= 0, in its place.
            scatterer_optical_depth, scatterer_single_scattering_albedo, scatterer_asymmetry:
                         tau_c >= 0, omega_c in [0, 1] and g_c in [0, 1), shaped like the
                         atmosphere's temperature, finite; together or not at all.
            quantities: any of "upward_flux", "downward_flux", "direct_irradiance",
                         "diffuse_downward_flux" (at every interface) and "heating_rate".

        Returns:
            Like compute_flux: the fluxes on the "interface" dim (L + 1: interface i of the
            result lies between levels i-1 and i), then "wavenumber" ("W m-2 (cm-1)-1") or "band"
            ("W m-2"); "heating_rate" with the level dim ("K day-1 (cm-1)-1" / "K day-1").
        Raises ValueError where the blocks of one path (beta, two work blocks and one block per
        interface quantity) exceed device_output_limit: a run holds whole paths.
        """
        request = two_stream._solar_flux_request(
            self, layer_thickness, solar_zenith_cosine, solar_irradiance, solar_wavenumber,
            distance_factor, surface, surface_albedo, albedo_wavenumber, rayleigh,
            rayleigh_cross_section, scatterer_optical_depth, scatterer_single_scattering_albedo,
            scatterer_asymmetry, quantities, band_edges, range_policy)
        return two_stream.solar_flux(self, request, remove_pedestal, range_policy)

    def compute_solar_flux_spectral(self, layer_thickness, solar_zenith_cosine,
                                    scatterer_wavenumber, scatterer_optical_depth,
                                    scatterer_single_scattering_albedo, scatterer_asymmetry,
                                    solar_irradiance=None, solar_wavenumber=None,
                                    distance_factor=1., surface="first", surface_albedo=0.,
                                    albedo_wavenumber=None, rayleigh=True,
                                    rayleigh_cross_section=None,
                                    quantities=("upward_flux", "downward_flux"),
                                    band_edges=None, remove_pedestal=None,
                                    range_policy="reference"):
        """compute_solar_flux with cloud and aerosol optics that vary with wavenumber: no real
        cloud or aerosol is grey (liquid water goes from omega = 0.999999 in the visible to 0.5 at
        3 um, aerosol extinction falls roughly as nu^1.3).  The scatterer of every level is a
        table over wavenumber, as the surface's albedo_wavenumber is: k_0 < ... < k_{M-1} [cm-1]
        with tau_c, omega_c and g_c of the level at every knot.  At grid point nu (the optics are
        constant outside the knots), each operation rounded as written:
            j = the largest index with k_j <= nu, limited to 0 .. M-2
            u = (nu - k_j)/(k_{j+1} - k_j), limited to [0, 1]
            for each of e in {tau_c, omega_c, g_c} of the level:
              v = e_j + u*(e_{j+1} - e_j), then limited to [min(e_j, e_{j+1}), max(e_j, e_{j+1})]
        (the limit keeps tau_c >= 0, 0 <= omega_c <= 1 and 0 <= g_c < 1 whatever the rounding
        does), and w_c = omega_c*tau_c, h_c = w_c*g_c are formed per grid point on the GPU; the
        layer and the adding are compute_solar_flux's, line by line.  A table that is flat in nu
        gives compute_solar_flux's fluxes for the grey scatterer bit for bit.

        Args:
            scatterer_wavenumber: [M] knots [cm-1], finite and strictly ascending,
                         2 <= M <= 1024.
            scatterer_optical_depth, scatterer_single_scattering_albedo, scatterer_asymmetry:
                         tau_c >= 0, omega_c in [0, 1] and g_c in [0, 1), finite, shaped like the
                         atmosphere's temperature with one more axis of M at the end.
            Everything else as in compute_solar_flux.

        Returns:
            Like compute_solar_flux, with the attribute (the key) "scatterer": "spectral".
        Raises ValueError like compute_solar_flux, all of them before the GPU is touched; the
        knot table (24 bytes per level and knot) counts against device_output_limit.
        """
        request = two_stream._solar_flux_request(
            self, layer_thickness, solar_zenith_cosine, solar_irradiance, solar_wavenumber,
            distance_factor, surface, surface_albedo, albedo_wavenumber, rayleigh,
            rayleigh_cross_section, scatterer_optical_depth, scatterer_single_scattering_albedo,
            scatterer_asymmetry, quantities, band_edges, range_policy,
            scatterer_wavenumber=two_stream._given_knots(scatterer_wavenumber),
            caller="compute_solar_flux_spectral")
        return two_stream.solar_flux(self, request, remove_pedestal, range_policy)

    def compute_thermal_flux(self, layer_thickness, surface_temperature, surface_emissivity=1.,
                             emissivity_wavenumber=None, surface="first", diffusivity=1.66,
                             scatterer_optical_depth=None,
                             scatterer_single_scattering_albedo=None, scatterer_asymmetry=None,
                             quantities=("upward_flux", "downward_flux"), band_edges=None,
                             remove_pedestal=None, range_policy="reference"):
        """Longwave fluxes in an atmosphere that absorbs, emits and holds a cloud: upward and
        downward fluxes at every layer interface and heating rates, from a two-stream solution
        of every layer with a thermal source (delta-scaled, one grey scatterer per level: a cloud
        or aerosol layer) and the adding method, formed on the GPU in two sweeps over the "total"
        absorption block.  The longwave counterpart of compute_solar_flux; without scatterers it
        is compute_flux with the one angle mu = 1/D.  Levels are isothermal (there is no
        source="linear_in_tau": that is compute_thermal_flux_linear); sunlight is not included.

        Paths, levels, `surface` and layer_thickness as in compute_flux.  With beta the absorption
        coefficient [m-1] of compute_absorption("total", remove_pedestal, range_policy), nu the
        grid [cm-1], D the diffusivity factor and piB(T) = pi*B(nu, T) (pi = numpy.pi, B as in
        compute_radiance, 0 for nu <= 0), per level l with the row (s_l, tau_c, w_c, g_c, T_l) --
        s_l = layer_thickness [m], tau_c the scatterer's extinction optical depth, w_c =
        omega_c*tau_c formed on the host, g_c its asymmetry, T_l the level temperature -- per path
        and grid point, each product, sum and quotient rounded as written:
            tau_a = s_l*beta ; tau = tau_a + tau_c
            clear level (w_c == 0, the same for the whole wavefront):
              x = D*tau ; R = 0 ; T = exp(-x) ; em = -expm1(-x)
            cloudy level (w_c > 0; f = g_c*g_c and gp = g_c/(1 + g_c) are level scalars):
              omega = w_c/tau ; sc = 1 - omega*f ; t = sc*tau ; w = ((1 - f)*omega)/sc
              g2 = (D*(w*(1 - gp)))/2 ; dif = D*(1 - w) ; g1 = g2 + dif ; su = g1 + g2 ; k2 = dif*su
              conservative, where k2*(1 + t*t) <= 1e-10:
                x = g1*t ; R = x/(1 + x) ; T = 1/(1 + x) ; em = (dif*t)/(1 + x)
              general:
                k = sqrt(k2) ; E = exp(-(k*t)) ; E2 = E*E ; o1 = -expm1(-(2*(k*t)))
                den = k*(1 + E2) + g1*o1 ; R = (g2*o1)/den ; T = (2*(k*E))/den
                em = (k*((1 - E)*(1 - E)) + dif*o1)/den     (= 1 - R - T, without the cancellation)
            S = piB(T_l)*em        the layer's own emission, the same upward and downward
        This is the two-stream system with gamma1 = D(1 - omega(1 + g)/2) and gamma2 =
        D*omega(1 - g)/2 after compute_solar_flux's delta scaling; gamma1 - gamma2 = D(1 - omega),
        so F = piB solves an isothermal layer and the layer emits piB*(1 - R - T).
        Adding: interface 0 faces space, level i lies between interfaces i and i + 1 in the order
        space -> surface, eps is the surface emissivity and T_s its temperature:
            up, from the surface:  Rs[L] = 1 - eps ; U[L] = eps*piB(T_s) ;  for i = L-1 .. 0:
              m1 = 1/(1 - R_i*Rs[i+1])
              U[i] = S_i + T_i*((U[i+1] + Rs[i+1]*S_i)*m1)
              Rs[i] = R_i + T_i*((T_i*Rs[i+1])*m1)
            down, from space:  Dn = 0, Rd = 0 ;  at every interface i = 0 .. L:
              m2 = 1/(1 - Rd*Rs[i])
              down[i] = (Dn + Rd*U[i])*m2 ; up[i] = (U[i] + Rs[i]*Dn)*m2
              then through level i:  m3 = 1/(1 - Rd*R_i)
              Dn = S_i + T_i*((Dn + Rd*S_i)*m3) ; Rd = R_i + T_i*((T_i*Rd)*m3)
        Band fluxes F_b = (band mean of F)*(n_b/n_per_v) and the heating rate, paths.heating_rate
        of the returned upward and downward fluxes, as in compute_flux.
        A scatterer whose optics vary with wavenumber: compute_thermal_flux_spectral.

        Args:
            layer_thickness, surface_temperature, surface, band_edges: as in compute_flux.
            surface_emissivity: eps in [0, 1]: a scalar or one per path; with
                         emissivity_wavenumber [..., M] or [M], interpolated onto the grid as
                         compute_radiance's boundary_emissivity.
            emissivity_wavenumber: None, or [M] knots [cm-1], finite and strictly ascending,
                         2 <= M <= 1024.
            diffusivity: D, one number in [1, 2]: 1.66, or 2 for the hemispheric mean of Toon
                         et al. (1989).
            scatterer_optical_depth, scatterer_single_scattering_albedo, scatterer_asymmetry:
                         as in compute_solar_flux.
            quantities: any of "upward_flux", "downward_flux" (at every interface) and
                         "heating_rate".

        Returns:
            Like compute_solar_flux: the fluxes on the "interface" dim (L + 1: interface i of the
            result lies between levels i-1 and i), then "wavenumber" ("W m-2 (cm-1)-1") or "band"
            ("W m-2"); "heating_rate" with the level dim ("K day-1 (cm-1)-1" / "K day-1").
        Raises ValueError where the blocks of one path (beta, two work blocks and one block per
        flux) exceed device_output_limit: a run holds whole paths.
        """
        request = two_stream._thermal_flux_request(
            self, layer_thickness, surface_temperature, surface_emissivity,
            emissivity_wavenumber, surface, diffusivity, scatterer_optical_depth,
            scatterer_single_scattering_albedo, scatterer_asymmetry, quantities, band_edges,
            range_policy)
        return two_stream.thermal_flux(self, request, remove_pedestal, range_policy)

    def compute_thermal_flux_linear(self, layer_thickness, surface_temperature,
                                    interface_temperature, surface_emissivity=1.,
                                    emissivity_wavenumber=None, surface="first",
                                    diffusivity=1.66, scatterer_optical_depth=None,
                                    scatterer_single_scattering_albedo=None,
                                    scatterer_asymmetry=None,
                                    quantities=("upward_flux", "downward_flux"),
                                    band_edges=None, remove_pedestal=None,
                                    range_policy="reference"):
        """compute_thermal_flux with a source that is linear in optical depth: within every
        level the Planck function runs linearly in the layer's optical depth between its values
        at the level's two interfaces, as compute_flux(source="linear_in_tau") has it for the
        clear sky (line-by-line benchmark work; RRTMGP's lw_source_2str), so that cloudy and
        clear fluxes -- a cloud radiative effect -- share one source treatment.  The isothermal
        layer's error goes as the Planck difference across the layer and does not shrink with
        spectral resolution.

        Everything up to em is compute_thermal_flux's, bit for bit; the level temperature enters
        beta only.  Per level and grid point, Bt = piB(T at the level's space-side interface),
        Bb = piB(T at its surface-side interface) and dB = Bb - Bt, each product, sum and
        quotient rounded as written:
            S_up = Bt*em + dB*q        what the layer sends out of its space-side face
            S_dn = Bb*em - dB*q        what it sends out of its surface-side face
        q = (1 - T + R)/(su*t) - T comes from the particular solution F+- = pi*(B(tau) +- B'/su)
        and is formed without the difference, which cancels in thin layers:
            clear level (w_c == 0):
              q = a - linear_weight(x, a)
                (a = em; linear_weight is compute_radiance's w = 1 - a/x in its two-branch form)
            cloudy, general:  y = k*t ; z = y*y
              p = o1 - 2*(y*E)        for y >= 1/2, and for y < 1/2
              p = E*(((y*z)/3)*(1 + z*(1/20 + z*(1/840 + z*(1/60480 + z*(1/6652800
                  + z*(1/1037836800 + z*(1/217945728000 + z*(1/59281238016000)))))))))
              q = ((k*(o1*o1))/(su*((1 + E)*(1 + E))) + p)/(den*t)
            cloudy, conservative:
              q = ((dif*t)*(1 + (su*t)/3))/(2*(1 + x))
        Adding is compute_thermal_flux's with the two sources told apart:
            U[i] = S_up_i + T_i*((U[i+1] + Rs[i+1]*S_dn_i)*m1)
            Dn = S_dn_i + T_i*((Dn + Rd*S_up_i)*m3)
        and Rs, Rd, m1, m2, m3, the interface lines and the surface unchanged.  With dB = 0 both
        sources are Bt*em: where all interface and level temperatures of a path are equal the
        fluxes are compute_thermal_flux's bit for bit.

        Args:
            interface_temperature: the atmosphere's shape with L + 1 along the last axis, finite
                         and > 0 [K]; interface i lies between levels i-1 and i, as in
                         compute_flux.  surface_temperature stays apart from the interface
                         temperature at the surface: a skin-temperature jump is allowed.
            Everything else as in compute_thermal_flux.

        Returns:
            Like compute_thermal_flux, with the attribute (the key) "source": "linear_in_tau".
        Raises ValueError like compute_thermal_flux, all of them before the GPU is touched.
        """
        request = two_stream._thermal_flux_linear_request(
            self, layer_thickness, surface_temperature, interface_temperature,
            surface_emissivity, emissivity_wavenumber, surface, diffusivity,
            scatterer_optical_depth, scatterer_single_scattering_albedo, scatterer_asymmetry,
            quantities, band_edges, range_policy)
        return two_stream.thermal_flux(self, request, remove_pedestal, range_policy)

    def compute_thermal_flux_spectral(self, layer_thickness, surface_temperature,
                                      scatterer_wavenumber, scatterer_optical_depth,
                                      scatterer_single_scattering_albedo, scatterer_asymmetry,
                                      interface_temperature=None, surface_emissivity=1.,
                                      emissivity_wavenumber=None, surface="first",
                                      diffusivity=1.66,
                                      quantities=("upward_flux", "downward_flux"),
                                      band_edges=None, remove_pedestal=None,
                                      range_policy="reference"):
        """compute_thermal_flux -- with interface_temperature compute_thermal_flux_linear -- with
        cloud and aerosol optics that vary with wavenumber.  The scatterer of every level is a
        table over the knots scatterer_wavenumber, interpolated and limited per grid point as in
        compute_solar_flux_spectral; w_c = omega_c*tau_c, f = g_c*g_c and gp = g_c/(1 + g_c) are
        then formed per grid point on the GPU, and the layer and the adding are those of the grey
        call, line by line.  A level whose knots all have omega_c*tau_c == 0 (no scatterer, or one
        that only absorbs) is a clear level, with tau = tau_a + tau_c(nu); in any other level
        every grid point takes the cloudy branches, but where tau == 0 (which a grey cloudy level
        cannot have, and where omega = w_c/tau would be 0/0) the clear one: x = 0, the identity.
        A table that is flat in nu gives the grey call's fluxes bit for bit.

        Args:
            scatterer_wavenumber, scatterer_optical_depth, scatterer_single_scattering_albedo,
            scatterer_asymmetry: as in compute_solar_flux_spectral.
            interface_temperature: None (isothermal levels, compute_thermal_flux's source) or
                         compute_thermal_flux_linear's interface temperatures.
            Everything else as in compute_thermal_flux.

        Returns:
            Like compute_thermal_flux or compute_thermal_flux_linear, with the attribute (the
            key) "scatterer": "spectral".
        Raises ValueError like them, all of them before the GPU is touched.
        """
        arguments = (surface_emissivity, emissivity_wavenumber, surface, diffusivity,
                     scatterer_optical_depth, scatterer_single_scattering_albedo,
                     scatterer_asymmetry, quantities, band_edges, range_policy)
        knots = two_stream._given_knots(scatterer_wavenumber)
        if interface_temperature is None:
            request = two_stream._thermal_flux_request(
                self, layer_thickness, surface_temperature, *arguments,
                scatterer_wavenumber=knots, caller="compute_thermal_flux_spectral")
        else:
            request = two_stream._thermal_flux_linear_request(
                self, layer_thickness, surface_temperature, interface_temperature, *arguments,
                scatterer_wavenumber=knots, caller="compute_thermal_flux_spectral")
        return two_stream.thermal_flux(self, request, remove_pedestal, range_policy)

    def compute_thermal_radiance(self, layer_thickness, surface_temperature,
                                 view_zenith_cosine=1., surface_emissivity=1.,
                                 emissivity_wavenumber=None, surface="first", diffusivity=1.66,
                                 scatterer_optical_depth=None,
                                 scatterer_single_scattering_albedo=None,
                                 scatterer_asymmetry=None, quantities=("radiance",),
                                 band_edges=None, instrument=None, remove_pedestal=None,
                                 range_policy="reference"):
        """Sounder radiances through clouds: the radiance a viewer above the atmosphere sees
        along the zenith cosine mu of each path, in an atmosphere that absorbs, emits and holds
        one grey scatterer per level, by the two-stream source-function technique (Toon et al.
        1989): compute_thermal_flux's two-stream fluxes are the scattering source and the
        transfer equation is integrated exactly along the viewing direction, on the GPU, in one
        more sweep behind the two of compute_thermal_flux.  The all-sky counterpart of
        compute_radiance: without scatterers, with eps = 1 and mu = 1 it returns
        compute_radiance(layer_thickness, boundary_temperature=surface_temperature) bit for bit.

        Paths, levels, `surface`, layer_thickness, the level row (s_l, tau_c, w_c, g_c, T_l), D,
        tau, the clear/cloudy branch and omega, sc, t, w, g2, dif, g1, su, k2, the conservative
        criterion and k, E of the general branch are compute_thermal_flux's, bit for bit.  up[i]
        and down[i] are its fluxes at interface i: level i lies between interfaces i and i + 1,
        interface 0 faces space, down[0] = 0.  B = B(nu, T_l) as in compute_radiance, piB = pi*B,
            gp = g_c/(1 + g_c) ; a = (3*(gp*mu))/2
        Within a level the source is
            J(tau) = B + (w/(2 pi))*[f+(tau)(1 + a) + f-(tau)(1 - a)],  f+- = F+- - piB
        (the two-stream phase function 1 + 3 g' mu mu' with hemispherically isotropic I+- =
        F+-/pi).  Per path and grid point, each product, sum and quotient rounded as written, with
            u1 = up[i+1] - piB ; d0 = down[i] - piB ; Dm = exp(-t/mu) ; Em = -expm1(-t/mu)
        the level maps the radiance entering its surface-side face, I_bot, to
            I_top = I_bot*Dm + B*Em + (w/(2 pi))*C
            clear level (w_c == 0):  x = tau/mu and C = 0:
              I_top = I_bot*exp(-x) + B*(-expm1(-x))
            cloudy, general:
              Gamma = g2/(g1 + k) ; n = 1 - (Gamma*E)*(Gamma*E)
              P = (u1 - (Gamma*E)*d0)/n ; Q = (d0 - (Gamma*E)*u1)/n
              C = P*((1 + a) + Gamma*(1 - a))*h + Q*(Gamma*(1 + a) + (1 - a))*((1 - E*Dm)/(1 + k*mu))
              h = (E - Dm)/(1 - k mu), formed without its pole and without overflow:
                y = ((1 - k*mu)*t)/mu ; phi(z) = -expm1(-z)/z for z > 0, phi(0) = 1
                h = E*((t/mu)*phi(y)) for y >= 0 ; h = Dm*((t/mu)*phi(-y)) for y < 0
            cloudy, conservative:
              x = g1*t ; N = (u1 - d0)/(1 + x)
              C = ((u1 + d0) - x*N + a*N)*Em + (2*(g1*N))*(mu*W)
              W = Em - (t/mu)*Dm, formed without its cancellation as
                W = (t/mu)*(Em - linear_weight(t/mu, Em))
                (compute_radiance's w = 1 - Em/(t/mu) of the linear source, in its two-branch form)
        The surface is Lambertian: I_L = eps*B(T_s) + (1 - eps)*(down[L]/pi); the result is I at
        interface 0.  Levels are isothermal, the scatterers grey, the view is upward from above
        the atmosphere with one cosine per path; sunlight is not included.

        Args:
            layer_thickness, surface_temperature, surface_emissivity, emissivity_wavenumber,
            surface, diffusivity, scatterer_optical_depth, scatterer_single_scattering_albedo,
            scatterer_asymmetry: as in compute_thermal_flux.
            view_zenith_cosine: mu in (0, 1]: a scalar or one per path.
            quantities: any of "radiance" and "brightness_temperature".
            band_edges, instrument: as in compute_radiance: band means of the radiance alone;
                         with an instrument channel radiances are formed on the GPU and their
                         brightness temperatures at the channel centres on the host.

        Returns:
            Like compute_radiance: "radiance" ("W m-2 sr-1 (cm-1)-1") / "brightness_temperature"
            ("K") with the atmosphere's dims without the last, then "wavenumber", "band" or
            "channel".
        Raises ValueError, before the GPU is touched, like compute_thermal_flux and
        compute_radiance, and where the blocks of one path (beta, two work blocks and the two
        flux blocks) exceed device_output_limit: a run holds whole paths.
        """
        request = two_stream._thermal_radiance_request(
            self, layer_thickness, surface_temperature, view_zenith_cosine, surface_emissivity,
            emissivity_wavenumber, surface, diffusivity, scatterer_optical_depth,
            scatterer_single_scattering_albedo, scatterer_asymmetry, quantities, band_edges,
            instrument, range_policy)
        return two_stream.thermal_radiance(self, request, remove_pedestal, range_policy)

    def compute_thermal_radiance_linear(self, layer_thickness, surface_temperature,
                                        interface_temperature, view_zenith_cosine=1.,
                                        surface_emissivity=1., emissivity_wavenumber=None,
                                        surface="first", diffusivity=1.66,
                                        scatterer_optical_depth=None,
                                        scatterer_single_scattering_albedo=None,
                                        scatterer_asymmetry=None, quantities=("radiance",),
                                        band_edges=None, instrument=None, remove_pedestal=None,
                                        range_policy="reference"):
        """compute_thermal_radiance with a source that is linear in optical depth: within every
        level the Planck function runs linearly in the level's delta-scaled optical depth
        between its values at the level's two interfaces, as
        compute_radiance(source="linear_in_tau") has it for the clear sky and
        compute_thermal_flux_linear for the fluxes through clouds, so that a cloudy and a clear
        sounder spectrum share one source treatment.  An isothermal optically thick level
        radiates at its mean temperature instead of the temperature of the face the radiation
        leaves through: tenths of a kelvin of brightness temperature in line cores.

        The fluxes are compute_thermal_flux_linear's.  Every level scalar (tau, omega, sc, t, w,
        g1, g2, dif, su, k2, k, E, Gamma, gp, a), the clear / conservative / general decisions,
        Dm, Em, h, W, the surface line and the result at interface 0 are
        compute_thermal_radiance's, bit for bit; the level temperature enters beta only.  With B
        as in compute_radiance, per level and grid point, each product, sum and quotient rounded
        as written:
            Bt = B(T at the level's space-side interface) ; Bb = B(T at its surface-side one)
            dB = Bb - Bt ; B(tau) = Bt + dB*tau/t for tau in [0, t] from the space-side face
        The two-stream system with this source has the particular solution
        F+-p = pi*(B(tau) +- B'/su), so with
            c = (pi*dB)/(su*t)
        f+ = [compute_thermal_radiance's homogeneous part] + c, f- = [the same] - c and
            u1 = (up[i+1] - pi*Bb) - c ; d0 = (down[i] - pi*Bt) + c      (P, Q, N from these)
            C = [compute_thermal_radiance's C of its branch] + (2*(a*c))*Em
            cloudy level:
              I_top = I_bot*Dm + (Bt*Em + dB*(Em - linear_weight(t/mu, Em))) + (w/(2 pi))*C
            clear level (w_c == 0):
              x = tau/mu ; A = -expm1(-x) ; lw = linear_weight(x, A)
              I_top = I_bot*exp(-x) + (Bb*(A - lw) + Bt*lw)
        The clear line is compute_radiance's own: without scatterers, with eps = 1 and mu = 1 the
        call returns compute_radiance(layer_thickness, boundary_temperature=surface_temperature,
        source="linear_in_tau", interface_temperature=...) bit for bit.  The cloudy line is exact
        at dB = 0: a path whose levels are all cloudy and whose interface and level temperatures
        are all equal has compute_thermal_radiance's bits; a clear level under equal
        temperatures agrees with it to roundings.

        Args:
            interface_temperature: the atmosphere's shape with L + 1 along the last axis, finite
                         and > 0 [K]; interface i lies between levels i-1 and i, as in
                         compute_thermal_flux_linear.  surface_temperature stays apart from the
                         interface temperature at the surface: a skin-temperature jump is allowed.
            Everything else as in compute_thermal_radiance.

        Returns:
            Like compute_thermal_radiance, with the attribute (the key) "source":
            "linear_in_tau".
        Raises ValueError like compute_thermal_radiance and compute_thermal_flux_linear, all of
        them before the GPU is touched.
        """
        request = two_stream._thermal_radiance_linear_request(
            self, layer_thickness, surface_temperature, interface_temperature,
            view_zenith_cosine, surface_emissivity, emissivity_wavenumber, surface, diffusivity,
            scatterer_optical_depth, scatterer_single_scattering_albedo, scatterer_asymmetry,
            quantities, band_edges, instrument, range_policy)
        return two_stream.thermal_radiance(self, request, remove_pedestal, range_policy)

    def compute_thermal_radiance_at(self, layer_thickness, surface_temperature,
                                    observer_interface=None, looking="down",
                                    interface_temperature=None, view_zenith_cosine=1.,
                                    surface_emissivity=1., emissivity_wavenumber=None,
                                    surface="first", diffusivity=1.66,
                                    scatterer_optical_depth=None,
                                    scatterer_single_scattering_albedo=None,
                                    scatterer_asymmetry=None, quantities=("radiance",),
                                    band_edges=None, instrument=None, remove_pedestal=None,
                                    range_policy="reference"):
        """compute_thermal_radiance (with interface_temperature:
        compute_thermal_radiance_linear) for an observer at any interface of the atmosphere,
        looking down or up: what a zenith-viewing spectrometer on the ground sees of a cloud
        base, and what a sounder on an aircraft or a balloon sees above, between or below cloud
        decks.

        A ray that travels downward through a level is the ray that travels upward through the
        mirrored level, and the layer's two-stream solution is symmetric under that mirror.  So
        with E the face by which the ray enters a level and X the face by which it leaves,
        F_with the flux travelling with the ray at E, F_against the flux travelling against it
        at X and B_E, B_X the Planck values at the two faces, the level maps I_E to I_X by
        compute_thermal_radiance's lines (compute_thermal_radiance_linear's with
        interface_temperature), each product, sum and quotient rounded as written, with
            up[i+1] := F_with ; down[i] := F_against ; Bb := B_E ; Bt := B_X
        and every level scalar, a = (3*(gp*mu))/2 among them, unchanged.
            looking="down": the radiance travelling away from the surface at the observer.  It
              starts from compute_thermal_radiance's Lambertian surface line and passes the
              levels between the surface and the observer (E is a level's surface-side face).
            looking="up": the radiance travelling toward the surface at the observer.  It starts
              from 0 at the interface facing space and passes the levels between space and the
              observer (E is a level's space-side face); with interface_temperature
                c = (pi*(B_space - B_surface))/(su*t)
                u1 = (down[i] - pi*B_space) - c ; d0 = (up[i+1] - pi*B_surface) + c
        down = 0 at the interface facing space is used only where the outermost level itself is
        passed; an observer inside the atmosphere has a downward flux at its interface, which
        is read.  Looking down from the interface facing space the call returns
        compute_thermal_radiance's (compute_thermal_radiance_linear's) bits; without
        scatterers, with eps = 1 and mu = 1 every interface gives the matching level of
        compute_radiance(..., cumulative=True) bit for bit, in both directions.

        Args:
            observer_interface: an integer, or one per path (the atmosphere's shape without its
                         last axis), in 0 ... L: the index on the "interface" dim of
                         compute_thermal_flux's result.  Interface i lies on the level-0 side of
                         level i, interface L beyond the last level.  None: the far end of the
                         view -- looking down the interface facing space, looking up the
                         surface.  An observer at the near end passes no level and sees the
                         surface line (down) or 0 (up).
            looking: "down" or "up".
            interface_temperature: None for isothermal levels, or
                         compute_thermal_radiance_linear's interface temperatures (L + 1 along
                         the last axis), which make the source linear in tau.
            Everything else as in compute_thermal_radiance.

        Returns:
            Like compute_thermal_radiance, with the per-path coordinate "observer_interface" and
            the attribute "looking" (both keys without xarray), and with interface_temperature
            the attribute "source": "linear_in_tau".
        Raises ValueError like compute_thermal_radiance and compute_thermal_radiance_linear, and
        for an observer_interface that is no integer, out of range or of a wrong shape and a
        `looking` other than "down" or "up", all of them before the GPU is touched.
        """
        request = two_stream._thermal_radiance_at_request(
            self, layer_thickness, surface_temperature, observer_interface, looking,
            interface_temperature, view_zenith_cosine, surface_emissivity,
            emissivity_wavenumber, surface, diffusivity, scatterer_optical_depth,
            scatterer_single_scattering_albedo, scatterer_asymmetry, quantities, band_edges,
            instrument, range_policy)
        return two_stream.thermal_radiance_at(self, request, remove_pedestal, range_policy)

    def compute_solar_radiance(self, layer_thickness, solar_zenith_cosine, view_zenith_cosine=1.,
                               relative_azimuth=180., solar_irradiance=None,
                               solar_wavenumber=None, distance_factor=1., surface="first",
                               surface_albedo=0., albedo_wavenumber=None, rayleigh=True,
                               rayleigh_cross_section=None, scatterer_optical_depth=None,
                               scatterer_single_scattering_albedo=None,
                               scatterer_asymmetry=None, quantities=("radiance",),
                               band_edges=None, instrument=None, remove_pedestal=None,
                               range_policy="reference"):
        """Sunlight scattered to a sensor: the radiance a viewer above the atmosphere sees along
        the zenith cosine mu and the relative azimuth phi of each path, in an atmosphere that
        absorbs, scatters by Rayleigh's law and holds one grey scatterer per level, over a
        Lambertian surface, by the two-stream source-function technique (Toon et al. 1989):
        compute_solar_flux's two-stream fluxes are the source of multiply scattered light, the
        singly scattered direct beam is treated with the true phase functions (the TMS
        correction of Nakajima & Tanaka 1988), and the transfer equation is integrated exactly
        along the viewing direction, on the GPU, in one more sweep behind the two of
        compute_solar_flux.  The scattering counterpart of compute_solar's
        "reflected_radiance"; thermal emission is not included: compute_thermal_radiance's
        result superposes.

        Paths, levels, `surface`, layer_thickness, the level row (s_l, c_l, tau_c, w_c, h_c),
        sigma(nu), A, F0 = mu0*S and the layer scalars tau, tau_s, omega, g, f, sc, t, w, gp, g1,
        g2, g3, g4, a1, a2, k2, the conservative criterion and, in the general branch, k, the
        cosine m that the guard around k*mu0 = 1 may have moved, x = k*m, Dm = exp(-t/m) and E are
        compute_solar_flux's, bit for bit (m = mu0 in the conservative branch).  Inside the guard
        the level uses m for the beam, as the flux rows do.  up[i], diffuse[i] and direct[i] are
        its fluxes at interface i: level i lies between interfaces i (space side) and i + 1,
        interface 0 faces space, direct[0] = F0 and diffuse[0] = 0.  The host forms, in float64,
            cosT = -mu*mu0 + (sqrt((1 - mu)*(1 + mu))*sqrt((1 - mu0)*(1 + mu0)))*cos(phi*pi/180)
        limited to [-1, 1].  With tau' in [0, t] measured from the level's space-side face and
        S_i = direct[i]:
            Dv = exp(-t/mu) ; a = (3*(gp*mu))/2
            beam       B(tau') = S_i*exp(-tau'/m)
            diffuse    F+(tau'), F-(tau'): the two-stream solution in the level (below)
            source     J(tau') = (w/(2 pi))*[F+(tau')(1 + a) + F-(tau')(1 - a)]
                               + ((omega/sc)*Pmix/(4 pi))*(S_i/m)*exp(-tau'/m)
            Pmix = (tau_R*PR + w_c*PH)/tau_s ;  PR = (3/4)(1 + cosT^2)
            PH = (1 - gc^2)/(1 + gc^2 - 2 gc cosT)^(3/2),  gc = h_c/w_c  (0 where w_c == 0)
            transfer   I_top = I_bot*Dv + Integral_0^t J(tau') exp(-tau'/mu) dtau'/mu
        F+- solve the Meador-Weaver equations
            dF+/dtau' = g1 F+ - g2 F- - w g3 (B/m) ;  dF-/dtau' = g2 F+ - g1 F- + w g4 (B/m)
        whose particular solution Z+- exp(-tau'/m) has, with X = (1 - x)*(1 + x) (X = 1,
        conservative), each product, sum and quotient rounded as written:
            ws = w*S_i ; Z+ = (ws*(g3 - a2*m))/X ; Z- = -((ws*(g4 + a1*m))/X)
            u1 = up[i+1] - Z+*Dm ; d0 = diffuse[i] - Z-
            bm = (m/(m + mu))*(-expm1(-(t/m + t/mu)))
            I_top = I_bot*Dv + (w/(2 pi))*C + (((omega/sc)*Pmix)/(4 pi))*((S_i/m)*bm)
            general:
              Gamma = g2/(g1 + k) ; n = 1 - (Gamma*E)*(Gamma*E)
              P = (u1 - (Gamma*E)*d0)/n ; Q = (d0 - (Gamma*E)*u1)/n
              C = P*((1 + a) + Gamma*(1 - a))*h + Q*(Gamma*(1 + a) + (1 - a))*((1 - E*Dv)/(1 + k*mu))
                  + (Z+*(1 + a) + Z-*(1 - a))*bm
              h = (E - Dv)/(1 - k mu), formed without its pole and without overflow:
                y = ((1 - k*mu)*t)/mu ; phi(z) = -expm1(-z)/z for z > 0, phi(0) = 1
                h = E*((t/mu)*phi(y)) for y >= 0 ; h = Dv*((t/mu)*phi(-y)) for y < 0
            conservative:
              x = g1*t ; N = (u1 - d0)/(1 + x) ; Ev = -expm1(-t/mu)
              C = ((u1 + d0) - x*N + a*N)*Ev + (2*(g1*N))*(mu*W) + (Z+*(1 + a) + Z-*(1 - a))*bm
              W = Ev - (t/mu)*Dv, formed without its cancellation as
                W = (t/mu)*(Ev - linear_weight(t/mu, Ev))
        A level with tau == 0 is the identity; one with tau_s == 0 only attenuates, I_top =
        I_bot*exp(-tau/mu).  The surface is Lambertian: I_L = A*((direct[L] + diffuse[L])/pi); the
        result is I at interface 0.  The diffuse field is two-stream: against a multi-stream code
        radiances are good to several per cent; the single scattering is exact.  The scatterers
        are grey, the view is upward from above the atmosphere with one direction per path.

        Args:
            layer_thickness, solar_zenith_cosine, solar_irradiance, solar_wavenumber,
            distance_factor, surface, surface_albedo, albedo_wavenumber, rayleigh,
            rayleigh_cross_section, scatterer_optical_depth,
            scatterer_single_scattering_albedo, scatterer_asymmetry: as in compute_solar_flux.
            view_zenith_cosine: mu in (0, 1]: a scalar or one per path.
            relative_azimuth: phi [degrees], finite: a scalar or one per path; the angle between
                         the horizontal directions of propagation of the sunlight and of the
                         viewed light: 180 is the backscatter side, with the Sun behind the
                         sensor.
            quantities: "radiance".
            band_edges, instrument: as in compute_thermal_radiance: band means of the radiance,
                         or channel radiances, formed on the GPU.

        Returns:
            Like compute_radiance: "radiance" ("W m-2 sr-1 (cm-1)-1") with the atmosphere's dims
            without the last, then "wavenumber", "band" or "channel".
        Raises ValueError, before the GPU is touched, like compute_solar_flux and
        compute_thermal_radiance, and where the blocks of one path (beta, two work blocks and the
        three flux blocks) exceed device_output_limit: a run holds whole paths.
        """
        request = two_stream._solar_radiance_request(
            self, layer_thickness, solar_zenith_cosine, view_zenith_cosine, relative_azimuth,
            solar_irradiance, solar_wavenumber, distance_factor, surface, surface_albedo,
            albedo_wavenumber, rayleigh, rayleigh_cross_section, scatterer_optical_depth,
            scatterer_single_scattering_albedo, scatterer_asymmetry, quantities, band_edges,
            instrument, range_policy)
        return two_stream.solar_radiance(self, request, remove_pedestal, range_policy)

    def compute_thermal_radiance_spectral(self, layer_thickness, surface_temperature,
                                          scatterer_wavenumber, scatterer_optical_depth,
                                          scatterer_single_scattering_albedo,
                                          scatterer_asymmetry, view_zenith_cosine=1.,
                                          surface_emissivity=1., emissivity_wavenumber=None,
                                          surface="first", diffusivity=1.66,
                                          quantities=("radiance",), band_edges=None,
                                          instrument=None, remove_pedestal=None,
                                          range_policy="reference"):
        """compute_thermal_radiance with cloud and aerosol optics that vary with wavenumber: the
        cloudy spectrum a sounder measures.  The scatterer of every level is a table over the
        knots scatterer_wavenumber, interpolated and limited per grid point as in
        compute_solar_flux_spectral (include/lbl_amd_scatterer.h):
            j = the largest index with k_j <= nu, limited to 0 .. M-2
            u = (nu - k_j)/(k_{j+1} - k_j), limited to [0, 1]
            v = e_j + u*(e_{j+1} - e_j), limited to [min(e_j, e_{j+1}), max(e_j, e_{j+1})]
            w_c = omega_c*tau_c
        The fluxes are compute_thermal_flux_spectral's (isothermal levels), and the view sweep
        behind them places every grid point among the knots by the same lines.  A level whose
        knots all have omega_c*tau_c == 0 is a clear level, with tau = tau_a + tau_c(nu):
            x = tau/mu ; I_top = I_bot*exp(-x) + B*(-expm1(-x))
        In any other level every grid point takes compute_thermal_radiance's cloudy lines with
        its own tau_c, w_c, f = g_c*g_c, gp = g_c/(1 + g_c) and a = (3*(gp*mu))/2; where tau == 0
        the clear line (x = 0, the identity).  A table that is flat in nu gives
        compute_thermal_radiance's result bit for bit; with no scatterer anywhere, eps = 1 and
        mu = 1 the result is compute_radiance's bit for bit.  Levels are isothermal: there is no
        interface_temperature.

        Args:
            scatterer_wavenumber, scatterer_optical_depth, scatterer_single_scattering_albedo,
            scatterer_asymmetry: as in compute_solar_flux_spectral.
            Everything else as in compute_thermal_radiance.

        Returns:
            Like compute_thermal_radiance, with the attribute (the key) "scatterer": "spectral".
        Raises ValueError like it, all of them before the GPU is touched.
        """
        request = two_stream._thermal_radiance_request(
            self, layer_thickness, surface_temperature, view_zenith_cosine, surface_emissivity,
            emissivity_wavenumber, surface, diffusivity, scatterer_optical_depth,
            scatterer_single_scattering_albedo, scatterer_asymmetry, quantities, band_edges,
            instrument, range_policy,
            scatterer_wavenumber=two_stream._given_knots(scatterer_wavenumber),
            caller="compute_thermal_radiance_spectral")
        return two_stream.thermal_radiance(self, request, remove_pedestal, range_policy)

    def compute_solar_radiance_spectral(self, layer_thickness, solar_zenith_cosine,
                                        scatterer_wavenumber, scatterer_optical_depth,
                                        scatterer_single_scattering_albedo, scatterer_asymmetry,
                                        view_zenith_cosine=1., relative_azimuth=180.,
                                        solar_irradiance=None, solar_wavenumber=None,
                                        distance_factor=1., surface="first", surface_albedo=0.,
                                        albedo_wavenumber=None, rayleigh=True,
                                        rayleigh_cross_section=None, quantities=("radiance",),
                                        band_edges=None, instrument=None, remove_pedestal=None,
                                        range_policy="reference"):
        """compute_solar_radiance with cloud and aerosol optics that vary with wavenumber: the
        cloudy or hazy spectrum a shortwave spectrometer measures.  The scatterer of every level
        is a table over the knots scatterer_wavenumber, interpolated and limited per grid point
        as in compute_solar_flux_spectral (j, u and v as in compute_thermal_radiance_spectral),
        with w_c = omega_c*tau_c and h_c = w_c*g_c formed per grid point on the GPU.  The fluxes
        are compute_solar_flux_spectral's, and the view sweep behind them places every grid
        point among the knots by the same lines.  Per grid point tau_c, w_c and h_c go into
        compute_solar_radiance's level, and the Henyey-Greenstein factor PH is per grid point
        too, from gc = h_c/w_c (0 where w_c == 0; limited to 1 - 2^-53, which it can only reach
        where w_c is a subnormal number).  Without Rayleigh scattering a level none of whose
        knots scatters only attenuates: I_top = I_bot*exp(-(tau_a + tau_c(nu))/mu).  A table
        that is flat in nu gives compute_solar_radiance's result bit for bit.

        Args:
            scatterer_wavenumber, scatterer_optical_depth, scatterer_single_scattering_albedo,
            scatterer_asymmetry: as in compute_solar_flux_spectral.
            Everything else as in compute_solar_radiance.

        Returns:
            Like compute_solar_radiance, with the attribute (the key) "scatterer": "spectral".
        Raises ValueError like it, all of them before the GPU is touched.
        """
        request = two_stream._solar_radiance_request(
            self, layer_thickness, solar_zenith_cosine, view_zenith_cosine, relative_azimuth,
            solar_irradiance, solar_wavenumber, distance_factor, surface, surface_albedo,
            albedo_wavenumber, rayleigh, rayleigh_cross_section, scatterer_optical_depth,
            scatterer_single_scattering_albedo, scatterer_asymmetry, quantities, band_edges,
            instrument, range_policy,
            scatterer_wavenumber=two_stream._given_knots(scatterer_wavenumber),
            caller="compute_solar_radiance_spectral")
        return two_stream.solar_radiance(self, request, remove_pedestal, range_policy)

    def compute_kdistribution(self, band_edges, g_edges=16, g_points=None,
                              quantities=("absorption_g_mean",), remove_pedestal=None,
                              range_policy="reference", weighting=None,
                              weighting_temperature=None):
        """Band k-distributions, what a correlated-k table is built from: within every band and
        at every level the absorption coefficient re-ordered by size and summarised on intervals
        of the cumulative probability g, formed on the GPU from the "total" absorption block
        without handing that block to the host.  A per-level product: no path lengths.

        A table stores k(g) and, beside it, the share of the band's source that falls into
        each g interval (RRTMG's `fracs`, RRTMGP's `planck_frac`; for the shortwave the same of
        the solar spectrum), and averages k within an interval with that source as the weight.
        `weighting` gives both: the sort then carries every value's column, and a weight per
        column travels through the permutation.

        With beta the absorption coefficient [m-1] of compute_absorption("total",
        remove_pedestal, range_policy), band b the N grid points e_b <= grid < e_b+1, and
        k_0 <= ... <= k_N-1 the band's beta at one level sorted ascending -- in the total order
        of the fp64 bits u read as keys, u ^ 2^63 for a clear sign bit and ~u for a set one,
        compared unsigned (-inf < negatives < -0 < +0 < positives < +inf < NaN; numpy.sort
        apart from +-0 ties and NaN payloads), which makes the result unique: repeated calls
        and any device_output_limit give the same bits.  pi is the permutation that sorts the
        pairs (key, column offset j in the band) lexicographically,
        numpy.argsort(keys, kind="stable"): k_i = beta_pi(i).  With a weight w_j >= 0 per column,
        W_i = w_pi(i) and WK_i = W_i*k_i (one rounding); sw_q and swk_q are the sums of W and WK
        over interval q, added in a fixed order on the GPU.

        Args:
            band_edges: strictly increasing finite edges e_0 < ... < e_B, as compute_path's.
            g_edges: an int Q in 1..64 -- the edges [0, cumsum(w/2)] of x, w = leggauss(Q), the
                     last set to exactly 1: intervals of the Gauss weights -- or Q + 1 strictly
                     increasing edges from exactly 0 to exactly 1.  Interval q of a band holds
                     the sorted samples ceil(G_q N) <= i < ceil(G_q+1 N) (products in fp64).
            g_points: None -- (x + 1)/2 of the same Q -- or values in [0, 1].
            quantities: any of
                "absorption_g_mean" [..., band, g_interval]: the arithmetic mean of the
                    interval's samples (NaN for an interval or band without points);
                "absorption_g_quantile" [..., band, g_point]: with x = min(max(g N - 0.5, 0),
                    N - 1), i = floor(x), f = x - i: k_i + f*(k_min(i+1, N-1) - k_i), each
                    operation rounded as written (NaN for a band without points);
                "sorted_absorption" [..., wavenumber]: every band's columns holding its sorted
                    values, NaN in the columns of no band;
                and, with `weighting` only (ValueError without it),
                "weight_g_fraction" [..., band, g_interval]: sw_q / sum_q sw_q -- 0 for an
                    interval without points, NaN where the band's sum is 0 or the band is empty;
                "absorption_g_weighted_mean" [..., band, g_interval]: swk_q / sw_q, NaN where
                    sw_q is 0;
                "sorted_column" [..., wavenumber], int32: pi(i) in column band start + i, an
                    offset from the band's first column; -1 in the columns of no band.  Like
                    "sorted_absorption" it travels to the host only when asked for.
            weighting: None; "planck" -- w_j = B(nu_j, T) [W m-2 sr-1 (cm-1)-1] as
                    compute_radiance forms it (0 for nu <= 0), T the level's own temperature or
                    `weighting_temperature`; or an array of one finite weight >= 0 per grid
                    point, the same for every level, uploaded once per call.  The default Sun of
                    compute_solar, for one:
                    weighting=paths.SOLAR_SOLID_ANGLE*planck(grid, paths.SOLAR_TEMPERATURE) with
                    planck(nu, T) = (((paths.PLANCK_C1*nu)*nu)*nu)/numpy.expm1(
                    (paths.PLANCK_C2*nu)/T).
            weighting_temperature: with weighting="planck" only: one number, or an array of the
                    atmosphere's shape, finite and > 0 [K].

        Returns:
            Like compute_absorption: an xarray Dataset when xarray is installed, else a dict of
            numpy arrays [m-1], with the coordinates "band_lower", "band_upper", "band_points",
            "g_lower", "g_upper", "g_weight" (the interval widths), "g_interval_points"
            [band, g_interval], "g_point", and with "sorted_absorption" or "sorted_column" also
            "wavenumber" and "g" = (i + 0.5)/N on the wavenumber dim.  With a weighting the
            result carries it as the attribute (the key) "weighting": "planck" or "array".
        """
        request = paths._kdistribution_request(self, band_edges, g_edges, g_points, quantities,
                                               range_policy, weighting, weighting_temperature)
        want_means = "absorption_g_mean" in request.quantities
        want_quantiles = "absorption_g_quantile" in request.quantities
        bands, points = request.starts.size - 1, request.g_points.size
        # The device takes one flat list of intervals: every band's Q + 1 starts in a row, the
        # last "interval" of a band being the gap to the next band (dropped on the host).
        intervals = request.interval_starts.ravel()
        level_quantities = tuple(q for q in ("absorption_g_mean", "absorption_g_quantile")
                                 if q in request.quantities)
        widths = {"absorption_g_mean": intervals.size - 1,
                  "absorption_g_quantile": bands*points, paths._BETA: self.grid.size}
        products = [_Product(q, q, True) for q in level_quantities]
        if "sorted_absorption" in request.quantities:
            products.append(_Product("sorted_absorption", paths._BETA, True))
        if request.weighting is not None:
            return self._weighted_kdistribution(request, intervals, level_quantities, widths,
                                                products, remove_pedestal, range_policy)

        def sweeper(call, run):
            scratch = call.take(run)

            def sweep(index, beta, a, b, outputs):
                call.engine.band_distribution(
                    beta, call.columns, request.starts, scratch=scratch.rows(b - a),
                    interval_start=intervals if want_means else None,
                    means=outputs.get("absorption_g_mean"),
                    point_index=request.point_index if want_quantiles else None,
                    point_fraction=request.point_fraction if want_quantiles else None,
                    quantiles=outputs.get("absorption_g_quantile"), asynchronous=True)
            return sweep
        # Two blocks per level: beta, sorted in place, and the sort's scratch.
        values = self._sweep_runs(
            request, [_Pass(False, level_quantities, ())], remove_pedestal, range_policy, sweeper,
            level_blocks=2, products=products, widths=widths)
        return paths._create_kdistribution_dataset(self, values, request)

    def _weighted_kdistribution(self, request, intervals, level_quantities, widths, products,
                                remove_pedestal, range_policy):
        """compute_kdistribution with a weighting: the same sweep through
        Engine.band_distribution_weighted."""
        want_means = "absorption_g_mean" in request.quantities
        want_quantiles = "absorption_g_quantile" in request.quantities
        want_weighted = "absorption_g_weighted_mean" in request.quantities
        want_sums = want_weighted or "weight_g_fraction" in request.quantities
        want_columns = "sorted_column" in request.quantities
        # pi as int32: two to a float64 of a block, rows of 2*pairs >= grid points.
        pairs = (self.grid.size + 1)//2
        sums = ((paths._WEIGHT_SUMS,) if want_sums else ()) + \
            ((paths._WEIGHTED_SUMS,) if want_weighted else ())
        level_quantities = level_quantities + sums + (("sorted_column",) if want_columns else ())
        widths = dict(widths, sorted_column=pairs,
                      **{name: intervals.size - 1 for name in sums})
        products = products + [_Product(name, name, True) for name in sums]
        if want_columns:
            products.append(_Product("sorted_column", "sorted_column", True))

        def sweeper(call, run):
            fills = paths._FilledOnce(call)
            grid = fills.grid
            scratch, index_scratch = call.take(run), call.take(run, columns=pairs)
            index_rows = None if want_columns else call.take(run, columns=pairs)
            weight_rows = call.take(run) if want_sums else None
            weighted_rows = call.take(run) if want_sums else None
            # scale*irradiance with scale = 1: the caller's weights, bit for bit.
            weight_row = None if request.weights is None else fills.take(
                1, lambda row: call.engine.solar_spectrum(
                    grid, row, call.columns, irradiance=request.weights, scale=1.,
                    asynchronous=True))

            def sweep(index, beta, a, b, outputs):
                fills.queue()
                rows = b - a
                call.engine.band_distribution_weighted(
                    beta, call.columns, request.starts,
                    outputs["sorted_column"] if want_columns else index_rows.rows(rows),
                    scratch=scratch.rows(rows), index_scratch=index_scratch.rows(rows), grid=grid,
                    row_temperature=None if weight_row is not None
                    else request.weight_temperature[a:b],
                    weight_row=weight_row,
                    weight_rows=weight_rows.rows(rows) if want_sums else None,
                    weighted_rows=weighted_rows.rows(rows) if want_sums else None,
                    interval_start=intervals if want_means or want_sums else None,
                    weight_sums=outputs.get(paths._WEIGHT_SUMS),
                    weighted_sums=outputs.get(paths._WEIGHTED_SUMS),
                    means=outputs.get("absorption_g_mean"),
                    point_index=request.point_index if want_quantiles else None,
                    point_fraction=request.point_fraction if want_quantiles else None,
                    quantiles=outputs.get("absorption_g_quantile"), asynchronous=True)
            return sweep
        # Five blocks per level: beta, sorted in place, the sort's scratch, W and W*k on the
        # grid, and pi with its scratch, half a block each.
        values = self._sweep_runs(
            request, [_Pass(False, level_quantities, ())], remove_pedestal, range_policy, sweeper,
            level_blocks=5, products=products, widths=widths)
        return paths._create_kdistribution_dataset(self, values, request)

    # The host side of the path products is paths.py and that of compute_absorption is
    # absorption.py: their functions take the Spectroscopy first.
    _compute_levels, total_into = absorption.compute_levels, absorption.total_into
    _path_request, _radiance_request = paths._path_request, paths._radiance_request
    _flux_request, _sweep_runs = paths._flux_request, paths._sweep_runs
    _flux_interfaces = paths._flux_interfaces
    _solar_request, _solar_interfaces = paths._solar_request, paths._solar_interfaces
    _create_solar_dataset = paths._create_solar_dataset
    _solar_flux_request = two_stream._solar_flux_request
    _thermal_flux_request = two_stream._thermal_flux_request
    _thermal_flux_linear_request = two_stream._thermal_flux_linear_request
    _thermal_radiance_request = two_stream._thermal_radiance_request
    _thermal_radiance_linear_request = two_stream._thermal_radiance_linear_request
    _thermal_radiance_at_request = two_stream._thermal_radiance_at_request
    _solar_radiance_request = two_stream._solar_radiance_request
    _create_path_dataset = paths._create_path_dataset
    _create_flux_dataset = paths._create_flux_dataset

    def _create_output_dataset(self, absorption, output_format):
        dims = list(self.output.dims)
        if output_format == "all":
            variables = dict(absorption)
            extra = {"mechanism": np.asarray(self.output.mechanisms)}
        elif output_format == "gas":
            dims.pop(-2)
            variables = dict(absorption)
            extra = {}
        else:
            dims.pop(-2)
            parts = list(absorption.values())
            variables = {"absorption": parts[0] if len(parts) == 1 else sum(parts)} \
                if parts else {}
            extra = {}
        xarray = _optional_xarray()
        if xarray is None:
            out = {"wavenumber": self.grid}
            out.update(extra)
            out.update(variables)
            return out
        DataArray, Dataset = xarray.DataArray, xarray.Dataset
        data_vars = {"wavenumber": DataArray(self.grid, dims=("wavenumber",),
                                             attrs={"units": "cm-1"})}
        for key, value in extra.items():
            data_vars[key] = DataArray(value, dims=("mechanism",))
        for key, value in variables.items():
            data_vars[key] = DataArray(value, dims=dims, attrs=self.output.units)
        return Dataset(data_vars=data_vars)
