"""Engine: one GPU's handle of the C ABI (include/lbl_amd.h), its calls as methods that check
shapes and fill in the arguments, and the process-wide engine per device.

The binding itself -- prototypes, constants, the loader -- is pylbl_amd/abi.py; the HBM and
pinned-memory pools are pylbl_amd/device_memory.py.  There is no CPU fallback: if the library is
missing or no MI355X is visible, creating an Engine raises.
"""
from ctypes import byref, c_double, c_int32, c_int64, c_void_p
import os
import threading

import numpy as np

# What the methods below use, and what the rest of the package, the tests and the benchmark read
# from this module.
from .abi import (ACCUMULATE, ASYNC, DEFER_FINISH, EXPORTED_SYMBOLS, FARFIELD, LBL_OK, MAX_BANDS,
                  MAX_XSEC_BANDS, OUT_DEVICE, PATH_BRIGHTNESS, PATH_CONTINUE, PATH_CUMULATIVE,
                  PATH_FLUX_UP, PATH_FROM_LAST, PATH_JACOBIAN_BOUNDARY_E,
                  PATH_JACOBIAN_BOUNDARY_T, PATH_JACOBIAN_DEPTH, PATH_JACOBIAN_LOG_DEPTH,
                  PATH_JACOBIAN_OUTPUTS, PATH_JACOBIAN_PER_LEVEL, PATH_JACOBIAN_TEMPERATURE,
                  PATH_OPTICAL_DEPTH, PATH_RADIANCE, PATH_THERMAL_OUTPUTS, PATH_TRANSMITTANCE,
                  PATH_TWO_STREAM_OUTPUTS, RANGE_POLICIES,
                  SCALE_DENSITY, TABLE_NO_ALIAS, TABLE_NO_ISOTOPOLOGUES, TABLE_NO_TIPS,
                  TABLE_NO_TRANSITIONS, TABLE_NOT_RECTANGULAR, TABLE_OPEN_FAILED, VMR_COUNT,
                  VMR_H2O, VMR_N2, VMR_O2, VMR_SELF, VMR_TOTAL, BandDescriptor, library,
                  read_line_table)
from .device_memory import DevicePool, DeviceSpectra, PinnedPool
from .errors import EngineError


def _f64(array):
    return np.ascontiguousarray(array, dtype=np.float64)


def _slot_levels(temperature, pressure, accumulate, asynchronous):
    """(temperature, pressure, flags) of a slot call: float64 arrays [levels] and ACCUMULATE /
    ASYNC."""
    t, p = _f64(np.atleast_1d(temperature)), _f64(np.atleast_1d(pressure))
    return t, p, (ACCUMULATE if accumulate else 0) | (ASYNC if asynchronous else 0)


def _path_run(band_start, level_begin, rows, levels_per_path, from_last, asynchronous):
    """(int64 band starts or None, n_bands, flags) of a path call on the levels [level_begin,
    level_begin + rows): PATH_FROM_LAST, ASYNC and PATH_CONTINUE when the run's first level in
    sweep order lies inside a path."""
    starts = None if band_start is None else np.ascontiguousarray(band_start, dtype=np.int64)
    n_bands = 0 if starts is None else starts.size - 1
    flags = (PATH_FROM_LAST if from_last else 0) | (ASYNC if asynchronous else 0)
    end = int(level_begin) + rows
    if (end % int(levels_per_path) if from_last else int(level_begin) % int(levels_per_path)):
        flags |= PATH_CONTINUE
    return starts, n_bands, flags


def _per_row(beta, message, *values):
    """(rows, row length of the DeviceSpectra `beta`, float64 arrays of one value per row);
    ValueError(message) where one of `values` is not that."""
    rows, stride = int(beta.shape[0]), int(beta.shape[1])
    arrays = [_f64(np.atleast_1d(x)) for x in values]
    if any(x.shape != (rows,) for x in arrays):
        raise ValueError(message)
    return (rows, stride, *arrays)


def _per_path(n_paths, message, *values):
    """Each of `values` as a float64 array of one value per path, None as it is."""
    arrays = [None if x is None else _f64(np.atleast_1d(x)) for x in values]
    if any(x is not None and x.shape != (int(n_paths),) for x in arrays):
        raise ValueError(message)
    return arrays


def _whole_paths(beta, level_table, n_paths, surface_rows, surface_name, band_start, level_begin,
                 levels_per_path, from_last, asynchronous, work=None):
    """(rows, row length, float64 level table, int64 band starts or None, n_bands, flags) of a
    two-stream call on the whole paths in `beta`, checked: level_table [rows, 5], work (where
    the entry has one) [>= 2*rows, row length], the surface's rows -- albedo_rows or
    emissivity_rows, named by surface_name -- None or [n_paths, row length]; the flags are
    _path_run's of a run that starts at a path's end, with PATH_FROM_LAST."""
    rows, stride = int(beta.shape[0]), int(beta.shape[1])
    table = _f64(level_table)
    if table.shape != (rows, 5):
        raise ValueError(f"level_table has shape {table.shape}, need {rows} x 5.")
    if work is not None and (work.shape[1] != stride or work.shape[0] < 2*rows):
        raise ValueError(f"work has shape {work.shape}, need {2*rows} x {stride}.")
    if surface_rows is not None and tuple(surface_rows.shape) != (int(n_paths), stride):
        raise ValueError(f"{surface_name} must be [n_paths, row length of beta].")
    starts, n_bands, flags = _path_run(band_start, level_begin, rows, levels_per_path, False,
                                       asynchronous)
    return rows, stride, table, starts, n_bands, flags | (PATH_FROM_LAST if from_last else 0)


def _output_pointers(name, names, outputs, rows, n_paths, stride, n_bands):
    """The addresses of a two-stream entry's outputs in the order of `names`
    (PATH_TWO_STREAM_OUTPUTS, PATH_THERMAL_OUTPUTS), None for one not wanted, checked: *_rows
    [>= rows, or n_paths for top_*, row length], *_mean [the same, bands]."""
    unknown = set(outputs) - set(names)
    if unknown:
        raise TypeError(f"{name} has no output {sorted(unknown)}.")
    pointers = []
    for output in names:
        out = outputs.get(output)
        need = int(n_paths) if output.startswith("top_") else rows
        _check_outputs((out,), need, n_bands if output.endswith("_mean") else stride)
        pointers.append(_address(out))
    return pointers


def _edge_rows(edge_temperature, rows):
    """None, or the interface temperatures of a path call as a float64 array [rows, 2]."""
    if edge_temperature is None:
        return None
    edges = _f64(edge_temperature)
    if edges.shape != (rows, 2):
        raise ValueError(f"edge_temperature has shape {edges.shape}, need {rows} x 2.")
    return edges


def _knot_table(knot_wavenumber, knot_optics, rows):
    """(float64 knots [M], float64 optics [rows, M, 3], M) of a spectral scatterer's table."""
    knots, optics = _f64(knot_wavenumber), _f64(knot_optics)
    if knots.ndim != 1 or optics.shape != (rows, knots.size, 3):
        raise ValueError(f"knot_wavenumber has shape {knots.shape} and knot_optics "
                         f"{optics.shape}, need [M] and {rows} x M x 3.")
    return knots, optics, knots.size


def _check_outputs(outputs, rows, width):
    for out in outputs:
        if out is not None and (out.shape[1] != width or out.shape[0] < rows):
            raise ValueError(f"an output has shape {out.shape}, need rows x {width}.")


def _interval_table(interval_start, outputs, rows):
    """(int64 interval starts or None, n_intervals) of band_distribution's interval_start, which
    goes together with at least one of `outputs` (DeviceSpectra [rows, n_intervals] or None)."""
    wanted = [out for out in outputs if out is not None]
    if (interval_start is None) != (not wanted):
        raise ValueError("interval_start and means go together.")
    if not wanted:
        return None, 0
    intervals = np.ascontiguousarray(interval_start, dtype=np.int64)
    if intervals.ndim != 1 or intervals.size < 2:
        raise ValueError("interval_start must hold n_intervals + 1 >= 2 column starts.")
    _check_outputs(wanted, rows, intervals.size - 1)
    return intervals, intervals.size - 1


def _point_tables(point_index, point_fraction, quantiles, rows, n_bands):
    """(int64 index, float64 fraction, n_points) of band_distribution's quantile tables [n_bands,
    n_points], which go together with quantiles (DeviceSpectra [rows, n_bands*n_points]);
    (None, None, 0) without them."""
    if (point_index is None) != (quantiles is None) or \
            (point_fraction is None) != (quantiles is None):
        raise ValueError("point_index, point_fraction and quantiles go together.")
    if quantiles is None:
        return None, None, 0
    index = np.ascontiguousarray(point_index, dtype=np.int64)
    fraction = _f64(point_fraction)
    if index.ndim != 2 or index.shape[0] != n_bands or index.shape[1] < 1 or \
            fraction.shape != index.shape:
        raise ValueError("point_index and point_fraction must be [n_bands, n_points].")
    _check_outputs((quantiles,), rows, n_bands*index.shape[1])
    return index, fraction, index.shape[1]


def _address(x):
    """What a C entry takes for a DeviceSpectra or an array: None for None."""
    if x is None:
        return None
    return x.pointer if hasattr(x, "pointer") else x.ctypes.data


def _levels(values):
    """Per-level input as a contiguous 1-d float64 array (no copy, and none of numpy's dispatch,
    when it already is one: a call on a small grid costs the host ~35 us all told)."""
    if type(values) is np.ndarray and values.dtype == np.float64 and values.ndim == 1 and \
            values.flags.c_contiguous:
        return values
    return _f64(np.atleast_1d(values))


class Engine(object):
    """One GPU's engine: resident line tables plus the batched compute call."""
    def __init__(self, device=0):
        self.lib = library()
        self.handle = c_void_p()
        status = self.lib.lbl_engine_create(int(device), byref(self.handle))
        if status != LBL_OK:
            message = self.lib.lbl_last_error(None).decode()
            self.handle = c_void_p()
            raise EngineError(f"lbl_engine_create failed ({status}): {message}")
        self.device = int(device)
        self.pinned = PinnedPool(self)
        self.blocks = DevicePool(self)
        # Held by callers whose result takes SEVERAL calls on this engine that must not be
        # interleaved with another thread's (Spectroscopy.compute_absorption: calls that add into
        # one block in a fixed order, one deferred call per engine).  Single calls need no lock:
        # the C ABI serialises them per handle (include/lbl_amd.h, "Threads").
        self.pipeline = threading.RLock()
        # Channel count of each instrument handle made by instrument_create: the width of `out`
        # that instrument_apply checks before anything is launched.
        self._instrument_channels = {}
        # Options for every engine of the process, for experiments: PYLBL_AMD_OPTIONS="name=value,..."
        # (kept in `environment_options` so that whoever reports numbers can say so: bench.py
        # echoes them).  "ablate" leaves work out -- results are wrong -- and is refused here: a
        # left-over environment variable must not change what every Gas object returns.
        self.environment_options = {}
        for pair in filter(None, os.environ.get("PYLBL_AMD_OPTIONS", "").split(",")):
            name, _, value = pair.partition("=")
            name = name.strip()
            if name == "ablate":
                self.close()
                raise EngineError("PYLBL_AMD_OPTIONS must not set 'ablate' (results would be "
                                  "wrong for every engine of the process); use "
                                  "Engine.set_option('ablate', ...) on the one engine being timed.")
            self.set_option(name, float(value))
            self.environment_options[name] = float(value)

    def host_array(self, shape):
        """float64 array of the given shape in page-locked host memory (recycled, see
        PinnedPool): the place to receive spectra from HBM."""
        return self.pinned.array(shape)

    def _check(self, status):
        if status != LBL_OK:
            raise EngineError(f"status {status}: {self.lib.lbl_last_error(self.handle).decode()}")

    def close(self):
        if self.handle:
            self.pinned.clear()
            self.blocks.clear()
            self.lib.lbl_engine_destroy(self.handle)
            self.handle = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, name, value):
        self._check(self.lib.lbl_set_option(self.handle, name.encode(), int(value)))

    def load(self, table):
        """Uploads a pylbl_amd.database.LineTable; returns the molecule handle."""
        columns = [_f64(getattr(table, x)) for x in
                   ("nu", "sw", "gamma_air", "gamma_self", "n_air", "elower", "delta_air")]
        iso = np.ascontiguousarray(table.local_iso_id, dtype=np.int32)
        mass = _f64(table.mass_by_slot())
        tips_t = _f64(table.tips_temperature)
        tips_q = _f64(table.tips_data)
        if tips_q.ndim != 2 or tips_q.shape[1] != tips_t.size:
            raise ValueError("tips_data must be [num_iso, num_t] with num_t temperatures.")
        handle = c_int32(-1)
        self._check(self.lib.lbl_molecule_load(
            self.handle, columns[0].size, *[x.ctypes.data for x in columns], iso.ctypes.data,
            mass.ctypes.data, tips_q.shape[0], tips_q.shape[1], tips_t.ctypes.data,
            tips_q.ctypes.data, byref(handle)))
        return handle.value

    def load_sqlite(self, path, name):
        """File -> HBM in one call (lbl_molecule_load_sqlite): molecule `name` (any alias) of the
        SQLite file at `path` in pyLBL's schema, read by the C reader and uploaded; returns the
        molecule handle.  Raises EngineError with the reader's message when the file lacks
        something (status LBL_TABLE_*, include/lbl_amd.h)."""
        handle = c_int32(-1)
        self._check(self.lib.lbl_molecule_load_sqlite(self.handle, os.fsencode(str(path)),
                                                      str(name).encode(), byref(handle)))
        return handle.value

    def free(self, molecule):
        self._check(self.lib.lbl_molecule_free(self.handle, int(molecule)))

    def compute(self, molecule, temperature, pressure, vmr, v0, vn, n_per_v, cut_off=25,
                remove_pedestal=False, range_policy="reference", out=None, scale_density=False,
                accumulate=False, asynchronous=False, want_evals=False, farfield=False,
                deliver=None, pieces=4, defer_finish=False):
        """Cross sections [m2] for every level: returns float64[levels, (vn-v0)*n_per_v]
        (or fills `out`: a host array or a DeviceSpectra).

        deliver: (until engine.synchronize() the delivered part of `out` must not be written again:
        calls are ordered by the memory they write, not by what a copy still reads.)
        With a device `out`, a float64 [levels, columns] host view with contiguous rows
        (page-locked: Engine.host_array) that receives the first `columns` points of every level
        while the call computes, in `pieces` runs of tiles (lbl_compute_streamed).
        defer_finish: keep the call's last kernels (the ones that touch `out`) back until
        finish_deferred() / synchronize(): LBL_DEFER_FINISH."""
        t, p, x = _levels(temperature), _levels(pressure), _levels(vmr)
        if not (t.shape == p.shape == x.shape and t.ndim == 1):
            raise ValueError("temperature, pressure and vmr must be 1-d and equally long.")
        n = (int(vn) - int(v0))*int(n_per_v)
        flags = (SCALE_DENSITY if scale_density else 0) | (ACCUMULATE if accumulate else 0) | \
                (ASYNC if asynchronous else 0) | (FARFIELD if farfield else 0) | \
                (DEFER_FINISH if defer_finish else 0)
        if hasattr(out, "pointer"):
            # Device memory: a DeviceSpectra or anything exposing .pointer and .shape.
            if tuple(out.shape) != (t.size, n):
                raise ValueError(f"out has shape {out.shape}, need {(t.size, n)}.")
            pointer, flags = out.pointer, flags | OUT_DEVICE
        else:
            if out is None:
                # Page-locked and recycled: the copy back runs at the rate of the host link.
                out = self.host_array((t.size, max(n, 0)))
                if accumulate:
                    out[...] = 0.
            if out.shape != (t.size, n) or out.dtype != np.float64 or \
                    not out.flags["C_CONTIGUOUS"]:
                raise ValueError("out must be C-contiguous float64[levels, n].")
            pointer = c_void_p(out.ctypes.data)
        if deliver is not None:
            if not (flags & OUT_DEVICE) or want_evals:
                raise ValueError("deliver needs a device `out` (and no eval count).")
            if deliver.ndim != 2 or deliver.shape[0] != t.size or deliver.dtype != np.float64 \
                    or deliver.strides[1] != 8 or deliver.shape[1] > n:
                raise ValueError("deliver must be float64[levels, columns <= n], rows contiguous.")
            self._check(self.lib.lbl_compute_streamed(
                self.handle, int(molecule), t.size, t.ctypes.data, p.ctypes.data, x.ctypes.data,
                int(v0), int(vn), int(n_per_v), int(cut_off), 1 if remove_pedestal else 0,
                RANGE_POLICIES[range_policy], flags, pointer, 0, c_void_p(deliver.ctypes.data),
                int(deliver.strides[0]) if t.size > 1 else max(int(deliver.strides[0]),
                                                               8*deliver.shape[1]),
                int(deliver.shape[1]), int(pieces)))
            return out
        evals = c_int64(0)
        self._check(self.lib.lbl_compute(
            self.handle, int(molecule), t.size, t.ctypes.data, p.ctypes.data, x.ctypes.data,
            int(v0), int(vn), int(n_per_v), int(cut_off), 1 if remove_pedestal else 0,
            RANGE_POLICIES[range_policy], flags, pointer, 0,
            byref(evals) if want_evals else None))
        return (out, evals.value) if want_evals else out

    def fill_zero(self, out, asynchronous=False):
        """Zeroes a [levels, n] output (host array or DeviceSpectra): the spectrum the
        reference returns for a molecule it has nothing to compute for (absorption.c:41)."""
        if hasattr(out, "pointer"):
            self._check(self.lib.lbl_fill_zero(
                self.handle, out.pointer, int(out.shape[0]), int(out.shape[1]), 0,
                OUT_DEVICE | (ASYNC if asynchronous else 0)))
        else:
            out[...] = 0.
        return out

    def line_scalars(self, molecule, num_lines, temperature, pressure, vmr, v0, vn, n_per_v,
                     cut_off=25, range_policy="reference"):
        """Per-line derived scalars in reference row order (see lbl_line_scalars)."""
        derived = np.zeros((max(int(num_lines), 1), 8), dtype=np.float64)
        self._check(self.lib.lbl_line_scalars(
            self.handle, int(molecule), float(temperature), float(pressure), float(vmr),
            int(v0), int(vn), int(n_per_v), int(cut_off), 0, RANGE_POLICIES[range_policy],
            derived.ctypes.data))
        return derived[:int(num_lines)]

    def finish_deferred(self):
        """Queues what a call with defer_finish=True kept back."""
        self._check(self.lib.lbl_finish_deferred(self.handle))

    def deferred(self):
        """True while a call is kept back (False right after a call whose defer_finish could
        not be honoured: no pedestal pass, several level passes, host output)."""
        return bool(self.lib.lbl_deferred(self.handle))

    def cancel_deferred(self):
        """Drops what a call with defer_finish=True kept back: its `out` block and `deliver`
        array are never written by it (for callers that fail before finish_deferred())."""
        self._check(self.lib.lbl_cancel_deferred(self.handle))

    def synchronize(self):
        self._check(self.lib.lbl_synchronize(self.handle))

    # -- continua (slot 1) -----------------------------------------------------------------
    def load_continuum(self, bands):
        """Uploads a list of bands, each (kind, lower_bound, resolution, [columns]); returns
        the continuum handle."""
        if not 1 <= len(bands) <= MAX_BANDS:
            raise ValueError(f"a continuum has 1 to {MAX_BANDS} bands.")
        descriptors = (BandDescriptor*len(bands))()
        pieces, offset = [], 0
        for d, (kind, lower, resolution, columns) in zip(descriptors, bands):
            columns = [_f64(c) for c in columns]
            size = columns[0].size
            if any(c.shape != (size,) for c in columns) or len(columns) > 4:
                raise ValueError("the columns of a band must be 1-d and equally long (<= 4).")
            d.kind, d.size, d.lower_bound, d.resolution = int(kind), size, float(lower), \
                float(resolution)
            for i in range(4):
                d.column[i] = -1
            for i, c in enumerate(columns):
                d.column[i] = offset
                offset += size
                pieces.append(c)
        table = _f64(np.concatenate(pieces))
        handle = c_int32(-1)
        self._check(self.lib.lbl_continuum_load(self.handle, len(bands), descriptors,
                                                table.ctypes.data, table.size, byref(handle)))
        return handle.value

    def free_continuum(self, continuum):
        self._check(self.lib.lbl_continuum_free(self.handle, int(continuum)))

    def load_grid(self, wavenumber):
        """Uploads a spectral grid [cm-1]; returns the grid handle."""
        grid = _f64(wavenumber)
        if grid.ndim != 1 or grid.size < 1:
            raise ValueError("the grid must be a non-empty 1-d array.")
        handle = c_int32(-1)
        self._check(self.lib.lbl_grid_load(self.handle, grid.size, grid.ctypes.data,
                                           byref(handle)))
        return handle.value

    def free_grid(self, grid):
        self._check(self.lib.lbl_grid_free(self.handle, int(grid)))

    def continuum_compute(self, continuum, grid, n, temperature, pressure, vmr, out=None,
                          accumulate=False, asynchronous=False):
        """Continuum extinction [m-1]: float64[levels, n] (or fills `out`, host array or
        DeviceSpectra).  vmr is [levels, VMR_COUNT]; pressure in Pa."""
        t, p, flags = _slot_levels(temperature, pressure, accumulate, asynchronous)
        x = _f64(vmr).reshape(-1, VMR_COUNT)
        if not (t.ndim == 1 and t.shape == p.shape and x.shape[0] == t.size):
            raise ValueError("temperature, pressure [levels] and vmr [levels, 5] disagree.")
        out, pointer, flags, stride = self._output(out, t.size, n, flags)
        self._check(self.lib.lbl_continuum_compute(
            self.handle, int(continuum), int(grid), t.size, t.ctypes.data, p.ctypes.data,
            x.ctypes.data, flags, pointer, stride))
        return out

    def path_compute(self, beta, columns, n_paths, levels_per_path, level_begin, lengths, carry,
                     optical_depth=None, transmittance=None, band_start=None, cumulative=False,
                     from_last=False, asynchronous=False):
        """Optical depth / transmittance along paths through the DeviceSpectra `beta` (its rows
        are the flat levels level_begin, level_begin + 1, ... of n_paths paths of levels_per_path
        levels; `lengths` [m] one per row) -- lbl_path_compute.  carry: DeviceSpectra
        [n_paths, >= beta's row length] holding each path's running tau between runs.
        optical_depth / transmittance: DeviceSpectra outputs (None: not wanted) --
        [n_paths or rows, row length] without bands, [n_paths or rows, bands] with them.
        band_start: int64 column starts of the bands (n_bands + 1 values) or None."""
        rows, stride, lengths = _per_row(beta, "one path length per row of beta.", lengths)
        if tuple(carry.shape) != (int(n_paths), stride):
            raise ValueError("carry must be [n_paths, row length of beta].")
        starts, n_bands, flags = _path_run(band_start, level_begin, rows, levels_per_path,
                                           from_last, asynchronous)
        flags |= (PATH_OPTICAL_DEPTH if optical_depth is not None else 0) | \
                 (PATH_TRANSMITTANCE if transmittance is not None else 0) | \
                 (PATH_CUMULATIVE if cumulative else 0)
        _check_outputs((optical_depth, transmittance), rows if cumulative else int(n_paths),
                       n_bands if n_bands > 0 else stride)
        self._check(self.lib.lbl_path_compute(
            self.handle, beta.pointer, stride, int(columns), int(n_paths), int(levels_per_path),
            int(level_begin), rows, lengths.ctypes.data, n_bands, _address(starts), carry.pointer,
            _address(optical_depth), _address(transmittance), flags))

    def band_distribution(self, values, columns, band_start, scratch=None, interval_start=None,
                          means=None, point_index=None, point_fraction=None, quantiles=None,
                          asynchronous=False):
        """Sorts every band of every row of the DeviceSpectra `values` in place, ascending in the
        total order of lbl_band_distribution (the fp64 bits as integer keys), and forms what a
        k-distribution stores of the sorted rows.  band_start: int64 column starts of the bands
        (n_bands + 1 values).  scratch: a DeviceSpectra shaped like `values` (None is enough while
        no band is longer than 4096 columns).  interval_start (int64, n_intervals + 1 column
        starts) with means (DeviceSpectra [rows, n_intervals]): the arithmetic mean of the sorted
        row over each interval of columns.  point_index (int64) and point_fraction, both
        [n_bands, n_points], with quantiles (DeviceSpectra [rows, n_bands*n_points]):
        k_i + f*(k_min(i+1, N-1) - k_i) of each sorted band; NaN where i < 0."""
        rows, stride = int(values.shape[0]), int(values.shape[1])
        starts = np.ascontiguousarray(band_start, dtype=np.int64)
        if starts.ndim != 1 or starts.size < 2:
            raise ValueError("band_start must hold n_bands + 1 >= 2 column starts.")
        n_bands = starts.size - 1
        if scratch is not None and tuple(scratch.shape) != (rows, stride):
            raise ValueError("scratch must be shaped like values.")
        intervals, n_intervals = _interval_table(interval_start, (means,), rows)
        index, fraction, n_points = _point_tables(point_index, point_fraction, quantiles, rows,
                                                  n_bands)
        self._check(self.lib.lbl_band_distribution(
            self.handle, values.pointer, stride, int(columns), rows, starts.ctypes.data, n_bands,
            _address(scratch), _address(intervals), n_intervals, _address(means),
            _address(index), _address(fraction), n_points, _address(quantiles),
            ASYNC if asynchronous else 0))

    def band_distribution_weighted(self, values, columns, band_start, index_rows, scratch=None,
                                   index_scratch=None, index_stride=None, grid=-1,
                                   row_temperature=None, weight_row=None, weight_rows=None,
                                   weighted_rows=None, interval_start=None, weight_sums=None,
                                   weighted_sums=None, means=None, point_index=None,
                                   point_fraction=None, quantiles=None, asynchronous=False):
        """band_distribution with the permutation kept and weights carried through it --
        lbl_band_distribution_weighted.  values, columns, band_start, scratch, interval_start,
        means, point_index, point_fraction and quantiles as for band_distribution, with the same
        bits.  index_rows: where pi goes, as int32 [rows, index_stride], column band start + i
        holding the offset in its band of the column that the sorted value i came from
        (numpy.argsort(keys, kind="stable")); index_scratch: shaped like it (with scratch: None is
        enough while no band is longer than 4096 columns).  Both are blocks that hold
        rows*index_stride int32 values from their `pointer`; index_stride None: DeviceSpectra
        [rows, m] read as int32 [rows, 2 m].  The weights, exactly one of: row_temperature [K]
        one per row with grid, a handle of load_grid -- w = B(nu, T) -- or weight_row, a
        DeviceSpectra whose first row holds w on the columns.  weight_rows / weighted_rows:
        DeviceSpectra shaped like values (both or neither) for W_i = w_pi(i) and W_i*k_i;
        weight_sums / weighted_sums: DeviceSpectra [rows, n_intervals] for their sums over each
        interval of columns (they need weight_rows and weighted_rows)."""
        rows, stride = int(values.shape[0]), int(values.shape[1])
        starts = np.ascontiguousarray(band_start, dtype=np.int64)
        if starts.ndim != 1 or starts.size < 2:
            raise ValueError("band_start must hold n_bands + 1 >= 2 column starts.")
        n_bands = starts.size - 1
        for block in (scratch, weight_rows, weighted_rows):
            if block is not None and tuple(block.shape) != (rows, stride):
                raise ValueError("scratch, weight_rows and weighted_rows must be shaped like "
                                 "values.")
        if index_stride is None:
            index_stride = 2*int(index_rows.shape[1])
        for block in (index_rows, index_scratch):
            if block is not None and (int(block.shape[0]) < rows or
                                      tuple(block.shape) != tuple(index_rows.shape)):
                raise ValueError("index_rows and index_scratch must be shaped alike, one row "
                                 "per row of values.")
        if (row_temperature is None) == (weight_row is None):
            raise ValueError("exactly one of row_temperature and weight_row must be given.")
        temperature = None
        if row_temperature is not None:
            temperature = _f64(row_temperature)
            if temperature.shape != (rows,):
                raise ValueError("one temperature per row of values.")
        elif int(weight_row.shape[1]) < int(columns):
            raise ValueError("weight_row must hold `columns` values.")
        intervals, n_intervals = _interval_table(interval_start,
                                                 (weight_sums, weighted_sums, means), rows)
        index, fraction, n_points = _point_tables(point_index, point_fraction, quantiles, rows,
                                                  n_bands)
        self._check(self.lib.lbl_band_distribution_weighted(
            self.handle, values.pointer, stride, int(columns), rows, starts.ctypes.data, n_bands,
            _address(scratch), int(grid), _address(temperature), _address(weight_row),
            index_rows.pointer, _address(index_scratch), int(index_stride),
            _address(weight_rows), _address(weighted_rows), _address(intervals), n_intervals,
            _address(weight_sums), _address(weighted_sums), _address(means), _address(index),
            _address(fraction), n_points, _address(quantiles), ASYNC if asynchronous else 0))

    def path_radiance(self, beta, columns, grid, n_paths, levels_per_path, level_begin, lengths,
                      temperature, carry, boundary_temperature=None, boundary_emissivity=None,
                      radiance=None, brightness_temperature=None, band_start=None,
                      cumulative=False, from_last=False, asynchronous=False,
                      edge_temperature=None, emissivity_rows=None, reflection=None):
        """Thermal emission along paths through the DeviceSpectra `beta` -- lbl_path_radiance.
        Rows, lengths, carry, band_start, cumulative, from_last and asynchronous as for
        path_compute; grid: handle of load_grid (the wavenumbers of the columns); temperature
        [K] one per row; boundary_temperature [K] (0: none) / boundary_emissivity one per path
        (None: no boundary / 1).  radiance / brightness_temperature: DeviceSpectra outputs (None:
        not wanted), shaped as path_compute's.  edge_temperature: None (isothermal layers), or
        [rows, 2] interface temperatures [K] -- [r, 0] on the first-level side of row r, [r, 1]
        on the last-level side, continuous within a path -- for the linear-in-tau source
        (lbl_path_radiance_source).  emissivity_rows / reflection: None, or DeviceSpectra
        [n_paths, row length of beta] read where a path starts behind a boundary -- E per column
        (surface_emissivity's rows) in place of boundary_emissivity, and D, the radiance that
        arrives at the boundary: the path starts from E*B(nu, T_b) + (1. - E)*D
        (lbl_path_radiance_surface; with both None the call is lbl_path_radiance_source's)."""
        rows, stride, lengths, temperature = _per_row(
            beta, "one path length and one temperature per row of beta.", lengths, temperature)
        if tuple(carry.shape) != (int(n_paths), stride):
            raise ValueError("carry must be [n_paths, row length of beta].")
        for name, block in (("emissivity_rows", emissivity_rows), ("reflection", reflection)):
            if block is not None and tuple(block.shape) != (int(n_paths), stride):
                raise ValueError(f"{name} must be [n_paths, row length of beta].")
        edge_temperature = _edge_rows(edge_temperature, rows)
        boundary = _per_path(n_paths, "one boundary value per path.", boundary_temperature,
                             boundary_emissivity)
        starts, n_bands, flags = _path_run(band_start, level_begin, rows, levels_per_path,
                                           from_last, asynchronous)
        flags |= (PATH_RADIANCE if radiance is not None else 0) | \
                 (PATH_BRIGHTNESS if brightness_temperature is not None else 0) | \
                 (PATH_CUMULATIVE if cumulative else 0)
        _check_outputs((radiance, brightness_temperature),
                       rows if cumulative else int(n_paths), n_bands if n_bands > 0 else stride)
        arguments = (
            self.handle, beta.pointer, stride, int(columns), int(grid), int(n_paths),
            int(levels_per_path), int(level_begin), rows, lengths.ctypes.data,
            temperature.ctypes.data, _address(edge_temperature), *map(_address, boundary),
            n_bands, _address(starts), carry.pointer, _address(radiance),
            _address(brightness_temperature), flags)
        if emissivity_rows is None and reflection is None:
            self._check(self.lib.lbl_path_radiance_source(*arguments))
        else:
            self._check(self.lib.lbl_path_radiance_surface(
                *arguments, _address(emissivity_rows), _address(reflection)))

    def surface_emissivity(self, grid, rows, knot_wavenumber, knot_emissivity, path_begin=0,
                           asynchronous=False):
        """Fills rows path_begin, path_begin + 1, ... of the DeviceSpectra `rows` [n_paths, row
        length] with the emissivity of each path on the grid (handle of load_grid) --
        lbl_surface_emissivity: knot_emissivity [paths of the call, M] at the knots
        knot_wavenumber [M] (strictly ascending, 2 <= M <= 1024), interpolated like numpy.interp:
        for k_j <= nu < k_{j+1}, E = e_j + (nu - k_j)*((e_{j+1} - e_j)/(k_{j+1} - k_j)); E = e_0
        for nu <= k_0 and E = e_{M-1} for nu >= k_{M-1}."""
        knots = _f64(knot_wavenumber)
        values = _f64(knot_emissivity)
        if knots.ndim != 1 or values.ndim != 2 or values.shape[1] != knots.size or \
                values.shape[0] < 1:
            raise ValueError("knot_wavenumber must be [M] and knot_emissivity [paths, M].")
        self._check(self.lib.lbl_surface_emissivity(
            self.handle, int(grid), int(rows.shape[0]), int(path_begin), values.shape[0],
            knots.size, knots.ctypes.data, values.ctypes.data, rows.pointer, int(rows.shape[1]),
            ASYNC if asynchronous else 0))

    def path_jacobian(self, beta, columns, grid, n_paths, levels_per_path, level_begin, lengths,
                      temperature, work, boundary_temperature=None, boundary_emissivity=None,
                      radiance=None, optical_depth_jacobian=None,
                      log_optical_depth_jacobian=None, temperature_jacobian=None,
                      boundary_temperature_jacobian=None, boundary_emissivity_jacobian=None,
                      band_start=None, from_last=False, asynchronous=False):
        """Analytic radiance Jacobians along whole paths through the DeviceSpectra `beta` --
        lbl_path_jacobian.  Rows (whole paths), lengths, temperature, grid, the boundary values,
        band_start, from_last and asynchronous as for path_radiance.  Outputs (DeviceSpectra,
        None: not wanted): the three per-level Jacobians [rows, row length], radiance and the
        two boundary Jacobians [n_paths, row length]; with bands [rows or n_paths, bands].
        work: DeviceSpectra [>= rows, row length] without bands (optical_depth_jacobian or
        log_optical_depth_jacobian may be it), with bands [>= max(P, 1)*rows + Q*paths of the
        run, row length] for P per-level and Q per-path outputs."""
        rows, stride, lengths, temperature = _per_row(
            beta, "one path length and one temperature per row of beta.", lengths, temperature)
        boundary = _per_path(n_paths, "one boundary value per path.", boundary_temperature,
                             boundary_emissivity)
        starts, n_bands, flags = _path_run(band_start, level_begin, rows, levels_per_path,
                                           from_last, asynchronous)
        given = dict(radiance=radiance, optical_depth_jacobian=optical_depth_jacobian,
                     log_optical_depth_jacobian=log_optical_depth_jacobian,
                     temperature_jacobian=temperature_jacobian,
                     boundary_temperature_jacobian=boundary_temperature_jacobian,
                     boundary_emissivity_jacobian=boundary_emissivity_jacobian)
        width = n_bands if n_bands > 0 else stride
        work_rows, run_paths = rows, -(-rows//int(levels_per_path))
        if n_bands > 0:
            per_level = sum(given[q] is not None for q in PATH_JACOBIAN_PER_LEVEL)
            per_path = sum(out is not None for out in given.values()) - per_level
            work_rows = max(per_level, 1)*rows + per_path*run_paths
        if work.shape[1] != stride or work.shape[0] < work_rows:
            raise ValueError(f"work has shape {work.shape}, need {work_rows} x {stride}.")
        pointers = []
        for name, flag in PATH_JACOBIAN_OUTPUTS:
            out = given[name]
            pointers.append(_address(out))
            if out is None:
                continue
            flags |= flag
            need = rows if name in PATH_JACOBIAN_PER_LEVEL else int(n_paths)
            if out.shape[1] != width or out.shape[0] < need:
                raise ValueError(f"{name} has shape {out.shape}, need {need} x {width}.")
        self._check(self.lib.lbl_path_jacobian(
            self.handle, beta.pointer, stride, int(columns), int(grid), int(n_paths),
            int(levels_per_path), int(level_begin), rows, lengths.ctypes.data,
            temperature.ctypes.data, *map(_address, boundary), n_bands, _address(starts),
            work.pointer, *pointers, flags))

    def instrument_create(self, grid, shape, centers, parameter=None, half_width=None,
                          offsets=None, response=None):
        """Binds an instrument (pylbl_amd.instrument: its shape code, centres [N] and per-channel
        parameter / half_width [N], or the offsets [K] and response [K] or [N, K] of a table) to
        the grid handle `grid` -- lbl_instrument_create.  Returns the instrument handle."""
        centers = _f64(np.atleast_1d(centers))
        arrays = [None if x is None else _f64(x) for x in (parameter, half_width, offsets,
                                                            response)]
        parameter, half_width, offsets, response = arrays
        n_table = 0 if offsets is None else offsets.size
        rows = 0 if response is None else (1 if response.ndim == 1 else response.shape[0])
        handle = c_int32(-1)
        self._check(self.lib.lbl_instrument_create(
            self.handle, int(grid), int(shape), centers.size, centers.ctypes.data,
            _address(parameter), _address(half_width), n_table, _address(offsets),
            _address(response), rows, byref(handle)))
        self._instrument_channels[handle.value] = centers.size
        return handle.value

    def instrument_free(self, instrument):
        self._check(self.lib.lbl_instrument_free(self.handle, int(instrument)))
        self._instrument_channels.pop(int(instrument), None)

    def instrument_apply(self, values, rows, instrument, out, transmittance=False,
                         asynchronous=False):
        """out[r][c] = channel c's weighted mean of row r of the DeviceSpectra `values` (of
        exp(-value) with `transmittance`) for its first `rows` rows -- lbl_instrument_apply.
        out: DeviceSpectra [>= rows, channels]: the kernel writes row r at out + r*channels, so
        for a handle of instrument_create any other width is refused."""
        rows = int(rows)
        if not 0 < rows <= values.shape[0] or out.shape[0] < rows:
            raise ValueError(f"{rows} rows of values {values.shape} into {out.shape}.")
        channels = self._instrument_channels.get(int(instrument))
        if channels is not None and out.shape[1] != channels:
            raise ValueError(f"out has shape {out.shape}, need rows x {channels} channels.")
        flags = (PATH_TRANSMITTANCE if transmittance else 0) | (ASYNC if asynchronous else 0)
        self._check(self.lib.lbl_instrument_apply(
            self.handle, values.pointer, int(values.shape[1]), rows, int(instrument), flags,
            out.pointer))

    def path_flux(self, beta, columns, grid, n_paths, levels_per_path, level_begin, lengths,
                  weight, temperature, carry, reflection, level_flux, surface_temperature=None,
                  surface_emissivity=None, flux=None, surface_flux=None, band_start=None,
                  up=False, from_last=False, asynchronous=False, edge_temperature=None):
        """One sweep of K angles through the DeviceSpectra `beta` -- lbl_path_flux.  Rows,
        columns, grid, temperature, band_start, from_last and asynchronous as for path_radiance;
        lengths [rows, K]: s_l/mu_k [m]; weight [K]; carry [n_paths*K, row length];
        reflection [n_paths, row length]; level_flux [>= rows, row length] (F after each level);
        surface_temperature / surface_emissivity one per path (up sweep); flux [>= rows, bands]
        and, up, surface_flux [n_paths, bands]: the band means (with band_start only).
        edge_temperature: as for path_radiance (lbl_path_flux_source)."""
        lengths = _f64(lengths)
        weight = _f64(np.atleast_1d(weight))
        temperature = _f64(np.atleast_1d(temperature))
        rows, stride = int(beta.shape[0]), int(beta.shape[1])
        angles = weight.size
        if weight.ndim != 1 or lengths.shape != (rows, angles) or temperature.shape != (rows,):
            raise ValueError("lengths [rows, K], weight [K] and temperature [rows] disagree.")
        if tuple(carry.shape) != (int(n_paths)*angles, stride) or \
                tuple(reflection.shape) != (int(n_paths), stride):
            raise ValueError("carry must be [n_paths*K, row length], reflection [n_paths, "
                             "row length].")
        if level_flux.shape[1] != stride or level_flux.shape[0] < rows:
            raise ValueError(f"level_flux has shape {level_flux.shape}, need rows x {stride}.")
        surface = _per_path(n_paths, "one surface value per path.", surface_temperature,
                            surface_emissivity)
        starts, n_bands, flags = _path_run(band_start, level_begin, rows, levels_per_path,
                                           from_last, asynchronous)
        for out, count in ((flux, rows), (surface_flux, int(n_paths))):
            if out is not None and (out.shape[1] != n_bands or out.shape[0] < count):
                raise ValueError(f"a band output has shape {out.shape}, need {count} x {n_bands}.")
        flags |= PATH_FLUX_UP if up else 0
        edge_temperature = _edge_rows(edge_temperature, rows)
        self._check(self.lib.lbl_path_flux_source(
            self.handle, beta.pointer, stride, int(columns), int(grid), int(n_paths),
            int(levels_per_path), int(level_begin), rows, angles, lengths.ctypes.data,
            weight.ctypes.data, temperature.ctypes.data, _address(edge_temperature),
            *map(_address, surface), n_bands, _address(starts), carry.pointer,
            reflection.pointer, level_flux.pointer, _address(flux), _address(surface_flux),
            flags))

    def solar_spectrum(self, grid, row, columns, irradiance=None, wavenumber=None,
                       temperature=0., scale=1., asynchronous=False):
        """Fills the first `columns` values of the DeviceSpectra `row` (its first row) with the
        solar irradiance S on the grid (handle of load_grid) -- lbl_solar_spectrum: with
        irradiance None scale*B(nu, temperature); with irradiance [columns] and wavenumber None
        scale*irradiance; with wavenumber [M] (strictly ascending, 2 <= M <= 2**22) and
        irradiance [M] scale times the table interpolated as surface_emissivity does."""
        knots = None if wavenumber is None else _f64(wavenumber)
        values = None if irradiance is None else _f64(irradiance)
        if values is None and knots is not None:
            raise ValueError("wavenumber without irradiance.")
        if values is not None and (values.ndim != 1 or
                                   (knots is not None and knots.shape != values.shape)):
            raise ValueError("irradiance must be [columns], or [M] with wavenumber [M].")
        if not 0 < int(columns) <= int(row.shape[1]):
            raise ValueError(f"{columns} columns into a row of {row.shape[1]}.")
        self._check(self.lib.lbl_solar_spectrum(
            self.handle, int(grid), int(columns), 0 if values is None else values.size,
            _address(knots), _address(values), float(temperature), float(scale), row.pointer,
            ASYNC if asynchronous else 0))

    def path_solar(self, beta, columns, n_paths, levels_per_path, level_begin, solar_lengths,
                   solar_zenith_cosine, solar_row, carry, view_lengths=None, albedo=None,
                   albedo_rows=None, interface_rows=None, space_rows=None, surface_rows=None,
                   reflected_rows=None, interface_mean=None, space_mean=None, surface_mean=None,
                   reflected_mean=None, band_start=None, from_last=False, asynchronous=False):
        """The direct solar beam and the reflected sunlight along paths through the DeviceSpectra
        `beta` -- lbl_path_solar.  Rows, columns, band_start, from_last and asynchronous as for
        path_compute: the sweep runs from space to the surface.  solar_lengths / view_lengths [m]
        one per row (view_lengths None: no viewer); solar_zenith_cosine one per path; solar_row:
        DeviceSpectra whose first row holds S (solar_spectrum's); carry [2*n_paths, row length]:
        tau and tv of each path; albedo one per path or albedo_rows [n_paths, row length] (with
        view_lengths, one of them).  Outputs (DeviceSpectra, None: not wanted): interface_rows
        [>= rows, row length], space_rows, surface_rows and reflected_rows [n_paths, row length];
        with band_start their band means interface_mean [>= rows, bands], space_mean,
        surface_mean and reflected_mean [n_paths, bands]."""
        rows, stride, solar_lengths = _per_row(beta, "one solar length per row of beta.",
                                               solar_lengths)
        if view_lengths is not None:
            _, _, view_lengths = _per_row(beta, "one view length per row of beta.", view_lengths)
        if tuple(carry.shape) != (2*int(n_paths), stride):
            raise ValueError("carry must be [2*n_paths, row length of beta].")
        if solar_row.shape[1] < int(columns):
            raise ValueError(f"solar_row has {solar_row.shape[1]} values, need {columns}.")
        mu0, albedo = _per_path(n_paths, "one cosine and one albedo per path.",
                                solar_zenith_cosine, albedo)
        starts, n_bands, flags = _path_run(band_start, level_begin, rows, levels_per_path,
                                           from_last, asynchronous)
        per_path = (albedo_rows, space_rows, surface_rows, reflected_rows)
        if any(x is not None and tuple(x.shape) != (int(n_paths), stride) for x in per_path):
            raise ValueError("albedo_rows, space_rows, surface_rows and reflected_rows must be "
                             "[n_paths, row length of beta].")
        _check_outputs((interface_rows,), rows, stride)
        _check_outputs((interface_mean,), rows, n_bands)
        _check_outputs((space_mean, surface_mean, reflected_mean), int(n_paths), n_bands)
        self._check(self.lib.lbl_path_solar(
            self.handle, beta.pointer, stride, int(columns), int(n_paths), int(levels_per_path),
            int(level_begin), rows, solar_lengths.ctypes.data, _address(view_lengths),
            _address(mu0), solar_row.pointer, _address(albedo_rows), _address(albedo), n_bands,
            _address(starts), carry.pointer, _address(interface_rows), _address(space_rows),
            _address(surface_rows), _address(reflected_rows), _address(interface_mean),
            _address(space_mean), _address(surface_mean), _address(reflected_mean), flags))

    def rayleigh_row(self, grid, row, columns, cross_section=None, asynchronous=False):
        """Fills the first `columns` values of the DeviceSpectra `row` (its first row) with the
        Rayleigh scattering cross-section sigma [m2] on the grid (handle of load_grid) --
        lbl_rayleigh_row: the Bucholtz (1995) fit, or cross_section [columns] (finite and >= 0)
        as it is."""
        values = None if cross_section is None else _f64(cross_section)
        if values is not None and values.shape != (int(columns),):
            raise ValueError(f"cross_section has shape {values.shape}, need [{int(columns)}].")
        if not 0 < int(columns) <= int(row.shape[1]):
            raise ValueError(f"{columns} columns into a row of {row.shape[1]}.")
        self._check(self.lib.lbl_rayleigh_row(
            self.handle, int(grid), int(columns), _address(values), row.pointer,
            ASYNC if asynchronous else 0))

    def path_two_stream(self, beta, columns, n_paths, levels_per_path, level_begin, level_table,
                        solar_zenith_cosine, solar_row, work, rayleigh_row=None, albedo=None,
                        albedo_rows=None, band_start=None, from_last=False, asynchronous=False,
                        **outputs):
        """Two-stream shortwave fluxes at every interface of the whole paths in the DeviceSpectra
        `beta` -- lbl_path_two_stream.  Rows (whole paths), columns, band_start and asynchronous
        as for path_jacobian; from_last: the surface lies behind level 0 of each path.
        level_table [rows, 5]: s_l, c_l, tau_c, w_c, h_c of each row; solar_zenith_cosine one
        per path; solar_row / rayleigh_row: DeviceSpectra whose first rows hold S and sigma
        (rayleigh_row None: no Rayleigh scattering); albedo one per path or albedo_rows [n_paths,
        row length], one of them; work [>= 2*rows, row length].  Outputs (DeviceSpectra
        keywords, None: not wanted), named PATH_TWO_STREAM_OUTPUTS: up_rows, down_rows,
        direct_rows and diffuse_rows [>= rows, row length] at the interface below each level,
        the four top_*_rows [n_paths, row length] at interface 0, and with band_start their band
        means *_mean [>= rows or n_paths, bands]."""
        self._path_two_stream("path_two_stream", beta, columns, n_paths, levels_per_path,
                              level_begin, level_table, None, solar_zenith_cosine, solar_row,
                              work, rayleigh_row, albedo, albedo_rows, band_start, from_last,
                              asynchronous, outputs)

    def path_two_stream_spectral(self, beta, columns, grid, n_paths, levels_per_path, level_begin,
                                 level_table, knot_wavenumber, knot_optics, solar_zenith_cosine,
                                 solar_row, work, rayleigh_row=None, albedo=None, albedo_rows=None,
                                 band_start=None, from_last=False, asynchronous=False, **outputs):
        """path_two_stream with the scatterer of every level as a table over wavenumber --
        lbl_path_two_stream_spectral.  grid as for path_flux; knot_wavenumber [M] and knot_optics
        [rows, M, 3]: tau_c, omega_c and g_c of each row at every knot, interpolated onto the
        grid; tau_c, w_c and h_c of level_table are 0; everything else as for path_two_stream."""
        rows = int(beta.shape[0])
        self._path_two_stream("path_two_stream_spectral", beta, columns, n_paths, levels_per_path,
                              level_begin, level_table,
                              (int(grid),) + _knot_table(knot_wavenumber, knot_optics, rows),
                              solar_zenith_cosine, solar_row, work, rayleigh_row, albedo,
                              albedo_rows, band_start, from_last, asynchronous, outputs)

    def _path_two_stream(self, name, beta, columns, n_paths, levels_per_path, level_begin,
                         level_table, spectral, solar_zenith_cosine, solar_row, work,
                         rayleigh_row, albedo, albedo_rows, band_start, from_last, asynchronous,
                         outputs):
        """The call of path_two_stream (spectral None) and of path_two_stream_spectral (spectral:
        grid, knots, optics, M): lbl_<name>."""
        rows, stride, table, starts, n_bands, flags = _whole_paths(
            beta, level_table, n_paths, albedo_rows, "albedo_rows", band_start, level_begin,
            levels_per_path, from_last, asynchronous, work)
        if solar_row.shape[1] < int(columns) or \
                (rayleigh_row is not None and rayleigh_row.shape[1] < int(columns)):
            raise ValueError(f"solar_row and rayleigh_row need {columns} values.")
        mu0, albedo = _per_path(n_paths, "one cosine and one albedo per path.",
                                solar_zenith_cosine, albedo)
        pointers = _output_pointers(name, PATH_TWO_STREAM_OUTPUTS, outputs, rows, n_paths, stride,
                                    n_bands)
        knots = []
        if spectral is not None:
            grid, knot, optics, n_knots = spectral
            knots = [grid, n_knots, knot.ctypes.data, optics.ctypes.data]
        self._check(getattr(self.lib, "lbl_" + name)(
            self.handle, beta.pointer, stride, int(columns), int(n_paths), int(levels_per_path),
            int(level_begin), rows, table.ctypes.data, *knots, _address(mu0), solar_row.pointer,
            _address(rayleigh_row), _address(albedo_rows), _address(albedo), n_bands,
            _address(starts), work.pointer, *pointers, flags))

    def path_thermal_two_stream(self, beta, columns, grid, n_paths, levels_per_path, level_begin,
                                level_table, surface_temperature, work, diffusivity=1.66,
                                emissivity=None, emissivity_rows=None, band_start=None,
                                from_last=False, asynchronous=False, **outputs):
        """Two-stream longwave fluxes at every interface of the whole paths in the DeviceSpectra
        `beta` -- lbl_path_thermal_two_stream.  Rows (whole paths), columns, band_start,
        from_last and asynchronous as for path_two_stream; grid as for path_flux.
        level_table [rows, 5]: s_l, tau_c, w_c, g_c, T_l of each row; diffusivity: D in [1, 2];
        surface_temperature one per path; emissivity one per path or emissivity_rows [n_paths,
        row length], one of them; work [>= 2*rows, row length].  Outputs (DeviceSpectra
        keywords, None: not wanted), named PATH_THERMAL_OUTPUTS: up_rows and down_rows [>= rows,
        row length] at the interface below each level, top_up_rows and top_down_rows [n_paths,
        row length] at interface 0, and with band_start their band means *_mean [>= rows or
        n_paths, bands]."""
        self._path_thermal("path_thermal_two_stream", beta, columns, grid, n_paths,
                           levels_per_path, level_begin, level_table, None, surface_temperature,
                           work, diffusivity, emissivity, emissivity_rows, band_start, from_last,
                           asynchronous, outputs)

    def path_thermal_two_stream_source(self, beta, columns, grid, n_paths, levels_per_path,
                                       level_begin, level_table, edge_temperature,
                                       surface_temperature, work, diffusivity=1.66,
                                       emissivity=None, emissivity_rows=None, band_start=None,
                                       from_last=False, asynchronous=False, **outputs):
        """path_thermal_two_stream with the linear-in-tau source --
        lbl_path_thermal_two_stream_source.  edge_temperature [rows, 2]: the interface
        temperatures of each row on its first-level and its last-level side [K], as for
        path_flux; everything else as for path_thermal_two_stream."""
        if edge_temperature is None:
            raise ValueError("path_thermal_two_stream_source needs edge_temperature.")
        self._path_thermal("path_thermal_two_stream_source", beta, columns, grid, n_paths,
                           levels_per_path, level_begin, level_table, edge_temperature,
                           surface_temperature, work, diffusivity, emissivity, emissivity_rows,
                           band_start, from_last, asynchronous, outputs)

    def path_thermal_two_stream_spectral(self, beta, columns, grid, n_paths, levels_per_path,
                                         level_begin, level_table, knot_wavenumber, knot_optics,
                                         surface_temperature, work, edge_temperature=None,
                                         diffusivity=1.66, emissivity=None, emissivity_rows=None,
                                         band_start=None, from_last=False, asynchronous=False,
                                         **outputs):
        """path_thermal_two_stream (edge_temperature None) or path_thermal_two_stream_source with
        the scatterer of every level as a table over wavenumber --
        lbl_path_thermal_two_stream_spectral.  knot_wavenumber [M] and knot_optics [rows, M, 3]:
        tau_c, omega_c and g_c of each row at every knot, interpolated onto the grid; tau_c, w_c
        and g_c of level_table are 0; everything else as for those two."""
        rows = int(beta.shape[0])
        self._path_thermal("path_thermal_two_stream_spectral", beta, columns, grid, n_paths,
                           levels_per_path, level_begin, level_table, edge_temperature,
                           surface_temperature, work, diffusivity, emissivity, emissivity_rows,
                           band_start, from_last, asynchronous, outputs,
                           spectral=_knot_table(knot_wavenumber, knot_optics, rows))

    def _path_thermal(self, name, beta, columns, grid, n_paths, levels_per_path, level_begin,
                      level_table, edge_temperature, surface_temperature, work, diffusivity,
                      emissivity, emissivity_rows, band_start, from_last, asynchronous, outputs,
                      spectral=None):
        """The call of path_thermal_two_stream (edge_temperature None), of
        path_thermal_two_stream_source and of path_thermal_two_stream_spectral (spectral: knots,
        optics, M; its edge_temperature goes as NULL where None): lbl_<name>."""
        rows, stride, table, starts, n_bands, flags = _whole_paths(
            beta, level_table, n_paths, emissivity_rows, "emissivity_rows", band_start,
            level_begin, levels_per_path, from_last, asynchronous, work)
        edges = _edge_rows(edge_temperature, rows)
        ts, emissivity = _per_path(n_paths, "one surface temperature and one emissivity per "
                                   "path.", surface_temperature, emissivity)
        pointers = _output_pointers(name, PATH_THERMAL_OUTPUTS, outputs, rows, n_paths, stride,
                                    n_bands)
        tables = [table.ctypes.data] + ([] if edges is None else [edges.ctypes.data])
        if spectral is not None:
            knot, optics, n_knots = spectral
            tables = [table.ctypes.data, _address(edges), n_knots, knot.ctypes.data,
                      optics.ctypes.data]
        self._check(getattr(self.lib, "lbl_" + name)(
            self.handle, beta.pointer, stride, int(columns), int(grid), int(n_paths),
            int(levels_per_path), int(level_begin), rows, *tables, float(diffusivity),
            _address(ts), _address(emissivity_rows), _address(emissivity), n_bands,
            _address(starts), work.pointer, *pointers, flags))

    def path_thermal_radiance(self, beta, columns, grid, n_paths, levels_per_path, level_begin,
                              level_table, view_cosine, surface_temperature, up_rows, down_rows,
                              diffusivity=1.66, emissivity=None, emissivity_rows=None,
                              band_start=None, from_last=False, asynchronous=False,
                              radiance_rows=None, brightness_rows=None, radiance_mean=None):
        """The radiance a viewer above the atmosphere sees through the whole paths in the
        DeviceSpectra `beta`, from the two-stream fluxes path_thermal_two_stream left in up_rows
        and down_rows [>= rows, row length] (read only) -- lbl_path_thermal_radiance.  Rows,
        columns, grid, level_table, diffusivity, surface_temperature, emissivity /
        emissivity_rows, band_start, from_last and asynchronous as for path_thermal_two_stream;
        view_cosine one per path, in (0, 1].  Outputs (DeviceSpectra, None: not wanted):
        radiance_rows and brightness_rows [n_paths, row length], and with band_start
        radiance_mean [n_paths, bands]."""
        self._path_thermal_radiance(
            "path_thermal_radiance", beta, columns, grid, n_paths, levels_per_path, level_begin,
            level_table, None, view_cosine, surface_temperature, up_rows, down_rows, diffusivity,
            emissivity, emissivity_rows, band_start, from_last, asynchronous, radiance_rows,
            brightness_rows, radiance_mean)

    def path_thermal_radiance_source(self, beta, columns, grid, n_paths, levels_per_path,
                                     level_begin, level_table, edge_temperature, view_cosine,
                                     surface_temperature, up_rows, down_rows, diffusivity=1.66,
                                     emissivity=None, emissivity_rows=None, band_start=None,
                                     from_last=False, asynchronous=False, radiance_rows=None,
                                     brightness_rows=None, radiance_mean=None):
        """path_thermal_radiance with the linear-in-tau source, from the fluxes
        path_thermal_two_stream_source left in up_rows and down_rows for the same edge table --
        lbl_path_thermal_radiance_source.  edge_temperature [rows, 2] as for
        path_thermal_two_stream_source; everything else as for path_thermal_radiance."""
        if edge_temperature is None:
            raise ValueError("path_thermal_radiance_source needs edge_temperature.")
        self._path_thermal_radiance(
            "path_thermal_radiance_source", beta, columns, grid, n_paths, levels_per_path,
            level_begin, level_table, None, view_cosine, surface_temperature, up_rows, down_rows,
            diffusivity, emissivity, emissivity_rows, band_start, from_last, asynchronous,
            radiance_rows, brightness_rows, radiance_mean, edge_temperature=edge_temperature)

    def path_thermal_radiance_observer(self, beta, columns, grid, n_paths, levels_per_path,
                                       level_begin, level_table, view_cosine, observer_levels,
                                       surface_temperature, up_rows, down_rows,
                                       edge_temperature=None, view_up=False, diffusivity=1.66,
                                       emissivity=None, emissivity_rows=None, band_start=None,
                                       from_last=False, asynchronous=False, radiance_rows=None,
                                       brightness_rows=None, radiance_mean=None):
        """path_thermal_radiance (edge_temperature None) or path_thermal_radiance_source for an
        observer after observer_levels[p] levels of path p, a whole number in [0,
        levels_per_path], looking down (from the surface towards space) or, with view_up, up
        (from space towards the surface) -- lbl_path_thermal_radiance_observer.  up_rows and
        down_rows are the fluxes of path_thermal_two_stream or, with edge_temperature, of
        path_thermal_two_stream_source; everything else as for path_thermal_radiance."""
        rows, stride, table, starts, n_bands, flags = _whole_paths(
            beta, level_table, n_paths, emissivity_rows, "emissivity_rows", band_start,
            level_begin, levels_per_path, from_last, asynchronous)
        mu, ts, emissivity = _per_path(n_paths, "one view cosine, one surface temperature and one "
                                       "emissivity per path.", view_cosine, surface_temperature,
                                       emissivity)
        passed = np.asarray(observer_levels)
        if passed.shape != (int(n_paths),) or passed.dtype.kind not in "iu":
            raise ValueError("observer_levels needs one whole number per path.")
        passed = np.ascontiguousarray(passed, dtype=np.int32)
        _check_outputs((up_rows, down_rows), rows, stride)
        _check_outputs((radiance_rows, brightness_rows), int(n_paths), stride)
        _check_outputs((radiance_mean,), int(n_paths), n_bands)
        edges = _edge_rows(edge_temperature, rows)
        self._check(self.lib.lbl_path_thermal_radiance_observer(
            self.handle, beta.pointer, stride, int(columns), int(grid), int(n_paths),
            int(levels_per_path), int(level_begin), rows, table.ctypes.data, _address(edges),
            float(diffusivity), _address(mu), passed.ctypes.data, int(bool(view_up)),
            _address(ts), _address(emissivity_rows), _address(emissivity), _address(up_rows),
            _address(down_rows), n_bands, _address(starts), _address(radiance_rows),
            _address(brightness_rows), _address(radiance_mean), flags))

    def path_thermal_radiance_spectral(self, beta, columns, grid, n_paths, levels_per_path,
                                       level_begin, level_table, knot_wavenumber, knot_optics,
                                       view_cosine, surface_temperature, up_rows, down_rows,
                                       diffusivity=1.66, emissivity=None, emissivity_rows=None,
                                       band_start=None, from_last=False, asynchronous=False,
                                       radiance_rows=None, brightness_rows=None,
                                       radiance_mean=None):
        """path_thermal_radiance with the scatterer of every level as a table over wavenumber,
        from the fluxes path_thermal_two_stream_spectral left in up_rows and down_rows --
        lbl_path_thermal_radiance_spectral.  knot_wavenumber [M] and knot_optics [rows, M, 3] as
        for path_thermal_two_stream_spectral; tau_c, w_c and g_c of level_table are 0;
        everything else as for path_thermal_radiance."""
        self._path_thermal_radiance(
            "path_thermal_radiance_spectral", beta, columns, grid, n_paths, levels_per_path,
            level_begin, level_table, _knot_table(knot_wavenumber, knot_optics,
                                                  int(beta.shape[0])),
            view_cosine, surface_temperature, up_rows, down_rows, diffusivity, emissivity,
            emissivity_rows, band_start, from_last, asynchronous, radiance_rows, brightness_rows,
            radiance_mean)

    def _path_thermal_radiance(self, name, beta, columns, grid, n_paths, levels_per_path,
                               level_begin, level_table, spectral, view_cosine,
                               surface_temperature, up_rows, down_rows, diffusivity, emissivity,
                               emissivity_rows, band_start, from_last, asynchronous,
                               radiance_rows, brightness_rows, radiance_mean,
                               edge_temperature=None):
        """The call of path_thermal_radiance (spectral None), of path_thermal_radiance_spectral
        (spectral: knots, optics, M) and of path_thermal_radiance_source (edge_temperature):
        lbl_<name>."""
        rows, stride, table, starts, n_bands, flags = _whole_paths(
            beta, level_table, n_paths, emissivity_rows, "emissivity_rows", band_start,
            level_begin, levels_per_path, from_last, asynchronous)
        mu, ts, emissivity = _per_path(n_paths, "one view cosine, one surface temperature and one "
                                       "emissivity per path.", view_cosine, surface_temperature,
                                       emissivity)
        _check_outputs((up_rows, down_rows), rows, stride)
        _check_outputs((radiance_rows, brightness_rows), int(n_paths), stride)
        _check_outputs((radiance_mean,), int(n_paths), n_bands)
        edges = _edge_rows(edge_temperature, rows)
        knots = [] if edges is None else [edges.ctypes.data]
        if spectral is not None:
            knot, optics, n_knots = spectral
            knots = [n_knots, knot.ctypes.data, optics.ctypes.data]
        self._check(getattr(self.lib, "lbl_" + name)(
            self.handle, beta.pointer, stride, int(columns), int(grid), int(n_paths),
            int(levels_per_path), int(level_begin), rows, table.ctypes.data, *knots,
            float(diffusivity),
            _address(mu), _address(ts), _address(emissivity_rows), _address(emissivity),
            _address(up_rows), _address(down_rows), n_bands, _address(starts),
            _address(radiance_rows), _address(brightness_rows), _address(radiance_mean), flags))

    def path_solar_radiance(self, beta, columns, n_paths, levels_per_path, level_begin,
                            level_table, solar_zenith_cosine, view_cosine, scattering_cosine,
                            solar_row, up_rows, direct_rows, diffuse_rows, rayleigh_row=None,
                            albedo=None, albedo_rows=None, band_start=None, from_last=False,
                            asynchronous=False, radiance_rows=None, radiance_mean=None):
        """The sunlight a viewer above the atmosphere sees scattered towards it through the whole
        paths in the DeviceSpectra `beta`, from the two-stream fluxes path_two_stream left in
        up_rows, direct_rows and diffuse_rows [>= rows, row length] (read only) --
        lbl_path_solar_radiance.  Rows, columns, level_table, solar_zenith_cosine, solar_row,
        rayleigh_row, albedo / albedo_rows, band_start, from_last and asynchronous as for
        path_two_stream; view_cosine one per path, in (0, 1]; scattering_cosine one per path, in
        [-1, 1].  Outputs (DeviceSpectra): radiance_rows [n_paths, row length], and with
        band_start radiance_mean [n_paths, bands]."""
        self._path_solar_radiance(
            "path_solar_radiance", beta, columns, n_paths, levels_per_path, level_begin,
            level_table, None, solar_zenith_cosine, view_cosine, scattering_cosine, solar_row,
            up_rows, direct_rows, diffuse_rows, rayleigh_row, albedo, albedo_rows, band_start,
            from_last, asynchronous, radiance_rows, radiance_mean)

    def path_solar_radiance_spectral(self, beta, columns, grid, n_paths, levels_per_path,
                                     level_begin, level_table, knot_wavenumber, knot_optics,
                                     solar_zenith_cosine, view_cosine, scattering_cosine,
                                     solar_row, up_rows, direct_rows, diffuse_rows,
                                     rayleigh_row=None, albedo=None, albedo_rows=None,
                                     band_start=None, from_last=False, asynchronous=False,
                                     radiance_rows=None, radiance_mean=None):
        """path_solar_radiance with the scatterer of every level as a table over wavenumber, from
        the fluxes path_two_stream_spectral left in up_rows, direct_rows and diffuse_rows --
        lbl_path_solar_radiance_spectral.  grid, knot_wavenumber [M] and knot_optics [rows, M, 3]
        as for path_two_stream_spectral; tau_c, w_c and h_c of level_table are 0; everything
        else as for path_solar_radiance."""
        self._path_solar_radiance(
            "path_solar_radiance_spectral", beta, columns, n_paths, levels_per_path, level_begin,
            level_table,
            (int(grid),) + _knot_table(knot_wavenumber, knot_optics, int(beta.shape[0])),
            solar_zenith_cosine, view_cosine, scattering_cosine, solar_row, up_rows, direct_rows,
            diffuse_rows, rayleigh_row, albedo, albedo_rows, band_start, from_last, asynchronous,
            radiance_rows, radiance_mean)

    def _path_solar_radiance(self, name, beta, columns, n_paths, levels_per_path, level_begin,
                             level_table, spectral, solar_zenith_cosine, view_cosine,
                             scattering_cosine, solar_row, up_rows, direct_rows, diffuse_rows,
                             rayleigh_row, albedo, albedo_rows, band_start, from_last,
                             asynchronous, radiance_rows, radiance_mean):
        """The call of path_solar_radiance (spectral None) and of path_solar_radiance_spectral
        (spectral: grid, knots, optics, M): lbl_<name>."""
        rows, stride, table, starts, n_bands, flags = _whole_paths(
            beta, level_table, n_paths, albedo_rows, "albedo_rows", band_start, level_begin,
            levels_per_path, from_last, asynchronous)
        if solar_row.shape[1] < int(columns) or \
                (rayleigh_row is not None and rayleigh_row.shape[1] < int(columns)):
            raise ValueError(f"solar_row and rayleigh_row need {columns} values.")
        mu0, mu, cos_theta, albedo = _per_path(
            n_paths, "one solar cosine, one view cosine, one scattering cosine and one albedo "
            "per path.", solar_zenith_cosine, view_cosine, scattering_cosine, albedo)
        _check_outputs((up_rows, direct_rows, diffuse_rows), rows, stride)
        _check_outputs((radiance_rows,), int(n_paths), stride)
        _check_outputs((radiance_mean,), int(n_paths), n_bands)
        knots = []
        if spectral is not None:
            grid, knot, optics, n_knots = spectral
            knots = [grid, n_knots, knot.ctypes.data, optics.ctypes.data]
        self._check(getattr(self.lib, "lbl_" + name)(
            self.handle, beta.pointer, stride, int(columns), int(n_paths), int(levels_per_path),
            int(level_begin), rows, table.ctypes.data, *knots, _address(mu0), _address(mu),
            _address(cos_theta), solar_row.pointer, _address(rayleigh_row),
            _address(albedo_rows), _address(albedo), _address(up_rows), _address(direct_rows),
            _address(diffuse_rows), n_bands, _address(starts), _address(radiance_rows),
            _address(radiance_mean), flags))

    def continuum_compute_many(self, continua, grid, n, temperature, pressure, vmr, out,
                               accumulate=False, asynchronous=False):
        """Several continua in one pass over the grid (lbl_continuum_compute_many): summed, in
        the order given, into the DeviceSpectra `out` [levels, >= n] -- the same bits as one
        continuum_compute per handle, at a third of the HBM traffic for three of them.
        vmr: [len(continua), levels, VMR_COUNT]."""
        t, p, flags = _slot_levels(temperature, pressure, accumulate, asynchronous)
        handles = np.ascontiguousarray(continua, dtype=np.int32)
        x = _f64(vmr).reshape(handles.size, -1, VMR_COUNT)
        if not (t.ndim == 1 and t.shape == p.shape and x.shape[1] == t.size):
            raise ValueError("temperature, pressure [levels] and vmr [continua, levels, 5] disagree.")
        if not hasattr(out, "pointer"):
            raise ValueError("continuum_compute_many writes a block in HBM (DeviceSpectra).")
        out, pointer, flags, stride = self._output(out, t.size, n, flags)
        self._check(self.lib.lbl_continuum_compute_many(
            self.handle, handles.size, handles.ctypes.data, int(grid), t.size, t.ctypes.data,
            p.ctypes.data, x.ctypes.data, flags, pointer, stride))
        return out

    def _output(self, out, levels, n, flags):
        """(array or DeviceSpectra, pointer, flags, row stride) for a [levels, >= n] block."""
        if out is None:
            out = self.host_array((levels, n))
            if flags & ACCUMULATE:
                out[...] = 0.
        # Rows may be longer than the grid (the lines path pads them to whole wavenumbers).
        if len(out.shape) != 2 or out.shape[0] != levels or out.shape[1] < n:
            raise ValueError(f"out has shape {out.shape}, need ({levels}, >= {n}).")
        if hasattr(out, "pointer"):
            return out, out.pointer, flags | OUT_DEVICE, int(out.shape[1])
        if out.dtype != np.float64 or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("out must be C-contiguous float64[levels, >= n].")
        return out, c_void_p(out.ctypes.data), flags, int(out.shape[1])

    # -- cross-sections (slot 2) -----------------------------------------------------------
    def load_xsec(self, bands):
        """Uploads [(frequency [Hz], coefficients [4, nfreq]), ...]; returns the handle."""
        if not 1 <= len(bands) <= MAX_XSEC_BANDS:
            raise ValueError(f"a molecule has 1 to {MAX_XSEC_BANDS} cross-section bands.")
        sizes = np.zeros(len(bands), dtype=np.int32)
        frequency, coefficients = [], []
        for i, (f, c) in enumerate(bands):
            f, c = _f64(f), _f64(c)
            if f.ndim != 1 or c.shape != (4, f.size):
                raise ValueError("a band is (frequency[nfreq], coefficients[4, nfreq]).")
            sizes[i] = f.size
            frequency.append(f)
            coefficients.append(c.ravel())
        frequency, coefficients = _f64(np.concatenate(frequency)), _f64(np.concatenate(coefficients))
        handle = c_int32(-1)
        self._check(self.lib.lbl_xsec_load(self.handle, len(bands), sizes.ctypes.data,
                                           frequency.ctypes.data, coefficients.ctypes.data,
                                           byref(handle)))
        return handle.value

    def free_xsec(self, xsec):
        self._check(self.lib.lbl_xsec_free(self.handle, int(xsec)))

    def xsec_compute(self, xsec, grid, n, temperature, pressure, vmr=None, out=None,
                     accumulate=False, asynchronous=False):
        """Cross sections [m2] (or, with vmr, n k [m-1]): float64[levels, n] or fills `out`."""
        t, p, flags = _slot_levels(temperature, pressure, accumulate, asynchronous)
        if not (t.ndim == 1 and t.shape == p.shape):
            raise ValueError("temperature and pressure must be 1-d and equally long.")
        x = None
        if vmr is not None:
            x = _f64(np.atleast_1d(vmr))
            if x.shape != t.shape:
                raise ValueError("vmr must be shaped like temperature.")
            flags |= SCALE_DENSITY
        out, pointer, flags, stride = self._output(out, t.size, n, flags)
        self._check(self.lib.lbl_xsec_compute(
            self.handle, int(xsec), int(grid), t.size, t.ctypes.data, p.ctypes.data,
            x.ctypes.data if x is not None else None, flags, pointer, stride))
        return out

    def xsec_bands(self, xsec, sizes, temperature, pressure):
        """The clipped fit on the bands' own grids for one level (list of arrays)."""
        values = np.zeros(int(sum(sizes)), dtype=np.float64)
        self._check(self.lib.lbl_xsec_bands(self.handle, int(xsec), float(temperature),
                                            float(pressure), values.ctypes.data))
        return np.split(values, np.cumsum(sizes)[:-1])

    def continuum_bands(self, continuum, sizes, temperature, pressure_mb, vmr):
        """Coarse spectra [cm-1] of each band for one level (list of arrays)."""
        x = _f64(vmr).reshape(VMR_COUNT)
        spectra = np.zeros(int(sum(sizes)), dtype=np.float64)
        self._check(self.lib.lbl_continuum_bands(self.handle, int(continuum), float(temperature),
                                                 float(pressure_mb), x.ctypes.data,
                                                 spectra.ctypes.data))
        return np.split(spectra, np.cumsum(sizes)[:-1])

    def timing(self, reset=False):
        """(milliseconds[8], launches[8]) for prepare (prologue), far-field series (and the tile
        schedule of host-side prep), accumulate, pedestal, continuum band spectra, continuum
        interpolation, cross-section fit, cross-section interpolation."""
        ms = (c_double*8)()
        launches = (c_int64*8)()
        self._check(self.lib.lbl_timing(self.handle, ms, launches, 1 if reset else 0))
        return list(ms), list(launches)

    def timing_busy(self):
        """milliseconds[8] (indices as timing()) during which at least one timed launch of the kind
        was running since the last reset: launches of calls on different lanes overlap, and what
        timing() sums twice this counts once.  Read it before timing(reset=True)."""
        ms = (c_double*8)()
        self._check(self.lib.lbl_timing_busy(self.handle, ms))
        return list(ms)

    @property
    def stream(self):
        return self.lib.lbl_stream(self.handle)

    def order_stream_after(self, stream):
        """Work queued on `stream` (a raw hipStream_t, e.g. torch.cuda.Stream.cuda_stream) from
        now on runs after everything queued on the engine so far; the host does not wait."""
        self._check(self.lib.lbl_order_stream_after_engine(self.handle, c_void_p(stream or None)))

    def order_after_stream(self, stream):
        """Everything the engine queues from now on runs after what `stream` holds now."""
        self._check(self.lib.lbl_order_engine_after_stream(self.handle, c_void_p(stream or None)))


_default_engines = {}
_default_engines_lock = threading.Lock()


def default_engine(device=0):
    """Process-wide engine per device (what Gas objects share, from any thread)."""
    with _default_engines_lock:
        if device not in _default_engines:
            _default_engines[device] = Engine(device)
        return _default_engines[device]
