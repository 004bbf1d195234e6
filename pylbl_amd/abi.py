"""ctypes binding of the C ABI in include/lbl_amd.h, include/lbl_amd_twostream.h,
include/lbl_amd_thermal.h, include/lbl_amd_thermal_source.h, include/lbl_amd_kdist.h,
include/lbl_amd_scatterer.h, include/lbl_amd_thermal_radiance.h,
include/lbl_amd_solar_radiance.h, include/lbl_amd_scatterer_radiance.h,
include/lbl_amd_thermal_radiance_source.h, include/lbl_amd_thermal_radiance_observer.h and
include/lbl_amd_wing.h
(pylbl_amd/liblbl_amd.so), and nothing else:
the mirrors of the header's #defines, struct lbl_band, one table of every function's prototype,
the loader that applies it, and the one call sequence that needs no engine (the SQLite table
reader).

This is the only Python<->native boundary of the package, the counterpart of
pyLBL/c_lib/gas_optics.py:11-26,68-91 in the reference.  There is no CPU fallback: if the
library is missing, loading it raises.  tests/test_abi_host.py compares PROTOTYPES, BandDescriptor
and the mirrors with the header, declaration by declaration.
"""
from ctypes import CDLL, POINTER, Structure, byref, c_char_p, c_double, c_int32, c_int64, \
                   c_void_p
import os
from pathlib import Path

import numpy as np

from .errors import EngineError

LIBRARY_PATH = Path(__file__).resolve().parent / "liblbl_amd.so"

# Mirrors of the #defines in include/lbl_amd.h.
LBL_OK = 0
# Status codes of lbl_table_read.
TABLE_OPEN_FAILED, TABLE_NO_ALIAS, TABLE_NO_TIPS, TABLE_NOT_RECTANGULAR, TABLE_NO_ISOTOPOLOGUES, \
    TABLE_NO_TRANSITIONS = 10, 11, 12, 13, 14, 15
RANGE_REFERENCE, RANGE_SKIP = 0, 1
PREP_DEVICE, PREP_HOST = 0, 1
OUT_DEVICE, ASYNC, SCALE_DENSITY, ACCUMULATE, FARFIELD, DEFER_FINISH = 1, 2, 4, 8, 16, 32
RANGE_POLICIES = {"reference": RANGE_REFERENCE, "skip": RANGE_SKIP}
# lbl_path_compute flags: a namespace of their own, clear of the call flags above.
PATH_OPTICAL_DEPTH, PATH_TRANSMITTANCE, PATH_CUMULATIVE, PATH_FROM_LAST, PATH_CONTINUE = \
    0x100, 0x200, 0x400, 0x800, 0x1000
# lbl_path_radiance adds two outputs to them.
PATH_RADIANCE, PATH_BRIGHTNESS = 0x2000, 0x4000
# lbl_path_flux: the up sweep.
PATH_FLUX_UP = 0x8000
# lbl_path_jacobian: its five Jacobians, beside PATH_RADIANCE.
PATH_JACOBIAN_DEPTH, PATH_JACOBIAN_LOG_DEPTH, PATH_JACOBIAN_TEMPERATURE, \
    PATH_JACOBIAN_BOUNDARY_T, PATH_JACOBIAN_BOUNDARY_E = \
    0x10000, 0x20000, 0x40000, 0x80000, 0x100000
# Engine.path_jacobian's outputs and their flags, in the order of lbl_path_jacobian's arguments.
PATH_JACOBIAN_OUTPUTS = (
    ("radiance", PATH_RADIANCE), ("optical_depth_jacobian", PATH_JACOBIAN_DEPTH),
    ("log_optical_depth_jacobian", PATH_JACOBIAN_LOG_DEPTH),
    ("temperature_jacobian", PATH_JACOBIAN_TEMPERATURE),
    ("boundary_temperature_jacobian", PATH_JACOBIAN_BOUNDARY_T),
    ("boundary_emissivity_jacobian", PATH_JACOBIAN_BOUNDARY_E))
PATH_JACOBIAN_PER_LEVEL = ("optical_depth_jacobian", "log_optical_depth_jacobian",
                           "temperature_jacobian")
# Engine.path_two_stream's outputs, in the order of lbl_path_two_stream's arguments: the fluxes at
# the interface below each level and at interface 0 of each path, then their band means.
PATH_TWO_STREAM_OUTPUTS = tuple(
    prefix + name + suffix for suffix in ("_rows", "_mean") for prefix in ("", "top_")
    for name in ("up", "down", "direct", "diffuse"))
# Engine.path_thermal_two_stream's, in the order of lbl_path_thermal_two_stream's arguments.
PATH_THERMAL_OUTPUTS = tuple(
    prefix + name + suffix for suffix in ("_rows", "_mean") for prefix in ("", "top_")
    for name in ("up", "down"))

VMR_SELF, VMR_H2O, VMR_O2, VMR_N2, VMR_TOTAL, VMR_COUNT = 0, 1, 2, 3, 4, 5
MAX_BANDS = 8
MAX_XSEC_BANDS = 16


class BandDescriptor(Structure):
    """struct lbl_band of include/lbl_amd.h."""
    _fields_ = [("kind", c_int32), ("size", c_int32), ("lower_bound", c_double),
                ("resolution", c_double), ("column", c_int64*4)]


_ptr, _i32, _i64, _f64 = c_void_p, c_int32, c_int64, c_double
_f64p, _i32p, _i64p = POINTER(c_double), POINTER(c_int32), POINTER(c_int64)
# What the path entries begin with: engine, beta, row_stride, columns ...
_BLOCK = [_ptr, _ptr, _i64, _i64]
# ... and, lbl_path_compute and lbl_path_solar at once, the others behind `grid`: n_paths,
# levels_per_path, level_begin, level_count.
_RUN = [_i32, _i32, _i32, _i32]
# lbl_compute and lbl_compute_streamed up to `level_stride`: engine, molecule, n_levels,
# temperature, pressure, vmr, v0, vn, n_per_v, cut_off, remove_pedestal, range_policy, flags, k,
# level_stride.
_COMPUTE = [_ptr, _i32, _i32, _ptr, _ptr, _ptr] + [_i32]*7 + [_ptr, _i64]
# The reference's absorption(): pressure, temperature, volume_mixing_ratio, v0, vn, n_per_v, k,
# database, formula, cut_off, remove_pedestal.
_ABSORPTION = [_f64]*3 + [_i32]*3 + [_ptr, c_char_p, c_char_p, _i32, _i32]

# Every function of include/lbl_amd.h and its argument types, in the header's order.  Each returns
# int (c_int32) unless RESULT_TYPES says otherwise.  Pointers the callers fill with addresses
# (numpy's .ctypes.data, DeviceSpectra.pointer) are c_void_p; POINTER(T) where they pass byref()
# or a ctypes array.
PROTOTYPES = {
    # -- engine, molecules, the lines call ------------------------------------------------------
    "lbl_engine_create": [_i32, POINTER(c_void_p)],
    "lbl_engine_destroy": [_ptr],
    "lbl_last_error": [_ptr],
    "lbl_molecule_load": [_ptr, _i64] + [_ptr]*7 + [_ptr, _ptr, _i32, _i32, _ptr, _ptr, _i32p],
    "lbl_molecule_free": [_ptr, _i32],
    "lbl_compute": _COMPUTE + [_i64p],
    "lbl_compute_streamed": _COMPUTE + [_ptr, _i64, _i64, _i32],
    "lbl_finish_deferred": [_ptr],
    "lbl_deferred": [_ptr],
    "lbl_cancel_deferred": [_ptr],
    "lbl_synchronize": [_ptr],
    "lbl_fill_zero": [_ptr, _ptr, _i32, _i64, _i64, _i32],
    # -- paths ----------------------------------------------------------------------------------
    # path_length, n_bands, band_start, carry, optical_depth, transmittance, flags
    "lbl_path_compute": _BLOCK + _RUN + [_ptr, _i32, _ptr, _ptr, _ptr, _ptr, _i32],
    # grid, the run, path_length, temperature, boundary_temperature, boundary_emissivity, n_bands,
    # band_start, carry, radiance, brightness_temperature, flags
    "lbl_path_radiance": _BLOCK + [_i32] + _RUN + [_ptr, _ptr, _ptr, _ptr, _i32, _ptr, _ptr,
                                                   _ptr, _ptr, _i32],
    # grid, the run, n_angles, path_length, weight, temperature, surface_temperature,
    # surface_emissivity, n_bands, band_start, carry, reflection, level_flux, flux, surface_flux,
    # flags
    "lbl_path_flux": _BLOCK + [_i32] + _RUN + [_i32, _ptr, _ptr, _ptr, _ptr, _ptr, _i32, _ptr,
                                               _ptr, _ptr, _ptr, _ptr, _ptr, _i32],
    # lbl_path_radiance's with edge_temperature after temperature
    "lbl_path_radiance_source": _BLOCK + [_i32] + _RUN + [_ptr, _ptr, _ptr, _ptr, _ptr, _i32,
                                                          _ptr, _ptr, _ptr, _ptr, _i32],
    # lbl_path_flux's with edge_temperature after temperature
    "lbl_path_flux_source": _BLOCK + [_i32] + _RUN + [_i32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr,
                                                      _i32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr,
                                                      _i32],
    # engine, grid, n_paths, path_begin, path_count, n_knots, knot_wavenumber, knot_emissivity,
    # rows, row_stride, flags
    "lbl_surface_emissivity": [_ptr, _i32, _i32, _i32, _i32, _i32, _ptr, _ptr, _ptr, _i64, _i32],
    # lbl_path_radiance_source's with emissivity_rows and reflection after flags
    "lbl_path_radiance_surface": _BLOCK + [_i32] + _RUN + [_ptr, _ptr, _ptr, _ptr, _ptr, _i32,
                                                           _ptr, _ptr, _ptr, _ptr, _i32, _ptr,
                                                           _ptr],
    # grid, the run, path_length, temperature, boundary_temperature, boundary_emissivity, n_bands,
    # band_start, work, radiance and the five Jacobians, flags
    "lbl_path_jacobian": _BLOCK + [_i32] + _RUN + [_ptr, _ptr, _ptr, _ptr, _i32, _ptr, _ptr] +
                         [_ptr]*6 + [_i32],
    # -- instruments ----------------------------------------------------------------------------
    "lbl_instrument_create": [_ptr, _i32, _i32, _i32, _ptr, _ptr, _ptr, _i32, _ptr, _ptr, _i32,
                              _i32p],
    "lbl_instrument_free": [_ptr, _i32],
    "lbl_instrument_apply": [_ptr, _ptr, _i64, _i32, _i32, _i32, _ptr],
    # -- options, timing, streams, memory -------------------------------------------------------
    "lbl_set_option": [_ptr, c_char_p, _i64],
    "lbl_timing": [_ptr, _f64p, _i64p, _i32],
    "lbl_timing_busy": [_ptr, _f64p],
    "lbl_stream": [_ptr],
    "lbl_order_stream_after_engine": [_ptr, _ptr],
    "lbl_order_engine_after_stream": [_ptr, _ptr],
    "lbl_device_alloc": [_ptr, _i64, POINTER(c_void_p)],
    "lbl_device_free": [_ptr, _ptr],
    "lbl_copy_to_host": [_ptr, _ptr, _ptr, _i64],
    "lbl_copy_rows_to_host": [_ptr, _ptr, _i64, _ptr, _i64, _i64, _i64, _i32],
    "lbl_host_alloc": [_ptr, _i64, POINTER(c_void_p)],
    "lbl_host_free": [_ptr, _ptr],
    "lbl_line_scalars": [_ptr, _i32] + [_f64]*3 + [_i32]*6 + [_ptr],
    # -- continua (slot 1) ----------------------------------------------------------------------
    "lbl_continuum_load": [_ptr, _i32, POINTER(BandDescriptor), _ptr, _i64, _i32p],
    "lbl_continuum_free": [_ptr, _i32],
    "lbl_grid_load": [_ptr, _i64, _ptr, _i32p],
    "lbl_grid_free": [_ptr, _i32],
    "lbl_continuum_compute": [_ptr, _i32, _i32, _i32, _ptr, _ptr, _ptr, _i32, _ptr, _i64],
    "lbl_continuum_compute_many": [_ptr, _i32, _ptr, _i32, _i32, _ptr, _ptr, _ptr, _i32, _ptr,
                                   _i64],
    "lbl_continuum_bands": [_ptr, _i32, _f64, _f64, _ptr, _ptr],
    # -- cross-sections (slot 2) ----------------------------------------------------------------
    "lbl_xsec_load": [_ptr, _i32, _ptr, _ptr, _ptr, _i32p],
    "lbl_xsec_free": [_ptr, _i32],
    "lbl_xsec_compute": [_ptr, _i32, _i32, _i32, _ptr, _ptr, _ptr, _i32, _ptr, _i64],
    "lbl_xsec_bands": [_ptr, _i32, _f64, _f64, _ptr],
    # -- the reference's entry, the table reader ------------------------------------------------
    "lbl_absorption": _ABSORPTION,
    "absorption": _ABSORPTION,
    "lbl_table_read": [c_char_p, c_char_p, POINTER(c_void_p)],
    "lbl_table_shape": [_ptr, _i64p, _i32p, _i32p, _i32p, _i32p, c_char_p, _i32],
    "lbl_table_copy": [_ptr] + [_ptr]*6,
    "lbl_table_free": [_ptr],
    "lbl_molecule_load_sqlite": [_ptr, c_char_p, c_char_p, _i32p],
    "lbl_compat_state": [_i32p, _i32p],
    "lbl_version": [],
    "lbl_wing_batches": [_ptr],
    # -- sunlight, band k-distributions ---------------------------------------------------------
    # engine, grid, columns, n_knots, knot_wavenumber, knot_irradiance, temperature, scale, row,
    # flags
    "lbl_solar_spectrum": [_ptr, _i32, _i64, _i32, _ptr, _ptr, _f64, _f64, _ptr, _i32],
    # solar_length, view_length, solar_zenith_cosine, solar_row, albedo_rows, albedo, n_bands,
    # band_start, carry, four blocks of rows, their four means, flags
    "lbl_path_solar": _BLOCK + _RUN + [_ptr]*6 + [_i32] + [_ptr]*10 + [_i32],
    # engine, values, row_stride, columns, n_rows, band_start, n_bands, scratch, interval_start,
    # n_intervals, means, point_index, point_fraction, n_points, quantiles, flags
    "lbl_band_distribution": [_ptr, _ptr, _i64, _i64, _i32, _ptr, _i32, _ptr, _ptr, _i32, _ptr,
                              _ptr, _ptr, _i32, _ptr, _i32],
}
# The three that do not return int.
RESULT_TYPES = {"lbl_last_error": c_char_p, "lbl_stream": c_void_p, "lbl_version": c_char_p}
EXPORTED_SYMBOLS = tuple(PROTOTYPES)
# Every function of include/lbl_amd_twostream.h, the header beside lbl_amd.h that declares the
# two-stream shortwave entries of the same library, in its order; each returns int.
# tests/test_two_stream_host.py compares this table with that header as test_abi_host.py compares
# PROTOTYPES with lbl_amd.h.
TWO_STREAM_PROTOTYPES = {
    # engine, grid, columns, cross_section, row, flags
    "lbl_rayleigh_row": [_ptr, _i32, _i64, _ptr, _ptr, _i32],
    # level_table, solar_zenith_cosine, solar_row, rayleigh_row, albedo_rows, albedo, n_bands,
    # band_start, work, eight blocks of rows, their eight means, flags
    "lbl_path_two_stream": _BLOCK + _RUN + [_ptr]*6 + [_i32] + [_ptr]*18 + [_i32],
}
# Every function of include/lbl_amd_thermal.h, the header of the two-stream longwave entry of the
# same library; each returns int.  tests/test_thermal_host.py compares this table with that header.
THERMAL_PROTOTYPES = {
    # grid, the run, level_table, diffusivity, surface_temperature, emissivity_rows, emissivity,
    # n_bands, band_start, work, four blocks of rows, their four means, flags
    "lbl_path_thermal_two_stream": _BLOCK + [_i32] + _RUN + [_ptr, _f64, _ptr, _ptr, _ptr, _i32] +
                                   [_ptr]*10 + [_i32],
}
# Every function of include/lbl_amd_thermal_source.h, the header of the same entry with the
# linear-in-tau source; each returns int.  tests/test_thermal_source_host.py compares this table
# with that header.
THERMAL_SOURCE_PROTOTYPES = {
    # lbl_path_thermal_two_stream's with edge_temperature after level_table
    "lbl_path_thermal_two_stream_source": _BLOCK + [_i32] + _RUN + [_ptr, _ptr, _f64, _ptr, _ptr,
                                                                    _ptr, _i32] + [_ptr]*10 +
                                          [_i32],
}
# Every function of include/lbl_amd_kdist.h, the header of the weighted band k-distribution entry
# of the same library; each returns int.  tests/test_kdistribution_weighted_host.py compares this
# table with that header.
KDIST_PROTOTYPES = {
    # engine, values, row_stride, columns, n_rows, band_start, n_bands, scratch, grid,
    # row_temperature, weight_row, index_rows, index_scratch, index_stride, weight_rows,
    # weighted_rows, interval_start, n_intervals, weight_sums, weighted_sums, means, point_index,
    # point_fraction, n_points, quantiles, flags
    "lbl_band_distribution_weighted": [_ptr, _ptr, _i64, _i64, _i32, _ptr, _i32, _ptr, _i32,
                                       _ptr, _ptr, _ptr, _ptr, _i64, _ptr, _ptr, _ptr, _i32,
                                       _ptr, _ptr, _ptr, _ptr, _ptr, _i32, _ptr, _i32],
}
# Every function of include/lbl_amd_scatterer.h, the header of the two-stream entries with spectral
# cloud and aerosol optics of the same library, in its order; each returns int.
# tests/test_scatterer_host.py compares this table with that header.
SCATTERER_PROTOTYPES = {
    # lbl_path_two_stream's with grid, n_knots, knot_wavenumber and knot_optics after level_table
    "lbl_path_two_stream_spectral": _BLOCK + _RUN + [_ptr, _i32, _i32, _ptr, _ptr] + [_ptr]*5 +
                                    [_i32] + [_ptr]*18 + [_i32],
    # lbl_path_thermal_two_stream_source's with n_knots, knot_wavenumber and knot_optics after
    # edge_temperature
    "lbl_path_thermal_two_stream_spectral": _BLOCK + [_i32] + _RUN + [_ptr, _ptr, _i32, _ptr, _ptr,
                                                                      _f64, _ptr, _ptr, _ptr,
                                                                      _i32] + [_ptr]*10 + [_i32],
}
# Every function of include/lbl_amd_thermal_radiance.h, the header of the all-sky radiance entry of
# the same library; each returns int.  tests/test_thermal_radiance_host.py compares this table with
# that header.
THERMAL_RADIANCE_PROTOTYPES = {
    # grid, the run, level_table, diffusivity, view_cosine, surface_temperature, emissivity_rows,
    # emissivity, up_rows, down_rows, n_bands, band_start, radiance_rows, brightness_rows,
    # radiance_mean, flags
    "lbl_path_thermal_radiance": _BLOCK + [_i32] + _RUN + [_ptr, _f64] + [_ptr]*6 + [_i32] +
                                 [_ptr]*4 + [_i32],
}
# Every function of include/lbl_amd_solar_radiance.h, the header of the scattered-sunlight radiance
# entry of the same library; each returns int.  tests/test_solar_radiance_host.py compares this
# table with that header.
SOLAR_RADIANCE_PROTOTYPES = {
    # the run, level_table, solar_zenith_cosine, view_cosine, scattering_cosine, solar_row,
    # rayleigh_row, albedo_rows, albedo, up_rows, direct_rows, diffuse_rows, n_bands, band_start,
    # radiance_rows, radiance_mean, flags
    "lbl_path_solar_radiance": _BLOCK + _RUN + [_ptr]*11 + [_i32] + [_ptr]*3 + [_i32],
}
# Every function of include/lbl_amd_scatterer_radiance.h, the header of the two radiance entries
# with spectral cloud and aerosol optics of the same library, in its order; each returns int.
# tests/test_scatterer_radiance_host.py compares this table with that header.
SCATTERER_RADIANCE_PROTOTYPES = {
    # lbl_path_thermal_radiance's with n_knots, knot_wavenumber and knot_optics after level_table
    "lbl_path_thermal_radiance_spectral": _BLOCK + [_i32] + _RUN + [_ptr, _i32, _ptr, _ptr, _f64] +
                                          [_ptr]*6 + [_i32] + [_ptr]*4 + [_i32],
    # lbl_path_solar_radiance's with grid, n_knots, knot_wavenumber and knot_optics after
    # level_table
    "lbl_path_solar_radiance_spectral": _BLOCK + _RUN + [_ptr, _i32, _i32, _ptr, _ptr] +
                                        [_ptr]*10 + [_i32] + [_ptr]*3 + [_i32],
}
# Every function of include/lbl_amd_thermal_radiance_source.h, the header of the all-sky radiance
# entry with the linear-in-tau source; each returns int.
# tests/test_thermal_radiance_source_host.py compares this table with that header.
THERMAL_RADIANCE_SOURCE_PROTOTYPES = {
    # lbl_path_thermal_radiance's with edge_temperature after level_table
    "lbl_path_thermal_radiance_source": _BLOCK + [_i32] + _RUN + [_ptr, _ptr, _f64] + [_ptr]*6 +
                                        [_i32] + [_ptr]*4 + [_i32],
}
# Every function of include/lbl_amd_thermal_radiance_observer.h, the header of the all-sky radiance
# entry for an observer at any interface, looking down or up; each returns int.
# tests/test_thermal_radiance_observer_host.py compares this table with that header.
THERMAL_RADIANCE_OBSERVER_PROTOTYPES = {
    # lbl_path_thermal_radiance_source's with observer_levels and view_up after view_cosine
    "lbl_path_thermal_radiance_observer": _BLOCK + [_i32] + _RUN + [_ptr, _ptr, _f64, _ptr, _ptr,
                                                                    _i32] + [_ptr]*5 + [_i32] +
                                          [_ptr]*4 + [_i32],
}
# Every function of include/lbl_amd_wing.h, the header of the far-wing group records of the same
# library; each returns int.  tests/test_wing_scaled_host.py compares this table with that header.
WING_PROTOTYPES = {
    # centre, g2, bl, lines, record
    "lbl_wing_group": [_ptr, _ptr, _ptr, _i32, _ptr],
}

_library = None


def _preload_hip_runtime():
    """One process must hold ONE HIP runtime.  PyTorch-ROCm wheels ship their own
    libamdhip64.so.7 (same SONAME as /opt/rocm's): when torch is imported first, this library
    binds to torch's copy and all is well; the other way round torch finds the system runtime
    already resident beside its own HSA libraries and sees no GPU.  So when a ROCm torch is
    installed but not imported yet, its runtime is loaded here first (no torch import: only the
    shared object), which makes the order irrelevant."""
    import importlib.util
    import os
    import sys
    from ctypes import RTLD_GLOBAL
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    for location in spec.submodule_search_locations:
        candidate = os.path.join(location, "lib", "libamdhip64.so")
        if os.path.exists(candidate):
            try:
                CDLL(candidate, mode=RTLD_GLOBAL)
            except OSError:
                pass
            return


def library():
    """Loads liblbl_amd.so (once) and declares the argument types of every entry point."""
    global _library
    if _library is not None:
        return _library
    path = LIBRARY_PATH
    if os.environ.get("PYLBL_AMD_LIBRARY"):
        # Another build of the same engine (sanitizer / diagnostics builds, A/B of two libraries):
        # the shipped file is never overwritten to try one.
        path = Path(os.environ["PYLBL_AMD_LIBRARY"]).resolve()
        if not path.exists():
            raise EngineError(f"$PYLBL_AMD_LIBRARY names {path}, which does not exist.")
    elif not LIBRARY_PATH.exists():
        # A fresh checkout: compile in-tree (hipcc cross-compiles without a GPU).
        try:
            from . import build
            build.build()
        except Exception as error:
            raise EngineError(
                f"{LIBRARY_PATH} is missing and could not be built ({error}); build it with "
                "`python -m pylbl_amd.build` (there is no CPU fallback).")
    _preload_hip_runtime()
    lib = CDLL(str(path))
    for name, arguments in list(PROTOTYPES.items()) + list(TWO_STREAM_PROTOTYPES.items()) + \
            list(THERMAL_PROTOTYPES.items()) + list(THERMAL_SOURCE_PROTOTYPES.items()) + \
            list(KDIST_PROTOTYPES.items()) + list(SCATTERER_PROTOTYPES.items()) + \
            list(THERMAL_RADIANCE_PROTOTYPES.items()) + \
            list(SOLAR_RADIANCE_PROTOTYPES.items()) + \
            list(SCATTERER_RADIANCE_PROTOTYPES.items()) + \
            list(THERMAL_RADIANCE_SOURCE_PROTOTYPES.items()) + \
            list(THERMAL_RADIANCE_OBSERVER_PROTOTYPES.items()) + list(WING_PROTOTYPES.items()):
        function = getattr(lib, name)
        function.argtypes = arguments
        function.restype = RESULT_TYPES.get(name, c_int32)
    _library = lib
    return lib


def read_line_table(path, name):
    """One molecule's rows out of an SQLite file in pyLBL's schema through the engine's own C
    reader (lbl_table_read: the reference C reader's SELECTs, absorption.c:69-70,
    spectral_database.c:55, :113, :143) -- no GPU involved.  Returns (status, message, fields):
    status LBL_OK and a dict of arrays, or a TABLE_* status and the reader's message."""
    from ctypes import create_string_buffer
    lib = library()
    table = c_void_p()
    status = lib.lbl_table_read(os.fsencode(str(path)), str(name).encode(), byref(table))
    if status != LBL_OK:
        return status, lib.lbl_last_error(None).decode(), None
    try:
        n_lines, molecule_id = c_int64(), c_int32()
        rows, num_iso, num_t = c_int32(), c_int32(), c_int32()
        formula = create_string_buffer(256)
        lib.lbl_table_shape(table, byref(n_lines), byref(molecule_id), byref(rows), byref(num_iso),
                            byref(num_t), formula, 256)
        columns = np.empty((7, n_lines.value))
        local_iso_id = np.empty(n_lines.value, dtype=np.int32)
        isoid = np.empty(rows.value, dtype=np.int64)
        mass = np.empty(rows.value)
        tips_temperature = np.empty(num_t.value)
        tips_data = np.empty((num_iso.value, num_t.value))
        lib.lbl_table_copy(table, columns.ctypes.data, local_iso_id.ctypes.data, isoid.ctypes.data,
                           mass.ctypes.data, tips_temperature.ctypes.data, tips_data.ctypes.data)
    finally:
        lib.lbl_table_free(table)
    return LBL_OK, "", {"formula": formula.value.decode(), "molecule_id": molecule_id.value,
                        "columns": columns, "local_iso_id": local_iso_id, "isoid": isoid,
                        "mass": mass, "tips_temperature": tips_temperature,
                        "tips_data": tips_data}
