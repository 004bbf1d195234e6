"""Instrument line shapes: the channels a sounder or an FTS measures, each a weighted mean of the
fine spectrum under its line shape (Spectroscopy.compute_path / compute_radiance with
`instrument`; the kernels are csrc/instrument.h, the C entries lbl_instrument_*).

For channel c with centre nu_c, window [lo_c, hi_c] and weight w_c(Delta), Delta = nu_j - nu_c,
the channel value of fine-grid values v_j is

    R_c = (sum_j w_c(nu_j - nu_c) v_j) / (sum_j w_c(nu_j - nu_c)),
          searchsorted(grid, lo_c, "left") <= j < searchsorted(grid, hi_c, "right"),

normalised on the discrete grid; NaN when the window holds no points, when the weights do not sum
to > 0, or when [lo_c, hi_c] is not wholly inside [grid[0], grid[-1]] (a channel only partly
covered by the grid is not a measurement).
"""
import weakref

import numpy as np

# 4 ln 2, one fp64 literal: the Gaussian of FWHM f is exp(-G*(Delta/f)**2).
GAUSSIAN_G = 2.772588722239781

# Shape codes of lbl_instrument_create (include/lbl_amd.h).
BOXCAR, TRIANGLE, GAUSSIAN, FTS, FTS_HAMMING, TABULATED = range(6)
_SHAPE_NAMES = {BOXCAR: "boxcar", TRIANGLE: "triangle", GAUSSIAN: "gaussian", FTS: "fts",
                FTS_HAMMING: "fts-hamming", TABULATED: "tabulated"}
FTS_APODIZATIONS = ("none", "hamming")


def _centers(centers):
    values = np.array(centers, dtype=np.float64, ndmin=1)
    if values.ndim != 1 or values.size < 1:
        raise ValueError("centers must be a 1-d array of at least one channel.")
    if not np.all(np.isfinite(values)):
        raise ValueError("centers must be finite.")
    return values


def _per_channel(value, name, count):
    """A scalar or one value per channel, finite and > 0, as float64 [count]."""
    values = np.asarray(value, dtype=np.float64)
    if values.shape not in ((), (count,)):
        raise ValueError(f"{name} has shape {values.shape}: give a scalar or one value per "
                         f"channel ({count}).")
    values = np.array(np.broadcast_to(values, (count,)))
    if not np.all(np.isfinite(values)) or np.any(values <= 0.):
        raise ValueError(f"{name} must be finite and > 0.")
    return values


def _sinc(x):
    """sin(pi x)/(pi x), 1 at 0, formed as the kernel forms it."""
    x = np.asarray(x, dtype=np.float64)
    y = np.pi*x
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.sin(y)/y
    return np.where(x == 0., 1., out)


class Instrument(object):
    """N instrument channels: centres, a line shape and its window.  Immutable; build it with
    the constructors boxcar, triangle, gaussian, fts and tabulated.  Channels come back in the
    order of the centres given (any order)."""
    __slots__ = ("_shape", "_centers", "_parameter", "_half_width", "_offsets", "_response",
                 "__weakref__")

    def __init__(self, shape, centers, parameter=None, half_width=None, offsets=None,
                 response=None):
        if shape not in _SHAPE_NAMES:
            raise ValueError(f"unknown instrument shape {shape!r}.")
        arrays = {"_centers": centers, "_parameter": parameter, "_half_width": half_width,
                  "_offsets": offsets, "_response": response}
        for name, value in arrays.items():
            if value is not None:
                value = np.array(value, dtype=np.float64)
                value.setflags(write=False)
            object.__setattr__(self, name, value)
        object.__setattr__(self, "_shape", shape)

    def __setattr__(self, name, value):
        raise AttributeError("Instrument is immutable.")

    # Constructors.
    @classmethod
    def boxcar(cls, centers, width):
        """w = 1 on the window nu_c -/+ width/2."""
        c = _centers(centers)
        return cls(BOXCAR, c, parameter=_per_channel(width, "width", c.size))

    @classmethod
    def triangle(cls, centers, fwhm):
        """w = 1 - |Delta|/fwhm on the window nu_c -/+ fwhm."""
        c = _centers(centers)
        return cls(TRIANGLE, c, parameter=_per_channel(fwhm, "fwhm", c.size))

    @classmethod
    def gaussian(cls, centers, fwhm, half_width=None):
        """w = exp(-G*(Delta/fwhm)**2), G = 4 ln 2, on the window nu_c -/+ half_width (default
        3*fwhm)."""
        c = _centers(centers)
        fwhm = _per_channel(fwhm, "fwhm", c.size)
        half_width = 3.*fwhm if half_width is None else \
            _per_channel(half_width, "half_width", c.size)
        return cls(GAUSSIAN, c, parameter=fwhm, half_width=half_width)

    @classmethod
    def fts(cls, centers, max_path_difference, apodization="none", half_width=None):
        """An FTS of maximum optical path difference L [cm]: S(Delta) = sinc(2 L Delta),
        sinc(x) = sin(pi x)/(pi x); with apodization "hamming" w = 0.54 S(Delta) +
        0.23 (S(Delta - 1/(2L)) + S(Delta + 1/(2L))).  Window nu_c -/+ half_width (required)."""
        c = _centers(centers)
        if apodization not in FTS_APODIZATIONS:
            raise ValueError(f"apodization must be one of {FTS_APODIZATIONS}, not "
                             f"{apodization!r}.")
        if half_width is None:
            raise ValueError("fts needs half_width: the sinc has no natural end.")
        length = _per_channel(max_path_difference, "max_path_difference", c.size)
        half_width = _per_channel(half_width, "half_width", c.size)
        return cls(FTS if apodization == "none" else FTS_HAMMING, c, parameter=length,
                   half_width=half_width)

    @classmethod
    def tabulated(cls, centers, offsets, response):
        """w = linear interpolation of `response` at Delta on `offsets` (>= 2 finite, strictly
        increasing values [cm-1]); `response` is [K] (shared by all channels) or [N, K] (one row
        per channel), finite.  Window [nu_c + offsets[0], nu_c + offsets[-1]]."""
        c = _centers(centers)
        offsets = np.asarray(offsets, dtype=np.float64)
        if offsets.ndim != 1 or offsets.size < 2:
            raise ValueError("offsets must be a 1-d array of at least two values.")
        if not np.all(np.isfinite(offsets)) or not np.all(np.diff(offsets) > 0.):
            raise ValueError("offsets must be finite and strictly increasing.")
        response = np.asarray(response, dtype=np.float64)
        if response.shape not in ((offsets.size,), (c.size, offsets.size)):
            raise ValueError(f"response has shape {response.shape}: give [{offsets.size}] or "
                             f"[{c.size}, {offsets.size}].")
        if not np.all(np.isfinite(response)):
            raise ValueError("response must be finite.")
        return cls(TABULATED, c, offsets=offsets, response=response)

    # What it is.
    @property
    def shape(self):
        return _SHAPE_NAMES[self._shape]

    @property
    def centers(self):
        return self._centers

    def __len__(self):
        return self._centers.size

    def __repr__(self):
        return f"Instrument.{self.shape}({len(self)} channels)"

    def window(self):
        """(lo, hi) [N]: the closed window of every channel [cm-1]."""
        c = self._centers
        if self._shape == TABULATED:
            return c + self._offsets[0], c + self._offsets[-1]
        if self._shape == BOXCAR:
            h = self._parameter/2.
        elif self._shape == TRIANGLE:
            h = self._parameter
        else:
            h = self._half_width
        return c - h, c + h

    def columns(self, grid):
        """(start, end) int64 [N]: channel c covers the columns start_c <= j < end_c of an
        ascending grid."""
        grid = np.asarray(grid, dtype=np.float64)
        lo, hi = self.window()
        return (np.searchsorted(grid, lo, side="left").astype(np.int64),
                np.searchsorted(grid, hi, side="right").astype(np.int64))

    def covered(self, grid):
        """bool [N]: the window holds points and lies wholly inside [grid[0], grid[-1]]."""
        grid = np.asarray(grid, dtype=np.float64)
        lo, hi = self.window()
        start, end = self.columns(grid)
        return (end > start) & (lo >= grid[0]) & (hi <= grid[-1])

    def _weights(self, delta, rows):
        """w(Delta) of the channels `rows` (int [N]) at Delta [N, M]."""
        shape = self._shape
        if shape == BOXCAR:
            return np.ones_like(delta)
        if shape == TABULATED:
            table = self._response if self._response.ndim == 2 else self._response[None, :]
            out = np.empty_like(delta)
            for i, c in enumerate(rows):
                out[i] = np.interp(delta[i], self._offsets,
                                   table[c if table.shape[0] > 1 else 0])
            return out
        p = self._parameter[rows][:, None]
        if shape == TRIANGLE:
            return 1. - np.abs(delta)/p
        if shape == GAUSSIAN:
            x = delta/p
            return np.exp(-GAUSSIAN_G*(x*x))
        two_l = 2.*p
        if shape == FTS:
            return _sinc(two_l*delta)
        shift = 1./(2.*p)
        side = _sinc(two_l*(delta - shift)) + _sinc(two_l*(delta + shift))
        return 0.54*_sinc(two_l*delta) + 0.23*side

    def response(self, nu):
        """The reference formula: float64 [N, len(nu)], w_c(nu - nu_c) inside each channel's
        closed window [lo_c, hi_c] (by searchsorted on `nu`, which must be ascending), 0
        outside."""
        nu = np.asarray(nu, dtype=np.float64)
        if nu.ndim != 1:
            raise ValueError("nu must be 1-d.")
        rows = np.arange(len(self))
        delta = nu[None, :] - self._centers[:, None]
        weights = self._weights(delta, rows)
        start, end = self.columns(nu)
        j = np.arange(nu.size)[None, :]
        return np.where((j >= start[:, None]) & (j < end[:, None]), weights, 0.)

    def apply(self, nu, values):
        """The numpy reference of the channel values of `values` [..., len(nu)] on the grid
        `nu`: [..., N], NaN as in the module's rules."""
        nu = np.asarray(nu, dtype=np.float64)
        w = self.response(nu)
        total = w.sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            out = (np.asarray(values, dtype=np.float64) @ w.T)/total
        bad = ~self.covered(nu) | ~(total > 0.)
        return np.where(bad, np.nan, out)

    # The engine's copy.
    def _create(self, engine, grid_handle):
        shape = self._shape
        table = shape == TABULATED
        return engine.instrument_create(
            grid_handle, shape, self._centers, None if table else self._parameter,
            self._half_width, self._offsets if table else None,
            self._response if table else None)


def resident_instrument(engine, instrument, grid):
    """Handle of `instrument` bound to the engine's resident copy of `grid` (mt_ckd.resident_grid):
    created once per (Instrument, resident grid) and kept while both live; nothing is uploaded
    again per call."""
    from .mt_ckd import resident_grid
    grid_handle = resident_grid(engine, grid)
    cache = engine.__dict__.setdefault("_resident_instruments", [])
    grids = {entry[1]: entry[2] for entry in engine.__dict__.get("_resident_grids", [])}
    found = None
    for entry in list(cache):
        target = entry[0]()
        # An entry whose instrument is gone, or whose grid copy is not resident any more (freed,
        # or uploaded again after the array changed), goes.
        if target is None or grids.get(entry[1]) != entry[2]:
            engine.synchronize()    # queued kernels may still read its tables
            engine.instrument_free(entry[3])
            cache[:] = [other for other in cache if other is not entry]
        elif target is instrument and entry[1] == grid_handle:
            found = entry
    if found is None:
        handle = instrument._create(engine, grid_handle)
        found = (weakref.ref(instrument), grid_handle, grids[grid_handle], handle)
        cache.append(found)
    return found[3]


def brightness_temperature(radiance, nu):
    """Brightness temperature [K] of channel radiances at their centres nu [cm-1]:
    (C2*nu)/log1p((((C1*nu)*nu)*nu)/R), 0 where R <= 0, NaN where R is NaN."""
    from .spectroscopy import PLANCK_C1, PLANCK_C2
    radiance = np.asarray(radiance, dtype=np.float64)
    nu = np.asarray(nu, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t = (PLANCK_C2*nu)/np.log1p((((PLANCK_C1*nu)*nu)*nu)/radiance)
    return np.where(np.isnan(radiance), np.nan, np.where(radiance > 0., t, 0.))
