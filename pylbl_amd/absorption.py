"""Spectroscopy.compute_absorption on the host: which gases some mechanism computes
(present_gases), the levels [a, b) of the atmosphere and how kernels are queued onto them into
blocks in HBM (_Levels), the "total" block in its two queue orders (queue_total, total_into), the
guard around everything a call queues (pipeline), and compute_levels: a driver over one function
per route, whose blocks and results a _Results collects.  The functions take the Spectroscopy
first; total_into and compute_levels (as _compute_levels) are also its methods.
"""
from collections import namedtuple
import contextlib
import ctypes
import threading

import numpy as np

from .synthetic import grid_arguments

# A gas that some mechanism computes: its Gas, continua (a list) and cross-section, or None; and
# all of them: their engine (None without any), in queue order, the one with the most lines.
PresentGas = namedtuple("PresentGas", "name lines continua cross")
Present = namedtuple("Present", "engine gases heavy")


def present_gases(spec, levels, total=False):
    """Present: the gases of the atmosphere that some mechanism computes, lightest lines table
    first (with `total`: in "total" order, the heaviest first and the others behind it as they
    were).  levels: a _Levels, whose first level a gas with a deferred error is tried on."""
    engine, gases = None, []
    for name in spec.atmosphere.gases:
        data = spec._molecule(name)
        lines = data.gas
        if lines is not None and lines.molecule is None:
            # Deferred errors (unknown alias) surface here like in the reference.
            lines.absorption_coefficients(levels.temperature[:1], levels.pressure[:1],
                                          levels.mole_fractions[name][:1], spec.grid)
            lines = None
        continua = data.gas_continua or []
        cross = data.cross_section
        if lines is None and not continua and cross is None:
            continue
        if engine is None:
            engine = lines.engine if lines is not None else \
                (continua[0].engine if continua else cross.engine)
        gases.append(PresentGas(name, lines, continua, cross))
    # "total" (one block for everything): the gas with the most transitions is queued FIRST and
    # finished LAST.  Its lines call is the longest (with the pedestal removed it ends in a
    # serial chain), so everything it does in buffers of its own -- prologue, far-field series,
    # accumulate, pedestal pre-pass -- starts at once and runs beside the other gases' calls,
    # while the kernels that touch its block, and the copies that hand that block to the host
    # piece by piece, are kept back (LBL_DEFER_FINISH) until the others have been queued: it
    # stays the last to add into a shared block, and its copies queue up behind the other gases'
    # copies, not in front of them.  (Units are independent, spectroscopy.py:166,179; results
    # are reported in the atmosphere's order.) Per-gas blocks ("gas", "all") are the other way
    # round: the link to the host is the bottleneck there (one block per gas to copy), so the
    # lightest gas goes first -- its block is complete early and travels beside the kernels of
    # the others -- and the heaviest last, delivering its block piece by piece while it computes
    # (profiles/r03_ab_api.txt).
    gases.sort(key=lambda gas: gas.lines.num_lines if gas.lines is not None else -1)
    heavy = gases[-1] if gases and gases[-1].lines is not None else None
    if total and heavy is not None:
        gases = [heavy] + gases[:-1]
    return Present(engine, gases, heavy)


class _Levels(object):
    """The flat levels [a, b) of the atmosphere, and how the kernels of one (gas, mechanism) are
    queued onto them into a block in HBM, which the first of them writes and the others add
    into.  pieces: runs of tiles of a lines call that delivers its result (default: the
    Spectroscopy's delivery_pieces)."""
    def __init__(self, spec, a, b, remove_pedestal, range_policy, pieces=None):
        self.spec, atmosphere = spec, spec.atmosphere
        self.temperature = atmosphere.temperature.ravel()[a:b]
        self.pressure = atmosphere.pressure.ravel()[a:b]
        # Every gas at every level, the dictionary the continua read (spectroscopy.py:173).
        self.mole_fractions = {name: x.ravel()[a:b] for name, x in atmosphere.gases.items()}
        self.count = self.temperature.size
        self.remove_pedestal, self.range_policy = remove_pedestal, range_policy
        self.pieces = spec.delivery_pieces if pieces is None else pieces
        self.written = set()        # ids of the blocks something was queued into

    def adds(self, block):
        """True if the next kernel must add to what `block` holds."""
        written = id(block) in self.written
        self.written.add(id(block))
        return written

    def zero_unless_written(self, block):
        """Clears a block that nothing wrote yet: the kernels that follow only add."""
        if not self.adds(block):
            block.engine.fill_zero(block, asynchronous=True)

    def lines_into(self, gas, block, deliver=None, defer=False):
        """The lines of `gas`.  deliver: the page-locked view that receives the block piece by
        piece while the call computes; defer: LBL_DEFER_FINISH."""
        gas.lines.absorption_coefficients(
            self.temperature, self.pressure, self.mole_fractions[gas.name], self.spec.grid,
            remove_pedestal=self.remove_pedestal, range_policy=self.range_policy,
            scale_density=True, out=block, accumulate=self.adds(block),
            asynchronous=True, farfield=self.spec.farfield, deliver=deliver,
            pieces=self.pieces, defer_finish=defer)

    def continua_into(self, continua, block):
        """The continua of a list (of any gases; nothing for an empty one)."""
        # All of them in one pass over the grid where they are this package's (one launch that
        # writes the block once instead of a read-modify-write pass per continuum; the same
        # bits: csrc/continuum.h, group kernels); anything else one by one.
        if not continua:
            return
        from .mt_ckd import BandedContinuum, spectra_levels_many
        if all(isinstance(c, BandedContinuum) for c in continua):
            spectra_levels_many(continua, self.temperature, self.pressure,
                                self.mole_fractions, self.spec.grid, block,
                                accumulate=self.adds(block), asynchronous=True)
            return
        for continuum in continua:
            continuum.spectra_levels(self.temperature, self.pressure, self.mole_fractions,
                                     self.spec.grid, out=block,
                                     accumulate=self.adds(block), asynchronous=True)

    def cross_into(self, gas, block):
        """The cross-section of `gas` (nothing where it has none)."""
        if gas.cross is not None:
            gas.cross.absorption_coefficients(
                self.spec.grid, self.temperature, self.pressure,
                volume_mixing_ratio=self.mole_fractions[gas.name], out=block,
                accumulate=self.adds(block), asynchronous=True)


@contextlib.contextmanager
def pipeline(engine, give_back=()):
    """Everything from the first queued call of a result to its final wait is one pipeline on the
    engine: calls add into shared blocks in a fixed order and one of them may be kept back, so
    another thread's calls must not come in between (Engine.pipeline; single calls from other
    threads -- Gas.absorption_coefficient -- only wait for their turn).  If anything fails on the
    way, what the engine still holds for this call is dropped and waited for BEFORE the blocks and
    page-locked arrays go back to their pools: a call kept back (LBL_DEFER_FINISH) would otherwise
    apply itself, and copy, into recycled memory the next time the engine is synchronized.
    engine: None where no mechanism computes anything.  give_back: pooled blocks that go back last,
    inside the pipeline, whether the body failed or not (paths._sweep_runs).  compute_levels gives
    its own back only on success: after a failure garbage collection frees them, behind this."""
    with (engine.pipeline if engine is not None else contextlib.nullcontext()):
        try:
            yield
        except BaseException:
            if engine is not None:
                try:
                    engine.cancel_deferred()
                    engine.synchronize()
                except Exception:       # the first error is the one to report
                    pass
            raise
        finally:
            for block in give_back:
                engine.blocks.give(block)


def queue_total(spec, levels, present, total, deliver):
    """Queues every gas's kernels into the one block `total` (`present` in "total" order: the
    heavy gas first), in the order spec.total_order names.  deliver and the value returned: see
    total_into."""
    if present.heavy is not None and spec.total_order == "heavy_last":
        return _total_heavy_last(levels, present, total, deliver)
    return _total_kept_back(levels, present, total, deliver)


def _total_heavy_last(levels, present, total, deliver):
    # The short continuum and cross-section kernels of every gas first, the lighter gases'
    # lines behind them, the heaviest gas last: each run of tiles it finishes completes
    # that part of the block, which goes to the host while the next run computes (its
    # pedestal pass is short since round 4, so the first copy starts a third of the way
    # into the call instead of behind everything).  (Lines first and the slot kernels
    # behind them was tried: the slot kernels then wait for the first gas's pedestal to be
    # applied and the heaviest gas is queued later, 1.58 -> 1.70 ms.)
    # (every continuum of every gas in ONE pass -- the block is written once -- then the
    # cross-sections.  The additions into the block therefore run c(g1), c(g2), ..., x(g1),
    # x(g2), ..., lines -- not the reference's gas-by-gas order, spectroscopy.py:225-234:
    # the continua are bit-identical to the one-by-one sum among themselves, the total may
    # differ from the reference's order of additions in its last bits, within the parity
    # bar: tests/test_gpu_api.py::test_total_with_continuum_and_cross_section_of_two_gases)
    levels.continua_into([c for gas in present.gases for c in gas.continua], total)
    for gas in present.gases:
        levels.cross_into(gas, total)
    levels.zero_unless_written(total)
    for gas in present.gases[1:]:
        if gas.lines is not None:
            levels.lines_into(gas, total)
    levels.lines_into(present.heavy, total, deliver=deliver)
    return False


def _total_kept_back(levels, present, total, deliver):
    # Every gas adds into one block.  The heavy gas's slot kernels go first (the first of them
    # writes the block -- or the engine clears it), then its lines call, kept back; the other
    # gases' lines with their short continuum and cross-section kernels behind them; then the
    # heavy gas's last kernels and the delivery of the finished block.
    kept_back, others = False, present.gases
    if present.heavy is not None:
        heavy, others = others[0], others[1:]
        levels.continua_into(heavy.continua, total)
        levels.cross_into(heavy, total)
        levels.zero_unless_written(total)
        levels.lines_into(heavy, total, deliver=deliver, defer=deliver is not None)
        kept_back = deliver is not None and total.engine.deferred()
    for gas in others:
        if gas.lines is not None:
            levels.lines_into(gas, total)
        levels.continua_into(gas.continua, total)
        levels.cross_into(gas, total)
    if kept_back:
        total.engine.finish_deferred()
        return False
    # (No gas with lines -- or a call the engine could not keep back, e.g. without a pedestal
    # pass: it added at once and delivered a block that was not complete; the copy the caller
    # queues behind everything is the one that counts.)
    return True


def total_into(spec, block, a, b, remove_pedestal, range_policy="reference", deliver=None,
               gases=None):
    """Queues the "total" absorption of the flat levels [a, b) of the atmosphere into `block`
    (DeviceSpectra [b - a, >= padded grid]) the way compute_absorption("total") does: the
    heaviest gas first in line and last to add (queue_total), or zeros where no mechanism
    computes any gas.  The block is complete behind what is queued (Engine.synchronize).
    deliver: the page-locked [levels, columns] view the last lines call hands the finished block
    to, piece by piece -- or None: the block stays in HBM.  Returns True when `deliver` was not
    handed the finished block: the caller copies it behind everything.  gases: what
    present_gases(..., total=True) returned, for callers that queue several ranges in one call."""
    levels = _Levels(spec, a, b, remove_pedestal, range_policy)
    present = present_gases(spec, levels, total=True) if gases is None else gases
    if not present.gases:
        block.engine.fill_zero(block, asynchronous=True)
        return True
    return queue_total(spec, levels, present, block, deliver)


def _zero_rows(views):
    for view in views:
        for row in view:
            ctypes.memset(row.ctypes.data, 0, row.size*8)


class _Results(object):
    """What the routes of compute_levels leave behind: page-locked result arrays by name, filled
    by queued copies; views of them that read zero; blocks in HBM that go back to the pool once
    everything has arrived; and the host route's finished blocks by (gas, mechanism)."""
    def __init__(self, engine, levels, n):
        self.engine, self.levels, self.n = engine, levels, n
        self.arrays, self.host_blocks = {}, {}
        self.zero_views, self.in_flight = [], []

    def block(self):
        return self.engine.blocks.take(self.levels, self.n)         # recycled: engine.DevicePool

    def array(self, name, shape):
        return self.arrays.setdefault(name, self.engine.host_array(shape))

    def home(self, block, view, delivered=False):
        """The first columns of `block` go home to `view` (page-locked, rows contiguous) -- by one
        copy queued now, from HBM straight into its place, which runs beside what is queued
        later; or (delivered) by the lines call that was handed `view` -- and the block goes back
        to the pool after the wait.  block None: no mechanism writes `view`, which reads zero
        (40 MB per level at 5 M points; zeroed in wait())."""
        if block is None:
            self.zero_views.append(view)
            return
        if not delivered:
            block.to_host_into(view, view.shape[1], asynchronous=True)
        self.in_flight.append(block)

    def wait(self):
        # float64 [rows, columns] views with contiguous rows are zeroed by a helper thread beside
        # the kernels (ctypes releases the interpreter lock during memset).
        filler = threading.Thread(target=_zero_rows, args=(self.zero_views,)) \
            if self.zero_views else None
        if filler is not None:
            filler.start()
        if self.engine is not None:
            self.engine.synchronize()
        if filler is not None:
            filler.join()
        for block in self.in_flight:
            self.engine.blocks.give(block)


def _host_route(spec, levels, present, out):
    # Too large to keep: one host block per mechanism, summed by numpy in _assemble.
    blocks = out.host_blocks
    for gas in present.gases:
        if gas.lines is not None:
            blocks[(gas.name, 0)] = gas.lines.absorption_coefficients(
                levels.temperature, levels.pressure, levels.mole_fractions[gas.name], spec.grid,
                remove_pedestal=levels.remove_pedestal, range_policy=levels.range_policy,
                scale_density=True, farfield=spec.farfield)[:, :spec.grid.size]
        for continuum in gas.continua:
            values = continuum.spectra_levels(levels.temperature, levels.pressure,
                                              levels.mole_fractions, spec.grid)
            blocks[(gas.name, 1)] = blocks[(gas.name, 1)] + values \
                if (gas.name, 1) in blocks else values
        if gas.cross is not None:
            blocks[(gas.name, 2)] = gas.cross.absorption_coefficients(
                spec.grid, levels.temperature, levels.pressure,
                volume_mixing_ratio=levels.mole_fractions[gas.name])


def _gas_route(spec, levels, present, out):
    for gas in present.gases:
        block = out.block()
        view = out.array(gas.name, (levels.count, spec.grid.size))
        # The lines call goes last and delivers the block itself; or first, and the block goes
        # home in one copy while the next gas computes.
        delivers = gas.lines is not None and \
            (gas is present.gases[-1] or spec.gas_delivery == "each")
        if gas.lines is not None and not delivers:
            levels.lines_into(gas, block)
        levels.continua_into(gas.continua, block)
        levels.cross_into(gas, block)
        if delivers:
            levels.lines_into(gas, block, deliver=view)
        out.home(block, view, delivered=delivers)


def _all_route(spec, levels, present, out):
    for gas in present.gases:
        last = gas is present.gases[-1]
        values = out.array(gas.name, [levels.count, len(spec.output.mechanisms), spec.grid.size])
        continuum_sum = out.block() if gas.continua else None
        cross_sum = out.block() if gas.cross is not None else None
        levels.continua_into(gas.continua, continuum_sum)
        levels.cross_into(gas, cross_sum)
        out.home(continuum_sum, values[:, 1, :])
        out.home(cross_sum, values[:, 2, :])
        lines_sum = out.block() if gas.lines is not None else None
        if lines_sum is not None:
            levels.lines_into(gas, lines_sum, deliver=values[:, 0, :] if last else None)
        out.home(lines_sum, values[:, 0, :], delivered=last)


def _assemble(spec, mode, levels, out):
    """{variable name: array}: the routes' arrays; where a name has none, zeros -- a gas that
    nothing computes -- with the host route's blocks added ("all": put in their slots)."""
    columns, slots = spec.grid.size, len(spec.output.mechanisms)
    beta = {}
    for name in (["total"] if mode == "total" else spec.atmosphere.gases):
        values = out.arrays.get(name)
        if values is None:
            values = np.zeros((levels, slots, columns) if mode == "all" else (levels, columns))
            for (gas, slot), block in out.host_blocks.items():
                if mode == "all" and gas == name:
                    values[:, slot, :] = block
                elif mode == "total" or gas == name:
                    values += block
        beta[name if mode == "total" else "{}_absorption".format(name)] = values
    return beta


def compute_levels(spec, a, b, mode, remove_pedestal, range_policy):
    """The three mechanism slots for the flat levels [a, b) of the atmosphere: {variable name:
    array with the levels as leading dimension} ("total" under mode "total")."""
    # ("all" is bound by the link -- four 40 MB blocks per level for H2O + CO2 -- and its
    # copies are queued back to back as they are: cutting the last one into pieces only
    # puts gaps into that queue, 3.6 -> 4.1 ms per call.)
    levels = _Levels(spec, a, b, remove_pedestal, range_policy,
                     pieces=1 if mode == "all" else None)
    if levels.count == 0:
        # A rank without levels (fewer levels than GPUs): empty blocks of the right shape.
        return _assemble(spec, mode, 0, _Results(None, 0, 0))
    v0, vn, n_per_v = grid_arguments(spec.grid)
    n = (vn - v0)*n_per_v
    present = present_gases(spec, levels, total=mode == "total")
    out = _Results(present.engine, levels.count, n)
    # Queue every kernel before waiting: one batched call per (molecule, mechanism) for
    # all levels, n*k applied in the kernel epilogue, spectra left in HBM until the end;
    # the sums over mechanisms ("gas") and over gases ("total") happen on the device.
    # Within a block the short continuum and cross-section kernels go first and the lines
    # last: the lines call that completes the LAST block of the whole call hands its result
    # to the host itself, piece by piece while it computes (lbl_compute_streamed), so no
    # copy is left standing behind the last kernel.
    with pipeline(present.engine):
        if levels.count*n*8 > spec.device_output_limit:
            _host_route(spec, levels, present, out)
        elif mode == "total" and present.gases:
            total, view = out.block(), out.array("total", (levels.count, spec.grid.size))
            out.home(total, view, delivered=not queue_total(spec, levels, present, total, view))
        elif mode == "gas":
            _gas_route(spec, levels, present, out)
        elif mode == "all":
            _all_route(spec, levels, present, out)
        out.wait()      # and only here, not where the pipeline fails, the blocks go back
    return _assemble(spec, mode, levels.count, out)
