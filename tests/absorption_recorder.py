"""What tests/test_absorption_queue_host.py and tests/golden/make_absorption_queue_log.py share: a
stand-in for pylbl_amd.engine.Engine that computes nothing and writes down every call the host side
of Spectroscopy.compute_absorption makes on it, and the matrix of cases whose logs are compared.

The real back ends (Gas, the MT-CKD continua, CrossSection) run on the stand-in, so the flags and
per-level arrays they pass are in the log.  A log is a list of strings "method(name=value, ...)":
blocks in HBM and page-locked host arrays are named by order of first appearance in the log
("block0", "host1"; a view of a host array adds its offset, shape and strides), any other array is
its shape and the first 8 hex digits of the SHA-1 of its float64 bytes."""
from collections import namedtuple
import contextlib
import hashlib
import os

import numpy as np

from pylbl_amd import arts_crossfit, synthetic
from pylbl_amd.database import MemoryDatabase

MT_CKD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mt_ckd_bands.npz")

# The calls that queue work for the GPU: `fail_at` counts these.
KERNEL_CALLS = ("compute", "continuum_compute", "continuum_compute_many", "xsec_compute",
                "fill_zero", "path_compute")


class StandInFailure(RuntimeError):
    """Raised by the call the case asked to fail."""


class SecondFailure(RuntimeError):
    """Raised by synchronize() after a StandInFailure: the error that must not be reported."""


def _digest(values):
    a = np.ascontiguousarray(values, dtype=np.float64)
    shape = "x".join(str(s) for s in a.shape) or "scalar"
    return "{}#{}".format(shape, hashlib.sha1(a.tobytes()).hexdigest()[:8])


class Block(object):
    """DeviceSpectra stand-in: [levels, n] in an HBM that is not there."""
    pointer = 1

    def __init__(self, engine, levels, n, parent=None):
        self.engine, self.shape, self.parent = engine, (int(levels), int(n)), parent

    def to_host_into(self, target, columns=None, asynchronous=False):
        columns = self.shape[1] if columns is None else int(columns)
        if target.shape != (self.shape[0], columns) or columns > self.shape[1]:
            raise ValueError("target must be float64[rows, columns] with contiguous rows.")
        self.engine.record("to_host_into", block=self, target=target, columns=columns,
                           asynchronous=asynchronous)
        return target

    def rows(self, count):
        if not 0 < int(count) <= self.shape[0]:
            raise ValueError(f"rows({count}) of a block of {self.shape[0]} rows.")
        return Block(self.engine, count, self.shape[1], parent=self)


class Pool(object):
    """DevicePool stand-in: blocks come back to it and are handed out again, last in first out."""
    def __init__(self, engine):
        self.engine, self.idle = engine, {}

    def take(self, levels, n):
        shape = (int(levels), int(n))
        idle = self.idle.get(shape)
        block = idle.pop() if idle else Block(self.engine, *shape)
        self.engine.record("blocks.take", levels=shape[0], n=shape[1], block=block)
        return block

    def give(self, block):
        self.engine.record("blocks.give", block=block)
        self.idle.setdefault(block.shape, []).append(block)


class Pipeline(object):
    def __init__(self, engine):
        self.engine = engine

    def __enter__(self):
        self.engine.record("pipeline.enter")

    def __exit__(self, *error):
        self.engine.record("pipeline.exit")
        return False


class RecordingEngine(object):
    """Engine stand-in.  deferred_answer: what deferred() says right after a call with
    defer_finish=True (both answers occur on a real engine: it cannot keep back a call without a
    pedestal pass).  begin() starts the log of a case; fail_at=k makes the k-th kernel call of the
    case raise StandInFailure, after which synchronize() raises SecondFailure once."""
    handle = 1

    def __init__(self):
        self.blocks, self.pipeline = Pool(self), Pipeline(self)
        self.handles = 0
        self.begin()

    def begin(self, deferred_answer=True, fail_at=None):
        self.log, self.names, self.hosts = [], {}, []
        self.deferred_answer, self.fail_at = deferred_answer, fail_at
        self.kept_back = self.failed = False
        self.kernel_calls = 0

    # -- the log ---------------------------------------------------------------------------
    def describe(self, value):
        if isinstance(value, Block):
            if value.parent is not None:
                return "{}[:{}]".format(self.describe(value.parent), value.shape[0])
            return self.names.setdefault(id(value), "block{}".format(
                sum(1 for x in self.names.values() if x.startswith("block"))))
        if isinstance(value, np.ndarray):
            base = value
            while isinstance(base.base, np.ndarray):
                base = base.base
            for host in self.hosts:
                if host is base:
                    name = self.names.setdefault(id(host), "host{}".format(
                        sum(1 for x in self.names.values() if x.startswith("host"))))
                    if value.shape == host.shape and value.strides == host.strides:
                        return name
                    offset = (value.__array_interface__["data"][0] -
                              host.__array_interface__["data"][0])//8
                    return "{}[+{} {} /{}]".format(
                        name, offset, "x".join(map(str, value.shape)),
                        ":".join(str(s//8) for s in value.strides))
            return _digest(value)
        if isinstance(value, (list, tuple)) and value and \
                all(isinstance(x, (float, np.floating)) for x in value):
            return _digest(value)
        if isinstance(value, (list, tuple)):
            return "[{}]".format(", ".join(self.describe(x) for x in value))
        if isinstance(value, (bool, np.bool_)) or value is None:
            return str(value)
        if isinstance(value, (int, np.integer)):
            return str(int(value))
        if isinstance(value, (float, np.floating)):
            return repr(float(value))
        return str(value)

    def record(self, method, **arguments):
        self.log.append("{}({})".format(method, ", ".join(
            "{}={}".format(k, self.describe(v)) for k, v in arguments.items())))
        if method in KERNEL_CALLS:
            self.kernel_calls += 1
            if self.kernel_calls == self.fail_at:
                self.failed = True
                raise StandInFailure("kernel call {} of the case".format(self.fail_at))

    def _upload(self, method, **arguments):
        self.handles += 1
        self.record(method, handle=self.handles, **arguments)
        return self.handles

    def _host_result(self, levels, n):
        """What a call without `out` returns: a host array that holds the call's number, so that
        the sums the caller forms of such arrays show in the digest of its result."""
        out = self.host_array((levels, n), log=False)
        out[...] = float(len(self.log))
        return out

    # -- uploads ---------------------------------------------------------------------------
    def load(self, table):
        return self._upload("load", formula=table.formula, num_lines=table.num_lines)

    def load_sqlite(self, path, name):
        return self._upload("load_sqlite", path=os.path.basename(str(path)), name=name)

    def load_grid(self, wavenumber):
        return self._upload("load_grid", grid=np.asarray(wavenumber))

    def load_continuum(self, bands):
        return self._upload("load_continuum", kinds=[int(band[0]) for band in bands])

    def load_xsec(self, bands):
        return self._upload("load_xsec", sizes=[int(f.size) for f, _ in bands])

    def free(self, molecule):
        pass

    free_grid = free_continuum = free_xsec = free

    # -- memory ----------------------------------------------------------------------------
    def host_array(self, shape, log=True):
        array = np.zeros(tuple(int(x) for x in shape))
        self.hosts.append(array)
        if log:
            self.record("host_array", shape=list(array.shape), array=array)
        return array

    def fill_zero(self, out, asynchronous=False):
        self.record("fill_zero", out=out, asynchronous=asynchronous)
        return out

    # -- kernels ---------------------------------------------------------------------------
    def compute(self, molecule, temperature, pressure, vmr, v0, vn, n_per_v, cut_off=25,
                remove_pedestal=False, range_policy="reference", out=None, scale_density=False,
                accumulate=False, asynchronous=False, want_evals=False, farfield=False,
                deliver=None, pieces=4, defer_finish=False):
        levels, n = np.atleast_1d(temperature).size, (int(vn) - int(v0))*int(n_per_v)
        if out is not None and tuple(out.shape) != (levels, n):
            raise ValueError(f"out has shape {out.shape}, need {(levels, n)}.")
        if deliver is not None and (not isinstance(out, Block) or deliver.ndim != 2 or
                                    deliver.shape[0] != levels or deliver.shape[1] > n):
            raise ValueError("deliver must be float64[levels, columns <= n] with a device `out`.")
        self.record("compute", molecule=molecule, t=np.atleast_1d(temperature),
                    p=np.atleast_1d(pressure), vmr=np.atleast_1d(vmr), v0=v0, vn=vn,
                    n_per_v=n_per_v, cut_off=cut_off, remove_pedestal=remove_pedestal,
                    range_policy=range_policy, out=out, scale_density=scale_density,
                    accumulate=accumulate, asynchronous=asynchronous, farfield=farfield,
                    deliver=deliver, pieces=pieces, defer_finish=defer_finish)
        if defer_finish:
            self.kept_back = bool(self.deferred_answer)
        return self._host_result(levels, n) if out is None else out

    def _slot(self, method, levels, n, out, **arguments):
        if out is not None and (out.shape[0] != levels or out.shape[1] < n):
            raise ValueError(f"out has shape {out.shape}, need ({levels}, >= {n}).")
        self.record(method, n=n, out=out, **arguments)
        return self._host_result(levels, n) if out is None else out

    def continuum_compute(self, continuum, grid, n, temperature, pressure, vmr, out=None,
                          accumulate=False, asynchronous=False):
        t = np.atleast_1d(temperature)
        return self._slot("continuum_compute", t.size, n, out, continuum=continuum, grid=grid,
                          t=t, p=np.atleast_1d(pressure), vmr=np.asarray(vmr),
                          accumulate=accumulate, asynchronous=asynchronous)

    def continuum_compute_many(self, continua, grid, n, temperature, pressure, vmr, out,
                               accumulate=False, asynchronous=False):
        if not isinstance(out, Block):
            raise ValueError("continuum_compute_many writes a block in HBM (DeviceSpectra).")
        t = np.atleast_1d(temperature)
        return self._slot("continuum_compute_many", t.size, n, out,
                          continua=[int(c) for c in continua], grid=grid, t=t,
                          p=np.atleast_1d(pressure), vmr=np.asarray(vmr), accumulate=accumulate,
                          asynchronous=asynchronous)

    def xsec_compute(self, xsec, grid, n, temperature, pressure, vmr=None, out=None,
                     accumulate=False, asynchronous=False):
        t = np.atleast_1d(temperature)
        return self._slot("xsec_compute", t.size, n, out, xsec=xsec, grid=grid, t=t,
                          p=np.atleast_1d(pressure),
                          vmr=None if vmr is None else np.atleast_1d(vmr),
                          accumulate=accumulate, asynchronous=asynchronous)

    def path_compute(self, beta, columns, n_paths, levels_per_path, level_begin, lengths, carry,
                     optical_depth=None, transmittance=None, band_start=None, cumulative=False,
                     from_last=False, asynchronous=False):
        self.record("path_compute", beta=beta, columns=columns, n_paths=n_paths,
                    levels_per_path=levels_per_path, level_begin=level_begin,
                    lengths=np.asarray(lengths), carry=carry, optical_depth=optical_depth,
                    transmittance=transmittance,
                    band_start=None if band_start is None else np.asarray(band_start),
                    cumulative=cumulative, from_last=from_last, asynchronous=asynchronous)

    # -- the queue -------------------------------------------------------------------------
    def deferred(self):
        self.record("deferred", answer=self.kept_back)
        return self.kept_back

    def finish_deferred(self):
        self.record("finish_deferred")
        self.kept_back = False

    def cancel_deferred(self):
        self.record("cancel_deferred")
        self.kept_back = False

    def synchronize(self):
        self.record("synchronize")
        self.kept_back = False
        if self.failed:
            self.failed = False
            raise SecondFailure("synchronize after the failed call")


@contextlib.contextmanager
def installed(engine):
    """`engine` as the default engine of every back end, and the MT-CKD tables of tests/golden."""
    from pylbl_amd import engine as engine_module, gas_optics, mt_ckd
    modules = (gas_optics, mt_ckd, arts_crossfit, engine_module)
    before = [module.default_engine for module in modules]
    tables = os.environ.get("PYLBL_MT_CKD")
    for module in modules:
        module.default_engine = lambda device=0: engine
    os.environ["PYLBL_MT_CKD"] = MT_CKD
    try:
        yield engine
    finally:
        for module, function in zip(modules, before):
            module.default_engine = function
        if tables is None:
            del os.environ["PYLBL_MT_CKD"]
        else:
            os.environ["PYLBL_MT_CKD"] = tables


# ---------------------------------------------------------------------------------------------
# The gases.  Each entry: formula -> (lines or None, cross-section or not); the continua come
# with the formula (H2O two, CO2 and O3 one, the others none).  A formula without lines is in the
# database without partition sums, as the reference's ingest leaves a molecule it has no lines for.
GAS_SETS = {
    # H2O with lines and both continua; CO2 with fewer lines, a continuum and a cross-section.
    "lighter second": {"H2O": (40, False), "CO2": (20, True)},
    # The second gas is the heavier one.
    "heavier second": {"H2O": (40, False), "CO2": (90, True)},
    # Also a gas with only a continuum (O3), one with only a cross-section (CFC11), one that
    # nothing computes (Ar), and the lines gases not in order of their size.
    "mixed": {"H2O": (40, True), "O3": (None, False), "CFC11": (None, True), "Ar": (None, False),
              "CO2": (90, False), "CH4": (7, False)},
    # No gas has lines: nothing is the heaviest.
    "no lines": {"H2O": (None, False), "CFC11": (None, True)},
    # Nothing is present: no engine either.
    "nothing": {"Ar": (None, False)},
    # HCl is not in the database.
    "unknown alias": {"H2O": (40, False), "HCl": (None, False)},
}
GRID = np.arange(20., 60., 0.25)        # 160 points, rows padded to 164


def spectroscopy(gas_set, levels, directory, shape=None):
    """(Spectroscopy on a new RecordingEngine, the engine).  The back ends are built here, so the
    engine's log holds their uploads when this returns."""
    from pylbl_amd import Spectroscopy
    gases = GAS_SETS[gas_set]
    tables, files = [], {}
    for i, (formula, (lines, cross)) in enumerate(gases.items()):
        if formula == "HCl":
            continue
        table = synthetic.line_table(formula, 1., 100., num_lines=lines or 3, seed=300 + i,
                                     tips_range=(150, 400))
        if lines is None:
            table.tips_data = np.zeros((0, 0))
        tables.append(table)
        if cross:
            files[formula] = os.path.join(str(directory), formula + ".npz")
            if not os.path.exists(files[formula]):
                arts_crossfit.write_npz(files[formula], synthetic.cross_section_bands(
                    seed=21 + i, ranges=((25. + 5*i, 45. + 5*i),), spacing=0.5))
    rng = np.random.default_rng(17)
    count = levels if shape is None else int(np.prod(shape))
    atmosphere = synthetic.Atmos(
        p=np.linspace(2.e4, 9.e4, count).reshape(shape or (count,)),
        t=np.linspace(210., 290., count).reshape(shape or (count,)),
        vmr={formula: rng.uniform(1e-6, 1e-3, count).reshape(shape or (count,))
             for formula in gases})
    engine = RecordingEngine()
    with installed(engine):
        spec = Spectroscopy(atmosphere, GRID, MemoryDatabase(tables, cross_sections=files))
        for formula in gases:
            data = spec._molecule(formula)
            if data.gas is not None and data.gas.molecule is None:
                _record_probe(engine, data.gas)
    return spec, engine


def _record_probe(engine, gas):
    """A Gas without a table never reaches the engine: its calls are written down here."""
    inner = gas.absorption_coefficients

    def absorption_coefficients(temperature, pressure, volume_mixing_ratio, grid, **keywords):
        engine.record("Gas.absorption_coefficients", formula=gas.formula,
                      t=np.atleast_1d(temperature), p=np.atleast_1d(pressure),
                      vmr=np.atleast_1d(volume_mixing_ratio), grid=np.asarray(grid),
                      **{k: v for k, v in sorted(keywords.items())})
        return inner(temperature, pressure, volume_mixing_ratio, grid, **keywords)
    gas.absorption_coefficients = absorption_coefficients


# ---------------------------------------------------------------------------------------------
# The cases.
Case = namedtuple("Case", "gas_set levels call mode remove_pedestal settings deferred_answer "
                          "fail_at")
Case.__new__.__defaults__ = ("absorption", "total", True, (), True, None)
DEFAULTS = dict(total_order="heavy_last", gas_delivery="each", delivery_pieces=4,
                device_output_limit=8 << 30, farfield=True)


def case_id(case):
    parts = [case.gas_set, "{} levels".format(case.levels), case.call, case.mode,
             "pedestal removed" if case.remove_pedestal else "pedestal kept"]
    parts += ["{}={}".format(k, v) for k, v in case.settings]
    if any(k == "total_order" for k, _ in case.settings):
        parts.append("deferred() says {}".format(case.deferred_answer))
    if case.fail_at is not None:
        parts.append("kernel call {} fails".format(case.fail_at))
    return ", ".join(parts)


def cases():
    out = []
    for gas_set in ("lighter second", "heavier second", "mixed", "no lines", "nothing"):
        for levels in (1, 3):
            for mode in ("all", "gas", "total"):
                for remove_pedestal in (True, False):
                    out.append(Case(gas_set, levels, mode=mode, remove_pedestal=remove_pedestal))
    for gas_set in ("lighter second", "heavier second", "mixed", "no lines"):
        for order in ("heavy_last", "deferred"):
            for answer in (True, False):
                out.append(Case(gas_set, 3, settings=(("total_order", order),),
                                deferred_answer=answer))
    for gas_set in ("lighter second", "heavier second", "mixed"):
        for delivery in ("each", "last"):
            out.append(Case(gas_set, 3, mode="gas", settings=(("gas_delivery", delivery),
                                                              ("delivery_pieces", 3))))
    for mode in ("all", "gas", "total"):
        out.append(Case("lighter second", 3, mode=mode, settings=(("farfield", False),)))
        for gas_set in ("mixed", "nothing"):
            out.append(Case(gas_set, 3, mode=mode, settings=(("device_output_limit", 0),)))
        out.append(Case("mixed", 3, call="no levels", mode=mode))
        out.append(Case("unknown alias", 3, mode=mode))
    out.append(Case("mixed", 3, call="range_policy skip"))
    # 4 levels as 2 paths of 2, one path per run: total_into through paths._sweep_runs.
    out.append(Case("mixed", 4, call="path"))
    out.append(Case("nothing", 4, call="path"))
    # The third kernel call fails: with the kept-back order that is the call after the one kept
    # back (H2O's continua, H2O's lines kept back, CO2's lines).
    for mode in ("all", "gas", "total"):
        out.append(Case("lighter second", 3, mode=mode, fail_at=3))
    out.append(Case("lighter second", 3, settings=(("total_order", "deferred"),), fail_at=3))
    out.append(Case("lighter second", 4, call="path", fail_at=3))
    return out


def _result(engine, values):
    return {name: engine.describe(np.asarray(value)) if np.asarray(value).dtype.kind == "f"
            else ",".join(str(x) for x in np.asarray(value).ravel())
            for name, value in values.items()}


def run_cases(directory):
    """{case id: {"log": [...], "result": {variable: description} or "error": [type, text]}}.
    The first entries, "uploads of <gas set>, <levels> levels", hold what building the back ends
    logged; the Spectroscopy of a gas set and level count serves all its cases."""
    records, built = {}, {}
    for case in cases():
        key = (case.gas_set, case.levels)
        if key not in built:
            built[key] = spectroscopy(case.gas_set, case.levels, directory,
                                      shape=(2, 2) if case.call == "path" else None)
            records["uploads of {}, {} levels".format(*key)] = {"log": built[key][1].log}
        spec, engine = built[key]
        records[case_id(case)] = run_case(case, spec, engine)
    return records


def run_case(case, spec, engine):
    settings = dict(DEFAULTS, **dict(case.settings))
    for name, value in settings.items():
        setattr(spec, name, value)
    engine.begin(deferred_answer=case.deferred_answer, fail_at=case.fail_at)
    record = {}
    with installed(engine):
        try:
            if case.call == "path":
                # Two runs of one path each.
                spec.device_output_limit = 2*164*8
                values = spec.compute_path(np.full((2, 2), 100.), remove_pedestal=True)
            elif case.call == "no levels":
                values = spec._compute_levels(1, 1, case.mode, case.remove_pedestal, "reference")
            else:
                values = spec.compute_absorption(
                    output_format=case.mode, remove_pedestal=case.remove_pedestal,
                    range_policy="skip" if case.call == "range_policy skip" else "reference")
            record["result"] = _result(engine, values)
        except (Exception, KeyboardInterrupt) as error:
            record["error"] = [type(error).__name__, str(error)]
    record["log"] = engine.log
    return record
