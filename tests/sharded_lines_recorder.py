"""What tests/test_sharded_lines_log_host.py and tests/golden/make_sharded_lines_log.py share: real
gloo ranks on the CPU that run pylbl_amd.distributed.ShardedLines.run on a stand-in `compute`
and write down, per rank and in order, what the host path does -- and the grid of cases.

A log is a list of strings.  Per run() call: "run(async_op=...)", then every compute call (formula,
number of levels, shape of `out`, "block" if `out` is the whole kept block or "rows[lo:hi]" of it,
accumulate), every _zero, every flush, every P2POp handed to batch_isend_irecv (isend or irecv, the
peer's global rank, the tensor's shape and, for a receive, its offset in the collected array in
elements), every reduce / all_reduce (destination as a global rank, shape), then the finished
Pending's peers and byte counts and the shape of what run() returned (with whether its values are
those the stand-in computes: formula index + 1000 x level temperature, summed over the gases for
"total").  One set of spawned ranks per world size runs all of that world's cases."""
from collections import namedtuple
import os
import socket

import numpy as np

THREE = ("H2O", "CO2", "O3")
EIGHT = ("H2O", "CO2", "O3", "N2O", "CO", "CH4", "O2", "N2")
WEIGHTS = {THREE: (3., 2., 1.),
           EIGHT: (110_000., 400_000., 400_000., 160_000., 6_000., 300_000., 15_000., 1_000.)}
POINTS = 16

# members: global ranks of the sub-group that does the work (None: every rank); `dst` is a rank
# within that group.
Case = namedtuple("Case", "world members levels output dst molecules")


def cases():
    out = [Case(world, None, levels, output, dst, THREE)
           for world in (2, 3) for levels in (1, 2, 3, 5) for output in ("gas", "total")
           for dst in (0, 1, None)]
    out += [Case(3, (1, 2), levels, output, dst, THREE)
            for levels in (1, 3) for output in ("gas", "total") for dst in (0, 1, None)]
    out.append(Case(8, None, 1, "total", None, EIGHT))
    return out


def case_id(case):
    group = "" if case.members is None else " as group {}".format(list(case.members))
    return "world {}{}, {} levels x {} molecules, {}, dst {}".format(
        case.world, group, case.levels, len(case.molecules), case.output, case.dst)


def _shape(tensor):
    return "x".join(str(s) for s in tensor.shape)


class _Log(object):
    """The list the patched calls append to; None between cases."""
    entries = None

    def add(self, text):
        if self.entries is not None:
            self.entries.append(text)


def _patch_exchange(dist, log):
    """batch_isend_irecv, reduce and all_reduce write themselves down, then run."""
    real = {name: getattr(dist, name) for name in ("batch_isend_irecv", "reduce", "all_reduce")}

    def batch_isend_irecv(ops):
        for op in ops:
            if op.op is dist.isend:
                log.add("isend(peer={}, shape={})".format(op.peer, _shape(op.tensor)))
            else:
                assert op.op is dist.irecv
                log.add("irecv(peer={}, shape={}, offset={})".format(
                    op.peer, _shape(op.tensor), op.tensor.storage_offset()))
        return real["batch_isend_irecv"](ops)

    def reduce(tensor, dst, **keywords):
        log.add("reduce(dst={}, shape={})".format(dst, _shape(tensor)))
        return real["reduce"](tensor, dst=dst, **keywords)

    def all_reduce(tensor, **keywords):
        log.add("all_reduce(shape={})".format(_shape(tensor)))
        return real["all_reduce"](tensor, **keywords)
    dist.batch_isend_irecv, dist.reduce, dist.all_reduce = batch_isend_irecv, reduce, all_reduce


def _run_case(case, group, rank_in_group, log):
    import torch
    from pylbl_amd import distributed
    molecules = case.molecules

    def compute(formula, temperature, pressure, x, out, accumulate):
        whole = out.untyped_storage().nbytes()//8 == out.numel()
        lo = out.storage_offset()//POINTS
        log.add("compute({}, levels={}, out={} {}, accumulate={})".format(
            formula, len(temperature), _shape(out),
            "block" if whole else "rows[{}:{}]".format(lo, lo + out.shape[0]), accumulate))
        rows = torch.from_numpy(np.asarray(temperature)*1000. + molecules.index(formula))
        if accumulate:
            out += rows[:, None]
        else:
            out.copy_(rows[:, None].expand_as(out))

    sharded = distributed.ShardedLines(compute, molecules, POINTS, weights=WEIGHTS[molecules],
                                       group=group, flush=lambda: log.add("flush()"))
    zero = sharded._zero

    def recorded_zero(tensor):
        log.add("_zero({})".format(_shape(tensor)))
        zero(tensor)
    sharded._zero = recorded_zero
    receives = case.dst is None or rank_in_group == case.dst
    for call, async_op in enumerate((False, True)):
        t = 200. + 10.*call + np.arange(case.levels, dtype=np.float64)
        log.add("run(async_op={})".format(async_op))
        out = sharded.run(t, t*100., {f: t*1e-6 for f in molecules}, dst=case.dst,
                          output=case.output, async_op=async_op)
        if async_op:
            out = out.wait()
        done = sharded.last_exchange
        log.add("pending(peers={}, bytes_sent={}, bytes_received={})".format(
            list(done.peers), done.bytes_sent, done.bytes_received))
        expect = {f: np.repeat((t*1000. + m)[:, None], POINTS, axis=1)
                  for m, f in enumerate(molecules)}
        if case.output == "total":
            correct = receives and bool(np.array_equal(out.numpy(), sum(expect.values())))
            log.add("result({}, correct={})".format(None if out is None else _shape(out), correct))
        else:
            correct = receives and all(np.array_equal(out[f].numpy(), expect[f]) for f in molecules)
            log.add("result({}, correct={})".format(
                {f: None if out[f] is None else _shape(out[f]) for f in molecules}, correct))


def _worker(rank, world, port, todo, queue):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    groups = {None: None}
    for members in sorted({case.members for case in todo if case.members is not None}):
        groups[members] = dist.new_group(list(members))
    log = _Log()
    _patch_exchange(dist, log)
    logs = {}
    for case in todo:
        if case.members is None or rank in case.members:
            log.entries = logs[case_id(case)] = []
            group = groups[case.members]
            _run_case(case, group, dist.get_rank(group), log)
            log.entries = None
        dist.barrier()
    queue.put((rank, logs))
    dist.barrier()
    dist.destroy_process_group()


def run_cases(todo=None):
    """{case id: {"rank r": log}} (global ranks; a rank outside the case's group has none)."""
    import torch.multiprocessing as mp
    todo = cases() if todo is None else list(todo)
    records = {case_id(case): {} for case in todo}
    context = mp.get_context("spawn")
    for world in sorted({case.world for case in todo}):
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        queue = context.Queue()
        mine = [case for case in todo if case.world == world]
        procs = [context.Process(target=_worker, args=(rank, world, port, mine, queue))
                 for rank in range(world)]
        for p in procs:
            p.start()
        results = sorted(queue.get(timeout=240) for _ in procs)
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
        for rank, logs in results:
            for name, log in logs.items():
                records[name]["rank {}".format(rank)] = log
    return records
