"""The multi-GPU product path (pylbl_amd.distributed.ShardedLines.for_engine) on a real GPU:
at world size 1 in this process, and as two ranks that share GPU 0 and exchange over gloo
(an 8-GPU node is not available to the tests; the partition and exchange code is the same
that bench.py --gpus N runs over RCCL)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from pylbl_amd import distributed, synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("output", ["gas", "total"])
def test_for_engine_single_rank_against_oracle(oracle, output):
    from pylbl_amd.engine import Engine
    engine = Engine(0)
    formulas = ("H2O", "CO2")
    tables = {f: synthetic.line_table(f, 600., 700., num_lines=1500, seed=11 + i)
              for i, f in enumerate(formulas)}
    handles = {f: engine.load(tables[f]) for f in formulas}
    atmos = synthetic.fixture_atmosphere()
    v0, vn, npv = 610, 650, 500
    vmr = {f: atmos.vmr[f] for f in formulas}
    for ped in (False, True):
        sharded = distributed.ShardedLines.for_engine(engine, handles, (v0, vn, npv),
                                                      remove_pedestal=ped,
                                                      scale_density=(output == "total"))
        out = sharded.run(atmos.t, atmos.p, vmr, output=output)
        expect = {f: np.asarray([oracle.absorption_port(tables[f], atmos.t[i], atmos.p[i],
                                                        vmr[f][i], v0, vn, npv,
                                                        remove_pedestal=ped)[0]
                                 for i in range(4)]) for f in formulas}
        if output == "total":
            kb = 1.38064852e-23
            total = sum(expect[f]*(atmos.p*vmr[f]/(kb*atmos.t))[:, None] for f in formulas)
            got = out.cpu().numpy()
            assert np.max(np.abs(got - total)/np.max(total, axis=1, keepdims=True)) <= 1e-6
        else:
            for f in formulas:
                got = out[f].cpu().numpy()
                scale = np.max(expect[f], axis=1, keepdims=True)
                assert np.max(np.abs(got - expect[f])/scale) <= 1e-6
    engine.close()


def _run_children(world, script, arguments, settings, patience, says="rank {} ok", tail=3000):
    """Starts `world` fresh interpreters of tests/<script> as the ranks of one rendezvous (RANK,
    WORLD_SIZE, LOCAL_RANK, MASTER_ADDR and a free MASTER_PORT, plus `settings`), gives each
    `patience` seconds -- all are killed when one runs out of them -- and wants exit code 0 and
    the line `says` (with the rank) from every one.  Returns what rank 0 printed."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), LOCAL_RANK=str(rank), **settings)
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(ROOT, "tests", script)] + list(arguments),
            env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    printed = []
    for rank, proc in enumerate(procs):
        try:
            out, err = proc.communicate(timeout=patience)
        except subprocess.TimeoutExpired:
            for other in procs:
                other.kill()
            raise
        assert proc.returncode == 0 and says.format(rank) in out, out + err[-tail:]
        printed.append(out)
    return printed[0]


def _run_ranks(n_levels, output, backend, world=2, order_on_device=False):
    _run_children(world, "dist_gpu_worker.py", [str(n_levels), output],
                  {"DIST_BACKEND": backend,
                   "PYLBL_AMD_ORDER_ON_DEVICE": "1" if order_on_device else "0"}, patience=300)


@pytest.mark.parametrize("ordering", ["host", "device"])
@pytest.mark.parametrize("n_levels,output", [(5, "gas"), (1, "gas"), (1, "total"), (4, "total")])
def test_two_ranks_share_one_gpu(n_levels, output, ordering):
    """Levels >= ranks shards levels; one level shards its three molecules over the two ranks
    (and the total then needs the cross-rank sum).  ordering "device": the kernels and the
    exchange are ordered the way the RCCL path orders them -- torch's stream waits for the
    engine's events (ShardedLines.order, lbl_order_stream_after_engine), the host does not --
    with gloo carrying the blocks: what is left untested for the 8-GPU box is RCCL's transport."""
    _run_ranks(n_levels, output, "gloo", order_on_device=(ordering == "device"))


def test_config3_shape_over_the_ranks_the_card_allows():
    """BASELINE configs[3]'s partition -- the 64-level standard atmosphere, H2O + CO2 + O3, blocks
    of levels per rank -- and configs[2]'s unit mode (one level, three molecules, the cross-rank
    reduce) with FIVE child ranks on GPU 0 (the pool ends a run with more than six processes on
    the card, and the test runner, which has computed on it, is one of them; the 8-way cut itself
    is checked on the CPU, tests/test_distributed_gloo.py, and ranks 0 and 7 of 8 at full size
    in tests/test_gpu_baseline_configs.py): 1-101 cm-1 at 0.001
    cm-1, gloo, kernels and exchange ordered on the device.  Rank 0 compares two levels of every
    rank's block with the oracle (tests/dist_config3_worker.py)."""
    _run_children(5, "dist_config3_worker.py", ["64"], {"PYLBL_AMD_ORDER_ON_DEVICE": "1"},
                  patience=600)


def _visible_gpus():
    """Counted without initialising HIP in the test process (the ranks are child processes)."""
    import torch
    return torch.cuda.device_count()


@pytest.mark.parametrize("n_levels,output", [(9, "gas"), (1, "gas"), (1, "total"), (11, "total")])
def test_every_visible_gpu_over_rccl(n_levels, output):
    """The same checks with one GPU per rank and RCCL carrying the exchange (backend "nccl"), on
    as many GPUs as the box shows (at most 6 here: the pool's limit on processes that use the
    card from one run; the driver's 8-GPU bench covers 8): uneven level blocks, the one-level
    case cut into (level, molecule) units with its cross-rank sum, Spectroscopy(group=True).
    Single-GPU boxes skip it."""
    world = min(_visible_gpus(), 6)
    if world < 2:
        pytest.skip("needs two GPUs")
    _run_ranks(n_levels, output, "nccl", world=world)


def test_exchange_is_ordered_behind_the_kernels_without_a_host_wait(oracle):
    """lbl_order_stream_after_engine / lbl_order_engine_after_stream: a torch stream that reads
    what the engine's lanes are still computing, and engine work that overwrites what a torch
    stream is still reading, see each other's results without the host waiting in between."""
    import torch
    from pylbl_amd.engine import Engine
    engine = Engine(0)
    device = torch.device("cuda", 0)
    table = synthetic.line_table("H2O", 1., 400., num_lines=30000, seed=71, tips_range=(150, 400))
    handle = engine.load(table)
    v0, vn, npv = 1, 361, 500
    n = (vn - v0)*npv
    expect = engine.compute(handle, [250.], [3e4], [5e-3], v0, vn, npv, remove_pedestal=True)

    class Slot(object):
        def __init__(self, tensor):
            self.pointer, self.shape = tensor.data_ptr(), tuple(tensor.shape)
    block = torch.zeros((1, n), dtype=torch.float64, device=device)
    copies = []
    torch.cuda.synchronize(device)
    stream = torch.cuda.current_stream(device)
    for turn in range(6):
        # engine overwrites `block` (after torch has finished reading the previous contents) ...
        engine.order_after_stream(stream.cuda_stream)
        if turn % 2:
            engine.fill_zero(Slot(block), asynchronous=True)
        else:
            engine.compute(handle, [250.], [3e4], [5e-3], v0, vn, npv, remove_pedestal=True,
                           out=Slot(block), asynchronous=True)
        # ... and torch reads it on its own stream, ordered on the device only.
        engine.order_stream_after(stream.cuda_stream)
        copies.append(block.clone())
    torch.cuda.synchronize(device)
    for turn, copy in enumerate(copies):
        got = copy.cpu().numpy()
        assert np.array_equal(got, np.zeros_like(got) if turn % 2 else expect), turn
    engine.close()


def test_rccl_at_world_size_one():
    """RCCL executed once on the GPU a one-GPU box has, in a child process (a process that holds
    a GPU is never re-executed): init_process_group("nccl", world_size=1), ShardedLines through
    its collection step with the rank's blocks sent to itself in one grouped send/recv (strided
    views of the collected array), calls queued back to back without waiting, all_reduce / reduce
    on an engine-written block ordered by lbl_order_stream_after_engine, Pending.wait's device
    branch -- all oracle-checked (tests/rccl_one_rank_worker.py)."""
    legacy = os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0")          # (kept where it is set)
    out = _run_children(1, "rccl_one_rank_worker.py", [], {"HSA_ENABLE_IPC_MODE_LEGACY": legacy},
                        patience=300, says="rccl one rank ok", tail=4000)
    assert "librccl" in out
