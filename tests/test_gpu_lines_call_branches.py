"""Branches of the batched lines call that no other test reaches, each compared bit for bit with a
path the rest of the suite covers: host output that is added to, the pedestal pre-pass on the
main stream (option overlap_pedestal = 0), and a level that fails in a later pass.

Where the other branches of compute() (csrc/compute_call.inc) are reached:
  several passes (small workspace_bytes)    test_gpu_api: test_level_chunking_and_strides,
                                            test_gases_added_into_one_block_in_several_passes
  pieces > 1, with and without pedestal     test_gpu_api:
                                            test_streamed_call_delivers_what_the_plain_call_computes;
                                            test_gpu_fuzz_delivery, test_gpu_fuzz_pipeline
  an empty piece                            test_gpu_api: test_streamed_call_with_empty_runs_of_tiles
  host output, dense and padded rows        test_gpu_api: test_level_chunking_and_strides;
                                            test_gpu_parity
  host output with LBL_ACCUMULATE           here
  add into a block with pedestal (lane.raw) test_gpu_api:
                                            test_gases_added_into_one_block_in_several_passes,
                                            test_deferred_finish_queued_first_adds_last
  evals                                     test_gpu_parity: test_eval_count_matches_oracle;
                                            test_gpu_baseline_configs
  derived, prep on the device and the host  test_gpu_parity: test_line_scalars_match_oracle;
                                            test_gpu_line_scalars (slots, window edges, row order)
  inline / copied levels (kInlineLevels 4)  test_gpu_fuzz_delivery (1-5 levels); test_gpu_api:
                                            test_level_chunking_and_strides (7 levels, then fewer
                                            per pass)
  the schedule's bracketed table searches   test_gpu_schedule_search (every cell scale, no cell
                                            table, keys off either end of it, empty cells; both
                                            prologues, inline and copied levels)
  more than 65 535 levels                   test_gpu_many_levels (65 535, 65 536, 65 547 and 131 073
                                            levels: gridDim.y == 65535, passes at base 65535 and
                                            131070, every output route; the passes counted)
  grids past 2^28 points                    test_gpu_many_levels: test_largest_grid (1 073 709 056
                                            points, lines on the indices 0, 2^28, 2^29, 3 2^28 and
                                            n - 1) and the refusal of 2^30
  blocking calls of several threads         test_gpu_threads
  overlap_pedestal = 0                      here
  fill_level failing in a later pass        here (in the first pass: test_gpu_api:
                                            test_error_paths)"""
import numpy as np
import pytest

from pylbl_amd import synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup():
    from pylbl_amd.engine import Engine
    e = Engine(0)
    table = synthetic.line_table("CH4", 1200., 1400., num_lines=20000, seed=81,
                                 tips_range=(150, 400))
    yield e, e.load(table), synthetic.standard_atmosphere(7)
    e.close()


@pytest.mark.parametrize("remove_pedestal", [False, True])
def test_host_output_that_is_added_to(setup, remove_pedestal):
    """LBL_ACCUMULATE without LBL_OUT_DEVICE: the spectra of a pass are added to the caller's host
    rows by the host -- in one pass and in several, the rows end up as what was there plus what
    the plain call returns."""
    e, h, atmos = setup
    v0, vn, npv = 1250, 1330, 200
    x = atmos.vmr["CH4"]
    plain = e.compute(h, atmos.t, atmos.p, x, v0, vn, npv, remove_pedestal=remove_pedestal,
                      scale_density=True).copy()
    before = np.random.default_rng(5).uniform(0., float(plain.max()), plain.shape)
    try:
        for budget in (4 << 30, 1 << 20):
            e.set_option("workspace_bytes", budget)
            out = before.copy()
            e.compute(h, atmos.t, atmos.p, x, v0, vn, npv, remove_pedestal=remove_pedestal,
                      scale_density=True, accumulate=True, out=out)
            assert np.array_equal(out, before + plain), budget
    finally:
        e.set_option("workspace_bytes", 4 << 30)


@pytest.mark.parametrize("farfield", [False, True])
def test_pedestal_pre_pass_on_the_main_stream(setup, farfield):
    """overlap_pedestal = 0 queues the pre-pass, the chain and the apply kernels on the lane's main
    stream instead of its side stream: the same kernels in another place, so the same bits --
    to host memory, into a device block in several passes, added into a block, and delivered
    piece by piece."""
    from pylbl_amd.engine import DeviceSpectra
    e, h, atmos = setup
    v0, vn, npv = 1250, 1330, 200
    n = (vn - v0)*npv
    x = atmos.vmr["CH4"]
    expect = e.compute(h, atmos.t, atmos.p, x, v0, vn, npv, remove_pedestal=True,
                       scale_density=True, farfield=farfield).copy()
    e.set_option("overlap_pedestal", 0)
    try:
        got = e.compute(h, atmos.t, atmos.p, x, v0, vn, npv, remove_pedestal=True,
                        scale_density=True, farfield=farfield)
        assert np.array_equal(got, expect)
        out = DeviceSpectra(e, 7, n)
        target = e.host_array((7, n - 5))
        e.set_option("workspace_bytes", 1 << 20)
        e.compute(h, atmos.t, atmos.p, x, v0, vn, npv, remove_pedestal=True, scale_density=True,
                  farfield=farfield, out=out)
        e.set_option("workspace_bytes", 4 << 30)
        assert np.array_equal(out.to_host(), expect)
        e.fill_zero(out, asynchronous=True)
        target[...] = -1.
        e.compute(h, atmos.t, atmos.p, x, v0, vn, npv, remove_pedestal=True, scale_density=True,
                  farfield=farfield, out=out, accumulate=True, asynchronous=True, deliver=target,
                  pieces=4)
        e.synchronize()
        assert np.array_equal(out.to_host(), expect)        # (0 + k == k)
        assert np.array_equal(target, expect[:, :n - 5])
        out.free()
    finally:
        e.set_option("overlap_pedestal", 1)
        e.set_option("workspace_bytes", 4 << 30)


def test_level_that_fails_in_a_later_pass(setup):
    """A temperature outside the partition-function table at the last of seven levels, with a
    workspace budget of a level or so per pass: the call fails from inside a later pass, names the
    level by its index in the whole call, and leaves the engine usable."""
    from pylbl_amd.errors import EngineError
    e, h, atmos = setup
    v0, vn, npv = 1250, 1330, 200
    x = atmos.vmr["CH4"]
    whole = e.compute(h, atmos.t, atmos.p, x, v0, vn, npv).copy()
    t = np.array(atmos.t, dtype=np.float64)
    t[6] = 100.
    e.set_option("workspace_bytes", 1 << 20)
    try:
        with pytest.raises(EngineError, match=r"level 6: temperature 100\.0+ K \(or 296 K\) lies "
                                              r"outside the partition-function table\."):
            e.compute(h, t, atmos.p, x, v0, vn, npv)
        assert np.array_equal(e.compute(h, atmos.t, atmos.p, x, v0, vn, npv), whole)
    finally:
        e.set_option("workspace_bytes", 4 << 30)
