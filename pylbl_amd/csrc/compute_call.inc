// compute(): one batched lines call -- what replaces the body of the reference's
// absorption() row loop (absorption.c:76-86) for every level of the call: lane choice and
// ordering against other calls, level scalars, prologue, pedestal pre-pass, far-field series,
// accumulate launches piece by piece, the part that finishes (pedestal applied, copies).
// The stages themselves are in compute_stages.inc.
// Included by engine.hip after compute_stages.inc.
namespace {

// Runs inside an entry()'s frame: the engine's mutex held, failures thrown.
// wait_for: where a blocking call (no LBL_ASYNC) leaves an event behind its last operation instead
// of waiting for it -- the caller waits after it has released the engine's mutex, so that other
// threads queue their calls meanwhile.  nullptr: wait here.
int compute(lbl_engine * engine, const ComputeRequest & rq, Event * wait_for = nullptr)
{
    CallShape shape;
    const int checked = shape_of(engine, rq, shape);
    if (checked != LBL_OK) return checked;
    HIP_TRY(hipSetDevice(engine->device));
    const CallTraits traits = traits_of(engine, rq, shape);
    const long long out_bytes = ((long long)(rq.n_levels - 1)*shape.stride + shape.n_long)*8;
    Lane & lane = take_lane(engine, rq, shape, traits, out_bytes);
    hipStream_t stream = lane.main;
    const bool streamed = rq.host != nullptr && traits.out_device && traits.want_k;
    const int pieces = streamed ? std::max(1, std::min<int>(rq.pieces, std::min(shape.tiling.n_tiles, 8)))
                                : 1;
    const Molecule::Plan & plan = plan_for(engine, shape.farfield, *shape.m, shape.g, shape.tiling,
                                           shape.points, stream, pieces);
    const bool with_pedestal = traits.pedestal_pass && traits.want_k;
    const LinesCall call{engine, rq, shape, traits, lane, stream, plan, streamed, pieces,
                         with_pedestal, out_bytes,
                         levels_per_pass(engine, rq, shape, traits, plan)};
    reserve_for_call(call);

    HostPrep host_prep;
    for (long long base = 0; base < rq.n_levels; base += call.chunk)
    {
        const int count = (int)std::min<long long>(call.chunk, rq.n_levels - base);
        const int staged = stage_levels(call, base, count);
        if (staged != LBL_OK) return staged;
        launch_prologue(call, count, host_prep);
        if (!traits.want_k) continue;

        const Lane::Pass pass = pass_of(call, base, count);
        if (with_pedestal) start_pedestal_search(call, pass);
        const AccumulateArgs args = accumulate_args(call, pass);
        if (with_pedestal && engine->overlap_pedestal)
        {
            HIP_TRY(hipStreamWaitEvent(stream, lane.runs_found, 0));
        }
        if (shape.farfield) launch_far_series(engine, lane, shape, count, stream);
        describe_finish(call, pass);
        // A piece = a run of tiles: its accumulate launch (+ the sums of its split tiles), then --
        // once the pedestal chain has been queued -- the kernel that applies the pedestal to its
        // points and, for a streamed call, the copy of its columns, which runs beside the kernels
        // of the next piece.  One piece unless the call is streamed.  All accumulate launches go
        // back to back; without a pedestal only the copy finishes a piece, right behind its launch.
        // (Chaining the accumulate launches of successive calls by events -- one grid after the
        // other, only the light kernels of the next call beside it -- was measured in round 5:
        // -2.5 % with the pedestal, +11 % without it, where the overlap of one grid's tail with
        // the next grid's head is what the two lanes are for: profiles/r05_ab_farped.txt.)
        for (int piece = 0; piece < pieces; ++piece)
        {
            launch_piece(call, pass, args, piece);
            if (!with_pedestal)
            {
                engine->copy_piece_home(lane, piece, stream);
            }
            else if (pass.finish_stream != stream)
            {
                lane.piece_summed[piece].record(stream);
            }
        }
        if (with_pedestal) finish_with_pedestal(call, pass);
        if (!traits.out_device) spectra_to_host(lane, rq, shape, base, count, stream);
    }
    return end_call(call, host_prep, wait_for);
}

// lbl_compute: compute() in entry()'s frame, but the wait of a blocking call outside the lock --
// the one thing entry() alone would not give.
int locked_compute(lbl_engine * engine, const ComputeRequest & rq)
{
    Event last;
    int status = entry(engine, [&] { return compute(engine, rq, &last); });
    if (last != nullptr)
    {
        const hipError_t waited = hipEventSynchronize(last);
        EngineLock lock(engine->mutex);
        engine->event_pool.push_back(std::move(last));
        if (waited != hipSuccess && status == LBL_OK)
        {
            status = fail(engine, LBL_ERROR, hipGetErrorString(waited));
        }
    }
    return status;
}

}  // namespace
