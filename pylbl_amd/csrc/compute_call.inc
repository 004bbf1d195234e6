// compute(): one batched lines call -- what replaces the body of the reference's
// absorption() row loop (absorption.c:76-86) for every level of the call: lane choice and
// ordering against other calls, level scalars, prologue, pedestal pre-pass, far-field series,
// accumulate launches piece by piece, the part that finishes (pedestal applied, copies).
// The stages that stand on their own are in compute_stages.inc.
// Included by engine.hip after compute_stages.inc.
namespace {

// wait_for: where a blocking call (no LBL_ASYNC) leaves an event behind its last operation instead
// of waiting for it -- the caller waits after it has released the engine's mutex, so that other
// threads queue their calls meanwhile.  nullptr: wait here.
int compute(lbl_engine * engine, const ComputeRequest & rq, hipEvent_t * wait_for = nullptr)
{
    CallShape shape;
    const int checked = shape_of(engine, rq, shape);
    if (checked != LBL_OK) return checked;
    Molecule * m = shape.m;
    const GridSpec & g = shape.g;
    const RangeRule & rule = shape.rule;
    const Tiling & tiling = shape.tiling;
    const long long n_long = shape.n_long, stride = shape.stride;
    const int farfield = shape.farfield, points = shape.points;
    const int n_tiles = tiling.n_tiles;
    const int n_cells = rq.vn - rq.v0;
    const long long n_lines = m->n_lines;

    try
    {
        HIP_TRY(hipSetDevice(engine->device));
        const CallTraits traits = traits_of(engine, rq, shape);
        const bool out_device = traits.out_device, want_k = traits.want_k;
        const bool small = traits.small, alternate = traits.alternate;
        const bool add_into_block = traits.add_into_block;
        if ((rq.flags & LBL_DEFER_FINISH) ||
            (!alternate && engine->deferred == &engine->lanes[0]))
        {
            // There is one deferral at a time; and a call about to reuse lane 0's buffers must not
            // find a kept-back call still needing them.  (Kept-back calls stay off lane 0, below,
            // so a plain call -- another thread's, say -- leaves a deferral alone: the order in
            // which a pipeline's calls add into their block does not depend on who else uses the
            // engine.  The kept-back kernels order themselves behind every write of their block
            // when they are queued, run_finish.)
            engine->finish_deferred();
        }
        const int lane_index = alternate ? next_lane_for(engine, rq, shape, traits) : 0;
        Lane & lane = engine->lanes[lane_index];
        hipStream_t stream = lane.main;
        const long long out_bytes = ((long long)(rq.n_levels - 1)*stride + n_long)*8;
        if (!alternate)
        {
            if ((rq.flags & LBL_ASYNC) && out_device)
            {
                engine->join_lanes(stream);     // the host keeps queueing
            }
            else
            {
                for (int i = 1; i < kAllLanes; ++i) engine->lanes[i].drain();
            }
        }
        else
        {
            lane.used = true;
            if (out_device && !add_into_block)
            {
                // Calls on different lanes run side by side; two that write the same memory must
                // not: the later one waits for the earlier one's last kernel.  (A call that adds
                // into the block waits later, in front of the one kernel that does the adding.)
                engine->order_after_writers(stream, rq.k, out_bytes, &lane);
            }
        }

        const bool streamed = rq.host != nullptr && out_device && want_k;
        const int pieces = streamed ? std::max(1, std::min<int>(rq.pieces, std::min(n_tiles, 8)))
                                    : 1;
        Molecule::Plan & plan = plan_for(engine, farfield, *m, g, tiling, points, stream, pieces);

        // Levels per pass, bounded by the workspace budget.
        const long long per_level = plan.partial_slots*64*points*8 + n_lines*(long long)(sizeof(LineWing) + sizeof(LineCore)) +
                                    (long long)n_tiles*sizeof(TileSchedule) +
                                    (out_device ? 0 : n_long*8) +
                                    (rq.remove_pedestal ? pedestal_bytes_per_level(n_lines, n_cells, rq.cut_off) : 0);
        long long chunk = std::max(1ll, engine->workspace_bytes/std::max(per_level, 1ll));
        chunk = std::min<long long>(chunk, rq.n_levels);
        if (chunk > 65535) chunk = 65535;

        const bool with_pedestal = rq.remove_pedestal && n_lines > 0 && want_k;
        const bool add_into = add_into_block;
        reserve_for_call(lane, rq, shape, traits, plan, chunk, stream);

        HostPrep host_prep_data;
        bool deferred_finish = false;

        for (long long base = 0; base < rq.n_levels; base += chunk)
        {
            const int count = (int)std::min<long long>(chunk, rq.n_levels - base);
            // The previous pass may still be reading the pinned block.
            if (base > 0) HIP_TRY(hipStreamSynchronize(stream));
            for (int l = 0; l < count; ++l)
            {
                std::string why;
                LevelScalars & lv = lane.pinned_levels[l];
                if (!fill_level(*m, rq.temperature[base + l], rq.pressure[base + l],
                                rq.vmr[base + l], lv, why))
                {
                    return fail(engine, LBL_OUT_OF_RANGE,
                                "level " + std::to_string(base + l) + ": " + why);
                }
                bound_inner_regions(*m, rule, lv);
            }
            // A few levels travel as kernel arguments of the prologue kernel (no copy in front
            // of it); more go through the pinned block.
            const bool host_prep = engine->prep == LBL_PREP_HOST;
            const bool inline_levels = !host_prep && count <= kInlineLevels;
            InlineLevels packed;
            int prepare_blocks = 0;
            unsigned prologue_blocks = 1;
            if (!inline_levels)
            {
                HIP_TRY(hipMemcpyAsync(lane.levels.data, lane.pinned_levels,
                                       count*sizeof(LevelScalars), hipMemcpyHostToDevice, stream));
                HIP_TRY(hipEventRecord(lane.levels_copied, stream));
                lane.levels_in_flight = true;
            }

            // K1: per-line scalars (+ the tile cut points, in the same launch).
            if (host_prep)
            {
                prepare_on_host(engine, lane, rq, shape, count, stream, host_prep_data);
            }
            else
            {
                if (inline_levels)
                {
                    std::memcpy(packed.level, lane.pinned_levels, count*sizeof(LevelScalars));
                }
                prepare_blocks = (int)((n_lines + 255)/256);
                const int schedule_blocks = want_k ? (int)((8ll*n_tiles + 255)/256) : 0;
                prologue_blocks = (unsigned)std::max(prepare_blocks + schedule_blocks, 1);
                // (every bound starts at kWingBoundsFill: byte 0x7f)
                HIP_TRY(hipMemsetAsync(lane.wing_bounds.data, 0x7f,
                                       (size_t)count*kWingBounds*sizeof(int), stream));
                engine->timed(kTimePrepare, stream, [&] {
                    dim3 grid((unsigned)std::max(prepare_blocks + schedule_blocks, 1),
                              (unsigned)count);
                    hipLaunchKernelGGL(prologue_kernel, grid, dim3(256), 0, stream, m->view(),
                                       lane.levels.data, packed, inline_levels ? 1 : 0, g, rule,
                                       tiling, farfield, prepare_blocks, lane.wing.data,
                                       lane.core.data, lane.schedule.data,
                                       rq.derived != nullptr ? lane.derived.data : nullptr,
                                       rq.evals != nullptr ? lane.evals.data : nullptr,
                                       lane.wing_bounds.data);
                    HIP_TRY(hipGetLastError());
                });
            }

            if (!want_k) continue;

            // The pedestal pre-pass only needs the per-line scalars: it runs on the side
            // stream next to the accumulate kernel (its serial chain keeps one CU busy).
            // Its run-finding kernels go first: once the accumulate grid owns the chip their
            // wide workgroups would wait for it to drain.
            hipStream_t ped_stream = engine->overlap_pedestal ? lane.side : stream;
            if (with_pedestal)
            {
                if (engine->overlap_pedestal)
                {
                    HIP_TRY(hipEventRecord(lane.prepared, stream));
                    HIP_TRY(hipStreamWaitEvent(lane.side, lane.prepared, 0));
                }
                engine->timed(kTimePedestal, ped_stream, [&] {
                    pedestal_find_runs(lane.pedestal, ped_stream, m->view(), lane.wing.data, g,
                                       count, n_cells, engine->scan_chain != 0,
                                       engine->poison_workspace != 0);
                }, 0);
                if (engine->overlap_pedestal)
                {
                    HIP_TRY(hipEventRecord(lane.runs_found, lane.side));
                }
            }

            // Where the spectra of this pass end up, and where the accumulate kernel writes.
            double * target = out_device ? rq.k + base*stride : lane.staging.data;
            const long long target_stride = out_device ? stride : n_long;
            double * sums = target;
            long long sums_stride = target_stride;
            if (with_pedestal && out_device && add_into)
            {
                sums = lane.raw.data;
                sums_stride = n_long;
            }

            AccumulateArgs args;
            args.wing = lane.wing.data;
            args.core = lane.core.data;
            args.schedule = lane.schedule.data;
            args.levels = lane.levels.data;
            args.items = plan.items.data;
            args.far_series = farfield ? lane.far_series.data : nullptr;
            args.wing_bounds = lane.wing_bounds.data;
            args.wing_batches = engine->wing_batches;
            args.partial = lane.partial.data;
            args.partial_slots = plan.partial_slots;
            args.level_stride = sums_stride;
            args.k = sums;
            args.n_lines = n_lines;
            args.tiling = tiling;
            args.n_tiles = n_tiles;
            args.n = g.n;
            args.v0 = g.v0;
            args.n_per_v = g.n_per_v;
            args.dv = g.dv;
            args.v0_real = (double)g.v0;
            // With a pedestal the kernel stores plain sums; pedestal_apply_kernel finishes.
            args.scale_density = (!with_pedestal && (rq.flags & LBL_SCALE_DENSITY)) ? 1 : 0;
            args.accumulate = (!with_pedestal && out_device && add_into) ? 1 : 0;
            args.inner_everywhere = inner_points_everywhere(lane.pinned_levels, count, rq, shape);
#ifdef LBL_ABLATE
            args.ablate = engine->ablate;
#endif

            if (with_pedestal && engine->overlap_pedestal)
            {
                HIP_TRY(hipStreamWaitEvent(stream, lane.runs_found, 0));
            }
            if (farfield)
            {
                launch_far_series(engine, lane, shape, count, stream);
            }
            // A piece = a run of tiles: its accumulate launch (+ the sums of its split tiles),
            // then -- once the pedestal chain has been queued -- the kernel that applies the
            // pedestal to its points and, for a streamed call, the copy of its columns, which
            // runs beside the kernels of the next piece.  One piece unless the call is streamed.
            auto point_range = [&](int piece, long long & q0, long long & q1) {
                long long unused = 0;
                q0 = q1 = 0;
                if (plan.tile_begin[piece + 1] > plan.tile_begin[piece])
                {
                    tile_bounds(tiling, plan.tile_begin[piece], g.n_per_v, g.n, q0, unused);
                    tile_bounds(tiling, plan.tile_begin[piece + 1] - 1, g.n_per_v, g.n, unused, q1);
                    q1 += 1;
                }
            };
            // Where a piece is finished: with a pedestal on the stream the chain runs on (the
            // apply kernels follow it there, while the main stream goes on with the accumulate
            // launches of the later pieces), else on the main stream.
            hipStream_t finish_stream = with_pedestal ? ped_stream : stream;
            auto finish_piece = [&](int piece) {        // (without a pedestal: only the copy)
                long long q0, q1;
                point_range(piece, q0, q1);
                if (q1 <= q0) return;
                if (streamed && q0 < rq.columns)
                {
                    const long long c1 = std::min<long long>(q1, rq.columns);
                    HIP_TRY(hipEventRecord(lane.piece_done[piece], stream));
                    HIP_TRY(hipStreamWaitEvent(engine->copy_stream, lane.piece_done[piece], 0));
                    HIP_TRY(hipMemcpy2DAsync(rq.host + base*rq.host_pitch + q0*8,
                                             (size_t)rq.host_pitch, target + q0,
                                             (size_t)target_stride*8, (size_t)(c1 - q0)*8,
                                             (size_t)count, hipMemcpyDeviceToHost,
                                             engine->copy_stream));
                }
            };
            // All accumulate launches back to back, then the pedestal chain (the host waits for the
            // run counts inside), and whatever finishes pieces last.  (Queueing the chain in front of
            // the accumulate launches of a far-field call: +-0, profiles/r05_ab_chain_first.txt.)
            auto queue_chain = [&]() {
                engine->timed(kTimePedestal, ped_stream, [&] {
                    pedestal_finish(lane.pedestal, ped_stream, m->view(), lane.wing.data,
                                    lane.core.data, g, count, n_cells, engine->scan_chain != 0,
                                    engine->relax_launches, engine->poison_workspace != 0);
                });
            };
            // (Chaining the accumulate launches of successive calls by events -- one grid after the
            // other, only the light kernels of the next call beside it -- was measured in round 5:
            // -2.5 % with the pedestal, +11 % without it, where the overlap of one grid's tail with
            // the next grid's head is what the two lanes are for: profiles/r05_ab_farped.txt.)
            for (int piece = 0; piece < pieces; ++piece)
            {
                const int item0 = plan.item_begin[piece], item1 = plan.item_begin[piece + 1];
                const int split0 = plan.split_begin[piece], split1 = plan.split_begin[piece + 1];
                engine->timed(kTimeAccumulate, stream, [&] {
                    if (item1 > item0)
                    {
                        // One workgroup per work item, heaviest items first.
                        AccumulateArgs mine = args;
                        mine.items = plan.items.data + item0;
                        dim3 grid((unsigned)(item1 - item0), (unsigned)count);
                        launch_accumulate(points, grid, stream, mine);
                    }
                    if (split1 > split0)
                    {
                        const int units = (split1 - split0)*points;     // (split tile, 64-point row)
                        hipLaunchKernelGGL(combine_kernel,
                                           dim3((unsigned)((units + 3)/4), (unsigned)count),
                                           dim3(256), 0, stream, args, plan.split.data + split0,
                                           split1 - split0, 64*points);
                        HIP_TRY(hipGetLastError());
                    }
                });
                if (!with_pedestal)
                {
                    finish_piece(piece);
                }
                else if (finish_stream != stream)
                {
                    HIP_TRY(hipEventRecord(lane.piece_summed[piece], stream));
                }
            }
            if (with_pedestal)
            {
                queue_chain();
                Lane::Finish & f = lane.finish;
                f.pieces = pieces;
                f.count = count;
                f.n_cells = n_cells;
                f.n_per_v = g.n_per_v;
                f.cut_off = g.cut_off;
                f.flags = rq.flags;
                // (a run of tiles may be empty -- few tiles, uneven weights -- and must not move
                // its neighbours' bounds: entry i is both the end of run i-1 and the start of run i)
                long long reached = 0;
                for (int piece = 0; piece < pieces; ++piece)
                {
                    long long q0, q1;
                    point_range(piece, q0, q1);
                    if (q1 <= q0)
                    {
                        q0 = q1 = reached;
                    }
                    f.point_begin[piece] = q0;
                    f.point_begin[piece + 1] = q1;
                    reached = q1;
                }
                f.sums = sums;
                f.sums_stride = sums_stride;
                f.target = target;
                f.target_stride = target_stride;
                f.streamed = streamed;
                f.order_writers = alternate && out_device && add_into;
                f.add_into = out_device && add_into;
                f.host = rq.host;
                f.host_pitch = rq.host_pitch;
                f.columns = rq.columns;
                f.base = base;
                // The block's write record: only once, behind the call's last pass.
                const bool last_pass = base + count >= rq.n_levels;
                f.k = (out_device && last_pass) ? rq.k : nullptr;
                f.block = rq.k;
                f.out_bytes = out_bytes;
                f.finish_stream = finish_stream;
                f.pending = true;
                // Kept back for lbl_finish_deferred only if nothing of this call comes after it:
                // one pass, spectra in device memory, the host not waiting.
                deferred_finish = (rq.flags & LBL_DEFER_FINISH) && (rq.flags & LBL_ASYNC) &&
                                  out_device && alternate && chunk >= rq.n_levels &&
                                  rq.evals == nullptr;
                if (deferred_finish)
                {
                    engine->deferred = &lane;
                }
                else
                {
                    engine->run_finish(lane);
                }
            }

            if (!out_device)
            {
                spectra_to_host(lane, rq, shape, base, count, stream);
            }
        }

        if (out_device && want_k && !with_pedestal)
        {
            lane.note_write(rq.k, out_bytes, stream);   // (with a pedestal: run_finish does)
        }
        if (rq.evals != nullptr && !(engine->prep == LBL_PREP_HOST))
        {
            unsigned long long total = 0;
            HIP_TRY(hipMemcpyAsync(&total, lane.evals.data, sizeof(total),
                                   hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            *rq.evals = (int64_t)total;
        }
        if (rq.derived != nullptr)
        {
            derived_to_host(engine, lane, rq, shape, host_prep_data, stream);
        }
        if (!(rq.flags & LBL_ASYNC))
        {
            if (wait_for != nullptr)
            {
                *wait_for = engine->take_event();
                HIP_TRY(hipEventRecord(*wait_for, stream));
            }
            else
            {
                HIP_TRY(hipStreamSynchronize(stream));
            }
        }
    }
    catch (const HipFailure & f)
    {
        return fail(engine, LBL_ERROR, f.message);
    }
    catch (const std::bad_alloc &)
    {
        return fail(engine, LBL_ERROR, "host allocation failed.");
    }
    catch (const std::exception & e)
    {
        return fail(engine, LBL_ERROR, e.what());
    }
    return LBL_OK;
}

// compute() under the engine's mutex; the wait of a blocking call outside it.
int locked_compute(lbl_engine * engine, const ComputeRequest & rq)
{
    hipEvent_t last = nullptr;
    int status;
    {
        EngineLock lock(engine->mutex);
        status = compute(engine, rq, &last);
    }
    if (last != nullptr)
    {
        const hipError_t waited = hipEventSynchronize(last);
        EngineLock lock(engine->mutex);
        engine->event_pool.push_back(last);
        if (waited != hipSuccess && status == LBL_OK)
        {
            status = fail(engine, LBL_ERROR, hipGetErrorString(waited));
        }
    }
    return status;
}

}  // namespace
