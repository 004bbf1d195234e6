// The handle tables (find_slot, store_slot, free_slot: every load and free entry), and what the
// slot entries share (lbl_continuum_compute and lbl_continuum_compute_many in
// continuum_entry.inc, lbl_xsec_compute in xsec_entry.inc): the grid and stride checks, the lane a
// call runs on and its ordering, and the chunked run over the levels with its copy back to a host
// output.  Included by engine.hip before its entries.
namespace {

template <typename T>
T * find_slot(std::vector<std::unique_ptr<T>> & slots, int32_t handle)
{
    if (handle < 0 || (size_t)handle >= slots.size()) return nullptr;
    return slots[handle].get();
}

template <typename T>
int32_t store_slot(std::vector<std::unique_ptr<T>> & slots, std::unique_ptr<T> value)
{
    size_t slot = slots.size();
    for (size_t i = 0; i < slots.size(); ++i)
    {
        if (!slots[i]) { slot = i; break; }
    }
    if (slot == slots.size()) slots.emplace_back();
    slots[slot] = std::move(value);
    return (int32_t)slot;
}

// A free entry: drops what `handle` stands for in `table` once everything queued has run (a
// kernel on any lane may still read it).  `unknown`: the message for a handle that is not in
// use; `before`: what else goes with the object, dropped first.
template <typename T>
int free_slot(lbl_engine * engine, std::vector<std::unique_ptr<T>> lbl_engine::* table,
              int32_t handle, const char * unknown, const std::function<void()> & before = {})
{
    return entry(engine, [&] {
        auto & slots = engine->*table;
        if (find_slot(slots, handle) == nullptr) return fail(engine, LBL_BAD_ARGUMENT, unknown);
        (void)hipSetDevice(engine->device);
        engine->drain_lanes();
        if (before) before();
        slots[handle].reset();
        return LBL_OK;
    });
}

// One slot call: n_levels rows of the grid's n points, `stride` apart, written or (LBL_ACCUMULATE)
// added into `out`, a device block (LBL_OUT_DEVICE) or host memory.
struct SlotCall
{
    lbl_engine * engine;
    int32_t n_levels, flags;
    double * out;
    const SpectralGrid * g = nullptr;
    long long n = 0, stride = 0;
    bool out_device = false, add_into = false;
    Lane * lane = nullptr;
    hipStream_t stream = nullptr;

    // The grid, then the entry's own argument check (`bad`: fails with `what`), then the stride.
    int check(int32_t grid, int64_t level_stride, bool bad, const char * what)
    {
        g = find_slot(engine->grids, grid);
        if (g == nullptr) return fail(engine, LBL_BAD_ARGUMENT, "unknown grid handle.");
        if (bad) return fail(engine, LBL_BAD_ARGUMENT, what);
        n = g->n;
        stride = level_stride > 0 ? level_stride : n;
        if (stride < n) return fail(engine, LBL_BAD_ARGUMENT, "level_stride < grid points.");
        out_device = (flags & LBL_OUT_DEVICE) != 0;
        add_into = (flags & LBL_ACCUMULATE) != 0;
        return LBL_OK;
    }

    long long out_bytes() const { return ((long long)(n_levels - 1)*stride + n)*8; }

    // Queued device-to-device calls run on the slot lane's urgent stream, behind whatever the
    // other lanes have queued for this block; everything else on lane 0 with the other lanes
    // drained (a call that adds into its output lets them finish first, as lbl_compute does).
    void open()
    {
        HIP_TRY(hipSetDevice(engine->device));
        const bool queued = out_device && (flags & LBL_ASYNC);
        lane = &engine->lanes[queued ? kSlotLane : 0];
        stream = lane->main;
        if (queued)
        {
            lane->used = true;
            engine->order_after_writers(stream, out, out_bytes(), lane);
        }
        else
        {
            for (int i = 1; i < kAllLanes; ++i) engine->lanes[i].drain();
        }
    }

    int close()
    {
        if (out_device) lane->note_write(out, out_bytes(), stream);
        if (!(flags & LBL_ASYNC)) HIP_TRY(hipStreamSynchronize(stream));
        return LBL_OK;
    }

    // The levels of a one-slot call, up to 65535 at a time (for a host output, as many as
    // workspace_bytes holds): stage(level) gives a level's scalars, model(count) fills `values`
    // and feed.slopes ([count][points]), interp(count, target, target_stride, add) launches the
    // interpolation onto the grid, timed as `interp_span`.  A host output is copied back chunk
    // by chunk, or added into row by row.
    template <typename Feed, typename Stage, typename Model, typename Interp>
    int run(Feed & feed, DeviceBuffer<double> & values, long long points, int interp_span,
            Stage stage, Model model, Interp interp)
    {
        open();
        long long chunk = std::min<long long>(n_levels, 65535);
        if (!out_device) chunk = std::max(1ll, std::min(chunk, engine->workspace_bytes/(n*8)));
        // (waits first: the previous call's copy may still read the pinned level block)
        auto * staged = feed.pinned.refill((size_t)chunk);
        feed.levels.reserve((size_t)chunk);
        values.reserve((size_t)(chunk*points));
        feed.slopes.reserve((size_t)(chunk*points));
        if (!out_device) feed.staging.reserve((size_t)(chunk*n));
        for (long long base = 0; base < n_levels; base += chunk)
        {
            const int count = (int)std::min<long long>(chunk, n_levels - base);
            for (int l = 0; l < count; ++l) staged[l] = stage(base + l);
            feed.pinned.upload(feed.levels.data, (size_t)count, stream);
            model(count);
            double * target = out_device ? out + base*stride : feed.staging.data;
            const long long target_stride = out_device ? stride : n;
            engine->timed(interp_span, stream, [&] {
                interp(count, target, target_stride, (out_device && add_into) ? 1 : 0);
                HIP_TRY(hipGetLastError());
            });
            feed.mark(stream);
            if (out_device)
            {
                if (base + count < n_levels) feed.pinned.wait();
                continue;
            }
            std::vector<double> row;
            for (int l = 0; l < count; ++l)
            {
                double * dst = out + (base + l)*stride;
                const double * src = feed.staging.data + (size_t)l*n;
                if (add_into)
                {
                    row.resize((size_t)n);
                    HIP_TRY(hipMemcpyAsync(row.data(), src, (size_t)n*8, hipMemcpyDeviceToHost,
                                           stream));
                    HIP_TRY(hipStreamSynchronize(stream));
                    for (long long i = 0; i < n; ++i) dst[i] += row[i];
                }
                else
                {
                    HIP_TRY(hipMemcpyAsync(dst, src, (size_t)n*8, hipMemcpyDeviceToHost, stream));
                }
            }
            HIP_TRY(hipStreamSynchronize(stream));
        }
        return close();
    }
};

}  // namespace
