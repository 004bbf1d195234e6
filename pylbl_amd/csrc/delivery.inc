// Getting results out and sharing HBM blocks with other users of the device: the probe that
// finds the lanes whose copies would queue behind their own kernels, stream hand-overs
// (lbl_order_*), device and page-locked host memory, zero fill and the copies to the host.
// Included by engine.hip after compute_call.inc.
namespace {

// Spins for about `ticks` of the constant-rate clock (100 MHz): something that keeps a queue busy.
__global__ void spin_kernel(long long ticks, int * sink)
{
    const long long begin = wall_clock64();
    int turns = 0;
    while (wall_clock64() - begin < ticks && turns < (1 << 26)) turns += 1;
    if (sink != nullptr && turns < 0) *sink = turns;
}

__global__ void touch_kernel() {}

// Which lanes' main streams share a hardware queue with the copy stream (lbl_engine::
// delivers_badly): the lane's main stream is kept busy for ~40 us, an empty kernel goes to the copy
// stream, and if that only gets through when the lane is done, the two are one queue.
void calibrate_delivery_lanes(lbl_engine * e)
{
    Event lane_done(true), through(true);
    lane_done.create();
    through.create();
    // The runtime creates a stream's hardware queue at its first submission: every stream gets
    // an empty kernel first, so that no probe below times a queue being set up.
    hipLaunchKernelGGL(touch_kernel, dim3(1), dim3(64), 0, e->copy_stream);
    for (int l = 0; l < kLanes; ++l)
    {
        hipLaunchKernelGGL(touch_kernel, dim3(1), dim3(64), 0, e->lanes[l].main);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    const long long ticks = 4000;       // 40 us at 100 MHz
    const int probes = 3;               // the verdict of the majority: one late probe (a busy
                                        // GPU, a descheduled host thread) does not flip a lane
    for (int l = 0; l < kLanes; ++l)
    {
        int shared = 0;
        for (int probe = 0; probe < probes; ++probe)
        {
            hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, e->lanes[l].main, ticks,
                               (int *)nullptr);
            lane_done.record(e->lanes[l].main);
            hipLaunchKernelGGL(touch_kernel, dim3(1), dim3(64), 0, e->copy_stream);
            through.record(e->copy_stream);
            HIP_TRY(hipGetLastError());
            lane_done.synchronize();
            through.synchronize();
            float ahead = 0.f;
            HIP_TRY(hipEventElapsedTime(&ahead, through, lane_done));
            if (!(ahead > 0.01f)) shared += 1;
        }
        e->delivers_badly[l] = 2*shared > probes;
    }
}

}  // namespace

extern "C" {

void * lbl_stream(lbl_engine * engine)
{
    if (engine == nullptr) return nullptr;
    EngineLock lock(engine->mutex);
    return (void *)engine->stream;
}

// The two halves of sharing HBM blocks with another HIP user of the device (e.g. the library
// that runs the RCCL exchange of pylbl_amd/distributed.py) without stopping the host: each is a
// handful of event records and stream waits.
int lbl_order_stream_after_engine(lbl_engine * engine, void * stream)
{
    return entry(engine, [&] {
        HIP_TRY(hipSetDevice(engine->device));
        // "Everything queued so far" includes what a call kept back (LBL_DEFER_FINISH): the
        // caller's stream is about to read the block.
        engine->finish_deferred();
        hipStream_t theirs = reinterpret_cast<hipStream_t>(stream);
        // Side streams end in an event their lane's main stream waits for (pedestal_done), so
        // the main streams and the copy stream stand for everything the engine has queued.
        for (auto & lane : engine->lanes)
        {
            lane.handed_over.record(lane.main);
            HIP_TRY(hipStreamWaitEvent(theirs, lane.handed_over, 0));
        }
        engine->copies_handed_over.record(engine->copy_stream);
        HIP_TRY(hipStreamWaitEvent(theirs, engine->copies_handed_over, 0));
        return LBL_OK;
    });
}

int lbl_order_engine_after_stream(lbl_engine * engine, void * stream)
{
    return entry(engine, [&] {
        HIP_TRY(hipSetDevice(engine->device));
        engine->taken_over.record(reinterpret_cast<hipStream_t>(stream));
        for (auto & lane : engine->lanes)
        {
            HIP_TRY(hipStreamWaitEvent(lane.main, engine->taken_over, 0));
            HIP_TRY(hipStreamWaitEvent(lane.side, engine->taken_over, 0));
        }
        HIP_TRY(hipStreamWaitEvent(engine->copy_stream, engine->taken_over, 0));
        return LBL_OK;
    });
}

int lbl_device_alloc(lbl_engine * engine, int64_t bytes, void ** pointer)
{
    if (engine == nullptr || pointer == nullptr || bytes < 0) return LBL_BAD_ARGUMENT;
    (void)hipSetDevice(engine->device);
    const int64_t size = std::max<int64_t>(bytes, 8);
    // (the allocation itself outside the lock: only the list of blocks is the engine's state)
    hipError_t status = hipMalloc(pointer, (size_t)size);
    if (status != hipSuccess) return fail(engine, LBL_ERROR, hipGetErrorString(status));
    return entry(engine, [&] {
        engine->device_blocks.push_back(lbl_engine::Block{static_cast<const char *>(*pointer), size});
        return LBL_OK;
    });
}

int lbl_device_free(lbl_engine * engine, void * pointer)
{
    return entry(engine, [&] {
        (void)hipSetDevice(engine->device);
        // A call kept back (LBL_DEFER_FINISH) that still has THIS block to write is finished first,
        // like in lbl_synchronize -- never left to run into freed memory.  (Any other block: the
        // deferral stays; a free from a finalizer thread must not reorder a pipeline's additions.)
        if (engine->deferred_touches(pointer, lbl_engine::forget(engine->device_blocks, pointer)))
        {
            // (a failure here is not the free's: what cannot be finished is dropped, and the
            // memory is freed all the same)
            try { engine->finish_deferred(); } catch (const HipFailure &) { engine->cancel_deferred(); }
        }
        engine->drain_lanes();
        hipError_t status = hipFree(pointer);
        if (status != hipSuccess) return fail(engine, LBL_ERROR, hipGetErrorString(status));
        return LBL_OK;
    });
}

int lbl_copy_to_host(lbl_engine * engine, void * host, const void * device, int64_t bytes)
{
    if (engine == nullptr || host == nullptr || device == nullptr || bytes < 0)
    {
        return LBL_BAD_ARGUMENT;
    }
    return entry(engine, [&] {
        (void)hipSetDevice(engine->device);
        engine->finish_deferred();
        // The memory may have been written on any lane (asynchronous calls with a pedestal rotate
        // over them): wait for all of them, not only for lane 0.
        hipError_t status = hipSuccess;
        for (auto & lane : engine->lanes)
        {
            if (status == hipSuccess) status = hipStreamSynchronize(lane.main);
        }
        if (status == hipSuccess)
        {
            status = hipMemcpyAsync(host, device, (size_t)bytes, hipMemcpyDeviceToHost,
                                    engine->stream);
        }
        if (status == hipSuccess) status = hipStreamSynchronize(engine->stream);
        if (status != hipSuccess) return fail(engine, LBL_ERROR, hipGetErrorString(status));
        return LBL_OK;
    });
}

int lbl_fill_zero(lbl_engine * engine, double * k, int32_t n_levels, int64_t n,
                  int64_t level_stride, int32_t flags)
{
    return entry(engine, [&] {
        if (k == nullptr || n_levels < 0 || n < 0 || (level_stride != 0 && level_stride < n))
        {
            return fail(engine, LBL_BAD_ARGUMENT, "lbl_fill_zero: bad argument.");
        }
        const int64_t stride = level_stride > 0 ? level_stride : n;
        if (n_levels == 0 || n == 0) return LBL_OK;
        if (!(flags & LBL_OUT_DEVICE))
        {
            for (int32_t l = 0; l < n_levels; ++l) std::memset(k + l*stride, 0, (size_t)n*8);
            return LBL_OK;
        }
        HIP_TRY(hipSetDevice(engine->device));
        // Ordered like a plain compute call: after everything queued on the other lanes --
        // by events when the caller does not wait either, so that the host keeps queueing.
        if (flags & LBL_ASYNC)
        {
            engine->join_lanes(engine->stream);
        }
        else
        {
            for (int i = 1; i < kAllLanes; ++i) engine->lanes[i].drain();
        }
        HIP_TRY(hipMemset2DAsync(k, (size_t)stride*8, 0, (size_t)n*8, (size_t)n_levels,
                                 engine->stream));
        engine->lanes[0].note_write(k, ((long long)(n_levels - 1)*stride + n)*8, engine->stream);
        if (!(flags & LBL_ASYNC)) HIP_TRY(hipStreamSynchronize(engine->stream));
        return LBL_OK;
    });
}

int lbl_copy_rows_to_host(lbl_engine * engine, void * host, int64_t host_pitch,
                          const void * device, int64_t device_pitch, int64_t row_bytes,
                          int64_t rows, int32_t flags)
{
    if (engine == nullptr || host == nullptr || device == nullptr || row_bytes < 0 || rows < 0 ||
        host_pitch < row_bytes || device_pitch < row_bytes)
    {
        return LBL_BAD_ARGUMENT;
    }
    if (rows == 0 || row_bytes == 0) return LBL_OK;
    return entry(engine, [&] {
        HIP_TRY(hipSetDevice(engine->device));
        engine->finish_deferred();      // the rows may be what a call kept back still has to write
        // The rows may have been written on any lane: the copy stream waits for what each of
        // them holds now, then copies beside whatever is queued afterwards.
        for (auto & lane : engine->lanes)
        {
            lane.queued.record(lane.main);
            HIP_TRY(hipStreamWaitEvent(engine->copy_stream, lane.queued, 0));
        }
        HIP_TRY(hipMemcpy2DAsync(host, (size_t)host_pitch, device, (size_t)device_pitch,
                                 (size_t)row_bytes, (size_t)rows, hipMemcpyDeviceToHost,
                                 engine->copy_stream));
        if (!(flags & LBL_ASYNC)) HIP_TRY(hipStreamSynchronize(engine->copy_stream));
        return LBL_OK;
    });
}

int lbl_host_alloc(lbl_engine * engine, int64_t bytes, void ** pointer)
{
    if (engine == nullptr || pointer == nullptr || bytes < 0) return LBL_BAD_ARGUMENT;
    (void)hipSetDevice(engine->device);
    const int64_t size = std::max<int64_t>(bytes, 8);
    hipError_t status = hipHostMalloc(pointer, (size_t)size, hipHostMallocDefault);    // (outside the lock)
    if (status != hipSuccess) return fail(engine, LBL_ERROR, hipGetErrorString(status));
    return entry(engine, [&] {
        engine->host_blocks.push_back(lbl_engine::Block{static_cast<const char *>(*pointer), size});
        return LBL_OK;
    });
}

int lbl_host_free(lbl_engine * engine, void * pointer)
{
    return entry(engine, [&] {
        (void)hipSetDevice(engine->device);
        if (engine->deferred_touches(pointer, lbl_engine::forget(engine->host_blocks, pointer)))
        {
            // The copies of the streamed call kept back target this memory.  (Any other array --
            // e.g. one a finalizer thread hands back while a pipeline is between its deferred call
            // and lbl_finish_deferred -- leaves the deferral alone.)  As in lbl_device_free, a
            // failure to finish drops the call instead of failing the free.
            try { engine->finish_deferred(); } catch (const HipFailure &) { engine->cancel_deferred(); }
            engine->drain_lanes();
        }
        engine->copy_stream.drain();
        hipError_t status = hipHostFree(pointer);
        if (status != hipSuccess) return fail(engine, LBL_ERROR, hipGetErrorString(status));
        return LBL_OK;
    });
}

}  // extern "C"
