// Owners of the HIP resources the host side holds: one type each for an event, a stream, a device
// buffer and a page-locked staging block with the event behind its last upload.  Each releases
// what it owns in its destructor, without throwing, and none can be copied.  HipFailure is what
// every failed HIP call on the host side becomes (HIP_TRY); the entry frame turns it into a status.
// Included by pedestal.h and engine_core.h; no kernel in here.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <utility>

namespace lbl {

struct HipFailure
{
    std::string message;
};

inline void hip_check(hipError_t status, const char * what)
{
    if (status != hipSuccess) throw HipFailure{std::string(what) + ": " + hipGetErrorString(status)};
}

#define HIP_TRY(call) ::lbl::hip_check((call), #call)

// One event, made at first use -- record() or create() -- so that it is made with the device of
// the entry that uses it current, and an object nobody calls costs none.  Without timing unless
// asked for.  Converts to the handle (null until made) for hipStreamWaitEvent and the like.
struct Event
{
    hipEvent_t handle = nullptr;
    bool timing = false;

    explicit Event(bool with_timing = false) : timing(with_timing) {}
    Event(Event && other) noexcept : handle(other.handle), timing(other.timing) { other.handle = nullptr; }
    Event & operator=(Event && other) noexcept
    {
        std::swap(handle, other.handle);
        std::swap(timing, other.timing);
        return *this;
    }
    ~Event() { if (handle != nullptr) (void)hipEventDestroy(handle); }

    void create()
    {
        if (handle != nullptr) return;
        HIP_TRY(hipEventCreateWithFlags(&handle, timing ? hipEventDefault : hipEventDisableTiming));
    }
    void record(hipStream_t stream)
    {
        create();
        HIP_TRY(hipEventRecord(handle, stream));
    }
    // Stops the host until what was recorded has run; nothing to wait for if nothing ever was.
    void synchronize() const
    {
        if (handle != nullptr) HIP_TRY(hipEventSynchronize(handle));
    }
    operator hipEvent_t() const { return handle; }
};

// One non-blocking stream, plain or (urgent) at the greatest priority the device has.  Destroying
// it does not wait: whoever owns it drains it first where that matters.
struct Stream
{
    hipStream_t handle = nullptr;

    void create(bool urgent = false)
    {
        if (!urgent) return HIP_TRY(hipStreamCreateWithFlags(&handle, hipStreamNonBlocking));
        int least = 0, greatest = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIP_TRY(hipStreamCreateWithPriority(&handle, hipStreamNonBlocking, greatest));
    }
    // Stops the host until the stream is empty; a stream never made has nothing queued.
    void drain() const noexcept
    {
        if (handle != nullptr) (void)hipStreamSynchronize(handle);
    }
    operator hipStream_t() const { return handle; }
    ~Stream() { if (handle != nullptr) (void)hipStreamDestroy(handle); }
    Stream() = default;
    Stream(const Stream &) = delete;
    Stream & operator=(const Stream &) = delete;
};

template <typename T>
struct DeviceBuffer
{
    T * data = nullptr;
    size_t capacity = 0;   // elements

    void reserve(size_t count)
    {
        if (count <= capacity) return;
        release();
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&data), count*sizeof(T)));
        capacity = count;
    }
    void release()
    {
        if (data != nullptr)
        {
            (void)hipFree(data);
            data = nullptr;
            capacity = 0;
        }
    }
    void upload(const T * host, size_t count, hipStream_t stream)
    {
        reserve(count);
        if (count > 0)
        {
            HIP_TRY(hipMemcpyAsync(data, host, count*sizeof(T), hipMemcpyHostToDevice, stream));
        }
    }
    ~DeviceBuffer() { release(); }
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer & operator=(const DeviceBuffer &) = delete;
};

// A page-locked block the host fills and a stream uploads from, again and again: the block, the
// event behind the last upload out of it and whether that upload may still be running.  The host
// may refill the block once the copy that read it has run; everything on the device side is
// ordered by the stream.
template <typename T>
struct PinnedFeed
{
    T * block = nullptr;
    size_t capacity = 0;   // elements
    Event copied;          // behind the last upload out of `block`
    bool in_flight = false;

    void wait()
    {
        if (in_flight) copied.synchronize();
        in_flight = false;
    }
    // The block, free to be written, with room for `count` elements.
    T * refill(size_t count)
    {
        wait();
        if (count > capacity)
        {
            release();
            HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&block), count*sizeof(T),
                                  hipHostMallocDefault));
            capacity = count;
        }
        return block;
    }
    void upload(T * device, size_t count, hipStream_t stream)
    {
        HIP_TRY(hipMemcpyAsync(device, block, count*sizeof(T), hipMemcpyHostToDevice, stream));
        copied.record(stream);
        in_flight = true;
    }
    void release() noexcept
    {
        if (block != nullptr) (void)hipHostFree(block);
        block = nullptr;
        capacity = 0;
    }
    ~PinnedFeed()
    {
        if (copied != nullptr) (void)hipEventSynchronize(copied);
        release();
    }
};

}  // namespace lbl
