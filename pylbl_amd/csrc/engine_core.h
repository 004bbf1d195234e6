// State of the engine: a molecule's resident line table and work-item plans, the lanes (stream
// pair + workspace) asynchronous calls rotate over, and struct lbl_engine itself -- options,
// timing spans, the write records calls are ordered by and the part of a call that
// LBL_DEFER_FINISH keeps back.  Every stream, event, device buffer and page-locked block in here
// is held by an owner type of hip_owners.h: nothing is released by hand, and ~lbl_engine and the
// order of its members decide what leaves when.  Included by engine.hip only (one translation
// unit).
#pragma once

#include "hip_owners.h"

namespace {

using namespace lbl;

thread_local std::string g_create_error;
// The message of the calling thread's last failure and the handle it belongs to: what
// lbl_last_error returns, so that a thread never reads a message another thread is writing.
thread_local std::string g_thread_error;
thread_local const void * g_thread_error_engine = nullptr;

struct Molecule
{
    long long n_lines = 0;
    // Host copies: row order (for the range rule) and sorted order (host prep, inspection).
    std::vector<double> nu_row;
    bool ascending = true;
    std::vector<int> order;                 // sorted position -> row
    std::vector<double> column[7];          // sorted: nu, sw, gamma_air, gamma_self, n_air, elower, delta_air
    std::vector<int> iso_slot;              // sorted
    double mass[kMassSlots];
    unsigned used_slots = 0;                // bit per isotopologue slot that has lines
    // Rows whose local_iso_id has no mass or no partition-function row.  The reference reads
    // past its tables for them (spectra.c:41-42); here they are an error -- but only when a
    // compute call would actually reach them (rows behind the range `break` never are).
    struct BadRow { int row; double nu; int local_iso_id; };
    std::vector<BadRow> bad_rows;
    double max_abs_delta = 0.;
    // Extremes over the table's rows, for the bound on y below which a level can have inner points.
    double min_gamma_air = 1.e300, min_gamma_self = 1.e300, min_n_air = 1.e300, max_n_air = -1.e300;
    int num_iso = 0, num_t = 0;
    std::vector<double> tips_t, tips_q;
    // Device copies (sorted).
    DeviceBuffer<double> d_column[7];
    DeviceBuffer<int> d_iso_slot, d_row, d_sorted_of_row;
    // cell_first of LineTableView (tile_schedule.h): where the sorted table reaches every
    // 1/cell_scale cm-1.
    DeviceBuffer<int> d_cell_first;
    double cell_base = 0., cell_scale = 0.;
    int cell_entries = 0;

    // Work-item plans, one per (grid, cut_off, tiling) this molecule has been computed on.
    struct Plan
    {
        int v0, vn, n_per_v, cut_off, points, aligned, farfield;
        int pieces = 1;         // the tiles in `pieces` runs of about equal weight (streamed calls)
        int n_items = 0, n_split = 0;
        long long partial_slots = 0;
        DeviceBuffer<WorkItem> items;       // piece-major, heaviest first within a piece
        DeviceBuffer<SplitTile> split;      // piece-major
        std::vector<int> item_begin, split_begin, tile_begin;   // [pieces + 1] each

        // The grid points [q0, q1) of a piece's run of tiles; q0 == q1 == 0 where the run is empty.
        void point_range(int piece, const Tiling & tiling, const GridSpec & g, long long & q0,
                         long long & q1) const
        {
            long long unused = 0;
            q0 = q1 = 0;
            if (tile_begin[piece + 1] > tile_begin[piece])
            {
                tile_bounds(tiling, tile_begin[piece], g.n_per_v, g.n, q0, unused);
                tile_bounds(tiling, tile_begin[piece + 1] - 1, g.n_per_v, g.n, unused, q1);
                q1 += 1;
            }
        }
    };
    std::vector<std::unique_ptr<Plan>> plans;

    LineTableView view() const
    {
        LineTableView v;
        v.nu = d_column[0].data; v.sw = d_column[1].data; v.gamma_air = d_column[2].data;
        v.gamma_self = d_column[3].data; v.n_air = d_column[4].data;
        v.elower = d_column[5].data; v.delta_air = d_column[6].data;
        v.iso_slot = d_iso_slot.data; v.row = d_row.data;
        v.sorted_of_row = d_sorted_of_row.data; v.n_lines = n_lines;
        v.cell_first = cell_entries > 0 ? d_cell_first.data : nullptr;
        v.cell_base = cell_base; v.cell_scale = cell_scale; v.cell_entries = cell_entries;
        return v;
    }
};

// (kTimeSchedule: schedule_kernel alone, which only host-side prep launches; the far-field series
// kernels are booked there too -- with device prep the index would otherwise stay empty)
enum { kTimePrepare = 0, kTimeSchedule = 1, kTimeAccumulate = 2, kTimePedestal = 3,
       kTimeBandSpectra = 4, kTimeContinuum = 5, kTimeXsecModel = 6, kTimeXsec = 7,
       kTimeKinds = 8 };

// One in-flight compute call: its own pair of streams and its own workspace, so that
// several molecules can be in the pipeline at once (the serial pedestal chain of one
// overlaps the accumulate kernels of the others, and its own).
struct Lane
{
    // (The streams first: members leave in reverse order, so every event and buffer below is
    // gone before the streams are.)
    Stream main;                    // prepare, schedule, accumulate, apply, copies
    Stream side;                    // the pedestal pre-pass
    Event prepared, pedestal_done, runs_found;
    Event queued;                   // what the copy stream waits for (lbl_copy_rows_to_host)
    Event handed_over;              // what a caller's stream waits for (lbl_order_stream_after_engine)
    Event piece_done[8];            // behind the last kernel of each piece of a streamed call
    Event piece_summed[8];          // behind a piece's accumulate launch (pedestal: applied elsewhere)
    // One pass of a lines call (levels [base, base + count) of the request): where its spectra end
    // up, where the accumulate kernel writes, and the streams its later stages run on.
    struct Pass
    {
        long long base = 0;
        int count = 0;
        double * target = nullptr;      // the caller's block, or the lane's staging block
        long long target_stride = 0;
        double * sums = nullptr;        // == target unless a pedestal is applied on the way into it
        long long sums_stride = 0;
        hipStream_t ped_stream = nullptr;       // the pedestal pre-pass
        hipStream_t finish_stream = nullptr;    // where the pieces are finished
    };
    // How the pieces of a pass are finished (compute_stages.inc, describe_finish).  Without a
    // pedestal that is the copy of a streamed call's columns, queued behind each piece's launch.
    // With one it is the last part of the call -- the kernels that apply the pedestal to the
    // caller's block, piece by piece, and those copies -- which LBL_DEFER_FINISH keeps back until
    // lbl_finish_deferred: everything before works in the lane's own buffers, so a long call can be
    // queued FIRST and still be the LAST to add into a block other calls write meanwhile.
    struct Finish
    {
        bool pending = false;
        Pass pass;
        GridSpec g;
        int pieces = 1, flags = 0;
        long long point_begin[9] = {};      // piece p covers points [point_begin[p], point_begin[p+1])
        bool streamed = false, order_writers = false, add_into = false;
        char * host = nullptr;
        long long host_pitch = 0, columns = 0;
        double * k = nullptr;          // the block, for its write record: set by the call's last pass only
        const double * block = nullptr; // the block, for ordering behind its earlier writers: every pass
        long long out_bytes = 0;
    } finish;
    // The last few writes of device output queued on this lane: where, and an event behind the
    // kernel that wrote.  A call on another lane that touches the same memory waits for it.
    struct Write { const char * begin = nullptr; const char * end = nullptr; Event done; };
    static constexpr int kWrites = 4;
    Write writes[kWrites];
    int next_write = 0;
    bool writes_wrapped = false;
    bool used = false;              // something was queued here since lane 0 last joined it
    DeviceBuffer<LineWing> wing;
    DeviceBuffer<LineCore> core;
    DeviceBuffer<WingGroup> groups; // [levels][ceil(n_lines/8)]: the table-aligned eights, scaled
    DeviceBuffer<TileSchedule> schedule;
    DeviceBuffer<LevelScalars> levels;
    DeviceBuffer<double> staging;   // spectra on their way to host memory
    DeviceBuffer<double> raw;       // un-pedestalled sums when the output must be added to
    DeviceBuffer<double> partial;   // partial sums of split tiles
    DeviceBuffer<double> far_series; // [levels][tiles][kFarTerms]
    DeviceBuffer<double> derived;
    DeviceBuffer<unsigned long long> evals;
    DeviceBuffer<int> wing_bounds;  // [levels][kWingBounds] of the pass (line_prep.h)
    PedestalWorkspace pedestal;
    PinnedFeed<LevelScalars> level_feed;    // the level scalars of a pass on their way to `levels`

    // The events are made here, not at first use: no call pays for one.
    void create(bool urgent = false)
    {
        // The pre-pass is short and latency-bound (a serial chain): its queue goes first
        // whenever the accumulate grid frees a slot.
        main.create(urgent);
        side.create(true);
        for (Event * e : {&prepared, &pedestal_done, &runs_found, &queued, &handed_over,
                          &level_feed.copied})
        {
            e->create();
        }
        for (auto & e : piece_done) e.create();
        for (auto & e : piece_summed) e.create();
        for (auto & w : writes) w.done.create();
    }
    void drain()
    {
        main.drain();
        side.drain();
    }
    // Nothing a lane owns is released while its streams still run.
    ~Lane() { drain(); }
    // Everything queued on `stream` (this lane's) so far has written [begin, end).
    void note_write(const void * begin, long long bytes, hipStream_t stream)
    {
        Write & w = writes[next_write];
        w.begin = reinterpret_cast<const char *>(begin);
        w.end = w.begin + bytes;
        w.done.record(stream);
        next_write = (next_write + 1) % kWrites;
        if (next_write == 0) writes_wrapped = true;
    }
};

constexpr int kLanes = 8;           // lanes the lines calls rotate over
// One more lane carries the continuum and cross-section calls: short, bandwidth-bound kernels
// on a stream of the highest priority, so that they are dispatched as soon as workgroup slots
// free up instead of queueing behind a resident accumulate grid of another lane (a 6 us
// band_spectra_kernel was seen waiting 0.9 ms for one).
constexpr int kSlotLane = kLanes;
constexpr int kAllLanes = kLanes + 1;

// Level scalars of a batched call on their way to the device: a pinned block, its device
// copy and an event that marks the last kernel reading them (and the per-level workspace that
// goes with them), so that a later call on the same object waits for that only.
template <typename Level>
struct LevelFeed
{
    DeviceBuffer<Level> levels;
    PinnedFeed<Level> pinned;
    Event done;                     // last kernel of the last call (the destructor waits for it)

    void mark(hipStream_t stream) { done.record(stream); }
    ~LevelFeed() { if (done != nullptr) (void)hipEventSynchronize(done); }
};

// One continuum (continuum.h): its bands, their coefficient table and the per-level
// workspace of coarse spectra.
struct ContinuumSet : LevelFeed<ContinuumLevel>
{
    BandSet set;
    DeviceBuffer<double> table;
    DeviceBuffer<double> coarse;        // [levels][set.coarse_points]
    DeviceBuffer<double> slopes;        // same shape: slope of the interval after each knot
    DeviceBuffer<double> staging;       // extinction on its way to host memory
    int widest = 0;                     // points of the largest band
};

// The cross-section bands of one molecule (xsec.h).
struct XsecData : LevelFeed<XsecLevel>
{
    XsecSet set;
    DeviceBuffer<double> fgrid;         // concatenated band frequency grids [Hz]
    DeviceBuffer<double> coeffs;        // per band [4][size]
    DeviceBuffer<double> values;        // [levels][set.total]: the fit on the bands' grids
    DeviceBuffer<double> slopes;        // same shape
    DeviceBuffer<double> staging;
};

struct SpectralGrid
{
    long long n = 0;
    bool ascending = true;
    // wavenumber[i] == start + (double)i*step for every i, checked element by element at load
    // (what numpy.arange produces): the interpolation kernels then form x in registers.
    bool arithmetic = false;
    double start = 0., step = 0.;
    DeviceBuffer<double> wavenumber;

    GridForm form() const
    {
        return GridForm{wavenumber.data, arithmetic ? 1 : 0, start, step};
    }
};

// An instrument bound to a grid: its channels, tiles and items, the tables of its shape and a
// copy of the grid's wavenumbers, all on the device in one block of 8-byte words.
struct Instrument
{
    int shape = 0, n_channels = 0, n_items = 0, n_table = 0;
    long long grid_points = 0;
    DeviceBuffer<double> words;
    const InstrChannel * channel = nullptr;
    const InstrItem * item = nullptr;
    const long long * tile_channel = nullptr;
    const double * offsets = nullptr;
    const double * response = nullptr;
    const double * nu = nullptr;
};

// Several continua evaluated in one pass (continuum.h, group kernels): the bands of all of them
// in one list on the device, one workspace of coarse spectra, one block of level scalars
// [continuum][level].  Kept per list of handles; dropped when one of them is freed.
struct ContinuumGroup : LevelFeed<ContinuumLevel>
{
    std::vector<int32_t> members;
    DeviceBuffer<GroupBand> bands;
    int n_bands = 0, level_points = 0, widest = 0;
    DeviceBuffer<double> coarse, slopes;    // [levels][level_points]
};

// Tables of lbl_path_compute (path.h): the path lengths of a run, the band starts, each band's
// first segment and the segments, staged in one page-locked block and uploaded in one copy; and
// the band partial sums.  Every kernel that reads them runs on the engine's first stream, behind
// the upload of the next call's tables.
struct PathWorkspace
{
    DeviceBuffer<double> tables;
    DeviceBuffer<double> partial;       // [rows][segments]
    PinnedFeed<double> staged;
};

}  // namespace

struct lbl_engine
{
    // Every entry point of the C ABI that takes this handle holds the mutex while it reads or
    // changes the engine's host-side state (lanes, plans, workspaces, write records, options) and
    // queues its work; the GPU work itself runs asynchronously.  The reference's absorption() has
    // no state at all (absorption.c:19-99) and ctypes releases the GIL around it
    // (gas_optics.py:79-91), so any number of threads may call it at once: so may they here.
    // (Recursive: lbl_synchronize finishes a deferred call through the public entry.)
    std::recursive_mutex mutex;
    int device = 0;
    hipStream_t stream = nullptr;   // == lanes[0].main: uploads, and what lbl_stream() returns
    // The runtime multiplexes its streams onto a handful of hardware queues (GPU_MAX_HW_QUEUES, 4
    // by default) in an order of its own, and a queue runs its packets one after the other: a copy
    // that shares its queue with the main stream of the lane that is computing waits for that
    // lane's accumulate launches instead of running beside them.  For the call that delivers its
    // result piece by piece that was 1.9 against 1.6 ms (Spectroscopy's "total"), decided by
    // nothing but which lane the call had been dealt (profiles/r04_copy_streams.txt).  The engine
    // asks the GPU once, when it is created, which lanes share a queue with the copy stream
    // (calibrate_delivery_lanes), and a delivering call skips those.  (One copy stream per lane,
    // each chosen to run beside it, was tried first: slower than the best single one -- every
    // further stream in use is one more queue for the hardware to take turns on.)
    bool delivers_badly[kLanes] = {};
    // Members leave in reverse order, after the destructor's body has drained every stream and
    // dropped the handle tables: the timing events and `path` first, then the lanes, then the
    // copy stream, then these two.  Nothing waits on a stream that is gone.
    Event copies_handed_over, taken_over;   // lbl_order_*_after_*
    Stream copy_stream;             // results on their way to host memory
    std::string error;
    std::vector<std::unique_ptr<Molecule>> molecules;
    std::vector<std::unique_ptr<ContinuumSet>> continua;
    std::vector<std::unique_ptr<SpectralGrid>> grids;
    std::vector<std::unique_ptr<XsecData>> xsecs;
    std::vector<std::unique_ptr<ContinuumGroup>> groups;
    std::vector<std::unique_ptr<Instrument>> instruments;
    Lane lanes[kAllLanes];
    unsigned next_lane = 0;
    PathWorkspace path;             // lbl_path_compute

    // Options.
    int prep = LBL_PREP_DEVICE;
    int points_per_lane = 0;
    int timing = 0;
    long long workspace_bytes = 4ll << 30;
    int ablate = 0;
    int aligned_tiles = 0;          // measured: no gain at 0.001 cm-1
    int wing_batches = kWingBatchesMax; // cap on the far-wing batches per reciprocal (line_prep.h)
    int overlap_pedestal = 1;       // run the pedestal pre-pass beside the accumulate kernel
    int farfield = 0;               // sum distant lines by their power series (farfield.h)
    int scan_chain = 1;             // pedestal chain by relaxation (pedestal.h), serial chain behind it
    int relax_launches = 0;         // relaxation launches before the serial chain (2 ... 7; 0: by the table)
    int poison_workspace = 0;       // test hook: NaN-fill the pre-pass's double buffers first (pedestal.h)
    int lanes_in_use = 0;           // lanes the asynchronous calls rotate over; 0: by kind of call
    long long small_points = 1ll << 20;    // grids (points x levels) up to this size count as small
    int overlap_plain = 1;          // plain asynchronous calls on larger grids take turns on two lanes too
    int skip_delivery_lanes = 1;    // delivering calls avoid lanes that share the copy stream's queue

    // Timing.
    struct Span { Event begin, end; int kind, counts; };
    std::vector<Span> spans;
    std::vector<Event> event_pool;      // timing events between uses
    double time_ms[kTimeKinds] = {};
    double busy_ms[kTimeKinds] = {};    // time during which AT LEAST ONE timed span of the kind ran
    double busy_reach[kTimeKinds] = {}; // where the union of the kind's spans ends so far [ms from epoch]
    Event epoch;                        // origin of the spans' positions (reset_epoch)
    long long launches[kTimeKinds] = {};

    Event take_event()
    {
        Event e(true);
        if (!event_pool.empty())
        {
            e = std::move(event_pool.back());
            event_pool.pop_back();
        }
        e.create();
        return e;
    }

    // Every stream drained, then whatever the handles stand for; the members follow (see above).
    ~lbl_engine()
    {
        drain_lanes();
        molecules.clear();
        groups.clear();
        continua.clear();
        xsecs.clear();
        grids.clear();
        instruments.clear();
    }

    template <typename F>
    void timed(int kind, hipStream_t on, F && launch, int counts = 1)
    {
        if (!timing || (timing == 2 && kind != kTimeAccumulate && kind != kTimeSchedule))
        {
            launch();
            return;
        }
        Span s{take_event(), take_event(), kind, counts};
        s.begin.record(on);
        launch();
        s.end.record(on);
        spans.push_back(std::move(s));
        if (spans.size() >= 4096) drain_spans();
    }

    // Sums the spans' durations per kind (time_ms) and, because calls on different lanes run side
    // by side, also the length of the UNION of the spans of a kind on the device's clock (busy_ms:
    // two launches that overlap count once).  Positions are milliseconds (double) from `epoch`, an
    // event recorded on the engine's first stream when timing was last reset: it precedes every
    // span on the device's clock, whichever lane a span ran on, and it is the same origin for every
    // batch, so that the reach of the union carries over from one batch to the next (a launch that
    // straddles a batch boundary is counted once).  A span whose position cannot be read (an event
    // the runtime places before the epoch) is clamped to the epoch.
    void drain_spans()
    {
        if (spans.empty()) return;
        std::vector<std::pair<double, double>> placed[kTimeKinds];
        for (auto & s : spans) s.end.synchronize();
        epoch.synchronize();
        for (auto & s : spans)
        {
            float ms = 0.f, from = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, s.begin, s.end));
            time_ms[s.kind] += ms;
            launches[s.kind] += s.counts;
            if (epoch == nullptr || hipEventElapsedTime(&from, epoch, s.begin) != hipSuccess ||
                !(from > 0.f))
            {
                (void)hipGetLastError();
                from = 0.f;
            }
            placed[s.kind].push_back({(double)from, (double)from + (double)ms});
        }
        for (int kind = 0; kind < kTimeKinds; ++kind)
        {
            auto & list = placed[kind];
            std::sort(list.begin(), list.end());
            double & reach = busy_reach[kind];      // end of the union so far, carried over batches
            for (const auto & interval : list)
            {
                if (interval.first > reach)
                {
                    busy_ms[kind] += interval.second - interval.first;
                    reach = interval.second;
                }
                else if (interval.second > reach)
                {
                    busy_ms[kind] += interval.second - reach;
                    reach = interval.second;
                }
            }
        }
        for (auto & s : spans)
        {
            event_pool.push_back(std::move(s.begin));
            event_pool.push_back(std::move(s.end));
        }
        spans.clear();
    }

    // A fresh origin for the spans' positions (lbl_timing with reset, option "timing" switched on).
    void reset_epoch()
    {
        if (epoch == nullptr) epoch = take_event();
        epoch.record(stream);
        for (int kind = 0; kind < kTimeKinds; ++kind) busy_reach[kind] = 0.;
    }

    void drain_lanes()
    {
        for (auto & lane : lanes) lane.drain();
        copy_stream.drain();
    }

    // Orders `stream` (a stream of lane `self`) behind every write of [begin, begin + bytes) queued
    // on the other lanes.  Each lane remembers its last few writes; older ones were queued before
    // the oldest it remembers, whose event therefore stands in for them.
    void order_after_writers(hipStream_t stream, const void * begin, long long bytes,
                             const Lane * self)
    {
        const char * b = reinterpret_cast<const char *>(begin);
        const char * e = b + bytes;
        for (auto & lane : lanes)
        {
            if (&lane == self) continue;
            for (const auto & w : lane.writes)
            {
                if (w.begin != nullptr && b < w.end && w.begin < e)
                {
                    HIP_TRY(hipStreamWaitEvent(stream, w.done, 0));
                }
            }
            if (lane.writes_wrapped)
            {
                HIP_TRY(hipStreamWaitEvent(stream, lane.writes[lane.next_write].done, 0));
            }
        }
    }

    Lane * deferred = nullptr;      // the lane whose call waits for lbl_finish_deferred

    // Memory handed out by lbl_device_alloc / lbl_host_alloc: base address and size, so that a
    // free knows whether a call kept back (LBL_DEFER_FINISH) still has that memory to write.
    struct Block { const char * begin; long long bytes; };
    std::vector<Block> device_blocks, host_blocks;

    static long long forget(std::vector<Block> & blocks, const void * pointer)
    {
        for (size_t i = 0; i < blocks.size(); ++i)
        {
            if (blocks[i].begin == pointer)
            {
                const long long bytes = blocks[i].bytes;
                blocks.erase(blocks.begin() + i);
                return bytes;
            }
        }
        return -1;      // not one of ours (or freed twice): the caller assumes the worst
    }

    // Does the call kept back write into [begin, begin + bytes)?  bytes < 0: size unknown, yes.
    bool deferred_touches(const void * begin, long long bytes) const
    {
        if (deferred == nullptr || !deferred->finish.pending) return false;
        if (bytes < 0) return true;
        const Lane::Finish & f = deferred->finish;
        const char * b = reinterpret_cast<const char *>(begin);
        const char * e = b + bytes;
        auto meets = [&](const void * p, long long n) {
            const char * q = reinterpret_cast<const char *>(p);
            return p != nullptr && n > 0 && q < e && b < q + n;
        };
        const Lane::Pass & p = f.pass;
        const long long rows = ((long long)(p.count - 1)*p.target_stride + f.point_begin[f.pieces])*8;
        return meets(f.k, f.out_bytes) || meets(p.target, rows) ||
               (f.streamed && meets(f.host + p.base*f.host_pitch,
                                    (long long)(p.count - 1)*f.host_pitch + f.columns*8));
    }

    // A streamed call: the columns of a finished piece to page-locked host memory, behind what
    // `after` holds now, beside the kernels of the next piece.  (The runtime's device-to-host copy
    // is a kernel of its own here, not a DMA engine; queued beside an accumulate grid it costs the
    // grid nothing, and a hand-written copy kernel of 8..1024 workgroups did worse:
    // profiles/r03_perf_deliver.txt.)
    void copy_piece_home(Lane & lane, int piece, hipStream_t after)
    {
        const Lane::Finish & f = lane.finish;
        const Lane::Pass & p = f.pass;
        const long long q0 = f.point_begin[piece], q1 = f.point_begin[piece + 1];
        if (!f.streamed || q1 <= q0 || q0 >= f.columns) return;
        const long long c1 = std::min<long long>(q1, f.columns);
        lane.piece_done[piece].record(after);
        HIP_TRY(hipStreamWaitEvent(copy_stream, lane.piece_done[piece], 0));
        HIP_TRY(hipMemcpy2DAsync(f.host + p.base*f.host_pitch + q0*8, (size_t)f.host_pitch,
                                 p.target + q0, (size_t)p.target_stride*8, (size_t)(c1 - q0)*8,
                                 (size_t)p.count, hipMemcpyDeviceToHost, copy_stream));
    }

    // Queues what Lane::Finish describes: apply kernels (+ copies) of every piece, then ties the
    // lane's main stream and the block's write record to the last of them.
    void run_finish(Lane & lane)
    {
        Lane::Finish & f = lane.finish;
        const Lane::Pass & p = f.pass;
        const GridSpec & g = f.g;
        hipStream_t stream = lane.main;
        // (what is queued here is queued NOW: a call that joined this lane since the kept-back
        // call was made has to join it again)
        lane.used = true;
        if (f.order_writers)
        {
            // (every pass of a call in several passes: the FIRST pass's kernels are the ones that
            // must not add into rows another lane's earlier call is still adding into)
            order_after_writers(p.finish_stream, f.block, f.out_bytes, &lane);
        }
        for (int piece = 0; piece < f.pieces; ++piece)
        {
            const long long q0 = f.point_begin[piece], q1 = f.point_begin[piece + 1];
            if (q1 <= q0) continue;
            if (p.finish_stream != stream)
            {
                // (recorded behind this piece's accumulate launch)
                HIP_TRY(hipStreamWaitEvent(p.finish_stream, lane.piece_summed[piece], 0));
            }
            constexpr int per_block = 256*kApplyPoints;
            dim3 grid((unsigned)((q1 - q0 + per_block - 1)/per_block), (unsigned)p.count);
            hipLaunchKernelGGL(pedestal_apply_kernel, grid, dim3(256),
                               pedestal_apply_lds_bytes(g.cut_off, g.n_per_v), p.finish_stream,
                               p.sums, p.sums_stride, p.target, p.target_stride,
                               lane.pedestal.bin_sum.data, lane.levels.data, (int)q0, (int)q1,
                               g.n_per_v, g.vn - g.v0 + 2*g.cut_off + 3, g.cut_off,
                               pedestal_apply_span(g.n_per_v),
                               (f.flags & LBL_SCALE_DENSITY) ? 1 : 0, f.add_into ? 1 : 0);
            HIP_TRY(hipGetLastError());
            copy_piece_home(lane, piece, p.finish_stream);
        }
        if (p.finish_stream != stream)
        {
            // Later users of the lane's main stream (and of the block) come after the last apply.
            lane.pedestal_done.record(p.finish_stream);
            HIP_TRY(hipStreamWaitEvent(stream, lane.pedestal_done, 0));
        }
        if (f.k != nullptr)
        {
            lane.note_write(f.k, f.out_bytes, stream);
        }
        f.pending = false;
        if (deferred == &lane) deferred = nullptr;
    }

    void finish_deferred()
    {
        if (deferred != nullptr && deferred->finish.pending)
        {
            run_finish(*deferred);
        }
        deferred = nullptr;
    }

    // Drops what a call kept back instead of queueing it (lbl_cancel_deferred): its target block
    // and host range are never touched by that call.  What it has queued already works in the
    // lane's own buffers only.
    void cancel_deferred()
    {
        if (deferred != nullptr) deferred->finish.pending = false;
        deferred = nullptr;
    }

    // Orders `stream` (lane 0's) behind everything queued on the other lanes so far, without
    // stopping the host: what a call that adds into its output, or reuses lane 0 after calls
    // that rotated over the lanes, needs.
    void join_lanes(hipStream_t stream)
    {
        for (int i = 1; i < kAllLanes; ++i)
        {
            if (!lanes[i].used) continue;
            lanes[i].queued.record(lanes[i].main);
            HIP_TRY(hipStreamWaitEvent(stream, lanes[i].queued, 0));
            lanes[i].used = false;
        }
    }
};

namespace {

struct ComputeRequest
{
    int32_t molecule, n_levels;
    const double * temperature, * pressure, * vmr;
    int32_t v0, vn, n_per_v, cut_off, remove_pedestal, range_policy, flags;
    double * k;
    int64_t level_stride;
    int64_t * evals;
    double * derived;      // host, n_lines x 8 in row order, single level only
    // lbl_compute_streamed: the first `columns` points of every level also go to host memory,
    // piece by piece as the kernels of a piece finish.
    char * host = nullptr;
    int64_t host_pitch = 0, columns = 0;
    int32_t pieces = 1;
};

}  // namespace
