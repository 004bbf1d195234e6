// lbl_instrument_create / lbl_instrument_free / lbl_instrument_apply: channel means of rows of
// fine-grid values under an instrument line shape (kernels: instrument.h).  Included by
// engine.hip after path_entry.inc (PathWorkspace, path_entry).
namespace {

template <typename T>
size_t words_of(size_t count)
{
    static_assert(sizeof(T) % 8 == 0, "staged as 8-byte words");
    return count*sizeof(T)/8;
}

// nullptr, or what is wrong with the arguments of lbl_instrument_create.
const char * instrument_check(int32_t shape, int32_t n_channels, const double * centers,
                              const double * parameter, const double * half_width,
                              int32_t n_table, const double * offsets, const double * response,
                              int32_t response_rows)
{
    if (shape < kInstrBoxcar || shape > kInstrTabulated) return "unknown shape.";
    if (n_channels < 1 || centers == nullptr) return "need n_channels >= 1 and centers.";
    for (int c = 0; c < n_channels; ++c)
    {
        if (!std::isfinite(centers[c])) return "centers must be finite.";
    }
    if (shape == kInstrTabulated)
    {
        if (n_table < 2 || offsets == nullptr || response == nullptr)
        {
            return "a tabulated shape needs n_table >= 2, offsets and response.";
        }
        if (response_rows != 1 && response_rows != n_channels)
        {
            return "response_rows must be 1 or n_channels.";
        }
        for (int k = 0; k < n_table; ++k)
        {
            if (!std::isfinite(offsets[k])) return "offsets must be finite.";
            if (k > 0 && !(offsets[k] > offsets[k - 1]))
            {
                return "offsets must be strictly increasing.";
            }
        }
        for (long long i = 0; i < (long long)n_table*response_rows; ++i)
        {
            if (!std::isfinite(response[i])) return "response must be finite.";
        }
        return nullptr;
    }
    if (parameter == nullptr || !finite_at_least_zero(parameter, n_channels, true))
    {
        return "widths, fwhm or max path differences must be finite and > 0.";
    }
    if (shape == kInstrGaussian || shape == kInstrFts || shape == kInstrFtsHamming)
    {
        if (half_width == nullptr || !finite_at_least_zero(half_width, n_channels, true))
        {
            return "half widths must be finite and > 0.";
        }
    }
    return nullptr;
}

}  // namespace

extern "C" {

int lbl_instrument_create(lbl_engine * engine, int32_t grid, int32_t shape, int32_t n_channels,
                          const double * centers, const double * parameter,
                          const double * half_width, int32_t n_table, const double * offsets,
                          const double * response, int32_t response_rows, int32_t * handle)
{
    return entry(engine, [&] {
        auto bad = [&](const char * what) {
            return fail(engine, LBL_BAD_ARGUMENT, std::string("lbl_instrument_create: ") + what);
        };
        if (handle == nullptr) return bad("handle is NULL.");
        const SpectralGrid * g = find_slot(engine->grids, grid);
        if (g == nullptr) return bad("unknown grid handle.");
        if (!g->ascending) return bad("the grid must be ascending.");
        if (const char * problem = instrument_check(shape, n_channels, centers, parameter,
                                                    half_width, n_table, offsets, response,
                                                    response_rows))
        {
            return bad(problem);
        }
        HIP_TRY(hipSetDevice(engine->device));
        std::vector<double> nu((size_t)g->n);
        HIP_TRY(hipMemcpyAsync(nu.data(), g->wavenumber.data, nu.size()*8,
                               hipMemcpyDeviceToHost, engine->stream));
        HIP_TRY(hipStreamSynchronize(engine->stream));

        // Windows [lo, hi] and their columns: searchsorted(grid, lo, "left") <= j <
        // searchsorted(grid, hi, "right").  A channel counts when its window holds points and
        // lies wholly inside [grid[0], grid[n - 1]].
        std::unique_ptr<Instrument> in(new Instrument());
        in->shape = shape;
        in->n_channels = n_channels;
        in->n_table = shape == kInstrTabulated ? n_table : 0;
        in->grid_points = g->n;
        std::vector<InstrChannel> channel((size_t)n_channels);
        std::vector<int> order;
        for (int c = 0; c < n_channels; ++c)
        {
            const double center = centers[c];
            double lo, hi;
            if (shape == kInstrTabulated)
            {
                lo = center + offsets[0];
                hi = center + offsets[n_table - 1];
            }
            else
            {
                const double h = shape == kInstrBoxcar ? parameter[c]/2.
                               : shape == kInstrTriangle ? parameter[c] : half_width[c];
                lo = center - h;
                hi = center + h;
            }
            InstrChannel & ch = channel[c];
            ch = InstrChannel{};
            ch.begin = std::lower_bound(nu.begin(), nu.end(), lo) - nu.begin();
            ch.end = std::upper_bound(nu.begin(), nu.end(), hi) - nu.begin();
            ch.center = center;
            ch.parameter = shape == kInstrTabulated ? 0. : parameter[c];
            ch.row = shape == kInstrTabulated && response_rows > 1 ? c : 0;
            ch.valid = ch.begin < ch.end && lo >= nu.front() && hi <= nu.back() ? 1 : 0;
            if (ch.valid) order.push_back(c);
        }
        // Tiles of kInstrTile channels in window order; their items are the segments of the
        // union of their windows that some window touches, cut at multiples of kInstrSegment
        // from the union's first column.
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
            return channel[x].begin != channel[y].begin ? channel[x].begin < channel[y].begin
                                                        : channel[x].end < channel[y].end;
        });
        const size_t tiles = (order.size() + kInstrTile - 1)/kInstrTile;
        std::vector<long long> tile_channel(tiles*kInstrTile, -1);
        std::vector<InstrItem> items;
        for (size_t t = 0; t < tiles; ++t)
        {
            const size_t first = t*kInstrTile, last = std::min(order.size(), first + kInstrTile);
            const long long base = channel[order[first]].begin;
            long long union_end = base;
            for (size_t i = first; i < last; ++i) union_end = std::max(union_end, channel[order[i]].end);
            const long long n_segments = (union_end - base + kInstrSegment - 1)/kInstrSegment;
            std::vector<long long> item_of((size_t)n_segments, -1);
            for (long long s = 0; s < n_segments; ++s)
            {
                const long long b = base + s*kInstrSegment;
                const long long e = std::min(b + kInstrSegment, union_end);
                bool touched = false;
                for (size_t i = first; i < last && !touched; ++i)
                {
                    touched = channel[order[i]].begin < e && channel[order[i]].end > b;
                }
                if (!touched) continue;
                item_of[(size_t)s] = (long long)items.size();
                items.push_back(InstrItem{b, e, (long long)t});
            }
            for (size_t i = first; i < last; ++i)
            {
                InstrChannel & ch = channel[order[i]];
                tile_channel[i] = order[i];
                ch.slot = (int)(i - first);
                // Its segments are consecutive, each touched by it: consecutive items.
                ch.first_item = (int)item_of[(size_t)((ch.begin - base)/kInstrSegment)];
                ch.n_items = (int)((ch.end - 1 - base)/kInstrSegment - (ch.begin - base)/kInstrSegment + 1);
            }
        }
        if (items.size() > (size_t)std::numeric_limits<int32_t>::max()/kInstrTile)
        {
            return bad("too many channel segments.");
        }
        in->n_items = (int)items.size();

        // One block: channels, items, tile slots, offsets, response, grid.
        const size_t table_rows = shape == kInstrTabulated ? (size_t)response_rows : 0;
        const size_t at_item = words_of<InstrChannel>(channel.size());
        const size_t at_tile = at_item + words_of<InstrItem>(items.size());
        const size_t at_offsets = at_tile + tile_channel.size();
        const size_t at_response = at_offsets + (size_t)in->n_table;
        const size_t at_nu = at_response + table_rows*(size_t)in->n_table;
        const size_t total = at_nu + nu.size();
        std::vector<double> staged(total);
        std::memcpy(staged.data(), channel.data(), channel.size()*sizeof(InstrChannel));
        if (!items.empty())
        {
            std::memcpy(staged.data() + at_item, items.data(), items.size()*sizeof(InstrItem));
        }
        if (!tile_channel.empty())
        {
            std::memcpy(staged.data() + at_tile, tile_channel.data(), tile_channel.size()*8);
        }
        if (in->n_table > 0)
        {
            std::memcpy(staged.data() + at_offsets, offsets, (size_t)n_table*8);
            std::memcpy(staged.data() + at_response, response, table_rows*(size_t)n_table*8);
        }
        std::memcpy(staged.data() + at_nu, nu.data(), nu.size()*8);
        in->words.upload(staged.data(), total, engine->stream);
        HIP_TRY(hipStreamSynchronize(engine->stream));
        double * base = in->words.data;
        in->channel = reinterpret_cast<const InstrChannel *>(base);
        in->item = reinterpret_cast<const InstrItem *>(base + at_item);
        in->tile_channel = reinterpret_cast<const long long *>(base + at_tile);
        in->offsets = base + at_offsets;
        in->response = base + at_response;
        in->nu = base + at_nu;
        *handle = store_slot(engine->instruments, std::move(in));
        return LBL_OK;
    });
}

int lbl_instrument_free(lbl_engine * engine, int32_t handle)
{
    return free_slot(engine, &lbl_engine::instruments, handle,
                     "lbl_instrument_free: unknown instrument handle.");
}

int lbl_instrument_apply(lbl_engine * engine, const double * values, int64_t row_stride,
                         int32_t rows, int32_t handle, int32_t flags, double * out)
{
    return path_entry(engine, flags, [&] {
        auto bad = [&](const char * what) {
            return fail(engine, LBL_BAD_ARGUMENT, std::string("lbl_instrument_apply: ") + what);
        };
        const Instrument * in = find_slot(engine->instruments, handle);
        if (in == nullptr) return bad("unknown instrument handle.");
        if (values == nullptr || out == nullptr) return bad("values and out must not be NULL.");
        if (rows < 1) return bad("need rows >= 1.");
        if (row_stride < in->grid_points)
        {
            return bad("row_stride is shorter than the instrument's grid.");
        }
        if ((flags & ~(LBL_ASYNC | LBL_PATH_TRANSMITTANCE)) != 0) return bad("unknown flags.");

        HIP_TRY(hipSetDevice(engine->device));
        engine->finish_deferred();
        if (flags & LBL_ASYNC)
        {
            engine->join_lanes(engine->stream);
        }
        else
        {
            for (int i = 1; i < kAllLanes; ++i) engine->lanes[i].drain();
        }
        PathWorkspace & w = engine->path;
        hipStream_t stream = engine->stream;
        const long long slots = (long long)in->n_items*kInstrTile;
        // Rows go in chunks that share one block of partial sums: at most kPathGridY rows, and
        // no more than 2^24 partials (whole row groups) unless one group needs more.
        long long chunk = kPathGridY;
        if (slots > 0)
        {
            const long long fit = ((1ll << 24)/(slots + 1)/kInstrRowGroup)*kInstrRowGroup;
            chunk = std::min<long long>(chunk, std::max<long long>(fit, kInstrRowGroup));
        }
        chunk = std::min<long long>(chunk, rows);
        w.partial.reserve((size_t)(chunk*slots + slots + 1));

        InstrApply a;
        a.row_stride = row_stride;
        a.transmittance = (flags & LBL_PATH_TRANSMITTANCE) ? 1 : 0;
        a.nu = in->nu;
        a.channel = in->channel;
        a.item = in->item;
        a.tile_channel = in->tile_channel;
        a.n_items = in->n_items;
        a.n_channels = in->n_channels;
        a.shape = in->shape;
        a.n_table = in->n_table;
        a.offsets = in->offsets;
        a.response = in->response;
        a.weight_partial = w.partial.data;
        a.partial = w.partial.data + slots;
        for (long long r0 = 0; r0 < rows; r0 += chunk)
        {
            a.rows = (int)std::min<long long>(chunk, rows - r0);
            a.values = values + r0*row_stride;
            a.out = out + r0*in->n_channels;
            if (in->n_items > 0)
            {
                const dim3 grid((unsigned)in->n_items,
                                (unsigned)((a.rows + kInstrRowGroup - 1)/kInstrRowGroup));
                hipLaunchKernelGGL(instrument_partial_kernel, grid, dim3(kInstrThreads), 0,
                                   stream, a);
                HIP_TRY(hipGetLastError());
            }
            const dim3 grid((unsigned)((in->n_channels + kInstrThreads - 1)/kInstrThreads),
                            (unsigned)a.rows);
            hipLaunchKernelGGL(instrument_mean_kernel, grid, dim3(kInstrThreads), 0, stream, a);
            HIP_TRY(hipGetLastError());
        }
        engine->lanes[0].note_write(out, (long long)rows*in->n_channels*8, stream);
        return LBL_OK;
    });
}

}  // extern "C"
