// lbl_path_flux: one sweep (down from space or up from the surface) of K angles through a block
// of absorption coefficients in HBM (kernel: flux.h; band means: path.h).  Included by engine.hip
// after radiance_entry.inc; shares path_entry.inc's PathRun and PathBands.
namespace {

template <bool kVector, int K>
void launch_flux(const PathFlux & a, const dim3 & grid, hipStream_t stream)
{
    hipLaunchKernelGGL((path_flux_kernel<kVector, K>), grid, dim3(kPathThreads), 0, stream, a);
}

template <bool kVector>
void launch_flux(int angles, const PathFlux & a, const dim3 & grid, hipStream_t stream)
{
    switch (angles)
    {
    case 1: launch_flux<kVector, 1>(a, grid, stream); break;
    case 2: launch_flux<kVector, 2>(a, grid, stream); break;
    case 3: launch_flux<kVector, 3>(a, grid, stream); break;
    case 4: launch_flux<kVector, 4>(a, grid, stream); break;
    case 5: launch_flux<kVector, 5>(a, grid, stream); break;
    case 6: launch_flux<kVector, 6>(a, grid, stream); break;
    case 7: launch_flux<kVector, 7>(a, grid, stream); break;
    default: launch_flux<kVector, 8>(a, grid, stream); break;
    }
}

}  // namespace

extern "C" {

int lbl_path_flux(lbl_engine * engine, double * beta, int64_t row_stride, int64_t columns,
                  int32_t grid, int32_t n_paths, int32_t levels_per_path, int32_t level_begin,
                  int32_t level_count, int32_t n_angles, const double * path_length,
                  const double * weight, const double * temperature,
                  const double * surface_temperature, const double * surface_emissivity,
                  int32_t n_bands, const int64_t * band_start, double * carry,
                  double * reflection, double * level_flux, double * flux, double * surface_flux,
                  int32_t flags)
{
    if (engine == nullptr) return LBL_BAD_ARGUMENT;
    EngineLock lock(engine->mutex);
    auto bad = [&](const char * what) {
        return fail(engine, LBL_BAD_ARGUMENT, std::string("lbl_path_flux: ") + what);
    };
    const bool up = (flags & LBL_PATH_FLUX_UP) != 0;
    const bool from_last = (flags & LBL_PATH_FROM_LAST) != 0;
    if (beta == nullptr || path_length == nullptr || weight == nullptr ||
        temperature == nullptr || carry == nullptr || reflection == nullptr ||
        level_flux == nullptr)
    {
        return bad("beta, path_length, weight, temperature, carry, reflection and level_flux "
                   "must not be NULL.");
    }
    if (level_flux == beta) return bad("level_flux must not be beta: the up sweep reads it.");
    if (up && (surface_temperature == nullptr || surface_emissivity == nullptr))
    {
        return bad("the up sweep needs surface_temperature and surface_emissivity.");
    }
    if (n_angles < 1 || n_angles > kFluxMaxAngles) return bad("need 1 <= n_angles <= 8.");
    const SpectralGrid * g = find_slot(engine->grids, grid);
    if (g == nullptr) return bad("unknown grid handle.");
    if (columns < 1 || row_stride < columns) return bad("need 1 <= columns <= row_stride.");
    if (g->n < columns) return bad("the grid has fewer than `columns` points.");
    if (n_paths < 1 || levels_per_path < 1 ||
        (int64_t)n_paths*levels_per_path > (int64_t)std::numeric_limits<int32_t>::max() ||
        (int64_t)n_paths*n_angles > (int64_t)std::numeric_limits<int32_t>::max())
    {
        return bad("need n_paths >= 1 and levels_per_path >= 1.");
    }
    const int levels = n_paths*levels_per_path;
    if (level_begin < 0 || level_count < 1 || level_count > levels - level_begin)
    {
        return bad("the run [level_begin, level_begin + level_count) is not inside the levels.");
    }
    const int level_end = level_begin + level_count;
    const PathRun run = path_run(level_begin, level_end, levels_per_path, from_last);
    if (run.continues != ((flags & LBL_PATH_CONTINUE) != 0))
    {
        return bad(run.continues ? "the run starts inside a path: LBL_PATH_CONTINUE is needed."
                                 : "the run starts a path: LBL_PATH_CONTINUE must not be set.");
    }
    for (int i = 0; i < level_count*n_angles; ++i)
    {
        if (!(path_length[i] >= 0.) || !std::isfinite(path_length[i]))
        {
            return bad("path lengths must be finite and >= 0.");
        }
    }
    for (int k = 0; k < n_angles; ++k)
    {
        if (!(weight[k] >= 0.) || !std::isfinite(weight[k]))
        {
            return bad("weights must be finite and >= 0.");
        }
    }
    for (int i = 0; i < level_count; ++i)
    {
        if (!(temperature[i] > 0.) || !std::isfinite(temperature[i]))
        {
            return bad("temperatures must be finite and > 0.");
        }
    }
    if (up)
    {
        for (int p = 0; p < n_paths; ++p)
        {
            if (!(surface_temperature[p] > 0.) || !std::isfinite(surface_temperature[p]))
            {
                return bad("surface temperatures must be finite and > 0.");
            }
            if (!(surface_emissivity[p] >= 0. && surface_emissivity[p] <= 1.))
            {
                return bad("surface emissivities must lie in [0, 1].");
            }
        }
    }
    PathBands bands;
    if (const char * problem = bands.check(n_bands, band_start, columns)) return bad(problem);
    if (n_bands > 0 && (flux == nullptr || (up && surface_flux == nullptr)))
    {
        return bad("band means need flux (and surface_flux on the up sweep).");
    }
    // Paths the run starts in sweep order: upward those whose first level p L is in the run,
    // downward those whose last level (p + 1) L - 1 is.  The up sweep writes their
    // surface-interface flux.
    int start_row0 = 0, start_rows = 0;
    if (up)
    {
        if (from_last)
        {
            start_row0 = level_begin/levels_per_path;
            start_rows = std::max(level_end/levels_per_path - start_row0, 0);
        }
        else
        {
            start_row0 = (level_begin + levels_per_path - 1)/levels_per_path;
            start_rows = std::max((level_end + levels_per_path - 1)/levels_per_path - start_row0,
                                  0);
        }
    }
    try
    {
        HIP_TRY(hipSetDevice(engine->device));
        PathWorkspace & w = engine->path;
        // The tables: lengths [level_count][n_angles], weights [n_angles], temperatures
        // [level_count], surface temperatures and emissivities of the run's paths [run.paths]
        // each, then the bands' words.
        const size_t length_words = (size_t)level_count*n_angles;
        const size_t words = length_words + n_angles + level_count + 2*(size_t)run.paths +
                             bands.words();
        double * staged = w.stage(words);
        std::memcpy(staged, path_length, length_words*8);
        std::memcpy(staged + length_words, weight, (size_t)n_angles*8);
        std::memcpy(staged + length_words + n_angles, temperature, (size_t)level_count*8);
        double * surface = staged + length_words + n_angles + level_count;
        for (int i = 0; i < run.paths; ++i)
        {
            const int p = run.first_path + i;
            surface[i] = up ? surface_temperature[p] : 0.;
            surface[run.paths + i] = up ? surface_emissivity[p] : 0.;
        }
        bands.stage(reinterpret_cast<long long *>(surface + 2*(size_t)run.paths), band_start);
        hipStream_t stream = engine->stream;
        // Ordered as lbl_path_compute orders its sweep.
        engine->finish_deferred();
        if (flags & LBL_ASYNC)
        {
            engine->join_lanes(stream);
        }
        else
        {
            for (int i = 1; i < kAllLanes; ++i) engine->lanes[i].drain();
        }
        w.upload(words, stream);
        const double * d_words = w.tables.data;
        const long long * d_table = reinterpret_cast<const long long *>(
            d_words + length_words + n_angles + level_count + 2*(size_t)run.paths);

        PathFlux a;
        a.beta = beta;
        a.stride = row_stride;
        a.columns = columns;
        a.nu = g->wavenumber.data;
        a.length = d_words;
        a.weight = d_words + length_words;
        a.temperature = a.weight + n_angles;
        a.surface_t = a.temperature + level_count;
        a.surface_e = a.surface_t + run.paths;
        a.first = level_begin;
        a.count = level_count;
        a.row_base = level_begin;
        a.levels_per_path = levels_per_path;
        a.first_path = run.first_path;
        a.table_path = run.first_path;
        a.from_last = from_last ? 1 : 0;
        a.up = up ? 1 : 0;
        a.carry = carry;
        a.reflection = reflection;
        a.level_flux = level_flux;
        const bool vector = row_stride % 2 == 0 && aligned16(beta) && aligned16(carry) &&
                            aligned16(a.nu) && aligned16(reflection) && aligned16(level_flux);
        const long long per_block = (long long)kPathThreads*kPathWidth;
        // Paths go in the grid's y dimension, at most kPathGridY of them per launch.
        for (int y0 = 0; y0 < run.paths; y0 += kPathGridY)
        {
            a.first_path = run.first_path + y0;
            const dim3 launch((unsigned)((columns + per_block - 1)/per_block),
                              (unsigned)std::min(run.paths - y0, kPathGridY));
            if (vector)
            {
                launch_flux<true>(n_angles, a, launch, stream);
            }
            else
            {
                launch_flux<false>(n_angles, a, launch, stream);
            }
            HIP_TRY(hipGetLastError());
        }
        const long long last_row = (long long)(level_count - 1)*row_stride + columns;
        const long long path_rows = (long long)(n_paths - 1)*row_stride + columns;
        // The block counts as written even where it is only read (as in lbl_path_compute).
        engine->lanes[0].note_write(beta, last_row*8, stream);
        engine->lanes[0].note_write(level_flux, last_row*8, stream);
        engine->lanes[0].note_write(
            carry, ((long long)n_paths*n_angles - 1)*row_stride*8 + columns*8, stream);
        engine->lanes[0].note_write(reflection, path_rows*8, stream);

        if (n_bands > 0)
        {
            bands.means(w, d_table, level_flux, (long long)row_stride, level_count, false, flux,
                        stream);
            engine->lanes[0].note_write(flux, (long long)level_count*n_bands*8, stream);
            if (start_rows > 0)
            {
                // The surface-interface rows of the paths this run starts.
                double * out = surface_flux + (long long)start_row0*n_bands;
                bands.means(w, d_table, reflection + (long long)start_row0*row_stride,
                            (long long)row_stride, start_rows, false, out, stream);
                engine->lanes[0].note_write(out, (long long)start_rows*n_bands*8, stream);
            }
        }
        if (!(flags & LBL_ASYNC)) HIP_TRY(hipStreamSynchronize(stream));
    }
    catch (const HipFailure & f)
    {
        return fail(engine, LBL_ERROR, f.message);
    }
    return LBL_OK;
}

}  // extern "C"
