// lbl_path_radiance: thermal emission along paths through a block of absorption coefficients in
// HBM (kernel: radiance.h; band means: path.h).  Included by engine.hip after path_entry.inc,
// whose PathRun and PathBands it shares, and after continuum_entry.inc (grid handles).
extern "C" {

int lbl_path_radiance(lbl_engine * engine, double * beta, int64_t row_stride, int64_t columns,
                      int32_t grid, int32_t n_paths, int32_t levels_per_path, int32_t level_begin,
                      int32_t level_count, const double * path_length, const double * temperature,
                      const double * boundary_temperature, const double * boundary_emissivity,
                      int32_t n_bands, const int64_t * band_start, double * carry,
                      double * radiance, double * brightness_temperature, int32_t flags)
{
    if (engine == nullptr) return LBL_BAD_ARGUMENT;
    EngineLock lock(engine->mutex);
    auto bad = [&](const char * what) {
        return fail(engine, LBL_BAD_ARGUMENT, std::string("lbl_path_radiance: ") + what);
    };
    const bool want_rad = (flags & LBL_PATH_RADIANCE) != 0;
    const bool want_bt = (flags & LBL_PATH_BRIGHTNESS) != 0;
    const bool cumulative = (flags & LBL_PATH_CUMULATIVE) != 0;
    const bool from_last = (flags & LBL_PATH_FROM_LAST) != 0;
    if (beta == nullptr || path_length == nullptr || temperature == nullptr || carry == nullptr)
    {
        return bad("beta, path_length, temperature and carry must not be NULL.");
    }
    if (!want_rad && !want_bt) return bad("no quantity requested.");
    if ((want_rad && radiance == nullptr) || (want_bt && brightness_temperature == nullptr))
    {
        return bad("an output requested by the flags is NULL.");
    }
    if (want_bt && n_bands != 0) return bad("brightness temperature has no band means.");
    const SpectralGrid * g = find_slot(engine->grids, grid);
    if (g == nullptr) return bad("unknown grid handle.");
    if (columns < 1 || row_stride < columns) return bad("need 1 <= columns <= row_stride.");
    if (g->n < columns) return bad("the grid has fewer than `columns` points.");
    if (n_paths < 1 || levels_per_path < 1 ||
        (int64_t)n_paths*levels_per_path > (int64_t)std::numeric_limits<int32_t>::max())
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
    for (int i = 0; i < level_count; ++i)
    {
        if (!(path_length[i] >= 0.) || !std::isfinite(path_length[i]))
        {
            return bad("path lengths must be finite and >= 0.");
        }
        if (!(temperature[i] > 0.) || !std::isfinite(temperature[i]))
        {
            return bad("temperatures must be finite and > 0.");
        }
    }
    for (int p = 0; p < n_paths; ++p)
    {
        const double t = boundary_temperature != nullptr ? boundary_temperature[p] : 0.;
        const double e = boundary_emissivity != nullptr ? boundary_emissivity[p] : 1.;
        if (!(t >= 0.) || !std::isfinite(t))
        {
            return bad("boundary temperatures must be finite and >= 0 (0: no boundary).");
        }
        if (!(e >= 0. && e <= 1.)) return bad("boundary emissivities must lie in [0, 1].");
    }
    PathBands bands;
    if (const char * problem = bands.check(n_bands, band_start, columns)) return bad(problem);
    // Rows whose band means this call forms: every level of the run (cumulative) or the paths
    // the run finishes -- upward those whose last level (p + 1) L - 1 is in the run, downward
    // those whose first level p L is.
    int band_rows = 0, band_row0 = 0;
    if (n_bands > 0)
    {
        if (cumulative)
        {
            band_rows = level_count;
        }
        else if (from_last)
        {
            band_row0 = (level_begin + levels_per_path - 1)/levels_per_path;
            band_rows = std::max((level_end + levels_per_path - 1)/levels_per_path - band_row0, 0);
        }
        else
        {
            band_row0 = level_begin/levels_per_path;
            band_rows = std::max(level_end/levels_per_path - band_row0, 0);
        }
    }
    try
    {
        HIP_TRY(hipSetDevice(engine->device));
        PathWorkspace & w = engine->path;
        // The tables: lengths and temperatures [level_count] each, boundary temperatures and
        // emissivities of the run's paths [run.paths] each, then the bands' words.
        const size_t words = 2*(size_t)level_count + 2*(size_t)run.paths + bands.words();
        double * staged = w.stage(words);
        std::memcpy(staged, path_length, (size_t)level_count*8);
        std::memcpy(staged + level_count, temperature, (size_t)level_count*8);
        double * boundary = staged + 2*(size_t)level_count;
        for (int i = 0; i < run.paths; ++i)
        {
            const int p = run.first_path + i;
            boundary[i] = boundary_temperature != nullptr ? boundary_temperature[p] : 0.;
            boundary[run.paths + i] = boundary_emissivity != nullptr ? boundary_emissivity[p] : 1.;
        }
        bands.stage(reinterpret_cast<long long *>(boundary + 2*(size_t)run.paths), band_start);
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
        const long long * d_table =
            reinterpret_cast<const long long *>(d_words + 2*(size_t)level_count + 2*(size_t)run.paths);

        PathRadiance a;
        a.beta = beta;
        a.stride = row_stride;
        a.columns = columns;
        a.nu = g->wavenumber.data;
        a.length = d_words;
        a.temperature = d_words + level_count;
        a.boundary_t = d_words + 2*(size_t)level_count;
        a.boundary_e = a.boundary_t + run.paths;
        a.first = level_begin;
        a.count = level_count;
        a.row_base = level_begin;
        a.levels_per_path = levels_per_path;
        a.first_path = run.first_path;
        a.table_path = run.first_path;
        a.from_last = from_last ? 1 : 0;
        a.carry = carry;
        a.level_rad = a.level_bt = a.final_rad = a.final_bt = nullptr;
        a.keep_final = 0;
        if (cumulative && n_bands > 0)
        {
            a.level_rad = beta;         // in place: the band means read the rows back
        }
        else if (cumulative)
        {
            a.level_rad = want_rad ? radiance : nullptr;
            a.level_bt = want_bt ? brightness_temperature : nullptr;
        }
        else if (n_bands > 0)
        {
            a.keep_final = 1;
        }
        else
        {
            a.final_rad = want_rad ? radiance : nullptr;
            a.final_bt = want_bt ? brightness_temperature : nullptr;
        }
        const bool vector = row_stride % 2 == 0 && aligned16(beta) && aligned16(carry) &&
                            aligned16(a.nu) && aligned16(a.level_rad) && aligned16(a.level_bt) &&
                            aligned16(a.final_rad) && aligned16(a.final_bt);
        const long long per_block = (long long)kPathThreads*kPathWidth;
        // Paths go in the grid's y dimension, at most kPathGridY of them per launch.
        for (int y0 = 0; y0 < run.paths; y0 += kPathGridY)
        {
            a.first_path = run.first_path + y0;
            const dim3 launch((unsigned)((columns + per_block - 1)/per_block),
                              (unsigned)std::min(run.paths - y0, kPathGridY));
            if (vector)
            {
                hipLaunchKernelGGL(path_radiance_kernel<true>, launch, dim3(kPathThreads), 0,
                                   stream, a);
            }
            else
            {
                hipLaunchKernelGGL(path_radiance_kernel<false>, launch, dim3(kPathThreads), 0,
                                   stream, a);
            }
            HIP_TRY(hipGetLastError());
        }
        const long long last_row = (long long)(level_count - 1)*row_stride + columns;
        const long long path_rows = (long long)(n_paths - 1)*row_stride + columns;
        // The block counts as written even where it is only read (as in lbl_path_compute).
        engine->lanes[0].note_write(beta, last_row*8, stream);
        if (a.level_rad != nullptr && a.level_rad != beta)
        {
            engine->lanes[0].note_write(a.level_rad, last_row*8, stream);
        }
        if (a.level_bt != nullptr) engine->lanes[0].note_write(a.level_bt, last_row*8, stream);
        engine->lanes[0].note_write(carry, path_rows*8, stream);
        if (a.final_rad != nullptr) engine->lanes[0].note_write(a.final_rad, path_rows*8, stream);
        if (a.final_bt != nullptr) engine->lanes[0].note_write(a.final_bt, path_rows*8, stream);

        if (n_bands > 0 && band_rows > 0)
        {
            // Values: the run's rows of beta (cumulative, in place) or the finished paths' carry
            // rows; outputs [rows][n_bands] from the first row this call forms.
            const double * values = cumulative ? beta : carry + (long long)band_row0*row_stride;
            double * out = radiance + (cumulative ? 0 : (long long)band_row0*n_bands);
            bands.means(w, d_table, values, (long long)row_stride, band_rows, false, out, stream);
            engine->lanes[0].note_write(out, (long long)band_rows*n_bands*8, stream);
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
