// lbl_path_jacobian: analytic radiance Jacobians along whole paths through a block of absorption
// coefficients in HBM (kernel: jacobian.h; band means: path.h).  Included by engine.hip after
// path_entry.inc, whose PathCall, PathTables and PathBands it shares.
extern "C" {

int lbl_path_jacobian(lbl_engine * engine, const double * beta, int64_t row_stride,
                      int64_t columns, int32_t grid, int32_t n_paths, int32_t levels_per_path,
                      int32_t level_begin, int32_t level_count, const double * path_length,
                      const double * temperature, const double * boundary_temperature,
                      const double * boundary_emissivity, int32_t n_bands,
                      const int64_t * band_start, double * work, double * radiance,
                      double * optical_depth_jacobian, double * log_optical_depth_jacobian,
                      double * temperature_jacobian, double * boundary_temperature_jacobian,
                      double * boundary_emissivity_jacobian, int32_t flags)
{
    return path_entry(engine, flags, [&] {
        PathCall call{engine, "lbl_path_jacobian", row_stride, columns, n_paths, levels_per_path,
                      level_begin, level_count, flags};
        // The quantities in the order of their flags: three per level, then three per path.
        constexpr int kQuantities = 6, kPerLevel = 3;
        const int32_t bit[kQuantities] = {
            LBL_PATH_JACOBIAN_DEPTH, LBL_PATH_JACOBIAN_LOG_DEPTH, LBL_PATH_JACOBIAN_TEMPERATURE,
            LBL_PATH_RADIANCE, LBL_PATH_JACOBIAN_BOUNDARY_T, LBL_PATH_JACOBIAN_BOUNDARY_E};
        double * const out[kQuantities] = {
            optical_depth_jacobian, log_optical_depth_jacobian, temperature_jacobian, radiance,
            boundary_temperature_jacobian, boundary_emissivity_jacobian};
        bool want[kQuantities];
        int per_level = 0, per_path = 0;
        for (int q = 0; q < kQuantities; ++q)
        {
            want[q] = (flags & bit[q]) != 0;
            (q < kPerLevel ? per_level : per_path) += want[q] ? 1 : 0;
        }
        if (beta == nullptr || path_length == nullptr || temperature == nullptr ||
            work == nullptr)
        {
            return call.bad("beta, path_length, temperature and work must not be NULL.");
        }
        if (per_level + per_path == 0) return call.bad("no quantity requested.");
        for (int q = 0; q < kQuantities; ++q)
        {
            if (want[q] && out[q] == nullptr)
            {
                return call.bad("an output requested by the flags is NULL.");
            }
        }
        if (flags & (LBL_PATH_CONTINUE | LBL_PATH_CUMULATIVE))
        {
            return call.bad("LBL_PATH_CONTINUE and LBL_PATH_CUMULATIVE must not be set: a call "
                            "takes whole paths and returns every level.");
        }
        if (levels_per_path >= 1 &&
            (level_begin % levels_per_path != 0 || level_count % levels_per_path != 0))
        {
            return call.bad("the run must consist of whole paths: level_begin and level_count "
                            "must be multiples of levels_per_path.");
        }
        if (const char * problem = call.find_grid(grid)) return call.bad(problem);
        if (const char * problem = call.check(path_length, 1)) return call.bad(problem);
        if (!finite_at_least_zero(temperature, level_count, true))
        {
            return call.bad("temperatures must be finite and > 0.");
        }
        const PathRun & run = call.run;
        for (int p = 0; p < n_paths; ++p)
        {
            if (const char * problem = check_boundary(boundary_temperature, boundary_emissivity, p))
            {
                return call.bad(problem);
            }
            const bool none = boundary_temperature == nullptr || boundary_temperature[p] == 0.;
            if (none && (want[4] || want[5]) && p >= run.first_path &&
                p < run.first_path + run.paths)
            {
                return call.bad("a boundary Jacobian is requested for a path without a boundary "
                                "(boundary temperature 0).");
            }
        }
        PathBands bands;
        if (const char * problem = bands.check(n_bands, band_start, columns))
        {
            return call.bad(problem);
        }
        // Without bands the kernel writes the outputs themselves; at most one of dI/dx and
        // dI/dln x may be W.  With bands it writes fine rows into `work`: the per-level
        // quantities into blocks of level_count rows (the first of them over W, in place), then
        // the per-path ones into blocks of run.paths rows, and the means read them.
        const bool fine = n_bands == 0;
        if (fine && work == optical_depth_jacobian && work == log_optical_depth_jacobian)
        {
            return call.bad("only one of the outputs may be the work block.");
        }
        if (fine && (work == temperature_jacobian || work == radiance ||
                     work == boundary_temperature_jacobian ||
                     work == boundary_emissivity_jacobian))
        {
            return call.bad("only dI/dx or dI/dln x may be written over the work block.");
        }

        PathTables tables;
        const size_t length_at = tables.add(level_count, path_length);
        const size_t temperature_at = tables.add(level_count, temperature);
        const size_t boundary_at =
            tables.add_pair(run, boundary_temperature, 0., boundary_emissivity, 1.);
        tables.add(bands, band_start);
        const double * d_tables = call.begin(tables);

        // Where the kernel writes quantity q: row 0 is flat level level_begin (per level) or
        // path 0 (per path).
        double * rows[kQuantities];
        {
            const long long level_block = (long long)level_count*row_stride;
            const long long path_block = (long long)run.paths*row_stride;
            double * next_level = work;
            double * next_path = work + std::max(per_level, 1)*level_block;
            for (int q = 0; q < kQuantities; ++q)
            {
                rows[q] = nullptr;
                if (!want[q]) continue;
                if (fine)
                {
                    rows[q] = out[q];
                }
                else if (q < kPerLevel)
                {
                    rows[q] = next_level;
                    next_level += level_block;
                }
                else
                {
                    rows[q] = next_path - (long long)run.first_path*row_stride;
                    next_path += path_block;
                }
            }
        }

        PathJacobian a;
        call.fill(a, beta, nullptr);
        a.nu = call.grid->wavenumber.data;
        a.length = d_tables + length_at;
        a.temperature = d_tables + temperature_at;
        a.boundary_t = d_tables + boundary_at;
        a.boundary_e = a.boundary_t + run.paths;
        a.table_path = run.first_path;
        a.work = work;
        a.d_depth = rows[0];
        a.d_log_depth = rows[1];
        a.d_temperature = rows[2];
        a.radiance = rows[3];
        a.d_boundary_t = rows[4];
        a.d_boundary_e = rows[5];
        const bool vector = path_vector(row_stride, {beta, a.nu, work, rows[0], rows[1], rows[2],
                                                     rows[3], rows[4], rows[5]});
        call.launch(a, [&](const dim3 & launch) {
            dispatch([&](auto v) {
                hipLaunchKernelGGL(path_jacobian_kernel<v.value>, launch, dim3(kPathThreads), 0,
                                   engine->stream, a);
            }, vector);
        });
        call.note_rows(beta, level_count);
        call.note_rows(work, level_count);
        for (int q = 0; q < kQuantities; ++q)
        {
            if (!want[q] || rows[q] == work) continue;
            if (q < kPerLevel)
            {
                call.note_rows(rows[q], level_count);
            }
            else
            {
                // Per path: the rows of the run's paths (all n_paths rows of a caller's output,
                // as lbl_path_radiance records them).
                call.note_rows(fine ? rows[q] : rows[q] + (long long)run.first_path*row_stride,
                               fine ? n_paths : run.paths);
            }
        }

        // The fine rows' means: per level every level of the run, per path its (whole) paths.
        for (int q = 0; q < kQuantities && !fine; ++q)
        {
            if (!want[q]) continue;
            call.means(bands, q < kPerLevel ? PathMeanRows::kLevels : PathMeanRows::kFinished,
                       rows[q], out[q]);
        }
        return LBL_OK;
    });
}

}  // extern "C"
