// lbl_path_radiance_source: thermal emission along paths through a block of absorption
// coefficients in HBM (kernel: radiance.h; band means: path.h), and lbl_path_radiance, the same
// call without edge temperatures.  lbl_path_radiance_surface: the same call with the start value
// of a surface that has a spectral emissivity and/or reflects, and lbl_surface_emissivity, which
// fills the emissivity rows it reads (kernel: surface.h).  Included by engine.hip after
// path_entry.inc, whose PathCall, PathTables and PathBands it shares.
namespace {

// The three radiance entries: `name` is the entry's, emissivity_rows / reflection are
// lbl_path_radiance_surface's (device, both null for the others: their kernels and their bits).
int path_radiance_call(const char * name, lbl_engine * engine, double * beta, int64_t row_stride,
                       int64_t columns, int32_t grid, int32_t n_paths, int32_t levels_per_path,
                       int32_t level_begin, int32_t level_count, const double * path_length,
                       const double * temperature, const double * edge_temperature,
                       const double * boundary_temperature, const double * boundary_emissivity,
                       int32_t n_bands, const int64_t * band_start, double * carry,
                       double * radiance, double * brightness_temperature, int32_t flags,
                       const double * emissivity_rows, const double * reflection)
{
    return path_entry(engine, flags, [&] {
        PathCall call{engine, name, row_stride, columns, n_paths, levels_per_path,
                      level_begin, level_count, flags};
        const bool want_rad = (flags & LBL_PATH_RADIANCE) != 0;
        const bool want_bt = (flags & LBL_PATH_BRIGHTNESS) != 0;
        const bool cumulative = (flags & LBL_PATH_CUMULATIVE) != 0;
        if (beta == nullptr || path_length == nullptr || temperature == nullptr ||
            carry == nullptr)
        {
            return call.bad("beta, path_length, temperature and carry must not be NULL.");
        }
        if (!want_rad && !want_bt) return call.bad("no quantity requested.");
        if ((want_rad && radiance == nullptr) || (want_bt && brightness_temperature == nullptr))
        {
            return call.bad("an output requested by the flags is NULL.");
        }
        if (want_bt && n_bands != 0) return call.bad("brightness temperature has no band means.");
        if (const char * problem = call.find_grid(grid)) return call.bad(problem);
        if (const char * problem = call.check(path_length, 1)) return call.bad(problem);
        if (!finite_at_least_zero(temperature, level_count, true))
        {
            return call.bad("temperatures must be finite and > 0.");
        }
        if (const char * problem = check_edge_temperatures(edge_temperature, level_begin,
                                                           level_count, levels_per_path))
        {
            return call.bad(problem);
        }
        for (int p = 0; p < n_paths; ++p)
        {
            if (const char * problem = check_boundary(boundary_temperature, boundary_emissivity, p))
            {
                return call.bad(problem);
            }
        }
        PathBands bands;
        if (const char * problem = bands.check(n_bands, band_start, columns))
        {
            return call.bad(problem);
        }
        const bool surface = emissivity_rows != nullptr || reflection != nullptr;
        for (int i = 0; reflection != nullptr && i < call.run.paths; ++i)
        {
            const int p = call.run.first_path + i;
            if (boundary_temperature == nullptr || !(boundary_temperature[p] > 0.))
            {
                return call.bad("a reflecting surface needs a boundary temperature > 0 for "
                                "every path of the run.");
            }
        }

        // The boundary temperatures and emissivities of the run's paths.
        const PathRun & run = call.run;
        PathTables tables;
        const size_t length_at = tables.add(level_count, path_length);
        const size_t temperature_at = tables.add(level_count, temperature);
        const size_t boundary_at =
            tables.add_pair(run, boundary_temperature, 0., boundary_emissivity, 1.);
        tables.add(bands, band_start);
        // After the tables every call has, so that theirs lie where they always lay.
        const bool linear = edge_temperature != nullptr;
        const size_t edge_at = linear ? tables.add(2*(size_t)level_count, edge_temperature) : 0;
        const double * d_tables = call.begin(tables);

        // One set of arguments: the kernels without a surface take its PathRadiance part.
        PathSurface a;
        call.fill(a, beta, carry);
        a.nu = call.grid->wavenumber.data;
        a.length = d_tables + length_at;
        a.temperature = d_tables + temperature_at;
        a.boundary_t = d_tables + boundary_at;
        a.boundary_e = a.boundary_t + run.paths;
        a.edge = linear ? d_tables + edge_at : nullptr;
        a.table_path = run.first_path;
        const PathOutputs o(cumulative, n_bands > 0, beta, want_rad ? radiance : nullptr,
                            want_bt ? brightness_temperature : nullptr);
        a.level_rad = o.level[0];
        a.level_bt = o.level[1];
        a.final_rad = o.final[0];
        a.final_bt = o.final[1];
        a.keep_final = o.keep_final;
        a.emissivity_rows = emissivity_rows;
        a.reflection = reflection;
        const bool vector = path_vector(row_stride, {beta, carry, a.nu, a.level_rad, a.level_bt,
                                                     a.final_rad, a.final_bt, emissivity_rows,
                                                     reflection});
        call.launch(a, [&](const dim3 & launch) {
            dispatch([&](auto v, auto l) {
                const dim3 block(kPathThreads);
                if (surface)
                {
                    hipLaunchKernelGGL((path_radiance_surface_kernel<v.value, l.value>), launch,
                                       block, 0, engine->stream, a);
                }
                else
                {
                    hipLaunchKernelGGL((path_radiance_kernel<v.value, l.value>), launch, block, 0,
                                       engine->stream, static_cast<const PathRadiance &>(a));
                }
            }, vector, linear);
        });
        call.note_sweep(beta, carry, o);
        call.note_rows(emissivity_rows, n_paths);
        call.note_rows(reflection, n_paths);

        // Rows: every level of the run (cumulative, in place in beta) or the paths the run
        // finishes, from their carry rows.
        call.means(bands, cumulative ? PathMeanRows::kLevels : PathMeanRows::kFinished,
                   cumulative ? beta : carry, radiance);
        return LBL_OK;
    });
}

}  // namespace

extern "C" {

int lbl_path_radiance_source(lbl_engine * engine, double * beta, int64_t row_stride,
                             int64_t columns, int32_t grid, int32_t n_paths,
                             int32_t levels_per_path, int32_t level_begin, int32_t level_count,
                             const double * path_length, const double * temperature,
                             const double * edge_temperature,
                             const double * boundary_temperature,
                             const double * boundary_emissivity, int32_t n_bands,
                             const int64_t * band_start, double * carry, double * radiance,
                             double * brightness_temperature, int32_t flags)
{
    return path_radiance_call("lbl_path_radiance_source", engine, beta, row_stride, columns, grid,
                              n_paths, levels_per_path, level_begin, level_count, path_length,
                              temperature, edge_temperature, boundary_temperature,
                              boundary_emissivity, n_bands, band_start, carry, radiance,
                              brightness_temperature, flags, nullptr, nullptr);
}

int lbl_path_radiance_surface(lbl_engine * engine, double * beta, int64_t row_stride,
                              int64_t columns, int32_t grid, int32_t n_paths,
                              int32_t levels_per_path, int32_t level_begin, int32_t level_count,
                              const double * path_length, const double * temperature,
                              const double * edge_temperature,
                              const double * boundary_temperature,
                              const double * boundary_emissivity, int32_t n_bands,
                              const int64_t * band_start, double * carry, double * radiance,
                              double * brightness_temperature, int32_t flags,
                              const double * emissivity_rows, const double * reflection)
{
    return path_radiance_call("lbl_path_radiance_surface", engine, beta, row_stride, columns,
                              grid, n_paths, levels_per_path, level_begin, level_count,
                              path_length, temperature, edge_temperature, boundary_temperature,
                              boundary_emissivity, n_bands, band_start, carry, radiance,
                              brightness_temperature, flags, emissivity_rows, reflection);
}

int lbl_surface_emissivity(lbl_engine * engine, int32_t grid, int32_t n_paths, int32_t path_begin,
                           int32_t path_count, int32_t n_knots, const double * knot_wavenumber,
                           const double * knot_emissivity, double * rows, int64_t row_stride,
                           int32_t flags)
{
    return path_entry(engine, flags, [&] {
        // Paths stand where a sweep has its levels: one row per path, [path_begin, + path_count).
        PathCall call{engine, "lbl_surface_emissivity", row_stride, 0, n_paths, 1, path_begin,
                      path_count, flags};
        if (knot_wavenumber == nullptr || knot_emissivity == nullptr || rows == nullptr)
        {
            return call.bad("knot_wavenumber, knot_emissivity and rows must not be NULL.");
        }
        if (const char * problem = call.find_grid(grid)) return call.bad(problem);
        call.columns = call.grid->n;
        if (call.columns < 1 || row_stride < call.columns)
        {
            return call.bad("row_stride is less than the grid's points.");
        }
        if (n_paths < 1 || path_begin < 0 || path_count < 1 || path_count > n_paths - path_begin)
        {
            return call.bad("the paths [path_begin, path_begin + path_count) are not inside "
                            "n_paths.");
        }
        if (n_knots < 2 || n_knots > kSurfaceMaxKnots)
        {
            return call.bad("n_knots must lie in 2..1024.");
        }
        if (const char * problem = check_knots(knot_wavenumber, n_knots)) return call.bad(problem);
        const long long values = (long long)path_count*n_knots;
        for (long long i = 0; i < values; ++i)
        {
            if (!(knot_emissivity[i] >= 0. && knot_emissivity[i] <= 1.))
            {
                return call.bad("emissivities must lie in [0, 1].");
            }
        }
        call.run = PathRun{path_begin, path_count, false};

        PathTables tables;
        const size_t knot_at = tables.add(n_knots, knot_wavenumber);
        const size_t value_at = tables.add((size_t)values, knot_emissivity);
        const double * d_tables = call.begin(tables);

        SurfaceEmissivity a;
        a.nu = call.grid->wavenumber.data;
        a.columns = call.columns;
        a.stride = row_stride;
        a.knot = d_tables + knot_at;
        a.n_knots = n_knots;
        a.ascending = call.grid->ascending ? 1 : 0;
        const bool vector = path_vector(row_stride, {rows, a.nu});
        call.launch([&](const dim3 & launch, int first_path) {
            a.value = d_tables + value_at + (long long)(first_path - path_begin)*n_knots;
            a.rows = rows + (long long)first_path*row_stride;
            dispatch([&](auto v) {
                hipLaunchKernelGGL(surface_emissivity_kernel<v.value>, launch, dim3(kPathThreads),
                                   0, engine->stream, a);
            }, vector);
        });
        call.note_rows(rows + (long long)path_begin*row_stride, path_count);
        return LBL_OK;
    });
}

int lbl_path_radiance(lbl_engine * engine, double * beta, int64_t row_stride, int64_t columns,
                      int32_t grid, int32_t n_paths, int32_t levels_per_path, int32_t level_begin,
                      int32_t level_count, const double * path_length, const double * temperature,
                      const double * boundary_temperature, const double * boundary_emissivity,
                      int32_t n_bands, const int64_t * band_start, double * carry,
                      double * radiance, double * brightness_temperature, int32_t flags)
{
    return lbl_path_radiance_source(engine, beta, row_stride, columns, grid, n_paths,
                                    levels_per_path, level_begin, level_count, path_length,
                                    temperature, nullptr, boundary_temperature,
                                    boundary_emissivity, n_bands, band_start, carry, radiance,
                                    brightness_temperature, flags);
}

}  // extern "C"
