// lbl_solar_spectrum: the solar irradiance on the grid, from a blackbody, from values on the grid
// or from a table of knots; lbl_path_solar: the direct beam at every interface and the sunlight a
// Lambertian surface reflects to a viewer, one sweep through a block of absorption coefficients in
// HBM (kernels: solar.h; band means: path.h).  Included by engine.hip after flux_entry.inc; shares
// path_entry.inc's PathCall, PathTables and PathBands.
extern "C" {

int lbl_solar_spectrum(lbl_engine * engine, int32_t grid, int64_t columns, int32_t n_knots,
                       const double * knot_wavenumber, const double * knot_irradiance,
                       double temperature, double scale, double * row, int32_t flags)
{
    return path_entry(engine, flags, [&] {
        PathCall call{engine, "lbl_solar_spectrum", columns, columns, 1, 1, 0, 1, flags};
        if (row == nullptr) return call.bad("row must not be NULL.");
        if (const char * problem = call.find_grid(grid)) return call.bad(problem);
        if (columns < 1 || columns > call.grid->n)
        {
            return call.bad("need 1 <= columns <= the grid's points.");
        }
        if (!(scale > 0.) || !std::isfinite(scale)) return call.bad("scale must be finite and > 0.");
        int mode = kSolarBlackbody;
        if (n_knots == 0)
        {
            if (!(temperature > 0.) || !std::isfinite(temperature))
            {
                return call.bad("the temperature must be finite and > 0.");
            }
        }
        else
        {
            mode = knot_wavenumber == nullptr ? kSolarOnGrid : kSolarTable;
            if (knot_irradiance == nullptr) return call.bad("knot_irradiance must not be NULL.");
            if (mode == kSolarOnGrid && n_knots != columns)
            {
                return call.bad("without knot_wavenumber n_knots must equal columns.");
            }
            if (mode == kSolarTable && (n_knots < 2 || n_knots > kSolarMaxKnots))
            {
                return call.bad("n_knots must lie in 2..4194304.");
            }
            if (const char * problem =
                    mode == kSolarTable ? check_knots(knot_wavenumber, n_knots) : nullptr)
            {
                return call.bad(problem);
            }
            if (!finite_at_least_zero(knot_irradiance, n_knots, false))
            {
                return call.bad("irradiances must be finite and >= 0.");
            }
        }

        PathTables tables;
        const size_t knot_at = mode == kSolarTable ? tables.add(n_knots, knot_wavenumber) : 0;
        const size_t value_at = mode != kSolarBlackbody ? tables.add(n_knots, knot_irradiance) : 0;
        tables.add(1);                              // (never an empty copy)
        const double * d_tables = call.begin(tables);

        SolarSpectrum a;
        a.nu = call.grid->wavenumber.data;
        a.columns = columns;
        a.mode = mode;
        a.knot = d_tables + knot_at;
        a.value = d_tables + value_at;
        a.n_knots = n_knots;
        a.ascending = call.grid->ascending ? 1 : 0;
        a.temperature = temperature;
        a.scale = scale;
        a.row = row;
        const long long per_block = (long long)kPathThreads*kPathWidth;
        const dim3 launch((unsigned)((columns + per_block - 1)/per_block));
        dispatch([&](auto v) {
            hipLaunchKernelGGL(solar_spectrum_kernel<v.value>, launch, dim3(kPathThreads), 0,
                               engine->stream, a);
        }, path_vector(0, {row, a.nu}));
        HIP_TRY(hipGetLastError());
        call.note_rows(row, 1);
        return LBL_OK;
    });
}

int lbl_path_solar(lbl_engine * engine, double * beta, int64_t row_stride, int64_t columns,
                   int32_t n_paths, int32_t levels_per_path, int32_t level_begin,
                   int32_t level_count, const double * solar_length, const double * view_length,
                   const double * solar_zenith_cosine, const double * solar_row,
                   const double * albedo_rows, const double * albedo, int32_t n_bands,
                   const int64_t * band_start, double * carry, double * interface_rows,
                   double * space_rows, double * surface_rows, double * reflected_rows,
                   double * interface_mean, double * space_mean, double * surface_mean,
                   double * reflected_mean, int32_t flags)
{
    return path_entry(engine, flags, [&] {
        PathCall call{engine, "lbl_path_solar", row_stride, columns, n_paths, levels_per_path,
                      level_begin, level_count, flags};
        const bool view = view_length != nullptr;
        if (beta == nullptr || solar_length == nullptr || solar_zenith_cosine == nullptr ||
            solar_row == nullptr || carry == nullptr)
        {
            return call.bad("beta, solar_length, solar_zenith_cosine, solar_row and carry must "
                            "not be NULL.");
        }
        if (view && (albedo_rows == nullptr) == (albedo == nullptr))
        {
            return call.bad("a view needs an albedo: albedo_rows or albedo, not both.");
        }
        if (!view && (albedo_rows != nullptr || albedo != nullptr))
        {
            return call.bad("an albedo is only used with view_length.");
        }
        if (view != (reflected_rows != nullptr))
        {
            return call.bad("reflected_rows goes with view_length: both or neither.");
        }
        if (interface_rows == nullptr && space_rows == nullptr && surface_rows == nullptr &&
            reflected_rows == nullptr)
        {
            return call.bad("no output requested.");
        }
        if (interface_rows == beta) return call.bad("interface_rows must not be beta.");
        if (const char * problem = call.check(solar_length, 1)) return call.bad(problem);
        if (view && !finite_at_least_zero(view_length, level_count, false))
        {
            return call.bad("view lengths must be finite and >= 0.");
        }
        for (int p = 0; p < n_paths; ++p)
        {
            const double mu0 = solar_zenith_cosine[p];
            if (!(mu0 > 0. && mu0 <= 1.)) return call.bad("solar zenith cosines must lie in (0, 1].");
            if (albedo != nullptr && !(albedo[p] >= 0. && albedo[p] <= 1.))
            {
                return call.bad("albedos must lie in [0, 1].");
            }
        }
        PathBands bands;
        if (const char * problem = bands.check(n_bands, band_start, columns))
        {
            return call.bad(problem);
        }
        if ((interface_mean != nullptr && interface_rows == nullptr) ||
            (space_mean != nullptr && space_rows == nullptr) ||
            (surface_mean != nullptr && surface_rows == nullptr) ||
            (reflected_mean != nullptr && reflected_rows == nullptr))
        {
            return call.bad("a band mean needs the rows it is the mean of.");
        }
        if (n_bands == 0 && (interface_mean != nullptr || space_mean != nullptr ||
                             surface_mean != nullptr || reflected_mean != nullptr))
        {
            return call.bad("band means need n_bands > 0.");
        }

        // mu0 and the scalar albedo of the run's paths.
        const PathRun & run = call.run;
        PathTables tables;
        const size_t length_at = tables.add(level_count, solar_length);
        const size_t view_at = tables.add(level_count, view ? view_length : nullptr);
        const size_t mu0_at = tables.add(run.paths, solar_zenith_cosine + run.first_path);
        const size_t albedo_at =
            tables.add(run.paths, albedo != nullptr ? albedo + run.first_path : nullptr);
        tables.add(bands, band_start);
        const double * d_tables = call.begin(tables);

        PathSolar a;
        call.fill(a, beta, carry);
        a.length = d_tables + length_at;
        a.view = d_tables + view_at;
        a.mu0 = d_tables + mu0_at;
        a.albedo = d_tables + albedo_at;
        a.table_path = run.first_path;
        a.solar = solar_row;
        a.albedo_rows = albedo_rows;
        a.level_flux = interface_rows;
        a.space = space_rows;
        a.surface = surface_rows;
        a.reflected = reflected_rows;
        const bool vector = path_vector(row_stride, {beta, carry, solar_row, albedo_rows,
                                                     interface_rows, space_rows, surface_rows,
                                                     reflected_rows});
        call.launch(a, [&](const dim3 & launch) {
            dispatch([&](auto v, auto w) {
                hipLaunchKernelGGL((path_solar_kernel<v.value, w.value>), launch,
                                   dim3(kPathThreads), 0, engine->stream, a);
            }, vector, view);
        });
        call.note_rows(beta, level_count);
        call.note_rows(interface_rows, level_count);
        call.note_rows(carry, 2*(long long)n_paths);
        call.note_rows(space_rows, n_paths);
        call.note_rows(surface_rows, n_paths);
        call.note_rows(reflected_rows, n_paths);

        // Every interface of the run; the top rows of the paths the run starts; the surface rows
        // of the paths it finishes.
        call.means(bands, PathMeanRows::kLevels, interface_rows, interface_mean);
        call.means(bands, PathMeanRows::kStarted, space_rows, space_mean);
        call.means(bands, PathMeanRows::kFinished, surface_rows, surface_mean);
        call.means(bands, PathMeanRows::kFinished, reflected_rows, reflected_mean);
        return LBL_OK;
    });
}

}  // extern "C"
