// Host side of the cross-section entry points of include/lbl_amd.h (kernels: xsec.h).
// Included at the end of engine.hip after slot_entry.inc and continuum_entry.inc.

namespace {

void launch_xsec_model(lbl_engine * engine, XsecData & x, int n_levels, hipStream_t stream)
{
    engine->timed(kTimeXsecModel, stream, [&] {
        dim3 grid((unsigned)x.set.n_bands, (unsigned)n_levels);
        hipLaunchKernelGGL(xsec_model_kernel, grid, dim3(kModelThreads), 0, stream, x.set, x.fgrid.data,
                           x.coeffs.data, x.levels.data, x.values.data, x.slopes.data);
        HIP_TRY(hipGetLastError());
    });
}

}  // namespace

extern "C" {

int lbl_xsec_load(lbl_engine * engine, int32_t n_bands, const int32_t * sizes,
                  const double * frequency, const double * coefficients, int32_t * xsec)
{
    return entry(engine, [&] {
        if (xsec == nullptr || sizes == nullptr || frequency == nullptr ||
            coefficients == nullptr || n_bands < 1 || n_bands > kMaxXsecBands)
        {
            return fail(engine, LBL_BAD_ARGUMENT, "lbl_xsec_load: bad argument.");
        }
        HIP_TRY(hipSetDevice(engine->device));
        std::unique_ptr<XsecData> x(new XsecData());
        x->set.n_bands = n_bands;
        long long total = 0;
        for (int k = 0; k < n_bands; ++k)
        {
            if (sizes[k] < 2)
            {
                return fail(engine, LBL_BAD_ARGUMENT,
                            "band " + std::to_string(k) + ": fewer than two frequencies.");
            }
            const double * f = frequency + total;
            for (int j = 0; j + 1 < sizes[k]; ++j)
            {
                if (!(f[j] < f[j + 1]))
                {
                    return fail(engine, LBL_BAD_ARGUMENT,
                                "band " + std::to_string(k) +
                                ": frequencies must be strictly ascending.");
                }
            }
            x->set.band[k].size = sizes[k];
            x->set.band[k].offset = total;
            total += sizes[k];
        }
        if (total > 0x3fffffff) return fail(engine, LBL_BAD_ARGUMENT, "too many frequencies.");
        x->set.total = (int)total;
        x->fgrid.upload(frequency, (size_t)total, engine->stream);
        x->coeffs.upload(coefficients, (size_t)(4*total), engine->stream);
        HIP_TRY(hipStreamSynchronize(engine->stream));
        *xsec = store_slot(engine->xsecs, std::move(x));
        return LBL_OK;
    });
}

int lbl_xsec_free(lbl_engine * engine, int32_t xsec)
{
    return free_slot(engine, &lbl_engine::xsecs, xsec, "unknown cross-section handle.");
}

int lbl_xsec_compute(lbl_engine * engine, int32_t xsec, int32_t grid, int32_t n_levels,
                     const double * temperature, const double * pressure, const double * vmr,
                     int32_t flags, double * out, int64_t level_stride)
{
    return entry(engine, [&] {
        XsecData * x = find_slot(engine->xsecs, xsec);
        if (x == nullptr) return fail(engine, LBL_BAD_ARGUMENT, "unknown cross-section handle.");
        const bool scale = (flags & LBL_SCALE_DENSITY) != 0;
        SlotCall call{engine, n_levels, flags, out};
        const int status = call.check(
            grid, level_stride,
            n_levels < 0 || out == nullptr ||
            (n_levels > 0 && (temperature == nullptr || pressure == nullptr ||
                              (scale && vmr == nullptr))),
            "lbl_xsec_compute: bad argument.");
        if (status != LBL_OK || n_levels == 0) return status;
        const SpectralGrid * g = call.g;
        const long long n = call.n;
        return call.run(*x, x->values, x->set.total, kTimeXsec,
            [&](long long l) {
                // spectroscopy.py:18-29,199-203: n = P x /(kb T).
                const double t = temperature[l], p = pressure[l];
                return XsecLevel{t, p, scale ? p*vmr[l]/(kBoltzmann*t) : 1.};
            },
            [&](int count) { launch_xsec_model(engine, *x, count, call.stream); },
            [&](int count, double * target, long long target_stride, int add) {
                const int ascending = g->ascending ? 1 : 0;
                if (count == 1)
                {
                    dim3 blocks((unsigned)((n + 1023)/1024), 1u);
                    hipLaunchKernelGGL((xsec_interp_kernel<4, 1>), blocks, dim3(256), 0,
                                       call.stream, x->set, x->fgrid.data, x->values.data,
                                       x->slopes.data, x->levels.data, g->form(), n, count,
                                       ascending, target, target_stride, add);
                }
                else
                {
                    dim3 blocks((unsigned)((n + 511)/512), (unsigned)((count + 3)/4));
                    hipLaunchKernelGGL((xsec_interp_kernel<2, 4>), blocks, dim3(256), 0,
                                       call.stream, x->set, x->fgrid.data, x->values.data,
                                       x->slopes.data, x->levels.data, g->form(), n, count,
                                       ascending, target, target_stride, add);
                }
            });
    });
}

int lbl_xsec_bands(lbl_engine * engine, int32_t xsec, double temperature, double pressure,
                   double * values)
{
    return entry(engine, [&] {
        XsecData * x = find_slot(engine->xsecs, xsec);
        if (x == nullptr) return fail(engine, LBL_BAD_ARGUMENT, "unknown cross-section handle.");
        if (values == nullptr)
        {
            return fail(engine, LBL_BAD_ARGUMENT, "lbl_xsec_bands: bad argument.");
        }
        HIP_TRY(hipSetDevice(engine->device));
        hipStream_t stream = engine->stream;
        XsecLevel * staged = x->pinned.refill(1);
        staged[0] = XsecLevel{temperature, pressure, 1.};
        x->levels.reserve(1);
        x->values.reserve((size_t)x->set.total);
        x->slopes.reserve((size_t)x->set.total);
        // (no event behind this copy: the call waits for the stream below)
        HIP_TRY(hipMemcpyAsync(x->levels.data, staged, sizeof(XsecLevel),
                               hipMemcpyHostToDevice, stream));
        launch_xsec_model(engine, *x, 1, stream);
        HIP_TRY(hipMemcpyAsync(values, x->values.data, (size_t)x->set.total*8,
                               hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return LBL_OK;
    });
}

}  // extern "C"
