// Micro-benchmark of the far-wing loop body of accumulate_kernel<4> on gfx950: eight lines per
// reciprocal (lorentz_eight, K = 1) against the running merge of K = 2, 4 and 8 batches of eight
// (fast_ranges), P = 4 points per lane, records by scalar loads, 7 waves per SIMD on every SIMD
// of the chip.  Reports evals/s and the largest relative error against IEEE division.  Not part
// of the product.
//
//   hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -std=c++17 \
//         -I pylbl_amd/csrc scripts/ubench/ubench_wing_batches.hip -o /tmp/ubench_wing
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "voigt_profile.h"

#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { \
    printf("HIP error %s at %s:%d\n", hipGetErrorString(e), __FILE__, __LINE__); exit(1); } } while (0)

using lbl::WingTerm;

constexpr int P = 4;
constexpr int kLines = 4096;            // multiple of 64 (= 8 K for every K)
constexpr int kBlocks = 256*7;          // 256 CUs x 4 SIMDs x 7 waves, 4 waves per block
constexpr long kPoints = (long)kBlocks*256*P;

struct Rec { double centre, g2, bl, pad; };

template <int K>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(7)))
void wing_loop(const Rec * __restrict__ lines, double v0, double dv, double * __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const long wave = ((long)blockIdx.x*blockDim.x + threadIdx.x) >> 6;
    const long base = wave*64*P;
    double v[P], acc[P];
#pragma unroll
    for (int p = 0; p < P; ++p)
    {
        v[p] = v0 + (double)(base + p*64 + lane)*dv;
        acc[p] = 0.;
    }
    auto load = [&](int o, WingTerm (&l)[8]) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
        {
            const Rec r = lines[8*o + i];
            l[i] = WingTerm{r.centre, r.g2, r.bl};
        }
    };
    const int eights = kLines/8;
    for (int o = 0; o < eights; )
    {
        if (K == 1)
        {
            WingTerm l[8];
            load(o, l);
#pragma unroll
            for (int p = 0; p < P; ++p) acc[p] = lbl::lorentz_eight(v[p], l, acc[p]);
            ++o;
            continue;
        }
        const int stop = o + K;
        double num[P], den[P];
        {
            WingTerm l[8];
            load(o, l);
#pragma unroll
            for (int p = 0; p < P; ++p) lbl::wing_eight(v[p], l, num[p], den[p]);
        }
        for (++o; o < stop; ++o)
        {
            WingTerm l[8];
            load(o, l);
#pragma unroll
            for (int p = 0; p < P; ++p)
            {
                double n, t;
                lbl::wing_eight(v[p], l, n, t);
                num[p] = __builtin_fma(num[p], t, n*den[p]);
                den[p] = den[p]*t;
            }
        }
#pragma unroll
        for (int p = 0; p < P; ++p) acc[p] = __builtin_fma(num[p], lbl::rcp_newton(den[p]), acc[p]);
    }
#pragma unroll
    for (int p = 0; p < P; ++p) out[base + p*64 + lane] = acc[p];
}

__global__ void wing_divide(const Rec * __restrict__ lines, double v0, double dv,
                            double * __restrict__ out)
{
    const long i = (long)blockIdx.x*blockDim.x + threadIdx.x;
    if (i >= kPoints) return;
    const double v = v0 + (double)i*dv;
    double acc = 0.;
    for (int j = 0; j < kLines; ++j)
    {
        const double d = v - lines[j].centre;
        acc += lines[j].bl/(d*d + lines[j].g2);
    }
    out[i] = acc;
}

template <int K>
void run(const Rec * lines, double v0, double dv, double * out, const std::vector<double> & ref)
{
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a));
    CHECK(hipEventCreate(&b));
    hipLaunchKernelGGL(wing_loop<K>, dim3(kBlocks), dim3(256), 0, 0, lines, v0, dv, out);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    float best = 1.e30f;
    for (int rep = 0; rep < 10; ++rep)
    {
        CHECK(hipEventRecord(a));
        hipLaunchKernelGGL(wing_loop<K>, dim3(kBlocks), dim3(256), 0, 0, lines, v0, dv, out);
        CHECK(hipEventRecord(b));
        CHECK(hipEventSynchronize(b));
        float ms = 0.f;
        CHECK(hipEventElapsedTime(&ms, a, b));
        best = ms < best ? ms : best;
    }
    std::vector<double> got(kPoints);
    CHECK(hipMemcpy(got.data(), out, kPoints*sizeof(double), hipMemcpyDeviceToHost));
    double worst = 0.;
    for (long i = 0; i < kPoints; ++i) worst = fmax(worst, fabs(got[i] - ref[i])/fabs(ref[i]));
    const double evals = (double)kPoints*kLines;
    printf("K=%d (%2d lines per reciprocal)  %.4f ms  %.4e evals/s  max rel err %.3e\n",
           K, 8*K, best, evals/(best*1.e-3), worst);
    CHECK(hipEventDestroy(a));
    CHECK(hipEventDestroy(b));
}

int main()
{
    // Lines of the far-wing loop of the default workload: centres 0.2 ... 25 cm-1 from the points
    // on either side, Lorentz widths of tropospheric pressure, strengths over 11 decades.
    std::vector<Rec> lines(kLines);
    srand(7);
    const double v0 = 1000., dv = 1.e-3 * 10./(double)kPoints;   // all points within 0.01 cm-1
    for (int j = 0; j < kLines; ++j)
    {
        const double u = (double)rand()/RAND_MAX;
        const double side = (j & 1) ? 1. : -1.;
        const double gamma = 0.03 + 0.09*(double)rand()/RAND_MAX;
        const double strength = pow(10., -30. + 11.*(double)rand()/RAND_MAX);
        lines[j] = Rec{v0 + side*(0.2 + 24.8*u), gamma*gamma, strength*gamma/M_PI, 0.};
    }
    Rec * d_lines = nullptr;
    double * d_out = nullptr;
    CHECK(hipMalloc(&d_lines, kLines*sizeof(Rec)));
    CHECK(hipMalloc(&d_out, kPoints*sizeof(double)));
    CHECK(hipMemcpy(d_lines, lines.data(), kLines*sizeof(Rec), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(wing_divide, dim3((unsigned)((kPoints + 255)/256)), dim3(256), 0, 0,
                       d_lines, v0, dv, d_out);
    CHECK(hipGetLastError());
    std::vector<double> ref(kPoints);
    CHECK(hipMemcpy(ref.data(), d_out, kPoints*sizeof(double), hipMemcpyDeviceToHost));
    printf("%ld points x %d lines, P = %d, %d workgroups of 256\n", kPoints, kLines, P, kBlocks);
    // (the first pass warms the clocks up; three interleaved rounds follow)
    for (int round = 0; round < 4; ++round)
    {
        printf(round == 0 ? "warm-up\n" : "round %d\n", round);
        run<1>(d_lines, v0, dv, d_out, ref);
        run<2>(d_lines, v0, dv, d_out, ref);
        run<4>(d_lines, v0, dv, d_out, ref);
        run<8>(d_lines, v0, dv, d_out, ref);
    }
    CHECK(hipFree(d_lines));
    CHECK(hipFree(d_out));
    return 0;
}
