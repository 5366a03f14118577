// measure.hip -- the two mappings of the policy rollout side by side (profiles/policy_rollout/README.md), as a small shared library
// that measure.py loads beside libsddp_hip.so:
//   wave: sddp::policy_rollout_kernel<Srbd13>, the library's kernel (one wavefront per instance), instantiated here from the same header;
//   lane: one lane per instance, the mapping of model_step_kernel -- the candidate that was dropped.  It lives here only.
// Both run on the buffers of a solved handle (sddp_device_ptr), timed with HIP events on the null stream.
#include <hip/hip_runtime.h>

#include "sddp_kernels.hpp"
#include "sddp_models.hpp"

namespace {
using M = sddp::Srbd13;
using sddp::kWave;

__global__ __launch_bounds__(kWave) void rollout_lane_kernel(sddp::DevConsts c, int N, int first, int count, int start, int steps,
                                                             const double* __restrict__ xs, const double* __restrict__ us,
                                                             const double* __restrict__ P, const double* __restrict__ pol, int pol_words,
                                                             const double* __restrict__ x_meas, double* __restrict__ x_out,
                                                             double* __restrict__ u_out, double* __restrict__ cost_out) {
    constexpr int NX = M::NX, NU = M::NU, NP = M::NP;
    const int i = blockIdx.x * kWave + threadIdx.x;
    if (i >= count) return;
    const int b = first + i;
    const double* xb = xs + size_t(b) * (N + 1) * NX;
    const double* ub = us + size_t(b) * N * NU;
    const double* Pb = P + size_t(b) * (N + 1) * NP;
    const double* rec = pol + size_t(b) * pol_words;
    const bool feedback = rec[pol_words - 1] != 0.0;
    double* xo = x_out + size_t(i) * (steps + 1) * NX;
    double* uo = u_out + size_t(i) * steps * NU;
    double x[NX], u[NU], xn[NX];
#pragma unroll
    for (int t = 0; t < NX; ++t) xo[t] = x[t] = x_meas[size_t(i) * NX + t];
    double J = 0.0;
    for (int j = 0; j < steps; ++j) {
        const int k = start + j;
#pragma unroll
        for (int r = 0; r < NU; ++r) {
            const double* K = rec + size_t(k) * NU * (NX + 1) + NU + size_t(r) * NX;
            double acc = ub[k * NU + r];
            if (feedback)
#pragma unroll
                for (int t = 0; t < NX; ++t) acc = fma(K[t], x[t] - xb[k * NX + t], acc);
            uo[j * NU + r] = u[r] = acc;
        }
        J += M::step(c, x, u, Pb + k * NP, k, xn);
#pragma unroll
        for (int t = 0; t < NX; ++t) xo[(j + 1) * NX + t] = x[t] = xn[t];
    }
    if (cost_out) cost_out[i] = J;
}

template <class F>
int time_ms(F launch, int reps, float* best, float* mean) {
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return 1;
    for (int w = 0; w < 3; ++w) launch();
    *best = 1e30f;
    double sum = 0.0;
    for (int r = 0; r < reps; ++r) {
        (void)hipEventRecord(e0, 0);
        launch();
        (void)hipEventRecord(e1, 0);
        if (hipEventSynchronize(e1) != hipSuccess) return 2;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e0, e1) != hipSuccess) return 2;
        *best = ms < *best ? ms : *best;
        sum += ms;
    }
    *mean = float(sum / reps);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}
}  // namespace

// out_* [count][...] as sddp_policy_rollout_device lays them out, one set per mapping; ms[4] = wave best, wave mean, lane best, lane mean
extern "C" int measure_rollouts(const sddp_model_consts* consts, int N, int count, int start, int steps, const double* xs, const double* us,
                                const double* P, const double* pol, int pol_words, const double* x_meas, double* x_wave, double* u_wave,
                                double* c_wave, double* x_lane, double* u_lane, double* c_lane, int reps, float* ms) {
    const sddp::DevConsts dc = sddp::make_dev_consts(*consts);
    int rc = time_ms([&] {
        hipLaunchKernelGGL((sddp::policy_rollout_kernel<M>), dim3(count), dim3(kWave), 0, 0, dc, N, 0, count, start, steps, xs, us, P, pol, pol_words,
                           x_meas, x_wave, u_wave, c_wave);
    }, reps, ms + 0, ms + 1);
    if (rc) return rc;
    return time_ms([&] {
        hipLaunchKernelGGL(rollout_lane_kernel, dim3((count + kWave - 1) / kWave), dim3(kWave), 0, 0, dc, N, 0, count, start, steps, xs, us, P, pol,
                           pol_words, x_meas, x_lane, u_lane, c_lane);
    }, reps, ms + 2, ms + 3);
}
