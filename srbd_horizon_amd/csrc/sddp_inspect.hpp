// sddp_inspect.hpp -- the kernels that only read: one model step, the policy rolled out and the plan inspectors (audit, stationarity
// certificate, cost breakdown, parameter and constant sensitivities).  They run the same device model code as the solve (M::step, M::derivs,
// M::F_entry, ...; the sensitivities M::param_grad, which the solve has no use for) on one wavefront per instance, and store to
// nothing but the caller's outputs.  (The knot evaluation of the parity tests reads only as
// well and stays in sddp_kernels.hpp, which says why.)
//
// Instantiated by the inspect unit of a model build alone (sddp_launch_inspect.hpp, sddp_inst.hip with -DSDDP_INST_INSPECT): a device
// module of their own, so that nothing written here can reach the code generation of the solve kernels (sddp_kernels.hpp,
// sddp_kernels_mw.hpp), which no longer share a module with them.  The record sizes that sddp_api.hip reports (kStationarityWords,
// kCostTermsWords, kCostTermsFamilies, kParamGradientWords, kConstGradientWords) are in sddp_kernels.hpp, where it finds them without this file.
#pragma once
#include "sddp_kernels.hpp"

namespace sddp {

// -----------------------------------------------------------------------------------------------------------------
// one model step per instance, x+ = f(x, u, p_k) (ddp.py:228-230): the closed-loop simulator step of the examples
// (dsrbd_example.py:158-159) through the same device model code as the solver.  One thread per instance.
// -----------------------------------------------------------------------------------------------------------------
// One thread per instance: b is not wave-uniform, so with a table every lane loads its own row (vector loads), not consts_of's.
__device__ __forceinline__ const DevConsts& lane_consts_of(const DevConsts& c, const int) { return c; }
__device__ __forceinline__ DevConsts lane_consts_of(const DevConsts* __restrict__ ctab, const int b) { return ctab[b]; }
template <class M, class... Tab>
__global__ __launch_bounds__(kWave) void model_step_kernel(ConstsArg<Tab...> consts, int B, int k, const double* __restrict__ x,
                                                           const double* __restrict__ u, const double* __restrict__ p,
                                                           double* __restrict__ xn) {
    constexpr int NX = M::NX, NU = M::NU, NP = M::NP;
    const int b = blockIdx.x * kWave + threadIdx.x;
    if (b >= B) return;
    const DevConsts& c = lane_consts_of(consts, b);
    double xv[NX], uv[NU], pv[NP], xo[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) xv[i] = x[size_t(b) * NX + i];
#pragma unroll
    for (int i = 0; i < NU; ++i) uv[i] = u[size_t(b) * NU + i];
#pragma unroll
    for (int i = 0; i < NP; ++i) pv[i] = p[size_t(b) * NP + i];
    (void)M::step(c, xv, uv, pv, k, xo);
#pragma unroll
    for (int i = 0; i < NX; ++i) xn[size_t(b) * NX + i] = xo[i];
}

// -----------------------------------------------------------------------------------------------------------------
// Closed-loop rollout of the exported policy from a measured state (sddp_policy_rollout_device): for the instances b = first + i,
//   x_0' = x_meas[i];  u_j' = u_k[b] + K_k[b] (x_j' - x_k[b]);  x_{j+1}' = f(x_j', u_j'; P[b][k], k),  k = start + j,  j < steps,
// through M::step, the model code of the solve's own rollout: its prediction, no renormalisation.  cost (may be null): the sum of
// the stage costs L_k(x_j', u_j') in knot order.  ok = 0 in the policy record `pol` [B][pol_words]: K is not multiplied (0 x NaN is
// not 0), the open-loop rollout of u_k from x_meas.
// One wavefront per instance.  Per knot, lane r < NU owns row r of K_k with apply_policy_kernel's FMA chain (u' at start = 0 is
// bit-equal to it), reading x_j' from LDS (every lane the same word: a broadcast, no conflict); lane 0 then runs the scalar model
// code as eval_knots_kernel does and leaves x_{j+1}' in LDS, from where the wave stores it.  Static LDS only, nothing of the
// slots' work buffers, plain vector stores to the caller's outputs alone.
template <class M, class... Tab>
__global__ __launch_bounds__(kWave) void policy_rollout_kernel(ConstsArg<Tab...> consts, int N, int first, int count, int start, int steps,
                                                               const double* __restrict__ xs, const double* __restrict__ us,
                                                               const double* __restrict__ P, const double* __restrict__ pol, int pol_words,
                                                               const double* __restrict__ x_meas, double* __restrict__ x_out,
                                                               double* __restrict__ u_out, double* __restrict__ cost_out) {
    constexpr int NX = M::NX, NU = M::NU, NP = M::NP;
    static_assert(NU <= kWave, "one lane per row of K_k");
    __shared__ double sz[NX + NU];                         // x_j' | u_j'
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= count) return;
    const int b = first + i;
    const DevConsts& c = consts_of(consts, b);
    const double* xb = xs + size_t(b) * (N + 1) * NX;
    const double* ub = us + size_t(b) * N * NU;
    const double* Pb = P + size_t(b) * (N + 1) * NP;
    const double* rec = pol + size_t(b) * pol_words;
    const bool feedback = rec[pol_words - 1] != 0.0;
    double* xo = x_out + size_t(i) * (steps + 1) * NX;
    double* uo = u_out + size_t(i) * steps * NU;
    for (int e = lane; e < NX; e += kWave) {
        const double v = x_meas[size_t(i) * NX + e];
        sz[e] = v;
        xo[e] = v;
    }
    wave_sync();
    double J = 0.0;
    for (int j = 0; j < steps; ++j) {
        const int k = start + j;
        if (lane < NU) {
            const double* K = rec + size_t(k) * NU * (NX + 1) + NU + size_t(lane) * NX;
            const double* xk = xb + k * NX;
            double acc = ub[k * NU + lane];
            if (feedback)
                for (int t = 0; t < NX; ++t) acc = fma(K[t], sz[t] - xk[t], acc);
            sz[NX + lane] = acc;
            uo[j * NU + lane] = acc;
        }
        wave_sync();
        if (lane == 0) {
            double xl[NX], ul[NU], xn[NX];
#pragma unroll
            for (int t = 0; t < NX; ++t) xl[t] = sz[t];
#pragma unroll
            for (int t = 0; t < NU; ++t) ul[t] = sz[NX + t];
            J += M::step(c, xl, ul, Pb + k * NP, k, xn);
#pragma unroll
            for (int t = 0; t < NX; ++t) sz[t] = xn[t];
        }
        wave_sync();
        for (int e = lane; e < NX; e += kWave) xo[(j + 1) * NX + e] = sz[e];
    }
    if (lane == 0 && cost_out) cost_out[i] = J;
}

// -----------------------------------------------------------------------------------------------------------------
// Plan audit (sddp_audit_range_device): how far a trajectory is from what the solver only penalises -- friction cone, unilateral
// force, load on a swing foot, quaternion norm, foot height, slip, rigid foot, dynamics defect -- as SDDP_AUDIT_WORDS maxima per
// instance (include/sddp.h has the table).  x [..][steps + 1][NX], u [..][steps][NU]: row j sits at node start + j; instance
// b = first + i reads block xoff + i of them (the handle's own xs / us: xoff = first, steps = N; a caller's: xoff = 0) and row b of P.
// ml: the linearised friction coefficient of the call.
// One wavefront per instance; lane l audits the nodes j = l, l + 64, ... on its own (one M::step per stage node, the model code of
// the solve's rollout) into private maxima, one butterfly of shuffles merges them, lane 0 stores the record.  Read-only but for
// `out`: no LDS, no atomics, no work buffer.
// Every maximum propagates NaN (fmax would drop it), and a NaN maximum has no index.
__device__ __forceinline__ double nan_max(const double a, const double b) { return a != a ? a : (b != b ? b : (b > a ? b : a)); }
// a maximum with the place it was found at: key = node * NC + contact, smaller key on ties (first in node-major order)
struct AuditMax {
    double v;
    int key;
};
constexpr int kAuditNoKey = 0x7fffffff;
__device__ __forceinline__ void audit_take(AuditMax& m, const double v, const int key) {
    if (m.v != m.v) return;
    if (v != v) { m.v = v; m.key = kAuditNoKey; }
    else if (v > m.v || (v == m.v && key < m.key)) { m.v = v; m.key = key; }
}
__device__ __forceinline__ void audit_merge(AuditMax& m) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double v = __shfl_xor(m.v, o, kWave);
        const int key = __shfl_xor(m.key, o, kWave);
        audit_take(m, v, key);
    }
}
__device__ __forceinline__ double audit_merge(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = nan_max(v, __shfl_xor(v, o, kWave));
    return v;
}
__device__ __forceinline__ double audit_index(const AuditMax& m, const int div, const bool rem) {
    if (m.v != m.v || m.key == kAuditNoKey) return -1.0;
    return double(rem ? m.key % div : m.key / div);
}
template <class M, class... Tab>
__global__ __launch_bounds__(kWave) void plan_audit_kernel(ConstsArg<Tab...> consts, int N, int first, int count, int start, int steps,
                                                            const double* __restrict__ x, const double* __restrict__ u, int xoff,
                                                            const double* __restrict__ P, double ml, double* __restrict__ out) {
    constexpr int NX = M::NX, NU = M::NU, NP = M::NP, NC = M::NC;
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= count) return;
    const int b = first + i;
    const DevConsts& c = consts_of(consts, b);
    const double* xb = x + size_t(xoff + i) * (steps + 1) * NX;
    const double* ub = u + size_t(xoff + i) * steps * NU;
    const double* Pb = P + (size_t(b) * (N + 1) + start) * NP;
    const double inf = __builtin_huge_val();
    AuditMax cone{-inf, kAuditNoKey}, pull{-inf, kAuditNoKey}, defect{0.0, kAuditNoKey};
    double swing = 0.0, drift = 0.0, height = 0.0, slip = 0.0, rigid = 0.0;
    int stance_pairs = 0;
    for (int j = lane; j <= steps; j += kWave) {
        const double* xj = xb + size_t(j) * NX;
        if constexpr (M::AUDIT_QUAT) {
            const double* o = xj + M::XO;
            drift = nan_max(drift, fabs(sqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2] + o[3] * o[3]) - 1.0));
        }
        if (j == steps) break;
        const int k = start + j;
        const double* uj = ub + size_t(j) * NU;
        const double* pj = Pb + size_t(j) * NP;
#pragma unroll
        for (int n = 0; n < NC; ++n) {
            const bool stance = M::p_sw(pj, n) > 0.5;
            if constexpr (M::AUDIT_FORCES) {
                const double* f = uj + M::uf(n);
                const double side = nan_max(fabs(f[0]), fabs(f[1]));
                if (stance) {
                    audit_take(cone, side - ml * f[2], k * NC + n);
                    audit_take(pull, -f[2], k * NC + n);
                    ++stance_pairs;
                } else {
                    swing = nan_max(swing, nan_max(side, fabs(f[2])));
                }
            }
            if constexpr (M::AUDIT_CONTACT_STATES) {
                height = nan_max(height, fabs(xj[M::XC + 3 * n + 2] - M::p_cref(pj, n)));
                if (stance) slip = nan_max(slip, nan_max(fabs(xj[M::XCD + 3 * n]), fabs(xj[M::XCD + 3 * n + 1])));
            }
        }
        if constexpr (M::AUDIT_CONTACT_STATES) {
            if (c.w_rv != 0.0) {
#pragma unroll
                for (int q = 0; q < M::NRV; ++q)
#pragma unroll
                    for (int e = 0; e < 2; ++e)
                        rigid = nan_max(rigid, fabs(xj[M::XCD + 3 * M::rv_a(q) + e] - xj[M::XCD + 3 * M::rv_b(q) + e]));
            }
        }
        double xn[NX];
        (void)M::step(c, xj, uj, pj, k, xn);
        double d = 0.0;
#pragma unroll
        for (int e = 0; e < NX; ++e) d = nan_max(d, fabs(xj[NX + e] - xn[e]));
        audit_take(defect, d, k);
    }
    audit_merge(cone);
    audit_merge(pull);
    audit_merge(defect);
    swing = audit_merge(swing);
    drift = audit_merge(drift);
    height = audit_merge(height);
    slip = audit_merge(slip);
    rigid = audit_merge(rigid);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) stance_pairs += __shfl_xor(stance_pairs, o, kWave);
    if (lane == 0) {
        double* r = out + size_t(i) * SDDP_AUDIT_WORDS;
        r[0] = cone.v;  r[1] = audit_index(cone, NC, false);  r[2] = audit_index(cone, NC, true);
        r[3] = pull.v;  r[4] = audit_index(pull, NC, false);
        r[5] = swing;   r[6] = drift;  r[7] = height;  r[8] = slip;  r[9] = rigid;
        r[10] = defect.v;  r[11] = audit_index(defect, 1, false);
        r[12] = double(steps);  r[13] = double(stance_pairs);
        r[14] = 0.0;  r[15] = 0.0;
    }
}

// -----------------------------------------------------------------------------------------------------------------
// Stationarity certificate (sddp_stationarity_range_device): the costates and the reduced gradient of a whole-horizon trajectory,
//   lambda_N = l_x,N;   q_k = [l_x,k ; l_u,k] + F_k^T lambda_{k+1},  F_k = [f_x f_u] at (x_k, u_k, p_k);   lambda_k = q_k[0:NX],  s_k = q_k[NX:NZ],
// k = N - 1 .. 0, every derivative at the STORED (x_k, u_k) whatever the gaps (the multiple-shooting linearisation), and 8 doubles per
// instance (include/sddp.h has the table).  x [..][N + 1][NX], u [..][N][NU]; instance b = first + i reads block xoff + i of them
// (the handle's own xs / us: xoff = first; a caller's: xoff = 0) and row b of P.
// One wavefront per instance, the knots backward.  Per knot, lane 0 runs the scalar model code as eval_knots_kernel does -- M::derivs
// into a knot record in LDS, with a zero input vector at the terminal knot -- and M::step on the operands plan_audit_kernel gives it
// (word 6 is its word 10); the wave then expands F_k into an LDS tile through M::F_entry exactly as eval_knots_kernel does, and lane
// z < NZ, two passes where NZ > 64, forms q[z] = g[z] + sum_j F[j][z] lambda_{k+1}[j] as one FMA chain over j = 0 .. NX - 1, lambda_{k+1}
// read from LDS (every lane the same word: a broadcast; F[j][.]: consecutive words).  The tile is kept because the committed results
// are defined by it: the records the tests and profiles/stationarity hold are the FMA chain over F_k as this expansion stores it.  It
// came in while this kernel shared a device module with the solve kernels, where calling M::F_entry with other index expressions than
// eval_knots_kernel's changed the instruction streams of the srbd13 solve, backward and policy kernels (profiles/stationarity).  The
// solve kernels no longer share a module with this kernel (sddp_launch_inspect.hpp), so that reason is gone; doing without the tile
// is a change of what is computed and when, with evidence of its own.
// lambda ping-pongs between two LDS vectors, so a pass never reads what it writes.  The maxima are the audit's: NaN propagates, a NaN
// maximum has no index, the smaller key = node * NU + input wins a tie.  Static LDS only (NREC + 2 NX + NX NZ doubles: 56.7 KB for
// srbd61), nothing of the slots' work buffers, plain vector stores to the caller's outputs alone (lam / grad may be null).
template <class M, class... Tab>
__global__ __launch_bounds__(kWave) void stationarity_kernel(ConstsArg<Tab...> consts, int N, int first, int count,
                                                              const double* __restrict__ x, const double* __restrict__ u, int xoff,
                                                              const double* __restrict__ P, double* __restrict__ out,
                                                              double* __restrict__ lam_out, double* __restrict__ grad_out) {
    constexpr int NX = M::NX, NU = M::NU, NZ = M::NZ, NP = M::NP, NREC = M::NREC;
    __shared__ double srec[NREC];                          // the record of knot k
    __shared__ double slam[2][NX];                         // lambda_{k+1} | lambda_k, swapping
    __shared__ double sF[NX * NZ];                         // F_k, row-major
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= count) return;
    const int b = first + i;
    const DevConsts& c = consts_of(consts, b);
    const double* xb = x + size_t(xoff + i) * (N + 1) * NX;
    const double* ub = u + size_t(xoff + i) * N * NU;
    const double* Pb = P + size_t(b) * (N + 1) * NP;
    double* lo = lam_out ? lam_out + size_t(i) * (N + 1) * NX : nullptr;
    double* go = grad_out ? grad_out + size_t(i) * N * NU : nullptr;
    AuditMax stat{0.0, kAuditNoKey}, defect{0.0, kAuditNoKey};
    double scale = 0.0, lam0 = 0.0, lam_rest = 0.0;
    int cur = 0;
    for (int k = N; k >= 0; --k) {
        const double* xk = xb + size_t(k) * NX;
        const double* pk = Pb + size_t(k) * NP;
        if (lane == 0) {
            double xl[NX], ul[NU];
#pragma unroll
            for (int t = 0; t < NX; ++t) xl[t] = xk[t];
#pragma unroll
            for (int t = 0; t < NU; ++t) ul[t] = k < N ? ub[size_t(k) * NU + t] : 0.0;
            M::derivs(c, xl, ul, pk, k, N, srec);
            if (k < N) {
                double xn[NX];
                (void)M::step(c, xk, ub + size_t(k) * NU, pk, k, xn);
                double d = 0.0;
#pragma unroll
                for (int e = 0; e < NX; ++e) d = nan_max(d, fabs(xk[NX + e] - xn[e]));
                audit_take(defect, d, k);
            }
        }
        wave_sync();
        if (k == N) {
            for (int z = lane; z < NX; z += kWave) {
                const double v = srec[M::REC_G + z];
                slam[cur][z] = v;
                if (lo) lo[size_t(k) * NX + z] = v;
                lam_rest = nan_max(lam_rest, fabs(v));
            }
        } else {
            const double* ln = slam[cur];
            for (int e = lane; e < NX * NZ; e += kWave) sF[e] = M::F_entry(c, srec, e / NZ, e % NZ);
            wave_sync();
            for (int z = lane; z < NZ; z += kWave) {
                const double g = srec[M::REC_G + z];
                double acc = g, mag = fabs(g);
                for (int j = 0; j < NX; ++j) {
                    const double f = sF[j * NZ + z], l = ln[j];
                    acc = fma(f, l, acc);
                    mag = fma(fabs(f), fabs(l), mag);
                }
                if (z < NX) {
                    slam[cur ^ 1][z] = acc;
                    if (lo) lo[size_t(k) * NX + z] = acc;
                    if (k == 0) lam0 = nan_max(lam0, fabs(acc));
                    else lam_rest = nan_max(lam_rest, fabs(acc));
                } else {
                    if (go) go[size_t(k) * NU + (z - NX)] = acc;
                    audit_take(stat, fabs(acc), k * NU + (z - NX));
                    scale = nan_max(scale, mag);
                }
            }
            cur ^= 1;
        }
        wave_sync();                                       // lambda_k is in LDS, and the record is free for knot k - 1
    }
    audit_merge(stat);
    scale = audit_merge(scale);
    lam0 = audit_merge(lam0);
    lam_rest = audit_merge(lam_rest);
    if (lane == 0) {
        double* r = out + size_t(i) * kStationarityWords;
        r[0] = stat.v;  r[1] = audit_index(stat, NU, false);  r[2] = audit_index(stat, NU, true);
        r[3] = scale;  r[4] = lam0;  r[5] = lam_rest;
        r[6] = defect.v;  r[7] = double(N);
    }
}

// -----------------------------------------------------------------------------------------------------------------
// Cost breakdown (sddp_cost_terms_range_device): the cost of a whole-horizon trajectory family by family, kCostTermsWords doubles per
// instance (include/sddp.h has the table).  No model code of its own: column 0 of a node is M::step / M::term_cost on the instance's
// constants as they are, column 1 + f the same code on a copy that keeps family f's weights and has 0.0 in every other one, so the
// terms of a family are formed and added exactly as inside the full cost.  The copy is made BY DATA (w' = keep ? w : 0.0, a pointer
// select for the user rows' table, whose second copy `xr_zero` has zero weights), so the wave runs one instruction stream whatever
// families its lanes hold; what diverges is k == N (term_cost) and what the model branches on itself.  One weight is no constant but
// a parameter (M::P_WEIGHT, orientation_tracking_gain): the instance's parameter rows are staged in LDS twice, as they are and with
// that column 0.0, and a column reads the second copy unless it is the total or `unweighted` -- the family of what is left when every
// weight of DevConsts is 0.0.  A user build's rows may read any parameter, so there family 11 is evaluated on the rows as they are
// and the node's `unweighted` is taken off it afterwards (the one place a family is a difference).
// x [..][N + 1][NX], u [..][N][NU]; instance b = first + i reads block xoff + i of them (the handle's own xs / us: xoff = first; a
// caller's: xoff = 0) and row b of P.  One wavefront per instance; the work items are the (node, column) pairs e = k * 14 + col,
// strided over the lanes; M::step's next state is discarded.  The addends go to a tile [N + 1][14] in dynamic LDS (the launcher
// refuses horizons whose tile and parameter copies exceed it) and from there to `nodes` when given; then lane col < 14 adds its
// column in node order, which is the record: no lane mapping enters a sum.  Plain vector stores to out / nodes alone.
constexpr int kCostTermsCols = kCostTermsFamilies + 1;
template <class M>
constexpr size_t cost_terms_lds(int N) {
    return sizeof(double) * (size_t(N + 1) * (kCostTermsCols + (M::P_WEIGHT >= 0 ? 2 * M::NP : 0)) + kCostTermsCols);
}
// the constants of column col: the total (0) keeps everything, family f = col - 1 what include/sddp.h's table says
__device__ __forceinline__ DevConsts cost_terms_consts(const DevConsts& c, const int col, const double* xr_zero) {
    const int f = col - 1;
    const bool all = col == 0;
    DevConsts m = c;
    m.w_rz = (all || f == 0) ? c.w_rz : 0.0;
    m.w_rxy = (all || f == 0) ? c.w_rxy : 0.0;
    m.w_rd = (all || f == 1) ? c.w_rd : 0.0;
    m.w_w = (all || f == 2) ? c.w_w : 0.0;
    m.w_rel = (all || f == 3) ? c.w_rel : 0.0;
    m.w_f = (all || f == 4) ? c.w_f : 0.0;
    m.w_sw = (all || f == 5) ? c.w_sw : 0.0;
    m.gq = (all || f == 6) ? c.gq : 0.0;
    m.w_zmp = (all || f == 7) ? c.w_zmp : 0.0;
    m.w_pen = (all || f == 8) ? c.w_pen : 0.0;
    m.w_rv = (all || f == 8) ? c.w_rv : 0.0;
    m.bar_w = (all || f == 9) ? c.bar_w : 0.0;
    m.box_w = (all || f == 10) ? c.box_w : 0.0;
    m.xr = (all || f == 11) ? c.xr : xr_zero;
    return m;
}
template <class M, class... Tab>
__global__ __launch_bounds__(kWave) void cost_terms_kernel(ConstsArg<Tab...> consts, const double* __restrict__ xr_zero, int N, int first,
                                                            int count, const double* __restrict__ x, const double* __restrict__ u, int xoff,
                                                            const double* __restrict__ P, double* __restrict__ out,
                                                            double* __restrict__ nodes) {
    constexpr int NX = M::NX, NU = M::NU, NP = M::NP, NCOL = kCostTermsCols;
    constexpr bool PW = M::P_WEIGHT >= 0;
    extern __shared__ __attribute__((aligned(16))) double s[];
    double* tile = s;                                      // [N + 1][NCOL] the addends
    double* sums = tile + size_t(N + 1) * NCOL;            // [NCOL] their sums
    double* sp = sums + NCOL;                              // PW: [2][N + 1][NP] the parameters | with column P_WEIGHT = 0.0
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= count) return;
    const int b = first + i;
    const DevConsts& c = consts_of(consts, b);
    const double* xb = x + size_t(xoff + i) * (N + 1) * NX;
    const double* ub = u + size_t(xoff + i) * N * NU;
    const double* Pb = P + size_t(b) * (N + 1) * NP;
    const int items = (N + 1) * NCOL;
    if constexpr (PW) {
        for (int e = lane; e < (N + 1) * NP; e += kWave) {
            const double v = Pb[e];
            sp[e] = v;
            sp[(N + 1) * NP + e] = e % NP == M::P_WEIGHT ? 0.0 : v;
        }
        wave_sync();
    }
    for (int e = lane; e < items; e += kWave) {
        const int k = e / NCOL, col = e % NCOL;
        const DevConsts m = cost_terms_consts(c, col, xr_zero);
        const double* pk = Pb + size_t(k) * NP;
        if constexpr (PW) {
            const bool as_is = col == 0 || col == NCOL - 1 || (M::HAS_UR && col == NCOL - 2);
            pk = sp + (as_is ? 0 : (N + 1) * NP) + k * NP;
        }
        const double* xk = xb + size_t(k) * NX;
        double v;
        if (k == N) {
            v = M::term_cost(m, xk, pk);
        } else {
            double xn[NX];
            v = M::step(m, xk, ub + size_t(k) * NU, pk, k, xn);
        }
        tile[e] = v;
    }
    wave_sync();
    if constexpr (M::HAS_UR && PW) {
        for (int k = lane; k <= N; k += kWave) tile[k * NCOL + NCOL - 2] -= tile[k * NCOL + NCOL - 1];
        wave_sync();
    }
    if (nodes) {
        double* no = nodes + size_t(i) * items;
        for (int e = lane; e < items; e += kWave) no[e] = tile[e];
    }
    if (lane < NCOL) {
        double acc = 0.0;
        for (int k = 0; k <= N; ++k) acc += tile[k * NCOL + lane];
        sums[lane] = acc;
        out[size_t(i) * kCostTermsWords + lane] = acc;
    }
    wave_sync();
    if (lane == 0) {
        int best = 0;
        bool nan = false;
        for (int f = 0; f < kCostTermsFamilies - 1; ++f) {
            const double v = sums[1 + f];
            nan = nan || v != v;
            if (v > sums[1 + best]) best = f;
        }
        out[size_t(i) * kCostTermsWords + 14] = nan ? -1.0 : double(best);
        out[size_t(i) * kCostTermsWords + 15] = double(N);
    }
}

// -----------------------------------------------------------------------------------------------------------------
// Parameter sensitivities (sddp_param_gradient_range_device): the gradient of the Lagrangian of a whole-horizon trajectory in the
// per-knot parameters,
//   G_k[j] = dL_k/dp_k[j] + sum_i lambda_{k+1}[i] df_k[i]/dp_k[j]  (k < N),    G_N[j] = dL_N/dp_N[j],
// through M::param_grad, and kParamGradientWords doubles per instance (include/sddp.h has the table).  The costates are not formed
// here: lam [count][N + 1][NX] and stat [count][kStationarityWords] are what stationarity_kernel stored for the same range just
// before on the same stream (sddp_api.hip), block i for instance first + i, and words 4 - 6 of the record are words 4, 0, 6 of stat as
// they are.  x [..][N + 1][NX], u [..][N][NU]; instance b = first + i reads block xoff + i of them and row b of P.
// With lambda given the nodes are independent.  One wavefront per instance, lane l on the nodes k = l, l + 64, ..., as
// plan_audit_kernel does it, rather than a flat grid over count (N + 1) nodes: the record is a maximum over the nodes of one instance
// with its place, which one butterfly of shuffles merges inside the wave; a flat grid would split an instance across wavefronts and
// need a second pass or atomics for it.  A lane keeps G_k and its magnitudes (2 NP doubles: 70 on srbd61_x) and what M::param_grad
// needs of the knot: on the models with contact states (srbd37, srbd61, lip30) no parameter enters f, so that is a handful of state
// entries and no model core; on srbd13 the core of one knot (the solve's rollout keeps the same).  x and u are read in place, not
// copied to per-lane arrays: no LDS, no scratch (profiles/param_gradient has the compiler's figures per build).
// Read-only but for out / grad: plain vector stores to the caller's outputs alone, no atomics, no work buffer.  The maxima are the
// audit's: NaN propagates, a NaN maximum has no place, the smaller key = node * NP + column wins a tie.
template <class M, class... Tab>
__global__ __launch_bounds__(kWave) void param_gradient_kernel(ConstsArg<Tab...> consts, int N, int first, int count,
                                                                const double* __restrict__ x, const double* __restrict__ u, int xoff,
                                                                const double* __restrict__ P, const double* __restrict__ lam,
                                                                const double* __restrict__ stat, double* __restrict__ out,
                                                                double* __restrict__ grad) {
    constexpr int NX = M::NX, NU = M::NU, NP = M::NP;
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= count) return;
    const int b = first + i;
    const DevConsts& c = consts_of(consts, b);
    const double* xb = x + size_t(xoff + i) * (N + 1) * NX;
    const double* ub = u + size_t(xoff + i) * N * NU;
    const double* Pb = P + size_t(b) * (N + 1) * NP;
    const double* lb = lam + size_t(i) * (N + 1) * NX;
    double* go = grad ? grad + size_t(i) * (N + 1) * NP : nullptr;
    AuditMax top{0.0, kAuditNoKey};
    double scale = 0.0;
    for (int k = lane; k <= N; k += kWave) {
        double g[NP], m[NP];
        // (k == N: no input and no next costate; param_grad reads neither there, the pointers stay inside the buffers)
        M::param_grad(c, xb + size_t(k) * NX, ub + size_t(k < N ? k : 0) * NU, Pb + size_t(k) * NP, k, N,
                      lb + size_t(k < N ? k + 1 : k) * NX, g, m);
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            if (go) go[size_t(k) * NP + j] = g[j];
            audit_take(top, fabs(g[j]), k * NP + j);
            scale = nan_max(scale, m[j]);
        }
    }
    audit_merge(top);
    scale = audit_merge(scale);
    if (lane == 0) {
        const double* s = stat + size_t(i) * kStationarityWords;
        double* r = out + size_t(i) * kParamGradientWords;
        r[0] = top.v;  r[1] = audit_index(top, NP, false);  r[2] = audit_index(top, NP, true);
        r[3] = scale;  r[4] = s[4];  r[5] = s[0];  r[6] = s[6];  r[7] = double(N);
    }
}

// -----------------------------------------------------------------------------------------------------------------
// Constant sensitivities (sddp_const_gradient_range_device): the gradient of the Lagrangian of a whole-horizon trajectory in the derived
// constants the kernels read (ConstCol, sddp_models.hpp),
//   C[c] = sum_{k < N} ( dL_k/dtheta_c + sum_i lambda_{k+1}[i] df_k[i]/dtheta_c ) + dL_N/dtheta_c,
// through M::const_grad, and kConstGradientWords doubles per instance (include/sddp.h has the table).  The costates and stat are the
// stationarity launch's, as for param_gradient_kernel; words 34 - 36 of the record are words 4, 0, 6 of stat as they are.
// One wavefront per instance, lane l on the nodes k = l, l + 64, ...; with per-instance constants instance b reads its own row.
// A column is a SUM over the nodes, so its order is fixed as the cost breakdown fixes it: the addends of node k go to row k of a tile
// [N + 1][32] in dynamic LDS (the launcher refuses horizons whose tile exceeds it), from there to `nodes` when given, and lane c < 32
// then adds column c in node order: no lane mapping enters a sum.  Inside a row the columns are rotated by the node (entry c of node k
// at k * 32 + ((c + k) & 31)): a lane writes its row and the summing lanes walk down theirs without meeting on one bank.
// Plain vector stores to out / nodes alone, no atomics, no work buffer.
template <class M, class... Tab>
__global__ __launch_bounds__(kWave) void const_gradient_kernel(ConstsArg<Tab...> consts, int N, int first, int count,
                                                                const double* __restrict__ x, const double* __restrict__ u, int xoff,
                                                                const double* __restrict__ P, const double* __restrict__ lam,
                                                                const double* __restrict__ stat, double* __restrict__ out,
                                                                double* __restrict__ nodes) {
    constexpr int NX = M::NX, NU = M::NU, NP = M::NP, NCOL = kConstGradientCols;
    static_assert(NCOL == 32, "the rotation of a row and the summing lanes");
    extern __shared__ __attribute__((aligned(16))) double s[];
    double* tile = s;                                      // [N + 1][NCOL] the addends
    double* rel = tile + size_t(N + 1) * NCOL;             // [NCOL] |C theta| of the columns
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= count) return;
    const int b = first + i;
    const DevConsts& c = consts_of(consts, b);
    const double* xb = x + size_t(xoff + i) * (N + 1) * NX;
    const double* ub = u + size_t(xoff + i) * N * NU;
    const double* Pb = P + size_t(b) * (N + 1) * NP;
    const double* lb = lam + size_t(i) * (N + 1) * NX;
    for (int k = lane; k <= N; k += kWave) {
        double g[NCOL];
        // (k == N: no input and no next costate; const_grad reads neither there, the pointers stay inside the buffers)
        M::const_grad(c, xb + size_t(k) * NX, ub + size_t(k < N ? k : 0) * NU, Pb + size_t(k) * NP, k, N,
                      lb + size_t(k < N ? k + 1 : k) * NX, g);
#pragma unroll
        for (int j = 0; j < NCOL; ++j) tile[k * NCOL + ((j + k) & (NCOL - 1))] = g[j];
    }
    wave_sync();
    if (nodes) {
        double* no = nodes + size_t(i) * (N + 1) * NCOL;
        for (int e = lane; e < (N + 1) * NCOL; e += kWave) {
            const int k = e / NCOL, j = e % NCOL;
            no[e] = tile[k * NCOL + ((j + k) & (NCOL - 1))];
        }
    }
    double* r = out + size_t(i) * kConstGradientWords;
    if (lane < NCOL) {
        double acc = 0.0;
        for (int k = 0; k <= N; ++k) acc += tile[k * NCOL + ((lane + k) & (NCOL - 1))];
        r[lane] = acc;
        double th = 0.0;      // (a select over compile-time columns: a run-time index into the constants would put the table form's copy in scratch)
#pragma unroll
        for (int j = 0; j < NCOL; ++j) th = lane == j ? const_col_value(c, j) : th;
        rel[lane] = fabs(acc * th);
    }
    wave_sync();
    if (lane == 0) {
        int best = 0;
        bool nan = false;
        for (int j = 0; j < NCOL; ++j) {
            const double v = rel[j];
            nan = nan || v != v;
            if (v > rel[best]) best = j;
        }
        const double* st = stat + size_t(i) * kStationarityWords;
        r[NCOL] = nan ? __builtin_nan("") : rel[best];
        r[NCOL + 1] = nan ? -1.0 : double(best);
        r[NCOL + 2] = st[4];  r[NCOL + 3] = st[0];  r[NCOL + 4] = st[6];  r[NCOL + 5] = double(N);
        r[NCOL + 6] = 0.0;  r[NCOL + 7] = 0.0;
    }
}

// -----------------------------------------------------------------------------------------------------------------
// Plan uncertainty (sddp_policy_covariance_device): the covariance of the state under the exported policy, linearised along the plan,
//   S_0 = Sigma0[i];   S_{j+1} = A_k S_j A_k^T + B_k diag(r) B_k^T + diag(q),   A_k = f_x + f_u K_k  (ok = 0: f_x),  B_k = f_u,   k = start + j,
// [f_x f_u] = F_k at the STORED (x_k, u_k, p_k) through M::derivs + M::F_entry as stationarity_kernel takes it, the feedback's share of
// the input covariance U_j = K_k S_j K_k^T, the cone margin of every stance force in standard deviations of it, and kPolicyCovWords
// doubles per instance (include/sddp.h has the table and the order of every FMA chain; nothing below may change a chain).
// One wavefront per instance, the knots forward.  Per knot, lane 0 runs M::derivs into the knot record in LDS; then
//   U:  lane r < NU holds row r of K_k in registers and forms row r of K S_j (S_j from LDS: every lane the same word, a broadcast) into
//       the tile; lanes then form diag U and the lower triangles of the 3 x 3 force blocks from it and K;
//   A:  f_u goes to the tile (rows padded to an odd length: a lane walks its own row); lane m < NX forms row m of A_k in registers;
//   G:  lane m forms G[i][m] = q / r terms, i >= m, into the NEXT triangle, where the chain of S'[i][m] starts;
//   T:  lane i forms row i of T = A S_j into the tile, S_j again a broadcast;
//   S': lane m adds sum_l T[i][l] A[m][l] for i >= m: T[i][.] a broadcast, A[m][.] its registers.
// So the NX^2 products of a stage cost a lane one LDS broadcast and one FMA each, nothing crosses lanes, and a lane keeps one row of A
// (NX doubles) and nothing else across the phases.  S is symmetric by construction (one word per pair), so it lives as two lower
// triangles, this knot's and the next; with the one tile that K S, f_u and T share in turn, srbd61 (NX = 61) needs 62.7 KB where two
// full S tiles and a T tile would need 89: static LDS, at most 64 KB on every build (asserted).  Nothing of the slots' work buffers,
// plain vector stores to the caller's outputs alone (cov / ucov may be null).  The maxima are the audit's (nan_max, audit_take); a
// minimum is the maximum of the negated operands.
// where the mapping fits: one lane per row of A_k, of K_k and per entry of the force blocks, f_u inside the shared tile, and the static
// LDS of one workgroup at most 64 KB.  The four models and their _x builds do; a user build that does not gets no kernel, and the call
// answers SDDP_ERR_ARG
template <class M>
constexpr bool policy_covariance_fits() {
    constexpr int NX = M::NX, NU = M::NU, NCF = M::AUDIT_FORCES ? M::NC : 0;
    return NX <= kWave && (NU | 1) <= NX && 6 * NCF <= kWave &&
           sizeof(double) * (M::NREC + NX * (NX + 1) + NX * NX + NU + 6 * NCF + 1) <= 64 * 1024;
}
// The model code of this kernel is an instantiation of its own.  Every device function is internal to the module and inlined, but until
// it is, the compiler's interprocedural passes see M::derivs and M::F_entry with all their callers: with this kernel among them,
// stationarity_kernel of the SRBD builds -- until now their one caller here -- came out as another instruction stream (up to every
// line of it on the _x builds; profiles/policy_covariance).  So for the library's SRBD models the kernel calls the same code through a
// twin type, SrbdModel<..., CovTwinTag>: the user-rows parameter set to a tag that means what void means (no such rows), hence the
// same source, constants and layout, instantiated apart.  lip30's stationarity_kernel did not move, and a user build has no parent to
// be compared with: they use M itself.
struct CovTwinTag;
template <>
struct UrInfo<CovTwinTag> : UrInfo<void> {};
template <class M>
struct cov_twin { using type = M; };
template <int NC, bool CS, bool BAR, bool SO2, int XR>
struct cov_twin<SrbdModel<NC, CS, BAR, SO2, XR, void>> { using type = SrbdModel<NC, CS, BAR, SO2, XR, CovTwinTag>; };
__device__ __forceinline__ int cov_tri(const int i, const int m) { return i >= m ? i * (i + 1) / 2 + m : m * (m + 1) / 2 + i; }
template <class M, class... Tab>
__global__ __launch_bounds__(kWave) void policy_covariance_kernel(ConstsArg<Tab...> consts, int N, int first, int count, int start, int steps,
                                                                   const double* __restrict__ xs, const double* __restrict__ us,
                                                                   const double* __restrict__ P, const double* __restrict__ pol, int pol_words,
                                                                   const double* __restrict__ sigma0, const double* __restrict__ qv,
                                                                   const double* __restrict__ rv, double ml, double* __restrict__ out,
                                                                   double* __restrict__ cov, double* __restrict__ ucov) {
    constexpr int NX = M::NX, NU = M::NU, NP = M::NP, NREC = M::NREC, NTRI = NX * (NX + 1) / 2, NUP = NU | 1;
    using MM = typename cov_twin<M>::type;                 // derivs and F_entry: see cov_twin
    static_assert(MM::NX == M::NX && MM::NZ == M::NZ && MM::NREC == M::NREC && MM::REC_G == M::REC_G, "the twin is the model");
    constexpr int NCF = M::AUDIT_FORCES ? M::NC : 0;      // contacts whose force is an input
    static_assert(policy_covariance_fits<M>(), "instantiated only where it fits (sddp_launch_inspect.hpp leaves the entry null elsewhere)");
    __shared__ double srec[NREC];                          // the record of knot k
    __shared__ double sS[2][NTRI];                         // S_j | S_{j+1}, swapping: lower triangles, row-major
    __shared__ double sT[NX * NX];                         // K S_j [NU][NX], then f_u [NX][NUP], then T = A S_j [NX][NX]
    __shared__ double sU[NU + 6 * NCF + 1];                // diag U_j | per contact the block's (0,0) (1,0) (1,1) (2,0) (2,1) (2,2)
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= count) return;
    const int b = first + i;
    const DevConsts& c = consts_of(consts, b);
    const double* xb = xs + size_t(b) * (N + 1) * NX;
    const double* ub = us + size_t(b) * N * NU;
    const double* Pb = P + size_t(b) * (N + 1) * NP;
    const double* rec = pol + size_t(b) * pol_words;
    const bool feedback = rec[pol_words - 1] != 0.0;
    const double* qi = qv ? qv + size_t(i) * NX : nullptr;
    const double* ri = rv ? rv + size_t(i) * NU : nullptr;
    double* co = cov ? cov + size_t(i) * (steps + 1) * NX * NX : nullptr;
    double* uo = ucov ? ucov + size_t(i) * steps * NU : nullptr;
    const double inf = __builtin_huge_val();
    AuditMax zneg{-inf, kAuditNoKey}, trmax{-inf, kAuditNoKey}, umax{-inf, kAuditNoKey};
    double dneg = -inf;                                    // max of -S_j[i][i]
    const double* s0 = sigma0 + size_t(i) * NX * NX;
    for (int e = lane; e < NX * NX; e += kWave)
        if (e % NX <= e / NX) sS[0][cov_tri(e / NX, e % NX)] = s0[e];
    wave_sync();
    // what the record keeps of S_j (in sS[cur]), and row j of cov
    auto note = [&](const int cur, const int j) {
        if (lane == 0) {
            double tr = 0.0;
            for (int t = 0; t < NX; ++t) tr += sS[cur][cov_tri(t, t)];
            audit_take(trmax, tr, start + j);
        }
        if (lane < NX) dneg = nan_max(dneg, -sS[cur][cov_tri(lane, lane)]);
        if (co)
            for (int e = lane; e < NX * NX; e += kWave) co[size_t(j) * NX * NX + e] = sS[cur][cov_tri(e / NX, e % NX)];
    };
    for (int j = 0; j < steps; ++j) {
        const int k = start + j, cur = j & 1, nxt = cur ^ 1;
        const double* pk = Pb + size_t(k) * NP;
        const double* K = rec + size_t(k) * NU * (NX + 1) + NU;
        const double* Sc = sS[cur];
        double* Sn = sS[nxt];
        note(cur, j);
        if (lane == 0) {
            double xl[NX], ul[NU];
#pragma unroll
            for (int t = 0; t < NX; ++t) xl[t] = xb[size_t(k) * NX + t];
#pragma unroll
            for (int t = 0; t < NU; ++t) ul[t] = ub[size_t(k) * NU + t];
            MM::derivs(c, xl, ul, pk, k, N, srec);
        }
        // ---- U: K S_j, then diag U and the force blocks
        if (feedback) {
            if (lane < NU) {
                double kr[NX];
#pragma unroll
                for (int t = 0; t < NX; ++t) kr[t] = K[lane * NX + t];
                for (int l = 0; l < NX; ++l) {
                    double acc = 0.0;
#pragma unroll
                    for (int t = 0; t < NX; ++t) acc = fma(kr[t], Sc[cov_tri(t, l)], acc);
                    sT[lane * NX + l] = acc;
                }
            }
            wave_sync();
            if (lane < NU) {
                double acc = 0.0;
                for (int l = 0; l < NX; ++l) acc = fma(sT[lane * NX + l], K[lane * NX + l], acc);
                sU[lane] = acc;
            }
            if constexpr (NCF > 0) {
                if (lane < 6 * NCF) {
                    const int n = lane / 6, p = lane % 6, ra = p >= 3 ? 2 : (p >= 1 ? 1 : 0), rb = p - ra * (ra + 1) / 2;
                    const int row = M::uf(n) + ra, col = M::uf(n) + rb;
                    double acc = 0.0;
                    for (int l = 0; l < NX; ++l) acc = fma(sT[row * NX + l], K[col * NX + l], acc);
                    sU[NU + lane] = acc;
                }
            }
            wave_sync();
        }
        if (lane < NU) {
            const double v = feedback ? sU[lane] : 0.0;
            if (uo) uo[size_t(j) * NU + lane] = v;
            audit_take(umax, v, k * NU + lane);
        }
        if constexpr (NCF > 0) {
            // lane = contact * 5 + row of the pyramid: a = (+-1, 0, -ml), (0, +-1, -ml), (0, 0, -1)
            if (feedback && lane < 5 * NCF) {
                const int n = lane / 5, row = lane % 5;
                if (M::p_sw(pk, n) > 0.5) {
                    const double* f = ub + size_t(k) * NU + M::uf(n);
                    const double* C = sU + NU + 6 * n;
                    const double a0 = row == 0 ? 1.0 : (row == 1 ? -1.0 : 0.0), a1 = row == 2 ? 1.0 : (row == 3 ? -1.0 : 0.0);
                    const double a2 = row == 4 ? -1.0 : -ml;
                    const double w0 = fma(C[3], a2, fma(C[1], a1, C[0] * a0));      // C a, row by row, the columns ascending
                    const double w1 = fma(C[4], a2, fma(C[2], a1, C[1] * a0));
                    const double w2 = fma(C[5], a2, fma(C[4], a1, C[3] * a0));
                    const double spread = sqrt(fma(a2, w2, fma(a1, w1, a0 * w0)));
                    const double margin = -fma(a2, f[2], fma(a1, f[1], a0 * f[0]));
                    if (spread != 0.0) audit_take(zneg, -(margin / spread), (k * NCF + n) * 5 + row);
                }
            }
        }
        wave_sync();                                       // the record is in LDS, and the tile is free for f_u
        // ---- A: row m of A_k in registers
        const bool noise = ri != nullptr;
        if (feedback || noise) {
            for (int e = lane; e < NX * NU; e += kWave) sT[(e / NU) * NUP + e % NU] = MM::F_entry(c, srec, e / NU, NX + e % NU);
            wave_sync();
        }
        double a[NX];
        if (lane < NX) {
#pragma unroll
            for (int t = 0; t < NX; ++t) a[t] = MM::F_entry(c, srec, lane, t);
            if (feedback) {
                for (int r = 0; r < NU; ++r) {
                    const double br = sT[lane * NUP + r];
#pragma unroll
                    for (int t = 0; t < NX; ++t) a[t] = fma(br, K[r * NX + t], a[t]);
                }
            }
            // ---- G: where the chain of S'[i][lane] starts, i >= lane
            // (r2 runs over every row in every lane, the lanes below it masked: sT[r2][.] is then one word for the wave, a broadcast)
            for (int r2 = 0; r2 < NX; ++r2) {
                if (r2 < lane) continue;
                double g = r2 == lane && qi ? qi[r2] : 0.0;
                if (noise)
                    for (int r = 0; r < NU; ++r) g = fma(sT[r2 * NUP + r] * ri[r], sT[lane * NUP + r], g);
                Sn[cov_tri(r2, lane)] = g;
            }
        }
        wave_sync();                                       // f_u has been read: the tile is free for T
        // ---- T = A S_j, row by row
        if (lane < NX) {
            for (int l = 0; l < NX; ++l) {
                double acc = 0.0;
#pragma unroll
                for (int t = 0; t < NX; ++t) acc = fma(a[t], Sc[cov_tri(t, l)], acc);
                sT[lane * NX + l] = acc;
            }
        }
        wave_sync();
        // ---- S'[i][lane] += sum_l T[i][l] A[lane][l], i >= lane
        if (lane < NX) {
            for (int r2 = 0; r2 < NX; ++r2) {
                if (r2 < lane) continue;
                double acc = Sn[cov_tri(r2, lane)];
#pragma unroll
                for (int t = 0; t < NX; ++t) acc = fma(sT[r2 * NX + t], a[t], acc);
                Sn[cov_tri(r2, lane)] = acc;
            }
        }
        wave_sync();                                       // S_{j+1} is in LDS, and the record is free for knot k + 1
    }
    const int last = steps & 1;
    note(last, steps);
    AuditMax dtop{-inf, kAuditNoKey};
    double trace = 0.0;
    if (lane < NX) audit_take(dtop, sS[last][cov_tri(lane, lane)], lane);
    if (lane == 0)
        for (int t = 0; t < NX; ++t) trace += sS[last][cov_tri(t, t)];
    audit_merge(zneg);
    audit_merge(trmax);
    audit_merge(umax);
    audit_merge(dtop);
    dneg = audit_merge(dneg);
    if (lane == 0) {
        double* r = out + size_t(i) * kPolicyCovWords;
        const bool none = zneg.v != zneg.v || zneg.key == kAuditNoKey;
        r[0] = -zneg.v;
        r[1] = none ? -1.0 : double(zneg.key / (5 * (NCF > 0 ? NCF : 1)));
        r[2] = none ? -1.0 : double(zneg.key / 5 % (NCF > 0 ? NCF : 1));
        r[3] = none ? -1.0 : double(zneg.key % 5);
        r[4] = trmax.v;  r[5] = audit_index(trmax, 1, false);
        r[6] = trace;  r[7] = dtop.v;  r[8] = audit_index(dtop, 1, false);
        r[9] = umax.v;  r[10] = audit_index(umax, NU, false);  r[11] = audit_index(umax, NU, true);
        r[12] = -dneg;
        r[13] = double(steps);  r[14] = feedback ? rec[pol_words - 1] : 0.0;  r[15] = 0.0;
    }
}

// -----------------------------------------------------------------------------------------------------------------
// Cost-to-go at a measured state (sddp_value_at_device): the quadratic model of the value record `val` [B][vnodes][value_words(NX)]
// (sddp_enable_value: per node c | expected | Vx | Vxx) of instance b = first + i at node `node`, evaluated at
// delta = x_meas[i] - x_node[b]:
//     t[r] = sum_j Vxx[r][j] delta[j];   lin = sum_r Vx[r] delta[r];   quad = 0.5 * sum_r delta[r] t[r]
// every sum one FMA chain from 0.0 in ascending index order (include/sddp.h has the table of the eight output words), so that no
// lane mapping, range or slot changes a bit.  ok = 0 in the policy record `pol` [B][pol_words]: words 0 .. 4 are 0.0.
// One wavefront per instance, no model code: the constants argument is the launcher's (launch_waves) and is not read.  The node's
// Vxx is fetched once by coalesced loads into LDS with an odd row stride, so that the row products -- lane r owns row r, delta read
// as a broadcast -- are LDS reads without a bank conflict: 61 x 61 words of LDS traffic for 2 x 61 x 61 flops on srbd61, the reads
// are the cost.  The two short chains over r run in every lane on broadcasts; lane 0 stores.  Static LDS only, nothing of the slots'
// work buffers, plain vector stores to the caller's output alone.
template <class M, class... Tab>
__global__ __launch_bounds__(kWave) void value_at_kernel(ConstsArg<Tab...>, int N, int first, int count, int node,
                                                         const double* __restrict__ xs, const double* __restrict__ val, int vnodes,
                                                         const double* __restrict__ pol, int pol_words,
                                                         const double* __restrict__ x_meas, double* __restrict__ out) {
    constexpr int NX = M::NX, SV = NX | 1, VW = value_words(NX);
    static_assert(NX <= kWave, "one lane per row of Vxx");
    static_assert(sizeof(double) * (NX * SV + 3 * NX) <= 64 * 1024, "static LDS");
    __shared__ double sV[NX * SV];                         // Vxx, row stride SV
    __shared__ double sx[3 * NX];                          // Vx | delta | t
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= count) return;
    const int b = first + i;
    const double* rec = val + (size_t(b) * vnodes + node) * VW;
    const double* xk = xs + (size_t(b) * (N + 1) + node) * NX;
    const bool ok = pol[size_t(b) * pol_words + pol_words - 1] != 0.0;
    for (int e = lane; e < NX * NX; e += kWave) sV[(e / NX) * SV + e % NX] = rec[2 + NX + e];
    if (lane < NX) {
        sx[lane] = rec[2 + lane];
        sx[NX + lane] = x_meas[size_t(i) * NX + lane] - xk[lane];
    }
    wave_sync();
    if (lane < NX) {
        double t = 0.0;
        for (int j = 0; j < NX; ++j) t = fma(sV[lane * SV + j], sx[NX + j], t);
        sx[2 * NX + lane] = t;
    }
    wave_sync();
    double lin = 0.0, q2 = 0.0, dinf = 0.0;
    for (int r = 0; r < NX; ++r) {
        const double d = sx[NX + r];
        lin = fma(sx[r], d, lin);
        q2 = fma(d, sx[2 * NX + r], q2);
        dinf = nan_max(dinf, fabs(d));
    }
    if (lane == 0) {
        double* o = out + size_t(i) * kValueAtWords;
        const double quad = 0.5 * q2, c = rec[0], expected = rec[1];
        o[0] = ok ? ((c + expected) + lin) + quad : 0.0;
        o[1] = ok ? lin : 0.0;
        o[2] = ok ? quad : 0.0;
        o[3] = ok ? c : 0.0;
        o[4] = ok ? expected : 0.0;
        o[5] = dinf;
        o[6] = ok ? 1.0 : 0.0;
        o[7] = double(node);
    }
}

}  // namespace sddp
