// sddp_kernels_host.hpp -- the model-independent kernels of the library (queue order by history, class labels, receding-horizon shift,
// first-knot packing, the time budget's deadline stamp).  Included by sddp_api.hip only: they are not templates, so they must live in ONE translation unit.
#pragma once
#include <hip/hip_runtime.h>

#include "sddp.h"

namespace sddp {

// Queue order for the next launch: instances [first, first + count) sorted by the iteration count of their previous solve,
// longest first, never-solved ones before all others (longest-processing-time-first list scheduling: a launch ends with its
// slowest instance, so the slow ones must start first; a fleet's robots recur tick after tick and the previous count is the
// predictor at hand).  Counting sort in one workgroup; ties in arbitrary order (results do not depend on the order).
constexpr int kOrderBins = 258;   // key = min(hist, 256), -1 -> 257
__global__ __launch_bounds__(1024) void queue_order_kernel(int first, int count, const int* __restrict__ hist, int* __restrict__ order) {
    __shared__ int bins[kOrderBins];
    const int tid = threadIdx.x;
    for (int i = tid; i < kOrderBins; i += 1024) bins[i] = 0;
    __syncthreads();
    for (int i = tid; i < count; i += 1024) {
        const int h = hist[first + i];
        atomicAdd(&bins[h < 0 ? kOrderBins - 1 : (h > 256 ? 256 : h)], 1);
    }
    __syncthreads();
    if (tid == 0) {   // exclusive prefix, largest key first
        int run = 0;
        for (int k = kOrderBins - 1; k >= 0; --k) { const int n = bins[k]; bins[k] = run; run += n; }
    }
    __syncthreads();
    for (int i = tid; i < count; i += 1024) {
        const int h = hist[first + i];
        const int pos = atomicAdd(&bins[h < 0 ? kOrderBins - 1 : (h > 256 ? 256 : h)], 1);
        order[pos] = first + i;
    }
}

// Queue order 3 (class history): the key of an instance is the mean iteration count that earlier solves of its CLASS took on this
// handle (sddp_set_instance_classes: the caller's label of what kind of problem an instance is -- gait phase, command, ...), the
// initial cost (the key of queue order 2, already in `key`) breaking ties inside a class; classes never solved before sort first.
// cls_stat: [n_cls][2] = sum of iterations, solves.  The sum / count are read here and updated by class_update_kernel after the
// solve launch, both on the handle's stream.
__global__ __launch_bounds__(256) void class_key_kernel(int count, const int* __restrict__ idx, const int* __restrict__ cls, int n_cls,
                                                        const unsigned long long* __restrict__ cls_stat, double* __restrict__ key) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int c = cls[idx[i]];
    double mean = 1e6;                                         // unlabelled instance / class without history: first
    if (c >= 0 && c < n_cls && cls_stat[2 * c + 1] > 0) mean = double(cls_stat[2 * c]) / double(cls_stat[2 * c + 1]);
    const double j0 = key[i];                                  // initial cost; non-finite: stays first
    key[i] = (j0 == j0 && j0 < 1e300) ? mean + 1e-3 * j0 / (fabs(j0) + 1e9) : j0;      // tie-break in (-1e-3, 1e-3), monotone in j0
}
__global__ __launch_bounds__(256) void class_update_kernel(int first, int count, const int* __restrict__ cls, int n_cls,
                                                           const sddp_stats* __restrict__ st, unsigned long long* __restrict__ cls_stat) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int c = cls[first + i];
    if (c < 0 || c >= n_cls) return;
    atomicAdd(&cls_stat[2 * c], (unsigned long long)st[first + i].iters);
    atomicAdd(&cls_stat[2 * c + 1], 1ull);
}

// The class statistics of a handle with resumable solves (sddp_enable_resume): an instance is counted once, with its total iteration
// count, by the launch in which it leaves status 1.  A fresh solve launch (cont = 0) skips the instances it leaves resumable; a
// continue launch counts the instances it resumed (`ran`, zeroed before the launch) and finished.
__global__ __launch_bounds__(256) void class_update_resume_kernel(int first, int count, const int* __restrict__ cls, int n_cls,
                                                                  const sddp_stats* __restrict__ st, unsigned long long* __restrict__ cls_stat,
                                                                  const int* __restrict__ resumable, const int* __restrict__ ran, int cont) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int b = first + i, c = cls[b];
    if (c < 0 || c >= n_cls) return;
    if (resumable[b] == 1 || (cont && ran[b] != 1)) return;
    atomicAdd(&cls_stat[2 * c], (unsigned long long)st[b].iters);
    atomicAdd(&cls_stat[2 * c + 1], 1ull);
}

// Auto classes (sddp_enable_auto_classes): the label of every instance of [first, first + count), computed from the parameter tensor
// of the launch, in front of its key pre-pass (what workload.schedule_classes states in numpy):
//   sw[k][j] = P[b][k][col_sw[j]] > 0.5 (a NaN is "not in stance"), stance0 = 2 sw[0][0] + sw[0][1],
//   first_change = smallest k in 1..N with sw[k] != sw[0], N + 1 if none, cmd(v) = 0 / 1 / 2 for |v| <= 1e-12 / v > 1e-12 / v < -1e-12,
//   label = ((stance0 (N + 2) + first_change) 3 + cmd(P[b][N][col_cmd0])) 3 + cmd(P[b][N][col_cmd1])      in [0, 36 (N + 2))
// One wavefront per instance, four per workgroup: lane l looks at node 64 c + l of chunk c and compares its two switches with node 0's,
// lane 0's of chunk 0; the first set bit of the first non-empty ballot is first_change (node 0 never differs from itself).  np: the
// handle's parameter row width.  About N + 1 cache lines per instance are touched, two words of each.
// (the label of ONE instance, by one whole wavefront: the range kernel and the masked one below call it)
__device__ __forceinline__ void class_label_instance(int N, int np, int col_cmd0, int col_cmd1, int col_sw0, int col_sw1, int b, int lane,
                                                     const double* __restrict__ P, int* __restrict__ cls) {
    const double* Pb = P + size_t(b) * (N + 1) * np;
    int s0 = 0, first_change = N + 1;
    for (int k0 = 0; k0 <= N; k0 += 64) {
        const int k = k0 + lane;
        int s = 0;
        if (k <= N) {
            const double* p = Pb + size_t(k) * np;
            s = (p[col_sw0] > 0.5 ? 2 : 0) + (p[col_sw1] > 0.5 ? 1 : 0);
        }
        if (k0 == 0) s0 = __shfl(s, 0);
        const unsigned long long differs = __ballot(k <= N && s != s0);
        if (differs) { first_change = k0 + __ffsll(differs) - 1; break; }      // (uniform: every lane sees the same ballot)
    }
    if (lane == 0) {
        const double vx = Pb[size_t(N) * np + col_cmd0], vy = Pb[size_t(N) * np + col_cmd1];
        const int cx = vx > 1e-12 ? 1 : (vx < -1e-12 ? 2 : 0), cy = vy > 1e-12 ? 1 : (vy < -1e-12 ? 2 : 0);
        cls[b] = ((s0 * (N + 2) + first_change) * 3 + cx) * 3 + cy;
    }
}
__global__ __launch_bounds__(256) void class_label_kernel(int N, int np, int col_cmd0, int col_cmd1, int col_sw0, int col_sw1, int first, int count,
                                                          const double* __restrict__ P, int* __restrict__ cls) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= count) return;                                    // (the whole wavefront)
    class_label_instance(N, np, col_cmd0, col_cmd1, col_sw0, col_sw1, first + i, lane, P, cls);
}

// ---- masked launches (sddp_*_masked_device): mask[i] != 0 selects instance first + i of the range; every other instance of it is
// handed out by no queue and written by no kernel below.  A mask is `count` words that are only compared with 0: there is no index in
// it to validate, so whatever it holds no kernel here reads or writes outside [first, first + count).
// The solve kernels take queue positions i = atomicAdd(qhead, 1) while i < count and solve order[i].  A masked launch is therefore an
// order array whose first count - n_selected entries are the unselected instances and a queue head that STARTS at count - n_selected:
// the kernels below build exactly that, and the solve kernels do not know.
//
// auto classes: the labels of the selected instances alone (class_label_kernel's, by the same code)
__global__ __launch_bounds__(256) void class_label_masked_kernel(int N, int np, int col_cmd0, int col_cmd1, int col_sw0, int col_sw1, int first,
                                                                 int count, const int* __restrict__ mask, const double* __restrict__ P,
                                                                 int* __restrict__ cls) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= count || mask[i] == 0) return;                    // (the whole wavefront)
    class_label_instance(N, np, col_cmd0, col_cmd1, col_sw0, col_sw1, first + i, lane, P, cls);
}
// the head of a masked launch's queue, by ONE thread: qhead = count - n_selected, and sel = n_selected | queue start
// (SDDP_BUF_SELECTED; null: a policy launch, which leaves the words of the last solve launch alone).  Ordinary vector stores.
__device__ __forceinline__ void write_mask_head(int count, int n_selected, int* __restrict__ qhead, int* __restrict__ sel) {
    *qhead = count - n_selected;
    if (sel) { sel[0] = n_selected; sel[1] = count - n_selected; }
}
// queue order 0 under a mask, and the order of a masked policy launch: a STABLE partition in one workgroup -- the unselected
// instances in index order at [0, count - n_selected), the selected ones in index order behind them.  Thread t owns the contiguous
// chunk [t per, (t + 1) per) of the range; an inclusive scan of the chunks' selected counts gives every chunk its two write positions,
// and its last word is n_selected: the kernel writes the queue head itself.
__global__ __launch_bounds__(1024) void queue_index_masked_kernel(int first, int count, const int* __restrict__ mask, int* __restrict__ order,
                                                                  int* __restrict__ qhead, int* __restrict__ sel) {
    __shared__ int part[1024];
    const int tid = threadIdx.x;
    const int per = (count + 1023) / 1024;
    const int lo = min(tid * per, count), hi = min(lo + per, count);
    int n = 0;
    for (int i = lo; i < hi; ++i) n += mask[i] != 0 ? 1 : 0;
    part[tid] = n;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    const int n_uns = count - part[1023];
    if (tid == 0) write_mask_head(count, part[1023], qhead, sel);
    int s = part[tid] - n;                                     // selected instances in front of this chunk
    for (int i = lo; i < hi; ++i) {
        if (mask[i] != 0) order[n_uns + s++] = first + i;
        else order[i - s] = first + i;
    }
}
// queue order 1 under a mask: queue_order_kernel's counting sort with one more bin, in front of all others, for the unselected
// instances: the partition is a bin of its own and no property of a key, and that bin's count gives the queue head
__global__ __launch_bounds__(1024) void queue_order_masked_kernel(int first, int count, const int* __restrict__ hist, const int* __restrict__ mask,
                                                                  int* __restrict__ order, int* __restrict__ qhead, int* __restrict__ sel) {
    __shared__ int bins[kOrderBins + 1];
    const int tid = threadIdx.x;
    for (int i = tid; i < kOrderBins + 1; i += 1024) bins[i] = 0;
    __syncthreads();
    for (int i = tid; i < count; i += 1024) {
        const int h = hist[first + i];
        atomicAdd(&bins[mask[i] == 0 ? kOrderBins : (h < 0 ? kOrderBins - 1 : (h > 256 ? 256 : h))], 1);
    }
    __syncthreads();
    if (tid == 0) {   // exclusive prefix, the unselected bin, then the largest key first
        write_mask_head(count, count - bins[kOrderBins], qhead, sel);
        int run = 0;
        for (int k = kOrderBins; k >= 0; --k) { const int n = bins[k]; bins[k] = run; run += n; }
    }
    __syncthreads();
    for (int i = tid; i < count; i += 1024) {
        const int h = hist[first + i];
        const int pos = atomicAdd(&bins[mask[i] == 0 ? kOrderBins : (h < 0 ? kOrderBins - 1 : (h > 256 ? 256 : h))], 1);
        order[pos] = first + i;
    }
}
// queue orders 2 and 3 under a mask: the keys of the whole range are evaluated as for a range launch (the unselected instances' keys
// are computed and discarded here: the model's key kernel stays as it is), then mapped so that the descending sort IS the partition:
// an unselected instance gets +infinity, a selected one its key clamped into [-DBL_MAX, DBL_MAX] -- a non-finite initial cost
// ("stays first" in a range launch: +infinity, or NaN) becomes DBL_MAX: first among the SELECTED, and strictly behind every
// unselected instance.  No selected key can tie with the sentinel.
__global__ __launch_bounds__(256) void masked_key_kernel(int count, const int* __restrict__ mask, double* __restrict__ key) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    constexpr double kMax = 1.7976931348623157e308;
    const double k = key[i];
    key[i] = mask[i] == 0 ? __builtin_huge_val() : (k == k ? fmin(fmax(k, -kMax), kMax) : kMax);
}
// the head of a masked launch's queue for the orders whose order array comes out of the sort (2, 3): one workgroup counts the mask
__global__ __launch_bounds__(256) void mask_head_kernel(int count, const int* __restrict__ mask, int* __restrict__ qhead, int* __restrict__ sel) {
    __shared__ int part[256];
    int n = 0;
    for (int i = threadIdx.x; i < count; i += 256) n += mask[i] != 0 ? 1 : 0;
    part[threadIdx.x] = n;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) write_mask_head(count, part[0], qhead, sel);
}
// the class statistics behind a masked launch: class_update_kernel / class_update_resume_kernel (resumable != null) for the selected
// instances alone
__global__ __launch_bounds__(256) void class_update_masked_kernel(int first, int count, const int* __restrict__ mask, const int* __restrict__ cls,
                                                                  int n_cls, const sddp_stats* __restrict__ st,
                                                                  unsigned long long* __restrict__ cls_stat, const int* __restrict__ resumable,
                                                                  const int* __restrict__ ran, int cont) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count || mask[i] == 0) return;
    const int b = first + i, c = cls[b];
    if (c < 0 || c >= n_cls) return;
    if (resumable && (resumable[b] == 1 || (cont && ran[b] != 1))) return;
    atomicAdd(&cls_stat[2 * c], (unsigned long long)st[b].iters);
    atomicAdd(&cls_stat[2 * c + 1], 1ull);
}

// sddp_add_class_stats: another handle's history (sums of iterations, solves; both additive) onto the words [2 first_class, ...) of
// this one's, on the handle's stream like class_update_kernel
__global__ __launch_bounds__(256) void class_stats_add_kernel(int words, const unsigned long long* __restrict__ in,
                                                              unsigned long long* __restrict__ cls_stat) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < words) cls_stat[i] += in[i];
}

// sddp_unfinished_count: how many instances of [first, first + count) can be continued (flag 1).  One workgroup.
__global__ __launch_bounds__(256) void unfinished_count_kernel(int first, int count, const int* __restrict__ resumable, int* __restrict__ out) {
    __shared__ int part[256];
    int n = 0;
    for (int i = threadIdx.x; i < count; i += 256) n += resumable[first + i] == 1 ? 1 : 0;
    part[threadIdx.x] = n;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = part[0];
}

// Time budget (sddp_set_time_budget): one thread, in front of the first kernel of a solve or continue launch sequence on the handle's
// stream.  w[0] = the 100 MHz constant-rate clock now, w[1] = the deadline, `ticks` later: what the RESUME solve kernels compare
// their own clock reads with (sddp_kernels.hpp deadline_passed).  The budget so counts device time from the moment the stream
// reaches the launch sequence; the host clock plays no part.  Ordinary vector stores.
__global__ __launch_bounds__(64) void deadline_stamp_kernel(unsigned long long* __restrict__ w, unsigned long long ticks) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const unsigned long long start = wall_clock64();
    w[0] = start;
    w[1] = start + ticks;
}

// what an MPC tick applies: the first input u_0 and the state the plan expects next, x_1, of every instance, packed
// [B][nu + nx] (+ cost, iterations, status as three more doubles) for one small copy to the host instead of the whole trajectories
__global__ __launch_bounds__(256) void first_knot_kernel(int N, int B, int nx, int nu, const double* __restrict__ xs,
                                                         const double* __restrict__ us, const sddp_stats* __restrict__ st,
                                                         double* __restrict__ out) {
    const int w = nu + nx + 3;
    for (size_t e = size_t(blockIdx.x) * 256 + threadIdx.x; e < size_t(B) * w; e += size_t(gridDim.x) * 256) {
        const int b = int(e / w), j = int(e % w);
        double v;
        if (j < nu) v = us[size_t(b) * N * nu + j];
        else if (j < nu + nx) v = xs[(size_t(b) * (N + 1) + 1) * nx + (j - nu)];
        else v = j == nu + nx ? st[b].cost : (j == nu + nx + 1 ? double(st[b].iters) : double(st[b].status));
        out[e] = v;
    }
}

// The record an instance-sharded fleet exchanges after a launch: per instance
//   mode 0: x [N+1][nx] | u [N][nu] | cost | iterations            ((N+1) nx + N nu + 2 doubles: the whole plan)
//   mode 1: u_0 [nu] | x_1 [nx] | cost | iterations                (nu + nx + 2 doubles: what a closed loop applies next)
//   mode 2: mode 1 | kff_0 [nu] | K_0 [nu][nx]                       (+ nu (nx + 1): the first knot's feedback policy, from the policy
//           buffer `pol` [B][pol_words] of sddp_policy_range_device)
// written [count][words] contiguous into the collective's send buffer: one kernel, whole-wave contiguous stores (the trajectories
// of consecutive instances are consecutive in xs / us, so the loads are contiguous runs too).
__global__ __launch_bounds__(256) void pack_records_kernel(int N, int nx, int nu, int first, int count, int mode,
                                                           const double* __restrict__ xs, const double* __restrict__ us,
                                                           const sddp_stats* __restrict__ st, double* __restrict__ out,
                                                           const double* __restrict__ pol, int pol_words) {
    const int nxw = mode == 0 ? (N + 1) * nx : nx, nuw = mode == 0 ? N * nu : nu;
    const int w = nxw + nuw + 2 + (mode == 2 ? nu * (nx + 1) : 0);
    for (size_t e = size_t(blockIdx.x) * 256 + threadIdx.x; e < size_t(count) * w; e += size_t(gridDim.x) * 256) {
        const int i = int(e / w), j = int(e % w), b = first + i;
        double v;
        if (mode == 0) {
            if (j < nxw) v = xs[size_t(b) * nxw + j];
            else if (j < nxw + nuw) v = us[size_t(b) * nuw + (j - nxw)];
            else v = j == nxw + nuw ? st[b].cost : double(st[b].iters);
        } else {
            if (j < nu) v = us[size_t(b) * N * nu + j];
            else if (j < nu + nx) v = xs[(size_t(b) * (N + 1) + 1) * nx + (j - nu)];
            else if (j < nu + nx + 2) v = j == nu + nx ? st[b].cost : double(st[b].iters);
            else v = pol[size_t(b) * pol_words + (j - nu - nx - 2)];
        }
        out[e] = v;
    }
}

// The feedback policy between two ticks of a fleet (sddp_apply_policy_device, sddp_apply_policy_knot_device):
// u[i] = u_k[b] + K_k[b] (x_meas[i] - x_k[b]) for the instances b = first + i of a range, k = `knot` < the knots kept, from the policy
// buffer (per knot: kff [nu] then K [nu][nx] row-major) and the handle's xs / us.
// An instance without a policy (ok = 0: zero gains) gets u_k[b] exactly.
// A B x nu x nx mat-vec: nu lanes per instance, one row of K_k each (nx <= 61 terms, fp64 FMA chain); no LDS.
__global__ __launch_bounds__(256) void apply_policy_kernel(int N, int nx, int nu, int first, int count, int knot, const double* __restrict__ xs,
                                                           const double* __restrict__ us, const double* __restrict__ pol, int pol_words,
                                                           const double* __restrict__ x_meas, double* __restrict__ u_out) {
    for (size_t e = size_t(blockIdx.x) * 256 + threadIdx.x; e < size_t(count) * nu; e += size_t(gridDim.x) * 256) {
        const int i = int(e / nu), r = int(e % nu), b = first + i;
        const double* K = pol + size_t(b) * pol_words + size_t(knot) * nu * (nx + 1) + nu + size_t(r) * nx;
        const double* x0 = xs + (size_t(b) * (N + 1) + knot) * nx;
        const double* xm = x_meas + size_t(i) * nx;
        double acc = us[(size_t(b) * N + knot) * nu + r];
        // ok = 0 (the record's last word): there is no feedback -- u_k itself, whatever x_k holds (0 x NaN is not 0)
        if (pol[size_t(b) * pol_words + pol_words - 1] != 0.0)
            for (int j = 0; j < nx; ++j) acc = fma(K[j], xm[j] - x0[j], acc);
        u_out[e] = acc;
    }
}

// diagnostic (sddp_debug_poison_lds): a workgroup that owns a CU's whole LDS and fills it with NaNs.  What a kernel finds in LDS
// is whatever the previous one left there; after this one a read of a word the kernel never wrote cannot pass a parity test.
__global__ __launch_bounds__(256) void poison_lds_kernel(int words, int* __restrict__ sink) {
    extern __shared__ __attribute__((aligned(16))) double lds_all[];
    for (int e = threadIdx.x; e < words; e += 256) lds_all[e] = __builtin_nan("");
    __syncthreads();
    if (lds_all[threadIdx.x] == 1.0) *sink = 1;          // (never true: keeps the stores)
}

constexpr int kAdvanceWords = 4096;   // longest array advance_kernel shifts in one workgroup: (N+1) * max(nx, np) words

// receding-horizon tick on the device: shift parameters and warm start by one knot (one workgroup per instance; every element
// is read before the barrier and written after it, so the in-place shift is safe)
// (instance b by one whole workgroup; row `src` of p_last / x0_new is its new last parameter row and its new initial state)
__device__ __forceinline__ void advance_instance(int N, int nx, int nu, int np, double* __restrict__ P, double* __restrict__ xs,
                                                 double* __restrict__ us, double* __restrict__ x0, const double* __restrict__ p_last,
                                                 const double* __restrict__ x0_new, const int b, const int src) {
    const int tid = threadIdx.x;
    double* Pb = P + size_t(b) * (N + 1) * np;
    double* xb = xs + size_t(b) * (N + 1) * nx;
    double* ub = us + size_t(b) * N * nu;
    constexpr int R = kAdvanceWords / 256;                 // elements per thread and array
    double rp[R], rx[R], ru[R];
    const int np_all = (N + 1) * np, nx_all = (N + 1) * nx, nu_all = N * nu;
#pragma unroll
    for (int t = 0; t < R; ++t) {
        const int e = tid + t * 256;
        rp[t] = e < np_all ? (e + np < np_all ? Pb[e + np] : p_last[size_t(src) * np + (e - N * np)]) : 0.0;
        rx[t] = e < nx_all ? xb[e + nx < nx_all ? e + nx : e] : 0.0;
        ru[t] = e < nu_all ? ub[e + nu < nu_all ? e + nu : e] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < R; ++t) {
        const int e = tid + t * 256;
        if (e < np_all) Pb[e] = rp[t];
        if (e < nx_all) xb[e] = rx[t];
        if (e < nu_all) ub[e] = ru[t];
    }
    if (tid < nx) x0[size_t(b) * nx + tid] = x0_new[size_t(src) * nx + tid];
}
__global__ __launch_bounds__(256) void advance_kernel(int N, int nx, int nu, int np, double* __restrict__ P, double* __restrict__ xs,
                                                      double* __restrict__ us, double* __restrict__ x0, const double* __restrict__ p_last,
                                                      const double* __restrict__ x0_new) {
    advance_instance(N, nx, nu, np, P, xs, us, x0, p_last, x0_new, blockIdx.x, blockIdx.x);
}
// sddp_advance_masked_device: the same tick for the selected instances of [first, first + count) alone, from device rows [count][np]
// / [count][nx] indexed like the mask; and (resumable != null: sddp_enable_resume) their resume flags cleared, as the invalidation
// behind sddp_advance does for the whole batch.  An unselected instance's workgroup leaves before the barrier, whole.
__global__ __launch_bounds__(256) void advance_masked_kernel(int N, int nx, int nu, int np, double* __restrict__ P, double* __restrict__ xs,
                                                             double* __restrict__ us, double* __restrict__ x0, const double* __restrict__ p_last,
                                                             const double* __restrict__ x0_new, int first, const int* __restrict__ mask,
                                                             int* __restrict__ resumable) {
    const int i = blockIdx.x;
    if (mask[i] == 0) return;                              // (the whole workgroup)
    advance_instance(N, nx, nu, np, P, xs, us, x0, p_last, x0_new, first + i, i);
    if (resumable && threadIdx.x == 0) resumable[first + i] = 0;
}

}  // namespace sddp
