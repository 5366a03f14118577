// sddp_kernels.hpp -- the DDP engine as CDNA4 HIP kernels (gfx950, fp64, wave64).
//
// Replaces the arithmetic the reference delegates to the external `pyddp.DdpSolver.solve()` (reference
// python/ddp.py:101): derivative evaluation at every knot, backward Riccati sweep, forward line-search rollout,
// acceptance / termination -- see DESIGN.md "Algorithm" for the exact iteration (it is the one restated in
// oracle/ddp.py).
//
// Mapping (DESIGN.md "Kernel design"):
//   * one 64-lane wavefront (= one workgroup) per MPC instance, persistent over all DDP iterations: no host
//     round trip and no inter-workgroup traffic inside a solve;
//   * derivative phase: one LANE per knot (scalar register code, all knots of the horizon at once);
//   * Riccati sweep: serial over knots; the Vxx / [fx fu] / Q tiles of the current knot live in LDS, one lane per
//     tile element, Quu solved by a register-resident Gauss-Jordan (one lane per right-hand-side column),
//     small reductions by wavefront shuffles;
//   * line search: one LANE per step length alpha_j = alpha_0 * factor^j -- the whole backtracking ladder is
//     rolled out in one pass, the largest acceptable alpha is picked by a ballot;
//   * the knot sequence (trajectory, parameters, gains, derivative records) is read and written coalesced,
//     one knot per wave-wide access, and stays L2-resident (no MFMA: 13x13 / 6x6 tiles are too small to win).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "sddp_models.hpp"

namespace sddp {

constexpr int kWave = 64;
constexpr int kSlots = 6;   // line-search candidates whose trajectories are kept per pass (one-wave kernel)
constexpr int kScal = 24;  // doubles per instance in the scratch `scal` record (test kernels / diagnostic stamps)
// the record sizes of the kernels of sddp_inspect.hpp that sddp_api.hip reports, here so that it needs none of that file:
constexpr int kStationarityWords = 8;      // doubles per record of the stationarity certificate (sddp.h sddp_stationarity_words)
constexpr int kCostTermsWords = 16, kCostTermsFamilies = 13;   // ... of the cost breakdown, and its families (sddp.h sddp_cost_terms_words)
constexpr int kParamGradientWords = 8;     // ... of the parameter sensitivities (sddp.h sddp_param_gradient_words)
// ... of the constant sensitivities (sddp.h sddp_const_gradient_words): the kConstGradientCols columns, 6 words, 2 reserved; and the
// dynamic LDS of its kernel: the tile of addends [N + 1][kConstGradientCols] and one row for the columns' |C theta|
constexpr int kConstGradientWords = 40;
// doubles per node of a value record (sddp.h sddp_value_words): c | expected | Vx [nx] | Vxx [nx][nx]; and of one sddp_value_at_device row
__host__ __device__ constexpr int value_words(int nx) { return nx * nx + nx + 2; }
constexpr int kValueAtWords = 8;
constexpr int kPolicyCovWords = 16;        // ... of the plan uncertainty (sddp.h sddp_policy_covariance_words, SDDP_POLICY_COV_WORDS there)
constexpr size_t const_gradient_lds(int N) { return sizeof(double) * (size_t(N + 1) + 1) * kConstGradientCols; }

// Diagnostic build only (-DSDDP_STAMPS): per-phase shader-cycle sums, written to `scal`; never in the shipped library.
#ifdef SDDP_STAMPS
#define SDDP_T_DECL unsigned long long T_[kScal] = {0}; unsigned long long t_last_ = clock64();
#define SDDP_T_ARG , unsigned long long* T_, unsigned long long& t_last_
#define SDDP_T_PASS , T_, t_last_
#define SDDP_TICK(i) { const unsigned long long t_ = clock64(); T_[i] += t_ - t_last_; t_last_ = t_; }
#elif defined(SDDP_MARKS)
// Listing build only (-DSDDP_MARKS, `hipcc -S`): the phase boundaries as assembler comments, for tools/isa_phase_mix.py.  No
// instruction is emitted; the volatile asm only keeps the compiler from moving code across a boundary.
#define SDDP_T_DECL
#define SDDP_T_ARG
#define SDDP_T_PASS
#define SDDP_TICK(i) asm volatile("; SDDP_MARK " #i ::: "memory");
#else
#define SDDP_T_DECL
#define SDDP_T_ARG
#define SDDP_T_PASS
#define SDDP_TICK(i)
#endif

// THE layout of the packed buffer `hist` (SolveArgs::hist, sddp_handle::hist): the iteration counts [B], padded to an even count of
// ints so that the slot clocks [wslots][2] of uint64 behind them are 8-byte aligned.
struct HistLayout {
    __host__ __device__ static constexpr int counts(int B) { return (B + 1) & ~1; }      // ints in front of the slot clocks
    __host__ __device__ static constexpr size_t bytes(int B, int wslots) {               // (a handle has at least one slot)
        return size_t(counts(B)) * sizeof(int) + size_t(wslots > 1 ? wslots : 1) * 2 * sizeof(unsigned long long);
    }
};
static_assert(HistLayout::counts(1) == 2 && HistLayout::counts(2) == 2 && HistLayout::counts(3) == 4, "the counts are padded to an even count");
static_assert(HistLayout::bytes(1, 1) == 24 && HistLayout::bytes(2, 0) == 24 && HistLayout::bytes(3, 4) == 80, "counts, then 16 bytes a slot");

struct SolveArgs {
    DevConsts c;
    sddp_options o;
    int N, B;
    const double* x0;   // [B][NX]
    const double* P;    // [B][N+1][NP]
    double* xs;         // [B][N+1][NX]  current iterate (in: warm start, out: solution)
    double* us;         // [B][N][NU]
    double* xn;         // [B][N+1][NX]  candidate (4-wave kernels, single-phase test kernels)
    double* un;         // [B][N][NU]
    double* xc;         // [B][2][kSlots][N+1][NX]  line-search candidates of the one-wave kernel: the first kSlots step lengths of
    double* uc;         // [B][2][kSlots][N][NU]    a pass each keep their trajectory; two sets, written alternately
    double* dft;        // [B][N][NX]    defects d_{k+1} stored at k
    double* gains;      // [B][N][NU*(NX+1)]  kff (NU) then K (NU x NX, row-major)
    double* rec;        // [B][N+1][NREC]
    sddp_stats* stats;  // [B]
    double* scal;       // [B][kScal] (test kernels / diagnostic stamps)
    double alpha;       // forward test kernel only
    double mu;          // backward test kernel only
    // work queue (solve kernels).  The launch covers `count` instances; the grid is the resident workgroups ("slots"), at most
    // `count` of them.  qhead == nullptr: workgroup w solves instance first + w (grid == count).  Otherwise every workgroup
    // takes queue positions i = atomicAdd(qhead, 1) until i >= count and solves instance order[i] (order == nullptr:
    // first + i).  The work buffers xn/un/xc/uc/dft/gains/rec are per SLOT (indexed by blockIdx.x), x0/P/xs/us/stats/scal/hist
    // per instance.
    // The one-wave test kernels (backward_kernel, forward_kernel) index by blockIdx.x and B and never read `first` as a range: to
    // them first != 0 says "closed gaps" (sddp_debug_set_phase_mode: the sweep and the rollout run their has_gap = false path).
    // The flag rides here because the struct must not grow (static_assert below); no other kernel is launched with it set.
    int first, count;
    int* qhead;
    const int* order;   // [count] absolute instance indices, or nullptr
    int* hist;          // [B] iterations of the last solve of each instance (-1: never solved): the queue-order key; behind it (no
                        // kernel argument of its own: the solve kernels live on their scalar registers; HistLayout) the slot clocks
                        // [slots][2]: constant-rate clock (wall_clock64, 100 MHz) when a slot started its first instance and when it
                        // found the queue empty -- how long a launch drains (bench.py drain_frac)
    __device__ __forceinline__ unsigned long long* slot_clock(int slot) const {
        return reinterpret_cast<unsigned long long*>(hist + HistLayout::counts(B)) + 2 * slot;
    }
};
// the size of the kernel-argument segment is part of the solve kernels' code (see ResumeArgs): a new field goes elsewhere
static_assert(sizeof(SolveArgs) == 584, "SolveArgs must not grow or shrink: it changes the register allocation of the solve kernels");

// Resumable solves (sddp_enable_resume): what the RESUME instantiations of the solve kernels take beside SolveArgs, as a kernel
// argument of their own behind it.  (Not fields of SolveArgs: the size of the kernel-argument segment decides how the compiler
// widens the scalar loads of the arguments, and 24 bytes more moved the register allocation of the ordinary one-wave kernels.)
// Both buffers are per INSTANCE: slots are reused within a launch and differ from one launch to the next.
// THE layout of the packed buffer `resumable` (ResumeArgs::resumable, sddp_handle::Resume::resumable), in ints: three rows of B, one
// word, and (padded to 8 bytes) the two uint64 clock words of the time budget.  The rows take the type of B they are asked with: the
// kernels index in int, as they always did, the host in size_t.
struct ResumeLayout {
    template <class I> __host__ __device__ static constexpr I flags(I) { return 0; }            // 1: instance b can be continued
    template <class I> __host__ __device__ static constexpr I lanes(I B) { return B; }          // the 4-wave kernel's stored `guess`
    template <class I> __host__ __device__ static constexpr I ran(I B) { return 2 * B; }        // 1: resumed by the launch in flight
    template <class I> __host__ __device__ static constexpr I count_word(I B) { return 3 * B; } // result of sddp_unfinished_count
    __host__ __device__ static constexpr size_t clock_words(size_t B) { return (count_word(B) + 2) & ~size_t(1); }
    __host__ __device__ static constexpr size_t ints(size_t B) { return clock_words(B) + 2 * sizeof(unsigned long long) / sizeof(int); }
};
// pinned at an odd, an even and an odd B again: rows disjoint, the count word behind them, the clock words aligned and clear of it;
// and the offsets are what every place of use once wrote out (B | 2 B | 3 B | (3 B + 2) & ~1)
constexpr bool resume_layout_is(int B, int lanes, int ran, int count_word, size_t clock_words, size_t ints) {
    using L = ResumeLayout;
    return L::flags(B) == 0 && L::lanes(B) == lanes && L::ran(B) == ran && L::count_word(B) == count_word
        && L::clock_words(size_t(B)) == clock_words && L::ints(size_t(B)) == ints
        && L::flags(B) + B <= L::lanes(B) && L::lanes(B) + B <= L::ran(B) && L::ran(B) + B <= L::count_word(B)
        && size_t(L::count_word(B)) + 1 <= L::clock_words(size_t(B)) && L::clock_words(size_t(B)) % 2 == 0
        && L::lanes(size_t(B)) == size_t(lanes) && L::ran(size_t(B)) == size_t(ran) && L::count_word(size_t(B)) == size_t(count_word);
}
static_assert(resume_layout_is(1, 1, 2, 3, 4, 8) && resume_layout_is(2, 2, 4, 6, 8, 12) && resume_layout_is(3, 3, 6, 9, 10, 14),
              "the layout of ResumeArgs::resumable moved");

struct ResumeArgs {
    double* carry;      // [B][N][NX]  the defects (the slot's dft) of an instance whose solve was cut at max_iters (status 1)
    int* resumable;     // ResumeLayout.  flag: the instance's last solve ended with status 1 and nothing of it was rewritten since;
                        // ran: class history (sddp_api.hip launch_class_update)
    int cont;           // 1: a continue launch (sddp_continue_*): resumable instances are taken up where they stopped, every other
                        // instance is left as it is
    int budget_iters;   // time budget (sddp_set_time_budget).  < 0: not armed -- the clock and the clock words are never read.
                        // >= 0: armed, and the iterations every instance that THIS launch runs is owed before the deadline is
                        // consulted (min_iters).  It sits in the struct's tail padding: the argument segment keeps its size
    __device__ __forceinline__ int& flag(int b) const { return resumable[b]; }
    __device__ __forceinline__ int& lane(int B, int b) const { return resumable[ResumeLayout::lanes(B) + b]; }
    __device__ __forceinline__ int& ran(int B, int b) const { return resumable[ResumeLayout::ran(B) + b]; }
    // the clock words: the constant-rate clock at the start of the launch sequence and the deadline, written by
    // deadline_stamp_kernel (sddp_kernels_host.hpp) in front of the launch on the same stream
    __device__ __forceinline__ const unsigned long long* clock_words(int B) const {
        return reinterpret_cast<const unsigned long long*>(resumable + ResumeLayout::clock_words(B));
    }
};
static_assert(sizeof(ResumeArgs) == 24, "ResumeArgs must not grow: budget_iters lives in what was padding");
struct NoResume {};    // stands in its place in the ordinary instantiations: nothing is passed, nothing is read
// Time budget: has the launch's deadline passed?  Called in the RESUME instantiations only, and only while the budget is armed.  The
// deadline is constant for the whole launch (an earlier kernel of the stream wrote it) and its address is wave-uniform, so it is
// read through the constant address space like a table row (row_of): a scalar load, no vector register.  wall_clock64 is the scalar
// read of the 100 MHz constant-rate clock the slot clocks use.
__device__ __forceinline__ bool deadline_passed(const ResumeArgs& R, const int B) {
    typedef const unsigned long long __attribute__((address_space(4))) * WordPtr;
    return wall_clock64() >= ((WordPtr)R.clock_words(B))[1];
}
// Iteration log (sddp_enable_iteration_log): one record of kLogWords doubles per line search an instance ran, in the layout of the
// first 12 words of the C oracle's trace record (oracle/c/ddp_engine.inc) and four words more:
//   0 J of the iterate the search starts from | 1 A1 | 2 B2 | 3 rho | 4 gap | 5 expected | 6 accepted alpha (0: none) |
//   7 accepted J (0: none) | 8 theta of this sweep | 9 mu of this sweep (after any bump) | 10 candidates tried (index of the accepted
//   step length in the ladder + 1, or the ladder's length) | 11 slack | 12 iters after this search | 13 rollouts after this search
//   (cumulative, as sddp_stats.rollouts) | 14 mu bumps in this sweep | 15 reserved, 0
// The LOG instantiations of the solve kernels (always RESUME instantiations as well: a continue launch appends to the records of
// the cut solve) take it as a kernel argument of their own behind ResumeArgs.  Both buffers are per INSTANCE.
constexpr int kLogWords = SDDP_LOG_WORDS;
static_assert(kLogWords == 16, "log_record writes 16 words");
struct LogArgs {
    double* log;        // [B][rows][kLogWords]
    int* count;         // [B]  records written; saturates at rows (later searches are not logged)
    int rows;
};
struct NoLog {};
// what an instance's solve keeps for its records: the records written so far, the mu bumps of the sweep, the step lengths tried
template <bool LOG> struct LogState {};
template <> struct LogState<true> { int n = 0, bumps = 0, tried = 0; };
// one record, by the calling lane alone: 16 contiguous doubles
__device__ __forceinline__ void log_record(const LogArgs& G, const int b, const int row, const double J, const double A1, const double B2,
                                           const double rho, const double gap, const double expected, const double a_acc, const double J_acc,
                                           const double theta, const double mu, const int tried, const double slack, const int iters,
                                           const int rollouts, const int bumps) {
    double* r = G.log + (size_t(b) * G.rows + row) * kLogWords;
    r[0] = J; r[1] = A1; r[2] = B2; r[3] = rho; r[4] = gap; r[5] = expected; r[6] = a_acc; r[7] = J_acc;
    r[8] = theta; r[9] = mu; r[10] = double(tried); r[11] = slack; r[12] = double(iters); r[13] = double(rollouts);
    r[14] = double(bumps); r[15] = 0.0;
}
// a trailing kernel argument as the kernel declares it: the table pointer __restrict__ as it always was, ResumeArgs by value
template <class T> struct KernelArg { using type = T; };
template <class T> struct KernelArg<T*> { using type = T* __restrict__; };

// Hand-off between phases of a ONE-WAVEFRONT workgroup.  LDS (and global) accesses of one wave are performed in issue order, so a
// later ds_read of any lane sees an earlier ds_write of any lane without waiting; what must not happen is the COMPILER moving
// accesses across the hand-off.  A wavefront-scope fence does exactly that and costs no instruction, where __syncthreads()
// costs an s_waitcnt lgkmcnt(0) that also drains loads still in flight.  (The 4-wave kernels use real barriers.)
// s_waitcnt vmcnt(0) (gfx9 encoding: vmcnt 0, expcnt / lgkmcnt at their maxima): every load and store of this wave has completed.
// In front of a knot loop: whatever the code before the loop left in flight is otherwise "pending" on the loop's entry edge in the
// compiler's wait-count bookkeeping, and the waits it inserts for that stay inside the loop body, behind the knot's prefetch.
__device__ __forceinline__ void drain_vmem() { __builtin_amdgcn_s_waitcnt(0x0F70); }

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}
// value of lane `l` (compile-time constant after unrolling) broadcast to the wave through SGPRs: 2 x v_readlane_b32
__device__ __forceinline__ double readlane_d(double v, int l) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_readlane(lo, l);
    hi = __builtin_amdgcn_readlane(hi, l);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, kWave));
    return v;
}

// LDS tile layout of one instance (offsets in doubles).  Tiles are stored so that every inner product of the sweep
// runs over CONTIGUOUS, 16-byte aligned rows (ds_read_b128, two fp64 per load):
//   VXX [NXP][NXP]  Vxx+ (symmetric; pad row/col zero)
//   FT  [NZP][NIP]  F~^T : FT[j][l] = F~[l][j],  F~ = [fx fu ; Je]  (NX dynamics rows + NE extra residual rows)
//   WT  [NZP][NIP]  (V~ F~)^T : WT[j][l<NX] = sum_m Vxx[l][m] F[m][j] ;  WT[j][NX+m] = lambda_m(k) * Je[m][j]
//   Q   [NZP][NZP]  diag(D) + F~^T (V~ F~)   (symmetric, both triangles written)
template <class M>
struct Lds {
    static constexpr int NX = M::NX, NU = M::NU, NZ = M::NZ, NE = M::NE, NEV = M::NEV, NI = NX + NEV;   // product rows only
    static constexpr int NXP = (NX + 1) & ~1;
    static constexpr int NIP = (((NI + 1) & ~1) % 4 == 0) ? ((NI + 1) & ~1) + 2 : ((NI + 1) & ~1);   // even, == 2 (mod 4): rows on distinct 16-B slots
    static constexpr int NZP = (NZ + 3) & ~3;
    static constexpr int SQ = (NZP % 4 == 0) ? NZP + 2 : NZP;          // row stride of the Q tile: == 2 (mod 4) as well
    static constexpr int NUP = (NU + 1) & ~1;
    static constexpr int NRECP = (((M::NREC + 1) & ~1) + M::NSO2T + 1) & ~1;   // record, then the second-order factors (SO2 builds)
    static constexpr int SO2T = (M::NREC + 1) & ~1;                             // ... at this offset from REC
    static constexpr int NPP = (M::NP + 1) & ~1;
    static constexpr int VXX = 0;
    static constexpr int FT = VXX + NXP * NXP;
    static constexpr int WT = FT + NZP * NIP;
    static constexpr int Q = WT + NZP * NIP;
    static constexpr int VX = Q + NZP * SQ;
    static constexpr int VP = VX + NXP;
    static constexpr int DK = VP + NXP;
    static constexpr int QV = DK + NXP;
    static constexpr int REC = QV + NZP;
    static constexpr int PK = REC + NRECP;
    static constexpr int KT = PK + NPP;            // [NXP][NUP]: KT[c][i] = K[i][c]
    static constexpr int KF = KT + NXP * NUP;      // kff [NUP]
    static constexpr int PIV = KF + NUP;           // [NUP]
    static constexpr int DS = PIV + NUP;           // constant diagonal, state part   [NZP]
    static constexpr int DG = DS + NZP;            // constant diagonal, stage part   [NZP]
    static constexpr int LS = DG + NZP;            // extra-row weights, state / stage [NE] each
    static constexpr int LG = LS + ((NE + 1) & ~1);
    static constexpr int LAM = LG + ((NE + 1) & ~1);   // LS + LG: extra-row weights of a stage node k >= 1
    static constexpr int KI = LAM + ((NE + 1) & ~1);   // ints: dkind[NZP], dci[NZP], tri LUT
    static constexpr int NBQ = NZP / 2, NTRIQ = NBQ * (NBQ + 1) / 2;
    static constexpr int ntriv(int nx) { int n = 0; for (int a = 0; a < nx; ++a) n += a / 2 + 1; return n; }
    static constexpr int NTRIV = ntriv(NX);        // Vxx update: 1 x 2 blocks (row a, column pair 2bp, 2bp+1 with 2bp <= a)
    static constexpr int SO2L = 2 * NZP + NTRIQ + NTRIV;       // SO2 builds: pair codes of the second-order contraction
    static constexpr int KI_INTS = SO2L + M::NSO2L;
    static constexpr int RO = KI + (KI_INTS + 1) / 2;  // rollout staging: xs | us | p | gains | dft of one knot
    static constexpr int RO_X = 0, RO_U = NXP, RO_P = RO_U + NUP, RO_G = RO_P + NPP, RO_D = RO_G + ((NU * (NX + 1) + 1) & ~1);
    static constexpr int RO_N = RO_D + NXP;
    static constexpr int TOTAL = RO + RO_N;
    static constexpr size_t BYTES = size_t(TOTAL) * sizeof(double);
};

typedef double double2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double2_t lds2(const double* p) { return *reinterpret_cast<const double2_t*>(p); }
// Pins a loaded pair in its registers: the read that produces it has completed here, and (placed after the reads of later
// stages in program order) those stay in flight behind it.  See DESIGN.md section 5, "exposed LDS round trips".
__device__ __forceinline__ void pin2(double2_t& v) { asm volatile("" : "+v"(v)); }

// -----------------------------------------------------------------------------------------------------------------
// derivative phase: one lane per knot -> compact records in HBM/L2
// -----------------------------------------------------------------------------------------------------------------
template <class M>
__device__ __forceinline__ void phase_derivs(const DevConsts& c, int N, const double* __restrict__ xs,
                                             const double* __restrict__ us, const double* __restrict__ P,
                                             double* __restrict__ rec, int lane) {
    for (int k = lane; k <= N; k += kWave) {
        double x[M::NX], u[M::NU];
#pragma unroll
        for (int i = 0; i < M::NX; ++i) x[i] = xs[k * M::NX + i];
        const int ku = k < N ? k : N - 1;
#pragma unroll
        for (int i = 0; i < M::NU; ++i) u[i] = us[ku * M::NU + i];
        M::derivs(c, x, u, P + k * M::NP, k, N, rec + size_t(k) * M::NREC);
    }
    if (M::SO2) {   // full second-order builds: the factors of the wdot Hessian, stage knots only (a pass of its own: registers)
        for (int k = lane; k < N; k += kWave) {
            double x[M::NX], u[M::NU];
#pragma unroll
            for (int i = 0; i < M::NX; ++i) x[i] = xs[k * M::NX + i];
#pragma unroll
            for (int i = 0; i < M::NU; ++i) u[i] = us[k * M::NU + i];
            M::so2_knot(c, x, u, P + k * M::NP, rec + size_t(k) * M::NREC);
        }
    }
}

// initial defects d_{k+1} = f(x_k,u_k) - x_{k+1}, total cost and defect 1-norm of the current iterate
template <class M>
__device__ __forceinline__ void phase_defects(const DevConsts& c, int N, const double* __restrict__ xs,
                                              const double* __restrict__ us, const double* __restrict__ P,
                                              double* __restrict__ dft, int lane, double& J, double& gap) {
    double Jl = 0.0, gl = 0.0;
    for (int k = lane; k <= N; k += kWave) {
        double x[M::NX];
#pragma unroll
        for (int i = 0; i < M::NX; ++i) x[i] = xs[k * M::NX + i];
        if (k < N) {
            double u[M::NU], xn[M::NX];
#pragma unroll
            for (int i = 0; i < M::NU; ++i) u[i] = us[k * M::NU + i];
            Jl += M::step(c, x, u, P + k * M::NP, k, xn);
#pragma unroll
            for (int i = 0; i < M::NX; ++i) {
                const double d = xn[i] - xs[(k + 1) * M::NX + i];
                dft[k * M::NX + i] = d;
                gl += fabs(d);
            }
        } else {
            Jl += M::term_cost(c, x, P + k * M::NP);
        }
    }
    J = wave_sum(Jl);
    gap = wave_sum(gl);
}

// -----------------------------------------------------------------------------------------------------------------
// one-time (per kernel) constant tables in LDS: constant part of F~^T, diagonal tables, extra-row weights, block LUTs
// -----------------------------------------------------------------------------------------------------------------
template <class M>
__device__ void sweep_tables(const DevConsts& c, double* s, int lane) {
    using L = Lds<M>;
    constexpr int NX = M::NX, NZ = M::NZ, NE = M::NE, NEV = M::NEV;
    for (int e = lane; e < L::TOTAL; e += kWave) s[e] = 0.0;
    wave_sync();
    for (int e = lane; e < M::NREC; e += kWave) s[L::REC + e] = 0.0;         // zero record -> constant part of F
    wave_sync();
    for (int e = lane; e < NZ * NX; e += kWave) {
        const int j = e / NX, i = e % NX;
        s[L::FT + j * L::NIP + i] = M::F_entry(c, s + L::REC, i, j);
    }
    for (int e = lane; e < NZ * NEV; e += kWave) {
        const int j = e / NEV, m = e % NEV;
        s[L::FT + j * L::NIP + NX + m] = M::E_const(c, m, j);
    }
    int* ki = reinterpret_cast<int*>(s + L::KI);
    for (int i = lane; i < NZ; i += kWave) {
        s[L::DS + i] = M::dg_state(c, i);
        s[L::DG + i] = M::dg_stage(c, i);
        ki[i] = M::dkind(i);
        ki[L::NZP + i] = M::dci(i);
    }
    for (int m = lane; m < NE; m += kWave) {
        s[L::LS + m] = M::lam_state(c, m);
        s[L::LG + m] = M::lam_stage(c, m);
        s[L::LAM + m] = M::lam_state(c, m) + M::lam_stage(c, m);
    }
    // lower-triangle block LUTs: t -> (ba << 8) | bc with ba >= bc
    for (int t = lane; t < L::NTRIQ; t += kWave) {
        int ba = 0;
        while ((ba + 1) * (ba + 2) / 2 <= t) ++ba;
        ki[2 * L::NZP + t] = (ba << 8) | (t - ba * (ba + 1) / 2);
    }
    for (int t = lane; t < L::NTRIV; t += kWave) {          // t -> (row a << 8) | column pair bp
        int a = 0, first = 0;
        while (first + a / 2 + 1 <= t) { first += a / 2 + 1; ++a; }
        ki[2 * L::NZP + L::NTRIQ + t] = (a << 8) | (t - first);
    }
    for (int e = lane; e < M::NSO2L / 2; e += kWave) M::so2_pair_code(e, ki[L::SO2L + 2 * e], ki[L::SO2L + 2 * e + 1]);
    wave_sync();
}

// -----------------------------------------------------------------------------------------------------------------
// backward Riccati sweep.  Returns false when a Quu is not positive definite (caller bumps mu, ddp.py:34-35).
// Requires sweep_tables() to have run in this kernel.  One knot per loop trip; the next knot's record / parameters /
// defect are prefetched into registers while the current knot is processed.
// -----------------------------------------------------------------------------------------------------------------
template <class M, bool KEEP = false>
__device__ bool backward_sweep(const DevConsts& c, int N, const double* __restrict__ P, const double* __restrict__ dft,
                               const double* __restrict__ rec, double* __restrict__ gains, double mu, double theta, double* s,
                               int lane, double& dV1, double& G1, double& G2, double& qu_inf, bool has_gap SDDP_T_ARG, int keep = 0,
                               double* __restrict__ val = nullptr, int vnodes = 0) {
    // has_gap = false: all defects are zero (every iteration after the first full step): v' = Vx, no Vxx d product
    // KEEP (policy export, policy_kernel): only the gains of the knots < keep are stored; `gains` then holds `keep` knots
    // val (KEEP only; value export, sddp_enable_value; null: off): the instance's value record, the nodes < vnodes of it (store_value)
    using L = Lds<M>;
    constexpr int NX = M::NX, NU = M::NU, NZ = M::NZ, NE = M::NE, NEV = M::NEV, NREC = M::NREC, NP = M::NP;
    constexpr int NXP = L::NXP, NIP = L::NIP, NZP = L::NZP, NUP = L::NUP, SQ = L::SQ;
    constexpr int NCOL = NU + 1 + NX;
    static_assert(NEV == NE || !M::CONST_ROWS_STATE_WEIGHTED, "constant rows with node-dependent weights must stay in the product");
    constexpr int RREC = (NREC + kWave - 1) / kWave;
    constexpr bool PADROW = (NXP > NX);      // odd NX: the pad row of the Vxx tile carries v' through the W product
    static_assert(NCOL <= kWave, "one lane per augmented column");
    static_assert(NX <= kWave && NP <= kWave, "one lane per state row / parameter");
    const int* ki = reinterpret_cast<const int*>(s + L::KI);
    dV1 = G1 = G2 = qu_inf = 0.0;
    bool ok = true;
    // the blocks this lane owns in the Q and Vxx phases never change: read the block LUT once per sweep, not once per knot
    // (one dependent LDS round trip less in each of the two phases)
    constexpr int PQ = (L::NTRIQ + kWave - 1) / kWave, PV = (L::NTRIV + kWave - 1) / kWave;
    int codeq[PQ], codev[PV];
#pragma unroll
    for (int q = 0; q < PQ; ++q) codeq[q] = (lane + q * kWave < L::NTRIQ) ? ki[2 * NZP + lane + q * kWave] : 0;
#pragma unroll
    for (int q = 0; q < PV; ++q) codev[q] = (lane + q * kWave < L::NTRIV) ? ki[2 * NZP + L::NTRIQ + lane + q * kWave] : 0;
    // constant extra rows (m >= NEV): their share sum_m lambda_m E[m][row] E[m][col] of the lane's four Q entries, once per sweep
    double qconst[PQ][4];
#pragma unroll
    for (int q = 0; q < PQ; ++q) {
        const int a0 = 2 * (codeq[q] >> 8), c0 = 2 * (codeq[q] & 255);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            double v = 0.0;
            if (NEV < NE) {
                const int row = a0 + (e >> 1), col = c0 + (e & 1);
                if (row < NZ && col < NZ)
                    for (int m = NEV; m < NE; ++m) v += s[L::LG + m] * M::E_const(c, m, row) * M::E_const(c, m, col);
            }
            qconst[q][e] = v;
        }
    }
    // diagonal blocks: what the diagonal term D of the lane's two diagonal entries needs is knot-invariant except for the knot's
    // parameters, so it is read once per sweep (zeros on the lanes that own an off-diagonal block: the per-knot code below is
    // then branch-free and its parameter reads are issued ahead of the tile product)
    int dkind[PQ][2], dcidx[PQ][2];
    double dsv[PQ][2], dgv[PQ][2];
#pragma unroll
    for (int q = 0; q < PQ; ++q) {
        const int a0 = 2 * (codeq[q] >> 8), c0 = 2 * (codeq[q] & 255);
        const bool on = lane + q * kWave < L::NTRIQ && a0 == c0;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const bool one = on && a0 + e < NZ;
            const int idx = one ? a0 + e : 0;
            dkind[q][e] = one ? ki[idx] : 0;
            dcidx[q][e] = one ? ki[NZP + idx] : 0;
            dsv[q][e] = one ? s[L::DS + idx] : 0.0;
            dgv[q][e] = one ? s[L::DG + idx] : 0.0;
        }
    }
    // ---- terminal node: Vx = lx_N, Vxx = lxx_N = diag(D_state) + Je^T Lambda_state Je  (ddp.py:216-226)
    {
        const double* rN = rec + size_t(N) * NREC;
        if (lane < NXP) s[L::VX + lane] = lane < NX ? rN[M::REC_G + lane] : 0.0;
        if (lane < NP) s[L::PK + lane] = P[N * NP + lane];
        if constexpr (M::HAS_UR) M::expand_term(rN, s + L::FT, NIP, lane, kWave);   // user build: the user rows' Jacobian at node N
        wave_sync();
        for (int e = lane; e < NXP * NXP; e += kWave) {
            const int a = e / NXP, b = e % NXP;
            double v = 0.0;
            if (a < NX && b < NX) {
                for (int m = 0; m < NEV; ++m) v += s[L::LS + m] * s[L::FT + a * NIP + NX + m] * s[L::FT + b * NIP + NX + m];
                if (a == b) v += s[L::DS + a] + M::dparam(c, s + L::PK, ki[a], ki[NZP + a], 1.0, 0.0);
            }
            s[L::VXX + e] = v;
        }
        // extra-row part of WT = (V~ F~)^T for the nodes k >= 1: lambda_m Je[m][j].  Constant entries are written here once per
        // sweep, the per-knot variable ones by expand_var together with F~^T; node 0 (other weights) rescales them below
        for (int e = lane; e < NZ * NEV; e += kWave) {
            const int j = e / NEV, m = e % NEV;
            s[L::WT + j * NIP + NX + m] = s[L::LAM + m] * s[L::FT + j * NIP + NX + m];
        }
        wave_sync();
    }
    // ---- knot operands record | parameters | defect.  The last record word group and the parameters share one load: lanes past
    //      the record's tail take the parameters (fixed per-lane source / knot stride / LDS slot).  The defect is staged only
    //      while there is one (has_gap); otherwise its slot stays zero.
    constexpr int RTAIL = NREC - (RREC - 1) * kWave;                  // record words in the last group
    constexpr bool MERGE_P = RTAIL + NP <= kWave;
    const bool tail_rec = lane < RTAIL, tail_par = MERGE_P && lane >= RTAIL && lane < RTAIL + NP;
    const double* t_src = tail_rec ? rec + (RREC - 1) * kWave + lane : P + (lane - RTAIL);
    const int t_stride = tail_rec ? NREC : NP;
    const int t_dst = tail_rec ? L::REC + (RREC - 1) * kWave + lane : L::PK + (lane - RTAIL);
    const bool t_on = tail_rec || tail_par;
    double r_rec[RREC], r_p = 0.0, r_d = 0.0;
    auto fetch = [&](int k) {
        const double* rk = rec + size_t(k) * NREC;
#pragma unroll
        for (int t = 0; t + 1 < RREC; ++t) r_rec[t] = rk[lane + t * kWave];
        if (t_on) r_rec[RREC - 1] = t_src[size_t(k) * t_stride];
        if (!MERGE_P && lane < NP) r_p = P[k * NP + lane];
        if (has_gap && lane < NX) r_d = dft[k * NX + lane];
    };
    if (lane < NXP) s[L::DK + lane] = 0.0;
    // gains of knot kk, LDS (KF | K^T, as the solve phase left them) -> HBM/L2: word e of the knot's record = kff[e] for e < NU, else
    // K[i][c] = KT[c][i] with (i, c) = divmod(e - NU, NX); whole-wave contiguous stores
    constexpr int NGW = NU * (NX + 1), RGW = (NGW + kWave - 1) / kWave;
    int g_src[RGW];
#pragma unroll
    for (int t = 0; t < RGW; ++t) {
        const int e = lane + t * kWave, ec = e < NGW ? e : 0;
        g_src[t] = ec < NU ? L::KF + ec : L::KT + ((ec - NU) % NX) * NUP + (ec - NU) / NX;
    }
    auto store_gains = [&](int kk) {
        if constexpr (KEEP) { if (kk >= keep) return; }
        double* gk = gains + size_t(kk) * NGW;
        double v[RGW];
#pragma unroll
        for (int t = 0; t < RGW; ++t) v[t] = s[g_src[t]];
#pragma unroll
        for (int t = 0; t < RGW; ++t)
            if (lane + t * kWave < NGW) gk[lane + t * kWave] = v[t];
    };
    // value export: the quadratic model of the cost-to-go at node kk as the tiles hold it, LDS -> HBM/L2, whole-wave contiguous stores:
    // word 1 = expected_kk = -(dV1 + dV2) of the knots >= kk, then Vx (NX), then Vxx (NX x NX) row-major without the pad row / column of
    // an odd NX.  Entry (i, j) is read from the lower triangle, so the record is symmetric bit for bit at the terminal node as well.
    // Word 0 (the cost from node kk on) is policy_instance's (value_costs).
    auto store_value = [&](int kk, double expected) {
        if constexpr (KEEP) {
            if (val == nullptr || kk >= vnodes) return;
            double* vk = val + size_t(kk) * value_words(NX);
            for (int e = lane; e < NX + NX * NX; e += kWave) {
                const int i = e < NX ? 0 : (e - NX) / NX, j = e < NX ? 0 : (e - NX) % NX;
                vk[2 + e] = e < NX ? s[L::VX + e] : s[L::VXX + (i > j ? i : j) * NXP + (i > j ? j : i)];
            }
            if (lane == 0) vk[1] = expected;
        }
    };
    store_value(N, 0.0);
    drain_vmem();
    fetch(N - 1);
    for (int k = N - 1; k >= 0; --k) {
        // ---- stage this knot from the prefetch registers; start the next knot's loads; then the previous knot's gains go out
#pragma unroll
        for (int t = 0; t + 1 < RREC; ++t) s[L::REC + lane + t * kWave] = r_rec[t];
        if (t_on) s[t_dst] = r_rec[RREC - 1];
        if (!MERGE_P && lane < NP) s[L::PK + lane] = r_p;
        if (has_gap && lane < NX) s[L::DK + lane] = r_d;
        if (k < N - 1) store_gains(k + 1);
        if (k > 0) fetch(k - 1);
        wave_sync();
        SDDP_TICK(1)
        const double state = k >= 1 ? 1.0 : 0.0;
        // ---- expand: variable entries of F~^T; v' = Vx + Vxx d ; gap terms
        M::expand_var(c, s + L::REC, s + L::FT, NIP, lane, kWave, s + L::WT, s + L::LAM);
        if (lane < NX) {
            double acc = 0.0;
            if (has_gap) {
                double2_t vv[NXP / 2], dd[NXP / 2];
#pragma unroll
                for (int m = 0; m < NXP; m += 2) { vv[m / 2] = lds2(s + L::VXX + lane * NXP + m); dd[m / 2] = lds2(s + L::DK + m); }
#pragma unroll
                for (int m = 0; m < NXP / 2; ++m) { pin2(vv[m]); pin2(dd[m]); }
#pragma unroll
                for (int m = 0; m < NXP / 2; ++m) acc = fma(vv[m].y, dd[m].y, fma(vv[m].x, dd[m].x, acc));
            }
            const double d = s[L::DK + lane], vx = s[L::VX + lane];
            s[L::VP + lane] = vx + acc;
            if (PADROW) s[L::VXX + NX * NXP + lane] = vx + acc;   // pad row of Vxx := v': the W product then yields F^T v'
            G1 = fma(d, vx, G1);                 // per-lane partial sums, reduced once after the sweep
            G2 = fma(0.5 * d, acc, G2);
        }
        wave_sync();
        SDDP_TICK(2)
        // ---- WT = (V~ F~)^T : 2 (l) x JB (j) register blocks, inner product over the NX dynamics rows.  JB = 3 when that still
        //      fits one pass of the wave (more lanes, a shorter chain per lane), else 4.  A block may reach one row past the
        //      F~^T tile (the row after it is the first row of WT: finite, never stored).
        constexpr int JB = ((NXP / 2) * ((NZP + 2) / 3) <= kWave) ? 3 : 4;
        constexpr int NJB = (NZP + JB - 1) / JB;
        for (int blk = lane; blk < (NXP / 2) * NJB; blk += kWave) {
            const int l0 = 2 * (blk % (NXP / 2)), j0 = JB * (blk / (NXP / 2));
            double a0[JB], a1[JB];
#pragma unroll
            for (int jj = 0; jj < JB; ++jj) a0[jj] = a1[jj] = 0.0;
            constexpr int NSW = NXP / 2, PFW = 2;       // operands two steps ahead, as in the Q phase below
            double2_t v0[NSW], v1[NSW], ff[NSW][JB];
            auto ldw = [&](int st) {
                v0[st] = lds2(s + L::VXX + l0 * NXP + 2 * st); v1[st] = lds2(s + L::VXX + (l0 + 1) * NXP + 2 * st);
#pragma unroll
                for (int jj = 0; jj < JB; ++jj) ff[st][jj] = lds2(s + L::FT + (j0 + jj) * NIP + 2 * st);
            };
#pragma unroll
            for (int st = 0; st < PFW && st < NSW; ++st) ldw(st);
#pragma unroll
            for (int st = 0; st < NSW; ++st) {
                if (st + PFW < NSW) ldw(st + PFW);
                pin2(v0[st]); pin2(v1[st]);
#pragma unroll
                for (int jj = 0; jj < JB; ++jj) pin2(ff[st][jj]);
#pragma unroll
                for (int jj = 0; jj < JB; ++jj) {
                    a0[jj] = fma(v0[st].y, ff[st][jj].y, fma(v0[st].x, ff[st][jj].x, a0[jj]));
                    a1[jj] = fma(v1[st].y, ff[st][jj].y, fma(v1[st].x, ff[st][jj].x, a1[jj]));
                }
            }
#pragma unroll
            for (int jj = 0; jj < JB; ++jj) {
                if (j0 + jj >= NZP) continue;
                if (l0 + 1 < NX) {
                    double2_t w;
                    w.x = a0[jj];
                    w.y = a1[jj];
                    *reinterpret_cast<double2_t*>(s + L::WT + (j0 + jj) * NIP + l0) = w;
                } else {
                    s[L::WT + (j0 + jj) * NIP + l0] = a0[jj];        // odd NX: slot NX belongs to the first extra row;
                    if (j0 + jj < NZ) s[L::QV + j0 + jj] = s[L::REC + M::REC_G + j0 + jj] + a1[jj];   // row NX of Vxx holds v'
                }
            }
        }
        if (k == 0) {   // node 0 carries no state residuals: rescale the extra rows with the stage-only weights
            wave_sync();
            for (int e = lane; e < NZ * NEV; e += kWave) {
                const int j = e / NEV, m = e % NEV;
                s[L::WT + j * NIP + NX + m] = s[L::LG + m] * s[L::FT + j * NIP + NX + m];
            }
        }
        wave_sync();
        SDDP_TICK(3)
        // ---- Q = diag(D) + F~^T (V~ F~): lower-triangle 2x2 blocks, mirrored ; q = g + F^T v'
#pragma unroll
        for (int q = 0; q < PQ; ++q) {
            if (lane + q * kWave >= L::NTRIQ) break;
            const int code = codeq[q];
            const int a0 = 2 * (code >> 8), c0 = 2 * (code & 255);
            double q00 = 0, q01 = 0, q10 = 0, q11 = 0;
            // operands two steps ahead of the step being multiplied (three register stages, pinned stage by stage): the reads of
            // the whole product stay in flight behind the FMAs instead of a round trip every other step
            constexpr int NS = NIP / 2, PF = 2;
            double2_t fa[NS], fb[NS], wa[NS], wb[NS];
            auto ldq = [&](int st) {
                fa[st] = lds2(s + L::FT + a0 * NIP + 2 * st); fb[st] = lds2(s + L::FT + (a0 + 1) * NIP + 2 * st);
                wa[st] = lds2(s + L::WT + c0 * NIP + 2 * st); wb[st] = lds2(s + L::WT + (c0 + 1) * NIP + 2 * st);
            };
#pragma unroll
            for (int st = 0; st < PF && st < NS; ++st) ldq(st);
            // diagonal term of this knot (zero on off-diagonal blocks): its parameter reads queue behind the first product operands
            const double dd0 = state * dsv[q][0] + dgv[q][0] + M::dparam(c, s + L::PK, dkind[q][0], dcidx[q][0], state, 1.0);
            const double dd1 = state * dsv[q][1] + dgv[q][1] + M::dparam(c, s + L::PK, dkind[q][1], dcidx[q][1], state, 1.0);
#pragma unroll
            for (int st = 0; st < NS; ++st) {
                if (st + PF < NS) ldq(st + PF);
                pin2(fa[st]); pin2(fb[st]); pin2(wa[st]); pin2(wb[st]);
                q00 = fma(fa[st].y, wa[st].y, fma(fa[st].x, wa[st].x, q00));
                q01 = fma(fa[st].y, wb[st].y, fma(fa[st].x, wb[st].x, q01));
                q10 = fma(fb[st].y, wa[st].y, fma(fb[st].x, wa[st].x, q10));
                q11 = fma(fb[st].y, wb[st].y, fma(fb[st].x, wb[st].x, q11));
            }
            if (NEV < NE) { q00 += qconst[q][0]; q01 += qconst[q][1]; q10 += qconst[q][2]; q11 += qconst[q][3]; }
            {   // diagonal block: add D, keep it exactly symmetric (selects, no branch)
                q00 += dd0;
                q11 += dd1;
                const double off = 0.5 * (q01 + q10);
                q01 = a0 == c0 ? off : q01;
                q10 = a0 == c0 ? off : q10;
            }
            double2_t r0, r1;
            r0.x = q00; r0.y = q01; r1.x = q10; r1.y = q11;
            *reinterpret_cast<double2_t*>(s + L::Q + a0 * SQ + c0) = r0;
            *reinterpret_cast<double2_t*>(s + L::Q + (a0 + 1) * SQ + c0) = r1;
            if (a0 != c0) {
                double2_t m0, m1;
                m0.x = q00; m0.y = q10; m1.x = q01; m1.y = q11;
                *reinterpret_cast<double2_t*>(s + L::Q + c0 * SQ + a0) = m0;
                *reinterpret_cast<double2_t*>(s + L::Q + (c0 + 1) * SQ + a0) = m1;
            }
        }
        if (!PADROW) {
            for (int j = lane; j < NZ; j += kWave) {
                double acc = s[L::REC + M::REC_G + j];
#pragma unroll
                for (int m = 0; m < NXP; m += 2) {
                    const double2_t f = lds2(s + L::FT + j * NIP + m), v = lds2(s + L::VP + m);
                    acc = fma(f.y, (m + 1 < NX) ? v.y : 0.0, fma(f.x, (m < NX) ? v.x : 0.0, acc));
                }
                s[L::QV + j] = acc;
            }
        }
        wave_sync();
        if (theta != 0.0) {   // exact second-order torque term (wave-uniform switch)
            if (M::NSO2T) {   // full second-order builds: the per-knot factors of the contraction first
                M::so2_prepare(c, s + L::REC, s + L::VP, s + L::REC + L::SO2T, lane, kWave);
                wave_sync();
            }
            M::add_second_order(c, s + L::REC, s + L::VP, QFull{s + L::Q, SQ}, theta, lane, kWave, s + L::REC + L::SO2T, ki + L::SO2L);
            wave_sync();
        }
        if (M::BAR) {         // friction-cone barrier builds: its Hessian blocks on the force-force diagonal of Q
            M::add_barrier(s + L::REC, QFull{s + L::Q, SQ}, lane, kWave, M::SO2 ? theta : 0.0);
            wave_sync();
        }
        SDDP_TICK(4)
        // ---- [k K] = -Quu^-1 [Qu Qux]: Gauss-Jordan, lane j owns column j of [Quu+mu I | Qu | Qux]
        double a[NU];
        const double qx = s[L::QV + (lane > NU && lane < NCOL ? lane - NU - 1 : 0)];     // Qx of this lane's state column, for the Vx update
        {
            // column of Q this lane reads (any valid one for lane NU, which takes q instead; lanes >= NCOL are zeroed)
            const int qcol = lane < NU ? NX + lane : (lane > NU && lane < NCOL ? lane - NU - 1 : 0);
#pragma unroll
            for (int i = 0; i < NU; ++i) {
                const double qv = s[L::QV + NX + i];
                double v = s[L::Q + (NX + i) * SQ + qcol];
                v = lane == NU ? qv : v;
                v += (i == lane) ? mu : 0.0;
                a[i] = lane < NCOL ? v : 0.0;
            }
        }
        double qu_abs = 0.0, qu_save[NU];
#pragma unroll
        for (int i = 0; i < NU; ++i) { qu_save[i] = a[i]; qu_abs = fmax(qu_abs, fabs(a[i])); }
        qu_inf = fmax(qu_inf, readlane_d(qu_abs, NU));
        // pivot column broadcast with v_readlane (through SGPRs): no LDS hand-off, no barrier inside the elimination
#pragma unroll
        for (int p = 0; p < NU; ++p) {
            double pv[NU];
#pragma unroll
            for (int i = 0; i < NU; ++i) pv[i] = readlane_d(a[i], p);
            if (!(pv[p] > 0.0) || !(pv[p] < 1e300)) ok = false;
            const double t = a[p] * fast_rcp(pv[p]);
#pragma unroll
            for (int i = 0; i < NU; ++i) a[i] = (i == p) ? t : fma(-pv[i], t, a[i]);
        }
        // a = Quu^-1 * column ; publish kff and K^T (negated) in LDS.  The copy to HBM/L2 (kff (NU) then K (NU x NX) row-major) is
        // made from there one knot later, behind the next staging wait (store_gains): a store in flight makes every wait for a
        // prefetched load a full vmcnt(0) (gfx9 counts loads and stores in one counter and returns them out of order with respect
        // to each other), so stores issued at the end of a knot were waited for at the start of the next
        if (lane >= NU && lane < NCOL) {
            double* dst = lane == NU ? s + L::KF : s + L::KT + (lane - NU - 1) * NUP;            // KF follows KT: one region
#pragma unroll
            for (int i = 0; i < NU; ++i) dst[i] = -a[i];
        }
        // kff broadcast from lane NU; then ONE dot product per lane with the column it loaded gives both
        //   lane NU:        kff . Qu           -> dV1 (dV2 = 1/2 kff^T Quu kff = -1/2 dV1 exactly, not accumulated separately)
        //   lane NU+1+c:    (Qux^T kff)[c]     -> Vx[c] = Qx[c] + Qux^T kff
        {
            double dot = 0.0;
#pragma unroll
            for (int i = 0; i < NU; ++i) dot = fma(readlane_d(-a[i], NU), qu_save[i], dot);
            dV1 += readlane_d(dot, NU);
            if (lane > NU && lane < NCOL) s[L::VX + lane - NU - 1] = qx + dot;
        }
        wave_sync();
        SDDP_TICK(5)
        if (!ok) return false;
        // ---- Vxx = Qxx + Qux^T K.  Qux^T K = -Qux^T (Quu + mu I)^-1 Qux is symmetric, so only the lower triangle is formed (one
        //      product per element, 1 x 2 blocks: 49 lanes with a 12-FMA chain each) and mirrored
#pragma unroll
        for (int q = 0; q < PV; ++q) {
            if (lane + q * kWave >= L::NTRIV) break;
            const int code = codev[q];
            const int a0 = code >> 8, c0 = 2 * (code & 255);        // row a0, columns c0, c0 + 1 (c0 <= a0)
            const bool two = c0 + 1 <= a0;                          // the second column is in the lower triangle too
            const int c1 = two ? c0 + 1 : c0;
            double v0 = s[L::Q + a0 * SQ + c0], v1 = s[L::Q + a0 * SQ + c1];
            double qa[NU], k0[NU], k1[NU];           // all operands in flight before the first FMA
#pragma unroll
            for (int i = 0; i < NU; ++i) {
                qa[i] = s[L::Q + a0 * SQ + NX + i];
                k0[i] = s[L::KT + c0 * NUP + i];
                k1[i] = s[L::KT + c1 * NUP + i];
            }
#pragma unroll
            for (int i = 0; i < NU; ++i) { asm volatile("" : "+v"(qa[i])); asm volatile("" : "+v"(k0[i])); asm volatile("" : "+v"(k1[i])); }
#pragma unroll
            for (int i = 0; i < NU; ++i) {
                v0 = fma(qa[i], k0[i], v0);
                v1 = fma(qa[i], k1[i], v1);
            }
            s[L::VXX + a0 * NXP + c0] = v0;
            if (c0 != a0) s[L::VXX + c0 * NXP + a0] = v0;
            if (two) {
                s[L::VXX + a0 * NXP + c1] = v1;
                if (c1 != a0) s[L::VXX + c1 * NXP + a0] = v1;
            }
        }
        wave_sync();
        SDDP_TICK(6)
        store_value(k, -0.5 * dV1);
    }
    store_gains(0);
    G1 = wave_sum(G1);
    G2 = wave_sum(G2);
    return ok;
}

// -----------------------------------------------------------------------------------------------------------------
// forward pass: one lane per step length.  Every lane rolls the whole horizon with its own alpha; the lane
// `store_lane` also writes its trajectory to xn/un.  OPEN_LOOP: plain rollout of us (single-shooting start).
// The knot's wave-uniform operands (x_k, u_k, p_k, gains_k, d_k) are fetched by ONE coalesced wave-wide load each,
// staged in LDS and read back as broadcasts; the next knot is prefetched into registers meanwhile.
// -----------------------------------------------------------------------------------------------------------------
template <class M, bool OPEN_LOOP>
__device__ double rollout(const DevConsts& c, int N, const double* __restrict__ x0, const double* __restrict__ P,
                          const double* __restrict__ xs, const double* __restrict__ us, const double* __restrict__ dft,
                          const double* __restrict__ gains, double* __restrict__ xn, double* __restrict__ un,
                          double alpha, int store_lane, int lane, double* s, bool has_gap = true) {
    // has_gap = false: all defects are zero, the (1 - alpha) d correction is skipped.
    // store_lane >= 0: that lane writes its trajectory to xn / un.  store_lane < 0: lanes 0 .. kSlots-1 each write theirs to
    // slot `lane` of xn / un (slot strides (N+1) NX and N NU): same instruction count, no second pass to fetch the winner.
    using L = Lds<M>;
    constexpr int NX = M::NX, NU = M::NU, NP = M::NP, NG = NU * (NX + 1), RG = (NG + kWave - 1) / kWave;
    double* ro = s + L::RO;
    const bool storing = store_lane >= 0 ? lane == store_lane : lane < kSlots;
    if (store_lane < 0 && storing) { xn += size_t(lane) * (N + 1) * NX; un += size_t(lane) * N * NU; }
    double x[NX];
    if (lane < NX) ro[L::RO_X + lane] = x0[lane];
    wave_sync();
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = ro[L::RO_X + i];
    wave_sync();
    // knot operands x_k | u_k | p_k | d_k: when they fit one wave (2 NX + NU + NP <= 64) every lane owns ONE word of the knot:
    // its source pointer / knot stride / LDS slot are fixed for the whole pass, so a knot costs one load and one LDS store
    // (plus the gain rows) instead of four masked pairs
    constexpr bool MERGED = !OPEN_LOOP && (2 * NX + NU + NP <= kWave);
    const double* m_src = nullptr;
    int m_stride = 0, m_dst = 0;
    bool m_on = false;
    if (MERGED) {
        int l = lane;
        if (l < NX) { m_src = xs + l; m_stride = NX; m_dst = L::RO_X + l; m_on = true; }
        else if ((l -= NX) < NU) { m_src = us + l; m_stride = NU; m_dst = L::RO_U + l; m_on = true; }
        else if ((l -= NU) < NP) { m_src = P + l; m_stride = NP; m_dst = L::RO_P + l; m_on = true; }
        else if ((l -= NP) < NX) { m_src = dft + l; m_stride = NX; m_dst = L::RO_D + l; m_on = true; }
    }
    double r_x = 0, r_u = 0, r_p = 0, r_d = 0, r_m = 0, r_g[RG];
    auto fetch = [&](int k) {
        // the gain rows first: their registers are zero-filled for the lanes past the row's end, and that write waits for whatever
        // the compiler still counts as pending on those registers -- in front of the knot's first load it waits for nothing
        if (!OPEN_LOOP) {
            const double* gk = gains + size_t(k) * NG;
#pragma unroll
            for (int t = 0; t < RG; ++t) r_g[t] = (lane + t * kWave < NG) ? gk[lane + t * kWave] : 0.0;
        }
        if (MERGED) {
            if (m_on) r_m = m_src[size_t(k) * m_stride];
        } else {
            if (lane < NU) r_u = us[k * NU + lane];
            if (lane < NP) r_p = P[k * NP + lane];
            if (!OPEN_LOOP && lane < NX) { r_x = xs[k * NX + lane]; r_d = dft[k * NX + lane]; }
        }
    };
    drain_vmem();
    fetch(0);
    double J = 0.0;
    const double oma = 1.0 - alpha;
    for (int k = 0; k < N; ++k) {
        if (MERGED) {
            if (m_on) ro[m_dst] = r_m;
        } else {
            if (lane < NU) ro[L::RO_U + lane] = r_u;
            if (lane < NP) ro[L::RO_P + lane] = r_p;
            if (!OPEN_LOOP && lane < NX) { ro[L::RO_X + lane] = r_x; ro[L::RO_D + lane] = r_d; }
        }
        if (!OPEN_LOOP) {
#pragma unroll
            for (int t = 0; t < RG; ++t)
                if (lane + t * kWave < NG) ro[L::RO_G + lane + t * kWave] = r_g[t];
        }
        if (k + 1 < N) fetch(k + 1);
        wave_sync();
        double u[NU];
        if (OPEN_LOOP) {
#pragma unroll
            for (int i = 0; i < NU; ++i) u[i] = ro[L::RO_U + i];
        } else {
            // u = u_k + alpha kff + K (x - x_k).  The gain rows are fetched one row ahead of the row being used (two register rows,
            // pinned row by row): left to the compiler every LDS read of the NU NX-long chain is issued just in time, one exposed
            // round trip per two FMAs
            double dx[NX], ub[NU], kf[NU], g[2][NX];
#pragma unroll
            for (int j = 0; j < NX; ++j) dx[j] = x[j] - ro[L::RO_X + j];
#pragma unroll
            for (int i = 0; i < NU; ++i) { ub[i] = ro[L::RO_U + i]; kf[i] = ro[L::RO_G + i]; }
#pragma unroll
            for (int j = 0; j < NX; ++j) g[0][j] = ro[L::RO_G + NU + j];
#pragma unroll
            for (int i = 0; i < NU; ++i) {
                if (i + 1 < NU) {
#pragma unroll
                    for (int j = 0; j < NX; ++j) g[(i + 1) & 1][j] = ro[L::RO_G + NU + (i + 1) * NX + j];
                }
#pragma unroll
                for (int j = 0; j < NX; ++j) asm volatile("" : "+v"(g[i & 1][j]));
                double acc = ub[i] + alpha * kf[i];
#pragma unroll
                for (int j = 0; j < NX; ++j) acc += g[i & 1][j] * dx[j];
                u[i] = acc;
            }
        }
        if (storing) {
#pragma unroll
            for (int i = 0; i < NX; ++i) xn[k * NX + i] = x[i];
#pragma unroll
            for (int i = 0; i < NU; ++i) un[k * NU + i] = u[i];
        }
        J += M::step(c, x, u, ro + L::RO_P, k, x);               // in place: every component is read before it is written
        if (!OPEN_LOOP && has_gap) {
#pragma unroll
            for (int i = 0; i < NX; ++i) x[i] -= oma * ro[L::RO_D + i];
        }
        wave_sync();
    }
    if (lane < NP) ro[L::RO_P + lane] = P[N * NP + lane];
    wave_sync();
    J += M::term_cost(c, x, ro + L::RO_P);
    if (storing) {
#pragma unroll
        for (int i = 0; i < NX; ++i) xn[N * NX + i] = x[i];
    }
    wave_sync();
    return J;
}

// -----------------------------------------------------------------------------------------------------------------
// fused persistent solve: one wavefront per MPC instance, all iterations in one launch (replaces ddp.py:101)
// -----------------------------------------------------------------------------------------------------------------
// RESUME (sddp_enable_resume): the instantiation that can stop at max_iters and be taken up again.  It differs in three places --
// entry (a continue launch skips the starting point of a resumable instance and loads what the iteration carries from one accepted
// step to the next: stats and the carried defects; it returns at once for any other instance), and exit (the defects go to the
// instance's carry row when status == 1; the flag is set).  Nothing is recomputed from the trajectory: recomputed defects equal
// (1 - alpha) d only up to rounding (and are noise where the engine carries exact zeros), and phase_defects sums the cost in
// another order than the rollout that produced J -- either would break the bit identity with the uncut solve.  With RESUME false
// every such line is behind `if constexpr`: the ordinary instantiation is the code it was.
// LOG (sddp_enable_iteration_log; RESUME instantiations only): one record per line search goes to the instance's rows of the log, written
// by lane 0 behind the search, where the accepted trajectory's pointers flip -- after the rollout's stores and before the next loads.
// Every value of a record is wave-uniform as the iteration has it.  Every such line is behind `if constexpr (LOG)`.
template <class M, bool RESUME = false, class Res = NoResume, bool LOG = false, class Lg = NoLog>
__device__ __forceinline__ void solve_instance(const SolveArgs& A, double* s, const int b, const int slot, const Res& R = Res(), const Lg& G = Lg()) {
    static_assert(!LOG || RESUME, "the iteration log rides on the resumable instantiation");
    constexpr int NX = M::NX, NU = M::NU, NP = M::NP, NREC = M::NREC;
    const int lane = threadIdx.x;
    const int N = A.N;
    const sddp_options& o = A.o;
    // `resumed`: a run-time flag in the RESUME instantiation, a compile-time false in the ordinary one (the conditions on it fold in
    // the front end: the ordinary instantiation is compiled from the statements it always had)
    std::conditional_t<RESUME, bool, const std::false_type> resumed{};
    if constexpr (RESUME) {
        if (R.cont) {   // wave-uniform: a kernel argument and instance b's flag
            if (R.flag(b) != 1) return;
            resumed = true;
        }
    }
    const double* x0 = A.x0 + size_t(b) * NX;
    const double* P = A.P + size_t(b) * (N + 1) * NP;
    double* xs = A.xs + size_t(b) * (N + 1) * NX;
    double* us = A.us + size_t(b) * N * NU;
    // candidate sets: set w of this instance = kSlots trajectories; the pass of an iteration writes set `wr`, the current
    // iterate lives in the other set (or in A.xs / A.us before the first accepted step)
    const size_t XS = size_t(N + 1) * NX, US = size_t(N) * NU;
    double* xc = A.xc + size_t(slot) * 2 * kSlots * XS;
    double* uc = A.uc + size_t(slot) * 2 * kSlots * US;
    int wr = 0;
    double* dft = A.dft + size_t(slot) * N * NX;
    double* gains = A.gains + size_t(slot) * N * (NU * (NX + 1));
    double* rec = A.rec + size_t(slot) * (N + 1) * NREC;

    double J = 0.0, gap = 0.0;
    SDDP_T_DECL
    sweep_tables<M>(A.c, s, lane);
    // ---- starting point
    if (resumed) {   // the iterate is in A.xs / A.us; its defects as the cut solve left them
        if constexpr (RESUME) {
            const double* cr = R.carry + size_t(b) * N * NX;
            for (int e = lane; e < N * NX; e += kWave) dft[e] = cr[e];
            wave_sync();
        }
    } else if (o.initial_rollout) {
        J = rollout<M, true>(A.c, N, x0, P, xs, us, dft, gains, xc, uc, 0.0, 0, lane, s);
        wave_sync();
        for (int e = lane; e < (N + 1) * NX; e += kWave) xs[e] = xc[e];
        for (int e = lane; e < N * NX; e += kWave) dft[e] = 0.0;
        wave_sync();
    } else {
        if (lane < NX) xs[lane] = x0[lane];
        wave_sync();
        phase_defects<M>(A.c, N, xs, us, P, dft, lane, J, gap);
        wave_sync();
    }
    double mu = o.mu0, rho = 0.0, alpha = 0.0, expected = 0.0, theta = 0.0;
    int iters = 0, converged = 0, status = 1, rollouts = 0, win = 0;
    if constexpr (RESUME) {
        if (resumed) {
            const sddp_stats st = A.stats[b];
            J = st.cost; gap = st.gap; mu = st.mu; rho = st.rho; alpha = st.alpha; expected = st.expected;
            theta = (o.second_order && alpha == o.alpha_0) ? 1.0 : 0.0;
            iters = st.iters; rollouts = st.rollouts;
            if (lane == 0) R.ran(A.B, b) = 1;
        }
    }
    LogState<LOG> lg;
    if constexpr (LOG) {
        if (resumed) lg.n = __builtin_amdgcn_readfirstlane(G.count[b]);      // a continue launch appends
    }
    std::conditional_t<RESUME, int, const std::false_type> iters_at_entry{};      // what this launch owes an instance counts from here
    if constexpr (RESUME) iters_at_entry = iters;
    if (!(fabs(J) < 1e300)) { status = 3; }
    else
        while (iters < o.max_iters) {
            if constexpr (RESUME) {
                // Time budget: one clock read per accepted iteration, here at the loop head and nowhere inside the iteration.  Leaving
                // here is leaving at `iters < o.max_iters` turned false: status is still 1, nothing of the iterate is half-made, and
                // the exit below stores what a solve at max_iters = iters stores.  The decision is wave-uniform by construction:
                // kernel arguments, `iters` (the same in every lane) and two scalar reads (the clock, the deadline word).
                if (R.budget_iters >= 0 && iters - iters_at_entry >= R.budget_iters && deadline_passed(R, A.B)) break;
            }
            SDDP_TICK(9)
            phase_derivs<M>(A.c, N, xs, us, P, rec, lane);
            wave_sync();
            SDDP_TICK(0)
            double dV1, G1, G2, qu_inf, a_win = 0.0, J_win = 0.0;
            bool ok = true, stop = false, accepted = false;
            do {   // at most twice: a failed sweep / line search with the second-order term is redone without it
                if constexpr (LOG) { lg.bumps = 0; lg.tried = 0; }
                while (true) {
                    ok = backward_sweep<M>(A.c, N, P, dft, rec, gains, mu, theta, s, lane, dV1, G1, G2, qu_inf, gap > 0.0 SDDP_T_PASS);
                    if (ok) break;
                    if (theta != 0.0) { theta = 0.0; continue; }
                    mu = fmax(mu, 0.0) * 10.0 + o.mu_min;
                    if constexpr (LOG) ++lg.bumps;
                    if (mu > o.mu_max) break;
                }
                if (!ok) { status = 2; stop = true; break; }
                const double dV2 = -0.5 * dV1;
                expected = -(dV1 + dV2);
                if (expected < o.cost_reduction_ths && gap <= o.gap_tol) { converged = 1; status = 0; stop = true; break; }
                const double A1 = dV1 + G1, B2 = dV2 + G2;
                if (gap > 0.0) rho = fmax(rho, 2.0 * fmax(fmax(A1, A1 + B2), 0.0) / gap);
                const double slack = 1e-13 * (fabs(J) + rho * gap);
                // ---- line search: lane j tries alpha_0 * factor^j (the ladder of ddp.py:20-28 in one pass)
                accepted = false;
                double a_base = o.alpha_0;
                while (a_base >= o.alpha_converge_threshold) {
                    double a = a_base;
                    for (int j = 0; j < lane; ++j) a *= o.line_search_decrease_factor;
                    const bool valid = a >= o.alpha_converge_threshold;
                    SDDP_TICK(9)
                    double* xw = xc + size_t(wr) * kSlots * XS;
                    double* uw = uc + size_t(wr) * kSlots * US;
                    double Jl = rollout<M, false>(A.c, N, x0, P, xs, us, dft, gains, xw, uw, a, -1, lane, s, gap > 0.0);
                    SDDP_TICK(8)
                    ++rollouts;
                    const double pred = a * A1 + a * a * B2 - a * rho * gap;
                    const double dphi = (Jl + rho * (1.0 - a) * gap) - (J + rho * gap);
                    const bool good = valid && (fabs(Jl) < 1e300) && (dphi <= o.beta * pred + slack);
                    const unsigned long long mask = __ballot(good);
                    if (mask) {
                        win = __ffsll((long long)mask) - 1;
                        if constexpr (LOG) lg.tried += win + 1;
                        a_win = __shfl(a, win, kWave);
                        J_win = __shfl(Jl, win, kWave);
                        if (win >= kSlots) {   // the winner is not one of the kept candidates: roll it again into slot 0
                            wave_sync();
                            rollout<M, false>(A.c, N, x0, P, xs, us, dft, gains, xw, uw, a, win, lane, s, gap > 0.0);
                            ++rollouts;
                            win = 0;
                        }
                        accepted = true;
                        break;
                    }
                    if constexpr (LOG) lg.tried += __popcll(__ballot(valid));
                    a_base = __shfl(a, kWave - 1, kWave) * o.line_search_decrease_factor;
                }
                if constexpr (LOG) {
                    if (lg.n < G.rows) {
                        if (lane == 0)
                            log_record(G, b, lg.n, J, A1, B2, rho, gap, expected, accepted ? a_win : 0.0, accepted ? J_win : 0.0, theta, mu,
                                       lg.tried, slack, iters + (accepted ? 1 : 0), rollouts, lg.bumps);
                        ++lg.n;
                    }
                }
                if (accepted) break;
                if (theta != 0.0) { theta = 0.0; continue; }                       // redo with the plain Gauss-Newton step
                // alpha fell below alpha_converge_threshold: stop.  An optimum only with closed gaps and (next to) no predicted
                // decrease either; otherwise the line search has stalled (status 4, not converged)
                alpha = 0.0; stop = true;
                converged = (gap <= o.gap_tol && expected <= o.cost_reduction_ths * fmax(1.0, fabs(J))) ? 1 : 0;
                status = converged ? 0 : 4;
                break;
            } while (true);
            if (stop) break;
            alpha = a_win;
            theta = (o.second_order && alpha == o.alpha_0) ? 1.0 : 0.0;
            const double dJ = J - J_win;
            J = J_win;
            wave_sync();
            xs = xc + (size_t(wr) * kSlots + win) * XS;          // the accepted candidate becomes the iterate; next pass writes
            us = uc + (size_t(wr) * kSlots + win) * US;          // the other set
            wr ^= 1;
            const double oma = 1.0 - alpha;
            if (gap > 0.0) {
                for (int e = lane; e < N * NX; e += kWave) dft[e] *= oma;     // a full step writes exact zeros
            }
            gap *= oma;
            ++iters;
            if (mu > o.mu0) mu = fmax(o.mu0, mu * 0.1);
            wave_sync();
            if (fabs(dJ) < o.cost_reduction_ths && gap <= o.gap_tol) { converged = 1; status = 0; break; }
        }
    // ---- results live in A.xs/A.us: copy back if the iterate ended in the candidate buffers
    wave_sync();
    double* xs0 = A.xs + size_t(b) * (N + 1) * NX;
    if (xs != xs0) {
        double* us0 = A.us + size_t(b) * N * NU;
        for (int e = lane; e < (N + 1) * NX; e += kWave) xs0[e] = xs[e];
        for (int e = lane; e < N * NU; e += kWave) us0[e] = us[e];
    }
#ifdef SDDP_STAMPS
    SDDP_TICK(9)
    if (lane == 0) for (int i = 0; i < kScal; ++i) A.scal[size_t(b) * kScal + i] = (double)T_[i];
#endif
    if (lane == 0) {
        sddp_stats st;
        st.cost = J; st.alpha = alpha; st.gap = gap; st.mu = mu; st.expected = expected; st.rho = rho;
        st.iters = iters; st.converged = converged; st.status = status; st.rollouts = rollouts;
        A.stats[b] = st;
        A.hist[b] = iters;
    }
    if constexpr (RESUME) {
        if (status == 1) {
            double* cr = R.carry + size_t(b) * N * NX;
            for (int e = lane; e < N * NX; e += kWave) cr[e] = dft[e];
        }
        if (lane == 0) R.flag(b) = status == 1 ? 1 : 0;
    }
    if constexpr (LOG) {
        if (lane == 0) G.count[b] = lg.n;      // (a fresh solve that wrote nothing: 0)
    }
    wave_sync();
}

// -----------------------------------------------------------------------------------------------------------------
// Heterogeneous fleets (sddp_set_instance_consts): a kernel that runs the model is ONE template with two instantiations.
// `Tab...` is empty (the homogeneous kernel: its argument list is the one it always had, the constants are the kernel-argument
// copy `A.c` / `c`) or holds one `const DevConsts*`, a table with one DevConsts row per instance, passed behind the common
// arguments; the per-instance body then runs on a copy of the arguments whose `c` is instance b's row.  The body rebuilds
// everything it derives from `c` (LDS tables, constant blocks) at the start of every instance, so nothing of one robot outlives
// its solve.  b is wave-uniform (blockIdx, readfirstlane, the LDS queue word) and the table is read-only for the whole launch:
// the row is read through the constant address space, i.e. by scalar loads into the registers the kernel-argument copy occupies
// in the homogeneous instantiation.  consts_of / args_of / index_of are all that tells the instantiations apart: without a table
// they hand their argument back, so the homogeneous kernel contains nothing it did not contain before there was a table.  (The
// policy kernels are the exception: policy_kernel_h below.)
// -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ DevConsts row_of(const DevConsts* __restrict__ ctab, const int b) {
    static_assert(sizeof(DevConsts) % sizeof(unsigned long long) == 0, "a row is copied in 64-bit words");
    constexpr int W = int(sizeof(DevConsts) / sizeof(unsigned long long));
    typedef const unsigned long long __attribute__((address_space(4))) * WordPtr;
    const WordPtr src = (WordPtr)(ctab + b);
    unsigned long long w[W];
#pragma unroll
    for (int i = 0; i < W; ++i) w[i] = src[i];
    DevConsts c;
    __builtin_memcpy(&c, w, sizeof(c));
    return c;
}
// the constants of instance b for the kernels that take them first (ConstsArg): the kernel's own, or row b of the table
__device__ __forceinline__ const DevConsts& consts_of(const DevConsts& c, const int) { return c; }
__device__ __forceinline__ DevConsts consts_of(const DevConsts* __restrict__ ctab, const int b) { return row_of(ctab, b); }
// The trailing arguments of a kernel that takes SolveArgs first are a subset of (ResumeArgs, LogArgs, const DevConsts* table), in
// this order, and are picked out of the pack BY TYPE: the types of the pack are all that tells a kernel's instantiations apart.
// Types are compared as the kernels declare them (KernelArg: a pointer is __restrict__ there, and is deduced so).
template <class T, class... Pack>
constexpr bool has_arg() { return (std::is_same_v<typename KernelArg<T>::type, typename KernelArg<Pack>::type> || ...); }
// the argument of type T out of a..., or the stand-in `none` where there is no such argument; by reference either way
template <class T, class None>
__device__ __forceinline__ const None& arg_of(const None& none) { return none; }
template <class T, class None, class Head, class... Rest>
__device__ __forceinline__ decltype(auto) arg_of(const None& none, const Head& head, const Rest&... rest) {
    if constexpr (has_arg<T, Head>()) return (head); else return arg_of<T>(none, rest...);
}
// ... and its type: T, or None
template <class T, class None, class... Pack>
using ArgOr = std::conditional_t<has_arg<T, Pack...>(), T, None>;
// the lookup on the six packs in use: the argument asked for where the pack holds it, the stand-in where it does not
template <class T, class None, class... Pack>
using ArgOfResult = decltype(arg_of<T>(std::declval<const None&>(), std::declval<const typename KernelArg<Pack>::type&>()...));
template <bool RES, bool LOG, bool TAB, class... Pack>
constexpr bool arg_lookup_is =
    std::is_same_v<ArgOfResult<ResumeArgs, NoResume, Pack...>, std::conditional_t<RES, const ResumeArgs&, const NoResume&>> &&
    std::is_same_v<ArgOfResult<LogArgs, NoLog, Pack...>, std::conditional_t<LOG, const LogArgs&, const NoLog&>> &&
    std::is_same_v<ArgOfResult<const DevConsts*, NoLog, Pack...>, std::conditional_t<TAB, const DevConsts* __restrict__ const&, const NoLog&>> &&
    has_arg<ResumeArgs, Pack...>() == RES && has_arg<LogArgs, Pack...>() == LOG && has_arg<const DevConsts*, Pack...>() == TAB;
static_assert(arg_lookup_is<false, false, false> && arg_lookup_is<false, false, true, const DevConsts*>, "the ordinary kernels");
static_assert(arg_lookup_is<true, false, false, ResumeArgs> && arg_lookup_is<true, false, true, ResumeArgs, const DevConsts*>, "the RESUME kernels");
static_assert(arg_lookup_is<true, true, false, ResumeArgs, LogArgs> && arg_lookup_is<true, true, true, ResumeArgs, LogArgs, const DevConsts*>, "the LOG kernels");
// the arguments of instance b: the kernel's own, or with a table a copy whose `c` is row b of it.  The copy is made behind a
// __restrict__ parameter of its own: with the table handed to row_of straight out of the pack, every table kernel of the srbd
// models came out with another schedule and register allocation.
__device__ __forceinline__ SolveArgs args_with_row(const SolveArgs& A, const int b, const DevConsts* __restrict__ ctab) {
    SolveArgs R = A;
    R.c = row_of(ctab, b);
    return R;
}
template <class... Extra>
__device__ __forceinline__ decltype(auto) args_of(const SolveArgs& A, const int b, const Extra&... extra) {
    if constexpr (has_arg<const DevConsts*, Extra...>()) return args_with_row(A, b, arg_of<const DevConsts*>(nullptr, extra...));
    else return (A);
}
// a queue position's instance index: with a table made wave-uniform, for the scalar loads of the row
template <class... Extra>
__device__ __forceinline__ int index_of(const int b, const Extra&...) {
    if constexpr (has_arg<const DevConsts*, Extra...>()) return __builtin_amdgcn_readfirstlane(b); else return b;
}
// first argument of the kernels that take their constants by value: the table stands in its place
template <class... Tab>
using ConstsArg = std::conditional_t<sizeof...(Tab) == 0, DevConsts, const DevConsts*>;

// The launch as a work queue: one resident wavefront (slot) per workgroup, each solving instances until the queue is empty.
// No workgroup ever waits for another one, so any grid size terminates; a slot's work buffers are private to its wavefront
// (its own loads and stores are seen in program order), the per-instance inputs were written before the launch.
// Every instance starts from freshly built LDS tables, so a result does not depend on which slot solved it or on what that
// slot solved before: bit-identical to one launch per instance.
// Which instantiation of the instance body runs is read off the pack: RESUME with ResumeArgs in it, LOG with LogArgs.
template <class M, class... Tab>
__device__ __forceinline__ void solve_queue(const SolveArgs& A, double* s, typename KernelArg<Tab>::type... ctab) {
    constexpr bool RESUME = has_arg<ResumeArgs, Tab...>(), LOG = has_arg<LogArgs, Tab...>();
    using Res = ArgOr<ResumeArgs, NoResume, Tab...>;
    using Lg = ArgOr<LogArgs, NoLog, Tab...>;
    const int slot = blockIdx.x;
    const bool queued = A.qhead != nullptr;
    int i = slot;                                      // no queue: workgroup w solves instance first + w
    if (threadIdx.x == 0) A.slot_clock(slot)[0] = wall_clock64();
    if (queued) {
        if (threadIdx.x == 0) i = atomicAdd(A.qhead, 1);
        i = __builtin_amdgcn_readfirstlane(i);
    }
    while (i < A.count) {                              // every wavefront reaches the exit: the head only grows
        const int b = index_of((queued && A.order) ? A.order[i] : A.first + i, ctab...);
        // one call site: the body is compiled once
        solve_instance<M, RESUME, Res, LOG, Lg>(args_of(A, b, ctab...), s, b, slot, arg_of<ResumeArgs>(NoResume(), ctab...), arg_of<LogArgs>(NoLog(), ctab...));
        if (!queued) break;
        if (threadIdx.x == 0) i = atomicAdd(A.qhead, 1);
        i = __builtin_amdgcn_readfirstlane(i);
    }
    if (threadIdx.x == 0) A.slot_clock(slot)[1] = wall_clock64();
}

// two builds of the same body: the register allocation is the only difference (sddp_options.waves_per_simd)
template <class M, bool RESUME, class... Tab>
__global__ __launch_bounds__(kWave) void solve_kernel(SolveArgs A, typename KernelArg<Tab>::type... ctab) {
    static_assert(RESUME == has_arg<ResumeArgs, Tab...>(), "RESUME names the instantiation, the pack decides it");
    extern __shared__ __attribute__((aligned(16))) double s[];
    solve_queue<M, Tab...>(A, s, ctab...);
}
template <class M, bool RESUME, class... Tab>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(2))) void solve_kernel_w2(SolveArgs A, typename KernelArg<Tab>::type... ctab) {
    static_assert(RESUME == has_arg<ResumeArgs, Tab...>(), "RESUME names the instantiation, the pack decides it");
    extern __shared__ __attribute__((aligned(16))) double s[];
    solve_queue<M, Tab...>(A, s, ctab...);
}

// -----------------------------------------------------------------------------------------------------------------
// Policy export (sddp_policy_range_device): ONE backward sweep per instance at the RETURNED iterate, behind the solve launch; the
// gains of the first `keep` knots of every instance go to a compact per-instance record
//     pol [B][keep * NU * (NX + 1) + kPolicyTail]:  knot 0 .. keep - 1: kff (NU) then K (NU x NX) row-major  |  mu_used | theta_used |
//                                                   expected = -(dV1 + dV2) | ok
// The sweep is the solve's own device code (backward_sweep<M, KEEP>: same knot loop, same Gauss-Jordan, same expand_var); what it
// carries in is what the solve would carry into its NEXT sweep: mu = stats.mu, theta = 1 iff second_order and the last step was a
// full one, the defects of the returned trajectory -- exact zeros once the gaps are closed (stats.gap <= gap_tol: the engines carry
// exact zeros from the first full step on) -- and on a non-positive pivot the solve's rule (theta -> 0, then mu <- 10 max(mu, 0) +
// mu_min, give up above mu_max: ok = 0 and the record's gains are zeros); behind a solve that ended with status 3 (non-finite cost)
// no sweep is made: ok = 0, zeros, mu_used = stats.mu.  dft / rec are the work buffers of the queue SLOT; the
// slot's gains buffer (sddp_device_ptr(3)) is not touched.
// -----------------------------------------------------------------------------------------------------------------
constexpr int kPolicyTail = 4;
// Value export (sddp_enable_value): word 0 of the nodes < vnodes of an instance's value record, c_k = the cost of the stored trajectory
// from node k on: c_N = L_N, c_k = L_k + c_{k+1}, added in this order.  L is the model code's own (M::step / M::term_cost: what
// sddp_eval_knots returns), one lane per knot, 64 knots at a time from the horizon's end; the running sum passes through the lanes in
// knot order (one shuffle and one add per knot), so the sum does not depend on N's relation to the wavefront.  Called by ONE wavefront.
template <class M>
__device__ __forceinline__ void value_costs(const DevConsts& c, const int N, const double* __restrict__ xs, const double* __restrict__ us,
                                            const double* __restrict__ P, double* __restrict__ vout, const int vnodes, const int lane) {
    constexpr int NX = M::NX, NU = M::NU, NP = M::NP;
    double run = 0.0;                                    // c_{k+1}: wave-uniform
    for (int base = (N / kWave) * kWave; base >= 0; base -= kWave) {
        const int k = base + lane;
        double Lk = 0.0;
        if (k <= N) {
            double x[NX];
#pragma unroll
            for (int i = 0; i < NX; ++i) x[i] = xs[k * NX + i];
            if (k < N) {
                double u[NU], xn[NX];
#pragma unroll
                for (int i = 0; i < NU; ++i) u[i] = us[k * NU + i];
                Lk = M::step(c, x, u, P + k * NP, k, xn);
            } else {
                Lk = M::term_cost(c, x, P + k * NP);
            }
        }
        double ck = 0.0;
        for (int j = (N - base < kWave - 1 ? N - base : kWave - 1); j >= 0; --j) {
            const double Lj = __shfl(Lk, j, kWave);
            run = base + j == N ? Lj : Lj + run;
            if (lane == j) ck = run;
        }
        if (k <= N && k < vnodes) vout[size_t(k) * value_words(NX)] = ck;
    }
}
template <class M>
__device__ __forceinline__ void policy_instance(const SolveArgs& A, double* s, const int b, const int slot, double* __restrict__ pol,
                                                const int keep, double* __restrict__ val, const int vnodes) {
    constexpr int NX = M::NX, NU = M::NU, NP = M::NP, NREC = M::NREC, NGW = NU * (NX + 1);
    const int lane = threadIdx.x;
    const int N = A.N;
    const sddp_options& o = A.o;
    const double* P = A.P + size_t(b) * (N + 1) * NP;
    const double* xs = A.xs + size_t(b) * (N + 1) * NX;
    const double* us = A.us + size_t(b) * N * NU;
    double* dft = A.dft + size_t(slot) * N * NX;
    double* rec = A.rec + size_t(slot) * (N + 1) * NREC;
    double* out = pol + size_t(b) * (size_t(keep) * NGW + kPolicyTail);
    double* vout = val ? val + size_t(b) * vnodes * value_words(NX) : nullptr;      // value export: null = off (wave-uniform)
    const sddp_stats st = A.stats[b];
    sweep_tables<M>(A.c, s, lane);
    const bool has_gap = st.gap > o.gap_tol;
    if (has_gap) {
        double J, gap;
        phase_defects<M>(A.c, N, xs, us, P, dft, lane, J, gap);
    }
    phase_derivs<M>(A.c, N, xs, us, P, rec, lane);
    wave_sync();
    double mu = st.mu, theta = (o.second_order && st.alpha == o.alpha_0) ? 1.0 : 0.0;
    double dV1, G1, G2, qu_inf;
    bool ok = false;
    SDDP_T_DECL
    // an iterate the solve refused for its non-finite cost (status 3) has no policy: the solve makes no sweep there, and a sweep
    // whose Quu happens to stay finite would pass and put the NaN into the gains.  Wave-uniform: one record read by every lane.
    if (st.status != 3) while (true) {
        ok = backward_sweep<M, true>(A.c, N, P, dft, rec, out, mu, theta, s, lane, dV1, G1, G2, qu_inf, has_gap SDDP_T_PASS, keep, vout, vnodes);
        if (ok) break;
        if (theta != 0.0) { theta = 0.0; continue; }
        mu = fmax(mu, 0.0) * 10.0 + o.mu_min;
        if (!(mu <= o.mu_max)) break;
    }
    if (!ok) {   // regularisation overflow or a status-3 iterate: zeros, never the rows a failed sweep left behind
        drain_vmem();
        for (int e = lane; e < keep * NGW; e += kWave) out[e] = 0.0;
    }
    if (vout) {   // the value record of the sweep that passed: its costs c_k; ok = 0: every word 0.0, like the gains
        if (ok) value_costs<M>(A.c, N, xs, us, P, vout, vnodes, lane);
        else for (int e = lane; e < vnodes * value_words(NX); e += kWave) vout[e] = 0.0;
    }
    if (lane == 0) {
        double* tail = out + size_t(keep) * NGW;
        tail[0] = mu; tail[1] = theta; tail[2] = ok ? -0.5 * dV1 : 0.0; tail[3] = ok ? 1.0 : 0.0;
    }
    wave_sync();
}

// a work queue like the solve launch (solve_queue), in index order: every instance costs one sweep (A.order set: a masked launch, the
// solve's hand-out).  The table kernel is written out beside the plain one: every form that folded the two into one template moved
// the register allocation of one of them (profiles/hetero_merge/README.md).
template <class M>
__global__ __launch_bounds__(kWave) void policy_kernel(SolveArgs A, double* __restrict__ pol, int keep, double* __restrict__ val, int vnodes) {
    extern __shared__ __attribute__((aligned(16))) double s[];
    const int slot = blockIdx.x;
    const bool queued = A.qhead != nullptr;
    int i = slot;
    if (queued) {
        if (threadIdx.x == 0) i = atomicAdd(A.qhead, 1);
        i = __builtin_amdgcn_readfirstlane(i);
    }
    while (i < A.count) {
        policy_instance<M>(A, s, A.order ? A.order[i] : A.first + i, slot, pol, keep, val, vnodes);
        if (!queued) break;
        if (threadIdx.x == 0) i = atomicAdd(A.qhead, 1);
        i = __builtin_amdgcn_readfirstlane(i);
    }
}
template <class M>
__global__ __launch_bounds__(kWave) void policy_kernel_h(SolveArgs A, double* __restrict__ pol, int keep, double* __restrict__ val, int vnodes,
                                                         const DevConsts* __restrict__ ctab) {
    extern __shared__ __attribute__((aligned(16))) double s[];
    const int slot = blockIdx.x;
    const bool queued = A.qhead != nullptr;
    int i = slot;
    if (queued) {
        if (threadIdx.x == 0) i = atomicAdd(A.qhead, 1);
        i = __builtin_amdgcn_readfirstlane(i);
    }
    while (i < A.count) {
        const int b = index_of(A.order ? A.order[i] : A.first + i, ctab);
        policy_instance<M>(args_of(A, b, ctab), s, b, slot, pol, keep, val, vnodes);
        if (!queued) break;
        if (threadIdx.x == 0) i = atomicAdd(A.qhead, 1);
        i = __builtin_amdgcn_readfirstlane(i);
    }
}

// Queue order for a COLD queue (sddp_options.queue_order = 2): the key of an instance is the total cost of its warm start
// (x_0 := x0 as the solve does; multiple-shooting cost of the given xs / us), evaluated here by one wavefront per instance, one
// lane per knot -- the same model code and the same sum the solve itself starts from.  The keys are then sorted in descending
// order (sddp_sort.hip): the instances farthest from their optimum start first.  Nothing here depends on an earlier solve.
// With a table (a heterogeneous fleet) every instance's warm start is priced with its own robot.
template <class M, class... Tab>
__global__ __launch_bounds__(kWave) void queue_cost_key_kernel(ConstsArg<Tab...> consts, int N, int first, int count,
                                                               const double* __restrict__ x0, const double* __restrict__ P,
                                                               const double* __restrict__ xs, const double* __restrict__ us,
                                                               double* __restrict__ key, int* __restrict__ idx) {
    constexpr int NX = M::NX, NU = M::NU, NP = M::NP;
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= count) return;
    const int b = first + i;
    const DevConsts& c = consts_of(consts, b);
    const double* xb = xs + size_t(b) * (N + 1) * NX;
    const double* ub = us + size_t(b) * N * NU;
    const double* Pb = P + size_t(b) * (N + 1) * NP;
    double Jl = 0.0;
    for (int k = lane; k <= N; k += kWave) {
        double x[NX];
        const double* xk = k == 0 ? x0 + size_t(b) * NX : xb + k * NX;
#pragma unroll
        for (int j = 0; j < NX; ++j) x[j] = xk[j];
        if (k < N) {
            double u[NU], xn[NX];
#pragma unroll
            for (int j = 0; j < NU; ++j) u[j] = ub[k * NU + j];
            Jl += M::step(c, x, u, Pb + k * NP, k, xn);
        } else {
            Jl += M::term_cost(c, x, Pb + k * NP);
        }
    }
    const double J = wave_sum(Jl);
    if (lane == 0) {
        key[i] = (J == J) ? J : __builtin_huge_val();      // a non-finite start sorts first (it ends at once with status 3)
        idx[i] = b;
    }
}

// -----------------------------------------------------------------------------------------------------------------
// single-phase kernels for the parity tests (same device code as the fused kernel): the knot evaluation, one backward sweep, one
// forward rollout.  The other kernels that only read -- model step, policy rollout, the plan inspectors -- are in sddp_inspect.hpp,
// which a unit of its own instantiates.  eval_knots_kernel reads only as well and stays here, in the main unit, on purpose: it is the
// second caller of M::F_entry beside the sweeps, and without it in their module six of the eight 4-wave main units come out with
// reordered address arithmetic in their solve, backward and policy kernels (profiles/inspect_unit/README.md).  It has one
// instantiation per build and no table form.
// -----------------------------------------------------------------------------------------------------------------
// one wavefront per knot: lane 0 runs the scalar model code, all lanes expand the dense tiles
template <class M>
__global__ __launch_bounds__(kWave) void eval_knots_kernel(DevConsts c, int N, int nk, const int* __restrict__ kk,
                                                           const double* __restrict__ x, const double* __restrict__ u,
                                                           const double* __restrict__ p, double* __restrict__ rec,
                                                           double* f_out, double* F_out, double* H_out, double* g_out,
                                                           double* L_out) {
    constexpr int NX = M::NX, NU = M::NU, NZ = M::NZ, NP = M::NP, NREC = M::NREC;
    const int t = blockIdx.x, lane = threadIdx.x;
    if (t >= nk) return;
    const int k = kk[t];
    double* r = rec + size_t(t) * NREC;
    if (lane == 0) {
        double xl[NX], ul[NU], xn[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) xl[i] = x[t * NX + i];
#pragma unroll
        for (int i = 0; i < NU; ++i) ul[i] = u[t * NU + i];
        M::derivs(c, xl, ul, p + t * NP, k, N, r);
        double L;
        if (k < N) {
            L = M::step(c, xl, ul, p + t * NP, k, xn);
        } else {
            L = M::term_cost(c, xl, p + t * NP);
#pragma unroll
            for (int i = 0; i < NX; ++i) xn[i] = xl[i];
        }
        L_out[t] = L;
#pragma unroll
        for (int i = 0; i < NX; ++i) f_out[t * NX + i] = xn[i];
    }
    wave_sync();
    for (int e = lane; e < NX * NZ; e += kWave) F_out[size_t(t) * NX * NZ + e] = k < N ? M::F_entry(c, r, e / NZ, e % NZ) : 0.0;
    for (int e = lane; e < NZ * NZ; e += kWave) {
        const int i = e / NZ, j = e % NZ;
        H_out[size_t(t) * NZ * NZ + e] = (k < N || (i < NX && j < NX)) ? M::H_entry(c, r, p + t * NP, k, N, i, j) : 0.0;
    }
    for (int e = lane; e < NZ; e += kWave) g_out[t * NZ + e] = r[M::REC_G + e];
}

template <class M, class... Tab>
__global__ __launch_bounds__(kWave) void backward_kernel(SolveArgs K, Tab __restrict__... ctab) {
    extern __shared__ __attribute__((aligned(16))) double s[];
    constexpr int NX = M::NX, NU = M::NU, NP = M::NP, NREC = M::NREC;
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= K.B) return;
    const SolveArgs& A = args_of(K, b, ctab...);
    const int N = A.N;
    const double* P = A.P + size_t(b) * (N + 1) * NP;
    double* xs = A.xs + size_t(b) * (N + 1) * NX;
    double* us = A.us + size_t(b) * N * NU;
    double* dft = A.dft + size_t(b) * N * NX;
    double* gains = A.gains + size_t(b) * N * (NU * (NX + 1));
    double* rec = A.rec + size_t(b) * (N + 1) * NREC;
    double J, gap;
    sweep_tables<M>(A.c, s, lane);
    phase_defects<M>(A.c, N, xs, us, P, dft, lane, J, gap);
    phase_derivs<M>(A.c, N, xs, us, P, rec, lane);
    wave_sync();
    double dV1, G1, G2, qu_inf;
    SDDP_T_DECL
    const bool has_gap = K.first == 0;      // (SolveArgs::first: closed gaps of sddp_debug_set_phase_mode; A.alpha: its theta)
    const bool ok = backward_sweep<M>(A.c, N, P, dft, rec, gains, A.mu, A.alpha, s, lane, dV1, G1, G2, qu_inf, has_gap SDDP_T_PASS);
    if (lane == 0) {
        double* sc = A.scal + size_t(b) * kScal;
        sc[0] = dV1; sc[1] = -0.5 * dV1; sc[2] = G1; sc[3] = G2; sc[4] = ok ? 1.0 : 0.0; sc[5] = A.mu; sc[6] = qu_inf; sc[7] = J;
    }
}

template <class M, class... Tab>
__global__ __launch_bounds__(kWave) void forward_kernel(SolveArgs K, Tab __restrict__... ctab) {
    extern __shared__ __attribute__((aligned(16))) double s[];
    constexpr int NX = M::NX, NU = M::NU, NP = M::NP;
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= K.B) return;
    const SolveArgs& A = args_of(K, b, ctab...);
    const int N = A.N;
    const double J = rollout<M, false>(A.c, N, A.x0 + size_t(b) * NX, A.P + size_t(b) * (N + 1) * NP,
                                       A.xs + size_t(b) * (N + 1) * NX, A.us + size_t(b) * N * NU,
                                       A.dft + size_t(b) * N * NX, A.gains + size_t(b) * N * (NU * (NX + 1)),
                                       A.xn + size_t(b) * (N + 1) * NX, A.un + size_t(b) * N * NU, A.alpha, 0, lane, s,
                                       K.first == 0);      // (SolveArgs::first: closed gaps of sddp_debug_set_phase_mode)
    if (lane == 0) A.scal[size_t(b) * kScal] = J;
}

}  // namespace sddp
