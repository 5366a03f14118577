// sddp_handle.hpp -- the handle behind include/sddp.h and the per-model operation table.
//
// The library is built from the translation units of the model builds (sddp_inst.hip, compiled per entry of
// srbd_horizon_amd/_lib.py INSTANCES as its main unit, its inspect unit and, for a plain build, one unit per further solve variant:
// _lib.translation_units, in parallel) plus the model-independent host code (sddp_api.hip).  A model build reaches
// the API through a ModelOps table: what the build is (model, traits), and plain function pointers to what it can do.  Nothing
// templated crosses a translation unit, and sddp_api.hip asks the table instead of knowing the builds.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sddp.h"
#include "sddp_kernels.hpp"

struct sddp_handle;

namespace sddp {

struct Dims {
    int nx, nu, np, nrec;
};

// the built-in model (SDDP_MODEL_*) of a model name, -1: none
inline int model_of_name(const char* name) {
    static const char* const names[] = {"srbd13", "srbd37", "lip30", "srbd61"};      // in the order of sddp.h's SDDP_MODEL_* values
    static_assert(SDDP_MODEL_SRBD13 == 0 && SDDP_MODEL_SRBD37 == 1 && SDDP_MODEL_LIP30 == 2 && SDDP_MODEL_SRBD61 == 3, "order of names");
    for (int i = 0; i < 4; ++i)
        if (std::strcmp(name, names[i]) == 0) return i;
    return -1;
}

// The variants of the solve kernels: what a solve launch passes behind SolveArgs, and so which instantiation it runs: nothing,
// ResumeArgs (a handle with a carry buffer, sddp_enable_resume), ResumeArgs and LogArgs (... and a log buffer,
// sddp_enable_iteration_log).  THE list: a variant is a value here, its arguments in sddp_launch.hpp variant_args and its units'
// suffix in srbd_horizon_amd/_lib.py VARIANTS, in the same order.
enum SolveVariant { kSolvePlain = 0, kSolveResume, kSolveLog, kSolveVariants };

// the solve kernel of a launch (ModelOps::SolveOps::choose): its address, the build it belongs to (wavefronts per SIMD: 1, or 2 for
// the half-register-file build), its resident workgroups on this device, and its launch shape
struct SolveChoice {
    const void* kern;
    int wps, slots, threads;
    size_t lds;
};

// The trajectory a plan inspector reads (plan audit, stationarity certificate, cost breakdown: sddp_api.hip plan_source).  An inspector
// runs one wavefront per instance of a range [first, first + count) of a handle that has solved at least once; instance first + i reads
// trajectory block xoff + i of x / u -- the handle's own plan {h->xs, h->us, first} or a caller's trajectory {d_x, d_u, 0}, whose block
// i belongs to instance first + i --, row first + i of the last solve's parameters and its own constants, and stores to nothing but
// the caller's outputs.
struct PlanSource {
    const double *x, *u;
    int xoff;
};

// what a model build is and provides (sddp_launch.hpp: make_ops<M>)
struct ModelOps {
    // the build's key: a handle's build is the one whose model and traits are the ones asked for (sddp_api.hip model_ops)
    int model;             // the built-in model it is a build of (a user build: the model it was generated for)
    bool bar, so2, xr;     // barrier build; full second-order build (second_order = 2); user rows.  None of them: a plain build
    bool table_kernels;    // every kernel has a table form (per-instance constants, sddp_set_instance_consts): the plain builds
    Dims dims;
    // the parameter columns the class label reads (sddp_enable_auto_classes; sddp_models.hpp P_CMD0 / P_CMD1 / P_SW_L / P_SW_R): the
    // commanded velocity x, y and the switch of the first contact of the left and of the right foot
    int col_cmd[2] = {0, 0}, col_sw[2] = {0, 0};
    bool uses_mw;          // 4 wavefronts per instance (sddp_kernels_mw.hpp); else one
    bool w2_build;         // a half-register-file build exists (two instances per SIMD / two workgroups per CU)
    const char* name;      // kernel-facing model name (bench / profiles)
    int (*max_slots)(sddp_handle*, int*);
    // what a solve launch asks of the build, per variant of the solve kernels: choose = the kernel that the handle's state selects
    // (waves_per_simd, the table), launch = that kernel on `grid` workgroups.  The launch sequence around them is the core's
    // (sddp_api.hip launch_solve_sequence).  [kSolvePlain] is always set; the others are null where the build has none (every build
    // with traits), and are compiled in a translation unit of their own each (sddp_inst.hip with -DSDDP_INST_VARIANT=<variant>).
    struct SolveOps {
        int (*choose)(sddp_handle*, SolveChoice*) = nullptr;
        int (*launch)(sddp_handle*, const SolveChoice&, int grid, const SolveArgs&) = nullptr;
    };
    SolveOps solve[kSolveVariants];
    // the queue_order 2 / 3 key pre-pass: the initial cost of every instance of the launch, into h->cold.qkey / h->cold.order_in (main unit)
    int (*launch_cost_keys)(sddp_handle*, const SolveArgs&, int, int) = nullptr;
    int (*launch_backward)(sddp_handle*, const SolveArgs&);
    int (*launch_forward)(sddp_handle*, const SolveArgs&);
    // policy export: first, count, the policy buffer and its knots, the value buffer (or null) and its nodes; null: the build has none
    int (*launch_policy)(sddp_handle*, SolveArgs, int, int, double*, int, double*, int) = nullptr;
    // the knot evaluation of the parity tests (sddp_eval_knots; main unit, on purpose: sddp_kernels.hpp eval_knots_kernel)
    void (*launch_eval_knots)(const DevConsts&, int, int, const int*, const double*, const double*, const double*, double*, double*,
                              double*, double*, double*, double*);
    // The other kernels that only read (sddp_inspect.hpp), of every build.  They are compiled in a translation unit of their own, the
    // build's inspect unit (sddp_inst.hip with -DSDDP_INST_INSPECT; a user build: one unit holds both), so that they share no device
    // module with the solve kernels; the main unit enters the table whole (sddp_launch.hpp side_inspect_ops).
    struct InspectOps {
        // the policy rolled out from a measured state: first, count, start, steps, x_meas, x_out, u_out, cost_out; null with launch_policy
        int (*policy_rollout)(sddp_handle*, int, int, int, int, const double*, double*, double*, double*) = nullptr;
        // the covariance propagated under the policy: first, count, start, steps, Sigma0, q or null, r or null, linearised friction
        // coefficient, out, the covariances or null, diag of the input covariances or null; null with launch_policy
        int (*policy_covariance)(sddp_handle*, int, int, int, int, const double*, const double*, const double*, double, double*, double*,
                                 double*) = nullptr;
        // the value records evaluated at a measured state: first, count, node, x_meas, out; null with launch_policy
        int (*value_at)(sddp_handle*, int, int, int, const double*, double*) = nullptr;
        // the plan inspectors (PlanSource): first, count, [audit: start, steps,] the trajectory, then the inspector's own arguments --
        // audit: linearised friction coefficient, out; stationarity: out, lambda or null, reduced gradient or null; cost breakdown: the
        // user rows' table with zero weights or null, out, the per-node addends or null
        int (*audit)(sddp_handle*, int, int, int, int, PlanSource, double, double*) = nullptr;
        int (*stationarity)(sddp_handle*, int, int, PlanSource, double*, double*, double*) = nullptr;
        int (*cost_terms)(sddp_handle*, int, int, PlanSource, const double*, double*, double*) = nullptr;
        // parameter sensitivities: the costates and the record the stationarity launch stored for the range, out, the gradient or
        // null; null: a user build (its rows have no d/dp code)
        int (*param_gradient)(sddp_handle*, int, int, PlanSource, const double*, const double*, double*, double*) = nullptr;
        // constant sensitivities: the same inputs, out, the per-node addends or null; null: a user build
        int (*const_gradient)(sddp_handle*, int, int, PlanSource, const double*, const double*, double*, double*) = nullptr;
        int (*model_step)(sddp_handle*, int, const double*, const double*, const double*, double*) = nullptr;
    } inspect;
};

}  // namespace sddp

struct sddp_handle {
    int model_id = 0, N = 0, B = 0;
    sddp::Dims d{};
    const sddp::ModelOps* ops = nullptr;
    sddp_options opts{};
    sddp_model_consts consts{};
    sddp::DevConsts dc{};
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // device buffers
    double *x0 = nullptr, *P = nullptr, *xs = nullptr, *us = nullptr, *xn = nullptr, *un = nullptr, *xc = nullptr, *uc = nullptr, *dft = nullptr,
           *gains = nullptr, *rec = nullptr, *scal = nullptr;
    sddp_stats* stats = nullptr;
    // timing
    bool timing = false;
    std::vector<hipEvent_t> ev;     // pairs (start, stop), one pair per launch since the last synchronize
    size_t pending = 0;            // launches whose events have not been read yet
    double last_ms = 0.0, sum_ms = 0.0;
    long long n_ms = 0;
    std::string err;
    bool have_x0 = false, have_xws = false, have_uws = false, have_params = false;
    // work queue: the solve launch runs on `slots` resident workgroups that pull instances from a queue
    int wslots = 0;                 // slots the work buffers (xn un xc uc dft gains rec) are allocated for = min(B, resident capacity)
    int cus = 0;
    int* qhead = nullptr;           // device queue head; behind it (kQheadSelected) the two words of SDDP_BUF_SELECTED
    static constexpr int kQheadSelected = 2, kQheadInts = 4;
    int* order = nullptr;           // [B] queue order of the next launch
    int* pol_order = nullptr;       // [B] the order of a masked policy launch (made by the first one): `order` stays the last solve launch's
    bool last_masked = false;       // the last solve launch was a masked one: its order array is whole ([count]) whatever queue_order
    int* hist = nullptr;            // iterations of each instance's previous solve (-1: none), then the slot clocks (HistLayout)
    bool gains_by_instance = false; // the last solve launch ran instance b on slot b (no queue, first = 0): sddp_device_ptr(3)
    // every kernel of the model build that this handle has launched (solve builds, policy, backward, forward, without and with
    // the constants table), by address: its dynamic-LDS attribute is set and `slots` workgroups of it are resident on this device.
    // An entry is made by the first launch of the kernel and kept for the handle's life (sddp_launch.hpp kernel_slots)
    struct KInfo { const void* fn; int slots; };
    std::vector<KInfo> kernels;
    int last_grid = 0, last_queued = 0;
    int last_build = 0;             // waves_per_simd of the kernel build the last solve launch ran (sddp_kernel_info)
    const void* last_kernel = nullptr;   // ... and that kernel, its dynamic LDS bytes and its workgroups per CU (sddp_kernel_resources)
    int last_lds = 0, last_per_cu = 0;
    double* box_dev = nullptr;      // lower[64] | upper[64] of the bound barrier (barrier builds)
    double* xr_dev = nullptr;       // user rows: coefficients | weights | constants (DevConsts::xr, "_x" builds)
    double* xr_zero = nullptr;      // ... the same table with its weight words zeroed: made by the first cost breakdown (sddp_cost_terms_range_device)
    const double* last_params = nullptr;   // the parameter tensor of the last solve launch (continue launches, policy export, audit)
    // phase-level mode (sddp_debug_set_phase_mode, diagnostics): what sddp_backward / sddp_forward launch with.  Default (0, 0): the
    // Gauss-Newton sweep on open gaps, as those entry points always ran
    double phase_theta = 0.0;       // weight of the second-order term of the sweep (the solve's theta: 0 or 1)
    int phase_closed = 0;           // 1: the one-wave kernels take their closed-gap path (has_gap = false: all defects count as zero)
    // The optional state, one group per feature.  The buffers of a group exist together or not at all (sddp_api.hip acquire_group), and
    // on() is the one statement of whether they do.
    // cold-queue order (queue_order = 2): initial-cost keys of the launch, their sorted copy, the unsorted index list, sort scratch;
    // allocated together at sddp_create when the option asks for it, or on the first launch that needs them
    struct ColdQueue {
        double *qkey = nullptr, *qkey2 = nullptr;
        int* order_in = nullptr;
        void* sort_tmp = nullptr; size_t sort_tmp_bytes = 0;
        bool on() const { return sort_tmp != nullptr; }
    } cold;
    // class history (queue_order = 3): the class label per instance -- the caller's, or the handle's own (auto_cls) --, and per class
    // the iterations / solves so far.  Made by the first call that labels, for the handle's life
    struct Classes {
        int* cls = nullptr;             // [B], -1: unlabelled
        int n_cls = 0;
        unsigned long long* cls_stat = nullptr;   // [n_cls][2]
        unsigned long long* cls_in = nullptr;     // [n_cls][2] device staging of sddp_add_class_stats, made by its first call
        bool auto_cls = false;          // sddp_enable_auto_classes: every fresh solve launch labels its range first (implies on())
        bool on() const { return cls != nullptr; }
    } classes;
    // resumable solves (sddp_enable_resume): on = every solve launch runs the kernels' kSolveResume variant.  The time budget and the
    // iteration log ride on those kernels: neither exists while this group is off (sddp_api.hip drop_resume)
    struct Resume {
        double* carry = nullptr;        // [B][N][nx] defects of the instances cut at max_iters (SolveArgs::carry)
        int* resumable = nullptr;       // ResumeArgs::resumable: the flags and what shares their buffer (sddp_kernels.hpp ResumeLayout)
        // time budget (sddp_set_time_budget): budget_us > 0 = armed, and every solve / continue launch sequence is led by
        // deadline_stamp_kernel and passes budget_min_iters to the resumable kernels (ResumeArgs::budget_iters; -1 while not armed)
        double budget_us = 0.0; int budget_min_iters = 0;
        bool continuing = false;        // the solve launch being enqueued is a continue launch (sddp_continue_*)
        bool on() const { return carry != nullptr; }
    } resume;
    // iteration log (sddp_enable_iteration_log; needs `resume`): on = every solve launch runs the kSolveLog variant
    struct IterationLog {
        double* ilog = nullptr;         // [B][ilog_rows][kLogWords] one record per line search of an instance's last solve (LogArgs::log)
        int* ilog_n = nullptr;          // [B] records written (LogArgs::count)
        int ilog_rows = 0;
        bool on() const { return ilog != nullptr; }
    } log;
    // policy export (sddp_enable_policy)
    struct Policy {
        double* policy = nullptr;       // [B][policy_knots * nu * (nx + 1) + 4]
        int policy_knots = 0;
        bool on() const { return policy != nullptr; }
    } pol;
    // value export (sddp_enable_value; needs `pol`): on = every policy launch stores the value records of its range as well
    struct Value {
        double* value = nullptr;        // [B][nodes][nx * nx + nx + 2]
        int nodes = 0;
        bool on() const { return value != nullptr; }
    } val;
    // heterogeneous fleet (sddp_set_instance_consts): one DevConsts row per instance; on = every kernel of the handle is launched in
    // its table instantiation, which reads instance b's row instead of the kernel-argument copy of `dc`
    struct InstanceTable {
        sddp::DevConsts* ctab = nullptr;   // [B]
        bool on() const { return ctab != nullptr; }
    } table;
    // costates of a call (sddp_api.hip costates: the parameter and the constant sensitivities): where the stationarity launch of a call
    // leaves the costates and its record for the kernel behind it; made by the first call, for the handle's life.  Block i belongs to
    // instance first + i of the call
    struct Costates {
        double* lam = nullptr;          // [B][N + 1][nx]
        double* stat = nullptr;         // [B][kStationarityWords]
        bool on() const { return lam != nullptr; }
    } costate;
    // host staging: each buffer is made by the first call that uses it and kept for the handle's life, so there is nothing to switch
    // and no on(); a pinned buffer that could not be had stays null and its caller takes the pageable path (sddp_api.hip staging)
    struct Staging {
        double* tick_in = nullptr;      // [B][np + nx] staging of sddp_advance
        char* tick_pin = nullptr; int tick_flip = 0, tick_unsynced = 0;   // two pinned images of tick_in (small batches): the one last used, uploads not waited for
        double* step_buf = nullptr;     // [B][2 nx + nu + np] operands and result of sddp_model_step
        double* step_pin = nullptr;     // pinned host image of step_buf (small batches)
        char* pinned = nullptr;         // small batches: pinned host staging of x | u | stats, so the three result copies are truly asynchronous
        double *first_dev = nullptr, *first_pin = nullptr;   // [B][nu + nx + 3] packed first knots of sddp_solve_resident_first, and its pinned host image
        char* up_pin = nullptr; size_t up_off = 0;   // pinned ring for small host->device uploads of the setters (no wait per call), and its fill
    } stage;
    // every device and pinned allocation above, registered where it is made (sddp_api.hip acquire / release): what sddp_destroy frees
    struct Owned { void* p; bool pinned; };
    std::vector<Owned> owned;

    size_t n_x() const { return size_t(B) * (N + 1) * d.nx; }
    size_t n_u() const { return size_t(B) * N * d.nu; }
    size_t n_p() const { return size_t(B) * (N + 1) * d.np; }
    int policy_words() const { return pol.policy_knots * d.nu * (d.nx + 1) + 4; }
    int value_words() const { return val.nodes * sddp::value_words(d.nx); }      // per instance
    size_t n_g() const { return size_t(B) * N * d.nu * (d.nx + 1); }
};

namespace sddp {

// (a call without a handle -- sddp_create, sddp_eval_knots -- reports through sddp_api.hip's own overload: no launcher sees one)
inline int fail(sddp_handle* h, int code, const std::string& msg) { h->err = msg; return code; }

#define HIP_TRY(h, expr)                                                                               \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return sddp::fail(h, SDDP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));     \
    } while (0)

// one kernel launch on the handle's stream
template <class Fn, class... A>
int launch(sddp_handle* h, Fn kern, int grid, int threads, size_t lds, const A&... args) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, h->stream, args...);
    HIP_TRY(h, hipGetLastError());
    return SDDP_OK;
}

// The grid of a launch over `count` instances by a kernel with `slots` resident workgroups: at most the slots the work buffers exist
// for, and opts.max_slots.  More instances than that make a work queue: its head is zeroed on the stream and entered in `a`.
// A masked launch (a.order set by its pre-pass, sddp_api.hip launch_masked_order) is a queue whatever its size, and its head is
// already on the stream: the pre-pass wrote it (the order kernel of orders 0 / 1 and of a policy launch, mask_head_kernel behind the
// sort of orders 2 / 3).
inline int queue_grid(sddp_handle* h, SolveArgs& a, int slots, int count, int* grid) {
    *grid = std::min(count, std::min(slots, h->wslots));
    if (h->opts.max_slots > 0) *grid = std::min(*grid, h->opts.max_slots);
    if (a.order) {
        a.qhead = h->qhead;
    } else if (count > *grid) {
        HIP_TRY(h, hipMemsetAsync(h->qhead, 0, sizeof(int), h->stream));
        a.qhead = h->qhead;
    }
    return SDDP_OK;
}

}  // namespace sddp
