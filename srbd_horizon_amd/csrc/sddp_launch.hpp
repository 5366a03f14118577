// sddp_launch.hpp -- host-side launchers of one model build (templates on the device model), collected into a ModelOps table.
// Included by sddp_inst.hip (and by a user build's generated unit).  What a unit instantiates of it decides which kernels its
// device module holds: the main unit make_ops<M> -- the solve, policy, backward / forward and cost-key kernels --, a variant unit
// solve_ops<M, V> alone, the inspect unit (sddp_launch_inspect.hpp, which includes this file) the kernels that only read.
#pragma once
#include <algorithm>
#include <tuple>
#include <utility>

#include "sddp_handle.hpp"
#include "sddp_kernels.hpp"
#include "sddp_kernels_mw.hpp"
#include "sddp_models.hpp"

namespace sddp {

// large models (> 48 KB of LDS per instance: srbd37, srbd61, lip30) run on 4 waves per instance (sddp_kernels_mw.hpp)
template <class M>
constexpr bool use_mw() { return Lds<M>::BYTES > 48 * 1024; }
template <class M>
constexpr size_t lds_bytes() {
    if constexpr (use_mw<M>()) return LdsMW<M>::BYTES; else return Lds<M>::BYTES;
}
// a half-register-file build pays where two workgroups fit a CU's 160 KB (4-wave kernel) / always (one-wave kernel)
template <class M>
constexpr bool has_w2() {
    if constexpr (use_mw<M>()) return 2 * LdsMW<M>::BYTES <= size_t(160) * 1024; else return true;
}

template <class M>
constexpr int threads_of() { return use_mw<M>() ? kThreadsMW : kWave; }

// A build's traits are M::BAR (barrier build), M::SO2 (full second order) and M::NXR > 0 (user rows; the user builds too).  A
// PLAIN build has none of them.  This is the one statement of the rule: what only the plain builds have refers to it, and
// sddp_api.hip reads the outcome from the build's table (ModelOps::table_kernels, solve[]) instead of deriving it.
template <class M>
constexpr bool is_plain() { return !M::BAR && !M::SO2 && M::NXR == 0; }

// Heterogeneous fleets (sddp_set_instance_consts): on the plain builds every kernel has a table form that takes the handle's
// constants table behind its arguments and reads instance b's row of it (sddp_kernels.hpp args_of): a second instantiation of
// the same template, except for the policy export, whose table form is a kernel of its own (policy_kernel[_mw]_h).  sddp_api.hip
// refuses the table on every other build, so h->table.on() implies has_hetero<M>().
template <class M>
constexpr bool has_hetero() { return is_plain<M>(); }
// f(tab...): a launcher with the kernels' trailing argument pack, the handle's table when it is active and nothing otherwise.  A
// build without has_hetero never instantiates f(table), and so none of the table kernels.
template <class M, class F>
int with_table(sddp_handle* h, F f) {
    if constexpr (has_hetero<M>()) {
        if (h->table.on()) return f((const DevConsts*)h->table.ctab);
    }
    return f();
}
// the constants argument of the kernels that take it first: the handle's own constants, or the table in their place
inline const DevConsts& consts_arg(sddp_handle* h) { return h->dc; }
inline const DevConsts* consts_arg(sddp_handle*, const DevConsts* tab) { return tab; }

// Solve variants (sddp_handle.hpp SolveVariant): on the plain builds the solve kernels have two more instantiations per variant
// beyond kSolvePlain (without and with the table), told apart by what they take behind SolveArgs.  A handle with a carry buffer
// (sddp_enable_resume) launches kSolveResume, one with a log buffer as well (sddp_enable_iteration_log) kSolveLog; sddp_api.hip
// refuses either buffer on every other build.  Each variant is compiled in a translation unit of its own (sddp_inst.hip with
// -DSDDP_INST_VARIANT; solve_ops<M, V> is instantiated nowhere else): with them in the same device module the ordinary
// one-wave kernels come out with another register allocation and 4 bytes less or more scratch, though not a statement of theirs
// differs (profiles/resume/README.md, profiles/iteration_log/README.md).
// What variant V passes behind SolveArgs, in the kernels' order (the table, if any, follows): the one place that says so.
template <SolveVariant V>
auto variant_args(const sddp_handle* h) {
    [[maybe_unused]] const ResumeArgs res{h->resume.carry, h->resume.resumable, h->resume.continuing ? 1 : 0,
                                          h->resume.budget_us > 0.0 ? h->resume.budget_min_iters : -1};
    if constexpr (V == kSolveResume) return std::make_tuple(res);
    else if constexpr (V == kSolveLog) return std::make_tuple(res, LogArgs{h->log.ilog, h->log.ilog_n, h->log.ilog_rows});
    else return std::tuple<>();
}
// Policy export: the plain builds and their user-row forms, which are plain builds but for the rows (sddp_models.hpp: NXR > 0
// excludes BAR and SO2).  The barrier and second_order = 2 builds have no policy kernel.
template <class M>
constexpr bool has_policy() { return is_plain<M>() || M::NXR > 0; }

// only the kernel a model actually uses is instantiated
template <class M, class... Tab> auto pick_solve(int waves_per_simd) {      // Tab: the kernel's trailing arguments, a variant's and the table
    [[maybe_unused]] const bool w2 = waves_per_simd >= 2;
    constexpr bool RES = has_arg<ResumeArgs, Tab...>();
    if constexpr (!use_mw<M>()) return w2 ? solve_kernel_w2<M, RES, Tab...> : solve_kernel<M, RES, Tab...>;
    else if constexpr (has_w2<M>()) return w2 ? solve_kernel_mw_w2<M, RES, Tab...> : solve_kernel_mw<M, RES, Tab...>;
    else return solve_kernel_mw<M, RES, Tab...>;
}
template <class M, class... Tab> auto pick_backward() {
    if constexpr (use_mw<M>()) return backward_kernel_mw<M, Tab...>; else return backward_kernel<M, Tab...>;
}
template <class M, class... Tab> auto pick_forward() {
    if constexpr (use_mw<M>()) return forward_kernel_mw<M, Tab...>; else return forward_kernel<M, Tab...>;
}
template <class M, class... Tab> auto pick_policy() {   // the one entry point whose table kernel is a kernel of its own
    if constexpr (sizeof...(Tab) != 0) { if constexpr (use_mw<M>()) return policy_kernel_mw_h<M>; else return policy_kernel_h<M>; }
    else { if constexpr (use_mw<M>()) return policy_kernel_mw<M>; else return policy_kernel<M>; }
}

// The handle's entry for `kern` (sddp_handle::kernels), made the first time the handle meets the kernel: its dynamic-LDS attribute
// is set, and its resident workgroups on this device (the queue's slot count) are what the occupancy query gives per CU, at most
// `cap` (0: no cap) and within [1, 32], times the CUs.  slots may be null: a launch that needs the attribute only.
template <class M, class Fn>
int kernel_slots(sddp_handle* h, Fn kern, int cap, int* slots) {
    const void* fn = reinterpret_cast<const void*>(kern);
    for (const auto& k : h->kernels)
        if (k.fn == fn) { if (slots) *slots = k.slots; return SDDP_OK; }
    try { h->kernels.reserve(h->kernels.size() + 1); } catch (...) { return fail(h, SDDP_ERR_NOMEM, "out of host memory"); }
    HIP_TRY(h, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes<M>()));
    int per_cu = 0;
    HIP_TRY(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, threads_of<M>(), lds_bytes<M>()));
    if (cap > 0) per_cu = std::min(per_cu, cap);
    per_cu = std::max(1, std::min(per_cu, 32));
    h->kernels.push_back({fn, per_cu * std::max(1, h->cus)});
    if (slots) *slots = h->kernels.back().slots;
    return SDDP_OK;
}
// the one-wave solve kernel's two builds run 1 or 2 wavefronts per SIMD; the four-wave kernels take what fits
template <class M>
constexpr int solve_cap(int wps) { return use_mw<M>() ? 0 : 4 * (wps >= 2 ? 2 : 1); }

// A kernel that takes the constants first (ConstsArg<Tab...>) on `grid` workgroups of one wavefront: pick(tab...) names its
// instantiation, and the handle's constants, or its table in their place, go in front of args..., which are the kernel's remaining
// parameters in its own order.  No kernel_slots entry (at most 64 KB of LDS, no attribute) and no work buffer.
template <class M, class Pick, class... A>
int launch_waves(sddp_handle* h, Pick pick, int grid, size_t lds, const A&... args) {
    return with_table<M>(h, [&](auto... tab) { return launch(h, pick(tab...), grid, kWave, lds, consts_arg(h, tab...), args...); });
}
// the pick of a kernel template <M, Tab...>
#define SDDP_PICK(kernel) [](auto... tab) { return kernel<M, decltype(tab)...>; }

// the queue_order 2 / 3 pre-pass: the initial cost of every instance of the launch, into h->cold.qkey / h->cold.order_in
template <class M>
int launch_cost_keys(sddp_handle* h, const SolveArgs& a, int first, int count) {
    return launch_waves<M>(h, SDDP_PICK(queue_cost_key_kernel), count, 0, a.N, first, count, a.x0, a.P, a.xs, a.us, h->cold.qkey, h->cold.order_in);
}

// The solve kernels of variant V as the handle launches them: f(pick, extra...), with pick(w) the kernel of the build for w wavefronts
// per SIMD and extra... the kernels' trailing arguments, the variant's and then the table when it is active.  That one pack names the
// instantiation and is what the launch passes.
template <class M, SolveVariant V, class F>
int with_solve_kernels(sddp_handle* h, F f) {
    static_assert(V == kSolvePlain || is_plain<M>(), "the plain builds alone have solve variants");
    return with_table<M>(h, [&](auto... tab) {
        return std::apply([&](const auto&... x) { return f([](int w) { return pick_solve<M, std::decay_t<decltype(x)>...>(w); }, x...); },
                          std::tuple_cat(variant_args<V>(h), std::make_tuple(tab...)));
    });
}
// ModelOps::SolveOps of variant V.  choose: the build opts.waves_per_simd asks for, where the model has it
template <class M, SolveVariant V>
int choose_solve(sddp_handle* h, SolveChoice* c) {
    return with_solve_kernels<M, V>(h, [&](auto pick, const auto&...) {
        int wps = h->opts.waves_per_simd >= 2 && has_w2<M>() ? 2 : 1;
        auto kern = pick(wps);
        int slots = 0;
        int rc = kernel_slots<M>(h, kern, solve_cap<M>(wps), &slots);
        if (rc != SDDP_OK) return rc;
        if constexpr (use_mw<M>()) {   // a half-register-file build that the device still runs one per CU (barrier builds) has nothing to offer
            if (wps >= 2) {
                auto k1 = pick(1);
                int s1 = 0;
                rc = kernel_slots<M>(h, k1, solve_cap<M>(1), &s1);
                if (rc != SDDP_OK) return rc;
                if (s1 >= slots) { kern = k1; slots = s1; wps = 1; }
            }
        }
        *c = {reinterpret_cast<const void*>(kern), wps, slots, threads_of<M>(), lds_bytes<M>()};
        return SDDP_OK;
    });
}
template <class M, SolveVariant V>
int launch_solve(sddp_handle* h, const SolveChoice& c, int grid, const SolveArgs& a) {
    return with_solve_kernels<M, V>(h, [&](auto pick, const auto&... x) { return launch(h, pick(c.wps), grid, c.threads, c.lds, a, x...); });
}
template <class M, SolveVariant V>
ModelOps::SolveOps solve_ops() { return {choose_solve<M, V>, launch_solve<M, V>}; }
// solve_ops<M, V> for V > 0 as the build's main unit names it without instantiating it: declared here, defined (an explicit
// specialisation) by the unit compiled with -DSDDP_INST_VARIANT=V alone.  A build whose side unit is missing does not load.
template <class M, SolveVariant V>
ModelOps::SolveOps side_solve_ops();
template <class M, int... V>
void enter_side_units(ModelOps& o, std::integer_sequence<int, V...>) {
    if constexpr (is_plain<M>()) ((o.solve[V + 1] = side_solve_ops<M, SolveVariant(V + 1)>()), ...);
}
// resident capacity over the builds a handle may switch between (sddp_set_options): sizes the work buffers
template <class M>
int max_slots(sddp_handle* h, int* slots) {
    int s1 = 0, s2 = 0;
    int rc = kernel_slots<M>(h, pick_solve<M>(1), solve_cap<M>(1), &s1);
    if (has_w2<M>() && rc == SDDP_OK) rc = kernel_slots<M>(h, pick_solve<M>(2), solve_cap<M>(2), &s2);
    *slots = std::max(s1, s2);
    return rc;
}
// the phase-level entry points: one backward sweep / one forward rollout of every instance, instance b on workgroup b.  They go
// through kernel_slots for the dynamic-LDS attribute alone: the grid is h->B, the slot count of the entry is not read
template <class M, class Pick>
int launch_phase(sddp_handle* h, const SolveArgs& a, Pick pick) {
    return with_table<M>(h, [&](auto... tab) {
        auto kern = pick(tab...);
        const int rc = kernel_slots<M>(h, kern, 0, nullptr);
        if (rc != SDDP_OK) return rc;
        return launch(h, kern, h->B, threads_of<M>(), lds_bytes<M>(), a, tab...);
    });
}
template <class M>
int launch_backward(sddp_handle* h, const SolveArgs& a) {
    return launch_phase<M>(h, a, [](auto... tab) { return pick_backward<M, decltype(tab)...>(); });
}
template <class M>
int launch_forward(sddp_handle* h, const SolveArgs& a) {
    return launch_phase<M>(h, a, [](auto... tab) { return pick_forward<M, decltype(tab)...>(); });
}

// policy export behind a solve: one sweep per instance of [first, first + count) at the returned iterate (policy_kernel /
// policy_kernel_mw), as a work queue over the resident workgroups of THAT kernel (the one-wave kernel: at most 8 per CU); the work
// buffers dft / rec are the solve's, per slot.  has_policy<M>() builds only: make_ops leaves the entry null elsewhere.
// val: the value buffer (sddp_enable_value) and the nodes it keeps, filled for the range by the same sweep; null: the export is off.
// a.order set: a masked launch -- the queue hands out order[i] from the head its pre-pass left on the stream (queue_grid).
template <class M>
int launch_policy(sddp_handle* h, SolveArgs a, int first, int count, double* pol, int keep, double* val, int vnodes) {
    return with_table<M>(h, [&](auto... tab) {
        auto kern = pick_policy<M, decltype(tab)...>();
        int slots = 0;
        int rc = kernel_slots<M>(h, kern, use_mw<M>() ? 0 : 8, &slots);
        if (rc != SDDP_OK) return rc;
        a.first = first; a.count = count; a.qhead = nullptr;      // a.order: null, or the order of a masked launch (sddp_policy_masked_device)
        int grid = 0;
        rc = queue_grid(h, a, slots, count, &grid);
        if (rc != SDDP_OK) return rc;
        return launch(h, kern, grid, threads_of<M>(), lds_bytes<M>(), a, pol, keep, val, vnodes, tab...);
    });
}

// the knot evaluation of the parity tests: the one kernel that only reads and stays in the main unit (sddp_kernels.hpp says why)
template <class M>
void launch_eval_knots(const DevConsts& dc, int N, int nk, const int* dk, const double* dx, const double* du, const double* dp, double* drec,
                       double* df, double* dF, double* dH, double* dg, double* dL) {
    hipLaunchKernelGGL(eval_knots_kernel<M>, dim3(nk), dim3(kWave), 0, 0, dc, N, nk, dk, dx, du, dp, drec, df, dF, dH, dg, dL);
}

// The launchers of the kernels that only read (ModelOps::InspectOps) as the build's main unit names them without instantiating a
// kernel of theirs: declared here, defined (an explicit specialisation, SDDP_DEFINE_INSPECT_OPS of sddp_launch_inspect.hpp) by the
// build's inspect unit alone, or by a user build's one unit in front of its make_ops.  This is side_solve_ops' mechanism for every
// build: what those kernels are, and what is done to them later, cannot reach the code generation of the solve kernels of this
// unit.  A build whose inspect unit is missing does not load.
template <class M>
ModelOps::InspectOps side_inspect_ops();

template <class M>
ModelOps make_ops(const char* name) {
    ModelOps o;
    o.model = model_of_name(name);
    o.bar = M::BAR; o.so2 = M::SO2; o.xr = M::NXR > 0;
    o.table_kernels = has_hetero<M>();
    o.dims = {M::NX, M::NU, M::NP, M::NREC};
    o.col_cmd[0] = M::P_CMD0; o.col_cmd[1] = M::P_CMD1; o.col_sw[0] = M::P_SW_L; o.col_sw[1] = M::P_SW_R;
    o.uses_mw = use_mw<M>();
    o.w2_build = has_w2<M>();
    o.name = name;
    o.max_slots = max_slots<M>;
    o.solve[kSolvePlain] = solve_ops<M, kSolvePlain>();
    enter_side_units<M>(o, std::make_integer_sequence<int, kSolveVariants - 1>());
    o.launch_cost_keys = launch_cost_keys<M>;
    o.launch_backward = launch_backward<M>;
    o.launch_forward = launch_forward<M>;
    if constexpr (has_policy<M>()) o.launch_policy = launch_policy<M>;
    o.launch_eval_knots = launch_eval_knots<M>;
    o.inspect = side_inspect_ops<M>();
    return o;
}

}  // namespace sddp
