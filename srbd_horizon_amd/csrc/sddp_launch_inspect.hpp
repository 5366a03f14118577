// sddp_launch_inspect.hpp -- host-side launchers of the kernels that only read (sddp_inspect.hpp), collected into
// ModelOps::InspectOps.  Included by the inspect unit of a model build alone (sddp_inst.hip with -DSDDP_INST_INSPECT) and by a user
// build's one unit (srbd_horizon_amd/userterms.py): whoever includes it defines side_inspect_ops<M> with SDDP_DEFINE_INSPECT_OPS,
// which is what make_ops<M> of the main unit enters in its table (sddp_launch.hpp).
#pragma once
#include "sddp_inspect.hpp"
#include "sddp_launch.hpp"

namespace sddp {

// the exported policy rolled out through the model from a measured state: one wavefront per instance of the range, static LDS only.
// has_policy<M>() builds only, like launch_policy.
template <class M>
int launch_policy_rollout(sddp_handle* h, int first, int count, int start, int steps, const double* dxm, double* dx, double* du, double* dcost) {
    return launch_waves<M>(h, SDDP_PICK(policy_rollout_kernel), count, 0, h->N, first, count, start, steps, h->xs, h->us, h->last_params,
                           (const double*)h->pol.policy, h->policy_words(), dxm, dx, du, dcost);
}

// the plan uncertainty under the exported policy: one wavefront per instance of the range, static LDS only (at most 64 KB: asserted in
// the kernel).  dq / dr / dcov / ducov may be null.  has_policy<M>() builds that the mapping fits
// (policy_covariance_fits<M>(): nx <= 64 and 64 KB of LDS), else the entry stays null.
template <class M>
int launch_policy_covariance(sddp_handle* h, int first, int count, int start, int steps, const double* dsigma0, const double* dq, const double* dr,
                             double ml, double* dout, double* dcov, double* ducov) {
    return launch_waves<M>(h, SDDP_PICK(policy_covariance_kernel), count, 0, h->N, first, count, start, steps, h->xs, h->us, h->last_params,
                           (const double*)h->pol.policy, h->policy_words(), dsigma0, dq, dr, ml, dout, dcov, ducov);
}

// the value records of the range evaluated at measured states (sddp_value_at_device): one wavefront per instance, static LDS only.
// has_policy<M>() builds only, like launch_policy.
template <class M>
int launch_value_at(sddp_handle* h, int first, int count, int node, const double* dxm, double* dout) {
    return launch_waves<M>(h, SDDP_PICK(value_at_kernel), count, 0, h->N, first, count, node, (const double*)h->xs, (const double*)h->val.value,
                           h->val.nodes, (const double*)h->pol.policy, h->policy_words(), dxm, dout);
}

// The plan inspectors (sddp_handle.hpp PlanSource): one wavefront per instance of the range.  Every build has them.
// the plan audit: nothing but registers
template <class M>
int launch_audit(sddp_handle* h, int first, int count, int start, int steps, PlanSource s, double ml, double* dout) {
    return launch_waves<M>(h, SDDP_PICK(plan_audit_kernel), count, 0, h->N, first, count, start, steps, s.x, s.u, s.xoff, h->last_params, ml, dout);
}
// the stationarity certificate: static LDS only
template <class M>
int launch_stationarity(sddp_handle* h, int first, int count, PlanSource s, double* dout, double* dlam, double* dgrad) {
    return launch_waves<M>(h, SDDP_PICK(stationarity_kernel), count, 0, h->N, first, count, s.x, s.u, s.xoff, h->last_params, dout, dlam, dgrad);
}
// the cost breakdown: dynamic LDS sized from N (cost_terms_lds: the tile of addends and, where a parameter is a weight, two copies of
// the instance's parameter rows).  A horizon whose LDS exceeds the 64 KB a kernel has without an attribute is refused, there is no
// chunked path.  xr_zero: the user rows' table with zero weights (null: the build has no such table).
template <class M>
int launch_cost_terms(sddp_handle* h, int first, int count, PlanSource s, const double* xr_zero, double* dout, double* dnodes) {
    const size_t lds = cost_terms_lds<M>(h->N);
    if (lds > size_t(64) * 1024)
        return fail(h, SDDP_ERR_ARG, "sddp_cost_terms_range_device: the horizon's tile of addends needs " + std::to_string(lds) +
                                         " bytes of LDS, more than the 65536 one workgroup has here");
    return launch_waves<M>(h, SDDP_PICK(cost_terms_kernel), count, lds, xr_zero, h->N, first, count, s.x, s.u, s.xoff, h->last_params, dout, dnodes);
}
// the parameter sensitivities: nothing but registers.  dlam / dstat: what launch_stationarity stored for the same range just before
// (sddp_api.hip).  Not on a user build, whose rows have no d/dp code (SrbdModel::param_grad)
template <class M>
int launch_param_gradient(sddp_handle* h, int first, int count, PlanSource s, const double* dlam, const double* dstat, double* dout, double* dgrad) {
    return launch_waves<M>(h, SDDP_PICK(param_gradient_kernel), count, 0, h->N, first, count, s.x, s.u, s.xoff, h->last_params, dlam, dstat, dout,
                           dgrad);
}
// the constant sensitivities: dynamic LDS sized from N (const_gradient_lds: the tile of addends); sddp_api.hip, the one caller, has
// refused a horizon whose tile exceeds 64 KB before the stationarity launch.  dlam / dstat: see launch_param_gradient.  Not on a user
// build (SrbdModel::const_grad)
template <class M>
int launch_const_gradient(sddp_handle* h, int first, int count, PlanSource s, const double* dlam, const double* dstat, double* dout, double* dnodes) {
    return launch_waves<M>(h, SDDP_PICK(const_gradient_kernel), count, const_gradient_lds(h->N), h->N, first, count, s.x, s.u, s.xoff,
                           h->last_params, dlam, dstat, dout, dnodes);
}

template <class M>
int launch_model_step(sddp_handle* h, int k, const double* dx, const double* du, const double* dp, double* dxn) {
    return launch_waves<M>(h, SDDP_PICK(model_step_kernel), (h->B + kWave - 1) / kWave, 0, h->B, k, dx, du, dp, dxn);
}

template <class M>
ModelOps::InspectOps inspect_ops() {
    ModelOps::InspectOps o;
    if constexpr (has_policy<M>()) o.policy_rollout = launch_policy_rollout<M>;
    if constexpr (has_policy<M>()) o.value_at = launch_value_at<M>;
    if constexpr (has_policy<M>() && policy_covariance_fits<M>()) o.policy_covariance = launch_policy_covariance<M>;
    o.audit = launch_audit<M>;
    o.stationarity = launch_stationarity<M>;
    o.cost_terms = launch_cost_terms<M>;
    if constexpr (!M::HAS_UR) o.param_gradient = launch_param_gradient<M>;
    if constexpr (!M::HAS_UR) o.const_gradient = launch_const_gradient<M>;
    o.model_step = launch_model_step<M>;
    return o;
}

// THE definition of side_inspect_ops<M> (sddp_launch.hpp), inside namespace sddp: what the inspect unit of a library build and the
// one unit of a user build both say, so the two cannot drift.
#define SDDP_DEFINE_INSPECT_OPS(M) \
    template <>                    \
    ModelOps::InspectOps side_inspect_ops<M>() { return inspect_ops<M>(); }

}  // namespace sddp
