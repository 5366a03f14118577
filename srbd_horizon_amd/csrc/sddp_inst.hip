// sddp_inst.hip -- the translation units of one model build of the library: compiled per entry of srbd_horizon_amd/_lib.py INSTANCES
// with
//   -DSDDP_INST_MODEL=<device model type>  -DSDDP_INST_FN=<name of the accessor>  -DSDDP_INST_NAME="<model name>"
// (in parallel: the solve kernels of one model build are 10-30 s of device code generation each), once per unit of the build
// (_lib.translation_units).  Each unit is a device module of its own, and holds what the one thing it defines instantiates:
//   * the main unit (nothing further defined): the accessor.  It returns the build's table (sddp_handle.hpp ModelOps): which model it
//     is a build of, its traits and its launchers -- the solve, policy, backward / forward and cost-key kernels.  sddp_api.hip receives
//     the accessors' names from the same list and finds a handle's build among them by (model, traits);
//   * the inspect unit (-DSDDP_INST_INSPECT, every build): side_inspect_ops<model>, the launchers of the kernels that only read
//     (sddp_launch_inspect.hpp), which the main unit enters in its table whole.  No solve kernel shares a module with them;
//   * the plain builds (the entries without traits) once more per solve variant beyond kSolvePlain (sddp_handle.hpp SolveVariant), with
//     -DSDDP_INST_VARIANT=<its value>: nothing but that variant's instantiations of the solve kernels and their two table entries,
//     which the main unit enters in its table (sddp_launch.hpp enter_side_units).  A variant unit of a build with traits does not
//     compile (with_solve_kernels).
// A library that lacks a unit its main unit names does not load.
#include "sddp_launch.hpp"
#ifdef SDDP_INST_INSPECT
#include "sddp_launch_inspect.hpp"
#endif

#if !defined(SDDP_INST_MODEL) || !defined(SDDP_INST_FN) || !defined(SDDP_INST_NAME)
#error "compile with -DSDDP_INST_MODEL=... -DSDDP_INST_FN=... -DSDDP_INST_NAME=..."
#endif
#ifndef SDDP_INST_VARIANT
#define SDDP_INST_VARIANT 0
#endif
#if defined(SDDP_INST_INSPECT) && SDDP_INST_VARIANT != 0
#error "-DSDDP_INST_INSPECT and -DSDDP_INST_VARIANT name two different units"
#endif

namespace sddp {
#if defined(SDDP_INST_INSPECT)
SDDP_DEFINE_INSPECT_OPS(SDDP_INST_MODEL)
#elif SDDP_INST_VARIANT != 0
static_assert(SDDP_INST_VARIANT > 0 && SDDP_INST_VARIANT < kSolveVariants, "-DSDDP_INST_VARIANT: a value of SolveVariant");
template <>
ModelOps::SolveOps side_solve_ops<SDDP_INST_MODEL, SolveVariant(SDDP_INST_VARIANT)>() {
    return solve_ops<SDDP_INST_MODEL, SolveVariant(SDDP_INST_VARIANT)>();
}
#else
const ModelOps* SDDP_INST_FN() {
    static const ModelOps ops = make_ops<SDDP_INST_MODEL>(SDDP_INST_NAME);
    return &ops;
}
#endif
}  // namespace sddp
