// sddp_inst.hip -- one model build of the library: compiled once per entry of srbd_horizon_amd/_lib.py INSTANCES with
//   -DSDDP_INST_MODEL=<device model type>  -DSDDP_INST_FN=<name of the accessor>  -DSDDP_INST_NAME="<model name>"
// (in parallel: the solve kernels of one model build are 10-30 s of device code generation each).  The accessor returns the
// build's table (sddp_handle.hpp ModelOps): which model it is a build of, its traits and its launchers.  sddp_api.hip receives
// the accessors' names from the same list and finds a handle's build among them by (model, traits).
// The plain builds (the entries without traits) are compiled once more per solve variant beyond kSolvePlain (sddp_handle.hpp
// SolveVariant), with -DSDDP_INST_VARIANT=<its value>: such a side unit holds nothing but that variant's instantiations of the
// solve kernels and their two table entries, which the main unit (no such definition, or 0) enters in its table (sddp_launch.hpp
// enter_side_units).  A side unit of a build with traits does not compile (with_solve_kernels).
#include "sddp_launch.hpp"

#if !defined(SDDP_INST_MODEL) || !defined(SDDP_INST_FN) || !defined(SDDP_INST_NAME)
#error "compile with -DSDDP_INST_MODEL=... -DSDDP_INST_FN=... -DSDDP_INST_NAME=..."
#endif
#ifndef SDDP_INST_VARIANT
#define SDDP_INST_VARIANT 0
#endif

namespace sddp {
#if SDDP_INST_VARIANT != 0
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
