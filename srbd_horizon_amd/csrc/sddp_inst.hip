// sddp_inst.hip -- one model build of the library: compiled once per entry of srbd_horizon_amd/_lib.py INSTANCES with
//   -DSDDP_INST_MODEL=<device model type>  -DSDDP_INST_FN=<name of the accessor>  -DSDDP_INST_NAME="<model name>"
// (in parallel: the solve kernels of one model build are 10-30 s of device code generation each).  The accessor returns the
// build's table (sddp_handle.hpp ModelOps): which model it is a build of, its traits and its launchers.  sddp_api.hip receives
// the accessors' names from the same list and finds a handle's build among them by (model, traits).
// The plain builds (the entries without traits) are compiled a second time with -DSDDP_INST_RESUME: that unit holds nothing but
// the RESUME instantiations of the solve kernels and their launcher, which the main unit (-DSDDP_INST_HAS_RESUME) enters in its
// table.  Either flag on a build with traits does not compile (sddp_launch.hpp launch_solve_resume) or does not link.
// The iteration log's kernels (the RESUME and LOG instantiations) are a third unit of the same builds in the same way:
// -DSDDP_INST_LOG compiles it, -DSDDP_INST_HAS_LOG tells the main unit.
#include "sddp_launch.hpp"

#if !defined(SDDP_INST_MODEL) || !defined(SDDP_INST_FN) || !defined(SDDP_INST_NAME)
#error "compile with -DSDDP_INST_MODEL=... -DSDDP_INST_FN=... -DSDDP_INST_NAME=..."
#endif
#define SDDP_CAT2(a, b) a##b
#define SDDP_CAT(a, b) SDDP_CAT2(a, b)
#define SDDP_INST_RESUME_FN SDDP_CAT(SDDP_INST_FN, _resume_solve)
#define SDDP_INST_LOG_FN SDDP_CAT(SDDP_INST_FN, _log_solve)

namespace sddp {
#if defined(SDDP_INST_RESUME)
int SDDP_INST_RESUME_FN(sddp_handle* h, SolveArgs a, int first, int count) { return launch_solve_resume<SDDP_INST_MODEL>(h, a, first, count); }
#elif defined(SDDP_INST_LOG)
int SDDP_INST_LOG_FN(sddp_handle* h, SolveArgs a, int first, int count) { return launch_solve_log<SDDP_INST_MODEL>(h, a, first, count); }
#else
#ifdef SDDP_INST_HAS_RESUME
int SDDP_INST_RESUME_FN(sddp_handle* h, SolveArgs a, int first, int count);
#endif
#ifdef SDDP_INST_HAS_LOG
int SDDP_INST_LOG_FN(sddp_handle* h, SolveArgs a, int first, int count);
#endif
const ModelOps* SDDP_INST_FN() {
    static const ModelOps ops = [] {
        ModelOps o = make_ops<SDDP_INST_MODEL>(SDDP_INST_NAME);
#ifdef SDDP_INST_HAS_RESUME
        o.launch_solve_resume = SDDP_INST_RESUME_FN;
#endif
#ifdef SDDP_INST_HAS_LOG
        o.launch_solve_log = SDDP_INST_LOG_FN;
#endif
        return o;
    }();
    return &ops;
}
#endif
}  // namespace sddp
