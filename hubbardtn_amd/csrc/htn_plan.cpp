// Contraction compiler of the two-site DMRG path: sector tables + reduced MPO -> task lists for the grouped GEMM,
// SVD staging, the global truncation rule, post-SVD finalisation.  Host C++ (no HIP).
//
// This is the MI355X-first replacement for what TensorKit does with fusion trees and tree transformers around every
// contraction: instead of permuting tensors between matricisations at run time,
// every contraction is compiled ONCE per bond geometry into (output tile, segment) records; recoupling coefficients
// (closed-form 9j) become the segments' alpha.  tests/test_cplan_cpu.py holds the Python statement of the same
// planner (tests/ref_planner.py) and asserts byte-identical task lists.
//
// This file holds the error text; the planner sits in one file per concern and is compiled as part of THIS translation unit
// (included below), as htn_engine.cpp does with the engine: a build line names htn_plan.cpp and htn_engine.cpp, as it always
// did.  htn_recouple.cpp (fusion rules, 6j / 9j, coef_*), htn_layout.cpp (bonds; site, theta, env and overlap layouts),
// htn_tasks.h (TaskList: blocks + segments -> tile / segment records), htn_balance.cpp (the launch balancer),
// htn_plan_apply.cpp (H_eff on two, one and no site), htn_plan_env.cpp (gauge move, theta, H environments), htn_plan_svd.cpp
// (SVD staging, truncation, finalisation), htn_plan_ovl.cpp (overlap environments, projector).
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <mutex>

#include "htn_core.h"

namespace htn {

// ---- error string ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
char* err_buf() { return g_err; }
int set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return 1;
}

}  // namespace htn

#include "htn_recouple.cpp"
#include "htn_layout.cpp"
#include "htn_tasks.h"
#include "htn_balance.cpp"
#include "htn_plan_apply.cpp"
#include "htn_plan_env.cpp"
#include "htn_plan_svd.cpp"
#include "htn_plan_ovl.cpp"
