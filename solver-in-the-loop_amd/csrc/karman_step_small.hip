// The kernels of karman_step.hip that run the small-grid direct pressure solve (fd_solve_small: k_karman_fwd / k_karman_bwd<CPT, 3> and the
// fused 64 x 32 adjoint k_karman_bwd_bww_small), as a translation unit of their own: _build.py compiles this one WITHOUT the
// iterative-ILP scheduler strategy, which mis-schedules kernels that inline fd_solve_small (karman_step.hip, above karman_bwd_body).
#define SOL_K2D_SMALL_TU 1
#include "karman_step.hip"
