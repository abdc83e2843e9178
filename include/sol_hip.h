/*
 * sol_hip.h  --  C ABI of libsol_hip.so, the MI355X (gfx950) engine for the
 * solver-in-the-loop hot path.
 *
 * The reference exposes no FFI of its own for this path: the seam is
 * the Python call surface of karman_train.py / burgers_train.py, and the nearest plug
 * point is PhiFlow's PressureSolver / CUDASolver custom op imported at
 * /root/reference/karman-2d/karman_train.py:51.  Each entry point below cites the
 * reference lines whose arithmetic it replaces.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; sol_last_error() gives the text
 *     (thread local).  Nothing is allocated inside: all buffers, including workspaces,
 *     are caller-owned DEVICE pointers (fp32 unless noted).
 *   - workspaces are SCRATCH: their contents on entry are ignored (any bit pattern, NaN and stale results of an earlier call
 *     included; whatever an entry point needs cleared it clears in its own launches) and their contents on exit are unspecified.
 *     Every element of every output is written, so outputs may be uninitialised memory too.  The exceptions are named where
 *     they occur: buffers documented as accumulated onto (`accumulate` flags, g_re / g_vy / g_vx "to add onto"), the warm-start
 *     guess of sol_karman_step_fwd_large_cg_warm (read, then overwritten with the step's pressure), absmax slots and
 *     weight-gradient partials the caller zeroes -- none of these is part of a workspace -- and ONE region that is: under the
 *     opt-in cnn_persistent the hand-off flags of the persistent CNN launches live inside the workspace of sol_train_fwd_bwd /
 *     sol_rollout, and the library zeroes them once, when a control word in that workspace does not hold the configuration's
 *     magic value -- stale contents that happen to hold it are the one case where the contents on entry matter, so with that
 *     option on zero the workspace before its first use (k3d_conv_persist likewise: its flag region is zero before first use).
 *     tests/test_gpu_poison.py holds the solver steps, adjoints, pressure solves, trainers and roll-outs to this, under the
 *     default options, with four fill patterns.
 *   - `stream` is a hipStream_t passed as void*; calls are asynchronous on that stream.  The only
 *     process-wide mutable state is the option table behind sol_set_option() (kernel-variant
 *     selection, read at every call) and the launch profiler (sol_prof_begin/end); the library never
 *     reads the environment.  Calls on distinct streams are thread-safe as long as no thread changes
 *     an option or profiles concurrently.
 *   - layouts: density d [B,Y,X]; v_y [B,Y+1,X]; v_x [B,Y,X+1]  (component 0 = y, the
 *     reference's `velocity.data[0]`, karman_train.py:367); images NHWC; conv kernels
 *     HWIO (Keras layout); `params`/`grads` = Keras get_weights() order, flattened.
 */
#ifndef SOL_HIP_H
#define SOL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SOL_OK 0
#define SOL_ERR_ARG (-1)      /* invalid argument / unsupported shape */
#define SOL_ERR_HIP (-2)      /* HIP runtime error (text in sol_last_error) */
#define SOL_ERR_WORKSPACE (-3)
#define SOL_ERR_GRAPH (-4)    /* a captured graph holds a node type that is refused (sol_graph_check) */

#define SOL_MARS_MOON_PARAMS 260354   /* model_mars_moon, karman_train.py:101-138 */

const char* sol_last_error(void);
int sol_version(void);
/* sizeof() of the ABI structs below, for bindings that mirror them (ctypes): a stale library is detected at load time */
int sol_abi_sizes(int32_t* karman_cfg, int32_t* burgers_cfg, int32_t* train_cfg);

/* Kernel-variant options (process wide; defaults in parentheses).  The reference's knob of this kind is the
 * `pressure_solver=` argument of KarmanFlow (karman_train.py:167) and the `--cuda` switch (:51); everything else is
 * new.  Unknown names / out-of-range values return SOL_ERR_ARG.
 *   conv_precision (0)  0: fp32-equivalent split arithmetic on the 16-bit matrix pipe (fp16 x3 where the operand's absmax
 *                          is known, bf16 x6 otherwise); 1: bf16 x6 always; 2: strict fp32 MFMA (v_mfma_f32_*_f32) everywhere
 *   cnn_persistent (0)  the ten 32->32 CNN layers of a pass as ONE persistent launch (tagged-granule halo exchange between
 *                       neighbouring workgroups) where the shape allows it (W == 64, ceil(B*H/3) <= #CUs); measured on par
 *                       with the per-layer launches at B = 6
 *   bww_fuse (1), correct_fuse (1), density_mode (0), conv_thin (1), conv_r3 (1), conv_bww32 (1): fusion / kernel choices
 *   k3d_conv_fused (1)  32 -> 32 and 32 -> (<= 16) Conv3D layers (W == 64, operand absmax given) as ONE launch that keeps its accumulators over all
 *                       125 taps (0: five passes of the 2-D kernel with the running sum in HBM); k3d_fused_tf (1): sine transforms
 *                       of the 3-D pressure solve as LDS-resident plane / slab kernels (0: batched GEMMs)
 *   k3d_conv_rows (8)   rows per workgroup of the one-launch Conv3D kernel: 8 = one 64 px x 32 co tile per wave, eight waves (two per
 *                       SIMD), operands prefetched one tap ahead; 6 = 32 x 32 tiles, twelve waves; 3 = 16 x 32 tiles, twelve waves
 *   k3d_tile (0)        1: karman-3d advection from LDS tiles that hold the full z column + halo; 0: wave-per-column gathers
 *                       straight from the L2-resident fields (measured 3x faster at batch 1-2: the tile form is instruction bound)
 *   conv_dx (11)        bit set: 1 the 32 -> 32 fp16 x3 convolutions on the dx-major kernel, 2 thin layers in one-row launches, 4 thin layers
 *                       everywhere, 8 half-channel workgroups in one-row launches
 *   conv_thin_valu (1)  the thin 32 -> (<= 4) layers of 64-pixel images without residual / activation (the trainer's output layer with the
 *                       correction + loss epilogue, the first layer's data gradient) in exact fp32 on the vector ALU; 2: its eight-wave
 *                       form; 0: the split-precision MFMA kernels
 *   seed_fuse (1)       trainer, 64-pixel rows: the loss-gradient seed of an unrolled step (d loss / d v_i + the adjoint of step i+1, scaled
 *                       to the network's output gradient) is computed by the 2 -> 32 backward-data launch in its staging phase; 0: a k_seed
 *                       launch per unrolled step in front of it
 *   fwd_bands (1)       trainer / roll-out, 128 x 64, direct solver, B <= 40: the forward solver step of a simulation as FIVE workgroups in one
 *                       launch (four row bands run the stencil phases with recomputed 8-row halos, a fifth runs the direct solve; hand-offs
 *                       of divergence and pressure through a workspace region); 0: one workgroup per simulation.  Same results bit for bit
 *                       (departure points beyond the halo: recomputed from the step's input, 1e-6)
 *   conv_thin_t3 (1)    thin-input layers (3 -> 32 first layer, 2 -> 32 last backward-data layer incl. the seed form) of 64-pixel rows as three rows
 *                       of the batch x height stack per twelve-wave workgroup; 0: one row per 256-thread workgroup.  Same results bit for bit
 *   k3d_adj_tile (1)    karman-3d: the advection adjoint's fixed-point scatter goes through an int64 LDS window per workgroup (4 x 4 columns + halo 2),
 *                       flushed with one global atomic per non-zero cell; 0: every contribution is a global atomic.  Same results bit for bit
 *   k2d_adj_tile (1)    karman-2d large grids: the advection adjoint's fixed-point scatter goes through an int64 LDS window per workgroup (16 x 16 cells
 *                       + halo 4), flushed with one global atomic per non-zero cell; 0: every contribution is a global atomic.  Same results bit for bit
 *   k2d_dens_adj_tile (1) karman-2d, any grid: the density adjoint's fixed-point scatter (sol_karman_density_bwd) goes through an int64 LDS window per
 *                       workgroup (16 x 16 cells + halo 4), flushed with one global atomic per non-zero cell; 0: every contribution is a global atomic.
 *                       Same results bit for bit
 *   k2d_mc_tile (1)     karman-2d large grids: the MacCormack advection ("MACCORMACK ADVECTION" below) as one launch on 16 x 32 tiles with the
 *                       semi-Lagrangian values of a halo of 2 in LDS (a corner beyond the halo is evaluated on the fly); 0: two launches through
 *                       the workspace.  Same results bit for bit
 *   k2d_solve_one_wg (1) karman-2d, scenes built with multi_launch on a grid of at most 8192 cells with X <= 64: the one-window direct pressure solve as
 *                       ONE launch, one workgroup per simulation (sol_karman_solve_one_wg_supported); 0: the chain of GEMM launches.  The same fp32
 *                       sums in another order; measured faster at 64 x 32 and at 128 x 64 (profiles/k2d_multi_launch_small_time.json)
 *   k3d_dens_adj_tile (1) karman-3d: the density adjoint's fixed-point scatter (sol_karman3d_density_bwd) goes through an int64 LDS window per
 *                       workgroup (4 x 4 columns + halo 2, all k), flushed with one global atomic per non-zero cell; 0, or a window beyond
 *                       64 KB (Z > 128): every contribution is a global atomic.  Same results bit for bit
 *   k3d_conv_persist (0) karman-3d: 1 = the one-launch Conv3D kernel as 256 workgroups of consecutive eight-row tiles (the next tile's rows and weight
 *                       sets requested during the last tap rows of the tile) when the tile count is a multiple of 256; same results bit for bit,
 *                       measured slower (register spills), kept as a tested experiment
 *   k3d_bww_jobs (2)    karman-3d: the five depth slices of a 32 -> 32 Conv3D weight gradient (sol_conv3d_bwd_weight*) as ONE launch of ONE round of
 *                       workgroups (51 per slice; other block partition: sums equal to round-off); 1: one launch of five rounds of 32-row
 *                       workgroups (bit-identical to 0); 0: five launches
 *   cpt (0), conv_split3 (0), dbg_skip (0), step_prof (0): experiments, debugging */
int sol_set_option(const char* name, int32_t value);
int sol_get_option(const char* name, int32_t* value);

/* Launch profiler: between sol_prof_begin() and sol_prof_end() every kernel the library launches (eagerly, not under
 * stream capture) carries its own pair of HIP events on the stream it is launched on (hipExtLaunchKernelGGL start/stop:
 * the dispatch's begin/end timestamps, the quantity rocprofv3 --kernel-trace reports).  sol_prof_end synchronises the
 * device and returns the number n of distinct kernels; names (n x 64 chars), total_us[n], calls[n] are HOST arrays. */
int sol_prof_begin(void);
int sol_prof_end(int32_t max_classes, char* names, double* total_us, int32_t* calls);

/* ------------------------------------------------------------------------------------
 * Solver step:  KarmanFlow.step  (karman-2d/karman_train.py:173-185) =
 *   explicit diffusion + velocity BC (lines 175-183) followed by PhiFlow's
 *   IncompressibleFlow.step: semi-Lagrangian advection of density and velocity, inflow,
 *   divergence_free() with the obstacle (hard-BC face masks, divergence, CG pressure
 *   solve, gradient subtraction).  One workgroup per simulation; everything between the
 *   input load and the output store stays in LDS / registers.
 * ---------------------------------------------------------------------------------- */
typedef struct sol_karman_cfg {
    int32_t B, Y, X;        /* batch, cells in y, cells in x (Y%8==0, X in {8,16,32,64}) */
    float dx;               /* cell size = len / X  (karman_train.py:363)              */
    float dt;               /* time step (step(..., dt=1.0))                            */
    float res;              /* `res` argument of step(): alpha = dt*res*res/Re (l.175)  */
    float cg_rtol;          /* CG stops when |r|_2 <= max(cg_rtol*|b|_2, cg_atol)       */
    float cg_atol;
    int32_t cg_max_iter;    /* PhiFlow SparseCG: 2000                                   */
    int32_t grad_pad;       /* 0: replicate (PhiFlow 1.x), 1: dirichlet0                */
    int32_t inflow_before;  /* 0: density += inflow*dt after advection (phi 1.x),
                               1: before advection (karman-2d-phi2/karman_train.py:182) */
    int32_t coarse_n;       /* 0, or (Y/8)*(X/8): size of the coarse space of the CG preconditioner */
    const float* coarse_inv;/* NULL (plain CG), or DEVICE [coarse_n,coarse_n]: inverse of P^T(-A)P for
                               8x8-cell aggregates P of the scene's `active` mask, prepared by the host
                               (see sol_karman_precond_supported).  Only the iteration count changes:
                               the solve still converges to the same tolerance.                      */
    int32_t direct_n;       /* 0, or the number of 32-bit words of `direct`                                   */
    const float* direct;    /* NULL, or DEVICE blob of the DIRECT pressure solver (PhiFlow's PressureSolver plug
                               point, KarmanFlow(pressure_solver=...) karman_train.py:167): fast diagonalisation
                               of the rectangle Laplacian by sine transforms + a dense capacitance correction for
                               the obstacle cells, prepared by the host for the scene's `active` mask (layout:
                               precond.direct_solver_blob).  Takes precedence over the CG; no iteration, the
                               solution equals the converged CG solution up to fp32 round-off.  Built for
                               128 x 64 and for small grids (sol_karman_direct_supported).                     */
} sol_karman_cfg;

/* 1 if the two-level CG preconditioner can be used for a Y x X grid, else 0 */
int sol_karman_precond_supported(int32_t Y, int32_t X);
/* 1 if the direct pressure solver is built for a Y x X grid (128 x 64, and grids of at most 2048 cells with
 * Y % 16 == 0, X in {16, 32, 64}, e.g. the reference's 64 x 32 training recipe), else 0 */
int sol_karman_direct_supported(int32_t Y, int32_t X);
/* 1 if the one-launch form of the multi-launch path's direct pressure solve (one workgroup per simulation, option k2d_solve_one_wg) serves
 * a Y x X grid with a one-window blob of window `win`: Y, X >= 16, at most 8192 cells, X <= 64, win in {16, 32, 64} within the grid.  It
 * runs inside every entry point that takes `direct_header_host` when word 8 of that HOST header copy has bit 0 set (the scene was built
 * with multi_launch: ops.SceneMasks) and the option is 1; otherwise the entry points issue the launches they always did. */
int sol_karman_solve_one_wg_supported(int32_t Y, int32_t X, int32_t win);

/* Forward step for grids beyond the one-workgroup kernels (the reference generates its data at 256 x 128:
 * karman-2d/karman.py:98-159, Makefile:19-28 `-r 128`).  Same arithmetic and argument meaning as sol_karman_step_fwd,
 * decomposed into chip-wide launches on global memory; the pressure system is solved DIRECTLY, so cfg.direct (blob
 * with a 16/32/64 window, precond.direct_solver_blob(active, max_window=64)) is required.  This form keeps no state
 * (the differentiable pair is sol_karman_step_fwd_large_saved / sol_karman_step_bwd_large below).  Outputs must not alias inputs.  `direct_header_host`: HOST copy of the first 16 words of the blob
 * (grid, window origin/size, number of perturbed cells: they size the launches).  `workspace`: DEVICE scratch of
 * sol_karman_step_large_workspace_bytes(cfg) bytes. */
size_t sol_karman_step_large_workspace_bytes(const sol_karman_cfg* cfg);
/* The same, sized from the HOST header of the blob in cfg.direct.  The direct entry points of the large-grid step read the header's
 * magic word: "FD02" = the one-window blob above, "FDS1" = the SCATTERED blob (precond.scattered_solver_blob: the support set S of the
 * obstacle -- solid cells and their neighbours, at most 4096 -- as a row list R, a column list C and a slot index per cell; any scene,
 * however spread out).  The scattered solve runs box forward, U = T2 Qx[:,C], X0 = Qy[R,:] U, the capacitance product on the rows of K'
 * split over workgroups (fixed summation order, no atomics), V = Qy[:,R] W2, T1 = V Qx[C,:], scale-add, box back; its scratch follows
 * |R| and |C|, so size the workspace with this function (for an FD02 header or NULL it returns sol_karman_step_large_workspace_bytes). */
size_t sol_karman_step_large_workspace_bytes_for(const sol_karman_cfg* cfg, const int32_t* direct_header_host);
int sol_karman_step_fwd_large(const sol_karman_cfg* cfg, void* stream,
                              const float* d_in, const float* vy_in, const float* vx_in,
                              const float* re, const float* active, const float* inflow,
                              const float* velBCy, const float* velBCyMask, int64_t bc_batch_stride,
                              float* d_out, float* vy_out, float* vx_out,
                              float* feat_out, const float* feat_scale,
                              const int32_t* direct_header_host,
                              void* workspace, size_t workspace_bytes);
/* The same step with a preconditioned CG pressure solve, for ANY obstacle mask (scenes whose direct blob is refused: perturbed cells
 * beyond one 64 x 64 window, an ill-conditioned capacitance system).  Arguments as sol_karman_step_fwd_large, except: cfg.direct is
 * not read; `box_blob` = DEVICE blob of the empty-box solve (precond.box_solver_blob(Y, X): header with nS = 0, Qy, Qx, 1/lam), the
 * preconditioner; `box_header_host` = HOST copy of its first 16 words; `cg_info` = DEVICE int32 [2][B] written by the call: row 0 the
 * iterations used, row 1 converged (0/1) -- a simulation that does not converge within cfg.cg_max_iter is reported there, its pressure
 * is the last iterate.  A simulation stops when |r|_2 <= max(cfg.cg_rtol |b|_2, cfg.cg_atol) (cg_max_iter >= 1, tolerances >= 0, not
 * both zero); the dot products are fixed-order fp64 sums, so results are bit-reproducible.  Under stream capture the call issues
 * the full cg_max_iter budget and never synchronises; an eager call reads one 4-byte device word back every 16 iterations and stops
 * issuing iterations once every simulation has converged.  `workspace`: DEVICE scratch of
 * sol_karman_step_large_cg_workspace_bytes(cfg) bytes. */
size_t sol_karman_step_large_cg_workspace_bytes(const sol_karman_cfg* cfg);
int sol_karman_step_fwd_large_cg(const sol_karman_cfg* cfg, void* stream,
                                 const float* d_in, const float* vy_in, const float* vx_in,
                                 const float* re, const float* active, const float* inflow,
                                 const float* velBCy, const float* velBCyMask, int64_t bc_batch_stride,
                                 float* d_out, float* vy_out, float* vx_out,
                                 float* feat_out, const float* feat_scale,
                                 const float* box_blob, const int32_t* box_header_host, int32_t* cg_info,
                                 void* workspace, size_t workspace_bytes);
/* sol_karman_step_fwd_large_cg with a WARM-STARTED solve: `p_inout` [B,Y,X] DEVICE is read as the initial guess x0 and overwritten with
 * the step's pressure -- a roll-out hands the same buffer to consecutive steps (same matrix, a right-hand side that has barely moved).
 * The solve starts from x = x0, r = b - M x0 and runs as the cold one: same test |r|_2 <= max(cfg.cg_rtol |b|_2, cfg.cg_atol) against
 * |b| (a guess that already meets it reports 0 iterations, converged), same fixed-order fp64 sums, bit-reproducible; an all-zero guess
 * gives the cold call's bits.  A simulation whose guess holds a NaN or an Inf starts from x0 = 0.  Same workspace as the cold call
 * (sol_karman_step_large_cg_workspace_bytes); p_inout must not lie inside it. */
int sol_karman_step_fwd_large_cg_warm(const sol_karman_cfg* cfg, void* stream,
                                      const float* d_in, const float* vy_in, const float* vx_in,
                                      const float* re, const float* active, const float* inflow,
                                      const float* velBCy, const float* velBCyMask, int64_t bc_batch_stride,
                                      float* d_out, float* vy_out, float* vx_out,
                                      float* feat_out, const float* feat_scale,
                                      const float* box_blob, const int32_t* box_header_host, int32_t* cg_info,
                                      float* p_inout, void* workspace, size_t workspace_bytes);
/* The corrector's output applied to a staggered velocity (to_staggered + add, karman_train.py:88-90, 424-426), one launch for both
 * components, any Y, X >= 1:  vy[b,j,i] += s0 * out[b,j,i,0] (j < Y),  vx[b,j,i] += s1 * out[b,j,i,1] (i < X), each fl(v + fl(s * o));
 * the last row of vy [B,Y+1,X] and the last column of vx [B,Y,X+1] are not touched.  out [B,Y,X,2] (8-byte aligned).  cor_y [B,Y+1,X] /
 * cor_x [B,Y,X+1] (both NULL, or both given): receive the applied correction, zero on that row and column (the corTf frame of
 * karman_apply.py:138-158). */
int sol_karman_correct(void* stream, const float* out, float* vy, float* vx, float* cor_y, float* cor_x,
                       int32_t B, int32_t Y, int32_t X, float s0, float s1);
/* The CG step's pressure solve alone: M p = rhs with M = -A for the scene's `active` mask [Y,X] (precond.scene_matrix); rhs, p
 * [B,Y,X] (rhs is read only); other arguments as sol_karman_step_fwd_large_cg. */
int sol_karman_pressure_solve_large(const sol_karman_cfg* cfg, void* stream, const float* active, const float* rhs, float* p,
                                    const float* box_blob, const int32_t* box_header_host, int32_t* cg_info,
                                    void* workspace, size_t workspace_bytes);
/* The direct step's pressure solve alone, for either blob of cfg.direct (one window or scattered): M p = rhs; rhs, p [B,Y,X] (rhs is read
 * only).  `workspace`: sol_karman_step_large_workspace_bytes_for(cfg, direct_header_host) bytes serve.  No iteration, capturable. */
int sol_karman_pressure_solve_large_direct(const sol_karman_cfg* cfg, void* stream, const float* rhs, float* p,
                                           const int32_t* direct_header_host, void* workspace, size_t workspace_bytes);

/* PERIODIC BOUNDARIES of the large-grid step (csrc/karman_periodic.hip).  A direct blob built with precond's periodic=(py, px) carries
 * the axes in its header's flags word -- word 8 of an "FD02" blob (one window, or the box blob with nS = 0 that serves an EMPTY periodic
 * scene: box forward, box back), word 9 of an "FDS1" blob (its word 8 is CP): bit 1 (value 2) = y periodic, bit 2 (value 4) = x
 * periodic; bit 0 of word 8 stays the host-only one-launch flag.  Every entry point that takes `direct_header_host` reads the bits from
 * that host copy: clear, it issues the launches it always did; set, its stencil phases run with wrapped indices and its solve runs the
 * same launches on the blob's Hartley tables (precond.hartley_matrix: symmetric, orthogonal, diagonalises the periodic second difference).
 *   - Array shapes do not change.  On a periodic axis the last face plane DUPLICATES the first: vy[:, Y, :] = vy[:, 0, :] (y),
 *     vx[:, :, X] = vx[:, :, 0] (x).  The step never reads the duplicate plane of an input (a NaN there changes nothing) and writes
 *     the duplicate plane of vy_out / vx_out / saved_vy / saved_vx equal to plane 0 bit for bit.
 *   - Every index the open step clamps or sends to the density's zero ghost ring -- the replicate-padded Laplacian, the face averages
 *     of the advecting velocity, the bilinear gathers of v_y, v_x and the density, the face masks, the divergence, the pressure
 *     gradient -- is taken modulo n over the unique planes 0 .. n-1 (a true modulo: a departure point several periods away lands
 *     correctly).  The pressure gradient ignores cfg.grad_pad on a periodic axis: there is no boundary face.  The open axis of a
 *     mixed scene behaves as in the open step (velBC blend, clamp, grad_pad).  velBCy / velBCyMask are read on unique faces only.
 *   - Adjoint (sol_karman_step_bwd_large): the cotangent of an output duplicate plane is first added onto plane 0's (one fp32 add);
 *     the duplicate planes of g_vy_in / g_vx_in are exactly zero; the advection scatter stays in 64-bit fixed point with global
 *     atomics (order independent, bit-reproducible, capturable; the option k2d_adj_tile does not apply).
 *   - Doubly periodic: the scene must be empty, the matrix is singular, and the solve returns the zero-mean pressure (1/lam = 0 at
 *     the zero mode; the right-hand side -div has zero mean by construction).
 *   - Refused (SOL_ERR_ARG) on a periodic scene: the CG solve, advection = 1 (MacCormack), a non-zero buoyancy force, the _re forms.
 * sol_karman_seam_sync: plane 0 copied onto the duplicate plane of vy [B,Y+1,X] / vx [B,Y,X+1] for the axes in periodic_bits (2 = y,
 * 4 = x, 6 = both; 0: nothing is launched) -- what follows a launch that leaves the duplicate plane stale (sol_karman_correct).
 * sol_karman_seam_fold: its adjoint on a cotangent, g[plane 0] += g[duplicate] (one fp32 add), then g[duplicate] = 0.  Any Y, X >= 1. */
int sol_karman_seam_sync(void* stream, float* vy, float* vx, int32_t B, int32_t Y, int32_t X, int32_t periodic_bits);
int sol_karman_seam_fold(void* stream, float* g_vy, float* g_vx, int32_t B, int32_t Y, int32_t X, int32_t periodic_bits);

/* Adjoint of the large-grid step with respect to its input velocity, for both solvers (csrc/karman_large_bwd.hip).  The solver is
 * chosen by the cfg: cfg.direct set = the direct solve (direct_header_host required; box_blob / box_header_host / cg_info are not read
 * and may be NULL), cfg.direct NULL = the preconditioned CG (box_blob, box_header_host, cg_info [2][B] required as for
 * sol_karman_step_fwd_large_cg; direct_header_host is not read).
 *   sol_karman_step_fwd_large_saved: the forward step (same launches and results as sol_karman_step_fwd_large / _large_cg without
 *     features) that also hands out the post-diffusion velocity saved_vy [B,Y+1,X] / saved_vx [B,Y,X+1], the only state the adjoint
 *     needs.  `workspace`: the forward workspace of the solver (sol_karman_step_large_workspace_bytes / _large_cg_workspace_bytes).
 *   sol_karman_step_bwd_large: g_vy_in / g_vx_in = (d step / d v_in)^T (g_vy_out, g_vx_out); the density carries no gradient.  Stages:
 *     rhs of the adjoint projection, the forward step's pressure solve (same symmetric matrix), g_a, the advection adjoint as a scatter
 *     in 64-bit fixed point (order independent: results are bit-reproducible; LDS window per 16 x 16 tile, option k2d_adj_tile), the
 *     diffusion adjoint.  A non-finite output gradient makes that simulation's input gradient NaN.  With the CG solve, cg_info reports
 *     the adjoint solve's iterations / converged; under stream capture the call issues the full cfg.cg_max_iter budget and never
 *     synchronises, an eager call stops issuing iterations (checked every 16) once every simulation has converged.
 *     `workspace`: DEVICE scratch of sol_karman_step_bwd_large_workspace_bytes(cfg) bytes (covers either solver as the cfg selects it). */
size_t sol_karman_step_bwd_large_workspace_bytes(const sol_karman_cfg* cfg);
/* the same, sized from the host header of cfg.direct (required for a scattered blob, see sol_karman_step_large_workspace_bytes_for) */
size_t sol_karman_step_bwd_large_workspace_bytes_for(const sol_karman_cfg* cfg, const int32_t* direct_header_host);
int sol_karman_step_fwd_large_saved(const sol_karman_cfg* cfg, void* stream,
                                    const float* d_in, const float* vy_in, const float* vx_in,
                                    const float* re, const float* active, const float* inflow,
                                    const float* velBCy, const float* velBCyMask, int64_t bc_batch_stride,
                                    float* d_out, float* vy_out, float* vx_out, float* saved_vy, float* saved_vx,
                                    const int32_t* direct_header_host,
                                    const float* box_blob, const int32_t* box_header_host, int32_t* cg_info,
                                    void* workspace, size_t workspace_bytes);
int sol_karman_step_bwd_large(const sol_karman_cfg* cfg, void* stream,
                              const float* saved_vy, const float* saved_vx, const float* re, const float* active,
                              const float* velBCyMask, int64_t bc_batch_stride,
                              const float* g_vy_out, const float* g_vx_out, float* g_vy_in, float* g_vx_in,
                              const int32_t* direct_header_host,
                              const float* box_blob, const int32_t* box_header_host, int32_t* cg_info,
                              void* workspace, size_t workspace_bytes);

/* Adjoint of the step's marker DENSITY, for every grid the 2-D step runs on (csrc/karman_density_bwd.hip; any Y, X >= 2, B <= 65535): the
 * gradient of a loss on d_out with respect to d_in and, through the departure points of the density's advection, to the step's input
 * velocity.  The entry points above carry no density gradient; this one is a separate set of launches that a caller adds when its loss
 * looks at the density.  It needs the step's input density d_in [B,Y,X], the saved post-diffusion velocity of the forward step
 * (sol_karman_step_fwd or sol_karman_step_fwd_large_saved) and g_d_out [B,Y,X]; `inflow` [Y,X] is read only with cfg.inflow_before (the
 * advected field is then d_in + inflow) and may be NULL otherwise.  Per cell (j,i), c = saved velocity, g = g_d_out[j,i]:
 *     uy = (cy[j,i] + cy[j+1,i]) / 2, ux = (cx[j,i] + cx[j,i+1]) / 2; (oy, ox) = -(uy, ux) dt/dx; (fy, fx) = floor; (wy, wx) = o - f
 *     g_d_in[j+fy+dj, i+fx+di] += by(dj) bx(di) g   inside the grid (the zero ghost ring takes nothing)
 *     gU_y[j,i] = -dt/dx g s_y,  gU_x[j,i] = -dt/dx g s_x   with the bilinear slopes s of the gathered field
 *   then g_c = the cell-to-face transpose of gU (g_cy[jf,i] = (gU_y[jf-1,i] + gU_y[jf,i]) / 2, out-of-range cells zero; g_cx likewise) and
 *     g_vy_in = (I + alpha L^T)((1 - velBCyMask) g_cy),  g_vx_in = (I + alpha L^T) g_cx,  alpha = dt res^2 / re[b]
 * as the velocity adjoints apply it.  The scatter into g_d_in is 64-bit fixed point (order independent: results are bit-reproducible; LDS
 * window per 16 x 16 tile, option k2d_dens_adj_tile), scaled by max|g_d_out| of the simulation; a non-finite g_d_out makes EVERY gradient
 * of that simulation NaN.  g_d_in [B,Y,X] is written.  accumulate = 0: g_vy_in / g_vx_in are written; accumulate = 1: the density's part
 * is ADDED onto them (the velocity adjoint wrote there first; one fp32 add per face, deterministic).  Outputs must not alias inputs or
 * each other.  No synchronisation, no allocation, nothing read on the host: capturable.  `workspace`: DEVICE scratch of
 * sol_karman_density_bwd_workspace_bytes(cfg) bytes.  The gradient with respect to `re`: the _re forms below. */
size_t sol_karman_density_bwd_workspace_bytes(const sol_karman_cfg* cfg);
int sol_karman_density_bwd(const sol_karman_cfg* cfg, void* stream,
                           const float* d_in, const float* inflow, const float* saved_vy, const float* saved_vx,
                           const float* re, const float* velBCyMask, int64_t bc_batch_stride,
                           const float* g_d_out, float* g_d_in, float* g_vy_in, float* g_vx_in, int accumulate,
                           void* workspace, size_t workspace_bytes);

/* Gradient with respect to the REYNOLDS NUMBER (csrc/karman_re_bwd.hip).  The step diffuses u = v_in + alpha L v_in with alpha = dt res^2 /
 * re[b], L the replicate-padded 5-point Laplacian; with g' the cotangent of u -- what the adjoints above apply (I + alpha L^T) to: the
 * velocity adjoint's g_c ((1 - velBCyMask) g_c on v_y), the density adjoint's cell-to-face transpose of gU --
 *     g_re[b] = -(dt res^2 / re[b]^2) * sum over the faces of v_y and v_x of  g'_e (L v_in)_e
 * The _re forms take every argument of the plain call and, after `workspace_bytes`, the step's INPUT velocity vy_in [B,Y+1,X], vx_in
 * [B,Y,X+1] (not the saved post-diffusion one), g_re [B] and accumulate_re (0: g_re is written; 1: added onto with one fp32 add -- the
 * density's part after the velocity's).  They issue the plain call's launches (g_vy_in, g_vx_in, g_d_in are the plain call's bits) and two
 * more: fp32 terms, fp64 products and sums in a fixed order whose workgroup count depends on Y, X alone, no floating-point atomics -- g_re
 * is bit-reproducible and independent of the device.  A non-finite cotangent of simulation b makes g_re[b] NaN like its other gradients.
 * sol_karman_step_bwd_large_re serves EVERY grid with Y, X >= 16, the one-workgroup grids included (their saved velocity is the same
 * field; scene blobs as for a large grid: the direct blob, or the box blob for the CG solve); sol_karman_density_bwd_re any Y, X >= 2.
 * The workspace is the plain call's plus the partial sums.  vy_in / vx_in / g_re must not alias an output / an input.  Capturable. */
size_t sol_karman_step_bwd_large_re_workspace_bytes_for(const sol_karman_cfg* cfg, const int32_t* direct_header_host);
int sol_karman_step_bwd_large_re(const sol_karman_cfg* cfg, void* stream,
                                 const float* saved_vy, const float* saved_vx, const float* re, const float* active,
                                 const float* velBCyMask, int64_t bc_batch_stride,
                                 const float* g_vy_out, const float* g_vx_out, float* g_vy_in, float* g_vx_in,
                                 const int32_t* direct_header_host,
                                 const float* box_blob, const int32_t* box_header_host, int32_t* cg_info,
                                 void* workspace, size_t workspace_bytes,
                                 const float* vy_in, const float* vx_in, float* g_re, int accumulate_re);
size_t sol_karman_density_bwd_re_workspace_bytes(const sol_karman_cfg* cfg);
int sol_karman_density_bwd_re(const sol_karman_cfg* cfg, void* stream,
                              const float* d_in, const float* inflow, const float* saved_vy, const float* saved_vx,
                              const float* re, const float* velBCyMask, int64_t bc_batch_stride,
                              const float* g_d_out, float* g_d_in, float* g_vy_in, float* g_vx_in, int accumulate,
                              void* workspace, size_t workspace_bytes,
                              const float* vy_in, const float* vx_in, float* g_re, int accumulate_re);

/* BUOYANCY on the large-grid step (csrc/karman_buoyancy.hip; multi-launch path only): the marker density pushes the velocity, as PhiFlow's
 * IncompressibleFlow.step does with buoyancy_factor != 0.  F = (fy, fx) is a force per unit density (PhiFlow's -gravity * buoyancy_factor
 * with Gravity() = -9.81 along y gives F = (9.81 beta, 0)); it travels as two floats, sol_karman_cfg is unchanged.  With c the
 * post-diffusion velocity, one step is
 *     d_out = SL(d_in [+ inflow], c) [+ inflow dt]                                                          (unchanged)
 *     a_y[jf,i] = mask_y[jf,i] * ( SL_y(c)[jf,i] + dt F_y * (dz(jf-1,i) + dz(jf,i)) / 2 )   jf = 0..Y
 *     a_x[j,if] = mask_x[j,if] * ( SL_x(c)[j,if] + dt F_x * (dz(j,if-1) + dz(j,if)) / 2 )   if = 0..X
 *     dz = d_out inside the grid, 0 outside (the zero ghost ring the density's advection uses)
 *     v_out = a - mask * grad( solve(div a) )                                                               (unchanged)
 * The force acts on the step's OUTPUT density, the inflow already in it (advect, effects, buoyancy, projection: PhiFlow 1.5.1's order as
 * recalled, unpinned -- DESIGN.md section 4.7).  fp32 spelling of a face: fl(v + fl(fl(dt*F) * fl(0.5f * (d0 + d1)))) * mask, no
 * contraction; fl(dt*F) is formed on the host.  A component whose force is zero is not touched; F = (0, 0) issues the plain call's
 * launches and gives its bits.  One extra streaming launch (k_l_buoyancy) between the advection and the divergence, for the direct, the
 * scattered-direct and the CG solve alike.  A non-zero force needs d_in, inflow and d_out.
 *   sol_karman_step_fwd_large_saved_buoy: sol_karman_step_fwd_large_saved with the force.
 *   sol_karman_step_fwd_large_buoy: the no-grad step with features, either solver as the cfg selects it (cfg.direct set: arguments as
 *     sol_karman_step_fwd_large, the box / cg arguments and p_inout unread and p_inout must be NULL; cfg.direct NULL: as
 *     sol_karman_step_fwd_large_cg, p_inout given = the warm-started form), workspace as for that plain call.
 * Adjoint.  With g_a the cotangent of a that the velocity adjoint forms (it carries the face mask),
 *     g_dsum[j,i] = g_d_out[j,i] + dt F_y (g_ay[j,i] + g_ay[j+1,i]) / 2 + dt F_x (g_ax[j,i] + g_ax[j,i+1]) / 2
 * and then the two existing adjoints, unchanged: the velocity adjoint's scatter and diffusion adjoint on g_a, the density adjoint on g_dsum.
 *   sol_karman_step_bwd_large_buoy / _buoy_re: every argument of sol_karman_step_bwd_large / _re, then fy, fx, g_d_out [B,Y,X] (the
 *     cotangent of the step's output density; NULL = zero) and g_dsum [B,Y,X] (written).  They issue the plain call's launches (g_vy_in,
 *     g_vx_in, g_re are the plain call's bits) and one more (k_lb_buoyancy_adj: a gather, no atomics, fixed order, bit-reproducible); same
 *     workspace as the plain call.  The caller then runs sol_karman_density_bwd(_re) with g_dsum as its g_d_out and accumulate = 1.  A
 *     non-finite g_a of a simulation makes ALL of that simulation's g_dsum NaN, so the density adjoint poisons g_d_in and, through the
 *     accumulation, every other gradient of the simulation.  g_dsum must not alias another argument.
 *   sol_karman_buoyancy_add / _add_bwd: the term alone and its exact transpose, any Y, X >= 1, for tests and callers that compose by hand:
 *     vy, vx (in place) = (v + f * face average of d) * mask with f = (fy_dt, fx_dt) = dt F;  g_dsum = g_d_out (NULL = zero) + the
 *     transpose applied to (mask g_vy, mask g_vx).
 * None of these synchronises, allocates or reads anything on the host: capturable. */
int sol_karman_step_fwd_large_saved_buoy(const sol_karman_cfg* cfg, void* stream,
                                         const float* d_in, const float* vy_in, const float* vx_in,
                                         const float* re, const float* active, const float* inflow,
                                         const float* velBCy, const float* velBCyMask, int64_t bc_batch_stride,
                                         float* d_out, float* vy_out, float* vx_out, float* saved_vy, float* saved_vx,
                                         const int32_t* direct_header_host,
                                         const float* box_blob, const int32_t* box_header_host, int32_t* cg_info,
                                         void* workspace, size_t workspace_bytes, float fy, float fx);
int sol_karman_step_fwd_large_buoy(const sol_karman_cfg* cfg, void* stream,
                                   const float* d_in, const float* vy_in, const float* vx_in,
                                   const float* re, const float* active, const float* inflow,
                                   const float* velBCy, const float* velBCyMask, int64_t bc_batch_stride,
                                   float* d_out, float* vy_out, float* vx_out,
                                   float* feat_out, const float* feat_scale,
                                   const int32_t* direct_header_host,
                                   const float* box_blob, const int32_t* box_header_host, int32_t* cg_info,
                                   float* p_inout, void* workspace, size_t workspace_bytes, float fy, float fx);
int sol_karman_step_bwd_large_buoy(const sol_karman_cfg* cfg, void* stream,
                                   const float* saved_vy, const float* saved_vx, const float* re, const float* active,
                                   const float* velBCyMask, int64_t bc_batch_stride,
                                   const float* g_vy_out, const float* g_vx_out, float* g_vy_in, float* g_vx_in,
                                   const int32_t* direct_header_host,
                                   const float* box_blob, const int32_t* box_header_host, int32_t* cg_info,
                                   void* workspace, size_t workspace_bytes,
                                   float fy, float fx, const float* g_d_out, float* g_dsum);
int sol_karman_step_bwd_large_buoy_re(const sol_karman_cfg* cfg, void* stream,
                                      const float* saved_vy, const float* saved_vx, const float* re, const float* active,
                                      const float* velBCyMask, int64_t bc_batch_stride,
                                      const float* g_vy_out, const float* g_vx_out, float* g_vy_in, float* g_vx_in,
                                      const int32_t* direct_header_host,
                                      const float* box_blob, const int32_t* box_header_host, int32_t* cg_info,
                                      void* workspace, size_t workspace_bytes,
                                      const float* vy_in, const float* vx_in, float* g_re, int accumulate_re,
                                      float fy, float fx, const float* g_d_out, float* g_dsum);
int sol_karman_buoyancy_add(void* stream, int32_t B, int32_t Y, int32_t X, const float* active, const float* d,
                            float fy_dt, float fx_dt, float* vy, float* vx);
int sol_karman_buoyancy_add_bwd(void* stream, int32_t B, int32_t Y, int32_t X, const float* active,
                                const float* g_vy, const float* g_vx, float fy_dt, float fx_dt,
                                const float* g_d_out, float* g_dsum);

/* DIFFUSION SUBSTEPS of the karman-2d step (csrc/karman_diffuse_sub.hip; diffusion_substeps = n on the Python surface, PhiFlow's
 * diffuse(field, amount, substeps)).  The step diffuses the velocity with one explicit stencil v += alpha Lap(v), alpha = dt res^2 / Re,
 * which is a convex combination only while alpha <= 1/4; beyond that it amplifies the checkerboard mode.  With n substeps the velocity is
 * diffused n times by alpha / n and the boundary blend comes once, after the last one (the reference's order: diffuse, then blend,
 * karman_train.py:177-181); the rest of the step is unchanged.  Write M = I + (alpha / n) L, L the 5-point Laplacian with replicate
 * padding on each face grid.  Then
 *     step_n(d, v; alpha) = step_1(d, M^(n-1) v; alpha / n)
 * so no existing kernel, entry point or struct changes: the caller computes M^(n-1) v with the entry point below and runs the existing
 * step on a copy of the cfg whose res is float32(res / sqrt(n)); the entry point forms its coefficient from the cfg it is given by the
 * step's own expression, (dt * res * res) / re[b], so on that same copy all n substeps share one coefficient bit for bit.
 * Adjoint: L is symmetric on both face grids, so M^(n-1) is its own transpose -- the existing adjoint on the scaled cfg yields the
 * cotangent of M^(n-1) v and the same entry point applied to it yields the cotangent of v; no scatter, no atomics.  The density is not
 * diffused.  Gradient in re: the factors commute, d(M^n v)/d alpha = L M^(n-1) v, so the existing re reduction on the scaled cfg, given
 * M^(n-1) v as its input velocity, yields 1/n of the gradient: the caller multiplies by n.
 *   sol_karman_diffuse_sub: vy_out, vx_out = (I + a_b L)^m (vy_in, vx_in), a_b = cfg.dt * cfg.res^2 / re[b], m >= 1; of the cfg only B,
 *     Y, X, dt and res are read; Y, X >= 16.  chunk: substeps per launch, 1 .. sol_karman_diffuse_sub_max() (0 = that maximum); a launch
 *     runs its substeps in LDS on tiles with a halo (temporal blocking).  Every substep is fmaf(a_b, lap, c) with lap summed in the
 *     step's order, so the result does not depend on chunk: m launches of one substep and one launch of m substeps give equal bits.
 *     More than one launch ping-pongs through `workspace` (sol_karman_diffuse_sub_workspace_bytes(cfg, m, chunk); 0 bytes and NULL for a
 *     single launch).  The outputs must not alias the inputs.  Does not synchronise, allocate or read device memory on the host: capturable. */
int32_t sol_karman_diffuse_sub_max(void);
size_t sol_karman_diffuse_sub_workspace_bytes(const sol_karman_cfg* cfg, int32_t m, int32_t chunk);
int sol_karman_diffuse_sub(const sol_karman_cfg* cfg, void* stream, const float* vy_in, const float* vx_in, const float* re,
                           float* vy_out, float* vx_out, int32_t m, int32_t chunk, void* workspace, size_t workspace_bytes);

/* MACCORMACK ADVECTION on the large-grid step (csrc/karman_maccormack.hip; multi-launch path only; advection = "mac_cormack" on the
 * Python surface, PhiFlow's advect.mac_cormack(field, velocity, dt, correction_strength)).  The plain step advects semi-Lagrangian
 * (k_l_advect), whose numerical diffusion is the coarse solver's largest error.  c is the post-diffusion velocity (sv_y, sv_x); f is one
 * advected array: c_y on its faces, c_x on its faces, or the density on cells (with inflow added first when cfg.inflow_before); u is c
 * interpolated to the array's sample point with exactly the expressions of k_l_advect; S_g(x) is the bilinear sample of array g in the
 * array's own extrapolation mode: index clamp for the velocity, one ring of zero ghost cells for the density.
 *     h(x)   = S_f(x - u dt)                     the semi-Lagrangian value, unmasked, no inflow added
 *     b(x)   = S_h(x + u dt)                     h carried back, same u, same extrapolation mode
 *     cor(x) = h(x) + (s/2) (f(x) - b(x))        s = correction_strength, 0 <= s <= 1
 *     lo, hi = min, max of the four values the FIRST gather read (after clamping; ghost zeros count)
 *     out(x) = cor(x) if lo <= cor(x) <= hi else h(x)
 * then as in the plain step: velocity times the hard-BC face mask, density + inflow dt when the inflow comes after.  TIE RULE: the compare
 * is inclusive on both sides and has no tolerance (cor == lo or cor == hi keeps cor); a NaN cor reverts to h.  fp32 spelling: h is the
 * bilinear expression of k_l_advect with contraction off, cor = fl(h + fl(fl(0.5f s) * fl(f - b))).
 * The three-term form is PhiFlow 1.5's mac_cormack, the revert-to-semi-Lagrangian limiter is Selle et al. 2008 / PhiFlow 2: both as
 * RECALLED -- parity with PhiFlow is unpinned, as for the buoyancy term.
 * The gradient is the derivative with every decision frozen as the forward step took it: the floorf's, the clamps and the limiter (what
 * torch.where gives a reference).  Where a point reverted, its adjoint is the plain semi-Lagrangian one.  For a cotangent g of out (the
 * velocity's is g_a) and kept = 1 where cor was kept:  g_b = -(s/2) kept g;  g_f += (s/2) kept g;  g_h = g + (g_b scattered through the
 * four corners of the gather at x + u dt);  g_u += +(dt/dx) g_b dS_h/d(offset);  then the semi-Lagrangian adjoint applied to g_h in place
 * of g.  h is recomputed from the saved c: the forward step saves nothing new.  Every scattered sum (g_h included) is 64-bit fixed point
 * with the one scale of its cotangent (csrc/fixed_scatter.hpp): bit-reproducible; a non-finite cotangent poisons its simulation as in the
 * plain adjoints.  Options: k2d_mc_tile (forward), k2d_adj_tile / k2d_dens_adj_tile (the adjoints' LDS windows), equal bits either way.
 *   sol_karman_step_fwd_large_adv / _saved_adv: every argument of the _buoy form, then advection (0 semi-Lagrangian: that form's launches
 *     and bits; 1 MacCormack) and correction_strength (checked to lie in [0, 1] for either).  A zero force is the unbuoyant step.  Workspace:
 *     the *_adv_workspace_bytes_for function of the entry point (advection = 0: the plain size).
 *   sol_karman_step_bwd_large_adv / _adv_re, sol_karman_density_bwd_adv / _adv_re: every argument of the _buoy / _buoy_re form (of the
 *     plain / _re form for the density), then the same two.  Workspace: sol_karman_step_bwd_large_adv_workspace_bytes_for(cfg, header,
 *     with_re, advection), sol_karman_density_bwd_adv_workspace_bytes(cfg, with_re, advection).  The density forms take Y, X >= 16 under
 *     advection = 1.
 *   sol_karman_advect / sol_karman_advect_bwd: the stage alone and its transpose, any Y, X >= 16, for tests and callers that compose by
 *     hand: (d_in, sv_y, sv_x) -> (d_out, a_y, a_x) masked / with inflow as above; cotangents of those -> (g_d_in, g_sv_y, g_sv_x).
 *     tile_window: 1 = LDS windows, 0 = global atomics only.  Workspaces: sol_karman_advect_workspace_bytes(cfg, advection) (0 bytes and
 *     NULL for advection = 0), sol_karman_advect_bwd_workspace_bytes(cfg).
 * None of these synchronises, allocates or reads anything on the host: capturable.  The one-workgroup kernels advect
 * semi-Lagrangian only; karman-3d has its own form ("MACCORMACK ADVECTION on the karman-3d step" below). */
size_t sol_karman_advect_workspace_bytes(const sol_karman_cfg* cfg, int32_t advection);
int sol_karman_advect(const sol_karman_cfg* cfg, void* stream, const float* d_in, const float* svy, const float* svx,
                      const float* active, const float* inflow, int32_t advection, float correction_strength,
                      float* d_out, float* ay, float* ax, void* workspace, size_t workspace_bytes);
size_t sol_karman_advect_bwd_workspace_bytes(const sol_karman_cfg* cfg);
int sol_karman_advect_bwd(const sol_karman_cfg* cfg, void* stream, const float* d_in, const float* svy, const float* svx,
                          const float* active, const float* inflow, int32_t advection, float correction_strength,
                          const float* g_d_out, const float* g_ay, const float* g_ax,
                          float* g_d_in, float* g_svy, float* g_svx, int32_t tile_window, void* workspace, size_t workspace_bytes);
size_t sol_karman_step_fwd_large_adv_workspace_bytes_for(const sol_karman_cfg* cfg, const int32_t* direct_header_host, int32_t advection);
size_t sol_karman_step_fwd_large_saved_adv_workspace_bytes_for(const sol_karman_cfg* cfg, const int32_t* direct_header_host, int32_t advection);
int sol_karman_step_fwd_large_adv(const sol_karman_cfg* cfg, void* stream,
                                  const float* d_in, const float* vy_in, const float* vx_in,
                                  const float* re, const float* active, const float* inflow,
                                  const float* velBCy, const float* velBCyMask, int64_t bc_batch_stride,
                                  float* d_out, float* vy_out, float* vx_out,
                                  float* feat_out, const float* feat_scale,
                                  const int32_t* direct_header_host,
                                  const float* box_blob, const int32_t* box_header_host, int32_t* cg_info,
                                  float* p_inout, void* workspace, size_t workspace_bytes, float fy, float fx,
                                  int32_t advection, float correction_strength);
int sol_karman_step_fwd_large_saved_adv(const sol_karman_cfg* cfg, void* stream,
                                        const float* d_in, const float* vy_in, const float* vx_in,
                                        const float* re, const float* active, const float* inflow,
                                        const float* velBCy, const float* velBCyMask, int64_t bc_batch_stride,
                                        float* d_out, float* vy_out, float* vx_out, float* saved_vy, float* saved_vx,
                                        const int32_t* direct_header_host,
                                        const float* box_blob, const int32_t* box_header_host, int32_t* cg_info,
                                        void* workspace, size_t workspace_bytes, float fy, float fx,
                                        int32_t advection, float correction_strength);
size_t sol_karman_step_bwd_large_adv_workspace_bytes_for(const sol_karman_cfg* cfg, const int32_t* direct_header_host, int32_t with_re,
                                                         int32_t advection);
int sol_karman_step_bwd_large_adv(const sol_karman_cfg* cfg, void* stream,
                                  const float* saved_vy, const float* saved_vx, const float* re, const float* active,
                                  const float* velBCyMask, int64_t bc_batch_stride,
                                  const float* g_vy_out, const float* g_vx_out, float* g_vy_in, float* g_vx_in,
                                  const int32_t* direct_header_host,
                                  const float* box_blob, const int32_t* box_header_host, int32_t* cg_info,
                                  void* workspace, size_t workspace_bytes,
                                  float fy, float fx, const float* g_d_out, float* g_dsum,
                                  int32_t advection, float correction_strength);
int sol_karman_step_bwd_large_adv_re(const sol_karman_cfg* cfg, void* stream,
                                     const float* saved_vy, const float* saved_vx, const float* re, const float* active,
                                     const float* velBCyMask, int64_t bc_batch_stride,
                                     const float* g_vy_out, const float* g_vx_out, float* g_vy_in, float* g_vx_in,
                                     const int32_t* direct_header_host,
                                     const float* box_blob, const int32_t* box_header_host, int32_t* cg_info,
                                     void* workspace, size_t workspace_bytes,
                                     const float* vy_in, const float* vx_in, float* g_re, int accumulate_re,
                                     float fy, float fx, const float* g_d_out, float* g_dsum,
                                     int32_t advection, float correction_strength);
size_t sol_karman_density_bwd_adv_workspace_bytes(const sol_karman_cfg* cfg, int32_t with_re, int32_t advection);
int sol_karman_density_bwd_adv(const sol_karman_cfg* cfg, void* stream,
                               const float* d_in, const float* inflow, const float* saved_vy, const float* saved_vx,
                               const float* re, const float* velBCyMask, int64_t bc_batch_stride,
                               const float* g_d_out, float* g_d_in, float* g_vy_in, float* g_vx_in, int accumulate,
                               void* workspace, size_t workspace_bytes, int32_t advection, float correction_strength);
int sol_karman_density_bwd_adv_re(const sol_karman_cfg* cfg, void* stream,
                                  const float* d_in, const float* inflow, const float* saved_vy, const float* saved_vx,
                                  const float* re, const float* velBCyMask, int64_t bc_batch_stride,
                                  const float* g_d_out, float* g_d_in, float* g_vy_in, float* g_vx_in, int accumulate,
                                  void* workspace, size_t workspace_bytes,
                                  const float* vy_in, const float* vx_in, float* g_re, int accumulate_re,
                                  int32_t advection, float correction_strength);

/* active  [Y,X]  1 - obstacle mask (cell centres inside Obstacle geometries -> 0)
 * inflow  [Y,X]  inflow rate mask (Inflow(box[5:10,25:75]) -> 1 inside)
 * velBCy, velBCyMask  [Y+1,X] (bc_batch_stride 0) or [B,Y+1,X] (stride (Y+1)*X)
 * saved_vy/saved_vx: post-diffusion+BC velocity kept for the backward pass (NULL: inference)
 * feat_out [B,Y,X,4] (NULL to skip): fused to_feature (karman_train.py:77-86) scaled by
 *   feat_scale[3] = 1/std (l.416-419), a HOST array; channel 3 is zero padding.
 * iters [B]: CG iterations used per simulation (may be NULL).                           */
int sol_karman_step_fwd(const sol_karman_cfg* cfg, void* stream,
                        const float* d_in, const float* vy_in, const float* vx_in,
                        const float* re, const float* active, const float* inflow,
                        const float* velBCy, const float* velBCyMask, int64_t bc_batch_stride,
                        float* d_out, float* vy_out, float* vx_out,
                        float* saved_vy, float* saved_vx,
                        float* feat_out, const float* feat_scale,
                        int32_t* iters);

/* Adjoint of the step w.r.t. its input velocity (density is a passive tracer and has no
 * adjoint: buoyancy_factor=0, karman_train.py:363).  The pressure adjoint is a second CG
 * solve with the same symmetric matrix (PhiFlow's custom gradient).
 * dfeat [B,Y,X,2] (may be NULL): gradient w.r.t. the fused feature channels 0,1; it is
 *   added as g_v_out += feat_scale[c]*dfeat[...,c] before the adjoint runs.              */
int sol_karman_step_bwd(const sol_karman_cfg* cfg, void* stream,
                        const float* saved_vy, const float* saved_vx,
                        const float* re, const float* active,
                        const float* velBCyMask, int64_t bc_batch_stride,
                        const float* g_vy_out, const float* g_vx_out,
                        const float* dfeat, const float* feat_scale,
                        float* g_vy_in, float* g_vx_in,
                        int32_t* iters);

/* ------------------------------------------------------------------------------------
 * Burgers step: BurgersTest.step / step_with_f (burgers/burgers_train.py:182-187) =
 *   semi-Lagrangian self-advection on the periodic staggered grid followed by PhiFlow's
 *   periodic (spectral) diffusion, expressed as two real circulant matrices cy [Y+1,Y+1]
 *   (for v_y rows) ... see sol_burgers_cfg; then v += dt*f.
 * ---------------------------------------------------------------------------------- */
typedef struct sol_burgers_cfg {
    int32_t B, Y, X;        /* cells; staggered arrays v_y [B,Y+1,X], v_x [B,Y,X+1]  (<= 64; *_large: <= 1024) */
    float dx, dt;
} sol_burgers_cfg;

/* circ_* are the symmetric circulant matrices of exp(-(2 pi k)^2 * nu*dt), row major:
 * circ_yp1 [Y+1,Y+1], circ_x [X,X] act on v_y; circ_y [Y,Y], circ_xp1 [X+1,X+1] on v_x.
 * f_y/f_x may be NULL (BurgersTest.step).  saved_* keep the input velocity for backward. */
int sol_burgers_step_fwd(const sol_burgers_cfg* cfg, void* stream,
                         const float* vy_in, const float* vx_in,
                         const float* f_y, const float* f_x,
                         const float* circ_yp1, const float* circ_x,
                         const float* circ_y, const float* circ_xp1,
                         float* vy_out, float* vx_out);
int sol_burgers_step_bwd(const sol_burgers_cfg* cfg, void* stream,
                         const float* vy_in, const float* vx_in,
                         const float* circ_yp1, const float* circ_x,
                         const float* circ_y, const float* circ_xp1,
                         const float* g_vy_out, const float* g_vx_out,
                         float* g_vy_in, float* g_vx_in);

/* Burgers step for grids beyond the one-workgroup kernels (up to 1024 x 1024): the reference generates its training data at
 * 128 x 128 (burgers/Makefile:19-29, `burgers.py -r 128`; PhiFlow Burgers.step on the CPU there).  Same arguments as
 * sol_burgers_step_fwd plus a workspace of sol_burgers_step_large_workspace_bytes(cfg).  The step's input velocity is what its
 * adjoint, sol_burgers_step_bwd_large below, takes. */
size_t sol_burgers_step_large_workspace_bytes(const sol_burgers_cfg* cfg);
int sol_burgers_step_fwd_large(const sol_burgers_cfg* cfg, void* stream, const float* vy_in, const float* vx_in,
                               const float* f_y, const float* f_x, const float* circ_yp1, const float* circ_x,
                               const float* circ_y, const float* circ_xp1, float* vy_out, float* vx_out,
                               void* workspace, size_t workspace_bytes);

/* Adjoint of sol_burgers_step_fwd_large with respect to the input velocity (d f = dt * g_out is the caller's): arguments as
 * sol_burgers_step_bwd plus a workspace.  Seven kernel launches on `stream` and nothing else (no memset / memcpy, no host
 * synchronisation), so the call can be captured: clear, the forward's four circulant products on the cotangent (the circulants are
 * symmetric), the advection adjoint as an order-independent scatter in 64-bit fixed point (bit-reproducible; a non-finite cotangent
 * makes every input gradient of ITS simulation NaN), conversion to fp32.  B <= 65535, 2 <= Y, X <= 1024; g_vy_in / g_vx_in must not
 * alias the inputs.  With F = (Y+1) X + Y (X+1) faces and r(n) = n rounded up to a multiple of 256, the workspace is
 * r(8 B F) + 2 r(4 B F) + r(256 B) + 256 bytes (accumulators, g_a, one product, absmax slots, alignment of `workspace`);
 * sol_burgers_step_bwd_large_workspace_bytes returns 0 for a cfg the adjoint does not take. */
size_t sol_burgers_step_bwd_large_workspace_bytes(const sol_burgers_cfg* cfg);
int sol_burgers_step_bwd_large(const sol_burgers_cfg* cfg, void* stream, const float* vy_in, const float* vx_in,
                               const float* circ_yp1, const float* circ_x, const float* circ_y, const float* circ_xp1,
                               const float* g_vy_out, const float* g_vx_out, float* g_vy_in, float* g_vx_in,
                               void* workspace, size_t workspace_bytes);

/* ------------------------------------------------------------------------------------
 * 5x5 SAME convolution, NHWC fp32 tensors.  32-input-channel layers with W % 64 == 0 evaluate their fp32 products as
 * exact 16-bit MFMA products of operand splits with fp32 accumulation (option conv_precision; 2 = fp32 MFMA
 * v_mfma_f32_16x16x4_f32 throughout); the thin 3->32 / 32->2 layers and other shapes run on fp32 MFMA.
 * Replaces keras.layers.Conv2D(filters, 5, padding='same') + LeakyReLU / add
 * (karman_train.py:101-138) and its TF gradients.
 * ---------------------------------------------------------------------------------- */
#define SOL_CONV_FWD 0        /* pack for y = conv(x, w)                       */
#define SOL_CONV_BWD_DATA 1   /* pack for dx = conv(dy, flip(w)^T)             */
/* number of floats of a packed weight buffer for (cin, cout, mode) */
size_t sol_conv5x5_packed_floats(int32_t cin, int32_t cout, int32_t mode);
/* w_hwio [5,5,cin,cout] -> packed (zero padded to the MFMA tile shape) */
int sol_conv5x5_pack(void* stream, const float* w_hwio, int32_t cin, int32_t cout,
                     int32_t mode, float* packed);

/* n <= 24 (layer, mode) pack jobs in ONE launch -- same packed layout as n calls of sol_conv5x5_pack (cin[k], cout[k] as there: of the
 * convolution being RUN; packed[k] of sol_conv5x5_packed_floats(cin[k], cout[k], mode[k]) floats).  For hosts that compose the unrolled
 * step themselves (the Python schedules of model_mercury / the Burgers path): one launch per training step instead of ~100.          */
int sol_conv5x5_pack_jobs(void* stream, int32_t n, const float* const* w_hwio, const int32_t* cin, const int32_t* cout,
                          const int32_t* mode, float* const* packed);

#define SOL_EPI_NONE 0        /* y = conv + bias (+ residual)                       */
#define SOL_EPI_LRELU 1       /* y = lrelu(conv + bias (+ residual))                */
#define SOL_EPI_DLRELU 2      /* y = (conv (+ residual)) * lrelu'(act_ref)  (backward) */
/* x [B,H,W,cin]; packed from sol_conv5x5_pack with the same (cin,cout) (for BWD_DATA pass
 * cin = channels of dy, cout = channels of dx, and the weights packed with mode BWD_DATA
 * from the forward layer's (cout_fwd=cin, cin_fwd=cout)); bias [cout] or NULL;
 * residual/act_ref [B,H,W,cout] or NULL; y [B,H,W,cout].  H*W % 64 == 0, W | 64 or 64 | W. */
int sol_conv5x5(void* stream, const float* x, const float* packed, const float* bias,
                const float* residual, const float* act_ref, float* y,
                int32_t B, int32_t H, int32_t W, int32_t cin, int32_t cout,
                int32_t epilogue, float slope);

/* sol_conv5x5 with per-tensor absmax bookkeeping: `x_absmax` / `y_absmax` are DEVICE arrays of SOL_ABSMAX_SLOTS
 * uint32 slots (16-byte aligned; one slot per workgroup of a full-chip launch, because same-address atomics serialise
 * in the L2) whose maximum holds the bit pattern of max|x| / max|y| (non-negative floats compare like unsigned integers).
 * y_absmax (or NULL): slots are raised with atomic max by this launch (the caller zeroes them once per tensor).
 * x_absmax (or NULL): when given for a 32-input-channel, W % 64 == 0 convolution, the fp32 products are evaluated as
 * THREE fp16 MFMA products of operands scaled by a power of two derived from the absmax (22-bit operand splits, fp32
 * accumulation; error relative to max|x| max|w| like the fp32 kernel's) instead of six bf16 products.  The producer of x
 * publishes its absmax in the unrolled training graph, so no extra pass over the data exists. */
#define SOL_ABSMAX_SLOTS 256
int32_t sol_absmax_slots(void);   /* == SOL_ABSMAX_SLOTS of the library that was loaded */
/* slots[0..SOL_ABSMAX_SLOTS) = bit patterns whose maximum is max|x| over x[0..n): for tensors whose producer did not publish it */
int sol_absmax(void* stream, const float* x, int64_t n, uint32_t* slots);
int sol_conv5x5_scaled(void* stream, const float* x, const float* packed, const float* bias,
                       const float* residual, const float* act_ref, float* y,
                       int32_t B, int32_t H, int32_t W, int32_t cin, int32_t cout,
                       int32_t epilogue, float slope, const uint32_t* x_absmax, uint32_t* y_absmax);

/* sol_conv5x5_scaled on PITCHED rows: the tensors x, residual, act_ref and y are [B,H,W,c] buffers whose rows hold WV <= W pixels of
 * data followed by W - WV pad pixels, W (the pitch) a multiple of 64 and 1 <= WV <= W -- the layout in which an image of any width
 * WV runs on the 64-pixel-tile kernels (pitch 64 * ceil(WV / 64)).
 *   - Columns >= WV of x, residual and act_ref are ZERO.  This is the caller's duty and is not checked: with zero pad columns the
 *     SAME-padding halo of the valid columns is what a dense [B,H,WV,c] image has, so the valid columns of y are the dense result.
 *   - Columns >= WV of y are WRITTEN as 0.0f (every pad pixel is stored; the caller never clears an output buffer), so y can be
 *     the next layer's x as it is.
 *   - y_absmax covers the valid columns only.
 * x_absmax / y_absmax may be NULL; the kernel choice then follows sol_conv5x5.  WV == W launches exactly what sol_conv5x5_scaled
 * launches; WV < W launches the column-masked instantiation of that same kernel.  Rejected before any launch: W % 64 != 0, WV < 1,
 * WV > W, NULL x / packed / y.
 * The weight gradient needs no such form: with x and dz zero in the pad columns, sol_conv5x5_bwd_weight at the pitch W returns the
 * dense image's dw and db (the pad pixels contribute exact zeros). */
int sol_conv5x5_cols(void* stream, const float* x, const float* packed, const float* bias,
                     const float* residual, const float* act_ref, float* y,
                     int32_t B, int32_t H, int32_t W, int32_t WV, int32_t cin, int32_t cout,
                     int32_t epilogue, float slope, const uint32_t* x_absmax, uint32_t* y_absmax);

/* CIRCULAR PADDING of the 5x5 convolutions on a periodic scene (csrc/conv_halo.hip).  The convolution kernels pad with zeros; on a
 * periodic axis the network runs in buffers that carry a two-pixel HALO on either side of that axis instead, and this launch refreshes
 * the halo between the convolutions.  With py, px in {0, 1} from periodic_bits (2 = y, 4 = x, 6 = both, as for sol_karman_seam_sync; 0:
 * nothing is launched) an [H, W] image lives in buf [B, H + 4 py, P, C]: valid pixels at rows [2 py, 2 py + H) and columns
 * [2 px, 2 px + W), the halo two rows / columns on either side, columns >= W + 4 px the zero pad of the pitched layout.  Every
 * convolution is sol_conv5x5_cols at the pitch P with WV = W + 4 px and H + 4 py rows: its halo outputs (computed with zeros beyond the
 * buffer edge) are wrong and are overwritten by the next call of this function; its valid outputs are the circular convolution, because
 * their stencils read halos that hold wrapped copies.
 *   mode 0 (wrap): every halo cell = the valid cell at its index modulo H / W (a true modulo: any H, W >= 1; with both axes periodic the
 *                  2x2 corners come from the diagonally opposite corners).
 *   mode 1 (zero): every halo cell = 0 -- the dz operand of sol_conv5x5_bwd_weight, so that only valid pixels contribute to dw and db
 *                  (x keeps its wrapped halo: dw[k] = sum over valid p of x[p + k] dz[p]).  The backward-data convolution then takes
 *                  the WRAPPED dz: the adjoint of a circular convolution is the circular correlation.
 * Valid cells and pad columns are never written.  C: a multiple of 4 up to 32; P: a multiple of 64, P >= W + 4 px.  One launch, vector
 * stores, no atomics, no host synchronisation: capturable.  SOL_ERR_ARG with a message: NULL buf, P < W + 4 px, P % 64 != 0, bits other
 * than 0 / 2 / 4 / 6, a mode other than 0 / 1, a C it does not take. */
int sol_conv_halo(void* stream, float* buf, int32_t B, int32_t H, int32_t W, int32_t P, int32_t C, int32_t periodic_bits, int32_t mode);

/* dW[5,5,cin,cout] += sum_px x[px+tap] * dz[px];  db[cout] += sum_px dz[px].
 * `partial` is a caller workspace of sol_conv5x5_bwd_weight_ws_floats() floats that the
 * caller zeroes once and may reuse to ACCUMULATE over many calls (the unrolled steps share
 * the weights); sol_conv5x5_bwd_weight_reduce() folds it into dw/db.
 * W: 4 <= W <= 64 with W % 4 == 0, or a multiple of 64 (W / 64 column tiles per row block, each
 * with its own slice of `partial`: the workspace grows by that factor).
 * THE REDUCE FOLDS IN PLACE: despite the `const`, sol_conv5x5_bwd_weight_reduce (and _reduce_jobs, and
 * sol_conv5x5_bwd_weight_segments_reduce) write chunk sums of 16 row blocks back into `partial` whenever it
 * holds more than 16 blocks.  After a reduce the contents of `partial` are unspecified: zero it (or launch
 * with overwrite) before the next accumulation, and reduce a copy if the partial sums are still needed. */
size_t sol_conv5x5_bwd_weight_ws_floats(int32_t B, int32_t H, int32_t W, int32_t cin, int32_t cout);
int sol_conv5x5_bwd_weight(void* stream, const float* x, const float* dz, float* partial,
                           int32_t B, int32_t H, int32_t W, int32_t cin, int32_t cout);
int sol_conv5x5_bwd_weight_reduce(void* stream, const float* partial, float* dw_hwio, float* db,
                                  int32_t B, int32_t H, int32_t W, int32_t cin, int32_t cout,
                                  int32_t accumulate);

/* sol_conv5x5_bwd_weight_reduce for n <= 12 layers of one image size (B, H, W) in two launches; same summation order.  dw_hwio[k] /
 * db[k] may point into a flat gradient buffer (Keras get_weights() order).  cin[k] = real input channels of layer k.            */
int sol_conv5x5_bwd_weight_reduce_jobs(void* stream, int32_t n, float* const* partial, float* const* dw_hwio, float* const* db,
                                       int32_t B, int32_t H, int32_t W, const int32_t* cin, const int32_t* cout, int32_t accumulate);

/* The scaled, segmented form that the fused trainers launch, W <= 64: `nseg` tensors of [B,H,W,c] (the unrolled steps of one layer)
 * in ONE launch.  Segment s reads x + s * x_seg and dz + s * dz_seg (strides in floats); the rows of all segments form one sequence
 * of nseg * B * H rows that is cut into row blocks of 8 rows, or of ceil(rows / 256) rows (ceil(rows / 1024) for cin == 4 or
 * cout == 2) beyond 4096 rows.  `partial`: sol_conv5x5_bwd_weight_segments_ws_floats() floats.
 *   overwrite  1: every word of `partial` that the reduce reads is stored (no zeroing needed); 0: added to, as sol_conv5x5_bwd_weight.
 *   x_absmax / dz_absmax (both or NULL): SOL_ABSMAX_SLOTS slots per segment, segment s at x_absmax + s * absmax_seg (uint32 words).
 *              With both given, (cin, cout) == (32, 32), W == 64, conv_precision 0 and B * H a multiple of the row block, the products
 *              are three fp16 MFMA products of operands scaled PER SEGMENT; a row block that would hold rows of two segments takes
 *              the six-product bf16 body instead, which reads no slots.  Slots may over-report the maximum: that costs fp16 range, not
 *              mantissa bits (elements below 2^-19 of the REPORTED maximum lose their low part); slots that under-report it
 *              overflow fp16.
 *   cin_real   1..3 with cin == 4, cout == 32, W == 64: the channels of x beyond cin_real are zero padding and their gradient rows
 *              are NOT computed (nor stored under overwrite): reduce with cin = cin_real.  0: all cin channels are data.
 * Rejected before any launch: nseg < 1, W > 64, and everything sol_conv5x5_bwd_weight rejects.
 * sol_conv5x5_bwd_weight_segments_reduce: partial -> dw_hwio [5,5,cin,cout], db [cout] for the same (nseg, B, H); cin = real input
 * channels (1..32).  Folds in place (see above). */
size_t sol_conv5x5_bwd_weight_segments_ws_floats(int32_t nseg, int32_t B, int32_t H, int32_t cin, int32_t cout);
int sol_conv5x5_bwd_weight_segments(void* stream, const float* x, const float* dz, float* partial, int32_t nseg, int64_t x_seg, int64_t dz_seg,
                                    int32_t overwrite, int32_t B, int32_t H, int32_t W, int32_t cin, int32_t cout,
                                    const uint32_t* x_absmax, const uint32_t* dz_absmax, int64_t absmax_seg, int32_t cin_real);
int sol_conv5x5_bwd_weight_segments_reduce(void* stream, float* partial, float* dw_hwio, float* db, int32_t nseg, int32_t B, int32_t H,
                                           int32_t cin, int32_t cout, int32_t accumulate);

/* ------------------------------------------------------------------------------------
 * Whole training step: the unrolled msteps graph of karman_train.py:397-457
 *   for i in range(msteps): state = simulator_lo.step(state);  state.velocity += CNN(state)
 *   loss = sum_i l2_loss((gt_i - prd_i)/std_v)/msteps;  Adam.
 * ---------------------------------------------------------------------------------- */
typedef struct sol_train_cfg {
    sol_karman_cfg karman;
    int32_t msteps;
    float std_v0, std_v1;   /* dataStats['std'][1]  (karman_train.py:234-255,419,432) */
    float std_re;           /* dataStats['ext.std'][0]                                 */
    float lrelu_slope;      /* Keras LeakyReLU default 0.3                              */
    /* --pretf (karman_train.py:351-355, 416-421): a pre-trained supervised model brings its OWN input / output
     * normalisation ('in.std', 'out.std' of its stats.pickle) while the loss keeps dataStats['std'].  0 = use std_v*. */
    float in_std_v0, in_std_v1;     /* feature scale of the velocity channels: feat = v / in_std       */
    float out_std_v0, out_std_v1;   /* correction scale: velocity += out_std * CNN(feat)                */
} sol_train_cfg;

size_t sol_train_workspace_bytes(const sol_train_cfg* cfg);

/* params/grads: SOL_MARS_MOON_PARAMS floats.  gt_vy [msteps,B,Y+1,X], gt_vx [msteps,B,Y,X+1].
 * Outputs: grads (overwritten), loss_steps[msteps] (device, the per-step l2_loss values,
 * NOT yet divided by msteps), optional prd_* = final corrected state (may be NULL),
 * iters_fwd/iters_bwd [msteps*B] CG iteration counts (device, may be NULL).             */
int sol_train_fwd_bwd(const sol_train_cfg* cfg, void* stream,
                      const float* params,
                      const float* d0, const float* vy0, const float* vx0, const float* re,
                      const float* active, const float* inflow,
                      const float* velBCy, const float* velBCyMask, int64_t bc_batch_stride,
                      const float* gt_vy, const float* gt_vx,
                      void* workspace, size_t workspace_bytes,
                      float* grads, float* loss_steps,
                      float* d_final, float* vy_final, float* vx_final,
                      int32_t* iters_fwd, int32_t* iters_bwd);

/* The same step as a replayable hipGraph: one host call per training step instead of ~1000 kernel
 * launches.  All pointers are baked in at creation (re-create when a buffer moves); new data is
 * fed by copying into the same buffers.  sol_train_graph_launch replays it on the caller's stream;
 * the library opens no streams of its own for training.                                        */
typedef struct sol_train_graph sol_train_graph;
int sol_train_graph_create(const sol_train_cfg* cfg, const float* params,
                           const float* d0, const float* vy0, const float* vx0, const float* re,
                           const float* active, const float* inflow,
                           const float* velBCy, const float* velBCyMask, int64_t bc_batch_stride,
                           const float* gt_vy, const float* gt_vx,
                           void* workspace, size_t workspace_bytes,
                           float* grads, float* loss_steps,
                           float* d_final, float* vy_final, float* vx_final,
                           int32_t* iters_fwd, int32_t* iters_bwd, sol_train_graph** out);
int sol_train_graph_launch(sol_train_graph* graph, void* stream);
int sol_train_graph_destroy(sol_train_graph* graph);

/* Graph-capture guard.  The reference builds its TF graph once and runs it many times (karman_train.py:385-391, 502); here that shape is a
 * captured hipGraph, and a graph on this path may hold KERNEL nodes only (plus empty / event / child-graph nodes): memset nodes replay
 * unreliably on ROCm 7.2 (a torch reduction's semaphore clear inside a captured trainer made the reported losses 0.5x / 2x the true values
 * after a few replays), memcpy / host / alloc nodes mean work that is not a kernel of this path sits in the replayed region.
 *   sol_graph_census  counts[t] = number of nodes of hipGraphNodeType t in `graph` (a hipGraph_t; child graphs are entered), t < ncounts <= 64
 *   sol_graph_check   SOL_ERR_GRAPH (and a message naming the node types and `what`) when the graph holds a memset, memcpy, memcpy-to/from-
 *                     symbol, host, mem-alloc or mem-free node; SOL_OK otherwise.  sol_train_graph_create applies it to its own capture; a
 *                     host that captures the per-op entry points itself calls it between hipStreamEndCapture and hipGraphInstantiate.    */
/*   sol_copy_words    dst[0..nwords) = src[0..nwords) (32-bit words; src NULL: zero fill) as ONE KERNEL launch: the copy a host uses inside
 *                     a stream capture instead of hipMemcpyAsync / hipMemsetAsync (torch: tensor.copy_ / clone() of a contiguous tensor).   */
int sol_copy_words(void* stream, void* dst, const void* src, int64_t nwords);
/*   sol_clock_probe   measurement aid (bench.py): every SIMD runs a chain of `iters` dependent v_mfma_f32_16x16x16_f16; out4 (device) =
 *                     {duration in 10 ns ticks (s_memrealtime), duration in s_memtime ticks, iters, 0}.  ns per dependent MFMA follows
 *                     the engine clock the device holds under matrix load: it tells a slow box from a slower kernel.                  */
int sol_clock_probe(void* stream, uint64_t* out4, int32_t iters);
/*   sol_clock_stamp   out16 (device, zero it first) [xcd] = {s_memtime, s_memrealtime} of XCD `xcd` (0..7) at this point of the stream (every XCD
 *                     has its own counter).  Two stamps around a region give the AVERAGE shader clock the device held while the region ran:
 *                     100 MHz x d(memtime) / d(memrealtime) per XCD (gfx950: s_memtime counts engine clocks).  bench.py brackets its timed steps.  */
int sol_clock_stamp(void* stream, uint64_t* out16);
/*   sol_latency_probe measurement aid (bench.py): one lane walks `steps` dependent loads through a ZERO-FILLED device buffer of `nlines` 128-byte
 *                     lines (a power of two) in a pseudo-random order; out4 (device) = {duration in 10 ns ticks, steps, last index, -}.  ns per
 *                     load = the memory round trip a kernel's first loads pay (the L2 is invalid at every kernel boundary).                   */
int sol_latency_probe(void* stream, const uint32_t* buf, int64_t nlines, int32_t steps, uint64_t* out4);
int sol_graph_census(void* graph, int32_t* counts, int32_t ncounts);
int sol_graph_check(void* graph, const char* what);
const char* sol_graph_node_type_name(int32_t type);

/* Forward only (karman_apply.py:138-158 roll-out without the frame dump): runs `nsteps`
 * solver+CNN steps in place of d/vy/vx.  workspace: sol_rollout_workspace_bytes().       */
size_t sol_rollout_workspace_bytes(const sol_train_cfg* cfg);
int sol_rollout(const sol_train_cfg* cfg, void* stream, const float* params,
                float* d, float* vy, float* vx, const float* re,
                const float* active, const float* inflow,
                const float* velBCy, const float* velBCyMask, int64_t bc_batch_stride,
                int32_t nsteps, void* workspace, size_t workspace_bytes, int32_t* iters);

/* Stand-alone loss of ONE unrolled step (karman_train.py:428-436: tf.nn.l2_loss((gt.staggered - prd.staggered) / std_v)):
 *   loss (+)= 0.5 * sum_c sum_e ((gt_c[e] - v_c[e]) / std[c])^2        (accumulate_loss = 0 overwrites loss[0])
 *   g_c[e] (+)= gscale * (v_c[e] - gt_c[e]) / std[c]^2                  (d loss / d v; g may be NULL: forward only; gscale = 1/msteps
 *                                                                        for the reference's loss = sum_i / msteps, l.436)
 * v / gt / g / n / std: HOST arrays of ncomp (1..3) entries -- the staggered components v_y [B,Y+1,X], v_x [B,Y,X+1] (, v_z): the
 * zero-padded faces of staggered_tensor() contribute nothing.  scratch: sol_l2_loss_scratch_floats() device floats.  The sum is
 * folded in a fixed order (bit-reproducible).  The trainers (sol_train_*) fuse this loss into their last CNN layer; this entry
 * point serves hosts that compose the step from the per-op ABI. */
int32_t sol_l2_loss_scratch_floats(void);
int sol_l2_loss_fwd_bwd(void* stream, int32_t ncomp, const float* const* v, const float* const* gt, float* const* g,
                        const int64_t* n, const float* std, float gscale, int32_t accumulate_g,
                        float* loss, int32_t accumulate_loss, float* scratch);

/* tf.compat.v1.train.AdamOptimizer update (karman_train.py:449-457), epsilon-hat form:
 *   lr_t = lr*sqrt(1-b2^t)/(1-b1^t);  p -= lr_t*m/(sqrt(v)+eps).
 * clip_norm > 0: per-tensor tf.clip_by_norm(g, clip_norm) first (l.451-454), tensors given
 * by tensor_offsets[n_tensors+1] (HOST array, element offsets).  t is the 1-based step.  */
int sol_adam_tf_step(void* stream, float* params, const float* grads, float* m, float* v,
                     int64_t n, int32_t t, float lr, float beta1, float beta2, float eps,
                     float clip_norm, const int64_t* tensor_offsets, int32_t n_tensors,
                     float* scratch /* >= n_tensors floats, device */);

/* ------------------------------------------------------------------------------------
 * Data-parallel exchange (new capability; the reference is single device, karman_train.py:22,49):
 * the gradients of independent simulations add (the loss is a batch SUM, karman_train.py:430), so N ranks, one per
 * GPU, run the full unroll on their shard and SUM the flat gradient once per training step over RCCL / xGMI.
 * RCCL is bound at run time (dlopen librccl.so.1); nothing here is needed on one GPU.
 *   rank 0: sol_comm_unique_id(id) -> the host distributes the 128 bytes (any side channel) ->
 *   every rank: sol_comm_init(id, nranks, rank, &comm) with ITS device current -> sol_allreduce_grads per step.
 * ---------------------------------------------------------------------------------- */
#define SOL_COMM_ID_BYTES 128
typedef struct sol_comm sol_comm;
int sol_comm_unique_id(char* id /* [SOL_COMM_ID_BYTES], host */);
int sol_comm_init(const char* id, int32_t nranks, int32_t rank, sol_comm** out);
/* in-place SUM over all ranks of flat_grad[count] (device fp32), asynchronous on `stream` */
int sol_allreduce_grads(sol_comm* comm, void* stream, float* flat_grad, int64_t count);
int sol_comm_destroy(sol_comm* comm);

/* ------------------------------------------------------------------------------------
 * karman-3d (BASELINE.json configs[4]: 128 x 64 x 64).  The reference has NO 3-D code (/root/reference/README.md:37-38);
 * these entry points are the dimension-generic twins of the 2-D ones: the same KarmanFlow.step
 * (karman-2d/karman_train.py:173-185) with a third axis, and model_mars_moon (karman_train.py:101-138) with Conv3D(5)
 * layers.  Layout: density [B,Y,X,Z], v_y [B,Y+1,X,Z], v_x [B,Y,X+1,Z], v_z [B,Y,X,Z+1] (y = flow direction, z
 * contiguous); CNN tensors NDHWC = [B,Y,X,Z,C].  Forward step (sol_karman3d_step_fwd), its adjoint w.r.t. the input
 * velocity (sol_karman3d_step_bwd), the Conv3D forward / backward-data (sol_conv3d, incl. the fused SOL_EPI_DLRELU reverse
 * sweep epilogue) and the Conv3D weight gradient (sol_conv3d_bwd_weight): everything karman3d.Karman3DTrainer composes.
 * ---------------------------------------------------------------------------------- */
typedef struct sol_karman3d_cfg {
    int32_t B, Y, X, Z;     /* batch, cells per axis                                                   */
    float dx;               /* cell size = len / X                                                      */
    float dt;               /* time step                                                                */
    float res;              /* `res` of step(): alpha = dt*res*res/Re (karman_train.py:175)             */
    int32_t grad_pad;       /* 0: replicate (PhiFlow 1.x), 1: dirichlet0                                */
    int32_t inflow_before;  /* 0: density += inflow*dt after advection, 1: before                       */
    int32_t direct_n;       /* number of 32-bit words of `direct`                                        */
    const float* direct;    /* DEVICE blob of the direct pressure solver for the scene's `active` mask
                               (three sine-transform matrices, 1/eigenvalues, capacitance matrix of the
                               obstacle cells; layout: precond3d.direct_solver_blob3d).  Required.
                               Two layouts, told apart by the magic in word 0 (32-bit words; N = Y X Z):
                               "FD33" header[16] = {magic, Y, X, Z, nS, SP}; Qy[Y*Y]; Qx[X*X]; Qz[Z*Z]; invlam[N];
                                      KpT[SP][SP] (K' transposed, zero padded, SP % 64 == 0); sidx[SP] int32 (cell index
                                      (j X + i) Z + k, -1 = padding).  nS = 0: the empty box (what the CG solve takes).
                               "FD3E" (precond3d.extruded_solver_blob3d: an obstacle extruded along z, active[j][i][k] =
                                      a2[j][i]) header[16] = {magic, Y, X, Z, nS2, SP2}; Qy, Qx, Qz, invlam as above;
                                      KpT[Z][SP2][SP2] (K'_m of z mode m, transposed, zero padded, SP2 % 32 == 0);
                                      sidx2[SP2] int32 (in-plane cell index j X + i, -1 = padding).  1 <= nS2 <= SP2 <= 1024,
                                      SP2 <= Y X, Z <= 128, Z SP2^2 <= 2^26.  Direct solve only (pressure_solver = 0): the
                                      capacitance product becomes Z products of size SP2 between two sine transforms
                                      along z of the support columns; same entry points, same workspace sizes.            */
    /* pressure solver (all zero = the direct solve; appended in ABI 216) */
    int32_t pressure_solver;   /* 0: direct (capacitance blob), 1: preconditioned CG (blob with nS = 0)  */
    int32_t cg_max_iter;       /* CG: launch budget in iterations (>= 1); the launch sequence is fixed    */
    float cg_rtol, cg_atol;    /* CG: a simulation stops when |r|_2 <= max(cg_rtol |b|_2, cg_atol)        */
    int32_t* cg_info;          /* CG: DEVICE [B][2] or NULL: iterations used, converged (0/1), written by
                                  every solve (the adjoint's solve overwrites the forward's)              */
} sol_karman3d_cfg;
int32_t sol_abi_size_karman3d(void);      /* sizeof(sol_karman3d_cfg) of the library (checked by the ctypes mirror) */

/* Arguments as sol_karman_step_fwd_large with the third component; active / inflow [Y,X,Z]; velBCy / velBCyMask
 * [Y+1,X,Z] (bc_batch_stride 0) or [B,Y+1,X,Z]; feat_out [B,Y,X,Z,4] (or NULL): fused to_feature = the three components
 * at the low faces of every cell and Re, each times feat_scale[c] (HOST array of 4 = 1/std).  direct_header_host: HOST
 * copy of the first 16 words of the blob.  workspace: sol_karman3d_step_workspace_bytes(cfg) bytes of DEVICE scratch.
 * saved_vy/vx/vz (all three, or all NULL): receive the post-diffusion + BC velocity, the only state the adjoint needs.
 * Outputs must not alias inputs. */
size_t sol_karman3d_step_workspace_bytes(const sol_karman3d_cfg* cfg);
int sol_karman3d_step_fwd(const sol_karman3d_cfg* cfg, void* stream,
                          const float* d_in, const float* vy_in, const float* vx_in, const float* vz_in,
                          const float* re, const float* active, const float* inflow,
                          const float* velBCy, const float* velBCyMask, int64_t bc_batch_stride,
                          float* d_out, float* vy_out, float* vx_out, float* vz_out,
                          float* saved_vy, float* saved_vx, float* saved_vz,
                          float* feat_out, const float* feat_scale, const int32_t* direct_header_host,
                          void* workspace, size_t workspace_bytes);
/* Adjoint of the step w.r.t. its input velocity (the density is a passive tracer: buoyancy_factor = 0, karman_train.py:363).
 * saved_v*: the post-diffusion + BC velocity the forward call stored (saved_vy/vx/vz, all three or NULL there).  The
 * pressure adjoint is a second solve with the same symmetric matrix and the same solver as the forward step (PhiFlow's
 * custom gradient of the CG solve).
 * The advection adjoint scatters in 64-bit fixed point (integer global atomics, power-of-two scale from max|gradient|):
 * the result is reproducible BIT FOR BIT from run to run.
 * workspace: sol_karman3d_step_bwd_workspace_bytes(cfg) bytes, 16-byte aligned. */
size_t sol_karman3d_step_bwd_workspace_bytes(const sol_karman3d_cfg* cfg);
int sol_karman3d_step_bwd(const sol_karman3d_cfg* cfg, void* stream,
                          const float* saved_vy, const float* saved_vx, const float* saved_vz,
                          const float* re, const float* active, const float* velBCyMask, int64_t bc_batch_stride,
                          const float* g_vy_out, const float* g_vx_out, const float* g_vz_out,
                          float* g_vy_in, float* g_vx_in, float* g_vz_in,
                          const int32_t* direct_header_host, void* workspace, size_t workspace_bytes);
/* Adjoint of the 3-D step's marker DENSITY (csrc/karman3d_density_bwd.hip; Y, X, Z >= 8, even face count, B <= 65535): the 3-D twin of
 * sol_karman_density_bwd, a separate set of launches (no pressure solve) that a caller adds when its loss looks at the density.  It needs
 * the step's input density d_in [B,Y,X,Z], the saved post-diffusion velocity of the forward step and g_d_out [B,Y,X,Z]; `inflow` [Y,X,Z]
 * is read only with cfg.inflow_before (the advected field is then d_in + inflow) and may be NULL otherwise.  Per cell, c = saved velocity,
 * g = g_d_out there: the centre velocity is the mean of the two faces per axis, o = -u dt/dx, f = floor(o), w = o - f;
 *     g_d_in[cell + f + corner] += w(corner) g   inside the grid (the zero ghost ring takes nothing)
 *     gU_a[cell] = -dt/dx g d(sample)/d(offset_a)   for the three axes, with the trilinear slopes of the gathered field
 *   then g_c = the cell-to-face transpose of gU (a face takes half of each adjacent cell, out-of-range cells zero) and
 *     g_vy_in = (I + alpha L^T)((1 - velBCyMask) g_cy),  g_vx_in = (I + alpha L^T) g_cx,  g_vz_in = (I + alpha L^T) g_cz,  alpha = dt res^2 / re[b]
 * with the replicate-padded 7-point Laplacian.  The scatter into g_d_in is 64-bit fixed point (order independent: results are
 * bit-reproducible; LDS window per tile of 4 x 4 columns, option k3d_dens_adj_tile), scaled by max|g_d_out| of the simulation; a non-finite
 * g_d_out makes EVERY gradient of that simulation NaN.  g_d_in is written.  accumulate = 0: g_v*_in are written; accumulate = 1: the
 * density's part is ADDED onto them (the velocity adjoint wrote there first; one fp32 add per face, deterministic).  Outputs must not alias
 * inputs or each other.  Kernel launches only: capturable.  `workspace`: DEVICE scratch of sol_karman3d_density_bwd_workspace_bytes(cfg)
 * bytes, 16-byte aligned. */
size_t sol_karman3d_density_bwd_workspace_bytes(const sol_karman3d_cfg* cfg);
int sol_karman3d_density_bwd(const sol_karman3d_cfg* cfg, void* stream,
                             const float* d_in, const float* inflow, const float* saved_vy, const float* saved_vx, const float* saved_vz,
                             const float* re, const float* velBCyMask, int64_t bc_batch_stride,
                             const float* g_d_out, float* g_d_in, float* g_vy_in, float* g_vx_in, float* g_vz_in, int accumulate,
                             void* workspace, size_t workspace_bytes);
/* Gradient of the 3-D step with respect to the REYNOLDS NUMBER (csrc/karman3d_re_bwd.hip), as the 2-D _re forms: with g' the cotangent of
 * u = v_in + alpha L v_in -- the velocity adjoint's g_c ((1 - velBCyMask) g_c on v_y), the density adjoint's cell-to-face transpose of gU --
 *     g_re[b] = -(dt res^2 / re[b]^2) * sum over the faces of v_y, v_x and v_z of  g'_e (L v_in)_e
 * The _re forms take every argument of the plain call and, after `workspace_bytes`, the step's INPUT velocity vy_in / vx_in / vz_in (not
 * the saved post-diffusion one), g_re [B] and accumulate_re (0: g_re is written; 1: added onto with one fp32 add).  They issue the plain
 * call's launches (the other gradients are the plain call's bits) and two more: fp32 terms, fp64 products and sums in a fixed order whose
 * workgroup count depends on the grid alone, no floating-point atomics.  A non-finite cotangent of simulation b makes g_re[b] NaN.  The
 * workspace is the plain call's plus the partial sums.  v*_in / g_re must not alias an output / an input.  Capturable. */
size_t sol_karman3d_step_bwd_re_workspace_bytes(const sol_karman3d_cfg* cfg);
int sol_karman3d_step_bwd_re(const sol_karman3d_cfg* cfg, void* stream,
                             const float* saved_vy, const float* saved_vx, const float* saved_vz,
                             const float* re, const float* active, const float* velBCyMask, int64_t bc_batch_stride,
                             const float* g_vy_out, const float* g_vx_out, const float* g_vz_out,
                             float* g_vy_in, float* g_vx_in, float* g_vz_in,
                             const int32_t* direct_header_host, void* workspace, size_t workspace_bytes,
                             const float* vy_in, const float* vx_in, const float* vz_in, float* g_re, int accumulate_re);
size_t sol_karman3d_density_bwd_re_workspace_bytes(const sol_karman3d_cfg* cfg);
int sol_karman3d_density_bwd_re(const sol_karman3d_cfg* cfg, void* stream,
                                const float* d_in, const float* inflow, const float* saved_vy, const float* saved_vx, const float* saved_vz,
                                const float* re, const float* velBCyMask, int64_t bc_batch_stride,
                                const float* g_d_out, float* g_d_in, float* g_vy_in, float* g_vx_in, float* g_vz_in, int accumulate,
                                void* workspace, size_t workspace_bytes,
                                const float* vy_in, const float* vx_in, const float* vz_in, float* g_re, int accumulate_re);
/* BUOYANCY on the karman-3d step (csrc/karman3d_buoyancy.hip): the definition of "BUOYANCY on the large-grid step" above with a third axis.
 * F = (fy, fx, fz) is a force per unit density (PhiFlow's -gravity * buoyancy_factor with Gravity() = -9.81 along y gives
 * F = (9.81 beta, 0, 0)); it travels as three floats, sol_karman3d_cfg is unchanged.  With c the post-diffusion velocity, one step is
 *     d_out = SL(d_in [+ inflow], c) [+ inflow dt]                                                                  (unchanged)
 *     a_y[jf,i,k] = mask_y * ( SL_y(c) + dt F_y * (dz(jf-1,i,k) + dz(jf,i,k)) / 2 )   jf = 0..Y     (a_x, a_z likewise along their axis)
 *     dz = d_out inside the grid, 0 outside (the zero ghost ring the density's advection uses)
 *     v_out = a - mask * grad( solve(div a) )                                                                       (unchanged)
 * The force acts on the step's OUTPUT density, the inflow already in it (advect, effects, buoyancy, projection: PhiFlow 1.5.1's order as
 * recalled, unpinned -- DESIGN.md sections 4.7 and 4.8).  fp32 spelling of a face: fl(v + fl(fl(dt*F) * fl(0.5f * (d0 + d1)))) * mask, no
 * contraction; fl(dt*F) is formed on the host.  A component whose force is zero is not touched; F = (0, 0, 0) issues the plain call's
 * launches and gives its bits.  One extra streaming launch (k3_buoyancy) between the advection and the divergence, for the direct and the
 * CG solve, both advection kernels and both inflow orders alike.
 *   sol_karman3d_step_fwd_buoy: every argument of sol_karman3d_step_fwd, then fy, fx, fz.  A non-zero force needs d_in, inflow and d_out;
 *     saved_* (training) and feat_out (roll-out) as in the plain call; same workspace.
 * Adjoint.  With g_a the cotangent of a that the velocity adjoint forms (k3b_gva; it carries the face mask),
 *     g_dsum[j,i,k] = g_d_out[j,i,k] + dt F_y (g_ay[j,i,k] + g_ay[j+1,i,k]) / 2 + dt F_x (g_ax[j,i,k] + g_ax[j,i+1,k]) / 2
 *                                    + dt F_z (g_az[j,i,k] + g_az[j,i,k+1]) / 2
 * and then the two existing adjoints, unchanged: the velocity adjoint's scatter and diffusion adjoint on g_a, the density adjoint on g_dsum.
 *   sol_karman3d_step_bwd_buoy / _buoy_re: every argument of sol_karman3d_step_bwd / _re, then fy, fx, fz, g_d_out [B,Y,X,Z] (the cotangent
 *     of the step's output density; NULL = zero) and g_dsum [B,Y,X,Z] (written).  They issue the plain call's launches (g_v*_in, g_re are the
 *     plain call's bits) and one more (k3b_buoyancy_adj: a gather, no atomics, fixed order, bit-reproducible); same workspace as the plain
 *     call.  The caller then runs sol_karman3d_density_bwd(_re) with g_dsum as its g_d_out and accumulate = 1.  A non-finite g_a of a
 *     simulation makes ALL of that simulation's g_dsum NaN, so the density adjoint poisons g_d_in and, through the accumulation, every other
 *     gradient of the simulation.  g_dsum must not alias another argument.
 *   sol_karman3d_buoyancy_add / _add_bwd: the term alone and its exact transpose, any Y, X, Z >= 1, for tests and callers that compose by
 *     hand: vy, vx, vz (in place) = (v + f * face average of d) * mask with f = (fy_dt, fx_dt, fz_dt) = dt F;  g_dsum = g_d_out (NULL =
 *     zero) + the transpose applied to (mask g_vy, mask g_vx, mask g_vz).
 * None of these synchronises, allocates or reads anything on the host: capturable. */
int sol_karman3d_step_fwd_buoy(const sol_karman3d_cfg* cfg, void* stream,
                               const float* d_in, const float* vy_in, const float* vx_in, const float* vz_in,
                               const float* re, const float* active, const float* inflow,
                               const float* velBCy, const float* velBCyMask, int64_t bc_batch_stride,
                               float* d_out, float* vy_out, float* vx_out, float* vz_out,
                               float* saved_vy, float* saved_vx, float* saved_vz,
                               float* feat_out, const float* feat_scale, const int32_t* direct_header_host,
                               void* workspace, size_t workspace_bytes, float fy, float fx, float fz);
int sol_karman3d_step_bwd_buoy(const sol_karman3d_cfg* cfg, void* stream,
                               const float* saved_vy, const float* saved_vx, const float* saved_vz,
                               const float* re, const float* active, const float* velBCyMask, int64_t bc_batch_stride,
                               const float* g_vy_out, const float* g_vx_out, const float* g_vz_out,
                               float* g_vy_in, float* g_vx_in, float* g_vz_in,
                               const int32_t* direct_header_host, void* workspace, size_t workspace_bytes,
                               float fy, float fx, float fz, const float* g_d_out, float* g_dsum);
int sol_karman3d_step_bwd_buoy_re(const sol_karman3d_cfg* cfg, void* stream,
                                  const float* saved_vy, const float* saved_vx, const float* saved_vz,
                                  const float* re, const float* active, const float* velBCyMask, int64_t bc_batch_stride,
                                  const float* g_vy_out, const float* g_vx_out, const float* g_vz_out,
                                  float* g_vy_in, float* g_vx_in, float* g_vz_in,
                                  const int32_t* direct_header_host, void* workspace, size_t workspace_bytes,
                                  const float* vy_in, const float* vx_in, const float* vz_in, float* g_re, int accumulate_re,
                                  float fy, float fx, float fz, const float* g_d_out, float* g_dsum);
int sol_karman3d_buoyancy_add(void* stream, int32_t B, int32_t Y, int32_t X, int32_t Z, const float* active, const float* d,
                              float fy_dt, float fx_dt, float fz_dt, float* vy, float* vx, float* vz);
int sol_karman3d_buoyancy_add_bwd(void* stream, int32_t B, int32_t Y, int32_t X, int32_t Z, const float* active,
                                  const float* g_vy, const float* g_vx, const float* g_vz, float fy_dt, float fx_dt, float fz_dt,
                                  const float* g_d_out, float* g_dsum);
/* DIFFUSION SUBSTEPS of the karman-3d step (csrc/karman3d_diffuse_sub.hip; diffusion_substeps = n on the Python surface): the definition
 * of "DIFFUSION SUBSTEPS" above with a third axis.  The single stencil v += alpha Lap(v), alpha = dt res^2 / Re (k3_diffuse), is a convex
 * combination only while alpha <= 1/6.  With M = I + (alpha / n) L, L the 7-point Laplacian with replicate padding on each of the three
 * face grids [Y+1,X,Z], [Y,X+1,Z], [Y,X,Z+1],
 *     step_n(d, v; alpha) = step_1(d, M^(n-1) v; alpha / n)
 * -- n substeps of alpha / n, the boundary blend once, after the last one; the density is not diffused.  No existing kernel, entry point
 * or struct changes: the caller computes M^(n-1) v with the entry point below and runs the existing step on a copy of the cfg whose res
 * is float32(res / sqrt(n)) (res enters every 3-D kernel through dt * res * res alone); the entry point forms its coefficient from the cfg
 * it is given by the step's own expression, (dt * res * res) / re[b].  re itself is not scaled: the fused feature output keeps carrying
 * the true Reynolds number.  Adjoint: L is symmetric on every face grid, so the existing adjoints on the scaled cfg yield the cotangent of
 * M^(n-1) v and the same entry point applied to it yields the cotangent of v.  Gradient in re: the existing _re reductions on the scaled
 * cfg, given M^(n-1) v as their input velocity, yield 1/n of the gradient: the caller multiplies by n.
 *   sol_karman3d_diffuse_sub: v*_out = (I + a_b L)^m v*_in, a_b = cfg.dt * cfg.res^2 / re[b], m in [1, 4096]; of the cfg only B, Y, X, Z,
 *     dt and res are read; Y >= 16, X, Z >= 8, B <= 65535.  chunk: substeps per launch, 1 .. sol_karman3d_diffuse_sub_max() (0 = that
 *     maximum); a launch covers the three components and the batch and runs its substeps in LDS on tiles with a halo (temporal blocking).
 *     Every substep is fmaf(a_b, lap, c) with lap summed in the step's order, so the result does not depend on chunk: m launches of one
 *     substep and one launch of m substeps give equal bits.  More than one launch ping-pongs through `workspace`
 *     (sol_karman3d_diffuse_sub_workspace_bytes(cfg, m, chunk): two velocity triples; 0 bytes and NULL for a single launch).  The outputs
 *     must not alias the inputs or each other.  Does not synchronise, allocate or read device memory on the host: capturable. */
int32_t sol_karman3d_diffuse_sub_max(void);
size_t sol_karman3d_diffuse_sub_workspace_bytes(const sol_karman3d_cfg* cfg, int32_t m, int32_t chunk);
int sol_karman3d_diffuse_sub(const sol_karman3d_cfg* cfg, void* stream,
                             const float* vy_in, const float* vx_in, const float* vz_in, const float* re,
                             float* vy_out, float* vx_out, float* vz_out,
                             int32_t m, int32_t chunk, void* workspace, size_t workspace_bytes);
/* MACCORMACK ADVECTION on the karman-3d step (csrc/karman3d_maccormack.hip; advection = "mac_cormack" on the Python surface): the
 * definition of "MACCORMACK ADVECTION on the large-grid step" above with a third axis.  c = (sv_y, sv_x, sv_z); f is c_y, c_x or c_z on its
 * own faces or the density on cells (inflow added first when cfg.inflow_before); u is c at the array's sample point by exactly the
 * expressions of k3_advect (own component stored, the others averaged over four faces with clamped indices, cells as two-face means);
 * S_g is the TRILINEAR sample in the array's own mode; lo, hi = min, max of the EIGHT values the first gather read.  Tie rule (inclusive,
 * no tolerance), NaN rule (a NaN cor reverts to h) and the fp32 spelling cor = fl(h + fl(fl(0.5f s) * fl(f - b))), contraction off, carry
 * over; h is ONE spelled-out trilinear expression (z pairs first, then x, then y) wherever it is evaluated.  Parity with PhiFlow is
 * unpinned, as for 2-D.  Forward: two launches (k3m_hat: h of the four arrays to the workspace; k3m_out: b, limiter, mask / inflow) in
 * place of the advection launch.  Gradient: every decision frozen as the forward took it; h recomputed from the saved c (nothing new is
 * saved).  Stage A (k3m_vel_adj / k3m_den_adj, global int64 atomics): g_f += (s/2) kept g; g_b = -(s/2) kept g scattered through the eight
 * corners of the gather at x + u dt into accumulators G_h; g_u += (dt/dx) g_b dS_h/d(offset), a face's onto the nine samples that formed
 * u, a cell's into gU.  Stage B: the EXISTING semi-Lagrangian adjoint kernels (k3b_advect_adj*, k3d_advect_adj*, their LDS-window options
 * included) on g_h = g + G_h.  Every scattered sum is 64-bit fixed point with the one scale of its cotangent: bit-reproducible; a
 * non-finite cotangent poisons its own simulation only.
 *   sol_karman3d_step_fwd_adv: every argument of sol_karman3d_step_fwd_buoy, then advection (0 semi-Lagrangian: that form's launches, bits
 *     and workspace size; 1 MacCormack) and correction_strength (checked to lie in [0, 1] for either).  A zero force is the unbuoyant
 *     step.  Workspace: sol_karman3d_step_fwd_adv_workspace_bytes(cfg, advection).
 *   sol_karman3d_step_bwd_adv / _adv_re: every argument of the _buoy / _buoy_re form, then the same two; with a zero force g_d_out and
 *     g_dsum may be NULL.  sol_karman3d_density_bwd_adv / _adv_re: every argument of the plain / _re form, then the same two.  Workspaces:
 *     sol_karman3d_step_bwd_adv_workspace_bytes / sol_karman3d_density_bwd_adv_workspace_bytes(cfg, with_re, advection).
 *   sol_karman3d_advect / sol_karman3d_advect_bwd: the stage alone and its transpose, any Y, X, Z >= 8 (odd extents included), for tests
 *     and callers that compose by hand: (d_in, sv_y, sv_x, sv_z) -> (d_out, a_y, a_x, a_z) masked / with inflow as above; cotangents of
 *     those -> (g_d_in, g_sv_y, g_sv_x, g_sv_z).  advection = 0 is the plain stage.  tile_window: 1 = the semi-Lagrangian scatters through
 *     their LDS windows where the grid admits them (velocity: Z <= 64), 0 = global atomics only; equal bits.  Workspaces:
 *     sol_karman3d_advect_workspace_bytes(cfg, advection) (0 bytes and NULL for advection = 0), sol_karman3d_advect_bwd_workspace_bytes(cfg).
 * None of these synchronises, allocates or reads anything on the host: capturable. */
size_t sol_karman3d_advect_workspace_bytes(const sol_karman3d_cfg* cfg, int32_t advection);
int sol_karman3d_advect(const sol_karman3d_cfg* cfg, void* stream, const float* d_in, const float* svy, const float* svx, const float* svz,
                        const float* active, const float* inflow, int32_t advection, float correction_strength,
                        float* d_out, float* ay, float* ax, float* az, void* workspace, size_t workspace_bytes);
size_t sol_karman3d_advect_bwd_workspace_bytes(const sol_karman3d_cfg* cfg);
int sol_karman3d_advect_bwd(const sol_karman3d_cfg* cfg, void* stream, const float* d_in, const float* svy, const float* svx, const float* svz,
                            const float* active, const float* inflow, int32_t advection, float correction_strength,
                            const float* g_d_out, const float* g_ay, const float* g_ax, const float* g_az,
                            float* g_d_in, float* g_svy, float* g_svx, float* g_svz, int32_t tile_window, void* workspace, size_t workspace_bytes);
size_t sol_karman3d_step_fwd_adv_workspace_bytes(const sol_karman3d_cfg* cfg, int32_t advection);
int sol_karman3d_step_fwd_adv(const sol_karman3d_cfg* cfg, void* stream,
                              const float* d_in, const float* vy_in, const float* vx_in, const float* vz_in,
                              const float* re, const float* active, const float* inflow,
                              const float* velBCy, const float* velBCyMask, int64_t bc_batch_stride,
                              float* d_out, float* vy_out, float* vx_out, float* vz_out,
                              float* saved_vy, float* saved_vx, float* saved_vz,
                              float* feat_out, const float* feat_scale, const int32_t* direct_header_host,
                              void* workspace, size_t workspace_bytes, float fy, float fx, float fz,
                              int32_t advection, float correction_strength);
size_t sol_karman3d_step_bwd_adv_workspace_bytes(const sol_karman3d_cfg* cfg, int32_t with_re, int32_t advection);
int sol_karman3d_step_bwd_adv(const sol_karman3d_cfg* cfg, void* stream,
                              const float* saved_vy, const float* saved_vx, const float* saved_vz,
                              const float* re, const float* active, const float* velBCyMask, int64_t bc_batch_stride,
                              const float* g_vy_out, const float* g_vx_out, const float* g_vz_out,
                              float* g_vy_in, float* g_vx_in, float* g_vz_in,
                              const int32_t* direct_header_host, void* workspace, size_t workspace_bytes,
                              float fy, float fx, float fz, const float* g_d_out, float* g_dsum,
                              int32_t advection, float correction_strength);
int sol_karman3d_step_bwd_adv_re(const sol_karman3d_cfg* cfg, void* stream,
                                 const float* saved_vy, const float* saved_vx, const float* saved_vz,
                                 const float* re, const float* active, const float* velBCyMask, int64_t bc_batch_stride,
                                 const float* g_vy_out, const float* g_vx_out, const float* g_vz_out,
                                 float* g_vy_in, float* g_vx_in, float* g_vz_in,
                                 const int32_t* direct_header_host, void* workspace, size_t workspace_bytes,
                                 const float* vy_in, const float* vx_in, const float* vz_in, float* g_re, int accumulate_re,
                                 float fy, float fx, float fz, const float* g_d_out, float* g_dsum,
                                 int32_t advection, float correction_strength);
size_t sol_karman3d_density_bwd_adv_workspace_bytes(const sol_karman3d_cfg* cfg, int32_t with_re, int32_t advection);
int sol_karman3d_density_bwd_adv(const sol_karman3d_cfg* cfg, void* stream,
                                 const float* d_in, const float* inflow, const float* saved_vy, const float* saved_vx, const float* saved_vz,
                                 const float* re, const float* velBCyMask, int64_t bc_batch_stride,
                                 const float* g_d_out, float* g_d_in, float* g_vy_in, float* g_vx_in, float* g_vz_in, int accumulate,
                                 void* workspace, size_t workspace_bytes, int32_t advection, float correction_strength);
int sol_karman3d_density_bwd_adv_re(const sol_karman3d_cfg* cfg, void* stream,
                                    const float* d_in, const float* inflow, const float* saved_vy, const float* saved_vx, const float* saved_vz,
                                    const float* re, const float* velBCyMask, int64_t bc_batch_stride,
                                    const float* g_d_out, float* g_d_in, float* g_vy_in, float* g_vx_in, float* g_vz_in, int accumulate,
                                    void* workspace, size_t workspace_bytes,
                                    const float* vy_in, const float* vx_in, const float* vz_in, float* g_re, int accumulate_re,
                                    int32_t advection, float correction_strength);
/* PERIODIC SPANWISE BOUNDARIES on the karman-3d step (csrc/karman3d_periodic.hip; Scene3D(boundaries="periodic-z") on the Python
 * surface): the text of "PERIODIC BOUNDARIES" above with z as the axis.  A direct blob built periodic (precond3d.periodic_solver_blob3d,
 * layout "FD33"; precond3d.extruded_solver_blob3d(periodic=True), layout "FD3E") carries the axes in header word 6: SOL_K3_PERIODIC_Z = 8;
 * 2 and 4 are reserved for y and x and refused.  sol_karman3d_cfg is unchanged; with the word clear every entry issues the launches it
 * always did.
 *   Array shapes do not change: v_z [B,Y,X,Z+1], and plane Z is a DUPLICATE of plane 0.  It is never read on input (a NaN there changes
 *   nothing) and is written equal to plane 0, bit for bit, in vz_out and saved_vz; the adjoint first adds the cotangent of the output
 *   duplicate plane onto plane 0's (one fp32 add) and returns g_vz_in[..., Z] = 0 exactly.
 *   Every z index wraps modulo the Z unique planes (a true modulo: a departure point several periods away lands on its plane): the
 *   Laplacian, the four-face averages of the advecting velocity, the trilinear gathers of the three components and of the density, the
 *   accessible mask, the divergence and the pressure gradient along z, which has no boundary face (grad_pad is not read there).  floorf
 *   and the weights are the open kernels'; y and x keep clamp, velBC blend, grad_pad and the zero ghost ring.
 *   The pressure solve runs the open step's launches on the blob's tables (Q_z = the Hartley matrix, eigenvalues 2 - 2 cos(2 pi m / Z)).
 *   The z-constant mode is held down by the open y and x axes: the system is non-singular.
 * sol_karman3d_step_fwd, sol_karman3d_step_bwd and sol_karman3d_pressure_solve dispatch on the word.  On a periodic blob
 * pressure_solver = 1 (CG) and the _buoy, _adv and _re forms return SOL_ERR_ARG with a message.
 * sol_karman3d_seam_sync: v_z[..., Z] = v_z[..., 0] (after a correction that leaves the duplicate plane behind).  sol_karman3d_seam_fold,
 * its adjoint: g[..., 0] += g[..., Z], then g[..., Z] = 0.  periodic_bits = 0: nothing is launched; 2 or 4: SOL_ERR_ARG. */
#define SOL_K3_PERIODIC_Z 8
int sol_karman3d_seam_sync(void* stream, float* vz, int32_t B, int32_t Y, int32_t X, int32_t Z, int32_t periodic_bits);
int sol_karman3d_seam_fold(void* stream, float* g_vz, int32_t B, int32_t Y, int32_t X, int32_t Z, int32_t periodic_bits);
/* The step's pressure solve alone: M p = rhs with M = -A for the scene's `active` mask (the solver cfg->pressure_solver selects;
 * the CG solve reports to cfg->cg_info).  rhs, p [B,Y,X,Z] (rhs is read only); workspace: sol_karman3d_step_workspace_bytes(cfg). */
int sol_karman3d_pressure_solve(const sol_karman3d_cfg* cfg, void* stream, const float* active, const float* rhs, float* p,
                                const int32_t* direct_header_host, void* workspace, size_t workspace_bytes);
/* velocity += s_c * out[..., c] for the three components (to_staggered + add, karman_train.py:88-90, 424-426):
 * out [B,Y,X,Z,cout], cout >= 3; the last face of each component's own axis receives no correction. */
int sol_karman3d_correct(void* stream, const float* out, int32_t cout, float s0, float s1, float s2,
                         float* vy, float* vx, float* vz, int32_t B, int32_t Y, int32_t X, int32_t Z);
/* The reverse-sweep counterparts (one launch each between the CNN's reverse sweep and sol_karman3d_step_bwd):
 * sol_karman3d_correct_bwd: g_v* += gin_v* on every face (the adjoint of the NEXT unrolled step w.r.t. its input; all three NULL: nothing to add) and
 *   d_out4 [B,Y,X,Z,4] = (s0 g_vy, s1 g_vx, s2 g_vz, 0) at the low faces of every cell -- the adjoint of sol_karman3d_correct, zero padded to the four
 *   channels the thin-layer launches read;
 * sol_karman3d_feature_bwd: g_v*[low faces] += f_c dx4[..., c] -- the adjoint of the scaled feature output of sol_karman3d_step_fwd (f_c = 1 / std_in). */
int sol_karman3d_correct_bwd(void* stream, float* g_vy, float* g_vx, float* g_vz, const float* gin_vy, const float* gin_vx, const float* gin_vz,
                             float s0, float s1, float s2, float* d_out4, int32_t B, int32_t Y, int32_t X, int32_t Z);
int sol_karman3d_feature_bwd(void* stream, const float* dx4, float f0, float f1, float f2, float* g_vy, float* g_vx, float* g_vz,
                             int32_t B, int32_t Y, int32_t X, int32_t Z);

/* 5 x 5 x 5 SAME convolution, NDHWC fp32 (keras.layers.Conv3D(filters, 5, padding='same') + bias / LeakyReLU / add).
 * w_dhwio [5,5,5,cin,cout] (Keras layout, D = y).  Layers with cin = 32 and cout = 32 or <= 16 on W == 64 with x_absmax given run as
 * ONE launch that keeps its accumulators over all 125 taps (conv3d_sb.hip; options k3d_conv_fused, k3d_conv_rows); everything
 * else runs as five passes of the 2-D kernels over the (H, W) planes with the running sum in y, the centre slice last (bias,
 * activation, absmax publish).  Same per-product arithmetic as sol_conv5x5 in both forms.
 * x [B,D,H,W,cin] with cin in {4 (zero padded), 32}; residual [B,D,H,W,cout] or NULL is added before the activation;
 * epilogue SOL_EPI_NONE / SOL_EPI_LRELU / SOL_EPI_DLRELU (times LeakyReLU'(act_ref), act_ref [B,D,H,W,cout]: the backward pass'
 * "data gradient (+ skip gradient) times the activation derivative" in one launch; act_ref NULL otherwise); x_absmax / y_absmax
 * as in sol_conv5x5_scaled (may be NULL).  x != y, D >= 3.
 * Backward-data is the same entry point on weights packed with mode SOL_CONV_BWD_DATA (cin = channels of dy = the forward
 * layer's cout, cout = channels of dx = the forward layer's cin; w_dhwio is the FORWARD kernel): dx = conv3d(dy, flip(w)^T).
 * The weight gradient: sol_conv3d_bwd_weight below. */
size_t sol_conv3d_packed_floats(int32_t cin, int32_t cout);
int sol_conv3d_pack(void* stream, const float* w_dhwio, int32_t cin, int32_t cout, int32_t mode, float* packed);
int sol_conv3d(void* stream, const float* x, const float* packed, const float* bias, const float* residual, const float* act_ref, float* y,
               int32_t B, int32_t D, int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t epilogue, float slope,
               const uint32_t* x_absmax, uint32_t* y_absmax);

/* Thin-INPUT Conv3D layers (<= 4 -> 32 channels: the first layer of model_mars_moon in 3-D, karman_train.py:103 generalised, and the
 * output layer's data gradient) with the depth taps packed into the channel axis: x'[..][4 s + c] = x[d + s - 2][..][c] is gathered
 * into ws and the layer runs as ONE 2-D 32 -> 32 convolution over the (H, W) planes (25 taps of K = 32 on the 16-bit matrix pipe
 * instead of 125 taps of K = 4 on the fp32 one; per-product arithmetic of sol_conv5x5 with 32 input channels, option conv_precision).
 * x [B,D,H,W,4] (zero padded from cin channels), y [B,D,H,W,32]; packed: sol_conv3d_thin_packed_floats() floats from
 * sol_conv3d_thin_pack (w_dhwio = the FORWARD kernel: [5,5,5,cin,32] for SOL_CONV_FWD, [5,5,5,32,cin] for SOL_CONV_BWD_DATA; cin = the
 * channels the convolution that is RUN reads, 1..4); ws: sol_conv3d_thin_ws_floats() floats of scratch (the gathered tensor + the
 * absmax slots of x, which this call computes itself); bias / act_ref / epilogue / y_absmax as in sol_conv3d. */
size_t sol_conv3d_thin_packed_floats(void);
size_t sol_conv3d_thin_ws_floats(int32_t B, int32_t D, int32_t H, int32_t W);
int sol_conv3d_thin_pack(void* stream, const float* w_dhwio, int32_t cin, int32_t mode, float* packed);
int sol_conv3d_thin(void* stream, const float* x, const float* packed, const float* bias, const float* act_ref, float* y, float* ws,
                    int32_t B, int32_t D, int32_t H, int32_t W, int32_t epilogue, float slope, uint32_t* y_absmax);

/* Thin-OUTPUT Conv3D layers (32 -> cout <= 4 channels: the network's output layer, karman_train.py:137 generalised, and the first layer's data
 * gradient) with the depth taps packed into the OUTPUT channel axis: ONE 2-D 32 -> 32 convolution y'[q][..][4 s + c] over the (H, W) planes into
 * ws, then y[d][..][c] = bias[c] + sum_s y'[d + s - 2][..][4 s + c].  x [B,D,H,W,32] with its absmax slots (or NULL: computed here), y [B,D,H,W,cout];
 * packed: sol_conv3d_thin_packed_floats() floats from sol_conv3d_thin_out_pack (w_dhwio = the FORWARD kernel: [5,5,5,32,cout] for SOL_CONV_FWD,
 * [5,5,5,cout,32] for SOL_CONV_BWD_DATA; cout = the channels the convolution that is RUN writes); ws: sol_conv3d_thin_ws_floats(); no activation. */
int sol_conv3d_thin_out_pack(void* stream, const float* w_dhwio, int32_t cout, int32_t mode, float* packed);
int sol_conv3d_thin_out(void* stream, const float* x, const float* packed, const float* bias, float* y, float* ws,
                        int32_t B, int32_t D, int32_t H, int32_t W, int32_t cout, const uint32_t* x_absmax);

/* Weight gradient of a thin-input layer in the same packing: ONE pass of the 2-D 32 -> 32 fp16 three-product weight-gradient kernel over
 * the gathered tensor instead of five passes of the thin fp32 kernel.  x [B,D,H,W,4], dz [B,D,H,W,32], W == 64; dz_absmax: the slots the
 * producer of dz published, or NULL (computed here); ws: sol_conv3d_thin_ws_floats(); partial: sol_conv3d_thin_bwd_weight_ws_floats();
 * dw_dhwio [5,5,5,cin_real,32], db [32] are written when do_reduce is set; accumulate_partial / do_reduce as in sol_conv3d_bwd_weight_acc. */
size_t sol_conv3d_thin_bwd_weight_ws_floats(int32_t B, int32_t D, int32_t H, int32_t W);
int sol_conv3d_thin_bwd_weight_acc(void* stream, const float* x, const float* dz, const uint32_t* dz_absmax, float* ws, float* partial,
                                   float* dw_dhwio, float* db, int32_t B, int32_t D, int32_t H, int32_t W, int32_t cin_real,
                                   int32_t accumulate_partial, int32_t do_reduce);

/* ... and of a thin-OUTPUT layer (32 -> cout_real <= 4: the network's last layer): dz4 [B,D,H,W,4] (zero padded) is gathered with the opposite
 * depth offsets and dW [5,5,5,32,cout_real], db [cout_real] come from ONE pass of the 32 -> 32 kernel (the five-pass form pads dz to 32
 * channels and runs five full 32 -> 32 passes).  x [B,D,H,W,32] with x_absmax (or NULL: computed here); ws / partial as above. */
int sol_conv3d_thin_out_bwd_weight_acc(void* stream, const float* x, const uint32_t* x_absmax, const float* dz4, float* ws, float* partial,
                                       float* dw_dhwio, float* db, int32_t B, int32_t D, int32_t H, int32_t W, int32_t cout_real,
                                       int32_t accumulate_partial, int32_t do_reduce);

/* Conv3D weight gradient: dw_dhwio [5,5,5,cin_real,cout] = sum_px x[px + tap] * dz[px], db [cout] = sum_px dz[px]; five passes
 * of the 2-D weight-gradient kernels over the shifted plane ranges.  x [B,D,H,W,cin] (cin in {4, 32}, zero padded from
 * cin_real), dz [B,D,H,W,cout] (cout in {2, 32}); x_absmax / dz_absmax (or NULL): absmax slots of the two tensors -> fp16
 * three-product kernels for the 32 -> 32 case.  partial: sol_conv3d_bwd_weight_ws_floats() floats of scratch; db_scratch: 5 * cout floats. */
size_t sol_conv3d_bwd_weight_ws_floats(int32_t B, int32_t D, int32_t H, int32_t W, int32_t cin, int32_t cout);
int sol_conv3d_bwd_weight(void* stream, const float* x, const float* dz, const uint32_t* x_absmax, const uint32_t* dz_absmax,
                          float* partial, float* dw_dhwio, float* db, float* db_scratch,
                          int32_t B, int32_t D, int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t cin_real, int32_t cout_real);
/* The same for a trainer that unrolls n steps (karman_train.py:397-457: one gradient per layer over ALL unrolled steps): called n times
 * per layer on ONE partial buffer -- accumulate_partial = 0 on the first call, 1 afterwards -- with do_reduce = 1 on the last call only;
 * dw / db are written when do_reduce is set and then hold the sum over the n calls. */
int sol_conv3d_bwd_weight_acc(void* stream, const float* x, const float* dz, const uint32_t* x_absmax, const uint32_t* dz_absmax,
                              float* partial, float* dw_dhwio, float* db, float* db_scratch,
                              int32_t B, int32_t D, int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t cin_real, int32_t cout_real,
                              int32_t accumulate_partial, int32_t do_reduce);

/* CIRCULAR PADDING, KARMAN-3D (csrc/conv3d_circular.hip): circular z padding of the Conv3D network on a z-periodic scene.  The network's
 * tensors are [B,Y,X,Z,C] with z as the pixel axis of a row, and a row of Z + 4 pixels has no legal width; so the network runs on the
 * TRANSPOSED volume [B,Y,HB,X,C] -- depth y, image rows z, pixels x -- with every layer's kernel axes 1 and 2 swapped by the caller:
 *   rows [2, 2 + Z)            the Z planes (row 2 + z = plane z, transposed);
 *   rows 0, 1, Z + 2, Z + 3    the circular halo (row r = plane (r - 2) mod Z);
 *   rows [Z + 4, HB)           pad rows: HB >= Z + 4 is Z + 4 rounded up to what the convolutions ask of a row count (a multiple of
 *                              64 / X when X < 64).
 * sol_conv3d / _thin / _thin_out / the weight gradients run at (B, D = Y, H = HB, W = X) as they are, zero padding beyond the buffer.
 * What a launch writes into halo and pad rows is wrong and is replaced by sol_conv3d_halo before the next consumer; its valid rows are
 * the circular convolution, because their stencils read rows [0, Z + 4) only: wrapped copies, never pad rows.  The absmax slots a launch
 * publishes also cover its halo and pad rows before the refresh: an upper bound of the true maximum.
 *   sol_conv3d_circ_pack    src [B,Y,X,Z,C] -> dst [B,Y,HB,X,C], C == 4: every (X, Z) plane transposed into rows [2, Z + 2); halo rows
 *                           wrapped (mode 0) or zero (mode 1); pad rows zero.
 *   sol_conv3d_circ_unpack  src [B,Y,HB,X,C] -> dst [B,Y,X,Z,C], C in {3, 4}: the inverse on rows [2, Z + 2).
 *   sol_conv3d_halo         buf [planes = B Y, HB, X, C] in place, C in {4, 32}: mode 0 -- halo rows = the wrapped valid rows, pad rows = 0
 *                           (every activation; a dz before its backward-data convolution: the adjoint of a circular convolution is the
 *                           circular correlation); mode 1 -- halo and pad rows = 0 (a dz before its weight gradient: only valid rows
 *                           contribute to dw and db).  Valid rows are never written.
 * Each is ONE launch through an LDS tile (pack, unpack: both global sides contiguous) or a plain copy (halo), vector stores, no atomics,
 * no host synchronisation: capturable.  Every element of dst (pack, unpack) is written.  SOL_ERR_ARG with a message: NULL buffer, B, Y,
 * planes, X < 1, Z < 2, HB < Z + 4, a C or mode it does not take, more than 2^31 pixels. */
int sol_conv3d_circ_pack(void* stream, const float* src, float* dst, int32_t B, int32_t Y, int32_t X, int32_t Z, int32_t HB, int32_t C, int32_t mode);
int sol_conv3d_circ_unpack(void* stream, const float* src, float* dst, int32_t B, int32_t Y, int32_t X, int32_t Z, int32_t HB, int32_t C);
int sol_conv3d_halo(void* stream, float* buf, int32_t planes, int32_t Z, int32_t HB, int32_t X, int32_t C, int32_t mode);

/* offsets (in floats) of layer l's kernel / bias inside the flat mars_moon parameter
 * vector; l in [0,12).  cin/cout may be NULL.                                            */
int sol_mars_moon_layer(int32_t l, int64_t* kernel_off, int64_t* bias_off, int32_t* cin, int32_t* cout);

#ifdef __cplusplus
}
#endif
#endif /* SOL_HIP_H */
