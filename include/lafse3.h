/*
 * lafse3.h — C ABI of the MI355X-native batched SE(3) MPC solve + gradient engine.
 *
 * Drop-in boundary for the optimal-control hot path of yanrui89/LearningAgileFlight_SE3:
 *
 *   lafse3_ocp_solve      replaces OCSys.ocSolver            quad_OC.py:104-212
 *                         (cost configured as run_quad does:  quad_policy.py:35-56, :74-77,
 *                          traversal cost quad_model.py:200-213, setTraCost quad_OC.py:98-101)
 *   lafse3_objective      replaces run_quad.objective         quad_policy.py:67-91
 *   lafse3_sol_gradient   replaces run_quad.sol_gradient      quad_policy.py:94-112
 *   lafse3_get_input      replaces run_quad.get_input         quad_policy.py:202-211
 *   lafse3_ocp_sensitivity  ocSolver + dx, du / d(p_tra, a_tra, t)  (the PDP auxiliary system, quad_OC.py:214-306)
 *   lafse3_ocp_sensitivity_ex  the same with ini_state and goal columns and the feedback gain du_0 / dx_0
 *   lafse3_ocp_sensitivity_w   the same with per-instance cost weights and the columns of the ten weights
 *   lafse3_ocp_solve_rec / lafse3_ocp_vjp   the solve that saves its optimum, and g^T dz* / dparam from it in one sweep
 *
 * Every array argument is a DEVICE pointer (HBM; e.g. a torch.cuda tensor's data_ptr()), owned by
 * the caller, row-major, contiguous.  B is the batch size.  N is params.horizon (<= LAFSE3_MAX_N).
 * The library keeps no global mutable state: all state is in the opaque context (device workspace,
 * parameters).  Calls on one context must not overlap, and a context must be used from ONE stream at a
 * time: the workspace, scratch and counters are shared by every call on it and each call runs on the
 * caller's stream (use one context per stream); distinct contexts are independent.  No entry point changes the
 * calling thread's current HIP device: work for a context bound to another device switches to it and back.
 *
 * Return codes: 0 ok; LAFSE3_EINVAL bad argument; LAFSE3_EDEVICE HIP error (message via
 * lafse3_last_error).  Per-instance solver outcome is reported in `status` (never aborts):
 *   0 solved (IPOPT tol), 1 solved to acceptable level, 2 max_iter, 3 line-search failure,
 *   4 non-finite, 5 tiny step, 6 inertia regularisation failed (in lafse3_sol_gradient's IFT mode also: the
 *   factorisation at the nominal optimum failed, so the p/a probe rewards fell back to the nominal reward),
 *   7 device error (a sol_gradient slot no solve wrote: reward NaN; lafse3_check_device reports it),
 *   8 restoration phase failed (its line search; IPOPT Restoration_Failed), 9 the restoration phase converged to
 *   a point that is not feasible for the original problem (IPOPT Infeasible_Problem_Detected).  After 8 and 9 the
 *   outputs hold the point where the restoration phase started.
 * Outputs are always written with the last iterate (the reference uses IPOPT's last iterate too).
 */
#ifndef LAFSE3_H
#define LAFSE3_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LAFSE3_NX 13
#define LAFSE3_NU 4
#define LAFSE3_MAX_N 50

#define LAFSE3_OK 0
#define LAFSE3_EINVAL (-1)
#define LAFSE3_EDEVICE (-2)

/* Problem + solver parameters.  Defaults (lafse3_default_params) equal the reference:
 * model quad_policy.py:37 + quad_model.py:37, weights quad_policy.py:38 + quad_OC.py:145,150,
 * bounds quad_policy.py:46-51, dt quad_policy.py:43, horizon quad_policy.py:17, winglen :19,
 * IPOPT 3.12 defaults for the solver options (quad_OC.py:170 sets only print options). */
typedef struct lafse3_params {
    double mass, Jx, Jy, Jz, arm_l, c_tau, grav, dt;
    double wrt, wqt, wthrust, wrf, wvf, wqf, wwf;
    double tra_w_peak, tra_w_decay, du_weight;
    double u_lb, u_ub, w_lb, w_ub;
    double wing_len, d_min;
    int32_t horizon;
    int32_t max_iter;
    double tol, acceptable_tol;
    int32_t acceptable_iter;
    double mu_init, bound_relax;
    int32_t lsq_mult_init;
    int32_t variant;          /* must be LAFSE3_VARIANT_WAVE (kept for ABI layout; LANE was removed in 0.3) */
    int32_t max_soc;          /* IPOPT max_soc (default 4): second-order corrections per line search */
    int32_t costate_option;   /* lam output of lafse3_ocp_solve: 0 = IPOPT lam_g (default, quad_OC.py:185-187),
                                 1 = PMP costates recomputed on the optimum (quad_OC.py:188-201) */
    int32_t grad_mode;        /* lafse3_sol_gradient: 0 = FD, the reference's 9 solves per sample (default,
                                 quad_policy.py:94-112); 1 = IFT: 3 solves (nominal, t -+ 0.1) and the six
                                 p/a probes R(p + 1e-3 e_i) replaced by R(xs + 1e-3 dxs_i), xs the nominal
                                 optimum and dxs_i its sensitivity to parameter i from the nominal solve's last
                                 KKT factorisation (implicit function theorem, one refinement sweep per
                                 parameter); requires u_last == NULL */
    int32_t restoration;      /* 1 (default): IPOPT's restoration phase after a failed line search (feasibility
                                 problem min rho ||p + n||_1 + eta/2 ||D_R (v - v_R)||^2, IpRestoPhase); 0: the solve
                                 ends there (status 3, or 1 at an acceptable point) as up to 0.4 */
    int32_t watchdog;         /* IPOPT watchdog_shortened_iter_trigger (default 10; 0 disables): after this many
                                 successive iterations whose line search rejected the first trial point, up to 3
                                 (watchdog_trial_iter_max) full steps are taken before the stored iterate resumes */
} lafse3_params;

/* Kernel variant: one NLP instance per 64-lane wavefront (the only one).  The value 0 (a lane-per-instance
 * variant up to 0.2) is rejected with LAFSE3_EINVAL. */
#define LAFSE3_VARIANT_WAVE 1

typedef struct lafse3_ctx lafse3_ctx;

/* Fill *p with the reference defaults.  Returns 0. */
int lafse3_default_params(lafse3_params *p);

/* Create a context bound to HIP device `device` (the caller's current device if < 0). */
int lafse3_create(lafse3_ctx **ctx, int device);
int lafse3_destroy(lafse3_ctx *ctx);
int lafse3_set_params(lafse3_ctx *ctx, const lafse3_params *p);
int lafse3_get_params(const lafse3_ctx *ctx, lafse3_params *p);

/* Pre-allocate device workspace for launches of up to `n_instances` NLP instances so that later calls
 * with at most that many instances do no allocation (required before hipGraph capture).  A solve of B
 * instances needs B instances; sol_gradient needs 9*B.  The solver kernel is persistent (one wave per
 * SIMD slot pulling instances from a queue), so the workspace held is min(n_instances, slots) slots of
 * lafse3_workspace_bytes_per_instance() bytes, slots = CUs x 4 (1024 on MI355X). */
int lafse3_reserve(lafse3_ctx *ctx, int64_t n_instances);
/* Bytes of device workspace one NLP instance uses. */
int64_t lafse3_workspace_bytes_per_instance(void);

/* A HIP stream with a hardware queue of its own (every CU enabled), for launches of several contexts that are meant
 * to run concurrently.  HIP maps ordinary streams onto a small pool of hardware queues (GPU_MAX_HW_QUEUES, 4 by
 * default) by the process's stream history, and two streams that share a queue run their kernels one after the
 * other (the configs[4] episode groups then ran at 2/3 of the rate: profiles/r05_moving_trace.log).  Not a
 * reference entry point (serving plumbing).  device < 0: the caller's current device. */
int lafse3_stream_create(int device, void **stream);
int lafse3_stream_destroy(void *stream);

/* Batched OCSys.ocSolver (quad_OC.py:104-212) with the traversal cost of quad_model.py:200-213:
 *   ini_state B x 13, goal B x 3, p_tra B x 3, a_tra B x 3 (the 'tra_ang' vector of Rd2Rp,
 *   quad_policy.py:10-13, float64), t B (traversal time, used as given), u_last B x 4 or NULL (=0).
 * Outputs (each nullable): x B x (N+1) x 13 (state_traj_opt), u B x N x 4 (control_traj_opt),
 *   lam B x N x 13 (costate_traj_opt = IPOPT lam_g), cost B (sol['f']), status B, iters B. */
int lafse3_ocp_solve(lafse3_ctx *ctx, int64_t B, const double *ini_state, const double *goal,
                     const double *p_tra, const double *a_tra, const double *t, const double *u_last,
                     double *x, double *u, double *lam, double *cost, int32_t *status, int32_t *iters,
                     void *stream);

/* lafse3_ocp_solve plus the analytic sensitivities of its solution to theta = (p_tra[0..2], a_tra[0..2], t), the
 * derivative the reference sketched as the PDP auxiliary system (quad_OC.py:214-306, commented out there).  The
 * first 14 arguments and the outputs x .. iters are lafse3_ocp_solve's, bit for bit.  Then, each nullable:
 *   dx B x 7 x (N+1) x 13 = dx_k / dtheta_q, du B x 7 x N x 4 = du_k / dtheta_q, parameter order along the axis of
 *   7 as above; sens_status B (int32): 0 ok, 1 the solve ended with status > 1, 2 the factorisation at the optimum
 *   met a wrong inertia -- after 1 and 2 that instance's dx and du are zero.  With dx == du == NULL the call is
 *   lafse3_ocp_solve (sens_status is then not written).
 * One Newton-system factorisation at the optimum z* (final mu and bound duals, delta_w = 0) and one refinement sweep
 * per parameter, on the wave that solved the instance (implicit function theorem; grad_mode 1 of
 * lafse3_sol_gradient uses the same sweeps for its six reward probes).  t is used as given; u_last is accepted and,
 * like ini_state and goal, treated as a constant, so dx at stage 0 is zero.  The derivative is that of the barrier
 * problem at the final mu: across an active-set change it is a one-sided smoothing, not a subgradient.  A solver
 * launch for lafse3_reserve, lafse3_last_kernel_ms, the counters and lafse3_check_device. */
int lafse3_ocp_sensitivity(lafse3_ctx *ctx, int64_t B, const double *ini_state, const double *goal,
                           const double *p_tra, const double *a_tra, const double *t, const double *u_last,
                           double *x, double *u, double *lam, double *cost, int32_t *status, int32_t *iters,
                           double *dx, double *du, int32_t *sens_status, void *stream);

/* lafse3_ocp_sensitivity with selectable parameter groups and the MPC feedback gain.  The columns, in this fixed
 * order and restricted to the groups selected in `groups`:
 *   LAFSE3_SENS_THETA  p_tra[0..2], a_tra[0..2], t   7 columns, lafse3_ocp_sensitivity's bit for bit
 *   LAFSE3_SENS_INI    ini_state[0..12]              13 columns; the quaternion entries are differentiated as the
 *                                                    four raw numbers the solver reads (it does not normalise them)
 *   LAFSE3_SENS_GOAL   goal[0..2]                    3 columns
 * lafse3_sens_columns gives their number P = 7 [THETA] + 13 [INI] + 3 [GOAL] (LAFSE3_EINVAL for bits outside the
 * three groups).  The first 14 arguments and the outputs x .. iters are lafse3_ocp_solve's, bit for bit.  Then, each
 * nullable:
 *   dx B x P x (N+1) x 13, du B x P x N x 4 as lafse3_ocp_sensitivity's; dx at stage 0 is the identity in the
 *   ini_state columns and zero in the others;
 *   gain B x 4 x P = du*_0[a] / dparam_q, the first control's row of du: over the ini_state columns it is the MPC
 *   feedback gain du*_0 / dx_0 (4 x 13), the local linear policy around the current state;
 *   sens_status B as lafse3_ocp_sensitivity's -- after 1 and 2 that instance's dx, du and gain are zero.
 * With dx == du == gain == NULL the call is lafse3_ocp_solve; otherwise groups == 0 or a bit outside the three
 * groups is LAFSE3_EINVAL.
 * dx and du cost one refinement sweep per selected column, as lafse3_ocp_sensitivity.  gain is computed by the
 * adjoint use of the same factorisation: the Newton matrix K is symmetric, so the sweep on the unit right-hand side
 * of row (u_0, a) returns a column of -K^{-1}, and its dot product with dF/dparam_q is du*_0[a] / dparam_q: four
 * sweeps for any P, and with dx == du == NULL nothing else.  u_last stays a constant: its influence on the optimum
 * is too weak for a finite-difference check, and a column that cannot be checked is not offered.  A solver launch
 * for lafse3_reserve, lafse3_last_kernel_ms, the counters and lafse3_check_device; it runs on the caller's stream
 * and leaves the caller's current device alone. */
#define LAFSE3_SENS_THETA 1   /* p_tra[0..2], a_tra[0..2], t : 7 columns */
#define LAFSE3_SENS_INI   2   /* ini_state[0..12]            : 13 columns */
#define LAFSE3_SENS_GOAL  4   /* goal[0..2]                  : 3 columns */
int lafse3_sens_columns(int32_t groups);
int lafse3_ocp_sensitivity_ex(lafse3_ctx *ctx, int64_t B, const double *ini_state, const double *goal,
                              const double *p_tra, const double *a_tra, const double *t, const double *u_last,
                              double *x, double *u, double *lam, double *cost, int32_t *status, int32_t *iters,
                              int32_t groups, double *dx, double *du, double *gain, int32_t *sens_status,
                              void *stream);

/* lafse3_ocp_sensitivity_ex with per-instance cost weights and the sensitivities of the optimum to them: the derivative
 * with respect to the learnable parameters of the cost (the auxvar of the PDP auxiliary system, quad_OC.py:214-306).
 *   weights B x LAFSE3_NW (device) or NULL: instance b solves the NLP whose ten cost weights are
 *   weights[b * 10 .. b * 10 + 9], in the order of lafse3_params: wrt wqt wthrust wrf wvf wqf wwf tra_w_peak
 *   tra_w_decay du_weight; every other field comes from the context's params.  NULL stands for the context's own
 *   weights in every instance (the row lafse3_params_weights gives).  The values are used as given, with no
 *   device-side validation: a non-finite weight ends that instance with status 4, and negative weights are the
 *   caller's business (the inertia correction copes, or the solve reports its status).
 * A fourth parameter group follows the three of lafse3_ocp_sensitivity_ex, in the same fixed order:
 *   LAFSE3_SENS_WEIGHTS  the ten weights, in the order above   10 columns
 * lafse3_sens_columns_w gives P = 7 [THETA] + 13 [INI] + 3 [GOAL] + 10 [WEIGHTS] (LAFSE3_EINVAL for bits outside
 * the four groups).  The outputs are lafse3_ocp_sensitivity_ex's with that P; the columns of the first three groups
 * are its columns bit for bit; dx at stage 0 is zero in the weight columns.  With dx == du == gain == NULL the call
 * is a plain solve with per-instance weights and `groups` is ignored; otherwise groups == 0 or a bit outside the four
 * groups is LAFSE3_EINVAL.  The cost is linear in nine of the weights, so their dF/dw is the cost gradient at unit
 * weight; tra_w_decay enters through the stage weights w_k as t does.  A solver launch for lafse3_reserve,
 * lafse3_last_kernel_ms, the counters and lafse3_check_device; it runs on the caller's stream and leaves the
 * caller's current device alone.  lafse3_sens_columns and lafse3_ocp_sensitivity_ex keep refusing
 * LAFSE3_SENS_WEIGHTS. */
#define LAFSE3_NW 10            /* wrt wqt wthrust wrf wvf wqf wwf tra_w_peak tra_w_decay du_weight (lafse3_params order) */
#define LAFSE3_SENS_WEIGHTS 8   /* 10 columns, after THETA, INI, GOAL */
int lafse3_sens_columns_w(int32_t groups);
/* The ten cost weights of *p in the column order: the row a NULL `weights` stands for. */
int lafse3_params_weights(const lafse3_params *p, double w[LAFSE3_NW]);
int lafse3_ocp_sensitivity_w(lafse3_ctx *ctx, int64_t B, const double *ini_state, const double *goal,
                             const double *p_tra, const double *a_tra, const double *t, const double *u_last,
                             const double *weights,
                             double *x, double *u, double *lam, double *cost, int32_t *status, int32_t *iters,
                             int32_t groups, double *dx, double *du, double *gain, int32_t *sens_status,
                             void *stream);

/* Adjoint backward from a saved optimum: the vector-Jacobian product g^T dz* / dparam of a loss gradient g = (g_x, g_u)
 * with the sensitivities of lafse3_ocp_sensitivity_w, without forming them.  Two calls:
 *
 * lafse3_ocp_solve_rec is lafse3_ocp_sensitivity_w called as a plain solve (weights B x LAFSE3_NW or NULL; the outputs
 * x .. iters are that call's bit for bit; a solver launch for lafse3_reserve, lafse3_last_kernel_ms, the counters and
 * lafse3_check_device) that also writes the optimum record rec, B x lafse3_rec_width() doubles (2223, independent of the
 * horizon; required: NULL is LAFSE3_EINVAL).  The record is the point at which the sensitivity passes factorise, i.e.
 * after the final clamp to the original bounds, in the solver's internal quantities.  One instance, every array
 * stage-major and padded to LAFSE3_MAX_N stages as the iterate block of lafse3_debug_dump (entries of stages beyond the
 * horizon are not written):
 *      0  x    51 x 13   equal to the x output bit for bit
 *    663  u    50 x 4    equal to the u output bit for bit
 *    863  lam  50 x 13   multipliers of the problem whose objective is scaled by s (the lam output is lam / s)
 *   1513  zLu  50 x 4    bound duals of u, lower
 *   1713  zUu  50 x 4                      upper
 *   1913  zLw  51 x 3    bound duals of omega, lower (stage 0, which is fixed, holds 0)
 *   2066  zUw  51 x 3                          upper
 *   2219  mu             the final barrier parameter
 *   2220  s              the objective scaling
 *   2221  status         the solve's status, as a double
 *   2222  horizon        params.horizon of the solve, as a double
 *
 * lafse3_ocp_vjp: grad B x P, grad[b, q] = sum g_x . dx* / dparam_q + sum g_u . du* / dparam_q over the P columns of
 * `groups`, which are lafse3_ocp_sensitivity_w's (lafse3_sens_columns_w).  g_x B x (N+1) x 13 and g_u B x N x 4 are the
 * gradients of the loss with respect to the x and u outputs (each nullable: zero).  The first nine arguments must be
 * the ones the record was solved with, under the same context parameters; ini_state is read from stage 0 of the
 * record.  K is symmetric, so one factorisation at the recorded point and one sweep on the right-hand side (g_x of
 * stages 1..N, g_u) give every column: the sweep's result is contracted with dF / dparam_q as the gain of
 * lafse3_ocp_sensitivity_ex is, and g_x of stage 0 goes to the ini_state columns directly (dx_0 / dini_state is the
 * identity).  sens_status B (nullable): 0 ok, 1 the recorded status > 1, 2 wrong inertia at z*, 3 the record's horizon
 * is not the context's (checked before anything is read by horizon); after 1, 2 and 3 the row of grad is zero.
 * groups == 0, a bit outside the four groups, NULL rec or NULL grad are LAFSE3_EINVAL before any launch.  It uses the
 * context's workspace (covered by lafse3_reserve) and runs on the caller's stream.  Like lafse3_reward it is not a
 * solver launch: the timing, counters and device error word of the most recent solver launch are kept. */
int lafse3_rec_width(void);
int lafse3_ocp_solve_rec(lafse3_ctx *ctx, int64_t B, const double *ini_state, const double *goal,
                         const double *p_tra, const double *a_tra, const double *t, const double *u_last,
                         const double *weights,
                         double *x, double *u, double *lam, double *cost, int32_t *status, int32_t *iters,
                         double *rec, void *stream);
int lafse3_ocp_vjp(lafse3_ctx *ctx, int64_t B, const double *ini_state, const double *goal,
                   const double *p_tra, const double *a_tra, const double *t, const double *u_last,
                   const double *weights, const double *rec, const double *g_x, const double *g_u,
                   int32_t groups, double *grad, int32_t *sens_status, void *stream);

/* Warm start from a saved optimum: lafse3_ocp_solve_rec whose instances start from the record of an earlier solve of the
 * same or of a neighbouring problem (the receding-horizon successor: `shift` stages later) instead of the cold initial
 * point.  The first nine arguments and the outputs x .. iters are lafse3_ocp_solve_rec's.
 *   rec_in       B x lafse3_rec_width() (device; required: NULL is LAFSE3_EINVAL), records as lafse3_ocp_solve_rec or
 *                this call wrote them
 *   opts         NULL: lafse3_default_warm_opts (shift 0, mu_init 1e-3, the three pushes 1e-3: IPOPT's warm_start_*
 *                defaults).  A negative shift, a negative push or a non-finite field is LAFSE3_EINVAL before any
 *                launch; a shift of N or more acts as N (every stage is the record's last); mu_init <= 0 stands for
 *                the context's params.mu_init
 *   warm_status  B (nullable): 0 the instance started from its record, 1 the record was unusable and it started cold
 *   rec_out      B x lafse3_rec_width() (nullable), the record of this solve; may alias rec_in: an instance reads the
 *                whole of its record before it writes, and touches no other instance's
 * One instance, N = params.horizon:
 *   A record is usable when word 2222 equals N, word 2221 (status) is 0 or 1, words 2219 (mu) and 2220 (s) are finite
 *   and positive, and every entry read below is finite.  The test comes before anything of the instance is written.
 *   After an unusable record the instance is lafse3_ocp_solve_rec's: the cold start, every output bit for bit.
 *   Shift.  With j = k + shift: x_k (k = 1..N) and the omega duals of stage k are the record's stage min(j, N);
 *   u_k, lam_k and the duals of u_k (k = 0..N-1) its stage min(j, N-1), so past the record's end the last stage
 *   repeats.  x_0 = ini_state; the omega duals of stage 0 are 0 (the stage is fixed).
 *   Primal push.  u and the omega rows of x_1..x_N are moved into the relaxed bounds [lo, hi] (params.bound_relax) by
 *   the cold start's formula with opts' numbers in place of its 1e-2:
 *     pl = min(bound_push max(1, |lo|), bound_frac (hi - lo)),  pu = min(bound_push max(1, |hi|), bound_frac (hi - lo)),
 *     v = min(max(v, lo + pl), hi - pu);
 *   the other state rows are copied bit for bit.
 *   Objective scaling.  s_new = min(1, 100 / max |dJ/d(x, u)|) at the loaded point (floor 1e-8), the rule of every
 *   solve.  The record's multipliers are those of the problem whose objective is scaled by s_rec (word 2220), so
 *     lam = lam_rec (s_new / s_rec),   z = max(z_rec (s_new / s_rec), mult_bound_push)  for the four bound-dual arrays.
 *   Start.  No least-squares multiplier estimate (IPOPT with warm_start_init_point); mu = opts->mu_init.  The
 *   iterations, the restoration phase, the watchdog and the final clamp are lafse3_ocp_solve's from there; the monotone
 *   update lowers mu further at iteration 0 when the point is better than mu says.  With params.max_iter == 0 the
 *   outputs and rec_out are the loaded point (status 2 unless it passes the convergence test).
 * The problem is nonconvex: a warm start may end in another local optimum than the cold solve of the same arguments.  A
 * warm start that fails (status > 1) is not retried here; the caller re-solves those instances with
 * lafse3_ocp_solve_rec (Engine.ocp_solve_warm does).  rec_out is a valid `rec` of lafse3_ocp_vjp.  A solver launch for
 * lafse3_reserve, lafse3_last_kernel_ms, the counters and lafse3_check_device; it runs on the caller's stream, allocates
 * nothing once reserved, and leaves the caller's current device alone. */
typedef struct lafse3_warm_opts {
    int32_t shift;            /* stages the record is advanced by, 0 .. LAFSE3_MAX_N (more acts as the horizon) */
    double  mu_init;          /* barrier parameter the warm solve starts with; <= 0: the context's params.mu_init */
    double  bound_push, bound_frac;   /* IPOPT warm_start_bound_push / _frac */
    double  mult_bound_push;          /* IPOPT warm_start_mult_bound_push */
} lafse3_warm_opts;
int lafse3_default_warm_opts(lafse3_warm_opts *o);
int lafse3_ocp_solve_warm(lafse3_ctx *ctx, int64_t B, const double *ini_state, const double *goal,
                          const double *p_tra, const double *a_tra, const double *t, const double *u_last,
                          const double *weights, const double *rec_in, const lafse3_warm_opts *opts,
                          double *x, double *u, double *lam, double *cost, int32_t *status, int32_t *iters,
                          int32_t *warm_status, double *rec_out, void *stream);

/* fp32 twin of lafse3_ocp_solve: the same arguments as float32 device buffers.  Inputs are
 * widened to fp64 and outputs rounded to fp32 on the device; the NLP itself is solved in fp64 (IPOPT's
 * 1e-8 tolerance, quad_OC.py:172, is below float32 resolution). */
int lafse3_ocp_solve_f32(lafse3_ctx *ctx, int64_t B, const float *ini_state, const float *goal,
                         const float *p_tra, const float *a_tra, const float *t, const float *u_last,
                         float *x, float *u, float *lam, float *cost, int32_t *status, int32_t *iters,
                         void *stream);

/* Batched run_quad.objective (quad_policy.py:67-91): t is rounded to one decimal (round(t,1) on a
 * float64), the NLP is solved, the rotor tracks (quad_model.py:239-276) are scored against the gate
 * gate12 B x 12 (4 corners, solid_geometry.obstacle) and the goal.  reward B, status B (nullable). */
int lafse3_objective(lafse3_ctx *ctx, int64_t B, const double *ini_state, const double *goal,
                     const double *gate12, const double *p_tra, const double *a_tra, const double *t,
                     const double *u_last, double *reward, int32_t *status, void *stream);

/* Batched run_quad.sol_gradient (quad_policy.py:94-112) on DNN outputs as emitted by torch:
 *   dnn_out B x 7 float32 = [p_tra(3), tra_ang(3), t].  9 NLP solves per sample (nominal, +1e-3 on
 *   each of the 6 pose variables, t-0.1, t+0.1), reference dtype quirks reproduced.
 *   u_last B x 4 or NULL (passed to the 6 perturbed solves only, as the reference does).
 * out8 B x 8 = [-drdx,-drdy,-drdz,-drda,-drdb,-drdc,-drdt, j]; rewards9 B x 9 and status9 B x 9
 * (nullable) expose the 9 rewards / solver statuses. */
int lafse3_sol_gradient(lafse3_ctx *ctx, int64_t B, const double *ini_state, const double *goal,
                        const double *gate12, const float *dnn_out, const double *u_last, double *out8,
                        double *rewards9, int32_t *status9, void *stream);

/* Batched run_quad.get_input (quad_policy.py:202-211): one NLP solve per sample on float32 DNN
 * outputs (t used unrounded), returns the first control u0 B x 4 and optionally the state
 * trajectory x B x (N+1) x 13 (nn_train_2.py:37-39 reads it). */
int lafse3_get_input(lafse3_ctx *ctx, int64_t B, const double *ini_state, const double *goal,
                     const double *u_last, const float *dnn_out, double *u0, double *x, int32_t *status,
                     void *stream);

/* Reward of given state trajectories x B x (N+1) x 13 (the scoring half of run_quad.objective,
 * quad_policy.py:78-91: rotor tips quad_model.py:239-276, obstacle.collis_det solid_geometry.py:104-168,
 * goal path term over rows N-4..N-1).  reward B.  Not a solver launch: the timing, counters and device error
 * word of the most recent solver launch (lafse3_last_kernel_ms / _last_counters / _check_device) are kept.
 * Short horizons: the path term indexes a numpy array of N+1 rows, so at N = 2 and 3 a negative row N-1-p wraps to
 * row N-1-p + N+1 (N = 3: rows 2, 1, 0, 3; N = 2: rows 1, 0, 2, 1), as collis_det's t-1 already does.  At N = 1 the
 * reference raises IndexError (row -3 of 2): lafse3_reward, lafse3_objective and lafse3_sol_gradient return
 * LAFSE3_EINVAL there, before any allocation or launch.  The solves that score no reward (lafse3_ocp_solve, _f32,
 * lafse3_ocp_sensitivity, lafse3_get_input) accept horizon 1. */
int lafse3_reward(lafse3_ctx *ctx, int64_t B, const double *x, const double *goal, const double *gate12,
                  double *reward, void *stream);

/* Traversal time of the moving-gate loop for B episodes: quad_moving.py:29-57 (solver) -- the fixed point
 * t1 += (t2 - t1) / 2 of DNN2's time output on the gate advanced by velo t1 and pitched by w t1 (main.py:90-94
 * inputs), from t1 = |centroid - r| / 3 until |t2 - t1| <= 0.001 (at most 200 updates).  state B x 13, final_point
 * B x 3, gate12 B x 12 (4 corners), velo B x 3 (gate velocity of this plant step); dnn2_weights: the trained
 * DNN2 (18-128-128-7, nn3_1.pth) packed as l1.weight (128 x 18), l1.bias, l2.weight (128 x 128, row-major), l2.bias,
 * row 6 of l3.weight, l3.bias[6] (lafse3_dnn2_weight_count() floats, float32 as the reference evaluates it;
 * 16-byte aligned).
 * t_out B, iters B (updates taken; nullable). */
int lafse3_traversal_time(lafse3_ctx *ctx, int64_t B, const double *state, const double *final_point,
                          const double *gate12, const double *velo, double w, const float *dnn2_weights,
                          double *t_out, int32_t *iters, void *stream);
int lafse3_dnn2_weight_count(void);

/* Time (ms, HIP events on `stream`) of the most recent solver-kernel launch on this context (lafse3_reward
 * launches are not solver launches). */
float lafse3_last_kernel_ms(const lafse3_ctx *ctx);
/* Sum over the last launch of per-instance IPM iterations, Riccati sweeps and line-search trials
 * (written by the kernel; read back synchronously). counters[3].  Returns LAFSE3_EDEVICE (counters still
 * filled) while the device error word is set, i.e. when a solver launch since the last lafse3_check_device
 * raised it (not necessarily the last launch); lafse3_check_device reports and clears it. */
int lafse3_last_counters(lafse3_ctx *ctx, int64_t counters[3]);
/* Wait for the most recent solver launch on this context and return LAFSE3_EDEVICE (message via
 * lafse3_last_error) when a solver launch since the last such report raised the device error word: a
 * sol_gradient probe task whose queue entry never landed (its rewards9/status9 slot then holds NaN / status 7).
 * Launches do not clear the word; this call does, after reporting it.  0 otherwise. */
int lafse3_check_device(lafse3_ctx *ctx);
/* Restoration-phase counts of the last launch, summed over its NLP instances: counters[0] entries into the
 * restoration phase, counters[1] returns to the original problem (entries - returns ended the solve with
 * status 2, 4, 6, 8 or 9).  Read back synchronously; EDEVICE as lafse3_last_counters. */
int lafse3_last_resto_counters(lafse3_ctx *ctx, int64_t counters[2]);
/* Debug: subsequent launches write, per instance and per IPM iteration (< iters), 16 doubles to the device buffer
 * buf (instances x iters x 16):
 *    0 mu                 barrier parameter of the iteration
 *    1 E0                 overall NLP error (mu = 0) at the iterate
 *    2 theta              constraint violation at the iterate
 *    3 phi                barrier objective at the iterate
 *    4 gradphi.d          directional derivative of phi along the step
 *    5 alpha_max          fraction-to-the-boundary primal step
 *    6 alpha_z            dual step
 *    7 alpha              accepted primal step
 *    8 delta_w            inertia regularisation the step was computed with (0: none was needed)
 *    9 accepted           1 when the line search accepted a trial point
 *   10 filter_size        entries of the filter after the iteration
 *   11 sweeps             Riccati sweeps so far (cumulative)
 *   12 ratio 0            residual ratio of the step before iterative refinement
 *   13 ratio 1            residual ratio after the first refinement sweep (-1: none)
 *   14 J                  unscaled objective at the iterate
 *   15 barrier log sum    sum of log(v - lo) + log(hi - v) over the bounded variables at the iterate
 * Iterations spent inside a restoration phase write no row.  buf = NULL disables. */
int lafse3_debug_trace(lafse3_ctx *ctx, double *buf, int iters);
/* Debug: dump the Newton step of IPM iteration `it` (before or after iterative refinement) and the iterate the
 * Newton system was formed at into buf (instances x 3732).  One record, every array stage-major and padded to
 * LAFSE3_MAX_N stages (entries of stages beyond the horizon are not written):
 *   the step     dx (51x13) | du (50x4) | lam+ (50x13)                                          1513 doubles
 *   the iterate  x (51x13) | u (50x4) | lam (50x13) | zLu (50x4) | zUu (50x4) | zLw (51x3) | zUw (51x3)
 * in the solver's internal quantities: lam+ and lam are multipliers of the problem whose objective is scaled by
 * s_obj (the multipliers lafse3_ocp_solve returns are lam / s_obj), zL / zU the bound duals of u and of omega
 * (stage 0, which is fixed, has zLw = zUw = 0).  mu and delta_w of that iteration are words 0 and 8 of
 * lafse3_debug_trace.  With an inertia retry the pre-refinement record is that of the last retry.
 * The iterate is written by lafse3_ocp_solve / lafse3_ocp_solve_f32 launches, which run a kernel of their own while
 * a dump (this one or lafse3_debug_dump_resto) is armed (the extra stores are compiled out of the production kernel); the
 * other entry points write the step only, at the same stride of 3732 doubles per instance.  buf = NULL disables. */
int lafse3_debug_dump(lafse3_ctx *ctx, double *buf, int it, int after_refine);
/* Debug: dump one Newton step of the restoration phase (resto.inc) into buf (instances x 9153): iteration `it` of the
 * entry-th entry into the phase of each solve, both 0-based (an instance that never gets there writes nothing).  One
 * record per instance, every array stage-major and padded to LAFSE3_MAX_N stages (entries of stages beyond the horizon
 * are not written), in this order:
 *   the step       dx (51x13) | du (50x4) | lam+ (50x13) | dp (50x13) | dn (50x13)                     2813 doubles
 *                  before (after_refine = 0) or after the iterative refinement; with an inertia retry, of the last retry
 *   the iterate    x (51x13) | u (50x4) | lam (50x13) | zLu (50x4) | zUu (50x4) | zLw (51x3) | zUw (51x3) |
 *                  p (50x13) | n (50x13) | z_p (50x13) | z_n (50x13)                                    4819 doubles
 *                  the point the system was formed at; row k of p, n, z_p, z_n belongs to the constraint
 *                  f_d(x_k, u_k) - x_{k+1} - p_k + n_k = 0, whose multiplier is lam_k (L = f_R + lam^T c_R)
 *   the reference  x_R (51x13) | u_R (50x4)          the point where the phase started                  863 doubles
 *   scalars        mu | eta | delta_w of the dumped factorisation | written (1.0 once the step is there) |
 *                  residual ratio before the refinement | after it                                        6 doubles
 *   least squares  lam+ (50x13) of the multiplier estimate at the start point, before the cut at 1e3 |
 *                  ok (1: factorised, 0: wrong inertia, lam+ not written) | IPM iterations taken before this
 *                  entry (iteration `it` of the entry is IPM iteration that + it)                        652 doubles
 * The least-squares part is written at the entry itself, whatever `it`.  Written by lafse3_ocp_solve /
 * lafse3_ocp_solve_f32 launches only, which run the kernel of lafse3_debug_dump while either dump is armed (the stores
 * are compiled out of the production kernels); both dumps may be armed together.  buf = NULL disables. */
int lafse3_debug_dump_resto(lafse3_ctx *ctx, double *buf, int entry, int it, int after_refine);
/* Debug: per-instance record of 32 x uint64 into buf (instances x 32).  The timer build (-DLAFSE3_PHASE_TIMERS)
 * fills columns 0..15 and 24..31, every build the placement record 16..23: 12 phase timers in s_memtime cycles (init, errors, table, backward, forward, adjoint, residual, refine-backward,
 * line search, accept, reward, other), 4 backward-sweep stage-phase timers, then the placement record: start and
 * end s_memrealtime (100 MHz), HW_ID and XCC_ID of the wave, then iterations, sweeps, status, trials; then 8
 * wait-probe sums (cycles spent in the factorisation stage's vector-memory waits, the last one the probes' own
 * cost). */
int lafse3_debug_timers(lafse3_ctx *ctx, uint64_t *buf);
/* Per-instance IPM iteration counts of subsequent launches into buf (int32, one per NLP instance: B for
 * ocp_solve / objective / get_input, B x 9 for sol_gradient in the rewards9 slot order; entry points that take
 * their own iters argument use that).  One store per instance; bench.py reads its percentiles.  capacity = the
 * entries buf holds: a later launch that would write more fails with LAFSE3_EINVAL.  NULL disables. */
int lafse3_record_iters(lafse3_ctx *ctx, int32_t *buf, int64_t capacity);
/* Debug (tests of the probe-queue guard): in later sol_gradient launches the queue entry of sample `sample`'s
 * probe solves is reserved but never written, so those probes are lost and the device error word is raised.
 * -1 disables. */
int lafse3_debug_drop_push(lafse3_ctx *ctx, int64_t sample);
const char *lafse3_last_error(void);
const char *lafse3_version(void);

#ifdef __cplusplus
}
#endif
#endif /* LAFSE3_H */
