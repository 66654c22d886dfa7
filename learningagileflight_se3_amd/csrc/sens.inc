// sens.inc — analytic sensitivities of a finished MODE_SOLVE instance to theta, ini_state, goal and the ten cost
// weights, and the MPC feedback gain (lafse3_ocp_sensitivity / _ex / _w; #included by ipm_kernel.hip after ift_probes,
// compiled into ipm_kernel_ext only; vjp.inc contracts with the same columns).
//
// By the implicit function theorem on the KKT system F(z, param) = 0 of the barrier problem at the final mu,
// dz*/dparam_q = -K^{-1} dF/dparam_q with K the Newton matrix at z* (delta_w = 0): one factorisation, then refinement
// sweeps (backward_chain + forward_chain) as ift_probes runs them for its six reward probes.  The derivative is that of
// the barrier problem: across an active-set change it is a one-sided smoothing, not a subgradient.
//
// Columns, in this order, restricted to the selected groups (LAFSE3_SENS_THETA | _INI | _GOAL | _WEIGHTS):
//   theta       p_tra[0..2], a_tra[0..2], t   7   x rows k = 1..N-1: only the traversal cost w_k(t) tra(x_k; p_tra,
//                                                 a_tra) of stages 1..N-1 depends on theta (quad_model.py:200-213)
//                                                   q < 6   s d(grad_x cost_k)/dtheta_q, the central difference
//                                                           ift_probes uses (tra_grad_fd);
//                                                   q = 6   s dw_k/dt grad_x tra(x_k), analytic: w_k = peak exp(-decay
//                                                           (k dt - t)^2), dw_k/dt = 2 decay (k dt - t) w_k, and
//                                                           grad_x tra = state_cost_grad at weight 1 minus at weight 0
//                                                           (it is affine in the weight).
//   ini_state   ini_state[0..12]             13   stage 0 only (x_0 is not a decision variable): dynamics rows
//                                                 A_0 e_i, u rows the q-u cross term of the Lagrangian Hessian
//                                                 (StageHess::qu from lam_0, the same value for every rotor)
//   goal        goal[0..2]                    3   x rows k = 1..N, position row i: -2 wrf s (state_cost_grad's
//                                                 goal term; the terminal cost carries the same weight, and the
//                                                 attitude-to-goal term has a fixed target)
//   weights     wrt wqt wthrust wrf wvf wqf wwf tra_w_peak tra_w_decay du_weight   10   (lafse3_params order)
//                                                 x rows k = 1..N and u rows k = 0..N-1 from the closed forms of
//                                                 weight_columns.hpp times the objective scaling C.s; no dynamics rows
// Each is dF/dparam_q in the three row blocks linear_solve reads (x rows WS_RQ, u rows WS_RR, dynamics rows WS_RC); a
// chain sweep on the right-hand side r returns d = -K^{-1} r in (dx, du, lam+), so dz*/dparam_q is the sweep's result
// as it stands.  dx at stage 0 is the identity in the ini_state columns and zero otherwise.
// The instance's weights are those run_instance<.., EXT> put into S.mdl and S.wk; `decay` is its tra_w_decay (the
// context's when the caller gave no weights), which S.mdl does not carry.
//
// Forward route (dx, du): one sweep per selected column.
// Adjoint route (gain = du*_0 / dparam, 4 x P): K is symmetric (row blocks x, u, dynamics against the unknowns dx,
// du, lam+), so the sweep on r = e_(u_0, a) returns d_a = -K^{-1} e_(u_0, a), and
//   du*_0[a] / dparam_q = e^T (-K^{-1} c_q) = d_a . c_q
// summed over the three blocks: dx against the x rows, du against the u rows, lam+ (what costates_identity<false>
// with fac = 0 leaves in lamp, the sweep's own sign) against the dynamics rows.  Four sweeps for any number of
// columns (sens_contract).
// u_last stays a constant: its influence on the optimum is too weak for a finite-difference yardstick.
constexpr int SENS_G_THETA = 1, SENS_G_INI = 2, SENS_G_GOAL = 4, SENS_G_W = 8;
constexpr int SENS_W_ALL = SENS_G_THETA | SENS_G_INI | SENS_G_GOAL | SENS_G_W;
enum { SENS_OK = 0, SENS_UNCONVERGED = 1, SENS_INERTIA = 2 };

__host__ __device__ inline int sens_group_size(int grp)
{
    return (grp == SENS_G_THETA) ? 7 : (grp == SENS_G_INI ? NX : (grp == SENS_G_GOAL ? 3 : NW));
}

__host__ __device__ inline int sens_columns(int groups)
{
    return ((groups & SENS_G_THETA) ? 7 : 0) + ((groups & SENS_G_INI) ? NX : 0) + ((groups & SENS_G_GOAL) ? 3 : 0) +
           ((groups & SENS_G_W) ? NW : 0);
}

// dF/dparam at stage k (the caller's lane, k <= N) of column q of group grp (theta, ini_state or goal): vx the x rows
// (k >= 1), vu the u rows and vc the dynamics rows (k < N), scaled by the objective scaling C.s
__device__ __attribute__((always_inline)) inline void sens_column(const Model &M, const Smem &S, const Ctl &C,
                                                                  const double *a3, double dt, double decay,
                                                                  double tt, int grp, int q, int k, double *vx,
                                                                  double *vu, double *vc)
{
    const int N = C.N;
#pragma unroll
    for (int i = 0; i < NX; ++i) vx[i] = vc[i] = 0.0;
#pragma unroll
    for (int a = 0; a < NU; ++a) vu[a] = 0.0;
    if (grp == SENS_G_THETA) {
        if (k >= 1 && k < N) {
            if (q < 6) {
                tra_grad_fd(M, S, C, a3, q, k, vx);
            } else {
                double xk[NX], g1[NX], g0[NX];
                load_stage(S, k, xk);
                state_cost_grad(M, S.at, S.goal, S.ptra, 1.0, xk, g1);
                state_cost_grad(M, S.at, S.goal, S.ptra, 0.0, xk, g0);
                const double dwk = 2 * decay * (dt * k - tt) * S.wk[k];
#pragma unroll
                for (int i = 0; i < NX; ++i) vx[i] = C.s * dwk * (g1[i] - g0[i]);
            }
        }
    } else if (grp == SENS_G_GOAL) {
        if (k >= 1) {
#pragma unroll
            for (int i = 0; i < 3; ++i) vx[i] = (i == q) ? -2 * M.wrf * C.s : 0.0;
        }
    } else if (k == 0) {
        double x0[NX], u0[NU], l0[NX], e[NX];
        load_stage(S, 0, x0);
        load_u(S, 0, u0);
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            l0[i] = S.lam[i * SX];
            e[i] = (i == q) ? 1.0 : 0.0;
        }
        A_times(M, x0, u0, e, vc);
        StageHess H;
        stage_hessian(M, S.at, C.s, 0.0, x0, u0, l0, H);
        const double hq = (q >= 6 && q < 10) ? sel4(q - 6, H.qu[0], H.qu[1], H.qu[2], H.qu[3]) : 0.0;
#pragma unroll
        for (int a = 0; a < NU; ++a) vu[a] = hq;
    }
}

// dF/dw_q at stage k (the caller's lane, k <= N): vx the x rows (k >= 1), vu the u rows (k < N)
__device__ __attribute__((always_inline)) inline void sens_w_column(const Model &M, const Smem &S, const Ctl &C,
                                                                    double dt, double decay, double tt, int q, int k,
                                                                    double *vx, double *vu)
{
    const int N = C.N;
#pragma unroll
    for (int i = 0; i < NX; ++i) vx[i] = 0.0;
#pragma unroll
    for (int a = 0; a < NU; ++a) vu[a] = 0.0;
    if (q == W_WTHRUST || q == W_DU) {
        if (k < N) {
            double um[NU], uk[NU], up[NU];
            load_u(S, k, uk);
#pragma unroll
            for (int a = 0; a < NU; ++a) {
                um[a] = (k == 0) ? S.ulast[a] : S.u[a * SX + k - 1];
                up[a] = (k + 1 < N) ? S.u[a * SX + k + 1] : 0.0;
            }
            weight_column_u(q, um, uk, up, k + 1 >= N, vu);
#pragma unroll
            for (int a = 0; a < NU; ++a) vu[a] *= C.s;
        }
    } else if (k >= 1) {
        double xk[NX];
        load_stage(S, k, xk);
        weight_column_x(M, S.at, S.goal, S.ptra, (k < N) ? S.wk[k] : 0.0, dt * k - tt, decay, k >= N, q, xk, vx);
#pragma unroll
        for (int i = 0; i < NX; ++i) vx[i] *= C.s;
    }
}

// Contracts a finished sweep d = (dx, du, lam+) (S.dx, S.du, S.lamp) with dF/dparam_q of every selected column:
// o[col] = d . c_q, col = 0..P-1.  The theta and goal columns have x rows only, the weight columns x rows against dx
// and u rows against du: one wsum over the stages per column.  The ini_state columns live on stage 0 alone, so their
// contraction is (A_0^T lam+_0)_i (At_times) plus qu_i times the sum of du_0, with no reduction; gx0 (nullable, 13
// values) is added to them.  `lane` is the caller's lane index: vjp.inc passes an opaque one.
__device__ __attribute__((always_inline)) inline void sens_contract(const Model &M, const Smem &S, const Ctl &C,
                                                                    const double *a3, double dt, double decay,
                                                                    double tt, int groups, int lane, const double *gx0,
                                                                    double *o)
{
    const int N = C.N;
    const double *DX = S.dx, *DU = S.du, *LAM = S.lam, *LP = S.lamp;
    int col = 0;
    for (int grp = SENS_G_THETA; grp <= SENS_G_W; grp <<= 1) {
        if (!(groups & grp)) continue;
        if (grp == SENS_G_INI) {
            // the same in every lane
            double x0[NX], u0[NU], l0[NX], lp0[NX], atl[NX];
            load_stage(S, 0, x0);
            load_u(S, 0, u0);
#pragma unroll
            for (int i = 0; i < NX; ++i) {
                l0[i] = LAM[i * SX];
                lp0[i] = LP[i * SX];
            }
            At_times(M, x0, u0, lp0, atl);
            StageHess H;
            stage_hessian(M, S.at, C.s, 0.0, x0, u0, l0, H);
            double sdu = 0.0;
#pragma unroll
            for (int b = 0; b < NU; ++b) sdu += DU[b * SX];
#pragma unroll
            for (int i = 0; i < 4; ++i) atl[6 + i] += H.qu[i] * sdu;
            if (lane < NX) {
                double v = atl[0];
#pragma unroll
                for (int i = 1; i < NX; ++i) v = (lane == i) ? atl[i] : v;
                o[col + lane] = gx0 ? v + gx0[lane] : v;
            }
            col += NX;
            continue;
        }
        const int nq = sens_group_size(grp);
        for (int q = 0; q < nq; ++q, ++col) {
            double acc = 0.0;
            if (grp == SENS_G_W) {
                if (lane <= N) {   // x rows k = 1..N against dx, u rows k = 0..N-1 against du
                    const int k = lane;
                    double vx[NX], vu[NU];
                    sens_w_column(M, S, C, dt, decay, tt, q, k, vx, vu);
                    if (k >= 1) {
#pragma unroll
                        for (int i = 0; i < NX; ++i) acc = fma(DX[i * SX + k], vx[i], acc);
                    }
                    if (k < N) {
#pragma unroll
                        for (int b = 0; b < NU; ++b) acc = fma(DU[b * SX + k], vu[b], acc);
                    }
                }
            } else if (lane >= 1 && lane <= N) {   // theta and goal columns have x rows only
                const int k = lane;
                double vx[NX], vu[NU], vc[NX];
                sens_column(M, S, C, a3, dt, decay, tt, grp, q, k, vx, vu, vc);
#pragma unroll
                for (int i = 0; i < NX; ++i) acc = fma(DX[i * SX + k], vx[i], acc);
            }
            acc = wsum(acc);
            if (lane == 0) o[col] = acc;
        }
    }
}

// The outputs of one instance: dxo P x (N+1) x 13, duo P x N x 4, gno 4 x P (each nullable), P = sens_columns(groups).
// dt: the context's; decay: the instance's tra_w_decay.  `ok`: the solve ended solved or acceptable.  Returns the
// instance's sens_status; the outputs are zero unless it is SENS_OK.
__device__ __noinline__ int sens_pass(const Model &M, Smem &S, const Ctl &C, gdouble *ws, const double *a3, double dt,
                                      double decay, double tt, int ok, int groups, double *dxo, double *duo,
                                      double *gno)
{
    WS_TRAJ(ws);
    const int lane = lane_id();
    const int N = C.N;
    const int P = sens_columns(groups);
    gdouble *rq = ws + WS_RQ, *rr = ws + WS_RR, *rc = ws + WS_RC;
    int st = ok ? SENS_OK : SENS_UNCONVERGED;
    if (ok) {
        int sw = 0;
        double rat[4];
        if (!linear_solve(M, S.at, S, C, ws, 0.0, 1, 0, 0, 0, sw, rat, nullptr)) st = SENS_INERTIA;
    }
    for (int e = lane; e < NU * SX; e += WAVE) rr[e] = 0.0;
    for (int e = lane; e < NX * SX; e += WAVE) rc[e] = 0.0;
    vm_sync();
    // ---- forward route: one sweep per selected column
    if (dxo || duo) {
        int col = 0;
        for (int grp = SENS_G_THETA; grp <= SENS_G_W; grp <<= 1) {
            if (!(groups & grp)) continue;
            const int nq = sens_group_size(grp);
            for (int q = 0; q < nq; ++q, ++col) {
                if (st == SENS_OK) {
                    if (lane <= N) {
                        const int k = lane;
                        double vx[NX], vu[NU], vc[NX];
                        if (grp == SENS_G_W) {
                            sens_w_column(M, S, C, dt, decay, tt, q, k, vx, vu);
#pragma unroll
                            for (int i = 0; i < NX; ++i) vc[i] = 0.0;
                        } else {
                            sens_column(M, S, C, a3, dt, decay, tt, grp, q, k, vx, vu, vc);
                        }
#pragma unroll
                        for (int i = 0; i < NX; ++i) rq[i * SX + k] = vx[i];
                        if (k < N) {   // zero again behind an ini_state column
#pragma unroll
                            for (int a = 0; a < NU; ++a) rr[a * SX + k] = vu[a];
#pragma unroll
                            for (int i = 0; i < NX; ++i) rc[i * SX + k] = vc[i];
                        }
                    }
                    vm_sync();
                    int sw = 0;
                    double rat[4];
                    linear_solve(M, S.at, S, C, ws, 0.0, 0, 0, 0, 0, sw, rat, nullptr);
                    sync();
                }
                // LDS SoA [i][k] -> stage-major [k][i]; every index is below (N+1) * 13 resp. N * 4 of this column's
                // block.  Stage 0 of dx is the identity in the ini_state columns and zero otherwise.
                if (dxo) {
                    double *o = dxo + (int64_t)col * (N + 1) * NX;
                    for (int e = lane; e < (N + 1) * NX; e += WAVE) {
                        double v = 0.0;
                        if (st == SENS_OK) v = (e >= NX) ? DX[(e % NX) * SX + e / NX]
                                                         : ((grp == SENS_G_INI && e == q) ? 1.0 : 0.0);
                        o[e] = v;
                    }
                }
                if (duo) {
                    double *o = duo + (int64_t)col * N * NU;
                    for (int e = lane; e < N * NU; e += WAVE) o[e] = (st == SENS_OK) ? DU[(e % NU) * SX + e / NU] : 0.0;
                }
            }
        }
    }
    // ---- adjoint route: one sweep per control of stage 0
    if (gno) {
        if (st != SENS_OK) {
            for (int e = lane; e < NU * P; e += WAVE) gno[e] = 0.0;
            return st;
        }
        for (int a = 0; a < NU; ++a) {
            for (int e = lane; e < NX * SX; e += WAVE) {
                rq[e] = 0.0;
                rc[e] = 0.0;
            }
            for (int e = lane; e < NU * SX; e += WAVE) rr[e] = (e == a * SX) ? 1.0 : 0.0;
            vm_sync();
            int sw = 0;
            double rat[4];
            linear_solve(M, S.at, S, C, ws, 0.0, 0, 0, 0, 0, sw, rat, nullptr);
            sync();
            sens_contract(M, S, C, a3, dt, decay, tt, groups, lane, nullptr, gno + (int64_t)a * P);
        }
    }
    return st;
}
