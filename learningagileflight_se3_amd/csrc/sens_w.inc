// sens_w.inc — sens_ex.inc's pass with a fourth parameter group, the ten cost weights (lafse3_ocp_sensitivity_w;
// #included by ipm_kernel.hip after sens_ex.inc, compiled into ipm_kernel_sens_w only).
//
// Columns, in this order, restricted to the selected groups: theta 7, ini_state 13, goal 3 exactly as sens_ex.inc
// (sens_column, the same code: the same bits), then
//   weights     wrt wqt wthrust wrf wvf wqf wwf tra_w_peak tra_w_decay du_weight   10   (lafse3_params order)
//               x rows k = 1..N and u rows k = 0..N-1 from the closed forms of weight_columns.hpp times the objective
//               scaling C.s; no dynamics rows.  dx at stage 0 is zero.
// The instance's weights are those run_instance<.., SENSW> put into S.mdl and S.wk; `wv` is its row of ten (the
// context's when the caller gave none), read here for tra_w_decay, which S.mdl does not carry.
// sens_w_pass repeats sens_ex_pass's structure instead of sharing it through a template: sens_ex_pass and with it
// ipm_kernel_sens_ex stay the code they are.
// Forward route: one sweep per selected column.  Adjoint route: sens_ex.inc's four sweeps; a weight column is
// contracted over its x rows against DX and its u rows against DU.
constexpr int SENS_G_W = 8;
constexpr int SENS_W_ALL = SENS_G_THETA | SENS_G_INI | SENS_G_GOAL | SENS_G_W;

__host__ __device__ inline int sens_w_columns(int groups)
{
    return sens_ex_columns(groups & ~SENS_G_W) + ((groups & SENS_G_W) ? NW : 0);
}

__device__ inline int sens_w_group_size(int grp)
{
    return (grp == SENS_G_THETA) ? 7 : (grp == SENS_G_INI ? NX : (grp == SENS_G_GOAL ? 3 : NW));
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

// As sens_ex_pass with P = sens_w_columns(groups).  prm: the context's parameters (dt, and what sens_column reads of
// them with tra_w_decay replaced by the instance's).
__device__ __noinline__ int sens_w_pass(const lafse3_params &prm, const Model &M, Smem &S, const Ctl &C, gdouble *ws,
                                        const double *a3, double tt, double decay, int ok, int groups, double *dxo,
                                        double *duo, double *gno)
{
    WS_TRAJ(ws);
    const int lane = lane_id();
    const int N = C.N;
    const int P = sens_w_columns(groups);
    gdouble *rq = ws + WS_RQ, *rr = ws + WS_RR, *rc = ws + WS_RC;
    // sens_column's t column reads tra_w_decay and dt of its params argument: the instance's decay
    lafse3_params pw;
    pw.dt = prm.dt;
    pw.tra_w_decay = decay;
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
            const int nq = sens_w_group_size(grp);
            for (int q = 0; q < nq; ++q, ++col) {
                if (st == SENS_OK) {
                    if (lane <= N) {
                        const int k = lane;
                        double vx[NX], vu[NU], vc[NX];
                        if (grp == SENS_G_W) {
                            sens_w_column(M, S, C, prm.dt, decay, tt, q, k, vx, vu);
#pragma unroll
                            for (int i = 0; i < NX; ++i) vc[i] = 0.0;
                        } else {
                            sens_column(pw, M, S, C, a3, tt, grp, q, k, vx, vu, vc);
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
            double *o = gno + (int64_t)a * P;
            int col = 0;
            for (int grp = SENS_G_THETA; grp <= SENS_G_W; grp <<= 1) {
                if (!(groups & grp)) continue;
                if (grp == SENS_G_INI) {
                    // stage 0 only: (A_0^T lam+_0)_i + qu_i (du_0[0] + .. + du_0[3]), the same in every lane
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
                        o[col + lane] = v;
                    }
                    col += NX;
                    continue;
                }
                const int nq = sens_w_group_size(grp);
                for (int q = 0; q < nq; ++q, ++col) {
                    double acc = 0.0;
                    if (grp == SENS_G_W) {
                        if (lane <= N) {   // x rows k = 1..N against dx, u rows k = 0..N-1 against du
                            const int k = lane;
                            double vx[NX], vu[NU];
                            sens_w_column(M, S, C, prm.dt, decay, tt, q, k, vx, vu);
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
                        sens_column(pw, M, S, C, a3, tt, grp, q, k, vx, vu, vc);
#pragma unroll
                        for (int i = 0; i < NX; ++i) acc = fma(DX[i * SX + k], vx[i], acc);
                    }
                    acc = wsum(acc);
                    if (lane == 0) o[col] = acc;
                }
            }
        }
    }
    return st;
}
