// sens.inc — analytic trajectory sensitivities dx*/dtheta, du*/dtheta of a finished MODE_SOLVE instance
// (lafse3_ocp_sensitivity; #included by ipm_kernel.hip after ift_probes, compiled into ipm_kernel_sens only).
//
// theta = (p_tra[0..2], a_tra[0..2], t).  By the implicit function theorem on the KKT system F(z, theta) = 0 of the
// barrier problem at the final mu, dz*/dtheta_q = -K^{-1} dF/dtheta_q with K the Newton matrix at z* (delta_w = 0):
// one factorisation, then one refinement sweep (backward_chain + forward_chain) per parameter, as ift_probes does for
// its six reward probes.  Only the traversal cost w_k(t) tra(x_k; p_tra, a_tra) of stages 1..N-1 depends on theta
// (quad_model.py:200-213), so dF/dtheta_q has x rows k = 1..N-1 only:
//   q < 6   s d(grad_x cost_k)/dtheta_q, the central difference ift_probes uses (tra_grad_fd);
//   q = 6   s dw_k/dt grad_x tra(x_k), analytic: w_k = peak exp(-decay (k dt - t)^2), dw_k/dt = 2 decay (k dt - t) w_k,
//           and grad_x tra = state_cost_grad at weight 1 minus at weight 0 (it is affine in the weight).
// u_last and the initial state are constants, so dx at stage 0 is zero.  The derivative is that of the barrier
// problem: across an active-set change it is a one-sided smoothing, not a subgradient.
constexpr int SENS_NP = 7;
enum { SENS_OK = 0, SENS_UNCONVERGED = 1, SENS_INERTIA = 2 };

// dxo: 7 x (N+1) x 13, duo: 7 x N x 4 of this instance (each nullable), stage-major.  `ok`: the solve ended solved or
// acceptable.  Returns the instance's sens_status; the outputs are zero unless it is SENS_OK.
__device__ __noinline__ int sens_pass(const lafse3_params &prm, const Model &M, Smem &S, const Ctl &C, gdouble *ws,
                                      const double *a3, double tt, int ok, double *dxo, double *duo)
{
    WS_TRAJ(ws);
    const int lane = lane_id();
    const int N = C.N;
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
    for (int q = 0; q < SENS_NP; ++q) {
        if (st == SENS_OK) {
            if (lane <= N) {
                const int k = lane;
                double v[NX];
#pragma unroll
                for (int i = 0; i < NX; ++i) v[i] = 0.0;
                if (k >= 1 && k < N) {
                    if (q < 6) {
                        tra_grad_fd(M, S, C, a3, q, k, v);
                    } else {
                        double xk[NX], g1[NX], g0[NX];
                        load_stage(S, k, xk);
                        state_cost_grad(M, S.at, S.goal, S.ptra, 1.0, xk, g1);
                        state_cost_grad(M, S.at, S.goal, S.ptra, 0.0, xk, g0);
                        const double dwk = 2 * prm.tra_w_decay * (prm.dt * k - tt) * S.wk[k];
#pragma unroll
                        for (int i = 0; i < NX; ++i) v[i] = C.s * dwk * (g1[i] - g0[i]);
                    }
                }
#pragma unroll
                for (int i = 0; i < NX; ++i) rq[i * SX + k] = v[i];
            }
            vm_sync();
            int sw = 0;
            double rat[4];
            linear_solve(M, S.at, S, C, ws, 0.0, 0, 0, 0, 0, sw, rat, nullptr);
            sync();
        }
        // LDS SoA [i][k] -> stage-major [k][i]; every index is below (N+1) * 13 resp. N * 4 of this parameter's block
        if (dxo) {
            double *o = dxo + (int64_t)q * (N + 1) * NX;
            for (int e = lane; e < (N + 1) * NX; e += WAVE)
                o[e] = (st == SENS_OK && e >= NX) ? DX[(e % NX) * SX + e / NX] : 0.0;
        }
        if (duo) {
            double *o = duo + (int64_t)q * N * NU;
            for (int e = lane; e < N * NU; e += WAVE) o[e] = (st == SENS_OK) ? DU[(e % NU) * SX + e / NU] : 0.0;
        }
    }
    return st;
}
