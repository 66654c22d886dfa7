// vjp.inc — one-sweep adjoint of the optimum's sensitivities from a saved optimum record (lafse3_ocp_vjp; #included by
// ipm_kernel.hip after the solver kernels; vjp_kernel is no instantiation of run_instance).
//
//   grad[q] = sum_k g_x[k] . dx*_k/dparam_q + sum_k g_u[k] . du*_k/dparam_q      for every selected column q
//
// The forward route (sens.inc) computes dz*/dparam_q = -K^{-1} c_q with one sweep per column.  K is symmetric, so
//   g^T (-K^{-1} c_q) = (-K^{-1} g)^T c_q = d . c_q,       d = the sweep on the right-hand side r = g,
// which is sens.inc's adjoint route with the unit vector e_(u_0, a) replaced by the incoming gradient: g_x of
// stages 1..N in the x rows (WS_RQ), g_u in the u rows (WS_RR), zero in the dynamics rows (WS_RC).  One factorisation
// and one sweep per instance for any number of columns; the contraction is sens_contract, the one sens_pass's gain
// uses.  Stage 0 is not a decision variable: dx_0/dini_state is the identity, so g_x[0] is added to the ini_state
// columns directly (sens_contract's gx0).
//
// The point comes from the record ipm_kernel_ext stored (REC_*), not from a solve on this wave: the instance prologue
// of run_instance (Model and the weight row, attitude forms, S.wk, relaxed bounds, goal / p_tra / u_last) is repeated
// here from the same arguments, then x, u, the scaled lam, the bound duals, mu and the objective scaling are loaded.
constexpr int VJP_HORIZON = 3;   // sens_status: the record's horizon is not the context's

struct VjpArgs {
    lafse3_params prm;
    int64_t n_inst;
    const double *goal, *ptra, *atra, *t, *ulast;   // as KernelArgs (ini_state is stage 0 of the record's x)
    const double *weights;                          // B x LAFSE3_NW or null, as ExtArgs
    const double *rec;                              // B x REC_W
    const double *gx, *gu;                          // B x (N+1) x 13, B x N x 4 (each nullable: zero)
    double *grad;                                   // B x P
    int32_t *sens_out;                              // B (nullable)
    int32_t groups;                                 // LAFSE3_SENS_THETA | _INI | _GOAL | _WEIGHTS
    unsigned long long *counters;                   // [3] the work-queue head
    double *ws;
};

__device__ __attribute__((always_inline)) inline void vjp_instance(const VjpArgs &A, Smem &S, const int64_t inst,
                                                                   gdouble *ws)
{
    const int lane = lane_id();
    const lafse3_params &prm = A.prm;
    const int N = prm.horizon;
    const int groups = A.groups;
    const int P = sens_columns(groups);
    const double *rec = A.rec + inst * (int64_t)REC_W;
    double *o = A.grad + inst * (int64_t)P;
    // the scalars first: nothing is read by horizon from a record of another horizon
    int st = SENS_OK;
    if (!(rec[REC_STATUS] >= 0.0 && rec[REC_STATUS] <= 1.0)) st = SENS_UNCONVERGED;
    if (!(rec[REC_N] == (double)N)) st = VJP_HORIZON;
    st = __builtin_amdgcn_readfirstlane(st);   // every lane read the same words: uniform for the compiler too

    if (st == SENS_OK) {
        // ---- instance prologue (run_instance, MODE_SOLVE with EXT)
        Model &M = S.mdl;
        M = make_model(prm);
        double w_peak = prm.tra_w_peak, w_decay = prm.tra_w_decay;
        if (A.weights) {
            const double *w = A.weights + inst * (int64_t)NW;
            M.wrt = w[W_WRT]; M.wqt = w[W_WQT]; M.wthrust = w[W_WTHRUST]; M.wrf = w[W_WRF]; M.wvf = w[W_WVF];
            M.wqf = w[W_WQF]; M.wwf = w[W_WWF]; M.du_w = w[W_DU];
            w_peak = uniform(w[W_PEAK]);
            w_decay = uniform(w[W_DECAY]);
        }
        WS_TRAJ(ws);
        // Whatever the contraction at the end reads of this prologue is wave-uniform and kept in SGPRs (uniform()), or
        // in LDS: the loops below retire their lanes one by one, and the compiler has parked vector registers that
        // live across such a loop in AGPRs at its exit before the lanes were switched on again (tra_w_decay and
        // dt k - t came back as garbage in the weight columns).  The contraction forms its per-lane values afresh.
        double p3[3], a3[3], q4[4];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            p3[i] = uniform(A.ptra[inst * 3 + i]);
            a3[i] = uniform(A.atra[inst * 3 + i]);
        }
        const double tt = uniform(A.t[inst]);
        rd2quat(magni3(a3), a3, q4);
        Ctl &C = S.C;
        C.N = N;
        C.ulo = prm.u_lb - prm.bound_relax * fmax(1.0, fabs(prm.u_lb));
        C.uhi = prm.u_ub + prm.bound_relax * fmax(1.0, fabs(prm.u_ub));
        C.wlo = prm.w_lb - prm.bound_relax * fmax(1.0, fabs(prm.w_lb));
        C.whi = prm.w_ub + prm.bound_relax * fmax(1.0, fabs(prm.w_ub));
        C.s = uniform(rec[REC_S]);
        C.mu = uniform(rec[REC_MU]);
#ifdef LAFSE3_PHASE_TIMERS
        S.timing = 0;
#endif
        if (lane < 3) {
            S.goal[lane] = A.goal[inst * 3 + lane];
            S.ptra[lane] = p3[lane];
        }
        if (lane < 4) S.ulast[lane] = A.ulast ? A.ulast[inst * 4 + lane] : 0.0;
        Attitude &at = S.at;
        {
            double Rt[9], Rg[9], St[16], Sg[16];
            dcm(q4, Rt);
            attitude_form(Rt, St);
            const double qg[4] = {1, 0, 0, 0};
            dcm(qg, Rg);
            attitude_form(Rg, Sg);
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    at.St[i] = St[i];
                    at.Sg[i] = Sg[i];
                }
                at.trRt = Rt[0] + Rt[4] + Rt[8];
                at.trRg = Rg[0] + Rg[4] + Rg[8];
            }
        }
        // ---- the record: stage-major [k][i] -> SoA [i][k]; every index is below the block's (N+1) or N rows
        for (int e = lane; e < (N + 1) * NX; e += WAVE) S.x[(e % NX) * SX + e / NX] = rec[REC_X + e];
        for (int e = lane; e < N * NU; e += WAVE) {
            S.u[(e % NU) * SX + e / NU] = rec[REC_U + e];
            ZLU[(e % NU) * SX + e / NU] = rec[REC_ZLU + e];
            ZUU[(e % NU) * SX + e / NU] = rec[REC_ZUU + e];
        }
        for (int e = lane; e < N * NX; e += WAVE) LAM[(e % NX) * SX + e / NX] = rec[REC_LAM + e];
        for (int e = lane; e < (N + 1) * 3; e += WAVE) {
            ZLW[(e % 3) * SX + e / 3] = rec[REC_ZLW + e];
            ZUW[(e % 3) * SX + e / 3] = rec[REC_ZUW + e];
        }
        for (int e = lane; e < NX * SX; e += WAVE) {
            DX[e] = 0.0;
            LP[e] = 0.0;
        }
        for (int e = lane; e < NU * SX; e += WAVE) DU[e] = 0.0;
        if (lane <= N) {
            const double dtk = prm.dt * lane - tt;
            S.wk[lane] = w_peak * exp(-w_decay * dtk * dtk);   // run_instance's expression
        }
        vm_sync();

        // ---- factorise at the recorded point, as sens_pass does
        int sw = 0;
        double rat[4];
        if (!linear_solve(M, S.at, S, C, ws, 0.0, 1, 0, 0, 0, sw, rat, nullptr)) st = SENS_INERTIA;
        if (st == SENS_OK) {
            // ---- right-hand side: g_x of stages 1..N in the x rows, g_u in the u rows, no dynamics rows
            gdouble *rq = ws + WS_RQ, *rr = ws + WS_RR, *rc = ws + WS_RC;
            const double *gx = A.gx ? A.gx + inst * (int64_t)(N + 1) * NX : nullptr;
            const double *gu = A.gu ? A.gu + inst * (int64_t)N * NU : nullptr;
            for (int e = lane; e < NX * SX; e += WAVE) {
                const int i = e / SX, k = e % SX;
                rq[e] = (gx && k >= 1 && k <= N) ? gx[k * NX + i] : 0.0;
                rc[e] = 0.0;
            }
            for (int e = lane; e < NU * SX; e += WAVE) {
                const int a = e / SX, k = e % SX;
                rr[e] = (gu && k < N) ? gu[k * NU + a] : 0.0;
            }
            vm_sync();
            linear_solve(M, S.at, S, C, ws, 0.0, 0, 0, 0, 0, sw, rat, nullptr);
            sync();
            // ---- contraction with dF/dparam_q, column by column
            // nothing per-lane is carried over from before the sweep (see above); the mask keeps the index's range
            // known, which the shared inline helpers' compares are specialised on in every kernel
            const int lane = opaque_lane() & (WAVE - 1);
            sens_contract(M, S, C, a3, prm.dt, w_decay, tt, groups, lane, gx, o);
        }
    }
    if (st != SENS_OK)
        for (int e = lane; e < P; e += WAVE) o[e] = 0.0;
    if (lane == 0 && A.sens_out) A.sens_out[inst] = st;
    sync();   // the next instance's prologue writes the LDS this one's last lanes may still read
}

// One wave per instance, the persistent queue-head loop and workspace slots of ipm_kernel_ext.
__global__ __launch_bounds__(64, 1) void vjp_kernel(VjpArgs A)
{
    Smem &S = instance_smem();
    init_mf_tables(S);   // linear_solve's factorisation sweep reads them
    gdouble *ws = (gdouble *)(A.ws + slot_id() * (int64_t)WS_SIZE);
    for (;;) {
        unsigned long long v = 0ull;
        if (lane_id() == 0) v = atomicAdd(&A.counters[3], 1ull);
        const int64_t inst = bcast_i64((int64_t)v);
        if (inst >= A.n_inst) break;
        typedef const VjpArgs __attribute__((address_space(4))) *KArgPtr;   // as in ipm_kernel
        KArgPtr Ap = (KArgPtr)__builtin_amdgcn_kernarg_segment_ptr();
        __asm__ volatile("" : "+s"(Ap));
        vjp_instance(*(const VjpArgs *)Ap, S, inst, ws);
    }
}
