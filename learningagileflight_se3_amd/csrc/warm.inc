// warm.inc — start of an instance from a saved optimum record instead of the cold initial point (lafse3_ocp_solve_warm;
// #included by ipm_kernel.hip before run_instance, compiled into ipm_kernel_warm only: run_instance<.., .., WARM>).
//
// The record is the one rec_store writes (REC_*): the inverse of dump_point, with the stage remap of a receding
// horizon.  With j = k + shift
//   x_k (k >= 1) and the omega duals of stage k   <- the record's stage min(j, N)
//   u_k, lam_k and the u duals of stage k         <- the record's stage min(j, N - 1)   (the tail repeats the last stage)
//   x_0 = the new ini_state, omega duals of stage 0 = 0 (the stage is fixed).
// Three passes, each a strided walk over the destination elements e = k * width + i, lane after lane: a wave reads 64
// consecutive doubles of the record (coalesced; in the clamped tail the same few lines again) and writes the SoA
// arrays [i][k] at stride SX, dump_point's pattern mirrored.
//   warm_usable        the vote: scalars first, then every entry the other two passes will read is finite.  Nothing
//                      is written before it, so an unusable record leaves the instance to the cold fill untouched.
//   warm_load_primal   x, u with IPOPT's warm_start_bound_push / _frac against the relaxed bounds (the cold start's
//                      formula, its 1e-2 replaced), and everything else the cold fill writes: the step and lam+ zeroed,
//                      the stage weights S.wk.
//   warm_load_duals    after the objective scaling s_new of the loaded point is known: the record's multipliers belong
//                      to the problem scaled by s_rec, so lam = lam_rec (s_new / s_rec) and
//                      z = max(z_rec (s_new / s_rec), mult_bound_push).
// The filter needs no reset (nfilt = 0 at the start of every solve); S.P, the sweeps' scratch in Smem's W / M union
// and the refinement arrays of the workspace are written by each linear_solve before it reads them, as after a cold fill.

// third argument of ipm_kernel_warm.  Not part of KernelArgs or ExtArgs, as RestoDumpArgs.
struct WarmArgs {
    const double *rec_in;           // B x REC_W (may alias ExtArgs::rec: an instance reads its record before rec_store)
    int32_t *warm_out;              // B: 0 started from the record, 1 the record was unusable and the start was cold
    int32_t shift;                  // stages the record is advanced by, >= 0
    double mu_init;                 // barrier parameter of a warm start (the host has resolved <= 0 to prm.mu_init)
    double bound_push, bound_frac;  // IPOPT warm_start_bound_push / _frac
    double mult_bound_push;         // IPOPT warm_start_mult_bound_push
};

__device__ inline int warm_src(int k, int shift, int last) { return (k + shift < last) ? k + shift : last; }

// 1 when the record can start this instance (wave-uniform).  The scalars decide first: nothing is read by horizon from
// a record of another horizon.
__device__ __noinline__ int warm_usable(const gdouble *rec, int N, int shift)
{
    const int lane = lane_id();
    const double mu = rec[REC_MU], s = rec[REC_S], st = rec[REC_STATUS];
    int ok = (rec[REC_N] == (double)N) && (st == 0.0 || st == 1.0) && (mu > 0.0) && isfinite(mu) && (s > 0.0) &&
             isfinite(s);
    ok = __builtin_amdgcn_readfirstlane(ok);   // every lane read the same words
    if (!ok) return 0;
    const int kx = warm_src(1, shift, N), ku = warm_src(0, shift, N - 1);   // first stages read
    int fin = 1;
    for (int e = kx * NX + lane; e < (N + 1) * NX; e += WAVE) fin &= (int)isfinite(rec[REC_X + e]);
    for (int e = ku * NX + lane; e < N * NX; e += WAVE) fin &= (int)isfinite(rec[REC_LAM + e]);
    for (int e = ku * NU + lane; e < N * NU; e += WAVE)
        fin &= (int)(isfinite(rec[REC_U + e]) && isfinite(rec[REC_ZLU + e]) && isfinite(rec[REC_ZUU + e]));
    for (int e = kx * 3 + lane; e < (N + 1) * 3; e += WAVE)
        fin &= (int)(isfinite(rec[REC_ZLW + e]) && isfinite(rec[REC_ZUW + e]));
    return __builtin_amdgcn_readfirstlane(__all(fin) ? 1 : 0);
}

// wk: the stage weight's peak and decay of this instance (ExtArgs::weights or the context's)
__device__ __noinline__ void warm_load_primal(Smem &S, const gdouble *rec, const double *ini, int shift, double push,
                                              double frac, double dt, double tt, double w_peak, double w_decay)
{
    const int lane = lane_id();
    const Ctl &C = S.C;
    const int N = C.N;
    const double upl = fmin(push * fmax(1.0, fabs(C.ulo)), frac * (C.uhi - C.ulo));
    const double upu = fmin(push * fmax(1.0, fabs(C.uhi)), frac * (C.uhi - C.ulo));
    const double wpl = fmin(push * fmax(1.0, fabs(C.wlo)), frac * (C.whi - C.wlo));
    const double wpu = fmin(push * fmax(1.0, fabs(C.whi)), frac * (C.whi - C.wlo));
    for (int e = lane; e < (N + 1) * NX; e += WAVE) {
        const int k = e / NX, i = e % NX;
        double v;
        if (k == 0) {
            v = ini[i];
        } else {
            v = rec[REC_X + warm_src(k, shift, N) * NX + i];
            if (i >= 10) v = fmin(fmax(v, C.wlo + wpl), C.whi - wpu);
        }
        S.x[i * SX + k] = v;
        S.dx[i * SX + k] = 0.0;
    }
    for (int e = lane; e < N * NU; e += WAVE) {
        const int k = e / NU, a = e % NU;
        const double v = rec[REC_U + warm_src(k, shift, N - 1) * NU + a];
        S.u[a * SX + k] = fmin(fmax(v, C.ulo + upl), C.uhi - upu);
        S.du[a * SX + k] = 0.0;
    }
    for (int e = lane; e < N * NX; e += WAVE) S.lamp[(e % NX) * SX + e / NX] = 0.0;
    if (lane <= N) {
        const double dtk = dt * lane - tt;
        S.wk[lane] = w_peak * exp(-w_decay * dtk * dtk);
    }
}

// r = s_new / s_rec
__device__ __noinline__ void warm_load_duals(Smem &S, gdouble *ws, const gdouble *rec, int shift, double r, double mbp)
{
    const int lane = lane_id();
    const int N = S.C.N;
    WS_TRAJ(ws);
    for (int e = lane; e < N * NX; e += WAVE) {
        const int k = e / NX, i = e % NX;
        LAM[i * SX + k] = rec[REC_LAM + warm_src(k, shift, N - 1) * NX + i] * r;
    }
    for (int e = lane; e < N * NU; e += WAVE) {
        const int k = e / NU, a = e % NU, src = warm_src(k, shift, N - 1) * NU + a;
        ZLU[a * SX + k] = fmax(rec[REC_ZLU + src] * r, mbp);
        ZUU[a * SX + k] = fmax(rec[REC_ZUU + src] * r, mbp);
    }
    for (int e = lane; e < (N + 1) * 3; e += WAVE) {
        const int k = e / 3, c = e % 3, src = warm_src(k, shift, N) * 3 + c;
        ZLW[c * SX + k] = (k >= 1) ? fmax(rec[REC_ZLW + src] * r, mbp) : 0.0;
        ZUW[c * SX + k] = (k >= 1) ? fmax(rec[REC_ZUW + src] * r, mbp) : 0.0;
    }
}
