// resto.inc — IPOPT's restoration phase on the device (included by ipm_kernel.hip after the IPM phases).
//
// Same algorithm, decisions and order as oracle/lafse3_oracle.c orc_restoration (IPOPT 3.12
// RestoIpoptNLP / RestoIterateInitializer / RestoFilterConvergenceCheck): when the filter line search and the
// soft restoration phase both fail, the wave solves
//     min  rho sum(p + n) + eta/2 ||D_R (v - v_R)||^2     s.t.  f_d(x_k, u_k) - x_{k+1} - p_k + n_k = 0,  p, n >= 0
// (rho = 1000, eta = sqrt(mu_R), D_R = min(1, 1/|v_R|), v_R the start point) with the same primal-dual IPM until
// a point acceptable to the original filter with theta <= 0.9 theta_start appears.
//
// Newton system of the restoration problem: eliminating p, n leaves the original Riccati structure with a
// SOFT dynamics constraint, x_{k+1} = A x + B u + c' - D lam_k (D = 1/Sp' + 1/Sn' per row).  The backward sweep
// maps the value function (P, p) of x_{k+1} through it (S' = I + D^1/2 P D^1/2, a 13 x 13 Cholesky per stage, lane-
// parallel left-looking) and then runs the plain dense Riccati stage; there is no du smoothing term in the
// restoration objective, so the u_prev augmentation of the main sweep is identically zero and the state is 13-wide.
// This phase is rare (0.05 % of the bench's solves, a few to ~15 iterations each), so it is written for clarity
// and lane parallelism, not for the cycle budget of the main sweep: stage matrices are dense in LDS (the main
// sweep's stage working set, free while the phase runs), per-stage records go to the restoration workspace
// (KernelArgs::rws, offset R_STG).

constexpr double RESTO_RHO = 1000.0;

// LDS scratch (S.rw, in the union with the main sweep's W / M): stage matrices of the restoration sweep
constexpr int RW_A = 0, RW_B = 169, RW_Q = 221, RW_S = 390, RW_PA = 442, RW_PB = 611, RW_QX = 663, RW_K = 715;
constexpr int RW_L = 0, RW_X = 169;     // transform: L (13 x 13) and X (13 x 14) alias A, B, Q
static_assert(RW_K + NU * NX <= RW_SIZE, "resto scratch");
static_assert(RW_X + NX * (NX + 1) <= RW_PA, "transform scratch");
// small vectors: S.vec = c' | D | sqrt(D); S.hv = q | r | R | qu | kff | ph; S.cc = Quu; S.hh[0] = pivot
constexpr int V_C = 0, V_D = 16, V_S = 32;
constexpr int HV_Q = 0, HV_R = 16, HV_RD = 20, HV_QU = 24, HV_KF = 28, HV_PH = 32;

// packed lower triangle of a symmetric / lower 13 x 13
__device__ inline int tri13(int i, int j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }
__device__ inline void tri13_rc(int e, int &i, int &j)
{
    int r = 0;
    while ((r + 1) * (r + 2) / 2 <= e) ++r;
    i = r;
    j = e - r * (r + 1) / 2;
}
// v[i] for a lane-dependent i without dynamic register indexing (a select chain)
__device__ inline double sel13(const double *v, int i)
{
    double r = v[0];
#pragma unroll
    for (int m = 1; m < NX; ++m) r = (i == m) ? v[m] : r;
    return r;
}

// p / n row data of constraint row idx = i * SX + k (oracle resto_pn_terms)
struct PNRow {
    double Sp, Sn, rp, rn;
};
__device__ inline PNRow pn_terms(const gdouble *rs, int idx, double mu, double dw, int lsq, int refine)
{
    PNRow t;
    const double zp = rs[R_ZP + idx], zn = rs[R_ZN + idx];
    if (lsq) {
        t.Sp = 1.0;
        t.Sn = 1.0;
        t.rp = RESTO_RHO - zp;
        t.rn = RESTO_RHO - zn;
        return t;
    }
    const double p = rs[R_P + idx], n = rs[R_N + idx];
    t.Sp = zp / p + dw;
    t.Sn = zn / n + dw;
    if (refine) {
        t.rp = rs[R_RP + idx];
        t.rn = rs[R_RN + idx];
    } else {
        t.rp = RESTO_RHO - mu / p;
        t.rn = RESTO_RHO - mu / n;
    }
    return t;
}

// 4 x 4 Cholesky with reciprocal diagonal in L[16..19] (oracle chol4 / chol4_solve, same operation order)
__device__ inline int chol4_o(const double *M, double *L)
{
#pragma unroll
    for (int e = 0; e < 20; ++e) L[e] = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double d = M[j * 4 + j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[j * 4 + k] * L[j * 4 + k];
        if (!(d > 0.0)) return 0;
        const double ljj = sqrt(d);
        L[j * 4 + j] = ljj;
        L[16 + j] = 1.0 / ljj;
#pragma unroll
        for (int i = j + 1; i < 4; ++i) {
            double s = M[i * 4 + j];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= L[i * 4 + k] * L[j * 4 + k];
            L[i * 4 + j] = s * L[16 + j];
        }
    }
    return 1;
}
__device__ inline void chol4_solve_o(const double *L, double *b)
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double s = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= L[i * 4 + k] * b[k];
        b[i] = s * L[16 + i];
    }
#pragma unroll
    for (int i = 3; i >= 0; --i) {
        double s = b[i];
#pragma unroll
        for (int k = i + 1; k < 4; ++k) s -= L[k * 4 + i] * b[k];
        b[i] = s * L[16 + i];
    }
}

// dense stage QP of the restoration problem at stage k (oracle build_stage_resto): A, B, Q, S_xu into S.rw,
// q, r, diag R into S.hv.  Lanes 0..12 build the columns of A, 13..16 of B, 17..29 of the lambda-Hessian, 30..33
// of S_xu; then lanes 0..12 the diagonal and q, lanes 13..16 R and r.
__device__ void resto_stage(const Model &M, const Attitude &at, Smem &S, const Ctl &C, gdouble *ws, gdouble *rs, int k, double mu,
                            double eta, double dw, int lsq, int refine)
{
    WS_TRAJ(ws);
    const int lane = lane_id();
    double *rw = S.rw;
    double xk[NX], uk[NU];
    load_stage(S, k, xk);
    load_u(S, k, uk);
    const bool hl = (k >= 1) && !lsq;
    StageHess H;
    if (hl) {
        double lk[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) lk[i] = LAM[i * SX + k];
        stage_hessian(M, at, 0.0, 0.0, xk, uk, lk, H);   // s = 0, wk = 0: the lambda part alone
    }
    double o[NX];
    if (lane < NX) {
        double e[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) e[i] = (i == lane) ? 1.0 : 0.0;
        A_times(M, xk, uk, e, o);
#pragma unroll
        for (int m = 0; m < NX; ++m) rw[RW_A + m * NX + lane] = o[m];
    } else if (lane < NX + NU) {
        const int a = lane - NX;
        double e[NU];
#pragma unroll
        for (int b = 0; b < NU; ++b) e[b] = (b == a) ? 1.0 : 0.0;
        B_times(M, xk, e, o);
#pragma unroll
        for (int m = 0; m < NX; ++m) rw[RW_B + m * NU + a] = o[m];
    } else if (lane < 2 * NX + NU) {
        const int j = lane - NX - NU;
        if (hl) {
            double e[NX];
#pragma unroll
            for (int i = 0; i < NX; ++i) e[i] = (i == j) ? 1.0 : 0.0;
            Hxx_times(H, e, o);
        } else {
#pragma unroll
            for (int m = 0; m < NX; ++m) o[m] = 0.0;
        }
#pragma unroll
        for (int m = 0; m < NX; ++m) rw[RW_Q + m * NX + j] = o[m];
    } else if (lane < 2 * NX + 2 * NU) {
        const int a = lane - 2 * NX - NU;
#pragma unroll
        for (int m = 0; m < NX; ++m) rw[RW_S + m * NU + a] = (hl && m >= 6 && m <= 9) ? H.qu[m - 6] : 0.0;
    }
    sync();
    if (lane < NX) {
        const int i = lane, idx = i * SX + k;
        double qi = 0.0;
        if (k >= 1) {
            const double d2 = rs[R_DX2 + idx], v = S.x[idx];
            qi = eta * d2 * (v - rs[R_XR + idx]);
            double qd = rw[RW_Q + i * NX + i] + (lsq ? 1.0 : eta * d2 + dw);
            if (i >= 10) {
                const int c = i - 10;
                const double zl = ZLW[c * SX + k], zu = ZUW[c * SX + k];
                if (lsq) {
                    qi += -zl + zu;
                } else {
                    double gb, sg;
                    bar_terms(v, C.wlo, C.whi, zl, zu, mu, gb, sg);
                    qd += sg;
                    qi += gb;
                }
            }
            rw[RW_Q + i * NX + i] = qd;
        }
        if (refine) qi = (k >= 1) ? ws[WS_RQ + idx] : 0.0;
        S.hv[HV_Q + i] = qi;
    } else if (lane < NX + NU) {
        const int a = lane - NX, idx = a * SX + k;
        const double v = S.u[idx], d2 = rs[R_DU2 + idx];
        const double zl = ZLU[idx], zu = ZUU[idx];
        double ra = eta * d2 * (v - rs[R_UR + idx]), Ra;
        if (lsq) {
            Ra = 1.0;
            ra += -zl + zu;
        } else {
            double gb, sg;
            bar_terms(v, C.ulo, C.uhi, zl, zu, mu, gb, sg);
            Ra = eta * d2 + sg + dw;
            ra += gb;
        }
        if (refine) ra = ws[WS_RR + idx];
        S.hv[HV_R + a] = ra;
        S.hv[HV_RD + a] = Ra;
    }
    sync();
}

// Newton step of the restoration problem (oracle riccati_resto): fills DX, DU, LP (lam+), R_DP, R_DN.  lsq: the
// least-squares multiplier system of the start point; refine: right-hand sides from the residual (WS_RQ / RR / RC,
// R_RP / RN).  Returns 0 on wrong inertia (S' or Quu not positive definite), uniform across the wave.
__device__ __noinline__ int resto_riccati(const Model &M, const Attitude &at, Smem &S, const Ctl &C, gdouble *ws, gdouble *rs,
                                          double mu, double eta, double dw, int lsq, int refine)
{
    WS_TRAJ(ws);
    const int lane = lane_id();
    const int N = C.N;
    double *P = S.P, *p = S.p, *rw = S.rw;   // value function of x_{k+1}: P 13 x 13 row-major, p 13
    // terminal value function (oracle build_terminal_resto)
    if (lane < NX) {
        const int i = lane, idx = i * SX + N;
        const double d2 = rs[R_DX2 + idx], v = S.x[idx];
        double pi = eta * d2 * (v - rs[R_XR + idx]);
        double Pd = lsq ? 1.0 : eta * d2 + dw;
        if (i >= 10) {
            const int c = i - 10;
            const double zl = ZLW[c * SX + N], zu = ZUW[c * SX + N];
            if (lsq) {
                pi += -zl + zu;
            } else {
                double gb, sg;
                bar_terms(v, C.wlo, C.whi, zl, zu, mu, gb, sg);
                Pd += sg;
                pi += gb;
            }
        }
        if (refine) pi = ws[WS_RQ + idx];
        p[i] = pi;
#pragma unroll
        for (int j = 0; j < NX; ++j) P[i * NX + j] = (j == i) ? Pd : 0.0;
    }
    sync();
    for (int k = N - 1; k >= 0; --k) {
        gdouble *rec = rs + R_STG + k * RS_STG;
        // (0) P_{k+1}, p_{k+1} for the forward sweep; c', D, sqrt(D) of the stage's soft constraint
        for (int e = lane; e < 91 + NX; e += WAVE) {
            double v;
            if (e < 91) {
                int i, j;
                tri13_rc(e, i, j);
                v = P[i * NX + j];
            } else {
                v = p[e - 91];
            }
            rec[RS_PK + e] = v;   // RS_PV follows RS_PK
        }
        if (lane < NX) {
            const int i = lane, idx = i * SX + k;
            const PNRow t = pn_terms(rs, idx, mu, dw, lsq, refine);
            double c = 0.0;
            if (!lsq) {
                if (refine) {
                    c = ws[WS_RC + idx];
                } else {
                    double xk[NX], uk[NU], xn[NX];
                    load_stage(S, k, xk);
                    load_u(S, k, uk);
                    f_disc(M, xk, uk, xn);
                    c = sel13(xn, i) - S.x[i * SX + k + 1] - rs[R_P + idx] + rs[R_N + idx];
                }
            }
            const double cp = c + t.rp / t.Sp - t.rn / t.Sn;
            const double D = 1.0 / t.Sp + 1.0 / t.Sn;
            S.vec[V_C + i] = cp;
            S.vec[V_D + i] = D;
            S.vec[V_S + i] = sqrt(D);
            rs[R_D + idx] = D;
            rs[R_C + idx] = cp;
        }
        sync();
        // (T) value function through the soft constraint (oracle resto_transform)
        for (int e = lane; e < NX * NX; e += WAVE) {
            const int i = e / NX, j = e % NX;
            rw[RW_L + e] = (i == j ? 1.0 : 0.0) + S.vec[V_S + i] * P[e] * S.vec[V_S + j];
        }
        sync();
        for (int j = 0; j < NX; ++j) {   // left-looking Cholesky, column j: lane i >= j reduces row i
            double t = 0.0;
            if (lane >= j && lane < NX) {
                t = rw[RW_L + lane * NX + j];
                for (int m = 0; m < j; ++m) t -= rw[RW_L + lane * NX + m] * rw[RW_L + j * NX + m];
            }
            if (lane == j) S.hh[0] = t;
            sync();
            const double d = S.hh[0];
            if (!(d > 0.0)) return 0;
            const double ljj = sqrt(d);
            if (lane == j) rw[RW_L + j * NX + j] = ljj;
            else if (lane > j && lane < NX) rw[RW_L + lane * NX + j] = t / ljj;
            sync();
        }
        if (lane < NX + 1) {   // X = S'^-1 diag(s) [P | p], lane = column
            const int c = lane;
            double b[NX];
#pragma unroll
            for (int i = 0; i < NX; ++i) b[i] = S.vec[V_S + i] * (c < NX ? P[i * NX + c] : p[i]);
#pragma unroll
            for (int i = 0; i < NX; ++i) {
                double s = b[i];
#pragma unroll
                for (int m = 0; m < i; ++m) s -= rw[RW_L + i * NX + m] * b[m];
                b[i] = s / rw[RW_L + i * NX + i];
            }
#pragma unroll
            for (int i = NX - 1; i >= 0; --i) {
                double s = b[i];
#pragma unroll
                for (int m = i + 1; m < NX; ++m) s -= rw[RW_L + m * NX + i] * b[m];
                b[i] = s / rw[RW_L + i * NX + i];
            }
#pragma unroll
            for (int i = 0; i < NX; ++i) rw[RW_X + i * (NX + 1) + c] = b[i];
        }
        sync();
        for (int e = lane; e < NX * NX; e += WAVE) {
            const int i = e / NX, j = e % NX;
            P[e] = 0.5 * (rw[RW_X + i * (NX + 1) + j] / S.vec[V_S + i] + rw[RW_X + j * (NX + 1) + i] / S.vec[V_S + j]);
        }
        if (lane < NX) p[lane] = rw[RW_X + lane * (NX + 1) + NX] / S.vec[V_S + lane];
        for (int e = lane; e < 91 + NX; e += WAVE) {
            double v;
            if (e < 91) {
                int i, j;
                tri13_rc(e, i, j);
                v = rw[RW_L + i * NX + j];
            } else {
                v = S.vec[V_S + e - 91];
            }
            rec[RS_L + e] = v;   // RS_SD follows RS_L
        }
        sync();
        // (B) the stage QP; (R) the dense Riccati stage on the transformed value function (oracle riccati_resto)
        resto_stage(M, at, S, C, ws, rs, k, mu, eta, dw, lsq, refine);
        for (int e = lane; e < NX * NX + NX * NU + NX; e += WAVE) {
            if (e < NX * NX) {
                const int i = e / NX, j = e % NX;
                double acc = 0.0;
#pragma unroll
                for (int m = 0; m < NX; ++m) acc += P[i * NX + m] * rw[RW_A + m * NX + j];
                rw[RW_PA + e] = acc;
            } else if (e < NX * NX + NX * NU) {
                const int f = e - NX * NX, i = f / NU, a = f % NU;
                double acc = 0.0;
#pragma unroll
                for (int m = 0; m < NX; ++m) acc += P[i * NX + m] * rw[RW_B + m * NU + a];
                rw[RW_PB + f] = acc;
            } else {
                const int i = e - NX * NX - NX * NU;
                double acc = p[i];
#pragma unroll
                for (int m = 0; m < NX; ++m) acc += P[i * NX + m] * S.vec[V_C + m];
                S.hv[HV_PH + i] = acc;
            }
        }
        sync();
        for (int e = lane; e < NU * NU + NU * NX + NU; e += WAVE) {
            if (e < NU * NU) {
                const int a = e / NU, b = e % NU;
                double acc = (a == b) ? S.hv[HV_RD + a] : 0.0;
#pragma unroll
                for (int m = 0; m < NX; ++m) acc += rw[RW_B + m * NU + a] * rw[RW_PB + m * NU + b];
                S.cc[e] = acc;
            } else if (e < NU * NU + NU * NX) {
                const int f = e - NU * NU, a = f / NX, j = f % NX;
                double acc = rw[RW_S + j * NU + a];
#pragma unroll
                for (int m = 0; m < NX; ++m) acc += rw[RW_B + m * NU + a] * rw[RW_PA + m * NX + j];
                rw[RW_QX + f] = acc;
            } else {
                const int a = e - NU * NU - NU * NX;
                double acc = S.hv[HV_R + a];
#pragma unroll
                for (int m = 0; m < NX; ++m) acc += rw[RW_B + m * NU + a] * S.hv[HV_PH + m];
                S.hv[HV_QU + a] = acc;
            }
        }
        sync();
        {
            double Q4[16], Lq[20];
#pragma unroll
            for (int e = 0; e < 16; ++e) Q4[e] = S.cc[e];
#pragma unroll
            for (int a = 0; a < NU; ++a)
#pragma unroll
                for (int b = a + 1; b < NU; ++b) {
                    const double v = 0.5 * (Q4[a * NU + b] + Q4[b * NU + a]);
                    Q4[a * NU + b] = Q4[b * NU + a] = v;
                }
            if (!chol4_o(Q4, Lq)) return 0;
            if (lane <= NX) {   // K column j (lane j < 13), feed-forward (lane 13)
                double col[NU];
#pragma unroll
                for (int a = 0; a < NU; ++a) col[a] = (lane < NX) ? rw[RW_QX + a * NX + lane] : S.hv[HV_QU + a];
                chol4_solve_o(Lq, col);
                if (lane < NX) {
#pragma unroll
                    for (int a = 0; a < NU; ++a) {
                        rw[RW_K + a * NX + lane] = -col[a];
                        rec[RS_K + a * NX + lane] = -col[a];
                    }
                } else {
#pragma unroll
                    for (int a = 0; a < NU; ++a) {
                        S.hv[HV_KF + a] = -col[a];
                        rec[RS_KF + a] = -col[a];
                    }
                }
            }
        }
        sync();
        for (int e = lane; e < NX * NX + NX; e += WAVE) {
            if (e < NX * NX) {
                const int i = e / NX, j = e % NX;
                double acc = rw[RW_Q + e];
#pragma unroll
                for (int m = 0; m < NX; ++m) acc += rw[RW_A + m * NX + i] * rw[RW_PA + m * NX + j];
#pragma unroll
                for (int a = 0; a < NU; ++a) acc += rw[RW_QX + a * NX + i] * rw[RW_K + a * NX + j];
                P[e] = acc;
            } else {
                const int i = e - NX * NX;
                double acc = S.hv[HV_Q + i];
#pragma unroll
                for (int m = 0; m < NX; ++m) acc += rw[RW_A + m * NX + i] * S.hv[HV_PH + m];
#pragma unroll
                for (int a = 0; a < NU; ++a) acc += rw[RW_QX + a * NX + i] * S.hv[HV_KF + a];
                p[i] = acc;
            }
        }
        sync();
        for (int e = lane; e < 91; e += WAVE) {   // symmetrise: (i, j) <-> (j, i) for the strictly lower entries
            int i, j;
            tri13_rc(e, i, j);
            if (i != j) {
                const double v = 0.5 * (P[i * NX + j] + P[j * NX + i]);
                P[i * NX + j] = v;
                P[j * NX + i] = v;
            }
        }
        sync();
    }
    vm_sync();
    // forward: du = K dx + k, y' = A dx + B du + c', dx_{k+1} = s (L L^T)^-1 (y' - D p_{k+1}) / s,
    // lam+_k = P_{k+1} dx_{k+1} + p_{k+1}, then dp, dn (all lanes run the chain; lane i stores row i)
    double dxk[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) dxk[i] = 0.0;
    if (lane < NX) DX[lane * SX] = 0.0;
    for (int k = 0; k < N; ++k) {
        const gdouble *rec = rs + R_STG + k * RS_STG;
        double xk[NX], uk[NU];
        load_stage(S, k, xk);
        load_u(S, k, uk);
        double du[NU];
#pragma unroll
        for (int a = 0; a < NU; ++a) {
            double acc = rec[RS_KF + a];
#pragma unroll
            for (int j = 0; j < NX; ++j) acc += rec[RS_K + a * NX + j] * dxk[j];
            du[a] = acc;
        }
        double adx[NX], bdu[NX], b[NX];
        A_times(M, xk, uk, dxk, adx);
        B_times(M, xk, du, bdu);
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const int idx = i * SX + k;
            const double y = rs[R_C + idx] + adx[i] + bdu[i];
            b[i] = (y - rs[R_D + idx] * rec[RS_PV + i]) / rec[RS_SD + i];
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            double s = b[i];
#pragma unroll
            for (int m = 0; m < i; ++m) s -= rec[RS_L + tri13(i, m)] * b[m];
            b[i] = s / rec[RS_L + tri13(i, i)];
        }
#pragma unroll
        for (int i = NX - 1; i >= 0; --i) {
            double s = b[i];
#pragma unroll
            for (int m = i + 1; m < NX; ++m) s -= rec[RS_L + tri13(m, i)] * b[m];
            b[i] = s / rec[RS_L + tri13(i, i)];
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) dxk[i] = rec[RS_SD + i] * b[i];
        if (lane < NX) {
            const int i = lane, idx = i * SX + k;
            DX[i * SX + k + 1] = sel13(dxk, i);
            double acc = rec[RS_PV + i];
#pragma unroll
            for (int j = 0; j < NX; ++j) acc += rec[RS_PK + tri13(i, j)] * dxk[j];
            LP[idx] = acc;
            const PNRow t = pn_terms(rs, idx, mu, dw, lsq, refine);
            rs[R_DP + idx] = (acc - t.rp) / t.Sp;
            rs[R_DN + idx] = (-acc - t.rn) / t.Sn;
        }
        if (lane < NU) DU[lane * SX + k] = (lane == 0) ? du[0] : (lane == 1) ? du[1] : (lane == 2) ? du[2] : du[3];
    }
    vm_sync();
    return 1;
}

// residual of the full restoration Newton system at (dx, du, lam+, dp, dn) (oracle kkt_residual_resto): writes
// WS_RQ / RR / RC and R_RP / RN, returns IPOPT's residual ratio.  Lane = stage k (u, dynamics, p / n and x_k rows),
// lane N the terminal x rows.
__device__ __noinline__ double resto_residual(const Model &M, const Attitude &at, Smem &S, const Ctl &C, gdouble *ws, gdouble *rs,
                                              double mu, double eta, double dw)
{
    WS_TRAJ(ws);
    const int lane = lane_id();
    const int N = C.N;
    double nres = 0.0, nsol = 0.0, nrhs = 0.0;
    if (lane < N) {
        const int k = lane;
        double xk[NX], uk[NU], dxk[NX], duk[NU], lk[NX];
        load_stage(S, k, xk);
        load_u(S, k, uk);
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            dxk[i] = DX[i * SX + k];
            lk[i] = LP[i * SX + k];
        }
#pragma unroll
        for (int a = 0; a < NU; ++a) duk[a] = DU[a * SX + k];
        StageHess H;
        if (k >= 1) {
            double lam[NX];
#pragma unroll
            for (int i = 0; i < NX; ++i) lam[i] = LAM[i * SX + k];
            stage_hessian(M, at, 0.0, 0.0, xk, uk, lam, H);
        }
        // u rows
        double btl[NU];
        Bt_times(M, xk, lk, btl);
        const double sdx = (k >= 1) ? H.qu[0] * dxk[6] + H.qu[1] * dxk[7] + H.qu[2] * dxk[8] + H.qu[3] * dxk[9] : 0.0;
#pragma unroll
        for (int a = 0; a < NU; ++a) {
            const int idx = a * SX + k;
            const double v = uk[a], d2 = rs[R_DU2 + idx];
            double gb, sg;
            bar_terms(v, C.ulo, C.uhi, ZLU[idx], ZUU[idx], mu, gb, sg);
            const double Ra = eta * d2 + sg + dw, g = eta * d2 * (v - rs[R_UR + idx]) + gb;
            const double acc = Ra * duk[a] + sdx + g + btl[a];
            ws[WS_RR + idx] = acc;
            nres = fmax(nres, fabs(acc));
            nrhs = fmax(nrhs, fabs(g));
            nsol = fmax(nsol, fabs(duk[a]));
        }
        // dynamics rows and the p / n rows
        double xn[NX], adx[NX], bdu[NX];
        f_disc(M, xk, uk, xn);
        A_times(M, xk, uk, dxk, adx);
        B_times(M, xk, duk, bdu);
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const int idx = i * SX + k;
            const double pe = rs[R_P + idx], ne = rs[R_N + idx], dpe = rs[R_DP + idx], dne = rs[R_DN + idx];
            const double c = xn[i] - S.x[i * SX + k + 1] - pe + ne;
            const double acc = c - DX[i * SX + k + 1] - dpe + dne + adx[i] + bdu[i];
            ws[WS_RC + idx] = acc;
            nres = fmax(nres, fabs(acc));
            nrhs = fmax(nrhs, fabs(c));
            nsol = fmax(nsol, fabs(lk[i]));
            const PNRow t = pn_terms(rs, idx, mu, dw, 0, 0);
            const double ap = t.Sp * dpe - lk[i] + t.rp, an = t.Sn * dne + lk[i] + t.rn;
            rs[R_RP + idx] = ap;
            rs[R_RN + idx] = an;
            nres = fmax(nres, fmax(fabs(ap), fabs(an)));
            nrhs = fmax(nrhs, fmax(fabs(t.rp), fabs(t.rn)));
            nsol = fmax(nsol, fmax(fabs(dpe), fabs(dne)));
        }
        // x_k rows (k >= 1)
        if (k >= 1) {
            double hdx[NX], atl[NX];
            Hxx_times(H, dxk, hdx);
            At_times(M, xk, uk, lk, atl);
            const double su = duk[0] + duk[1] + duk[2] + duk[3];
#pragma unroll
            for (int i = 0; i < NX; ++i) {
                const int idx = i * SX + k;
                const double d2 = rs[R_DX2 + idx], v = xk[i];
                double q = eta * d2 * (v - rs[R_XR + idx]), Qd = eta * d2 + dw;
                if (i >= 10) {
                    double gb, sg;
                    bar_terms(v, C.wlo, C.whi, ZLW[(i - 10) * SX + k], ZUW[(i - 10) * SX + k], mu, gb, sg);
                    q += gb;
                    Qd += sg;
                }
                double acc = q - LP[i * SX + k - 1] + hdx[i] + Qd * dxk[i] + atl[i];
                if (i >= 6 && i <= 9) acc += H.qu[i - 6] * su;
                ws[WS_RQ + idx] = acc;
                nres = fmax(nres, fabs(acc));
                nrhs = fmax(nrhs, fabs(q));
                nsol = fmax(nsol, fabs(dxk[i]));
            }
        }
    } else if (lane == N) {
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const int idx = i * SX + N;
            const double d2 = rs[R_DX2 + idx], v = S.x[idx];
            double pv = eta * d2 * (v - rs[R_XR + idx]), Pd = eta * d2 + dw;
            if (i >= 10) {
                double gb, sg;
                bar_terms(v, C.wlo, C.whi, ZLW[(i - 10) * SX + N], ZUW[(i - 10) * SX + N], mu, gb, sg);
                pv += gb;
                Pd += sg;
            }
            const double dxn = DX[idx];
            const double acc = pv - LP[i * SX + N - 1] + Pd * dxn;
            ws[WS_RQ + idx] = acc;
            nres = fmax(nres, fabs(acc));
            nrhs = fmax(nrhs, fabs(pv));
            nsol = fmax(nsol, fabs(dxn));
        }
    }
    nres = wmax(nres);
    nsol = wmax(nsol);
    nrhs = wmax(nrhs);
    vm_sync();
    if (nrhs + nres == 0.0) return nres;
    return nres / (fmin(nsol, 1e6 * nrhs) + nrhs);
}

// Restoration dump record (lafse3_debug_dump_resto, RD_* in ipm_kernel.hip), written by ipm_kernel_dump only.  The
// step: dx | du | lam+ | dp | dn, stage-major and padded to MAXN
__device__ __noinline__ void resto_dump_step(const Smem &S, const gdouble *rs, int N, double *out)
{
    const int lane = lane_id();
    for (int e = lane; e < (N + 1) * NX; e += WAVE) out[e] = S.dx[(e % NX) * SX + e / NX];
    out += (MAXN + 1) * NX;
    for (int e = lane; e < N * NU; e += WAVE) out[e] = S.du[(e % NU) * SX + e / NU];
    out += MAXN * NU;
    for (int e = lane; e < N * NX; e += WAVE) {
        const int idx = (e % NX) * SX + e / NX;
        out[e] = S.lamp[idx];
        out[MAXN * NX + e] = rs[R_DP + idx];
        out[2 * MAXN * NX + e] = rs[R_DN + idx];
    }
}
// the iterate the dumped system is formed at (dump_point's arrays, then p | n | z_p | z_n) and the reference point
// x_R | u_R
__device__ __noinline__ void resto_dump_point(const Smem &S, const gdouble *ws, const gdouble *rs, int N, double *out)
{
    const int lane = lane_id();
    dump_point(S, ws, N, out);
    out += DUMP_W - DUMP_STEP_W;
    for (int e = lane; e < N * NX; e += WAVE) {
        const int idx = (e % NX) * SX + e / NX;
        out[e] = rs[R_P + idx];
        out[MAXN * NX + e] = rs[R_N + idx];
        out[2 * MAXN * NX + e] = rs[R_ZP + idx];
        out[3 * MAXN * NX + e] = rs[R_ZN + idx];
    }
    out += 4 * MAXN * NX;
    for (int e = lane; e < (N + 1) * NX; e += WAVE) out[e] = rs[R_XR + (e % NX) * SX + e / NX];
    out += (MAXN + 1) * NX;
    for (int e = lane; e < N * NU; e += WAVE) out[e] = rs[R_UR + (e % NU) * SX + e / NU];
}

// Newton step with IPOPT's iterative refinement (oracle newton_step_resto); 0 on wrong inertia.  DUMP: rec (nullable)
// is the dump record of this iteration, its step the refined one when drefine; the production kernels instantiate
// DUMP = false, which compiles none of it.
template <bool DUMP>
__device__ __noinline__ int resto_newton(const Model &M, const Attitude &at, Smem &S, const Ctl &C, gdouble *ws, gdouble *rs,
                                         double mu, double eta, double dw, int &sweeps, [[maybe_unused]] double *rec = nullptr,
                                         [[maybe_unused]] int drefine = 0)
{
    WS_TRAJ(ws);
    const int lane = lane_id();
    const int ok = resto_riccati(M, at, S, C, ws, rs, mu, eta, dw, 0, 0);
    sweeps++;
    if (!ok) return 0;
    if constexpr (DUMP)
        if (rec && !drefine) resto_dump_step(S, rs, C.N, rec);
    double ratio = resto_residual(M, at, S, C, ws, rs, mu, eta, dw);
    [[maybe_unused]] const double ratio_pre = ratio;
    gdouble *bdx = ws + WS_BDX, *bdu = ws + WS_BDU, *blp = ws + WS_BLP, *bdp = rs + R_BP, *bdn = rs + R_BN;
    for (int step = 0; step < 10; ++step) {
        if (step >= 1 && ratio <= 1e-10) break;
        for (int e = lane; e < NX * SX; e += WAVE) {
            bdx[e] = DX[e];
            blp[e] = LP[e];
            bdp[e] = rs[R_DP + e];
            bdn[e] = rs[R_DN + e];
        }
        for (int e = lane; e < NU * SX; e += WAVE) bdu[e] = DU[e];
        vm_sync();
        resto_riccati(M, at, S, C, ws, rs, mu, eta, dw, 0, 1);
        sweeps++;
        for (int e = lane; e < NX * SX; e += WAVE) {
            DX[e] = bdx[e] + DX[e];
            LP[e] = blp[e] + LP[e];
            rs[R_DP + e] = bdp[e] + rs[R_DP + e];
            rs[R_DN + e] = bdn[e] + rs[R_DN + e];
        }
        for (int e = lane; e < NU * SX; e += WAVE) DU[e] = bdu[e] + DU[e];
        vm_sync();
        const double nr = resto_residual(M, at, S, C, ws, rs, mu, eta, dw);
        if (!(nr < ratio)) {
            for (int e = lane; e < NX * SX; e += WAVE) {
                DX[e] = bdx[e];
                LP[e] = blp[e];
                rs[R_DP + e] = bdp[e];
                rs[R_DN + e] = bdn[e];
            }
            for (int e = lane; e < NU * SX; e += WAVE) DU[e] = bdu[e];
            vm_sync();
            break;
        }
        ratio = nr;
    }
    if constexpr (DUMP) {
        if (rec) {
            if (drefine) resto_dump_step(S, rs, C.N, rec);
            if (lane == 0) {
                double *sc = rec + RD_SCAL;
                sc[0] = mu; sc[1] = eta; sc[2] = dw; sc[3] = 1.0; sc[4] = ratio_pre; sc[5] = ratio;
            }
        }
    }
    return 1;
}

// optimality errors of the restoration problem (oracle compute_errors_resto), lane = stage
__device__ __noinline__ Errs resto_errors(const Model &M, const Smem &S, const Ctl &C, gdouble *ws, gdouble *rs, double mu, double eta)
{
    WS_TRAJ(ws);
    const int lane = lane_id();
    const int N = C.N;
    double dinf = 0, pinf = 0, cmu = 0, c0 = 0, smult = 0, sz = 0;
    if (lane < N) {
        const int k = lane, k1 = k + 1;
        double xk[NX], uk[NU], lk[NX];
        load_stage(S, k, xk);
        load_u(S, k, uk);
#pragma unroll
        for (int i = 0; i < NX; ++i) lk[i] = LAM[i * SX + k];
        double btl[NU];
        Bt_times(M, xk, lk, btl);
#pragma unroll
        for (int a = 0; a < NU; ++a) {
            const int idx = a * SX + k;
            const double zl = ZLU[idx], zu = ZUU[idx];
            const double acc = eta * rs[R_DU2 + idx] * (uk[a] - rs[R_UR + idx]) + btl[a] - zl + zu;
            dinf = fmax(dinf, fabs(acc));
            const double sl = uk[a] - C.ulo, su = C.uhi - uk[a];
            cmu = fmax(cmu, fmax(fabs(sl * zl - mu), fabs(su * zu - mu)));
            c0 = fmax(c0, fmax(fabs(sl * zl), fabs(su * zu)));
            sz += zl + zu;
        }
        double xn[NX];
        f_disc(M, xk, uk, xn);
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const int idx = i * SX + k;
            const double pe = rs[R_P + idx], ne = rs[R_N + idx], zp = rs[R_ZP + idx], zn = rs[R_ZN + idx];
            pinf = fmax(pinf, fabs(xn[i] - S.x[i * SX + k1] - pe + ne));
            smult += fabs(lk[i]);
            dinf = fmax(dinf, fmax(fabs(RESTO_RHO - lk[i] - zp), fabs(RESTO_RHO + lk[i] - zn)));
            cmu = fmax(cmu, fmax(fabs(pe * zp - mu), fabs(ne * zn - mu)));
            c0 = fmax(c0, fmax(fabs(pe * zp), fabs(ne * zn)));
            sz += zp + zn;
        }
        // x_{k+1} rows
        double x1[NX], g[NX];
        load_stage(S, k1, x1);
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const int idx = i * SX + k1;
            g[i] = eta * rs[R_DX2 + idx] * (x1[i] - rs[R_XR + idx]) - lk[i];
        }
        if (k1 < N) {
            double u1[NU], l1[NX], atl[NX];
            load_u(S, k1, u1);
#pragma unroll
            for (int i = 0; i < NX; ++i) l1[i] = LAM[i * SX + k1];
            At_times(M, x1, u1, l1, atl);
#pragma unroll
            for (int i = 0; i < NX; ++i) g[i] += atl[i];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double zl = ZLW[c * SX + k1], zu = ZUW[c * SX + k1];
            g[10 + c] += -zl + zu;
            const double sl = x1[10 + c] - C.wlo, su = C.whi - x1[10 + c];
            cmu = fmax(cmu, fmax(fabs(sl * zl - mu), fabs(su * zu - mu)));
            c0 = fmax(c0, fmax(fabs(sl * zl), fabs(su * zu)));
            sz += zl + zu;
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) dinf = fmax(dinf, fabs(g[i]));
    }
    dinf = wmax(dinf);
    pinf = wmax(pinf);
    cmu = wmax(cmu);
    c0 = wmax(c0);
    smult = wsum(smult);
    sz = wsum(sz);
    const double smax = 100.0;
    const double n_z = (double)(N * NU * 2 + N * 3 * 2 + 2 * N * NX);
    const double n_mult = (double)(N * NX) + n_z;
    Errs E;
    E.sd = fmax(smax, (smult + sz) / n_mult) / smax;
    E.sc = fmax(smax, sz / n_z) / smax;
    E.dinf = dinf;
    E.pinf = pinf;
    E.cmu = cmu;
    E.c0 = c0;
    return E;
}

// theta_R = ||c_R||_1 and phi_R = f_R - mu sum ln(slacks) at v + alpha dv, p + alpha dp, n + alpha dn
// (oracle merit_resto), lane = stage
__device__ __noinline__ Merit resto_merit(const Model &M, const Smem &S, const Ctl &C, gdouble *ws, gdouble *rs, double alpha, double mu,
                                          double eta)
{
    WS_TRAJ(ws);
    const int lane = lane_id();
    const int N = C.N;
    double th = 0, lb = 0, f = 0;
    int good = 1;
    if (lane < N) {
        const int k = lane, k1 = k + 1;
        double xk[NX], x1[NX], uk[NU], xn[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            xk[i] = S.x[i * SX + k] + alpha * DX[i * SX + k];
            x1[i] = S.x[i * SX + k1] + alpha * DX[i * SX + k1];
        }
#pragma unroll
        for (int a = 0; a < NU; ++a) uk[a] = S.u[a * SX + k] + alpha * DU[a * SX + k];
        f_disc(M, xk, uk, xn);
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const int idx = i * SX + k;
            const double pe = rs[R_P + idx] + alpha * rs[R_DP + idx], ne = rs[R_N + idx] + alpha * rs[R_DN + idx];
            if (!(pe > 0) || !(ne > 0)) good = 0;
            th += fabs(xn[i] - x1[i] - pe + ne);
            f += RESTO_RHO * (pe + ne);
            lb += log(pe) + log(ne);
        }
#pragma unroll
        for (int a = 0; a < NU; ++a) {
            const int idx = a * SX + k;
            const double d = uk[a] - rs[R_UR + idx];
            f += 0.5 * eta * rs[R_DU2 + idx] * d * d;
            const double sl = uk[a] - C.ulo, su = C.uhi - uk[a];
            if (!(sl > 0) || !(su > 0)) good = 0;
            lb += log(sl) + log(su);
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const int idx = i * SX + k1;
            const double d = x1[i] - rs[R_XR + idx];
            f += 0.5 * eta * rs[R_DX2 + idx] * d * d;
            if (i >= 10) {
                const double sl = x1[i] - C.wlo, su = C.whi - x1[i];
                if (!(sl > 0) || !(su > 0)) good = 0;
                lb += log(sl) + log(su);
            }
        }
    }
    th = wsum(th);
    lb = wsum(lb);
    f = wsum(f);
    good = wand(good);
    Merit R;
    R.theta = th;
    R.phi = f - mu * lb;
    R.ok = good && isfinite(R.phi) && isfinite(th);
    R.J = f;
    R.lb = lb;
    return R;
}

// directional derivative of phi_R (oracle gbd_resto) and the fraction to the boundary of the restoration
// direction (oracle ftb_resto: v bounds and p, n >= 0; bound duals of v and of p, n)
struct RestoDir {
    double gBD, amax, az;
};
__device__ __noinline__ RestoDir resto_direction(const Smem &S, const Ctl &C, gdouble *ws, gdouble *rs, double tau, double mu, double eta)
{
    WS_TRAJ(ws);
    const int lane = lane_id();
    const int N = C.N;
    double g = 0.0, am = 1.0, az = 1.0;
    if (lane < N) {
        const int k = lane, k1 = k + 1;
#pragma unroll
        for (int a = 0; a < NU; ++a) {
            const int idx = a * SX + k;
            const double v = S.u[idx], d = DU[idx];
            double gb, sg;
            bar_terms(v, C.ulo, C.uhi, 0, 0, mu, gb, sg);
            g += (eta * rs[R_DU2 + idx] * (v - rs[R_UR + idx]) + gb) * d;
            const double sl = v - C.ulo, su = C.uhi - v;
            if (d < 0) am = fmin(am, -tau * sl / d);
            if (d > 0) am = fmin(am, tau * su / d);
            const double zl = ZLU[idx], zu = ZUU[idx];
            const double dzl = mu / sl - zl - zl / sl * d, dzu = mu / su - zu + zu / su * d;
            if (dzl < 0) az = fmin(az, -tau * zl / dzl);
            if (dzu < 0) az = fmin(az, -tau * zu / dzu);
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const int idx = i * SX + k;
            const double pe = rs[R_P + idx], ne = rs[R_N + idx], dp = rs[R_DP + idx], dn = rs[R_DN + idx];
            const double zp = rs[R_ZP + idx], zn = rs[R_ZN + idx];
            g += (RESTO_RHO - mu / pe) * dp + (RESTO_RHO - mu / ne) * dn;
            if (dp < 0) am = fmin(am, -tau * pe / dp);
            if (dn < 0) am = fmin(am, -tau * ne / dn);
            const double dzp = mu / pe - zp - zp / pe * dp, dzn = mu / ne - zn - zn / ne * dn;
            if (dzp < 0) az = fmin(az, -tau * zp / dzp);
            if (dzn < 0) az = fmin(az, -tau * zn / dzn);
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const int idx = i * SX + k1;
            const double v = S.x[idx], d = DX[idx];
            double gr = eta * rs[R_DX2 + idx] * (v - rs[R_XR + idx]);
            if (i >= 10) {
                const int c = i - 10;
                double gb, sg;
                bar_terms(v, C.wlo, C.whi, 0, 0, mu, gb, sg);
                gr += gb;
                const double sl = v - C.wlo, su = C.whi - v;
                if (d < 0) am = fmin(am, -tau * sl / d);
                if (d > 0) am = fmin(am, tau * su / d);
                const double zl = ZLW[c * SX + k1], zu = ZUW[c * SX + k1];
                const double dzl = mu / sl - zl - zl / sl * d, dzu = mu / su - zu + zu / su * d;
                if (dzl < 0) az = fmin(az, -tau * zl / dzl);
                if (dzu < 0) az = fmin(az, -tau * zu / dzu);
            }
            g += gr * d;
        }
    }
    RestoDir R;
    R.gBD = wsum(g);
    R.amax = wmin(am);
    R.az = wmin(az);
    return R;
}

// accept a restoration step (oracle take_step_resto): p, n with alpha, their bound duals with alpha_z, then the
// original variables (accept_step, kappa_sigma safeguard included)
__device__ __noinline__ void resto_accept(Smem &S, const Ctl &C, gdouble *ws, gdouble *rs, double alpha, double az, double mu)
{
    const int lane = lane_id();
    const int N = C.N;
    if (lane < N) {
        const int k = lane;
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const int idx = i * SX + k;
            const double pe = rs[R_P + idx], ne = rs[R_N + idx], dp = rs[R_DP + idx], dn = rs[R_DN + idx];
            const double zp0 = rs[R_ZP + idx], zn0 = rs[R_ZN + idx];
            const double zp = zp0 + az * (mu / pe - zp0 - zp0 / pe * dp);
            const double zn = zn0 + az * (mu / ne - zn0 - zn0 / ne * dn);
            const double p1 = pe + alpha * dp, n1 = ne + alpha * dn;
            rs[R_P + idx] = p1;
            rs[R_N + idx] = n1;
            rs[R_ZP + idx] = fmax(fmin(zp, 1e10 * mu / p1), mu / (1e10 * p1));
            rs[R_ZN + idx] = fmax(fmin(zn, 1e10 * mu / n1), mu / (1e10 * n1));
        }
    }
    accept_step(S, C, ws, alpha, az, mu);
}

struct RestoOut {
    int status, iters, sweeps, trials;
};

// The restoration phase from the current iterate (oracle orc_restoration): mu_o the original barrier parameter,
// (th_ref, ph_ref) the start point, which the caller has added to the original filter (nfilt entries).  status 0:
// an iterate acceptable to the original problem was found (multipliers reset as IPOPT does); otherwise the final
// status (ST_RESTO_FAIL, ST_INFEASIBLE, ST_MAXITER, ST_REG_FAIL, ST_NONFINITE) with the wave back at the start point.
// DUMP: rdump (nullable) is this instance's restoration dump record when this entry is the armed one; iteration dit of
// the entry is dumped (lafse3_debug_dump_resto); the production kernels instantiate DUMP = false, which compiles none
// of it.
template <bool DUMP>
__device__ __noinline__ RestoOut restoration(const lafse3_params &prm, const Model &M, const Attitude &at, Smem &S,
                                             const Ctl &C, gdouble *ws, gdouble *rs, double mu_o, double th_ref, double ph_ref,
                                             int onfilt, int iters_left, [[maybe_unused]] double *rdump = nullptr,
                                             [[maybe_unused]] int dit = 0, [[maybe_unused]] int drefine = 0)
{
    WS_TRAJ(ws);
    const int lane = lane_id();
    const int N = C.N;
    const gdouble *FT = ws + WS_FILT, *FP = ws + WS_FILT + FMAX;
    gdouble *RFT = rs + R_FILT, *RFP = rs + R_FILT + FMAX;
    gdouble *Z = ws + WS_Z, *SZ = rs + R_SZ;
    RestoOut out = {ST_MAXITER, 0, 0, 0};
    // ||c||_inf of the original constraints at the current primal point
    auto orig_cmax = [&]() {
        double cm = 0.0;
        if (lane < N) {
            const int k = lane;
            double xk[NX], uk[NU], xn[NX];
            load_stage(S, k, xk);
            load_u(S, k, uk);
            f_disc(M, xk, uk, xn);
#pragma unroll
            for (int i = 0; i < NX; ++i) cm = fmax(cm, fabs(xn[i] - S.x[i * SX + k + 1]));
        }
        return wmax(cm);
    };
    // start point: reference point, D_R^2 = min(1, 1/|v_R|)^2, saved multipliers; mu_R = max(mu, ||c||_inf)
    const double cmax = orig_cmax();
    const double mu0 = fmax(mu_o, cmax);
    for (int e = lane; e < NX * SX; e += WAVE) {
        const double v = S.x[e];
        const double d = fmin(1.0, 1.0 / fabs(v));
        rs[R_XR + e] = v;
        rs[R_DX2 + e] = d * d;
        rs[R_SLAM + e] = LAM[e];
    }
    for (int e = lane; e < NU * SX; e += WAVE) {
        const double v = S.u[e];
        const double d = fmin(1.0, 1.0 / fabs(v));
        rs[R_UR + e] = v;
        rs[R_DU2 + e] = d * d;
    }
    for (int e = lane; e < 14 * SX; e += WAVE) SZ[e] = Z[e];
    vm_sync();
    if (lane < N) {
        // p, n from the barrier first-order conditions given c (RestoIterateInitializer), z_p = mu / p, z_n = mu / n
        const int k = lane;
        double xk[NX], uk[NU], xn[NX];
        load_stage(S, k, xk);
        load_u(S, k, uk);
        f_disc(M, xk, uk, xn);
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const int idx = i * SX + k;
            const double c = xn[i] - S.x[i * SX + k + 1];
            const double a = (mu0 - RESTO_RHO * c) / (2.0 * RESTO_RHO);
            const double n = a + sqrt(a * a + mu0 * c / (2.0 * RESTO_RHO));
            const double p = c + n;
            rs[R_N + idx] = n;
            rs[R_P + idx] = p;
            rs[R_ZP + idx] = mu0 / p;
            rs[R_ZN + idx] = mu0 / n;
            LAM[idx] = 0.0;
        }
#pragma unroll
        for (int a = 0; a < NU; ++a) {
            ZLU[a * SX + k] = fmin(RESTO_RHO, ZLU[a * SX + k]);
            ZUU[a * SX + k] = fmin(RESTO_RHO, ZUU[a * SX + k]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            ZLW[c * SX + k + 1] = fmin(RESTO_RHO, ZLW[c * SX + k + 1]);
            ZUW[c * SX + k + 1] = fmin(RESTO_RHO, ZUW[c * SX + k + 1]);
        }
    }
    vm_sync();
    // constraint multipliers: least-squares estimate (constr_mult_init_max = 1000)
    if (resto_riccati(M, at, S, C, ws, rs, mu0, sqrt(mu0), 0.0, 1, 0)) {
        if constexpr (DUMP)   // the least-squares multipliers before the cut
            if (rdump) {
                for (int e = lane; e < N * NX; e += WAVE) rdump[RD_LSQ + e] = LP[(e % NX) * SX + e / NX];
                if (lane == 0) rdump[RD_LSQ + MAXN * NX] = 1.0;
            }
        double mx = 0.0;
        if (lane < N)
#pragma unroll
            for (int i = 0; i < NX; ++i) mx = fmax(mx, fabs(LP[i * SX + lane]));
        mx = wmax(mx);
        if (mx <= 1e3 && lane < N)
#pragma unroll
            for (int i = 0; i < NX; ++i) LAM[i * SX + lane] = LP[i * SX + lane];
        vm_sync();
    } else {
        if constexpr (DUMP)
            if (rdump && lane == 0) rdump[RD_LSQ + MAXN * NX] = 0.0;
    }
    if constexpr (DUMP)   // the IPM iterations taken before this entry
        if (rdump && lane == 0) rdump[RD_LSQ + MAXN * NX + 1] = prm.max_iter - iters_left;
    out.sweeps++;
    double mu = mu0, eta = sqrt(mu0), tau = fmax(0.99, 1.0 - mu0);
    int nfilt = 0;
    double theta_max = -1, theta_min = -1, dw_last = 0.0;
    const double eps = 2.220446049250313e-16;
    for (;;) {
        Errs E = resto_errors(M, S, C, ws, rs, mu, eta);
        const double e0 = err_value(E, 0);
        if (!isfinite(e0)) { out.status = ST_NONFINITE; break; }
        if (e0 <= prm.tol) {
            // the restoration problem converged without a point the original filter accepts: IPOPT reports a
            // restoration failure when the original ||c||_inf is at most resto_failure_feasibility_threshold (its
            // documented default 1e2 tol), local infeasibility otherwise (oracle orc_restoration)
            out.status = (orig_cmax() <= 1e2 * prm.tol) ? ST_RESTO_FAIL : ST_INFEASIBLE;
            break;
        }
        if (iters_left <= 0) { out.status = ST_MAXITER; break; }
        {
            const double mu_min = prm.tol / 10.0;
            for (;;) {
                if (!(err_value(E, 1) <= 10.0 * mu)) break;
                const double nmu = fmax(mu_min, fmin(0.2 * mu, pow15(mu)));
                if (nmu == mu) break;
                mu = nmu;
                eta = sqrt(mu);
                tau = fmax(0.99, 1.0 - mu);
                nfilt = 0;
                E = resto_errors(M, S, C, ws, rs, mu, eta);
            }
        }
        // direction with inertia correction
        [[maybe_unused]] double *rec = nullptr;
        if constexpr (DUMP) {
            if (rdump && out.iters == dit) {
                rec = rdump;
                resto_dump_point(S, ws, rs, N, rec + RD_STEP_W);
            }
        }
        // (a lambda around the two calls would hide the wave-constant addresses of M, at, S and C from the
        // interprocedural constant propagation, which folds them into resto_newton and its callees)
        int ok = resto_newton<DUMP>(M, at, S, C, ws, rs, mu, eta, 0.0, out.sweeps, rec, drefine);
        if (!ok) {
            double dw = (dw_last == 0.0) ? 1e-4 : fmax(1e-20, dw_last / 3.0);
            for (;;) {
                ok = resto_newton<DUMP>(M, at, S, C, ws, rs, mu, eta, dw, out.sweeps, rec, drefine);
                if (ok) { dw_last = dw; break; }
                dw *= (dw_last == 0.0) ? 100.0 : 8.0;
                if (dw > 1e40) break;
            }
            if (!ok) { out.status = ST_REG_FAIL; break; }
        }
        const RestoDir D = resto_direction(S, C, ws, rs, tau, mu, eta);
        const Merit m0 = resto_merit(M, S, C, ws, rs, 0.0, mu, eta);
        const double th0 = m0.theta, ph0 = m0.phi, gBD = D.gBD;
        if (theta_max < 0) {
            theta_max = 1e4 * fmax(1.0, th0);
            theta_min = 1e-4 * fmax(1.0, th0);
        }
        double amin_base = 1e-5;
        if (gBD < 0) {
            amin_base = fmin(1e-5, 1e-8 * th0 / (-gBD));
            if (th0 <= theta_min) amin_base = fmin(amin_base, pow(th0, 1.1) / pow(-gBD, 2.3));
        }
        const double alpha_min = 0.05 * amin_base;
        double alpha = D.amax, pht = 0;
        int accepted = 0;
        for (;;) {
            const Merit mt = resto_merit(M, S, C, ws, rs, alpha, mu, eta);
            out.trials++;
            pht = mt.phi;
            if (ls_accept(RFT, RFP, nfilt, alpha, mt.theta, mt.phi, mt.ok, th0, ph0, gBD, theta_max, theta_min)) {
                accepted = 1;
                break;
            }
            alpha *= 0.5;
            if (alpha < alpha_min || !(alpha > 0.0)) break;   // alpha_min = 0 (theta_R = 0) must still end
        }
        if (!accepted) { out.status = ST_RESTO_FAIL; break; }
        {
            const int ftype = (gBD < 0) && (alpha * pow(-gBD, 2.3) > pow(th0, 1.1));
            const int armijo = (pht - ph0 - 1e-8 * alpha * gBD) <= 10.0 * eps * fabs(ph0);
            if (!ftype || !armijo) nfilt = filter_add(RFT, RFP, nfilt, th0, ph0);
        }
        resto_accept(S, C, ws, rs, alpha, D.az, mu);
        out.iters++;
        iters_left--;
        // back to the original problem? (RestoFilterConvergenceCheck::TestOrigProgress)
        const Merit mo = eval_merit(M, at, S, C, ws, 0.0, mu_o);
        if (mo.ok && mo.theta <= 0.9 * th_ref && filter_ok(FT, FP, onfilt, mo.theta, mo.phi) &&
            ((mo.theta - (1.0 - 1e-5) * th_ref) <= 10.0 * eps * fabs(th_ref) ||
             (mo.phi - ph_ref + 1e-8 * th_ref) <= 10.0 * eps * fabs(ph_ref))) {
            out.status = 0;
            break;
        }
    }
    if (out.status == 0) {
        // bound multipliers from the restoration problem, reset to 1 when one exceeds 1000; lam = 0
        double zmax = 0.0;
        if (lane < N) {
            const int k = lane;
#pragma unroll
            for (int a = 0; a < NU; ++a) zmax = fmax(zmax, fmax(ZLU[a * SX + k], ZUU[a * SX + k]));
#pragma unroll
            for (int c = 0; c < 3; ++c) zmax = fmax(zmax, fmax(ZLW[c * SX + k + 1], ZUW[c * SX + k + 1]));
        }
        zmax = wmax(zmax);
        if (lane < N) {
            const int k = lane;
            if (zmax > 1e3) {
#pragma unroll
                for (int a = 0; a < NU; ++a) ZLU[a * SX + k] = ZUU[a * SX + k] = 1.0;
#pragma unroll
                for (int c = 0; c < 3; ++c) ZLW[c * SX + k + 1] = ZUW[c * SX + k + 1] = 1.0;
            }
#pragma unroll
            for (int i = 0; i < NX; ++i) LAM[i * SX + k] = 0.0;
        }
    } else {
        // the solve ends at the point where the restoration started
        for (int e = lane; e < NX * SX; e += WAVE) {
            S.x[e] = rs[R_XR + e];
            LAM[e] = rs[R_SLAM + e];
        }
        for (int e = lane; e < NU * SX; e += WAVE) S.u[e] = rs[R_UR + e];
        for (int e = lane; e < 14 * SX; e += WAVE) Z[e] = SZ[e];
    }
    vm_sync();
    return out;
}

// IPOPT's watchdog (BacktrackingLineSearch::StartWatchDog / StopWatchDog; oracle wd_copy): save (save = 1) or
// restore the iterate x, u, lam, bound duals and the search direction dx, du, lam+ (rws region R_WD).  Inline: a
// call in the iteration loop costs the loop spills.
__device__ inline void wd_copy(Smem &S, gdouble *ws, gdouble *rs, int save)
{
    WS_TRAJ(ws);
    const int lane = lane_id();
    gdouble *Z = ws + WS_Z, *D = rs + R_WD;
    if (save) {
        for (int e = lane; e < NX * SX; e += WAVE) {
            D[WD_X + e] = S.x[e];
            D[WD_LAM + e] = LAM[e];
            D[WD_DX + e] = DX[e];
            D[WD_LP + e] = LP[e];
        }
        for (int e = lane; e < NU * SX; e += WAVE) {
            D[WD_U + e] = S.u[e];
            D[WD_DU + e] = DU[e];
        }
        for (int e = lane; e < 14 * SX; e += WAVE) D[WD_Z + e] = Z[e];
    } else {
        for (int e = lane; e < NX * SX; e += WAVE) {
            S.x[e] = D[WD_X + e];
            LAM[e] = D[WD_LAM + e];
            DX[e] = D[WD_DX + e];
            LP[e] = D[WD_LP + e];
        }
        for (int e = lane; e < NU * SX; e += WAVE) {
            S.u[e] = D[WD_U + e];
            DU[e] = D[WD_DU + e];
        }
        for (int e = lane; e < 14 * SX; e += WAVE) Z[e] = D[WD_Z + e];
    }
    vm_sync();
}
