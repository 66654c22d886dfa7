// riccati.inc — structured Riccati solve of the primal-dual Newton system (included by ipm_kernel.hip).
//
// Newton step of the barrier problem on the multiple-shooting NLP of quad_OC.py:124-167 with the
// state augmented by the previous control (the ||U_k - U_{k-1}||^2 term couples stages):
//   min sum_k 1/2 z_k^T H~_k z_k + h~_k^T z_k   s.t. dx~_{k+1} = G_k z_k + c~_k,  z_k = [dx~_k; du_k]
//
// The factorisation sweep itself (W = P G, M = G^T W + H~, Cholesky of Quu, K, k, P, p per stage) is
// riccati_mfma.inc backward_mfma; this file holds what stands around it:
// buffer helpers    wave-uniform workspace bases and the buffer loads / stores the sweeps step through HBM with
// build_table       stage-parallel (lane = stage): G_k's 54 stage-dependent entries, H~_k's 62 upper
//                   nonzeros (cost Hessian + lambda-Hessian of f_d + barrier Sigma), h~_k, c~_k  -> HBM table
// terminal          the value function at stage N (P_N, p_N -> S.P / S.p, packed P_N -> HBM), where the
//                   factorisation sweep and a refinement sweep start
// gslot, gconst, make_atab   A~ by rows and by columns: every coefficient's table slot or constant, for the chains
// forward_chain     du_s = K_s x~_s + k_s, dx_{s+1} = A~ dx_s + B~ du_s + c_s per stage
// costates_identity lam+_{k-1} = (P_k dx~_k + p_k)[x rows] stage-parallel (no adjoint recursion)
// backward_chain    iterative-refinement right-hand side with the last factorisation: P_s c~_{s-1}
//                   stage-parallel, then ph_s = A~^T ph_{s+1} + rq_s + K_s^T g_s + P_s c~_{s-1} per stage

__device__ inline dvec2 dv2(double a, double b)
{
    dvec2 v;
    v.x = a;
    v.y = b;
    return v;
}
__constant__ UpTab c_up = make_uptab();
typedef unsigned int v2u32 __attribute__((__vector_size__(8)));
typedef __amdgpu_buffer_rsrc_t Rsrc;
// buffer resource over an instance's workspace (base made wave-uniform); loads and stores through it take the
// stage offset in an SGPR (soffset) and a per-lane constant offset, and an offset past the range reads 0 / drops
// the store (the structural zeros of the gathers, the predicated stores)
__device__ inline Rsrc ws_rsrc(const gdouble *p, int bytes)
{
    const long long v = (long long)(const double *)p;
    const int lo = __builtin_amdgcn_readfirstlane((int)v), hi = __builtin_amdgcn_readfirstlane((int)(v >> 32));
    double *u = (double *)(((long long)hi << 32) | (unsigned)lo);
    return __builtin_amdgcn_make_buffer_rsrc(u, 0, bytes, 0x00020000);
}
constexpr unsigned MF_OOB = 0x40000000u;   // past any workspace
// a wave-uniform int in an SGPR: the stage offsets (soffset) of the buffer operations (a VGPR soffset costs a
// waterfall loop per load)
__device__ inline int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ inline double bld(Rsrc r, unsigned voff, int soff)
{
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0));
}
__device__ inline dvec2 bld2(Rsrc r, unsigned voff, int soff)
{
    return __builtin_bit_cast(dvec2, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}
__device__ inline void bst(double v, Rsrc r, unsigned voff, int soff)
{
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u32, v), r, voff, soff, 0);
}
// the workspace as a wave-uniform byte pointer (readfirstlane of both halves, as uniform() for doubles): a load
// from it plus a 32-bit per-lane byte offset is the SGPR-base form of global_load, whose stage stepping is
// scalar (the ws argument of the non-inlined linear_solve arrives in VGPRs: every address formed from it is
// 64-bit vector arithmetic per load)
typedef __attribute__((address_space(1))) char gchar;
__device__ inline const gchar *ws_uniform(const gdouble *p)
{
    const long long v = (long long)(const double *)p;
    const int lo = __builtin_amdgcn_readfirstlane((int)v), hi = __builtin_amdgcn_readfirstlane((int)(v >> 32));
    return (const gchar *)(((long long)hi << 32) | (unsigned)lo);
}
// (the offset is made opaque at the load: hoisted out of a loop, its zero extension reaches instruction selection
// as a 64-bit register and the load falls back to a 64-bit vector address)
__device__ inline double gld(const gchar *base, unsigned &voff)
{
    asm volatile("" : "+v"(voff));
    return *(const gdouble *)(base + voff);
}


// P_k store (WS_PST): stage-major [slot][PSTR], 16-byte aligned, so that the stage-parallel readers (refinement
// prepass, costates: lane = stage) stream a stage's packed upper triangle as 16-byte pieces.  (Entry-major, the
// entry e of every stage contiguous, measured +15 % kernel time: the scattered 8-byte stores of the stage.)
static_assert(WS_PST % 2 == 0 && PSTR % 2 == 0, "P_k stages read as 16-byte pieces");
__device__ inline size_t pst_at(int slot, int e)
{
    return (size_t)slot * PSTR + e;
}
// stage loops store without exec-mask branches (duplicate lanes write identical values to identical addresses)

// ---- stage table (lane = stage) ------------------------------------------------------------------
__device__ __attribute__((always_inline)) inline void build_table(const Model &M, const Attitude &at, const Smem &S, const Ctl &C,
                                         gdouble *ws, int mode_lsq)
{
    WS_TRAJ(ws);
    gdouble *tab = ws + WS_TAB;
    const int lane = opaque_lane();
    const int N = C.N;
    if (lane < N) {
        const int k = lane;
        const double s = C.s, dt = M.dt;
        gdouble *row = tab + (size_t)k * TB_W;
        double xk[NX], uk[NU], up[NU];
        load_stage(S, k, xk);
        load_u(S, k, uk);
#pragma unroll
        for (int a = 0; a < NU; ++a) up[a] = (k == 0) ? S.ulast[a] : S.u[a * SX + k - 1];
        // bound duals (HBM) loaded before the first table store: a load issued after a store waits for it
        double zlw_[3], zuw_[3], zlu_[NU], zuu_[NU];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            zlw_[c] = ZLW[c * SX + k];
            zuw_[c] = ZUW[c * SX + k];
        }
#pragma unroll
        for (int a = 0; a < NU; ++a) {
            zlu_[a] = ZLU[a * SX + k];
            zuu_[a] = ZUU[a * SX + k];
        }
        const double *q = xk + 6, *w = xk + 10;
        const double Tm = (uk[0] + uk[1] + uk[2] + uk[3]) / M.mass;
        const double g0 = 2 * (q[1] * q[3] + q[0] * q[2]);
        const double g1 = 2 * (q[2] * q[3] - q[0] * q[1]);
        const double g2 = 1 - 2 * (q[1] * q[1] + q[2] * q[2]);
        // ---- G stage-dependent slots (riccati_tables.hpp order)
        const double Dg[3][4] = {{2 * q[2], 2 * q[3], 2 * q[0], 2 * q[1]},
                                 {-2 * q[1], -2 * q[0], 2 * q[3], 2 * q[2]},
                                 {0.0, -4 * q[1], -4 * q[2], 0.0}};
        const double Om[4][4] = {{0.0, -w[0], -w[1], -w[2]},
                                 {w[0], 0.0, w[2], -w[1]},
                                 {w[1], -w[2], 0.0, w[0]},
                                 {w[2], w[1], -w[0], 0.0}};
        const double Xi[4][3] = {{-q[1], -q[2], -q[3]}, {q[0], -q[3], q[2]}, {q[3], q[0], -q[1]}, {-q[2], q[1], q[0]}};
        const double Jw[3][3] = {{0.0, -M.ax * w[2], -M.ax * w[1]},
                                 {-M.ay * w[2], 0.0, -M.ay * w[0]},
                                 {-M.az * w[1], -M.az * w[0], 0.0}};
        int v = TB_G;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int r = 0; r < 3; ++r) row[v++] = dt * Tm * Dg[r][c];
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (b != c) row[v++] = 0.5 * dt * Om[b][c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int b = 0; b < 4; ++b) row[v++] = 0.5 * dt * Xi[b][c];
#pragma unroll
            for (int d = 0; d < 3; ++d)
                if (d != c) row[v++] = dt * Jw[d][c];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            row[v++] = dt * g0 / M.mass;
            row[v++] = dt * g1 / M.mass;
            row[v++] = dt * g2 / M.mass;
        }
        // ---- H~ upper nonzeros (make_htab order), without delta_w
        double sgw[3] = {0, 0, 0}, gbw[3] = {0, 0, 0};
        if (k >= 1 && !mode_lsq)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                bar_terms(w[c], C.wlo, C.whi, zlw_[c], zuw_[c], C.mu, gbw[c], sgw[c]);
        double sgu[NU], gbu[NU];
#pragma unroll
        for (int a = 0; a < NU; ++a) {
            sgu[a] = 0.0;
            gbu[a] = 0.0;
            if (!mode_lsq) bar_terms(uk[a], C.ulo, C.uhi, zlu_[a], zuu_[a], C.mu, gbu[a], sgu[a]);
        }
        gdouble *hv = row + TB_H;
        const double d2 = 2 * M.du_w * s;
        if (mode_lsq) {
            const double one = (k >= 1) ? 1.0 : 0.0;
#pragma unroll
            for (int e = 0; e < NHV; ++e) hv[e] = 0.0;
#pragma unroll
            for (int e = 0; e < 6; ++e) hv[e] = one;
            hv[6] = one; hv[10] = one; hv[13] = one; hv[15] = one;   // q-q diagonal
            hv[28] = one; hv[31] = one; hv[33] = one;                // w-w diagonal
#pragma unroll
            for (int a = 0; a < 4; ++a) hv[58 + a] = 1.0;
        } else {
            StageHess H;
            if (k >= 1) {
                double lk[NX];
#pragma unroll
                for (int i = 0; i < NX; ++i) lk[i] = LAM[i * SX + k];
                stage_hessian(M, at, s, S.wk[k], xk, uk, lk, H);
                int e = 0;
#pragma unroll
                for (int a = 0; a < 3; ++a) hv[e++] = H.hr;
#pragma unroll
                for (int a = 0; a < 3; ++a) hv[e++] = H.hv;
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int c = b; c < 4; ++c) hv[e++] = H.qq[b * 4 + c];
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int c = 0; c < 3; ++c) hv[e++] = H.qw[b * 3 + c];
                hv[e++] = H.hw + sgw[0]; hv[e++] = H.wxy; hv[e++] = H.wxz;
                hv[e++] = H.hw + sgw[1]; hv[e++] = H.wyz;
                hv[e++] = H.hw + sgw[2];
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int a = 0; a < 4; ++a) hv[e++] = H.qu[b];
            } else {
#pragma unroll
                for (int e = 0; e < 50; ++e) hv[e] = 0.0;
            }
#pragma unroll
            for (int a = 0; a < 4; ++a) hv[50 + a] = d2;
#pragma unroll
            for (int a = 0; a < 4; ++a) hv[54 + a] = -d2;
#pragma unroll
            for (int a = 0; a < 4; ++a) hv[58 + a] = s * (2 * M.wthrust + 2 * M.du_w) + sgu[a];
        }
        // ---- h~ (21)
        gdouble *hh = row + TB_h;
        if (k >= 1) {
            double g[NX];
            state_cost_grad(M, at, S.goal, S.ptra, S.wk[k], xk, g);
#pragma unroll
            for (int i = 0; i < NX; ++i) g[i] *= s;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                g[10 + c] += mode_lsq ? (-zlw_[c] + zuw_[c]) : gbw[c];
#pragma unroll
            for (int i = 0; i < NX; ++i) hh[i] = g[i];
        } else {
#pragma unroll
            for (int i = 0; i < NX; ++i) hh[i] = 0.0;
        }
#pragma unroll
        for (int a = 0; a < NU; ++a) {
            hh[NX + a] = -d2 * (uk[a] - up[a]);
            double r = s * (2 * M.wthrust * uk[a] + 2 * M.du_w * (uk[a] - up[a]));
            r += mode_lsq ? (-zlu_[a] + zuu_[a]) : gbu[a];
            hh[17 + a] = r;
        }
        // ---- c~ (13)
        gdouble *cc = row + TB_c;
        if (mode_lsq) {
#pragma unroll
            for (int i = 0; i < NX; ++i) cc[i] = 0.0;
        } else {
            double xn[NX];
            f_disc(M, xk, uk, xn);
#pragma unroll
            for (int i = 0; i < NX; ++i) cc[i] = xn[i] - S.x[i * SX + k + 1];
        }
        // ---- constants of the MFMA stage's gathers (riccati_mfma.inc mf_gsrc)
        gdouble *kc = row + TB_K;
        kc[0] = 1.0;
        kc[1] = dt;
        kc[2] = M.bwx;
        kc[3] = -M.bwx;
        kc[4] = M.bwy;
        kc[5] = -M.bwy;
        kc[6] = M.bwz;
        kc[7] = -M.bwz;
        kc[8] = 0.0;   // the chains' structural zeros (acoef)
    }
    vm_sync();
}

// ---- terminal value function ------------------------------------------------------------------------
__device__ inline double sel3(const double *v, int c) { return c == 0 ? v[0] : (c == 1 ? v[1] : v[2]); }
__device__ void terminal(const Model &M, const Attitude &at, Smem &S, const Ctl &C, gdouble *ws, double dw,
                         int mode_lsq, int refine)
{
    WS_TRAJ(ws);
    const int lane = opaque_lane();
    const int N = C.N;
    const double s = C.s;
    // the omega bound duals at stage N, loaded once up front (in the loops below each use waited for its own load)
    double zlN[3], zuN[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        zlN[c] = ZLW[c * SX + N];
        zuN[c] = ZUW[c * SX + N];
    }
    for (int e = lane; e < NA * NA; e += WAVE) {
        const int i = e / NA, j = e % NA;
        double v = 0.0;
        if (i < NX && j < NX) {
            if (mode_lsq) {
                v = (i == j) ? 1.0 : 0.0;
            } else {
                if (i == j) {
                    if (i < 3) v = s * 2 * M.wrf;
                    else if (i < 6) v = s * 2 * M.wvf;
                    else if (i >= 10) v = s * 2 * M.wwf;
                    v += dw;
                }
                if (i >= 6 && i < 10 && j >= 6 && j < 10 && M.wqf != 0.0) v += s * M.wqf * (-2 * S.at.Sg[(i - 6) * 4 + (j - 6)]);
                if (i == j && i >= 10) {
                    const int c = i - 10;
                    double gb, sg;
                    bar_terms(S.x[i * SX + N], C.wlo, C.whi, sel3(zlN, c), sel3(zuN, c), C.mu, gb, sg);
                    v += sg;
                }
            }
        }
        S.P[i * PST + j] = v;
    }
    if (lane < NA) {
        double v = 0.0;
        if (lane < NX) {
            if (refine) {
                v = ws[WS_RQ + lane * SX + N];
            } else {
                double xN[NX], g[NX];
                load_stage(S, N, xN);
                state_cost_grad(M, at, S.goal, S.ptra, 0.0, xN, g);
                double gi = 0.0;
#pragma unroll
                for (int i = 0; i < NX; ++i)
                    if (i == lane) gi = g[i];
                v = s * gi;
                if (lane >= 10) {
                    const int c = lane - 10;
                    if (mode_lsq) {
                        v += -sel3(zlN, c) + sel3(zuN, c);
                    } else {
                        double gb, sg;
                        bar_terms(S.x[lane * SX + N], C.wlo, C.whi, sel3(zlN, c), sel3(zuN, c), C.mu, gb, sg);
                        v += gb;
                    }
                }
                ws[WS_PN + lane] = v;
            }
        }
        S.p[lane] = v;
    }
    sync();
    if (!refine) {
        // P_N -> HBM (packed upper), as [F] stores every later P_k
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int e3 = lane + 64 * r;
            if (e3 < NUP17) ws[WS_PST + pst_at(N - 1, e3)] = S.P[c_up.i17[e3] * PST + c_up.j17[e3]];
        }
    }
}

// ---- sweeps on the compact record ---------------------------------------------------------------------
// The closed loop is rebuilt per stage from the record (K, k) and the stage table (the G slots of A~ and B~)
// instead of a stored 17 x 17 Phi_k: 82 doubles per stage leave HBM instead of 334, and every chain reads
// K plus a handful of table slots instead of Phi and P (the kernel is bound by its workspace traffic).
//   forward_chain  du_s = K_s x~_s + k_s (4 dot products of 17, 16 lanes each + a DPP row sum), then
//                  dx_{s+1} = A~_s dx_s + B~_s du_s + c_s (A~ rows are <= 7 table slots / constants)
//   costates_identity  the costates from the Riccati identity, stage-parallel (the recursion
//                  lam+_{k-1} = r_k + A~_k^T lam+_k of oracle/lafse3_oracle.c riccati_solve, up to rounding)
//   backward_chain (refinement / SOC / IFT right-hand sides) g_s = B~_s^T ph_{s+1} + rr_s,
//                  ph_s = A~_s^T ph_{s+1} + rq_s + K_s^T g_s + P_s c~_{s-1} (P c~ from a stage-parallel prepass),
//                  then k_s = -Quu_s^{-1} g_s (stage-parallel)

// source of an A~ coefficient: G slot of the stage table (>= 0) or a constant
constexpr int SRC_ONE = -1, SRC_DT = -2, SRC_ZERO = -3;
__host__ __device__ constexpr int gslot(int j, int t)
{
    for (int v = 0; v < NGV; ++v)
        if (gv_col(v) == j && gv_pos(v) == t) return v;
    return -1;
}
__host__ __device__ constexpr int gconst(int j, int t)
{
    return j < 3 ? (t == 0 ? SRC_ONE : SRC_ZERO)
         : j < 6 ? (t == 0 ? SRC_DT : (t == 1 ? SRC_ONE : SRC_ZERO))
         : j < 10 ? (t == 3 + (j - 6) ? SRC_ONE : SRC_ZERO)
         : j < 13 ? (t == 4 + (j - 10) ? SRC_ONE : SRC_ZERO)
         : SRC_ZERO;
}
__host__ __device__ constexpr int gsrc(int j, int t) { return gslot(j, t) >= 0 ? gslot(j, t) : gconst(j, t); }
// A~ by rows (forward) and by columns (adjoint, backward): 8 (column | row, source) pairs per x row / column,
// half h of a lane pair takes entries 4h .. 4h + 3; unused entries carry SRC_ZERO
struct ATab {
    signed char rcol[NX][8], rsrc[NX][8];   // row i: columns and sources
    signed char crow[NX][8], csrc[NX][8];   // column j: rows and sources
};
__host__ __device__ constexpr ATab make_atab()
{
    ATab T{};
    for (int i = 0; i < NX; ++i) {
        int n = 0;
        for (int e = 0; e < 8; ++e) {
            T.rcol[i][e] = 0;
            T.rsrc[i][e] = SRC_ZERO;
            T.crow[i][e] = 0;
            T.csrc[i][e] = SRC_ZERO;
        }
        for (int j = 0; j < NX; ++j)
            for (int t = 0; t < GLEN; ++t)
                if (g_row(j, t) == i) {
                    T.rcol[i][n] = (signed char)j;
                    T.rsrc[i][n] = (signed char)gsrc(j, t);
                    ++n;
                }
        for (int t = 0; t < GLEN; ++t)
            if (g_row(i, t) >= 0) {
                T.crow[i][t] = (signed char)g_row(i, t);
                T.csrc[i][t] = (signed char)gsrc(i, t);
            }
    }
    return T;
}
__constant__ ATab c_at = make_atab();
constexpr int BV_SLOT = 42;   // G slots 42..44: B~ column u_0, rows v0..v2 (dt g(q) / m, the same for every rotor)

// one A~ coefficient: its table slot, a stage-dependent G slot or one of the row's constants (TB_K + 0: 1, + 1: dt,
// + 8: 0), so that every lane loads its coefficient and multiplies with it as it is
struct ACoef {
    int off;
};
__device__ inline ACoef acoef(int src)
{
    ACoef a;
    a.off = src >= 0 ? TB_G + src : (src == SRC_ONE ? TB_K + 0 : (src == SRC_DT ? TB_K + 1 : TB_K + 8));
    return a;
}

// a lane's double from lane l, as a wave-uniform value
__device__ inline double readlane_d(double v, int l)
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)b, l), hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
// sum over the 16 lanes of a DPP row (quad xor-1, quad xor-2, half-row mirror, row mirror), in every lane
__device__ inline double row16_sum(double v)
{
    v += dpp_d<0xB1>(v);
    v += dpp_d<0x4E>(v);
    v += dpp_d<0x141>(v);
    v += dpp_d<0x140>(v);
    return v;
}

// prefetch depth (stages) of the chains' coefficient loads

// ---- forward rollout: x~_{s+1} = [A~ dx_s + B~ du_s + c_s ; du_s], du_s = K_s x~_s + k_s ---------------------
// fac: k_s from the record and c_s = c~_s from the table (solve after a factorisation); otherwise the
// refinement sweep's k_ref (backward_chain post-pass) and c_s = rc_s.  Lanes: gain row a = lane / 16 over
// columns j = lane % 16 (+ column 16 on j = 0), DPP row sum, du broadcast by readlane; state row o = lane / 2,
// half h = lane % 2 (A~ entries 4h .. 4h + 3; the second half adds B~ du and c), DPP pair sum.
__device__ __attribute__((always_inline)) inline void forward_chain(const Model &M, Smem &S, const Ctl &C, gdouble *ws,
                                                                    int fac)
{
    WS_TRAJ(ws);
    const int lane = opaque_lane();
    const int N = C.N;
    const int a1 = lane >> 4, j1 = lane & 15;
    const double m16 = (j1 == 0) ? 1.0 : 0.0;
    const int h = lane & 1, o = min(lane >> 1, NA - 1), oi = min(o, NX - 1);
    const double bwx = uniform(M.bwx), bwy = uniform(M.bwy), bwz = uniform(M.bwz);
    int acol[4];
    ACoef ac[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int e = 4 * h + t;
        acol[t] = c_at.rcol[oi][e];
        ac[t] = acoef((o < NX) ? (int)c_at.rsrc[oi][e] : SRC_ZERO);
    }
    // B~ du on the second half of rows 3..5 (dt g(q) / m sum(du), table slot) and 10..12 (rotor torque map),
    // as per-lane coefficients (zero elsewhere) so that every lane runs the same instructions
    double isv = (h == 1 && o >= 3 && o < 6) ? 1.0 : 0.0;
    asm volatile("" : "+v"(isv));   // keep it a multiplier (a select on it compiles to a divergent branch)
    const int bvoff = TB_G + BV_SLOT + min(max(o - 3, 0), 2);
    const double tcx = (h == 1 && o == 10) ? bwx : 0.0, tcy = (h == 1 && o == 11) ? bwy : 0.0;
    const double tcz = (h == 1 && o == 12) ? bwz : 0.0;
    const double hm = (h == 1 && o < NX) ? 1.0 : 0.0;
    // B~ du and the u_prev rows as one per-lane weighted sum bt = sum_a (isv bv + tw_a) du_a: tw = the rotor torque
    // map on the w rows (tcx (du3 - du1), tcy (du2 - du0), tcz (du0 - du1 + du2 - du3)), one-hot on the u_prev rows
    // (o = 13..16: the row IS du_{o-13}; its A~ part is zero), zero on the first half; a two-level tree after the
    // du broadcast instead of the sum / three-FMA chain / four selects
    const double ur = (h == 1 && o >= NX) ? 1.0 : 0.0;
    const double tw0 = -tcy + tcz + ((o == 13) ? ur : 0.0), tw1 = -tcx - tcz + ((o == 14) ? ur : 0.0);
    const double tw2 = tcy + tcz + ((o == 15) ? ur : 0.0), tw3 = tcx - tcz + ((o == 16) ? ur : 0.0);
    const int dof = o * SX + (o < NX ? 1 : 0);   // dx_{s+1}[o] or du_s[o - 13] (Smem::du follows Smem::dx)
    if (lane < NA) S.ring[lane] = 0.0;           // x~_0 = 0
    if (lane < NX) DX[lane * SX] = 0.0;
    sync();
    // with backward_chain's 4.  An even PF keeps the ring slot (s & 1) a constant of each unrolled step: 5 and 7
    // measured +1.2 % kernel time against 4 and 6, which were equal (profiles/chain_ab_parts.log; round 5's
    // prefetch scan: profiles/r05_ab_prefetch.log, r05_ab_retune_final_flags.log)
    constexpr int PF = 6;
    static_assert(PF % 2 == 0, "ring slot of a step fixed by its place in the body");
    double fK0[PF], fK1[PF], fkf[PF], fa[PF][4], fbv[PF], fc[PF];
    // coefficient loads from the wave-uniform workspace base (SGPR pair) plus a 32-bit per-lane byte offset: the nine
    // offsets are fixed for the sweep (opaque, so that they stay nine registers) and the stage is scalar state.  The
    // record and the table row advance once per unrolled body, the fetches inside it reach their stage by a
    // constant (the load's immediate: the table's base stands FB stages ahead to keep it within +-4 KB); the
    // feed-forward and c, whose strides differ between the solve and a refinement sweep, advance by a scalar add
    // per fetch.  The pointers are opaque where they advance: otherwise base + lane offset is hoisted as nine 64-bit
    // vector invariants and every load adds the stage to one of them.  The fetches run PF - 1 stages ahead and past
    // stage N - 1 without a clamp: what they read there stays inside the instance's workspace and is never used.
    constexpr int FL = 9;   // loads per fetch
    constexpr int FB = 3;
    static_assert(WS_REC + (MAXN + PF) * REC <= WS_END && WS_TAB + (MAXN + PF) * TB_W <= WS_END &&
                      WS_KREF + NU * SX + PF <= WS_END && WS_RC + NX * SX + PF <= WS_END,
                  "forward_chain fetches up to PF - 1 stages past the horizon");
    static_assert((PF - 1) * REC * 8 < 4096 && (PF - 1 - FB) * TB_W * 8 < 4096 && FB * TB_W * 8 <= 4096,
                  "stage constants of a body within the load's immediate");
    const gchar *ub = ws_uniform(ws);
    unsigned oK0 = (unsigned)(WS_REC + RC_K + j1 * NU + a1) * 8u, oK1 = (unsigned)(WS_REC + RC_K + 16 * NU + a1) * 8u;
    unsigned okf = (unsigned)(fac ? WS_REC + RC_KF + a1 : WS_KREF + a1 * SX) * 8u;
    unsigned oa[4], obv = (unsigned)(WS_TAB + bvoff) * 8u;
    unsigned oc = (unsigned)(fac ? WS_TAB + TB_c + oi : WS_RC + oi * SX) * 8u;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        oa[t] = (unsigned)(WS_TAB + ac[t].off) * 8u;
        asm volatile("" : "+v"(oa[t]));
    }
    asm volatile("" : "+v"(oK0), "+v"(oK1), "+v"(okf), "+v"(obv), "+v"(oc));
    const int kstr8 = uni(fac ? REC * 8 : 8), cstr8 = uni(fac ? TB_W * 8 : 8);
    const gchar *sRec = ub, *sTab = ub + FB * TB_W * 8, *sKf = ub, *sC = ub;
    // q: the stage relative to the body's first
    auto fetch = [&](int q, double &K0, double &K1, double &kf, double *a4, double &bv, double &c) {
        const gchar *r = sRec + q * REC * 8, *t4 = sTab + (q - FB) * TB_W * 8;
        K0 = gld(r, oK0);
        K1 = gld(r, oK1);
        kf = gld(sKf, okf);
#pragma unroll
        for (int t = 0; t < 4; ++t) a4[t] = gld(t4, oa[t]);
        bv = gld(t4, obv);
        c = gld(sC, oc);
        sKf += kstr8;
        sC += cstr8;
        asm volatile("" : "+s"(sKf), "+s"(sC));
    };
    auto advance = [&](int n) {
        sRec += n * REC * 8;
        sTab += n * TB_W * 8;
        asm volatile("" : "+s"(sRec), "+s"(sTab));
    };
    // the next coefficient fetch is issued right after this step's ring reads, into the slot the previous step
    // consumed (prefetch distance PF - 1 stages), so that its ~9 global loads issue under the ring reads' LDS
    // latency instead of between the step's result and its ring store (the chain's critical path)
    auto step = [&](int q, int s, double &K0, double &K1, double &kf, double *a4, double &bv, double &c,
                    double &pK0, double &pK1, double &pkf, double *pa4, double &pbv, double &pc) {
        const double *xr = S.ring + (s & 1) * RING;
        // every LDS read of the step first: one wait, then the two independent halves of the step
        const double xj = xr[j1], x16 = xr[16];
        double xa[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) xa[t] = xr[acol[t]];
        __builtin_amdgcn_sched_barrier(0);
        fetch(q, pK0, pK1, pkf, pa4, pbv, pc);
        // one counted wait for the step's nine coefficients: loads return in order and the PF - 1 fetches issued
        // after theirs may stay in flight (the chain has no global stores; every step issues a fetch).  The
        // compiler's own waits stay in force behind it and add nothing while the count is right.
        __builtin_amdgcn_s_waitcnt(waitcnt_vm(chain_vm(PF, FL, 0, 0)));
        __builtin_amdgcn_sched_barrier(0);
        double y = K0 * xj;
        y = fma(K1 * m16, x16, y);
        double acc = 0.0;
#pragma unroll
        for (int t = 0; t < 4; ++t) acc = fma(a4[t], xa[t], acc);
        acc = fma(hm, c, acc);
        const double bvl = isv * bv;
        const double w0 = bvl + tw0, w1 = bvl + tw1, w2 = bvl + tw2, w3 = bvl + tw3;
        y = row16_sum(y) + kf;
        const double d0 = readlane_d(y, 0), d1 = readlane_d(y, 16), d2 = readlane_d(y, 32), d3 = readlane_d(y, 48);
        acc += fma(w0, d0, w1 * d1) + fma(w2, d2, w3 * d3);
        const double v = pair_sum(acc);
        // every lane stores: the two halves of a row and the lanes past 2 NA (o clamped to 16) hold identical
        // values for identical addresses (no exec-mask branch in the step)
        S.ring[((s + 1) & 1) * RING + o] = v;
        DX[dof + s] = v;
        sync();
    };
#pragma unroll
    for (int q = 0; q < PF - 1; ++q) {
        fetch(q, fK0[q], fK1[q], fkf[q], fa[q], fbv[q], fc[q]);
        __builtin_amdgcn_sched_barrier(0);   // fetch by fetch, the order the steps' counted waits assume
    }
    advance(PF - 1);
#define FSLOT(q) fK0[q], fK1[q], fkf[q], fa[q], fbv[q], fc[q]
    int s = 0;
    for (; s + PF <= N; s += PF) {   // straight-line body, step slot = s % PF, fetch slot = (s - 1) % PF
#pragma unroll
        for (int q = 0; q < PF; ++q) step(q, s + q, FSLOT(q), FSLOT((q + PF - 1) % PF));
        advance(PF);
    }
#pragma unroll
    for (int q = 0; q < PF - 1; ++q)
        if (s + q < N) step(q, s + q, FSLOT(q), FSLOT((q + PF - 1) % PF));
#undef FSLOT
    vm_sync();   // the step goes to other lanes' stage-parallel passes through HBM
}

// ---- P_k's packed rows 0..12 (the x rows) as a stream of 16-byte pieces, lane = stage --------------------------
// f(a, b, P(a, b)) for every packed entry (a, b >= a) of rows a < NX, in packed order.  The pieces go out in blocks of
// PB = 24, every load of a block issued before its first use (sched_barrier): left to itself the compiler issued
// four loads at a time and waited for them before the next four, 18 dependent round trips to L2 / MALL per pass
// (the costates pass took 2.3x its unloaded time in a full launch).  The order of the f calls is the packed order
// whatever the block size, so every sum built from them is the same FMA chain.
// issued(): called once, after the last block's loads are issued and before their first use: a caller's own loads
// placed there return behind the stream's and wait under the last block's arithmetic.
template <typename F, typename G>
__device__ __attribute__((always_inline)) inline void p_rows_stream(const gdvec2 *pp2, F &&f, G &&issued)
{
    constexpr int NE = up17(NX - 1, NA - 1) + 1;   // entries of rows 0..12
    constexpr int NP = (NE + 1) / 2;               // 16-byte pieces
    constexpr int PB = 24;
#pragma unroll
    for (int q0 = 0; q0 < NP; q0 += PB) {
        dvec2 buf[PB];
#pragma unroll
        for (int i = 0; i < PB; ++i)
            if (q0 + i < NP) buf[i] = pp2[q0 + i];
        if (q0 + PB >= NP) issued();
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int a = 0; a < NX; ++a)
#pragma unroll
            for (int b = a; b < NA; ++b) {
                const int e = up17(a, b), q = e >> 1;
                if (q < q0 || q >= q0 + PB) continue;
                f(a, b, (e & 1) ? buf[q - q0].y : buf[q - q0].x);
            }
    }
}

template <typename F>
__device__ __attribute__((always_inline)) inline void p_rows_stream(const gdvec2 *pp2, F &&f)
{
    p_rows_stream(pp2, f, [] {});
}

// ---- costates by the Riccati identity (stage-parallel, lane = k - 1) ------------------------------------------
// lam+_{k-1} = (P_k dx~_k + p_k)[x rows] after a factorisation (p_k from [F], p_N = h~ terminal gradient), and
// lam+_{k-1} = (P_k (dx~_k - c~_{k-1}) + ph_k)[x rows] after a refinement sweep (ph_k = p_k + P_k c~_{k-1} from
// backward_chain, c~ = rc): the cost-to-go gradient at the new state, equal to the adjoint recursion's value
// (the oracle's recursion) up to rounding.  dx~_k = [dx_k ; du_{k-1}].
// ADD: the instance that ends a refinement step (fac = 0) and also forms the refined solution.  dx, du and lam+ then
// hold the sweep's correction, `add` is the backup set with the solution the sweep started from, and lane l writes
// backup + correction over the elements of its own stage, the ones it reads and writes anyway: lam+ of stage l, dx of
// stage l + 1, du of stage l.  dx of stage 0 is left as forward_chain wrote it: 0 in every correction and every
// solution.  The 30 backup loads go out behind the last block of the P_k stream and return under its arithmetic; the
// correction is read from LDS again (xt has c~ subtracted) before any sum is written, and no lane touches another
// lane's elements.  A template parameter, not a run-time flag: with a wave-uniform branch around the loads inside the
// stream, linear_solve took 240 accumulation registers instead of 114 and ipm_kernel's scratch operations around the
// call went from 140 to 802.
template <bool ADD>
__device__ __attribute__((always_inline)) inline void costates_identity(Smem &S, const Ctl &C, gdouble *ws, int fac,
                                                                        const gdouble *add)
{
    WS_TRAJ(ws);
    const int lane = opaque_lane();
    const int N = C.N;
    if (lane < N) {
        const int k = lane + 1;
        const gdouble *pp = ws + WS_PST + pst_at(k - 1, 0);   // entry e at pp[pst_at(0, e)]
        const gdouble *rc = ws + WS_RC;
        double xt[NA];
#pragma unroll
        for (int j = 0; j < NX; ++j) xt[j] = DX[j * SX + k];
#pragma unroll
        for (int a = 0; a < NU; ++a) xt[NX + a] = DU[a * SX + k - 1];
        if (ADD || !fac) {
#pragma unroll
            for (int j = 0; j < NX; ++j) xt[j] -= rc[j * SX + k - 1];
        }
        const gdouble *pv = ws + WS_PVK + (size_t)k * 18;
        const bool term = !ADD && fac && k == N;   // p_N of a factorisation: the terminal gradient (u_prev part 0)
        double acc[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) acc[i] = term ? (double)ws[WS_PN + i] : (double)pv[i];
        double bx[NX], bu[NU], bl[NX];
        // row i's terms arrive in column order (P(a, i) for a < i, then row i): lam_i + sum_j P(i, j) xt_j
        p_rows_stream((const gdvec2 *)pp, [&](int a, int b, double P) {
            acc[a] = fma(P, xt[b], acc[a]);
            if (b != a && b < NX) acc[b] = fma(P, xt[a], acc[b]);
        }, [&] {
            if (ADD) {
#pragma unroll
                for (int i = 0; i < NX; ++i) bl[i] = add[BK_LP + i * SX + k - 1];
#pragma unroll
                for (int j = 0; j < NX; ++j) bx[j] = add[BK_DX + j * SX + k];
#pragma unroll
                for (int a = 0; a < NU; ++a) bu[a] = add[BK_DU + a * SX + k - 1];
            }
        });
        if (ADD) {
            double cx[NX], cu[NU];
#pragma unroll
            for (int j = 0; j < NX; ++j) cx[j] = DX[j * SX + k];
#pragma unroll
            for (int a = 0; a < NU; ++a) cu[a] = DU[a * SX + k - 1];
            sync();
#pragma unroll
            for (int i = 0; i < NX; ++i) LP[i * SX + k - 1] = bl[i] + acc[i];
#pragma unroll
            for (int j = 0; j < NX; ++j) DX[j * SX + k] = bx[j] + cx[j];
#pragma unroll
            for (int a = 0; a < NU; ++a) DU[a * SX + k - 1] = bu[a] + cu[a];
        } else {
#pragma unroll
            for (int i = 0; i < NX; ++i) LP[i * SX + k - 1] = acc[i];
        }
    }
    vm_sync();
}

// ---- backward sweep for a refinement right-hand side (rq, rr, rc) with the last factorisation ----------------
__device__ __attribute__((always_inline)) inline void backward_chain(const Model &M, Smem &S, const Ctl &C, gdouble *ws)
{
    const int lane = opaque_lane();
    const int N = C.N;
    const gdouble *rec = ws + WS_REC, *Pst = ws + WS_PST;
    const gdouble *rq = ws + WS_RQ, *rc = ws + WS_RC;
    gdouble *pcv = ws + WS_PC, *gs = ws + WS_GS, *kref = ws + WS_KREF;
    // (0) P_s c~_{s-1}, s = 1..N (lane = s)
    for (int rep = 0; rep < 1; ++rep)
    if (lane >= 1 && lane <= N) {
        const int s = lane;
        const gdouble *pp = Pst + pst_at(s - 1, 0);   // entry e at pp[pst_at(0, e)]
        double c[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) c[i] = rc[i * SX + s - 1];
        // P_s streamed in packed order as 16-byte pieces (72 loads instead of 221 scattered 8-byte ones; lane =
        // stage, so every load instruction touches one line per lane); each row's terms still arrive in column
        // order, so every sum is the same FMA chain as the row-wise form
        double acc[NA];
#pragma unroll
        for (int j = 0; j < NA; ++j) acc[j] = 0.0;
        p_rows_stream((const gdvec2 *)pp, [&](int a, int b, double P) {
            if (b < NX) acc[a] = fma(P, c[b], acc[a]);
            if (b != a) acc[b] = fma(P, c[a], acc[b]);
        });
#pragma unroll
        for (int j = 0; j < NA; ++j) pcv[s * 18 + j] = acc[j];
    }
    vm_sync();
    // (1) the chain, lanes (j, h): column j of A~ (x columns; u_prev columns of A~ are zero), K^T row j
    const int h = lane & 1, j = min(lane >> 1, NA - 1), jc = min(j, NX - 1);
    const double xcol = (j < NX) ? 1.0 : 0.0;
    const double bwx = uniform(M.bwx), bwy = uniform(M.bwy), bwz = uniform(M.bwz);
    int crow[4];
    ACoef ac[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int e = 4 * h + t;
        crow[t] = c_at.crow[jc][e];
        ac[t] = acoef((j < NX) ? (int)c_at.csrc[jc][e] : SRC_ZERO);
    }
    const double hm = (h == 1) ? 1.0 : 0.0;
    const bool st = h == 0 && lane < 2 * NA;
    const int gsl = min(lane, NU - 1);   // g_s entry this lane stores
    if (st) {
        const double v = xcol * rq[jc * SX + N] + pcv[N * 18 + j];   // ph_N = rq_N + P_N c~_{N-1}
        S.ring[j] = v;   // ring slot 0: the slots alternate with the steps taken, not with s
        ws[WS_PVK + (size_t)N * 18 + j] = v;
    }
    sync();
    // see forward_chain's PF: even, so that the ring slot is a constant of each unrolled step (with 5, the slot's
    // address arithmetic was 14 VALU instructions of the step); 4 and 6 measured equal (profiles/chain_ab_parts.log)
    constexpr int PF = 4;
    double fa[PF][4], fbv[PF][3], frr[PF][NU], fq[PF], fp[PF], fk[PF][NU];
    // coefficient loads and the step's stores through a buffer resource: per-lane constant offsets, the stage's
    // offsets in SGPRs (global loads needed a 64-bit address per load and stage; +0.3 % with the final build flags:
    // profiles/r05_ab_chain_buffer_loads.log, r05_ab_retest_final_flags.log; forward_chain takes the SGPR-base form)
    const Rsrc wr = ws_rsrc(ws, WS_SIZE * 8);
    constexpr int FL = 14, ST = 2;   // vector-memory operations of a step: loads of its fetch, its global stores
    // the stage as four scalar byte offsets (table row, [a][s] rows, 18-wide rows, record) that a fetch steps down;
    // they stand PF - 1 stages above the fetched stage, which is the stage a step stores while it fetches, so the
    // step's two stores take the same offsets and the loads carry the distance in their per-lane constants.  Below
    // stage 0 a fetch reads inside the workspace what no step uses; only rq, at the workspace's start, is clamped.
    constexpr int D = PF - 1;
    static_assert(WS_TAB >= D * TB_W && WS_RR >= D && WS_PC >= D * 18 && WS_REC >= D * REC && WS_RQ == 0,
                  "backward_chain fetches down to stage -(PF - 1)");
    int oT = uni((N - 1 + D) * TB_W * 8), o1 = uni((N - 1 + D) * 8), oP = uni((N - 1 + D) * 18 * 8);
    int oR = uni((N - 1 + D) * REC * 8);
    unsigned va[4], vq = (unsigned)(WS_RQ + jc * SX) * 8u, vp = (unsigned)(WS_PC + j - D * 18) * 8u;
    unsigned vk = (unsigned)(WS_REC + RC_K + j * NU - D * REC) * 8u;
    unsigned vpv = (unsigned)(WS_PVK + j) * 8u, vgs = (unsigned)(WS_GS + gsl * SX) * 8u;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        va[t] = (unsigned)(WS_TAB + ac[t].off - D * TB_W) * 8u;
        asm volatile("" : "+v"(va[t]));
    }
    asm volatile("" : "+v"(vq), "+v"(vp), "+v"(vk), "+v"(vpv), "+v"(vgs));
    auto fetch = [&](int, double *a4, double *bv3, double *r4, double &q1, double &p1, double *k4) {
#pragma unroll
        for (int t = 0; t < 4; ++t) a4[t] = bld(wr, va[t], oT);
#pragma unroll
        for (int i = 0; i < 3; ++i) bv3[i] = bld(wr, (unsigned)(WS_TAB + TB_G + BV_SLOT + i - D * TB_W) * 8u, oT);
        static_assert((WS_TAB + TB_G + BV_SLOT) % 2 == 0 && TB_W % 2 == 0, "the compiler joins bv3[0], bv3[1]: FL counts one");
#pragma unroll
        for (int a = 0; a < NU; ++a) r4[a] = bld(wr, (unsigned)(WS_RR + a * SX - D) * 8u, o1);
        q1 = bld(wr, vq, max(o1 - D * 8, 0));
        p1 = bld(wr, vp, oP);
        const dvec2 k01 = bld2(wr, vk, oR);
        const dvec2 k23 = bld2(wr, vk + 16u, oR);
        k4[0] = k01.x; k4[1] = k01.y; k4[2] = k23.x; k4[3] = k23.y;
    };
    auto step_down = [&]() {
        oT -= TB_W * 8;
        o1 -= 8;
        oP -= 18 * 8;
        oR -= REC * 8;
    };
    // stage gradient g_s = B~_s^T ph_{s+1} + rr_s (model.hpp Bt_times order), identical in every lane
    auto grad = [&](const double *xr, const double *bv3, const double *r4, double *g) {
        const double v = bv3[0] * xr[3] + bv3[1] * xr[4] + bv3[2] * xr[5];
        const double ex = bwx * xr[10], ey = bwy * xr[11], ez = bwz * xr[12];
        g[0] = (v - ey + ez) + xr[NX + 0] + r4[0];
        g[1] = (v - ex - ez) + xr[NX + 1] + r4[1];
        g[2] = (v + ey + ez) + xr[NX + 2] + r4[2];
        g[3] = (v + ex - ez) + xr[NX + 3] + r4[3];
    };
    // as forward_chain: the fetch (14 buffer loads) goes out under the ring reads' LDS latency, into the slot
    // the previous step consumed (distance PF - 1)
    auto step = [&](int q, int s, double *a4, double *bv3, double *r4, double &q1, double &p1, double *k4,
                    double *pa4, double *pbv3, double *pr4, double &pq1, double &pp1, double *pk4) {
        // ring slot of ph_{s+1}: the parity of the steps taken, which an even PF makes the parity of q (an odd one
        // works and pays the slot's address arithmetic in every step)
        const int par = (PF % 2 == 0) ? (q & 1) : ((N - 1 - s) & 1);
        const double *xr = S.ring + par * RING;
        double xa[4], xg[NA];
#pragma unroll
        for (int t = 0; t < 4; ++t) xa[t] = xr[crow[t]];
#pragma unroll
        for (int i = 3; i < NA; ++i) xg[i] = xr[i];
        __builtin_amdgcn_sched_barrier(0);
        fetch(s - PF + 1, pa4, pbv3, pr4, pq1, pp1, pk4);
        // one counted wait for the step's coefficients.  Operations return in order; behind this step's fetch
        // stand PF - 1 later fetches and the stores of the steps taken since (at most PF - 1 of them; the chain's
        // t-th step has taken t, and slot q of the unrolled body is never earlier than the q-th), and the counter
        // holds 63 at the most: a smaller count than the true one only waits for more.  The compiler's own waits
        // stay in force behind it and add nothing while the count is right.
        if (q == 0) __builtin_amdgcn_s_waitcnt(waitcnt_vm(chain_vm(PF, FL, ST, 0)));
        else if (q == 1) __builtin_amdgcn_s_waitcnt(waitcnt_vm(chain_vm(PF, FL, ST, 1)));
        else if (q == 2) __builtin_amdgcn_s_waitcnt(waitcnt_vm(chain_vm(PF, FL, ST, 2)));
        else if (q == 3) __builtin_amdgcn_s_waitcnt(waitcnt_vm(chain_vm(PF, FL, ST, 3)));
        else __builtin_amdgcn_s_waitcnt(waitcnt_vm(chain_vm(PF, FL, ST, PF - 1)));
        __builtin_amdgcn_sched_barrier(0);
        double acc = 0.0;
#pragma unroll
        for (int t = 0; t < 4; ++t) acc = fma(a4[t], xa[t], acc);
        double g[NU];
        grad(xg, bv3, r4, g);
        double kt = fma(xcol, q1, p1);
#pragma unroll
        for (int a = 0; a < NU; ++a) kt = fma(k4[a], g[a], kt);
        acc = fma(hm, kt, acc);
        acc = pair_sum(acc);
        double gl = g[0];
        gl = (gsl == 1) ? g[1] : gl;
        gl = (gsl == 2) ? g[2] : gl;
        gl = (gsl == 3) ? g[3] : gl;
        // unconditional (identical values to identical addresses: both halves of column j after pair_sum, lanes
        // past 2 NA with j clamped to 16, lanes >= NU with the g index clamped to NU - 1)
        S.ring[(par ^ 1) * RING + j] = acc;
        bst(acc, wr, vpv, oP);   // ph_s for the costate identity
        bst(gl, wr, vgs, o1);    // g_s
        step_down();
        sync();
    };
#define BSLOT(q) fa[q], fbv[q], frr[q], fq[q], fp[q], fk[q]
#pragma unroll
    for (int q = 0; q < PF - 1; ++q) {
        fetch(N - 1 - q, BSLOT(q));   // (the stage is in the scalar offsets; the argument names it)
        step_down();
        __builtin_amdgcn_sched_barrier(0);   // fetch by fetch, the order the steps' counted waits assume
    }
    int s = N - 1;
    for (; s - PF >= -1; s -= PF) {   // steps s .. s - PF + 1, slot (N - 1 - s) % PF, fetch slot one behind
#pragma unroll
        for (int q = 0; q < PF; ++q) step(q, s - q, BSLOT(q), BSLOT((q + PF - 1) % PF));
    }
#pragma unroll
    for (int q = 0; q < PF - 1; ++q)
        if (s - q >= 0) step(q, s - q, BSLOT(q), BSLOT((q + PF - 1) % PF));
#undef BSLOT
    vm_sync();
    // (2) k_ref_k = -Quu_k^{-1} g_k (lane = k)
    if (lane < N) {
        const int k = lane;
        double L[10], iL[4], g[NU];
#pragma unroll
        for (int e = 0; e < 10; ++e) L[e] = rec[(size_t)k * REC + RC_L + e];
        iL[0] = L[0]; iL[1] = L[2]; iL[2] = L[5]; iL[3] = L[9];   // stored diagonal slots hold 1/l_jj
#pragma unroll
        for (int a = 0; a < NU; ++a) g[a] = gs[a * SX + k];
        chol4_solve(L, iL, g[0], g[1], g[2], g[3]);
#pragma unroll
        for (int a = 0; a < NU; ++a) kref[a * SX + k] = -g[a];
    }
    vm_sync();
}
