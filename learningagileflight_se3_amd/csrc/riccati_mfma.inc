// riccati_mfma.inc — the factorisation sweep (backward sweep of the Riccati solve) on the f64 matrix cores
// (included by ipm_kernel.hip after riccati.inc).
//
// The Newton system is the stage QP of riccati.inc's header (stage table of build_table: G_k, H~_k, h~_k, c~_k).  The
// sweep runs k = N-1 .. 0, sequential over k with the wave's 64 lanes on one stage, from the terminal value function
// P_N, p_N (riccati.inc terminal).  A stage is the value-function update of the multiple-shooting NLP of
// quad_OC.py:124-167 (Δu term quad_OC.py:145-151 -> the u~ = u_{k-1} augmentation), in four phases (the letters
// name them in the comments and the phase timers):
//   [C]  W = P G                                      (P = P_{k+1}; with it the gradient's ph = p + P c~)
//   [D]  M = G^T W + H~ (+ delta_w on the flagged diagonal),  g = G^T ph + h~;  M = [[Qxx, Qxu], [Qux, Quu]]
//   [E]  Cholesky of Quu (4 x 4; a pivot that is not positive is wrong inertia),  K = -Quu^{-1} Qux,  k = -Quu^{-1} g_u
//   [F]  P' = Qxx + Qux^T K,  p' = g_x + Qux^T k      (P_k, p_k: the next stage's P, p)
// Outputs, in the x~ = [r v q w u~] order the chains read:
//   * the factor record of every stage k = 0..N-1 (WS_REC, REC doubles: K_k^T [j][4] at RC_K, k_k at RC_KF, the packed
//     factor L_k of Quu_k at RC_L with 1 / l_jj in its diagonal slots),
//   * P_k packed (upper triangle of the 17 x 17, NUP17 entries at stride PSTR) in slot k - 1 of WS_PST for k = 1..N
//     (terminal stores P_N),
//   * p_k at WS_PVK + 18 k for k = 1..N-1 (p_N: WS_PN, the x rows),
//   * the return value: 1, or 0 when some Quu_k is not positive definite (wrong inertia); the outputs of a failed
//     sweep are partial and the caller retries with another delta_w, which overwrites them.
//
// MFMA order.  The 17 x~ entries are taken as m = 0..15 <-> x~ index m + 1 (r1 r2 v q w u~) and m = 16 <-> r0,
// the 17 active G columns likewise (m = 0..11 <-> x 1..12, 12..15 <-> u, 16 <-> r0).  r0 enters the dynamics only
// through r0' = r0 + dt v0, so in this order
//   G = [[G11, 0], [dt e_2^T, 1]]       (e_2 = v0)
// and the 16 x 16 blocks go to v_mfma_f64_16x16x4_f64 while the r0 border is a handful of vector terms:
//   W11 = P11 G11 + dt p12 e_2^T,       M11 = G11^T W11 + dt e_2 w21 + H~11,   w21 = y^T + dt p22 e_2^T,
//   y = G11^T p12,                      M(:, r0) = w21^T,  M(r0, r0) = p22 (+ H~),
//   g11 = G11^T p + W11^T c~ + c~_r0 y + dt e_2 (p_r0 + p22 c~_r0) + h~   (= G^T (p + P c~) + h~).
// Register layouts (lane l, group g = l >> 4, column c = l & 15; gfx950 f64 MFMA: A lane l = A[l&15][k = l>>4],
// B lane l = B[k = l>>4][l&15], D reg s of lane l = D[4s + (l>>4)][l&15]):
//   * P11 in D layout.  P is symmetric, so its D registers are also the A operand of P G (k-step s = register s),
//     and the product's D registers W are the B operand of G^T W; G11 is gathered once per stage in B layout and
//     serves as B (P G) and, read as G^T, as A (G^T W).  P' = Qxx + Qux^T K is one more MFMA whose A operand
//     Qux(g, c) is register 3 of M11 in the lane itself (M11 row 12 + g = u_g) and whose B operand K(g, c) the lane
//     solves: P stays in registers from stage to stage, no W / M / P round trip through LDS.
//   * vectors indexed by x~ "row-group" (lane holds v[4s + g], s = 0..3) or "column" (lane holds v[c]); the one
//     transposition per stage (p12', p' column -> row-group) goes through 32 doubles of LDS.
//   * Quu (M11 rows / columns 12..15) and the r0 / g_u right-hand sides are read with v_readlane: the 4 x 4
//     Cholesky (inertia test) of [E] is a wave-uniform chain, the same in every lane.
// The f64 matrix core shares the FP64 pipeline with the VALU on gfx950 (tools/ubench_mfma.hip: an MFMA and
// independent v_fma_f64 do not overlap), so the gain is instruction count: 4 MFMAs form a dense 16 x 16 x 16
// product that takes ~60 FMAs per lane on the VALU, plus the LDS exchanges around them.

typedef double d4v __attribute__((ext_vector_type(4)));

__device__ inline d4v mfma64(double a, double b, d4v c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// 1 / sqrt(d) for the pivot chain: v_rsq_f64 (relative error <= 2^-23) and one third-order correction,
// y + y r (1/2 + 3 r / 8) with r = 1 - d y^2 (error O(r^3) < 2^-64): four dependent operations after the rsq where
// two Newton steps take six.  d <= 0 gives NaN, and the stage returns "wrong inertia" before any of it
// is stored.
__device__ inline double rsqrt_chol(double d)
{
    const double y = __builtin_amdgcn_rsq(d);
    const double r = fma(-(d * y), y, 1.0);
    return fma(y * r, fma(r, 0.375, 0.5), y);
}

// sum over the four 16-lane groups (lanes c, c + 16, c + 32, c + 48), identical in all four: two half exchanges
// (v_permlane32_swap, v_permlane16_swap; no LDS), each combining a lane with a partner that combines it back
__device__ inline double grp4_sum(double v)
{
    long long b = __double_as_longlong(v);
    int lo = (int)b, hi = (int)(b >> 32);
    const auto r0 = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    const auto r1 = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    const double a0 = __longlong_as_double(((long long)(unsigned)r1[0] << 32) | (unsigned)r0[0]);
    const double a1 = __longlong_as_double(((long long)(unsigned)r1[1] << 32) | (unsigned)r0[1]);
    const double s = a0 + a1;
    b = __double_as_longlong(s);
    lo = (int)b;
    hi = (int)(b >> 32);
    const auto q0 = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const auto q1 = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    const double c0 = __longlong_as_double(((long long)(unsigned)q1[0] << 32) | (unsigned)q0[0]);
    const double c1 = __longlong_as_double(((long long)(unsigned)q1[1] << 32) | (unsigned)q0[1]);
    return c0 + c1;
}

// the value of the lane 16 below (rows 1 and 3 take rows 0 and 2; v_permlane16_swap, both dwords)
__device__ inline double swap16_d(double v)
{
    const long long b = __double_as_longlong(v);
    const int lo = (int)b, hi = (int)(b >> 32);
    const auto r0 = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const auto r1 = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    return __longlong_as_double(((long long)(unsigned)r1[0] << 32) | (unsigned)r0[0]);
}

// ---- per-lane gather / store tables of the MFMA stage (compile time) --------------------------------------
__host__ __device__ constexpr int mf_x(int m) { return m + 1; }                                 // m -> x~ index
__host__ __device__ constexpr int mf_z(int m) { return (m + 1) < NX ? (m + 1) : (m + 1) + NU; }  // m -> z index
constexpr int MF_ZERO = -1;

// table slot of G(x~ row R, z column z): a stage-dependent slot, a per-row constant (TB_K: the identity entries, dt and
// the rotor torque map, which build_table writes into every row) or a structural zero
__host__ __device__ constexpr int mf_gsrc(int R, int z)
{
    for (int t = 0; t < GLEN; ++t) {
        if (g_row(z, t) != R) continue;
        const int v = gslot(z, t);
        if (v >= 0) return TB_G + v;
        if (z < 3) return TB_K + 0;                        // r columns: 1
        if (z < 6) return t == 0 ? TB_K + 1 : TB_K + 0;    // v columns: dt (r row), 1
        if (z < 13) return TB_K + 0;                       // q / w diagonal: 1
        if (z >= 17) {
            const int a = z - 17;
            if (t == 6) return TB_K + 0;                   // u~ row: 1
            const int d = t - 3;                           // rotor torque map Bw(d, a) (model.hpp)
            if (d == 0) return a == 1 ? TB_K + 3 : (a == 3 ? TB_K + 2 : MF_ZERO);
            if (d == 1) return a == 0 ? TB_K + 5 : (a == 2 ? TB_K + 4 : MF_ZERO);
            return (a & 1) ? TB_K + 7 : TB_K + 6;
        }
        return MF_ZERO;
    }
    return MF_ZERO;
}

struct MfTab {
    short g[WAVE][4];          // G11 in B layout: G(4s + g, c)
    short h[WAVE][4];          // H~11 in D layout: H~(4s + g, c)
    short ct[WAVE][4];         // c~ in row-group layout: c~(4s + g)
    short pst[WAVE][4];        // packed index of P'(4s + g, c) in x~ order when it is in the upper triangle, else -1
    unsigned char hf[WAVE][4]; // delta_w flag of that H~ entry (riccati_tables.hpp: 1 x diagonal, 2 u diagonal)
    short hc[16];              // h~ of active column c
    short hu[16];              // h~ of x~ column c >= 12 (u~), the value gradient's u~ entries
};
__host__ __device__ constexpr MfTab make_mftab()
{
    MfTab T{};
    const HTab H = make_htab();
    for (int l = 0; l < WAVE; ++l) {
        const int g = l >> 4, c = l & 15;
        for (int s = 0; s < 4; ++s) {
            const int r = 4 * s + g;
            T.g[l][s] = (short)mf_gsrc(mf_x(r), mf_z(c));
            const int zi = mf_z(r), zj = mf_z(c);
            const int e = H.idx[(zi < zj ? zi : zj) * 21 + (zi < zj ? zj : zi)];
            T.h[l][s] = (short)(e >= 0 ? TB_H + e : MF_ZERO);
            T.hf[l][s] = (unsigned char)(e >= 0 ? H.e[e].flag : 0);
            T.ct[l][s] = (short)(r < 12 ? TB_c + mf_x(r) : MF_ZERO);
            T.pst[l][s] = (short)(r <= c ? up17(mf_x(r), mf_x(c)) : -1);
        }
    }
    for (int c = 0; c < 16; ++c) {
        T.hc[c] = (short)(TB_h + mf_z(c));
        T.hu[c] = (short)(c >= 12 ? TB_h + NX + (c - 12) : MF_ZERO);
    }
    return T;
}
__constant__ MfTab c_mf = make_mftab();

// LDS of the sweep (in the W / M union of Smem, unused by the MFMA stage otherwise)
constexpr int MF_ROW = 0;                  // [168] the stage's table row (row[160] = 0: the structural zeros)
constexpr int MF_QB = 168;                 // [72] Qux columns [c][4]; M(u, r0) at 64..67, g_u at 68..71
constexpr int MF_TV = MF_QB + 72;          // [32] p12', p' transposed: [v][g][s] = v(4s + g)
constexpr int MF_DUM = MF_TV + 32;         // [64 * 4 + 32] per-lane write-only slots of the branch-free stores
constexpr int MF_TR = MF_DUM + 4 * WAVE + 32;   // [12 * 17] Qxx's x rows, row-major (the [F] transposition)
constexpr int MF_TRS = 17;   // its row stride: the transposed read (lane = row) at stride 16 was a 16-way bank conflict
constexpr int MF_QU = MF_TR + 12 * MF_TRS;   // [16] the u~ lanes' Qux column / right-hand side, diag(H~(u~_a, u_a)) (per sweep)
static_assert(MF_QU + 16 <= NA * GST + NZ * GST && MF_QU % 2 == 0, "MFMA sweep LDS inside the W / M union");
static_assert(TB_W <= 160 && MF_ROW + 168 <= MF_QB && MF_QB % 2 == 0 && MF_TV % 2 == 0 && MF_DUM % 2 == 0, "LDS map");

// The sweep's per-lane tables in LDS (Smem::mfo, Smem::mfp), built once per workgroup: the kernels are persistent
// and the tables depend on the lane alone, so every sweep of every instance reads them back with a few ds_read
// instead of rebuilding them from c_mf (seven constant-memory loads, a wait for them, the slot -> address arithmetic
// of 18 entries per lane) and from nested selects on the lane index (compiled to exec-mask branches).  All of mfo is
// stored ready to use, as 16-bit byte offsets from Smem: the gathers of G and H~ (four each), of h~ (2), and the
// lane's LDS targets qx_dst, q_src, tv_dst and its kbuf row.
constexpr int MFO_G = 0, MFO_H = 4, MFO_HC = 8, MFO_HU = 9, MFO_QX = 10, MFO_QS = 11, MFO_TV = 12, MFO_KB = 13;
__host__ __device__ constexpr unsigned mf_w_off(int e) { return (unsigned)(offsetof(Smem, W) + 8 * e); }   // &S.W[e]
__host__ __device__ constexpr unsigned mf_row_off(int slot) { return mf_w_off(MF_ROW + (slot < 0 ? 160 : slot)); }
static_assert(sizeof(Smem) < 65536, "Smem offsets fit 16 bits");
// a table entry as a 32-bit offset.  The empty asm keeps the zero extension at the load, where ds_read_u16 does it: left
// to the block of the first use it was a v_and per entry and sweep
__device__ inline unsigned mf_ld16(const unsigned short &e)
{
    unsigned v = e;
    asm volatile("" : "+v"(v));
    return v;
}
__device__ inline void init_mf_tables(Smem &S)
{
    const int lane = lane_id();
    const int g = lane >> 4, c = lane & 15;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        S.mfo[MFO_G + s][lane] = (unsigned short)mf_row_off(c_mf.g[lane][s]);
        S.mfo[MFO_H + s][lane] = (unsigned short)mf_row_off(c_mf.h[lane][s]);
        const int pe = c_mf.pst[lane][s];
        S.mfp[lane][s] = pe < 0 ? MF_OOB : (unsigned)(WS_PST + pe) * 8u;
    }
    S.mfo[MFO_HC][lane] = (unsigned short)mf_row_off(c_mf.hc[c]);
    S.mfo[MFO_HU][lane] = (unsigned short)mf_row_off(c_mf.hu[c]);
    // LDS targets of the stage's branch-free stores: Qux(u, r0) / g_u (lanes of columns 12..15), p12' / p' transposed
    // (group 0), the solved column's record row (lane 16: the r0 column, lane 17: k)
    const int dum = MF_DUM + lane;   // write-only: neighbouring lanes' slots may overlap
    S.mfo[MFO_QX][lane] = (unsigned short)mf_w_off((c >= 12) ? MF_QB + 64 + (c - 12) : dum);
    S.mfo[MFO_TV][lane] = (unsigned short)mf_w_off((g == 0) ? MF_TV + (c & 3) * 4 + (c >> 2) : dum);
    // Qux column c (u~ columns: H~(u~, u) e); lane 16 takes M(u, r0) instead, so that its p12' / p' are the r0
    // corner p22' / p_r0' (lane 16's own column is lane 0's, whose results it duplicates otherwise)
    S.mfo[MFO_QS][lane] = (unsigned short)mf_w_off((lane == 16) ? MF_QB + 64 : ((c < 12) ? MF_QB + 4 * c : MF_QU + 4 * (c - 12)));
    S.mfo[MFO_KB][lane] = (unsigned short)(offsetof(Smem, kbuf) + 8 * ((lane == 16) ? 0 : ((lane == 17) ? RC_KF : mf_x(c) * NU)));
    sync();
}
// c~ in row-group layout needs no table: c~(4 s + g) of the x rows (s < 3) is one lane offset plus 32 s bytes, and
// register 3 (the u~ rows) is the row's zero slot
__host__ __device__ constexpr bool mf_ct_is_strided()
{
    const MfTab T = make_mftab();
    for (int l = 0; l < WAVE; ++l)
        for (int s = 0; s < 4; ++s)
            if (T.ct[l][s] != (s < 3 ? TB_c + 1 + (l >> 4) + 4 * s : MF_ZERO)) return false;
    return true;
}
static_assert(mf_ct_is_strided(), "c~ gather of the MFMA stage: TB_c + 1 + g + 4 s, zero in register 3");
// The delta_w flags need no table: H~'s flagged entries are its diagonal, which lane (g, c) holds in register s
// where 4 s + g == c, and the u diagonal (flag 2) is columns 12..15, that is s == 3.
__host__ __device__ constexpr bool mf_flags_are_diagonal()
{
    const MfTab T = make_mftab();
    for (int l = 0; l < WAVE; ++l)
        for (int s = 0; s < 4; ++s) {
            const bool d = (l & 15) - (l >> 4) == 4 * s;
            if ((T.hf[l][s] != 0) != d || (T.hf[l][s] == 2) != (d && s == 3)) return false;
        }
    return true;
}
static_assert(mf_flags_are_diagonal(), "delta_w flags of the MFMA stage: the diagonal, u in register 3");

// diagnostic sub-phase timers of the stage (timer build with -DLAFSE3_PT_FINE: slots 16..23, tools/gpu_timers_fine.py)
#if defined(LAFSE3_PT_FINE) && defined(LAFSE3_PHASE_TIMERS)
#define PT_FINE(i) PT_END(S, 16 + (i))
#else
#define PT_FINE(i) ((void)0)
#endif

// Returns 1 on success, 0 when some Quu is not positive definite (wrong inertia).
__device__ __attribute__((always_inline)) inline int backward_mfma(const Model &M, const Attitude &at, Smem &S, const Ctl &C,
                                                                   gdouble *ws, double dw, int mode_lsq)
{
    const int lane = opaque_lane();
    const int g = lane >> 4, c = lane & 15;
    const int N = C.N;
    gdouble *Rec = ws + WS_REC;
    const Rsrc rs = ws_rsrc(ws, WS_SIZE * 8);
    // stage table rows: three coalesced loads one stage ahead, the row written to LDS and the stage's operands
    // gathered from there (a per-lane gather straight from HBM costs the CU's address unit ~17 scattered loads per
    // stage).  Stage N - 1's row goes out before the terminal stage, whose work covers its latency.
    auto load_row3 = [&](int k, double &t0, double &t1, double &t2) {
        const int so = uni((WS_TAB + k * TB_W) * 8);
        t0 = bld(rs, (unsigned)lane * 8u, so);
        t1 = bld(rs, (unsigned)(64 + lane) * 8u, so);
        t2 = bld(rs, (unsigned)(128 + min(lane, TB_W - 129)) * 8u, so);
    };
    double r0, r1, r2;
    load_row3(N - 1, r0, r1, r2);
    terminal(M, at, S, C, ws, dw, mode_lsq, 0);   // P_N, p_N -> S.P / S.p (x~ order), Pst[N-1], WS_PN
    double *L0 = S.W;   // sweep LDS base (MF_*)
    // the lane's tables from LDS (init_mf_tables): gather offsets in bytes from Smem, packed-P store offsets
    char *Sb = (char *)&S;
    auto lds = [&](unsigned off) { return *(const double *)(Sb + off); };
    unsigned og[4], oh[4], oc[4];
    unsigned op[4];
    double e2[4], e12[4];
    {
        const uint4 pv = *(const uint4 *)S.mfp[lane];
        op[0] = pv.x; op[1] = pv.y; op[2] = pv.z; op[3] = pv.w;
    }
    const unsigned ocb = mf_row_off(TB_c + 1) + 8u * (unsigned)g;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        og[s] = mf_ld16(S.mfo[MFO_G + s][lane]);
        oh[s] = mf_ld16(S.mfo[MFO_H + s][lane]);
        oc[s] = (s < 3) ? ocb + 32u * s : mf_row_off(MF_ZERO);
        e12[s] = (c - g == 4 * s) ? dw : 0.0;   // x and u diagonal: + delta_w (stages k >= 1)
        e2[s] = (s == 3) ? e12[s] : 0.0;        // u diagonal: + delta_w (stage 0: x_0 is fixed)
    }
    const unsigned ohc = mf_ld16(S.mfo[MFO_HC][lane]), ohu = mf_ld16(S.mfo[MFO_HU][lane]);
    // the lane's LDS targets (init_mf_tables has what they are); the right-hand side is the Qux column except in
    // lane 17, which solves for k from g_u
    const unsigned qx_dst = mf_ld16(S.mfo[MFO_QX][lane]), q_src = mf_ld16(S.mfo[MFO_QS][lane]);
    const unsigned tv_dst = mf_ld16(S.mfo[MFO_TV][lane]);
    const unsigned kb_dst = mf_ld16(S.mfo[MFO_KB][lane]);
    const unsigned rhs_src = (lane == 17) ? mf_w_off(MF_QB + 68) : q_src;
    const bool isx = c < 12;
    const double dt = M.dt;
    const double m2dt = (c == 2) ? dt : 0.0, r2dt = (g == 2) ? dt : 0.0;
    const double idm = (c >= 12) ? 1.0 : 0.0;   // W's u columns: + P(:, u~)
    const bool solve_col = lane != 16 && lane != 17;
    auto put_row = [&](double t0, double t1, double t2) {
        L0[MF_ROW + lane] = t0;
        L0[MF_ROW + 64 + lane] = t1;
        L0[MF_ROW + 128 + min(lane, TB_W - 129)] = t2;
    };
    if (lane == 0) L0[MF_ROW + 160] = 0.0;
    put_row(r0, r1, r2);
    // the u~ block of Q (the Δu coupling, the same on every stage): H~(u~_a, u~_a), H~(u~_a, u_a)
    const double dupup = L0[MF_ROW + TB_H + 50 + g];
    const double dupu = L0[MF_ROW + TB_H + 54 + (c >= 12 ? c - 12 : 0)];
    const double cf3 = (c == 12 + g) ? dupup : 0.0;           // Q(u~_g, u~_g): C of [F], register 3
    if (c >= 12 && g == 0) {
#pragma unroll
        for (int a = 0; a < 4; ++a) L0[MF_QU + 4 * (c - 12) + a] = (a == c - 12) ? dupu : 0.0;
    }
    const double hx = isx ? 0.5 : 0.0;   // [F]'s C: (M + M^T) / 2 on the x block, 0 in the u~ columns
    // P_N in registers: P11 (D layout), p12 / p (row-group), p22 / p_r0
    d4v Pm;
    double p12r[4], pr[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int R = mf_x(4 * s + g);
        Pm[s] = S.P[R * PST + mf_x(c)];
        p12r[s] = S.P[R * PST];
        pr[s] = S.p[R];
    }
    double p22 = S.P[0], p16 = S.p[0];
    struct Pf {
        double G[4], H[4], Ct[4], hc, hu, c16, hr0, Hr0;
    };
    auto gather = [&](Pf &f) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            f.G[s] = lds(og[s]);
            f.H[s] = lds(oh[s]);
            f.Ct[s] = lds(oc[s]);
        }
        f.hc = lds(ohc);
        f.hu = lds(ohu);
        f.c16 = L0[MF_ROW + TB_c];
        f.hr0 = L0[MF_ROW + TB_h];
        f.Hr0 = L0[MF_ROW + TB_H];
    };
    Pf cur;
    gather(cur);
    vm_sync();
    PT_BEGIN(S);
    // one stage: 0 = wrong inertia, 1 = next stage, 2 = done (stage 0); ee = the diagonal's delta_w
    auto stage = [&](const int k, const double (&ee)[4]) -> int {
        // the next stage's row: loaded first (pinned at the top), written to LDS and gathered just before this
        // stage's first store (a wait for a load issued before a store waits for the store too: LLVM orders vmcnt
        // by type on gfx9, so a row consumed after a store would wait for the store's completion)
        double t0, t1, t2;
        load_row3(max(k - 1, 0), t0, t1, t2);
        __builtin_amdgcn_sched_barrier(0);
        const double dwx = (k >= 1) ? dw : 0.0;
        PT_END(S, 12);
        // [C] W = P G + dt p12 e_v0^T.  G's u~ rows (k-step 3) are [0 | I]: W(:, u) += P(:, u~) in the lane's own
        // registers instead of a fourth MFMA (P's D layout holds P(4s + g, c) = P(c, 4s + g) up to rounding)
        d4v Wm = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 3; ++s) Wm = mfma64(Pm[s], cur.G[s], Wm);
#pragma unroll
        for (int s = 0; s < 4; ++s) Wm[s] = fma(m2dt, p12r[s], fma(idm, Pm[s], Wm[s]));
        PT_FINE(0);
        // [D] M = G^T W + H~ (+ delta_w on the flagged diagonal); k-step 3 again the identity: M(u~ rows) += W
        d4v Mm;
#pragma unroll
        for (int s = 0; s < 4; ++s) Mm[s] = cur.H[s] + ee[s];
#pragma unroll
        for (int s = 0; s < 3; ++s) Mm = mfma64(cur.G[s], Wm[s], Mm);
        Mm[3] += Wm[3];
        PT_FINE(1);
        // [E] the pivot chain first (the stage's critical path: Quu -> Cholesky -> solve -> the [F] MFMA -> the
        // next stage's products); the gradient and border vectors and the LDS traffic fill its latency
        const double M3 = Mm[3];
        int ok = 1;
        double L[10], iL[4];
        {
            const double q00 = readlane_d(M3, 12), q01 = readlane_d(M3, 13), q02 = readlane_d(M3, 14), q03 = readlane_d(M3, 15);
            const double q11 = readlane_d(M3, 29), q12 = readlane_d(M3, 30), q13 = readlane_d(M3, 31);
            const double q22 = readlane_d(M3, 46), q23 = readlane_d(M3, 47), q33 = readlane_d(M3, 63);
            double d = q00;
            if (!(d > 0.0)) ok = 0;
            iL[0] = rsqrt_chol(d);
            L[1] = q01 * iL[0];
            L[3] = q02 * iL[0];
            L[6] = q03 * iL[0];
            d = q11 - L[1] * L[1];
            if (!(d > 0.0)) ok = 0;
            iL[1] = rsqrt_chol(d);
            L[4] = (q12 - L[3] * L[1]) * iL[1];
            L[7] = (q13 - L[6] * L[1]) * iL[1];
            d = q22 - L[3] * L[3] - L[4] * L[4];
            if (!(d > 0.0)) ok = 0;
            iL[2] = rsqrt_chol(d);
            L[8] = (q23 - L[6] * L[3] - L[7] * L[4]) * iL[2];
            d = q33 - L[6] * L[6] - L[7] * L[7] - L[8] * L[8];
            if (!(d > 0.0)) ok = 0;
            iL[3] = rsqrt_chol(d);
            L[0] = iL[0]; L[2] = iL[1]; L[5] = iL[2]; L[9] = iL[3];
        }
        // r0 border and the gradient: y = G11^T p12, g11, p12 . c~ (column layout after the group sums)
        double yp = 0.0, gp = 0.0, pc = 0.0;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            yp = fma(cur.G[s], p12r[s], yp);
            gp = fma(cur.G[s], pr[s], gp);
            gp = fma(Wm[s], cur.Ct[s], gp);
            pc = fma(p12r[s], cur.Ct[s], pc);
        }
        const double y = grp4_sum(yp);
        gp = grp4_sum(gp);
        pc = grp4_sum(pc);
        const double w21 = fma(m2dt, p22, y);   // M(c, r0) = M(r0, c)
        Mm[0] = fma(r2dt, w21, Mm[0]);          // M row v0 += dt w21
        // Qxx's x block transposed through LDS (consumed only by [F], under the pivot chain's latency): [F]'s C operand
        // is (M + M^T) / 2, so that P' = C - Y^T Y comes out of the MFMA symmetric bit for bit (M = G^T (P G) is not,
        // and a P whose halves differ by rounding lost accuracy on the ill-conditioned delta_w = 0 systems of the IFT
        // mode: tests/test_gpu_parity.py::test_sol_gradient_ift_mode_matches_oracle)
        {
            double *T = L0 + MF_TR;
#pragma unroll
            for (int s = 0; s < 3; ++s) T[(4 * s + g) * MF_TRS + c] = Mm[s];
        }
        const double g11 = gp + fma(cur.c16, y, fma(m2dt, fma(p22, cur.c16, p16), cur.hc));
        const double gr0 = fma(p22, cur.c16, p16 + pc) + cur.hr0;
        const double m22 = p22 + (cur.Hr0 + dwx);
        const double pnb = (lane == 16) ? gr0 : (isx ? g11 : cur.hu);   // p' base (the last read of this stage's operands)
        const double p12b = (lane == 16) ? m22 : (isx ? w21 : 0.0);
        PT_END(S, 13);
        // one solve per lane: column c of Qux (u~ columns: H~(u~, u) e), lane 16 M(u, r0), lane 17 g_u
        L0[MF_QB + c * 4 + g] = M3;   // Qux(g, c)
        *(double *)(Sb + qx_dst) = w21;        // M(u_a, r0)
        *(double *)(Sb + qx_dst + 32) = g11;   // g_u
        sync();   // cross-lane LDS exchange: the compiler must not move the reads above the other lanes' writes
        double qc[4], tv[3];
        double x0, x1, x2, x3;
        {
            const double *T = L0 + MF_TR;
#pragma unroll
            for (int s = 0; s < 3; ++s) tv[s] = T[min(c, 11) * MF_TRS + 4 * s + g];   // M(c, 4s + g)
            const dvec2 *qp = (const dvec2 *)(Sb + q_src), *rp = (const dvec2 *)(Sb + rhs_src);
            const dvec2 q0 = qp[0], q1 = qp[1], r0 = rp[0], r1 = rp[1];
            qc[0] = q0.x; qc[1] = q0.y; qc[2] = q1.x; qc[3] = q1.y;
            x0 = r0.x; x1 = r0.y; x2 = r1.x; x3 = r1.y;
        }
        PT_FINE(4);
        // L y = b, then L^T x = y: x = -K(:, c) | -K(:, r0) | -k (chol4_solve's operation order), y for P' = C - Y^T Y
        x0 = x0 * iL[0];
        x1 = (x1 - L[1] * x0) * iL[1];
        x2 = (x2 - L[3] * x0 - L[4] * x1) * iL[2];
        x3 = (x3 - L[6] * x0 - L[7] * x1 - L[8] * x2) * iL[3];
        const double y0 = x0, y1 = x1, y2 = x2, y3 = x3;
        x3 = x3 * iL[3];
        x2 = (x2 - L[8] * x3) * iL[2];
        x1 = (x1 - L[4] * x2 - L[7] * x3) * iL[1];
        x0 = (x0 - L[1] * x1 - L[3] * x2 - L[6] * x3) * iL[0];
        PT_FINE(5);
        // [F] P' = Qxx + Qux^T K on the matrix core, B operand K(g, c) from the lane's own solve (lanes 16 and 17
        // solved K(:, r0) and k: their K(1, c) comes from lanes 0 and 1 through a row swap)
        {
            const double ys = swap16_d(y1);
            double yg = y0;   // y_g as a chain of selects (sel4's nested conditionals compile to branches here)
            yg = (g == 1) ? y1 : yg;
            yg = (g == 2) ? y2 : yg;
            yg = (g == 3) ? y3 : yg;
            yg = solve_col ? yg : ys;
            d4v CF;
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                asm volatile("" : "+v"(tv[s]));   // used by every lane: sunk under the select, the read was a branch + wait
                CF[s] = (Mm[s] + tv[s]) * hx;
            }
            CF[3] = cf3;
            Pm = mfma64(-yg, yg, CF);   // A(c, g) = -Y(g, c), B(g, c) = Y(g, c): P' = C - Y^T Y
        }
        PT_FINE(6);
        // factor record -> kbuf (x~ order): K^T row c + 1 (groups 1..3 duplicate group 0), row 0 = K(:, r0), k; L
        {
            dvec2 *kb = (dvec2 *)(Sb + kb_dst);
            kb[0] = dv2(-x0, -x1);
            kb[1] = dv2(-x2, -x3);
            if (lane == 0) {
                dvec2 *lp = (dvec2 *)&S.kbuf[RC_L];
#pragma unroll
                for (int e = 0; e < 5; ++e) lp[e] = dv2(L[2 * e], L[2 * e + 1]);
            }
        }
        PT_END(S, 14);
        sync();
        {
            constexpr int NP = REC / 2;
            static_assert(NP <= WAVE && RC_L + 10 == REC, "record: one 16-byte store per lane");
            const dvec2 v = ((const dvec2 *)S.kbuf)[min(lane, NP - 1)];   // ahead of the row's writes and gathers
            // the next stage's row to LDS and its gathers: before this stage's first store (the record's)
            PT_WAIT(S, 0, 0);   // timer build: the row loads' wait (issued at the stage's start), probe 0
            put_row(t0, t1, t2);
            sync();
            gather(cur);   // the next stage's operands into the buffer this stage has finished reading
            if (!ok) return 0;
            if (lane < NP) ((gdvec2 *)(Rec + (size_t)k * REC))[lane] = v;
        }
        PT_FINE(7);
        if (k == 0) return 2;
        // the r0 border p12' and the gradient p' (column layout); lane 16 (Qux column M(u, r0), bases m22 / gr0) forms
        // the r0 corner p22' and p_r0'
        double kr[4], kf[4];
        {
            const dvec2 *k0p = (const dvec2 *)&S.kbuf[0], *kfp = (const dvec2 *)&S.kbuf[RC_KF];
            const dvec2 a0 = k0p[0], a1 = k0p[1], b0 = kfp[0], b1 = kfp[1];
            kr[0] = a0.x; kr[1] = a0.y; kr[2] = a1.x; kr[3] = a1.y;
            kf[0] = b0.x; kf[1] = b0.y; kf[2] = b1.x; kf[3] = b1.y;
        }
        double p12n = p12b, pn = pnb;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            p12n = fma(qc[a], kr[a], p12n);
            pn = fma(qc[a], kf[a], pn);
        }
        // P_k packed (x~ order) and p_k for the refinement prepass / costates
        {
            const int pso = uni((k - 1) * PSTR * 8);
#pragma unroll
            for (int s = 0; s < 4; ++s) bst(Pm[s], rs, op[s], pso);
            const unsigned ob = lane < 16 ? (unsigned)(WS_PST + mf_x(c)) * 8u : (lane == 16 ? (unsigned)WS_PST * 8u : MF_OOB);
            bst(p12n, rs, ob, pso);
            const unsigned ov = lane < 16 ? (unsigned)(WS_PVK + mf_x(c)) * 8u : (lane == 16 ? (unsigned)WS_PVK * 8u : MF_OOB);
            bst(pn, rs, ov, uni(k * 18 * 8));
        }
        // column -> row-group layout of p12', p' for the next stage
        *(double *)(Sb + tv_dst) = p12n;
        *(double *)(Sb + tv_dst + 128) = pn;
        sync();
        {
            const dvec2 *t0p = (const dvec2 *)&L0[MF_TV + g * 4], *t1p = (const dvec2 *)&L0[MF_TV + 16 + g * 4];
            const dvec2 a0 = t0p[0], a1 = t0p[1], b0 = t1p[0], b1 = t1p[1];
            p12r[0] = a0.x; p12r[1] = a0.y; p12r[2] = a1.x; p12r[3] = a1.y;
            pr[0] = b0.x; pr[1] = b0.y; pr[2] = b1.x; pr[3] = b1.y;
        }
        p22 = readlane_d(p12n, 16);   // the wave-uniform r0 entries from lane 16
        p16 = readlane_d(pn, 16);
        PT_END(S, 15);
        return 1;
    };
    // stage 0 peeled (its own delta_w pattern, no border update)
    int r = 1;
    int k = N - 1;
    for (; k >= 1 && r == 1; --k) r = stage(k, e12);
    if (r == 1 && k == 0) r = stage(0, e2);
    vm_sync();
    return r == 2;
}
