// weight_columns.hpp — dF/dw of the KKT system for the ten cost weights, as closed forms on one lane's registers
// (host + device: sens.inc uses them on the GPU, tests/native/weight_columns_host.cpp on the CPU).
//
// Column order = lafse3_params order (LAFSE3_NW):
//   0 wrt  1 wqt  2 wthrust  3 wrf  4 wvf  5 wqf  6 wwf  7 tra_w_peak  8 tra_w_decay  9 du_weight
// The objective is  sum_{k=1..N} [wk_k tra(x_k) + path(x_k)] + sum_{k<N} [wthrust |u_k|^2 + du_weight |u_k - u_{k-1}|^2]
// with wk_k = tra_w_peak exp(-tra_w_decay (dt k - t)^2) for k < N and 0 at k = N, u_{-1} = u_last.  It is linear in
// every weight but tra_w_decay, so a column is the cost gradient at unit weight; the dynamics rows are zero.  The
// values here are unscaled: the caller multiplies by the objective scaling.
#pragma once
#include "model.hpp"

namespace lafse3 {

constexpr int NW = 10;
enum { W_WRT = 0, W_WQT, W_WTHRUST, W_WRF, W_WVF, W_WQF, W_WWF, W_PEAK, W_DECAY, W_DU };

// x rows of column q at stage k >= 1.  M: the instance's model (its wrt, wqt weigh the traversal gradient of the peak
// and decay columns); wk: the stage's traversal weight (0 at k = N); dtk = dt k - t; decay: the instance's
// tra_w_decay; last: k == N.  The wthrust and du_weight columns have no x rows.
__host__ __device__ inline void weight_column_x(const Model &M, const Attitude &at, const double *goal,
                                                const double *ptra, double wk, double dtk, double decay, bool last,
                                                int q, const double *xk, double *vx)
{
#pragma unroll
    for (int i = 0; i < NX; ++i) vx[i] = 0.0;
    if (q == W_WTHRUST || q == W_DU) return;
    if (q == W_PEAK || q == W_DECAY) {
        if (last) return;
        // grad tra = state_cost_grad at stage weight 1 minus at 0 (affine in it); d wk / d peak is the exponential
        // itself (not wk / peak: peak may be 0), d wk / d decay = -(dt k - t)^2 wk
        double g1[NX], g0[NX];
        state_cost_grad(M, at, goal, ptra, 1.0, xk, g1);
        state_cost_grad(M, at, goal, ptra, 0.0, xk, g0);
        const double f = (q == W_PEAK) ? exp(-decay * dtk * dtk) : -(dtk * dtk) * wk;
#pragma unroll
        for (int i = 0; i < NX; ++i) vx[i] = f * (g1[i] - g0[i]);
        return;
    }
    // the six weights the stage cost is linear in: its gradient at a model whose weights are zero but this one
    Model U = M;
    U.wrt = (q == W_WRT) ? 1.0 : 0.0;
    U.wqt = (q == W_WQT) ? 1.0 : 0.0;
    U.wrf = (q == W_WRF) ? 1.0 : 0.0;
    U.wvf = (q == W_WVF) ? 1.0 : 0.0;
    U.wqf = (q == W_WQF) ? 1.0 : 0.0;
    U.wwf = (q == W_WWF) ? 1.0 : 0.0;
    state_cost_grad(U, at, goal, ptra, wk, xk, vx);
}

// u rows of column q at stage k < N (grad_u's branches at unit weight): um = u_{k-1} (u_last at k = 0), up = u_{k+1}
// (ignored when `final`, k == N - 1).  The other eight columns have no u rows.
__host__ __device__ inline void weight_column_u(int q, const double *um, const double *uk, const double *up,
                                                bool final, double *vu)
{
#pragma unroll
    for (int a = 0; a < NU; ++a) {
        double v = 0.0;
        if (q == W_WTHRUST) v = 2 * uk[a];
        if (q == W_DU) {
            v = 2 * (uk[a] - um[a]);
            if (!final) v += -2 * (up[a] - uk[a]);
        }
        vu[a] = v;
    }
}

}  // namespace lafse3
