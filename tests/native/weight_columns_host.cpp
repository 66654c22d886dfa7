// Host build of the weight-column closed forms (csrc/weight_columns.hpp) for CPU unit tests.
// Compiled by tests/test_weight_columns_host.py with hipcc (host code only; no GPU needed).
#include "weight_columns.hpp"

using namespace lafse3;

extern "C" {

// For n points: the x rows of the ten weight columns, out n x 10 x 13.  prm: the instance's parameters (its weights
// and tra_w_decay); qtra the traversal quaternion, the goal attitude is the identity; wk the stage weight, dtk = dt k -
// t, last != 0 for a terminal stage (k = N).
int weight_columns_host_x(const lafse3_params *prm, int n, const double *x, const double *goal, const double *ptra,
                          const double *qtra, const double *wk, const double *dtk, const int *last, double *out)
{
    const Model M = make_model(*prm);
    for (int i = 0; i < n; ++i) {
        double Rt[9], Rg[9], St[16], Sg[16];
        dcm(qtra + i * 4, Rt);
        attitude_form(Rt, St);
        const double qg[4] = {1, 0, 0, 0};
        dcm(qg, Rg);
        attitude_form(Rg, Sg);
        Attitude at{};
        for (int e = 0; e < 16; ++e) {
            at.St[e] = St[e];
            at.Sg[e] = Sg[e];
        }
        at.trRt = Rt[0] + Rt[4] + Rt[8];
        at.trRg = Rg[0] + Rg[4] + Rg[8];
        for (int q = 0; q < NW; ++q)
            weight_column_x(M, at, goal + i * 3, ptra + i * 3, wk[i], dtk[i], prm->tra_w_decay, last[i] != 0, q,
                            x + i * NX, out + ((int64_t)i * NW + q) * NX);
    }
    return 0;
}

// The u rows of the ten weight columns over a control trajectory u (N x 4) with u_last (4): out 10 x N x 4.
int weight_columns_host_u(int N, const double *u, const double *ulast, double *out)
{
    const double zero[NU] = {0, 0, 0, 0};
    for (int q = 0; q < NW; ++q)
        for (int k = 0; k < N; ++k)
            weight_column_u(q, k == 0 ? ulast : u + (k - 1) * NU, u + k * NU, k + 1 < N ? u + (k + 1) * NU : zero,
                            k + 1 >= N, out + ((int64_t)q * N + k) * NU);
    return 0;
}
}
