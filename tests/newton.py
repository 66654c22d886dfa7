"""Dense, independent Newton (primal-dual KKT) system of one interior-point iteration of the quad_OC NLP.

Built on tests/kkt.py (the NLP restated in torch fp64, differentiated by autograd): no code is shared with the
oracle or the HIP kernels.  Given an iterate as `lafse3_debug_dump` records it, the barrier parameter `mu` and the
problem data, `NewtonSystem` forms

    unknowns  v = (x_1 .. x_N, u_0 .. u_{N-1})         x_0 is fixed                     n = 17 N
    rows      c_k = x_k + dt f(x_k, u_k) - x_{k+1}                                       m = 13 N
    W     = s_obj grad^2 J + sum_k lam_k grad^2 c_k     exact Hessian of the Lagrangian
    Jc    = dc / dv
    Sigma = z_L / (v - lo) + z_U / (hi - v)             on the u and omega entries, bounds relaxed by 1e-8
    gphi  = s_obj grad J - mu / (v - lo) + mu / (hi - v)
    K(d)  = [[W + Sigma + d I, Jc^T], [Jc, 0]]          b = [gphi ; c]

and a Newton step (d, lam+) of the solver satisfies K(delta_w) [d ; lam+] + b = 0.

Sign convention of the multipliers: CasADi's lam_g, L = J + lam^T c with c as above, as in kkt.py.  The dumped
`lam` and `lam+` are the solver's internal multipliers, those of the problem whose objective is scaled by s_obj
(L = s_obj J + lam^T c); the entry points return lam / s_obj (oracle/lafse3_oracle.c orc_solve_q writes
`W->lam[i] / W->s_obj`), which is what kkt.kkt_residual takes.

s_obj is IPOPT's gradient-based scaling, 100 / max|grad J| at the initial point when that maximum exceeds 100
(floored at 1e-8), recomputed here by autograd at the initial point: U at the bound midpoint, X_k = 0 (k >= 1),
both pushed 1e-2 inside the relaxed bounds.

`initial_point` and `NewtonSystem` take an optional `prm` (kkt.Problem: model constants, weights, bounds, possibly
asymmetric); the default is the reference's problem.
"""
from __future__ import annotations

import numpy as np
import torch

import kkt

NX, NU, MAXN = 13, 4, 50
BOUND_RELAX = 1e-8
# record of lafse3_debug_dump / orc_debug_dump: name, rows (stages), columns; every array padded to MAXN stages
STEP_FIELDS = (("dx", 1, NX), ("du", 0, NU), ("lamp", 0, NX))
POINT_FIELDS = (("x", 1, NX), ("u", 0, NU), ("lam", 0, NX), ("zLu", 0, NU), ("zUu", 0, NU), ("zLw", 1, 3), ("zUw", 1, 3))
DUMP_W = sum((MAXN + extra) * w for _, extra, w in STEP_FIELDS + POINT_FIELDS)
assert DUMP_W == 3732


def _relax(lo, hi):
    return lo - BOUND_RELAX * max(1.0, abs(lo)), hi + BOUND_RELAX * max(1.0, abs(hi))


U_LO, U_HI = _relax(0.0, kkt.U_UB)
W_LO, W_HI = _relax(-kkt.W_UB, kkt.W_UB)


def relaxed_bounds(prm=kkt.DEFAULT):
    """(u_lo, u_hi, w_lo, w_hi): the boxes of prm, each side relaxed by 1e-8 max(1, |bound|)."""
    return _relax(prm.u_lb, prm.u_ub) + _relax(prm.w_lb, prm.w_ub)


def split_record(rec, N):
    """One instance's dump record -> (step, point, padding): dicts of (stages, width) arrays cut to the horizon,
    and the concatenated entries of the stages beyond it (which the solver must not touch)."""
    rec = np.asarray(rec, dtype=np.float64)
    assert rec.shape == (DUMP_W,)
    out, pad, o = {}, [], 0
    for name, extra, w in STEP_FIELDS + POINT_FIELDS:
        a = rec[o:o + (MAXN + extra) * w].reshape(MAXN + extra, w)
        out[name] = a[:N + extra].copy()
        pad.append(a[N + extra:].ravel())
        o += (MAXN + extra) * w
    step = {k: out[k] for k, _, _ in STEP_FIELDS}
    point = {k: out[k] for k, _, _ in POINT_FIELDS}
    return step, point, np.concatenate(pad)


def _push(v, lo, hi):
    pl = min(1e-2 * max(1.0, abs(lo)), 1e-2 * (hi - lo))
    pu = min(1e-2 * max(1.0, abs(hi)), 1e-2 * (hi - lo))
    return min(max(v, lo + pl), hi - pu)


def initial_point(ini, N, prm=kkt.DEFAULT):
    """The iterate of IPM iteration 0 before the multiplier initialisation: x_0 = ini, x_k = 0, u at the bound
    midpoint (bound push 1e-2), bound duals 1 (0 on the fixed stage 0), lam = 0."""
    x = np.zeros((N + 1, NX))
    x[0] = ini
    u_lo, u_hi, w_lo, w_hi = relaxed_bounds(prm)
    x[1:, 10:13] = _push(0.5 * (prm.w_lb + prm.w_ub), w_lo, w_hi)
    u = np.full((N, NU), _push(0.5 * (prm.u_lb + prm.u_ub), u_lo, u_hi))
    zw = np.ones((N + 1, 3))
    zw[0] = 0.0
    return {"x": x, "u": u, "lam": np.zeros((N, NX)), "zLu": np.ones((N, NU)), "zUu": np.ones((N, NU)),
            "zLw": zw, "zUw": zw.copy()}


class NewtonSystem:
    def __init__(self, point, mu, ini, goal, ptra, qtra, t, ulast, N, prm=kkt.DEFAULT):
        f64 = torch.float64
        self.N, self.n, self.m = N, (NX + NU) * N, NX * N
        self.mu = float(mu)
        self.point = {k: np.asarray(v, dtype=np.float64) for k, v in point.items()}
        assert self.point["x"].shape == (N + 1, NX) and self.point["u"].shape == (N, NU)
        cst = [torch.tensor(np.asarray(a, dtype=np.float64), dtype=f64) for a in (ini, goal, ptra, qtra)]
        tt = torch.tensor(float(t), dtype=f64)
        ul = torch.zeros(NU, dtype=f64) if ulast is None else torch.tensor(np.asarray(ulast, np.float64), dtype=f64)
        x0 = cst[0]

        def J_and_c(v):
            x = torch.cat([x0[None], v[:NX * N].reshape(N, NX)], 0)
            u = v[NX * N:].reshape(N, NU)
            return kkt.objective_and_defects(x, u, cst[0], cst[1], cst[2], cst[3], tt, ul, prm)

        self._J_and_c = J_and_c
        # objective scaling from the gradient at the initial point
        p0 = initial_point(np.asarray(ini, dtype=np.float64), N, prm)
        g0 = torch.func.grad(lambda v: J_and_c(v)[0])(self._pack(p0["x"], p0["u"]))
        gmax = float(g0.abs().max())
        self.s_obj = max(100.0 / gmax, 1e-8) if gmax > 100.0 else 1.0

        v = self._pack(self.point["x"], self.point["u"])
        lam = torch.tensor(self.point["lam"].reshape(-1), dtype=f64)
        s = self.s_obj

        def lagrangian(w):
            J, c = J_and_c(w)
            return s * J + (lam * c.reshape(-1)).sum()

        self.W = torch.func.hessian(lagrangian)(v).numpy()
        self.Jc = torch.func.jacrev(lambda w: J_and_c(w)[1].reshape(-1))(v).numpy()
        self.gJ = torch.func.grad(lambda w: J_and_c(w)[0])(v).numpy()
        self.c = J_and_c(v)[1].reshape(-1).numpy()
        # bounded entries of v: omega of x_1..x_N, every u
        P = self.point
        u_lo, u_hi, w_lo, w_hi = relaxed_bounds(prm)
        self.sigma = np.zeros(self.n)
        self.gbar = np.zeros(self.n)
        self.zdiff = np.zeros(self.n)       # -z_L + z_U
        iw = (np.arange(1, N + 1)[:, None] - 1) * NX + np.arange(10, 13)[None]
        for idx, val, zl, zu, lo, hi in ((iw, P["x"][1:, 10:13], P["zLw"][1:], P["zUw"][1:], w_lo, w_hi),
                                         (NX * N + np.arange(NU * N).reshape(N, NU), P["u"], P["zLu"], P["zUu"],
                                          u_lo, u_hi)):
            self.sigma[idx] = zl / (val - lo) + zu / (hi - val)
            self.gbar[idx] = -self.mu / (val - lo) + self.mu / (hi - val)
            self.zdiff[idx] = -zl + zu
        self.b = np.concatenate([s * self.gJ + self.gbar, self.c])

    def _pack(self, x, u):
        return torch.tensor(np.concatenate([np.asarray(x)[1:].reshape(-1), np.asarray(u).reshape(-1)]),
                            dtype=torch.float64)

    def K(self, delta=0.0):
        n, m = self.n, self.m
        K = np.zeros((n + m, n + m))
        K[:n, :n] = self.W + np.diag(self.sigma + delta)
        K[:n, n:] = self.Jc.T
        K[n:, :n] = self.Jc
        return K

    def pack_step(self, step):
        """(d, lam+) of a dumped step as one vector in the order of K's columns."""
        return np.concatenate([np.asarray(step["dx"])[1:].reshape(-1), np.asarray(step["du"]).reshape(-1),
                               np.asarray(step["lamp"]).reshape(-1)])

    def residual(self, step, delta=0.0):
        ld = np.longdouble
        return self.K(delta).astype(ld) @ self.pack_step(step).astype(ld) + self.b.astype(ld)

    def residual_ratio(self, step, delta=0.0):
        """IPOPT's residual ratio |r|_inf / (min(|step|_inf, 1e6 |b|_inf) + |b|_inf), r = K(delta) [d; lam+] + b
        accumulated in long double."""
        r = float(np.max(np.abs(self.residual(step, delta))))
        nsol = float(np.max(np.abs(self.pack_step(step))))
        nrhs = float(np.max(np.abs(self.b)))
        return r / (min(nsol, 1e6 * nrhs) + nrhs)

    def neg_eigs(self, delta=0.0):
        """(number of negative eigenvalues of K(delta), smallest |eig| / largest |eig|)."""
        e = np.linalg.eigvalsh(self.K(delta))
        a = np.abs(e)
        return int(np.sum(e < 0)), float(a.min() / a.max())

    def lsq_multipliers(self):
        """IPOPT's least-squares multiplier initialisation at this point: [[I, Jc^T], [Jc, 0]] [. ; lam] =
        -[s_obj grad J - z_L + z_U ; 0]; zero when max|lam| > 1e3 (constr_mult_init_max)."""
        n, m = self.n, self.m
        A = np.zeros((n + m, n + m))
        A[:n, :n] = np.eye(n)
        A[:n, n:] = self.Jc.T
        A[n:, :n] = self.Jc
        rhs = -np.concatenate([self.s_obj * self.gJ + self.zdiff, np.zeros(m)])
        lam = np.linalg.solve(A, rhs)[n:].reshape(self.N, NX)
        return lam if np.max(np.abs(lam)) <= 1e3 else np.zeros_like(lam)
