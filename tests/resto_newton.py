"""Dense, independent Newton system of one iteration of the restoration phase (csrc/resto.inc, the oracle's
orc_restoration; IPOPT's RestoIpoptNLP).

Built on tests/kkt.py (the dynamics restated in torch fp64, differentiated by autograd): no code is shared with the
oracle or the HIP kernels.  The restoration problem of a start point v_R = (x_R, u_R) is

    min   rho sum(p + n) + eta / 2 ||D_R (v - v_R)||^2          rho = 1000, D_R = min(1, 1 / |v_R|) elementwise
    s.t.  c_k(v) - p_k + n_k = 0,   c_k = x_k + dt f(x_k, u_k) - x_{k+1}   (kkt.objective_and_defects' defects)
          p, n >= 0,   the u and omega boxes relaxed by 1e-8

in v = (x_1 .. x_N, u_0 .. u_{N-1}) (x_0 is fixed), p, n (13 N each).  Given an iterate as `lafse3_debug_dump_resto`
records it and the record's mu, eta, `RestoSystem` forms the primal-dual Newton system in (dv, dp, dn, lam+)

    [ W + Sigma_v + eta D_R^2 + d I        0             0         Jc^T ] [ dv   ]   [ g_v        ]
    [          0                     z_p / p + d I       0          -I  ] [ dp   ] + [ rho - mu/p ] = 0
    [          0                           0       z_n / n + d I     I  ] [ dn   ]   [ rho - mu/n ]
    [          Jc                         -I             I           0  ] [ lam+ ]   [ c - p + n  ]

    W       = sum_k lam_k grad^2 c_k        Hessian of the constraint part of the Lagrangian (the objective's is
                                            eta D_R^2, written out above)
    Sigma_v = z_L / (v - lo) + z_U / (hi - v)                 on the u and omega entries
    g_v     = eta D_R^2 (v - v_R) - mu / (v - lo) + mu / (hi - v)
    d       = delta_w, on the whole primal diagonal (v, p and n), as the solver places it

Sign convention of the multipliers: L = f_R + lam^T (c - p + n) with c as above, the convention of kkt.py and
newton.py (CasADi's lam_g); lam and lam+ are the restoration problem's own multipliers: its objective is not scaled,
so no s_obj enters.  Stationarity in p and n then reads rho - lam - z_p = 0 and rho + lam - z_n = 0.

The least-squares multiplier estimate at the start point (v = v_R, where the proximity term has no gradient) solves
the same system with the identity in the three primal diagonal blocks, no W, and the right-hand side
[-z_L + z_U ; rho - z_p ; rho - z_n ; 0]  (`lsq_multipliers`).
"""
from __future__ import annotations

import numpy as np
import torch

import kkt
import newton

NX, NU, MAXN = newton.NX, newton.NU, newton.MAXN
RHO = 1000.0
# record of lafse3_debug_dump_resto / orc_debug_dump_resto: name, extra rows, columns; arrays padded to MAXN stages
STEP_FIELDS = newton.STEP_FIELDS + (("dp", 0, NX), ("dn", 0, NX))
POINT_FIELDS = newton.POINT_FIELDS + (("p", 0, NX), ("n", 0, NX), ("zp", 0, NX), ("zn", 0, NX))
REF_FIELDS = (("xR", 1, NX), ("uR", 0, NU))
SCALARS = ("mu", "eta", "delta_w", "written", "ratio_pre", "ratio_post")
LSQ_FIELDS = (("lsq_lamp", 0, NX),)
LSQ_SCALARS = ("lsq_ok", "iters_before")
_ARRAYS = STEP_FIELDS + POINT_FIELDS + REF_FIELDS
SCAL_OFF = sum((MAXN + extra) * w for _, extra, w in _ARRAYS)
LSQ_OFF = SCAL_OFF + len(SCALARS)
DUMP_W = LSQ_OFF + MAXN * NX + len(LSQ_SCALARS)
assert DUMP_W == 9153


def _cut(rec, o, fields, N, out, pad):
    for name, extra, w in fields:
        a = rec[o:o + (MAXN + extra) * w].reshape(MAXN + extra, w)
        out[name] = a[:N + extra].copy()
        pad.append(a[N + extra:].ravel())
        o += (MAXN + extra) * w
    return o


def split_record(rec, N):
    """One instance's record -> (step, point, ref, scalars, lsq, padding): dicts of (stages, width) arrays cut to the
    horizon, the scalars by name, the least-squares part (lsq_lamp, lsq_ok, iters_before), and the concatenated
    entries of the stages beyond the horizon (which the solver must not touch)."""
    rec = np.asarray(rec, dtype=np.float64)
    assert rec.shape == (DUMP_W,)
    out, pad = {}, []
    o = _cut(rec, 0, _ARRAYS, N, out, pad)
    assert o == SCAL_OFF
    scal = dict(zip(SCALARS, rec[SCAL_OFF:LSQ_OFF]))
    lsq = {}
    o = _cut(rec, LSQ_OFF, LSQ_FIELDS, N, lsq, pad)
    lsq.update(zip(LSQ_SCALARS, rec[o:o + len(LSQ_SCALARS)]))
    return ({k: out[k] for k, _, _ in STEP_FIELDS}, {k: out[k] for k, _, _ in POINT_FIELDS},
            {k: out[k] for k, _, _ in REF_FIELDS}, scal, lsq, np.concatenate(pad))


def d_r2(v_ref):
    """D_R^2 = min(1, 1 / |v_R|)^2 elementwise (1 where v_R = 0)."""
    a = np.abs(np.asarray(v_ref, dtype=np.float64))
    return np.minimum(1.0, 1.0 / np.maximum(a, 1e-300)) ** 2


class RestoSystem:
    def __init__(self, point, ref, mu, eta, ini, N, prm=kkt.DEFAULT):
        f64 = torch.float64
        self.N, self.nv, self.m = N, (NX + NU) * N, NX * N
        self.mu, self.eta = float(mu), float(eta)
        P = self.point = {k: np.asarray(v, dtype=np.float64) for k, v in point.items()}
        R = {k: np.asarray(v, dtype=np.float64) for k, v in ref.items()}
        assert P["x"].shape == (N + 1, NX) and P["u"].shape == (N, NU) and P["p"].shape == (N, NX)
        x0 = torch.tensor(np.asarray(ini, dtype=np.float64), dtype=f64)
        zero3, q1 = torch.zeros(3, dtype=f64), torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=f64)

        def defects(v):     # the objective of the original problem plays no part in the restoration problem
            x = torch.cat([x0[None], v[:NX * N].reshape(N, NX)], 0)
            u = v[NX * N:].reshape(N, NU)
            return kkt.objective_and_defects(x, u, x0, zero3, zero3, q1, torch.tensor(0.0, dtype=f64),
                                             torch.zeros(NU, dtype=f64), prm)[1].reshape(-1)

        v = self._pack(P["x"], P["u"])
        lam = torch.tensor(P["lam"].reshape(-1), dtype=f64)
        self.W = torch.func.hessian(lambda w: (lam * defects(w)).sum())(v).numpy()
        self.Jc = torch.func.jacrev(defects)(v).numpy()
        self.c = defects(v).numpy()
        u_lo, u_hi, w_lo, w_hi = newton.relaxed_bounds(prm)
        self.sigma = np.zeros(self.nv)
        self.gbar = np.zeros(self.nv)
        self.zdiff = np.zeros(self.nv)      # -z_L + z_U
        iw = (np.arange(1, N + 1)[:, None] - 1) * NX + np.arange(10, 13)[None]
        for idx, val, zl, zu, lo, hi in ((iw, P["x"][1:, 10:13], P["zLw"][1:], P["zUw"][1:], w_lo, w_hi),
                                         (NX * N + np.arange(NU * N).reshape(N, NU), P["u"], P["zLu"], P["zUu"],
                                          u_lo, u_hi)):
            self.sigma[idx] = zl / (val - lo) + zu / (hi - val)
            self.gbar[idx] = -self.mu / (val - lo) + self.mu / (hi - val)
            self.zdiff[idx] = -zl + zu
        vr = self._pack(R["xR"], R["uR"]).numpy()
        self.d2 = d_r2(vr)
        self.gprox = self.eta * self.d2 * (v.numpy() - vr)
        p, n = P["p"].reshape(-1), P["n"].reshape(-1)
        self.Sp, self.Sn = P["zp"].reshape(-1) / p, P["zn"].reshape(-1) / n
        self.b = np.concatenate([self.gprox + self.gbar, RHO - self.mu / p, RHO - self.mu / n, self.c - p + n])

    def _pack(self, x, u):
        return torch.tensor(np.concatenate([np.asarray(x)[1:].reshape(-1), np.asarray(u).reshape(-1)]),
                            dtype=torch.float64)

    def _frame(self, Hv, Sp, Sn):
        nv, m = self.nv, self.m
        K = np.zeros((nv + 3 * m, nv + 3 * m))
        K[:nv, :nv] = Hv
        ip, in_, il = nv + np.arange(m), nv + m + np.arange(m), nv + 2 * m + np.arange(m)
        K[ip, ip], K[in_, in_] = Sp, Sn
        K[:nv, nv + 2 * m:] = self.Jc.T
        K[nv + 2 * m:, :nv] = self.Jc
        K[ip, il] = K[il, ip] = -1.0
        K[in_, il] = K[il, in_] = 1.0
        return K

    def K(self, delta=0.0):
        return self._frame(self.W + np.diag(self.sigma + self.eta * self.d2 + delta), self.Sp + delta, self.Sn + delta)

    def pack_step(self, step):
        """(dv, dp, dn, lam+) of a dumped step as one vector in the order of K's columns."""
        return np.concatenate([np.asarray(step["dx"])[1:].reshape(-1), np.asarray(step["du"]).reshape(-1),
                               np.asarray(step["dp"]).reshape(-1), np.asarray(step["dn"]).reshape(-1),
                               np.asarray(step["lamp"]).reshape(-1)])

    def unpack_step(self, sol):
        N, nv, m = self.N, self.nv, self.m
        return {"dx": np.concatenate([np.zeros((1, NX)), sol[:NX * N].reshape(N, NX)]),
                "du": sol[NX * N:nv].reshape(N, NU), "dp": sol[nv:nv + m].reshape(N, NX),
                "dn": sol[nv + m:nv + 2 * m].reshape(N, NX), "lamp": sol[nv + 2 * m:].reshape(N, NX)}

    def residual(self, step, delta=0.0):
        ld = np.longdouble
        return self.K(delta).astype(ld) @ self.pack_step(step).astype(ld) + self.b.astype(ld)

    def residual_ratio(self, step, delta=0.0):
        """IPOPT's residual ratio |r|_inf / (min(|step|_inf, 1e6 |b|_inf) + |b|_inf), r = K(delta) step + b
        accumulated in long double."""
        r = float(np.max(np.abs(self.residual(step, delta))))
        nsol = float(np.max(np.abs(self.pack_step(step))))
        nrhs = float(np.max(np.abs(self.b)))
        return r / (min(nsol, 1e6 * nrhs) + nrhs)

    def neg_eigs(self, delta=0.0):
        """(number of negative eigenvalues of K(delta), smallest |eig| / largest |eig|); the right inertia is m
        negative ones.  Computed on K with p and n eliminated, [[Hv, Jc^T], [Jc, -D]], D = 1 / Sp' + 1 / Sn': the
        eliminated blocks are positive diagonals (z, p, n > 0), so by Sylvester's law K has as many negative
        eigenvalues as the Schur complement."""
        nv, m = self.nv, self.m
        assert np.all(self.Sp + delta > 0) and np.all(self.Sn + delta > 0)
        S = np.zeros((nv + m, nv + m))
        S[:nv, :nv] = self.W + np.diag(self.sigma + self.eta * self.d2 + delta)
        S[:nv, nv:] = self.Jc.T
        S[nv:, :nv] = self.Jc
        S[nv + np.arange(m), nv + np.arange(m)] = -(1.0 / (self.Sp + delta) + 1.0 / (self.Sn + delta))
        e = np.linalg.eigvalsh(S)
        a = np.abs(e)
        return int(np.sum(e < 0)), float(a.min() / a.max())

    def lsq_multipliers(self):
        """The restoration problem's least-squares multiplier estimate at this point, before the cut at 1e3:
        [[I, 0, 0, Jc^T], [0, I, 0, -I], [0, 0, I, I], [Jc, -I, I, 0]] [. ; . ; . ; lam] =
        -[gprox - z_L + z_U ; rho - z_p ; rho - z_n ; 0]."""
        P, m = self.point, self.m
        A = self._frame(np.eye(self.nv), np.ones(m), np.ones(m))
        rhs = -np.concatenate([self.gprox + self.zdiff, RHO - P["zp"].reshape(-1), RHO - P["zn"].reshape(-1),
                               np.zeros(m)])
        return np.linalg.solve(A, rhs)[self.nv + 2 * m:].reshape(self.N, NX)
