"""Independent reference of what the interior-point method computes around its Newton step: the error measure, the
merit function and its directional derivative, the fraction-to-the-boundary steps and the accepted iterate.

Restated from IPOPT's definitions (Waechter & Biegler 2006: eq. 5, 6 the optimality error and its scaling, eq. 8 the
fraction to the boundary, eq. 15b the primal-dual step of the bound duals, eq. 16 the kappa_sigma safeguard, section
2.3 the merit pair theta = ||c||_1 and phi = f - mu sum log(slack)); no code is shared with the oracle or the HIP
kernels.  Like tests/newton.py it stands on tests/kkt.py (the NLP in torch fp64, differentiated by autograd), but
takes gradients and vector-Jacobian products only, never the dense Hessian.

Inputs of `Reference`: one instance's dumped record of an iteration (newton.split_record: the point x, u, lam, zLu,
zUu, zLw, zUw and the refined step dx, du, lam+), the mu of that iteration (word 0 of its trace row), the problem data
and its kkt.Problem.  The bounds are newton.relaxed_bounds, s_obj is IPOPT's gradient-based scaling at the initial
point as newton.NewtonSystem forms it.

Model-based quantities (torch fp64 autograd): theta, pinf, J, the barrier log sum, phi, grad phi . d with the sum of
its absolute terms, dinf, c0, s_d, s_c, E0.  From the dumped arrays alone (np.longdouble): tau, alpha_max, the dual
steps dz with their cancellation scale |mu/s| + |z| + |z d/s|, alpha_z, and the accepted point for a given
(alpha, alpha_z) with the duals the kappa_sigma clamp moved.

The second half of the module is the bookkeeping both test files share (test_globalisation_host.py on the oracle's
two builds, test_gpu_globalisation.py on the HIP engine): the cases, their classification from the oracle's traces,
the coverage they must have, and the error of a backend's trace words and accepted iterate against the reference.
"""
from __future__ import annotations

import numpy as np
import torch

import generic_params as GP
import kkt
import newton
import newton_cases as NC

NX, NU = newton.NX, newton.NU
LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
TAU_MIN = 0.99              # IPOPT tau_min
KAPPA_SIGMA = 1e10          # IPOPT kappa_sigma
S_MAX = 100.0               # IPOPT s_max
BLOCKS = (("zLu", "zUu", "u"), ("zLw", "zUw", "w"))

_s_obj = {}


def objective_scale(ini, goal, ptra, qtra, t, ulast, N, prm=kkt.DEFAULT):
    """IPOPT's gradient-based objective scaling at the initial point (newton.NewtonSystem's s_obj, gradient only)."""
    f64 = torch.float64
    cst = [torch.tensor(np.asarray(a, dtype=np.float64), dtype=f64) for a in (ini, goal, ptra, qtra)]
    ul = torch.tensor(np.asarray(ulast, np.float64), dtype=f64)
    p0 = newton.initial_point(np.asarray(ini, dtype=np.float64), N, prm)
    X = torch.tensor(p0["x"], dtype=f64, requires_grad=True)
    U = torch.tensor(p0["u"], dtype=f64, requires_grad=True)
    J, _ = kkt.objective_and_defects(X, U, cst[0], cst[1], cst[2], cst[3], torch.tensor(float(t), dtype=f64), ul, prm)
    gX, gU = torch.autograd.grad(J, [X, U])
    gmax = max(float(gX[1:].abs().max()), float(gU.abs().max()))
    return max(100.0 / gmax, 1e-8) if gmax > 100.0 else 1.0


class Reference:
    """The quantities of one iteration at a dumped point.  `step` may be None where only the merit is wanted (the
    point of iteration k + 1 under the mu of k + 1)."""

    def __init__(self, point, step, mu, ini, goal, ptra, qtra, t, ulast, N, prm=kkt.DEFAULT, s_obj=None):
        self.N, self.mu, self.prm = N, float(mu), prm
        self.point = {k: np.asarray(v, dtype=np.float64) for k, v in point.items()}
        self.step = None if step is None else {k: np.asarray(v, dtype=np.float64) for k, v in step.items()}
        assert self.point["x"].shape == (N + 1, NX) and self.point["u"].shape == (N, NU)
        ulast = np.zeros(NU) if ulast is None else ulast
        self.s_obj = objective_scale(ini, goal, ptra, qtra, t, ulast, N, prm) if s_obj is None else s_obj
        self._data = (ini, goal, ptra, qtra, t, ulast)
        self.u_lo, self.u_hi, self.w_lo, self.w_hi = newton.relaxed_bounds(prm)
        self._model = None

    # ---- torch fp64 autograd: objective, defects, gradient, J_c^T lam -------------------------------------------
    def model(self):
        if self._model is None:
            f64 = torch.float64
            ini, goal, ptra, qtra, t, ulast = self._data
            cst = [torch.tensor(np.asarray(a, dtype=np.float64), dtype=f64) for a in (ini, goal, ptra, qtra, ulast)]
            X = torch.tensor(self.point["x"], dtype=f64, requires_grad=True)
            U = torch.tensor(self.point["u"], dtype=f64, requires_grad=True)
            J, c = kkt.objective_and_defects(X, U, cst[0], cst[1], cst[2], cst[3], torch.tensor(float(t), dtype=f64),
                                             cst[4], self.prm)
            gJx, gJu = torch.autograd.grad(J, [X, U], retain_graph=True)
            lam = torch.tensor(self.point["lam"], dtype=f64)
            ax, au = torch.autograd.grad((lam * c).sum(), [X, U])          # J_c^T lam
            self._model = {"J": float(J.detach()), "c": c.detach().numpy(), "gJx": gJx.numpy()[1:], "gJu": gJu.numpy(),
                           "ax": ax.numpy()[1:], "au": au.numpy()}
        return self._model

    def slacks(self, x=None, u=None):
        """{block: (lower slack, upper slack)} of u (N, 4) and of the omega of x_1..x_N (N, 3), long double."""
        x = self.point["x"] if x is None else x
        u = self.point["u"] if u is None else u
        uu, ww = np.asarray(u, dtype=LD), np.asarray(x, dtype=LD)[1:, 10:13]
        return {"u": (uu - LD(self.u_lo), LD(self.u_hi) - uu), "w": (ww - LD(self.w_lo), LD(self.w_hi) - ww)}

    def duals(self):
        P = self.point
        return {"u": (P["zLu"].astype(LD), P["zUu"].astype(LD)),
                "w": (P["zLw"][1:].astype(LD), P["zUw"][1:].astype(LD))}

    def bounded_step(self):
        return {"u": self.step["du"].astype(LD), "w": self.step["dx"][1:, 10:13].astype(LD)}

    def merit(self):
        """theta, pinf, J, log sum, phi."""
        m = self.model()
        s = self.slacks()
        logsum = float(sum(np.sum(np.log(sl)) + np.sum(np.log(su)) for sl, su in s.values()))
        return {"theta": float(np.sum(np.abs(m["c"]))), "pinf": float(np.max(np.abs(m["c"]))), "J": m["J"],
                "logsum": logsum, "phi": self.s_obj * m["J"] - self.mu * logsum}

    def theta_floor(self):
        """What three roundings per defect entry (the product dt f, the sum with x_k, the difference with x_{k+1}),
        each of one eps of its largest term (|x_k| + |x_{k+1}| + |c| bounds all three), can move theta by, relative
        to 1 + theta: the floor of theta's bound where both oracle builds reproduce the reference exactly."""
        c, x = self.model()["c"], self.point["x"]
        return 3 * EPS * float(np.sum(np.abs(x[:-1]) + np.abs(x[1:]) + np.abs(c))) / (1.0 + float(np.sum(np.abs(c))))

    def barrier_gradient(self):
        """(g_x (N, 13) over x_1..x_N, g_u (N, 4)): s_obj grad J - mu / (v - lo) + mu / (hi - v)."""
        m, s = self.model(), self.slacks()
        gx, gu = self.s_obj * m["gJx"], self.s_obj * m["gJu"]
        gu = gu + np.asarray(-self.mu / s["u"][0] + self.mu / s["u"][1], dtype=np.float64)
        gx = gx.copy()
        gx[:, 10:13] += np.asarray(-self.mu / s["w"][0] + self.mu / s["w"][1], dtype=np.float64)
        return gx, gu

    def dphi(self):
        """(grad phi . d, sum |g_i d_i|): the sum cancels, the second figure is its scale."""
        gx, gu = self.barrier_gradient()
        t = np.concatenate([(gx * self.step["dx"][1:]).ravel(), (gu * self.step["du"]).ravel()]).astype(LD)
        return float(np.sum(t)), float(np.sum(np.abs(t)))

    def errors(self):
        """dinf, pinf, c0, s_d, s_c and E0 = max(dinf / s_d, pinf, c0 / s_c)."""
        m, s, z, P, N = self.model(), self.slacks(), self.duals(), self.point, self.N
        rx = self.s_obj * m["gJx"] + m["ax"]
        ru = self.s_obj * m["gJu"] + m["au"] - P["zLu"] + P["zUu"]
        rx[:, 10:13] += -P["zLw"][1:] + P["zUw"][1:]
        dinf = float(max(np.max(np.abs(rx)), np.max(np.abs(ru))))
        pinf = float(np.max(np.abs(m["c"])))
        c0 = float(max(max(np.max(s[b][0] * z[b][0]), np.max(s[b][1] * z[b][1])) for b in ("u", "w")))
        sum_z = float(sum(np.sum(z[b][0]) + np.sum(z[b][1]) for b in ("u", "w")))
        sum_mult = float(np.sum(np.abs(P["lam"])))
        n_z = 14 * N
        n_mult = 13 * N + n_z
        s_d = max(S_MAX, (sum_mult + sum_z) / n_mult) / S_MAX
        s_c = max(S_MAX, sum_z / n_z) / S_MAX
        return {"dinf": dinf, "pinf": pinf, "c0": c0, "s_d": s_d, "s_c": s_c,
                "E0": max(dinf / s_d, pinf, c0 / s_c)}

    # ---- long double, from the dumped arrays alone ---------------------------------------------------------------
    def tau(self):
        return max(LD(TAU_MIN), LD(1.0) - LD(self.mu))

    def alpha_max(self):
        """Largest alpha <= 1 with v + alpha d inside the fraction tau of its slacks (u and omega of x_1..x_N)."""
        tau, s, d = self.tau(), self.slacks(), self.bounded_step()
        a = LD(1.0)
        for b in ("u", "w"):
            lo, hi = d[b] < 0, d[b] > 0
            for cand in (-tau * s[b][0][lo] / d[b][lo], tau * s[b][1][hi] / d[b][hi]):
                if cand.size:
                    a = min(a, cand.min())
        return a

    def dual_steps(self):
        """{block: (dzL, dzU, scale L, scale U)}: dz = mu / s - z -/+ (z / s) d and |mu / s| + |z| + |z d / s|."""
        mu, s, z, d = LD(self.mu), self.slacks(), self.duals(), self.bounded_step()
        out = {}
        for b in ("u", "w"):
            (sl, su), (zl, zu) = s[b], z[b]
            out[b] = (mu / sl - zl - zl / sl * d[b], mu / su - zu + zu / su * d[b],
                      np.abs(mu / sl) + np.abs(zl) + np.abs(zl * d[b] / sl),
                      np.abs(mu / su) + np.abs(zu) + np.abs(zu * d[b] / su))
        return out

    def alpha_z(self):
        """(alpha_z, amplification): the largest alpha_z <= 1 keeping z + alpha_z dz >= (1 - tau) z, and the factor
        scale / |dz| of the binding dual (1 when none binds): a relative error e of the scale in dz is a relative
        error e * amplification in alpha_z."""
        tau, z, dz = self.tau(), self.duals(), self.dual_steps()
        best, amp = LD(1.0), 1.0
        for b in ("u", "w"):
            for zz, dd, sc in ((z[b][0], dz[b][0], dz[b][2]), (z[b][1], dz[b][1], dz[b][3])):
                neg = dd < 0
                if np.any(neg):
                    cand = -tau * zz[neg] / dd[neg]
                    i = int(np.argmin(cand))
                    if cand[i] < best:
                        best, amp = cand[i], float(sc[neg][i] / np.abs(dd[neg][i]))
        return best, amp

    def accepted_point(self, alpha, alpha_z, slack_at=None):
        """The iterate after the step: x + alpha dx, u + alpha du, lam + alpha (lam+ - lam), z + alpha_z dz clamped to
        [mu / (1e10 s'), 1e10 mu / s'] with s' the slack of the new point (of `slack_at` = {"x", "u"} when given: the
        stored new point, so that the clamp's bounds do not carry the rounding of x + alpha dx into a small slack).
        Returns (point in long double, {field: bool array of the duals the clamp moved}, {field: scale of dz})."""
        a, az, mu, P, S = LD(alpha), LD(alpha_z), LD(self.mu), self.point, self.step
        new = {"x": P["x"].astype(LD) + a * S["dx"].astype(LD), "u": P["u"].astype(LD) + a * S["du"].astype(LD),
               "lam": P["lam"].astype(LD) + a * (S["lamp"].astype(LD) - P["lam"].astype(LD))}
        at = new if slack_at is None else slack_at
        s1, z, dz = self.slacks(at["x"], at["u"]), self.duals(), self.dual_steps()
        moved, scale = {}, {}
        for fl, fu, b in BLOCKS:
            for f, zz, dd, sc, sn in ((fl, z[b][0], dz[b][0], dz[b][2], s1[b][0]),
                                      (fu, z[b][1], dz[b][1], dz[b][3], s1[b][1])):
                zn = zz + az * dd
                lo, hi = mu / (LD(KAPPA_SIGMA) * sn), LD(KAPPA_SIGMA) * mu / sn
                cl = np.maximum(np.minimum(zn, hi), lo)
                mv = cl != zn
                if b == "w":   # stage 0 is fixed: its duals stay 0
                    cl, mv, sc = (np.concatenate([np.zeros((1, 3), dtype=t.dtype), t]) for t in (cl, mv, sc))
                new[f], moved[f], scale[f] = cl, mv.astype(bool), sc
        return new, moved, scale


# ======== the cases and the bookkeeping of the two test files =====================================================
# trace words (include/lafse3.h)
MU, E0, THETA, PHI, GBD, AMAX, AZ, ALPHA, DELTA_W, ACCEPTED = range(10)
J, LOGSUM = 14, 15
WORDS_K = ("E0", "theta", "phi", "gBD", "amax", "az", "J", "logsum")            # words 1..6, 14, 15 of iteration k
WORDS_K1 = ("theta+", "phi+", "J+", "logsum+")                                   # words 2, 3, 14, 15 of iteration k + 1
HORIZONS = (1, 2, 3, 50)
BATCH = 64


def reference(prob, s, N, point, step, mu):
    prm = NC._prm(prob.get("prm"))
    key = (id(prm), N, tuple(prob["ini"][s]), tuple(prob["p"][s]), float(prob["t"][s]), tuple(prob["ulast"][s]))
    if key not in _s_obj:
        _s_obj[key] = objective_scale(prob["ini"][s], prob["goal"][s], prob["p"][s], prob["q"][s], prob["t"][s],
                                      prob["ulast"][s], N, prm)
    return Reference(point, step, mu, prob["ini"][s], prob["goal"][s], prob["p"][s], prob["q"][s], prob["t"][s],
                     prob["ulast"][s], N, prm, _s_obj[key])


def rel(a, ref):
    return abs(float(a) - float(ref)) / (1.0 + abs(float(ref)))


def ulps(got, want, *operands):
    """Largest |got - want| in units of the spacing of doubles at the largest magnitude among `want` and the
    operands it was summed from (a rounding is relative to the term rounded, not to a sum that cancels)."""
    mag = np.abs(np.asarray(want, dtype=np.float64))
    for o in operands:
        mag = np.maximum(mag, np.abs(np.asarray(o, dtype=np.float64)))
    d = np.abs(np.asarray(got, dtype=LD) - np.asarray(want, dtype=LD))
    return float(np.max(d / np.spacing(np.maximum(mag, np.finfo(np.float64).tiny)).astype(LD))) if d.size else 0.0


def oracle_traces(prob, N, fast=False, **opts):
    """(solve, trace (B, longest solve + 1, 16)) of every sample of prob on the oracle, solver options `opts`."""
    from oracle import oracle as O
    params = NC.oracle_params(prob.get("prm"), horizon=N, **opts)
    args = GP.solve_args(prob)
    r = O.solve(*args, ulast=prob["ulast"], params=params, fast=fast)
    TI = int(r["iters"].max()) + 1
    buf = np.zeros((len(r["iters"]), TI, 16))
    O.debug_trace(buf, TI, fast=fast)
    try:
        O.solve(*args, ulast=prob["ulast"], params=params, fast=fast)
    finally:
        O.debug_trace(None, 0, fast=fast)
    return r, buf


# ---- the cases ---------------------------------------------------------------------------------------------------
# Every group (parameter set, horizon) takes samples 0..3 of scenario.synthetic_batch(64, seed=2025) at the iterations
# KS; the full horizon adds the (sample, iteration) pairs of EXTRA, found on the oracle's traces of all 64 samples (the
# short horizons take no step halving, no second-order correction and no delta_w > 0 on any sample under either set).
SAMPLES = (0, 1, 2, 3)
KS = {1: (0, 1, 3), 2: (0, 1, 3), 3: (0, 1, 3, 7), 50: (0, 1, 3)}
EXTRA = {"default": ((2, 27), (2, 36), (35, 27), (14, 40)),      # mu decrease, late, halving, second-order correction
         "generic": ((26, 0), (2, 37), (2, 46), (11, 45))}       # correction, mu decrease, late, halving and late
LABELS = ("iteration 0", "iteration 1", "mu decrease", "halving", "delta_w > 0", "alpha_z < 1",
          "second-order correction", "late")
MAX_LEFT_OUT = 0.25         # share of a group's cases that may be left out of the accepted-point comparison


def cases_of(pset, N):
    return [(s, k) for s in SAMPLES for k in KS[N]] + (list(EXTRA[pset]) if N == 50 else [])


def groups():
    return [(pset, N) for pset in GP.SETS for N in HORIZONS]


def back_at_stored_point(tr, iters):
    """Iterations j of one solve's trace whose reference point (theta, phi, gBD: words 2..4) is exactly that of an
    iteration i < j - 1: the watchdog gave up its trial steps and resumed the point it had stored."""
    return [j for j in range(2, int(iters)) if any(np.array_equal(tr[j, 2:5], tr[i, 2:5]) for i in range(j - 1))]


def first_change(a, b):
    """First row at which two traces of one sample differ (None: they are equal)."""
    n = max(len(a), len(b))
    a, b = (np.concatenate([t, np.zeros((n - len(t), 16))]) for t in (a, b))
    d = np.nonzero(np.any(a != b, axis=1))[0]
    return int(d[0]) if d.size else None


def classify(N, res, tr, tro, s, k):
    """What the oracle's traces say of iteration k of sample s: (labels, reason why its next iterate is not x + alpha d
    along the dumped direction or None).  tr: the solve's trace, tro: the trace with max_soc = 0.  A second-order
    correction counts its sweep (word 11) whether or not its point is accepted, so the first row at which the two
    traces differ is the first iteration that tries one, and it accepted the corrected step iff alpha or the verdict
    differs there.  Later rows of such a solve say nothing (the two solves have parted): a case must lie at or before
    that row."""
    t, it = tr[s], int(res["iters"][s])
    assert k + 1 < it, (N, s, k, "iteration k + 1 takes no step", it)
    j = first_change(t, tro[s])
    assert j is None or k <= j, (N, s, k, "the traces cannot tell whether this iteration takes a correction", j)
    assert t[k, MU] > 0 and t[k + 1, MU] > 0, (N, s, k, "an iteration of the case lies in a restoration phase")
    back = back_at_stored_point(t, it)
    assert k not in back and k + 1 not in back, (N, s, k, "the trace words are those of the watchdog's stored point")
    soc = j == k and (t[k, ALPHA] != tro[s][k, ALPHA] or t[k, ACCEPTED] != tro[s][k, ACCEPTED])
    labels = set()
    if k < 2:
        labels.add(f"iteration {k}")
    if k > 0 and t[k, MU] < t[k - 1, MU]:
        labels.add("mu decrease")
    if t[k, ACCEPTED] == 1 and not soc and t[k, ALPHA] < t[k, AMAX]:
        h = np.log2(t[k, AMAX] / t[k, ALPHA])
        assert h == np.round(h) and h >= 1, (N, s, k, "alpha is no halving of alpha_max", t[k, AMAX], t[k, ALPHA])
        labels.add("halving")
    if t[k, DELTA_W] > 0:
        labels.add("delta_w > 0")
    if t[k, AZ] < 1:
        labels.add("alpha_z < 1")
    if soc:
        labels.add("second-order correction")
    if N == 50 and res["status"][s] == 0 and k >= it - 3:
        labels.add("late")
    reason = None
    if soc:
        reason = "second-order correction"
    elif t[k, ACCEPTED] != 1:
        reason = "restoration phase next"
    elif t[k, ALPHA] == t[k, AZ] and t[k, ALPHA] < 1 and not t[k, ALPHA] == t[k, AMAX]:
        reason = "soft restoration step"    # alpha_z set to the primal step: all multipliers move by one alpha
    return labels, reason


_groups = {}


def group(batch, pset, N):
    """One group on the oracle alone: the problem (all 64 samples, a case's sample is its index), the cases, their
    labels and the cases left out of the accepted-point comparison with the reason."""
    if (pset, N) not in _groups:
        prob = GP.problem(batch, N, tuple(range(BATCH)), pset)
        res, tr = oracle_traces(prob, N)
        _, tro = oracle_traces(prob, N, max_soc=0)
        cases = cases_of(pset, N)
        labels, left = {}, {}
        for s, k in cases:
            labels[(s, k)], why = classify(N, res, tr, tro, s, k)
            if why is not None:
                left[(s, k)] = why
        _groups[(pset, N)] = {"prob": prob, "cases": cases, "labels": labels, "left": left}
    return _groups[(pset, N)]


def coverage(batch):
    """{label: [(set, N, sample, k)]} over all groups, asserted complete; the share left out of the accepted-point
    comparison is at most MAX_LEFT_OUT in every group and every left-out case stays in the trace-word comparison
    (`measure` compares the words of every case)."""
    found = {lab: [] for lab in LABELS}
    for pset, N in groups():
        g = group(batch, pset, N)
        for c in g["cases"]:
            for lab in g["labels"][c]:
                found[lab].append((pset, N) + c)
        assert len(g["left"]) <= MAX_LEFT_OUT * len(g["cases"]), (pset, N, g["left"])
    for lab in LABELS:
        assert found[lab], ("no case is a", lab)
    assert any(N == 50 for _, N, _, _ in found["late"])
    return found


# ---- a backend's words and accepted iterate against the reference --------------------------------------------------
def measure(prob, N, data, left):
    """Per case the error of every compared figure: {(sample, k): {word: error}} (and under "floor:theta",
    "floor:theta+" Reference.theta_floor of the two points).  `data`: newton_cases.collect_pairs
    of one backend; `left`: the cases whose accepted point is not compared.  Errors are relative to 1 + |reference|,
    except gBD (relative to the sum of |g_i d_i|), alpha_z (divided by the amplification scale / |dz| of its binding
    dual), x, u, lam (ulps), the accepted duals (relative to the scale of dz) and the clamped duals (relative to the
    clamp's bound; absent where the clamp moved none)."""
    out = {}
    for (s, k), c in data.items():
        t = c["trace"]
        R = reference(prob, s, N, c["point"], c["step"], t[k, MU])
        m, e = R.merit(), R.errors()
        g, gs = R.dphi()
        az, amp = R.alpha_z()
        w = {"E0": rel(t[k, E0], e["E0"]), "theta": rel(t[k, THETA], m["theta"]), "phi": rel(t[k, PHI], m["phi"]),
             "gBD": abs(t[k, GBD] - g) / gs, "amax": rel(t[k, AMAX], R.alpha_max()),
             "J": rel(t[k, J], m["J"]), "logsum": rel(t[k, LOGSUM], m["logsum"]), "floor:theta": R.theta_floor()}
        if left.get((s, k)) != "second-order correction":   # there word 6 is the dual step of the corrected direction
            w["az"] = rel(t[k, AZ], az) / amp
        R1 = reference(prob, s, N, c["next_point"], None, t[k + 1, MU])
        m1 = R1.merit()
        w["floor:theta+"] = R1.theta_floor()
        w.update({"theta+": rel(t[k + 1, THETA], m1["theta"]), "phi+": rel(t[k + 1, PHI], m1["phi"]),
                  "J+": rel(t[k + 1, J], m1["J"]), "logsum+": rel(t[k + 1, LOGSUM], m1["logsum"])})
        if (s, k) not in left:
            P, S, Q, a = c["point"], c["step"], c["next_point"], t[k, ALPHA]
            new, moved, scale = R.accepted_point(a, t[k, AZ], slack_at=Q)
            w["x"] = ulps(Q["x"], new["x"], P["x"], a * S["dx"])
            w["u"] = ulps(Q["u"], new["u"], P["u"], a * S["du"])
            w["lam"] = ulps(Q["lam"], new["lam"], P["lam"], S["lamp"])
            zs, cl = [0.0], []
            for f in ("zLu", "zUu", "zLw", "zUw"):
                d = np.abs(Q[f].astype(LD) - new[f])
                free = ~moved[f] & (scale[f] > 0)
                zs.append(float(np.max(d[free] / scale[f][free], initial=0.0)))
                assert np.all(d[~moved[f] & ~(scale[f] > 0)] == 0), (s, k, f, "dual of the fixed stage 0 moved")
                cl += list(np.asarray(d[moved[f]] / np.abs(new[f][moved[f]]), dtype=np.float64))
            w["z"] = max(zs)
            if cl:
                w["clamped"] = max(cl)
        out[(s, k)] = w
    return out


def largest(errs):
    """{word: largest error over the cases that have it}."""
    words = sorted({w for e in errs.values() for w in e})
    return {w: max(e[w] for e in errs.values() if w in e) for w in words}


# ---- the bounds a device is held to ------------------------------------------------------------------------------
# A word's bound is the margin times the oracle's largest error on the group, and never below the word's floor: that
# many eps, the roundings of the shortest way to compute the word.  The floor decides where both oracle builds
# reproduce the reference exactly, and where their largest error on the group is below one spacing of the word at
# another case (default N = 1: E0 = c0 = 0.2287 at iteration 1 of samples 1 and 3, both builds exact there, their
# figure 1.7e-18 is one spacing of a smaller E0 elsewhere; the device is one spacing of 0.2287 off, 2.3e-17, after
# the two roundings of slack * z).
#   E0     on its shortest path c0 / s_c: the slack, slack * z, the quotient: three
#   amax   tau = 1 - mu, the slack, tau * slack, the quotient: four per candidate, and the minimum adds none
#   az     dz = mu / s - z -/+ (z / s) d: slack, two quotients, product, two differences; then tau, tau * z and the
#          quotient: nine (the error is already divided by the amplification of dz's cancellation)
#   z      dz as above (six), alpha_z * dz and the sum: eight, relative to the scale of dz
#   theta  Reference.theta_floor (three per defect entry, summed)
#   others (sums over the stages: J, the log sum, phi, grad phi . d) one: the rounding of the result itself
FLOOR_ROUNDINGS = {"E0": 3, "amax": 4, "az": 9, "z": 8}
ULP_BOUND = 2.0             # x + alpha dx, u + alpha du, lam + alpha (lam+ - lam): one fused or two separate roundings
                            # (three for lam), each at most half a spacing of its largest operand (`ulps`)
CLAMP_ROUNDINGS = 3         # a clamped dual: the slack, 1e10 * mu (or 1e10 * s'), the quotient
COMPARED = WORDS_K + WORDS_K1 + ("z",)      # words bounded by margin times the oracle's figure


def bounds(margin, oracle_figures):
    """{word: bound} of one group from the `largest` errors of the oracle's builds on it: margin times the larger
    figure, at least the floor."""
    out = {}
    for w in COMPARED:
        o = max(f[w] for f in oracle_figures)
        if w in ("theta", "theta+"):
            floor = max(f["floor:" + w] for f in oracle_figures)
        else:
            floor = FLOOR_ROUNDINGS.get(w, 1) * EPS
        out[w] = max(margin * o, floor)
    for w in ("x", "u", "lam"):
        out[w] = ULP_BOUND
    out["clamped"] = CLAMP_ROUNDINGS * EPS
    return out


def table_row(head, figs, words=COMPARED + ("x", "u", "lam", "clamped")):
    return head + " " + " ".join(f"{w} {figs[w]:.2e}" if w in figs else f"{w} -" for w in words)


BUILDS = (("strict", NC.oracle_run), ("FMA", NC.oracle_run_fma))
_figures = {}


def oracle_figures(batch, pset, N):
    """[(build, collected cases, per-case errors, largest error per word)] of one group on the two oracle builds."""
    if (pset, N) not in _figures:
        g = group(batch, pset, N)
        out = []
        for name, run in BUILDS:
            data = NC.collect_pairs(run, g["prob"], N, g["cases"])
            errs = measure(g["prob"], N, data, g["left"])
            out.append((name, data, errs, largest(errs)))
        _figures[(pset, N)] = out
    return _figures[(pset, N)]
