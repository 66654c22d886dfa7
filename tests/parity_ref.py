"""References that the parity tests at the default parameters (test_gpu_parity.py) and at the generic set
(test_gpu_generic.py) share: the reference's PMP costate recursion on the oracle's derivatives, and the north_star
bound on sol_gradient rows against the oracle."""
import numpy as np


def pmp_reference(x, u, goal, p, q, params=None):
    """quad_OC.py:188-201 restated on the oracle's model / cost derivatives: lam_{N-1} = dh/dx(x_N),
    lam_{k-1} = dc/dx(x_k) + A_k^T lam_k, c = h = the goal cost (quad_model.py:185-196, wk = 0).  params: the
    oracle's parameter block (None: the defaults)."""
    from oracle import oracle as O
    N = u.shape[0]
    _, A, _, _, _ = O.model_eval(x[:N], u, np.zeros((N, 13)), params=params)
    _, _, g, _ = O.cost_eval(x, np.repeat(goal[None], N + 1, 0), np.repeat(p[None], N + 1, 0),
                             np.repeat(q[None], N + 1, 0), 0.0, params=params)
    lam = np.zeros((N, 13))
    lam[N - 1] = g[N]
    for k in range(N - 1, 0, -1):
        lam[k - 1] = g[k] + A[k].T @ lam[k]
    return lam


def grad_parity(o8, s9, it9, args, label, params=None):
    """sol_gradient rows against the oracle (9 solves each) with the north_star bound: >= 95 % of the samples
    whose 18 solves converged agree within 1e-5 relative, and all of them within 1e-4.  Every sample at or
    above 1e-5 is listed with its per-solve iteration-count difference (GPU - oracle): a nonzero difference
    means the two IPMs took another accept/reject decision at IPOPT's 1e-8 tolerance on that solve.  params: the
    oracle's parameter block (None: the defaults)."""
    from oracle import oracle as O
    rit = np.zeros(it9.shape, np.int32)
    r8, rR, rS = O.sol_gradient(*args, iters=rit, params=params)
    ok = (s9 <= 1).all(1) & (rS <= 1).all(1)
    per = (np.abs(o8[:, :7] - r8[:, :7]) / (1.0 + np.abs(r8[:, :7]))).max(1)
    same = (it9 == rit).all(1)
    outl = [(int(i), float(per[i]), (it9[i] - rit[i]).tolist()) for i in np.nonzero(ok & (per >= 1e-5))[0]]
    stats = dict(n=len(per), converged=int(ok.sum()), same_path=int(same.sum()),
                 within_1e5=float(np.mean(per[ok] < 1e-5)), max=float(per[ok].max()),
                 max_same_path=float(per[ok & same].max()) if (ok & same).any() else None)
    print(f"{label}: {stats}; outliers (sample, rel diff, iteration difference per solve): {outl}")
    assert ok.mean() >= 0.9, stats
    # north_star: every converged sample within 1e-5 relative
    assert stats["max"] < 1e-5, (stats, outl)
    return stats, outl
