"""The Newton step of the HIP kernel at the horizons around the unroll depths of the two sequential chains
(riccati.inc forward_chain, backward_chain), in the dense system of tests/newton.py exactly as test_gpu_newton.py
checks it at N = 50, 1, 2, 3, 7: same samples, same dumped iterations, same bounds.

Both chains run PF coefficient slots in a straight-line body of PF steps followed by up to PF - 1 remainder steps,
with the fetches PF - 1 stages ahead of the steps (past the horizon's end in forward_chain, below stage 0 in
backward_chain) and one counted wait per step whose count depends on the step's place in the body.  The horizons are
the ones at which that structure changes shape:

    forward_chain, PF = 6:   4, 5 remainder only; 6 exactly one body; 11 a body and the longest remainder; 12 two bodies
    backward_chain, PF = 4:  4 exactly one body; 5, 6 a body and a remainder; 8 two bodies; 11 two bodies and the longest
                             remainder; 12 three bodies  (3: remainder only and 7: a body and the longest remainder are
                             test_gpu_newton.py's)

The step is dumped before and after the refinement: the unrefined step runs forward_chain on the factorisation's
record, the refined one runs backward_chain and forward_chain on the refinement right-hand sides.  `ipm_kernel_dump`
instantiates the same linear_solve as the production kernel (see test_gpu_newton.py).
"""
import pytest

torch = pytest.importorskip("torch")   # tests/newton.py needs it

import newton_cases as NC  # noqa: E402
from newton_gpu import horizon, step_solves_the_dense_system  # noqa: E402

pytestmark = pytest.mark.gpu

HORIZONS = (4, 5, 6, 8, 11, 12)


@pytest.fixture(scope="module")
def batch():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback by design)")
    from learningagileflight_se3_amd import scenario as S
    return S.synthetic_batch(64, seed=2025)


@pytest.mark.parametrize("N", HORIZONS)
def test_step_solves_the_dense_system(batch, N):
    """The refined step has a residual ratio <= 1e-5 in every case, and the largest ratio of the refined and of the
    unrefined steps is at most MARGIN times the oracle's on the same cases."""
    prob, ocases, gcases = horizon(batch, N)
    assert set(ocases) == set(gcases)
    step_solves_the_dense_system(f"N={N}", "-chain", prob, N, ocases, gcases)


@pytest.mark.parametrize("N", HORIZONS)
def test_dump_structure(batch, N):
    """dx of stage 0 exactly 0, every entry up to N written and finite, the padding beyond N untouched."""
    prob, _, gcases = horizon(batch, N)
    NC.structure(prob, N, gcases)
