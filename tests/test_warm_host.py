"""Host checks of the warm start's Python side (no device): moving_gate.reframe_record_t, which carries an optimum
record from one gate frame to the next, and the ctypes mirror of lafse3_warm_opts.

reframe_record_t: world-frame states are put into an old and a new gate frame with moving_gate.transform (the
reference's map, numpy / scipy); the record holding the old-frame states, reframed old -> new, must hold the new-frame
positions and velocities to 1e-12 (rotations of unit vectors and offsets of a few metres in float64: rounding is
~1e-15) and every other word bit for bit.  With both frames the identity matrix and equal centroids the map is the
identity, bit for bit.
"""
import ctypes
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from learningagileflight_se3_amd import _lib  # noqa: E402
from learningagileflight_se3_amd import moving_gate as MG  # noqa: E402
from learningagileflight_se3_amd import scenario as S  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "lafse3.h")
REC_W, NROW, NX = 2223, 51, 13


def _frames(B, seed):
    """Two gates per episode (corners (B, 4, 3)): the second is the first moved and pitched."""
    rs = np.random.RandomState(seed)
    samples = np.stack([S.nn_sample(rs) for _ in range(B)])
    gp0, _ = MG.initial_episodes(samples)
    old = MG.rotate_y(MG.translate(gp0, rs.uniform(-0.5, 0.5, (B, 3))), rs.uniform(-0.4, 0.4, B))
    new = MG.rotate_y(MG.translate(old, rs.uniform(-0.3, 0.3, (B, 3))), rs.uniform(-0.3, 0.3, B))
    return old, new


def test_reframe_record_moves_positions_and_velocities_only():
    B = 5
    old, new = _frames(B, 11)
    rs = np.random.RandomState(12)
    world = rs.uniform(-3, 3, (B, NROW, NX))
    world[:, :, 6:10] /= np.linalg.norm(world[:, :, 6:10], axis=2, keepdims=True)
    rec = rs.standard_normal((B, REC_W))
    x_old, x_new = np.zeros_like(world), np.zeros_like(world)
    for k in range(NROW):
        x_old[:, k] = MG.transform(MG.gate_frame(old), MG.centroid(old), world[:, k])
        x_new[:, k] = MG.transform(MG.gate_frame(new), MG.centroid(new), world[:, k])
    rec[:, :NROW * NX] = x_old.reshape(B, -1)
    t = lambda a: torch.as_tensor(a)   # noqa: E731
    rec_t = t(rec)
    keep = rec_t.clone()
    out = MG.reframe_record_t(rec_t, MG.gate_frame_t(t(old)), MG.centroid_t(t(old)), MG.gate_frame_t(t(new)),
                              MG.centroid_t(t(new)))
    assert torch.equal(rec_t, keep)                       # the input is not modified
    out = out.numpy()
    xo = out[:, :NROW * NX].reshape(B, NROW, NX)
    err = np.abs(xo[:, :, 0:6] - x_new[:, :, 0:6]).max()
    print(f"reframed positions / velocities against transform: max |diff| {err:.3e}")
    assert err <= 1e-12
    assert np.abs(xo[:, :, 0:6] - x_old[:, :, 0:6]).max() > 1e-2      # the frames differ: the map did something
    # every other word: quaternions and omega of the x block, and everything behind it
    assert np.array_equal(xo[:, :, 6:].view(np.int64), x_old[:, :, 6:].view(np.int64))
    assert np.array_equal(out[:, NROW * NX:].view(np.int64), rec[:, NROW * NX:].view(np.int64))


def test_reframe_record_identity_frame_change_is_the_identity():
    B = 4
    rs = np.random.RandomState(13)
    rec = torch.as_tensor(rs.standard_normal((B, REC_W)))
    eye = torch.eye(3, dtype=torch.float64).expand(B, 3, 3).contiguous()
    cen = torch.as_tensor(rs.uniform(-2, 2, (B, 3)))
    out = MG.reframe_record_t(rec, eye, cen, eye.clone(), cen.clone())
    assert out is not rec and torch.equal(out.view(torch.int64), rec.view(torch.int64))


def _header_struct(name):
    """ctypes fields of `typedef struct name { ... } name;` in include/lafse3.h (int32_t and double members)."""
    src = open(HEADER).read()
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S)
    assert m, f"{name} not declared in lafse3.h"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    ctype = {"int32_t": ctypes.c_int32, "double": ctypes.c_double}
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ty, names = decl.split(None, 1)
        fields += [(n.strip(), ctype[ty]) for n in names.split(",")]
    return fields


def test_warm_opts_mirror_has_the_headers_layout_and_defaults():
    fields = _header_struct("lafse3_warm_opts")
    assert [n for n, _ in fields] == ["shift", "mu_init", "bound_push", "bound_frac", "mult_bound_push"]
    assert fields == list(_lib.WarmOpts._fields_)
    header = type("HeaderWarmOpts", (ctypes.Structure,), {"_fields_": fields})
    assert ctypes.sizeof(_lib.WarmOpts) == ctypes.sizeof(header) == 40
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("liblafse3.so not built: run python -c 'import __graft_entry__ as g; g.build()'")
    lib = _lib.load()
    o = _lib.WarmOpts(7, -1.0, -1.0, -1.0, -1.0)
    assert lib.lafse3_default_warm_opts(ctypes.byref(o)) == 0
    # shift 0, mu_init 1e-3, the pushes IPOPT's warm_start_bound_push / _bound_frac / _mult_bound_push defaults
    assert (o.shift, o.mu_init, o.bound_push, o.bound_frac, o.mult_bound_push) == (0, 1e-3, 1e-3, 1e-3, 1e-3)
    assert lib.lafse3_default_warm_opts(None) == -1
    d = _lib.default_warm_opts(shift=2)
    assert (d.shift, d.mu_init) == (2, 1e-3)
    # a NULL context is refused before anything else (no device call)
    assert lib.lafse3_ocp_solve_warm(None, 1, *([None] * 7), None, None, *([None] * 6), None, None, None) == -1
