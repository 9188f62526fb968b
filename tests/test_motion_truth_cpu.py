"""The constants of tests/motion_truth.py (CHAIN, REC, NORMAL) against a float32 numpy restatement of
the chains k_guides_motion evaluates, over random poses of the kinds the GPU test moves shapes by
(translation, rotation with a non-uniform scale, a mirror), near the origin and 1000 units away.
Runs without a GPU; no kernel result is involved."""
import numpy as np
import pytest

import motion_truth as mt
from mcrt import scenes
from ray_truth import U

F = np.float32


def _poses(rng, far):
    base = scenes._affine(rng.uniform(0.3, 2.0), rng.uniform(0, 360), rng.uniform(-7, 7, 3) + far, rng.uniform(-40, 40))
    T = np.eye(4)
    T[:3, 3] = rng.uniform(-1, 1, 3)
    R = scenes._affine(1.0, rng.uniform(-30, 30), rng.uniform(-0.5, 0.5, 3), rng.uniform(-20, 20)).astype(np.float64)
    R[:3, :3] = R[:3, :3] @ np.diag(rng.uniform(0.5, 2.0, 3))
    Mi = np.diag([-1.0, 1.0, 1.0, 1.0])
    for move in (T, R, Mi):
        cur = (move @ base.astype(np.float64)).astype(F)
        yield base, cur


def _inv_t(M):
    return np.linalg.inv(np.asarray(M, np.float64)).T.astype(F)


@pytest.mark.parametrize("far", [0.0, 1000.0], ids=["origin", "far"])
def test_constants_hold_for_the_float32_restatement(far):
    rng = np.random.default_rng(11)
    worst = dict(chain=0.0, rec=0.0, normal=0.0)
    for _ in range(40):
        for M_prev, M_cur in _poses(rng, far):
            n = 500
            tris = (rng.uniform(-1.2, 1.2, (n, 1, 3)) + rng.uniform(-0.2, 0.2, (n, 3, 3))).astype(F)
            bary = rng.dirichlet((1, 1, 1), n)[:, :2].astype(F)
            P32, d32 = mt.restate_motion(M_prev, M_cur, tris, bary)
            b = bary.astype(np.float64)
            w = np.stack([1.0 - b[:, 0] - b[:, 1], b[:, 0], b[:, 1]], -1)
            q = (tris.astype(np.float64) * w[..., None]).sum(1)
            Mp, Mc = M_prev.astype(np.float64), M_cur.astype(np.float64)
            P_true = q @ Mc[:3, :3].T + Mc[:3, 3]
            d_true = (q @ Mp[:3, :3].T + Mp[:3, 3]) - P_true
            S_prev, S_cur = mt.chain_scale(M_prev, tris), mt.chain_scale(M_cur, tris)
            e = mt.CHAIN * U * (S_prev + S_cur) + U * np.abs(d_true).max(-1)
            worst["chain"] = max(worst["chain"], (np.abs(d32 - d_true).max(-1) / e).max())
            # the guide depth as k_guides forms it, and the point rebuilt from it along the exact direction
            cam = (np.array([0.0, 5.0, -13.0]) + far).astype(F)
            v = P32 - cam
            depth = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
            v64 = P32.astype(np.float64) - cam.astype(np.float64)
            P_rec = cam.astype(np.float64) + v64 / np.linalg.norm(v64, axis=-1, keepdims=True) * depth.astype(np.float64)[:, None]
            e = mt.REC * U * (depth.astype(np.float64) + np.abs(cam).max()) + mt.CHAIN * U * S_cur
            worst["rec"] = max(worst["rec"], (np.abs(P_rec - P_true).max(-1) / e).max())
            # vertex normals within 30 degrees of a common direction
            c = rng.normal(size=(n, 1, 3))
            c /= np.linalg.norm(c, axis=-1, keepdims=True)
            nrm = c + rng.uniform(-0.3, 0.3, (n, 3, 3))
            nrm = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(F)
            ITp, ITc = _inv_t(M_prev), _inv_t(M_cur)
            n_cur, n_prev = mt.restate_normal(ITc, nrm, bary), mt.restate_normal(ITp, nrm, bary)
            want, e_n = mt.truth_normal(n_cur, ITp, ITc)
            worst["normal"] = max(worst["normal"], np.abs(n_prev - want).max() / e_n)
    print("largest error / bound:", {k: round(float(v), 3) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst
