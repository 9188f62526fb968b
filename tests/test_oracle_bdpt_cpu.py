"""CPU tests: the oracle's BDPT restatement (oracle/mcrt_oracle.c, KRN/BDPT.cl in RTBDPTPass order)
against the REFERENCE's own BDPT.cl kernels run on an MI355X (committed fixtures
tests/golden/clref_bdpt_ieee.npz, tests/clref_job.py ... bdpt): frames rendered in sequence from
fresh (zero-filled) state, so the s = 1 strategy's previous-frame sampled light vertex
(BDPT.cl:585-586) is reproduced too.

Tolerance (as the PT oracle): per pixel |dL| <= 1e-4 * max(1, |L|) on >= 99.5 % of
pixels per 1-spp frame, the rest are path divergences (host libm and IEEE division vs the GPU's,
no contraction) -- in BDPT a diverged light subpath also moves its light-tracing splats; subpath
vertex counts equal on >= 99.5 % of pixels."""
import os

import numpy as np
import pytest

from clref_job import BDPT_CASES, BDPT_NAN_FRAME, BDPT_NAN_PIXEL, BDPT_TAA_CASES, bdpt_key, build_scene
from mcrt.camera import scene_camera
from oracle import pyoracle as po

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("case", BDPT_CASES, ids=[bdpt_key(c) for c in BDPT_CASES])
def test_bdpt_oracle_matches_reference(case):
    name, W, H, frames, D = case
    key = bdpt_key(case)
    z = np.load(os.path.join(GOLD, "clref_bdpt_ieee.npz"), allow_pickle=False)
    o = po.OracleScene(build_scene(name))
    o.build()
    b = po.OracleBDPT(o, W, H, D)
    cam = scene_camera(name, W, H)
    for f in frames:
        rad, cc, lc, st = b.render(cam, frame=f)
        ref = z[f"{key}_f{f}"][..., :3].astype(np.float64)
        d = np.abs(rad[..., :3] - ref)
        ok = (d <= 1e-4 * np.maximum(1.0, np.abs(ref))).all(-1).mean()
        assert ok >= 0.995, (key, f, ok)
        assert st[0] > 0 and st[2] > 0
    assert (cc == z[f"{key}_camera_counts"].view(np.int32)).mean() >= 0.995
    assert (lc == z[f"{key}_light_counts"].view(np.int32)).mean() >= 0.995


def test_bdpt_oracle_nonfinite_pixel_of_frame_10():
    """The precondition of the GPU tests that carry a non-finite pixel through every BDPT path
    (tests/test_gpu_bdpt.py): the mixed scene at 96 x 64, D = 2, frames 0..11 in order from fresh
    state with the TAA-jittered cameras.  In frame 10 the light subpath of pixel (row 35, column 78)
    starts on an area light with a cosine-hemisphere sample whose second random number is exactly
    1.0f, so cos = 0 and pdfDir = 0, and BDPT.cl:310's Le * absDot(n, d) / (lightPdf * pdfPos * pdfDir)
    is 0 / 0: the NaN light throughput reaches the pixel through its own (t = 2, s = 2) strategy,
    which BDPT.cl:904-906 adds without a test (the t = 1 splats are guarded by isNotBlack,
    BDPT.cl:893, which is false for NaN).  So the pixel is NaN when only its row is rendered and 0
    when every other row is."""
    name, W, H, D, frames = "mixed", 96, 64, 2, 12
    o = po.OracleScene(build_scene(name))
    o.build()
    cams = [scene_camera(name, W, H, frame=f, jitter=True) for f in range(frames)]
    others = np.array([r for r in range(H) if r != 35], np.int32)
    runs = {}
    for key, rows in (("all", None), ("row35", np.array([35], np.int32)), ("others", others)):
        b = po.OracleBDPT(o, W, H, D)
        runs[key] = [b.render(cams[f], frame=f, rows=rows)[0] for f in range(frames)]
    bad = [np.argwhere(~np.isfinite(r).all(-1)).tolist() for r in runs["all"]]
    print("oracle non-finite pixels per frame:", bad)
    assert sum(len(p) for p in bad) >= 1 and max(len(p) for p in bad) <= 4, bad
    assert bad[10] == [[35, 78]], bad[10]
    assert np.isnan(runs["all"][10][35, 78, :3]).all() and runs["all"][10][35, 78, 3] == 0
    assert not np.isfinite(runs["row35"][10][35, 78, :3]).any()
    assert not runs["others"][10][35, 78].any()
    assert all(np.isfinite(r).all() for r in runs["others"])
    # the case the GPU tests run against the reference live, and the pixel they pin, are these
    assert BDPT_TAA_CASES[0] == (name, W, H, tuple(range(frames)), D)
    assert (BDPT_NAN_FRAME, BDPT_NAN_PIXEL) == (10, (35, 78))


def test_bdpt_oracle_rows_and_no_lights():
    """Row-subset rendering (the bench's CPU baseline sample) fills only those rows' own
    strategies; a scene without lights renders black (RTBDPTPass.cpp:69)."""
    sc = build_scene("mixed")
    o = po.OracleScene(sc)
    o.build()
    W, H = 48, 32
    cam = scene_camera("mixed", W, H)
    full, _, _, _ = po.OracleBDPT(o, W, H, 2).render(cam, frame=0)
    rows = np.array([3, 17, 30], np.int32)
    part, cc, _, st = po.OracleBDPT(o, W, H, 2).render(cam, frame=0, rows=rows)
    assert (cc.reshape(H, W)[rows] >= 1).all() and (cc.reshape(H, W)[[0, 1, 2]] == 0).all()
    assert st[0] > 0 and np.abs(part).sum() > 0
    sc.lights = sc.lights[:0]
    o2 = po.OracleScene(sc)
    o2.build()
    rad, _, _, _ = po.OracleBDPT(o2, W, H, 2).render(cam, frame=0)
    assert not rad.any()
    assert full[..., :3].max() > 0
