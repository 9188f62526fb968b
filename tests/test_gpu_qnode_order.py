"""The compact records in line order (mcrt_qnodes.hip: treelets, the default, and sibling pairs).

Records: the device's compact copy is read back and followed from the root beside the 64-B tree
(qnode_order_util.decode): every record reached exactly once, in the 64-B tree's left / right roles,
where the host order (mcrt_accel_compact_order) puts it, siblings in one line (treelets: a node and
both its children).  The box words of every record -- origin, bytes, exponents; a leaf's twelve
words -- are those the depth-first converter before this order produced for the same node
(tests/golden/qnode_boxes.json holds their SHA-256 per tree, dumped from that converter), and the
same in both orders.

Walks: closest-hit and any-hit queries and 64 x 48 PT frames at D = 2 and D = 5 are bit-identical
with the compact records on and MCRT_QUANT_NODES=0, on a 5,000-triangle soup and a 20 k-triangle
San-Miguel proxy, with the stop rule at cap 1 and at its default, and again after a vertex refit."""
import hashlib
import json
import os

import numpy as np
import pytest

import qnode_order_util as qu
import vertex_refit_util as vu
from helpers import random_rays
from mcrt import scenes
from mcrt.camera import make_camera, scene_camera

pytestmark = pytest.mark.gpu

ORDERS = {"siblings": "1", "treelets": "2"}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qnode_boxes.json")
W, H = 64, 48
CAPS = {"cap1": {"MCRT_WALK_CAP": "1", "MCRT_WALK_LANES": "64", "MCRT_WALK_MIN_PATHS": "0", "MCRT_WALK_MAXB": "8"},
        "default": {}}
_scene_cache, _ref_cache = {}, {}


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _scene(name):
    if name not in _scene_cache:
        _scene_cache[name] = scenes.san_miguel_proxy(tris=20_000) if name == "sm20k" else qu.soup(int(name[4:]))
    return _scene_cache[name]


def _camera(name, frame):
    if name == "sm20k":
        return scene_camera("san_miguel_proxy", W, H, frame=frame, jitter=True)
    return make_camera((0.5, 1.0, -7.0), (0.0, 0.0, 0.0), W, H, fovy=45.0)


def box_hash(words):
    h = hashlib.sha256()
    for w in words:
        h.update(np.ascontiguousarray(w, np.uint32).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("name", ["soup1", "soup2", "soup3", "soup7", "soup5000", "sm20k"])
def test_records_read_back(hip_ctx, name):
    from mcrt import lib
    sc = _scene(name)
    with open(GOLDEN) as f:
        golden = json.load(f)
    words = {}
    for order, env in ORDERS.items():
        ds = _with_env({"MCRT_QNODE_ORDER": env, "MCRT_QUANT_NODES": "1"}, lambda: lib.DeviceScene(hip_ctx, sc))
        try:
            kids = qu.kids_of(ds.records())
            q, root = ds.compact_records()
            assert len(q) > 0, "compact records not built"
            assert ds.info()["bytes"] == 64 * len(kids) + 16 * len(q)
            off, words[order] = qu.decode(q, root, kids)
        finally:
            ds.close()
        want, total = lib.compact_order(kids, int(env))
        assert total == len(q) and np.array_equal(off, want)
        leaf = kids[:, 0] < 0
        line, last = off // qu.LINE_UNITS, (off + np.where(leaf, 3, 2) - 1) // qu.LINE_UNITS
        assert (line == last).all(), "a record crosses a line"
        inner = np.flatnonzero(~leaf)
        if order == "siblings":
            assert (line[kids[inner, 0]] == line[kids[inner, 1]]).all()
        else:
            heads = inner[qu.depths(kids)[inner] % 2 == 0]
            assert (line[kids[heads, 0]] == line[heads]).all() and (line[kids[heads, 1]] == line[heads]).all()
        assert box_hash(words[order]) == golden[name]["sha256"], f"{order}: box words differ from the depth-first converter's"
        assert len(kids) == golden[name]["records"]
    assert all(np.array_equal(a, b) for a, b in zip(words["siblings"], words["treelets"]))


def _answers(hip_ctx, name, refit):
    """D = 2 and D = 5 frames, closest-hit records and any-hit flags of one structure."""
    import torch
    from mcrt import lib
    sc = _scene(name)
    ds = lib.DeviceScene(hip_ctx, sc)
    fb = lib.FrameBuffer(hip_ctx, W, H)
    try:
        if refit:
            moved = vu.deformed(sc)
            ds.update_vertices(moved.positions)
            ds.refit()
            sc = moved
        built = ds.info()["bytes"] > 64 * ds.info()["nodes"]
        frames = []
        for D in (2, 5):
            fb.render_frames(ds, [_camera(name, k) for k in range(2)], frame=0, max_depth=D)
            hip_ctx.sync()
            frames.append(np.stack([fb.read_frame(k) for k in range(2)]))
        rays = random_rays(sc, 20_000, seed=9)
        n = len(rays)
        r = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
        hits = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
        occ = torch.zeros(n, dtype=torch.int32, device="cuda")
        ds.trace_closest(r.data_ptr(), n, hits.data_ptr())
        ds.trace_any(r.data_ptr(), n, occ.data_ptr())
        hip_ctx.sync()
        return built, np.stack(frames), hits.cpu().numpy().reshape(n, 32).copy(), occ.cpu().numpy().copy()
    finally:
        fb.close()
        ds.close()


def _reference(hip_ctx, name, refit):
    """The 64-B records' answers, once per scene (no compact records: no stop rule either)."""
    if (name, refit) not in _ref_cache:
        _ref_cache[name, refit] = _with_env({"MCRT_QUANT_NODES": "0"}, lambda: _answers(hip_ctx, name, refit))
    return _ref_cache[name, refit]


@pytest.mark.parametrize("refit", [False, True], ids=["built", "refitted"])
@pytest.mark.parametrize("cap", list(CAPS))
@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("name", ["soup5000", "sm20k"])
def test_answers_identical_to_64b_records(hip_ctx, name, order, cap, refit):
    env = dict(CAPS[cap], MCRT_QNODE_ORDER=ORDERS[order], MCRT_QUANT_NODES="1")
    built, frames, hits, occ = _with_env(env, lambda: _answers(hip_ctx, name, refit))
    rbuilt, rframes, rhits, rocc = _reference(hip_ctx, name, refit)
    assert built and not rbuilt, "compact records: on in one arm, off in the other"
    assert np.isfinite(frames).all() and frames[..., :3].max() > 0
    assert (occ == 1).any() and (occ != 1).any() and (hits.view(np.int32)[:, 0] >= 0).any()
    diff = frames.view(np.uint32) != rframes.view(np.uint32)
    assert not diff.any(), f"{int(diff.any(-1).sum())} pixels differ"
    assert np.array_equal(occ, rocc), int((occ != rocc).sum())
    assert np.array_equal(hits, rhits), int((hits != rhits).any(-1).sum())
