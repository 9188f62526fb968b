"""The float64 ground truth of tests/ray_truth.py, validated on the CPU against the reference's
arithmetic -- the oracle's restatement of intersect_bvh2_lds.cl (OracleScene.closest / .any) --
and never against a kernel.

  * the oracle shows ZERO strong and ZERO weak failures on every ray family, on the edge scene at
    the origin and 1000 units away, on the 1-, 2- and 3-triangle scenes and on the instanced
    scene (whose transforms the oracle bakes into world triangles): this is what fixes
    K = 32 (ray_truth.K; the value did not have to be raised) and UV_SLACK (the oracle needs
    none: its (u, v) stay inside the b half-widths, largest excess -1.5e-6);
  * the judge flags corrupted answers: the second-nearest hit, a neighbouring primitive and a
    miss turned into a hit always, t (1 + 1e-4) on at least 90 % of the rays;
  * the share of determined rays (the ones that get the strong check) has a floor per family, so
    the strong check cannot go vacuous; tmax, axis_on_plane and on_surface are ambiguous by design
    and get none, but tmax and axis_on_plane must hold at least 100 determined rays each.

Measured (seed 7; closest / any-hit share of determined rays, edge scene at the origin | at 1000):
  generic 1.000 / 1.000 | 0.973 / 0.993     axis  1.000 / 1.000 | 0.996 / 0.996
  tiny    1.000 / 1.000 | 0.989 / 0.993     aimed 0.897 / 0.967 | 0.854 / 0.956
  far     0.833 / 0.952 | 0.803 / 0.953     tmax  0.623 / 0.623 | 0.530 / 0.530
  axis_on_plane 0.387 / 0.483 | 0.387 / 0.483          on_surface 0 / 0.727 | 0 / 0.710
"""
import numpy as np
import pytest

import ray_truth as rt
from oracle import pyoracle as po

SEED = 7
FLOORS = {"generic": 0.95, "axis": 0.95, "tiny": 0.90, "far": 0.80, "aimed": 0.70}
SCENES = ["edge0", "edge1000", "tiny1", "tiny2", "tiny3", "instanced"]


def _scene(key):
    if key == "edge0":
        return rt.edge_scene(), True
    if key == "edge1000":
        return rt.edge_scene((1000.0, 1000.0, 1000.0)), True
    if key == "instanced":      # the oracle bakes the transforms: a flat scene of world triangles
        return rt.instanced_edge_scene(), True
    return rt.tiny_scenes()[int(key[-1]) - 1], False


_cache = {}


def _case(key):
    """(scene, rays, family per ray, truth, oracle closest, oracle any), computed once per scene."""
    if key not in _cache:
        sc, inside = _scene(key)
        rays, fam = rt.all_families(sc, SEED, inside)
        tris, sid, pid = rt.world_triangles64(sc)
        tr = rt.classify(tris, rays, shape=sid, prim=pid)
        o = po.OracleScene(sc)
        o.build()
        _cache[key] = (sc, rays, fam, tr, o.closest(rays), o.any(rays))
    return _cache[key]


def _only(rays, hits, occl, m):
    """The family's rays alone: the others inactive, their outputs at the sentinel."""
    r, h, a = rays.copy(), hits.copy(), occl.copy()
    r["extra"][~m, 1] = 0
    h["shapeid"][~m] = h["primid"][~m] = -7
    a[~m] = -7
    return r, h, a


@pytest.mark.parametrize("key", SCENES)
def test_oracle_agrees_with_truth(key):
    _, rays, fam, tr, hc, ha = _case(key)
    bad = []
    for i, f in enumerate(rt.FAMILIES):
        r, h, a = _only(rays, hc, ha, fam == i)
        vc, va = rt.judge(tr, r, hits=h), rt.judge(tr, r, occl=a)
        print(f"{key:9s} {f:14s} closest: {vc.share:.3f} determined, {vc.weak_only} weak-only, uv excess "
              f"{getattr(vc, 'uv_excess', float('nan')):.2e} | any: {va.share:.3f} determined, {va.weak_only} weak-only")
        if not (vc.ok() and va.ok()):
            bad.append(f"{key} {f}\n closest: {vc}\n any: {va}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("key", ["edge0", "edge1000"])
def test_determined_share_floors(key):
    _, rays, fam, tr, _, _ = _case(key)
    for f, floor in FLOORS.items():
        m = fam == rt.FAMILIES.index(f)
        assert tr.closest_det[m].mean() >= floor, (f, tr.closest_det[m].mean())
    for f in ("tmax", "axis_on_plane"):
        m = fam == rt.FAMILIES.index(f)
        assert tr.closest_det[m].sum() >= 100 and tr.any_det[m].sum() >= 100, f
    # every verdict kind occurs: determined hits and misses, ambiguous rays, occluded and free
    assert (tr.closest_det & (tr.closest_tri >= 0)).sum() > 1000 and (tr.closest_det & (tr.closest_tri < 0)).sum() > 100
    assert (~tr.closest_det).sum() > 500 and (tr.any_det & (tr.any_val == 1)).sum() > 1000


def test_uv_slack_covers_the_oracle():
    """UV_SLACK is measured here: how far the oracle's recomputed barycentrics leave the b
    half-widths (they do not: the largest excess is negative) -- and stays far below 2e-3."""
    worst = -np.inf
    for key in SCENES:
        _, rays, _, tr, hc, _ = _case(key)
        v = rt.judge(tr, rays, hits=hc, uv_slack=0.0)
        assert v.ok(), v
        worst = max(worst, v.uv_excess)
    print(f"largest (u, v) excess over the b half-widths: {worst:.3e}")
    assert worst <= 0.0 < rt.UV_SLACK <= 2e-3


def test_judge_flags_corruptions():
    """300 determined hits / misses each; every wrong triangle or invented hit must be flagged,
    and t (1 + 1e-4) on >= 90 % of the rays (the t half-width of a distant hit exceeds 1e-4 t)."""
    _, rays, fam, tr, hc, ha = _case("edge0")
    rng = np.random.default_rng(3)
    two = np.nonzero(tr.closest_det & (tr.closest_tri >= 0) & (tr.n_clear >= 2))[0]
    hit = np.nonzero(tr.closest_det & (tr.closest_tri >= 0))[0]
    miss = np.nonzero(tr.closest_det & (tr.closest_tri < 0))[0]
    assert len(two) >= 300 and len(hit) >= 300 and len(miss) >= 300
    two, hit, miss = (rng.choice(x, 300, replace=False) for x in (two, hit, miss))

    def flagged(h, idx):
        v = rt.judge(tr, rays, hits=h)
        got = {i for i, _ in v.strong + v.weak}
        assert got <= set(idx.tolist()), "an uncorrupted ray was flagged"
        return len(got)

    # the second-nearest clear hit, with its own correct t and (u, v)
    h = hc.copy()
    for i in two:
        s = np.arange(np.searchsorted(tr.ray, i), np.searchsorted(tr.ray, i + 1))
        s = s[(tr.kind[s] == rt.CLEAR) & (s != tr.closest_slot[i])]
        k = s[np.argmin(tr.t[s])]
        h["shapeid"][i], h["primid"][i] = tr.shape[tr.tri[k]], tr.prim[tr.tri[k]]
        h["uvwt"][i] = (tr.b1[k], tr.b2[k], 0.0, tr.t[k])
    assert flagged(h, two) == 300
    # the neighbouring primitive of the same shape, everything else unchanged
    h = hc.copy()
    cnt = tr.shape_count[h["shapeid"][hit]]
    h["primid"][hit] = (h["primid"][hit] + 1) % cnt
    assert (cnt > 1).all() and flagged(h, hit) == 300
    # a miss turned into a hit
    h = hc.copy()
    h["shapeid"][miss] = rng.integers(0, 27, 300)
    h["primid"][miss] = rng.integers(0, 48, 300)
    h["uvwt"][miss] = (0.25, 0.25, 0.0, 1.0)
    assert flagged(h, miss) == 300
    # a hit turned into a miss (closest and any-hit)
    h = hc.copy()
    h["shapeid"][hit] = h["primid"][hit] = -1
    assert flagged(h, hit) == 300
    a = ha.copy()
    occ = rng.choice(np.nonzero(tr.any_det & (tr.any_val == 1))[0], 300, replace=False)
    a[occ] = -1
    assert len(rt.judge(tr, rays, occl=a).strong) == 300
    # t (1 + 1e-4)
    h = hc.copy()
    h["uvwt"][hit, 3] *= np.float32(1.0 + 1e-4)
    n = flagged(h, hit)
    print(f"t (1 + 1e-4): {n} / 300 flagged")
    assert n >= 270


def test_mask_and_inactive_rays():
    """The mask removes a shape before classification; an inactive ray's output must stay."""
    sc, rays, fam, tr, hc, ha = _case("edge0")
    m = np.nonzero((fam == rt.FAMILIES.index("generic")) & (hc["shapeid"] >= 0))[0][:400]
    r = rays[m].copy()
    r["extra"][:, 0] = hc["shapeid"][m]
    tris, sid, pid = rt.world_triangles64(sc)
    trm = rt.classify(tris, r, shape=sid, prim=pid)
    o = po.OracleScene(sc)
    o.build()
    hm, am = o.closest(r), o.any(r)
    assert not (hm["shapeid"] == hc["shapeid"][m]).any()
    vc, va = rt.judge(trm, r, hits=hm), rt.judge(trm, r, occl=am)
    assert vc.ok() and va.ok() and vc.share > 0.9, f"{vc}\n{va}"
    assert not rt.judge(trm, r, hits=hc[m]).ok()          # the unmasked answers are flagged
    r["extra"][::3, 1] = 0
    hm["shapeid"][::3] = hm["primid"][::3] = -7
    assert rt.judge(trm, r, hits=hm).ok()
    hm["primid"][3] = 0
    assert len(rt.judge(trm, r, hits=hm).strong) == 1
