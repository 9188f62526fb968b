"""Every walk the ray-query API reaches (mcrt_trace_closest / mcrt_trace_any), judged against the
float64 brute-force ground truth of tests/ray_truth.py: zero strong failures (determined rays: exact
shape, primitive and hit-or-miss, t and (u, v) within the float32 bounds) and zero weak failures
(every other ray: the answer is one float32 arithmetic can give).  The truth's constants were fixed
on the CPU against the oracle (tests/test_ray_truth_cpu.py) and are not touched here.

Layouts: the default build (compact 32-B / 48-B records, qwalk), MCRT_QUANT_NODES=0 (64-B records,
traverseOct), device_build=1 (LBVH: another tree, 64-B records), device_build=3 (host SAH),
force_2level (traverse2L over identity instances) and an instanced scene on its natural two-level
path (rotation, non-uniform scale, mirror, a translation of 1000 units).  The two-level layouts are
judged with K_2L = 2 K: the walk transforms the ray once more (world -> object), a rounding of the
same size on o and on d, so every bound of the truth doubles.

Orders: shuffled (mixed waves: the generic loops) and sorted by the sign octant of safeInvDir(d)
with every octant padded to whole 64-ray blocks (one wave = one block = one octant: the
traverseOct<., 0..7> / slabHit<0..7> instantiations, reached without a render).

Shapes: 1, 63, 64, 65 and 4097 rays; every third ray inactive; a masked run; the 1-, 2- and
3-triangle scenes (the root is a leaf, one or two internal nodes); the edge scene 1000 units from
the origin through the compact and the 64-B walks.

Share of determined rays, closest / any-hit, measured (seed 7; the same for every walk of a
column: the truth does not depend on the walk; printed per family with -s):
                 edge scene, K   edge scene, K_2L  edge at 1000, K  instanced, K_2L
  generic        1.000 / 1.000   1.000 / 1.000     0.973 / 0.993    1.000 / 1.000
  axis           1.000 / 1.000   1.000 / 1.000     0.996 / 0.996    0.992 / 0.996
  axis_on_plane  0.387 / 0.483   0.387 / 0.483     0.387 / 0.483    0.967 / 0.967
  tiny           1.000 / 1.000   1.000 / 1.000     0.989 / 0.993    0.995 / 0.996
  aimed          0.897 / 0.967   0.897 / 0.967     0.854 / 0.956    0.576 / 0.712
  tmax           0.623 / 0.623   0.623 / 0.623     0.530 / 0.530    0.597 / 0.609
  far            0.833 / 0.952   0.745 / 0.857     0.803 / 0.953    0.702 / 0.810
  on_surface     0.000 / 0.727   0.000 / 0.727     0.000 / 0.710    0.000 / 0.495
Per launch of the edge scene's 7046 rays: 5356 determined / 1690 weak-only (closest), 5996 / 1050
(any-hit); with K_2L 5303 / 1743 and 5939 / 1107.  Every layout: 0 strong, 0 weak failures.

That the octant blocks reach the specialised loops was checked once with a deliberately wrong
library (z plane pick of traverseOct<., 5> swapped; the y byte permutation of qwalk dropped for
rays with a negative x direction): the 64-B layouts then pass shuffled and fail in octant blocks
only (311 strong + 75 weak closest failures, 386 any-hit), the compact layouts fail in both
orders (725 + 188), the two-level layout -- untouched code -- passes.
"""
import os

import numpy as np
import pytest

import ray_truth as rt
from mcrt import types as T

pytestmark = pytest.mark.gpu

SEED = 7
LAYOUTS = {
    # name: (environment at build time, DeviceScene options, two-level?)
    "compact": ({}, {}, False),
    "plain64": ({"MCRT_QUANT_NODES": "0"}, {}, False),
    "lbvh": ({}, {"device_build": 1}, False),
    "host_sah": ({}, {"device_build": 3}, False),
    "forced_2level": ({}, {"force_2level": True}, True),
}


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


def _build(ctx, scene, layout, check_records=True, opts=None):
    """The DeviceScene of `layout`, built inside its environment (the variables are read at build
    time), with the layout's own evidence that the intended records are in use.  opts: further
    DeviceScene options (tests/test_gpu_build_opts.py: cost / bins / sah)."""
    from mcrt import lib
    env, lopts, two_level = LAYOUTS[layout]
    opts = dict(lopts, **(opts or {}))
    ds = _with_env(env, lambda: lib.DeviceScene(ctx, scene, **opts))
    info = ds.info()
    if layout == "compact":
        assert info["bytes"] > 64 * info["nodes"], info        # the compact records are really on
    if layout == "plain64" or (layout == "lbvh" and check_records):
        assert info["bytes"] == 64 * info["nodes"], info
    if layout == "lbvh":
        assert ds.builder() == 1
    assert ds.layout()["two_level"] == (1 if two_level else 0)
    return ds


def _trace(ctx, ds, rays, init=-7):
    """(closest hits, any-hit answers) of `rays`; the outputs are pre-filled with `init`."""
    import torch
    n = len(rays)
    r = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    h0 = np.zeros(n, T.ISECT_DTYPE)
    h0["shapeid"] = init
    h0["primid"] = init
    h = torch.from_numpy(h0.view(np.uint8).copy()).cuda()
    a = torch.full((n,), init, dtype=torch.int32, device="cuda")
    ds.trace_closest(r.data_ptr(), n, h.data_ptr())
    ds.trace_any(r.data_ptr(), n, a.data_ptr())
    ctx.sync()
    return h.cpu().numpy().view(T.ISECT_DTYPE), a.cpu().numpy()


class Case:
    """A scene, its rays of every family and their truths (one per K, computed on first use)."""

    def __init__(self, scene, inside=True):
        self.scene = scene
        self.rays, self.fam = rt.all_families(scene, SEED, inside)
        self.tris, self.sid, self.pid = rt.world_triangles64(scene)
        self._truth = {}

    def truth(self, K):
        if K not in self._truth:
            self._truth[K] = rt.classify(self.tris, self.rays, K=K, shape=self.sid, prim=self.pid)
        return self._truth[K]

    def report(self, what, K):
        tr = self.truth(K)
        for i, f in enumerate(rt.FAMILIES):
            m = self.fam == i
            print(f"{what:24s} K={K:3.0f} {f:14s} {int(m.sum()):5d} rays, determined closest "
                  f"{tr.closest_det[m].mean():.3f} any {tr.any_det[m].mean():.3f}, weak-only closest "
                  f"{int((~tr.closest_det[m]).sum())} any {int((~tr.any_det[m]).sum())}")


_CASES = {"edge0": lambda: Case(rt.edge_scene()),
          "edge1000": lambda: Case(rt.edge_scene((1000.0, 1000.0, 1000.0))),
          "instanced": lambda: Case(rt.instanced_edge_scene())}
_shared = {}


def shared_case(name):
    """The Case `name`, made once per process: its truths do not depend on the tree, so every test
    module that walks these scenes (tests/test_gpu_build_opts.py too) judges against the same ones."""
    if name not in _shared:
        _shared[name] = _CASES[name]()
    return _shared[name]


@pytest.fixture(scope="module")
def edge0():
    return shared_case("edge0")


@pytest.fixture(scope="module")
def edge1000():
    return shared_case("edge1000")


@pytest.fixture(scope="module")
def instanced():
    return shared_case("instanced")


def _judge_launch(ctx, ds, case, tr, index, what, rays=None):
    """Traces case.rays[index] (or `rays`, which must be those rays with other flags) and judges
    both queries; returns the failures as text."""
    rays = case.rays[index] if rays is None else rays
    hits, occl = _trace(ctx, ds, rays)
    vc = rt.judge(tr, rays, hits=hits, index=index)
    va = rt.judge(tr, rays, occl=occl, index=index)
    print(f"{what}: closest {vc.active} rays, {vc.determined} determined, {vc.weak_only} weak-only, "
          f"{len(vc.strong)}/{len(vc.weak)} failures, uv excess {vc.uv_excess:.2e}; any {va.determined} determined, "
          f"{va.weak_only} weak-only, {len(va.strong)}/{len(va.weak)} failures")
    out = []
    for tag, v in (("closest", vc), ("any", va)):
        if not v.ok():
            fams = sorted({rt.FAMILIES[case.fam[i]] for i, _ in v.strong + v.weak})
            out.append(f"{what} {tag} (families {fams}): {v}")
            for i, _ in (v.strong + v.weak)[:8]:
                out.append(f"    ray {i}: o,tmax {case.rays['o'][i].tolist()} d {case.rays['d'][i].tolist()}")
    return out


def _both_orders(ctx, ds, case, tr, what):
    rng = np.random.default_rng(SEED)
    shuffled = rng.permutation(len(case.rays))
    blocks = rt.octant_blocks(case.rays)
    # every 64-ray block of the sorted order is one octant, and each octant fills whole blocks
    oc = rt.octant(case.rays[blocks]).reshape(-1, 64)
    assert (oc == oc[:, :1]).all()
    assert set(oc[:, 0].tolist()) == set(range(8))
    bad = _judge_launch(ctx, ds, case, tr, shuffled, f"{what} shuffled")
    bad += _judge_launch(ctx, ds, case, tr, blocks, f"{what} octant blocks")
    return bad


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_edge_scene_layouts(hip_ctx, edge0, layout):
    K = rt.K_2L if LAYOUTS[layout][2] else rt.K
    if layout in ("compact", "forced_2level"):
        edge0.report("edge scene", K)
    ds = _build(hip_ctx, edge0.scene, layout)
    try:
        bad = _both_orders(hip_ctx, ds, edge0, edge0.truth(K), layout)
    finally:
        ds.close()
    assert not bad, "\n".join(bad)


def test_instanced_two_level(hip_ctx, instanced):
    from mcrt import lib
    instanced.report("instanced scene", rt.K_2L)
    ds = lib.DeviceScene(hip_ctx, instanced.scene)
    try:
        lay = ds.layout()
        assert lay["two_level"] == 1 and lay["instances"] >= 4, lay
        bad = _both_orders(hip_ctx, ds, instanced, instanced.truth(rt.K_2L), "instanced")
    finally:
        ds.close()
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("layout", ["compact", "plain64"])
def test_far_scene(hip_ctx, edge1000, layout):
    """The compact walk far from the origin, against something other than the exact walk."""
    if layout == "compact":
        edge1000.report("edge scene at 1000", rt.K)
    ds = _build(hip_ctx, edge1000.scene, layout)
    try:
        bad = _both_orders(hip_ctx, ds, edge1000, edge1000.truth(rt.K), f"far {layout}")
    finally:
        ds.close()
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("layout", ["compact", "plain64", "forced_2level"])
def test_ray_counts_inactive_and_mask(hip_ctx, edge0, layout):
    K = rt.K_2L if LAYOUTS[layout][2] else rt.K
    tr = edge0.truth(K)
    rng = np.random.default_rng(SEED + 1)
    order = rng.permutation(len(edge0.rays))
    ds = _build(hip_ctx, edge0.scene, layout)
    try:
        bad = []
        for n in (1, 63, 64, 65, 4097):      # partial, whole and whole + 1 waves; more than one block
            bad += _judge_launch(hip_ctx, ds, edge0, tr, order[:n], f"{layout} n={n}")
        # every third ray inactive: its output keeps the sentinel
        idx = order[:4097]
        rays = edge0.rays[idx].copy()
        rays["extra"][::3, 1] = 0
        bad += _judge_launch(hip_ctx, ds, edge0, tr, idx, f"{layout} inactive", rays=rays)
        # masked: each ray masks the shape it hits first; judged against the truth without it
        g = np.nonzero(np.isin(edge0.fam, [rt.FAMILIES.index(f) for f in ("generic", "aimed", "axis")])
                       & (tr.closest_tri >= 0))[0][:1500]
        rays = edge0.rays[g].copy()
        rays["extra"][:, 0] = edge0.sid[tr.closest_tri[g]]
        trm = rt.classify(edge0.tris, rays, K=K, shape=edge0.sid, prim=edge0.pid)
        assert trm.closest_det.mean() > 0.9 and (trm.closest_tri >= 0).mean() > 0.3
        hits, occl = _trace(hip_ctx, ds, rays)
        assert not (hits["shapeid"] == rays["extra"][:, 0]).any()
        for v in (rt.judge(trm, rays, hits=hits), rt.judge(trm, rays, occl=occl)):
            print(f"{layout} masked: {v.active} rays, {v.determined} determined, {len(v.strong)}/{len(v.weak)} failures")
            if not v.ok():
                bad.append(f"{layout} masked: {v}")
    finally:
        ds.close()
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("layout", ["compact", "plain64", "lbvh", "forced_2level"])
def test_tiny_scenes(hip_ctx, layout):
    """1, 2 and 3 triangles, one shape each, flat boxes.  (An LBVH of one triangle is a single
    leaf, trivially depth-first, so it gets a compact record as well: its records are not
    checked here.)"""
    K = rt.K_2L if LAYOUTS[layout][2] else rt.K
    bad = []
    for sc in rt.tiny_scenes():
        case = Case(sc, inside=False)
        ds = _build(hip_ctx, sc, layout, check_records=layout != "lbvh")
        try:
            bad += _both_orders(hip_ctx, ds, case, case.truth(K), f"{sc.name} {layout}")
        finally:
            ds.close()
    assert not bad, "\n".join(bad)
