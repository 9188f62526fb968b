"""Scenes and comparisons shared by tests/test_refit_cpu.py and tests/test_gpu_refit.py."""
import copy

import numpy as np

from mcrt import scenes


def synthetic(n, place=None):
    """n shapes over two meshes: a 12-triangle box, a single triangle, then instances of both in
    turn.  place(i) -> 4x4 local-to-world of shape i (default: an 8-wide grid, spacing 3)."""
    if place is None:
        place = grid_place
    b = scenes.SceneBuilder(f"refit_{n}")
    m = b.add_material(kd=(0.7, 0.7, 0.7))
    box = b.add_mesh(*scenes.box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)), m, transform=place(0))
    tri = None
    for i in range(1, n):
        if i == 1:
            tri = b.add_mesh(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.tile([0, 0, 1], (3, 1)),
                             np.zeros((3, 2)), np.array([[0, 1, 2]]), m, transform=place(i))
        else:
            b.add_instance(box if i % 2 == 0 else tri, place(i))
    return b.build()


def translate(t):
    M = np.eye(4, dtype=np.float32)
    M[:3, 3] = t
    return M


def grid_place(i):
    return translate((3.0 * (i % 8), 0.0, 3.0 * (i // 8)))


def with_transforms(scene, mats):
    """Copy of `scene` whose shape i has local-to-world mats[i] (and its inverse transpose)."""
    sc = copy.copy(scene)
    sc.shapes = scene.shapes.copy()
    sc._desc = None
    for i, M in enumerate(mats):
        M = np.asarray(M, np.float32)
        sc.shapes["toWorldTransform"][i] = M
        sc.shapes["toWorldInverseTranspose"][i] = np.linalg.inv(M.astype(np.float64)).T.astype(np.float32)
    return sc


def similarity_transforms(n, seed, spread=40.0):
    """Seeded uniform scale x rotation (yaw, tilt) x translation per shape."""
    rng = np.random.default_rng(seed)
    return [scenes._affine(rng.uniform(0.3, 2.0), rng.uniform(0, 360), rng.uniform(-spread, spread, 3),
                           rng.uniform(-60, 60)) for _ in range(n)]


def power_of_two_line(n):
    """Shape i at x = 2^i: every SAH split peels one shape off, so the top tree degenerates."""
    return [translate((float(2.0 ** i), 0.0, 0.0)) for i in range(n)]


def lattice_line(n_min, bins):
    """(built scene, moved scene) of at least n_min instances of one unit box (centre 0).  Moved, box i
    stands at (x_i, 0, 0) with x_i over build_opts.lattice_spots: the centroids of the world boxes
    then lie exactly on, and one float below, the planes k * (E / bins) that the top level's root
    prices with `bins` bins (centroid minimum 0, extent E, y and z extents 0), so a plane that is an
    ulp off changes the partition.  tests/test_build_opts_cpu.py checks that premise on the host."""
    from build_opts import lattice_spots
    spots = lattice_spots(bins, TOP_LATTICE_EXTENT)
    x = np.repeat(spots, -(-n_min // len(spots)))
    b = scenes.SceneBuilder(f"lattice_line_{len(x)}_{bins}")
    m = b.add_material(kd=(0.7, 0.7, 0.7))
    box = b.add_mesh(*scenes.box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)), m, transform=grid_place(0))
    for i in range(1, len(x)):
        b.add_instance(box, grid_place(i))
    sc = b.build()
    return sc, with_transforms(sc, [translate((float(v), 0.0, 0.0)) for v in x])


def spill_blocks(depth):
    """Spill blocks of 16 entries the traversal needs for a tree of this depth (mcrt_accel.cpp apply_spill_cap)."""
    return (depth + 2 + 15) // 16


def normalised(rec, top_records):
    """Records as uint32 with the one permitted normalisation: -0.0 -> +0.0 in the 12 box words of
    the top level's internal records (order-free min / max reductions on the device)."""
    r = np.ascontiguousarray(rec, np.float32).view(np.uint32).reshape(-1, 16).copy()
    top = r[:top_records]
    internal = top[:, 12].view(np.int32) >= 0
    boxes = top[internal, :12]
    boxes[boxes == 0x80000000] = 0
    top[internal, :12] = boxes
    return r


# Cases of tests/test_gpu_refit.py run once per forced path (tests/refit_job.py).  n1 .. n5000:
# the smallest top levels, one-wave requests (<= 256 shapes) on both sides of the wave size, several
# large requests and level passes (5000); then the degenerate arrangements.
RECORD_SIZES = (1, 2, 3, 64, 65, 257, 300, 5000)
# Build options (cost / bins / SAH switch) the structure must remember for its refits, as
# "<case>-<tag>": one large request and one wave (n300), several levels of large requests (n5000),
# the degenerate line at the smallest bin count.
OPTION_TAGS = {"b2": {"bins": 2}, "b5": {"bins": 5}, "b63": {"bins": 63}, "mid": {"sah": False},
               "c1e6": {"cost": 1e6}, "cfltmax": {"cost": float(np.finfo(np.float32).max)}}
OPTION_CASES = tuple(f"{c}-{t}" for c in ("n300", "n5000") for t in ("b5", "b63", "mid", "c1e6", "cfltmax")) + ("pow2-b2",)
# "lattice<n>-b<bins>": at least n unit boxes moved onto the planes the top level's root prices
# (lattice_line): one-wave requests and a large one, at bin counts whose step is inexact
OPTION_CASES += ("lattice100-b5", "lattice100-b63", "lattice300-b5", "lattice300-b63")
TOP_LATTICE_EXTENT = 24.3   # float32 E * (1 / bins) != E / bins for 3, 5, 7, 33, 63 bins; E + 0.5 < 32
FORCED_CASES = tuple(f"n{n}" for n in RECORD_SIZES) + ("collapsed300", "one_axis", "pow2") + OPTION_CASES


def case_opts(name):
    """The build options of a forced-path case (none but for OPTION_CASES)."""
    tag = name.partition("-")[2]
    return dict(OPTION_TAGS[tag]) if tag else {}


def forced_case(name):
    """(built scene, moved scene, trace rays too) of a forced-path case."""
    if name.startswith("lattice"):
        return lattice_line(int(name[7:].partition("-")[0]), case_opts(name)["bins"]) + (False,)
    if "-" in name:
        sc, moved, _ = forced_case(name.partition("-")[0])
        return sc, moved, False
    if name.startswith("n"):
        n = int(name[1:])
        sc = synthetic(n)
        return sc, with_transforms(sc, similarity_transforms(n, 100 + n)), False
    if name == "collapsed300":
        sc = synthetic(300)
        return sc, with_transforms(sc, [translate((1.0, 2.0, 3.0))] * 300), False
    if name == "one_axis":
        sc = synthetic(100)
        return sc, with_transforms(sc, [translate((0.0, 1.25 * i, 0.0)) for i in range(100)]), False
    if name == "pow2":
        sc = synthetic(64)
        return sc, with_transforms(sc, power_of_two_line(64)), True
    raise KeyError(name)


def trace(ds, rays, any_hit=False):
    """Closest (ISECT_DTYPE records) or any-hit (int32) answers of a device scene; synchronises
    and so raises on a device error status (traversal stack overflow)."""
    import torch
    from mcrt import types as T
    r = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    if any_hit:
        out = torch.full((len(rays),), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()   # the fill runs on torch's stream, the query on the context's own
        ds.trace_any(r.data_ptr(), len(rays), out.data_ptr())
    else:
        h0 = np.zeros(len(rays), T.ISECT_DTYPE)
        h0["shapeid"] = -7
        h0["primid"] = -7
        out = torch.from_numpy(h0.view(np.uint8).copy()).cuda()
        ds.trace_closest(r.data_ptr(), len(rays), out.data_ptr())
    ds.ctx.sync()
    res = out.cpu().numpy()
    return res if any_hit else res.view(T.ISECT_DTYPE)
