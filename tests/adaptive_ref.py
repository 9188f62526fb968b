"""numpy restatement of adaptive sampling (csrc/mcrt_adaptive.hip, include/mcrt_capi.h): the tile
error, the active rule and list, the accumulate over a list and the denoiser's per-pixel n.

A tile is 8x8 pixels; tile t is column-block t % tilesX of row-block t // tilesX and its lane l is
pixel (l & 7, l >> 3).  Planes are (H, W, C) float32 arrays as in atrous_ref; counts, errors and
flags are one value per tile in tile order.
"""
import numpy as np

import atrous_ref as ar

F = np.float32


def tile_grid(W, H):
    """(tilesX, tilesY)."""
    return (W + 7) // 8, (H + 7) // 8


def tile_lanes(plane, W, H):
    """(tiles, 64) values of an (H, W) plane in lane order, 0 outside the image, and the (tiles, 64)
    mask of the lanes inside it."""
    tx, ty = tile_grid(W, H)
    pad = np.zeros((ty * 8, tx * 8), plane.dtype)
    pad[:H, :W] = plane
    inside = np.zeros((ty * 8, tx * 8), bool)
    inside[:H, :W] = True

    def lanes(a):
        return a.reshape(ty, 8, tx, 8).transpose(0, 2, 1, 3).reshape(ty * tx, 64)

    return lanes(pad), lanes(inside)


def tile_mask(ids, W, H):
    """(H, W) mask of the pixels of the listed tiles."""
    tx, ty = tile_grid(W, H)
    on = np.zeros(tx * ty, bool)
    on[np.asarray(ids, np.int64)] = True
    return np.repeat(np.repeat(on.reshape(ty, tx), 8, 0), 8, 1)[:H, :W]


def tile_error(moments, counts, W, H, floor, dtype=F):
    """k_tile_error.  dtype float32: every line one float32 operation in the kernel's order, the two
    sums by the kernel's butterfly s = s + s[lane ^ d], d = 32 .. 1.  dtype float64: the same
    formulas in float64 with plain sums.  +inf where the tile has fewer than 2 samples."""
    T = dtype
    counts = np.asarray(counts)
    m1, inside = tile_lanes(np.asarray(moments, F)[..., 0].astype(T), W, H)
    m2, _ = tile_lanes(np.asarray(moments, F)[..., 1].astype(T), W, H)
    n = np.maximum(counts, 2).astype(T)[:, None]   # tiles below 2 samples are overwritten at the end
    mean = m1 / n
    v = np.maximum(T(0), m2 / n - mean * mean) / (n - T(1))
    mean = np.where(inside, mean, T(0)).astype(T)
    v = np.where(inside, v, T(0)).astype(T)
    if T is F:
        lane = np.arange(64)
        sv, sm = v, mean
        for d in (32, 16, 8, 4, 2, 1):
            sv = sv + sv[:, lane ^ d]
            sm = sm + sm[:, lane ^ d]
        assert sv.dtype == F and (sv == sv[:, :1]).all() and (sm == sm[:, :1]).all()   # every lane the same bits
        sv, sm = sv[:, 0], sm[:, 0]
    else:
        sv, sm = v.sum(1), mean.sum(1)
    c = inside.sum(1).astype(T)
    err = np.sqrt(sv / c) / (sm / c + T(F(floor)))
    return np.where(counts >= 2, err, T(np.inf)).astype(T)


def active(err, counts, error_threshold, min_samples, max_samples=0):
    """mcrt_adaptive_update's decision per tile."""
    counts = np.asarray(counts, np.int64)
    judged = np.asarray(err, F) > F(error_threshold)
    if max_samples > 0:
        judged = judged & (counts < max_samples)
    return np.where(counts < min_samples, True, judged)


def active_list(err, counts, **params):
    """The active tiles, ascending (k_tile_list)."""
    return np.flatnonzero(active(err, counts, **params)).astype(np.uint32)


def new_state(W, H):
    tx, ty = tile_grid(W, H)
    return dict(W=W, H=H, wsum=np.zeros((H, W, 4), F), wts=np.zeros((H, W), F), mom=np.zeros((H, W, 2), F),
                counts=np.zeros(tx * ty, np.uint32))


def step(state, frames, ids):
    """k_accumulate and k_moments over the listed tiles (box filter: weight 1), then the counts:
    sequential float32 sums in frame order; a tile's first sample overwrites.  `frames` are (H, W, 4)
    radiance planes; only their listed tiles are read.  Returns a new state."""
    W, H = state["W"], state["H"]
    s = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in state.items()}
    ids = np.asarray(ids, np.int64)
    if len(ids) == 0:
        return s
    listed = tile_mask(ids, W, H)
    n = np.repeat(np.repeat(s["counts"].reshape(tile_grid(W, H)[::-1]), 8, 0), 8, 1)[:H, :W]
    w = F(1)
    for k, fr in enumerate(frames):
        r = ar.cl_clamp(np.asarray(fr, F), 0, 1000)
        l = ar.luminance(r[..., :3])
        ll = l * l
        first = listed & (n + k == 0)
        later = listed & ~first
        s["wsum"][first] = (r * w)[first]
        s["wts"][first] = w
        s["wsum"][later] = (s["wsum"] + r * w)[later]   # fma(r, 1, s): one rounding, as the sum
        s["wts"][later] = (s["wts"] + w)[later]
        s["mom"][first] = np.stack([l, ll], -1)[first]
        s["mom"][later] = np.stack([s["mom"][..., 0] + l, s["mom"][..., 1] + ll], -1).astype(F)[later]
    s["counts"][ids] += np.uint32(len(frames))
    return s


def prepare_var(moments, counts, W, H):
    """k_atrous_prep's variance in adaptive mode: n per pixel from its tile's count, n < 2: 1."""
    n = np.repeat(np.repeat(np.asarray(counts).reshape(tile_grid(W, H)[::-1]), 8, 0), 8, 1)[:H, :W]
    m = np.asarray(moments, F)
    nf = np.maximum(n, 2).astype(F)
    mean = m[..., 0] / nf
    var = np.maximum(F(0), m[..., 1] / nf - mean * mean) / (nf - F(1))
    return np.where(n >= 2, var, F(1)).astype(F)


def gap_threshold(err):
    """The midpoint of the widest gap between consecutive sorted errors in the middle half of the
    ranks, that gap relative to its midpoint, and the tiles on each side."""
    e = np.sort(np.asarray(err, np.float64))
    lo, hi = len(e) // 4, len(e) - len(e) // 4   # ranks lo .. hi - 1; a gap between ranks i - 1 and i, lo <= i - 1, i < hi
    i = lo + 1 + int(np.argmax(e[lo + 1:hi] - e[lo:hi - 1]))
    thr = 0.5 * (e[i - 1] + e[i])
    return float(thr), float((e[i] - e[i - 1]) / thr), i, len(e) - i
