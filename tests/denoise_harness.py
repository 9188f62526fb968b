"""What the denoiser's tests share (test_gpu_denoise_guided.py, test_gpu_temporal.py,
test_gpu_temporal_motion.py, test_temporal_ref_cpu.py): bit views, camera pair A, the synthetic
image / albedo / history planes, a frame buffer with such planes installed, and the comparison of
the temporal planes with their numpy restatement.  Imports without a GPU.
"""
import numpy as np

from mcrt import types as T
from mcrt.camera import make_camera

F = np.float32
# the kernels are the same class as k_denoise (exponential weights, a normalised sum):
# test_gpu_postprocess.py's bound
RTOL, ATOL = 2e-5, 1e-7


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def ndiff(a, b):
    return int((bits(a) != bits(b)).sum())


def pair_a(W, H, offset=(0.0, 0.0, 0.0)):
    o = np.asarray(offset, np.float64)
    prev = make_camera(tuple(o + (0.0, 1.0, -4.0)), tuple(o + (0.0, 0.6, 0.0)), W, H, fovy=50.0)
    cur = make_camera(tuple(o + (0.6, 1.1, -3.8)), tuple(o + (0.1, 0.6, 0.0)), W, H, fovy=50.0)
    return prev, cur


def tm_rmse(a, truth, mask=None):
    """RMS error of the Reinhard-mapped colours, over the masked pixels."""
    a, truth = a[..., :3].astype(np.float64), truth[..., :3].astype(np.float64)
    d = (a / (1 + a) - truth / (1 + truth)) ** 2
    return float(np.sqrt(np.mean(d if mask is None else d[mask])))


def synth_planes(rng, sid, depth, prev_depth):
    """(albedo-depth, image, colour history, moments history) for guides with surface ids `sid` and
    depths `depth`, the history written at `prev_depth`: zero and sub-1e-3 albedo channels, a colour
    history with values over six decades on a fifth of the pixels, N in 1..40, some zero-variance
    moments.  The draws from `rng` are in this order."""
    H, W = sid.shape
    ad = np.empty((H, W, 4), F)
    ad[..., :3] = rng.uniform(0.05, 1.0, (H, W, 3))
    ad[..., 0][rng.random((H, W)) < 0.1] = 0.0
    ad[..., 1][rng.random((H, W)) < 0.1] = 5e-4
    ad[sid == 0, :3] = 0.0
    ad[..., 3] = depth
    img = (np.linspace(0.5, 2.0, W)[None, :, None] * 10.0 ** rng.uniform(-0.05, 0.05, (H, W, 4))).astype(F)
    img[..., 3] = rng.uniform(0, 1, (H, W))
    hc = rng.uniform(0.3, 2.5, (H, W, 4)).astype(F)
    wild = rng.random((H, W)) < 0.2
    hc[wild] = (10.0 ** rng.uniform(-3, 3, (int(wild.sum()), 4))).astype(F)
    mu1 = rng.uniform(0.2, 3.0, (H, W)).astype(F)
    mu2 = (mu1 * mu1 + rng.uniform(0.0, 0.5, (H, W)).astype(F)).astype(F)
    flat = rng.random((H, W)) < 0.15
    mu2[flat] = (mu1 * mu1)[flat]              # zero variance
    hm = np.stack([mu1, mu2, rng.integers(1, 41, (H, W)).astype(F), prev_depth], -1).astype(F)
    return ad, img, hc, hm


class Installed:
    """A frame buffer holding a synthetic image (unit weights) and guides -- case["img"], ["npl"],
    ["ad"] -- and whichever of these the case has: luminance moments (["mom"] of ["frames"] frames),
    motion planes (["motion"], ["pnorm"]; motion=False leaves them out) and history planes (["hist"]
    of the camera ["prev"]; history=False leaves them out)."""

    def __init__(self, ctx, case, history=True, motion=True):
        import torch
        from mcrt import lib
        H, W = case["img"].shape[:2]
        self.fb = lib.FrameBuffer(ctx, W, H)
        self.keep = [torch.ones(H * W, dtype=torch.float32, device="cuda")]

        def dev(a):
            self.keep.append(torch.from_numpy(np.ascontiguousarray(a, F).reshape(-1)).cuda())
            return self.keep[-1].data_ptr()

        img, npl, ad = dev(case["img"]), dev(case["npl"]), dev(case["ad"])
        mom = dev(case["mom"]) if case.get("mom") is not None else None
        mot = [dev(case["motion"]), dev(case["pnorm"])] if motion and "motion" in case else None
        hist = [dev(a) for a in case["hist"]] if history and "hist" in case else None
        torch.cuda.synchronize()
        self.fb.set_accumulation(img, self.keep[0].data_ptr())
        self.fb.set_guides(npl, ad)
        if mom is not None:
            self.fb.set_moments(mom, case["frames"])
        if mot:
            self.fb.set_motion(*mot)
        if hist:
            self.fb.set_temporal_history(*hist, case["prev"])
        ctx.sync()

    def run(self, **kw):
        self.fb.denoise_guided(**kw)
        return self.fb.read(3), self.fb.read_guides(T.GUIDE_FILTERED_VARIANCE)

    def planes(self):
        return [self.fb.read_temporal(w) for w in (T.TEMPORAL_COLOUR, T.TEMPORAL_MOMENTS, T.TEMPORAL_VARIANCE,
                                                   T.TEMPORAL_NORMAL_PLANE)]

    def close(self):
        self.fb.close()


def compare_planes(got, ref, what):
    """The temporal planes (colour, moments, variance, normal-plane) against the restatement's."""
    colour, mom, var, nrm = got
    rc, rm, rv, rn = ref
    print(f"{what}: bit-different values: colour {ndiff(colour, rc)}, moments {ndiff(mom, rm)}, "
          f"variance {ndiff(var, rv)}, normal-plane {ndiff(nrm, rn)} of {var.size} pixels")
    assert all(np.isfinite(a).all() for a in got)
    np.testing.assert_allclose(colour, rc, rtol=RTOL, atol=ATOL, err_msg="colour history")
    np.testing.assert_allclose(mom, rm, rtol=RTOL, atol=ATOL, err_msg="moments history, N, depth")
    np.testing.assert_array_equal(bits(nrm), bits(rn))
    bound = 2e-5 * rm[..., 1].astype(np.float64) + 1e-7
    err = np.abs(var.astype(np.float64) - rv.astype(np.float64))
    assert (err <= bound).all(), (err.max(), np.max(err / bound))
