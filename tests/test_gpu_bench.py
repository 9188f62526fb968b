"""bench.py on one GPU at a small size: a plain run prints the headline line only, --dump-outputs
writes the last timed step's frame buffer (the same arrays from run to run), --full adds the other
legs to the line without changing the image."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, STEPS = 256, 200, 6
FULL_ONLY = ("rays_per_path", "shadow_hints", "queues_per_frame", "kernels", "cpu_baseline", "roofline", "bdpt")


def _bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--scene", "dragon_proxy", "--tris", "200000",
           "--width", str(W), "--height", str(H), "--steps", str(STEPS), "--warmup", "2", "--batch", "4",
           "--dump-outputs", str(out_dir), *extra]
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=280, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    arrays = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}
    return json.loads(lines[0]), arrays


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _bench(tmp_path_factory.mktemp("plain"))


def test_plain_line_is_the_headline(plain):
    line, arrays = plain
    assert line["unit"] == "Mpaths/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == STEPS and line["n_gpus"] == 1
    # value = paths of a step / ms_per_step (the line rounds ms_per_step to 1e-4 ms, value to 1e-3)
    assert abs(line["value"] - W * H / (line["ms_per_step"] * 1e-3) / 1e6) <= line["value"] * 1e-4 / line["ms_per_step"] + 2e-3
    assert not [k for k in FULL_ONLY if k in line], sorted(line)
    assert sorted(arrays) == ["image", "last_radiance"]
    for a in arrays.values():
        assert a.dtype == np.float32 and a.shape == (H, W, 4) and np.isfinite(a).all()
    assert arrays["image"][..., :3].max() > 0 and arrays["last_radiance"][..., :3].max() > 0


def test_dump_repeats_and_matches_saved_image(plain, tmp_path):
    img = str(tmp_path / "img.npy")
    _, again = _bench(tmp_path / "again", "--save-image", img)
    for k, a in plain[1].items():
        np.testing.assert_array_equal(again[k].view(np.uint32), a.view(np.uint32), err_msg=k)
    np.testing.assert_array_equal(np.load(img).view(np.uint32), again["image"].view(np.uint32))


def test_full_adds_the_other_legs_same_image(plain, tmp_path):
    line, arrays = _bench(tmp_path / "full", "--full", "--cpu-seconds", "0.5", "--no-reference-parity",
                          "--bdpt-steps", "4", "--bdpt-batch", "4")
    for k in ("rays_per_path", "shadow_hints", "queues_per_frame", "kernels", "cpu_baseline", "bdpt"):
        assert k in line, (k, sorted(line))
    assert line["steps"] == STEPS and line["metric"] == plain[0]["metric"]
    same = lambda c: {k: v for k, v in c.items() if k != "bvh_build_ms"}   # noqa: E731 (a measured time)
    assert same(line["config"]) == same(plain[0]["config"])
    for k, a in plain[1].items():
        np.testing.assert_array_equal(arrays[k].view(np.uint32), a.view(np.uint32), err_msg=k)
