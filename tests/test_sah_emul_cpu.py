"""CPU check of the device SAH build's algorithm (mcrt_sahbuild.hip): tests/sah_emul runs the
same split arithmetic (mcrt_sah.h: tabulated _mm_rcp_ps, _mm_dp_ps order, 4-wide/1-wide bins),
the closed-form two-pointer partition and the median fallback top-down on the host, and compares
every record with the host build (mcrt_bvh.cpp = RadeonRays Bvh2).  The GPU kernels themselves
are compared with the host build in tests/test_gpu_sah_build.py."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "monte-carlo-raytracer_amd", "csrc")


@pytest.fixture(scope="module")
def emul():
    if not os.path.exists(os.path.join(CSRC, "build", "mcrt_bvh.o")):
        subprocess.run(["make", "-C", CSRC, "build/mcrt_bvh.o"], check=True, capture_output=True)
    subprocess.run(["make", "-C", os.path.join(HERE, "sah_emul")], check=True, capture_output=True)
    return os.path.join(HERE, "sah_emul", "sah_emul")


def run_emul(emul, n, seed, kind, t=None):
    """t: an option tuple (bins, cost, sah) for both the host build and the emulation (default: the
    reference's 64 bins, cost 10, SAH on; tests/test_build_opts_cpu.py runs the grid)."""
    args = [emul, str(n), str(seed), str(kind)]
    if t is not None:
        args += [str(t[0]), repr(float(t[1])), "1" if t[2] else "0"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mismatched floats=0" in r.stdout


@pytest.mark.parametrize("n,seed,kind", [(1, 1, 0), (2, 3, 0), (9, 2, 0), (1000, 7, 1), (5000, 9, 2),
                                         (20000, 1, 0), (20000, 1, 1), (20000, 1, 2), (200000, 5, 0)])
def test_device_algorithm_matches_host_build(emul, n, seed, kind):
    run_emul(emul, n, seed, kind)
