"""The measurement entry points the bench's roofline uses (mcrt_probe.hip: mcrt_ctx_stream_copy,
mcrt_ctx_gather_chase, mcrt_ctx_gather_chase_compact): they run, give plausible rates, and order
as the memory hierarchy does (a dependent gather over an L2-resident array beats one over an
HBM-sized array)."""
import math
import time

import pytest

from helpers import refused
from mcrt import lib

pytestmark = pytest.mark.gpu
INVALID_ARG = 1


def test_stream_copy_rate(hip_ctx):
    g = hip_ctx.stream_copy_gbps(1 << 30, 2)
    assert 500.0 < g < 8000.0, g   # HBM3E: 8 TB/s peak


def test_gather_chase_hierarchy(hip_ctx):
    l2 = hip_ctx.gather_chase_gsteps(32768, 64, 2)
    hbm = hip_ctx.gather_chase_gsteps(20_000_000, 64, 2)
    assert l2 > hbm > 1.0, (l2, hbm)
    with pytest.raises(lib.MCRTError):
        hip_ctx.gather_chase_gsteps(8, 64, 1)   # fewer records than a wave's chains need


def test_gather_chase_compact_hierarchy(hip_ctx):
    """The chase over packed 32-B / 48-B records (bench.py's gather_ceiling): the same ordering at
    the walk's leaf share, and both ends of leaf_frac (every record 32 B, every record 48 B)."""
    l2 = hip_ctx.gather_chase_compact_gsteps(32768, 0.5, 64, 2)
    hbm = hip_ctx.gather_chase_compact_gsteps(20_000_000, 0.5, 64, 2)
    print(f"compact chase, G steps/s: 32768 records {l2:.2f}, 20 M records {hbm:.2f}")
    assert math.isfinite(l2) and math.isfinite(hbm)
    assert l2 > hbm > 1.0, (l2, hbm)
    for leaf_frac in (0.0, 1.0):
        g = hip_ctx.gather_chase_compact_gsteps(32768, leaf_frac, 64, 2)
        assert math.isfinite(g) and g > 0.0, (leaf_frac, g)


def test_gather_chase_compact_refusals(hip_ctx):
    bad = "bad gather-chase args"
    refused(lambda: hip_ctx.gather_chase_compact_gsteps(8, 0.5, 64, 1), INVALID_ARG, bad)
    refused(lambda: hip_ctx.gather_chase_compact_gsteps(32768, -0.1, 64, 1), INVALID_ARG, bad)
    refused(lambda: hip_ctx.gather_chase_compact_gsteps(32768, 1.5, 64, 1), INVALID_ARG, bad)
    refused(lambda: hip_ctx.gather_chase_compact_gsteps(32768, 0.5, 0, 1), INVALID_ARG, bad)
    assert hip_ctx.gather_chase_compact_gsteps(32768, 0.5, 64, 1) > 0.0   # a good call still works


def test_gather_chase_compact_refuses_links_past_31_bits(hip_ctx):
    """A record's link is (16-B unit offset << 1 | leaf) in 32 bits, so records * (2 + leaf_frac)
    must stay below 2^31 units.  0x3fffffff records of 3 units are 3.2e9: refused with the other
    argument checks, before anything is allocated -- the arrays would be 56 GB, the refusal takes
    no time.  (Before the check existed the call was accepted, allocated them, and chased links
    whose top bit was lost.)"""
    t0 = time.perf_counter()
    refused(lambda: hip_ctx.gather_chase_compact_gsteps(0x3fffffff, 1.0, 64, 2), INVALID_ARG, "bad gather-chase args")
    assert time.perf_counter() - t0 < 0.05   # no 56-GB allocation, no launch: argument checks only
