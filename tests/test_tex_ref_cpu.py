"""CPU tests of tests/tex_ref.py (the plain restatement of the reference's texture read and
material-slot functions) and of the texture-zoo scene it is used on.

  1. hand-known answers pin tex_ref before anything is compared with it;
  2. tex_ref against the oracle's readTex / getUberProps / hasMaterialNonDeltaComponents
     (oracle/mcrt_oracle.c through orc_read_tex / orc_uber_props): equal texel indices, values
     within the tolerance derived in tex_ref's docstring for unfused float32 mixes;
  3. the conditions the zoo must meet (tests/tex_zoo.py), from the oracle's primary hits;
  4. one oracle PT frame of the zoo: finite, and lit under every slot's quad.

A note on two of the hand-known answers: the reference subtracts half a texel BEFORE it wraps, so
its mirror and its clamp act on the shifted coordinate.  "Mirrored 1.25 equals 0.75" and "clamp at
1 reads texel 0" therefore hold for the shifted coordinate (u - 0.5 / w), which is how they are
stated below; at the literal inputs the two mirrored reads are one texel apart."""
import numpy as np
import pytest

import tex_ref
import tex_zoo as tz
from mcrt import scenes
from mcrt.camera import scene_camera
from oracle import pyoracle as po

f32 = np.float32


def tex_of(img, wrap):
    """(TextureDesc2D record, byte buffer) of one RGBA8 image through SceneBuilder.add_texture."""
    b = scenes.SceneBuilder("t")
    b.add_texture(img, wrap=wrap)
    sc = b.build()
    return sc.textures[0], sc.tex_data


IMG22 = np.array([[[10, 20, 30, 40], [50, 60, 70, 80]], [[90, 100, 110, 120], [130, 140, 150, 255]]], np.uint8)


@pytest.mark.parametrize("wrap", [0, 1, 2, 3])
def test_texel_centres_return_the_texels(wrap):
    tex, data = tex_of(IMG22, wrap)
    # the read blends texels x0 = floor(s * w) and x0 + 1 of the shifted coordinate s = uv - 0.5 / w
    # with weight frac(s * w): texel (x, y) is returned exactly at uv = ((x + 0.5) / w, (y + 0.5) / h),
    # i.e. s * w = x (all values here are exact in float32)
    for y in range(2):
        for x in range(2):
            r = tex_ref.read_tex(tex, data, [[x / 2 + 0.25, y / 2 + 0.25]])
            np.testing.assert_array_equal(r.value[0] * 255.0, IMG22[y, x].astype(np.float64))
            assert tuple(r.idx[0, :2]) == (x, y)


def test_border_returns_zeros_outside():
    tex, data = tex_of(IMG22, 3)
    uv = np.array([[-0.5, 0.5], [1.5, 0.5], [0.5, -0.5], [0.5, 1.5], [0.2, 0.5], [0.5, 0.2], [1.26, 0.5]], f32)
    r = tex_ref.read_tex(tex, data, uv)
    # 0.2 - 0.25 < 0 is outside too: the test is on the shifted coordinate
    assert r.border.tolist() == [True, True, True, True, True, True, True]
    assert not r.value.any() and (r.idx == -1).all()
    r = tex_ref.read_tex(tex, data, [[0.5, 0.5], [1.25, 1.25]])
    assert not r.border.any() and r.value.all()


def test_clamp_at_one_reads_texel_zero():
    tex, data = tex_of(IMG22, 2)
    # shifted coordinate >= 1 clamps to 1.0: floor(1.0 * 2) % 2 = 0, weight 0 -> texel 0 exactly
    for u in (1.25, 2.0, 1e6):
        r = tex_ref.read_tex(tex, data, [[u, 0.25]])
        assert r.idx[0, 0] == 0 and r.branch["x"]["one"][0]
        np.testing.assert_array_equal(r.value[0] * 255.0, IMG22[0, 0].astype(np.float64))
    # the literal u = 1: shifted 0.75 -> texel 1 blended half and half with texel 0 (x1 wraps)
    r = tex_ref.read_tex(tex, data, [[1.0, 0.25]])
    assert tuple(r.idx[0]) == (1, 0, 0, 1) and r.branch["x"]["around"][0]
    np.testing.assert_array_equal(r.value[0] * 255.0, (IMG22[0, 0].astype(np.float64) + IMG22[0, 1]) / 2)


def test_mirror():
    img = np.random.default_rng(3).integers(0, 256, (4, 8, 4), dtype=np.uint8)
    tex, data = tex_of(img, 1)
    h = 0.5 / 8   # shifted 1.25 mirrors to 1 - 0.25 = 0.75
    a = tex_ref.read_tex(tex, data, [[1.25 + h, 0.5]])
    b = tex_ref.read_tex(tex, data, [[0.75 + h, 0.5]])
    np.testing.assert_array_equal(a.value, b.value)
    np.testing.assert_array_equal(a.idx, b.idx)
    assert a.branch["x"]["above"][0] and b.branch["x"]["inside"][0]
    # below zero: shifted -0.25 -> 1 - 0.75 = 0.25
    a = tex_ref.read_tex(tex, data, [[-0.25 + h, 0.5]])
    b = tex_ref.read_tex(tex, data, [[0.25 + h, 0.5]])
    np.testing.assert_array_equal(a.value, b.value)
    # the literal inputs 1.25 and 0.75 sample one texel apart
    a = tex_ref.read_tex(tex, data, [[1.25, 0.5]])
    b = tex_ref.read_tex(tex, data, [[0.75, 0.5]])
    assert a.idx[0, 0] == b.idx[0, 0] + 1


@pytest.mark.parametrize("wrap", [0, 1, 2])
def test_one_by_one_returns_its_texel(wrap):
    tex, data = tex_of(np.array([[[7, 99, 201, 255]]], np.uint8), wrap)
    uv = np.array([[0.0, 0.0], [0.3, 0.9], [-5.5, 7.25], [1.0, 1.0], [1e6, -1e6], [-2.0 ** -30, 0.5]], f32)
    r = tex_ref.read_tex(tex, data, uv)
    np.testing.assert_allclose(r.value * 255.0, np.tile([7.0, 99.0, 201.0, 255.0], (len(uv), 1)), rtol=1e-15)
    assert (r.idx == 0).all()


def test_repeat_just_below_zero_wraps_to_texel_zero():
    """A shifted coordinate a few ulp below 0: u - floor(u) rounds to exactly 1.0, u * w reaches w
    and `% w` takes texel 0 with weight 0 (the texel a coordinate of +0 reads)."""
    img = np.random.default_rng(4).integers(0, 256, (3, 5, 4), dtype=np.uint8)
    tex, data = tex_of(img, 0)
    half = f32(0.5) / f32(5)
    below = np.nextafter(half, f32(0))
    r = tex_ref.read_tex(tex, data, [[below, 0.5], [half, 0.5]])
    assert r.branch["x"]["one"].tolist() == [True, False] and r.branch["x"]["below"].tolist() == [True, False]
    np.testing.assert_array_equal(r.idx[0], r.idx[1])
    np.testing.assert_array_equal(r.value[0], r.value[1])


def test_mip_offsets_and_lod():
    assert tex_ref.mip_level_byte_offset(7, 64, 0) == 0
    assert tex_ref.mip_level_byte_offset(7, 64, 1) == 7 * 64 * 4
    assert tex_ref.mip_level_byte_offset(7, 64, 3) == (7 * 64 + 3 * 32 + 1 * 16) * 4
    assert tex_ref.mip_level_size(100, 60, 6) == (1, 1) and tex_ref.mip_level_size(5, 3, 1) == (2, 1)
    # the packed chain of SceneBuilder.add_texture(mips=True) has exactly these offsets
    sc = tz.zoo()
    ends = [int(t["memOffset"]) for t in sc.textures[1:]] + [sc.tex_data.nbytes]
    for t, end in zip(sc.textures, ends):
        w, h, levels, _, off = tex_ref.desc_fields(t)
        assert tex_ref.mip_level_size(w, h, levels - 1) == (1, 1) or levels == 1
        assert off + tex_ref.mip_level_byte_offset(w, h, levels) == end   # the chain fills its chunk exactly
    lod = tex_ref.mipmap_lod(7, [[0.25, 0.0]], [[0.0, -0.125]])
    assert lod[0] == f32(4.0)
    assert tex_ref.mipmap_lod(3, [[0.0, 0.0]], [[0.0, 0.0]])[0] < 0   # log2(1e-8) floor
    # the three paths of the mip-mapped read
    tex = sc.textures[sc.zoo["textures"][(64, 64, True)]]
    uv = np.array([[0.3, 0.6]] * 4, f32)
    v, tol, path = tex_ref.read_lod(tex, sc.tex_data, uv, np.array([0.0, 2.5, 6.0, 9.0], f32))
    assert path.tolist() == [tex_ref.LOD_LINEAR, tex_ref.LOD_TRILINEAR, tex_ref.LOD_LAST, tex_ref.LOD_LAST]
    np.testing.assert_array_equal(v[0], tex_ref.read_tex(tex, sc.tex_data, uv[:1]).value[0])
    last = sc.tex_data[int(tex["memOffset"]) + tex_ref.mip_level_byte_offset(64, 64, 6):][:4]
    np.testing.assert_allclose(v[2] * 255.0, last.astype(np.float64), rtol=1e-15)
    np.testing.assert_array_equal(v[2], v[3])
    lo = tex_ref.read_linear(16, 16, int(tex["wrap"]), int(tex["memOffset"]) + tex_ref.mip_level_byte_offset(64, 64, 2),
                             sc.tex_data, uv[:1]).value[0]
    hi = tex_ref.read_linear(8, 8, int(tex["wrap"]), int(tex["memOffset"]) + tex_ref.mip_level_byte_offset(64, 64, 3),
                             sc.tex_data, uv[:1]).value[0]
    np.testing.assert_allclose(v[1], 0.5 * (lo + hi), rtol=1e-15)


# ---------------------------------------------------------------------------
# tex_ref against the oracle
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_zoo():
    sc = tz.zoo()
    o = po.OracleScene(sc)
    o.build()
    return sc, o


def uv_grid(w, h, rng):
    """Special coordinates (every pair of them) and random ones for a w x h texture."""
    def around(c):
        c = f32(c)
        lo1, hi1 = np.nextafter(c, f32(-np.inf)), np.nextafter(c, f32(np.inf))
        return [np.nextafter(lo1, f32(-np.inf)), lo1, c, hi1, np.nextafter(hi1, f32(np.inf))]
    one_m = np.nextafter(f32(1.0), f32(0.0))
    sp = [f32(0.0), f32(-0.0), f32(-2.0 ** -30), f32(2.0 ** -30), f32(1e6), f32(-1e6), f32(0.75), f32(1.25), f32(-0.25),
          f32(0.03), f32(0.97)]
    # what the zoo's edge strips aim at, and a few ulp either side
    for c in (1.0, -1.0, 2.0, one_m, f32(0.5) / f32(w), f32(0.5) / f32(h), f32(1.0) + f32(0.5) / f32(w), f32(1.0) / f32(w)):
        sp += around(c)
    sp = np.unique(np.array(sp, f32))
    sp = np.concatenate([sp, np.array([-0.0], f32)])   # np.unique folds -0 into 0
    g = np.stack(np.meshgrid(sp, sp, indexing="ij"), -1).reshape(-1, 2)
    r = rng.uniform(-2.0, 3.0, size=(1500, 2)).astype(f32)
    return np.concatenate([g, r]).astype(f32)


def test_read_matches_oracle(oracle_zoo):
    sc, o = oracle_zoo
    rng = np.random.default_rng(11)
    worst = 0.0
    for t, tex in enumerate(sc.textures):
        w, h, _, wrap, _ = tex_ref.desc_fields(tex)
        uv = uv_grid(w, h, rng)
        val, idx = o.read_tex(t, uv)
        r = tex_ref.read_tex(tex, sc.tex_data, uv)
        np.testing.assert_array_equal(idx, r.idx, err_msg=f"texture {t} ({w}x{h}, wrap {wrap}): texel indices")
        err = np.abs(val.astype(np.float64) - r.value)
        tol = tex_ref.K_UNFUSED * r.tol_ulps   # the oracle evaluates the weights as the text reads: no contraction term
        assert (err <= tol).all(), (t, w, h, wrap, uv[(err > tol).any(1)][:4], err.max())
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.where(r.tol_ulps > 0, err / r.tol_ulps, 0.0))))
        assert wrap != 3 or (r.border.any() and not r.border.all())
    print(f"largest error: {worst:.2f} ulp(M / 255) of {tex_ref.K_UNFUSED} allowed")


def test_uber_properties_match_oracle(oracle_zoo):
    sc, o = oracle_zoo
    rng = np.random.default_rng(12)
    uv = np.concatenate([uv_grid(64, 64, rng)[::7], rng.uniform(-0.5, 1.5, size=(500, 2)).astype(f32)])

    def reader(tex, data, q):
        r = tex_ref.read_tex(tex, data, q)
        return r.value, tex_ref.K_UNFUSED * r.tol_ulps

    decided = flipped = 0
    for m, mat in enumerate(sc.materials):
        got = o.uber_props(m, uv)
        want = tex_ref.uber_properties(mat, sc.textures, sc.tex_data, uv, reader)
        for key in ("Kd", "Ks", "Kr", "Kt", "opacity", "eta"):
            g, wv = got[key].astype(np.float64), want[key]
            # the texture tolerance carried through, plus one float32 rounding per product
            tol = want["tol_" + key] + 2.0 * tex_ref.ulp32(wv)
            assert (np.abs(g - wv) <= tol).all(), (m, key, float(np.abs(g - wv).max()))
        g, wv = got["roughness"].astype(np.float64), want["roughness"]
        assert (np.abs(g - wv) <= want["tol_roughness"]).all(), (m, "roughness", float(np.abs(g - wv).max()))
        nd, margin = tex_ref.has_non_delta_components(mat, sc.textures, sc.tex_data, uv, reader)
        sure = margin > 1.0
        np.testing.assert_array_equal(got["nonDelta"][sure] != 0, nd[sure], err_msg=f"material {m}: non-delta decision")
        decided += int(sure.sum())
        flipped += int((nd[sure] != nd[sure][0]).any()) if sure.any() else 0
    assert decided > 0.99 * len(uv) * len(sc.materials)
    # the decision is not constant: materials whose textures reach black flip it over the grid
    assert flipped >= 2
    # the zoo's point: shading and decision disagree unless both are right
    kd0 = sc.materials[sc.zoo["materials"]["diffuse_kd0"]]
    inside = np.array([[0.5, 0.9]], f32)
    assert not tex_ref.uber_properties(kd0, sc.textures, sc.tex_data, inside)["Kd"].any()
    assert tex_ref.has_non_delta_components(kd0, sc.textures, sc.tex_data, inside)[0][0]
    gl = sc.materials[sc.zoo["materials"]["glossy"]]
    black, lit = np.array([[0.2, 0.5]], f32), np.array([[0.8, 0.5]], f32)
    assert not tex_ref.has_non_delta_components(gl, sc.textures, sc.tex_data, black)[0][0]
    assert tex_ref.has_non_delta_components(gl, sc.textures, sc.tex_data, lit)[0][0]


# ---------------------------------------------------------------------------
# the zoo
# ---------------------------------------------------------------------------
def oracle_primary_hits(sc, o, W, H):
    cam = scene_camera("tex_zoo", W, H)
    log = o.path_log(W, H, 1)
    try:
        o.render(cam, frame=0, max_depth=1)
        log = log.copy()
    finally:
        o.path_log(None)
    shape, prim = log[:, 0, 0].view(np.int32), log[:, 0, 1].view(np.int32)
    uv = np.zeros((W * H, 2), f32)
    hit = shape >= 0
    uv[hit] = tz.hit_uv(sc, shape[hit], prim[hit], log[hit, 0, 2], log[hit, 0, 3])
    return shape.reshape(H, W), uv.reshape(H, W, 2)


def test_zoo_content():
    sc = tz.zoo()
    assert sc.num_triangles < 200 and len(sc.lights) == 2
    sizes = {(int(t["width"]), int(t["height"])) for t in sc.textures}
    assert sizes == set(scenes.ZOO_SIZES)
    pot = lambda n: n & (n - 1) == 0   # noqa: E731
    for mips in (False, True):
        for wrap in range(4):
            kinds = {pot(w) and pot(h) for (w, h, m), t in sc.zoo["textures"].items()
                     if m == mips and int(sc.textures[t]["wrap"]) == wrap}
            assert kinds == {True, False}, (mips, wrap)
    for (w, h, m), t in sc.zoo["textures"].items():
        assert (int(sc.textures[t]["numMipLevels"]) > 1) == (m and (w, h) != (1, 1))
    # one material per slot binding exactly that slot, and one binding all eight to different textures
    names = dict(zip(("normal", "diffuse", "glossy", "specReflection", "transmission", "opacity", "roughness", "ior"),
                     tex_ref.SLOTS))
    for name, slot in names.items():
        mat = sc.materials[sc.zoo["materials"][name]]
        assert [s for s in tex_ref.SLOTS if mat[s] != -1] == [slot], name
    allm = sc.materials[sc.zoo["materials"]["all"]]
    assert len({int(allm[s]) for s in tex_ref.SLOTS}) == 8 and -1 not in {int(allm[s]) for s in tex_ref.SLOTS}
    ior = [int(m["uber_iorTexId"]) for m in sc.materials if m["uber_iorTexId"] != -1]
    for t in ior:   # eta stays in [0.5, 1] on every level
        w, h, levels, wrap, off = tex_ref.desc_fields(sc.textures[t])
        assert wrap != 3
        n = tex_ref.mip_level_byte_offset(w, h, levels) // 4
        assert sc.tex_data[off: off + 4 * n].reshape(-1, 4)[:, 0].min() >= 128
    rough = sc.tex_data[int(sc.textures[int(allm["uber_roughnessTexId"])]["memOffset"]):][:400].reshape(-1, 4)
    assert (rough[:, 0] != rough[:, 1]).mean() > 0.9
    assert {float(m["uber_kt"][3]) for m in sc.materials if m["uber_transmissionTexId"] != -1} == {0.0, 1.0}


def test_zoo_conditions(oracle_zoo):
    sc, o = oracle_zoo
    shape, uv = oracle_primary_hits(sc, o, tz.W, tz.H)
    cov = tz.coverage(sc, shape, uv)
    print(tz.format_coverage(cov))
    assert not tz.check_coverage(sc, cov), tz.check_coverage(sc, cov)
    # the edge strips put every pixel on the constant they aim at, or within a few ulp of it
    for sid, kind in sc.zoo["shapes"].items():
        if kind[0] != "strip":
            continue
        _, wr, axis, c, _ = kind
        got = uv[shape == sid][:, axis]
        assert len(got) >= 24 and (np.abs(got - f32(c)) <= 4 * np.spacing(max(abs(f32(c)), f32(2.0 ** -20)))).all(), kind


def test_oracle_frame_of_the_zoo(oracle_zoo):
    sc, o = oracle_zoo
    W, H = 48, 32
    rad, _ = o.render(scene_camera("tex_zoo", W, H), frame=0, max_depth=3)
    assert np.isfinite(rad).all()
    shape, _ = oracle_primary_hits(sc, o, W, H)
    for sid, kind in sc.zoo["shapes"].items():
        if kind[0] == "slot":
            px = rad[shape == sid][:, :3]
            assert len(px) >= 24 and (px.sum(-1) > 0).mean() > 0.25, (kind, len(px), float((px.sum(-1) > 0).mean()))
