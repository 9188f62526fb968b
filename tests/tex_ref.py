"""Plain numpy restatement of the reference's texture read and of the material functions built
on it, written from the reference's text: readTexture2Df_linear (textures.cl:70-125),
computeMipLevelByteOffset (:127-141), readTexture2Df_lod (:148-196), computeMipmapLOD (:198-202),
getUberMaterialProperties (materials.cl:76-91) and hasMaterialNonDeltaComponents (:161-179).
It imports nothing from the product; textures and materials are the numpy records a scene
uploads (mcrt.types.TEXDESC_DTYPE / MATERIAL_DTYPE) and the RGBA8 byte buffer.

What is evaluated how
  * The half-texel shift, the wrap step, the texel indices and the interpolation weights are
    DECISIONS (which texels, which side of a branch), so they are evaluated in float32, operation
    by operation, as the text reads.  `1.0f / width` is a correctly rounded division (numpy's).
  * The bilinear mix, the 1/255 scale and the mip mix are VALUES: evaluated in float64 from the
    float32 weights, so the reference value carries no rounding of its own (~1e-16 relative).

Tolerance of a float32 evaluation against these values (per channel, `Read.tol`)
  M = the largest of the four texels of the channel (an integer <= 255), ulp(x) = float32 ulp.
  A float32 evaluation with fused mixes, mix(a, b, t) = fma(b - a, t, a), makes these roundings:
    1. mix(v00, v10, tx) and mix(v01, v11, tx): b - a is exact (integers), one rounding each,
       <= 0.5 ulp(M); they enter the third mix with weights (1 - ty) and ty, together <= 0.5 ulp(M);
    2. the third mix: m1 - m0 is rounded (<= 0.5 ulp(M), weight ty <= 1) and the fma rounds once
       more (<= 0.5 ulp(M));                                          so far <= 1.5 ulp(M)
    3. the scale by the constant 1.0f / 255.0f: 1.5 ulp(M) / 255 <= 1.5 * 256 / 255 ulp(M / 255)
       (ulp(M / 255) >= ulp(M) / 256), the constant's own rounding (relative <= 2^-24, i.e.
       <= 1 ulp(M / 255)) and the product's rounding (<= 0.5 ulp(M / 255)).
  Sum: 1.5 * 256 / 255 + 1 + 0.5 = 3.006 -> K_FUSED = 3.01 ulp(M / 255).
  An evaluation with unfused mixes, a + (b - a) * t (the C oracle, built without contraction),
  rounds twice per mix: 1 ulp(M) for the first two together, 1.5 ulp(M) in the third, 2.5 ulp(M)
  in all -> 2.5 * 256 / 255 + 1.5 = 4.01 -> K_UNFUSED = 4.02 ulp(M / 255).
  (The issue's estimate of "under 2 ulp" left out the rounding of m1 - m0 and counted the
  constant's error as half an ulp; the recount above is what the tests use.)

  Contraction of the weight.  OpenCL C leaves FP_CONTRACT on, so a compiler may evaluate
  `uv.x * w - floor(uv.x * w)` with one rounding (fma(uv.x, w, -floor(uv.x * w))) instead of two.
  Both are evaluations of the text and they can differ by up to half an ulp of uv.x * w, which
  moves a value by |dvalue/dt| times that.  `Read.tol` therefore adds, per sample and exactly,
  |dvalue/dtx| * |tx_fused - tx| + |dvalue/dty| * |ty_fused - ty| (zero wherever both agree,
  which is every power-of-two size).  The value itself uses the weights as the text reads.

  The mip mix (readTexture2Df_lod): t = lod - floor(lod) is exact in float32; mix(v0, v1, t) adds
  one rounding of v1 - v0 and one of the fma, each <= 0.5 ulp of the larger level's M / 255, to
  (1 - t) tol0 + t tol1.
"""
import numpy as np

f32 = np.float32
K_FUSED = 3.01
K_UNFUSED = 4.02
BLACK_EPS = f32(0.000001)   # BLACK_COLOR_COMPONENT_EPSILON (bxdfs.cl:61)
SLOTS = ("uber_normalMapId", "uber_diffuseTexId", "uber_glossyTexId", "uber_specReflectionTexId",
         "uber_transmissionTexId", "uber_opacityTexId", "uber_roughnessTexId", "uber_iorTexId")


def ulp32(x):
    """float32 ulp at magnitude x (float64 in, float64 out); the smallest normal's ulp below it."""
    x = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(x)) - 23)


class Read:
    """Result of read_linear for N uvs: value (N, 4) float64, tol (N, 4) float64 (see the module
    docstring; k = K_FUSED or K_UNFUSED), idx (N, 4) = x0, y0, x1, y1 (-1 where the border colour
    was returned), border (N,), texels (N, 4 corners, 4 channels) uint8 and `branch`: per axis
    ('x', 'y') boolean masks below / inside / above (the shifted coordinate against [0, 1], what
    each wrap mode branches on), around (x0 == w - 1 wrapped to x1 == 0) and one (the wrapped
    coordinate times the size reached the size itself, so `% size` took texel 0)."""

    def __init__(self, n):
        self.value = np.zeros((n, 4))
        self.tol_ulps = np.zeros((n, 4))      # ulp(M / 255) per channel
        self.tol_contract = np.zeros((n, 4))  # the contraction term
        self.idx = np.full((n, 4), -1, np.int64)
        self.border = np.zeros(n, bool)
        self.texels = np.zeros((n, 4, 4), np.uint8)
        self.branch = {}

    def tol(self, k=K_FUSED):
        return k * self.tol_ulps + self.tol_contract


def _wrap_axis(u, wrap):
    """The wrap step of one axis in float32; returns (wrapped, outside) -- outside is what
    TEX_WRAP_CLAMP_TO_BORDER tests."""
    outside = (u > f32(1.0)) | (u < f32(0.0))
    if wrap == 0:      # TEX_WRAP_REPEAT
        return (u - np.floor(u)).astype(f32), outside
    if wrap == 1:      # TEX_WRAP_MIRRORED_REPEAT
        m = (f32(1.0) - (u - np.floor(u)).astype(f32)).astype(f32)
        return np.where(outside, m, u).astype(f32), outside
    if wrap == 2:      # TEX_WRAP_CLAMP_TO_EDGE: clamp = fmin(fmax(x, 0), 1)
        return np.minimum(np.maximum(u, f32(0.0)), f32(1.0)).astype(f32), outside
    return u, outside  # TEX_WRAP_CLAMP_TO_BORDER (the early return is the caller's)


def _c_rem(a, n):
    """C's a % n for integers (the sign of the dividend)."""
    return np.fmod(a, n)


def read_linear(width, height, wrap, mem_offset, tex_data, uv):
    """readTexture2Df_linear (textures.cl:70-125) of N float32 uvs on one texture level."""
    uv = np.asarray(uv, f32).reshape(-1, 2)
    n = len(uv)
    w, h = int(width), int(height)
    r = Read(n)
    with np.errstate(invalid="ignore", over="ignore"):
        # uv.x -= 1.0f / tex->width * 0.5f
        u = (uv[:, 0] - (f32(1.0) / f32(w)) * f32(0.5)).astype(f32)
        v = (uv[:, 1] - (f32(1.0) / f32(h)) * f32(0.5)).astype(f32)
        for name, c in (("x", u), ("y", v)):
            r.branch[name] = {"below": c < f32(0.0), "above": c > f32(1.0)}
            r.branch[name]["inside"] = ~r.branch[name]["below"] & ~r.branch[name]["above"]
        u, out_u = _wrap_axis(u, wrap)
        v, out_v = _wrap_axis(v, wrap)
        if wrap == 3:
            r.border = out_u | out_v
        live = ~r.border
        sx, sy = (u * f32(w)).astype(f32), (v * f32(h)).astype(f32)
        fx, fy = np.floor(sx), np.floor(sy)
        ix, iy = fx.astype(np.int64), fy.astype(np.int64)
        x0, y0 = _c_rem(ix, w), _c_rem(iy, h)
        x1, y1 = _c_rem(x0 + 1, w), _c_rem(y0 + 1, h)
        x0, x1 = np.clip(x0, 0, w - 1), np.clip(x1, 0, w - 1)
        y0, y1 = np.clip(y0, 0, h - 1), np.clip(y1, 0, h - 1)
        tx, ty = (sx - fx).astype(f32), (sy - fy).astype(f32)
        # the same weights with the multiply-subtract contracted (u * w is exact in float64)
        txf = (u.astype(np.float64) * w - fx.astype(np.float64)).astype(f32)
        tyf = (v.astype(np.float64) * h - fy.astype(np.float64)).astype(f32)
    r.branch["x"]["around"] = live & (w > 1) & (x0 == w - 1) & (x1 == 0)
    r.branch["y"]["around"] = live & (h > 1) & (y0 == h - 1) & (y1 == 0)
    r.branch["x"]["one"] = live & (ix == w)
    r.branch["y"]["one"] = live & (iy == h)
    r.idx[live] = np.stack([x0, y0, x1, y1], -1)[live]
    texd = np.asarray(tex_data, np.uint8)[int(mem_offset): int(mem_offset) + 4 * w * h].reshape(h, w, 4)
    c00, c10, c01, c11 = texd[y0, x0], texd[y0, x1], texd[y1, x0], texd[y1, x1]
    r.texels = np.stack([c00, c10, c01, c11], 1)
    r.texels[r.border] = 0
    v00, v10, v01, v11 = (c.astype(np.float64) for c in (c00, c10, c01, c11))
    TX, TY = tx.astype(np.float64)[:, None], ty.astype(np.float64)[:, None]
    m0 = v00 + (v10 - v00) * TX
    m1 = v01 + (v11 - v01) * TX
    r.value = (m0 + (m1 - m0) * TY) / 255.0
    M = r.texels.max(1).astype(np.float64)
    r.tol_ulps = np.where(M > 0, ulp32(M / 255.0), 0.0)
    gx = np.abs((v10 - v00) * (1.0 - TY) + (v11 - v01) * TY)
    gy = np.abs(m1 - m0)
    dtx = np.abs(txf.astype(np.float64) - tx.astype(np.float64))[:, None]
    dty = np.abs(tyf.astype(np.float64) - ty.astype(np.float64))[:, None]
    r.tol_contract = (gx * dtx + gy * dty) / 255.0
    r.value[r.border] = 0.0   # TEX_BORDER_COLOR (kernel_data.h:307)
    r.tol_ulps[r.border] = 0.0
    r.tol_contract[r.border] = 0.0
    return r


def desc_fields(tex):
    """(width, height, numMipLevels, wrap, memOffset) of a TextureDesc2D record."""
    return (int(tex["width"]), int(tex["height"]), int(tex["numMipLevels"]), int(tex["wrap"]), int(tex["memOffset"]))


def read_tex(tex, tex_data, uv):
    """readTexture2Df (textures.cl:204-209): the bilinear read of level 0."""
    w, h, _, wrap, off = desc_fields(tex)
    return read_linear(w, h, wrap, off, tex_data, uv)


def mip_level_size(width, height, level):
    """Size of a mip level as the loops of textures.cl:133-138 / :170-175 halve it (ushort)."""
    w, h = int(width), int(height)
    for _ in range(level):
        w, h = max(w // 2, 1), max(h // 2, 1)
    return w, h


def mip_level_byte_offset(width, height, level, texel_stride=4):
    """computeMipLevelByteOffset (textures.cl:127-141)."""
    w, h, off = int(width), int(height), 0
    for _ in range(level):
        off += w * h * texel_stride
        w, h = max(w // 2, 1), max(h // 2, 1)
    return off


def mipmap_lod(num_mip_levels, duvdx, duvdy):
    """computeMipmapLOD (textures.cl:198-202) in float32 (log2 as numpy rounds it)."""
    dx, dy = np.asarray(duvdx, f32).reshape(-1, 2), np.asarray(duvdy, f32).reshape(-1, 2)
    sw = np.maximum(np.maximum(np.abs(dx[:, 0]), np.abs(dx[:, 1])), np.maximum(np.abs(dy[:, 0]), np.abs(dy[:, 1])))
    return (f32(num_mip_levels) - f32(1.0) + np.log2(np.maximum(sw, f32(1e-8))).astype(f32)).astype(f32)


LOD_LINEAR, LOD_LAST, LOD_TRILINEAR = 0, 1, 2


def read_lod(tex, tex_data, uv, lod, k=K_FUSED):
    """readTexture2Df_lod (textures.cl:148-196) of N uvs with N float32 lods on one texture.
    Returns (value (N, 4) float64, tol (N, 4), path (N,) = LOD_LINEAR / LOD_LAST / LOD_TRILINEAR)."""
    uv = np.asarray(uv, f32).reshape(-1, 2)
    lod = np.asarray(lod, f32).reshape(-1)
    w, h, levels, wrap, off = desc_fields(tex)
    n = len(uv)
    value, tol = np.zeros((n, 4)), np.zeros((n, 4))
    path = np.full(n, LOD_TRILINEAR, np.int64)
    lin = (lod < f32(1e-8)) | (levels < 2)
    last = ~lin & (lod >= f32(levels - 1))
    path[lin], path[last] = LOD_LINEAR, LOD_LAST
    if lin.any():
        r = read_linear(w, h, wrap, off, tex_data, uv[lin])
        value[lin], tol[lin] = r.value, r.tol(k)
    if last.any():   # the reference reads the last level as 1 x 1
        r = read_linear(1, 1, wrap, off + mip_level_byte_offset(w, h, levels - 1), tex_data, uv[last])
        value[last], tol[last] = r.value, r.tol(k)
    tri = path == LOD_TRILINEAR
    lower = np.floor(lod).astype(np.int64)
    for lv in np.unique(lower[tri]):
        sel = tri & (lower == lv)
        w0, h0 = mip_level_size(w, h, lv)
        off0 = mip_level_byte_offset(w, h, lv)
        w1, h1 = max(w0 // 2, 1), max(h0 // 2, 1)
        r0 = read_linear(w0, h0, wrap, off + off0, tex_data, uv[sel])
        r1 = read_linear(w1, h1, wrap, off + off0 + w0 * h0 * 4, tex_data, uv[sel])
        t = (lod[sel] - f32(lv)).astype(np.float64)[:, None]
        value[sel] = r0.value + (r1.value - r0.value) * t
        tol[sel] = (1.0 - t) * r0.tol(k) + t * r1.tol(k) + 1.0 * np.maximum(r0.tol_ulps, r1.tol_ulps)
    return value, tol, path


def roughness_to_alpha(r):
    """roughnessToAlpha (bxdfs.cl:385-390) in float64."""
    x = np.log(np.maximum(np.asarray(r, np.float64), float(f32(1e-3))))
    c = [float(f32(v)) for v in (1.62142, 0.819955, 0.1734, 0.0171201, 0.000640711)]
    return c[0] + c[1] * x + c[2] * x * x + c[3] * x * x * x + c[4] * x * x * x * x


def roughness_to_alpha_tol(r, tol_r=0.0):
    """Bound of a float32 roughnessToAlpha against roughness_to_alpha.  With A = the sum of the
    five terms' magnitudes: a term is a product of at most five float32 factors (<= 4 roundings)
    into which log's error (<= 2 ulp) enters at most four times (<= 8 more half-ulps... counted as
    8 roundings), and each of the four additions rounds a partial sum <= A: (4 + 8 + 4) 2^-24 A =
    2^-20 A.  A roughness that is itself off by tol_r moves alpha by |dalpha/dr| tol_r."""
    r = np.maximum(np.asarray(r, np.float64), float(f32(1e-3)))
    x = np.log(r)
    c = [float(f32(v)) for v in (1.62142, 0.819955, 0.1734, 0.0171201, 0.000640711)]
    A = sum(abs(c[i]) * np.abs(x) ** i for i in range(5))
    d = np.abs(c[1] + 2 * c[2] * x + 3 * c[3] * x * x + 4 * c[4] * x * x * x) / r
    return 2.0 ** -20 * A + d * np.asarray(tol_r, np.float64)


def _slot(material, name, textures, tex_data, uv, reader):
    """readTexture2Df*_ifValid: (value (N, 4), tol (N, 4)) or None where the slot is unbound."""
    t = int(material[name])
    return None if t == -1 else reader(textures[t], tex_data, uv)


def uber_properties(material, textures, tex_data, uv, reader=None):
    """getUberMaterialProperties (materials.cl:76-91) of N uvs on one material record.
    reader(tex, tex_data, uv) -> (value, tol); default the level-0 bilinear read.  Returns a dict of
    float64 arrays Kd, Ks, Kr (N, 3), Kt (N, 4), opacity (N, 3), roughness (N, 2: alpha), eta (N,)
    and, under the same keys prefixed 'tol_', what the texture tolerance becomes in each."""
    if reader is None:
        def reader(tex, data, q):
            r = read_tex(tex, data, q)
            return r.value, r.tol()
    uv = np.asarray(uv, f32).reshape(-1, 2)
    n = len(uv)
    one, zero = np.ones((n, 4)), np.zeros((n, 4))

    def slot(name):
        s = _slot(material, name, textures, tex_data, uv, reader)
        return (one, zero, False) if s is None else (s[0], s[1], True)

    col = lambda k: np.asarray(material[k], np.float64)[:3]   # noqa: E731
    out = {}
    kdo, kdo_tol, _ = slot("uber_diffuseTexId")
    out["Kd"], out["tol_Kd"] = kdo[:, :3] * col("uber_kd"), kdo_tol[:, :3] * col("uber_kd")
    for key, name, const in (("Ks", "uber_glossyTexId", "uber_ks"), ("Kr", "uber_specReflectionTexId", "uber_kr")):
        v, t, _ = slot(name)
        out[key], out["tol_" + key] = v[:, :3] * col(const), t[:, :3] * col(const)
    v, t, _ = slot("uber_transmissionTexId")
    ktw = float(np.asarray(material["uber_kt"], np.float64)[3])
    out["Kt"] = np.concatenate([v[:, :3] * col("uber_kt"), np.full((n, 1), ktw)], 1)
    out["tol_Kt"] = np.concatenate([t[:, :3] * col("uber_kt"), np.zeros((n, 1))], 1)
    v, t, _ = slot("uber_opacityTexId")
    out["opacity"] = v[:, :3] * col("uber_opacity") * kdo[:, 3:4]
    out["tol_opacity"] = (t[:, :3] * kdo[:, 3:4] + v[:, :3] * kdo_tol[:, 3:4]) * col("uber_opacity")
    v, t, bound = slot("uber_roughnessTexId")
    rough = v[:, :2] if bound else np.broadcast_to(np.asarray(material["uber_roughness"], np.float64), (n, 2))
    out["roughness_in"] = np.array(rough)
    out["roughness"] = roughness_to_alpha(rough)
    out["tol_roughness"] = roughness_to_alpha_tol(rough, t[:, :2] if bound else 0.0)
    v, t, bound = slot("uber_iorTexId")
    out["eta"] = v[:, 0] if bound else np.full(n, float(material["uber_eta"]))
    out["tol_eta"] = t[:, 0] if bound else np.zeros(n)
    return out


def has_non_delta_components(material, textures, tex_data, uv, reader=None):
    """hasMaterialNonDeltaComponents (materials.cl:161-179): here a bound texture REPLACES the
    material's constant.  Returns (decision (N,) bool, margin (N,)): margin is the distance of the
    deciding component from BLACK_COLOR_COMPONENT_EPSILON in units of its tolerance (a decision
    with margin <= 1 could legitimately fall either way in float32)."""
    if reader is None:
        def reader(tex, data, q):
            r = read_tex(tex, data, q)
            return r.value, r.tol()
    uv = np.asarray(uv, f32).reshape(-1, 2)
    n = len(uv)
    if int(material["type"]) != 0:   # RT_UBER_MATERIAL
        return np.zeros(n, bool), np.full(n, np.inf)

    def slot(name, const):
        s = _slot(material, name, textures, tex_data, uv, reader)
        if s is None:
            return np.broadcast_to(np.asarray(material[const], np.float64)[:3], (n, 3)), np.zeros((n, 3))
        return s[0][:, :3], s[1][:, :3]

    Kd, tKd = slot("uber_diffuseTexId", "uber_kd")
    Ks, tKs = slot("uber_glossyTexId", "uber_ks")
    op, top = slot("uber_opacityTexId", "uber_opacity")
    comp = np.concatenate([Kd * op, Ks * op], 1)
    tol = np.concatenate([tKd * op + Kd * top, tKs * op + Ks * top], 1) + ulp32(comp)
    eps = float(BLACK_EPS)
    decision = (comp >= eps).any(1)   # !isBlack(kd) || !isBlack(ks); isBlack: every component < eps
    margin = (np.abs(comp - eps) / np.maximum(tol, 1e-300)).min(1)
    return decision, margin
