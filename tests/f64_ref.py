"""A second opinion on the scalar physics: the reference's shading (textured or not), normal mapping, image sampler, procedural and image sky, light
sampling, path loop and tonemap restated in numpy float64, vectorised over samples, from the reference's formulas
(kernels/src/{lib,bsdf,util,skybox,light_pick,rng,intersection}.rs, shared_structs/src/image_polyfill.rs, src/resources/render.wgsl) and from nothing else.  It shares no code with the C++ CPU restatement the suite calls its checker, with the device's math header or with the package's native
libraries; the transcendental functions are numpy's.  That checker and, through probe scenes, the production kernels are held to this file within a
tolerance (tests/test_f64_reference.py, tests/test_gpu_f64_probes.py).

Numbers.  float64 throughout, with one exception that says so (ggx_half_angle).  A constant the reference writes as an f32 literal (EPS, pi, the sky
coefficients ...) has the literal's float32 value; the random numbers are the reference's exactly (integer product -> float32 -> * 2^-32).

Margins.  Every discrete decision of a path also yields the distance by which it was taken, in the units of the compared quantity (random numbers,
weights and barycentric coordinates as they are; distances along a ray relative to max(1, t); determinants relative to |edge1| |edge2|).  A sample
whose smallest margin is below a threshold may legitimately take the other branch in float32; callers flag it and do not compare it.

Textures.  The uv wrap of a textured hit is a decision like any other (margin: the distance of each uv component to its nearest integer).  The
bilinear sampler is continuous across texel boundaries and across the modulo seam, so those carry no margin.  The image sky takes its row from an
arcsine, which is ill-conditioned at the poles (a float32 y in error by 1e-7 moves v by 1e-7 / sqrt(1 - y^2)); trace reports the largest |y| of a
sample's sky lookup and callers flag a sample too close to a pole.

Small cosines.  float32 keeps the cosine of two unit vectors to about 1e-7 absolutely.  The specular pdf divides by halfway . view, which a near-mirror
bounce at grazing incidence makes small: there the reference's expression is ill-conditioned (1e-7 / cosine^2 relatively).  pbr_sample and trace report
that cosine (the smallest over a path's specular bounces); callers flag a sample below a threshold of their own like one that decides by a hair.
"""
import numpy as np


def f32(x):
    return float(np.float32(x))


EPS = f32(0.001)                         # util.rs:5
PI = f32(np.pi)                          # core::f32::consts::PI
FLT_MAX = float(np.finfo(np.float32).max)
T_MIN = f32(0.001)                       # intersection.rs: t > 0.001
T_FAR = 1000000.0                        # TraceResult::default().t
DET_MIN = f32(1e-6)
F0_DIELECTRIC = f32(np.float32(f32(0.5) / f32(2.5)) * np.float32(f32(0.5) / f32(2.5)))     # ((1.5 - 1) / (1.5 + 1))^2, evaluated in f32 as a const
ARBITRARY = np.array([f32(0.1), f32(0.5), f32(0.9)])
GGX_UP_SWITCH = f32(0.999)
INF = np.inf

LDS_PRIMES = np.array([
    0x6a09e667, 0xbb67ae84, 0x3c6ef372, 0xa54ff539, 0x510e527f, 0x9b05688a, 0x1f83d9ab, 0x5be0cd18, 0xcbbb9d5c, 0x629a2929, 0x91590159, 0x452fecd8,
    0x67332667, 0x8eb44a86, 0xdb0c2e0b, 0x47b5481d, 0xae5f9155, 0xcf6c85d1, 0x2f73477d, 0x6d1826ca, 0x8b43d455, 0xe360b595, 0x1c456002, 0x6f196330,
    0xd94ebeaf, 0x9cc4a611, 0x261dc1f2, 0x5815a7bd, 0x70b7ed67, 0xa1513c68, 0x44f93634, 0x720dcdfc], np.uint64)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# small vector helpers: arrays of shape (..., 3)
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def dot(a, b):
    return (a * b).sum(-1)


def col(s):
    return np.asarray(s)[..., None]


def normalize(a):
    return a / col(np.sqrt(dot(a, a)))


def cross(a, b):
    return np.cross(a, b)


def vec(x, y, z):
    return np.stack(np.broadcast_arrays(x, y, z), -1)


def finite32(v):
    """Vec3::is_finite of the float32 the reference holds: a float64 beyond the float32 range is an infinity there"""
    return (np.isfinite(v) & (np.abs(v) <= FLT_MAX)).all(-1)


def mask_nan(v):
    return np.where(col(finite32(v)), v, 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# rng.rs: integer exact
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def lds(n, dimension, offset):
    """(u32 product, value): PRIMES[dimension] *wrapping (n +wrapping offset) -> f32 (round to nearest even) * 2^-32.  The reference's table has 32
    entries; an index past it is an error there, and the configurations used never reach it (Rng asserts that)."""
    n, dimension, offset = (np.asarray(a, np.uint64) for a in (n, dimension, offset))
    product = (LDS_PRIMES[dimension] * ((n + offset) & np.uint64(0xffffffff))) & np.uint64(0xffffffff)
    return product.astype(np.uint32), (product.astype(np.uint32).astype(np.float32) * np.float32(1.0 / 4294967296.0)).astype(np.float64)


class Rng:
    """RngState of many samples at once; a draw advances only the samples of its mask"""

    def __init__(self, n, offset):
        self.n, self.offset = np.asarray(n, np.uint64), np.asarray(offset, np.uint64)
        self.dimension = np.zeros(self.n.shape, np.int64)

    def r1(self, mask):
        self.dimension = np.where(mask, self.dimension + 1, self.dimension)
        assert self.dimension.max() <= 31, "the path needs more dimensions than the reference's table holds"
        return lds(self.n, self.dimension, self.offset)[1]

    def r2(self, mask):
        return np.stack([self.r1(mask), self.r1(mask)], -1)

    def r3(self, mask):
        return np.stack([self.r1(mask), self.r1(mask), self.r1(mask)], -1)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# util.rs
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def cosine_sample_hemisphere(r1, r2):
    theta = np.arccos(np.sqrt(r1))
    phi = 2.0 * PI * r2
    return vec(np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi))


def create_cartesian(up):
    temp = normalize(cross(up, ARBITRARY))
    right = normalize(cross(temp, up))
    forward = normalize(cross(up, right))
    return up, right, forward


def reflect(i, normal):
    return i - normal * 2.0 * col(dot(i, normal))


def ggx_distribution(normal, halfway, roughness):
    a = roughness * roughness
    ndh = np.maximum(dot(normal, halfway), 0.0)
    den = ndh * ndh * (a - 1.0) + 1.0
    return a / np.maximum(PI * (den * den), EPS)


def ggx_half_angle(r2, roughness):
    """(cos, sin) of the sampled half vector's polar angle.  THE ONE PLACE WHERE THIS FILE COMPUTES IN FLOAT32: as the reference writes it,
    r2 * (a * a - 1) + 1 with a = roughness^2 loses a * a against 1 (a * a = 6e-6 at roughness 0.05, and below roughness 0.016 it vanishes: a perfect
    mirror), and 1 - cos^2 cancels again, so the float32 result is off the float64 one by up to a percent of the deflection: not rounding noise but what
    the formula MEANS in the reference's arithmetic.  The expression uses only +, -, *, / and sqrt of exact float32 inputs, which IEEE 754 defines
    bit for bit, so it is evaluated here in float32, in the order written (util.rs:68-72), and everything after it in float64 again."""
    one = np.float32(1.0)
    rough = np.asarray(roughness, np.float64).astype(np.float32)
    r2 = np.asarray(r2, np.float64).astype(np.float32)
    a = rough * rough
    cos_t = np.sqrt((one - r2) / (r2 * (a * a - one) + one))
    sin_t = np.sqrt(one - cos_t * cos_t)
    return cos_t.astype(np.float64), sin_t.astype(np.float64)


def sample_ggx(r1, r2, reflection, roughness):
    """-> (direction, margin of the choice of the tangent frame's helper axis)"""
    phi = 2.0 * PI * r1
    cos_t, sin_t = ggx_half_angle(r2, roughness)
    h = vec(np.cos(phi) * sin_t, np.sin(phi) * sin_t, cos_t)
    z = np.abs(reflection[..., 2])
    up = np.where(col(z < GGX_UP_SWITCH), np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0]))
    tangent = normalize(cross(up, reflection))
    bitangent = cross(reflection, tangent)
    return normalize(tangent * h[..., 0:1] + bitangent * h[..., 1:2] + reflection * h[..., 2:3]), np.abs(z - GGX_UP_SWITCH)


def geometry_schlick_ggx(normal, direction, roughness):
    num = np.maximum(dot(normal, direction), 0.0)
    k = (roughness * roughness) / 8.0
    return num / (num * (1.0 - k) + k)


def geometry_smith_schlick_ggx(normal, view, light, roughness):
    return geometry_schlick_ggx(normal, view, roughness) * geometry_schlick_ggx(normal, light, roughness)


def fresnel_schlick(cos_theta, f0):
    return f0 + (1.0 - f0) * col((1.0 - cos_theta) ** 5)


def fresnel_schlick_scalar(in_ior, out_ior, cos_theta):
    f0 = ((in_ior - out_ior) / (in_ior + out_ior)) ** 2
    return f0 + (1.0 - f0) * (1.0 - cos_theta) ** 5


def barycentric(p, a, b, c):
    v0, v1, v2 = b - a, c - a, p - a
    d00, d01, d11, d20, d21 = dot(v0, v0), dot(v0, v1), dot(v1, v1), dot(v2, v0), dot(v2, v1)
    den = d00 * d11 - d01 * d01
    v = (d11 * d20 - d01 * d21) / den
    w = (d00 * d21 - d01 * d20) / den
    return vec(1.0 - v - w, v, w)


def power_heuristic(p1, p2):
    return p1 * p1 / (p1 * p1 + p2 * p2)


def lerp(a, b, t):
    return a * (1.0 - t) + b * t


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# image_polyfill.rs: the sampler
# ---------------------------------------------------------------------------------------------------------------------------------------------------
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def as_i32(x32):
    """Rust's `f32 as i32` of float32 values -> int64 array: NaN -> 0, everything beyond the range (the infinities included) saturates"""
    x = np.asarray(x32, np.float32).astype(np.float64)
    return np.where(np.isnan(x), 0.0, np.clip(x, float(I32_MIN), float(I32_MAX))).astype(np.int64)


def texel_values(image):
    """(h, w, 4) texels in float64: an RGBA8 atlas as u8 / 255 with w = 1 (src/asset.rs builds the CPU image so), a float image as it is"""
    image = np.asarray(image)
    if image.dtype == np.uint8:
        t = image.astype(np.float64) / 255.0
        t[..., 3] = 1.0
        return t
    assert image.dtype == np.float32
    return image.astype(np.float64)


def sample_by_lod(image, width, height, coord):
    """Image::sample_by_lod of the CPU polyfill (image_polyfill.rs:32-55): bilinear, WRAPPING (sample_raw takes every coordinate modulo the extent),
    with NO half-texel offset: texel k sits at coordinate k / extent exactly.  The reference's GPU path samples through a hardware clamp-to-edge
    sampler instead; the CPU polyfill is what the oracle and the kernels follow, and what is restated here.
    image (height, width, 4) uint8 or float32, coord (n, 2) -> (value (n, 4), texels (n, 4, 2): the integer (x, y) of c00, c01, c10, c11, raw (n, 2, 2):
    floor_uv and ceil_uv as the i32 they are before sample_raw reduces them).
    The value is float64; the addressing is integer exact: floor and ceil of the FLOAT32 scaled coordinate (the number the reference holds) through the
    saturating cast `as i32`, sign-extended to 64 bits (`as usize`) and reduced by an unsigned remainder.  A scaled coordinate beyond the float32 range
    is an infinity there: its fract() is NaN and so is the value."""
    texels = texel_values(image).reshape(height, width, 4)
    coord = np.asarray(coord, np.float64)
    with np.errstate(all="ignore"):
        scaled = coord * np.array([float(np.float32(width)), float(np.float32(height))])
        scaled32 = scaled.astype(np.float32)
        scaled = np.where(np.isinf(scaled32), scaled32.astype(np.float64), scaled)
        frac = scaled - np.floor(scaled)                                          # Vec2::fract = self - self.floor()
    lo, hi = as_i32(np.floor(scaled32)), as_i32(np.ceil(scaled32))                # floor_uv, ceil_uv
    extent = np.array([width, height], np.uint64)
    lo_u, hi_u = lo.view(np.uint64) % extent, hi.view(np.uint64) % extent         # `as usize` keeps the two's complement; % is unsigned
    lo_u, hi_u = lo_u.astype(np.int64), hi_u.astype(np.int64)

    def raw(x, y):
        return texels[y, x]

    c00, c01 = raw(lo_u[:, 0], lo_u[:, 1]), raw(lo_u[:, 0], hi_u[:, 1])
    c10, c11 = raw(hi_u[:, 0], lo_u[:, 1]), raw(hi_u[:, 0], hi_u[:, 1])
    with np.errstate(all="ignore"):
        tx, ty = frac[:, 0:1], frac[:, 1:2]
        a = c00 + (c10 - c00) * tx                                                # Vec4::lerp: a + (b - a) * s
        b = c01 + (c11 - c01) * tx
        value = a + (b - a) * ty
    index = np.stack([np.stack([lo_u[:, 0], lo_u[:, 1]], -1), np.stack([lo_u[:, 0], hi_u[:, 1]], -1),
                      np.stack([hi_u[:, 0], lo_u[:, 1]], -1), np.stack([hi_u[:, 0], hi_u[:, 1]], -1)], 1)
    return value, index, np.stack([lo, hi], 1)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# bsdf.rs: PBR.  albedo (..., 3); roughness, metallic (...,) already through get_pbr_bsdf's guards (pbr_guards); clamp = (lo, hi)
# ---------------------------------------------------------------------------------------------------------------------------------------------------
DIFFUSE, SPECULAR = 0, 1


def pbr_guards(roughness, metallic):
    """get_pbr_bsdf after its texture lookups: roughness.max(EPS), metallic.min(1 - EPS) (the difference taken in f32, as the reference's f32 expression)"""
    return np.maximum(roughness, EPS), np.minimum(metallic, f32(np.float32(1.0) - np.float32(0.001)))


def specular_weight(view, normal, metallic, clamp):
    """-> (weight, margin).  The clamp is skipped for a weight of exactly 0 or 1; that is a decision only where the clamp would move the weight.  Seen
    from behind, the cosine is clamped to exactly 0 and the weight is exactly 1 in float32 as in float64 (x + (1 - x) and (1 - m) + m round to 1): that
    exemption is as far from its alternative as the view is from the surface plane."""
    ndv = dot(normal, view)
    w = lerp(fresnel_schlick_scalar(1.0, 1.5, np.maximum(ndv, 0.0)), 1.0, metallic)
    lo, hi = clamp
    exempt = (w == 0.0) | (w == 1.0)
    clamped = np.where(w < lo, lo, np.where(w > hi, hi, w))          # f32::clamp
    moves = clamped != w
    margin = np.where(moves, np.where(ndv <= 0.0, np.abs(ndv), np.minimum(np.abs(w), np.abs(1.0 - w))), INF)
    return np.where(exempt, w, clamped), margin


def _ks(view, direction, albedo, metallic):
    halfway = normalize(view + direction)
    f0 = F0_DIELECTRIC + (albedo - F0_DIELECTRIC) * col(metallic)      # Vec3::lerp: a + (b - a) * s
    return halfway, fresnel_schlick(np.maximum(dot(halfway, view), 0.0), f0)


def _diffuse(cos_theta, weight, ks, albedo, metallic):
    kd = (1.0 - ks) * col(1.0 - metallic)
    return kd * albedo / PI * col(cos_theta) / col(1.0 - weight)


def _specular(view, normal, direction, cos_theta, d_term, weight, ks, roughness):
    g_term = geometry_smith_schlick_ggx(normal, view, direction, roughness)
    num = col(d_term * g_term) * ks
    den = 4.0 * np.maximum(dot(normal, view), 0.0) * cos_theta
    return num / col(np.maximum(den, EPS)) * col(cos_theta) / col(weight)


def _pdf_specular(view, normal, halfway, d_term):
    return d_term * dot(normal, halfway) / (4.0 * dot(view, halfway))


def pbr_evaluate(view, normal, direction, lobe, albedo, roughness, metallic, clamp):
    weight, _ = specular_weight(view, normal, metallic, clamp)
    cos_theta = np.maximum(dot(normal, direction), 0.0)
    halfway, ks = _ks(view, direction, albedo, metallic)
    d_term = ggx_distribution(normal, halfway, roughness)
    return np.where(col(lobe == DIFFUSE), _diffuse(cos_theta, weight, ks, albedo, metallic),
                    _specular(view, normal, direction, cos_theta, d_term, weight, ks, roughness))


def pbr_pdf(view, normal, direction, lobe, roughness):
    halfway = normalize(view + direction)
    d_term = ggx_distribution(normal, halfway, roughness)
    return np.where(lobe == DIFFUSE, np.maximum(dot(normal, direction), 0.0) / PI, _pdf_specular(view, normal, halfway, d_term))


def pbr_sample(view, normal, r, albedo, roughness, metallic, clamp):
    """-> dict(pdf, lobe, spectrum, direction, margin, min_cosine); r (..., 3) are the three random numbers of gen_r3.  min_cosine: halfway . view of a
    specular sample, the denominator of its pdf (infinity for a diffuse one)"""
    weight, m_clamp = specular_weight(view, normal, metallic, clamp)
    diffuse = r[..., 2] >= weight
    up, nt, nb = create_cartesian(normal)
    s = cosine_sample_hemisphere(r[..., 0], r[..., 1])
    d_diffuse = normalize(s[..., 0:1] * nb + s[..., 1:2] * up + s[..., 2:3] * nt)
    d_specular, m_frame = sample_ggx(r[..., 0], r[..., 1], reflect(-view, normal), roughness)
    direction = np.where(col(diffuse), d_diffuse, d_specular)
    cos_theta = np.maximum(dot(normal, direction), EPS)
    halfway, ks = _ks(view, direction, albedo, metallic)
    d_term = ggx_distribution(normal, halfway, roughness)
    pdf = np.where(diffuse, cos_theta / PI, _pdf_specular(view, normal, halfway, d_term))
    spectrum = np.where(col(diffuse), _diffuse(cos_theta, weight, ks, albedo, metallic),
                        _specular(view, normal, direction, cos_theta, d_term, weight, ks, roughness))
    margin = np.minimum(np.minimum(np.abs(r[..., 2] - weight), m_clamp), np.where(diffuse, INF, m_frame))
    hv = np.nan_to_num(np.maximum(dot(halfway, view), 0.0), nan=0.0)
    min_cosine = np.where(diffuse, INF, hv)
    return dict(pdf=pdf, lobe=np.where(diffuse, DIFFUSE, SPECULAR), spectrum=spectrum, direction=direction, margin=margin, min_cosine=min_cosine)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# skybox.rs
# ---------------------------------------------------------------------------------------------------------------------------------------------------
RAY_COEFF = np.array([f32(58e-7), f32(135e-7), f32(331e-7)])          # scatter == effective: Rayleigh does not absorb
MIE_SCATTER = np.full(3, f32(2e-5))
MIE_EFFECTIVE = np.full(3, f32(np.float32(2e-5) * np.float32(1.1)))
EARTH_RADIUS, ATMOSPHERE_RADIUS, H_RAY, H_MIE = f32(6360e3), f32(6380e3), f32(8e3), f32(12e2)
CENTER = np.array([0.0, -EARTH_RADIUS, 0.0])
SKY_STEPS = 12


def _escape(p, d, r):
    v = p - CENTER
    b = dot(v, d)
    det = b * b - dot(v, v) + r * r
    root = np.sqrt(np.where(det < 0.0, 0.0, det))
    t1, t2 = -b - root, -b + root
    return np.where(det < 0.0, -1.0, np.where(t1 >= 0.0, t1, t2))


def _densities(p):
    h = np.maximum(np.sqrt(dot(p - CENTER, p - CENTER)) - EARTH_RADIUS, 0.0)
    return np.stack([np.exp(-h / H_RAY), np.exp(-h / H_MIE)], -1)


def sky(sun_direction4, origin, direction):
    """skybox::scatter; origin (3,) or (n, 3), direction (n, 3) -> rgb (n, 3)"""
    with np.errstate(all="ignore"):
        sun4 = np.asarray(sun_direction4, np.float64)
        sun, origin = sun4[:3], np.broadcast_to(np.asarray(origin, np.float64), direction.shape)
        step = _escape(origin, direction, ATMOSPHERE_RADIUS) / float(SKY_STEPS)
        i_r, i_m, total = np.zeros(direction.shape), np.zeros(direction.shape), np.zeros(direction.shape[:-1] + (2,))
        for i in range(SKY_STEPS):
            p = origin + direction * col(step * float(i))
            d_rm = _densities(p) * col(step)
            total = total + d_rm
            l = _escape(p, sun, ATMOSPHERE_RADIUS)
            to_sun = _densities(p) * col(l / 2.0) + _densities(p + sun * col(l)) * col(l / 2.0)
            depth = total + to_sun
            a = np.exp(-RAY_COEFF * depth[..., 0:1] - MIE_EFFECTIVE * depth[..., 1:2])
            i_r = i_r + a * d_rm[..., 0:1]
            i_m = i_m + a * d_rm[..., 1:2]
        mu = dot(direction, sun)
        res = col(sun4[3] * (1.0 + mu * mu)) * (i_r * RAY_COEFF * f32(0.0597) + i_m * MIE_SCATTER * f32(0.0196) / col((f32(1.58) - f32(1.52) * mu) ** 1.5))
        return mask_nan(np.sqrt(res)) ** f32(2.2)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the scene: plain float64 / integer arrays taken from the struct arrays of a World, its RGBA8 atlas (world.atlas, if any material has a texture flag)
# and the float image of the sky (skybox, if the configuration has has_skybox = 1).  A material's albedo / roughness / metallic / normals field holds the
# factor (untextured) or the atlas rectangle (x, y, width, height in atlas coordinates: textured); roughness and metallic are kept WITHOUT the guards of
# get_pbr_bsdf, which act after the lookup.
# ---------------------------------------------------------------------------------------------------------------------------------------------------
class Scene:
    def __init__(self, world, skybox=None):
        f = np.float64
        self.vertex = world.per_vertex["vertex"][:, :3].astype(f)
        self.normal = world.per_vertex["normal"][:, :3].astype(f)
        t = world.indices
        self.tri = np.stack([t["v0"], t["v1"], t["v2"]], 1).astype(np.int64)
        self.material = t["material"].astype(np.int64)
        m = world.materials
        self.uv, self.tangent = world.per_vertex["uv0"].astype(f), world.per_vertex["tangent"][:, :3].astype(f)
        self.emissive = m["emissive"][:, :3].astype(f)
        self.rect = {k: m[k].astype(f) for k in ("albedo", "roughness", "metallic", "normals")}           # (n_materials, 4): factor or rectangle
        self.flag = {k: m[f"has_{n}_texture"] != 0 for k, n in (("albedo", "albedo"), ("roughness", "roughness"), ("metallic", "metallic"), ("normals", "normal"))}
        self.textured = self.flag["albedo"] | self.flag["roughness"] | self.flag["metallic"] | self.flag["normals"]
        self.atlas = getattr(world, "atlas", None)
        assert self.atlas is not None or not self.textured.any(), "a texture flag without an atlas"
        self.skybox = skybox
        self.is_emitter = (self.emissive != 0.0).any(1)
        lp = world.light_pick
        self.light = {k: lp[k].astype(np.int64 if "index" in k else f) for k in lp.dtype.names}
        self.a, self.b, self.c = (self.vertex[self.tri[:, k]] for k in range(3))


def _moller_trumbore(sc, ro, rd):
    """all rays against all triangles: (hit, t, backface, margin), each (n_rays, n_triangles).  margin: how far the triangle's hit-or-miss decision is
    from the other outcome: a hit turns into a miss when its smallest slack is used up, a miss into a hit only when all its failed tests pass"""
    e1, e2 = sc.b - sc.a, sc.c - sc.a
    pv = cross(rd[:, None, :], e2[None])
    det = dot(e1[None], pv)
    backface = np.signbit(det)
    scale = np.sqrt(dot(e1, e1) * dot(e2, e2))[None]
    s_det = (np.abs(det) - DET_MIN) / scale
    inv = 1.0 / det
    tv = ro[:, None, :] - sc.a[None]
    u = dot(tv, pv) * inv
    qv = cross(tv, e1[None])
    v = dot(rd[:, None, :], qv) * inv
    t = dot(e2[None], qv) * inv
    tn = np.maximum(1.0, np.abs(t))
    slack = np.stack([s_det, u, 1.0 - u, v, 1.0 - (u + v), t / tn, (t - T_MIN) / tn, (T_FAR - t) / tn], 0)
    passed = np.stack([s_det >= 0.0, u >= 0.0, u <= 1.0, v >= 0.0, u + v <= 1.0, t >= 0.0, t > T_MIN, t < T_FAR], 0)
    hit = passed.all(0)
    slack = np.where(np.isfinite(slack), slack, 0.0)
    m_hit = np.abs(slack).min(0)
    m_miss = np.where(passed, 0.0, np.abs(slack)).max(0)
    margin = np.where(hit, m_hit, np.where(passed[0], m_miss, np.abs(s_det)))
    return hit, t, backface, margin


def intersect_nearest(sc, ro, rd):
    """-> hit, t, triangle index, backface, margin (every triangle's decision, the facing, and the gap to the second nearest hit)"""
    with np.errstate(all="ignore"):
        hit, t, backface, margin = _moller_trumbore(sc, ro, rd)
        tt = np.where(hit, t, INF)
        order = np.argsort(tt, axis=1, kind="stable")
        rows = np.arange(len(ro))
        first = order[:, 0]
        t1 = tt[rows, first]
        t2 = tt[rows, order[:, 1]] if tt.shape[1] > 1 else np.full(len(ro), INF)
        any_hit = np.isfinite(t1)
        gap = np.where(np.isfinite(t2), (t2 - t1) / np.maximum(1.0, t1), INF)
        return any_hit, np.where(any_hit, t1, T_FAR), first, backface[rows, first] & any_hit, np.minimum(margin.min(1), gap)


def intersect_any(sc, ro, rd, max_t):
    """-> occluded, margin"""
    with np.errstate(all="ignore"):
        hit, t, _, margin = _moller_trumbore(sc, ro, rd)
        within = t <= max_t[:, None]
        m_max = np.abs(max_t[:, None] - t) / np.maximum(1.0, np.abs(t))
        margin = np.where(hit, np.minimum(margin, m_max), margin)          # a miss stays a miss whatever max_t says
        return (hit & within).any(1), margin.min(1)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# light_pick.rs
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def light_pdf(area, distance, light_normal, direction):
    cos_theta = dot(light_normal, -direction)
    return np.where(cos_theta <= 0.0, 0.0, distance ** 2 / (area * cos_theta))


SHADOW_MATTERS = 1e-9       # radiance: a shadow ray whose term is below this whatever it finds (a light seen edge on, or from behind) decides nothing


def sample_direct_lighting(mis, sc, rng, mask, throughput, bsdf, point, normal, ray_direction, clamp):
    """-> dict(area, normal, pick_pdf, emission, triangle, throughput, contribution, margin) for the samples of mask (other rows are to be ignored)"""
    L = sc.light
    n_entries = len(L["ratio"])
    r = rng.r2(mask)
    x = r[:, 0] * float(n_entries)
    entry = np.minimum(x.astype(np.int64), n_entries - 1)              # r == 1.0 indexes past the table in the reference; never compared (margin 0)
    m_pick = np.where(x >= n_entries, 0.0, np.minimum(x - np.floor(x), np.floor(x) + 1.0 - x)) if n_entries > 1 else np.where(x >= n_entries, 0.0, INF)
    first = r[:, 1] < L["ratio"][entry]
    same = L["triangle_index_a"][entry] == L["triangle_index_b"][entry]
    m_pick = np.minimum(m_pick, np.where(same, INF, np.abs(r[:, 1] - L["ratio"][entry])))
    tri = np.where(first, L["triangle_index_a"][entry], L["triangle_index_b"][entry])
    area = np.where(first, L["triangle_area_a"][entry], L["triangle_area_b"][entry])
    pick_pdf = np.where(first, L["triangle_pick_pdf_a"][entry], L["triangle_pick_pdf_b"][entry])
    idx = sc.tri[tri]
    l_normal = (sc.normal[idx[:, 0]] + sc.normal[idx[:, 1]] + sc.normal[idx[:, 2]]) / 3.0
    emission = sc.emissive[sc.material[tri]]

    r = rng.r2(mask)
    s = np.sqrt(r[:, 0])
    l_point = col(1.0 - s) * sc.a[tri] + col(s * (1.0 - r[:, 1])) * sc.b[tri] + col(s * r[:, 1]) * sc.c[tri]
    to_light = l_point - point
    distance = np.sqrt(dot(to_light, to_light))
    direction = to_light / col(distance)
    occluded, m_shadow = intersect_any(sc, point + direction * EPS, direction, distance - EPS * 2.0)

    lp = light_pdf(area, distance, l_normal, direction)
    view = -ray_direction
    attenuation = pbr_evaluate(view, normal, direction, np.full(len(point), DIFFUSE), bsdf["albedo"], bsdf["roughness"], bsdf["metallic"], clamp)
    bp = pbr_pdf(view, normal, direction, np.full(len(point), DIFFUSE), bsdf["roughness"])
    weight = power_heuristic(lp, bp) if mis else 1.0
    direct = attenuation * emission * col(weight) / col(lp) / col(pick_pdf)
    unoccluded = np.where(col((lp > 0.0) & (bp > 0.0)), throughput * direct, 0.0)
    m_shadow = np.where(np.abs(unoccluded).max(-1) > SHADOW_MATTERS, m_shadow, INF)
    direct = np.where(col(~occluded & (lp > 0.0) & (bp > 0.0)), direct, 0.0)
    return dict(area=area, normal=l_normal, pick_pdf=pick_pdf, emission=emission, triangle=tri, throughput=throughput,
                contribution=throughput * direct, margin=np.minimum(m_pick, m_shadow))


def bsdf_mis_contribution(t, triangle, last_bsdf, last_light):
    lp = light_pdf(last_light["area"], t, last_light["normal"], last_bsdf["direction"])
    weight = power_heuristic(last_bsdf["pdf"], lp)
    direct = last_bsdf["spectrum"] * last_light["emission"] * col(weight) / col(last_bsdf["pdf"]) / col(last_light["pick_pdf"])
    return np.where(col((triangle == last_light["triangle"]) & (lp > 0.0)), last_light["throughput"] * direct, 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# lib.rs: camera ray and path loop
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def rotation_y(a):
    s, c = np.sin(a), np.cos(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])         # glam's columns (c, 0, -s), (0, 1, 0), (s, 0, c), written as rows of a matrix


def rotation_x(a):
    s, c = np.sin(a), np.cos(a)
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])         # columns (1, 0, 0), (0, c, s), (0, -s, c)


def camera_rays(cfg, px, py, jitter):
    W, H = float(cfg.width), float(cfg.height)
    sx, sy = px + jitter[:, 0], py + jitter[:, 1]
    u = sx / W * 2.0 - 1.0
    v = ((1.0 - sy / H) * 2.0 - 1.0) * (H / W)
    d = normalize(vec(u, v, 1.0))
    m = rotation_y(float(cfg.cam_rotation[1])) @ rotation_x(float(cfg.cam_rotation[0]))
    return np.broadcast_to(np.array([float(cfg.cam_position[k]) for k in range(3)]), d.shape).copy(), d @ m.T


def _update(old, new, mask):
    return {k: np.where(col(mask) if np.ndim(new[k]) > 1 else mask, new[k], old[k]) for k in old}


def _lookup(sc, field, mat, uv):
    """the atlas at the material's rectangle of `field`: material.field.xy + uv * material.field.zw -> (n, 4)"""
    r = sc.rect[field][mat]
    h, w = sc.atlas.shape[:2]
    return sample_by_lod(sc.atlas, w, h, r[:, 0:2] + uv * r[:, 2:4])[0]


def image_sky(cfg, skybox, direction):
    """lib.rs:72-77 -> (rgb (n, 3) before the throughput, |rotated.y| (n,)).  The arcsine's argument is held inside [-1, 1]: a float64 unit vector may
    exceed it by a rounding, and a sample that close to a pole is flagged anyway (the module's head)."""
    sun = [float(cfg.sun_direction[k]) for k in range(4)]
    rotation = np.arctan2(sun[2], sun[0])
    rotated = direction @ rotation_y(rotation).T
    u = 0.5 + np.arctan2(rotated[:, 2], rotated[:, 0]) / (2.0 * PI)
    v = 1.0 - (0.5 + np.arcsin(np.clip(rotated[:, 1], -1.0, 1.0)) / PI)
    intensity = sun[3] * f32(np.float32(1.0) / np.float32(15.0))
    h, w = skybox.shape[:2]
    return sample_by_lod(skybox, w, h, np.stack([u, v], -1))[0][:, :3] * intensity, np.abs(rotated[:, 1])


def trace(cfg, world, px, py, n, offset, skybox=None):
    """trace_pixel for the samples (px, py, rng n, rng offset), each an (N,) array -> (radiance (N, 3), margin (N,), min_cosine (N,): the smallest
    halfway . view of the path's specular bounces, sky_y (N,): |rotated.y| of the sample's lookup in the image sky, 0 if it made none)"""
    sc = world if isinstance(world, Scene) else Scene(world, skybox)
    assert cfg.has_skybox == 0 or sc.skybox is not None, "has_skybox = 1 needs the image"
    N = len(px)
    nee_mode = cfg.nee if cfg.nee <= 2 else 0
    nee, mis = nee_mode != 0, nee_mode == 1
    clamp = (float(cfg.specular_weight_clamp[0]), float(cfg.specular_weight_clamp[1]))
    rng = Rng(n, offset)
    every = np.ones(N, bool)
    with np.errstate(all="ignore"):
        origin, direction = camera_rays(cfg, np.asarray(px, np.float64), np.asarray(py, np.float64), rng.r2(every))
        throughput, radiance, margin, alive, min_cosine = np.ones((N, 3)), np.zeros((N, 3)), np.full(N, INF), every.copy(), np.full(N, INF)
        sky_y = np.zeros(N)
        last_bsdf = dict(pdf=np.zeros(N), lobe=np.zeros(N, np.int64), spectrum=np.zeros((N, 3)), direction=np.zeros((N, 3)))
        last_light = dict(area=np.zeros(N), normal=np.zeros((N, 3)), pick_pdf=np.zeros(N), emission=np.zeros((N, 3)), triangle=np.zeros(N, np.int64),
                          throughput=np.zeros((N, 3)))

        def decide(m, mask):
            nonlocal margin
            margin = np.where(mask, np.minimum(margin, m), margin)

        for bounce in range(cfg.max_bounces):
            if not alive.any():
                break
            hit, t, tri, backface, m_hit = intersect_nearest(sc, origin, direction)
            decide(m_hit, alive)
            point = origin + direction * col(t)
            miss = alive & ~hit
            if miss.any() and cfg.has_skybox == 0:
                radiance = radiance + np.where(col(miss), throughput * sky(cfg.sun_direction, origin, direction), 0.0)
            elif miss.any():
                rgb, y = image_sky(cfg, sc.skybox, direction)
                radiance = radiance + np.where(col(miss), throughput * rgb, 0.0)
                sky_y = np.where(miss, y, sky_y)
            alive = alive & hit

            mat = sc.material[tri]
            emitter = alive & sc.is_emitter[mat]
            front = emitter & ~backface
            direct_hit = front & (not nee or bounce == 0 or (last_bsdf["lobe"] != DIFFUSE))
            radiance = radiance + np.where(col(direct_hit), mask_nan(throughput * sc.emissive[mat]), 0.0)
            by_mis = front & ~direct_hit & mis
            radiance = radiance + np.where(col(by_mis), mask_nan(bsdf_mis_contribution(t, tri, last_bsdf, last_light)), 0.0)
            alive = alive & ~(emitter & backface) & ~direct_hit & ~by_mis

            idx = sc.tri[tri]
            bary = barycentric(point, sc.a[tri], sc.b[tri], sc.c[tri])
            normal = bary[:, 0:1] * sc.normal[idx[:, 0]] + bary[:, 1:2] * sc.normal[idx[:, 1]] + bary[:, 2:3] * sc.normal[idx[:, 2]]
            uv = bary[:, 0:1] * sc.uv[idx[:, 0]] + bary[:, 1:2] * sc.uv[idx[:, 1]] + bary[:, 2:3] * sc.uv[idx[:, 2]]
            outside = ((uv < 0.0) | (uv > 1.0)).any(1)                        # uv.clamp(0, 1) != uv: EITHER component, and then the whole Vec2 is wrapped
            uv = np.where(col(outside), uv - np.floor(uv), uv)
            textured = alive & sc.textured[mat]
            if textured.any():
                decide(np.abs(uv - np.rint(uv)).min(1), textured)
                if sc.flag["normals"].any():                                      # lib.rs:132-141
                    normal_map = _lookup(sc, "normals", mat, uv) * 2.0 - 1.0
                    tangent = bary[:, 0:1] * sc.tangent[idx[:, 0]] + bary[:, 1:2] * sc.tangent[idx[:, 1]] + bary[:, 2:3] * sc.tangent[idx[:, 2]]
                    mapped = normalize(tangent * normal_map[:, 0:1] + cross(tangent, normal) * normal_map[:, 1:2] + normal * normal_map[:, 2:3])
                    normal = np.where(col(sc.flag["normals"][mat]), mapped, normal)
            # get_pbr_bsdf (bsdf.rs:354-379): albedo .xyz, roughness and metallic .x of their own rectangles, then the guards
            albedo, roughness, metallic = sc.rect["albedo"][mat][:, :3], sc.rect["roughness"][mat][:, 0], sc.rect["metallic"][mat][:, 0]
            if textured.any():
                if sc.flag["albedo"].any():
                    albedo = np.where(col(sc.flag["albedo"][mat]), _lookup(sc, "albedo", mat, uv)[:, :3], albedo)
                if sc.flag["roughness"].any():
                    roughness = np.where(sc.flag["roughness"][mat], _lookup(sc, "roughness", mat, uv)[:, 0], roughness)
                if sc.flag["metallic"].any():
                    metallic = np.where(sc.flag["metallic"][mat], _lookup(sc, "metallic", mat, uv)[:, 0], metallic)
            roughness, metallic = pbr_guards(roughness, metallic)
            bsdf = dict(albedo=albedo, roughness=roughness, metallic=metallic)
            s = pbr_sample(-direction, normal, rng.r3(alive), bsdf["albedo"], bsdf["roughness"], bsdf["metallic"], clamp)
            decide(s.pop("margin"), alive)
            min_cosine = np.where(alive, np.minimum(min_cosine, s.pop("min_cosine")), min_cosine)
            last_bsdf = _update(last_bsdf, s, alive)

            lit = alive & nee & (s["lobe"] == DIFFUSE)
            if lit.any() and sc.light["ratio"][0] >= 0.0:                  # a negative ratio in the first entry: no lights
                ls = sample_direct_lighting(mis, sc, rng, lit, throughput, bsdf, point, normal, direction, clamp)
                decide(ls.pop("margin"), lit)
                radiance = radiance + np.where(col(lit), mask_nan(ls.pop("contribution")), 0.0)
                last_light = _update(last_light, ls, lit)

            throughput = np.where(col(alive), throughput * (s["spectrum"] / col(s["pdf"])), throughput)
            direction = np.where(col(alive), s["direction"], direction)
            origin = np.where(col(alive), point + direction * EPS, origin)

            if bounce > cfg.min_bounces:
                prob = throughput.max(1)
                r = rng.r1(alive)
                decide(np.abs(r - prob), alive)
                alive = alive & ~(r > prob)
                throughput = np.where(col(alive), throughput * col(1.0 / prob), throughput)
    return radiance, margin, min_cosine, sky_y


def trace_image(cfg, world, seeds, first_sample, n_samples, skybox=None):
    """samples first_sample .. of every pixel of the image -> (radiance (n_samples, H, W, 3), margin, min_cosine, sky_y (n_samples, H, W) each);
    seeds: the (H*W,) records (n, offset) of sample 0"""
    W, H = cfg.width, cfg.height
    sc = Scene(world, skybox)
    py, px = np.divmod(np.arange(W * H), W)
    out = [], [], [], []
    for k in range(first_sample, first_sample + n_samples):
        r, m, c, y = trace(cfg, sc, px, py, seeds["n"].astype(np.uint64) + np.uint64(k), seeds["offset"])
        for o, a in zip(out, (r.reshape(H, W, 3), m.reshape(H, W), c.reshape(H, W), y.reshape(H, W))):
            o.append(a)
    return tuple(np.stack(o) for o in out)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# render.wgsl: mean and the display tonemap operators 0..6
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _saturate(x):
    """clamp(x, 0, 1) = min(max(x, 0), 1).  WGSL leaves the result for a NaN (infinity / infinity at an infinite input) to the implementation; min and
    max that return their other operand, as IEEE minNum / maxNum do, give 0 there, and that is the reading taken here."""
    return np.fmin(np.fmax(x, 0.0), 1.0)


def _narkowicz(x):
    a, b, c, d, e = f32(2.51), f32(0.03), f32(2.43), f32(0.59), f32(0.14)
    return _saturate((x * (a * x + b)) / (x * (c * x + d) + e))


ACES_IN = np.array([[f32(0.59719), f32(0.35458), f32(0.04823)], [f32(0.07600), f32(0.90834), f32(0.01566)], [f32(0.02840), f32(0.13383), f32(0.83777)]])
ACES_OUT = np.array([[f32(1.60475), f32(-0.53108), f32(-0.07367)], [f32(-0.10208), f32(1.10813), f32(-0.00605)],
                     [f32(-0.00327), f32(-0.07276), f32(1.07602)]])


def _hill(x):
    # transpose(mat3x3(rows...)) * x: the vectors written in the shader are the ROWS of the matrix that multiplies x
    c = x @ ACES_IN.T
    a = c * (c + f32(0.0245786)) - f32(0.000090537)
    b = c * (f32(0.983729) * c + f32(0.4329510)) + f32(0.238081)
    return _saturate((a / b) @ ACES_OUT.T)


def _curve(x, a, b, c, d, e, f):
    return ((x * (a * x + c * b) + d * e) / (x * (a * x + b) + d * f)) - e / f


def resolve(accum_rgb, sample_count, op):
    """mean = sum / n, then operator op (0 none, 1 Reinhard, 2 Narkowicz ACES x 0.6, 3 Narkowicz ACES, 4 Hill ACES, 5 neutral, 6 Uncharted)"""
    with np.errstate(all="ignore"):
        x = np.asarray(accum_rgb, np.float64) / float(sample_count)
        if op == 1:
            return x / (x + 1.0)
        if op == 2:
            return _narkowicz(x * f32(0.6))
        if op == 3:
            return _narkowicz(x)
        if op == 4:
            return _hill(x)
        if op == 5:
            k = (f32(0.2), f32(0.29), f32(0.24), f32(0.272), f32(0.02), f32(0.3))
            white = 1.0 / _curve(f32(5.3), *k)
            return _curve(x * white, *k) * white / 1.0
        if op == 6:
            k = (f32(0.15), f32(0.50), f32(0.10), f32(0.20), f32(0.02), f32(0.30))
            return _curve(x * 2.0, *k) * (1.0 / _curve(f32(11.2), *k))
        return x
