"""A high-precision restatement of the shaders, and the cases of tests/test_shading_edges.py.

The restatement is written from the reference's text - Shading.fs:33-139, Light.fs:16-20, CommonTypes.fs:15-19 and 63-79,
Image.fs:25-26, Program.fs:59, and for the shadow rays Plane.fs:9-20 and Scene.fs:119-121 - and shares nothing with oracle/ or the
device.  It shades a GIVEN surface point: the hit's point and normal, the view ray, the material and the lights (directional with the
direction they store, or point lights with a falloff).  Which point is hit comes from closed forms of the scenes used here (a plane or
unit squares at y = 0: `plane_hit`); whether a light is blocked is either such a closed form (`plane_blocked`) or, where a ladder walks
across it, part of the text (`plane_in_the_way`, `square_in_the_way`).  The CPU half of the suite holds the oracle's `closest` and
`blocked` against all of them.

One text, two arithmetics (`Exact`, `Binary64`):

Exact     mpmath at 60 digits, the binary64 inputs taken as exact, every result fitted to binary64's RANGE (beyond the largest double
          it is inf, below half the smallest subnormal it is 0) and with the special values of IEEE 754: the formula as the reference
          means it, without its roundings.  `**` follows C `pow`; the three arguments at which .NET Core 2.0's Math.Pow answers
          otherwise are listed in `pow_differs` and compared device against oracle only.  Signed zeros are not told apart.
Binary64  Python floats: the reference's own operations in its own order, sqrt and division, no contraction.  It stands for the oracle
          where a BRANCH is asked for: both arithmetics record every decision they take (`branch`).  A case is kept when the two
          records agree, and rounding-decided when they do not.

The bound of a kept case (`evaluate`): the restatement is evaluated again with one perturbation at a time - every component of a
normalised vector, every dot product, the power's base and every libm result moved by +4 and by -4 units in its last binary64 place -
and the larger of the two changes of each is summed, per channel; a perturbed evaluation that leaves the finite numbers is skipped
when the opposite sign stays finite, and makes the bound infinite when neither does.  To that comes 64 * 2^-53 times the sum of the
absolute values of the fragments' parts: the roundings of the products and sums after the last perturbed value."""
import math
from collections import namedtuple

import mpmath
import numpy as np

import functracer_amd as ft

mpmath.mp.dps = 60
mpf = mpmath.mpf
INF, NAN = float("inf"), float("nan")
EPS = 0.0000001                                                    # CommonTypes.fs:65, Plane.fs:11
ULPS = 4
SUM_SLACK = 64 * 2.0 ** -53
_MAX = mpf(2) ** 1024 - mpf(2) ** 970                              # what rounds to inf
_MIN = mpf(2) ** -1075                                             # what rounds to 0
_TINY = mpf(2) ** -1074


# ---- the two arithmetics ----------------------------------------------------------------------------------------------------------------

class Arithmetic:
    def __init__(self, site=None, sign=0, forced=None):
        self.site_at, self.sign, self.forced = site, sign, forced
        self.sites, self.branches = 0, []
        self.parts = [0.0, 0.0, 0.0]                                # sum of |part| of every fragment, per channel

    def branch(self, name, taken):
        taken = bool(taken)
        if self.forced is not None and len(self.branches) < len(self.forced):
            taken = self.forced[len(self.branches)][1]
        self.branches.append((name, taken))
        return taken

    def dot(self, a, b):                                            # CommonTypes.fs:15-16
        return self.add(self.add(self.mul(a[0], b[0]), self.mul(a[1], b[1])), self.mul(a[2], b[2]))

    def fmax(self, a, b):                                           # F# max on floats is Math.Max: a NaN on either side is the result
        return self.num(NAN) if (a != a or b != b) else (b if a < b else a)

    def fmin(self, a, b):
        return self.num(NAN) if (a != a or b != b) else (a if a < b else b)


def _whole(y):
    return y == mpmath.floor(y)


class Exact(Arithmetic):
    exact = True

    def num(self, x):
        return mpf(x)

    def fit(self, x):
        if mpmath.isnan(x) or mpmath.isinf(x):
            return x
        a = abs(x)
        if a >= _MAX:
            return mpf("inf") if x > 0 else mpf("-inf")
        return mpf(0) if a <= _MIN else x

    def site(self, x):
        """A value the device or the oracle holds rounded: moved by +-ULPS units in its last binary64 place when it is this run's turn."""
        k = self.sites
        self.sites += 1
        if k != self.site_at or mpmath.isnan(x) or mpmath.isinf(x):
            return x
        ulp = _TINY if abs(x) < mpf(2) ** -1022 else mpf(2) ** (mpmath.floor(mpmath.log(abs(x), 2)) - 52)
        return x + self.sign * ULPS * ulp

    def add(self, a, b): return self.fit(a + b)
    def sub(self, a, b): return self.fit(a - b)
    def mul(self, a, b): return self.fit(a * b)
    def neg(self, a): return -a

    def div(self, a, b):
        if b == 0:
            return mpf(NAN) if (a == 0 or a != a) else (mpf("inf") if a > 0 else mpf("-inf"))
        return self.fit(a / b)

    def sqrt(self, a):
        return mpf(NAN) if (a != a or a < 0) else (a if mpmath.isinf(a) else mpmath.sqrt(a))

    def acos(self, a, what):
        if self.branch(what + ": acos outside [-1, 1]", not (-1 <= a <= 1)):
            return mpf(NAN)
        return mpmath.acos(a)

    def _trig(self, f, a):
        return mpf(NAN) if (a != a or mpmath.isinf(a)) else self.fit(f(a))

    def cos(self, a): return self._trig(mpmath.cos, a)
    def sin(self, a): return self._trig(mpmath.sin, a)
    def tan(self, a): return self._trig(mpmath.tan, a)

    def pow(self, x, y):
        """C pow (ISO C Annex F.10.4.4) over exact values."""
        inf = mpf("inf")
        if y == 0 or x == 1:
            return mpf(1)
        if x != x or y != y:
            return mpf(NAN)
        if mpmath.isinf(y):
            a = abs(x)
            return mpf(1) if a == 1 else (inf if (a > 1) == (y > 0) else mpf(0))
        odd = _whole(y) and abs(y) < mpf(2) ** 53 and int(y) % 2 == 1
        if x == 0:
            return mpf(0) if y > 0 else inf                         # the sign of zero is not kept
        if mpmath.isinf(x):
            big = inf if y > 0 else mpf(0)
            return -big if (x < 0 and odd) else big
        if x < 0 and not _whole(y):
            return mpf(NAN)
        t = y * mpmath.log(abs(x))
        r = inf if t > 711 else (mpf(0) if t < -746 else self.fit(mpmath.exp(t)))
        return -r if (x < 0 and odd) else r


class Binary64(Arithmetic):
    exact = False

    def num(self, x): return float(x)
    def site(self, x): return x
    def add(self, a, b): return a + b
    def sub(self, a, b): return a - b
    def mul(self, a, b): return a * b
    def neg(self, a): return -a

    def div(self, a, b):
        with np.errstate(all="ignore"):
            return float(np.float64(a) / np.float64(b))

    def sqrt(self, a):
        with np.errstate(all="ignore"):
            return float(np.sqrt(np.float64(a)))

    def acos(self, a, what):
        if self.branch(what + ": acos outside [-1, 1]", not (-1.0 <= a <= 1.0)):
            return NAN
        return math.acos(a)

    def _trig(self, f, a):
        return NAN if (a != a or math.isinf(a)) else f(a)

    def cos(self, a): return self._trig(math.cos, a)
    def sin(self, a): return self._trig(math.sin, a)
    def tan(self, a): return self._trig(math.tan, a)

    def pow(self, x, y):
        with np.errstate(all="ignore"):
            return float(np.power(np.float64(x), np.float64(y)))


def pow_differs(x, y):
    """The arguments at which C `pow` and .NET Core 2.0's Math.Pow (which returns NaN for a NaN on either side before anything else, and
    for a base of -1 under an infinite exponent) are not the same function; pow(+1, +-inf) is listed with them, as the issue has it."""
    return (y != y and x == 1.0) or (x != x and y == 0.0) or (math.isinf(y) and abs(x) == 1.0)


# ---- the reference's text ---------------------------------------------------------------------------------------------------------------

def normalise(K, v, what):                                         # CommonTypes.fs:63-67, Length: CommonTypes.fs:19
    l = K.sqrt(K.dot(v, v))
    if K.branch(what + ": |v| < 1e-7", l < K.num(EPS)):
        return list(v)
    s = K.div(K.num(1.0), l)
    return [K.site(K.mul(s, c)) for c in v]


def vneg(K, v):
    return [K.neg(c) for c in v]


def reflect(K, n, v):                                              # CommonTypes.fs:72: v - (2.0 * (v .* n) * n)
    k = K.mul(K.num(2.0), K.site(K.dot(v, n)))
    return [K.sub(a, K.mul(k, b)) for a, b in zip(v, n)]


def angle_between(K, a, b, what):                                  # CommonTypes.fs:74-75
    return K.site(K.acos(K.site(K.dot(normalise(K, a, what + " a"), normalise(K, b, what + " b"))), what))


def perpendicular_component(K, a, b, what):                        # CommonTypes.fs:77-79
    na = normalise(K, a, what)
    k = K.site(K.dot(b, na))
    return [K.sub(x, K.mul(k, y)) for x, y in zip(b, na)]


def specular_shader(K, n, view_d, mat, light_colour, light_dir):   # Shading.fs:78-87
    normal = normalise(K, n, "specular normal")
    reflected = normalise(K, reflect(K, normal, light_dir), "specular reflected")
    view = normalise(K, view_d, "specular view")
    base = K.site(K.dot(view, vneg(K, reflected)))
    sh = K.num(mat.shineyness)
    intensity = K.site(K.pow(base, sh))
    K.base = base
    K.differs = getattr(K, "differs", False) or (base == base and pow_differs(float(base), mat.shineyness))
    if K.branch("shineyness <= 0", sh <= 0) or K.branch("intensity <= 0", intensity <= 0):
        return [K.num(0.0)] * 3
    return [K.mul(c, intensity) for c in light_colour]


def lambertian_diffuse(K, n, mat, light_colour, light_dir):        # Shading.fs:65-70
    intensity = K.site(K.dot(vneg(K, light_dir), n))
    return [K.mul(intensity, K.mul(K.num(m), c)) for m, c in zip(mat.colour, light_colour)]


def rough_diffuse(K, n, view_d, mat, light_dir):                   # Shading.fs:50-63: the light's colour is read and not used
    r = K.num(mat.roughness)
    roughness = K.mul(r, r)                                         # roughness ** 2.0
    ray_angle = angle_between(K, n, vneg(K, view_d), "rayAngle")
    light_angle = angle_between(K, n, vneg(K, light_dir), "lightAngle")
    alpha, beta = K.fmax(ray_angle, light_angle), K.fmin(ray_angle, light_angle)
    A = K.sub(K.num(1.0), K.div(K.mul(K.num(0.5), roughness), K.add(roughness, K.num(0.33))))
    B = K.div(K.mul(K.num(0.45), roughness), K.add(roughness, K.num(0.09)))
    tangent_light = normalise(K, perpendicular_component(K, n, vneg(K, light_dir), "tangentLight normal"), "tangentLight")
    tangent_ray = normalise(K, perpendicular_component(K, n, vneg(K, view_d), "tangentRay normal"), "tangentRay")
    t = K.site(K.dot(tangent_light, tangent_ray))
    clamped = K.num(0.0) if K.branch("max 0.0 clamps", t < 0) else t          # max 0.0 t: NaN stays NaN
    if t != t:
        clamped = K.num(NAN)
    term = K.mul(K.mul(K.mul(B, clamped), K.site(K.sin(alpha))), K.site(K.tan(beta)))
    intensity = K.mul(K.site(K.cos(light_angle)), K.add(A, term))
    return [K.mul(intensity, K.num(m)) for m in mat.colour]


def attenuate(K, falloff, distance):                              # Light.fs:16-17
    c, l, q = [K.num(x) for x in falloff]
    return K.div(K.num(1.0), K.add(c, K.mul(distance, K.add(l, K.mul(distance, q)))))


def square_in_the_way(K, origin, direction, height, max_distance):
    """lightIsBocked (Scene.fs:119-121) for a lit unit square `height` above the receiver, the shadow ray inside its outline: the ray moved
    into the square's frame (a translation: one subtraction), Plane.intersect (Plane.fs:12-20; not the parallel rule: the callers' rays climb),
    then 0 <= t < maxDistance."""
    num = K.sub(K.num(0.0), K.sub(origin[1], K.num(height)))
    t = K.div(num, direction[1])
    return K.branch("the square is in the way", t >= 0 and t < max_distance)


def plane_in_the_way(K, origin, direction, max_distance, height=0.0):
    """lightIsBocked for a plane y = height with normal (0, 1, 0), the receiver itself among them (Plane.fs:12-20; a plane off y = 0 is
    translated: one subtraction): a direction within 1e-7 of parallel - one that normalise left 1e-7 short among them - meets it at t = 0
    when the origin is not 1e-7 under it."""
    num = K.sub(K.num(0.0), K.sub(origin[1], K.num(height)) if height else origin[1])
    if K.branch("shadow ray parallel to the plane", abs(direction[1]) < K.num(EPS)):
        t = K.num(0.0)
        if not num < K.num(EPS):
            return False
    else:
        t = K.div(num, direction[1])
    return K.branch("the plane is in the way", t >= 0 and t < max_distance)


def shade(K, n, view_d, mat, lights, p=(0.0, 0.0, 0.0), bounce=None, planes=(0.0,), scale=1.0):
    """Seq.sumBy over createFragments (Shading.fs:119-139) of multiPartShader [specular; reflection; diffuse] (Program.fs:59, Shading.fs:105-107)
    for a lit material at the hit (p, n).  lights: `Light`s, a directional one with its STORED direction.  bounce(direction): getColour of
    the fragment (Shading.fs:126, 132-134), the colour seen along the reflected direction - the same for every fragment of the hit; None: an
    open sky (Seq.sumBy over no fragments).  planes: the heights of the planes y = h a point light's shadow ray may meet, the receiver's first."""
    n, view_d, p = [K.num(c) for c in n], [K.num(c) for c in view_d], [K.num(c) for c in p]
    total = [K.num(0.0)] * 3
    reflection = [K.num(0.0)] * 3                                  # reflectionShader (Shading.fs:89-98)
    if K.branch("reflectance > 0", mat.reflectance > 0.0):
        seen = bounce(reflect(K, n, view_d)) if bounce else [K.num(0.0)] * 3
        reflection = [K.mul(c, K.num(mat.reflectance)) for c in seen]
    shadow_origin = [K.add(a, K.mul(K.num(0.0001), b)) for a, b in zip(p, n)]       # Shading.fs:111
    for light in lights:
        if light.kind == "point":                                  # shadowLightIntensity (Shading.fs:38-42), lightDirection (Shading.fs:48)
            pos = [K.num(c) for c in light.v]
            d = [K.sub(a, b) for a, b in zip(pos, shadow_origin)]
            distance = K.site(K.sqrt(K.dot(d, d)))
            towards = normalise(K, d, "shadow ray")
            shut = False
            for height in planes:
                shut = shut or plane_in_the_way(K, shadow_origin, towards, distance, height)
            if light.occluder is not None and not shut:
                shut = square_in_the_way(K, shadow_origin, towards, light.occluder, distance)
            intensity = K.num(0.0) if shut else attenuate(K, light.falloff, distance)
            light_dir = normalise(K, [K.sub(a, b) for a, b in zip(p, pos)], "lightDirection")
        else:                                                      # Shading.fs:36 and 46
            light_dir = [K.num(c) for c in light.v]
            if light.occluder is None:
                shut = plane_blocked([c / scale for c in light.v])  # (the shadow ray in the plane's own frame; a power of two here)
            else:
                shut = square_in_the_way(K, shadow_origin, vneg(K, light_dir), light.occluder, K.num(1.7976931348623157e308))
            intensity = K.num(0.0 if shut else 1.0)
        light_colour = [K.mul(intensity, K.num(c)) for c in light.colour]   # scaleColour intensity colour (Shading.fs:116)
        spec = specular_shader(K, n, view_d, mat, light_colour, light_dir)
        if K.branch("roughness = 0", mat.roughness == 0.0):        # diffuseShader (Shading.fs:72-76)
            diff = lambertian_diffuse(K, n, mat, light_colour, light_dir)
        else:
            diff = rough_diffuse(K, n, view_d, mat, light_dir)
        fragment = [K.add(K.add(K.add(K.num(0.0), s), r), d) for s, r, d in zip(spec, reflection, diff)]
        for c in range(3):
            for part in (spec[c], reflection[c], diff[c]):
                K.parts[c] += abs(float(part)) if part == part else 0.0
        total = [K.add(t, f) for t, f in zip(total, fragment)]
    return total


# ---- cases ------------------------------------------------------------------------------------------------------------------------------

Material = namedtuple("Material", "colour roughness reflectance shineyness", defaults=((0.0, 0.0, 0.0), 0.0, 0.0, 0.0))
# A light as the scene is given it: kind "directional" (v: its direction, before Light.directional normalises it) or "point" (v: its position);
# occluder: None, or the height over the receiver's point of a lit unit square around the shadow ray
Light = namedtuple("Light", "kind v colour falloff occluder", defaults=((1.0, 0.0, 0.0), None))
# lights: `Light`s, or (direction, colour) pairs for plain directional ones; p: the hit point where a light's position or an occluder asks for it
# ladder: the name of the ladder the case is a rung of (None: a single point); side: -1 / 0 / +1 of the ladder's point; watch: the
# decision the ladder walks across (None: a ladder over a value, not over a branch)
# above: what lies over the receiver at y = 2 - None, ("unlit", colour): a plane that ignores light, or ("mirror",): a lit plane of the
# receiver's own material, normal (0, 1, 0), or ("self",): nothing - the reflected ray meets the receiver again (a plane under a scale of
# 2^24 and more, below); depth: getColourForRay's recursion limit
# n: the hit's normal; scale: the uniform scale the receiving plane sits under (its normal is then normalise((0, 1 / scale, 0)): Transform.fs:86)
Case = namedtuple("Case", "name o d mat lights tile ladder side watch p above depth n scale",
                  defaults=(0, None, 0, None, (0.0, 0.0, 0.0), None, 8, (0.0, 1.0, 0.0), 1.0))
CEILING = 2.0
Verdict = namedtuple("Verdict", "colour bound branches kept differs base")


def as_lights(lights):
    return [l if isinstance(l, Light) else Light("directional", l[0], l[1]) for l in lights]


def shadow_query(light, p=(0.0, 0.0, 0.0), n=(0.0, 1.0, 0.0)):
    """(origin, direction, maxDistance) of the light's shadow ray from the hit (p, n) in binary64 (Shading.fs:111, 33-42): what `blocked` is asked."""
    K = Binary64()
    origin = [a + 0.0001 * b for a, b in zip(p, n)]
    if light.kind == "point":
        d = [a - b for a, b in zip(light.v, origin)]
        return origin, normalise(K, d, "shadow ray"), K.sqrt(K.dot(d, d))
    return origin, [-c for c in stored_direction(light.v)], 1.7976931348623157e308


def in_the_way(verdict):
    """Whether exact arithmetic finds a light of the case blocked by the receiver or the square over it."""
    return any(taken for name, taken in verdict.branches if name.endswith("is in the way"))


def stored_direction(v):
    """Light.directional (Light.fs:19-20): the direction a light stores, normalised once in binary64 when the scene is built."""
    return tuple(normalise(Binary64(), [float(c) for c in v], "light"))


def plane_hit(o, d, scale=1.0):
    """Plane.fs:9-20 for the plane y = 0 after slightOffset (Shading.fs:129), and Scene.closest (Scene.fs:112-116): whether the ray has a
    hit, and whether that is the hit of a parallel ray (t = 0, p the ray's own origin).  scale: a power of two the plane sits under - the
    ray is tested in the plane's frame, where it is 1 / scale as long."""
    oy, dy = (o[1] + 0.0001 * d[1]) / scale, d[1] / scale
    if abs(dy) < EPS:
        return (0.0 - oy) < EPS, True
    return (0.0 - oy) / dy >= 0.0, False


def plane_blocked(direction):
    """lightIsBocked (Scene.fs:119-121) for the shadow ray of a directional light from 1e-4 above the plane y = 0, which is the only thing
    in its way: parallel within 1e-7 it meets the plane at its own origin (t = 0 counts), from below at t > 0."""
    return direction[1] > -EPS


def evaluate(case):
    """The exact colour, the bound per channel, and whether binary64 takes the same decisions.  Where it does not, colour and bound are
    those of exact arithmetic made to take binary64's decisions: what such a case is compared with, against the oracle."""
    lights = as_lights(case.lights)
    lights = [l._replace(v=stored_direction(l.v)) if l.kind == "directional" else l for l in lights]
    n = case.n
    def seen_from(K, where, direction, limit):
        """getColourForDirection (Shading.fs:132-134) along the y axis between the floor (where = 0) and what lies above it (1)."""
        if limit <= 0:
            return [K.num(0.0)] * 3
        if case.above[0] == "self":                                 # the same plane, met at the reflected ray's own origin (Plane.fs:14-16)
            return shade(K, n, direction, case.mat, lights, case.p, lambda d: seen_from(K, 1, d, limit - 1), scale=case.scale)
        if where == 1 and case.above[0] == "unlit":                 # shadeIfRequired (Shading.fs:100-104): the colour once per fragment
            total = [K.num(0.0)] * 3
            for _ in lights:
                total = [K.add(t, K.num(c)) for t, c in zip(total, case.above[1])]
            return total
        here = (0.0, CEILING * where, 0.0)
        return shade(K, n, direction, case.mat, lights, here, lambda d: seen_from(K, 1 - where, d, limit - 1), (CEILING * where, CEILING * (1 - where)))
    bounce = (lambda K: None) if case.above is None else (lambda K: (lambda d: seen_from(K, 1, d, case.depth)))
    planes = (0.0,) if case.above is None else (0.0, CEILING)
    run = lambda K: ([float(c) for c in shade(K, n, case.d, case.mat, lights, case.p, bounce(K), planes, case.scale)], K)
    colour, K0 = run(Exact())
    _, Kf = run(Binary64())
    kept = K0.branches == Kf.branches
    forced = None if kept else Kf.branches
    if not kept:
        colour, K0 = run(Exact(forced=forced))
    bound = [SUM_SLACK * p for p in K0.parts]
    if any(math.isfinite(c) for c in colour):                       # (a channel that is NaN or inf is compared by its class alone)
        for site in range(K0.sites):
            moved = [run(Exact(site, sign, forced))[0] for sign in (1, -1)]
            for c in range(3):
                steps = [abs(m[c] - colour[c]) for m in moved if math.isfinite(m[c])]
                bound[c] = bound[c] + max(steps) if steps else INF
    differs = getattr(K0, "differs", False)                       # under any of the lights
    return Verdict(colour, bound, K0.branches, kept, differs, float(getattr(K0, "base", NAN)))


def classes(colour):
    """Per channel 'nan', '+inf', '-inf' or 'finite'."""
    return ["nan" if c != c else ("+inf" if c == INF else ("-inf" if c == -INF else "finite")) for c in colour]


def error_ratio(got, verdict):
    """The largest |got - exact| / bound over the channels (0 where both vanish); the classes must agree first."""
    worst = 0.0
    for g, c, b in zip(got, verdict.colour, verdict.bound):
        if not math.isfinite(c):
            continue
        e = abs(float(g) - c)
        worst = max(worst, 0.0 if e == 0.0 else (INF if b == 0.0 else e / b))
    return worst


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------

TILE_STEP = 2.0
FAR_ROUGH = ((0.0, -50.0, 1.0e6), 0.5)                              # a never-hit sphere with roughness 0.5: its scene takes the FANCY kernels


def tile_centre(k):
    return (TILE_STEP * (k % 8) + 0.5, 0.0, TILE_STEP * (k // 8) + 0.5)


def build_scene(b, mats, lights, tiles=False, fancy=False, above=None, scale=1.0):
    """The plane y = 0 under mats[0], or unit squares at y = 0 (tile k: x from 2 (k % 8), z from 2 (k // 8)) under one material each."""
    b.clear()
    as_args = lambda m: dict(colour=m.colour, roughness=m.roughness, reflectance=m.reflectance, shineyness=m.shineyness)
    if tiles:
        objs = []
        for k, m in enumerate(mats):
            x, _, z = tile_centre(k)
            sq = b.primitive(ft.SQUARE)
            if k:
                sq = b.translate((x - 0.5, 0.0, z - 0.5), sq)
            objs.append(b.material(sq, **as_args(m)))
    else:
        plane = b.primitive(ft.PLANE) if scale == 1.0 else b.transform([("scale", (scale, scale, scale))], b.primitive(ft.PLANE))
        objs = [b.material(plane, **as_args(mats[0]))]
    if above is not None and above[0] != "self":
        over = b.translate((0.0, CEILING, 0.0), b.primitive(ft.PLANE))
        objs.append(b.ignore_light(b.material(over, colour=above[1])) if above[0] == "unlit" else b.material(over, **as_args(mats[0])))
    if fancy:
        objs.append(b.material(b.translate(FAR_ROUGH[0], b.primitive(ft.SPHERE)), colour=(1, 1, 1), roughness=FAR_ROUGH[1]))
    lights = as_lights(lights)
    for l in lights:
        if l.occluder is not None:                                 # a lit unit square over the origin, the receiver's point in such cases
            objs.append(b.material(b.translate((-0.5, l.occluder, -0.5), b.primitive(ft.SQUARE)), colour=(1, 1, 1)))
    b.set_objects(b.group(objs))
    for l in lights:
        if l.kind == "point":
            b.add_positional(l.v, l.falloff, l.colour)
        else:
            b.add_directional(l.v, l.colour)
    b.commit()


def ray_onto(target, d, back=1.0):
    """A ray along d that reaches `target` at about t = back (after the 1e-4 of slightOffset)."""
    return [float(t - (back + 0.0001) * c) for t, c in zip(target, d)], [float(c) for c in d]


def parallel_ray(target, d):
    """A ray whose d.y is within 1e-7 of 0: Plane.fs:14-16 reports its own (offset) origin, half a unit above `target`, as the hit."""
    return [float(target[0] - 0.0001 * d[0]), 0.5, float(target[2] - 0.0001 * d[2])], [float(c) for c in d]


def aimed(target, d):
    """The ray for direction d at a tile or plane point: parallel rule where it applies, else from the side of the plane d comes from."""
    if abs(d[1]) < EPS:
        return parallel_ray(target, d)
    return ray_onto(target, d, back=1.0 / abs(d[1]))


K_RUNGS = (52, 51, 50, 48, 44, 40, 34, 28, 24, 23, 20, 16, 12, 10)
K_FEW = (52, 51, 46, 40, 30, 20, 10)
K_C = (52, 51, 46, 40, 30, 24, 23, 16, 10)
A_LIGHT = ((1.0, -2.0, 2.0), (1.0, 0.5, 0.25))                      # lattice: |(1, -2, 2)| = 3
SHINE_ONE = Material(shineyness=1.0)


def group_a():
    """normalise through the specular term: black diffuse colour, shineyness 1, so the colour is lightColour * (view^ . -reflected^)."""
    light = [A_LIGHT]
    cases = []
    def add(name, d, ladder=None, side=0, watch=None):
        o, d = aimed((0.0, 0.0, 0.0), d)
        cases.append(Case(name, o, d, SHINE_ONE, light, 0, ladder, side, watch))
    for axis, unit in (("-y", (0.0, -1.0, 0.0)), ("-x", (-1.0, 0.0, 0.0)), ("-z", (0.0, 0.0, -1.0))):
        ladder = f"|d| across 1e-7 along {axis}"
        add(f"{ladder}: on", [EPS * c for c in unit], ladder, 0, "specular view: |v| < 1e-7")
        for k in K_RUNGS:
            for s in (1, -1):
                m = EPS * (1.0 + s * 2.0 ** -k)
                add(f"{ladder}: {'+' if s > 0 else '-'}2^-{k}", [m * c for c in unit], ladder, s, "specular view: |v| < 1e-7")
    for m in (1e-150, 1e-160, 1e150 * (1.0 - 2.0 ** -20), 1e150, 1e150 * (1.0 + 2.0 ** -20), 1e155):
        for unit in ((-1.0, 0.0, 0.0), (0.0, 0.0, -1.0), (-3.0, 0.0, -4.0)):
            add(f"|d| = {m!r} along {unit}", [m * c for c in unit])
    for unit in ((-1.0, -2.0, -2.0), (-3.0, -4.0, 0.0), (-1.0, -1.0, -1.0), (-0.3, -1.0, -0.2), (0.7, -0.1, 0.4), (-5.0, -1.0, -7.0), (-3.0, 0.0, -4.0), (-1.0, 0.0, -1.0)):
        for m in (1.0, 0.37, 3.0, 1e-3, 1e5):
            add(f"|d|: {m!r} x {unit}", [m * c for c in unit])
    return cases


WHOLE = (1.0, 2.0, 3.0, 31.0, 32.0, 63.0, 64.0)
POW = (65.0, 1e3, 2.5, 0.5, 2.0 ** -1074, 1e-300, 1e300, INF)
BLACK = (0.0, -0.0, -1.0, -2.5, -INF)
EXPONENTS = WHOLE + POW + BLACK + (NAN,)
LEAN_EXPONENTS = WHOLE + (0.0, -0.0, -1.0, -2.5, -INF)             # what a scene may hold and still run the lean kernels (ft_capi.cpp:62)
B_LIGHT = ((0.0, -1.0, 0.0), (1.0, 0.5, 0.25))                      # straight down: reflected is (0, 1, 0) exactly and the base is -view^.y


def base_directions():
    """(name, d, ladder, side): view directions whose base -d.y / |d| is the wanted one, computed at 60 digits and rounded."""
    out = [("base 1", (0.0, -1.0, 0.0), "base 1 - 2^-k", 0), ("base 0", (1.0, 0.0, 0.0), "base 0 +- 2^-k", 0), ("base -0.5", (float(mpmath.sqrt(3)), 1.0, 0.0), None, 0)]
    for k in K_FEW:
        c = 1 - mpf(2) ** -k
        s = float(mpmath.sqrt(1 - c * c))
        out.append((f"base 1 - 2^-{k}", (s, -float(c), 0.0), "base 1 - 2^-k", -1))
        out.append((f"base -1 + 2^-{k}", (s, float(c), 0.0), "base -1 + 2^-k", 1))
        out.append((f"base +2^-{k}", (1.0, -(2.0 ** -k), 0.0), "base 0 +- 2^-k", 1))
        out.append((f"base -2^-{k}", (1.0, 2.0 ** -k, 0.0), "base 0 +- 2^-k", -1))
    return out


def group_b(exponents=EXPONENTS):
    """The routes of `**`: tile k holds exponent k; every base on every tile."""
    light = [B_LIGHT]
    mats = [Material(shineyness=e) for e in exponents]
    cases = []
    for k, m in enumerate(mats):
        for name, d, ladder, side in base_directions():
            o, d = aimed(tile_centre(k), d)
            cases.append(Case(f"{name} ** {m.shineyness!r}", o, d, m, light, k, f"{ladder}, ** {m.shineyness!r}" if ladder else None, side))
    return mats, cases


WAVE_VIEW = (0.3, -1.0, 0.2)


def wave_materials():
    """64 materials: every exponent class, with roughness zero and not."""
    mats = []
    for k in range(64):
        e = EXPONENTS[k % len(EXPONENTS)]
        rough = (0.0, 0.5, 1.0, 0.25)[k // len(EXPONENTS)]
        mats.append(Material((0.8, 0.6, 0.4), rough, 0.0, e))
    return mats


def wave_rays(order):
    o, d = zip(*(ray_onto(tile_centre(k), WAVE_VIEW) for k in order))
    return np.array(o), np.array(d)


C_COLOUR = (0.8, 0.6, 0.4)
ROUGH = Material(C_COLOUR, 0.5, 0.0, 0.0)
C_VIEW = (0.3, -1.0, 0.2)
C_LIGHT = (1.0, -2.0, 2.0)
ROUGHNESSES = (2.0 ** -1074, 1e-160, 1e-8, 0.5, 1.0, 1e150, 1e200, -0.5, NAN)
WHITE = (1.0, 1.0, 1.0)


def group_c():
    """Oren-Nayar at its singular points.  Returns the cases; a scene is one (material, lights) pair (`scenes_of`)."""
    cases = []
    def add(name, d, light_dir, mat=ROUGH, ladder=None, side=0, watch=None, colour=WHITE):
        o, d = aimed((0.0, 0.0, 0.0), d)
        cases.append(Case(name, o, d, mat, [(light_dir, colour)], 0, ladder, side, watch))
    down = (0.0, -1.0, 0.0)
    add("view along the normal", down, C_LIGHT)
    add("light along the normal", C_VIEW, down)
    add("view and light along the normal", down, down)
    add("a light that is not white", C_VIEW, C_LIGHT, colour=(0.2, 0.7, 0.1))
    add("light in the surface's plane", C_VIEW, (-1.0, 0.0, 0.0), ladder="light elevation across the horizon")
    for k in K_C:
        e = 2.0 ** -k
        add(f"light elevation +2^-{k}", C_VIEW, (-1.0, -e, 0.0), ladder="light elevation across the horizon", side=1)
        add(f"light elevation -2^-{k}", C_VIEW, (-1.0, e, 0.0), ladder="light elevation across the horizon", side=-1)
        add(f"view elevation 2^-{k}", (1.0, -e, 0.25), C_LIGHT, ladder="view elevation towards grazing", side=1)
        add(f"azimuth pi/2 - 2^-{k}", (-e, -1.0, 1.0), (1.0, -1.0, 0.0), ladder="azimuth around pi/2", side=1, watch="max 0.0 clamps")
        add(f"azimuth pi/2 + 2^-{k}", (e, -1.0, 1.0), (1.0, -1.0, 0.0), ladder="azimuth around pi/2", side=-1, watch="max 0.0 clamps")
        for s in (1, -1):
            t = EPS * (1.0 + s * 2.0 ** -k)
            add(f"|tangentLight| 1e-7 (1 {'+' if s > 0 else '-'} 2^-{k})", C_VIEW, (-t, -1.0, 0.0), ladder="|tangentLight| across 1e-7", side=s, watch="tangentLight: |v| < 1e-7")
    add("azimuth 0", (1.0, -1.0, 0.0), (1.0, -1.0, 0.0))
    add("azimuth pi/2", (0.0, -1.0, 1.0), (1.0, -1.0, 0.0), ladder="azimuth around pi/2", watch="max 0.0 clamps")
    add("azimuth pi", (-1.0, -1.0, 0.0), (1.0, -1.0, 0.0))
    for r in ROUGHNESSES:
        for d in (C_VIEW, down, (1.0, -1.0, 0.0)):
            add(f"roughness {r!r}, view {d}", d, C_LIGHT, mat=Material(C_COLOUR, r, 0.0, 0.0))
    return cases


OFFSET = 0.0001                                                     # Shading.fs:111
D_WHITE = Material((1.0, 1.0, 1.0))
D_COLOUR = (1.0, 0.5, 0.25)
GRAZING = ([-(2.0 ** 20), 1.0, 0.0], [1.0, -(2.0 ** -20), 0.0])      # meets y = 0 at x ~ 0 with p.y = 0 exactly: t = o'.y * 2^20, and stays under 1e-4 only beyond x = -104
FROM_BELOW = ([0.0, -1.0, 0.0], [0.0, 1.0, 0.0])                      # p = (0, 0, 0) exactly; the plane's normal is not turned towards the ray


def exact_height(h):
    """A light height h' near h whose shadow ray from (0, 1e-4, 0) has a direction of exactly (0, 1, 0) in binary64 (fl(fl(1 / l) * l) == 1
    for l = fl(h' - 1e-4)): then t along the ray is a height difference on both sides and a blocker AT the light's distance is a tie."""
    for k in range(64):
        l = h + k * 2.0 ** -40 - OFFSET
        if (1.0 / l) * l == 1.0:
            return h + k * 2.0 ** -40
    raise AssertionError(h)


def group_d():
    """Visibility: the 1e-4 offset and the point light's segment.  Every receiver point is (0, 0, 0) (GRAZING: to within 2^-32 in x, which
    nothing here reads) on the plane y = 0; the closed forms are `square_in_the_way` and `attenuate`, evaluated by `shade` itself."""
    cases = []
    def add(name, light, rays=(GRAZING, FROM_BELOW), ladder=None, side=0, watch=None):
        for (o, d), how in zip(rays, ("normal towards the ray", "normal away from the ray") if len(rays) == 2 else ("normal away from the ray",)):
            cases.append(Case(f"{name}, {how}", list(o), list(d), D_WHITE, [light], 0, f"{ladder}, {how}" if ladder else None, side, watch))
    rungs = [(0, "1e-4", OFFSET)] + [(s, f"1e-4 (1 {'+' if s > 0 else '-'} 2^-{k})", OFFSET * (1.0 + s * 2.0 ** -k)) for k in K_RUNGS for s in (1, -1)]
    for side, name, h in rungs:                                    # below the offset origin the square cannot block; at it (t = 0) and above it does
        add(f"occluder at {name} under a directional light", Light("directional", (0.0, -1.0, 0.0), D_COLOUR, occluder=h),
            ladder="occluder height across 1e-4", side=side, watch="the square is in the way")
    H = exact_height(2.0)
    few = [(0, "H", 1.0)] + [(s, f"H (1 {'+' if s > 0 else '-'} 2^-{k})", 1.0 + s * 2.0 ** -k) for k in K_FEW for s in (1, -1)]
    for side, name, f in few:                                      # Shading.fs:41 through Scene.fs:121: t < distance, so a blocker at the light's own height is none
        add(f"blocker at {name} under a point light at H", Light("point", (0.0, H, 0.0), D_COLOUR, (0.0, 0.0, 1.0), H * f), (FROM_BELOW,),
            "blocker distance across the light's", -side, "the square is in the way")
    # The light 2^-k over and under the offset origin (under it: between it and the surface, where L comes from p and the distance from
    # p + 1e-4 n, and the plane lies behind the light).  From 2^-24 on normalise leaves the shadow ray 1e-7 short and the plane's parallel rule
    # blocks it at t = 0.
    for k in (14, 16, 20, 22, 23, 24, 25, 30, 40, 52):
        for s in (1, -1):
            for falloff in ((0.0, 0.0, 1.0), (0.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.5, 0.25, 2.0)):
                add(f"point light at 1e-4 {'+' if s > 0 else '-'} 2^-{k}, falloff {falloff}", Light("point", (0.0, OFFSET + s * 2.0 ** -k, 0.0), (1.0, 0.5, 0.0), falloff),
                    (FROM_BELOW,), f"the light {'over' if s > 0 else 'under'} the offset origin, falloff {falloff}", 1 if k <= 23 else -1, "shadow ray: |v| < 1e-7")
    # The light ON the offset origin: a zero shadow ray of length 0.  The plane's parallel rule answers t = 0, which is not < 0: lit, by 1 / c.
    # (trace<true, ...> takes the light's record only into bundle_cull_to_light, which steps aside for directions that are not unit; no
    # loop's trip count reads the direction: the case runs on the device as well.)
    add("point light on the offset origin", Light("point", (0.0, OFFSET, 0.0), (1.0, 0.5, 0.0), (0.5, 0.25, 2.0)), (FROM_BELOW,))
    d = exact_height(1.0 + OFFSET) - OFFSET                        # the denominator -1 + dist^2 crosses 0 where the distance crosses 1
    for side, name, f in few[1:]:
        add(f"point light at distance 1{name[1:]}, falloff (-1, 0, 1)", Light("point", (0.0, d * f + OFFSET, 0.0), D_COLOUR, (-1.0, 0.0, 1.0)), (FROM_BELOW,),
            "attenuation's denominator across 0", side)
    return cases


F_COLOUR = (0.5, 0.25, 1.0)
F_SEEN = (0.25, 0.5, 0.125)
F_LIGHTS = [((0.0, -1.0, 0.0), (1.0, 0.5, 0.25)), ((1.0, -2.0, 2.0), (0.25, 1.0, 0.5)), ((-2.0, -2.0, 1.0), (0.5, 0.125, 1.0))]
F_VIEW = ([0.0, 1.0, 0.0], [0.0, -1.0, 0.0])                       # p = (0, 0, 0) and the reflected direction (0, 1, 0), exactly


def group_f():
    """The reflection weight.  A mirror floor under an unlit plane (every fragment of the floor adds reflectance x the L fragments of that
    plane), under an open sky (reflectance x black), and the corridor of two planes of reflectance 0.5 around a point light."""
    cases = []
    for r in (2.0 ** -1074, 1e-300, 1.0, 2.0, INF, -0.0, -1.0, NAN):
        for count in (1, 2, 3):
            for depth in ((0, 1, 8) if r in (1.0, INF) else (8,)):
                cases.append(Case(f"reflectance {r!r}, {count} lights, unlit plane above, depth {depth}", *F_VIEW, Material(F_COLOUR, 0.0, r, 0.0), F_LIGHTS[:count],
                                  above=("unlit", F_SEEN), depth=depth))
        cases.append(Case(f"reflectance {r!r}, 2 lights, open sky", *F_VIEW, Material(F_COLOUR, 0.0, r, 0.0), F_LIGHTS[:2]))
    for depth in (0, 8):                                           # no light, no fragment (Shading.fs:119-127): Colour.Zero, whatever would reflect
        cases.append(Case(f"reflectance inf, no light, unlit plane above, depth {depth}", *F_VIEW, Material(F_COLOUR, 0.0, INF, 0.0), [], above=("unlit", F_SEEN), depth=depth))
    cases.append(Case("reflectance inf, no light, open sky", *F_VIEW, Material(F_COLOUR, 0.0, INF, 0.0), []))
    lamp = Light("point", (0.0, 1.0, 0.0), (0.8, 0.6, 0.4), (1.0, 0.0, 0.0))
    for depth in (0, 1, 2, 8):
        cases.append(Case(f"two facing planes of reflectance 0.5, depth {depth}", [0.0, 1.5, 0.0], [0.0, -1.0, 0.0], Material(F_COLOUR, 0.0, 0.5, 0.0), [lamp],
                          above=("mirror",), depth=depth))
    return cases


SCALES = (2.0 ** 23, 2.0 ** 24, 2.0 ** 27)                             # 1 / scale: 1.19e-7 (normalised to a unit normal), 5.96e-8 and 7.45e-9 (returned as they are)
N_VIEWS = ((0.3, -1.0, 0.2), (0.0, -1.0, 0.0), (1.0, -1.0, 0.0), (-3.0, -4.0, 0.0), (1.0, -2.0 ** -10, 0.25))


def group_n():
    """A hit normal on normalise's slow path.  Transform.fs:86 normalises the transformed normal, and under a uniform scale of 2^24 the plane's
    is 2^-24 long and comes back unchanged; every shader then normalises it again and leaves it again, and reflect uses it as it is.  Such a
    plane is met by the parallel rule (Plane.fs:14-16: in its own frame every ray is within 1e-7 of parallel), at the ray's own origin, by
    view rays, shadow rays (so every light is blocked: the specular and Lambert terms see a black light, Oren-Nayar does not look) and
    reflected rays alike: a reflective one is met again by its own reflection until the recursion ends."""
    cases = []
    rough = Material(C_COLOUR, 0.5, 0.0, 1.0)
    for scale in SCALES:
        n = (0.0, 1.0, 0.0) if 1.0 / scale >= EPS else (0.0, 1.0 / scale, 0.0)
        for d in N_VIEWS:
            o, dd = ray_onto((0.0, 0.0, 0.0), d, back=1.0 / abs(d[1]) if abs(d[1]) >= 1e-2 else 1.0)
            o = [o[0], abs(o[1]) if abs(d[1]) >= 1e-2 else 0.5, o[2]]
            cases.append(Case(f"scale 2^{int(math.log2(scale))}, rough, view {d}", o, dd, rough, [(C_LIGHT, WHITE), ((0.0, -1.0, 0.0), (1.0, 0.5, 0.25))], n=n, scale=scale))
            if n[1] != 1.0 and abs(d[1]) / scale < EPS:              # (every level of the reflection met by the parallel rule)
                for depth in (1, 8):
                    cases.append(Case(f"scale 2^{int(math.log2(scale))}, rough mirror, view {d}, depth {depth}", o, dd, Material(C_COLOUR, 0.5, 0.5, 1.0),
                                      [(C_LIGHT, WHITE)], above=("self",), depth=depth, n=n, scale=scale))
    return cases


def group_b_inf():
    """An infinite light colour over the bases around 0: inf * 0 is NaN, so `intensity <= 0` must be decided BEFORE the product
    (Shading.fs:86-87).  The diffuse part is inf, the specular part black or inf: NaN nowhere."""
    light = [(B_LIGHT[0], (INF, 0.5, 0.25))]
    mats = [Material((0.5, 0.5, 0.5), 0.0, 0.0, e) for e in EXPONENTS]
    cases = []
    for k, m in enumerate(mats):
        for name, d, _, _ in base_directions():
            if name in ("base 1", "base 0", "base -0.5", "base +2^-20", "base -2^-20", "base 1 - 2^-20"):
                o, d = aimed(tile_centre(k), d)
                cases.append(Case(f"inf light, {name} ** {m.shineyness!r}", o, d, m, light, k))
    return mats, cases


def scenes_of(cases):
    """[(material, lights, indices of the cases)] in order of first appearance."""
    out = []
    for i, c in enumerate(cases):
        for mat, lights, idx in out:
            if repr((mat, lights) + cases[idx[0]][-4:]) == repr((c.mat, c.lights) + c[-4:]):
                idx.append(i)
                break
        else:
            out.append((c.mat, c.lights, [i]))
    return out


# ---- Jitter.fs:31: how close to 0.9 a binary64 normalise can still be trusted -------------------------------------------------------------

GENERATOR_SWITCH = 0.9


def generator_band(count=100000, seed=9):
    """Directions whose normalised x lies within a few units in the last place of 0.9 (Jitter.fs:28-31: `getX normalised > 0.9` chooses the
    generator): (the widest |exact x^ - 0.9| at which the reference's normalise in binary64 and the exact one fall on different sides, how
    many of `count` did).  The exact side is decided over rationals: x^ > c  <=>  x > 0 and x^2 > c^2 |v|^2."""
    from fractions import Fraction as F
    rng = np.random.default_rng(seed)
    c, K = F(GENERATOR_SWITCH), Binary64()
    widest, flips = 0.0, 0
    for _ in range(count):
        y, z = rng.normal(size=2)
        x = GENERATOR_SWITCH * math.hypot(y, z) / math.sqrt(0.19) * (1.0 + int(rng.integers(-8, 9)) * 2.0 ** -53)
        v = [x, float(y), float(z)]
        K.branches = []
        got = normalise(K, v, "v")[0] > GENERATOR_SWITCH
        X, Y, Z = F(v[0]), F(v[1]), F(v[2])
        if got != (X * X > c * c * (X * X + Y * Y + Z * Z)):
            flips += 1
            exact = mpf(v[0]) / mpmath.sqrt(mpf(v[0]) ** 2 + mpf(v[1]) ** 2 + mpf(v[2]) ** 2)
            widest = max(widest, float(abs(exact - mpf(GENERATOR_SWITCH))))
    return widest, flips


# ---- Jitter.fs on the seeded stream: soft lights and the depth of field ------------------------------------------------------------------
# The stream is DESIGN.md 2's: every draw a pure function of (seed, sample, depth, light, purpose, draw number) through splitmix64's output
# function.  sample is pixel * samples per pixel + sample in a frame and the ray's index in `colour_for_ray` (seed 0); purpose 1 is a soft
# light, 2 the depth of field.  This is the Python of tests/tools/derive_round3_answers.py, carried over two arithmetics.

MASK = (1 << 64) - 1


def sm64(z):
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def stream(seed, sample, depth, light, purpose):
    key = sm64(sm64(sm64(seed ^ sample) ^ ((depth << 32) | (light << 8) | purpose)))
    n = 0
    while True:
        yield (sm64((key + n) & MASK) >> 11) * (1.0 / 9007199254740992.0)
        n += 1


def circle(gen, rims=None):
    """Jitter.circle (Jitter.fs:15-21): rejection from [-1, 1]^2.  2 u - 1 is exact in binary64; rims collects |x^2 + y^2 - 1| of every
    candidate, so that a caller can show no draw was accepted or rejected by a rounding."""
    while True:
        x, y = 2.0 * next(gen) - 1.0, 2.0 * next(gen) - 1.0
        if rims is not None:
            rims.append(abs(x * x + y * y - 1.0))
        if x * x + y * y > 1.0:
            continue
        return x, y


def cross(K, a, b):                                                # CommonTypes.fs:17-18
    return [K.sub(K.mul(a[1], b[2]), K.mul(a[2], b[1])), K.sub(K.mul(b[0], a[2]), K.mul(b[2], a[0])), K.sub(K.mul(a[0], b[1]), K.mul(a[1], b[0]))]


def jitter_frame(K, v, angle):
    """Jitter.jitterVector's frame (Jitter.fs:28-35): (normalised, i, j, maxOffsetMagnitude)."""
    normalised = normalise(K, v, "jitter")
    m = K.tan(K.div(K.num(angle), K.num(2.0)))
    unit_y = K.branch("generator is unitY", normalised[0] > K.num(GENERATOR_SWITCH))
    generator = [K.num(c) for c in ((0.0, 1.0, 0.0) if unit_y else (1.0, 0.0, 0.0))]
    i = normalise(K, cross(K, generator, normalised), "jitter i")
    return normalised, i, cross(K, i, normalised), m


def jittered(K, frame, x, y):
    """Jitter.fs:39: normalised + maxOffsetMagnitude * x * i + maxOffsetMagnitude * y * j |> normalise."""
    normalised, i, j, m = frame
    a, b = K.mul(m, K.num(x)), K.mul(m, K.num(y))
    return normalise(K, [K.add(K.add(n, K.mul(a, p)), K.mul(b, q)) for n, p, q in zip(normalised, i, j)], "jittered")


def soft_directions(K, direction, samples, scatter, seed, sample, depth=0, light=0, rims=None):
    """The shadow-ray directions of softShadowLightIntensity (Shading.fs:24-31) for the light's STORED direction."""
    frame = jitter_frame(K, [K.num(-c) for c in direction], scatter)
    gen = stream(seed, sample, depth, light, 1)
    return [jittered(K, frame, *circle(gen, rims)) for _ in range(samples)]


BALL = ((5.0, 3.0, 3.0), 2.0)                                       # the occluder of the soft-light scenes: centre, radius


def ball_margin(K, origin, d):
    """How far the ray passes from the ball's surface (negative: through it), or None when the ball lies behind the origin or d is 0."""
    to_centre = [K.sub(K.num(c), o) for c, o in zip(BALL[0], origin)]
    dd = K.dot(d, d)
    if dd == 0:
        return None
    along = K.div(K.dot(to_centre, d), dd)
    if along <= 0:
        return None
    off = [K.sub(t, K.mul(along, c)) for t, c in zip(to_centre, d)]
    return K.sub(K.sqrt(K.dot(off, off)), K.num(BALL[1]))


def soft_occluded(K, origin, d):
    """(blocked, distance to the nearest decision) of one shadow ray from `origin` (1e-4 over the plane y = 0) under the ball: the ball, or
    the plane itself - met at t = 0 by a direction within 1e-7 of parallel, at t > 0 by one that points down (Plane.fs:12-20, Scene.fs:121)."""
    eps = K.num(EPS)
    margin = ball_margin(K, origin, d)
    near = abs(K.sub(d[1], eps))                                    # the plane's verdict changes where d.y crosses +1e-7
    if margin is not None:
        near = min(near, abs(margin))
    return (d[1] < eps) or (margin is not None and margin < 0), float(near)


def depth_of_field_ray(K, o, d, focal_length, aperture, seed, sample):
    """ImagePlane.depthOfFieldJitter (Image.fs:91-94, Ray.fs:13-18): shiftOrigin f, jitterDirection (one draw of jitterVector), shiftOrigin -f."""
    o, d, f = [K.num(c) for c in o], [K.num(c) for c in d], K.num(focal_length)
    shifted = [K.add(p, K.mul(f, c)) for p, c in zip(o, d)]
    d1 = jittered(K, jitter_frame(K, d, aperture), *circle(stream(seed, sample, 0, 0, 2)))
    return [K.add(p, K.mul(K.neg(f), c)) for p, c in zip(shifted, d1)], d1
