"""Stage A (ORB keypoints and steered-BRIEF descriptors) stated in vectorised numpy, the rules by which a result is compared with
that statement, and the inputs that tests/test_orb_ref_cpu.py and tests/test_orb_ref_gpu.py share. TEST CODE ONLY, not a test module.

Written from the published algorithm (Rublee et al., "ORB: an efficient alternative to SIFT or SURF", ICCV 2011; FAST-9/16 of
Rosten & Drummond; the Harris corner measure) and from the documented free choices (the header comment of oracle/orb_oracle.c and
include/todhip.h), not from the loops of the C restatement or of the kernels, and it shares no code with either:
  - every integer stage is exact in int64: the FAST score map as a maximum over arcs of a running minimum, the strict 3 x 3
    suppression, the threshold and the border, the cut to 2 n by (score desc, y, x), the 11-bit resize, the 8-bit blur with its two
    roundings, the gradient sums A, B, C, the patch moments (the disc's rows as the constant table DISC_HALF_WIDTH), the mask's rule;
  - every float stage is float64: the Harris response, the angle, the steering and the rotated pattern coordinates;
  - the float32 arithmetic that DEFINES sizes (level sizes, scales, quotas, the resize's sample positions) is float32 here too.
Beside it stand two plain float64 operations the fixed-point ones approximate: bilinear resize and a 7 x 7 Gaussian of sigma 2.

What float32 on the other side may change is bounded by the rules of compare(): u = 2^-24, A, B, C the integer gradient sums,
M = (|A B| + C^2 + 0.04 (A + B)^2) s4 the magnitude of the response's terms.
  positions, size, octave   equal
  response                  |got - ref| <= 20 u M   (3 + 3 + 9 roundings in the three terms, 2 in the subtractions, 8 in s4 and its
                            multiplication: 25 half-ulps of at most M, 12.5 u M, taken as 20)
  angle                     circular difference <= 16 ulp of 360 = 16 * 2^-15 degrees = 4.9e-4 (atan2f, the product with 180 / pi, the
                            wrap; the ROCm documentation states no ulp bound for atan2f that could replace the allowance), in [0, 360)
  descriptor bits           equal, except a bit one of whose four rotated coordinates lies within 2^-14 of a half-integer (the float32
                            chain is within about 300 u = 1.8e-5 of the exact value for |px| + |py| <= 60)
  selection                 the cut to 2 n is exact; inside it the result is the n best by float64 response, ties by (y, x); only a
                            keypoint whose response is within 20 u (M_i + M_j) of one on the other side of the boundary, and whose
                            (A, B, C) differ from that one's, may be swapped (Ref.ambiguous); the returned order has non-increasing
                            response, ties in (y, x) order
"""
import functools

import numpy as np

U = 2.0 ** -24
EDGE = 31                                   # a keypoint is at least this far inside its level
FAST_THRESHOLD = 20
RESPONSE_TOL = 20.0                         # in units of u M
ANGLE_TOL = 16 * 2.0 ** -15                 # degrees
HALF_INTEGER_GUARD = 2.0 ** -14
LEFT_OUT_LIMIT = 0.005                      # share of an input's bits that the guard may leave out
PATTERN_DOMAIN_R2 = 900                     # include/todhip.h at todhip_orb: every pattern point has x^2 + y^2 <= 900

# half-width of row |v| of the radius-15 disc of the intensity centroid, v = 0 .. 15
DISC_HALF_WIDTH = (15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3)
GAUSS_8BIT = (18, 33, 49, 56, 49, 33, 18)   # the blur's documented weights, sum 256
# the 16 pixels of the radius-3 circle, in order around it
CIRCLE = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1),
          (-2, -2), (-1, -3))
HARRIS_K = 0.04
HARRIS_S4 = (1.0 / (4 * 7 * 255)) ** 4

f32 = np.float32


# ------------------------------------------------------------------------------------------ geometry (float32 by definition)
def level_scale(level, scale_factor):
    s = f32(1)
    for _ in range(level):
        s = f32(s * f32(scale_factor))
    return s


def level_size(H, W, level, scale_factor):
    s = level_scale(level, scale_factor)
    return int(np.rint(f32(H) / s)), int(np.rint(f32(W) / s))


def quotas(n_features, n_levels, scale_factor):
    """OpenCV 2.4's geometric split: level l is asked for round(n (1 - q) / (1 - q^L) q^l), the last level for the rest"""
    q = f32(1) / f32(scale_factor)
    want = f32(f32(f32(n_features) * f32(f32(1) - q)) / f32(f32(1) - np.power(q, f32(n_levels), dtype=f32)))
    out = []
    for _ in range(n_levels - 1):
        out.append(int(np.rint(want)))
        want = f32(want * q)
    return out + [max(n_features - sum(out), 0)]


def default_pattern():
    """The built-in pattern as documented: a xorshift32 (13, 17, 5) from 0x9E3779B9 draws x, then y, as s mod 27 - 13 and keeps the
    point when x^2 + y^2 <= 169; 512 points, two per test. -> i8 [256, 4]"""
    s, pts = 0x9E3779B9, []

    def draw():
        nonlocal s
        s ^= (s << 13) & 0xFFFFFFFF
        s ^= s >> 17
        s ^= (s << 5) & 0xFFFFFFFF
        return s % 27 - 13

    while len(pts) < 512:
        x = draw()
        y = draw()
        if x * x + y * y <= 169:
            pts.append((x, y))
    return np.array(pts, np.int8).reshape(256, 4)


# ------------------------------------------------------------------------------------------ resize and blur
def _taps(src_n, dst_n):
    """source indices (clamped) and the 11-bit weight of the second one, from float32 sample positions (i + 0.5) src / dst - 0.5"""
    ratio = f32(src_n) / f32(dst_n)
    pos = (np.arange(dst_n, dtype=f32) + f32(0.5)) * ratio - f32(0.5)
    assert pos.dtype == f32
    i0 = np.floor(pos)
    w = np.rint((pos - i0) * f32(2048)).astype(np.int64)
    i0 = i0.astype(np.int64)
    return np.clip(i0, 0, src_n - 1), np.clip(i0 + 1, 0, src_n - 1), w


def resize_fixed(src, dh, dw):
    """bilinear with 11-bit weights per axis and one rounding: (sum + 2^21) >> 22"""
    s = np.asarray(src, np.int64)
    ya, yb, wy = _taps(s.shape[0], dh)
    xa, xb, wx = _taps(s.shape[1], dw)
    top = s[ya][:, xa] * (2048 - wx) + s[ya][:, xb] * wx
    bot = s[yb][:, xa] * (2048 - wx) + s[yb][:, xb] * wx
    return ((top * (2048 - wy)[:, None] + bot * wy[:, None] + (1 << 21)) >> 22).astype(np.uint8)


def resize_float64(src, dh, dw):
    """plain bilinear interpolation at the exact positions (i + 0.5) src / dst - 0.5, replicate border, no rounding"""
    s = np.asarray(src, np.float64)

    def axis(src_n, dst_n):
        pos = (np.arange(dst_n) + 0.5) * (src_n / dst_n) - 0.5
        i0 = np.floor(pos)
        return np.clip(i0, 0, src_n - 1).astype(int), np.clip(i0 + 1, 0, src_n - 1).astype(int), pos - i0

    ya, yb, ty = axis(s.shape[0], dh)
    xa, xb, tx = axis(s.shape[1], dw)
    top = s[ya][:, xa] * (1 - tx) + s[ya][:, xb] * tx
    bot = s[yb][:, xa] * (1 - tx) + s[yb][:, xb] * tx
    return top * (1 - ty)[:, None] + bot * ty[:, None]


def _conv7(a, weights, axis):
    n = a.shape[axis]
    idx = np.clip(np.arange(n)[:, None] + np.arange(-3, 4)[None, :], 0, n - 1)            # [n, 7], replicate border
    taken = np.take(a, idx, axis=axis)                                                    # axis -> (n, 7)
    return np.tensordot(taken, np.asarray(weights, a.dtype), axes=([axis + 1], [0]))


def blur_fixed(img):
    """rows then columns, each pass rounded to 8 bits: (sum + 128) >> 8"""
    a = np.asarray(img, np.int64)
    a = (_conv7(a, GAUSS_8BIT, 1) + 128) >> 8
    a = (_conv7(a, GAUSS_8BIT, 0) + 128) >> 8
    return a.astype(np.uint8)


def gauss7():
    g = np.exp(-np.arange(-3, 4) ** 2 / (2 * 2.0 ** 2))
    return g / g.sum()


def blur_float64(img):
    """the 7 x 7 separable Gaussian of sigma 2, normalised, replicate border"""
    a = np.asarray(img, np.float64)
    return _conv7(_conv7(a, gauss7(), 1), gauss7(), 0)


# ------------------------------------------------------------------------------------------ detection
def fast_scores(img):
    """FAST-9/16 score of every pixel at least 3 inside the image (0 elsewhere): over the 16 arcs of 9 contiguous circle pixels and
    both polarities, the largest of the arcs' smallest differences to the centre (not below 0)."""
    a = np.asarray(img, np.int64)
    H, W = a.shape
    c = a[3:H - 3, 3:W - 3]
    d = np.stack([a[3 + dy:H - 3 + dy, 3 + dx:W - 3 + dx] - c for dx, dy in CIRCLE])       # [16, h, w]
    best = np.zeros_like(c)
    for sign in (1, -1):
        e = sign * d
        m2 = np.minimum(e, np.roll(e, -1, axis=0))                                         # minimum over i, i + 1
        m4 = np.minimum(m2, np.roll(m2, -2, axis=0))
        m8 = np.minimum(m4, np.roll(m4, -4, axis=0))
        m9 = np.minimum(m8, np.roll(e, -8, axis=0))                                        # over i .. i + 8
        best = np.maximum(best, m9.max(axis=0))
    out = np.zeros((H, W), np.int64)
    out[3:H - 3, 3:W - 3] = best
    return out


def mask_pixel(v, n_level, n_image):
    """the level-0 mask coordinate of level coordinate v: floor((v + 0.5) n_image / n_level), at most n_image - 1. In integers;
    the float32 evaluation agrees while the quotient's distance 1 / (2 n_level) from an integer exceeds its rounding, n_level < 2000."""
    return np.minimum(((2 * np.asarray(v, np.int64) + 1) * n_image) // (2 * n_level), n_image - 1)


def candidates(img, mask=None):
    """(x, y, score) of the corners of one level, sorted by (score desc, y, x): score above the threshold, strictly above its eight
    neighbours, at least EDGE pixels inside, and on an open mask pixel. mask: (level-0 mask, H, W) or None"""
    s = fast_scores(img)
    h, w = s.shape
    ok = s > FAST_THRESHOLD
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                nb = np.full_like(s, np.iinfo(np.int64).max)
                nb[max(-dy, 0):h - max(dy, 0), max(-dx, 0):w - max(dx, 0)] = s[max(dy, 0):h + min(dy, 0), max(dx, 0):w + min(dx, 0)]
                ok &= s > nb
    inside = np.zeros_like(ok)
    inside[EDGE:h - EDGE, EDGE:w - EDGE] = True
    ok &= inside
    y, x = np.nonzero(ok)
    if mask is not None:
        m = np.asarray(mask)
        open_ = m[mask_pixel(y, h, m.shape[0]), mask_pixel(x, w, m.shape[1])] != 0
        y, x = y[open_], x[open_]
    sc = s[y, x]
    order = np.lexsort((x, y, -sc))
    return x[order], y[order], sc[order]


def gradient_sums(img, x, y):
    """A = sum ix^2, B = sum iy^2, C = sum ix iy over the 7 x 7 block, ix and iy the 3 x 3 Sobel differences -> int64 [n, 3]"""
    a = np.asarray(img, np.int64)
    p = lambda dx, dy: a[(y[:, None, None] + np.arange(-3, 4)[None, :, None] + dy), (x[:, None, None] + np.arange(-3, 4)[None, None, :] + dx)]
    ix = 2 * (p(1, 0) - p(-1, 0)) + (p(1, -1) - p(-1, -1)) + (p(1, 1) - p(-1, 1))
    iy = 2 * (p(0, 1) - p(0, -1)) + (p(-1, 1) - p(-1, -1)) + (p(1, 1) - p(1, -1))
    return np.stack([(ix * ix).sum(axis=(1, 2)), (iy * iy).sum(axis=(1, 2)), (ix * iy).sum(axis=(1, 2))], axis=1)


def harris(abc):
    """(response, M) in float64: det - k trace^2 of the gradient matrix, scaled by (1 / (4 * 7 * 255))^4"""
    A, B, C = (abc[:, i].astype(np.float64) for i in range(3))
    tr2 = (A + B) ** 2
    return (A * B - C * C - HARRIS_K * tr2) * HARRIS_S4, (np.abs(A * B) + C * C + HARRIS_K * tr2) * HARRIS_S4


@functools.lru_cache(maxsize=None)
def _disc():
    pts = [(u, v) for v in range(-15, 16) for u in range(-DISC_HALF_WIDTH[abs(v)], DISC_HALF_WIDTH[abs(v)] + 1)]
    return np.array(pts, np.int64)


def moments(img, x, y):
    """(m10, m01) = sum of u I and of v I over the disc, int64 [n] each"""
    d = _disc()
    val = np.asarray(img, np.int64)[y[:, None] + d[None, :, 1], x[:, None] + d[None, :, 0]]
    return (val * d[None, :, 0]).sum(axis=1), (val * d[None, :, 1]).sum(axis=1)


def angle_degrees(m10, m01):
    a = np.degrees(np.arctan2(m01.astype(np.float64), m10.astype(np.float64)))
    return np.where(a < 0, a + 360.0, a)


def describe(blur, x, y, m10, m01, pattern):
    """-> (bits u8 0/1 [n, 256], left_out bool [n, 256]): test t is blur[p0] < blur[p1] at the pattern's points rotated by the patch's
    direction (cos, sin) = (m10, m01) / |m|, (1, 0) without a direction, and rounded half to even; left_out where a rotated coordinate
    is within HALF_INTEGER_GUARD of a half-integer."""
    pat = np.asarray(pattern, np.float64).reshape(256, 4)
    fm10, fm01 = m10.astype(np.float64), m01.astype(np.float64)
    nrm = np.hypot(fm10, fm01)
    safe = np.where(nrm > 0, nrm, 1.0)
    ca = np.where(nrm > 0, fm10 / safe, 1.0)[:, None]
    sa = np.where(nrm > 0, fm01 / safe, 0.0)[:, None]
    b = np.asarray(blur, np.int64)
    vals, left_out = [], np.zeros((len(x), 256), bool)
    for k in (0, 2):
        px, py = pat[None, :, k], pat[None, :, k + 1]
        rx, ry = px * ca - py * sa, px * sa + py * ca
        for r in (rx, ry):
            left_out |= np.abs(r - np.floor(r) - 0.5) < HALF_INTEGER_GUARD
        vals.append(b[y[:, None] + np.rint(ry).astype(np.int64), x[:, None] + np.rint(rx).astype(np.int64)])
    return (vals[0] < vals[1]).astype(np.uint8), left_out


def pack_bits(bits):
    """bit i of byte j = test 8 j + i"""
    return np.packbits(np.asarray(bits, np.uint8), axis=1, bitorder="little")


# ------------------------------------------------------------------------------------------ the whole stage
class Level:
    """One pyramid level's cut to 2 n, described completely, in the order (float64 response desc, y, x). kept[i]: among the n best.
    ambiguous[i]: float32 may move it across the boundary (module docstring, selection)."""

    def __init__(self, level, scale, img, blur, quota, x, y, score, pattern):
        self.level, self.scale, self.img, self.blur, self.quota = level, scale, img, blur, quota
        abc = gradient_sums(img, x, y)
        resp, M = harris(abc)
        order = np.lexsort((x, y, -resp))
        self.x, self.y, self.score, self.abc, self.response, self.M = x[order], y[order], score[order], abc[order], resp[order], M[order]
        n = len(x)
        self.kept = np.arange(n) < quota
        self.m10, self.m01 = moments(img, self.x, self.y)
        self.angle = angle_degrees(self.m10, self.m01)
        self.bits, self.left_out = describe(blur, self.x, self.y, self.m10, self.m01, pattern)
        self.kp_xy = np.stack([self.x.astype(f32) * scale, self.y.astype(f32) * scale], axis=1).astype(f32)
        self.size = f32(31) * scale
        k, d = np.flatnonzero(self.kept), np.flatnonzero(~self.kept)
        self.ambiguous = np.zeros(n, bool)
        if len(k) and len(d):
            close = (self.response[k, None] - self.response[None, d]) <= RESPONSE_TOL * U * (self.M[k, None] + self.M[None, d])
            close &= (self.abc[k, None, :] != self.abc[None, d, :]).any(axis=2)
            self.ambiguous[k] = close.any(axis=1)
            self.ambiguous[d] = close.any(axis=0)

    @property
    def n_kept(self):
        return int(self.kept.sum())


class Ref:
    """levels: the Level of every pyramid level that can hold a keypoint (others yield nothing); images: every level's pixels"""

    def __init__(self, levels, images, n_levels):
        self.levels, self.images, self.n_levels = levels, images, n_levels

    @property
    def n(self):
        return sum(L.n_kept for L in self.levels)

    @property
    def ambiguous(self):
        """[(level, x, y)] of every keypoint the selection rule leaves open"""
        return [(L.level, int(L.x[i]), int(L.y[i])) for L in self.levels for i in np.flatnonzero(L.ambiguous)]

    def left_out_share(self):
        """share of the kept keypoints' bits that the half-integer guard leaves out"""
        lo = [L.left_out[L.kept] for L in self.levels]
        total = sum(a.size for a in lo)
        return (sum(int(a.sum()) for a in lo) / total) if total else 0.0


def orb(gray, n_features, n_levels, scale_factor, pattern=None, mask=None):
    """The stage on one frame. mask: level-0 u8 [H, W] or None. A level of at most 62 pixels either way yields nothing, and the next
    level is still resized from it."""
    img = np.ascontiguousarray(gray, np.uint8)
    H, W = img.shape
    pat = default_pattern() if pattern is None else np.asarray(pattern, np.int8).reshape(256, 4)
    want = quotas(n_features, n_levels, scale_factor)
    levels, images = [], []
    for lvl in range(n_levels):
        h, w = level_size(H, W, lvl, scale_factor)
        if lvl:
            img = resize_fixed(img, h, w) if h and w else np.zeros((h, w), np.uint8)
        images.append(img)
        if h <= 2 * EDGE or w <= 2 * EDGE or want[lvl] == 0:
            continue
        x, y, sc = candidates(img, mask)
        x, y, sc = x[:2 * want[lvl]], y[:2 * want[lvl]], sc[:2 * want[lvl]]
        levels.append(Level(lvl, level_scale(lvl, scale_factor), img, blur_fixed(img), want[lvl], x, y, sc, pat))
    return Ref(levels, images, n_levels)


# ------------------------------------------------------------------------------------------ the comparison rules
def circular(a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) % 360.0
    return np.minimum(d, 360.0 - d)


def compare(got, ref, bits_exact=False):
    """A result (kp_xy f32 [n, 2], aux f32 [n, 4] = size, angle, response, octave, desc u8 [n, 32], ...) against a Ref under the
    module's rules; asserts, and returns the measured figures: dict(n, response_err (in u M), angle_err (degrees), left_out (share of
    the result's bits not compared), rows: for every keypoint (position in ref.levels, index in that Level))."""
    kp, aux, desc = (np.asarray(a) for a in got[:3])
    assert kp.shape == (len(kp), 2) and aux.shape == (len(kp), 4) and desc.shape == (len(kp), 32)
    assert len(kp) == ref.n, (len(kp), ref.n)
    octave = aux[:, 3]
    assert (np.diff(octave) >= 0).all()                                                   # level ascending
    stats = dict(n=len(kp), response_err=0.0, angle_err=0.0, left_out=0.0, rows=[])
    n_left_out, at = 0, 0
    for li, L in enumerate(ref.levels):
        sel = np.flatnonzero(octave == L.level)
        assert len(sel) == L.n_kept, (L.level, len(sel), L.n_kept)
        assert len(sel) == 0 or (sel[0] == at and sel[-1] == at + len(sel) - 1)
        at += len(sel)
        where = {(a.tobytes(), b.tobytes()): i for i, (a, b) in enumerate(L.kp_xy)}
        idx = np.array([where.get((a.tobytes(), b.tobytes()), -1) for a, b in kp[sel]], np.int64)
        assert (idx >= 0).all(), "level %d: a keypoint outside the cut to 2 n" % L.level    # position = level pixel * float32 scale
        assert len(set(idx.tolist())) == len(idx)
        assert (L.kept[idx] | L.ambiguous[idx]).all(), "level %d: a keypoint that is not among the n best" % L.level
        sure = np.flatnonzero(L.kept & ~L.ambiguous)
        assert np.isin(sure, idx).all(), "level %d: one of the n best is missing" % L.level
        assert (aux[sel, 0] == L.size).all()
        r = aux[sel, 2].astype(np.float64)
        err = np.abs(r - L.response[idx]) / (U * np.maximum(L.M[idx], np.finfo(np.float64).tiny))
        assert (np.abs(r - L.response[idx]) <= RESPONSE_TOL * U * L.M[idx]).all(), "level %d: response off by %.2f u M" % (L.level, err.max())
        if len(sel):
            stats["response_err"] = max(stats["response_err"], float(err[L.M[idx] > 0].max(initial=0.0)))
        # the returned order: response non-increasing, equal responses in (y, x) order
        r32, xs, ys = aux[sel, 2], L.x[idx], L.y[idx]
        assert (np.diff(r32) <= 0).all()
        tie = np.diff(r32) == 0
        assert ((np.diff(ys)[tie] > 0) | ((np.diff(ys)[tie] == 0) & (np.diff(xs)[tie] > 0))).all()
        ang = aux[sel, 1].astype(np.float64)
        assert ((ang >= 0) & (ang < 360)).all()
        da = circular(ang, L.angle[idx])
        assert (da <= ANGLE_TOL).all(), "level %d: angle off by %.3g degrees" % (L.level, da.max())
        stats["angle_err"] = max(stats["angle_err"], float(da.max(initial=0.0)))
        bits = np.unpackbits(np.ascontiguousarray(desc[sel]), axis=1, bitorder="little")
        differ = bits != L.bits[idx]
        if bits_exact:
            assert not differ.any()
        assert not (differ & ~L.left_out[idx]).any(), "level %d: %d descriptor bits differ" % (L.level, int((differ & ~L.left_out[idx]).sum()))
        n_left_out += int(L.left_out[idx].sum())
        stats["rows"] += [(li, int(i)) for i in idx]
    assert at == len(kp)                                                                  # no keypoint of a level the reference has not
    stats["left_out"] = n_left_out / (256.0 * len(kp)) if len(kp) else 0.0
    assert stats["left_out"] <= LEFT_OUT_LIMIT
    return stats


def transposition_holds(a, b, ref_a):
    """results a of an image and b of its transpose, nothing cut: the same keypoints at (y, x), bit-equal responses (A and B change
    places, C stays), angles 90 - theta"""
    assert len(a[0]) == len(b[0]) == ref_a.n > 100
    ia = np.lexsort((a[0][:, 1], a[0][:, 0]))
    ib = np.lexsort((b[0][:, 0], b[0][:, 1]))
    assert np.array_equal(a[0][ia], b[0][ib][:, ::-1])
    assert np.array_equal(a[1][ia][:, [0, 2, 3]], b[1][ib][:, [0, 2, 3]])
    d = circular(90.0 - a[1][ia, 1].astype(np.float64), b[1][ib, 1])
    assert d.max() <= ANGLE_TOL
    return float(d.max())


def merge_stats(into, s):
    for k in ("response_err", "angle_err", "left_out"):
        into[k] = max(into.get(k, 0.0), s[k])
    return into


# ------------------------------------------------------------------------------------------ the shared inputs
def rectangles(H=160, W=200, n=400, seed=1, noise=3):
    """n seeded rectangles (value 0 .. 255, sides 2 .. 29) on a background of 100, plus uniform noise of +-noise"""
    rng = np.random.Generator(np.random.PCG64(seed))
    img = np.full((H, W), 100, np.int64)
    for _ in range(n):
        h, w = (int(t) for t in rng.integers(2, 30, 2))
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        img[y:y + h, x:x + w] = int(rng.integers(0, 256))
    img += rng.integers(-noise, noise + 1, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def white_noise(H=100, W=130, seed=2):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (H, W), dtype=np.uint8)


def padded_to(img, H, W, value=100):
    out = np.full((H, W), value, np.uint8)
    out[:img.shape[0], :img.shape[1]] = img
    return out


def two_rectangles_and_a_pixel(H, W, pixel):
    """a mask of two rectangles and one isolated open pixel at `pixel` = (x, y)"""
    m = np.zeros((H, W), np.uint8)
    m[20:90, 25:110] = 255
    m[70:140, 120:180] = 1                                                                # any non-zero value is open
    m[pixel[1], pixel[0]] = 255
    return m


def square_pattern():
    """The built-in pattern with its first rows replaced by points on the 31 x 31 square of cv::ORB patterns and at radius 30: inside
    the domain x^2 + y^2 <= 900, far outside the built-in pattern's radius 13."""
    pat = default_pattern().copy()
    wide = [(15, 15, -15, -15), (-15, 15, 15, -15), (15, -15, 13, 13), (30, 0, 0, -30), (18, 24, -15, 15), (0, -30, 18, 24),
            (-30, 0, 15, 15), (-24, -18, 30, 0)]
    pat[:len(wide)] = np.array(wide, np.int8)
    pat[255] = (0, 30, -18, -24)                                                          # and the table's last row
    assert in_domain(pat)
    return pat


def in_domain(pattern):
    p = np.asarray(pattern, np.int64).reshape(-1, 2)
    return bool(((p * p).sum(axis=1) <= PATTERN_DOMAIN_R2).all())


def bad_patterns():
    """name -> a pattern with one point outside the domain, everything else the built-in one"""
    out = {}
    for name, row, col, pt in (("31_0", 0, 0, (31, 0)), ("22_22", 7, 2, (22, 22)), ("-128_127", 100, 0, (-128, 127)),
                               ("last_row", 255, 2, (0, 31))):
        pat = default_pattern().copy()
        pat[row, col:col + 2] = pt
        assert not in_domain(pat)
        out[name] = pat
    return out


@functools.lru_cache(maxsize=None)
def image(name):
    import orb_inputs as I
    r = rectangles()
    img = {"rect": lambda: r, "rect_T": lambda: np.ascontiguousarray(r.T),
           "rect200": lambda: padded_to(r, 200, 200), "rect200_T": lambda: np.ascontiguousarray(padded_to(r, 200, 200).T),
           "flat200": lambda: np.full((200, 200), 90, np.uint8),
           "rect100": lambda: rectangles(100, 100, 150, seed=5),
           "noise": white_noise, "lattice": lambda: np.ascontiguousarray(I.dot_lattice()[:128, :160]),
           "tiny63": lambda: I.tiny(63, 63), "tiny62x200": lambda: I.tiny(62, 200)}[name]()
    img.setflags(write=False)
    return img


MANY = 5000                                  # above every level's candidate count: nothing is cut

# name -> (image, n_features, n_levels, scale_factor, masked, pattern): every input of the GPU tests (GPU_CASES) and the further ones
# of the CPU tests. tests/test_orb_ref_cpu.py asserts for each that no selection is ambiguous and that the guard leaves out <= 0.5 %.
CASES = {
    "rect_150_1": ("rect", 150, 1, 1.2, False, None),
    "rect_150_3": ("rect", 150, 3, 1.2, False, None),
    "rect_300_3": ("rect", 300, 3, 1.2, False, None),
    "rect_150_4": ("rect", 150, 4, 1.2, False, None),
    "rect_300_4": ("rect", 300, 4, 1.2, False, None),
    "rect_1_1": ("rect", 1, 1, 1.2, False, None),
    "rect_1_3": ("rect", 1, 3, 1.2, False, None),                  # the quotas round to 0, 0 and the rest, 1
    "rect_all_1": ("rect", MANY, 1, 1.2, False, None),
    "rect_T_all_1": ("rect_T", MANY, 1, 1.2, False, None),
    "rect_300_1": ("rect", 300, 1, 1.2, False, None),
    "rect100_x2": ("rect100", 60, 3, 2.0, False, None),            # 100, 50, 25 pixels: the upper levels yield nothing
    "rect_masked": ("rect", 150, 3, 1.2, True, None),
    "rect_square": ("rect", 150, 3, 1.2, False, "square"),
    "rect200": ("rect200", 150, 3, 1.2, False, None),
    "flat200": ("flat200", 150, 3, 1.2, False, None),
    "rect200_T": ("rect200_T", 150, 3, 1.2, False, None),
    "noise": ("noise", 150, 2, 1.2, False, None),
    "lattice": ("lattice", 100, 2, 1.2, False, None),
    "tiny63": ("tiny63", 10, 1, 1.2, False, None),
    "tiny62x200": ("tiny62x200", 10, 1, 1.2, False, None),
}
GPU_CASES = ("rect_150_1", "rect_150_3", "rect_300_4", "rect_1_1", "rect_1_3", "rect_all_1", "rect_T_all_1", "rect100_x2",
             "rect_masked", "rect_square", "rect200", "flat200", "rect200_T")


def case_args(name):
    """-> (image, n_features, n_levels, scale_factor, dict(pattern=, mask=))"""
    img_name, nf, nl, sf, masked, pattern = CASES[name]
    img = image(img_name)
    mask = None
    if masked:
        x, y, _ = candidates(img)
        alone = [(int(a), int(b)) for a, b in zip(x, y) if a >= 120 and b < 60]          # a level-0 corner outside both rectangles
        mask = two_rectangles_and_a_pixel(*img.shape, alone[0])
    return img, nf, nl, sf, dict(pattern=square_pattern() if pattern == "square" else None, mask=mask)


@functools.lru_cache(maxsize=None)
def case_ref(name):
    """the statement's result for a case, computed once and shared"""
    img, nf, nl, sf, kw = case_args(name)
    return orb(img, nf, nl, sf, **kw)
