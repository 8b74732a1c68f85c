"""Plain-numpy references of the three face-crop operations, and the case table their tests share.

Each reference is written from the operation's definition, vectorised over the output grid (a 4K rectangle takes well under a
second), and reads only ``img[y0:y1, x0:x1]`` -- so an implementation that reads one pixel or one row outside the rectangle
disagrees with it wherever the outside differs from the replicated border.

  resize_linear_u8_int  cv2.resize(u8, INTER_LINEAR) as OpenCV's fixed-point path computes it (integers only after the taps)
  resize_linear_f64     the same resampling in exact arithmetic: what the fixed-point path approximates
  crop_area_u8/_std     adaptive average pooling + .byte() (+ fixed_image_standardization), exact integer arithmetic
  crop_aligned_f64      DESIGN.md 8(f)-4's five-point similarity warp, bilinear sample in float64
"""
from __future__ import annotations

import numpy as np

# ---- cv2.resize(face, (80, 80)): INTER_LINEAR on u8 -------------------------------------------------------------------------
COEF_BITS = 11                       # OpenCV's INTER_RESIZE_COEF_BITS: coefficients are multiples of 1/2048
COEF_ONE = 1 << COEF_BITS


def _taps_f32(n_src: int, n_dst: int, horizontal: bool):
    """Source taps of n_dst output samples over n_src input samples: centre (d + 0.5) * scale - 0.5 (f64, then f32), floor,
    weights rounded half-even to 1/2048 as int16, tap indices replicated into the rectangle.  OpenCV treats the two directions
    differently at the border: a COLUMN centre left of sample 0 or at / after the last sample takes that sample alone (weight
    2048 / 0: the two clamps of resize.cpp's x loop), a ROW centre there keeps its fractional weights and only its two row
    indices are clamped -- the same row enters twice, and the two truncating shifts can make it one grey level less than the
    single tap would."""
    scale = 1.0 / (float(n_dst) / float(n_src))
    c = ((np.arange(n_dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(c)
    f = (c - s).astype(np.float32)
    s = s.astype(np.int64)
    if horizontal:
        f[(s < 0) | (s >= n_src - 1)] = np.float32(0)
    w1 = np.clip(np.rint(f * np.float32(COEF_ONE)), -32768, 32767).astype(np.int16)
    w0 = np.clip(np.rint((np.float32(1) - f) * np.float32(COEF_ONE)), -32768, 32767).astype(np.int16)
    return np.clip(s, 0, n_src - 1), np.clip(s + 1, 0, n_src - 1), w0.astype(np.int32), w1.astype(np.int32)


def resize_linear_u8_int(img: np.ndarray, y0: int, y1: int, x0: int, x1: int, oh: int = 80, ow: int = 80) -> np.ndarray:
    """cv2.resize(img[y0:y1, x0:x1], (ow, oh)) with INTER_LINEAR on uint8, u8 (oh, ow, 3): two horizontal taps into int32, then
    (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2, clipped to 0..255."""
    src = img[y0:y1, x0:x1].astype(np.int32)
    sh, sw = src.shape[:2]
    xa, xb, a0, a1 = _taps_f32(sw, ow, True)
    ya, yb, b0, b1 = _taps_f32(sh, oh, False)
    a0, a1 = a0[None, :, None], a1[None, :, None]
    ra, rb = src[ya], src[yb]                                   # (oh, sw, 3): the two source rows of every output row
    r0 = ra[:, xa] * a0 + ra[:, xb] * a1                        # int32 (oh, ow, 3)
    r1 = rb[:, xa] * a0 + rb[:, xb] * a1
    v = (((b0[:, None, None] * (r0 >> 4)) >> 16) + ((b1[:, None, None] * (r1 >> 4)) >> 16) + 2) >> 2
    return np.clip(v, 0, 255).astype(np.uint8)


def _taps_f64(n_src: int, n_dst: int):
    c = (np.arange(n_dst, dtype=np.float64) + 0.5) * (float(n_src) / float(n_dst)) - 0.5
    s = np.floor(c)
    f = c - s
    s = s.astype(np.int64)
    return np.clip(s, 0, n_src - 1), np.clip(s + 1, 0, n_src - 1), f


def resize_linear_f64(img: np.ndarray, y0: int, y1: int, x0: int, x1: int, oh: int = 80, ow: int = 80) -> np.ndarray:
    """Exact bilinear resampling of img[y0:y1, x0:x1] at the half-pixel centres, replicated borders, f64 (oh, ow, 3) in grey
    levels; nothing is rounded."""
    src = img[y0:y1, x0:x1].astype(np.float64)
    sh, sw = src.shape[:2]
    xa, xb, fx = _taps_f64(sw, ow)
    ya, yb, fy = _taps_f64(sh, oh)
    fx, fy = fx[None, :, None], fy[:, None, None]
    ra, rb = src[ya], src[yb]
    top = ra[:, xa] * (1.0 - fx) + ra[:, xb] * fx
    bot = rb[:, xa] * (1.0 - fx) + rb[:, xb] * fx
    return top * (1.0 - fy) + bot * fy


def resize_fixed_point_bound(max_side: int = 4096) -> float:
    """Largest |resize_linear_u8_int - resize_linear_f64| in grey levels for rectangles of up to max_side (<= 4096) px a side,
    term by term (tests/test_crops_cpu.py::test_fixed_point_stays_within_its_derived_bound quotes it):

      e    each of the four weights differs from the exact one by at most 2^-12 (rounding to 1/2048) + 2^-13 (the centre, below
           4096, rounded to f32: half an ulp of 2^-12) + 2^-25 (1 - f in f32);
      h    horizontal pass, per row: two taps of at most 255, so 2 * 255 * e;
      s4   r >> 4 leaves units of 1/128 grey level and drops less than one of them: 1/128;
      v    vertical weights on rows of at most 255 * (1 + 2e): 2 * 255 * (1 + 2e) * e;
      s16  each of the two (b * r) >> 16 drops less than one unit of 1/4 grey level: 2 * 1/4, downwards only;
      rnd  (.. + 2) >> 2 rounds to the nearest grey level: 1/2;
    and the clip to 0..255 moves the value towards the exact one, which lies in [0, 255]."""
    assert max_side <= 4096
    e = 2.0 ** -12 + 2.0 ** -13 + 2.0 ** -25
    h = 2 * 255 * e
    s4 = 1.0 / 128
    v = 2 * 255 * (1 + 2 * e) * e
    s16 = 2 * 0.25
    rnd = 0.5
    return h + s4 + v + s16 + rnd


# ---- extract_face() for tensor input: adaptive average pooling, .byte(), fixed_image_standardization ------------------------
def _bins(n: int, S: int):
    o = np.arange(S, dtype=np.int64)
    return (o * n) // S, -((-(o + 1) * n) // S)                 # floor(o*n/S), ceil((o+1)*n/S)


def crop_area_u8(img: np.ndarray, x0: int, y0: int, x1: int, y1: int, S: int = 160) -> np.ndarray:
    """img[y0:y1, x0:x1] pooled to S x S: output (oy, ox) is the mean over rows [floor(oy*h/S), ceil((oy+1)*h/S)) and columns
    likewise, truncated to a byte -- floor(sum / count) in exact integers, u8 (S, S, 3).

    Why an exact floor may stand for the float32 expression ``(float)sum / kh / kw`` truncated, with no element excluded --
    for bins of at most 16384 pixels (area_floor_is_exact): sum <= 255 * 16384 < 2^24 and the two bin sides are exact in f32,
    and each division rounds once, so the computed mean is within a relative 2 * 2^-24 (+ second order) of sum / count, i.e.
    within 255 * 2^-23 = 3.04e-5 of it.  An exact mean that is an integer k is computed exactly (sum / kh = k * kw and
    k * kw / kw = k are representable, and a correctly rounded division returns a representable quotient).  One that is not an
    integer lies at least 1 / count below the next integer and at least 1 / count above the previous one, and
    1 / count >= 1 / 16384 = 6.1e-5 is twice the rounding error: the truncation cannot land on another integer.  S = 160 is
    far inside: at most 25 x 14 = 350 pixels per bin for a 3840 x 2160 rectangle, 1 / count >= 2.8e-3.  Larger bins (a 4K
    rectangle pooled to 1 x 1 sums to 2e9, which (float) already rounds) are outside the argument, and this function is not
    a reference for them."""
    src = img[y0:y1, x0:x1].astype(np.int64)
    h, w = src.shape[:2]
    ys, ye = _bins(h, S)
    xs, xe = _bins(w, S)
    ii = np.zeros((h + 1, w + 1, 3), np.int64)                  # integral image: bins overlap, so no reduceat
    ii[1:, 1:] = src.cumsum(0).cumsum(1)
    tot = ii[ye][:, xe] - ii[ys][:, xe] - ii[ye][:, xs] + ii[ys][:, xs]
    cnt = ((ye - ys)[:, None] * (xe - xs)[None, :])[..., None]
    return (tot // cnt).astype(np.uint8)


def area_floor_is_exact(h: int, w: int, S: int) -> bool:
    """Whether crop_area_u8's exact floor provably equals the truncated f32 mean for an h x w rectangle pooled to S x S: every
    bin holds at most 16384 pixels (the argument is in crop_area_u8's docstring)."""
    ys, ye = _bins(h, S)
    xs, xe = _bins(w, S)
    return int((ye - ys).max()) * int((xe - xs).max()) <= 16384


def crop_area_std(img: np.ndarray, x0: int, y0: int, x1: int, y1: int, S: int = 160, rgb: bool = False) -> np.ndarray:
    """(crop_area_u8 - 127.5) / 128 in float32 (both steps exact or correctly rounded: bytes and 127.5 are representable, 128 is
    a power of two), channels reversed when rgb."""
    out = (crop_area_u8(img, x0, y0, x1, y1, S).astype(np.float32) - np.float32(127.5)) / np.float32(128.0)
    return np.ascontiguousarray(out[..., ::-1]) if rgb else out


# ---- embedding mode 3: five-point similarity alignment ----------------------------------------------------------------------
# The 112 x 112 five-point template (eyes, nose, mouth corners) scaled to 160 x 160: DESIGN.md 8(f)-4
TEMPLATE_X = (54.706571428571436, 105.04542857142857, 80.036, 59.35614285714286, 101.04271428571428)
TEMPLATE_Y = (73.85185714285714, 73.57342857142856, 102.48085714285713, 131.9507142857143, 131.72014285714286)


def align_params(pts) -> tuple:
    """(a, b, tx, ty, px, py) of the least-squares similarity that maps template coordinates to frame coordinates,
    x = a (u - tx) - b (v - ty) + px,  y = b (u - tx) + a (v - ty) + py:  d_j = T_j - mean T,  e_j = P_j - mean P,
    a = sum d.e / sum |d|^2,  b = sum (dx ey - dy ex) / sum |d|^2, accumulated in point order in float64."""
    p = np.asarray(pts, np.float32).reshape(10).astype(np.float64)
    tx = ty = px = py = np.float64(0)
    for j in range(5):
        tx = tx + TEMPLATE_X[j]; ty = ty + TEMPLATE_Y[j]; px = px + p[j]; py = py + p[5 + j]
    tx, ty, px, py = tx / 5.0, ty / 5.0, px / 5.0, py / 5.0
    sdd = sde = scr = np.float64(0)
    for j in range(5):
        dx, dy, ex, ey = TEMPLATE_X[j] - tx, TEMPLATE_Y[j] - ty, p[j] - px, p[5 + j] - py
        sdd = sdd + (dx * dx + dy * dy)
        sde = sde + (dx * ex + dy * ey)
        scr = scr + (dx * ey - dy * ex)
    with np.errstate(all="ignore"):
        return sde / sdd, scr / sdd, tx, ty, px, py


def _floor_index(c: np.ndarray, n: int):
    """floor(c) and floor(c) + 1 as indices replicated into [0, n - 1]; a NaN coordinate takes index 0 (its weight stays NaN)."""
    with np.errstate(all="ignore"):
        f = np.floor(c)
        f = np.where(f >= -1.0, np.minimum(f, float(n)), -1.0).astype(np.int64)
    return np.clip(f, 0, n - 1), np.clip(f + 1, 0, n - 1)


def crop_aligned_f64(img: np.ndarray, pts, S: int = 160, rgb: bool = True) -> np.ndarray:
    """The S x S aligned crop in float64: output (v, u) samples the frame bilinearly at the similarity image of (u, v), borders
    replicated, then (value - 127.5) / 128; channels reversed when rgb.  f64 (S, S, 3)."""
    H, W = img.shape[:2]
    a, b, tx, ty, px, py = align_params(pts)
    with np.errstate(all="ignore"):
        du = (np.arange(S, dtype=np.float64) - tx)[None, :]
        dv = (np.arange(S, dtype=np.float64) - ty)[:, None]
        x = (a * du - b * dv) + px
        y = (b * du + a * dv) + py
        fx, fy = (x - np.floor(x))[..., None], (y - np.floor(y))[..., None]
        xa, xb = _floor_index(x, W)
        ya, yb = _floor_index(y, H)
        src = img.astype(np.float64)
        top = src[ya, xa] + fx * (src[ya, xb] - src[ya, xa])
        bot = src[yb, xa] + fx * (src[yb, xb] - src[yb, xa])
        out = ((top + fy * (bot - top)) - 127.5) / 128.0
    return np.ascontiguousarray(out[..., ::-1]) if rgb else out


def aligned_f32_bound() -> float:
    """Largest |f32 aligned crop - crop_aligned_f64| where both are finite, u = 2^-24 the f32 unit roundoff, every intermediate
    at most 255 in magnitude: a row's lerp p00 + fx * (p01 - p00) rounds fx (255 u), the product (255 u) and the sum (255 u) --
    3 * 255 u for ``top``, the same for ``bot``; the third lerp top + fy * (bot - top) inherits top's error once and, through
    the difference, top's and bot's (9 * 255 u together), rounds the difference, fy, the product and the sum (4 * 255 u):
    13 * 255 u.  The subtraction of 127.5 rounds once more (128 u) and the division by 128 is exact: (13 * 255 + 128) / 128 u,
    plus 1 % for the second-order terms = 1.62e-6."""
    return (13 * 255 + 128) / 128.0 * 2.0 ** -24 * 1.01


# ---- the case table ---------------------------------------------------------------------------------------------------------
GEOMETRIES = ((180, 320), (97, 131), (1, 1), (1, 200), (200, 1), (720, 1280), (2160, 3840))     # (H, W)
SIDES = (1, 2, 3, 39, 40, 41, 79, 80, 81, 159, 160, 161, 240)
CONTENTS = ("random", "zeros", "ones", "checker")


def rect_table(H: int, W: int) -> list:
    """Rectangles (x0, y0, x1, y1) of an H x W frame: every square side of SIDES that fits plus the full frame, the mixed aspects
    (1 x full height, full width x 1, 2 x 161, 161 x 2, 3 x 80, 80 x 3, 240 x 39, 41 x 159, 160 x 80, 80 x 160, full width x 2,
    2 x full height), each at the four frame corners and once in the interior; duplicates dropped, order fixed."""
    sizes = [(s, s) for s in SIDES] + [(W, H), (1, H), (W, 1), (2, 161), (161, 2), (3, 80), (80, 3), (240, 39), (41, 159),
                                       (160, 80), (80, 160), (W, 2), (2, H)]
    out, seen = [], set()
    for w, h in sizes:
        if w > W or h > H:
            continue
        for x0, y0 in ((0, 0), (W - w, 0), (0, H - h), (W - w, H - h), ((W - w) // 3, (2 * (H - h)) // 5)):
            r = (x0, y0, x0 + w, y0 + h)
            if r not in seen:
                seen.add(r)
                out.append(r)
    return out


def content_frames(kind: str, k: int, H: int, W: int, seed: int) -> np.ndarray:
    """k frames (k, H, W, 3) u8: uniform random bytes, all 0, all 255, or a 1-px checkerboard of 0 / 255 whose phase alternates
    from frame to frame."""
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, (k, H, W, 3), dtype=np.uint8)
    if kind == "zeros":
        return np.zeros((k, H, W, 3), np.uint8)
    if kind == "ones":
        return np.full((k, H, W, 3), 255, np.uint8)
    assert kind == "checker"
    f, y, x = np.ogrid[:k, :H, :W]
    return np.ascontiguousarray(np.broadcast_to(((((f + y + x) & 1) * 255).astype(np.uint8))[..., None], (k, H, W, 3)))


def landmark_sets(H: int, W: int, seed: int = 5) -> list:
    """Named five-point sets (x0..x4, y0..y4, f32) for an H x W frame: the template itself, upright / rotated / scaled / jittered
    faces, the template shifted by whole pixels so that its 160 x 160 grid ends on the frame's last row and column (a = 1, b = 0 up
    to the f32 rounding of the points: samples within 1e-5 of integer coordinates, on either side), one centred on each frame corner (most samples outside: replicated borders), degenerate sets (five equal points:
    scale 0, every output pixel samples that one point) on integer coordinates inside, on the last pixel, one past it, at -1 and
    half a pixel inside the far corner, a face that spans the whole frame, one far outside it, and one with a NaN coordinate."""
    rng = np.random.default_rng(seed)
    tx, ty = np.array(TEMPLATE_X), np.array(TEMPLATE_Y)

    def place(scale, deg, cx, cy, jitter=0.0):
        t = np.deg2rad(deg)
        u, v = (tx - 80.0) * scale, (ty - 102.7) * scale
        px = np.cos(t) * u - np.sin(t) * v + cx + rng.normal(0, jitter, 5)
        py = np.sin(t) * u + np.cos(t) * v + cy + rng.normal(0, jitter, 5)
        return np.concatenate([px, py]).astype(np.float32)

    def point(x, y):
        return np.concatenate([np.full(5, x), np.full(5, y)]).astype(np.float32)
    nan = place(1.0, 0, W / 2, H / 2)
    nan[3] = np.nan
    return [("template", np.concatenate([tx, ty]).astype(np.float32)),
            ("integer shift", (np.concatenate([tx, ty]) + np.repeat([float(W - 160), float(H - 160)], 5)).astype(np.float32)),
            ("upright", place(1.0, 0, W / 2, H / 2)),
            ("small rotated", place(0.6, 17, W / 2 + 10, H / 2 - 10, 1.5)),
            ("large rotated", place(1.7, -33, W / 3, 2 * H / 3, 2.0)),
            ("corner 00", place(1.2, 0, 0, 0)), ("corner 01", place(1.2, 10, W - 1, 0)),
            ("corner 10", place(1.2, 20, 0, H - 1)), ("corner 11", place(1.2, 30, W - 1, H - 1)),
            ("upside down", place(1.2, 180, W - 20, H - 20, 1.0)),
            ("tiny at the edge", place(0.3, 90, W - 5, 3)),
            ("whole frame", place(min(H, W) / 160.0, 5, W / 2, H / 2)),
            ("far outside", place(40.0, 45, 5000 + W, -3000)),
            ("point inside", point(min(W - 1, 5), min(H - 1, 7))),
            ("point last pixel", point(W - 1, H - 1)), ("point one past", point(W, H)), ("point -1", point(-1, -1)),
            ("point half inside", point(W - 0.5, H - 0.5)), ("point quarter", point(W - 1.25, 0.25)),
            ("nan", nan)]
