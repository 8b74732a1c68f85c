"""Scalar restatement of the drawing kernel (csrc/trl_annotate.hip: k_draw and the list preparation of trl_draw), driven by the
lists of ``annotate.DrawList`` / ``annotate.draw_list``: per pixel, per segment, ``numpy.float32`` scalars, one rounding per
operation, numpy's float32 ``hypot`` as ``float32(sqrt(float64(x) * x + float64(y) * y))``.

``tests/test_annotate_cpu.py`` holds it against ``annotate.py``'s own array code byte for byte: that pins the rules the kernel
follows (order, sequential blending through uint8, weak-scalar rounding, the hypot form, the boxes) where no GPU is needed;
``tests/test_gpu_annotate.py`` then holds the kernel against ``annotate.py``."""
import math

import numpy as np

f32, f64 = np.float32, np.float64


def hypot_double(x, y):
    """The kernel's hypot: both squares exact in float64, one rounding for the sum, one for the root, one to float32."""
    return f32(np.sqrt(f64(x) * f64(x) + f64(y) * f64(y)))


def hypot_float(x, y):
    """What the kernel must NOT use: float32 sqrt(x*x + y*y)."""
    return f32(np.sqrt(f32(f32(x) * f32(x)) + f32(f32(y) * f32(y))))


def clip01(v):
    return np.minimum(np.maximum(v, f32(0)), f32(1))


def seg_box(s, H, W):
    """trl_draw's box of a segment: pixels outside have coverage 0.  One pixel wider than the reach, clipped to the frame."""
    x0, y0, dx, dy, reach = float(s["x0"]), float(s["y0"]), float(s["dx"]), float(s["dy"]), float(s["reach"])
    xe, ye, m = x0 + dx, y0 + dy, reach + 1.0
    xa = min(max(math.floor(min(x0, xe) - m), 0), W)
    ya = min(max(math.floor(min(y0, ye) - m), 0), H)
    xb = min(max(math.ceil(max(x0, xe) + m), -1), W - 1)
    yb = min(max(math.ceil(max(y0, ye) + m), -1), H - 1)
    return xa, ya, xb, yb


def fills(fr, H, W):
    """The rectangle's four inclusive fills, clipped to the frame (empty ones dropped)."""
    t = int(fr["thickness"])
    if t <= 0:
        return []
    x0, x1 = sorted((int(fr["x0"]), int(fr["x1"])))
    y0, y1 = sorted((int(fr["y0"]), int(fr["y1"])))
    h = t // 2
    out = []
    for xa, ya, xb, yb in ((x0 - h, y0 - h, x1 + h, y0 + h), (x0 - h, y1 - h, x1 + h, y1 + h),
                           (x0 - h, y0 - h, x0 + h, y1 + h), (x1 - h, y0 - h, x1 + h, y1 + h)):
        xa, ya, xb, yb = max(xa, 0), max(ya, 0), min(xb, W - 1), min(yb, H - 1)
        if xa <= xb and ya <= yb:
            out.append((xa, ya, xb, yb))
    return out


def blend_pixel(v, col, s, xx, yy, hypot=hypot_double):
    """One segment on the pixel (xx, yy): v = its three bytes as float32 -> the bytes after the segment, as float32.  Every
    operation is one float32 operation of the kernel, in its order.  (Written on float32 scalars; float32 arrays of pixels go
    through the same operations element by element, which is how the large cases are run.)"""
    x0, y0, dx, dy, L2, reach = (f32(s[k]) for k in ("x0", "y0", "dx", "dy", "L2", "reach"))
    assert xx.dtype == np.float32 and yy.dtype == np.float32 and all(c.dtype == np.float32 for c in v)
    t = f32(0)
    if L2 > 0:
        ux = (xx - x0) * dx
        uy = (yy - y0) * dy
        t = clip01((ux + uy) / L2)
    ex = xx - (x0 + t * dx)
    ey = yy - (y0 + t * dy)
    a = clip01(reach - hypot(ex, ey))
    ia = f32(1) - a
    return [np.minimum(np.maximum(np.rint(v[c] * ia + col[c] * a), f32(0)), f32(255)) for c in range(3)]


def draw(batch: np.ndarray, flist, segs, hypot=hypot_double, scalar: bool = True) -> None:
    """The kernel on a host batch (n, H, W, 3) uint8, in place.  ``scalar``: pixel by pixel on float32 scalars; otherwise the
    pixels of a segment's box at once, as float32 arrays through the same operations."""
    n, H, W = batch.shape[:3]
    for v in (segs[k] for k in ("x0", "y0", "dx", "dy", "L2", "reach")):
        assert v.dtype == np.float32 and np.isfinite(v).all()
    assert len(set(flist["frame"].tolist())) == len(flist)
    boxes = [seg_box(s, H, W) for s in segs]
    for fr in flist:
        assert 0 <= fr["frame"] < n and 0 <= fr["seg_begin"] <= fr["seg_end"] <= len(segs)
        img = batch[fr["frame"]]
        for xa, ya, xb, yb in fills(fr, H, W):            # opaque: the order of the four does not matter
            img[ya:yb + 1, xa:xb + 1] = fr["rect_bgr"]
        col = [f32(c) for c in fr["text_bgr"]]
        rng = range(int(fr["seg_begin"]), int(fr["seg_end"]))
        # the kernel walks the segments per pixel; segments are independent between pixels, so segment-major order is the same thing
        for k in rng:
            xa, ya, xb, yb = boxes[k]
            if xa > xb or ya > yb:
                continue
            if not scalar:
                yy, xx = (g.astype(np.float32) for g in np.mgrid[ya:yb + 1, xa:xb + 1])
                reg = img[ya:yb + 1, xa:xb + 1]
                out = blend_pixel([reg[..., c].astype(np.float32) for c in range(3)], col, segs[k], xx, yy, hypot)
                img[ya:yb + 1, xa:xb + 1] = np.stack(out, -1).astype(np.uint8)
                continue
            for y in range(ya, yb + 1):
                for x in range(xa, xb + 1):
                    out = blend_pixel([f32(c) for c in img[y, x]], col, segs[k], f32(x), f32(y), hypot)
                    img[y, x] = [int(c) for c in out]


# ---- the case grid shared by the CPU and the GPU tests -------------------------------------------------------------------------
INDICES = (7, 42, 968, 1350, 88888, 123456, 790)            # 1 to 6 digits, every digit 0-9 among them


def background(kind: str, n: int, H: int, W: int, seed: int = 0) -> np.ndarray:
    """(n, H, W, 3) uint8: "noise", "zeros", "ones" (255), or "ramp" -- b = x + 3y + 5f, g = b + 85, r = b + 170 (mod 256), so that
    a caption a few hundred pixels wide has every byte value under its partly covered pixels, in every channel."""
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    if kind in ("zeros", "ones"):
        return np.full((n, H, W, 3), 0 if kind == "zeros" else 255, np.uint8)
    assert kind == "ramp"
    f, y, x = np.ogrid[:n, :H, :W]
    b = x + 3 * y + 5 * f
    return np.stack([b, b + 85, b + 170], -1).astype(np.uint8)


BACKGROUNDS = ("noise", "zeros", "ones", "ramp")


def rects(H: int, W: int) -> list:
    """Rectangles inside, on every edge, partly and wholly outside the frame, degenerate, with swapped corners, and near the top
    (the "Real Frame" caption sits at y0 - 10: above the frame for the ones that start high)."""
    cx, cy = W // 2, H // 2
    return [(W // 4, H // 3, cx + W // 5, cy + H // 4),                  # inside
            (0, H // 3, cx, cy + H // 5), (W // 4, 0, cx, cy),           # on the left edge, on the top edge (caption above the frame)
            (cx, cy, W - 1, H - 1),                                      # on the right and bottom edges
            (-7, -5, cx, cy), (cx, cy, W + 9, H + 6),                    # partly outside
            (W + 20, H + 20, W + 60, H + 70), (-90, -80, -30, -20),      # wholly outside
            (cx, H // 4, cx, cy + 3), (W // 4, cy, cx, cy),              # degenerate: x0 = x1, y0 = y1
            (cx + W // 5, cy + H // 5, W // 4, H // 4),                  # swapped corners
            (W // 3, 4, cx, cy), (1, 1, 2, 2)]                           # caption partly above the frame; a tiny box in the corner


def host_annotate(batch: np.ndarray, notes) -> None:
    """annotate.annotate on the noted rows of a host batch: the reference every implementation is held against."""
    from truely_amd import annotate as A
    for row, index, rect, flagged in notes:
        A.annotate(batch[row], index, rect, flagged)


def thick_lines(n: int, H: int, W: int) -> "list":
    """One long caption per frame in strokes 21 to 51 pixels thick, at fractional origins and scales, as (row, text, org, scale,
    colour, thickness).  A last-place difference in a distance moves a blended value by colour x 2^-24 x distance, so it takes
    long edges far from the stroke's axis to make a wrong ``hypot`` visible in a byte: ordinary captions (reach 1.5) flip about
    two bytes per million partly covered pixels, these about thirty."""
    out = []
    for f in range(n):
        scale = 3.1 + 0.37 * f
        text = ("AI Detected - Frame 0123456789 Real " * 3)[f:f + 4 + int(W / (19 * scale))]
        out.append((f, text, (3.3 + 1.7 * f, H * (0.35 + 0.04 * (f % 8)) + 0.29 * f), scale, (255, 16 * f % 256, 255 - 16 * f % 256), 21 + 2 * f))
    return out
