"""Plain restatement of facenet-pytorch 2.6.0's face extraction as ``MTCNN.forward`` runs it -- ``select_boxes``,
``extract_face``'s box arithmetic, ``crop_resize``'s three resamplers and forward's return conventions -- the reference the
extraction tests (test_extract_cpu.py, test_gpu_extract.py) compare csrc/trl_extract.hip and mtcnn.MTCNN with.  TEST
INFRASTRUCTURE ONLY.

The library's semantics are RECALLED, not read from its source (no copy is installed); they are the ones the feature issue
"Add MTCNN face extraction on the GPU" states.  The Pillow rule is checked against Pillow itself (test_extract_cpu.py); the
torch rule against F.interpolate(mode="area"); the OpenCV INTER_AREA rule is a restatement that nothing installed here can pin
(tests/golden/dump_extract_goldens.py is the route to pinning it).

paths() says which path of the kernel a crop must take (status, OpenCV mode, Pillow pass order, tap counts, LDS chunks, output
slots per thread); TABLE holds the cases of test_gpu_extract_table.py, reached() what each of them reaches by paths().
"""
from __future__ import annotations

import math
import zlib

import numpy as np

F32, F64 = np.float32, np.float64
METHODS = ("largest", "probability", "largest_over_threshold", "center_weighted_size")
RESAMPLERS = ("torch", "pil", "cv2")


# ---- select_boxes (threshold 0.9, center_weight 2.0) -------------------------------------------------------------------------
def _last_max(key):
    """element 0 of np.argsort(key)[::-1] under a stable sort: the LAST of the tied maxima."""
    key = np.asarray(key)
    return int(len(key) - 1 - np.argmax(key[::-1]))


def select(boxes, probs, method, W, H, threshold=0.9, center_weight=2.0):
    """Index into detect's rows (in detect's order) of the box select_boxes keeps, or None (no face)."""
    if boxes is None or len(boxes) == 0:
        return None
    b = np.asarray(boxes, F32)
    p = np.asarray(probs, F32)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])                       # f32
    if method == "largest":
        return _last_max(area)
    if method == "probability":
        return _last_max(p)
    if method == "largest_over_threshold":
        idx = np.nonzero(p > F32(threshold))[0]
        return None if len(idx) == 0 else int(idx[_last_max(area[idx])])
    if method == "center_weighted_size":
        # box centres in f32, offsets from the frame centre in f64 (this package: the frame's W, H for every input kind)
        cx = ((b[:, 0] + b[:, 2]) / F32(2)).astype(F64) - W / 2
        cy = ((b[:, 1] + b[:, 3]) / F32(2)).astype(F64) - H / 2
        return _last_max(area.astype(F64) - (cx * cx + cy * cy) * center_weight)
    raise ValueError(method)


# ---- extract_face's box --------------------------------------------------------------------------------------------------------
def crop_box(box, S, margin, W, H):
    """(x0, y0, x1, y1) of extract_face: the margin in f64 from the f32 box values, clamp, int() truncation."""
    x1, y1, x2, y2 = (float(F32(v)) for v in box[:4])
    mx = margin * float(F32(F32(x2) - F32(x1))) / (S - margin)
    my = margin * float(F32(F32(y2) - F32(y1))) / (S - margin)
    return (int(max(x1 - mx / 2, 0.0)), int(max(y1 - my / 2, 0.0)), int(min(x2 + mx / 2, float(W))), int(min(y2 + my / 2, float(H))))


# ---- resamplers: (h, w, 3) uint8 crop -> (S, S, 3) uint8 --------------------------------------------------------------------
def resize_torch(crop, S):
    """imresample (F.interpolate mode="area" = adaptive average pooling) then .byte(): bins [floor(o*n/S), ceil((o+1)*n/S)),
    (float)sum / kh / kw, truncation."""
    crop = np.asarray(crop, np.uint8)
    h, w = crop.shape[:2]
    ii = np.zeros((h + 1, w + 1, 3), np.int64)
    ii[1:, 1:] = crop.astype(np.int64).cumsum(0).cumsum(1)
    o = np.arange(S)
    ys, ye = o * h // S, ((o + 1) * h + S - 1) // S
    xs, xe = o * w // S, ((o + 1) * w + S - 1) // S
    s = ii[ye][:, xe] - ii[ys][:, xe] - ii[ye][:, xs] + ii[ys][:, xs]
    kh = (ye - ys).astype(F32)[:, None, None]
    kw = (xe - xs).astype(F32)[None, :, None]
    return (s.astype(F32) / kh / kw).astype(np.uint8)


def pil_coeffs(n, S):
    """Pillow's precompute_coeffs for the bilinear filter (support 1) + normalize_coeffs_8bpc: (xmin [S], fixed [S][n]) int64."""
    scale = n / S
    fs = max(scale, 1.0)
    ss = 1.0 / fs
    xmin = np.zeros(S, np.int64)
    K = np.zeros((S, n), np.int64)
    for o in range(S):
        center = (o + 0.5) * scale
        lo = max(int(center - fs + 0.5), 0)
        cnt = min(int(center + fs + 0.5), n) - lo
        w = [max(0.0, 1.0 - abs((i + lo - center + 0.5) * ss)) for i in range(cnt)]
        ww = 0.0
        for v in w:
            ww += v
        for i, v in enumerate(w):
            k = v / ww if ww != 0.0 else v
            K[o, lo + i] = int(-0.5 + k * (1 << 22)) if k < 0 else int(0.5 + k * (1 << 22))
        xmin[o] = lo
    return xmin, K


def _pil_pass(a, K):      # a (rows, n, 3) int64 -> (rows, S, 3): clip8((2^21 + sum k * v) >> 22)
    out = np.empty((a.shape[0], K.shape[0], a.shape[2]), np.int64)
    for o in range(K.shape[0]):                                            # K is banded: only the taps of output o
        nz = np.flatnonzero(K[o])
        lo, hi = (int(nz[0]), int(nz[-1]) + 1) if len(nz) else (0, 1)
        out[:, o] = np.einsum("n,rnc->rc", K[o, lo:hi], a[:, lo:hi])
    return np.clip((out + (1 << 21)) >> 22, 0, 255)


def pil_vertical_first(h, w, S):
    """Image.resize's pass order.  ImagingResample itself always filters horizontally first, but Image.resize (Pillow 12.2,
    Image.py) splits the call in two -- vertical, then horizontal -- "if self.size[1] > self.size[0] * 100 and size[1] <
    self.size[1]": an image over 100 times as tall as wide that shrinks vertically.  Both passes round to 8 bits, so the order
    shows in the bytes (+-1 in many cells).  test_extract_cpu.py checks this predicate against Pillow on a grid of shapes."""
    return h > w * 100 and S < h


def resize_pil(crop, S, order=None):
    """Image.fromarray(crop).resize((S, S), Image.BILINEAR): two passes, each rounded to 8 bits, in Image.resize's order
    (pil_vertical_first); order "h" / "v" forces horizontal- / vertical-first."""
    a = np.asarray(crop, np.uint8).astype(np.int64)
    h, w = a.shape[:2]
    Kx, Ky = pil_coeffs(w, S)[1], pil_coeffs(h, S)[1]
    if order == "v" or (order is None and pil_vertical_first(h, w, S)):
        t = _pil_pass(a.transpose(1, 0, 2), Ky)                            # (w, S, 3) indexed [x][oy]
        return _pil_pass(t.transpose(1, 0, 2), Kx).astype(np.uint8)        # (S, S, 3)
    t = _pil_pass(a, Kx)                                                   # (h, S, 3)
    out = _pil_pass(t.transpose(1, 0, 2), Ky)                              # (S, S, 3) indexed [x][y]
    return out.transpose(1, 0, 2).astype(np.uint8)


# ---- OpenCV 4.x INTER_AREA  (RECALLED: every line of this block restates OpenCV from memory; unpinned) -------------------
def cv2_area_tab(n, S):
    """computeResizeAreaTab: per output (first source index, f32 weights) with the 1e-3 edge tolerances."""   # RECALLED
    scale = 1.0 / (S / n)                                                 # resize(): scale = 1 / inv_scale, inv_scale = S / n
    tab = []
    for d in range(S):
        f1 = d * scale
        f2 = f1 + scale
        cell = min(scale, n - f1)
        s1, s2 = math.ceil(f1), math.floor(f2)
        s2 = min(s2, n - 1)
        s1 = min(s1, s2)
        lo, w = s1, []
        if s1 - f1 > 1e-3:
            lo = s1 - 1
            w.append(F32((s1 - f1) / cell))
        for _ in range(s1, s2):
            w.append(F32(1.0 / cell))
        if f2 - s2 > 1e-3:
            w.append(F32(min(min(f2 - s2, 1.0), cell) / cell))
        tab.append((lo, w))
    return tab


def cv2_linear_tab(n, S):
    """The area coefficients of the generic (fixed-point linear) path: sx = floor(d*scale), fx = (d+1) - (sx+1)/scale,
    fx <= 0 ? 0 : fx - floor(fx), shorts scaled by 2048; sx at the right edge clamps with fx = 0."""                  # RECALLED
    inv = S / n
    scale = 1.0 / inv
    sx = np.zeros(S, np.int64)
    a = np.zeros((S, 2), np.int64)
    for d in range(S):
        s = math.floor(d * scale)
        fx = float(F32((d + 1) - (s + 1) * inv))
        fx = 0.0 if fx <= 0 else float(F32(fx - math.floor(fx)))
        if s >= n - 1:
            s, fx = n - 1, 0.0
        sx[d] = s
        a[d] = (int(np.rint(F32(F32(1.0) - F32(fx)) * F32(2048))), int(np.rint(F32(fx) * F32(2048))))
    return sx, a


def resize_cv2(crop, S):
    """cv2.resize(crop, (S, S), interpolation=cv2.INTER_AREA) on a (h, w, 3) uint8 array."""                         # RECALLED
    a = np.asarray(crop, np.uint8)
    h, w = a.shape[:2]
    sx, sy = 1.0 / (S / w), 1.0 / (S / h)
    kx, ky = int(np.rint(sx)), int(np.rint(sy))
    if sx >= 1 and sy >= 1 and abs(sx - kx) < 2.220446049250313e-16 and abs(sy - ky) < 2.220446049250313e-16:
        # resizeAreaFast (integer block means)                                                                       RECALLED
        s = a.astype(np.int64).reshape(S, ky, S, kx, 3).sum((1, 3))
        if kx == 2 and ky == 2:
            return ((s + 2) >> 2).astype(np.uint8)
        v = s.astype(F32) * F32(F32(1.0) / F32(kx * ky))
        return np.clip(np.rint(v), 0, 255).astype(np.uint8)
    if sx >= 1 and sy >= 1:                                              # resizeArea (float tables)               RECALLED
        tx, ty = cv2_area_tab(w, S), cv2_area_tab(h, S)
        af = a.astype(F32)
        buf = np.zeros((h, S, 3), F32)
        for d, (lo, wt) in enumerate(tx):
            acc = np.zeros((h, 3), F32)
            for i, al in enumerate(wt):
                acc = acc + af[:, lo + i] * al
            buf[:, d] = acc
        out = np.zeros((S, S, 3), F32)
        for d, (lo, wt) in enumerate(ty):
            acc = np.zeros((S, 3), F32)
            for i, be in enumerate(wt):
                acc = acc + be * buf[lo + i]
            out[d] = acc
        return np.clip(np.rint(out), 0, 255).astype(np.uint8)
    # an upscaled axis: the generic fixed-point linear path with area coefficients                                  RECALLED
    xo, ax = cv2_linear_tab(w, S)
    yo, by = cv2_linear_tab(h, S)
    ai = a.astype(np.int64)
    x1 = np.minimum(xo + 1, w - 1)
    rows = ai[:, xo] * ax[:, 0][None, :, None] + ai[:, x1] * ax[:, 1][None, :, None]       # (h, S, 3)
    r0, r1 = rows[np.clip(yo, 0, h - 1)], rows[np.clip(yo + 1, 0, h - 1)]
    v = (((by[:, 0][:, None, None] * (r0 >> 4)) >> 16) + ((by[:, 1][:, None, None] * (r1 >> 4)) >> 16) + 2) >> 2
    return np.clip(v, 0, 255).astype(np.uint8)


RESIZE = {"torch": resize_torch, "pil": resize_pil, "cv2": resize_cv2}


# ---- extract_face / forward --------------------------------------------------------------------------------------------------
def extract(frame, box, S=160, margin=0, resample="torch", post_process=True):
    """(S, S, 3) f32 face of one box, NHWC, channel order of the input; ValueError for an empty crop."""
    H, W = frame.shape[:2]
    x0, y0, x1, y1 = crop_box(box, S, margin, W, H)
    if x1 <= x0 or y1 <= y0:
        raise ValueError("empty crop")
    v = RESIZE[resample](frame[y0:y1, x0:x1], S).astype(F32)
    return (v - F32(127.5)) / F32(128.0) if post_process else v


def forward(frame, boxes, probs, S=160, margin=0, resample="torch", post_process=True, keep_all=False, method="largest",
            return_prob=False):
    """MTCNN.forward on one frame given detect's (boxes, probs) in detect's order: (3, S, S) / (k, 3, S, S) / None."""
    H, W = frame.shape[:2]
    if boxes is None or len(boxes) == 0:
        return (None, [None]) if return_prob else None
    if keep_all:
        faces = np.stack([extract(frame, b, S, margin, resample, post_process) for b in boxes]).transpose(0, 3, 1, 2)
        return (faces, np.asarray(probs, F32)) if return_prob else faces
    i = select(boxes, probs, method, W, H)
    if i is None:
        return (None, [None]) if return_prob else None
    face = extract(frame, boxes[i], S, margin, resample, post_process).transpose(2, 0, 1)
    return (face, F32(probs[i])) if return_prob else face


# ---- which path of csrc/trl_extract.hip a crop takes (from the definitions above, not from the kernel) ---------------------
LDS_WORDS = 16384          # words of horizontally filtered rows a workgroup stages: T = LDS_WORDS // (3 * S) rows per chunk
BLOCK = 256                # threads of a workgroup: ceil(3 * S / BLOCK) output slots per thread


def _pil_taps(n, S):
    """largest tap count of Pillow's bilinear filter on one axis: xmax - xmin of precompute_coeffs."""
    scale = n / S
    fs = max(scale, 1.0)
    c = (np.arange(S) + 0.5) * scale
    return int((np.minimum((c + fs + 0.5).astype(np.int64), n) - np.maximum((c - fs + 0.5).astype(np.int64), 0)).max())


def _torch_taps(n, S):
    o = np.arange(S)
    return int((((o + 1) * n + S - 1) // S - o * n // S).max())


def paths(h, w, S, resample):
    """What the plan of one (crop h, crop w, S, resampler) must say: status, OpenCV mode with kx / ky, Pillow pass order, the
    largest tap count per axis, the LDS chunks of the vertical taps (None where no row is staged) and the output slots per thread."""
    p = dict(status=1 if h > 0 and w > 0 else -1, mode=None, kx=0, ky=0, order=None, taps_x=0, taps_y=0, chunks=None,
             slots=-(-3 * S // BLOCK), T=LDS_WORDS // (3 * S))
    if p["status"] != 1:
        return p
    if resample == "torch":
        p.update(taps_x=_torch_taps(w, S), taps_y=_torch_taps(h, S))
    elif resample == "pil":
        p.update(order="v" if pil_vertical_first(h, w, S) else "h", taps_x=_pil_taps(w, S), taps_y=_pil_taps(h, S))
        if p["order"] == "h":
            p["chunks"] = -(-p["taps_y"] // p["T"])
    else:
        sx, sy = 1.0 / (S / w), 1.0 / (S / h)
        kx, ky = int(np.rint(sx)), int(np.rint(sy))
        p.update(kx=kx, ky=ky)
        if sx >= 1 and sy >= 1 and abs(sx - kx) < 2.220446049250313e-16 and abs(sy - ky) < 2.220446049250313e-16:
            p.update(mode="fast", taps_x=kx, taps_y=ky)
        elif sx >= 1 and sy >= 1:
            p.update(mode="area", taps_x=max(len(t[1]) for t in cv2_area_tab(w, S)), taps_y=max(len(t[1]) for t in cv2_area_tab(h, S)))
            p["chunks"] = -(-p["taps_y"] // p["T"])
        else:
            p.update(mode="linear", taps_x=2, taps_y=2, chunks=1)
    return p


# ---- the case table of test_gpu_extract_table.py (test_extract_cpu.py checks what it reaches) -----------------------------
def _case(name, dims, S, margin, post, rows, reach, seed=None):
    return dict(name=name, dims=dims, S=S, margin=margin, post=post, rows=rows, reach=reach,
                seed=zlib.crc32(name.encode()) if seed is None else seed)


def _edge_rows(H, W, n):
    """boxes over each frame edge and over all of them, in the first and last frame, tiny boxes (a margin of S - 1 multiplies
    the box size by S), a degenerate box, boxes outside the frame, and rows of no frame"""
    return [(0, (-6.5, 9.25, 20.5, 30.75)), (n - 1, (W - 21.25, 7.5, W + 5.5, 33.0)), (1, (8.0, -4.5, 30.75, 21.25)),
            (n - 1, (6.5, H - 24.0, 31.5, H + 3.25)), (0, (-3.0, -2.0, W + 4.0, H + 1.5)), (n - 1, (11.0, 13.0, 11.25, 13.5)),
            (0, (W - 0.5, 20.0, W - 0.25, 20.5)), (1, (0.25, 0.5, 0.75, 0.75)), (0, (30.0, 10.0, 20.0, 40.0)),
            (n - 1, (W + 3.0, 10.0, W + 30.0, 40.0)), (1, (5.0, -40.0, 25.0, -10.0)), (-1, (1.0, 1.0, 20.0, 20.0)),
            (n, (1.0, 1.0, 20.0, 20.0)), (1, (12.0, 10.0, 40.0, 38.0)), (n - 1, (20.0, H - 0.5, 20.25, H - 0.25)),
            (0, (W + 50.0, 10.0, W + 50.25, 10.25))]


def _table():
    t = [
        _case("tall80", (1, 5500, 80), 160, 0, True, [(0, (0, 0, 80, 5500))], ("pil:chunks3+", "cv2:linear:up_down>T", "S160")),
        _case("tall200", (1, 5500, 200), 160, 0, False, [(0, (0, 0, 200, 5500))], ("cv2:area:chunks2+", "pil:chunks3+")),
        _case("tall48", (1, 3200, 48), 160, 0, True, [(0, (0, 0, 48, 3200))], ("pil:chunks2",)),
        # S = 171 (3 * S = 513: a one-value last slot), T = 31: Pillow has 31 taps at h = 2567 and 32 at 2651, OpenCV's area table
        # 31 at h = 4961 and 32 at 5132
        _case("taps171", (1, 5132, 176), 171, 0, False,
              [(0, (0, 0, 176, 2567)), (0, (2, 100, 176, 2751)), (0, (0, 171, 176, 5132)), (0, (0, 0, 173, 5132))],
              ("S171", "pil:tapsT", "pil:tapsT+1", "cv2:area:tapsT", "cv2:area:tapsT+1", "partial_last_slot", "pil:chunks1")),
        # S = 86 (3 * S = 258): every integer-ratio form of resizeAreaFast, and crops one pixel off them
        _case("fast86", (2, 440, 350), 86, 0, True,
              [(0, (3, 5, 89, 91)), (1, (7, 2, 179, 174)), (0, (1, 9, 173, 353)), (1, (4, 6, 348, 178)), (0, (11, 8, 269, 438)),
               (1, (7, 2, 180, 174)), (0, (1, 9, 173, 352))],
              ("S86", "cv2:fast1x1", "cv2:fast2x2", "cv2:fast2x4", "cv2:fast4x2", "cv2:fast3x5", "cv2:area:one_off_integer",
               "partial_last_slot")),
        # S = 1024 (3 * S = 12 * 256, T = 5): 1-pixel crops, 6 Pillow taps, and a crop over 100 times as tall as wide
        _case("up1024", (1, 9, 11), 1024, 0, True, [(0, (4, 4, 5, 5)), (0, (0, 3, 11, 4)), (0, (2, 0, 3, 9))],
              ("S1024", "up_1x1_to_1024", "up_1xn_to_1024", "up_nx1_to_1024", "full_last_slot")),
        _case("tall1024", (1, 2561, 32), 1024, 0, False, [(0, (0, 0, 32, 2561)), (0, (3, 0, 28, 2561))],
              ("pil:chunks2", "pil:tapsT+1", "pil:vfirst")),
        _case("tall1023", (2, 2558, 40), 1023, 0, True, [(1, (0, 0, 40, 2558)), (0, (5, 7, 25, 27))], ("S1023", "pil:chunks2", "last_of_2+")),
        # Pillow's pass order, both sides of h > 100 * w and of S < h
        _case("order160", (1, 606, 8), 160, 0, False, [(0, (0, 0, 6, 600)), (0, (0, 0, 6, 601)), (0, (1, 0, 6, 606)), (0, (1, 3, 7, 603))],
              ("pil:vfirst", "pil:hfirst_at_switch")),
        _case("order700", (1, 606, 8), 700, 0, True, [(0, (1, 0, 6, 606))], ("pil:hfirst_upscaled_tall",)),
        _case("vtall40", (1, 5500, 40), 160, 0, True, [(0, (0, 0, 40, 5500))], ("pil:vfirst",)),
        _case("order4", (1, 606, 8), 4, 0, True, [(0, (0, 0, 6, 601)), (0, (0, 0, 6, 600))], ("pil:vfirst:both_down", "pil:hfirst_at_switch")),
        # a vertical-first crop of 87 columns: the vertically filtered row has 3 * 87 = 261 values, more than a workgroup has
        # threads.  S = 160 stretches it horizontally (2 taps); S = 40 and S = 7 shrink both axes, so the horizontal pass runs up to
        # 2 * 87 / S + 1 taps over that row.  The 90-column row is not over 100 times as tall as wide: horizontal first, 4 chunks
        _case("vfirst87s160", (1, 8800, 90), 160, 0, False, [(0, (2, 0, 89, 8800)), (0, (0, 0, 90, 8800))],
              ("pil:vfirst:cols>85", "pil:chunks3+")),
        _case("vfirst87s40", (1, 8800, 90), 40, 0, True, [(0, (2, 0, 89, 8800))], ("pil:vfirst:cols>85", "pil:vfirst:both_down")),
        _case("vfirst87s7", (1, 8800, 90), 7, 0, False, [(0, (2, 0, 89, 8800)), (0, (3, 100, 89, 8799))],
              ("pil:vfirst:cols>85", "pil:vfirst:both_down")),
        _case("whole_by_margin", (3, 96, 128), 160, 80, True, [(2, (32, 24, 96, 72)), (0, (32, 24, 96, 72))],
              ("whole_frame_by_margin", "first_of_3", "last_of_3")),
        _case("none", (1, 20, 20), 160, 0, True, [], ("m0",)),
    ]
    for S in (112, 160, 161):                                      # the sizes of the earlier tests, over a 270p batch
        t.append(_case(f"std{S}", (3, 270, 480), S, 20, S != 161,
                       [(0, (0, 0, 480, 270)), (2, (100.5, 30.25, 260.0, 250.75)), (1, (300, 100, 340, 150)), (2, (-10, 200, 90, 280))],
                       (f"S{S}", "cv2:area", "cv2:linear", "first_of_3", "last_of_3")))
    for S, dims in ((1, (3, 61, 47)), (2, (3, 61, 47)), (7, (3, 61, 47)), (85, (3, 97, 131)), (160, (3, 97, 131))):
        for margin in sorted({0, S // 2, S - 1}):
            mt = [k for k, v in (("margin0", 0), ("marginS/2", S // 2), ("marginS-1", S - 1)) if v == margin and (v or k == "margin0")]
            reach = [f"S{S}", "degenerate", "outside", "frame_of=-1", "frame_of=n", "first_of_3", "last_of_3"]
            reach += [f"{m}:{side}" for m in mt for side in ("left", "right", "top", "bottom", "all_sides")]
            t.append(_case(f"edges{S}m{margin}", dims, S, margin, (S + margin) % 2 == 0, _edge_rows(dims[1], dims[2], dims[0]), tuple(reach)))
    return t


TABLE = _table()

REQUIRED = (["pil:chunks1", "pil:chunks2", "pil:chunks3+", "cv2:area:chunks2+", "cv2:linear:up_down>T", "pil:tapsT", "pil:tapsT+1",
             "cv2:area:tapsT", "cv2:area:tapsT+1", "cv2:fast1x1", "cv2:fast2x2", "cv2:fast2x4", "cv2:fast4x2", "cv2:fast3x5",
             "cv2:area:one_off_integer", "up_1x1_to_1024", "up_1xn_to_1024", "up_nx1_to_1024", "whole_frame_by_margin", "degenerate",
             "outside", "frame_of=-1", "frame_of=n", "m0", "first_of_3", "last_of_3", "partial_last_slot", "full_last_slot",
             "pil:vfirst", "pil:vfirst:cols>85", "pil:vfirst:both_down", "pil:hfirst_at_switch", "pil:hfirst_upscaled_tall"]
            + [f"S{S}" for S in (1, 2, 7, 85, 86, 112, 160, 161, 171, 1023, 1024)]
            + [f"{m}:{side}" for m in ("margin0", "marginS/2", "marginS-1") for side in ("left", "right", "top", "bottom", "all_sides")])


def case_frames(case):
    n, H, W = case["dims"]
    return np.random.default_rng(case["seed"]).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def case_crops(case):
    """per row: (status, (h, w) of the crop or None) by extract_face's box arithmetic"""
    n, H, W = case["dims"]
    out = []
    for f, box in case["rows"]:
        if not 0 <= f < n:
            out.append((0, None))
            continue
        x0, y0, x1, y1 = crop_box(box, case["S"], case["margin"], W, H)
        out.append((1, (y1 - y0, x1 - x0)) if x1 > x0 and y1 > y0 else (-1, None))
    return out


def reached(case):
    """The tags of REQUIRED that a case reaches, according to paths() and the box arithmetic."""
    n, H, W = case["dims"]
    S, margin = case["S"], case["margin"]
    tags = {f"S{S}"}
    if not case["rows"]:
        tags.add("m0")
    if 3 * S > BLOCK and 3 * S % BLOCK:
        tags.add("partial_last_slot")
    if 3 * S == 12 * BLOCK:
        tags.add("full_last_slot")
    mts = [k for k, v in (("margin0", 0), ("marginS/2", S // 2), ("marginS-1", S - 1)) if v == margin and (v or k == "margin0")]
    for (f, box), (st, hw) in zip(case["rows"], case_crops(case)):
        if st == 0:
            tags.add("frame_of=-1" if f < 0 else "frame_of=n")
            continue
        bx1, by1, bx2, by2 = (float(F32(v)) for v in box)
        if st == -1:
            tags.add("degenerate" if bx2 < bx1 or by2 < by1 else "outside")
            continue
        if n == 3 and f in (0, 2):
            tags.add("first_of_3" if f == 0 else "last_of_3")
        if n > 1 and f == n - 1:
            tags.add("last_of_2+")
        mx, my = margin * (bx2 - bx1) / (S - margin), margin * (by2 - by1) / (S - margin)
        sides = [bx1 - mx / 2 < 0, bx2 + mx / 2 > W, by1 - my / 2 < 0, by2 + my / 2 > H]
        for m in mts:
            for side, out in zip(("left", "right", "top", "bottom"), sides):
                if out and sum(sides) < 4:
                    tags.add(f"{m}:{side}")
            if all(sides):
                tags.add(f"{m}:all_sides")
        h, w = hw
        if margin > 0 and (h, w) == (H, W) and not any(sides) and bx1 > 0 and by1 > 0 and bx2 < W and by2 < H:
            tags.add("whole_frame_by_margin")
        if S == 1024 and (h == 1 or w == 1):
            tags.add("up_1x1_to_1024" if h == w else ("up_1xn_to_1024" if h == 1 else "up_nx1_to_1024"))
        p = paths(h, w, S, "pil")
        if p["order"] == "v":
            tags.add("pil:vfirst")
            if 3 * w > BLOCK:                                      # the vertically filtered row takes a second round of the threads
                tags.add("pil:vfirst:cols>85")
            if S < w:                                              # more than 2 horizontal taps over that row
                tags.add("pil:vfirst:both_down")
        else:
            tags.add("pil:chunks%s" % ("3+" if p["chunks"] >= 3 else p["chunks"]))
            if p["taps_y"] in (p["T"], p["T"] + 1):
                tags.add("pil:tapsT" if p["taps_y"] == p["T"] else "pil:tapsT+1")
            if h == 100 * w and S < h:
                tags.add("pil:hfirst_at_switch")
            if h > 100 * w:
                tags.add("pil:hfirst_upscaled_tall")
        c = paths(h, w, S, "cv2")
        if c["mode"] == "fast":
            tags.add(f"cv2:fast{c['kx']}x{c['ky']}")
        elif c["mode"] == "area":
            tags.add("cv2:area")
            if c["chunks"] >= 2:
                tags.add("cv2:area:chunks2+")
            if c["taps_y"] in (c["T"], c["T"] + 1):
                tags.add("cv2:area:tapsT" if c["taps_y"] == c["T"] else "cv2:area:tapsT+1")
            if sorted((h % S, w % S)) in ([0, 1], [0, S - 1]):
                tags.add("cv2:area:one_off_integer")
        else:
            # the linear path reads 2 taps per axis whatever the scale, so no tap chunk follows from "shrunk past T": the tag
            # marks the geometry the issue names (one axis stretched, the other shrunk by more than T source rows per output)
            tags.add("cv2:linear")
            if (w < S and h > p["T"] * S) or (h < S and w > p["T"] * S):
                tags.add("cv2:linear:up_down>T")
    return tags


_EXPECTED = {}


def expected(case, resample):
    """(faces [m, S, S, 3] f32, status [m] int32) of a case: computed once, shared, read-only."""
    key = (case["name"], resample)
    if key not in _EXPECTED:
        fr = case_frames(case)
        S, m = case["S"], len(case["rows"])
        faces, status = np.zeros((m, S, S, 3), F32), np.zeros(m, np.int32)
        for r, ((f, box), (st, _hw)) in enumerate(zip(case["rows"], case_crops(case))):
            status[r] = st
            if st == 1:
                faces[r] = extract(fr[f], box, S, case["margin"], resample, case["post"])
        faces.setflags(write=False)
        status.setflags(write=False)
        _EXPECTED[key] = (faces, status)
    return _EXPECTED[key]
