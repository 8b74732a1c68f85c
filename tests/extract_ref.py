"""Plain restatement of facenet-pytorch 2.6.0's face extraction as ``MTCNN.forward`` runs it -- ``select_boxes``,
``extract_face``'s box arithmetic, ``crop_resize``'s three resamplers and forward's return conventions -- the reference the
extraction tests (test_extract_cpu.py, test_gpu_extract.py) compare csrc/trl_extract.hip and mtcnn.MTCNN with.  TEST
INFRASTRUCTURE ONLY.

The library's semantics are RECALLED, not read from its source (no copy is installed); they are the ones the feature issue
"Add MTCNN face extraction on the GPU" states.  The Pillow rule is checked against Pillow itself (test_extract_cpu.py); the
torch rule against F.interpolate(mode="area"); the OpenCV INTER_AREA rule is a restatement that nothing installed here can pin
(tests/golden/dump_extract_goldens.py is the route to pinning it).
"""
from __future__ import annotations

import math

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
    acc = np.einsum("on,rnc->roc", K, a) + (1 << 21)
    return np.clip(acc >> 22, 0, 255)


def resize_pil(crop, S):
    """Image.fromarray(crop).resize((S, S), Image.BILINEAR): horizontal pass (rounded to 8 bits) then vertical pass."""
    a = np.asarray(crop, np.uint8).astype(np.int64)
    h, w = a.shape[:2]
    t = _pil_pass(a, pil_coeffs(w, S)[1])                                  # (h, S, 3)
    out = _pil_pass(t.transpose(1, 0, 2), pil_coeffs(h, S)[1])             # (S, S, 3) indexed [x][y]
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
