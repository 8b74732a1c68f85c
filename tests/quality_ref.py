"""Face quality in plain numpy: the reference of csrc/trl_quality.h ("Face quality"), and the case tables the
CPU and GPU tests share.  Integers are int64; every float step is one numpy operation on float32 or float64 scalars, in the
header's order."""
import functools

import numpy as np

F32, F64, I64 = np.float32, np.float64, np.int64
RAW = ("n", "sum_y", "sum_y2", "sum_l", "sum_l2", "n_dark", "n_bright", "width")
FEAT = ("quality", "sharpness", "mean_luma", "dark_frac", "bright_frac", "contrast", "yaw", "pitch", "roll", "iod", "p05", "p95")
DEFAULTS = dict(sharp_ref=100.0, clip_ref=0.5, contrast_ref=64.0, yaw_ref=1.0, pitch_ref=1.0, size_ref=80.0)
H, W = 96, 128                                                              # the frames of the tables


# ---- the rules ----------------------------------------------------------------------------------------------------------------------
def _clamp(v, length: int) -> int:
    return 0 if v <= 0 else length if v >= length else int(v)


def rect_of(frame_of: int, n: int, H_: int, W_: int, box):
    """(status, (X0, Y0, X1, Y1))"""
    b = np.asarray(box, F32)
    if frame_of < 0 or frame_of >= n or not np.isfinite(b).all():
        return 0, (0, 0, 0, 0)
    X0, X1 = _clamp(np.floor(b[0]), W_), _clamp(np.ceil(b[2]), W_)
    Y0, Y1 = _clamp(np.floor(b[1]), H_), _clamp(np.ceil(b[3]), H_)
    if X1 <= X0 or Y1 <= Y0:
        return 0, (0, 0, 0, 0)
    return 1, (X0, Y0, X1, Y1)


def luma(bgr: np.ndarray) -> np.ndarray:
    p = bgr.astype(I64)
    return (1868 * p[..., 0] + 9617 * p[..., 1] + 4899 * p[..., 2] + 8192) >> 14


def reflect(i: np.ndarray, length: int) -> np.ndarray:
    """reflect-101 for -1 .. length: -1 -> 1, length -> length - 2; a single sample is its own neighbour"""
    i = np.asarray(i, I64)
    if length == 1:
        return np.zeros_like(i)
    return np.where(i < 0, 1, np.where(i >= length, length - 2, i))


def laplacian(Y: np.ndarray, y0: int = 0, y1: int | None = None) -> np.ndarray:
    """L of rows y0 .. y1 - 1 of the crop's luma Y, neighbours inside the crop"""
    h, w = Y.shape
    y1 = h if y1 is None else y1
    ys, xs = np.arange(y0, y1), np.arange(w)
    c = Y[ys]
    return Y[reflect(ys - 1, h)] + Y[reflect(ys + 1, h)] + c[:, reflect(xs - 1, w)] + c[:, reflect(xs + 1, w)] - 4 * c


def band_sums(Y: np.ndarray, y0: int, y1: int):
    """(hist[256], sum L, sum L^2) of rows y0 .. y1 - 1 of the crop"""
    L = laplacian(Y, y0, y1)
    return np.bincount(Y[y0:y1].reshape(-1), minlength=256).astype(I64), int(L.sum()), int((L * L).sum())


def raw_of(hist: np.ndarray, sl: int, sl2: int, width: int):
    """(raw[8], p05, p95) from the histogram and the Laplacian's sums"""
    v = np.arange(256, dtype=I64)
    n = int(hist.sum())
    cum = np.cumsum(hist)
    p05 = int(np.argmax(20 * cum >= n))
    p95 = int(np.argmax(20 * cum >= 19 * n))
    raw = np.array([n, (hist * v).sum(), (hist * v * v).sum(), sl, sl2, hist[:16].sum(), hist[240:].sum(), width], I64)
    return raw, p05, p95


def pose_of(pts) -> np.ndarray:
    """yaw, pitch, roll, iod in float32"""
    p = np.asarray(pts, F32)
    nan4 = np.full(4, np.nan, F32)
    if not np.isfinite(p).all():
        return nan4
    x, y = p[:5], p[5:]
    half, two, one = F32(0.5), F32(2), F32(1)
    ex, ey = x[1] - x[0], y[1] - y[0]
    with np.errstate(all="ignore"):
        e2 = ex * ex + ey * ey
        mx, my = (x[0] + x[1]) * half, (y[0] + y[1]) * half
        vx, vy = (x[3] + x[4]) * half - mx, (y[3] + y[4]) * half - my
        v2 = vx * vx + vy * vy
        if e2 == 0 or v2 == 0:
            return nan4
        iod = np.sqrt(e2)
        t = ((x[2] - x[0]) * ex + (y[2] - y[0]) * ey) / e2
        u = ((x[2] - mx) * vx + (y[2] - my) * vy) / v2
        return np.array([two * t - one, two * u - one, ey / iod, iod], F32)


def _pos(v):
    return v if v > 0 else F32(0)


def _unit_min(v):
    return F32(1) if v > 1 else v


def features(status: int, raw, p05: int, p95: int, height: int, pts, params=None) -> np.ndarray:
    prm = {k: F32(v) for k, v in {**DEFAULTS, **(params or {})}.items()}
    feat = np.zeros(12, F32)
    if not status:
        return feat
    n = F64(raw[0])
    a, b = F64(raw[4]) / n, F64(raw[3]) / n
    sharp = F32(a - b * b)
    mean, dark, bright = F32(F64(raw[1]) / n), F32(F64(raw[5]) / n), F32(F64(raw[6]) / n)
    contrast = F32(p95 - p05)
    pose, q_pose, one = np.full(4, np.nan, F32), F32(1), F32(1)
    with np.errstate(all="ignore"):
        if pts is not None:
            pose = pose_of(pts)
            q_pose = _pos(one - np.abs(pose[0]) / prm["yaw_ref"]) * _pos(one - np.abs(pose[1]) / prm["pitch_ref"])
        q_sharp = _unit_min(_pos(sharp) / prm["sharp_ref"])
        q_expo = _pos(one - (dark + bright) / prm["clip_ref"]) * _unit_min(contrast / prm["contrast_ref"])
        q_size = _unit_min(F32(min(int(raw[7]), height)) / prm["size_ref"])
        feat[0] = q_sharp * q_expo * q_pose * q_size
    feat[1:6] = sharp, mean, dark, bright, contrast
    feat[6:10] = pose
    feat[10:12] = p05, p95
    return feat


def quality_ref(frames: np.ndarray, frame_of, boxes, points=None, params=None) -> dict:
    """face_quality's outputs as numpy arrays: feat (m, 12), raw (m, 8), hist (m, 256), status (m,), and the features by name"""
    n, H_, W_, _ = frames.shape
    boxes = np.asarray(boxes, F32).reshape(-1, 4)
    m = len(boxes)
    out = dict(feat=np.zeros((m, 12), F32), raw=np.zeros((m, 8), I64), hist=np.zeros((m, 256), np.int32), status=np.zeros(m, np.int32))
    for r in range(m):
        status, (X0, Y0, X1, Y1) = rect_of(int(frame_of[r]), n, H_, W_, boxes[r])
        if not status:
            continue
        Y = luma(frames[int(frame_of[r]), Y0:Y1, X0:X1])
        hist, sl, sl2 = band_sums(Y, 0, Y1 - Y0)
        raw, p05, p95 = raw_of(hist, sl, sl2, X1 - X0)
        out["status"][r], out["raw"][r], out["hist"][r] = 1, raw, hist
        out["feat"][r] = features(1, raw, p05, p95, Y1 - Y0, None if points is None else points[r], params)
    out.update({name: out["feat"][:, i] for i, name in enumerate(FEAT)})
    return out


# ---- best shots -----------------------------------------------------------------------------------------------------------------------
def best_key(q, index: int) -> int:
    """trl_best_key (csrc/trl_bestkey.h): the larger quality wins, ties as floats (-0 == +0) go to the lower index, NaN is no candidate (0)"""
    q = F32(q)
    if np.isnan(q):
        return 0
    u = int(np.array(q, F32).view(np.uint32))
    negzero = int(u == 0x80000000)
    if negzero:
        u = 0
    ordered = (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)
    return (ordered << 32) | ((0x7FFFFFFF - index) << 1) | negzero


def best_update(keys: list, quality, gid, row_base: int, faces=None, best_faces=None) -> None:
    """one trl_best_update on host lists: pass 1 the keys, pass 2 the faces of the rows that are now their group's best"""
    G_ = len(keys)
    mine = [best_key(quality[r], row_base + r) for r in range(len(quality))]
    for r, k in enumerate(mine):
        if k and 0 <= gid[r] < G_:
            keys[gid[r]] = max(keys[gid[r]], k)
    if faces is not None:
        for r, k in enumerate(mine):
            if k and 0 <= gid[r] < G_ and keys[gid[r]] == k:
                best_faces[gid[r]] = faces[r]


def best_read(keys: list, quality_all) -> tuple:
    """(row (G,) int32, quality (G,) float32: the winner's own bits, NaN for none)"""
    row = np.array([-1 if k == 0 else 0x7FFFFFFF - ((k & 0xFFFFFFFF) >> 1) for k in keys], np.int32)
    q = np.array([np.nan if i < 0 else quality_all[i] for i in row], F32)
    return row, q


def best_brute(quality, gid, G_: int) -> np.ndarray:
    """the definition, without keys: per group the row of the largest quality, the first among equals, NaN never"""
    row = np.full(G_, -1, np.int32)
    for r in range(len(quality)):
        g, q = int(gid[r]), quality[r]
        if not 0 <= g < G_ or np.isnan(q):
            continue
        if row[g] < 0 or q > quality[row[g]]:
            row[g] = r
    return row


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the tables -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frame_batches() -> dict:
    """two batches of 4 x 96 x 128 BGR frames: flat -- constant, all 0, all 255, a 1-px checkerboard (|L| = 1020 everywhere); busy --
    noise, a horizontal ramp, coloured noise of low contrast, a diagonal ramp with its own colour per channel"""
    rng = np.random.default_rng(2024)
    yy, xx = np.mgrid[0:H, 0:W]
    flat = np.zeros((4, H, W, 3), np.uint8)
    flat[0] = (90, 140, 60)
    flat[2] = 255
    flat[3] = (((yy + xx) & 1) * 255)[..., None]
    busy = np.zeros((4, H, W, 3), np.uint8)
    busy[0] = rng.integers(0, 256, (H, W, 3))
    busy[1] = (xx * 2)[..., None]
    busy[2] = rng.integers(100, 140, (H, W, 3))
    busy[3] = np.stack([(xx + yy) % 256, (3 * xx + yy) % 256, (255 - 2 * yy) % 256], -1)
    for a in (flat, busy):
        a.setflags(write=False)
    return {"flat": flat, "busy": busy}


NAN, INF = float("nan"), float("inf")
# (name, frame, x1, y1, x2, y2); frame None: the row's index mod 4
RECTS = (
    ("1x1", None, 10, 10, 11, 11), ("1x5", None, 20, 30, 21, 35), ("5x1", None, 30, 40, 35, 41), ("2x2", None, 50, 50, 52, 52),
    ("3x3", None, 7, 7, 10, 10), ("w63", None, 1, 2, 64, 40), ("w64", None, 3, 5, 67, 41), ("w65", None, 0, 10, 65, 33),
    ("left", None, 0, 20, 30, 50), ("right", None, 100, 20, 128, 50), ("top", None, 40, 0, 70, 25), ("bottom", None, 40, 70, 70, 96),
    ("corner_tl", None, 0, 0, 9, 9), ("corner_tr", None, 119, 0, 128, 9), ("corner_bl", None, 0, 87, 9, 96),
    ("corner_br", None, 119, 87, 128, 96), ("larger", None, -10, -10, 200, 200), ("exact_frame", None, 0, 0, 128, 96),
    ("huge_finite", None, -1e30, -1e30, 1e30, 1e30), ("outside_right", None, 130, 10, 150, 30), ("outside_tl", None, -30, -30, -5, -5),
    ("outside_below", None, 10, 100, 30, 120), ("straddles", None, -5.5, 80.2, 20.7, 130), ("frac_out", None, 10.999, 20.001, 40.001, 50.999),
    ("frac_in", None, 11.0, 21.0, 40.0, 50.0), ("frac_1x1", None, 10.5, 20.5, 10.6, 20.6), ("empty", None, 30, 30, 30, 30),
    ("inverted", None, 50, 50, 40, 40), ("nan_x1", None, NAN, 1, 5, 5), ("inf_x2", None, 1, 1, INF, 5), ("ninf_x1", None, -INF, 1, 5, 5),
    ("nan_y2", None, 1, 1, 5, NAN), ("frame_-1", -1, 10, 10, 40, 40), ("frame_n", 4, 10, 10, 40, 40), ("frame_big", 2 ** 31 - 1, 10, 10, 40, 40),
    ("tall", None, 60, 0, 66, 96), ("wide", None, 0, 47, 128, 50), ("one_row_full", None, 0, 95, 128, 96), ("one_col_full", None, 127, 0, 128, 96),
)
NO_FACE = ("outside_right", "outside_tl", "outside_below", "empty", "inverted", "nan_x1", "inf_x2", "ninf_x1", "nan_y2", "frame_-1",
           "frame_n", "frame_big")


def rect_table():
    """(frame_of (m,) int32, boxes (m, 4) float32) of RECTS"""
    frame_of = np.array([i % 4 if r[1] is None else r[1] for i, r in enumerate(RECTS)], np.int32)
    return frame_of, np.array([r[2:] for r in RECTS], F32)


def _mirror(p, width=100.0):
    """the mirror image of a face: x -> width - x, and left and right trade names"""
    x, y = np.asarray(p[:5], F32), np.asarray(p[5:], F32)
    return list(F32(width) - x[[1, 0, 2, 4, 3]]) + list(y[[1, 0, 2, 4, 3]])


FRONTAL = [30, 70, 50, 35, 65, 40, 40, 60, 80, 80]                        # eyes, nose, mouth corners: x0..x4, y0..y4
TURNED = [30, 70, 58, 37, 66, 40, 43, 57, 80, 82]
# (name, points)
POINTS = (
    ("frontal", FRONTAL), ("turned", TURNED), ("turned_mirror", _mirror(TURNED)), ("nose_on_left_eye", [30, 70, 30, 35, 65, 40, 40, 40, 80, 80]),
    ("nose_on_right_eye", [30, 70, 70, 35, 65, 40, 40, 40, 80, 80]), ("nose_past_eye", [30, 70, 90, 35, 65, 40, 40, 55, 80, 80]),
    ("coincident_eyes", [50, 50, 50, 35, 65, 40, 40, 60, 80, 80]), ("mouth_on_eyes", [30, 70, 50, 30, 70, 40, 40, 60, 40, 40]),
    ("nan_point", [30, 70, NAN, 35, 65, 40, 40, 60, 80, 80]), ("inf_point", [30, 70, 50, 35, 65, 40, INF, 60, 80, 80]),
    ("fractional", [31.25, 69.5, 52.125, 36.75, 64.0625, 41.5, 39.25, 61.875, 79.5, 81.125]), ("rolled", [30, 60, 40, 20, 50, 40, 70, 60, 80, 95]),
    ("chin_down", [30, 70, 50, 35, 65, 40, 40, 78, 80, 80]),
)
NAN_POSE = ("coincident_eyes", "mouth_on_eyes", "nan_point", "inf_point")


def points_table() -> np.ndarray:
    return np.array([p for _, p in POINTS], F32)


PARAM_SETS = (None, dict(sharp_ref=2500.0, clip_ref=0.25, contrast_ref=200.0, yaw_ref=0.5, pitch_ref=0.75, size_ref=20.0),
              dict(sharp_ref=1e-3, size_ref=1.0, yaw_ref=3.0))


def best_qualities(m: int = 150, seed: int = 5) -> np.ndarray:
    """qualities with ties, NaN, -0 and +0, values repeated across the rows"""
    rng = np.random.default_rng(seed)
    q = rng.choice(np.array([0.0, -0.0, 0.25, 0.5, 0.5, 0.75, 1.0, np.nan, 0.1, -1.0], F32), m).astype(F32)
    q[:4] = [-0.0, 0.0, np.nan, -0.0]
    return q


BEST_SPLITS = ((0, 150), (0, 1, 2, 75, 75, 150), (0, 37, 64, 65, 129, 150))
