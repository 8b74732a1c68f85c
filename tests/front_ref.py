"""A plain restatement of the R-/O-Net front kernel (k_mtcnn_front, csrc/trl_front.hip) and the window table its tests share.

The kernel crops a window of a u8 frame, area-resamples it to S x S (S = 24 / 48), normalises, runs conv1 (3x3, 3 -> 28 / 32),
PReLU and MaxPool(3, 2, ceil), and writes only the pooled map.  Here the same operation is written from its definition:

  area_resample   adaptive-pool bins [floor(i a), ceil((i+1) a)), exact integer bin sums, ONE conversion to float32, / kh, / kw
                  in float32, (v - 127.5) * 0.0078125 -- and the float64 form next to it
  fma32 / conv1   acc = bias; k ascending; acc = fmaf(x[k], w[k], acc) with an exact fmaf (Python 3.10 has no math.fma: the
                  product of two float32 is exact in float64, TwoSum gives the sum's error, round-to-odd makes the final cast to
                  float32 a single rounding)
  prelu_pool      PReLU on the conv map, THEN the max pool, in the oracle's comparison order (not the kernel's pooled-PReLU identity)

front_path restates which of its code paths the kernel takes for a window.  There is no device-side plan to read back for this
kernel: every choice (small / big box, rows per bin, clamped loads, chunk count, segments, division) is made on the device from the
record alone, so the tests assert their coverage from this restatement, which is built from the kernel's constants (strip_caps
mirrors its constexpr arithmetic), as tests/test_gpu_pyramid.py does from the plan.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
NETS = {24: dict(C1=28, R=4, P=11, name="rnet"), 48: dict(C1=32, R=1, P=23, name="onet")}   # S -> conv1 channels, pooled rows per strip, pooled side
CLD = 36                 # channel stride of the conv1 strip
FASTDIV_BINS = 94        # fastdiv: ih <= 94 S and iw <= 94 S (every bin <= 96 x 96)
CSTRIDE = {True: 256, False: 252}   # payload bytes per chunk: same_phase / re-aligned


def strip_caps(S: int):
    """(COLCAP, CAP2) of the kernel: the per-wave column strip (words) and the half a bin pair's segment may fill."""
    R = NETS[S]["R"]
    CW, SR = S - 2, 2 * R + 1
    MROWS = (SR * CW + 15) & ~15
    COLCAP = min((MROWS * CLD - 16) // 4, 2048) & ~3
    return COLCAP, (COLCAP // 2) & ~3


def seg_limit(S: int) -> int:
    """Widest window (px) whose rows are ONE column segment: (iw - 0) * 3 <= CAP2 - 4."""
    return (strip_caps(S)[1] - 4) // 3


def bins(n: int, S: int):
    o = np.arange(S, dtype=np.int64)
    return (o * n) // S, -((-(o + 1) * n) // S)                 # floor(o n / S), ceil((o + 1) n / S)


# ---- crop + area resample + normalise --------------------------------------------------------------------------------------
def area_resample(img: np.ndarray, y0: int, x0: int, ih: int, iw: int, S: int):
    """img[y0:y0+ih, x0:x0+iw] pooled to S x S.  Returns (f32 form, f64 form, bin sums): the sums are exact integers (int64; the
    largest is 255 * ih * iw < 2^63), the f32 form converts each ONCE (round to nearest even, as the kernel's and the oracle's
    (float)uint32 does) and divides by kh, then by kw, in float32; the f64 form is (sum / (kh kw) - 127.5) / 128."""
    ys, ye = bins(ih, S)
    xs, xe = bins(iw, S)
    sums = np.zeros((S, S, 3), np.int64)
    for oy in range(S):
        col = img[y0 + ys[oy]:y0 + ye[oy], x0:x0 + iw].sum(axis=0, dtype=np.int64)          # (iw, 3)
        cs = np.concatenate([np.zeros((1, 3), np.int64), np.cumsum(col, axis=0)])
        sums[oy] = cs[xe] - cs[xs]
    kh, kw = (ye - ys), (xe - xs)
    v = sums.astype(F32) / kh.astype(F32)[:, None, None] / kw.astype(F32)[None, :, None]
    f32 = (v - F32(127.5)) * F32(0.0078125)
    assert f32.dtype == F32
    f64 = (sums.astype(np.float64) / (kh[:, None, None] * kw[None, :, None]).astype(np.float64) - 127.5) * 0.0078125
    return f32, f64, sums


def crop_f32_bound(max_bin_px: int) -> float:
    """Largest |f32 form - f64 form| of area_resample, u = 2^-24: the bin mean m <= 255 takes one relative rounding per division
    (two), one more for the conversion when the sum can pass 2^24 (bins of more than 65,793 px; exact below), so
    |m^ - m| <= 255 ((1 + u)^3 - 1); the subtraction rounds once more, <= u (127.5 + |m^ - m|); * 2^-7 is exact.  The f64 form's own
    rounding (a few 2^-53 relative) is covered by the last factor."""
    u = 2.0 ** -24
    k = 3 if max_bin_px * 255 >= 1 << 24 else 2
    dm = 255.0 * ((1 + u) ** k - 1)
    return (dm + u * (127.5 + dm)) * 2.0 ** -7 * (1 + 1e-9)


# ---- exact fused multiply-add in float32 -----------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf(a, b, c) for float32 arrays, one rounding: p = a b is exact in float64 (48 significant bits); s = fl(p + c) and its
    exact error e (TwoSum); when e != 0, s is replaced by the ODD one of the two float64 neighbours of the true sum (round to
    odd), whose round-to-nearest-even cast to float32 equals the true sum's (53 >= 24 + 2 bits).  Finite, non-overflowing inputs."""
    a, b, c = (np.asarray(v, F32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    s = np.ascontiguousarray(s)
    i = np.flatnonzero((e != 0).ravel())                          # inexact sums are rare: p has 48 bits, c 24
    if i.size:
        si, ei = s.ravel()[i], e.ravel()[i]
        even = (si.view(np.int64) & 1) == 0
        s.ravel()[i] = np.where(even, np.nextafter(si, np.where(ei > 0, np.inf, -np.inf)), si)
    return s.astype(F32)


def conv1(crop: np.ndarray, w: np.ndarray, b: np.ndarray) -> np.ndarray:
    """3x3 valid conv of crops (n, S, S, 3) with w [27][C1], k = (ky * 3 + kx) * 3 + c: acc = bias, k ascending, fmaf."""
    n, S = crop.shape[:2]
    CW, C1 = S - 2, w.shape[1]
    out = np.empty((n, CW, CW, C1), F32)
    for i0 in range(0, n, 8):                                     # a few crops at a time: the temporaries stay in cache
        x = crop[i0:i0 + 8]
        acc = np.broadcast_to(b.astype(F32), (len(x), CW, CW, C1)).copy()
        for k in range(27):
            ky, kx, c = k // 9, (k // 3) % 3, k % 3
            acc = fma32(x[:, ky:ky + CW, kx:kx + CW, c, None], w[k][None, None, None, :], acc)
        out[i0:i0 + 8] = acc
    return out


def prelu_pool(a: np.ndarray, slope: np.ndarray) -> np.ndarray:
    """PReLU (v > 0 ? v : slope v, float32) of the conv map (n, CW, CW, C), then MaxPool(3, 2, ceil_mode): windows clipped to the
    map, the running maximum starts at -inf and takes a tap only when it is GREATER (the oracle's order: zeros keep their sign)."""
    with np.errstate(invalid="ignore"):
        v = np.where(a > 0, a, (slope.astype(F32)[None, None, None, :] * a).astype(F32)).astype(F32)
    n, CW, _, C = v.shape
    P = -(-(CW - 3) // 2) + 1
    if (P - 1) * 2 >= CW:
        P -= 1
    out = np.full((n, P, P, C), -np.inf, F32)
    for ky in range(3):
        for kx in range(3):
            tap = v[:, ky::2, kx::2][:, :P, :P]                     # rows 2 p + ky that exist
            sub = out[:, :tap.shape[1], :tap.shape[2]]
            np.copyto(sub, tap, where=tap > sub)
    return out


def front(crops: np.ndarray, tensors: dict, S: int) -> np.ndarray:
    """The pooled map of prepared crops (n, S, S, 3) under the unpacked weight tensors (weights.unpack_tensors)."""
    nm = NETS[S]["name"]
    return prelu_pool(conv1(crops, tensors[f"{nm}.conv1.w"], tensors[f"{nm}.conv1.b"]), tensors[f"{nm}.prelu1"])


# ---- which code path the kernel takes --------------------------------------------------------------------------------------
def front_path(window, nf: int, H: int, W: int, S: int) -> dict:
    """The kernel's dispatch for window (frame, y0, x0, ih, iw) of an nf-frame batch of H x W frames, restated line by line:
      kind        "small" (ih, iw <= 3 S: one thread per output pixel), "wide" (a bin wider than half the strip: one bin per wave)
                  or "big" (column sums)
      rows        small: the ROWS instantiation (2, 3, 4; the clamped form is 4)
      fb3         byte phase of the frame's first byte (small path)
      safe        set of the SAFE template values over the window's passes ({True}, {False} or both)
      same_phase  big: row pitch % 4 == 0
      segments    big: column segments per row pair
      nch         big: set of (chunk count, instantiated NCH) over the passes (a clamped pass is instantiated with 4)
      passes      big: largest number of c0 iterations of one segment
      fastdiv     big: the reciprocal division is allowed
      max_bin     pixels of the largest bin"""
    f, y0, x0, ih, iw = (int(v) for v in window)
    total = nf * H * W * 3
    fbyte0 = f * H * W * 3
    last_dw = (total - 1) >> 2
    ys, ye = bins(ih, S)
    xs, xe = bins(iw, S)
    out = dict(max_bin=int((ye - ys).max() * (xe - xs).max()), fb3=fbyte0 & 3)
    if ih <= 3 * S and iw <= 3 * S:
        khmax_c = (ih + S - 1) // S + 1
        far = fbyte0 + ((y0 + ih - 1) * W + x0 + iw) * 3 + 16
        safe = far <= total
        out.update(kind="small", safe={safe}, rows=4 if not safe else min(max(khmax_c, 2), 4))
        return out
    CAP2 = strip_caps(S)[1]
    same_phase = (W * 3) % 4 == 0
    kwA0 = (iw + S - 1) // S
    out.update(same_phase=same_phase, fastdiv=ih <= FASTDIV_BINS * S and iw <= FASTDIV_BINS * S)
    if (kwA0 + 1) * 3 > CAP2 - 4:
        out.update(kind="wide")
        return out
    cstride = CSTRIDE[same_phase]
    safes, nchs, segs, passes = set(), set(), 0, 0
    for oyA in (o for o in range(S) if o % 8 < 4):
        oyB = oyA + 4
        khB = int(ye[oyB] - ys[oyB])
        oxa, nseg = 0, 0
        while oxa < S:
            xsa = (oxa * iw) // S
            oxb = oxa + 1
            if (iw - xsa) * 3 <= CAP2 - 4:
                oxb = S
            else:
                while oxb < S and (-(-(oxb + 1) * iw // S) - xsa) * 3 <= CAP2 - 4:
                    oxb += 1
            xeb = -(-oxb * iw // S)
            seg_bytes = (xeb - xsa) * 3
            assert seg_bytes <= CAP2 - 4, "a segment outgrew the strip half"
            o_segA = fbyte0 + ((y0 + int(ys[oyA])) * W + x0 + xsa) * 3
            o_segB = fbyte0 + ((y0 + int(ys[oyB])) * W + x0 + xsa) * 3
            sh0 = (o_segA & 3) if same_phase else 0
            span = seg_bytes + sh0
            np_ = 0
            for c0 in range(0, span, 4 * cstride):
                rem = span - c0
                nch = 1 + (rem > cstride) + (rem > 2 * cstride) + (rem > 3 * cstride)
                o_far = o_segB + (khB - 1) * W * 3 - sh0 + c0 + (nch - 1) * cstride + 255
                safe = (o_far >> 2) <= last_dw
                safes.add(safe)
                nchs.add((nch, nch if safe else 4))
                np_ += 1
            passes = max(passes, np_)
            nseg += 1
            oxa = oxb
        segs = max(segs, nseg)
    out.update(kind="big", safe=safes, nch=nchs, segments=segs, passes=passes)
    return out


# ---- the window table ------------------------------------------------------------------------------------------------------
def window_sizes(H: int, W: int, S: int) -> list:
    """(ih, iw) of the table, before placement; sizes the frame cannot hold are dropped."""
    L = seg_limit(S)
    big = 3 * S + 1
    sizes = [(s, s) for s in (1, 2, S - 1, S, S + 1, 2 * S, 2 * S + 1, 3 * S, 3 * S + 1)]
    for cs in CSTRIDE.values():                                  # either side of every chunk-count threshold (span = 3 iw + phase)
        for k in (1, 2, 3):
            t = k * cs // 3
            sizes += [(big, t - 1), (big, t), (big, t + 1)]
    sizes += [(big, L), (big, L + 1), (big, 2 * L + 1)]           # 1 | 2 | 3 column segments
    sizes += [(H, W), (H, 1), (1, W), (1, big), (big, 1), (S - 1, big), (big, S - 1), (2, W), (H, 2)]
    out = []
    for s in sizes:
        if 1 <= s[0] <= H and 1 <= s[1] <= W and s not in out:
            out.append(s)
    return out


def window_table(H: int, W: int, S: int) -> list:
    """Windows (y0, x0, ih, iw) of an H x W frame: window_sizes at the four frame corners and once inside, then a small and a big
    window with x0 through all four residues mod 4; duplicates dropped, order fixed."""
    out, seen = [], set()

    def add(y0, x0, ih, iw):
        r = (y0, x0, ih, iw)
        if r not in seen and 0 <= y0 and 0 <= x0 and y0 + ih <= H and x0 + iw <= W:
            seen.add(r)
            out.append(r)

    for ih, iw in window_sizes(H, W, S):
        for y0, x0 in ((0, 0), (0, W - iw), (H - ih, 0), (H - ih, W - iw), ((2 * (H - ih)) // 5, (W - iw) // 3)):
            add(y0, x0, ih, iw)
    for ih, iw in ((S + 1, S + 1), (3 * S + 1, 3 * S + 1), (min(H, 3 * S + 1), min(W, 86))):
        for r in range(4):
            add(min(3, H - ih), 4 + r, ih, iw)
            add(H - ih, W - iw - r, ih, iw)
    return out


def content_frames(kind: str, k: int, H: int, W: int, seed: int) -> np.ndarray:
    """k frames (k, H, W, 3) u8: random bytes, all 0, all 255, a 1-px checkerboard -- or "same": random, every frame alike."""
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, (k, H, W, 3), dtype=np.uint8)
    if kind == "same":
        return np.ascontiguousarray(np.broadcast_to(np.random.default_rng(seed).integers(0, 256, (1, H, W, 3), dtype=np.uint8), (k, H, W, 3)))
    if kind == "zeros":
        return np.zeros((k, H, W, 3), np.uint8)
    if kind == "ones":
        return np.full((k, H, W, 3), 255, np.uint8)
    assert kind == "checker"
    f, y, x = np.ogrid[:k, :H, :W]
    return np.ascontiguousarray(np.broadcast_to(((((f + y + x) & 1) * 255).astype(np.uint8))[..., None], (k, H, W, 3)))


# (nf, H, W): 360 x 640; the four row-pitch phases (at 333 a frame is 1 mod 4 bytes: five frames give fb3 = 0, 1, 2, 3, 0); the
# API's minimum; and two frames that are tiny in bytes but longer than 94 S px in one direction for both nets
BATCHES = ((3, 360, 640), (2, 211, 332), (5, 211, 333), (2, 211, 334), (2, 211, 335), (3, 12, 12), (2, 40, 4700), (2, 4700, 40))
HUGE = (1, 2500, 16383)      # R-Net only: the full-frame window has bins of ~71,700 px, whose sums pass 2^24, 683 px wide


WIDE = (2, 12, 16383)        # both nets: 590 KB a frame, yet wider than the widest window whose bins fit half the column strip


def wide_limit(S: int) -> int:
    """Widest window (px) that still takes the column sums: (ceil(iw / S) + 1) * 3 <= CAP2 - 4."""
    return (seg_limit(S) - 1) * S


def wide_records(S: int) -> np.ndarray:
    """Records of the WIDE batch: the widths on either side of wide_limit at the frame's left and right edge, and the full frame,
    each on frame 0 and on the last frame, where the right-edge windows end at the buffer's last byte."""
    nf, H, W = WIDE
    L = wide_limit(S)
    rec = []
    for f in (0, nf - 1):
        rec += [(f, 0, 0, H, L), (f, 0, 0, H, L + 1), (f, 0, W - L, H, L), (f, 0, W - L - 1, H, L + 1), (f, 0, 0, H, W), (f, H - 1, W - L - 1, 1, L + 1)]
    return np.array(rec, np.int32)


def placed(nf: int, H: int, W: int, S: int) -> np.ndarray:
    """The table as records (frame, y0, x0, ih, iw): windows go round the frames, and every window that ends at the frame's
    bottom-right corner, plus a small and a big one, is ALSO placed on frame 0 and on the last frame (unclamped / clamped loads)."""
    rec = []
    for i, (y0, x0, ih, iw) in enumerate(window_table(H, W, S)):
        fs = {i % nf}
        if (y0 + ih == H and x0 + iw == W) or (ih, iw) in ((S + 1, S + 1), (3 * S + 1, 3 * S + 1)):
            fs |= {0, nf - 1}
        rec += [(f, y0, x0, ih, iw) for f in sorted(fs)]
    return np.array(rec, np.int32)


SLOPE_VARIANTS = ("seeded", "slopes_above_one", "negative_slopes", "mixed_signs", "zero_one_slopes")   # MODE 2, 1, 0, 0, 2


def slope_blob(variant: str) -> bytes:
    """The packed weights of a conv1 slope class: the seeded ones, the variants of slope_variants.py, or conv1 slopes that include
    exactly 0.0, 1.0 and -0.0 (still the [0, 1] class: -0.0 >= 0)."""
    import truely_amd
    from truely_amd import weights
    if variant == "seeded":
        return weights.synthetic_blob(0)
    if variant != "zero_one_slopes":
        from slope_variants import slope_variant_blob
        return slope_variant_blob(variant)
    sds = [dict(sd) for sd in weights.synthetic_state_dicts(0)]
    for net in (sds[1], sds[2]):
        w = np.array(net["prelu1.weight"], np.float32, copy=True)
        w[0::4] = 0.0; w[1::4] = 1.0; w[2::4] = -0.0
        net["prelu1.weight"] = w
    return weights.pack_state_dicts(*sds)
