"""Plain restatement of the list post-processing of detect_face() (facenet_pytorch utils/detect_face.py) and MTCNN.detect's
selection, with server/model.py:49-54 -- the reference the list-kernel tests (test_lists_cpu.py, test_gpu_lists.py) compare the
cascade's k_nms_level / k_nms_frame / k_stage2_post / k_stage3_post / k_select with.  TEST INFRASTRUCTURE ONLY.

numpy / torch float32, one rounding per operation, in the reference's operation order; NMS, bbreg, rerec and pad are
oracle/torch_ref.py's.  `route` restates how the cascade's host code sends a list to an LDS tier or to the spill tier
(trl_cascade.hip: list_launch, k_nms_level, sort_and_suppress, big_greedy), so a test can show that a case reaches the edge it names.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle.torch_ref import _bbreg, _nms_iou, _nms_min, _pad, _rerec

F32 = np.float32
CAND = np.dtype([("box", F32, 4), ("score", F32), ("reg", F32, 4), ("cell", np.int32)])   # trl_ctx.h Cand, 40 bytes


def probs(expf, logits):
    """prob[:, 1] of the 2-way softmax of logits[:, 0:2] as the oracle computes it (softmax2_p1: max, orc_expf, one f32 division);
    expf = the oracle's orc_expf."""
    lg = np.asarray(logits, F32).reshape(len(logits), -1)
    out = np.empty(len(lg), F32)
    with np.errstate(over="ignore"):                          # a0 - m may overflow to -inf, as in C: orc_expf clamps it
        for i in range(len(lg)):
            a0, a1 = lg[i, 0], lg[i, 1]
            m = max(a0, a1)
            e0 = F32(expf(float(F32(a0 - m))))
            e1 = F32(expf(float(F32(a1 - m))))
            out[i] = F32(e1 / F32(e0 + e1))
    return out


def pad_ok(rows, W, H):
    """detect_face's crop test after pad(): ey > y - 1 and ex > x - 1 (trunc, clamp to [1, W] / [1, H])."""
    if len(rows) == 0:
        return np.zeros(0, bool)
    y, ey, x, ex = _pad(torch.as_tensor(np.ascontiguousarray(rows[:, :4], F32)), W, H)
    return (ey > y - 1) & (ex > x - 1)


def level_nms(rec):
    """batched_nms(0.5) of one (frame, level): detect_face lists a level's candidates in raster (cell) order, torchvision sorts
    them stably by descending score.  Returns indices into `rec` (any append order) in pick order."""
    if len(rec) == 0:
        return np.zeros(0, np.int64)
    order = np.argsort(rec["cell"], kind="stable")
    b = np.ascontiguousarray(rec["box"][order], F32)
    keep = _nms_iou(torch.as_tensor(b), torch.as_tensor(np.ascontiguousarray(rec["score"][order])), 0.5).numpy()
    return order[keep]


def stage1(recs, picks, W, H):
    """Per-frame batched_nms(0.7) over the concatenated per-level picks, PNet regression (widths without +1), rerec, pad test.
    recs / picks: per level, records and their pick lists.  Returns the stage-1 rows (x1, y1, x2, y2, score)."""
    parts = [r[p] for r, p in zip(recs, picks) if len(p)]
    if not parts:
        return np.zeros((0, 5), F32)
    allb = np.concatenate(parts)
    box = torch.as_tensor(np.ascontiguousarray(allb["box"], F32))
    pick = _nms_iou(box, torch.as_tensor(np.ascontiguousarray(allb["score"])), 0.7).numpy()
    b, s, r = box[pick], torch.as_tensor(allb["score"][pick]), torch.as_tensor(np.ascontiguousarray(allb["reg"][pick]))
    regw = b[:, 2] - b[:, 0]
    regh = b[:, 3] - b[:, 1]
    rows = torch.stack([b[:, 0] + r[:, 0] * regw, b[:, 1] + r[:, 1] * regh, b[:, 2] + r[:, 2] * regw, b[:, 3] + r[:, 3] * regh, s], 1)
    rows = _rerec(rows.contiguous()).numpy()
    return rows[pad_ok(rows, W, H)].astype(F32)


def stage2(rows1, prob, reg, W, H, thr=0.7):
    """R-Net tail: prob > thr, batched_nms(0.7) on the stage-1 boxes, bbreg (+1 widths), rerec, pad test.  Rows carry prob."""
    ipass = np.flatnonzero(prob > F32(thr))
    if len(ipass) == 0:
        return np.zeros((0, 5), F32)
    b = torch.as_tensor(np.ascontiguousarray(rows1[ipass, :4], F32))
    p = torch.as_tensor(np.ascontiguousarray(prob[ipass], F32))
    pick = _nms_iou(b, p, 0.7)
    rows = torch.cat([b[pick], p[pick].unsqueeze(1)], 1)
    rows = _rerec(_bbreg(rows, torch.as_tensor(np.ascontiguousarray(reg[ipass], F32))[pick])).numpy()
    return rows[pad_ok(rows, W, H)].astype(F32)


def stage3(rows2, prob, reg, pts, thr=0.7):
    """O-Net tail: prob > thr, bbreg (+1 widths), landmarks on the stage-2 boxes, nms 'Min' 0.7 (ties: higher index first).
    Returns (rows (x1, y1, x2, y2, prob), points x0..x4, y0..y4) in pick order."""
    ipass = np.flatnonzero(prob > F32(thr))
    if len(ipass) == 0:
        return np.zeros((0, 5), F32), np.zeros((0, 10), F32)
    b2 = np.ascontiguousarray(rows2[ipass, :4], F32)
    rows = torch.cat([torch.as_tensor(b2), torch.as_tensor(prob[ipass]).unsqueeze(1)], 1)
    rows = _bbreg(rows, torch.as_tensor(np.ascontiguousarray(reg[ipass], F32))).numpy()
    w = b2[:, 2] - b2[:, 0] + F32(1)
    h = b2[:, 3] - b2[:, 1] + F32(1)
    pt = np.asarray(pts, F32)[ipass]
    px = w[:, None] * pt[:, :5] + b2[:, 0:1] - F32(1)
    py = h[:, None] * pt[:, 5:] + b2[:, 1:2] - F32(1)
    pick = _nms_min(rows[:, :4], rows[:, 4], 0.7)
    return rows[pick].astype(F32), np.concatenate([px, py], 1)[pick].astype(F32)


def select(rows3, pts3, W, H, max_faces):
    """MTCNN.detect(select_largest=True): argsort(area)[::-1] (ties: higher index first); then model.py:49-54 on boxes[0]:
    astype(int) (toward zero), clamp to the frame, box[2] > box[0] and box[3] > box[1]."""
    n = len(rows3)
    out = {"count": min(n, max_faces), "boxes": np.zeros((0, 4), F32), "probs": np.zeros(0, F32), "points": np.zeros((0, 10), F32),
           "box0": np.zeros(4, F32), "prob0": F32(0), "rect": np.zeros(4, np.int32), "valid": 0}
    if n == 0:
        return out
    area = (rows3[:, 2] - rows3[:, 0]) * (rows3[:, 3] - rows3[:, 1])
    order = np.argsort(area, kind="stable")[::-1]
    top = order[:max_faces]
    out.update(boxes=rows3[top, :4], probs=rows3[top, 4], points=pts3[top], box0=rows3[order[0], :4], prob0=rows3[order[0], 4])
    box = rows3[order[0], :4].astype(np.int64)
    box[0] = max(0, box[0]); box[1] = max(0, box[1]); box[2] = min(W, box[2]); box[3] = min(H, box[3])
    out["rect"] = box.astype(np.int32)
    out["valid"] = int(box[2] > box[0] and box[3] > box[1])
    return out


# ---- routing of a list through the list kernels (trl_cascade.hip) ----
def next_pow2(n):
    p = 2
    while p < n:
        p <<= 1
    return p


def pow2_floor(n):
    p = 1
    while 2 * p <= n:
        p <<= 1
    return p


def launch(small, full, capl, capF):
    """list_launch(): LDS tiers and workgroup sizes for the level capacities capl and the per-frame capacity capF."""
    small = min(small, full)
    max_capl = max([4] + list(capl))
    full_l, full_f = min(max_capl, full), min(capF, full)
    return {"max_capl": max_capl, "full_l": full_l, "full_f": full_f, "small_cap": min(full_l, small),
            "th_l": 1024 if max_capl > full else 256, "th_f": 1024 if capF > full else 256}


def route(ll, cnt, level=True):
    """Which path a list of cnt entries takes: ("small" | "full" | "spill", threads, P = sorted slots, C = spill chunk or 0,
    TK = 'Min' tile of the spill tier or 0).  level: k_nms_level (two launches); otherwise k_nms_frame / k_stage2_post /
    k_stage3_post (one launch, LDS tier full_f)."""
    if level:
        if cnt <= ll["small_cap"]:
            return ("small", 256, next_pow2(cnt), 0, 0)
        cap, th = ll["full_l"], ll["th_l"]
    else:
        cap, th = ll["full_f"], ll["th_f"]
    if cnt <= cap:
        return ("full" if level else "lds", th, next_pow2(cnt), 0, 0)
    C = pow2_floor(cap)
    return ("spill", th, next_pow2(cnt), C, C * 8 // 20)


def spill_bytes(kind, part, cnt, W, H):
    """Bytes one spilled list of cnt entries takes from the spill pool (trl_cascade.hip: SpillWs::bytes, spill_alloc): sort keys
    and payloads for P = next_pow2(cnt) slots (12 bytes each), kept box + area per entry (20 bytes) plus the grid's `next` link
    (4) where the NMS is torchvision's -- kinds 1 and 2 -- and a kept-payload array of its own (4) where the list is not written
    straight into the kernel's output -- every list but k_nms_level's --, the grid's heads (one int per 32-px cell of the frame,
    kinds 1 and 2), rounded up to 256.  kind 1: part "level" = k_nms_level, "frame" = k_nms_frame."""
    entry = 24 if (kind == 1 and part == "level") or kind == 3 else 28
    grid = 0 if kind == 3 else ((W >> 5) + 1) * ((H >> 5) + 1) * 4
    return (next_pow2(cnt) * 12 + cnt * entry + grid + 255) // 256 * 256


# ---- lists built to sit on the kernels' edges ----
# A list is (boxes [n][4], rank [n]): rank 0 sorts first (highest score).  Families, all inside a W x H frame with 32-px grid cells:
#   "dup"   ceil(n/2) boxes 6 x 6 centred on a lattice of 8 px whose every fourth line is a cell edge (some centres past the frame,
#           in the clamped border cells), all kept, then a 1-px shifted copy of each in the same order: every copy is suppressed by
#           exactly its original, so a kept box missed by a tile, a chunk or a grid window shows up as a surviving copy;
#   "chain" chains of three 10 x 10 boxes on a 16-px lattice, step STEP[mode] px: A suppresses B, B would suppress C, so C is kept -- chunk edges fall
#           inside chains;
#   "cell"  1 x 1 boxes, 1024 per cell (one cell holds a long chain of kept boxes), then 1/8-px shifted copies.
# SPECIAL = boxes placed in a region the families leave empty: exact score ties, overlaps exactly at the threshold in f32,
# degenerate boxes (zero width, x2 < x1) and sub-pixel boxes whose pad() window is one pixel.
W0, H0 = 640, 480
HOLE = (256, 128, 448, 224)          # x0, y0, x1, y1 of the region the families leave to SPECIAL
STEP = {0.5: 3.0, 0.7: 1.0, "min": 3.0}   # chain steps: IoU(A, B) above the threshold, IoU(A, C) below


def _in_hole(cx, cy, pad=8):
    return HOLE[0] - pad <= cx < HOLE[2] + pad and HOLE[1] - pad <= cy < HOLE[3] + pad


def _lattice(W, H):
    pts = [(32 * i + 8 * a, 32 * j + 8 * b) for j in range(-1, H // 32 + 2) for i in range(-1, W // 32 + 2) for b in range(4) for a in range(4)]
    return [p for p in pts if not _in_hole(*p)]


def family(name, n, mode, W=W0, H=H0, seed=0):
    rng = np.random.default_rng(seed + 7919 * n)
    m = (n + 1) // 2
    if name == "dup":
        pts = _lattice(W, H)
        assert m <= len(pts), (n, len(pts))
        sel = rng.permutation(len(pts))[:m]
        c = np.array([pts[k] for k in sel], F32)
        base = np.stack([c[:, 0] - 3, c[:, 1] - 3, c[:, 0] + 3, c[:, 1] + 3], 1)
        boxes = np.concatenate([base, base[:n - m] + F32([1, 0, 1, 0])])
    elif name == "cell":
        k = np.arange(m)
        x = F32(64 + 32 * (k // 1024)) + (k % 32).astype(F32)
        y = F32(64) + ((k // 32) % 32).astype(F32)
        base = np.stack([x, y, x + 1, y + 1], 1).astype(F32)
        boxes = np.concatenate([base, base[:n - m] + F32([0.125, 0, 0.125, 0])])
    elif name == "chain":
        s = F32(STEP[mode])
        pts = [p for p in _lattice(W, H) if p[0] % 16 == 0 and p[1] % 16 == 0]
        k = np.arange(n)
        perm = rng.permutation(len(pts))
        c = np.array([pts[perm[q]] for q in k // 3], F32)
        assert n <= 3 * len(pts)
        x = c[:, 0] - 8 + (k % 3).astype(F32) * s
        boxes = np.stack([x, c[:, 1] - 5, x + 10, c[:, 1] + 5], 1).astype(F32)
    else:
        raise ValueError(name)
    return boxes.astype(F32), np.arange(n)


def special(mode):
    """(boxes, rank) of the edge cases of one NMS mode, in the HOLE region; equal ranks are exact ties."""
    ox, oy = F32(HOLE[0] + 8), F32(HOLE[1] + 8)
    B, R = [], []

    def add(b, r):
        B.append(np.asarray(b, F32) + F32([ox, oy, ox, oy])); R.append(r)
    # exact ties: pairs and a triple of overlapping boxes with one score -- the tie rule alone decides which survives
    add([0, 0, 10, 10], 0); add([1, 0, 11, 10], 0)
    add([20, 0, 30, 10], 1); add([20, 1, 30, 11], 1); add([20, 2, 30, 12], 1)
    # overlap exactly at the threshold in f32: kept (the suppression test is strict), and one just above: suppressed
    if mode == 0.5:
        add([40, 0, 44, 4], 2); add([40, 0, 44, 2], 3)            # IoU 8 / 16 = 0.5
        add([50, 0, 54, 4], 2); add([50, 0, 54, 2.125], 3)        # 8.5 / 16 > 0.5
    elif mode == 0.7:
        add([40, 0, 50, 1], 2); add([40, 0, 47, 1], 3)            # IoU 7 / 10 = 0.7f
        add([40, 4, 50, 5], 2); add([40, 4, 47.125, 5], 3)        # 7.125 / 10 > 0.7
    else:
        add([40, 0, 49, 0], 2); add([43, 0, 52, 0], 3)            # 'Min': (7 x 1) / 10 = 0.7f, kept
        add([40, 4, 49, 4], 2); add([42, 4, 51, 4], 3)            # 8 / 10, suppressed
    # degenerate boxes: zero width (twice the same), x2 < x1, y2 < y1, both; a box inside a degenerate one's span
    add([60, 0, 60, 10], 4); add([60, 0, 60, 10], 5)
    add([70, 0, 65, 10], 4); add([66, 2, 69, 8], 6)
    add([80, 10, 90, 5], 5); add([85, 0, 75, -5], 6)
    # sub-pixel boxes: trunc(y1) == trunc(y2), trunc(x1) == trunc(x2) -- pad() leaves a one-pixel window
    add([100.25, 0.25, 100.75, 0.75], 7); add([110.5, 3.5, 110.875, 3.625], 8)
    # a box that contains a later one entirely, and a long thin one crossing several
    add([120, 0, 160, 40], 9); add([130, 10, 140, 20], 10); add([118, 18, 170, 22], 11)
    return np.array(B, F32), np.array(R, np.int64)


def make_list(fam, n, mode, seed=0):
    """One list of n boxes: a family, or "special" padded to n with a "dup" filler ranked around it."""
    if fam != "special":
        return family(fam, n, mode, seed=seed)
    sb, sr = special(mode)
    if n <= len(sb):
        return sb[:n], sr[:n]
    fb, fr = family("dup", n - len(sb), mode, seed=seed)
    # specials spread through the filler's order (every ~n/len(sb) ranks), ties kept
    step = max(1, (n - len(sb)) // (int(sr.max()) + 2))
    rank = np.concatenate([fr * 2 + 1, sr * 2 * step])
    return np.concatenate([fb, sb]), rank


def scores_from_rank(rank, lo=0.61, hi=0.99):
    """Probabilities (f32, distinct per rank, exact ties for equal ranks) descending with the rank."""
    u = np.unique(rank)
    v = np.linspace(hi, lo, len(u)).astype(F32)
    return v[np.searchsorted(u, rank)]


def logits_from_rank(rank, lo=1.0, hi=6.0, below=()):
    """Logit pairs (0, t): t descending with the rank; entries listed in `below` get t = -1 (probability under 0.7)."""
    u = np.unique(rank)
    t = np.linspace(hi, lo, len(u)).astype(F32)[np.searchsorted(u, rank)]
    t[list(below)] = F32(-1)
    return np.stack([np.zeros_like(t), t], 1)


def _round4(k):
    return max(4, (int(k) + 3) // 4 * 4)


def _records(boxes, rank, rng, reg=True):
    rec = np.zeros(len(boxes), CAND)
    rec["box"] = boxes
    rec["score"] = scores_from_rank(rank)
    if reg:                                                   # PNet offsets, exact in f32; some boxes keep theirs
        rec["reg"] = rng.integers(-3, 4, (len(boxes), 4)).astype(F32) / F32(64)
    rec["cell"] = rng.permutation(8 * len(boxes) + 8)[:len(boxes)]   # distinct cells, not in score order
    return rec


SELECT_FRAMES = [   # stage-2 rows of extra frames of a kind-3 case (probability ranks, all above the threshold, no overlaps)
    # largest box entirely left of / above the frame with fractional negative x2, y2: astype(int) toward zero -> rect 0, invalid
    [([-20.5, -20.5, -0.5, -0.5], 0), ([10, 10, 20, 20], 1), ([40, 10, 45, 15], 2)],
    # two largest boxes of equal area (ties: the higher index ranks first), a third one smaller
    [([10, 10, 30, 30], 0), ([100, 10, 120, 30], 1), ([200, 10, 219, 30], 0)],
    # the largest box past the right and bottom edges (clamped to W, H), fractional
    [([600.7, 440.2, 660.9, 500.6], 1), ([10.9, 10.1, 30.2, 30.8], 0)],
    [],                                                       # no stage-2 rows at all
]


def build_case(kind, fam, n, part="level", seed=0, W=W0, H=H0):
    """A hook input: dict(kind, W, H, caps, counts, rows, logits) and what it is built to reach.  kind 1 part "level": one
    level holds the family list of n records (batched_nms 0.5), a second level the special list; part "frame": the list is
    spread over three levels so that no level suppresses anything and the per-frame list holds exactly n entries."""
    rng = np.random.default_rng(seed * 1000003 + n * 31 + len(fam) + kind)
    if kind == 1:
        if part == "level":
            b, r = make_list(fam, n, 0.5, seed)
            sb, sr = special(0.5)
            lv = [(b, r), (sb, sr)]
        else:
            b, r = make_list(fam, n, 0.7, seed)
            m = (n + 1) // 2
            lvl = np.arange(n) % 3 if fam == "chain" else (np.arange(n) >= m).astype(int)
            lv = [(b[lvl == q], r[lvl == q]) for q in range(3)]
        recs = [_records(bb, rr, rng, reg=(q == 0)) for q, (bb, rr) in enumerate(lv)]
        caps = [_round4(len(x)) for x in recs]
        capF = _round4(sum(len(x) for x in recs))
        return {"kind": 1, "W": W, "H": H, "caps": caps + [capF], "counts": np.array([[len(x) for x in recs]], np.int32),
                "recs": [recs], "n": n, "fam": fam, "part": part}
    mode = 0.7 if kind == 2 else "min"
    b, r = make_list(fam, n, mode, seed)
    frames = [(b, r)]
    if kind == 3 and fam == "special":
        frames += [(np.array([q[0] for q in fr], F32).reshape(-1, 4), np.array([q[1] for q in fr], np.int64)) for fr in SELECT_FRAMES]
    rows, lg, counts = [], [], []
    for fb, fr in frames:
        k = len(fb)
        below = [i for i in range(k) if i % 11 == 5] if fam != "special" or k != len(b) else []
        lt = logits_from_rank(fr, below=below) if k else np.zeros((0, 2), F32)
        no = 6 if kind == 2 else 16
        L = np.zeros((k, no), F32)
        L[:, :2] = lt
        L[:, 2:6] = rng.integers(-2, 3, (k, 4)).astype(F32) / F32(32) * (np.arange(k) % 3 == 0)[:, None]
        if kind == 3:
            L[:, 6:] = rng.integers(0, 17, (k, 10)).astype(F32) / F32(16)
        rows.append(np.concatenate([fb, scores_from_rank(fr)[:, None] if k else np.zeros((0, 1), F32)], 1).astype(F32))
        lg.append(L); counts.append(k)
    capF = _round4(max(counts))
    return {"kind": kind, "W": W, "H": H, "caps": [capF], "counts": np.array(counts, np.int32), "rows": rows, "logits": lg,
            "n": n, "fam": fam}


# Logit differences d = a1 - a0 that walk trl_softmax2_p1 over its whole range: equal logits, the smallest denormal, a difference
# that rounds away next to 1, an ordinary one, both sides of the difference from which e1 / (e0 + e1) rounds to 1.0f (16.665...),
# both sides of the exponent clamp at -87 and of the differences at which an unclamped exp turns denormal (-87.3) and zero (-103.97),
# and differences far past both.
RANGE_DIFFS = (0.0, 1e-45, 1e-8, 2.0, 16.6, 16.7, 17.4, 86.9, 87.0, 87.1, 88.7, 103.9, 104.0, 200.0, 1e4)
RANGE_A0 = (0.0, -8.0, 3.25, 8.0)
CLAMP_PROB = F32(1.6458115e-38)      # orc_expf(-87) / (1 + orc_expf(-87)): the smallest probability the reference softmax returns


def range_logits(seed=3):
    """Finite logit pairs (a0, a0 + d), f32: every RANGE_DIFFS difference and its negative at every RANGE_A0, the pair
    (3e38, -3e38) and its mirror (the difference itself overflows to infinity), and 200 uniform differences in [-20, 20]."""
    pairs = [(F32(a0), F32(a0) + F32(s * d)) for a0 in RANGE_A0 for d in RANGE_DIFFS for s in ((1,) if d == 0 else (1, -1))]
    pairs += [(F32(3e38), F32(-3e38)), (F32(-3e38), F32(3e38))]
    pairs += [(F32(0), d) for d in np.random.default_rng(seed).uniform(-20, 20, 200).astype(F32)]
    lt = np.array(pairs, F32)
    assert np.isfinite(lt).all()
    return lt


def range_case(kind, W=W0, H=H0, seed=3):
    """A kind 2 / 3 hook input of one frame whose logits are range_logits(): disjoint 10 x 10 boxes on a 16-px lattice well inside
    the frame (NMS and the pad test remove nothing: what comes out is decided by the probabilities alone), regression offsets zero
    on two rows of three and small dyadic values on the third, dyadic landmarks."""
    lt = range_logits(seed)
    k = len(lt)
    rng = np.random.default_rng(seed + 101 * kind)
    cols = W // 16 - 2
    assert k <= cols * (H // 16 - 2)
    cell = rng.permutation(cols * (H // 16 - 2))[:k]
    x, y = F32(16) * (cell % cols + 1).astype(F32), F32(16) * (cell // cols + 1).astype(F32)
    boxes = np.stack([x, y, x + 10, y + 10], 1).astype(F32)
    L = np.zeros((k, 6 if kind == 2 else 16), F32)
    L[:, :2] = lt
    L[:, 2:6] = rng.integers(-2, 3, (k, 4)).astype(F32) / F32(32) * (np.arange(k) % 3 == 0)[:, None]
    if kind == 3:
        L[:, 6:] = rng.integers(0, 17, (k, 10)).astype(F32) / F32(16)
    rows = np.concatenate([boxes, np.linspace(0.99, 0.61, k).astype(F32)[:, None]], 1).astype(F32)
    return {"kind": kind, "W": W, "H": H, "caps": [_round4(k)], "counts": np.array([k], np.int32), "rows": [rows], "logits": [L],
            "n": k, "fam": "range"}


def hook_args(case, order=None):
    """(caps, counts, rows, logits, sent) in the hook's packed layout; kind 1 records in append order `order` per list (a
    permutation seed; None = as built), sent[f][l] = the records of each list as sent (what the keep indices index)."""
    if case["kind"] == 1:
        sent = []
        for f, recs in enumerate(case["recs"]):
            sent.append([])
            for l, rec in enumerate(recs):
                perm = np.arange(len(rec)) if order is None else np.random.default_rng(order * 7 + l).permutation(len(rec))
                sent[f].append(rec[perm])
        return case["caps"], case["counts"], np.concatenate([r for fr in sent for r in fr]), None, sent
    return case["caps"], case["counts"], np.concatenate(case["rows"]), np.concatenate(case["logits"]), None


def reference(case, expf, max_faces=None, thr=0.7):
    """What detect_face computes for the case, per frame: kind 1 {"keep_cells": per level, "rows1"}, kind 2 {"rows2"},
    kind 3 {"rows3", "pts3", "sel"}.  thr: the stage's own threshold (kinds 2 and 3), any float."""
    out = []
    W, H = case["W"], case["H"]
    if case["kind"] == 1:
        for recs in case["recs"]:
            picks = [level_nms(rec) for rec in recs]
            out.append({"keep_cells": [rec["cell"][p] for rec, p in zip(recs, picks)], "rows1": stage1(recs, picks, W, H)})
        return out
    for rows, lg in zip(case["rows"], case["logits"]):
        p = probs(expf, lg) if len(lg) else np.zeros(0, F32)
        if case["kind"] == 2:
            out.append({"rows2": stage2(rows, p, lg[:, 2:6], W, H, thr)})
        else:
            r3, p3 = stage3(rows, p, lg[:, 2:6], lg[:, 6:16], thr)
            out.append({"rows3": r3, "pts3": p3, "sel": select(r3, p3, W, H, max_faces or 1)})
    return out


def list_lengths(case, ref):
    """The lengths of the lists each kernel sorts: kind 1 ([per level], [per frame total]); kinds 2 / 3 ([], [input rows])."""
    if case["kind"] == 1:
        return [len(x) for x in case["recs"][0]], [sum(len(k) for k in r["keep_cells"]) for r in ref]
    return [], [int(c) for c in case["counts"]]


def edges(small, full):
    """List lengths at the edges of one LDS tier pair: small / full tier -1, =, +1, power-of-two edges, the spill chunk C, C + 1,
    2 C + 1 and 3 C + 1, and 2 TK + 1 (capped at 4097: the reference is O(n x kept))."""
    C = pow2_floor(full)
    e = {small - 1, small, small + 1, full - 1, full, full + 1, C, C + 1, 2 * C + 1, 3 * C + 1, next_pow2(small) + 1, next_pow2(full),
         pow2_floor(small), pow2_floor(small) + 1, (C * 8 // 20) * 2 + 1}
    return sorted(x for x in e if 1 <= x <= 4097)
