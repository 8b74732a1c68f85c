"""CPU pins of tests/list_ref.py, the reference of the list-kernel tests (test_gpu_lists.py): its NMS equals the C oracle's on
every built list, fed the oracle's own R-Net / O-Net outputs it reproduces the oracle's stage boxes bit for bit, and the
routing restatement shows that the built lists reach the tier, power-of-two, chunk and tile edges they are named for."""
import numpy as np
import pytest
import torch

import list_ref as R
import truely_amd
from decision_audit import _crops

F32 = np.float32
TIERS = [(512, 2048), (16, 64), (100, 300), (500, 3072)]


@pytest.mark.parametrize("mode", [0.5, 0.7, "min"])
def test_reference_nms_equals_oracle_on_built_lists(oracle, mode):
    for fam in ("dup", "cell", "chain", "special"):
        for n in (1, 2, 17, 65, 129, 513, 2049):
            b, r = R.make_list(fam, n, mode, seed=n)
            s = R.scores_from_rank(r)
            if mode == "min":
                ref = R._nms_min(b, s, 0.7)
                orc = oracle.nms_min(b, s, 0.7)
            else:
                ref = R._nms_iou(torch.as_tensor(b), torch.as_tensor(s), mode).numpy()
                orc = oracle.nms_iou(b, s, mode)
            assert np.array_equal(ref, orc), (fam, n, mode)


def test_special_lists_decide_at_their_edges():
    """The special boxes do what they are there for: exact-threshold pairs are kept, the pairs just above are suppressed,
    tied pairs keep exactly one box."""
    for mode in (0.5, 0.7, "min"):
        b, r = R.special(mode)
        s = R.scores_from_rank(r)
        keep = set((R._nms_min(b, s, 0.7) if mode == "min" else R._nms_iou(torch.as_tensor(b), torch.as_tensor(s), mode).numpy()).tolist())
        assert (0 in keep) != (1 in keep), mode                       # a tied pair: one survives
        assert 5 in keep and 6 in keep, mode                          # exactly at the threshold: kept
        assert 7 in keep and 8 not in keep, mode                      # just above: suppressed


@pytest.mark.parametrize("H,W,seed", [(180, 320, 3), (240, 320, 11), (120, 160, 41)])
def test_reference_reproduces_oracle_detect(oracle, H, W, seed):
    """Fed the oracle's PNet maps and its own R-Net / O-Net outputs on its crops, the reference gives the boxes of every stage of
    oracle.detect(trace=True), and the selection of its result, bit for bit."""
    fr = truely_amd.synthetic.synthetic_frames(1, H, W, seed=seed)[0]
    boxes, probs, tr = oracle.detect(fr, trace=True)
    recs = []
    for sc, h, w in oracle.scales(H, W):
        p, r = oracle.pnet_level(oracle.area_resample_norm(fr, 0, H, 0, W, h, w))
        cells = np.flatnonzero(p.reshape(-1) >= F32(0.6))
        ys, xs = np.divmod(cells, p.shape[1])
        scf = F32(sc)
        rec = np.zeros(len(cells), R.CAND)
        rec["box"] = np.stack([np.floor((F32(2) * xs.astype(F32) + F32(1)) / scf), np.floor((F32(2) * ys.astype(F32) + F32(1)) / scf),
                               np.floor((F32(2) * xs.astype(F32) + F32(12)) / scf), np.floor((F32(2) * ys.astype(F32) + F32(12)) / scf)], 1)
        rec["score"] = p.reshape(-1)[cells]
        rec["reg"] = r.reshape(-1, 4)[cells]
        rec["cell"] = cells
        recs.append(rec[::-1].copy())                                   # any append order: the reference orders by cell
    rows1 = R.stage1(recs, [R.level_nms(x) for x in recs], W, H)
    assert len(rows1) > 0 and np.array_equal(rows1, tr["boxes1"])
    p2, r2 = oracle.rnet(_crops(oracle, fr, rows1, 24))
    rows2 = R.stage2(rows1, p2, r2, W, H)
    assert np.array_equal(rows2, tr["boxes2"])
    if len(rows2) == 0:
        return
    p3, r3, pt3 = oracle.onet(_crops(oracle, fr, rows2, 48))
    rows3, pts3 = R.stage3(rows2, p3, r3, pt3)
    assert np.array_equal(rows3, tr["boxes3"]) and np.array_equal(pts3, tr["points3"])
    sel = R.select(rows3, pts3, W, H, 64)
    if boxes is None:
        assert sel["count"] == 0
    else:
        assert np.array_equal(sel["boxes"], boxes) and np.array_equal(sel["probs"], probs)
        ref = oracle.detect_embed(fr[None])
        assert np.array_equal(sel["rect"], ref["rect"][0]) and sel["valid"] == ref["valid"][0]


def test_probabilities_from_logits(oracle):
    """R.probs is the oracle's softmax2_p1 (max first, orc_expf, one f32 division): equal logits give exactly 0.5, a logit
    difference past expf's clamp saturates, and equal logit pairs give equal probabilities (the ties the tests build)."""
    lg = np.array([[0, 0], [0, 1e-7], [1, 0.8472979], [-3, 2], [5, 5], [0, 88], [0, -88], [2.5, -1.25]], F32)
    got = R.probs(oracle.expf, lg)
    assert got[0] == F32(0.5) and got[4] == F32(0.5) and got[5] == F32(1) and got[6] < F32(1e-30)
    assert got[1] > got[0] and got[3] > F32(0.99)
    t = R.logits_from_rank(np.array([3, 1, 3, 0, 2]))
    p = R.probs(oracle.expf, t)
    assert p[0] == p[2] and p[3] > p[1] > p[4] > p[0] and (p > F32(0.7)).all()


def test_spill_bytes_per_kind():
    """The pool bytes of one spilled list in a 640 x 480 frame (21 x 16 grid cells = 1344 bytes of heads), by hand:
    k_nms_level 513: 1024 * 12 + 513 * 24 + 1344 = 25944 -> 102 * 256; k_nms_frame 513: 1024 * 12 + 513 * 28 + 1344 = 27996 ->
    110 * 256; k_stage2_post 2049: 4096 * 12 + 2049 * 28 + 1344 = 107868 -> 422 * 256; k_stage3_post 2049 (no grid):
    4096 * 12 + 2049 * 24 = 98328 -> 385 * 256, and 64: 64 * 12 + 64 * 24 = 2304 = 9 * 256 exactly (no rounding past it)."""
    assert R.spill_bytes(1, "level", 513, 640, 480) == 26112
    assert R.spill_bytes(1, "frame", 513, 640, 480) == 28160
    assert R.spill_bytes(2, "level", 2049, 640, 480) == 108032
    assert R.spill_bytes(3, "level", 2049, 640, 480) == 98560
    assert R.spill_bytes(3, "level", 64, 640, 480) == 2304


@pytest.mark.parametrize("tiers", TIERS, ids=lambda t: f"{t[0]}-{t[1]}")
def test_cases_reach_the_edges_they_name(oracle, tiers):
    """Restating list_launch / k_nms_level routing: the lengths test_gpu_lists.py builds for a tier pair reach the small tier
    -1 / = / +1, the full tier -1 / = / +1, power-of-two sort sizes above a non-power-of-two capacity, the spill chunk C, C + 1,
    2 C + 1, and, in the 'Min' spill tier, kept counts that cross TK and 2 TK before a later chunk."""
    small, full = tiers
    seen = set()
    for n in R.edges(small, full):
        for kind, part in ((1, "level"), (1, "frame"), (2, "level"), (3, "level")):
            case = R.build_case(kind, "dup", n, part=part)
            lv, fr = R.list_lengths(case, R.reference(case, oracle.expf, 64))
            ll = R.launch(small, full, case["caps"][:-1], case["caps"][-1])
            for cnt, level in [(c, True) for c in lv[:1]] + [(c, False) for c in fr[:1]]:
                tier, th, P, C, TK = R.route(ll, cnt, level)
                cap = (ll["small_cap"] if tier == "small" else ll["full_l"]) if level else ll["full_f"]
                if level and cnt == ll["small_cap"] + 1 and tier != "small":
                    seen.add("small+1")
                if level and cnt == ll["small_cap"] and tier == "small":
                    seen.add("small=")
                if level and cnt == ll["small_cap"] - 1:
                    seen.add("small-1")
                if cnt == cap and tier != "spill":
                    seen.add("full=" if level else "frame=")
                if cnt == cap + 1 and tier == "spill":
                    seen.add("full+1" if level else "frame+1")
                if cnt == R.pow2_floor(ll["full_l" if level else "full_f"]) and tier != "spill":
                    seen.add("C")                                              # the longest list one spill chunk holds
                if cnt == cap - 1:
                    seen.add("full-1" if level else "frame-1")
                if tier != "spill" and P > cap:
                    seen.add("sort past a non-power-of-two capacity")
                if tier == "spill":
                    assert th == 1024 and C <= 2 * th and TK * 20 <= C * 8
                    if cnt == C + 1:
                        seen.add("C+1")
                    if cnt == 2 * C + 1:
                        seen.add("2C+1")
            if kind == 3:
                tier, th, P, C, TK = R.route(ll, fr[0], False)
                if tier == "spill":
                    kept_before_last = min((fr[0] + 1) // 2, (fr[0] - 1) // C * C)   # "dup": the originals come first, all kept
                    if kept_before_last > 2 * TK:
                        seen.add("Min kept > 2 TK")
                    elif kept_before_last > TK:
                        seen.add("Min kept > TK")
    want = {"small-1", "small=", "small+1", "full-1", "full=", "full+1", "frame-1", "frame=", "frame+1", "C", "2C+1", "Min kept > 2 TK"}
    if full & (full - 1) == 0:                                         # C = full: C + 1 is the first spilled length
        want.add("C+1")
    if full <= 2048:
        want.add("Min kept > TK")
    if any(x & (x - 1) for x in (small, full) if x < 2048):
        want.add("sort past a non-power-of-two capacity")
    assert want <= seen, want - seen
