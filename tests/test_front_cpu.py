"""The R-/O-Net front kernel's references agree with each other, without a GPU: the C oracle (area_resample_norm + orc_front,
the reference tests/test_gpu_front.py holds the kernel to) against the plain restatement of tests/front_ref.py, bit for bit on
the whole window table; the exact float32 fma the restatement is built on; the coverage the table gives, read from front_path;
and the distance of the float32 crop from its float64 form against the derived bound."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import truely_amd
import front_ref as R

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _round_f32(x: Fraction) -> float:
    """The float32 nearest to a rational (ties to even), normal range."""
    if x == 0:
        return 0.0
    s, x = (-1, -x) if x < 0 else (1, x)
    e = 0
    while x >= 1 << 24:
        x /= 2; e += 1
    while x < 1 << 23:
        x *= 2; e -= 1
    n = x.numerator // x.denominator
    rem = x - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    return s * float(Fraction(n) * Fraction(2) ** e)


def test_fma32_is_a_single_rounding():
    """Constructed double-rounding cases -- p + c lands so close to a float32 midpoint that the float64 sum IS the midpoint and a
    plain cast then rounds the wrong way -- and random operands, against exact rational arithmetic."""
    a = F32(1 + 2.0 ** -23)
    b = F32((1 - 2.0 ** -23) * 2.0 ** -24)                    # a b = 2^-24 - 2^-70: just BELOW half an ulp of 1
    c = F32(1 + 2.0 ** -23)                                   # odd significand: the tie would round up
    cases = [(a, b, c), (-a, b, -c), (a, -b, F32(1 + 2.0 ** -22)), (F32(3) * a, b, F32(2 + 2.0 ** -22))]
    naive_wrong = 0
    for x, y, z in cases:
        want = _round_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)))
        got = R.fma32(x, y, z)
        assert got.dtype == F32 and got.item() == want, (x, y, z, got.item(), want)
        naive_wrong += float(F32(np.float64(x) * np.float64(y) + np.float64(z))) != want
    assert naive_wrong >= 2, "the constructed cases must defeat add-then-cast"
    rng = np.random.default_rng(1)
    x, y = rng.standard_normal(4000).astype(F32), rng.standard_normal(4000).astype(F32)
    z = (-x * y * (1 + rng.integers(-3, 4, 4000) * 2.0 ** -24)).astype(F32)     # heavy cancellation
    z[::2] = rng.standard_normal(2000).astype(F32)
    got = R.fma32(x, y, z)
    for i in range(4000):
        assert float(got[i]) == _round_f32(Fraction(float(x[i])) * Fraction(float(y[i])) + Fraction(float(z[i]))), i


@functools.lru_cache(maxsize=None)
def _oracle(variant):
    from oracle.oracle import Oracle
    blob = R.slope_blob(variant)
    return Oracle(blob), truely_amd.weights.unpack_tensors(blob)


CPU_BATCHES = tuple(b for b in R.BATCHES if b[1:] not in ((211, 332), (211, 334), (211, 335)))    # pitch phases change loads, not values


@pytest.mark.parametrize("S", [24, 48])
def test_oracle_equals_the_restatement(S):
    """Crop and pooled map of every window of the table, every slope class: oracle == restatement on every element's bits."""
    classes = set()
    for bi, (nf, H, W) in enumerate(CPU_BATCHES + (R.WIDE,)):
        frames = R.content_frames("random", nf, H, W, seed=31 * bi + S)
        rec = R.placed(nf, H, W, S) if (nf, H, W) != R.WIDE else R.wide_records(S)
        rec = rec[np.unique(rec[:, 1:], axis=0, return_index=True)[1]]             # the value does not depend on the frame index
        orc, _ = _oracle("seeded")
        crops = []
        for f, y0, x0, ih, iw in rec.tolist():
            c32, _, _ = R.area_resample(frames[f], y0, x0, ih, iw, S)
            assert np.array_equal(_bits(c32), _bits(orc.area_resample_norm(frames[f], y0, y0 + ih, x0, x0 + iw, S, S))), (H, W, y0, x0, ih, iw)
            crops.append(c32)
        crops = np.stack(crops)
        t0 = _oracle("seeded")[1]
        conv = R.conv1(crops, t0[f"{R.NETS[S]['name']}.conv1.w"], t0[f"{R.NETS[S]['name']}.conv1.b"])
        for variant in R.SLOPE_VARIANTS:
            orc, t = _oracle(variant)
            sl = t[f"{R.NETS[S]['name']}.prelu1"]
            assert np.array_equal(t[f"{R.NETS[S]['name']}.conv1.w"], t0[f"{R.NETS[S]['name']}.conv1.w"])
            classes.add(0 if (sl < 0).any() else (1 if (sl > 1).any() else 2))
            want = orc.front(crops, S)
            got = R.prelu_pool(conv, sl)
            assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), (variant, H, W)
    assert classes == {0, 1, 2}
    z = _oracle("zero_one_slopes")[1][f"{R.NETS[S]['name']}.prelu1"]
    assert (z == 1).any() and {0x00000000, 0x80000000} <= set(_bits(z).tolist())


def test_flat_frames_have_closed_forms():
    """All-0 and all-255 frames: every crop element is (v - 127.5) / 128 whatever the window, in both references."""
    orc, _ = _oracle("seeded")
    for kind, v in (("zeros", 0), ("ones", 255)):
        fr = R.content_frames(kind, 1, 211, 333, 0)[0]
        for S in (24, 48):
            for y0, x0, ih, iw in R.window_table(211, 333, S)[::7]:
                c32, c64, _ = R.area_resample(fr, y0, x0, ih, iw, S)
                assert (c32 == (F32(v) - F32(127.5)) * F32(0.0078125)).all() and (c64 == (v - 127.5) / 128).all()
                assert np.array_equal(c32, orc.area_resample_norm(fr, y0, y0 + ih, x0, x0 + iw, S, S))


def _paths(S, with_huge):
    out = []
    for nf, H, W in R.BATCHES + ((R.HUGE,) if with_huge else ()):
        rec = R.placed(nf, H, W, S) if (nf, H, W) != R.HUGE else np.array([(0, 0, 0, H, W), (0, 0, 0, H, 7000)], np.int32)
        out += [((nf, H, W), tuple(r), R.front_path(r, nf, H, W, S)) for r in rec.tolist()]
    out += [(R.WIDE, tuple(r), R.front_path(r, *R.WIDE, S)) for r in R.wide_records(S).tolist()]
    return out


@pytest.mark.parametrize("S", [24, 48])
def test_the_table_reaches_every_path(S):
    """Coverage, from the restatement of the kernel's dispatch (tests/test_gpu_front.py runs exactly these records)."""
    paths = _paths(S, with_huge=S == 24)
    small = [p for _, _, p in paths if p["kind"] == "small"]
    big = [p for _, _, p in paths if p["kind"] == "big"]
    assert {(p["rows"], True) for p in small if p["safe"] == {True}} == {(2, True), (3, True), (4, True)}       # every ROWS, unclamped
    assert any(p["safe"] == {False} for p in small)                                                               # the clamped small form
    assert {p["fb3"] for p in small} == {0, 1, 2, 3} and {p["fb3"] for p in small if p["safe"] == {False}} >= {0}
    assert {p["fb3"] for p in big} == {0, 1, 2, 3}
    assert {p["same_phase"] for p in big} == {True, False}
    L = R.seg_limit(S)
    assert L == {24: 309, 48: 213}[S]
    reach = {24: {1, 2, 3, 4}, 48: {1, 2, 3}}[S]             # safe chunk counts a segment of <= CAP2 - 4 (+ 3 phase) bytes can have
    for ph in (True, False):
        assert (R.strip_caps(S)[1] - 4 + (3 if ph else 0) > 3 * R.CSTRIDE[ph]) == (4 in reach)
        got = {n for p in big if p["same_phase"] == ph for n, inst in p["nch"] if n == inst}
        assert got == reach, (ph, got)
        assert any(inst == 4 and False in p["safe"] for p in big if p["same_phase"] == ph for n, inst in p["nch"])   # clamped big form
    assert {min(p["segments"], 3) for p in big} == {1, 2, 3}
    assert {p["passes"] for p in big} == {1}                 # the c0 loop never runs twice: span <= CAP2 - 1 < 4 * 252
    assert R.strip_caps(S)[1] - 4 + 3 < 4 * min(R.CSTRIDE.values())
    off = [(b, r) for b, r, p in paths if p["kind"] != "small" and not p["fastdiv"]]
    assert any(r[3] > R.FASTDIV_BINS * S for _, r in off) and any(r[4] > R.FASTDIV_BINS * S for _, r in off)     # off in each direction
    assert any(p["fastdiv"] for p in big)
    # a bin wider than half the strip, for both nets: the widths on either side of the limit, one window ending at the buffer's last byte
    L = R.wide_limit(S)
    assert L == {24: 7392, 48: 10176}[S]
    wk = {(r[4], p["kind"]) for b, r, p in paths if b == R.WIDE}
    assert wk == {(L, "big"), (L + 1, "wide"), (R.WIDE[2], "wide")}
    nfw, Hw, Ww = R.WIDE
    assert any(p["kind"] == "wide" and r[0] == nfw - 1 and r[1] + r[3] == Hw and r[2] + r[4] == Ww for b, r, p in paths if b == R.WIDE)
    assert any(p["kind"] == "big" and False in p["safe"] for b, r, p in paths if b == R.WIDE)
    if S == 24:
        wide = [p for _, _, p in paths if p["kind"] == "wide"]
        assert wide and max(p["max_bin"] for p in wide) > 65793                # sums that pass 2^24
        assert any(p["kind"] == "big" and not p["fastdiv"] and r[4] == 7000 for _, r, p in paths)


def test_crop_f32_distance_from_f64(capsys):
    """|f32 crop - f64 crop| over the table (random and checkerboard content) against crop_f32_bound, which is derived from the
    number format alone.  DESIGN section 2 quotes both figures."""
    worst = 0.0
    for S in (24, 48):
        for bi, (nf, H, W) in enumerate(CPU_BATCHES):
            for kind in ("random", "checker"):
                fr = R.content_frames(kind, 1, H, W, seed=5 + bi)[0]
                for y0, x0, ih, iw in R.window_table(H, W, S)[::3]:
                    c32, c64, sums = R.area_resample(fr, y0, x0, ih, iw, S)
                    assert sums.max() < 1 << 24
                    d = float(np.abs(c32.astype(np.float64) - c64).max())
                    assert d <= R.crop_f32_bound(1), (H, W, y0, x0, ih, iw, d)
                    worst = max(worst, d)
    fr = np.full((600, 16383, 3), 255, np.uint8)              # stacked five times below: bins of 125 x 683 = 85,375 px
    fr[::7, ::5] = 254
    big = np.broadcast_to(fr[None], (5, 600, 16383, 3)).reshape(3000, 16383, 3)
    d32, d64, dsum = R.area_resample(big, 0, 0, 3000, 16383, 24)
    assert dsum.max() >= 1 << 24
    dbig = float(np.abs(d32.astype(np.float64) - d64).max())
    assert dbig <= R.crop_f32_bound(125 * 683)
    with capsys.disabled():
        print(f"\n[front crop] max |f32 - f64| = {worst:.4g} (bound {R.crop_f32_bound(1):.4g}); with sums past 2^24: {dbig:.4g} "
              f"(bound {R.crop_f32_bound(125 * 683):.4g})")
    assert R.crop_f32_bound(1) < 3.0e-7 and R.crop_f32_bound(1 << 17) < 4.2e-7
