"""CPU checks of the 4:2:0 ingest restatement (tests/ingest_ref.py): it equals the oracle's nv12_to_bgr on every (Y, U, V) triple and
on the odd-edge shapes, the fixed-point rule stays within a DERIVED distance of the textbook float BT.601 formula on the whole
cube, its accumulators fit an int32 (what lets the kernel use `int`), and the generators do what their docstrings say."""
import numpy as np
import pytest

import ingest_ref as R


@pytest.fixture(scope="module")
def cube():
    return R.colour_cube_nv12()


@pytest.fixture(scope="module")
def triples():
    """Y, U, V as broadcastable int64 axes of the 256^3 cube."""
    a = np.arange(256, dtype=np.int64)
    return a[:, None, None], a[None, :, None], a[None, None, :]


def test_cube_holds_every_triple_exactly_once(cube):
    nv12, _ = cube
    n = R.CUBE
    Y, U, V = R.planes(nv12, n, n)
    key = (Y.astype(np.int64) << 16) | (np.repeat(np.repeat(U, 2, 0), 2, 1).astype(np.int64) << 8) | np.repeat(np.repeat(V, 2, 0), 2, 1)
    assert key.shape == (n, n) and np.array_equal(np.bincount(key.reshape(-1), minlength=1 << 24), np.ones(1 << 24, np.int64))
    # ... and where the docstring says: pixel -> triple and triple -> pixel
    rng = np.random.default_rng(0)
    y, x = rng.integers(0, n, 4096), rng.integers(0, n, 4096)
    ty, tu, tv = R.cube_triple(y, x)
    assert np.array_equal(key[y, x], (ty << 16) | (tu << 8) | tv)
    assert np.array_equal(y, 16 * tu + 2 * ((ty // 4) // 8) + (ty % 4) // 2) and np.array_equal(x, 16 * tv + 2 * ((ty // 4) % 8) + ty % 2)


def test_nv12_to_i420_round_trips(cube):
    nv12, i420 = cube
    n = R.CUBE
    for f, p, H, W in [(nv12, i420, n, n)] + [(a, R.nv12_to_i420(a, H, W), H, W) for H, W in ((2, 4), (38, 52), (6, 12))
                                               for a in R.content("noise", 3, H, W, seed=5)]:
        assert p.shape == f.shape and p.dtype == np.uint8
        for a, b in zip(R.planes(f, H, W), R.planes(p, H, W, planar=True)):
            assert np.array_equal(a, b)
        back = p.copy()                                                  # re-interleave by hand
        back[H * W::2], back[H * W + 1::2] = p[H * W:H * W + H * W // 4], p[H * W + H * W // 4:]
        assert np.array_equal(back, f)
    batch = R.content("edges", 4, 6, 12, seed=1)
    assert np.array_equal(R.nv12_to_i420(batch, 6, 12), np.stack([R.nv12_to_i420(f, 6, 12) for f in batch]))


def test_reference_equals_oracle_on_the_whole_cube(cube, oracle):
    nv12, i420 = cube
    n = R.CUBE
    ref = R.yuv420_to_bgr(nv12, n, n)
    got = oracle.nv12_to_bgr(nv12, n, n)
    if not np.array_equal(ref, got):
        y, x, c = (int(v[0]) for v in np.nonzero(ref != got))
        pytest.fail(f"(Y, U, V) = {tuple(int(t) for t in R.cube_triple(y, x))} channel {'BGR'[c]}: reference {ref[y, x, c]}, oracle {got[y, x, c]}")
    assert np.array_equal(R.yuv420_to_bgr(i420, n, n, planar=True), ref)       # both layouts by indexing: the same frame
    # the frame route and the per-sample route of the reference agree, so the cube-wide bounds below speak about the frame route
    yy, xx = np.meshgrid(np.arange(0, n, 7), np.arange(0, n, 5), indexing="ij")
    assert np.array_equal(ref[yy, xx], R.fixed_bgr(*R.cube_triple(yy, xx)))


@pytest.mark.parametrize("H,W", [(2, 4), (38, 52), (6, 12)])
@pytest.mark.parametrize("kind", R.KINDS)
def test_reference_equals_oracle_on_odd_edge_shapes(oracle, H, W, kind):
    for f in R.content(kind, 3, H, W, seed=H):
        ref = R.yuv420_to_bgr(f, H, W)
        assert ref.shape == (H, W, 3) and ref.dtype == np.uint8
        assert np.array_equal(ref, oracle.nv12_to_bgr(f, H, W))
        assert np.array_equal(R.yuv420_to_bgr(R.nv12_to_i420(f, H, W), H, W, planar=True), ref)


def test_fixed_point_within_derived_bound_of_float_bt601(triples):
    """|fixed - clip(float)| <= 0.5 + 3 * 255 * 0.5 / 2**20: half a unit from rounding half up, plus the constants' quantisation
    (each is within 0.5 of coefficient * 2**20 -- asserted -- and multiplies an operand of magnitude <= 255; three terms at most).
    Clamping both sides to [0, 255] cannot widen a gap.  Derived, not measured; the measured maximum is 0.5000000000000284."""
    for name, c in R.COEFF.items():
        assert abs(getattr(R, name) - c * 2 ** R.SHIFT) <= 0.5, name
    bound = 0.5 + 3 * 255 * 0.5 / 2 ** 20
    fixed = R.fixed_bgr(*triples).astype(np.float64)
    d = np.abs(fixed - R.bt601_float(*triples, clamp=True))
    worst = d.reshape(-1, 3).max(axis=0)
    print("max |fixed - clip(float)| per channel B, G, R:", worst.tolist())
    assert (worst <= bound).all(), worst
    # unclamped: the same distance wherever the float value is inside the range
    f = R.bt601_float(*triples)
    inside = (f >= 0) & (f <= 255)
    assert (np.abs(fixed - f)[inside] <= bound).all()


def test_accumulators_fit_int32(triples):
    peak = max(int(np.abs(a).max()) for a in R.fixed_accumulators(*triples))
    print("peak |accumulator|:", peak)
    assert peak < 2 ** 31
    # the partial sums the kernel forms on the way (y' alone, half + chroma terms alone) are smaller still
    assert 239 * R.CY < 2 ** 31 and (1 << 19) + 128 * (abs(R.CVG) + abs(R.CUG)) < 2 ** 31 and (1 << 19) + 128 * R.CUB < 2 ** 31


def test_cube_exercises_the_clamp(triples):
    bgr = R.fixed_bgr(*triples)
    for c in range(3):
        lo, hi = float((bgr[..., c] == 0).mean()), float((bgr[..., c] == 255).mean())
        print("BGR"[c], "share at 0:", lo, "at 255:", hi)
    assert (bgr[..., 0] == 0).mean() > 0.10 and (bgr[..., 0] == 255).mean() > 0.10


def test_content_kinds():
    H, W, n = 6, 12, 5
    for kind in R.KINDS:
        a, b = R.content(kind, n, H, W, seed=2), R.content(kind, n, H, W, seed=2)
        assert a.shape == (n, H * W * 3 // 2) and a.dtype == np.uint8 and np.array_equal(a, b)
        assert not np.array_equal(a, R.content(kind, n, H, W, seed=3))
        assert len({f.tobytes() for f in a}) == n                        # no two frames alike
    assert set(np.unique(R.content("edges", 4, 38, 52))) == set(R.EDGE_BYTES.tolist())
    for f in R.content("flat", 4, H, W):
        assert all(len(np.unique(p)) == 1 for p in R.planes(f, H, W))
    with pytest.raises(ValueError):
        R.content("stripes", 1, H, W)
    with pytest.raises(ValueError):
        R.yuv420_to_bgr(np.zeros(10, np.uint8), 2, 4)
