"""CPU checks of the per-input form of the fp16 conv3 screen's bound.

The kernel confirms an M-tile when some cell has d_screen + E >= dthr with E = sum_k ghat[channel(k)] |x_k| + B over the cell's
3 x 3 x 16 conv2 inputs (tools/pnet_screen_audit.py:screen_weights restates ghat; screen_bound is the older E = A X + B).  These
tests hold the restatement to its definition (sum_k g_k = A, ghat >= g) and check |d_screen - d_exact| <= E against the numpy
emulation of tests/test_pnet_screen_cpu.py -- fp16 operands and f32 accumulation against the exact f32 chain -- for the seeded
weights and the five PReLU slope classes, on bench-like cells, cells up to the fp16 maximum, subnormal-heavy cells, cells with one
huge input among 143 tiny ones (where A X + B was loosest) and cells whose inputs are all equal (where the per-input form is at
its loosest against A X + B).  A sanity check of the derivation, not its proof."""
import os
import sys

import numpy as np
import pytest

import truely_amd
from truely_amd import weights
from slope_variants import slope_variant_blob
from test_pnet_screen_cpu import _d_pair

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from pnet_screen_audit import screen_bound, screen_weights  # noqa: E402

VARIANTS = ["seeded", "slopes_above_one", "negative_slopes", "mixed_signs", "negative_deep_only", "generalise_prelu"]
KINDS = ["bench", "large", "subnormal", "one_huge", "all_equal"]
_cache = {}


def _tensors(variant):
    if variant not in _cache:
        blob = weights.synthetic_blob(0) if variant == "seeded" else slope_variant_blob(variant)
        _cache[variant] = weights.unpack_tensors(blob)
    return _cache[variant]


def _bench_cells(t, n):
    """receptive fields [n][144] (k = tap * 16 + channel) of conv2 cells of a bench-like level under the tensors t"""
    import torch
    import torch.nn.functional as F
    fr = truely_amd.synthetic.synthetic_frames(1, 180, 320, seed=0, faces=1)[0]
    src = torch.from_numpy(fr.astype(np.float32).transpose(2, 0, 1).copy())[None]
    lvl = ((F.adaptive_avg_pool2d(src, (108, 192))[0] - 127.5) * 0.0078125)[None]

    def conv(x, w, b, cin):
        return F.conv2d(x, torch.from_numpy(w.reshape(3, 3, cin, -1).transpose(3, 2, 0, 1).copy()), torch.from_numpy(b))

    def prelu(x, s):
        return torch.where(x >= 0, x, x * torch.from_numpy(s).view(1, -1, 1, 1))

    y = F.max_pool2d(prelu(conv(lvl, t["pnet.conv1.w"], t["pnet.conv1.b"], 3), t["pnet.prelu1"]), 2, 2, ceil_mode=True)
    a2 = prelu(conv(y, t["pnet.conv2.w"], t["pnet.conv2.b"], 10), t["pnet.prelu2"])[0].numpy()     # [16][h][w]
    rng = np.random.default_rng(1)
    h, w = a2.shape[1] - 2, a2.shape[2] - 2
    ys, xs = rng.integers(0, h, n), rng.integers(0, w, n)
    return np.stack([a2[:, ys + dy, xs + dx].T for dy in range(3) for dx in range(3)], axis=1).reshape(-1, 144)


def _cells(kind, t, n=600):
    rng = np.random.default_rng(KINDS.index(kind) + 11)
    if kind == "bench":
        return _bench_cells(t, n)
    if kind == "large":             # up to the fp16 maximum, the largest input the screen accepts
        return np.clip(rng.uniform(-1, 1, (n, 144)) * rng.choice([1e2, 3e3, 65504.0], (n, 1)), -65504, 65504)
    if kind == "subnormal":         # fp16 subnormals and below, a few ordinary values among them
        x = rng.uniform(-1, 1, (n, 144)) * rng.choice([1e-8, 6e-6, 6e-5], (n, 144))
        x[:, ::29] = rng.uniform(-1, 1, (n, 5))
        return x
    if kind == "one_huge":          # one input of every size up to 65504 at every position k, 143 tiny ones around it
        x = rng.uniform(-1, 1, (n, 144)) * rng.choice([1e-7, 1e-5, 1e-3], (n, 1))
        big = rng.choice([3.0, 2049.0, 3e4, 65504.0], n) * rng.choice([-1.0, 1.0], n)
        x[np.arange(n), np.arange(n) % 144] = big
        return x
    v = rng.choice([1e-6, 0.37, 2.5, 2049.0, 65504.0], (n, 1)) * rng.choice([-1.0, 1.0], (n, 1))   # all_equal
    return np.repeat(v, 144, axis=1)


def _E(x, ghat, B):
    """the bound as the kernel forms it, in double: sum over k = tap * 16 + channel of ghat[channel] |x_k|, + B"""
    return np.abs(x.astype(np.float32).astype(np.float64)) @ np.tile(np.asarray(ghat, np.float64), 9) + B


def _E_kernel(x, ghat, B):
    """E as the kernel evaluates it, in float32 and in its order: per conv2 cell (tap) and channel half m = eight fmaf from 0 (one
    rounding each), clamped to the largest finite float; a lane adds its half's nine m, tap ascending; the two lanes' sums are
    added; then + B"""
    f32, fmax = np.float32, np.float32(3.402823466e38)
    ax = np.abs(x.astype(f32)).reshape(-1, 9, 2, 8)
    gh = np.asarray(ghat, f32).reshape(2, 8)
    em = []
    for half in range(2):
        s = np.zeros(ax.shape[0], f32)
        for tap in range(9):
            m = np.zeros(ax.shape[0], f32)
            for j in range(8):      # fmaf: the product of two floats is exact in double, the sum is rounded once more to float
                m = (gh[half, j].astype(np.float64) * ax[:, tap, half, j].astype(np.float64) + m.astype(np.float64)).astype(f32)
            s = (s + np.minimum(m, fmax)).astype(f32)
        em.append(s)
    return ((em[0] + em[1]).astype(f32) + f32(B)).astype(f32)


@pytest.mark.parametrize("kind", KINDS + ["f32_tiny"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_kernel_float32_sum_covers_the_bound(variant, kind):
    """the 1 + 2^-10 on ghat and B has to cover the kernel's own float32 roundings (at most 18 per term) and the underflow of
    ghat |x| on inputs near the bottom of the float range: the kernel's E is at least the bound without any inflation,
    sum_k g_k |x_k| + B_0 with the per-tap g in double and B_0 <= B / (1 + 2^-10)"""
    t = _tensors(variant)
    _A, B, _ = screen_bound(t)
    g, ghat, _B, _ok = screen_weights(t)
    if kind == "f32_tiny":          # float32 subnormals and the smallest normals: every product ghat |x| underflows
        rng = np.random.default_rng(5)
        x = rng.uniform(-1, 1, (600, 144)) * rng.choice([1e-45, 1e-41, 1e-38, 1e-36], (600, 144))
    else:
        x = _cells(kind, t)
    x = x.astype(np.float32)
    true = np.abs(x.astype(np.float64)) @ g.reshape(-1) + B / (1 + 2.0 ** -10)
    Ek = _E_kernel(x, ghat, B)
    assert np.all(np.isfinite(Ek))
    assert np.all(Ek.astype(np.float64) >= true), float(np.min(Ek.astype(np.float64) - true))
    de, ds = _d_pair(t, x)
    assert np.all(np.abs(ds.astype(np.float64) - de) <= Ek)


@pytest.mark.parametrize("variant", VARIANTS)
def test_weights_sum_to_A_and_dominate_every_tap(variant):
    t = _tensors(variant)
    A, B, ok = screen_bound(t)
    g, ghat, Bw, okw = screen_weights(t)
    assert ok and okw and Bw == B
    assert g.shape == (9, 16) and np.all(g > 0) and len(ghat) == 16
    infl = 1 + 2.0 ** -10
    assert abs(g.sum() * infl - A) <= 2.0 ** -22 * A                     # A is that sum in double, rounded up to float once
    gh = np.asarray(ghat, np.float64)
    assert np.all(gh == gh.astype(np.float32)) and np.all(np.isfinite(gh))
    assert np.all(gh[None, :] >= g * infl)                               # every tap's coefficient, the inflation included
    assert np.all(gh <= g.max(0) * infl * (1 + 2.0 ** -22))


def test_weights_turn_off_with_the_screen():
    t = dict(_tensors("seeded"))
    t["pnet.conv3.w"] = t["pnet.conv3.w"].copy()
    t["pnet.conv3.w"][5, 3] = 7.0e4
    g, ghat, _B, ok = screen_weights(t)
    assert ok is False and np.all(np.isinf(g)) and all(np.isinf(v) for v in ghat)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_screen_within_the_per_input_bound(variant, kind):
    t = _tensors(variant)
    A, B, _ = screen_bound(t)
    g, ghat, _B, _ok = screen_weights(t)
    x = _cells(kind, t).astype(np.float32)
    de, ds = _d_pair(t, x)
    err = np.abs(ds.astype(np.float64) - de)
    E = _E(x, ghat, B)
    assert np.all(np.isfinite(err))
    assert np.all(err <= E), float(np.max(err - E))
    X = np.abs(x).max(1).astype(np.float64)
    if kind == "all_equal":
        # every |x_k| = X: E - B = X * 9 sum(ghat), above A X by the factor ghat-over-g allows and no more
        rho = 9.0 * g.max(0).sum() / g.sum()
        assert 1.0 <= rho < 9.0
        assert np.all(E - B <= rho * (1 + 2.0 ** -20) * A * X)
    if kind == "one_huge":
        # one input carries X, the others are at most 1e-3: E - B is one coefficient times X, not all 144 of them
        assert np.all(E - B <= max(ghat) * (X + 143e-3) * (1 + 2.0 ** -20))
