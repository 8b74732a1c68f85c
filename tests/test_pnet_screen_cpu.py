"""CPU checks of the fused PNet's fp16 conv3 screen bound.

The kernel confirms an M-tile when some cell has d_screen + A X + B >= dthr.  These tests restate the bound
(tools/pnet_screen_audit.py:screen_bound) and check it against a numpy emulation of the screen -- fp16 operands, f32
accumulation -- and of the exact f32 chain, on the bench clip's cells and on adversarial activations near the fp16 limits.  This is
a sanity check of the derivation, not its proof.  The library's own A and B are compared with the restatement in
tests/test_gpu_pnet_screen.py (creating a context needs a device)."""
import os
import sys

import numpy as np
import pytest

import truely_amd
from truely_amd import weights

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from pnet_screen_audit import screen_bound  # noqa: E402


def _tensors(seed=0):
    return weights.unpack_tensors(weights.synthetic_blob(seed))


def _prelu(v, s):
    return np.maximum(v, (s * v).astype(np.float32)) if np.all(s <= 1) else np.where(v >= 0, v, (s * v).astype(np.float32))


def _chain(terms, init):
    """f32 accumulation in k order: acc = RN(acc + RN(term)) (products of fp16 operands are exact in f32)."""
    acc = init.astype(np.float32)
    for k in range(terms.shape[-1]):
        acc = (acc.astype(np.float64) + terms[..., k]).astype(np.float32)
    return acc


def _d_pair(t, x):
    """x [n][144] conv2 inputs of n cells -> (d_exact, d_screen), each through its own arithmetic."""
    w3, b3, s3 = t["pnet.conv3.w"], t["pnet.conv3.b"], t["pnet.prelu3"]
    wl, bl = t["pnet.conv4_1.w"], t["pnet.conv4_1.b"]
    x = x.astype(np.float32)
    # exact: fmaf chain, bias first, k ascending (the product is exact in double, one rounding per step)
    ve = np.empty((x.shape[0], 32), np.float32)
    for c in range(32):
        ve[:, c] = _chain(x.astype(np.float64) * w3[:, c].astype(np.float64), np.full(x.shape[0], b3[c], np.float32))
    pe = _prelu(ve, s3)
    l0 = _chain(pe.astype(np.float64) * wl[:, 0].astype(np.float64), np.full(x.shape[0], bl[0], np.float32))
    l1 = _chain(pe.astype(np.float64) * wl[:, 1].astype(np.float64), np.full(x.shape[0], bl[1], np.float32))
    de = (l1 - l0).astype(np.float32)
    # screen: fp16 operands, f32 sums (here in reverse k order), PReLU, f32(w1 - w0) head in one chain
    xh = x.astype(np.float16).astype(np.float64)
    wh = w3.astype(np.float16).astype(np.float64)
    vs = np.empty_like(ve)
    for c in range(32):
        vs[:, c] = _chain((xh * wh[:, c])[:, ::-1], np.full(x.shape[0], b3[c], np.float32))
    ps = _prelu(vs, s3)
    wd = (wl[:, 1] - wl[:, 0]).astype(np.float32)
    ds = _chain(ps.astype(np.float64) * wd.astype(np.float64), np.zeros(x.shape[0], np.float32))
    ds = (ds + np.float32(bl[1] - bl[0])).astype(np.float32)
    return de, ds


def test_bound_is_positive_and_finite():
    A, B, ok = screen_bound(_tensors())
    assert ok and 0 < A < 1 and 0 < B < 0.1 and np.float32(A) == A and np.float32(B) == B


def test_bound_turns_screen_off_for_weights_beyond_fp16():
    t = _tensors()
    t["pnet.conv3.w"] = t["pnet.conv3.w"].copy()
    t["pnet.conv3.w"][5, 3] = 7.0e4
    assert screen_bound(t)[2] is False


def test_bound_grows_with_the_prelu_slope():
    t = _tensors()
    A0, B0, _ = screen_bound(t)
    t["pnet.prelu3"] = np.where(np.arange(32) % 2 == 0, 1.5, t["pnet.prelu3"]).astype(np.float32)
    A1, B1, _ = screen_bound(t)
    assert A1 > A0 and B1 >= B0


def test_screen_within_bound_on_bench_cells():
    import torch
    import torch.nn.functional as F
    t = _tensors()
    A, B, _ = screen_bound(t)
    fr = truely_amd.synthetic.synthetic_frames(1, 180, 320, seed=0, faces=1)[0]
    src = torch.from_numpy(fr.astype(np.float32).transpose(2, 0, 1).copy())[None]
    lvl = ((F.adaptive_avg_pool2d(src, (108, 192))[0] - 127.5) * 0.0078125)[None]

    def conv(x, w, b, cin):
        return F.conv2d(x, torch.from_numpy(w.reshape(3, 3, cin, -1).transpose(3, 2, 0, 1).copy()), torch.from_numpy(b))

    def prelu(x, s):
        return torch.where(x >= 0, x, x * torch.from_numpy(s).view(1, -1, 1, 1))

    y = F.max_pool2d(prelu(conv(lvl, t["pnet.conv1.w"], t["pnet.conv1.b"], 3), t["pnet.prelu1"]), 2, 2, ceil_mode=True)
    a2 = prelu(conv(y, t["pnet.conv2.w"], t["pnet.conv2.b"], 10), t["pnet.prelu2"])[0].numpy()     # [16][h][w]
    # receptive fields of a sample of cells: [n][3][3][16] -> k = tap * 16 + channel
    rng = np.random.default_rng(1)
    h, w = a2.shape[1] - 2, a2.shape[2] - 2
    ys, xs = rng.integers(0, h, 1500), rng.integers(0, w, 1500)
    x = np.stack([a2[:, ys + dy, xs + dx].T for dy in range(3) for dx in range(3)], axis=1).reshape(-1, 144)
    de, ds = _d_pair(t, x)
    X = np.abs(x).max(1)
    assert np.all(np.abs(ds.astype(np.float64) - de) <= A * X + B)


@pytest.mark.parametrize("kind", ["large", "tiny", "mixed"])
def test_screen_within_bound_near_fp16_limits(kind):
    t = _tensors()
    A, B, _ = screen_bound(t)
    rng = np.random.default_rng({"large": 2, "tiny": 3, "mixed": 4}[kind])
    n = 800
    if kind == "large":       # activations up to the fp16 maximum (the largest the screen accepts)
        x = rng.uniform(-1, 1, (n, 144)) * rng.choice([1e2, 3e3, 6.5e4], (n, 1))
        x = np.clip(x, -65504, 65504)
    elif kind == "tiny":      # fp16 subnormals and below
        x = rng.uniform(-1, 1, (n, 144)) * rng.choice([1e-8, 6e-6, 6e-5], (n, 1))
    else:                     # values that round badly in fp16 next to large ones
        x = rng.uniform(-1, 1, (n, 144)) * 10.0 ** rng.integers(-8, 4, (n, 144))
        x[:, ::7] = 2049.0 * np.sign(rng.uniform(-1, 1, (n, 1)))
    de, ds = _d_pair(t, x.astype(np.float32))
    X = np.abs(x.astype(np.float32)).max(1).astype(np.float64)
    err = np.abs(ds.astype(np.float64) - de)
    assert np.all(np.isfinite(err))
    assert np.all(err <= A * X + B), float(np.max(err - (A * X + B)))
