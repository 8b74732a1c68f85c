"""Reference of InceptionResnetV1's classifier head (trl_facenet_logits), and the inputs its tests share.

The device computes, per output, ONE float32 fma chain:

    logit[r][c] = chain(b[c]; k = 0..511 ascending: acc = fmaf(feat[r][k], w[k][c], acc))

:func:`logits_ref` restates it on front_ref.fma32, the exact float32 fma (product in float64, TwoSum, round to odd).  fma32 covers
finite operands; a step in which an operand is infinite or NaN is taken in float64 instead, where the product and the sum have
the class and sign IEEE gives the fused operation (once an operand is not finite, no rounding is left to get wrong)."""
from __future__ import annotations

import functools

import numpy as np

from front_ref import fma32

F32 = np.float32
K = 512
U = 2.0 ** -24


def logits_ref(feat: np.ndarray, w: np.ndarray, b: np.ndarray, block: int = 2048) -> np.ndarray:
    """feat (n, 512), w (512, C), b (C,) float32 -> (n, C) float32.  Columns are taken `block` at a time (temporaries in cache)."""
    feat, w, b = np.asarray(feat, F32), np.asarray(w, F32), np.asarray(b, F32)
    n, C = feat.shape[0], w.shape[1]
    assert feat.shape == (n, K) and w.shape == (K, C) and b.shape == (C,)
    out = np.empty((n, C), F32)
    odd_rows = ~np.isfinite(feat).all(axis=1)
    w_finite = bool(np.isfinite(w).all() and np.isfinite(b).all())
    with np.errstate(all="ignore"):
        for c0 in range(0, C, block):
            wb = w[:, c0:c0 + block]
            acc = np.broadcast_to(b[c0:c0 + block], (n, wb.shape[1])).copy()
            for k in range(K):
                x = feat[:, k, None]
                nxt = fma32(x, wb[k][None, :], acc)
                if odd_rows.any() or not w_finite:
                    bad = ~(np.isfinite(x) & np.isfinite(wb[k][None, :]) & np.isfinite(acc))
                    if bad.any():
                        plain = (x.astype(np.float64) * wb[k][None, :].astype(np.float64) + acc.astype(np.float64)).astype(F32)
                        nxt = np.where(bad, plain, nxt)
                acc = nxt
            out[:, c0:c0 + block] = acc
    return out


def gamma(m: int) -> float:
    """Higham's gamma_m = m u / (1 - m u) for float32."""
    return m * U / (1.0 - m * U)


def same_bits(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Elementwise: equal as uint32, or both NaN (NaN equals NaN by class)."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


# ---- shared inputs ---------------------------------------------------------------------------------------------------------------
N_TABLE = 65


@functools.lru_cache(maxsize=None)
def feature_table() -> np.ndarray:
    """65 feature rows: random normal ones, and at fixed places (inside the first tile, on both sides of the 32-row tile edge,
    and the one row of the third tile) rows of zeros, one-hot rows, a row holding +-inf, one holding NaN, and rows at the float32
    subnormal range."""
    rng = np.random.default_rng(4242)
    f = rng.standard_normal((N_TABLE, K)).astype(F32)
    f[1] = 0
    f[2] = 0; f[2, 0] = 1                                   # one-hot rows read w[k][c] + b[c] back
    f[3, 7] = np.inf; f[3, 300] = -np.inf                   # +-inf (some classes end at inf, some at NaN)
    f[4, 511] = np.nan
    f[5] = (rng.standard_normal(K) * 2.0 ** -126).astype(F32)          # subnormal and smallest-normal values
    f[6] = 0; f[6, 511] = 1
    f[7, ::3] = (rng.standard_normal(len(f[7, ::3])) * 2.0 ** -140).astype(F32)   # deep subnormals beside ordinary values
    f[30] = 0; f[30, 255] = -2
    f[31] = 0
    f[32, 100] = -np.inf
    f[33] = 0; f[33, 256] = 1
    f[63, 0] = np.nan
    f[64] = 0; f[64, 1] = 3
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def base_tensors():
    """The canonical tensors of synthetic_state_dicts(0) (no classifier), computed once."""
    from truely_amd import weights
    return weights.canonical_tensors(*weights.synthetic_state_dicts(0))


@functools.lru_cache(maxsize=None)
def head(C: int):
    """(w [512][C], b [C]) of synthetic_state_dicts(0, num_classes=C): the classifier comes from a generator of its own."""
    from truely_amd import weights
    sd = weights.synthetic_logits(0, C)
    w = np.ascontiguousarray(sd["logits.weight"].T)
    w.setflags(write=False)
    return w, sd["logits.bias"]


def blob_with_head(C: int, w: np.ndarray | None = None, b: np.ndarray | None = None) -> bytes:
    """The bytes of pack_state_dicts(*synthetic_state_dicts(0, num_classes=C)) (test_logits_cpu.py checks that) without
    generating the other tensors again; w / b override the two classifier tensors (refusal tests)."""
    from truely_amd import weights
    t = dict(base_tensors())
    hw, hb = head(C)
    t["facenet.logits.w"] = hw if w is None else w
    t["facenet.logits.b"] = hb if b is None else b
    return weights.pack_tensors(t)


@functools.lru_cache(maxsize=None)
def table_ref(C: int, n: int = N_TABLE) -> np.ndarray:
    """logits_ref of the first n table rows against head(C), computed once per C."""
    w, b = head(C)
    r = logits_ref(feature_table()[:n], w, b)
    r.setflags(write=False)
    return r
