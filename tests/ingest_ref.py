"""Plain restatement of the 4:2:0 -> BGR conversion that csrc/trl_ingest.hip (trl_ingest_nv12 / trl_ingest_i420) performs,
the reference the ingest tests (test_ingest_cpu.py, test_gpu_ingest.py) compare the kernel and the oracle with.  TEST
INFRASTRUCTURE ONLY.  It calls neither the oracle nor the library.

The rule, as include/truely_hip.h states it: OpenCV's integer BT.601 limited-range conversion (cvtColor COLOR_YUV2BGR_NV12) in
20-bit fixed point,

    y' = max(Y - 16, 0) * CY          u = U - 128          v = V - 128          half = 1 << 19
    B = clamp((y' + half + CUB * u) >> 20)     G = clamp((y' + half + CVG * v + CUG * u) >> 20)     R = clamp((y' + half + CVR * v) >> 20)

with clamp to 0..255, an arithmetic (floor) shift, and one chroma sample per 2x2 luma block.  The five constants are
round(coefficient * 2**20) of 1.164, 2.018, -0.391, -0.813, 1.596; they are RECALLED (no OpenCV is installed to pin them), so
``bt601_float`` -- the textbook formula with those three-decimal coefficients -- is the independent bound on them.
"""
from __future__ import annotations

import numpy as np

SHIFT = 20
CY, CUB, CUG, CVG, CVR = 1220542, 2116026, -409993, -852492, 1673527
COEFF = {"CY": 1.164, "CUB": 2.018, "CUG": -0.391, "CVG": -0.813, "CVR": 1.596}
EDGE_BYTES = np.array([0, 1, 15, 16, 17, 127, 128, 129, 234, 235, 236, 254, 255], np.uint8)
KINDS = ("noise", "edges", "flat", "ramp")
CUBE = 4096                                                   # the colour cube frame is CUBE x CUBE


# ---- the arithmetic, per sample ----------------------------------------------------------------------------------------------
def fixed_accumulators(Y, U, V):
    """The three sums before the shift, in int64, channel order B, G, R (broadcast over the inputs)."""
    Y, U, V = (np.asarray(a).astype(np.int64) for a in (Y, U, V))
    yy = np.maximum(Y - 16, 0) * CY
    half = 1 << (SHIFT - 1)
    u, v = U - 128, V - 128
    return yy + half + CUB * u + 0 * v, yy + half + CVG * v + CUG * u, yy + half + CVR * v + 0 * u


def fixed_bgr(Y, U, V) -> np.ndarray:
    """uint8 (..., 3) BGR of the integer rule."""
    acc = fixed_accumulators(Y, U, V)
    out = np.empty(acc[0].shape + (3,), np.uint8)
    for c, a in enumerate(acc):
        out[..., c] = np.clip(a >> SHIFT, 0, 255)
    return out


def bt601_float(Y, U, V, clamp: bool = False) -> np.ndarray:
    """float64 (..., 3) BGR of the textbook BT.601 limited-range formula (three-decimal coefficients), unclamped or clamped
    to [0, 255].  Not rounded."""
    Y, U, V = (np.asarray(a).astype(np.float64) for a in (Y, U, V))
    y = 1.164 * np.maximum(Y - 16.0, 0.0)
    u, v = U - 128.0, V - 128.0
    out = np.stack([y + 2.018 * u + 0.0 * v, y - 0.813 * v - 0.391 * u, y + 1.596 * v + 0.0 * u], axis=-1)
    return np.clip(out, 0.0, 255.0) if clamp else out


# ---- one frame -----------------------------------------------------------------------------------------------------------------
def planes(frame, H: int, W: int, planar: bool = False):
    """(Y [H, W], U [H/2, W/2], V [H/2, W/2]) views of one 4:2:0 frame of H*W*3/2 bytes: NV12 (interleaved U, V rows after the
    luma) or, with ``planar``, I420 (the U plane, then the V plane)."""
    f = np.asarray(frame)
    if f.dtype != np.uint8 or f.shape != (H * W * 3 // 2,) or H % 2 or W % 2:
        raise ValueError(f"a 4:2:0 frame of {H}x{W} is uint8 ({H * W * 3 // 2},), got {f.dtype} {f.shape}")
    hw, q = H * W, (H // 2) * (W // 2)
    Y = f[:hw].reshape(H, W)
    if planar:
        return Y, f[hw:hw + q].reshape(H // 2, W // 2), f[hw + q:].reshape(H // 2, W // 2)
    uv = f[hw:].reshape(H // 2, W // 2, 2)
    return Y, uv[:, :, 0], uv[:, :, 1]


def yuv420_to_bgr(frame, H: int, W: int, planar: bool = False) -> np.ndarray:
    """uint8 BGR [H, W, 3] of one NV12 (or, ``planar``, I420) frame: pixel (y, x) takes the chroma sample (y // 2, x // 2)."""
    Y, U, V = planes(frame, H, W, planar)
    up = lambda c: np.repeat(np.repeat(c.astype(np.int64), 2, axis=0), 2, axis=1)      # c[y // 2, x // 2] for every (y, x)
    return fixed_bgr(Y, up(U), up(V))


def nv12_to_i420(nv12, H: int, W: int) -> np.ndarray:
    """The same frame(s) with the interleaved chroma split into a U plane and a V plane; (fb,) or (n, fb)."""
    a = np.asarray(nv12)
    hw, q = H * W, (H // 2) * (W // 2)
    out = np.empty_like(a)
    out[..., :hw] = a[..., :hw]
    out[..., hw:hw + q] = a[..., hw::2]
    out[..., hw + q:] = a[..., hw + 1::2]
    return out


# ---- the whole colour cube in one frame ----------------------------------------------------------------------------------------
def cube_triple(y, x):
    """(Y, U, V) that the colour-cube frame holds at luma pixel (y, x) -- see colour_cube_nv12."""
    y, x = np.asarray(y), np.asarray(x)
    s = ((y // 2) % 8) * 8 + (x // 2) % 8
    return 4 * s + 2 * (y % 2) + x % 2, y // 16, x // 16


def colour_cube_nv12():
    """(nv12, i420): one 4096 x 4096 frame in which every (Y, U, V) triple occurs exactly once.

    Layout: the frame is a 256 x 256 grid of 16 x 16-pixel luma tiles; tile (row r, column c) has U = r and V = c in all of its
    8 x 8 = 64 chroma samples, and its 256 luma bytes are 0..255: chroma sample s = 8 * ((y // 2) % 8) + (x // 2) % 8 of the tile
    covers the 2 x 2 luma block Y = 4 s + 2 (y % 2) + (x % 2).  So luma pixel (y, x) holds the triple
    ``cube_triple(y, x)`` = (4 s + 2 (y % 2) + x % 2, y // 16, x // 16), and triple (Y, U, V) sits at
    y = 16 U + 2 ((Y // 4) // 8) + (Y % 4) // 2,  x = 16 V + 2 ((Y // 4) % 8) + Y % 2."""
    n = CUBE
    yy, xx = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    Y, _, _ = cube_triple(yy, xx)
    cy, cx = np.meshgrid(np.arange(n // 2), np.arange(n // 2), indexing="ij")
    nv12 = np.empty(n * n * 3 // 2, np.uint8)
    nv12[:n * n] = Y.astype(np.uint8).reshape(-1)
    uv = nv12[n * n:].reshape(n // 2, n // 2, 2)
    uv[:, :, 0] = cy // 8
    uv[:, :, 1] = cx // 8
    return nv12, nv12_to_i420(nv12, n, n)


# ---- content -------------------------------------------------------------------------------------------------------------------
def content(kind: str, n: int, H: int, W: int, seed: int = 0) -> np.ndarray:
    """n seeded NV12 frames (n, H*W*3/2).  ``noise``: uniform bytes; ``edges``: only the bytes where the rule changes regime
    (EDGE_BYTES); ``flat``: one (Y, U, V) triple per frame, different in every frame; ``ramp``: luma and chroma gradients that
    move with the frame index, so every frame and every row of a frame differ."""
    rng = np.random.default_rng([seed, KINDS.index(kind), H, W])
    hw, fb = H * W, H * W * 3 // 2
    if kind == "noise":
        return rng.integers(0, 256, (n, fb), dtype=np.uint8)
    if kind == "edges":
        return EDGE_BYTES[rng.integers(0, len(EDGE_BYTES), (n, fb))]
    out = np.empty((n, fb), np.uint8)
    if kind == "flat":
        t = rng.choice(1 << 24, n, replace=False)                      # distinct triples
        for i in range(n):
            out[i, :hw] = (t[i] >> 16) & 255
            out[i, hw::2] = (t[i] >> 8) & 255
            out[i, hw + 1::2] = t[i] & 255
        return out
    if kind == "ramp":
        o = rng.integers(0, 256, 3)
        y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        cy, cx = np.meshgrid(np.arange(H // 2), np.arange(W // 2), indexing="ij")
        for i in range(n):
            out[i, :hw] = ((x + 3 * y + 17 * i + o[0]) & 255).reshape(-1)
            out[i, hw::2] = ((5 * cx + cy + 29 * i + o[1]) & 255).reshape(-1)
            out[i, hw + 1::2] = ((cx + 7 * cy + 43 * i + o[2]) & 255).reshape(-1)
        return out
    raise ValueError(kind)
