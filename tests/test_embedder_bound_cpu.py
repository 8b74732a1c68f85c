"""CPU side of the reduced-precision embedder tests (tests/test_gpu_embedder.py): the numpy RNE16 helpers against torch's
conversions, and the per-element error bound of DESIGN.md section 2 ("Embedder dispatch under test") against f32 accumulations
emulated in random orders.  The helpers live here so that the GPU file imports exactly what this file checks."""
import numpy as np
import pytest
import torch

U32 = 2.0 ** -24                      # unit roundoff of f32
FMT = {1: dict(p=8, emin=-126, big=float(torch.finfo(torch.bfloat16).max)),
       2: dict(p=11, emin=-14, big=65504.0)}


def rne16(v, fmt):
    """Round float64 values to bf16 (fmt 1) or fp16 (fmt 2) with round-to-nearest-even, in one step (no double rounding through
    f32); overflow gives +-inf, NaN stays NaN.  Returns float64 values (exactly representable in the format)."""
    v = np.asarray(v, np.float64)
    p, emin, big = FMT[fmt]["p"], FMT[fmt]["emin"], FMT[fmt]["big"]
    with np.errstate(invalid="ignore", over="ignore"):
        _, e = np.frexp(v)                                    # |v| in [2^(e-1), 2^e)
        ulp = np.ldexp(1.0, np.maximum(e, emin + 1) - p)      # subnormals: the spacing of the smallest binade
        r = np.rint(v / ulp) * ulp                            # np.rint: ties to even
        r = np.where(np.abs(r) > big, np.copysign(np.inf, v), r)
    return np.where(np.isfinite(v), r, v)


def to_bits(v16, fmt):
    """float64 values already in the format -> their 16-bit patterns (uint16)."""
    v16 = np.asarray(v16, np.float64)
    if fmt == 2:
        return v16.astype(np.float16).view(np.uint16)
    return (v16.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


def from_bits(b, fmt):
    """16-bit patterns -> float64 values."""
    b = np.asarray(b, np.uint16)
    if fmt == 2:
        return b.view(np.float16).astype(np.float64)
    return (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


MFMA_K = 16                           # k per v_mfma_f32_32x32x16_{bf16,f16}: the accumulation's unit


def accumulate(A, W, bias, blk=MFMA_K):
    """Exact value S (float64) of bias + A @ W and a bound e0 on |f32 accumulation - S|.

    The kernel's chain: acc = bias, then one matrix instruction per block of `blk` consecutive k, ascending.  Each instruction adds
    its block's products (exact in f32: 16-bit x 16-bit operands) to acc in an order the hardware does not specify; every f32
    addition is assumed faithfully rounded (error < 2u of its result), so an instruction adds at most gamma(blk) (|acc| + T_b) with
    gamma(n) = 2 n u / (1 - 2 n u).  The device acc differs from the exact prefix P_j by e_j, so |acc| <= |P_j| + e_j."""
    A = np.asarray(A, np.float64)
    W = np.asarray(W, np.float64)
    K = A.shape[1]
    g = 2 * (blk + 1) * U32 / (1 - 2 * (blk + 1) * U32)
    P = np.broadcast_to(np.asarray(bias, np.float64), (A.shape[0], W.shape[1])).copy()
    e = np.zeros_like(P)
    absA, absW = np.abs(A), np.abs(W)
    for k0 in range(0, K, blk):
        Tb = absA[:, k0:k0 + blk] @ absW[k0:k0 + blk]
        e = e + g * (np.abs(P) + e + Tb)
        P = P + A[:, k0:k0 + blk] @ W[k0:k0 + blk]
    T = absA @ absW + np.abs(np.asarray(bias, np.float64))
    return P, e + 4 * K * 2.0 ** -53 * T                      # + the float64 reference's own summation error


def epilogue_interval(S, e0, scale=None, shift=None, res=None, res_scale=1.0, relu=True, fmt=1):
    """The interval [lo, hi] (16-bit values as float64) a device output must lie in, and the exact value.

    S, e0: from accumulate().  The epilogue: v1 = fma(acc, scale, shift), v2 = fl(fl(v1 * res_scale) + res), ReLU, one RNE to 16
    bits.  Each f32 rounding adds at most u times the magnitude of its result; the bound is carried as an absolute error through
    the monotone steps, so a negative scale (which flips [S - e0, S + e0]) needs no special case."""
    u = U32
    e = e0
    V = S
    if scale is not None:
        sc = np.asarray(scale, np.float64)
        V = S * sc + np.asarray(shift, np.float64)
        e = np.abs(sc) * e
        e = e + u * (np.abs(V) + e)
    if res is not None:
        rs = float(np.float32(res_scale))
        P = V * rs
        e = abs(rs) * e
        e = e + u * (np.abs(P) + e)
        V = P + res
        e = e + u * (np.abs(V) + e)
    e = e * (1 + 2.0 ** -40) + 2.0 ** -50 * np.abs(V)         # float64 evaluation of V itself
    lo, hi = V - e, V + e
    if relu:
        lo, hi = np.maximum(lo, 0.0), np.maximum(hi, 0.0)
    return rne16(lo, fmt), rne16(hi, fmt), V


# ---- the helpers equal torch's conversions -----------------------------------------------------------------------------------

def _special_values(fmt):
    rng = np.random.default_rng(fmt)
    p = FMT[fmt]["p"]
    vals = [0.0, -0.0, 1.0, -1.0, 65504.0, 65519.99, 65520.0, 65536.0, 1e30, -1e30, 3.0e38, 6e-8, 5.96e-8, 2.98e-8, 2.99e-8,
            1e-40, 1e-45, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -26, 2.0 ** -14 * (1 - 2.0 ** -11)]
    base = rng.uniform(-4, 4, 2000) * 2.0 ** rng.integers(-30, 20, 2000)
    ties = []
    for x in base[:500]:                                      # exact midpoints between neighbours: the ties-to-even cases
        f = float(rne16(x, fmt))
        if f == 0 or not np.isfinite(f):
            continue
        _, e = np.frexp(f)
        ulp = 2.0 ** (max(e, FMT[fmt]["emin"] + 1) - p)
        ties += [f + ulp / 2, f - ulp / 2]
    sub = (np.arange(-40, 40) + 0.5) * 2.0 ** (FMT[fmt]["emin"] - p + 1)    # subnormal midpoints
    return np.concatenate([vals, base, ties, sub, rng.standard_normal(2000)]).astype(np.float64)


@pytest.mark.parametrize("fmt", [1, 2])
def test_rne16_equals_torch(fmt):
    """rne16 / to_bits equal torch's .to(bfloat16) / .to(float16) bit for bit: ties, subnormals, overflow and signed zero included.
    torch converts from float32, so the inputs are float32 values (every midpoint of a 16-bit format is one)."""
    x = _special_values(fmt).astype(np.float32)
    t = torch.from_numpy(x).to(torch.bfloat16 if fmt == 1 else torch.float16)
    want = t.view(torch.int16).numpy().view(np.uint16)
    got = to_bits(rne16(x.astype(np.float64), fmt), fmt)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(float(x[i]), hex(got[i]), hex(want[i])) for i in bad[:5]]
    back = from_bits(want, fmt)
    fin = np.isfinite(back)
    assert np.array_equal(back[fin], t.to(torch.float64).numpy()[fin])


def test_rne16_fp16_subnormals_and_ties_directly():
    tiny = 2.0 ** -24                                         # the smallest fp16 subnormal
    assert rne16(0.5 * tiny, 2) == 0.0 and rne16(1.5 * tiny, 2) == 2 * tiny and rne16(2.5 * tiny, 2) == 2 * tiny
    assert rne16(65519.0, 2) == 65504.0 and np.isinf(rne16(65520.0, 2))
    assert rne16(1 + 2.0 ** -8, 1) == 1.0 and rne16(1 + 3 * 2.0 ** -8, 1) == 1 + 2.0 ** -6


# ---- the bound holds for emulated f32 accumulations in random orders -----------------------------------------------------------

def _emulate(terms, rng, mode):
    """f32 accumulation of the terms (bias first among them) in a random order: a sequential chain or a random pairwise tree."""
    t = terms.astype(np.float32)
    if mode == 0:
        order = rng.permutation(len(t))
        acc = np.float32(0)
        for i in order:
            acc = np.float32(acc + t[i])
        return acc
    vals = list(t[rng.permutation(len(t))])
    while len(vals) > 1:
        i = int(rng.integers(0, len(vals) - 1))
        vals[i:i + 2] = [np.float32(vals[i] + vals[i + 1])]
    return vals[0]


@pytest.mark.parametrize("fmt", [1, 2])
def test_bound_holds_for_random_orders(fmt):
    """Random layers (16-bit operands, f32 bias / scale / shift, a residual of the format, ReLU or not, negative scales included):
    every emulated device result -- f32 accumulation over blocks of 16 k with a random order inside each, the epilogue in f32 with
    the kernel's roundings, one RNE to 16 bits -- lies in the interval, and the interval mostly holds a single 16-bit value."""
    rng = np.random.default_rng(7 + fmt)
    single = total = 0
    for trial in range(60):
        K = int(rng.choice([9, 32, 96, 288, 896, 1792]))
        x = rne16(np.abs(rng.standard_normal(K)) * rng.uniform(0.1, 30), fmt)
        w = rne16(rng.standard_normal((K, 8)) * 0.05, fmt)
        bias = rng.standard_normal(8).astype(np.float32) * 0.1
        has_scale, has_res, relu = bool(rng.integers(2)), bool(rng.integers(2)), bool(rng.integers(2))
        sc = (rng.uniform(-2, 2, 8)).astype(np.float32) if has_scale else None
        sf = (rng.standard_normal(8) * 0.3).astype(np.float32) if has_scale else None
        res = rne16(rng.standard_normal(8) * 3, fmt) if has_res else None
        rs = float(rng.choice([0.17, 0.1, 0.2, 1.0]))
        prods = x[:, None] * w                                # exact in float64 and in f32 (<= 22 significant bits)
        S, e0 = accumulate(x[None, :], w, bias.astype(np.float64))
        lo, hi, _ = epilogue_interval(S[0], e0[0], sc, sf, res, rs, relu, fmt)
        for j in range(8):
            acc = np.float32(bias[j])
            for k0 in range(0, K, MFMA_K):                    # blocks ascending, a random order inside each
                acc = _emulate(np.concatenate([[acc], prods[k0:k0 + MFMA_K, j]]), rng, trial % 2)
            v = acc
            if has_scale:
                v = np.float32(np.float64(acc) * np.float64(sc[j]) + np.float64(sf[j]))    # fma: one rounding (exact in f64)
            if has_res:
                v = np.float32(np.float32(v * np.float32(rs)) + np.float32(res[j]))
            if relu:
                v = v if v > 0 else np.float32(0)
            d = rne16(np.float64(v), fmt)
            assert lo[j] <= d <= hi[j], (trial, j, float(lo[j]), float(d), float(hi[j]))
            single += lo[j] == hi[j]
            total += 1
    assert single >= 0.75 * total, (single, total)          # adversarial cancellation here; the network's share is the GPU test's
