"""The embedder (InceptionResnetV1) path by path, at the face counts the product and the benchmark use.

A kernel and tile are chosen per conv from M = faces x OH x OW (trl_launch_conv, trl_fn_eligible / pick_tile in trl_fnconv.hip,
launch_cfg, trl_launch_conv_bf16).  The cases below sit on both sides of every threshold of that dispatch; trl_debug_facenet_plan
records what each call chose, and test_plan_covers_every_path checks that the cases reach every path the shipped dispatch can take.

- f32 (the parity path): every row of every case has the bits of the same face embedded in a call of at most 8 faces; sampled rows
  have the oracle's bits.
- bf16 / fp16: every conv of the network, layer by layer from its captured 16-bit input (trl_debug_facenet_capture), against a
  float64 reference with the per-element bound of DESIGN.md section 2; the to-16-bit conversion, the 16-bit max pools and the
  16-bit average pool exactly.
- fp16 overflow: a face whose activations leave fp16's range gets a non-finite embedding, the other faces keep their bits; a conv
  weight outside the range is refused at load."""
import numpy as np
import pytest
import torch

import truely_amd
from test_embedder_bound_cpu import accumulate, epilogue_interval, from_bits, rne16, to_bits

pytestmark = pytest.mark.gpu

# (crop, faces, precision, no_fnconv).  Thresholds (faces): 80 px -- block35_grouped / block35 fn <-> conv_tap at 334 / 335
# (M = n x 49 > 16384); block17's four-chain tiles at 455 / 456 (M = n x 9 > 4096) and leaving the small-map family at 1820 / 1821
# (> 16384); block8's by-N tiles past 512 faces (M = n > 512); conv_bf16's 128-row tile for conv2d_4a at 31 / 32 (M = n x 256 >= 8192).
# 160 px -- block35 at 56 / 57 (n x 289), block17 at 256 / 257 (n x 64), block8 at 56 / 57 and 455 / 456 (n x 9), conv_bf16 at
# 6 / 7 (conv2d_4a, n x 1296).  Odd counts keep M off every tile multiple.
CASES = [
    (80, 2048, 0, False),    # bench.py's default call: --embed-group 8 x 256 faces
    (80, 1821, 0, False), (80, 1820, 0, False), (80, 457, 0, False), (80, 456, 0, False), (80, 455, 0, False),
    (80, 335, 0, False), (80, 334, 0, False), (80, 513, 0, False), (80, 57, 0, False), (80, 7, 0, False),
    (80, 457, 0, True), (80, 1821, 0, True), (80, 13, 0, True), (80, 3, 0, True),
    (160, 257, 0, False), (160, 256, 0, False), (160, 57, 0, False), (160, 56, 0, False), (160, 456, 0, False), (160, 455, 0, False),
    (160, 3, 0, False), (160, 57, 0, True), (160, 5, 0, True),
    (80, 1024, 1, False),    # configs[2]: 128 frames x --embed-group 8, bf16
    (80, 256, 2, False),     # configs[4]: 32 frames x 8, fp16
    (80, 31, 1, False), (80, 32, 1, False), (80, 31, 2, False), (80, 33, 2, False),
    (160, 6, 1, False), (160, 7, 1, False), (160, 6, 2, False), (160, 7, 2, False), (160, 1, 1, False),
]
PREC = {0: "f32", 1: "bf16", 2: "fp16"}

# Every (family, bm, bn, bk, pad) the dispatch selects for FaceNet's layer shapes at crops of 80 and 160 px (any face count, the
# small-map family on or off, f32 / bf16 / fp16); the fn_conv / fn_conv_split4 entries are every tile those families instantiate.
# test_gpu_embedder_sizes.py finds no other path at 75 to 224 px, square or not, within its workspace cap.  Instantiated but never
# selected for FaceNet at those sizes: conv_igemm_vec (no tap chunk divides Cin, or inputs past 32-bit element offsets),
# conv_tap48 (Cout 48: R-Net conv2, see test_gpu_stage_nets.py),
# conv_tap BK 28 and conv_splitk4 (no shipped network selects them: R-Net's conv2, the one Cin 28 layer, takes conv_tap48 where a
# 128 x 64 tile would apply, and the R-/O-Net dense layers take conv_splitk4_tap), conv_tap with padding and BK 16 (every padded
# conv has Cin % 32 == 0), conv_bf16 with padding and BK 16 (likewise).
EXPECTED_PATHS = {
    ("conv_igemm_scalar", 128, 32, 16, 0),                                            # the 3-channel stem
    ("fn_conv", 32, 32, 32, 0), ("fn_conv", 64, 64, 32, 0),
    ("fn_conv_split4", 16, 32, 32, 0), ("fn_conv_split4", 32, 32, 32, 0), ("fn_conv_split4", 48, 32, 32, 0),
    ("fn_conv_split4", 48, 64, 32, 0),
    ("conv_tap", 32, 128, 16, 0), ("conv_tap", 32, 128, 32, 0), ("conv_tap", 32, 128, 64, 0), ("conv_tap", 32, 128, 64, 1),
    ("conv_tap", 64, 64, 16, 0), ("conv_tap", 64, 64, 32, 0), ("conv_tap", 64, 64, 32, 1), ("conv_tap", 64, 64, 64, 0),
    ("conv_tap", 64, 64, 64, 1),
    ("conv_tap", 128, 32, 32, 0), ("conv_tap", 128, 32, 32, 1), ("conv_tap", 128, 64, 16, 0), ("conv_tap", 128, 64, 32, 0),
    ("conv_tap", 128, 64, 32, 1),
    ("conv_splitk4_tap", 32, 64, 16, 0), ("conv_splitk4_tap", 32, 64, 16, 1), ("conv_splitk4_tap", 32, 64, 32, 0),
    ("conv_splitk4_tap", 32, 64, 32, 1),
    ("conv_bf16", 64, 64, 16, 0), ("conv_bf16", 64, 64, 32, 0), ("conv_bf16", 64, 64, 32, 1),
    ("conv_bf16", 128, 64, 16, 0), ("conv_bf16", 128, 64, 32, 0), ("conv_bf16", 128, 64, 32, 1),
}
POOL_N = {80: 2048, 160: 457}


@pytest.fixture(scope="module")
def pools():
    return {S: np.random.default_rng(1000 + S).uniform(0, 1, (n, S, S, 3)).astype(np.float32) for S, n in POOL_N.items()}


@pytest.fixture(scope="module")
def engines(blob):
    from truely_amd.engine import Engine
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return {p: Engine(blob, embed_precision=PREC[p]) for p in (0, 1, 2)}


def _embed(eng, x):
    return eng.facenet_embed(torch.from_numpy(x)).cpu().numpy()


@pytest.fixture(scope="module")
def small_calls(engines, pools):
    """The f32 embedding of every pool face from calls of at most 8 faces (the reference of batch independence)."""
    eng = engines[0]
    return {S: np.concatenate([_embed(eng, pools[S][i:i + 8]) for i in range(0, len(pools[S]), 8)]) for S in pools}


@pytest.fixture(scope="module")
def case_runs(engines, pools):
    """Every case once: (embeddings, plan)."""
    out = {}
    for case in CASES:
        S, n, p, nofn = case
        eng = engines[p]
        if nofn:
            eng.option("no_fnconv", 1)
        try:
            emb = _embed(eng, pools[S][:n])
            out[case] = (emb, eng.facenet_plan())
        finally:
            if nofn:
                eng.option("no_fnconv", 0)
    return out


def _key(r):
    return (r["family"], r["bm"], r["bn"], r["bk"], r["pad"])


def test_plan_records_every_conv(case_runs):
    """One row per conv in walk order; the f32 stem and last_linear stay f32 in reduced-precision mode."""
    for (S, n, p, nofn), (_, plan) in case_runs.items():
        assert [r["conv"] for r in plan] == list(range(len(plan)))
        assert len(plan) == 1 + 5 + 5 * 5 + 4 + 10 * 4 + 5 + 6 * 4 + 1
        assert plan[0]["layer"] == "facenet.conv2d_1a" and plan[-1]["layer"] == "facenet.last_linear"
        assert plan[0]["m"] == n * ((S - 3) // 2 + 1) ** 2 and plan[-1]["m"] == n
        for r in plan:
            lowp = p if r["layer"] not in ("facenet.conv2d_1a", "facenet.last_linear") else 0
            assert r["precision"] == lowp, r
            assert (r["family"] == "conv_bf16") == (lowp > 0), r
            assert r["has_res"] == r["layer"].endswith(".conv2d"), r
            if nofn:
                assert not r["family"].startswith("fn_"), r
        assert all(r["family"].startswith("fn_") for r in plan if r["nz"] > 1)


def test_plan_covers_every_path(case_runs):
    seen = set()
    for _, plan in case_runs.values():
        seen |= {_key(r) for r in plan}
    assert EXPECTED_PATHS <= seen, sorted(EXPECTED_PATHS - seen)
    assert seen <= EXPECTED_PATHS, sorted(seen - EXPECTED_PATHS)          # a path the comment above does not know about


def test_plan_reaches_the_paths_the_suite_missed(case_runs):
    """block17's four-chain convs on conv_splitk4_tap at 2,048 faces with the small-map family on; their fn_conv_split4 M > 4096
    tile between 456 and 1,820 faces; block8's tiles chosen by N past 512 faces; conv_bf16<128, 64, 16> at configs[2]'s size."""
    def tiles(case, part):
        return {_key(r)[:3] for r in case_runs[case][1] if part in r["layer"] and not r["layer"].endswith(".conv2d")}
    assert tiles((80, 2048, 0, False), ".repeat_2.") == {("conv_splitk4_tap", 32, 64)}
    assert tiles((80, 457, 0, False), ".repeat_2.") == {("fn_conv_split4", 32, 32)}
    assert tiles((80, 513, 0, False), ".repeat_3.") == {("fn_conv_split4", 32, 32), ("fn_conv_split4", 48, 64)}
    assert tiles((80, 335, 0, False), ".repeat_2.") == {("fn_conv_split4", 48, 64), ("fn_conv_split4", 48, 32)}
    assert any(_key(r) == ("conv_bf16", 128, 64, 16, 0) and r["layer"] == "facenet.conv2d_4a" for r in case_runs[(80, 1024, 1, False)][1])


@pytest.mark.parametrize("case", [c for c in CASES if c[2] == 0], ids=str)
def test_f32_rows_are_batch_independent_and_exact(case, case_runs, small_calls, pools, oracle):
    S, n, _, _ = case
    emb, plan = case_runs[case]
    ref = small_calls[S][:n]
    bad = np.nonzero((emb != ref).any(1))[0]
    assert bad.size == 0, f"{bad.size} rows differ from <= 8-face calls, first {bad[:8]}"
    # the oracle: first and last rows, and the faces owning the last partial M-tile of the largest-M layer
    big = max(plan, key=lambda r: r["m"])
    per = big["m"] // n
    tile0 = (big["m"] - 1) // big["bm"] * big["bm"]
    idx = sorted({0, n - 1} | set(range(tile0 // per, n)))
    assert np.array_equal(emb[idx], oracle.facenet(pools[S][idx])), idx


def test_f32_largest_case_over_poisoned_workspace(blob, pools, small_calls):
    from truely_amd.engine import Engine
    eng = Engine(blob)
    eng.poison_workspaces(0xFF)
    emb = _embed(eng, pools[80][:2048])
    assert np.array_equal(emb, small_calls[80][:2048])
    eng.close()


@pytest.mark.parametrize("case", [c for c in CASES if c[2] > 0], ids=str)
def test_reduced_precision_cases_close_to_oracle(case, case_runs, pools, oracle):
    """End to end at the product's sizes, with the existing bars (bf16: cos >= 0.999, |diff| <= 3e-2; fp16: 0.99999, 3e-3)."""
    S, n, p, _ = case
    emb = case_runs[case][0]
    idx = np.unique(np.linspace(0, n - 1, min(n, 24)).astype(int))
    ref = oracle.facenet(pools[S][idx])
    cos = (emb[idx] * ref).sum(1)
    assert np.isfinite(emb).all()
    assert cos.min() >= (0.999 if p == 1 else 0.99999) and np.abs(emb[idx] - ref).max() <= (3e-2 if p == 1 else 3e-3)


# ---- bf16 / fp16 layer by layer ----------------------------------------------------------------------------------------------

_TOP = {"conv2d_2a": (3, 3, 1, 0, 0), "conv2d_2b": (3, 3, 1, 1, 1), "conv2d_3b": (1, 1, 1, 0, 0), "conv2d_4a": (3, 3, 1, 0, 0),
        "conv2d_4b": (3, 3, 2, 0, 0), "mixed_6a.branch0": (3, 3, 2, 0, 0), "mixed_6a.branch1.0": (1, 1, 1, 0, 0),
        "mixed_6a.branch1.1": (3, 3, 1, 1, 1), "mixed_6a.branch1.2": (3, 3, 2, 0, 0), "mixed_7a.fused": (1, 1, 1, 0, 0),
        "mixed_7a.branch0.1": (3, 3, 2, 0, 0), "mixed_7a.branch1.1": (3, 3, 2, 0, 0), "mixed_7a.branch2.1": (3, 3, 1, 1, 1),
        "mixed_7a.branch2.2": (3, 3, 2, 0, 0)}
_BRANCH = {"repeat_1": {"branch1.1": (3, 3, 1, 1, 1), "branch2.1": (3, 3, 1, 1, 1), "branch2.2": (3, 3, 1, 1, 1)},
           "repeat_2": {"branch1.1": (1, 7, 1, 0, 3), "branch1.2": (7, 1, 1, 3, 0)},
           "repeat_3": {"branch1.1": (1, 3, 1, 0, 1), "branch1.2": (3, 1, 1, 1, 0)}}
_BRANCH["block8"] = _BRANCH["repeat_3"]
_RES_SCALE = {"repeat_1": 0.17, "repeat_2": 0.10, "repeat_3": 0.20, "block8": 1.0}
FUSED_PARTS = {"repeat_1": ("branch0", "branch2.0", "branch1.0"), "repeat_2": ("branch0", "branch1.0"),
               "repeat_3": ("branch0", "branch1.0"), "block8": ("branch0", "branch1.0"),
               "mixed_7a": ("branch0.0", "branch1.0", "branch2.0")}


def _split(layer):
    """'facenet.repeat_2.3.branch1.1' -> ('repeat_2', 'facenet.repeat_2.3', 'branch1.1')."""
    l = layer[len("facenet."):]
    if l.startswith(("repeat_1.", "repeat_2.", "repeat_3.")):
        fam, i, leaf = l.split(".", 2)
        return fam, f"facenet.{fam}.{i}", leaf
    fam, leaf = l.split(".", 1)
    return fam, f"facenet.{fam}", leaf


def _geometry(layer):
    """(kh, kw, stride, ph, pw, relu, residual scale or None) of a FaceNet conv by name."""
    l = layer[len("facenet."):]
    if l in _TOP:
        return _TOP[l] + (True, None)
    fam, _, leaf = _split(layer)
    if leaf == "fused":
        return (1, 1, 1, 0, 0, True, None)
    if leaf == "conv2d":
        return (1, 1, 1, 0, 0, fam != "block8", _RES_SCALE[fam])
    return _BRANCH[fam][leaf] + (True, None)


def _layer_params(T, layer):
    """(w [K][Cout], bias or None, scale or None, shift or None) as the library packs them (a fused conv is its parts' columns side by side: csrc/trl_weights.h)."""
    if layer.endswith(".fused"):
        fam, blk, _ = _split(layer)
        cat = lambda suf: np.concatenate([T[f"{blk}.{q}.{suf}"] for q in FUSED_PARTS[fam]], axis=-1)
        return cat("w"), None, cat("scale"), cat("shift")
    if layer.endswith(".conv2d"):
        return T[layer + ".w"], T[layer + ".b"], None, None
    return T[layer + ".w"], None, T[layer + ".scale"], T[layer + ".shift"]


def _rows_to_check(M, bm, rng, n_random=768):
    """A random sample of output rows plus the last row of every M-tile (at most 256 of them) and the whole last partial tile."""
    tails = np.arange(bm - 1, M, bm)
    if tails.size > 256:
        tails = rng.choice(tails, 256, replace=False)
    last = np.arange((M - 1) // bm * bm, M)
    rand = rng.choice(M, min(M, n_random), replace=False)
    return np.unique(np.concatenate([rand, tails, last, [0, M - 1]])).astype(np.int64)


def _im2col(x, rows, OH, OW, kh, kw, st, ph, pw):
    """Patches of the selected output rows, k = (ky * kw + kx) * Cin + c (the weight rows' order), zero padding."""
    n, H, W, C = x.shape
    img, rem = rows // (OH * OW), rows % (OH * OW)
    oy, ox = rem // OW, rem % OW
    out = np.zeros((rows.size, kh * kw * C), np.float64)
    for ky in range(kh):
        for kx in range(kw):
            iy, ix = oy * st - ph + ky, ox * st - pw + kx
            ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
            t = (ky * kw + kx) * C
            out[ok, t:t + C] = x[img[ok], iy[ok], ix[ok], :]
    return out


def _check_layer(r, cap, T, fmt, rng):
    """The captured output of one conv lies, element by element, in the interval of DESIGN.md section 2 around the float64 value
    computed from the captured 16-bit input (and residual).  Returns (single-valued intervals, elements, outputs == RNE16(v))."""
    xin, res, y = cap
    kh, kw, st, ph, pw, relu, rs = _geometry(r["layer"])
    n, H, W, Cin = xin.shape
    _, OH, OW, Cout = y.shape
    assert kh * kw * Cin == r["k"] and Cout == r["cout"] and n * OH * OW == r["m"], r
    w, b, sc, sf = _layer_params(T, r["layer"])
    assert w.shape == (r["k"], Cout), (r["layer"], w.shape)
    wq = rne16(w.astype(np.float64), fmt)                               # the library's f2lp of the weights
    rows = _rows_to_check(r["m"], r["bm"], rng)
    A = _im2col(from_bits(xin, fmt), rows, OH, OW, kh, kw, st, ph, pw)
    bias = b.astype(np.float64) if b is not None else np.zeros(Cout)
    S, e0 = accumulate(A, wq, bias)
    resv = from_bits(res.reshape(-1, Cout)[rows], fmt) if res is not None else None
    lo, hi, V = epilogue_interval(S, e0, sc, sf, resv, rs if rs is not None else 1.0, relu, fmt)
    d = from_bits(y.reshape(-1, Cout)[rows], fmt)
    bad = np.argwhere(~((d >= lo) & (d <= hi)))
    assert bad.size == 0, (r["layer"], r["m"], r["bm"], f"{len(bad)} of {d.size} outside",
                           [(int(rows[i]), int(j), float(lo[i, j]), float(d[i, j]), float(hi[i, j])) for i, j in bad[:4]])
    return int((lo == hi).sum()), int(d.size), int((d == rne16(np.maximum(V, 0) if relu else V, fmt)).sum())


# one size per conv_bf16 row tile and crop: every conv of the network at 80 x 5 and 160 x 1 (all on the 64-row tile), and the
# layers that take the 128-row tile at 80 x 32 and 160 x 7
LAYER_SIZES = [(80, 5), (80, 32), (160, 1), (160, 7)]


@pytest.mark.parametrize("p", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("S,n", LAYER_SIZES, ids=[f"{s}x{n}" for s, n in LAYER_SIZES])
def test_reduced_precision_layers_within_bound(S, n, p, engines, pools, blob):
    eng = engines[p]
    T = truely_amd.weights.unpack_tensors(blob)
    x = torch.from_numpy(pools[S][:n])
    eng.facenet_embed(x)
    plan = eng.facenet_plan()
    only128 = (S, n) in ((80, 32), (160, 7))
    rng = np.random.default_rng(S * 100 + n + p)
    single = total = at_rne = 0
    tiles = set()
    for r in plan:
        if r["family"] != "conv_bf16" or (only128 and r["bm"] != 128):
            continue
        eng.facenet_capture(r["conv"])
        eng.facenet_embed(x)
        cap = eng.facenet_captured()
        assert cap[0].dtype == np.uint16 and cap[2].dtype == np.uint16 and (cap[1] is not None) == bool(r["has_res"])
        s1, t1, e1 = _check_layer(r, cap, T, p, rng)
        single, total, at_rne = single + s1, total + t1, at_rne + e1
        tiles.add(_key(r))
    assert total > 0 and (not only128 or {t[1] for t in tiles} == {128})
    print(f"{PREC[p]} {S}x{n}: {total} elements checked, single-valued interval {single / total:.5f}, "
          f"equal to RNE16(v) {at_rne / total:.5f}, paths {sorted(tiles)}")
    # Not vacuous: the device value is RNE16 of the exact value almost everywhere, and most intervals hold one 16-bit value (the
    # bound is a worst case over the hardware's summation order, so fp16's narrower ulp leaves more two-valued intervals)
    assert at_rne >= 0.999 * total, (single, total, at_rne)
    assert single >= (0.95 if p == 1 else 0.8) * total, (single, total, at_rne)


@pytest.mark.parametrize("p", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("S,n", [(80, 6), (160, 3)])
def test_reduced_precision_conversions_and_pools_exact(S, n, p, engines, pools):
    """to_bf16 after the f32 stem, the 16-bit max pools (conv2d_3b's input, the pool slices of mixed_6a / mixed_7a inside the
    inputs of block17[0] / block8[0]) and the 16-bit average pool in front of last_linear, bit for bit."""
    eng = engines[p]
    x = torch.from_numpy(pools[S][:n])
    eng.facenet_embed(x)
    at = {r["layer"][len("facenet."):]: r["conv"] for r in eng.facenet_plan()}

    def cap(layer):
        eng.facenet_capture(at[layer])
        eng.facenet_embed(x)
        return eng.facenet_captured()

    def maxpool(v):                                                     # 3x3 / 2, floor mode
        N, H, W, C = v.shape
        OH, OW = (H - 3) // 2 + 1, (W - 3) // 2 + 1
        out = np.full((N, OH, OW, C), -np.inf)
        for dy in range(3):
            for dx in range(3):
                out = np.maximum(out, v[:, dy:dy + 2 * OH - 1:2, dx:dx + 2 * OW - 1:2, :])
        return out

    stem = cap("conv2d_1a")[2]
    assert stem.dtype == np.float32
    assert np.array_equal(cap("conv2d_2a")[0], to_bits(rne16(stem.astype(np.float64), p), p))
    for src, dst, c0 in (("conv2d_2b", "conv2d_3b", 0), ("repeat_1.4.conv2d", "repeat_2.0.fused", 640),
                         ("repeat_2.9.conv2d", "repeat_3.0.fused", 896)):
        before = from_bits(cap(src)[2], p)
        got = cap(dst)[0][..., c0:]
        assert np.array_equal(got, to_bits(maxpool(before), p)), (src, dst)
    last = cap("block8.conv2d")[2]
    g = cap("last_linear")[0]
    assert g.dtype == np.float32
    v = from_bits(last, p).astype(np.float32).reshape(n, -1, last.shape[-1])
    s = np.zeros((n, last.shape[-1]), np.float32)
    for i in range(v.shape[1]):                                         # float32, pixel order, then / HW
        s = s + v[:, i]
    assert np.array_equal(g.reshape(n, -1), s / np.float32(v.shape[1]))


def test_capture_of_f32_layers_and_unarmed_calls(engines, pools):
    """Captures work on the f32 path too (block35_grouped's scattered destination included); an armed call computes what an unarmed
    one does, and an unarmed call leaves the captured views alone."""
    eng = engines[0]
    x = torch.from_numpy(pools[80][:9])
    base = eng.facenet_embed(x).cpu().numpy()
    at = {r["layer"][len("facenet."):]: r["conv"] for r in eng.facenet_plan()}
    eng.facenet_capture(at["repeat_1.0.fused"])
    assert np.array_equal(eng.facenet_embed(x).cpu().numpy(), base)
    fused_in, res, fused_out = eng.facenet_captured()
    assert res is None and fused_out.dtype == np.float32 and fused_out.shape == (9, 7, 7, 96) and fused_in.shape == (9, 7, 7, 256)
    eng.facenet_capture(at["repeat_1.0.conv2d"])
    eng.facenet_embed(x)
    cat_in, res, out = eng.facenet_captured()
    assert np.array_equal(res, fused_in) and out.shape == (9, 7, 7, 256)
    assert np.array_equal(cat_in[..., :32], fused_out[..., :32])         # branch0 reaches the up-projection untouched
    eng.facenet_embed(x)                                                # unarmed
    assert np.array_equal(eng.facenet_captured()[0], cat_in)


# ---- fp16 overflow --------------------------------------------------------------------------------------------------------------

def test_fp16_overflow_gives_a_non_finite_embedding(engines, pools):
    """One face's pixels x 1e6: the f32 stem's output exceeds 65504, so conv2d_2a's fp16 input holds +inf.  That face's embedding
    must come out non-finite (NaN through the 16-bit ReLU / max pool, not a finite wrong vector); the other faces keep their bits."""
    eng = engines[2]
    x = pools[80][:7].copy()
    base = _embed(eng, x)
    assert np.isfinite(base).all()
    x[3] *= 1e6
    eng.facenet_capture(1)                                              # conv2d_2a: its input is the first fp16 tensor
    got = _embed(eng, x)
    xin = from_bits(eng.facenet_captured()[0], 2)
    assert np.isinf(xin[3]).any() and np.isfinite(np.delete(xin, 3, axis=0)).all()
    assert not np.isfinite(got[3]).all(), got[3][:8]
    others = [i for i in range(7) if i != 3]
    assert np.array_equal(got[others], base[others])


def test_fp16_weight_outside_range_is_refused(blob):
    from truely_amd._lib import TrlError
    from truely_amd.engine import Engine
    T = {k: np.array(v) for k, v in truely_amd.weights.unpack_tensors(blob).items()}
    name = "facenet.repeat_2.3.branch1.1.w"
    T[name][5, 7] = 7e4
    with pytest.raises(TrlError) as e:
        Engine(truely_amd.weights.pack_tensors(T), embed_precision="fp16")
    assert e.value.status == -3 and name in str(e.value)
    Engine(truely_amd.weights.pack_tensors(T), embed_precision="bf16").close()   # bf16 has the range
    T[name][5, 7] = 65519.0                                             # rounds to 65504: accepted
    Engine(truely_amd.weights.pack_tensors(T), embed_precision="fp16").close()


def test_second_load_into_one_context_with_16bit_copies(blob):
    """trl_load_weights twice on one bf16 context: the first load's weights and 16-bit copies are freed, the second load's serve
    the same bits, and the context closes (every copy freed once)."""
    from truely_amd import _lib
    from truely_amd.engine import Engine
    eng = Engine(blob, embed_precision="bf16")
    faces = torch.from_numpy(np.random.default_rng(21).uniform(-1, 1, (2, 80, 80, 3)).astype(np.float32))
    first = eng.facenet_embed(faces).cpu().numpy()
    _lib.check(eng.lib.trl_load_weights(eng._h, blob, len(blob)))
    again = eng.facenet_embed(faces).cpu().numpy()
    assert np.isfinite(first).all() and np.array_equal(first, again)
    assert all(r["precision"] == 1 for r in eng.facenet_plan()[1:-1])
    eng.close()
    assert eng._h is None
