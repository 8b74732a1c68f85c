"""The embedder at every map geometry its API accepts: square and non-square faces of 75 px and up (trl_facenet_embed's only shape
check is h, w >= 75), where test_gpu_embedder.py covers the 80 and 160 px crops only.  facenet_geometry() gives every conv's
output map; the face counts of each geometry sit on both sides of every threshold of the dispatch on M = faces x OH x OW, derived
from the code below (_thresholds) for that geometry.

- f32: every row of every case is finite and has the bits of the same face embedded in a call of at most 8 faces; the first and
  last rows, the faces owning the last M-tile of the largest-M layer and of every four-chain layer have the oracle's bits.
- plan: every row's m is faces x OH x OW; a row is four-chain iff the oracle's rule holds for its map and K; every path is known
  (EXPECTED_PATHS of test_gpu_embedder.py, or SIZE_PATHS below); the paths only these geometries reach are reached.
- bf16 / fp16 at 112 x 112 and 139 x 107: every conv_bf16 layer within the float64 interval bound, the 16-bit conversion, max
  pools and average pool exact, end to end within the existing bars.
- the drop-in API: InceptionResnetV1 on a non-square batch, resnet(MTCNN(image_size=S)(img)), the smallest sizes accepted and
  the next smaller refused.

Each call's budget, faces x (h x w x 110 + 400000) x 4 bytes (workspace() below: the rule by which cases are chosen, not what a
call reserves), stays within that of the largest case of test_gpu_embedder.py (2,048 faces of 80 px).  That cap puts these
thresholds out of reach (faces needed; OUT_OF_REACH, checked against
_thresholds):
  75 x 75            block8, mixed_7a's stride-2 convs and last_linear (1 x 1 maps): the four-chain tile past M = 4,096 (4,097),
                     leaving the small-map family (16,385)
  112 x 112          block8 (2 x 2) leaving the small-map family (4,097); on 2 x 2 maps it does so only past 4,096 faces
  139 x 107          block8 (3 x 2) leaving the small-map family (2,731)
  80 x 112, 112 x 80 block8 (1 x 2, 2 x 1): its tiles past M = 4,096 (2,049), leaving the small-map family (8,193)
  80 x 362           block8 (1 x 9) leaving the small-map family (1,821)
  80 x 363           block8 (1 x 10) leaving the small-map family (1,639)
  224 x 224          last_linear's four-chain tile past M = 512 (513), block8 (5 x 5) leaving the small-map family (656)
  150 x 150          block8 (3 x 3) leaving the small-map family (1,821)
  171 x 171          block8 (4 x 4) leaving the small-map family (1,025)
  all of them        last_linear (M = faces) past M = 4,096 (4,097) and leaving the small-map family (16,385)
Inputs whose activations exceed 2^31 elements -- where conv_igemm_vec and conv_splitk4 would be selected, some 120 GB of
workspace -- are out of scope."""
import numpy as np
import pytest
import torch

import truely_amd
from test_embedder_bound_cpu import from_bits, rne16, to_bits
from test_facenet_sizes_cpu import facenet_geometry, four_chain
from test_gpu_embedder import EXPECTED_PATHS, PREC, _check_layer, _key

pytestmark = pytest.mark.gpu


def workspace(h, w, n):
    """The budget rule by which cases are chosen: n faces of h x w count as n x (h x w x 110 + 400000) x 4 bytes.  (What a call
    reserves is the dry-run count of its walk: Engine.workspace, tests/test_gpu_workspace.py.)"""
    return n * (h * w * 110 + 400000) * 4


CAP = workspace(80, 80, 2048)                          # test_gpu_embedder.py's largest case


def max_faces(h, w):
    return CAP // workspace(h, w, 1)


FOUR = ("fn_conv_split4", "conv_splitk4", "conv_splitk4_tap")


def _fn_eligible(c):
    """trl_fn_eligible for f32 layer c below M <= 16384: whole-tap chunks of 32 channels; a four-chain layer's quarters must be
    whole chunks, except on 1 x 1 maps with a padded 1 x 3 / 3 x 1 filter (only the centre tap is live)."""
    if c.cin % 32:
        return False
    if four_chain(c.OH, c.OW, c.K) and (c.K // 4) % 32:
        return c.OH * c.OW == 1 and c.pad
    return True


def _thresholds(h, w, lowp=False):
    """{n: reasons}: for each reason, some layer's kernel or tile at n faces differs from that at n + 1.  Restated from the
    dispatch: trl_run_facenet (block35_grouped while faces x block35 map <= 16384), trl_fn_eligible (M <= 16384), pick_tile
    (four-chain: M <= 512, M <= 4096; single chain: M <= 4096 with N >= 512, N of a group's convs summed), trl_launch_conv's
    launch_cfg tiers (M >= 1024, M >= 16384) for layers outside the small-map family, trl_launch_conv_bf16 (M >= 8192)."""
    geo = facenet_geometry(h, w)
    out = {}

    def at(n, why):
        if n >= 1:
            out.setdefault(n, []).append(why)

    def name(c):
        return f"{c.layer[len('facenet.'):]} {c.OH}x{c.OW}"

    if lowp:                                           # conv_bf16 takes every layer but the f32 stem and last_linear
        for c in geo[1:-1]:
            at((8192 - 1) // (c.OH * c.OW), "conv_bf16 128-row tile: " + name(c))
        return out
    b35 = geo[6]
    at(16384 // (b35.OH * b35.OW), "block35_grouped / block35")
    for c in geo[1:]:
        per = c.OH * c.OW
        four = four_chain(c.OH, c.OW, c.K)
        if _fn_eligible(c):
            at(16384 // per, "small-map family: " + name(c))
            if four:
                at(512 // per, "four-chain tile, M <= 512: " + name(c))
                at(4096 // per, "four-chain tile, M <= 4096: " + name(c))
            elif c.cout >= 512:
                at(4096 // per, "64 x 64 tile: " + name(c))
        elif not four and c.cout > 32:
            at((1024 - 1) // per, "launch_cfg M >= 1024: " + name(c))
            at((16384 - 1) // per, "launch_cfg M >= 16384: " + name(c))
    g = {c.layer[len("facenet.mixed_7a."):]: c for c in geo if c.layer.startswith("facenet.mixed_7a.branch")}
    if not four_chain(g["branch0.1"].OH, g["branch0.1"].OW, g["branch0.1"].K):   # the group of three, single chain, N = 896
        at(4096 // (g["branch2.1"].OH * g["branch2.1"].OW), "mixed_7a group 64 x 64 tile")
    return out


F32_GEOMETRIES = [(75, 75), (112, 112), (139, 107), (80, 112), (112, 80), (80, 362), (80, 363), (224, 224), (150, 150), (171, 171)]


def _counts(h, w):
    """Both sides of every threshold within the workspace cap, and one face."""
    cap = max_faces(h, w)
    return sorted({1} | {m for n in _thresholds(h, w) if n + 1 <= cap for m in (n, n + 1)})


# (h, w, faces, precision, no_fnconv).  f32: both sides of every threshold of _thresholds(h, w) within the cap -- for example at
# 112 x 112 (block35 11 x 11, block17 5 x 5, block8 2 x 2): block35_grouped at 135 / 136, block17 leaving the small-map family at
# 655 / 656, its 64 x 64 tiles at 163 / 164, block8's four-chain tiles at 128 / 129 and 1024 / 1025, last_linear's at 512 / 513.
# no_fnconv: every layer on the generic kernels (block35, conv_splitk4_tap for every four-chain layer).  bf16 / fp16: the
# conv_bf16 128-row tile of conv2d_2a / 2b at 2 / 3 faces, of the block35 maps at 67 / 68 (112) and 49 / 50 (139 x 107).
CASES = [(h, w, n, 0, False) for h, w in F32_GEOMETRIES for n in _counts(h, w)]
CASES += [(112, 112, 5, 0, True), (112, 112, 129, 0, True), (139, 107, 3, 0, True), (80, 112, 7, 0, True), (112, 80, 7, 0, True),
          (80, 362, 9, 0, True), (80, 363, 9, 0, True), (224, 224, 3, 0, True)]
CASES += [(h, w, n, p, False) for h, w, ns in ((112, 112, (2, 3, 67, 68)), (139, 107, (2, 3, 49, 50))) for n in ns for p in (1, 2)]

# Paths these geometries reach beyond EXPECTED_PATHS (the dispatch at 80 and 160 px): none.  The padded four-chain convs on 2 x 2,
# 1 x N and N x 1 maps take conv_splitk4_tap BK 16 with padding, which no_fnconv already reaches at 80 px.  A path that appears
# here must be listed with the case that reaches it; test_f32_rows_are_batch_independent_and_exact bit-checks it there.
SIZE_PATHS = set()


@pytest.fixture(scope="module")
def pools():
    """Per geometry, as many faces as its largest case: uniform in [0, 1)."""
    need = {}
    for h, w, n, _, _ in CASES:
        need[(h, w)] = max(need.get((h, w), 0), n)
    return {g: np.random.default_rng(g[0] * 1000 + g[1]).uniform(0, 1, (n, g[0], g[1], 3)).astype(np.float32) for g, n in need.items()}


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
    eng = engines[0]
    return {g: np.concatenate([_embed(eng, x[i:i + 8]) for i in range(0, len(x), 8)]) for g, x in pools.items()}


@pytest.fixture(scope="module")
def case_runs(engines, pools):
    out = {}
    for case in CASES:
        h, w, n, p, nofn = case
        assert workspace(h, w, n) <= CAP, case
        eng = engines[p]
        if nofn:
            eng.option("no_fnconv", 1)
        try:
            emb = _embed(eng, pools[(h, w)][:n])
            out[case] = (emb, eng.facenet_plan())
        finally:
            if nofn:
                eng.option("no_fnconv", 0)
    return out


OUT_OF_REACH = {(75, 75): [4097, 16385], (112, 112): [4097, 16385], (139, 107): [2731, 4097, 16385],
                (80, 112): [2049, 4097, 8193, 16385], (112, 80): [2049, 4097, 8193, 16385], (80, 362): [1821, 4097, 16385],
                (80, 363): [1639, 4097, 16385], (224, 224): [513, 656, 4097, 16385], (150, 150): [1821, 4097, 16385],
                (171, 171): [1025, 4097, 16385]}


def test_out_of_reach_thresholds_are_the_documented_ones():
    """The thresholds the workspace cap leaves out are those the module docstring lists (faces needed)."""
    for g in F32_GEOMETRIES:
        assert sorted(n + 1 for n in _thresholds(*g) if n + 1 > max_faces(*g)) == OUT_OF_REACH[g], g
    for g, first, b35 in (((112, 112), 2, 67), ((139, 107), 2, 49)):       # the bf16 / fp16 counts of CASES
        T = _thresholds(*g, lowp=True)
        assert any("conv2d_2a" in y for y in T[first]) and any("repeat_1.0.fused" in y for y in T[b35]), g
        assert {(n, p) for h, w, n, p, _ in CASES if (h, w) == g and p} == {(n, p) for n in (first, first + 1, b35, b35 + 1) for p in (1, 2)}


def test_plan_rows_have_the_geometry(case_runs):
    """Every row's m is faces x OH x OW of its conv; a f32 row is four-chain iff the oracle's rule holds for its map and K."""
    for (h, w, n, p, nofn), (_, plan) in case_runs.items():
        geo = facenet_geometry(h, w)
        assert [r["layer"] for r in plan] == [c.layer for c in geo], (h, w, n)
        for r, c in zip(plan, geo):
            assert r["m"] == n * c.OH * c.OW and r["k"] == c.K and r["cout"] == c.cout, (h, w, n, r, c)
            if r["precision"] == 0:
                assert (r["family"] in FOUR) == four_chain(c.OH, c.OW, c.K), (h, w, n, r, c)
            if nofn:
                assert not r["family"].startswith("fn_"), r


def test_plan_paths_are_known_and_size_paths_reached(case_runs):
    seen = set()
    for _, plan in case_runs.values():
        seen |= {_key(r) for r in plan}
    assert seen <= EXPECTED_PATHS | SIZE_PATHS, sorted(seen - EXPECTED_PATHS - SIZE_PATHS)
    assert SIZE_PATHS <= seen, sorted(SIZE_PATHS - seen)


def _rows_of(case_runs, pred):
    """(case, plan row, geometry row) of every f32 row satisfying pred(row, conv)."""
    out = []
    for case, (_, plan) in case_runs.items():
        if case[3] == 0:
            out += [(case, r, c) for r, c in zip(plan, facenet_geometry(case[0], case[1])) if pred(r, c)]
    return out


def test_plan_reaches_the_geometry_only_paths(case_runs):
    # a padded four-chain launch on a 2 x 2 map (block8's 1 x 3 / 3 x 1 at 112 px: K / 4 = 144 is no whole chunk)
    assert _rows_of(case_runs, lambda r, c: r["family"] in FOUR and r["pad"] and (c.OH, c.OW) == (2, 2))
    # padded 1 x 3 / 3 x 1 convs on a 1 x N map and an N x 1 map, N > 1
    for shape in (lambda c: c.OH == 1 and c.OW > 1, lambda c: c.OW == 1 and c.OH > 1):
        hits = _rows_of(case_runs, lambda r, c: r["pad"] and ".branch1." in r["layer"] and r["k"] == 576 and shape(c))
        assert {r["layer"].rsplit(".", 1)[1] for _, r, _ in hits} == {"1", "2"}
    # a 1 x 9 four-chain layer next to a 1 x 10 single-chain one
    assert _rows_of(case_runs, lambda r, c: (c.OH, c.OW) == (1, 9) and r["family"] in FOUR and r["layer"] == "facenet.block8.fused")
    assert _rows_of(case_runs, lambda r, c: (c.OH, c.OW) == (1, 10) and r["family"] not in FOUR and r["layer"] == "facenet.block8.fused")
    # block35_grouped (its 3x3 pair in one launch) and block35 at geometries other than 80 and 160
    grouped = {(case[0], case[1], r["nz"]) for case, r, _ in _rows_of(case_runs, lambda r, c: r["layer"] == "facenet.repeat_1.0.branch2.1")}
    for g in ((112, 112), (139, 107), (224, 224)):
        assert (g + (2,)) in grouped and (g + (1,)) in grouped, g
    # gap_kernel over a non-square map: some f32 case ends on one (its rows are bit-checked)
    assert any(case[3] == 0 and c.OH != c.OW for case, _, c in _rows_of(case_runs, lambda r, c: r["layer"] == "facenet.block8.conv2d"))


@pytest.mark.parametrize("case", [c for c in CASES if c[3] == 0], ids=str)
def test_f32_rows_are_batch_independent_and_exact(case, case_runs, small_calls, pools, oracle):
    h, w, n, _, _ = case
    emb, plan = case_runs[case]
    assert np.isfinite(emb).all()
    ref = small_calls[(h, w)][:n]
    bad = np.nonzero((emb != ref).any(1))[0]
    assert bad.size == 0, f"{bad.size} rows differ from <= 8-face calls, first {bad[:8]}"
    # the oracle: first and last rows, the faces owning the last M-tile of the largest-M layer and of every four-chain layer
    idx = {0, n - 1}
    for r in [max(plan, key=lambda r: r["m"])] + [r for r in plan if r["family"] in FOUR]:
        per = r["m"] // n
        idx |= set(range((r["m"] - 1) // r["bm"] * r["bm"] // per, n))
    idx = sorted(idx)
    assert np.array_equal(emb[idx], oracle.facenet(pools[(h, w)][idx])), idx


@pytest.mark.parametrize("case", [c for c in CASES if c[3] > 0], ids=str)
def test_reduced_precision_cases_close_to_oracle(case, case_runs, pools, oracle):
    """End to end, with the existing bars (bf16: cos >= 0.999, |diff| <= 3e-2; fp16: 0.99999, 3e-3)."""
    h, w, n, p, _ = case
    emb = case_runs[case][0]
    assert np.isfinite(emb).all()
    idx = np.unique(np.linspace(0, n - 1, min(n, 24)).astype(int))
    ref = oracle.facenet(pools[(h, w)][idx])
    cos = (emb[idx] * ref).sum(1)
    assert cos.min() >= (0.999 if p == 1 else 0.99999) and np.abs(emb[idx] - ref).max() <= (3e-2 if p == 1 else 3e-3)


# every conv_bf16 layer at 2 faces (64-row tiles only), the 128-row layers at 3 faces (conv2d_2a / 2b)
LAYER_SIZES = [(112, 112, 2), (112, 112, 3), (139, 107, 2), (139, 107, 3)]


@pytest.mark.parametrize("p", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("h,w,n", LAYER_SIZES, ids=[f"{h}x{w}x{n}" for h, w, n in LAYER_SIZES])
def test_reduced_precision_layers_within_bound(h, w, n, p, engines, pools, blob):
    eng = engines[p]
    T = truely_amd.weights.unpack_tensors(blob)
    x = torch.from_numpy(pools[(h, w)][:n])
    eng.facenet_embed(x)
    plan = eng.facenet_plan()
    only128 = n == 3
    rng = np.random.default_rng(h * 1000 + w + n + p)
    single = total = at_rne = 0
    tiles = set()
    for r in plan:
        if r["family"] != "conv_bf16" or (only128 and r["bm"] != 128):
            continue
        eng.facenet_capture(r["conv"])
        eng.facenet_embed(x)
        s1, t1, e1 = _check_layer(r, eng.facenet_captured(), T, p, rng)
        single, total, at_rne = single + s1, total + t1, at_rne + e1
        tiles.add(_key(r))
    assert total > 0 and {t[1] for t in tiles} == ({128} if only128 else {64})
    assert at_rne >= 0.999 * total, (single, total, at_rne)
    assert single >= (0.95 if p == 1 else 0.8) * total, (single, total, at_rne)


def _maxpool(v):                                                        # 3x3 / 2, floor mode, any H and W
    N, H, W, C = v.shape
    OH, OW = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    out = np.full((N, OH, OW, C), -np.inf)
    for dy in range(3):
        for dx in range(3):
            out = np.maximum(out, v[:, dy:dy + 2 * OH - 1:2, dx:dx + 2 * OW - 1:2, :])
    return out


@pytest.mark.parametrize("p", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("h,w,n", [(112, 112, 3), (139, 107, 2), (80, 363, 2)], ids=str)
def test_reduced_precision_conversions_and_pools_exact(h, w, n, p, engines, pools):
    """to-16-bit after the f32 stem, the three 16-bit max pools (odd and even maps, H != W) and the 16-bit average pool over a
    non-square map, bit for bit."""
    eng = engines[p]
    x = torch.from_numpy(pools[(h, w)][:n])
    eng.facenet_embed(x)
    at = {r["layer"][len("facenet."):]: r["conv"] for r in eng.facenet_plan()}

    def cap(layer):
        eng.facenet_capture(at[layer])
        eng.facenet_embed(x)
        return eng.facenet_captured()

    stem = cap("conv2d_1a")[2]
    assert stem.dtype == np.float32
    assert np.array_equal(cap("conv2d_2a")[0], to_bits(rne16(stem.astype(np.float64), p), p))
    for src, dst, c0 in (("conv2d_2b", "conv2d_3b", 0), ("repeat_1.4.conv2d", "repeat_2.0.fused", 640),
                         ("repeat_2.9.conv2d", "repeat_3.0.fused", 896)):
        before = from_bits(cap(src)[2], p)
        got = cap(dst)[0][..., c0:]
        assert np.array_equal(got, to_bits(_maxpool(before), p)), (src, dst)
    last = cap("block8.conv2d")[2]
    assert last.shape[1:3] == next((c.OH, c.OW) for c in facenet_geometry(h, w) if c.layer == "facenet.block8.conv2d")
    g = cap("last_linear")[0]
    assert g.dtype == np.float32
    v = from_bits(last, p).astype(np.float32).reshape(n, -1, last.shape[-1])
    s = np.zeros((n, last.shape[-1]), np.float32)
    for i in range(v.shape[1]):                                         # float32, pixel order, then / HW
        s = s + v[:, i]
    assert np.array_equal(g.reshape(n, -1), s / np.float32(v.shape[1]))


# ---- the drop-in API ----------------------------------------------------------------------------------------------------------

def test_inception_resnet_non_square_batch(engine, oracle):
    from truely_amd.inception_resnet_v1 import InceptionResnetV1
    net = InceptionResnetV1(pretrained="vggface2", engine=engine).eval()
    x = torch.rand(3, 3, 80, 112, generator=torch.Generator().manual_seed(5))
    y = net(x)
    assert y.shape == (3, 512)
    assert np.array_equal(y.numpy(), oracle.facenet(x.permute(0, 2, 3, 1).contiguous().numpy()))


@pytest.mark.parametrize("S", [112, 150])
def test_resnet_of_mtcnn_at_image_size(S, engine, oracle):
    import extract_ref as R
    from test_gpu_extract import _multiface
    from truely_amd.inception_resnet_v1 import InceptionResnetV1
    from truely_amd.mtcnn import MTCNN
    fr = _multiface()[0]
    m = MTCNN(engine=engine, image_size=S)
    b, p = m.detect(fr[None])
    ref = R.forward(fr, b[0], p[0], S=S, resample="torch")
    face = m(torch.from_numpy(fr))
    assert tuple(face.shape) == (3, S, S) and np.array_equal(face.numpy(), ref)
    emb = InceptionResnetV1(engine=engine)(face.unsqueeze(0))
    assert np.array_equal(emb.numpy(), oracle.facenet(ref.transpose(1, 2, 0)[None].copy()))


def test_smallest_sizes_accepted_and_smaller_refused(engine, oracle):
    from truely_amd._lib import TrlError
    rng = np.random.default_rng(75)
    for h, w in ((75, 75), (75, 300), (300, 75)):
        x = rng.uniform(0, 1, (2, h, w, 3)).astype(np.float32)
        assert np.array_equal(_embed(engine, x), oracle.facenet(x)), (h, w)
    for h, w in ((74, 80), (80, 74)):
        with pytest.raises(TrlError) as e:
            engine.facenet_embed(torch.zeros(1, h, w, 3))
        assert e.value.status == -1, (h, w)
