"""Stages 2 and 3 of the detector (R-Net / O-Net) per candidate, at the launch capacities the product uses.

Each stage is trl_stage_net: chunks of rnet_chunk / onet_chunk candidate slots, each one k_mtcnn_front launch (crop, area
resample, conv1, PReLU, pool) and a tail of generic layer kernels (trl_run_net from the descriptor's tail layer).  Two things make the
tail unusual: the kernel and tile of every conv are chosen from the CAPACITY (M = chunk slots x OH x OW, trl_launch_conv /
launch_cfg), because the live count exists only on the device; and every kernel skips the dead rows itself (trl_live_rows in the
conv kernels, the clamped N of maxpool_kernel's grid-stride loop).

`conv_path` below restates that dispatch for the tail's layer shapes.  The cases sit on both sides of every threshold it has, at
the production capacities, in small chunks whose count ends mid-chunk, and at live counts that end just before, at and just
after a row-tile boundary.  trl_debug_stage_net runs the production loop on them and trl_debug_mtcnn_plan records what each
launch chose.  Checks: the plan equals the restatement row by row; the plans reach every path the restatement can produce; every
live row has the bits of the same (frame, box) pair run in a call of at most 8 candidates, and those rows have the oracle's bits;
tiles past the live rows write nothing; the largest cases give the same bits over a poisoned workspace."""
import functools

import numpy as np
import pytest

import truely_amd
from test_gpu_parity import _slope_variant_blob, _softmax_p1

P = 389                      # unique (frame, box) pairs, a prime: candidate i of a case uses pair (i + shift) % P
NF, H, W = 4, 360, 640
SENTINEL = np.float32(-12345.678)   # what the output held before the call: tiles past the live rows must leave it
CAP_MAX = 49152              # the default R-Net chunk, and the largest per-launch capacity

# (layer, input side, Cin, kernel, Cout) of the two tails' convs, in launch order (trl_nets[] in csrc/trl_nets.hip, from each net's tail layer)
TAIL = {
    24: [("rnet.conv2", 11, 28, 3, 48), ("rnet.conv3", 4, 48, 2, 64), ("rnet.dense4", 3, 64, 3, 128), ("rnet.heads", 1, 128, 1, 6)],
    48: [("onet.conv2", 23, 32, 3, 64), ("onet.conv3", 10, 64, 3, 64), ("onet.conv4", 4, 64, 2, 128),
         ("onet.dense5", 3, 128, 3, 256), ("onet.heads", 1, 256, 1, 16)],
}
POOLS = {24: [(9, 48, 3, 2)], 48: [(21, 64, 3, 2), (8, 64, 2, 2)]}   # (input side, C, k, stride), ceil mode
CHUNK = {24: 49152, 48: 16384}                                      # trl_ctx defaults


def conv_path(N, side, Cin, k, Cout):
    """(family, bm, bn, bk, pad) trl_launch_conv picks for a valid-padding MTCNN conv over N items of side x side x Cin, with a
    device-sized batch (m_dev set: the small-map family never takes it) and the 256-byte aligned scratch (float4 loads)."""
    OH = side - k + 1
    K, ldw, M = k * k * Cin, (Cout + 31) // 32 * 32, N * OH * OH
    vec = Cin % 4 == 0
    small = N * side * side * Cin < 0x7FFFFFFF and K * ldw < 0x7FFFFFFF
    if OH * OH <= 9 and K >= 512 and K % 16 == 0:                 # the oracle's four-chain rule
        seg = K >> 2
        if small and Cin % 32 == 0 and seg % 32 == 0:
            return ("conv_splitk4_tap", 32, 64, 32, 0)
        if small and Cin % 16 == 0 and seg % 16 == 0:
            return ("conv_splitk4_tap", 32, 64, 16, 0)
        return ("conv_splitk4", 32, 64, 32, 0)
    deep = K >= 192
    if vec and small and Cout == 48 and ldw >= 48 and M >= 16384 and (Cin % 28 == 0 or Cin % 32 == 0):
        return ("conv_tap48", 128, 48, 32 if Cin % 32 == 0 else 28, 0)
    if Cout <= 32:
        bm, bn, bk = 128, 32, 64 if deep else 16
    elif M >= 16384:
        bm, bn, bk = 128, 64, 32 if deep else 16
    elif M >= 1024:
        bm, bn, bk = 64, 64, 64 if deep else 16
    else:
        bm, bn, bk = 32, 128, 64 if deep else 16
    # launch_cfg: whole-tap chunks when the channel count allows
    if vec and small:
        if bk >= 64 and Cin % 64 == 0:
            return ("conv_tap", bm, bn, 64, 0)
        if Cin % 32 == 0:
            return ("conv_tap", bm, bn, 32, 0)
        if bm == 128 and bn == 64 and Cin % 28 == 0:
            return ("conv_tap", bm, bn, 28, 0)
        if Cin % 16 == 0:
            return ("conv_tap", bm, bn, 16, 0)
    return ("conv_igemm_vec", bm, bn, bk, 0) if vec else ("conv_igemm_scalar", bm, bn, 16, 0)


def pool_capped(net, nc):
    """Does a max pool of this chunk run on trl_launch_maxpool's capped grid (32,768 blocks, grid-stride)?"""
    for s, c, k, st in POOLS[net]:
        oh = -(-(s - k) // st) + 1                            # trl_pool_out, ceil mode
        items = nc * oh * oh * (c // 4)                       # four channels per thread
        if -(-items // 256) > 32768:
            return True
    return False


def chunks(cap, chunk):
    return [(t0, min(chunk, cap - t0)) for t0 in range(0, cap, chunk)]


def plan_of(net, cap, chunk):
    """The plan rows trl_debug_mtcnn_plan must return for a call at this capacity and chunk."""
    rows = []
    for t0, nc in chunks(cap, chunk):
        for layer, side, cin, k, cout in TAIL[net]:
            fam, bm, bn, bk, pad = conv_path(nc, side, cin, k, cout)
            oh = side - k + 1
            rows.append(dict(conv=len(rows), layer=layer, family=fam, bm=bm, bn=bn, bk=bk, pad=pad, nz=1, m=nc * oh * oh, cout=cout,
                             k=k * k * cin, precision=0, has_res=0))
    return rows


@functools.lru_cache(maxsize=None)
def reachable(net):
    """{layer: {path}} the restatement produces for per-launch capacities 1 .. CAP_MAX, and the capacities where a layer's path
    changes."""
    paths, changes = {}, {}
    for layer, side, cin, k, cout in TAIL[net]:
        seq = [conv_path(n, side, cin, k, cout) for n in range(1, CAP_MAX + 1)]
        paths[layer] = set(seq)
        changes[layer] = tuple(n + 1 for n in range(1, CAP_MAX) if seq[n] != seq[n - 1])
    return paths, changes


# What the restatement gives (test_restatement_table pins it): the per-launch capacity at which each layer's path changes, and
# the path sets.  conv_tap with BK 28 and the plain conv_splitk4 are instantiated, but no shipped network selects them: R-Net's
# conv2 (the only Cin = 28 layer) takes conv_tap48 wherever a 128 x 64 tile would apply, and R-Net's dense4 (K / 4 = 144) fits
# conv_splitk4_tap's 16-channel chunks.
THRESHOLDS = {
    "rnet.conv2": (13, 203), "rnet.conv3": (114, 1821), "rnet.dense4": (), "rnet.heads": (),
    "onet.conv2": (3, 38), "onet.conv3": (16, 256), "onet.conv4": (114, 1821), "onet.dense5": (), "onet.heads": (),
}
POOL_CAP = {24: 43691, 48: 5243}    # first chunk size whose pool runs on the capped grid
EXPECTED_PATHS = {
    "rnet.conv2": {("conv_igemm_vec", 32, 128, 64, 0), ("conv_igemm_vec", 64, 64, 64, 0), ("conv_tap48", 128, 48, 28, 0)},
    "rnet.conv3": {("conv_tap", 32, 128, 16, 0), ("conv_tap", 64, 64, 16, 0), ("conv_tap", 128, 64, 16, 0)},
    "rnet.dense4": {("conv_splitk4_tap", 32, 64, 16, 0)},
    "rnet.heads": {("conv_tap", 128, 32, 32, 0)},
    "onet.conv2": {("conv_tap", 32, 128, 32, 0), ("conv_tap", 64, 64, 32, 0), ("conv_tap", 128, 64, 32, 0)},
    "onet.conv3": {("conv_tap", 32, 128, 64, 0), ("conv_tap", 64, 64, 64, 0), ("conv_tap", 128, 64, 32, 0)},
    "onet.conv4": {("conv_tap", 32, 128, 64, 0), ("conv_tap", 64, 64, 64, 0), ("conv_tap", 128, 64, 32, 0)},
    "onet.dense5": {("conv_splitk4_tap", 32, 64, 32, 0)},
    "onet.heads": {("conv_tap", 128, 32, 64, 0)},
}


def _expected_paths(net):
    return {l: p for l, p in EXPECTED_PATHS.items() if l.startswith("rnet" if net == 24 else "onet")}


# production capacities (candidates per frame x frames + 64): configs[1] (256 frames) and configs[0] (240 frames)
PROD = {24: (41024, 38464), 48: (12352, 11584)}


def _boundary_counts(net, cap):
    """Live counts <= cap at which the live rows (count x OH x OW) of some tail layer end one row before, at, or one row after
    a multiple of that layer's row tile BM at this capacity (where the residue is reachable: 64-pixel maps only meet BM at a
    candidate boundary)."""
    out = set()
    for layer, side, cin, k, cout in TAIL[net]:
        bm = conv_path(cap, side, cin, k, cout)[1]
        mper = (side - k + 1) ** 2
        for r in (bm - 1, 0, 1):
            c = next((c for c in range(cap, max(0, cap - 2 * bm), -1) if (c * mper) % bm == r), None)
            if c:
                out.add(c)
    return out


def _cases(net):
    """(capacity, chunk, live count) triples."""
    ch = CHUNK[net]
    cases = set()
    for layer, cuts in THRESHOLDS.items():                   # both sides of every threshold, one chunk, all live
        if layer.startswith("rnet" if net == 24 else "onet"):
            for x in cuts:
                cases |= {(x - 1, ch, x - 1), (x, ch, x)}
    cases |= {(POOL_CAP[net] - 1, ch, POOL_CAP[net] - 1), (POOL_CAP[net], ch, POOL_CAP[net])}
    for cap in PROD[net]:                                    # production capacities at realistic, full, empty and overfull counts
        cases |= {(cap, ch, int(cap * 0.76)), (cap, ch, cap), (cap, ch, cap - 1), (cap, ch, 0), (cap, ch, 1), (cap, ch, cap + 389)}
    if net == 24:                                            # two chunks: the count ends inside the second, or before it
        cases |= {(60001, ch, 52000), (60001, ch, 30000), (60001, ch, 60001)}
    else:
        cases |= {(20001, ch, 18000), (20001, ch, 9000)}
    for cap, chunk, count in ((1000, 16, 517), (1000, 16, 1000), (1000, 100, 455), (1000, 100, 1003), (2000, 500, 700),
                              (900, 128, 300), (37, 16, 5), (64, 16, 0)):   # t0 > 0, counts ending mid-chunk, dead chunks
        cases.add((cap, chunk, count))
    for cap in ((12, 113, 202, 1820, PROD[24][0]) if net == 24 else (2, 37, 255, 1820, PROD[48][0])):
        cases |= {(cap, ch, c) for c in _boundary_counts(net, cap)}   # tile boundaries of every family
    return sorted(cases)


CASES = {24: _cases(24), 48: _cases(48)}
SLOPE_VARIANTS = ["slopes_above_one", "negative_slopes"]     # front MODE 1 and 0 (the seeded weights take MODE 2)


# ---- the restatement itself (CPU) ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("net", [24, 48])
def test_restatement_table(net):
    """The restatement's thresholds and path sets are the ones written down above (and in the module docstring's reading of
    trl_launch_conv): a change to either shows up here before it reaches the GPU."""
    paths, changes = reachable(net)
    for layer in paths:
        assert changes[layer] == THRESHOLDS[layer], layer
        assert paths[layer] == EXPECTED_PATHS[layer], layer
    assert not pool_capped(net, POOL_CAP[net] - 1) and pool_capped(net, POOL_CAP[net])


@pytest.mark.parametrize("net", [24, 48])
def test_cases_reach_every_path_and_edge(net):
    """The case list straddles every threshold, reaches every path the restatement can produce, runs the capped pool grid with
    live candidates past its first pass, runs chunks with t0 > 0 whose count ends inside them and chunks past the count, and
    counts at 0, 1, capacity - 1, capacity and above."""
    got = {}
    for cap, chunk, count in CASES[net]:
        for r in plan_of(net, cap, chunk):
            got.setdefault(r["layer"], set()).add((r["family"], r["bm"], r["bn"], r["bk"], r["pad"]))
    assert got == _expected_paths(net)
    ncs = {nc for cap, chunk, _ in CASES[net] for _, nc in chunks(cap, chunk)}
    for cuts in (THRESHOLDS[l] for l in THRESHOLDS if l.startswith("rnet" if net == 24 else "onet")):
        for x in cuts:
            assert {x - 1, x} <= ncs
    assert any(pool_capped(net, nc) and count - t0 > POOL_CAP[net]
               for cap, chunk, count in CASES[net] for t0, nc in chunks(cap, chunk))
    assert any(0 < count - t0 < nc for cap, chunk, count in CASES[net] for t0, nc in chunks(cap, chunk) if t0 > 0)
    assert any(count <= t0 for cap, chunk, count in CASES[net] for t0, nc in chunks(cap, chunk))
    caps = {cap for cap, _, _ in CASES[net]}
    assert any(cap > CHUNK[net] for cap in caps) and set(PROD[net]) <= caps
    for cap in PROD[net]:
        counts = {count for c, _, count in CASES[net] if c == cap}
        assert {0, 1, cap - 1, cap} <= counts and max(counts) > cap
    # a live count whose last row is the first row of a tile (the tile holds one live row), for every path where one exists
    for layer, side, cin, k, cout in TAIL[net]:
        mper = (side - k + 1) ** 2
        hit = {conv_path(nc, side, cin, k, cout) for cap, chunk, count in CASES[net] for t0, nc in chunks(cap, chunk)
               if 0 < count - t0 <= nc and ((count - t0) * mper) % conv_path(nc, side, cin, k, cout)[1] == 1}
        for path in EXPECTED_PATHS[layer]:
            top = max(n for n in range(1, CAP_MAX + 1) if conv_path(n, side, cin, k, cout) == path)
            if any((c * mper) % path[1] == 1 for c in range(1, top + 1)):
                assert path in hit, (layer, path)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def frames():
    return truely_amd.synthetic.synthetic_frames(NF, H, W, seed=29)


@pytest.fixture(scope="module")
def pairs():
    """P (frame, x1, y1, x2, y2) records with non-empty pad() windows over NF frames: boxes of every crop path (tiny up-sampled,
    medium, large column-strip, larger than a strip, clipped by each frame edge, 1-pixel) as in test_front_kernel_on_chosen_boxes."""
    rng = np.random.default_rng(389)
    fixed = [[100.2, 80.7, 104.9, 85.1], [10, 10, 11, 11], [200.5, 100.5, 230.5, 130.5], [300, 50, 371.9, 121.9],
             [50.3, 40.2, 250.8, 240.7], [0.4, 0.6, W - 0.1, H - 0.1], [-30.5, -20.5, 80.5, 90.5], [W - 79.8, H - 109.9, W + 60.9, H + 40.3],
             [-100, 100, 20, 220], [W / 2, -200, W / 2 + 10, 40], [1, 1, 3, H - 1], [2, H - 20, W - 2, H - 2], [W - 200.5, H - 150.5, W, H],
             [W - 97, H - 97, W + 5, H + 5]]
    boxes = [b for b in fixed for _ in range(NF)]
    while len(boxes) < 3 * P:
        side = float(rng.choice([3, 6, 15, 40, 75, 110, 160, 260, 420]))
        x, y = rng.uniform(-40, W - 10), rng.uniform(-40, H - 10)
        boxes.append([x, y, x + side * rng.uniform(0.8, 1.2), y + side * rng.uniform(0.8, 1.2)])
    boxes = np.array(boxes, np.float32)
    tb = np.trunc(boxes).astype(np.int32)                                   # pad(): trunc, clamp to [1, W] x [1, H]
    x, y = np.maximum(tb[:, 0], 1), np.maximum(tb[:, 1], 1)
    ex, ey = np.minimum(tb[:, 2], W), np.minimum(tb[:, 3], H)
    boxes = boxes[(ey > y - 1) & (ex > x - 1)][:P]
    assert len(boxes) == P
    rec = np.zeros((P, 5), np.float32)
    rec[:, 0] = np.arange(P) % NF
    rec[:, 1:] = boxes
    return rec


def _crops(oracle, frames, rec, net):
    tb = np.trunc(rec[:, 1:]).astype(np.int32)
    x, y = np.maximum(tb[:, 0], 1), np.maximum(tb[:, 1], 1)
    ex, ey = np.minimum(tb[:, 2], W), np.minimum(tb[:, 3], H)
    return np.stack([oracle.area_resample_norm(frames[int(rec[i, 0])], y[i] - 1, ey[i], x[i] - 1, ex[i], net, net) for i in range(len(rec))])


def _assert_oracle(oracle, out, crops, net):
    if net == 24:
        p, r = oracle.rnet(crops)
    else:
        p, r, pts = oracle.onet(crops)
        assert np.array_equal(out[:, 6:16], pts), "landmarks differ from the oracle"
    assert np.array_equal(out[:, 2:6], r), "regression differs from the oracle"
    assert np.array_equal(_softmax_p1(oracle, out[:, :2]), p), "class probability differs from the oracle"


def _small_calls(eng, frames, pairs, net):
    """Every pair through calls with capacity == count <= 8: the per-candidate reference."""
    return np.concatenate([eng.stage_net(frames, pairs[i:i + 8], net, len(pairs[i:i + 8])).cpu().numpy() for i in range(0, P, 8)])


def _engine(blob):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from truely_amd.engine import Engine
    return Engine(blob)


@pytest.fixture(scope="module")
def eng(blob):
    """A context of this module's own: the chunk options it sets stay here."""
    e = _engine(blob)
    yield e
    e.close()


@pytest.fixture(scope="module")
def refs(eng, frames, pairs):
    return {net: _small_calls(eng, frames, pairs, net) for net in (24, 48)}


def _run(eng, frames, pairs, net, cap, chunk, count, shift, poison=0xFF):
    eng.option("rnet_chunk" if net == 24 else "onet_chunk", chunk)
    idx = (np.arange(count) + shift) % P
    eng.poison_workspaces(poison)
    out = eng.stage_net(frames, pairs[idx], net, cap, fill=float(SENTINEL)).cpu().numpy()
    plan = eng.mtcnn_plan()
    eng.option("rnet_chunk" if net == 24 else "onet_chunk", CHUNK[net])
    return out, plan, idx


def _check_rows(out, ref, idx, net, cap, chunk, count, what):
    live = min(count, cap)
    got, want = out[:live], ref[idx[:live]]
    bad = np.flatnonzero((got.view(np.int32) != want.view(np.int32)).any(axis=1))
    assert len(bad) == 0, f"{what}: {len(bad)} of {live} live rows differ, first at candidate {bad[:8].tolist()}"
    bmh = conv_path(1, 1, TAIL[net][-1][2], 1, TAIL[net][-1][4])[1]          # the heads' row tile (the launch writing d_out)
    for t0, nc in chunks(cap, chunk):
        lc = min(max(count - t0, 0), nc)
        first_dead_tile = t0 + -(-lc // bmh) * bmh
        if first_dead_tile < t0 + nc:
            tail = out[first_dead_tile:t0 + nc]
            assert (tail == SENTINEL).all(), f"{what}: chunk t0={t0} wrote rows of tiles past its {lc} live candidates"


@pytest.fixture(scope="module")
def case_runs(eng, frames, pairs, refs):
    """Every case once: its plan, and what checking its rows found (None = exact)."""
    plans, errors = {}, {}
    for net in (24, 48):
        for j, (cap, chunk, count) in enumerate(CASES[net]):
            out, plan, idx = _run(eng, frames, pairs, net, cap, chunk, count, shift=(7 * j) % P)
            try:
                _check_rows(out, refs[net], idx, net, cap, chunk, count, f"net {net} capacity {cap} chunk {chunk} count {count}")
            except AssertionError as e:
                errors[(net, cap, chunk, count)] = str(e)
            plans[(net, cap, chunk, count)] = plan
    return plans, errors


@pytest.mark.gpu
@pytest.mark.parametrize("net", [24, 48])
def test_reference_rows_equal_the_oracle(eng, oracle, frames, pairs, refs, net):
    """The per-candidate reference (calls of <= 8 candidates) has the oracle's bits for all P pairs: R-Net / O-Net on the
    oracle's crops, class probability through the shared softmax."""
    _assert_oracle(oracle, refs[net], _crops(oracle, frames, pairs, net), net)


@pytest.mark.gpu
def test_every_case_live_rows_exact(case_runs):
    """Every live row of every case equals its pair's reference row bit for bit, and no tile past the live rows wrote its
    output."""
    plans, errors = case_runs
    assert len(plans) == len(CASES[24]) + len(CASES[48])
    assert not errors, "\n".join(errors.values())


@pytest.mark.gpu
def test_plan_equals_restatement(case_runs):
    """Row by row, chunk after chunk: the kernel, tile, K chunk and GEMM shape each tail conv launched with."""
    for (net, cap, chunk, count), plan in case_runs[0].items():
        want = plan_of(net, cap, chunk)
        assert len(plan) == len(want), f"net {net} capacity {cap} chunk {chunk}: {len(plan)} rows, expected {len(want)}"
        for got, exp in zip(plan, want):
            assert got == exp, f"net {net} capacity {cap} chunk {chunk} count {count}"


@pytest.mark.gpu
def test_plans_reach_every_path(case_runs):
    """The union of the plans is exactly what the restatement can produce for per-launch capacities 1 .. 49,152."""
    got = {}
    for plan in case_runs[0].values():
        for r in plan:
            got.setdefault(r["layer"], set()).add((r["family"], r["bm"], r["bn"], r["bk"], r["pad"]))
    want = {**reachable(24)[0], **reachable(48)[0]}
    assert got == want


@pytest.mark.gpu
@pytest.mark.parametrize("net", [24, 48])
def test_largest_case_over_poisoned_workspaces(eng, frames, pairs, refs, net):
    """The largest case once over 0xFF (NaN) and once over 0x7F (huge finite) workspaces: dead rows compute on them, live rows
    keep their bits."""
    cap, chunk, count = max(CASES[net], key=lambda c: (c[0], c[2]))
    for byte in (0xFF, 0x7F):
        out, _, idx = _run(eng, frames, pairs, net, cap, chunk, count, shift=101, poison=byte)
        _check_rows(out, refs[net], idx, net, cap, chunk, count, f"net {net} capacity {cap} over 0x{byte:02X}")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", SLOPE_VARIANTS)
def test_front_slope_modes_at_production_capacity(frames, pairs, variant):
    """The front kernel's other two conv1 PReLU slope classes (slopes above 1: MODE 1; negative slopes: MODE 0) at one large
    capacity per net: live rows equal that blob's small calls, which equal that blob's oracle."""
    from oracle.oracle import Oracle
    blob = _slope_variant_blob(variant)
    e, orc = _engine(blob), Oracle(blob)
    try:
        for net in (24, 48):
            ref = _small_calls(e, frames, pairs, net)
            _assert_oracle(orc, ref, _crops(orc, frames, pairs, net), net)
            cap = PROD[net][0]
            count = cap - 3
            out, _, idx = _run(e, frames, pairs, net, cap, CHUNK[net], count, shift=13)
            _check_rows(out, ref, idx, net, cap, CHUNK[net], count, f"{variant} net {net} capacity {cap}")
    finally:
        e.close()
