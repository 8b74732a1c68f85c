"""The max pools of R-Net conv2 and O-Net conv2 / conv3 inside the conv kernel's epilogue, against the separate pool launch.

At launch capacities where trl_launch_conv picks a 128-row tile for these layers (conv_tap48 from 203 R-Net candidates, conv_tap
128 x 64 from 38 O-Net candidates for conv2 and from 256 for conv3), trl_run_net issues the conv with a pooling epilogue
(csrc/trl_tailpool.h: each tile reduces the part of every window it holds; a fix-up kernel combines the two parts of a window that
meets a tile boundary) and the conv's own map is never stored.  ``Engine.option("tail_pool", 0)`` issues conv and pool separately,
as below those capacities.

Every case runs the production loop (Engine.stage_net) once with the option off and once on, over 0xFF (NaN) and 0x7F (huge)
workspaces, and the live rows are compared as bits; the recorded plan is the same either way and equals the restatement of
test_gpu_stage_nets.py; the workspace high-water mark differs exactly where the restatement below says a layer fuses.  Capacities
sit on both sides of where fusing starts, live counts at 0, 1, capacity - 1, capacity, above, and where the last live row is one
before, at and one after a multiple of the 128-row tile; two-chunk cases end inside the second chunk.  One weight variant makes
some conv2 / conv3 channels exactly +-0 (zero weights, bias -0.0), so that pooling windows are full of ties whose winner the scan
order decides: fused, separate and the oracle agree bit for bit."""
import numpy as np
import pytest

from test_gpu_stage_nets import P, _assert_oracle, _crops, _engine, _small_calls, frames, pairs, plan_of  # noqa: F401 (fixtures)

BM = 128
# (layer, conv output side, first per-launch capacity with M = nc * side^2 >= 16384: the 128-row families) of the fused layers
FUSED = {24: [("rnet.conv2", 9, 203)], 48: [("onet.conv2", 21, 38), ("onet.conv3", 8, 256)]}
CHUNK = {24: ("rnet_chunk", 49152), 48: ("onet_chunk", 16384)}


def fuses(net, nc):
    """Does any layer of a chunk of nc candidate slots take its pooling epilogue?"""
    return any(nc >= first for _, _, first in FUSED[net])


def boundary_counts(net, cap):
    """Live counts <= cap whose last live row of a fused layer is one before, at, or one after a multiple of the row tile."""
    out = set()
    for _, side, first in FUSED[net]:
        if cap < first:
            continue
        for r in (BM - 1, 0, 1):
            c = next((c for c in range(cap, 0, -1) if (c * side * side) % BM == r), None)
            if c:
                out.add(c)
    return out


def cases(net):
    out = set()
    caps = (202, 203, 204) if net == 24 else (37, 38, 255, 256, 257)
    for cap in caps:
        out |= {(cap, CHUNK[net][1], n) for n in (0, 1, cap - 1, cap, cap + 5)}
    top = caps[-1]
    out |= {(top, CHUNK[net][1], n) for n in boundary_counts(net, top)}
    out |= {(500, 250, 377), (500, 250, 250)} if net == 24 else {(100, 50, 77), (100, 50, 50)}   # two chunks
    return sorted(out)


CASES = [(net,) + c for net in (24, 48) for c in cases(net)]


def test_cases_cover_the_edges():
    for net in (24, 48):
        cs = cases(net)
        for _, _, first in FUSED[net]:
            assert {first - 1, first} <= {cap for cap, _, _ in cs}
        top = max(cap for cap, chunk, _ in cs if chunk == CHUNK[net][1])
        side = FUSED[net][0][1]
        assert {(n * side * side) % BM for cap, _, n in cs if cap == top} >= {BM - 1, 0, 1}
        assert any(cap > chunk and chunk < n < cap for cap, chunk, n in cs)
    assert (257 * 64) % BM == 64                               # 257 O-Net slots: the last conv3 tile is half live


@pytest.fixture(scope="module")
def eng(blob):
    e = _engine(blob)
    yield e
    e.close()


def _run(eng, frames, pairs, net, cap, chunk, count, fused, poison, shift=0):
    key, default = CHUNK[net]
    eng.option(key, chunk)
    eng.option("tail_pool", fused)
    idx = (np.arange(count) + shift) % P
    eng.poison_workspaces(poison)
    try:
        out = eng.stage_net(frames, pairs[idx], net, cap).cpu().numpy()
        return out[:min(count, cap)], eng.mtcnn_plan(), eng.workspace()["scratch_high"], idx[:min(count, cap)]
    finally:
        eng.option(key, default)
        eng.option("tail_pool", 1)


def _same_bits(a, b, what):
    bad = np.flatnonzero((a.view(np.int32) != b.view(np.int32)).any(axis=1))
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(a)} live rows differ, first at candidate {bad[:8].tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("net,cap,chunk,count", CASES)
def test_fused_equals_separate(eng, frames, pairs, net, cap, chunk, count):
    what = f"net {net} capacity {cap} chunk {chunk} count {count}"
    want_plan = plan_of(net, cap, chunk)
    for poison in (0xFF, 0x7F):
        sep, plan0, high0, _ = _run(eng, frames, pairs, net, cap, chunk, count, 0, poison, shift=cap % P)
        fus, plan1, high1, _ = _run(eng, frames, pairs, net, cap, chunk, count, 1, poison, shift=cap % P)
        _same_bits(fus, sep, f"{what} over 0x{poison:02X}")
        assert plan0 == plan1 == want_plan, what
        # (the first chunk is the largest: it sizes the workspace)
        assert (high0 != high1) == fuses(net, min(cap, chunk)), f"{what}: workspace {high0} separate, {high1} fused"


@pytest.mark.gpu
def test_option_is_checked(eng):
    with pytest.raises(Exception):
        eng.option("tail_pool", 2)
    eng.option("tail_pool", 1)


def zero_tie_blob():
    """conv2 / conv3 of R-Net and O-Net with a few output channels of all-zero weights and bias -0.0: those channels are +0 or -0 by
    the signs of the window's inputs (a chain of fmaf(x, 0, acc) from -0 stays -0 only while every product is -0)."""
    from truely_amd import weights
    sds = [dict(sd) for sd in weights.synthetic_state_dicts(0)]
    for net, layers in ((sds[1], ("conv2",)), (sds[2], ("conv2", "conv3"))):
        for layer in layers:
            w = np.array(net[f"{layer}.weight"], np.float32, copy=True)
            b = np.array(net[f"{layer}.bias"], np.float32, copy=True)
            ch = np.arange(1, w.shape[0], 7)
            w[ch] = 0.0
            b[ch] = -0.0
            net[f"{layer}.weight"], net[f"{layer}.bias"] = w, b
    return weights.pack_state_dicts(*sds)


@pytest.mark.gpu
def test_sign_of_zero_ties(frames, pairs):
    from oracle.oracle import Oracle
    blob = zero_tie_blob()
    e, orc = _engine(blob), Oracle(blob)
    try:
        for net, cap in ((24, 204), (48, 257)):
            ref = _small_calls(e, frames, pairs, net)                       # calls of <= 8 candidates: separate pools
            _assert_oracle(orc, ref, _crops(orc, frames, pairs, net), net)
            sep, _, _, idx = _run(e, frames, pairs, net, cap, CHUNK[net][1], cap, 0, 0xFF, shift=3)
            fus, _, _, _ = _run(e, frames, pairs, net, cap, CHUNK[net][1], cap, 1, 0xFF, shift=3)
            _same_bits(fus, sep, f"zero ties, net {net}: fused against separate")
            _same_bits(fus, ref[idx], f"zero ties, net {net}: fused against the oracle's rows")
    finally:
        e.close()
