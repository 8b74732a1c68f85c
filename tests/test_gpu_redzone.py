"""Do the kernels store only inside the workspace block they were handed?

The other GPU tests compare results; an over-store that lands in alignment padding, in the next block (which its own producer
overwrites later) or in the slack trl_ensure adds behind the last block changes no result.  Engine.redzone(guard, byte) follows
every block of a context's two workspaces (cascade lists, scratch) with `guard` bytes that belong to no block, fills everything
outside the blocks with `byte`, and sweeps it at every rewind of the allocator, before a workspace is freed to grow, and at the
end of every call (include/truely_hip.h: trl_debug_redzone; the allocator itself: tests/test_arena_cpu.py).

Every scenario below runs on fresh engines: once with the switch off, and with a 64 KiB guard once over 0xA5 and once over 0x5A
-- a stray store that happens to equal one pattern cannot equal both.  Then: no hit; sweeps made and guard bytes checked are > 0
and the sweeps at least the rewinds the scenario is known to make; every output equals the switch-off run bit for bit; and the
counts hold (cascade: the list arena ends at its count; embedder: count and high-water mark equal the CPU restatement with the
guard).  The last tests turn the checker on itself: bytes poked into chosen gaps are found at the right place, once."""
import numpy as np
import pytest
import torch

import truely_amd
import front_ref
from logits_ref import blob_with_head
from test_gpu_extract import _multiface
from test_gpu_stage_nets import P as N_PAIRS, frames as stage_frames, pairs as stage_pairs  # noqa: F401  (two module-scoped fixtures)
from test_gpu_workspace import _ramp_frames
from test_workspace_cpu import embedder_bytes
from truely_amd import _lib
from truely_amd.engine import Engine
from truely_amd.pipeline import detect_embed_overlapped

pytestmark = pytest.mark.gpu
GUARD = 65536
FILLS = (0xA5, 0x5A)


@pytest.fixture
def make_engine(blob):
    """Fresh contexts, closed when the test ends (passed or not)."""
    made = []

    def make(blob_=None, **kw):
        made.append(Engine(blob_ or blob, **kw))
        return made[-1]
    yield make
    for e in made:
        e.close()


def _bytes_of(v):
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().contiguous().numpy()
    return np.ascontiguousarray(v).tobytes()


def _assert_same(got: dict, want: dict, what):
    assert got.keys() == want.keys()
    for k in want:
        assert _bytes_of(got[k]) == _bytes_of(want[k]), f"{what}: output '{k}' differs from the run without red zones"


def _clean(eng, what, min_sweeps):
    torch.cuda.synchronize()
    rep = eng.redzone_report()
    print(f"{what}: sweeps {rep['sweeps']} guard bytes checked {rep['bytes']} hits {rep['nhits']}")
    assert rep["nhits"] == 0 and not rep["hits"], (what, rep["hits"][:4])
    assert rep["sweeps"] >= max(1, min_sweeps) and rep["bytes"] > 0, (what, rep)
    return rep


def sweep_scenario(make, run, min_sweeps, what, check=None, **engine_kw):
    """run(eng) -> {name: tensor}; check(eng, guard) asserts the scenario's counts.  min_sweeps: the allocator rewinds the scenario
    is known to make.  Each is one sweep, but for the first rewind of a workspace that has not been allocated yet (nothing to look
    at: at most one per workspace); the two sweeps at the end of every call make up for those."""
    ref = make(**engine_kw)
    want = run(ref)
    torch.cuda.synchronize()
    if check:
        check(ref, 0)
    for fill in FILLS:
        eng = make(**engine_kw)
        eng.redzone(GUARD, fill)
        got = run(eng)
        _clean(eng, f"{what} over 0x{fill:02X}", min_sweeps)
        _assert_same(got, want, what)
        if check:
            check(eng, GUARD)
    return want


def _cascade_counts(eng, guard):
    ws = eng.workspace()
    assert 0 < ws["arena_off"] == ws["arena_need"] <= ws["arena_cap"] and 0 < ws["scratch_high"] <= ws["scratch_cap"], ws


# ---- the cascade ---------------------------------------------------------------------------------------------------------------

# One attempt of detect_embed rewinds: the list layout, trl_scratch_begin, stage_carve x 2, one chunk each, crop_embed = 7
@pytest.mark.parametrize("shape", [(3, 360, 640, 11), (2, 97, 131, 21)], ids=str)
@pytest.mark.parametrize("pnet_run", [0, 5])
def test_cascade_fused_one_attempt(make_engine, shape, pnet_run):
    n, H, W, seed = shape
    fr = truely_amd.synthetic.synthetic_frames(n, H, W, seed=seed)

    def run(eng):
        eng.pnet_run(pnet_run)
        out = eng.detect_embed(fr)
        assert eng.list_stats()["attempts"] == 1
        return out
    sweep_scenario(make_engine, run, 7, f"detect_embed {shape} pnet_run {pnet_run}", _cascade_counts)


@pytest.mark.parametrize("form", ["default", "rerun_from_stage_1", "resume_at_stage_2"])
def test_cascade_rerun_and_resume(make_engine, form):
    """_ramp_frames() in the three forms of test_gpu_workspace.py: a re-run lays the lists out again (one more of every rewind), a
    resume keeps them and carves the scratch again."""
    fr = _ramp_frames()
    kw = dict(cap_level=64, cap_frame=64) if form == "rerun_from_stage_1" else {}

    def run(eng):
        eng.batch_capacity(1.0 if form == "resume_at_stage_2" else 0.0, 0.0)
        out = eng.detect_embed(fr)
        attempts = eng.list_stats()["attempts"]
        assert attempts == 1 if form == "default" else attempts > 1, attempts
        return out
    got = sweep_scenario(make_engine, run, {"default": 7, "rerun_from_stage_1": 14, "resume_at_stage_2": 12}[form], f"ramp frames, {form}",
                         _cascade_counts, **kw)
    assert got["valid"].any()


def test_cascade_spill_tier(make_engine):
    """One 97 x 131 frame of uniform noise, every threshold 0, the LDS tiers lowered: the sort + NMS kernels work in the spill pool,
    a block of the list arena with a red zone behind it."""
    fr = np.random.default_rng(77).integers(0, 256, (1, 97, 131, 3), dtype=np.uint8)

    def run(eng):
        eng.nms_tiers(16, 64)
        out = eng.detect_embed(fr)
        st = eng.list_stats()
        assert st["spill_lists"] >= 1 and st["spill_used"] <= st["spill_cap"], st
        return out
    sweep_scenario(make_engine, run, 7, "spill tier", _cascade_counts, thresholds=(0.0, 0.0, 0.0))


@pytest.mark.parametrize("case", ["97x131", "17_levels"])
def test_cascade_generic_pnet(make_engine, case):
    """PNet level by level through the layer kernels: the scratch is rewound for every level (trl_pnet_generic_level)."""
    if case == "97x131":
        fr, kw = truely_amd.synthetic.synthetic_frames(2, 97, 131, seed=21), dict(pnet_mode=1)
    else:                                                   # more levels than the fused launch carries: the same path by itself
        fr, kw = truely_amd.synthetic.synthetic_frames(3, 180, 320, seed=17), dict(min_face_size=12, factor=0.85)
    levels = []

    def run(eng):
        levels.append(eng.levels(*fr.shape[1:3]))
        return eng.detect_embed(fr)
    # the rewinds: one per level that has a PNet map, on top of the 7 of a fused call
    sweep_scenario(make_engine, run, 7 + (17 if case == "17_levels" else 2), f"generic PNet {case}", _cascade_counts, **kw)
    assert len(set(levels)) == 1 and (levels[0] == 17 if case == "17_levels" else levels[0] >= 2)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_detect_crop_every_embed_mode(make_engine, mode):
    fr = truely_amd.synthetic.synthetic_frames(3, 360, 640, seed=11)
    got = sweep_scenario(make_engine, lambda eng: eng.detect_crop(fr), 6, f"detect_crop embed_mode {mode}", _cascade_counts, embed_mode=mode)
    assert got["valid"].any()


def test_extract_faces_and_landmarks(make_engine):
    fr = _multiface()

    def run(eng):
        out = eng.extract_faces(fr, keep_all=True, margin=20, image_size=160)
        boxes, probs, counts, points = eng.mtcnn_detect(fr, landmarks=True)
        assert int(out["counts"].sum()) > len(fr)           # more than one face in some frame
        return dict(faces=out["faces"], frame=out["frame"], box=out["box"], status=out["status"], boxes=boxes, probs=probs, counts=counts,
                    points=points)
    sweep_scenario(make_engine, run, 13, "extract_faces + mtcnn_detect(landmarks)", _cascade_counts)


# ---- R-Net / O-Net launch sets ------------------------------------------------------------------------------------------------

# (net, capacity, chunk or None, live count): one launch set at a path threshold of the tail convs, and chunked sets whose count
# ends inside the second chunk (test_gpu_stage_nets.py has the restatement of the paths)
# each with the tail pools in the conv epilogue and as launches of their own; an empty list once per net
STAGE_CASES = [c + (tp,) for c in ((24, 204, None, 204), (24, 500, 250, 377), (48, 257, None, 257), (48, 100, 50, 77)) for tp in (1, 0)] + \
              [(24, 64, None, 0, 1), (48, 64, None, 0, 1)]


@pytest.mark.parametrize("net,cap,chunk,count,tail_pool", STAGE_CASES, ids=str)
def test_stage_net_launch_sets(make_engine, stage_frames, stage_pairs, net, cap, chunk, count, tail_pool):
    rec = stage_pairs[(np.arange(count) + 7 * net) % N_PAIRS]

    def run(eng):
        eng.option("tail_pool", tail_pool)
        if chunk:
            eng.option("rnet_chunk" if net == 24 else "onet_chunk", chunk)
        out = eng.stage_net(stage_frames, rec, net, cap, fill=-12345.678)
        return dict(live=out[:min(count, cap)])             # rows past the count inside a live tile are not defined
    nchunks = -(-cap // chunk) if chunk else 1
    sweep_scenario(make_engine, run, 2 + nchunks, f"stage_net {net} cap {cap} chunk {chunk} count {count} tail_pool {tail_pool}")


@pytest.mark.parametrize("S", [24, 48])
def test_front_kernel_alone(make_engine, S):
    nf, H, W = front_ref.BATCHES[1]
    rec = front_ref.placed(nf, H, W, S)
    base = front_ref.content_frames("random", nf, H, W, seed=H + S)
    P, C1 = front_ref.NETS[S]["P"], front_ref.NETS[S]["C1"]

    def run(eng):
        out = torch.full((len(rec) + 5, P, P, C1), float("nan"), dtype=torch.float32, device=eng.device)
        return dict(pool=eng.front_pool(base, rec, S, len(rec) + 5, out=out))
    sweep_scenario(make_engine, run, 1, f"front_pool {S}")


# ---- the embedder ----------------------------------------------------------------------------------------------------------------

EMBED_CASES = [(1, 75, 75, "f32", 0), (2, 75, 107, "f32", 0), (3, 160, 160, "f32", 0), (334, 75, 75, "f32", 0), (335, 75, 75, "f32", 0),
               (1, 75, 75, "f32", 1), (5, 80, 80, "bf16", 0), (32, 80, 80, "bf16", 0), (5, 80, 80, "fp16", 0), (32, 80, 80, "fp16", 0)]


@pytest.mark.parametrize("n,h,w,prec,no_fnconv", EMBED_CASES, ids=str)
def test_embedder(make_engine, n, h, w, prec, no_fnconv):
    faces = torch.from_numpy(np.random.default_rng(n + h).uniform(0, 1, (n, h, w, 3)).astype(np.float32))
    es = 4 if prec == "f32" else 2

    def run(eng):
        try:
            if no_fnconv:
                eng.option("no_fnconv", 1)
            emb = eng.facenet_embed(faces)
            torch.cuda.synchronize()
        finally:
            if no_fnconv:
                eng.option("no_fnconv", 0)
        assert torch.isfinite(emb).all()
        return dict(emb=emb)

    def check(eng, guard):
        try:
            if no_fnconv:
                eng.option("no_fnconv", 1)
            ws = eng.workspace(1, n, h, w)
        finally:
            if no_fnconv:
                eng.option("no_fnconv", 0)
        want = embedder_bytes(n, h, w, es, bool(no_fnconv), guard=guard)
        assert ws["need"] == ws["scratch_high"] == want <= ws["scratch_cap"], (ws, want)
    sweep_scenario(make_engine, run, 1, f"facenet_embed {(n, h, w, prec, no_fnconv)}", check, embed_precision=prec)


def test_embedder_features_logits_and_mask(make_engine):
    blob_c = blob_with_head(33)
    rng = np.random.default_rng(80)
    faces = torch.from_numpy(rng.uniform(0, 1, (3, 80, 80, 3)).astype(np.float32))
    valid = torch.tensor([1, 0, 1], dtype=torch.uint8)

    def run(eng):
        feat = eng.facenet_features(faces)
        return dict(feat=feat, logits=eng.facenet_logits(feat), masked=eng.embed_faces(faces, valid))
    got = sweep_scenario(make_engine, run, 2, "features + logits + embed_faces", blob_=blob_c)
    assert not got["masked"][1].any() and got["masked"][0].any()


# ---- pyramid hooks -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("min_face_size,shapes,passes", [(20, ((3, 180, 320), (2, 97, 131)), "FS"), (12, ((1, 720, 1280),), "L")], ids=str)
def test_pyramid_batch_every_pass(make_engine, min_face_size, shapes, passes):
    """(180, 320) and (97, 131) choose the fine pass and the streaming pass; one 720 x 1280 frame at min_face_size 12 (its level 0 is
    larger than the frame: no fine pass, as in test_gpu_pyramid.py's table) the per-level kernels.  pyramid_plan() confirms it."""
    batches = [truely_amd.synthetic.synthetic_frames(n, H, W, seed=5 + n) for n, H, W in shapes]
    kernels = set()

    def run(eng):
        out = {}
        for i, fr in enumerate(batches):
            pyr, levels = eng.pyramid_batch(fr)
            kernels.update(r["kernel"] for r in eng.pyramid_plan())
            # the padding behind a level is not written by every pass: the level pixels are the output
            out[f"pyr{i}"] = torch.cat([pyr[:, g["pix0"]:g["pix0"] + g["h"] * g["w"]].reshape(-1) for g in levels])
        return out
    sweep_scenario(make_engine, run, len(shapes), f"pyramid_batch {shapes}", min_face_size=min_face_size)
    if passes == "FS":
        assert "F" in kernels and kernels & {"S4", "S8", "SW4", "SW8"}, kernels
    else:
        assert kernels & {"L0-3", "L0-4", "L0-5", "L1", "L2"}, kernels


# ---- begin / end: two cascade contexts and the embedder's ------------------------------------------------------------------------

def test_overlapped_begin_end(make_engine):
    batches = [truely_amd.synthetic.synthetic_frames(2, 180, 320, seed=40 + i) for i in range(6)]

    def run_all(guard, fill):
        engs = [make_engine(), make_engine(), make_engine()]
        for e in engs:
            if guard:
                e.redzone(guard, fill)
        outs = detect_embed_overlapped(engs[:2], batches, embed_group=2, embed_engine=engs[2])
        torch.cuda.synchronize()
        return engs, {f"{k}{i}": o[k] for i, o in enumerate(outs) for k in ("box", "prob", "rect", "valid", "emb")}
    _, want = run_all(0, 0)
    assert any(want[f"valid{i}"].any() for i in range(6))
    for fill in FILLS:
        engs, got = run_all(GUARD, fill)
        for j, e in enumerate(engs):                        # three calls per cascade context (6 rewinds each), three embedder calls
            _clean(e, f"overlapped context {j} over 0x{fill:02X}", 18 if j < 2 else 3)
        _assert_same(got, want, "overlapped")


# ---- the checker itself ------------------------------------------------------------------------------------------------------------

def _one_hit(eng, arena, block, offset, gap_range=None, site="report", trigger=None):
    eng.redzone_poke(arena, block, offset)
    if trigger:
        trigger()
        torch.cuda.synchronize()
    rep = eng.redzone_report(clear=True, sweep=trigger is None)
    assert rep["nhits"] == 1 and len(rep["hits"]) == 1, rep["hits"]
    h = rep["hits"][0]
    assert (h["arena"], h["site"], h["first"], h["last"], h["count"]) == (arena, site, offset, offset, 1), h
    if block >= 0:
        assert h["block"] == block and GUARD <= h["gap_bytes"] < GUARD + 256, h
    else:
        assert h["block_bytes"] == 0, h
    return h


def test_poked_bytes_are_found_once_and_where_they_are(make_engine):
    n, H, W = 2, 97, 131
    fr = truely_amd.synthetic.synthetic_frames(n, H, W, seed=21)
    eng = make_engine()
    eng.redzone(GUARD, 0xA5)
    eng.detect_embed(fr)
    _clean(eng, "before the pokes", 7)
    ws = eng.workspace()
    first_block = {0: n * eng.levels(H, W) * 4, 1: n * 80 * 80 * 3 * 4}      # the level counts [n][L]; the crops of crop_embed
    for arena, cap in ((0, ws["arena_cap"]), (1, ws["scratch_cap"])):
        h = _one_hit(eng, arena, 0, 0)
        assert h["block_bytes"] == first_block[arena] == h["gap_off"], h
        gap = h["gap_bytes"]
        _one_hit(eng, arena, 0, gap // 2)
        _one_hit(eng, arena, 0, gap - 1)
        for k in (1, 5):                                                         # another gap: the ordinal follows
            hk = _one_hit(eng, arena, k, 17)
            assert hk["gap_off"] > h["gap_off"] + gap
        with pytest.raises(_lib.TrlError) as e:                                  # one byte past the gap's last
            eng.redzone_poke(arena, 0, gap)
        assert e.value.status == -1
        t = _one_hit(eng, arena, -1, 12345)                                      # the tail, up to the capacity
        assert t["gap_off"] + t["gap_bytes"] == cap and t["block"] > 5, (t, cap)
        if arena == 0:
            assert t["gap_off"] == ws["arena_off"]
        rep = eng.redzone_report(clear=True, sweep=True)                         # every poke was repaired: a sweep of each workspace, clean
        assert rep["sweeps"] == 2 and rep["nhits"] == 0 and not rep["hits"], rep
    rep = eng.redzone_report()
    assert rep == dict(sweeps=0, bytes=0, nhits=0, hits=[])                      # after clear the report is empty
    # found by the sweep of the next call's first rewind, named by its site; repaired, so the call after that is clean
    faces = torch.rand((1, 75, 75, 3))
    _one_hit(eng, 1, 3, 1000, site="scratch_begin", trigger=lambda: eng.facenet_embed(faces))
    _one_hit(eng, 0, 2, 0, site="lists", trigger=lambda: eng.detect_embed(fr))
    eng.detect_embed(fr)
    _clean(eng, "after the pokes", 7)


def test_switch_off_again_is_an_engine_that_never_had_it(make_engine):
    fr = truely_amd.synthetic.synthetic_frames(2, 97, 131, seed=21)
    faces = torch.from_numpy(np.random.default_rng(3).uniform(0, 1, (2, 75, 75, 3)).astype(np.float32))

    def run(eng):
        out = dict(eng.detect_embed(fr))
        ws1 = eng.workspace()
        out["emb75"] = eng.facenet_embed(faces)
        torch.cuda.synchronize()
        return out, ws1, eng.workspace(1, 2, 75, 75)
    never, was = make_engine(), make_engine()
    was.redzone(GUARD, 0x5A)
    on = run(was)
    assert on[2]["need"] == embedder_bytes(2, 75, 75, guard=GUARD) > embedder_bytes(2, 75, 75)
    was.redzone(0)
    assert was.redzone_report(sweep=True) == dict(sweeps=0, bytes=0, nhits=0, hits=[])
    run(never)                                                                   # (the capacities follow the calls: the same history)
    a, b = run(never), run(was)
    _assert_same(b[0], a[0], "switched off again")
    _assert_same(on[0], a[0], "switched on")
    counts = ("scratch_high", "arena_off", "arena_need", "need")
    assert [b[1][k] for k in counts] == [a[1][k] for k in counts] and [b[2][k] for k in counts] == [a[2][k] for k in counts]
    assert b[2]["need"] == b[2]["scratch_high"] == embedder_bytes(2, 75, 75)
    was.poison_workspaces(0xFF)                                                  # allowed again


def test_refusals(make_engine):
    eng = make_engine()
    for guard in (100, 255, 257, -256, -1, (1 << 20) + 256, 1 << 21):
        with pytest.raises(_lib.TrlError) as e:
            eng.redzone(guard)
        assert e.value.status == -1, guard
    for byte in (-1, 256):
        with pytest.raises(_lib.TrlError) as e:
            eng.redzone(GUARD, byte)
        assert e.value.status == -1
    with pytest.raises(_lib.TrlError) as e:                                      # off: nothing to poke
        eng.redzone_poke(0, 0, 0)
    assert e.value.status == -5
    eng.redzone(1 << 20)                                                         # the limit itself, and 256
    eng.redzone(256)
    with pytest.raises(_lib.TrlError) as e:                                      # the fill byte is the poison while it is on
        eng.poison_workspaces(0xFF)
    assert e.value.status == -5
    with pytest.raises(_lib.TrlError) as e:                                      # no workspace yet
        eng.redzone_poke(1, 0, 0)
    assert e.value.status == -5
    fr = truely_amd.synthetic.synthetic_frames(2, 97, 131, seed=21)
    eng.detect_embed_begin(fr)
    try:
        for call in (lambda: eng.redzone(0), lambda: eng.redzone(GUARD), eng.redzone_report, lambda: eng.redzone_poke(0, 0, 0)):
            with pytest.raises(_lib.TrlError) as e:                              # a call in flight
                call()
            assert e.value.status == -5
    finally:
        eng.detect_embed_end()
    with pytest.raises(_lib.TrlError) as e:                                      # the fill byte itself is no poke
        eng.redzone_poke(0, 0, 0, value=0xA5)
    assert e.value.status == -1
    _clean(eng, "after the refusals", 7)
