"""Every workspace is sized by a dry run of the code that carves it: what the library counts is what it then takes.

- the embedder: on a fresh context the count Engine.workspace() reports for (faces, h, w) equals the CPU restatement of the
  walk's allocation rule (tests/test_workspace_cpu.py), the scratch high-water mark after facenet_embed equals it exactly, and
  the capacity covers it -- f32, both forms of block35, no_fnconv, bf16, fp16;
- 24 faces of 300 x 300 embed on a fresh context, every row with the bits of the same face embedded alone: a call's size does
  not depend on what the context ran before;
- whole R-Net / O-Net calls: high-water mark = count;
- the cascade: the list arena ends exactly at its count -- on a call that fits at once, on one that re-runs itself with larger
  lists and on one that resumes at stage 2 with a larger R-Net batch; the three deliver the same bits, and an equal second
  batch grows nothing."""
import numpy as np
import pytest
import torch

from test_workspace_cpu import embedder_bytes
from truely_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture
def make_engine(blob):
    """Fresh contexts, closed when the test ends (passed or not)."""
    made = []

    def make(**kw):
        made.append(Engine(blob, **kw))
        return made[-1]
    yield make
    for e in made:
        e.close()


# (faces, h, w, precision, no_fnconv): the smallest accepted size (its 1x1 block8 map skips the average pool), a non-square one,
# the 160 px crop, both sides of block35_grouped (faces x 49 <= 16384: the concat buffer is 128 or 96 wide), the option, 16 bits
EMBED_CASES = [(1, 75, 75, "f32", 0), (2, 75, 107, "f32", 0), (3, 160, 160, "f32", 0), (334, 75, 75, "f32", 0), (335, 75, 75, "f32", 0),
               (1, 75, 75, "f32", 1), (1, 75, 75, "bf16", 0), (1, 75, 75, "fp16", 0)]


@pytest.mark.parametrize("n,h,w,prec,no_fnconv", EMBED_CASES, ids=str)
def test_embedder_count_equals_restatement_equals_carved(make_engine, n, h, w, prec, no_fnconv):
    eng = make_engine(embed_precision=prec)
    want = embedder_bytes(n, h, w, 4 if prec == "f32" else 2, bool(no_fnconv))
    try:
        if no_fnconv:                                  # the need kept for (n, h, w) must not outlive the option it was counted under
            assert eng.workspace(1, n, h, w)["need"] == embedder_bytes(n, h, w) != want
            eng.option("no_fnconv", 1)
        ws = eng.workspace(1, n, h, w)
        print(f"need {ws['need']} restated {want}")
        assert ws["need"] == want and ws["scratch_cap"] == 0
        faces = torch.from_numpy(np.random.default_rng(n + h).uniform(0, 1, (n, h, w, 3)).astype(np.float32))
        emb = eng.facenet_embed(faces)
        torch.cuda.synchronize()
    finally:
        if no_fnconv:
            eng.option("no_fnconv", 0)
    assert torch.isfinite(emb).all()
    ws = eng.workspace()
    print(f"high {ws['scratch_high']} capacity {ws['scratch_cap']}")
    assert ws["scratch_high"] == want and ws["scratch_cap"] >= want


def test_fresh_context_embeds_24_faces_of_300(make_engine):
    """The walk of this call takes 1,241,926,464 bytes (test_workspace_cpu.py); a fresh context provides them."""
    faces = torch.from_numpy(np.random.default_rng(300).uniform(0, 1, (24, 300, 300, 3)).astype(np.float32))
    eng, one = make_engine(), make_engine()
    emb = eng.facenet_embed(faces)
    ws = eng.workspace(1, 24, 300, 300)
    assert ws["need"] == ws["scratch_high"] == embedder_bytes(24, 300, 300) <= ws["scratch_cap"]
    alone = torch.cat([one.facenet_embed(faces[i:i + 1]) for i in range(24)])
    assert torch.isfinite(emb).all() and torch.equal(emb, alone)


def test_mtcnn_net_count_equals_carved(make_engine):
    eng = make_engine()
    rng = np.random.default_rng(5)
    for what, side, run in ((24, 24, eng.rnet), (48, 48, eng.onet)):
        need = eng.workspace(what, 5)["need"]
        out = run(torch.from_numpy(rng.uniform(-1, 1, (5, side, side, 3)).astype(np.float32)))
        torch.cuda.synchronize()
        ws = eng.workspace()
        print(f"net {what}: need {need} high {ws['scratch_high']} capacity {ws['scratch_cap']}")
        assert torch.isfinite(out).all() and 0 < need == ws["scratch_high"] <= ws["scratch_cap"]


def _ramp_frames():
    """3 frames of 96 x 64: horizontal grey ramps of contrast 1, 0.9 and 0.8.  On the synthetic weights PNet fires along a ramp: the
    CPU oracle (Oracle.detect, trace=True) counts 80 / 64 / 16 candidates at pyramid level 1 (120 cells) and 43 + 38 + 27 = 108
    stage-1 boxes -- more than a 64-slot level list, and more than an R-Net batch of 1 per frame + 64."""
    x = np.linspace(0, 255, 64)
    return np.stack([np.ascontiguousarray(np.broadcast_to(r.astype(np.uint8)[None, :, None], (96, 64, 3))) for r in (x, 10 + 0.9 * x, 30 + 0.8 * x)])


def test_cascade_arena_ends_at_its_count_and_reruns_deliver_the_same(make_engine):
    """Default capacities (one attempt), 64-slot lists (the call re-runs from stage 1 with a new layout) and an R-Net batch of 67
    (the call resumes at stage 2 on the lists it has)."""
    fr = _ramp_frames()
    outs = []
    for caps, t2 in (({}, 0.0), ({"cap_level": 64, "cap_frame": 64}, 0.0), ({}, 1.0)):
        eng = make_engine(**caps)
        eng.batch_capacity(t2, 0.0)
        out = eng.detect_embed(fr)
        attempts, ws = eng.list_stats()["attempts"], eng.workspace()
        print(f"{caps} t2 {t2}: attempts {attempts} {ws}")
        assert attempts > 1 if (caps or t2) else attempts == 1
        assert 0 < ws["arena_off"] == ws["arena_need"] <= ws["arena_cap"] and 0 < ws["scratch_high"] <= ws["scratch_cap"]
        again = eng.detect_embed(fr)
        ws2 = eng.workspace()
        assert ws2["arena_off"] == ws2["arena_need"] and ws2["scratch_high"] <= ws2["scratch_cap"]
        assert (ws2["arena_cap"], ws2["scratch_cap"]) == (ws["arena_cap"], ws["scratch_cap"])      # an equal batch grows nothing
        for k in out:
            assert torch.equal(out[k], again[k]), k
        outs.append(out)
    assert outs[0]["valid"].any()
    for o in outs[1:]:
        for k in o:
            assert torch.equal(outs[0][k], o[k]), k
