"""InceptionResnetV1(classify=True) on the device: trl_facenet_logits against tests/logits_ref.py bit for bit, trl_facenet_features
against the embedder, the loader's rules for the two classifier tensors, the refusals, and the Python layer.

The kernel (trl_logits.hip) tiles rows by 32 and classes by 32 per wave / 128 per workgroup, so the small table sits on both sides
of every edge: C in {1, 31, 32, 33, 95, 257} (a lone column, a slab short of / equal to / past 32, three slabs with a partial one,
two workgroups and a lone column in the third), n in {1, 2, 16, 17, 31, 32, 33, 65} (the 16-row kernel up to n = 16, the 32-row
kernel past it: a partial tile, a full one, two and three tiles; test_row_invariance sets one against the other), the
output rows ld = C and ld = C + 5 apart, the features at a 16-byte and at a 4-byte aligned address (the tile fill has a path for
each).  The two production class counts run at n = 1 and n = 33."""
import ctypes as C_

import numpy as np
import pytest
import torch

import truely_amd
from truely_amd import _lib
from logits_ref import N_TABLE, blob_with_head, feature_table, head, logits_ref, same_bits, table_ref

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000
SMALL_C = (1, 31, 32, 33, 95, 257)
SMALL_N = (1, 2, 16, 17, 31, 32, 33, 65)
TRL_ERR_INVALID, TRL_ERR_WEIGHTS, TRL_ERR_STATE = -1, -3, -5


def _ptr(t):
    return C_.c_void_p(t.data_ptr() if t is not None else 0)


@pytest.fixture(scope="module")
def heads():
    """Engines by (classes, precision), built on first use from synthetic_state_dicts(0, num_classes=C)'s blob."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from truely_amd.engine import Engine
    made = {}

    def get(C, precision="f32"):
        if (C, precision) not in made:
            made[(C, precision)] = Engine(blob_with_head(C), embed_precision=precision)
        return made[(C, precision)]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def faces():
    return np.random.default_rng(1080).uniform(0, 1, (9, 80, 80, 3)).astype(np.float32)


def _dev_features(eng, rows: np.ndarray, misalign: bool = False) -> torch.Tensor:
    """rows on the device; misalign: at an address that is 4 but not 16 bytes aligned."""
    if not misalign:
        return torch.from_numpy(np.array(rows, np.float32)).to(eng.device)
    big = torch.zeros(rows.size + 8, dtype=torch.float32, device=eng.device)
    v = big[1:1 + rows.size]
    v.copy_(torch.from_numpy(np.array(rows, np.float32)).reshape(-1))
    assert v.data_ptr() % 16 == 4
    return v


def _raw_logits(eng, feat_t, n, ld, out_rows=None, null_out=False, null_feat=False):
    """trl_facenet_logits into the middle of a NaN-filled buffer with a guard row on either side: (status, buffer as uint32)."""
    rows = max(n, 1) if out_rows is None else out_rows
    buf = torch.full((rows + 2, max(ld, 1)), float("nan"), dtype=torch.float32, device=eng.device)
    st = eng.lib.trl_facenet_logits(eng._h, _ptr(None if null_feat else feat_t), n, _ptr(None if null_out else buf[1]), ld, eng._stream())
    torch.cuda.synchronize()
    return st, buf.cpu().numpy().view(np.uint32)


def _check_call(eng, rows, C, ld, ref, misalign=False):
    n = len(rows)
    st, bits = _raw_logits(eng, _dev_features(eng, rows, misalign), n, ld)
    assert st == 0, _lib.load().trl_last_error()
    assert (bits[0] == NAN_BITS).all() and (bits[-1] == NAN_BITS).all(), "guard row written"
    assert (bits[1:-1, C:] == NAN_BITS).all(), "guard columns written"
    got = bits[1:-1, :C].view(np.float32)
    ok = same_bits(got, ref)
    assert ok.all(), f"C={C} n={n} ld={ld}: {int((~ok).sum())} elements differ, first at {np.argwhere(~ok)[0]}"
    return got


@pytest.mark.parametrize("C", SMALL_C)
def test_small_table(heads, C):
    eng = heads(C)
    assert eng.num_classes == C
    f, ref = feature_table(), table_ref(C)
    for n in SMALL_N:
        for ld in (C, C + 5):
            _check_call(eng, f[:n], C, ld, ref[:n])
    _check_call(eng, f[:33], C, C + 5, ref[:33], misalign=True)
    # rows that start inside the table: the special rows also as row 0 of a call
    _check_call(eng, f[2:7], C, C, ref[2:7])


@pytest.mark.parametrize("C", (8631, 10575))
def test_production_class_counts(heads, C):
    eng = heads(C)
    assert eng.num_classes == C
    f, ref = feature_table(), table_ref(C, 33)
    _check_call(eng, f[:1], C, C, ref[:1])
    _check_call(eng, f[:33], C, C + 5, ref[:33])


@pytest.mark.parametrize("C", (95, 257))
def test_row_invariance(heads, C):
    """Row r of the 65-row call has the bits of the same row computed alone: no dependence on n, tile or position."""
    eng = heads(C)
    f = feature_table()
    whole = _check_call(eng, f, C, C, table_ref(C))
    for r in range(N_TABLE):
        st, bits = _raw_logits(eng, _dev_features(eng, f[r:r + 1]), 1, C)
        assert st == 0
        assert same_bits(bits[1, :C].view(np.float32), whole[r]).all(), r


def test_engine_logits_matches_raw_call(heads):
    eng = heads(33)
    got = eng.facenet_logits(torch.from_numpy(feature_table()[:33].copy()))
    assert got.shape == (33, 33) and got.device.type == "cuda"
    assert same_bits(got.cpu().numpy(), table_ref(33)[:33]).all()


def _unit(feat):
    f = feat.astype(np.float64)
    return f / np.maximum(np.sqrt((f * f).sum(axis=1, keepdims=True)), 1e-12)


def test_features(heads, faces):
    """trl_facenet_features is the walk in front of F.normalize: normalised in float64 it is the embedding to within 1e-6 (the
    device's normalisation costs a few units of 2^-24 on values of magnitude <= 1), masked rows are zero, and the embedder's own
    results keep their bits around it -- also over poisoned workspaces and on a side stream."""
    eng = heads(33)
    x1, x9 = torch.from_numpy(faces[:1]), torch.from_numpy(faces)
    valid = torch.tensor([1, 1, 1, 1, 0, 1, 1, 1, 1], dtype=torch.uint8)
    emb_before = eng.facenet_embed(x9).cpu().numpy()
    f1 = eng.facenet_features(x1).cpu().numpy()
    f9 = eng.facenet_features(x9, valid).cpu().numpy()
    plan = eng.facenet_plan()                                      # the plan hook sees the call like an embedder call
    assert plan[-1]["layer"] == "facenet.last_linear" and plan[-1]["m"] == 9
    emb_after = eng.facenet_embed(x9).cpu().numpy()
    assert np.array_equal(emb_before.view(np.uint32), emb_after.view(np.uint32))
    assert f1.shape == (1, 512) and f9.shape == (9, 512)
    assert np.isfinite(f9).all() and not f9[4].any() and (np.abs(f9[[0, 1, 2, 3, 5, 6, 7, 8]]).max(axis=1) > 0).all()
    live = valid.numpy().astype(bool)
    assert np.abs(_unit(f1) - emb_before[:1]).max() <= 1e-6
    assert np.abs(_unit(f9[live]) - emb_before[live]).max() <= 1e-6
    masked = eng.embed_faces(x9, valid).cpu().numpy()
    assert not masked[4].any() and np.abs(_unit(f9[live]) - masked[live]).max() <= 1e-6
    eng.poison_workspaces(0xFF)
    side = torch.cuda.Stream(device=eng.device)
    with torch.cuda.stream(side):
        g9 = eng.facenet_features(x9, valid)
        lg = eng.facenet_logits(g9)
        side.synchronize()
    assert np.array_equal(g9.cpu().numpy().view(np.uint32), f9.view(np.uint32))
    w, b = head(33)
    assert same_bits(lg.cpu().numpy(), logits_ref(f9, w, b)).all()
    assert np.array_equal(eng.facenet_embed(x9).cpu().numpy().view(np.uint32), emb_before.view(np.uint32))


@pytest.mark.parametrize("precision", ("bf16", "fp16"))
def test_reduced_precision_head_stays_f32(heads, faces, precision):
    eng = heads(33, precision)
    feat = eng.facenet_features(torch.from_numpy(faces[:3]))
    got = eng.facenet_logits(feat).cpu().numpy()
    w, b = head(33)
    f = feat.cpu().numpy()
    assert np.isfinite(f).all() and np.abs(f).max() > 0
    assert same_bits(got, logits_ref(f, w, b)).all()


def test_blob_without_logits(engine):
    assert engine.num_classes == 0
    feat = torch.zeros((2, 512), dtype=torch.float32, device=engine.device)
    st, bits = _raw_logits(engine, feat, 2, 8)
    assert st == TRL_ERR_WEIGHTS and b"no logits layer" in _lib.load().trl_last_error()
    assert (bits == NAN_BITS).all()
    with pytest.raises(_lib.TrlError):
        engine.facenet_logits(feat)


def _refused_load(blob, names):
    """A fresh context refuses `blob` naming one of `names`, and then has no weights."""
    lib = _lib.load()
    cfg = _lib.TrlConfig()
    assert lib.trl_default_config(C_.byref(cfg)) == 0
    cfg.device = torch.cuda.current_device()
    h = C_.c_void_p()
    assert lib.trl_create(C_.byref(cfg), C_.byref(h)) == 0
    try:
        assert lib.trl_load_weights(h, blob, len(blob)) == TRL_ERR_WEIGHTS
        msg = lib.trl_last_error().decode()
        assert any(nm in msg for nm in names), msg
        x = torch.zeros((1, 80, 80, 3), dtype=torch.float32, device="cuda")
        out = torch.zeros((1, 512), dtype=torch.float32, device="cuda")
        assert lib.trl_facenet_embed(h, _ptr(x), 1, 80, 80, _ptr(out), None) == TRL_ERR_STATE
        assert b"without weights" in lib.trl_last_error()
        c = C_.c_int(-1)
        assert lib.trl_facenet_num_classes(h, C_.byref(c)) == TRL_ERR_STATE
        assert lib.trl_facenet_logits(h, _ptr(out), 1, _ptr(out), 512, None) == TRL_ERR_STATE
    finally:
        lib.trl_destroy(h)


def test_loader_refuses_misshaped_heads():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from truely_amd import weights
    w, b = head(33)
    _refused_load(blob_with_head(33, w=w[:511]), ["facenet.logits.w"])
    _refused_load(blob_with_head(33, b=np.concatenate([b, b[:1]])), ["facenet.logits.b"])
    _refused_load(blob_with_head(33, w=w.reshape(-1)), ["facenet.logits.w"])
    t = weights.unpack_tensors(blob_with_head(33))
    for drop in ("facenet.logits.w", "facenet.logits.b"):
        _refused_load(weights.pack_tensors({k: v for k, v in t.items() if k != drop}), [drop])


def test_refusals(heads):
    eng = heads(33)
    feat = _dev_features(eng, feature_table()[:4])
    lib = _lib.load()
    for kw, n, ld in (({}, 4, 32), ({}, 0, 33), ({}, -1, 33), ({"null_out": True}, 4, 33), ({"null_feat": True}, 4, 33)):
        st, bits = _raw_logits(eng, feat, n, ld, out_rows=4, **kw)
        assert st == TRL_ERR_INVALID, (kw, n, ld)
        assert (bits == NAN_BITS).all()
    assert lib.trl_facenet_num_classes(eng._h, None) == TRL_ERR_INVALID
    assert lib.trl_facenet_logits(None, _ptr(feat), 4, _ptr(feat), 33, None) == TRL_ERR_STATE
    # a call in flight owns the context
    frames = truely_amd.synthetic.synthetic_frames(2, 180, 320, seed=3)
    x = torch.zeros((1, 80, 80, 3), dtype=torch.float32, device=eng.device)
    out = torch.zeros((1, 512), dtype=torch.float32, device=eng.device)
    eng.detect_embed_begin(frames)
    try:
        st, bits = _raw_logits(eng, feat, 4, 33)
        assert st == TRL_ERR_STATE and (bits == NAN_BITS).all()
        assert lib.trl_facenet_features(eng._h, _ptr(x), None, 1, 80, 80, _ptr(out), eng._stream()) == TRL_ERR_STATE
    finally:
        eng.detect_embed_end()
    st, bits = _raw_logits(eng, feat, 4, 33)
    assert st == 0 and same_bits(bits[1:5, :33].view(np.float32), table_ref(33)[:4]).all()


def test_python_layer(heads, engine, faces):
    from truely_amd.inception_resnet_v1 import InceptionResnetV1
    eng = heads(33)
    x = torch.from_numpy(faces[:3]).permute(0, 3, 1, 2).contiguous()           # (n, 3, H, W), on the CPU
    model = InceptionResnetV1(pretrained="vggface2", classify=True, engine=eng, dropout_prob=0.5).eval()
    assert model.num_classes == 33
    y = model(x)
    assert y.shape == (3, 33) and y.device.type == "cpu" and y.dtype == torch.float32
    want = eng.facenet_logits(eng.facenet_features(torch.from_numpy(faces[:3])))
    assert np.array_equal(y.numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))
    yc = model(x.to(eng.device))
    assert yc.device.type == "cuda" and torch.equal(yc.cpu(), y)
    emb = eng.facenet_embed(torch.from_numpy(faces[:3])).cpu()
    model.classify = False
    assert torch.equal(model(x), emb)
    model.classify = True
    assert torch.equal(model(x), y)
    plain = InceptionResnetV1(pretrained="vggface2", engine=eng)
    assert plain.classify is False and torch.equal(plain(x), emb)
    assert InceptionResnetV1(classify=True, num_classes=33, engine=eng).num_classes == 33
    with pytest.raises(ValueError, match="num_classes"):
        InceptionResnetV1(classify=True, num_classes=8631, engine=eng)
    with pytest.raises(ValueError, match="TRUELY_WEIGHTS"):
        InceptionResnetV1(classify=True, engine=engine)
    late = InceptionResnetV1(engine=engine)
    assert torch.equal(late(x), engine.facenet_embed(torch.from_numpy(faces[:3])).cpu())
    late.classify = True
    with pytest.raises(ValueError, match="synthetic_state_dicts"):
        late(x)
