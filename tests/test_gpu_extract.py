"""Face extraction on the GPU (csrc/trl_extract.hip, Engine.extract_faces, MTCNN.forward) against the restatement
tests/extract_ref.py: the kernel byte for byte in f32 for every resampler, margins 0 / 20 / 44, boxes over every frame edge,
multi-face batches; k_crop_area_std through the oracle; detect's detection order; every selection method; MTCNN(img) for
numpy / tensor / PIL, single and batch, keep_all both ways and return_prob; resnet(mtcnn(img)) == facenet_embed of the crop."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import extract_ref as R
import truely_amd
from truely_amd import _lib

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _multiface():
    z = np.load(os.path.join(GOLD, "clip_multiface_270p.npz"))
    return truely_amd.synthetic.synthetic_frames(int(z["n"]), int(z["H"]), int(z["W"]), seed=int(z["seed"]), faces=int(z["faces_per_frame"]))


def _rows(engine, fr):
    """every detected face of every frame (detect's area order) + hand-made boxes over every frame edge and one empty crop"""
    n, H, W, _ = fr.shape
    b, _p, c = (t.cpu().numpy() for t in engine.mtcnn_detect(fr))
    rows, boxes = [], []
    for i in range(n):
        for k in range(int(c[i])):
            rows.append(i); boxes.append(b[i, k])
    edge = [[-12.5, -7.25, 40.5, 33.75], [W - 30.25, -4.5, W + 9.5, 28.0], [-3.0, H - 25.5, 31.75, H + 6.25],
            [W - 41.5, H - 38.0, W + 2.5, H + 11.0], [-20.0, -20.0, W + 20.0, H + 20.0], [5.2, 7.9, 6.1, 40.3],
            [W + 3.0, 10.0, W + 30.0, 40.0]]                          # the last: right of the frame -> empty crop
    for j, e in enumerate(edge):
        rows.append(j % n); boxes.append(np.array(e, np.float32))
    rows.append(-1); boxes.append(np.array([1, 1, 20, 20], np.float32))   # no frame: zeros
    return np.array(rows, np.int32), np.array(boxes, np.float32)


@pytest.mark.parametrize("clip", ["multiface", "faces5"])
@pytest.mark.parametrize("resample", R.RESAMPLERS)
def test_extraction_kernel_equals_restatement(engine, clip, resample):
    fr = _multiface() if clip == "multiface" else truely_amd.synthetic.synthetic_frames(3, 180, 320, seed=7, faces=-1)
    n, H, W, _ = fr.shape
    rows, boxes = _rows(engine, fr)
    assert (rows >= 0).sum() - 7 >= n                                   # real faces as well as the hand-made boxes
    for S, margin, post in [(160, 0, True), (160, 20, False), (160, 44, True), (112, 20, True), (161, 0, False)]:
        faces, status = engine.extract_boxes(fr, torch.from_numpy(rows), torch.from_numpy(boxes), S, margin, resample, post)
        faces, status = faces.cpu().numpy(), status.cpu().numpy()
        assert faces.shape == (len(rows), 3, S, S)
        for r in range(len(rows)):
            if rows[r] < 0:
                assert status[r] == 0 and not faces[r].any()
                continue
            try:
                ref = R.extract(fr[rows[r]], boxes[r], S, margin, resample, post).transpose(2, 0, 1)
            except ValueError:
                assert status[r] == -1 and not faces[r].any(), r
                continue
            assert status[r] == 1
            assert np.array_equal(faces[r], ref), (S, margin, r, int((faces[r] != ref).sum()))


def test_torch_margin0_equals_oracle_crop_area_std(engine, oracle):
    fr = _multiface()
    rows, boxes = _rows(engine, fr)
    faces, status = engine.extract_boxes(fr, torch.from_numpy(rows), torch.from_numpy(boxes), 160, 0, "torch", True)
    faces, status = faces.cpu().numpy(), status.cpu().numpy()
    seen = 0
    for r in np.nonzero(status == 1)[0]:
        rect = R.crop_box(boxes[r], 160, 0, fr.shape[2], fr.shape[1])
        ref = oracle.crop_area_std(fr[rows[r]], rect, 160, rgb=False).transpose(2, 0, 1)
        assert np.array_equal(faces[r], ref), r
        seen += 1
    assert seen >= 6


def test_detect_in_detection_order_equals_stage3_rows(engine, oracle):
    from truely_amd.mtcnn import MTCNN
    m = MTCNN(engine=engine, select_largest=False)
    seen = 0
    for fr in (_multiface(), truely_amd.synthetic.synthetic_frames(2, 180, 320, seed=7, faces=-1)):
        seen += _detection_order(engine, oracle, m, fr)
    assert seen >= 6


def _detection_order(engine, oracle, m, fr):
    b, p, c = (t.cpu().numpy() for t in engine.mtcnn_detect(fr, select_largest=False))
    seen = 0
    for i in range(len(fr)):
        _b, _p, tr = oracle.detect(fr[i], trace=True)
        b3 = tr["boxes3"][:engine.cfg.max_faces]
        assert int(c[i]) == len(b3)
        assert np.array_equal(b[i, :len(b3)], b3[:, :4]) and np.array_equal(p[i, :len(b3)], b3[:, 4])
        bb, pp = m.detect(fr[i])
        if len(b3):
            assert np.array_equal(bb, b3[:, :4]) and np.array_equal(pp, b3[:, 4])
        seen += len(b3)
    # select_largest=True keeps the area order: the same rows, sorted by area
    b0, _p0, c0 = (t.cpu().numpy() for t in engine.mtcnn_detect(fr))
    assert np.array_equal(c0, c)
    for i in range(len(fr)):
        k = int(c[i])
        area = (b[i, :k, 2] - b[i, :k, 0]) * (b[i, :k, 3] - b[i, :k, 1])
        assert np.array_equal(b0[i, :k], b[i, :k][np.argsort(area, kind="stable")[::-1]])
    return seen


def test_selection_methods_on_hand_made_lists(engine):
    mf = engine.cfg.max_faces
    lists = [
        ([[0, 0, 10, 10], [20, 20, 30, 30], [5, 5, 12, 12], [40, 40, 50, 50]], [0.95, 0.99, 0.99, 0.91]),   # area / prob ties
        ([[0, 0, 10, 10], [40, 40, 50, 50]], [0.95, 0.97]),                       # mirror images about the centre (25, 25)
        ([[1, 1, 30, 30], [2, 2, 8, 8]], [0.9, 0.5]),                             # nothing over 0.9 (f32)
        ([[3, 4, 20.5, 19.25], [10, 10, 40, 40], [12, 14, 44, 47], [0, 0, 2, 2]], [0.93, 0.91, 0.995, 0.999]),
        ([], []),
    ]
    n = len(lists)
    boxes = np.zeros((n, mf, 4), np.float32); probs = np.zeros((n, mf), np.float32); counts = np.zeros(n, np.int32)
    for i, (b, p) in enumerate(lists):
        counts[i] = len(b)
        if b:
            boxes[i, :len(b)], probs[i, :len(b)] = b, p
    for method in R.METHODS:
        pick = engine.select_faces(torch.from_numpy(boxes), torch.from_numpy(probs), torch.from_numpy(counts), 50, 50, method).cpu().numpy()
        for i, (b, p) in enumerate(lists):
            ref = R.select(np.array(b, np.float32).reshape(-1, 4), np.array(p, np.float32), method, 50, 50)
            assert pick[i] == (-1 if ref is None else ref), (method, i)


@pytest.mark.parametrize("method", R.METHODS)
def test_selection_methods_on_real_frames(engine, method):
    from truely_amd.mtcnn import MTCNN
    for fr, sl in [(_multiface(), True), (_multiface(), False), (truely_amd.synthetic.synthetic_frames(3, 180, 320, seed=7, faces=-1), False)]:
        m = MTCNN(engine=engine, select_largest=sl, selection_method=method)
        b, p = m.detect(fr)
        out = m(fr, return_prob=True)
        for i in range(len(fr)):
            ref = R.forward(fr[i], b[i], p[i], method=method, resample="cv2", return_prob=True)
            if ref[0] is None:
                assert out[0][i] is None and out[1][i] is None
            else:
                assert np.array_equal(out[0][i].numpy(), ref[0]) and out[1][i] == ref[1]


def _check(got, ref, keep_all):
    if ref is None:
        assert got is None
        return
    assert isinstance(got, torch.Tensor) and got.device.type == "cpu" and tuple(got.shape) == ref.shape
    assert np.array_equal(got.numpy(), ref)


@pytest.mark.parametrize("kind", ["numpy", "tensor", "pil"])
@pytest.mark.parametrize("keep_all", [False, True])
def test_mtcnn_call_matches_restatement(engine, kind, keep_all):
    from truely_amd.mtcnn import MTCNN
    fr = np.concatenate([_multiface(), np.full((1, 270, 480, 3), 128, np.uint8)])     # the last frame holds no face
    resample = {"numpy": "cv2", "tensor": "torch", "pil": "pil"}[kind]
    conv = {"numpy": lambda a: a, "tensor": torch.from_numpy, "pil": Image.fromarray}[kind]
    m = MTCNN(engine=engine, keep_all=keep_all, margin=14, image_size=150)
    b, p = m.detect(fr)
    refs = [R.forward(fr[i], b[i], p[i], S=150, margin=14, resample=resample, keep_all=keep_all, return_prob=True) for i in range(len(fr))]
    assert refs[0][0] is not None and refs[-1][0] is None
    for i in range(len(fr)):                                                         # single images
        face, prob = m(conv(fr[i]), return_prob=True)
        _check(face, refs[i][0], keep_all)
        if refs[i][0] is None:
            assert (prob == [None]) if keep_all else (prob is None)
        elif keep_all:
            assert np.array_equal(prob, refs[i][1])
        else:
            assert np.ndim(prob) == 0 and prob == refs[i][1]
        _check(m(conv(fr[i])), refs[i][0], keep_all)
    batch = torch.from_numpy(fr) if kind == "tensor" else (fr if kind == "numpy" else [Image.fromarray(f) for f in fr])
    faces = m(batch)                                                                 # a batch gives a list
    assert isinstance(faces, list) and len(faces) == len(fr)
    for i in range(len(fr)):
        _check(faces[i], refs[i][0], keep_all)


def test_mtcnn_not_callable_before_is_now(engine):
    from truely_amd.mtcnn import MTCNN
    fr = _multiface()
    face = MTCNN(engine=engine)(fr[0])
    assert tuple(face.shape) == (3, 160, 160) and face.dtype == torch.float32
    with pytest.raises(NotImplementedError):
        MTCNN(engine=engine)(fr[0], save_path="x.png")


def test_engine_extract_faces_keep_all_compacts_on_device(engine):
    fr = _multiface()
    out = engine.extract_faces(fr, keep_all=True, resample="torch")
    counts = out["counts"].cpu().numpy()
    assert out["faces"].is_cuda and out["faces"].shape[0] == counts.sum() and counts.min() >= 2
    assert np.array_equal(out["frame"].cpu().numpy(), np.repeat(np.arange(len(fr)), counts))
    one = engine.extract_faces(fr)
    assert one["valid"].cpu().numpy().all() and tuple(one["faces"].shape) == (len(fr), 3, 160, 160)
    assert one["faces"].permute(0, 2, 3, 1).is_contiguous()                         # NHWC storage: what the embedder reads


def test_resnet_of_mtcnn_equals_facenet_embed(engine):
    from truely_amd.inception_resnet_v1 import InceptionResnetV1
    from truely_amd.mtcnn import MTCNN
    fr = _multiface()
    face = MTCNN(engine=engine)(torch.from_numpy(fr[0]))
    resnet = InceptionResnetV1(engine=engine)
    emb = resnet(face.unsqueeze(0))
    ref = engine.facenet_embed(face.unsqueeze(0).permute(0, 2, 3, 1).contiguous())
    assert np.array_equal(np.asarray(emb.cpu() if isinstance(emb, torch.Tensor) else emb), ref.cpu().numpy())


def test_extract_refuses_a_context_with_a_call_in_flight(engine):
    fr = truely_amd.synthetic.synthetic_frames(2, 180, 320, seed=3)
    eng = engine.clone()
    try:
        eng.detect_embed_begin(fr)
        with pytest.raises(_lib.TrlError) as e:
            eng.extract_boxes(fr, torch.tensor([0], dtype=torch.int32), torch.tensor([[10, 10, 60, 60]], dtype=torch.float32))
        assert e.value.status == -5
        with pytest.raises(_lib.TrlError):
            eng.select_faces(torch.zeros(2, eng.cfg.max_faces, 4), torch.zeros(2, eng.cfg.max_faces), torch.zeros(2, dtype=torch.int32), 180, 320)
        eng.detect_embed_end()
    finally:
        eng.close()


def test_extract_argument_checks(engine):
    fr = truely_amd.synthetic.synthetic_frames(1, 180, 320, seed=3)
    rows, box = torch.tensor([0], dtype=torch.int32), torch.tensor([[10, 10, 60, 60]], dtype=torch.float32)
    for S, margin in [(0, 0), (1025, 0), (160, 160), (160, -1)]:
        with pytest.raises(_lib.TrlError):
            engine.extract_boxes(fr, rows, box, S, margin)
    faces, status = engine.extract_boxes(fr, rows, box, 1, 0, "pil")
    assert tuple(faces.shape) == (1, 3, 1, 1) and int(status[0]) == 1
    assert np.array_equal(faces.cpu().numpy()[0].transpose(1, 2, 0), R.extract(fr[0], [10, 10, 60, 60], 1, 0, "pil"))
