"""The classifier head off the GPU: what the packer writes for `logits.weight` / `logits.bias`, that blobs without them keep
their bytes, and that tests/logits_ref.py -- the chain the device is held to bit for bit -- is a sound float32 evaluation of
feat @ W + b."""
import hashlib

import numpy as np
import pytest

import truely_amd
from truely_amd import weights
from logits_ref import K, blob_with_head, feature_table, gamma, head, logits_ref

# sha256 of synthetic_blob(0) as packed before the classifier existed (95 955 520 bytes)
SEED0_SHA256 = "8180357335893294c02123ed0530bc47b0ed619701342d14899884d58e151ed4"


@pytest.fixture(scope="module")
def sd33():
    return weights.synthetic_state_dicts(0, num_classes=33)


@pytest.fixture(scope="module")
def blob33(sd33):
    return weights.pack_state_dicts(*sd33)


def test_seed0_blob_keeps_its_bytes(blob):
    b = weights.synthetic_blob(0)
    assert len(b) == 95955520 and hashlib.sha256(b).hexdigest() == SEED0_SHA256
    assert b == blob
    assert "facenet.logits.w" not in weights.unpack_tensors(b)


def test_other_tensors_keep_their_bytes_beside_the_head(state_dicts, sd33, blob, blob33):
    for old, new in zip(state_dicts, sd33):
        assert [k for k in new if not k.startswith("logits.")] == list(old)
        for k in old:
            assert np.array_equal(np.asarray(old[k]), np.asarray(new[k])), k
    t0, t1 = weights.unpack_tensors(blob), weights.unpack_tensors(blob33)
    assert list(t1) == list(t0) + ["facenet.logits.w", "facenet.logits.b"]
    for k in t0:
        assert t0[k].shape == t1[k].shape and t0[k].tobytes() == t1[k].tobytes(), k


def test_round_trip_and_layout(sd33, blob33):
    t = weights.unpack_tensors(blob33)
    w, b = t["facenet.logits.w"], t["facenet.logits.b"]
    assert w.shape == (K, 33) and w.dtype == np.float32 and b.shape == (33,)
    lw = sd33[3]["logits.weight"]
    assert lw.shape == (33, K) and sd33[3]["logits.bias"].shape == (33,)
    for k, c in ((0, 0), (1, 0), (0, 1), (511, 32), (200, 17)):
        assert w[k][c] == lw[c][k]
    assert np.array_equal(w, lw.T) and np.array_equal(b, sd33[3]["logits.bias"])
    # the seeded scales: weight ~ N(0, 1/512), bias ~ 0.1 N(0, 1)
    big = weights.synthetic_logits(0, 4096)
    assert abs(float(big["logits.weight"].std()) * np.sqrt(512.0) - 1) < 0.01
    assert abs(float(big["logits.bias"].std()) / 0.1 - 1) < 0.05
    # a different class count draws from the same generator, a different seed from another
    assert not np.array_equal(weights.synthetic_logits(1, 33)["logits.bias"], sd33[3]["logits.bias"])


def test_test_side_blob_equals_the_packer(blob33):
    """blob_with_head (the GPU tests' contexts) is pack_state_dicts(*synthetic_state_dicts(0, num_classes=C))."""
    assert blob_with_head(33) == blob33
    w, b = head(33)
    t = weights.unpack_tensors(blob33)
    assert np.array_equal(t["facenet.logits.w"], w) and np.array_equal(t["facenet.logits.b"], b)


def test_pack_rules(state_dicts, sd33, blob, blob33):
    assert weights.pack_state_dicts(*sd33, include_logits=False) == blob
    assert weights.pack_state_dicts(*sd33, include_logits=True) == blob33
    assert weights.pack_state_dicts(*state_dicts, include_logits=True) == blob
    for drop in ("logits.weight", "logits.bias"):
        fn = {k: v for k, v in sd33[3].items() if k != drop}
        with pytest.raises(ValueError, match="logits"):
            weights.pack_state_dicts(sd33[0], sd33[1], sd33[2], fn)
        with pytest.raises(ValueError, match="logits"):
            weights.pack_state_dicts(sd33[0], sd33[1], sd33[2], fn, include_logits=False)
    fn = dict(sd33[3])
    fn["logits.weight"] = fn["logits.weight"][:, :511]
    with pytest.raises(ValueError):
        weights.pack_state_dicts(sd33[0], sd33[1], sd33[2], fn)


def _inputs():
    rng = np.random.default_rng(7)
    C = 37
    w = (rng.standard_normal((K, C)) * np.sqrt(1.0 / K)).astype(np.float32)
    b = (rng.standard_normal(C) * 0.1).astype(np.float32)
    onehot = np.zeros((4, K), np.float32)
    onehot[[0, 1, 2, 3], [0, 17, 255, 511]] = [1, -1, 0.5, 3]
    alt = np.ones((3, K), np.float32)
    alt[:, 1::2] = -1
    alt *= np.array([[1.0], [0.3], [1e4]], np.float32)
    return w, b, {
        "random": rng.standard_normal((6, K)).astype(np.float32),
        "one-hot": onehot,
        "all-equal": np.repeat(np.array([[1.0], [0.1], [-7.3]], np.float32), K, axis=1),
        "sign-alternating": alt,
    }


def test_reference_chain_against_float64():
    """|logits_ref - (feat @ W + b in float64)| <= gamma_513 (|b| + sum |x| |w|): the standard bound of a recursive sum of 512
    products and one addend, each step one rounding (an fma chain meets the bound of 513 roundings with room).  And the
    restatement is not numpy's float32 dot: on at least one input some element differs from it."""
    w, b, inputs = _inputs()
    w64, b64 = w.astype(np.float64), b.astype(np.float64)
    differs = False
    for name, x in inputs.items():
        got = logits_ref(x, w, b)
        assert got.dtype == np.float32 and got.shape == (len(x), w.shape[1])
        exact = x.astype(np.float64) @ w64 + b64
        bound = gamma(513) * (np.abs(b64) + np.abs(x.astype(np.float64)) @ np.abs(w64))
        err = np.abs(got.astype(np.float64) - exact)
        assert (err <= bound).all(), (name, float((err / bound).max()))
        naive = (np.dot(x, w) + b).astype(np.float32)
        differs |= bool((naive != got).any())
    assert differs
    # one-hot rows are one fma: fl(x w[k][c] + b[c]), a float64 sum of an exact product rounded once ... unless it is a tie
    oh = logits_ref(inputs["one-hot"][:1], w, b)[0]
    assert np.array_equal(oh, (w64[0] + b64).astype(np.float32))


def test_reference_is_the_sequential_chain():
    """Against a scalar evaluation in exact rational arithmetic rounded once per step."""
    from fractions import Fraction
    w, b, inputs = _inputs()
    x = inputs["random"][0]

    def rnd(fr):   # nearest-even float32 of a Fraction of ordinary magnitude: float64 first is safe only without a double
        d = float(fr)                      # rounding tie, so compare the two float32 neighbours exactly
        f = np.float32(d)
        lo, hi = np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))
        best = min((lo, f, hi), key=lambda v: (abs(Fraction(float(v)) - fr), int(np.float32(v).view(np.uint32)) & 1))
        return np.float32(best)

    for c in (0, 36):
        acc = np.float32(b[c])
        for k in range(K):
            acc = rnd(Fraction(float(x[k])) * Fraction(float(w[k][c])) + Fraction(float(acc)))
        assert logits_ref(x[None], w, b)[0, c] == acc


def test_reference_on_non_finite_rows():
    """Rows holding inf / NaN follow IEEE classes; the other rows are untouched by them."""
    w, b = head(33)
    f = feature_table()
    r = logits_ref(f[:8], w, b)
    assert np.isnan(r[4]).all()                                    # NaN at k = 511
    fin = np.isfinite(r[3])
    assert not fin.any()                                           # +inf at k = 7 and -inf at k = 300
    same_sign = np.sign(w[7]) == -np.sign(w[300])                  # inf * w7 and -inf * w300 agree in sign: stays infinite
    assert np.array_equal(np.isinf(r[3]), same_sign) and np.array_equal(np.isnan(r[3]), ~same_sign)
    assert np.array_equal(r[0], logits_ref(f[:1], w, b)[0])
    assert np.array_equal(r[1], b)                                 # a row of zeros leaves the bias
    assert np.array_equal(r[2], (w[0].astype(np.float64) + b).astype(np.float32))
