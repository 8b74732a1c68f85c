"""The embedder at map geometries other than the 80 / 160 px crops, on the CPU: the oracle's InceptionResnetV1 (orc_facenet) against
a float64 torch restatement (oracle/torch_ref.py) at square and non-square inputs whose block8 maps are 1x1, 2x2, 1x2, 2x1, 3x2,
1x9, 1x10 and 5x5, and facenet_geometry() -- every conv's output map in the library's walk order, which the GPU tests
(tests/test_gpu_embedder_sizes.py) use to check each plan row -- against the shapes torch's modules produce."""
import copy
from collections import namedtuple

import numpy as np
import pytest
import torch

# (h, w) of the faces: 75 is the smallest input the API takes; 112 gives block8 a 2x2 map, 139 x 107 a 3x2 one, 80 x 112 / 112 x 80
# 1x2 / 2x1, 80 x 362 / 80 x 363 1x9 (the last four-chain size) / 1x10, 224 a 5x5 one
GEOMETRIES = [(75, 75), (112, 112), (139, 107), (80, 112), (112, 80), (80, 362), (80, 363), (224, 224)]

# Measured on the geometries above and 80 / 160 px (2-3 faces each): max |oracle - float64 torch| 5.4e-7 per element.  The bound leaves 4x room; the
# f32 torch bound of test_oracle.py::test_networks_close_to_torch at 80 px is 1e-5.
F64_BOUND = 2e-6

_FUSED = {"repeat_1": ("branch0", "branch2.0", "branch1.0"), "repeat_2": ("branch0", "branch1.0"),
          "repeat_3": ("branch0", "branch1.0"), "block8": ("branch0", "branch1.0"), "mixed_7a": ("branch0.0", "branch1.0", "branch2.0")}


Conv = namedtuple("Conv", "layer OH OW K cin cout pad")


def _out(L, k, s, p):
    return (L + 2 * p - k) // s + 1


def facenet_geometry(h, w):
    """Every conv of the embedder on an h x w face, in the walk order of trl_run_facenet (the rows of Engine.facenet_plan()):
    a list of Conv(layer, OH, OW, K, cin, cout, pad) with K = kh * kw * cin.  Floor division throughout, like the layers."""
    rows = []

    def conv(name, H, W, cin, cout, kh, kw, s=1, ph=0, pw=0):
        OH, OW = _out(H, kh, s, ph), _out(W, kw, s, pw)
        rows.append(Conv("facenet." + name, OH, OW, kh * kw * cin, cin, cout, bool(ph or pw)))
        return OH, OW

    H, W = conv("conv2d_1a", h, w, 3, 32, 3, 3, 2)
    H, W = conv("conv2d_2a", H, W, 32, 32, 3, 3)
    H, W = conv("conv2d_2b", H, W, 32, 64, 3, 3, 1, 1, 1)
    H, W = _out(H, 3, 2, 0), _out(W, 3, 2, 0)                          # maxpool_3a
    H, W = conv("conv2d_3b", H, W, 64, 80, 1, 1)
    H, W = conv("conv2d_4a", H, W, 80, 192, 3, 3)
    H, W = conv("conv2d_4b", H, W, 192, 256, 3, 3, 2)
    for i in range(5):
        p = f"repeat_1.{i}."
        conv(p + "fused", H, W, 256, 96, 1, 1)
        for leaf in ("branch2.1", "branch1.1", "branch2.2"):
            conv(p + leaf, H, W, 32, 32, 3, 3, 1, 1, 1)
        conv(p + "conv2d", H, W, 96, 256, 1, 1)
    OH, OW = conv("mixed_6a.branch0", H, W, 256, 384, 3, 3, 2)
    conv("mixed_6a.branch1.0", H, W, 256, 192, 1, 1)
    conv("mixed_6a.branch1.1", H, W, 192, 192, 3, 3, 1, 1, 1)
    conv("mixed_6a.branch1.2", H, W, 192, 256, 3, 3, 2)
    H, W = OH, OW
    for i in range(10):
        p = f"repeat_2.{i}."
        conv(p + "fused", H, W, 896, 256, 1, 1)
        conv(p + "branch1.1", H, W, 128, 128, 1, 7, 1, 0, 3)
        conv(p + "branch1.2", H, W, 128, 128, 7, 1, 1, 3, 0)
        conv(p + "conv2d", H, W, 256, 896, 1, 1)
    conv("mixed_7a.fused", H, W, 896, 768, 1, 1)
    OH, OW = conv("mixed_7a.branch0.1", H, W, 256, 384, 3, 3, 2)
    conv("mixed_7a.branch1.1", H, W, 256, 256, 3, 3, 2)
    conv("mixed_7a.branch2.1", H, W, 256, 256, 3, 3, 1, 1, 1)
    conv("mixed_7a.branch2.2", H, W, 256, 256, 3, 3, 2)
    H, W = OH, OW
    for p in [f"repeat_3.{i}." for i in range(5)] + ["block8."]:
        conv(p + "fused", H, W, 1792, 384, 1, 1)
        conv(p + "branch1.1", H, W, 192, 192, 1, 3, 1, 0, 1)
        conv(p + "branch1.2", H, W, 192, 192, 3, 1, 1, 1, 0)
        conv(p + "conv2d", H, W, 384, 1792, 1, 1)
    conv("last_linear", 1, 1, 1792, 512, 1, 1)                         # after avgpool_1a
    return rows


def four_chain(OH, OW, K):
    """The oracle's rule (oracle/trl_oracle.c conv2d): four fmaf chains over the quarters of k when the map is tiny and K long."""
    return OH * OW <= 9 and K >= 512 and K % 16 == 0


@pytest.fixture(scope="module")
def f64_net(state_dicts):
    from oracle.torch_ref import TorchRef
    return copy.deepcopy(TorchRef(*state_dicts).facenet).double().eval()


@pytest.mark.parametrize("h,w", GEOMETRIES + [(150, 150), (171, 171), (80, 80), (160, 160)], ids=str)
def test_facenet_geometry_equals_torch_shapes(h, w, f64_net):
    """Every row of facenet_geometry has the output shape and reduction length of the torch module(s) it stands for (a fused 1x1
    row: each of its parts), and every torch conv is some row's."""
    shapes = {}
    hooks = [m.register_forward_hook(lambda m, i, o, name=name: shapes.__setitem__(name, (tuple(o.shape), m.weight[0].numel())))
             for name, m in f64_net.named_modules() if isinstance(m, (torch.nn.Conv2d, torch.nn.Linear))]
    try:
        with torch.no_grad():
            f64_net(torch.zeros(1, 3, h, w, dtype=torch.float64))
    finally:
        for hk in hooks:
            hk.remove()
    seen = set()
    for layer, OH, OW, K, _, cout, _ in facenet_geometry(h, w):
        name = layer[len("facenet."):]
        if name == "last_linear":
            parts = ["last_linear"]
        elif name.endswith(".fused"):
            blk = name[:-len(".fused")]
            parts = [f"{blk}.{q}.conv" for q in _FUSED[blk.split(".")[0]]]
        elif name.endswith(".conv2d"):
            parts = [name]
        else:
            parts = [name + ".conv"]
        for q in parts:
            shp, k = shapes[q]
            assert k == K and (shp[1] == cout or name.endswith(".fused")) and (shp[2:] == (OH, OW) if len(shp) == 4 else (OH, OW) == (1, 1)), (layer, q, shp, k, OH, OW, K)
            seen.add(q)
        assert sum(shapes[q][0][1] for q in parts) == cout, (layer, cout)
    assert seen == set(shapes), sorted(set(shapes) - seen)


@pytest.mark.parametrize("h,w", GEOMETRIES + [(80, 80), (160, 160)], ids=str)
def test_oracle_facenet_close_to_float64_torch(h, w, oracle, f64_net):
    x = np.random.default_rng(h * 1000 + w).uniform(0, 1, (3 if h * w < 20000 else 2, h, w, 3)).astype(np.float32)
    e = oracle.facenet(x)
    with torch.no_grad():
        ref = f64_net(torch.from_numpy(x).double().permute(0, 3, 1, 2)).numpy()
    err = np.abs(e.astype(np.float64) - ref).max(axis=1)
    assert (err <= F64_BOUND).all(), err
    assert np.allclose(np.linalg.norm(e.astype(np.float64), axis=1), 1.0, atol=1e-6)


def test_geometry_reaches_the_maps_it_is_meant_to():
    """The block8 maps the geometries above were chosen for, and the four-chain rule at the 1x9 / 1x10 pair."""
    b8 = {g: [(r.OH, r.OW) for r in facenet_geometry(*g) if r.layer == "facenet.block8.fused"][0] for g in GEOMETRIES}
    assert [b8[g] for g in GEOMETRIES] == [(1, 1), (2, 2), (3, 2), (1, 2), (2, 1), (1, 9), (1, 10), (5, 5)]
    assert four_chain(1, 9, 576) and not four_chain(1, 10, 576)
    assert facenet_geometry(75, 75)[6][1:3] == (7, 7)                 # conv2d_4b: the smallest block35 map
