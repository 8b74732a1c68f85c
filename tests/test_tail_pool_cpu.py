"""The geometry of the pooling epilogue (csrc/trl_tailpool.h), without a GPU.

R-Net conv2 and O-Net conv2 / conv3 reduce their max pool inside the conv kernel: a tile of 128 flattened (candidate, y, x) rows
reduces the part of every pooling window it holds, the tile with a window's first element writes the pooled map, a second tile
writes a side buffer, and a fix-up kernel combines the two where a window meets a tile boundary.  The kernels, the fix-up and
``tests/tail_pool_sim.cpp`` take the cell ranges and the first / second / straddle predicates from the one header; this module
restates them by brute force over the rows themselves:

- launches long enough that a tile starts at every offset modulo the candidate size the layer can produce, plus an unfinished
  last tile;
- every window element is reduced by exactly one tile, no cell has more than two parts, the second-part flag is "the first
  element lies in an earlier tile", and the fix-up's cells are exactly the cells with two parts, each once;
- a numpy emulation of "part, part, combine" with maxpool_kernel's comparison has the bits of the sequential scan, on random
  data and on data full of +0, -0, NaN and infinities.
"""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from truely_amd import jpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(jpeg.__file__), "csrc")
BM = 128
# (layer, conv output side, pool window, pool stride): trl_nets[] in csrc/trl_nets.hip
LAYERS = [("rnet.conv2", 9, 3, 2), ("onet.conv2", 21, 3, 2), ("onet.conv3", 8, 2, 2)]


def launches(S):
    """Candidate counts: every tile offset modulo S*S that multiples of BM reach (lcm / per candidates), then three more so that
    the last tile is unfinished, and a launch of one tile or less."""
    per = S * S
    full = BM // math.gcd(per, BM)
    return sorted({1, full, full + 3})


@pytest.fixture(scope="module")
def sim_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("tail_pool_sim") / "tail_pool_sim")
    base = [cxx, "-O1", "-g", "-std=c++17", "-I", CSRC, os.path.join(ROOT, "tests", "tail_pool_sim.cpp"), "-o", out]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(base + san, capture_output=True, text=True).returncode != 0:
        subprocess.run(base, check=True)
    return out


def run_sim(program, S, k, st, N, bm=BM):
    r = subprocess.run([program, str(S), str(k), str(st), str(bm), str(N)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = dict(tiles=[], cuts=[])
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "geom":
            out["geom"] = [int(x) for x in w[1:]]
        elif w[0] in ("first", "straddles"):
            out[w[0]] = np.array(w[1:], np.int64)
        elif w[0] == "tile":
            out["tiles"].append((int(w[1]), int(w[2]), int(w[3]), [int(x) for x in w[4:]]))
        elif w[0] == "cut":
            out["cuts"].append((int(w[1]), int(w[2]), int(w[3])))
    return out


def window_rows(S, k, st, N):
    """[cells][k*k] rows of every pooling window in scan order (ky, then kx), by the definition of the pool."""
    P = (S - k) // st + 1
    n, py, px, ky, kx = np.meshgrid(np.arange(N), np.arange(P), np.arange(P), np.arange(k), np.arange(k), indexing="ij")
    rows = n * S * S + (py * st + ky) * S + (px * st + kx)
    return rows.reshape(N * P * P, k * k)


@pytest.fixture(scope="module")
def sims(sim_program):
    return {(layer, N): (run_sim(sim_program, S, k, st, N), window_rows(S, k, st, N)) for layer, S, k, st in LAYERS for N in launches(S)}


@pytest.mark.parametrize("layer,S,k,st", LAYERS)
def test_geometry_constants(sim_program, layer, S, k, st):
    P = (S - k) // st + 1
    g = run_sim(sim_program, S, k, st, 1)["geom"]
    assert g == [P, S * S, P * P, (k - 1) * S + k, 1, int(BM % (S * S) != 0)]
    assert P == -(-(S - k) // st) + 1                     # the ceil-mode pool clips no window of these layers
    assert {"rnet.conv2": 21, "onet.conv2": 45, "onet.conv3": 10}[layer] == g[3] <= BM


def test_refused_geometries(sim_program):
    """A clipped window, a window longer than a tile: ok() is false (the walker then issues conv and pool separately)."""
    assert run_sim(sim_program, 10, 3, 2, 1)["geom"][4] == 0          # (10 - 3) % 2 != 0
    assert run_sim(sim_program, 70, 3, 2, 1)["geom"][4] == 0          # span 143 > 128
    assert run_sim(sim_program, 21, 3, 2, 1, bm=32)["geom"][4] == 0   # span 45 > 32
    assert run_sim(sim_program, 63, 3, 2, 1)["geom"][4] == 0          # span 2 * 63 + 3 = 129 > 128
    assert run_sim(sim_program, 61, 3, 2, 1)["geom"][4] == 1          # span 125


@pytest.mark.parametrize("layer,S,k,st", LAYERS)
def test_every_tile_offset_is_reached(layer, S, k, st):
    per = S * S
    N = max(launches(S))
    offsets = {(t * BM) % per for t in range(-(-N * per // BM))}
    assert offsets == {o for o in range(per) if o % math.gcd(per, BM) == 0}
    assert (N * per) % BM != 0 or layer == "onet.conv3"


@pytest.mark.parametrize("layer,S,k,st", LAYERS)
def test_parts_cover_every_window_element_once(sims, layer, S, k, st):
    for N in launches(S):
        sim, rows = sims[(layer, N)]
        assert np.array_equal(sim["first"], rows[:, 0])
        assert len(sim["tiles"]) == -(-N * S * S // BM)
        taken = np.zeros(rows.shape, np.int64)            # how many tiles reduced this window element
        parts = np.zeros(len(rows), np.int64)
        for t, g0, g1, second in sim["tiles"]:
            inside = (rows >= t * BM) & (rows < (t + 1) * BM)
            touched = np.flatnonzero(inside.any(axis=1))
            assert touched.tolist() == list(range(g0, g1)), (layer, N, t)   # the tile's range is exactly the cells it holds part of
            taken += inside
            parts[g0:g1] += 1
            assert second == (rows[g0:g1, 0] < t * BM).astype(int).tolist(), (layer, N, t)
        assert (taken == 1).all()
        assert parts.min() == 1 and parts.max() <= 2
        assert np.array_equal(sim["straddles"], (parts == 2).astype(np.int64))
        assert (parts == 2).any() == (layer != "onet.conv3" and N * S * S > BM)


@pytest.mark.parametrize("layer,S,k,st", LAYERS)
def test_fixup_cells_are_the_cells_with_two_parts(sims, layer, S, k, st):
    for N in launches(S):
        sim, rows = sims[(layer, N)]
        two = np.flatnonzero(rows[:, 0] // BM != rows[:, -1] // BM)
        fixed = [g for b, g0, g1 in sim["cuts"] for g in range(g0, g1)]
        assert len(sim["cuts"]) == len(sim["tiles"]) - 1
        assert fixed == two.tolist(), (layer, N)           # each once, in order
        for b, g0, g1 in sim["cuts"]:
            assert all(rows[g, 0] < b * BM <= rows[g, -1] for g in range(g0, g1))


def _scan(vals):
    """maxpool_kernel's scan over the last axis: best = -inf; best = v > best ? v : best."""
    best = np.full(vals.shape[:-1], -np.inf, np.float32)
    for j in range(vals.shape[-1]):
        v = vals[..., j]
        with np.errstate(invalid="ignore"):
            best = np.where(v > best, v, best)
    return best


def _special(rng, n):
    pool = np.array([0.0, -0.0, np.nan, -np.nan, np.inf, -np.inf, 1.0, -1.0, 1e-45, -1e-45], np.float32)
    return pool[rng.integers(0, len(pool), n)]


@pytest.mark.parametrize("data", ["random", "zeros_and_nans", "mixed"])
@pytest.mark.parametrize("layer,S,k,st", LAYERS)
def test_part_part_combine_equals_sequential_scan(sims, layer, S, k, st, data):
    N = max(launches(S))
    sim, rows = sims[(layer, N)]
    rng = np.random.default_rng(S * 100 + len(data))
    x = rng.standard_normal(N * S * S).astype(np.float32)
    if data == "zeros_and_nans":
        x = _special(rng, len(x))
    elif data == "mixed":
        m = rng.random(len(x)) < 0.5
        x[m] = _special(rng, int(m.sum()))
    want = _scan(x[rows])
    pooled = np.full(len(rows), np.float32(123.0))        # stale values: every cell must be written before it is read
    side = np.full(len(rows), np.float32(-321.0))
    written = np.zeros((2, len(rows)), bool)
    for t, g0, g1, second in sim["tiles"]:
        r = rows[g0:g1]
        inside = (r >= t * BM) & (r < (t + 1) * BM)
        # an element outside the tile is skipped; a NaN in its place is the same, since the comparison never adopts one
        vals = _scan(np.where(inside, x[r], np.float32(np.nan)))
        sec = np.array(second, bool)
        pooled[g0:g1][~sec] = vals[~sec]
        side[g0:g1][sec] = vals[sec]
        written[0, g0:g1] |= ~sec
        written[1, g0:g1] |= sec
    assert written[0].all()
    for b, g0, g1 in sim["cuts"]:
        assert written[1, g0:g1].all()
        A, B = pooled[g0:g1], side[g0:g1]
        with np.errstate(invalid="ignore"):
            pooled[g0:g1] = np.where(B > A, B, A)
    assert np.array_equal(pooled.view(np.int32), want.view(np.int32))
