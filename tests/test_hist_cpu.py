"""The score histograms without a GPU: tests/hist_ref.py (the reference the GPU tests hold trl_gallery_hist to) against a double
loop and against the shipped predicates, the edge sets the GPU tests use, gallery.py's pure functions against the reference's
loops, csrc/trl_gallery_bins.h -- the bin search of the kernel -- built for the host and run against a linear count, and the
host-only parts of the C ABI."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cluster_ref as CR
import gallery_ref as G
import hist_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "truely-real-time-ai-generated-video-detection-framework-for-social-platforms_amd", "csrc")
ALL_SETS = H.PLAIN_SETS + ("TIES",)


@pytest.mark.parametrize("metric", (G.COSINE, G.EUCLIDEAN))
def test_reference_equals_double_loop(metric):
    n = 33
    s = CR.table_scores(metric)[:n, :n]
    ids = H.gallery_ids()[:n]
    valid = CR.mask(n)
    assert np.isnan(s).any() and (valid == 0).any()
    for name in ("TIES", "INF", "ONE"):
        edges = H.edge_set(name, metric)
        E = len(edges)
        for upper in (False, True):
            for qv, gv in ((None, None), (valid, valid), (valid, None)):
                want = np.zeros((2, E + 2), np.int64)
                for i in range(n):
                    for j in range(n):
                        if (qv is not None and not qv[i]) or (gv is not None and not gv[j]) or (upper and j <= i):
                            continue
                        x = s[i, j]
                        if np.isnan(x):
                            b = E + 1
                        else:
                            b = sum(1 for e in edges if (e <= x if metric == G.COSINE else e < x))
                        want[int(ids[i] == ids[j]), b] += 1
                got = H.hist_ref(s, metric, edges, ids, ids, qv, gv, upper)
                assert np.array_equal(got, want), (name, upper)
                if qv is None:
                    assert got.sum() == (n * (n - 1) // 2 if upper else n * n)
    # the scores are symmetric bit for bit, so without a mask ALL = 2 UPPER + the diagonal
    edges = H.edge_set("TIES", metric)
    full = H.hist_ref(s, metric, edges, ids, ids)
    up = H.hist_ref(s, metric, edges, ids, ids, upper=True)
    diag = np.zeros_like(full)
    np.add.at(diag[1], H.bins_ref(np.diagonal(s), metric, edges), 1)
    assert np.array_equal(full, 2 * up + diag)


@pytest.mark.parametrize("metric", (G.COSINE, G.EUCLIDEAN))
def test_cumulative_sums_are_the_shipped_predicates(metric):
    """At every edge of TIES: the pairs identify / cluster accept at that threshold, in float32, are a cumulative sum of bins."""
    s = CR.table_scores(metric)
    edges = H.edge_set("TIES", metric)
    E = len(edges)
    ids = H.gallery_ids()
    c = H.hist_ref(s, metric, edges, ids, ids).sum(axis=0)
    with np.errstate(invalid="ignore"):
        for e in range(E):
            if metric == G.COSINE:
                assert c[e + 1:E + 1].sum() == (s >= edges[e]).sum(), e
            else:
                assert c[:e + 1].sum() == (s <= edges[e]).sum(), e
    assert c[E + 1] == np.isnan(s).sum() > 0 and c.sum() == s.size


@pytest.mark.parametrize("metric", (G.COSINE, G.EUCLIDEAN))
def test_edge_sets(metric):
    for name in ALL_SETS:
        e = H.edge_set(name, metric)
        assert e.dtype == np.float32 and 1 <= len(e) <= 1023 and not np.isnan(e).any() and (e[1:] > e[:-1]).all(), name
    assert [len(H.edge_set(k, metric)) for k in H.PLAIN_SETS] == [1, 2, 63, 64, 1023, 6]
    assert np.isinf(H.edge_set("INF", metric)[[0, -1]]).all()
    t = H.edge_set("TIES", metric)
    assert len(t) >= 700
    # TIES really ties: scores that EQUAL an edge are what tells <= from <
    s = CR.table_scores(metric)
    hits = np.isin(s[np.isfinite(s)], t).sum()
    assert hits >= 500, hits
    assert np.isin(G.table_scores(metric)[np.isfinite(G.table_scores(metric))], t).sum() >= 100
    # ... and both sides of a tie are edges too
    both = np.isin(np.nextafter(t, np.float32(np.inf)), t) & np.isin(np.nextafter(t, np.float32(-np.inf)), t)
    assert both.sum() >= 250
    thr = H.with_thresholds(metric)
    assert all(np.float32(x) in thr for x in CR.TABLE_THR[metric]) and (thr[1:] > thr[:-1]).all()
    gi, qi = H.gallery_ids(), H.query_ids()
    assert len(set(gi[list(G.DUPS)])) == 1 and qi[0] == qi[32] == gi[G.DUP_OF] and set(gi) == set(range(7))


def _count_cases():
    rng = np.random.default_rng(5)
    cases = []
    for E in (1, 2, 5, 64):
        cases.append((rng.integers(0, 50, E + 1), rng.integers(0, 1000, E + 1), rng.integers(0, 3, 2)))
        cases.append((rng.integers(0, 50, E + 1), rng.integers(0, 1000, E + 1), np.zeros(2, np.int64)))
    cases.append((np.zeros(6, np.int64), rng.integers(0, 9, 6), np.array([2, 0])))          # no genuine pair
    cases.append((rng.integers(0, 9, 6), np.zeros(6, np.int64), np.array([0, 1])))          # no impostor pair
    cases.append((np.zeros(4, np.int64), np.zeros(4, np.int64), np.array([0, 0])))          # nothing at all
    cases.append((np.zeros(4, np.int64), np.zeros(4, np.int64), np.array([3, 4])))          # nothing but NaN scores: rates 0
    cases.append((np.array([2 ** 40, 1, 2 ** 41]), np.array([3, 2 ** 45, 1]), np.array([1, 1])))   # past int32 and float32
    return cases


def test_roc_and_threshold_equal_reference_loops():
    import torch
    import truely_amd
    from truely_amd.gallery import roc_from_counts, threshold_at_far
    assert truely_amd.roc_from_counts is roc_from_counts and truely_amd.threshold_at_far is threshold_at_far
    assert {"roc_from_counts", "threshold_at_far", "cluster_embeddings"} <= set(truely_amd.__all__)
    raised = found = 0
    for name, metric in G.METRICS.items():
        for gen, imp, nan in _count_cases():
            E = len(gen) - 1
            want_t, want_f = H.roc_ref(gen, imp, nan, metric)
            for conv in (lambda a: np.asarray(a, np.int64), lambda a: torch.from_numpy(np.asarray(a, np.int64)), list):
                tar, far = roc_from_counts(conv(gen), conv(imp), conv(nan), name)
                assert tar.dtype == np.float64 and far.dtype == np.float64 and tar.shape == far.shape == (E,)
                assert np.array_equal(tar, np.array(want_t), equal_nan=True) and np.array_equal(far, np.array(want_f), equal_nan=True)
            if not int(np.sum(gen)) + int(nan[1]):
                assert np.isnan(tar).all()
            if not int(np.sum(imp)) + int(nan[0]):
                assert np.isnan(far).all()
            edges = np.linspace(-0.5, 0.75, E).astype(np.float32) if E > 1 else np.array([0.25], np.float32)
            for target in (0.0, 1e-3, 0.3, 0.5, 1.0):
                want = H.threshold_ref(edges, want_t, want_f, target, metric)
                if want is None:
                    with pytest.raises(ValueError):
                        threshold_at_far(edges, tar, far, target, name)
                    raised += 1
                else:
                    got = threshold_at_far(edges, tar, far, target, name)
                    assert all(isinstance(x, float) for x in got)
                    assert np.array_equal(np.array(got), np.array(want), equal_nan=True), (name, target)
                    found += 1
    assert raised >= 10 and found >= 50
    # far is monotone in the edge, so "loosest" is well defined: a hand-made curve
    far = np.array([0.5, 0.2, 0.2, 0.01, 0.0])
    tar = np.array([1.0, 0.9, 0.8, 0.7, 0.1])
    edges = np.array([0.1, 0.2, 0.3, 0.4, 0.5], np.float32)
    assert threshold_at_far(edges, tar, far, 0.2, "cosine") == (float(np.float32(0.2)), 0.9, 0.2)
    assert threshold_at_far(edges, tar[::-1], far[::-1], 0.2, "euclidean") == (float(np.float32(0.4)), 0.9, 0.2)
    with pytest.raises(ValueError):
        threshold_at_far(edges, tar, far + 0.1, 0.05, "cosine")
    with pytest.raises(ValueError):
        roc_from_counts([1, 2], [3, 4], [0, 0], "manhattan")


@pytest.fixture(scope="module")
def bins_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("gallery_bins") / "gallery_bins")
    base = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "tests", "gallery_bins_main.cpp"), "-o", out]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(base + san, capture_output=True, text=True).returncode != 0:
        subprocess.run(base, check=True)
    return out


def _hex(a) -> str:
    return " ".join(f"{int(x):08x}" for x in np.asarray(a, np.float32).view(np.uint32))


def test_bin_header_equals_linear_count(bins_program):
    """trl_gl_bin at E in {1, 2, 63, 64, 1023}, the INF and TIES sets: scores equal to edges and one ulp to either side, +-0, +-inf,
    NaN of both signs, the table's own scores.  The program compares with a linear count; its output is compared with numpy."""
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1.0, -1.0, 1e-45, -1e-45, 3.4e38, -3.4e38], np.float32)
    cases, script = [], []
    for metric in (G.COSINE, G.EUCLIDEAN):
        table = G.table_scores(metric)[[0, 3, 4, 7]].reshape(-1)
        for name in ALL_SETS:
            e = H.edge_set(name, metric)
            scores = np.concatenate([special, e, np.nextafter(e, np.float32(np.inf)), np.nextafter(e, np.float32(-np.inf)), table]).astype(np.float32)
            script += [f"{metric} {len(e)} {len(scores)}", _hex(e), _hex(scores)]
            cases.append((metric, e, scores))
        e = np.array([-0.0, 1.0], np.float32)                                   # an edge of -0 against scores of +0 and -0
        script += [f"{metric} 2 {len(special)}", _hex(e), _hex(special)]
        cases.append((metric, e, special))
    r = subprocess.run([bins_program], input="\n".join(script) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    got = np.array(r.stdout.split(), np.int64)
    want = np.concatenate([H.bins_ref(s, metric, e) for metric, e, s in cases])
    assert len(got) == len(want) > 8000 and np.array_equal(got, want)
    e = np.array([-0.0, 1.0], np.float32)
    assert H.bins_ref(np.array([0.0, -0.0], np.float32), G.COSINE, e).tolist() == [1, 1]
    assert H.bins_ref(np.array([0.0, -0.0], np.float32), G.EUCLIDEAN, e).tolist() == [0, 0]


def test_abi_declares_hist():
    from truely_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "truely_hip.h")).read()
    names = {"trl_gallery_hist_workspace", "trl_gallery_hist"}
    assert names <= set(re.findall(r"\b(trl_[a-z0-9_]+)\s*\(", hdr)) and names <= set(_lib.EXPORTS)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in names) and lib.trl_abi_version() == 7
    ws = lib.trl_gallery_hist_workspace
    # refused arguments: 0
    for args in ((33, 33, 0, 0), (33, 33, 1024, 0), (33, 33, -1, 0), (-1, 33, 10, 0), (33, -1, 10, 0), (33, 33, 10, 100),
                 (33, 33, 10, -128), (33, 1 << 31, 10, 0)):
        assert ws(*args) == 0, args
    assert ws(0, 33, 10, 0) == 0 and ws(33, 0, 10, 0) == 0                     # nothing to count: nothing needed
    # 2 (E + 2) uint32 counters per workgroup (row tile x strip)
    assert ws(1, 1, 1, 0) == 2 * 3 * 4
    assert ws(33, 257, 1023, 128) == 2 * 3 * 2 * 1025 * 4
    sizes = [ws(32768, 512, 100, cols) for cols in (0, 256, 128)]              # 1, 2 and 4 strips of 1,024 row tiles
    assert sizes == [1024 * s * 2 * 102 * 4 for s in (1, 2, 4)]
    assert ws(65536, 65536, 1023, 0) < 64 << 20                                # where the score matrix would be 17 GB
    big = [ws(1024, 1 << 20, 1000, cols) for cols in (0, 1 << 16, 1 << 12, 128)]
    assert all(a <= b for a, b in zip(big, big[1:])) and big[0] < big[-1]      # monotone in the strip count
