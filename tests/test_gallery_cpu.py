"""The embedding match without a GPU: tests/gallery_ref.py (the reference the GPU tests hold the kernels to) against float64 and
against numpy's own sort, and csrc/trl_gallery_order.h -- the list code of the search and merge kernels -- built for the host and
run against that reference.

Bounds, with u = 2^-24 and g = gamma(512) = 512 u / (1 - 512 u) (Higham), for rows whose values stay in float32's normal range:

  dot        512 fmas, one rounding each:  |dot^ - dot| <= g S,  S = sum |q_k g_k|.  Likewise n2^ = n2 (1 + t), |t| <= g
             (every term is positive), and S <= ||q|| ||g|| = D (Cauchy-Schwarz).
  cosine     c^ = dot^ / (sqrt(n2q^) sqrt(n2g^)) with a rounding for each square root, the product and the quotient:
             c^ = (dot + e) / D * rho,  |e| <= g S,  rho = (1 + d4) / (sqrt(1 + tq) sqrt(1 + tg) (1 + d1)(1 + d2)(1 + d3)), so
             |rho - 1| <= eta := (1 + u) / ((1 - g) (1 - u)^3) - 1   and
             |c^ - c| <= |c| eta + g (S / D) (1 + eta).
  euclidean  s^ = fl(n2q^ + n2g^):  |s^ - s| <= s a,  a := (1 + g)(1 + u) - 1.  d2^ = fl(s^ - 2 dot^) (one rounding, the fma):
             |d2^ - d2| <= (s a + 2 g S)(1 + u) + u d2 =: E.  The clamp at 0 moves d2^ towards d2 >= 0.  dist^ = fl(sqrt(d2^)):
             |sqrt(x) - sqrt(y)| <= min(sqrt|x - y|, |x - y| / sqrt(y)), so
             |dist^ - dist| <= min(sqrt(E), E / dist)(1 + u) + u dist.
The float64 values themselves carry about 512 * 2^-53 relative: every bound is multiplied by (1 + 1e-6)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import gallery_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "truely-real-time-ai-generated-video-detection-framework-for-social-platforms_amd", "csrc")
SLACK = 1 + 1e-6


def _ordinary_rows():
    """The table's rows that are finite and in the normal range (the random normal and the normalised ones, the duplicates)."""
    g, q = G.tables()
    special_g = {G.ZERO_G, 5, 6, G.NAN_G, G.INF_G, G.MIXINF_G, 12, 13, 128}
    special_q = {1, 2, 3, 4, 5, 31, 33, 63}
    gi = np.array([r for r in range(len(g)) if r not in special_g])
    qi = np.array([r for r in range(len(q)) if r not in special_q])
    return g, q, gi, qi


def test_dot_within_gamma_of_float64():
    g, q, gi, qi = _ordinary_rows()
    got = G.dot_ref(q[qi], g[gi]).astype(np.float64)
    q64, g64 = q[qi].astype(np.float64), g[gi].astype(np.float64)
    want = q64 @ g64.T
    S = np.abs(q64) @ np.abs(g64).T
    assert (np.abs(got - want) <= G.gamma(512) * S * SLACK).all()
    n2 = G.n2_ref(g[gi]).astype(np.float64)
    n2_64 = (g64 * g64).sum(axis=1)
    assert (np.abs(n2 - n2_64) <= G.gamma(512) * n2_64 * SLACK).all()
    assert np.array_equal(n2[:40].astype(np.float32), np.diagonal(G.dot_ref(g[gi][:40], g[gi][:40])))      # n2 IS dot(x, x)


def test_scores_within_derived_bounds_of_float64():
    g, q, gi, qi = _ordinary_rows()
    q64, g64 = q[qi].astype(np.float64), g[gi].astype(np.float64)
    dot = q64 @ g64.T
    S = np.abs(q64) @ np.abs(g64).T
    nq, ng = (q64 * q64).sum(axis=1), (g64 * g64).sum(axis=1)
    D = np.sqrt(nq)[:, None] * np.sqrt(ng)[None, :]
    u, gm = G.U, G.gamma(512)
    cos = G.table_scores(G.COSINE)[np.ix_(qi, gi)].astype(np.float64)
    c = dot / D
    eta = (1 + u) / ((1 - gm) * (1 - u) ** 3) - 1
    bound = np.abs(c) * eta + gm * (S / D) * (1 + eta)
    assert (np.abs(cos - c) <= bound * SLACK).all(), float((np.abs(cos - c) / bound).max())
    assert np.abs(cos - c).max() > 0                                         # (the comparison is not vacuous)
    euc = G.table_scores(G.EUCLIDEAN)[np.ix_(qi, gi)].astype(np.float64)
    s = nq[:, None] + ng[None, :]
    d2 = ((q64[:, None, :] - g64[None, :, :]) ** 2).sum(axis=2)              # the definition, not the matrix-product form
    dist = np.sqrt(d2)
    a = (1 + gm) * (1 + u) - 1
    E = (s * a + 2 * gm * S) * (1 + u) + u * d2
    with np.errstate(divide="ignore", invalid="ignore"):
        bound = np.minimum(np.sqrt(E), np.where(dist > 0, E / dist, np.inf)) * (1 + u) + u * dist
    assert (np.abs(euc - dist) <= bound * SLACK).all(), float((np.abs(euc - dist) / bound).max())
    # a row against its own copies: the product form cancels to within the bound, the definition gives exactly 0
    assert (d2[0, [list(gi).index(r) for r in G.DUPS]] == 0).all()


def test_special_rows_follow_numpy():
    g, q = G.tables()
    cos, euc = G.table_scores(G.COSINE), G.table_scores(G.EUCLIDEAN)
    assert np.isnan(cos[:, G.ZERO_G]).all() and np.isnan(cos[1]).all()          # a zero row: 0 / 0
    assert np.isnan(cos[:, G.NAN_G]).all() and np.isnan(euc[:, G.NAN_G]).all() and np.isnan(cos[3]).all() and np.isnan(euc[63]).all()
    assert np.isnan(cos[10, G.INF_G]) and euc[10, G.INF_G] == np.inf            # dot = inf, n2 = inf: inf / inf, sqrt(inf + inf - ... )
    assert np.isnan(euc[10, G.MIXINF_G]) or euc[10, G.MIXINF_G] == np.inf
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(g).all(axis=1)                                         # (0 * inf is NaN: the inf rows give NaN here)
        assert G.same_bits(euc[1][fin], np.sqrt(G.table_n2())[fin]).all()        # zero query: dist = sqrt(n2 g)
        assert np.isnan(euc[1][[G.INF_G, G.MIXINF_G]]).all()
    gz, qz = G.zero_sign_rows()
    cz = G.scores_ref(qz, gz, G.COSINE)[0]
    assert np.signbit(cz[[2, 4]]).all() and not np.signbit(cz[[0, 3]]).any() and (cz[[0, 2, 3, 4]] == 0).all() and cz[5] == 1 and cz[1] < 0
    idx, sc = G.topk_ref(cz[None], G.COSINE, 6)
    assert idx[0].tolist() == [5, 0, 2, 3, 4, 1]                                # -0 == +0: the lower index goes first
    # the near pairs: a query equal to one row of a pair scores the two rows within a few ulps of each other
    for (a, b), r in zip(G.NEAR_PAIRS, (7, 30, 64)):
        assert abs(int(cos[r, a].view(np.uint32)) - int(cos[r, b].view(np.uint32))) <= 4


def _lexsort_topk(scores, metric, k):
    """The order restated with numpy.lexsort on primitive keys, row by row."""
    n, m = scores.shape
    idx = np.full((n, k), -1, np.int32)
    for r in range(n):
        s = scores[r]
        nan = np.isnan(s)
        key = np.where(nan, 0, s.astype(np.float64) * (-1 if metric == G.COSINE else 1)) + 0.0   # (+ 0.0: -0 becomes +0)
        o = np.lexsort((np.arange(m), key, nan.astype(np.int8)))[:k]
        idx[r, :len(o)] = o
    return idx


@pytest.mark.parametrize("metric", (G.COSINE, G.EUCLIDEAN))
def test_order_against_lexsort(metric):
    s = G.table_scores(metric)
    for m in (1, 3, 33, 129, 257):
        for k in (1, 5, 16):
            idx, sc = G.topk_ref(s[:, :m], metric, k)
            assert np.array_equal(idx, _lexsort_topk(s[:, :m], metric, k)), (m, k)
            live = idx >= 0
            assert (live.sum(axis=1) == min(k, m)).all() and np.isnan(sc[~live]).all()
            rows = np.nonzero(live)
            assert G.same_bits(sc[rows], s[:, :m][rows[0], idx[rows]]).all()
    # the duplicates tie and come out in index order; NaN scores come last, in index order
    idx, sc = G.topk_ref(s, metric, 16)
    first5 = idx[0, :5].tolist()
    assert first5 == list(G.DUPS) and len(set(sc[0, :5].view(np.uint32).tolist())) == 1
    idx_all, sc_all = G.topk_ref(s[:1, :12], metric, 12)
    nan_at = np.nonzero(np.isnan(s[0, :12]))[0].tolist()
    assert nan_at and idx_all[0, -len(nan_at):].tolist() == nan_at
    valid = np.ones(len(s), np.uint8); valid[[0, 40]] = 0
    idx_v, sc_v = G.topk_ref(s, metric, 5, valid)
    assert (idx_v[[0, 40]] == -1).all() and np.isnan(sc_v[[0, 40]]).all() and np.array_equal(idx_v[1:40], idx[1:40, :5])


@pytest.fixture(scope="module")
def order_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("gallery_order") / "gallery_order")
    base = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "tests", "gallery_order_main.cpp"), "-o", out]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(base + san, capture_output=True, text=True).returncode != 0:
        subprocess.run(base, check=True)
    return out


def test_order_header_equals_reference(order_program):
    """trl_gl_insert / trl_gl_merge on the table's score rows, split at random into strips (1, a few, more than the merge kernel's
    64 lanes) and fed in random order: the k best in the reference's order, with duplicates, NaN, -0 and k > m."""
    rng = np.random.default_rng(77)
    cases, script = [], []
    gz, qz = G.zero_sign_rows()
    sources = [(metric, G.table_scores(metric)[r]) for metric in (G.COSINE, G.EUCLIDEAN) for r in (0, 1, 3, 6, 7, 20, 30, 64)]
    sources.append((G.COSINE, G.scores_ref(qz, gz, G.COSINE)[0]))
    for metric, row in sources:
        for m, k, strips in ((len(row), 5, 1), (len(row), 16, 3), (len(row), 1, 70), (min(len(row), 12), 16, 2), (len(row), 7, 130),
                             (min(len(row), 3), 2, 5)):
            s = row[:m]
            order = rng.permutation(m)
            strip = rng.integers(0, strips, m)
            script.append(f"{metric} {k} {m} {strips}")
            script += [f"{int(s[i].view(np.uint32)):08x} {int(i)} {int(strip[i])}" for i in order]
            cases.append((metric, k, s))
    r = subprocess.run([order_program], input="\n".join(script) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = iter(r.stdout.splitlines())
    for metric, k, s in cases:
        idx, sc = G.topk_ref(s[None], metric, k)
        for e in range(k):
            bits, index = next(lines).split()
            assert int(index) == idx[0, e], (metric, k, len(s), e)
            got = np.array([int(bits, 16)], np.uint32).view(np.float32)
            assert G.same_bits(got, sc[0, e:e + 1]).all()
    assert next(lines, None) is None


def test_abi_declares_gallery():
    import re
    from truely_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "truely_hip.h")).read()
    names = {"trl_gallery_pack", "trl_gallery_scores", "trl_gallery_search_workspace", "trl_gallery_search"}
    assert names <= set(re.findall(r"\b(trl_[a-z0-9_]+)\s*\(", hdr)) and names <= set(_lib.EXPORTS)
    lib = _lib.load()
    # host-only: the workspace of the search does not grow with m, and stays below 64 MB where the score matrix would be 1 GB
    assert lib.trl_gallery_search_workspace(256, 1_000_000, 5, 0) < 64 << 20
    assert lib.trl_gallery_search_workspace(256, 1_000_000, 16, 0) == lib.trl_gallery_search_workspace(256, 2_000_000_000, 16, 0) < 64 << 20
    assert lib.trl_gallery_search_workspace(1, 100, 5, 0) == 0                 # one strip writes the result itself
    assert lib.trl_gallery_search_workspace(3, 257, 5, 128) == 3 * 3 * 5 * 8   # three strips of n x k (score, index) pairs
    assert lib.trl_gallery_search_workspace(3, 257, 17, 0) == 0 and lib.trl_gallery_search_workspace(3, 257, 5, 100) == 0
