"""The label stage over neighbour lists without a GPU: the host-only part of its C ABI, and tests/cluster_lists_ref.py -- the lists
of a link matrix against the range search's reference, and the chain input's union-find against tests/cluster_ref.py on the dense
links of a size where those are affordable."""
import os
import re

import numpy as np
import pytest

import cluster_lists_ref as LR
import cluster_ref as CR
import gallery_ref as G
import range_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_LIST_N = 1 << 24


def test_abi_declares_cluster_lists():
    from truely_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "truely_hip.h")).read()
    names = {"trl_cluster_lists_workspace", "trl_cluster_labels_lists"}
    assert names <= set(re.findall(r"\b(trl_[a-z0-9_]+)\s*\(", hdr)) and names <= set(_lib.EXPORTS)
    lib = _lib.load()
    assert lib.trl_abi_version() == 7
    for n in (0, 1, 257, 65536, 65537, 66000, MAX_LIST_N):
        assert 12 * n <= lib.trl_cluster_lists_workspace(n) <= 12 * n + 4096, n
    assert lib.trl_cluster_lists_workspace(-1) == 0 and lib.trl_cluster_lists_workspace(MAX_LIST_N + 1) == 0
    assert lib.trl_cluster_workspace(65537) == 0                         # the bitmap's label stage keeps its limit
    assert lib.trl_cluster_lists_workspace(65536) == lib.trl_cluster_workspace(65536)      # (one carving function)


@pytest.mark.parametrize("metric", (G.COSINE, G.EUCLIDEAN))
def test_csr_from_link_is_the_range_search_of_the_table(metric):
    s = CR.table_scores(metric)
    for thr in CR.TABLE_THR[metric]:
        for invalid in ((), CR.INVALID):
            valid = CR.mask(CR.N_TABLE, invalid) if invalid else None
            link, _deg = CR.table_links(metric, thr, CR.N_TABLE, invalid)
            offsets, index = LR.csr_from_link(link)
            want_o, want_i, _s = RR.range_ref(s, metric, thr, valid, valid, skip_self=True)
            assert offsets.dtype == np.int64 and index.dtype == np.int32
            assert np.array_equal(offsets, want_o) and np.array_equal(index, want_i), (metric, thr, invalid)
            assert np.array_equal(RR.unpack(offsets, index, CR.N_TABLE, CR.N_TABLE), link)
    offsets, index = LR.csr_from_link(np.zeros((0, 0), bool))
    assert offsets.tolist() == [0] and index.shape == (0,)
    offsets, index = LR.csr_from_link(CR.empty_graph(3)[0])
    assert offsets.tolist() == [0, 0, 0, 0] and index.shape == (0,)


@pytest.mark.parametrize("n, chains", ((600, LR.SMALL_CHAINS), (4 * len(LR.chain_pairs()) + 77, LR.CHAINS)))
def test_chain_input_against_the_dense_reference(n, chains):
    """The generator of the 66,000-row GPU case at a size where the n x n scores fit: its scores stand far from the threshold, and
    the union-find over the types gives labels_ref's labels, core flags, degrees and count on the dense links."""
    emb, types, pairs = LR.chain_rows(n, chains)
    assert emb.shape == (n, 512) and len(np.unique(types)) == len(pairs)
    dot = emb @ emb.T                                                  # (exact: small integers)
    assert np.isin(dot, (0, 4, 8)).all() and (np.diagonal(dot) == 8).all()
    if n <= 600:                                                       # the bit-exact scores, at the size that affords their fma chains
        s = G.scores_ref(emb, emb, G.COSINE)
        assert ((s == 0) & (dot == 0) | (np.abs(s - 0.5) < 1e-6) & (dot == 4) | (np.abs(s - 1) < 1e-6) & (dot == 8)).all()
    else:                                                              # the same three values: dot / 8
        s = dot / np.float32(8)
    link = CR.links_ref(s, G.COSINE, LR.CHAIN_THR)
    deg = CR.degree_ref(link)
    border_ms = LR.chain_border_ms(types, pairs)
    for ms in (1, 2, border_ms, int(deg.max()), int(deg.max()) + 1):
        want_l, want_c, want_n = CR.labels_ref(link, deg, ms)
        labels, core, degree, count = LR.chain_expect(types, pairs, ms)
        assert labels.dtype == np.int32 and core.dtype == np.uint8 and degree.dtype == np.int32
        assert np.array_equal(degree, deg) and np.array_equal(core, want_c), (n, ms)
        assert np.array_equal(labels, want_l) and count == want_n, (n, ms)
    # min_samples = 1: one cluster per chain; at the border min_samples the end types are border rows, and the chains of 2 and 3
    # coordinates -- end types only -- are noise
    assert LR.chain_expect(types, pairs, 1)[3] == len(chains)
    labels, core, _d, count = LR.chain_expect(types, pairs, border_ms)
    assert count == len(chains) - 2 and (labels[core == 0] >= 0).any() and (labels == -1).any() and core.any()
