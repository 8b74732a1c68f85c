"""Inputs of the label stage over neighbour lists (trl_cluster_labels_lists, include/truely_hip.h).  The rules and their reference
are tests/cluster_ref.py's; here are the lists of a link matrix, and an input past the bitmap's 65,536 rows whose expected result
needs no n x n matrix.

The chain input: row i = 2 e_a + 2 e_b, where (a, b) = (c, c + 1) is a pair of neighbouring coordinates inside one of several
disjoint chains of coordinates (its "type"), the types dealt out evenly and the row order shuffled by a fixed seed.  Every dot
product is 8 (same type), 4 (the types share a coordinate) or 0, every squared norm 8, so a cosine score is ~1, ~0.5 or exactly 0:
at threshold 0.25 two rows link iff their types share a coordinate, with every score far from the threshold.  A row's degree is
then the number of rows of its own and its neighbouring types, and the labels follow from a union-find over the types."""
from __future__ import annotations

import numpy as np

DIM = 512
CHAIN_THR = 0.25
# coordinates per chain: a chain of 2 has one type (both of its coordinates are ends), a chain of 3 two end types and no interior
CHAINS = (2, 3) + (5, 8, 12, 7) * 15
SMALL_CHAINS = (2, 3, 5, 8)


def csr_from_link(link: np.ndarray):
    """link (n, n) bool -> (offsets (n + 1,) int64, index (total,) int32): row i's set columns, ascending, at offsets[i] .."""
    link = np.asarray(link, bool)
    offsets = np.zeros(link.shape[0] + 1, np.int64)
    np.cumsum(link.sum(axis=1), out=offsets[1:])
    index = np.nonzero(link)[1].astype(np.int32)                       # (row-major: ascending within a row)
    return offsets, index


def chain_pairs(chains=CHAINS) -> np.ndarray:
    """(T, 2): the types (c, c + 1) of every chain, the chains laid side by side over the coordinates."""
    assert sum(chains) <= DIM and min(chains) >= 2
    pairs, c0 = [], 0
    for length in chains:
        pairs += [(c, c + 1) for c in range(c0, c0 + length - 1)]
        c0 += length
    return np.array(pairs, np.int64)


def chain_rows(n: int, chains=CHAINS, seed: int = 66000):
    """(emb (n, 512) float32, types (n,) int64, pairs (T, 2))."""
    pairs = chain_pairs(chains)
    types = np.random.default_rng(seed).permutation(np.arange(n) % len(pairs))
    emb = np.zeros((n, DIM), np.float32)
    emb[np.arange(n), pairs[types, 0]] = 2
    emb[np.arange(n), pairs[types, 1]] = 2
    return emb, types, pairs


def _type_graph(types, pairs):
    """(rows per type (T,), near (T, T) bool: the types share a coordinate, a type with itself included)."""
    T = len(pairs)
    near = (pairs[:, None, :, None] == pairs[None, :, None, :]).any(axis=(2, 3))
    return np.bincount(types, minlength=T), near


def chain_border_ms(types, pairs) -> int:
    """A min_samples at which exactly the rows of end types (those with fewer than two neighbouring types) are not core."""
    count, near = _type_graph(types, pairs)
    deg = near.astype(np.int64) @ count
    ends = near.sum(axis=1) < 3
    ms = int(deg[ends].max()) + 1
    assert ms <= deg[~ends].min(), "too few rows per type for the end types to stand apart"
    return ms


def chain_expect(types, pairs, min_samples: int):
    """(labels (n,) int32, core (n,) uint8, degree (n,) int32, count) by the header's rules, from a union-find over the types."""
    count, near = _type_graph(types, pairs)
    T, n = len(pairs), len(types)
    deg_t = near.astype(np.int64) @ count                              # own type (the row itself among them) + neighbouring types
    core_t = (count > 0) & (deg_t >= min_samples)
    root = list(range(T))

    def find(t):
        while root[t] != t:
            root[t] = root[root[t]]
            t = root[t]
        return t

    for t, u in zip(*np.nonzero(near & core_t[:, None] & core_t[None, :])):
        root[find(int(t))] = find(int(u))
    comp_t = np.array([find(t) for t in range(T)])
    first = np.full(T, n, np.int64)                                    # per component: its smallest core row
    np.minimum.at(first, comp_t[types], np.where(core_t[types], np.arange(n), n))
    number = np.full(T, -1, np.int64)
    live = np.nonzero(first < n)[0]
    number[live[np.argsort(first[live])]] = np.arange(len(live))
    label_t = np.full(T, -1, np.int64)
    for t in range(T):
        if core_t[t]:
            label_t[t] = number[comp_t[t]]
        else:                                                          # border: the smallest number among the core neighbours' clusters
            nb = np.nonzero(near[t] & core_t)[0]
            if len(nb):
                label_t[t] = number[comp_t[nb]].min()
    return label_t[types].astype(np.int32), core_t[types].astype(np.uint8), deg_t[types].astype(np.int32), len(live)
