"""Embedding templates without a GPU: tests/pool_ref.py (the reference the GPU tests hold the kernels to) against a float64 mean of
unit vectors within a derived bound, its skip / ignore rule row by row, its invariance under permutation and splitting, the
representative against a brute-force argmax, csrc/trl_pool.h built for the host and held to the reference bit for bit, and the
ABI's host side."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import gallery_ref as G
import pool_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "truely-real-time-ai-generated-video-detection-framework-for-social-platforms_amd", "csrc")
F32 = np.float32


def _state(ids, weights, m=P.M):
    gid, G_ = P.gid_tables()[ids]
    w = P.weight_tables()[weights]
    return P.accumulate(P.empty_state(G_), G.tables()[0][:m], gid[:m], None if w is None else w[:m], 0, G.table_n2()[:m])


@pytest.mark.parametrize("weights", tuple(P.weight_tables()))
@pytest.mark.parametrize("ids", tuple(P.gid_tables()))
def test_reference_within_bound_of_float64_mean(ids, weights):
    gid, G_ = P.gid_tables()[ids]
    st = _state(ids, weights)
    t = st["A"].astype(F32) * F32(2.0 ** -32)
    want, mag, n = P.mean64(G.tables()[0], gid, P.weight_tables()[weights], G_)
    assert np.array_equal(n, st["N"])
    err = np.abs(t.astype(np.float64) - want)
    bound = P.sum_bound(mag, n, t)
    assert (err <= bound).all(), (ids, weights, float((err / bound).max()))
    assert bound.max() < 1e-3                                               # (252 rows in one group: 9 * gamma_512 / 2; small against |t|)


def test_skip_and_ignore_rule_row_by_row():
    x = G.tables()[0]
    n2 = G.table_n2()
    cls = P.classify(n2, np.zeros(P.M, np.int32), np.ones(P.M, F32), 1)
    assert np.nonzero(cls == P.SKIPPED)[0].tolist() == sorted(P.SKIPPED_ROWS) == [3, 9, 10, 11, 12]
    assert (cls != P.IGNORED).all() and (cls == P.CONTRIBUTES).sum() == 252
    q, wq, p = P.quantise(x[cls == P.CONTRIBUTES], n2[cls == P.CONTRIBUTES], np.ones(252, F32))
    assert np.abs(p).max() == 1.0 and (wq == 2 ** 32).all() and np.abs(q).max() <= 2 ** 32
    # the weights rule 3 decides on
    w = P.weight_tables()["edge"]
    cls = P.classify(n2, np.zeros(P.M, np.int32), w, 1)
    assert np.nonzero(cls == P.SKIPPED)[0].tolist() == sorted(set(P.SKIPPED_ROWS) | set(P.EDGE_SKIPPED))
    assert (cls[[100, 130, 131]] == P.CONTRIBUTES).all()
    st = _state("one", "edge")
    assert st["skipped"] == 11 and st["N"][0] == P.M - 11
    # ids outside the state are ignored, whatever the row holds, and counted nowhere
    gid, G_ = P.gid_tables()["outside"]
    cls = P.classify(n2, gid, np.ones(P.M, F32), G_)
    assert ((cls == P.IGNORED) == ((gid < 0) | (gid >= G_))).all() and 30 < (cls == P.IGNORED).sum() < 90
    st = _state("outside", "none")
    inside = (gid >= 0) & (gid < G_)
    assert st["N"].sum() + st["skipped"] == inside.sum()
    assert st["skipped"] == sum(1 for r in P.SKIPPED_ROWS if inside[r])
    # a state over groups g0 .. g0 + G - 1 sees the other groups' rows as ignored: chunks of groups give the whole
    whole = _state("div16", "random")
    for g0, c in ((0, 5), (5, 11), (16, 1)):
        part = P.accumulate(P.empty_state(c), x, P.gid_tables()["div16"][0], P.weight_tables()["random"], g0, n2)
        assert np.array_equal(part["A"], whole["A"][g0:g0 + c]) and np.array_equal(part["N"], whole["N"][g0:g0 + c])
    # empty groups, and a group whose sum cancels
    r = P.table_ref("dups", "none", P.UNIT)
    assert r["count"].tolist() == [P.M - 5 - 3 - 2, 5, 0, 0] and r["skipped"] == 5
    assert not r["template"][2:].any() and not np.signbit(r["template"][2:]).any()
    assert r["weight"][2:].tolist() == [0, 0] and r["cohesion"][2:].tolist() == [0, 0]
    assert abs(float(r["cohesion"][1]) - 1) < 1e-6 and r["weight"][1] == 5
    pair = np.stack([x[G.DUP_OF], x[G.NEG_OF_DUP]])
    z = P.pool_ref(pair, [0, 0], None, 1, P.UNIT)
    assert z["count"][0] == 2 and np.isnan(z["template"]).all() and z["cohesion"][0] == 0
    z = P.pool_ref(pair, [0, 0], None, 1, P.MEAN)
    assert not z["template"].any() and z["weight"][0] == 2


def test_permutation_and_split_invariance():
    x, n2 = G.tables()[0], G.table_n2()
    rng = np.random.default_rng(77)
    for ids, weights in (("mod3", "random"), ("outside", "edge"), ("runs", "none")):
        gid, G_ = P.gid_tables()[ids]
        w = P.weights_of(P.weight_tables()[weights], P.M)
        whole = _state(ids, weights)
        perm = rng.permutation(P.M)
        st = P.accumulate(P.empty_state(G_), x[perm], gid[perm], w[perm], 0, n2[perm])
        assert all(np.array_equal(st[k], whole[k]) for k in ("A", "W", "N")) and st["skipped"] == whole["skipped"]
        st = P.empty_state(G_)
        for a, b in ((0, 1), (1, 33), (33, 133), (133, 133), (133, 257)):
            P.accumulate(st, x[a:b], gid[a:b], w[a:b], 0, n2[a:b])
        assert all(np.array_equal(st[k], whole[k]) for k in ("A", "W", "N")) and st["skipped"] == whole["skipped"]


def _brute_representative(scores_row, candidates):
    best = -1
    for i in candidates:
        s = scores_row[i]
        if np.isnan(s):
            continue
        if best < 0 or s > scores_row[best]:                                  # (strictly: equal floats, -0 == +0, keep the lower row)
            best = i
    return best


def test_representative_against_brute_force():
    x = G.tables()[0]
    for ids, weights in (("dups", "none"), ("div16", "edge"), ("outside", "random"), ("one", "none")):
        gid, G_ = P.gid_tables()[ids]
        w = P.weight_tables()[weights]
        tmpl = P.table_ref(ids, weights, P.UNIT)["template"]
        index, score = P.representative_ref(x, gid, w, tmpl, G.table_n2())
        s = G.scores_ref(tmpl, x, G.COSINE)
        cls = P.classify(G.table_n2(), gid, P.weights_of(w, P.M), G_)
        for g in range(G_):
            want = _brute_representative(s[g], np.nonzero((cls == P.CONTRIBUTES) & (gid == g))[0])
            assert index[g] == want, (ids, g)
            assert np.isnan(score[g]) if want < 0 else G.same_bits(score[g:g + 1], s[g, want:want + 1]).all()
    # the five copies of one row alone in a group: every cosine ties, the lowest row wins
    index, score = P.representative_ref(x, P.gid_tables()["dups"][0], None, P.table_ref("dups", "none", P.UNIT)["template"])
    assert index.tolist()[1:] == [G.DUPS[0], -1, -1] and np.isnan(score[2:]).all() and abs(float(score[1]) - 1) < 1e-6
    # a group whose only rows are NaN: skipped rows are no candidates; and a NaN template row makes every cosine NaN
    only_nan = np.stack([x[G.NAN_G], x[G.NAN_G], x[0]])
    index, score = P.representative_ref(only_nan, [0, 0, 1], None, P.pool_ref(only_nan, [0, 0, 1], None, 2)["template"])
    assert index.tolist() == [-1, 2] and np.isnan(score[0])
    pair = np.stack([x[G.DUP_OF], x[G.NEG_OF_DUP]])
    index, score = P.representative_ref(pair, [0, 0], None, P.pool_ref(pair, [0, 0], None, 1)["template"])
    assert index.tolist() == [-1] and np.isnan(score[0])
    # -0 ties with +0: the lower row wins
    gz, qz = G.zero_sign_rows()
    sz = G.scores_ref(qz, gz, G.COSINE)[0]
    assert np.signbit(sz[2]) and sz[2] == 0 and not np.signbit(sz[0]) and sz[0] == 0
    index, score = P.representative_ref(gz[[2, 0, 4]], [0, 0, 0], None, qz)
    assert index.tolist() == [0] and G.same_bits(score, sz[2:3]).all()


@pytest.fixture(scope="module")
def pool_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("pool") / "pool")
    base = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "tests", "pool_main.cpp"), "-o", out]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(base + san, capture_output=True, text=True).returncode != 0:
        subprocess.run(base, check=True)
    return out


def _hex(a):
    return " ".join(f"{v:08x}" for v in np.ascontiguousarray(a, F32).view(np.uint32).tolist())


def _floats(words):
    return np.array([int(v, 16) for v in words], np.uint32).view(F32)


def test_header_equals_reference(pool_program):
    """csrc/trl_pool.h on the host: accumulators, both finishes and the representatives of the table's rows under id patterns with
    runs, ids outside the state, empty groups and a state that starts at g0 > 0, and of built rows (a cancelling pair, -0 cosines)."""
    x = G.tables()[0]
    cases = []
    for ids, weights, g0, c in (("div16", "edge", 0, 17), ("outside", "random", 0, 6), ("dups", "none", 0, 4), ("div16", "none", 5, 7),
                                ("one", "random", 0, 1)):
        w = P.weights_of(P.weight_tables()[weights], P.M)
        cases.append((c, g0, x, P.gid_tables()[ids][0], w))
    cases.append((1, 0, np.stack([x[G.DUP_OF], x[G.NEG_OF_DUP]]), np.zeros(2, np.int32), np.ones(2, F32)))
    gz, qz = G.zero_sign_rows()
    cases.append((2, 0, np.concatenate([gz[[2, 0, 4, 5]], qz]), np.array([0, 0, 0, 1, 1], np.int32), np.ones(5, F32)))
    script = []
    for c, g0, rows, gid, w in cases:
        script.append(f"{c} {g0} {len(rows)}")
        script += [f"{int(gid[i])} {_hex(w[i:i + 1])} {_hex(rows[i])}" for i in range(len(rows))]
    r = subprocess.run([pool_program], input="\n".join(script) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = iter(r.stdout.splitlines())
    for n, (c, g0, rows, gid, w) in enumerate(cases):
        st = P.accumulate(P.empty_state(c), rows, gid, w, g0)
        assert int(next(lines)) == st["skipped"], n
        for g in range(c):
            v = [int(t) for t in next(lines).split()]
            assert v[0] == st["N"][g] and v[1] == st["W"][g] and v[2:] == st["A"][g].tolist(), (n, g)
        fin = {}
        for mode in (P.UNIT, P.MEAN):
            fin[mode] = P.finish(st, mode)
            for g in range(c):
                v = next(lines).split()
                assert int(v[0]) == fin[mode]["count"][g], (n, mode, g)
                assert G.same_bits(_floats(v[1:2]), fin[mode]["weight"][g:g + 1]).all(), (n, mode, g)
                assert G.same_bits(_floats(v[2:3]), fin[mode]["cohesion"][g:g + 1]).all(), (n, mode, g)
                assert G.same_bits(_floats(v[3:]), fin[mode]["template"][g]).all(), (n, mode, g)
        index, score = P.representative_ref(rows, np.asarray(gid, np.int64) - g0, w, fin[P.UNIT]["template"])
        for g in range(c):
            key, i, s = next(lines).split()
            assert int(i) == index[g] and (int(key, 16) == 0) == (index[g] < 0), (n, g)
            assert G.same_bits(_floats([s]), score[g:g + 1]).all(), (n, g)
    assert next(lines, None) is None


def test_abi_rejections_need_no_device():
    from truely_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "truely_hip.h")).read()
    names = {"trl_pool_state_bytes", "trl_pool_reset", "trl_pool_add", "trl_pool_finish", "trl_pool_rep_reset", "trl_pool_rep_add",
             "trl_pool_rep_finish"}
    assert names <= set(re.findall(r"\b(trl_[a-z0-9_]+)\s*\(", hdr)) and names <= set(_lib.EXPORTS)
    assert "2^30" in hdr[hdr.index("Templates"):]                                 # the rows-per-group precondition is stated
    lib = _lib.load()
    assert lib.trl_abi_version() == 7
    sb = lib.trl_pool_state_bytes
    assert sb(0) == 8 and sb(1) == 8 * 515 and sb(257) == 8 * (514 * 257 + 1) and sb(-1) == 0 and sb(2 ** 31) == 0
    buf = (C.c_longlong * 1100)()
    p = C.addressof(buf)
    add = lambda state=p, groups=2, g0=0, rows=p, ld=512, n2=None, gid=p, w=None, m=1, tile=0: \
        lib.trl_pool_add(state, groups, g0, rows, ld, n2, gid, w, m, tile, None)
    bad = [add(state=None), add(state=p + 4), add(groups=-1), add(rows=None), add(gid=None), add(ld=511), add(m=-1), add(m=2 ** 30 + 1),
           add(tile=1), add(tile=7), add(tile=64), add(tile=-8)]
    fin = lambda state=p, groups=2, mode=0, t=p, c=p, w=p, h=p: lib.trl_pool_finish(state, groups, mode, t, c, w, h, None, None)
    bad += [fin(state=None), fin(state=p + 4), fin(groups=-1), fin(mode=2), fin(mode=-1), fin(t=None), fin(c=None), fin(w=None), fin(h=None)]
    rep = lambda key=p, groups=2, t=p, rows=p, ld=512, gid=p, row0=0, m=1, tile=0: \
        lib.trl_pool_rep_add(key, groups, 0, t, rows, ld, None, gid, None, row0, m, tile, None)
    bad += [rep(key=None), rep(key=p + 4), rep(groups=-1), rep(t=None), rep(rows=None), rep(gid=None), rep(ld=100), rep(m=-1),
            rep(m=2 ** 30 + 1), rep(row0=-1), rep(row0=2 ** 31 - 1), rep(row0=2 ** 31 - 2 ** 30, m=2 ** 30), rep(tile=3)]
    bad += [lib.trl_pool_reset(None, 2, None), lib.trl_pool_reset(p + 4, 2, None), lib.trl_pool_reset(p, -1, None),
            lib.trl_pool_rep_reset(None, 2, None), lib.trl_pool_rep_reset(p, -1, None),
            lib.trl_pool_rep_finish(None, 2, p, p, None), lib.trl_pool_rep_finish(p, 2, None, p, None), lib.trl_pool_rep_finish(p, 2, p, None, None)]
    assert all(b != 0 for b in bad) and len(set(bad)) == 1, bad
    assert b"trl_pool" in lib.trl_last_error()
    # nothing to do is no error, and needs no device either
    assert add(m=0) == 0 and add(m=0, rows=None, gid=None) == 0 and rep(m=0) == 0 and rep(m=0, row0=2 ** 31 - 1) == 0
    assert lib.trl_pool_rep_reset(p, 0, None) == 0 and lib.trl_pool_rep_finish(p, 0, None, None, None) == 0
