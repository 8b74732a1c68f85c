"""The host half of trl_load_weights (csrc/trl_weights.h) and FaceNet's table of convs (csrc/trl_facenet.h), without a GPU.

``tests/weights_sim.cpp`` includes the two headers alone (plain C++17, no HIP) and is built for the host like
``tests/arena_sim.cpp``: with ``-fsanitize=address,undefined`` where the toolchain links it, else without.  It stages a blob file
the way the library does before it uploads, prints the directory, the table and the resolved rows, and writes the host image --
the bytes the device receives.  Checked here: the image's layout against the packer's tensors, the table against the packer's
architecture tables, and every refusal the loader owes a malformed blob."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from truely_amd import weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(weights.__file__), "csrc")
HEADS = {"pnet.heads": ("pnet.conv4_1", "pnet.conv4_2"), "rnet.heads": ("rnet.dense5_1", "rnet.dense5_2"),
         "onet.heads": ("onet.dense6_1", "onet.dense6_2", "onet.dense6_3")}
VECS = {0: (".scale", ".shift"), 1: (".b",), 2: (".scale", ".shift")}       # per-column vectors of a row, by kind
REFUSED = -3                                                               # TRL_ERR_WEIGHTS


@pytest.fixture(scope="module")
def sim_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("weights_sim") / "weights_sim")
    base = [cxx, "-O1", "-g", "-std=c++17", "-I", CSRC, os.path.join(ROOT, "tests", "weights_sim.cpp"), "-o", out]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(base + san, capture_output=True, text=True).returncode != 0:
        subprocess.run(base, check=True)
    return out


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("weights_blobs")


def stage(program, workdir, blob, precision=0, image=False):
    """-> dict(status, error, rows, items, fn, logits, total[, image]) of weights_sim on ``blob``"""
    path = str(workdir / "case.blob")
    with open(path, "wb") as f:
        f.write(blob)
    img = str(workdir / "case.image") if image else "-"
    p = subprocess.run([program, path, str(precision), img], capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    out = {"rows": [], "items": [], "fn": [], "error": ""}
    for ln in p.stdout.split("\n")[:-1]:
        tag, _, rest = ln.partition(" ")
        f = rest.split(" ")
        if tag == "row":
            keys = ("kind", "kh", "kw", "sh", "sw", "ph", "pw", "cin", "cout", "f32_only", "nparts")
            row = dict(zip(keys, map(int, f[2:13])), name=f[1], parts=f[13:])
            assert int(f[0]) == len(out["rows"]) and len(row["parts"]) == row["nparts"]
            out["rows"].append(row)
        elif tag == "status":
            out["status"] = int(rest)
        elif tag == "error":
            out["error"] = rest
        elif tag == "item":
            assert int(f[0]) == len(out["items"])
            if f[2] == "m":
                out["items"].append(dict(name=f[1], mat=True, K=int(f[3]), Cout=int(f[4]), Kpad=int(f[5]), ld=int(f[6]), off=int(f[7])))
            else:
                out["items"].append(dict(name=f[1], mat=False, n=int(f[3]), off=int(f[4])))
        elif tag == "fn":
            assert int(f[0]) == len(out["fn"])
            out["fn"].append(tuple(map(int, f[1:])))
        elif tag == "logits":
            out["logits"] = tuple(map(int, f))
        elif tag == "total":
            out["total"] = int(rest)
        else:
            raise AssertionError(ln)
    if image and out["status"] == 0:
        out["image"] = np.fromfile(img, np.uint8)
    return out


@pytest.fixture(scope="module")
def tensors(blob):
    return weights.unpack_tensors(blob)


@pytest.fixture(scope="module")
def staged(sim_program, workdir, blob):
    st = stage(sim_program, workdir, blob, 0, image=True)
    assert st["status"] == 0, st["error"]
    return st


def fusions(rows):
    """{fused name: (part names, vector suffixes)}: FaceNet's from the table, and the three MTCNN heads"""
    out = {r["name"]: (tuple(r["parts"]), VECS[r["kind"]]) for r in rows if r["nparts"]}
    out.update({k: (v, (".b",)) for k, v in HEADS.items()})
    return out


def row_tensors(r):
    """names of the tensors a row resolves: its matrix, then its vectors"""
    base = "facenet.last_bn" if r["kind"] == 2 else r["name"]
    return [r["name"] + ".w"] + [base + s for s in VECS[r["kind"]]]


def test_the_headers_are_plain_cpp():
    ours = {"trl_facenet.h", "trl_weights.h"}
    for h in ours:
        with open(os.path.join(CSRC, h)) as f:
            includes = [ln.split()[1] for ln in f.read().split("\n") if ln.startswith("#include")]
        assert includes and all("hip" not in i and (i.startswith("<") or i.strip('"') in ours) for i in includes), (h, includes)
    for src in ("trl_api.hip", "trl_nets.hip", "trl_weights.hip"):      # every FaceNet name comes from the table
        with open(os.path.join(CSRC, src)) as f:
            assert '"facenet.' not in f.read(), src


# ---- the table ---------------------------------------------------------------------------------------------------------------

def walk_order():
    """the conv launches of the embedder's walk, in order (what trl_debug_facenet_plan numbers)"""
    names = ["conv2d_1a", "conv2d_2a", "conv2d_2b", "conv2d_3b", "conv2d_4a", "conv2d_4b"]
    for i in range(5):
        names += [f"repeat_1.{i}.{leaf}" for leaf in ("fused", "branch2.1", "branch1.1", "branch2.2", "conv2d")]
    names += [f"mixed_6a.{leaf}" for leaf in ("branch0", "branch1.0", "branch1.1", "branch1.2")]
    for i in range(10):
        names += [f"repeat_2.{i}.{leaf}" for leaf in ("fused", "branch1.1", "branch1.2", "conv2d")]
    names += [f"mixed_7a.{leaf}" for leaf in ("fused", "branch0.1", "branch1.1", "branch2.1", "branch2.2")]
    for p in [f"repeat_3.{i}" for i in range(5)] + ["block8"]:
        names += [f"{p}.{leaf}" for leaf in ("fused", "branch1.1", "branch1.2", "conv2d")]
    return ["facenet." + n for n in names + ["last_linear"]]


def test_table_rows_in_walk_order_with_the_packers_shapes(staged):
    rows = staged["rows"]
    assert len(rows) == 105 and [r["name"] for r in rows] == walk_order()
    shapes = dict(weights._facenet_shapes(), last_linear=(512, 1792, 1, 1))
    used = []
    for r in rows:
        members = r["parts"] or [r["name"]]
        got = [shapes[m[len("facenet."):]] for m in members]
        assert all(g[1:] == (r["cin"], r["kh"], r["kw"]) for g in got) and sum(g[0] for g in got) == r["cout"], r
        used += members
    every = weights.facenet_basic_convs() + weights.facenet_proj_convs() + ["last_linear"]
    assert sorted(used) == sorted("facenet." + n for n in every) and len(set(used)) == len(used)
    proj = {"facenet." + n for n in weights.facenet_proj_convs()}
    for r in rows:
        assert r["kind"] == (2 if r["name"] == "facenet.last_linear" else 1 if r["name"] in proj else 0), r
        assert r["f32_only"] == (r["name"] in ("facenet.conv2d_1a", "facenet.last_linear")), r
        assert r["nparts"] == 0 or (r["kind"] == 0 and (r["kh"], r["kw"], r["sh"], r["sw"], r["ph"], r["pw"]) == (1, 1, 1, 1, 0, 0)), r


def test_rows_resolve_to_their_tensors(staged):
    items = staged["items"]
    assert staged["logits"] == (-1, -1)
    for r, fn in zip(staged["rows"], staged["fn"]):
        want = row_tensors(r)
        assert [items[i]["name"] for i in fn if i >= 0] == want and fn[len(want):] == (-1,) * (3 - len(want)), r
        assert items[fn[0]]["mat"] and (items[fn[0]]["K"], items[fn[0]]["Cout"]) == (r["kh"] * r["kw"] * r["cin"], r["cout"])
        assert all(not items[i]["mat"] and items[i]["n"] == r["cout"] for i in fn[1:] if i >= 0)


# ---- the image ---------------------------------------------------------------------------------------------------------------

def test_image_layout(staged, tensors):
    """Every tensor of the blob, and every fusion as the concatenation of its parts in the table's order, lies in the image at its
    offset: a matrix as [ceil16(K)][ceil32(Cout)], a vector in ceil128(n) floats, zeros in all padding and between items; offsets
    are multiples of 256 and no two items overlap."""
    items, image = staged["items"], staged["image"]
    assert staged["total"] == len(image)
    want = dict(tensors)
    for out, (parts, sfx) in fusions(staged["rows"]).items():
        for s in (".w",) + sfx:
            want[out + s] = np.concatenate([tensors[p + s] for p in parts], axis=-1)
    assert [it["name"] for it in items[:len(tensors)]] == list(tensors)          # directory order, then the fusions
    assert sorted(it["name"] for it in items) == sorted(want)
    expect = np.zeros(len(image) // 4, np.float32)
    end = 0
    for it in items:
        a = want[it["name"]]
        assert it["off"] % 256 == 0 and it["off"] >= end, it
        if it["mat"]:
            assert a.shape == (it["K"], it["Cout"]) and it["Kpad"] == -(-it["K"] // 16) * 16 and it["ld"] == -(-it["Cout"] // 32) * 32, it
            n = it["Kpad"] * it["ld"]
            expect[it["off"] // 4:it["off"] // 4 + n].reshape(it["Kpad"], it["ld"])[:it["K"], :it["Cout"]] = a
        else:
            assert a.shape == (it["n"],), it
            n = -(-it["n"] // 128) * 128
            expect[it["off"] // 4:it["off"] // 4 + it["n"]] = a
        end = it["off"] + 4 * n
    assert end <= len(image) < end + 256
    assert np.array_equal(image, expect.view(np.uint8))                          # bit for bit, padding included


# ---- refusals ----------------------------------------------------------------------------------------------------------------

def refused(program, workdir, blob, names, precision=0):
    st = stage(program, workdir, blob, precision)
    assert st["status"] == REFUSED and any(n in st["error"] for n in names), (st["status"], st["error"], names)


def test_every_needed_tensor_is_missed_by_name(sim_program, workdir, blob, tensors, staged):
    """Each FaceNet tensor a row resolves and each part of each fusion (MTCNN heads included), removed in turn"""
    names = []
    for out, (parts, sfx) in fusions(staged["rows"]).items():
        names += [p + s for p in parts for s in (".w",) + sfx]
    for r in staged["rows"]:
        if not r["nparts"]:
            names += row_tensors(r)
    heads = {p + s for parts in HEADS.values() for p in parts for s in (".w", ".b")}
    assert len(names) == len(set(names)) and set(names) == {k for k in tensors if k.startswith("facenet.")} | heads   # every one is needed
    path = str(workdir / "drop.blob")
    with open(path, "wb") as f:
        f.write(blob)
    p = subprocess.run([sim_program, path, "0", "--drop"], input="\n".join(names) + "\n", capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    lines = p.stdout.split("\n")[:-1]
    assert len(lines) == len(names)
    for name, ln in zip(names, lines):
        tag, got, status, msg = ln.split(" ", 3)
        assert (tag, got, int(status)) == ("drop", name, REFUSED) and name in msg, ln


def test_misshaped_tensors_are_refused_by_name(sim_program, workdir, tensors):
    t = tensors
    wide = lambda a: np.concatenate([a, a[..., :1]], axis=-1)
    tall = lambda a: np.concatenate([a, a[:1]], axis=0)
    # a vector one element short: of a plain row, of an up-projection, of the final linear, of a fusion's part
    for name in ("facenet.conv2d_2a.scale", "facenet.repeat_2.3.conv2d.b", "facenet.last_bn.shift", "facenet.repeat_1.0.branch0.shift",
                 "onet.dense6_2.b"):
        refused(sim_program, workdir, weights.pack_tensors({**t, name: t[name][:-1]}), [name])
    # a matrix with one column or one K row too many
    for name in ("facenet.conv2d_2a.w", "facenet.repeat_3.1.conv2d.w", "facenet.last_linear.w"):
        for grow in (wide, tall):
            refused(sim_program, workdir, weights.pack_tensors({**t, name: grow(t[name])}), [name])
    # a part one column wider with its vectors: the fused conv no longer has the table's columns
    p = "facenet.repeat_2.0.branch1.0"
    refused(sim_program, workdir, weights.pack_tensors({**t, **{p + s: wide(t[p + s]) for s in (".w", ".scale", ".shift")}}),
            ["facenet.repeat_2.0.fused.w"])
    # two parts of a fusion that disagree on K
    for name in ("facenet.repeat_2.0.branch1.0.w", "facenet.mixed_7a.branch2.0.w", "rnet.dense5_2.w"):
        st = stage(sim_program, workdir, weights.pack_tensors({**t, name: tall(t[name])}))
        assert st["status"] == REFUSED and name in st["error"] and "disagree on K" in st["error"], st["error"]


def test_logits_pair_rule(sim_program, workdir, tensors):
    rng = np.random.default_rng(5)
    w, b = rng.standard_normal((512, 33)).astype(np.float32), rng.standard_normal(33).astype(np.float32)
    wn, bn = "facenet.logits.w", "facenet.logits.b"
    st = stage(sim_program, workdir, weights.pack_tensors({**tensors, wn: w, bn: b}))
    assert st["status"] == 0 and [st["items"][i]["name"] for i in st["logits"]] == [wn, bn]
    refused(sim_program, workdir, weights.pack_tensors({**tensors, wn: w}), [bn])
    refused(sim_program, workdir, weights.pack_tensors({**tensors, bn: b}), [wn])
    refused(sim_program, workdir, weights.pack_tensors({**tensors, wn: w[:511], bn: b}), [wn])
    refused(sim_program, workdir, weights.pack_tensors({**tensors, wn: w, bn: b[:-1]}), [bn])


def poked(blob, name, index, value):
    """``blob`` with element ``index`` of matrix ``name`` set to ``value``"""
    (n,) = struct.unpack_from("<I", blob, 8)
    for i in range(n):
        nm, ndim, d0, d1, _, _, off, _nb = weights._ENTRY.unpack_from(blob, 16 + i * weights._ENTRY.size)
        if nm.rstrip(b"\0").decode() == name:
            b = bytearray(blob)
            struct.pack_into("<f", b, off + 4 * (index[0] * d1 + index[1]), value)
            return bytes(b)
    raise KeyError(name)


def test_fp16_range_rule(sim_program, workdir, blob):
    """embed_precision 2 refuses a weight that fp16 would round to inf, in the convs that get an fp16 copy: named by the matrix the
    walk uses (a part's by its fused conv's).  The f32-only layers, 65519 (rounds to 65504) and precisions 0 / 1 take it."""
    plain = poked(blob, "facenet.repeat_2.3.branch1.1.w", (5, 7), 7e4)
    part = poked(blob, "facenet.repeat_1.0.branch2.0.w", (200, 31), -7e4)
    f32 = poked(poked(blob, "facenet.conv2d_1a.w", (26, 31), 7e4), "facenet.last_linear.w", (1791, 511), 7e4)
    refused(sim_program, workdir, plain, ["facenet.repeat_2.3.branch1.1.w[%d]" % (5 * 128 + 7)], 2)
    refused(sim_program, workdir, part, ["facenet.repeat_1.0.fused.w[%d]" % (200 * 96 + 32 + 31)], 2)
    refused(sim_program, workdir, poked(blob, "facenet.repeat_2.3.branch1.1.w", (5, 7), float("nan")), ["facenet.repeat_2.3.branch1.1.w"], 2)
    for b, precisions in ((f32, (2,)), (poked(blob, "facenet.repeat_2.3.branch1.1.w", (5, 7), 65519.0), (2,)), (plain, (0, 1)), (part, (0, 1))):
        for p in precisions:
            st = stage(sim_program, workdir, b, p)
            assert st["status"] == 0, (p, st["error"])


def test_broken_directories_are_refused(sim_program, workdir, blob):
    (n,) = struct.unpack_from("<I", blob, 8)
    ent = weights._ENTRY

    def patched(i, **kw):
        b = bytearray(blob)
        f = list(ent.unpack_from(b, 16 + i * ent.size))
        for k, v in kw.items():
            f[{"ndim": 1, "d0": 2, "d1": 3, "off": 6, "nb": 7}[k]] = v
        ent.pack_into(b, 16 + i * ent.size, *f)
        return bytes(b)
    _, _, d0, _, _, _, _, nb = ent.unpack_from(blob, 16)
    for bad, text in ((b"XXXXXXXX" + blob[8:], "magic"), (blob[:8], "magic"), (blob[:16 + ent.size * n - 8], "truncated"),
                      (patched(n - 1, off=len(blob) - 4), "bounds"), (patched(0, off=2 ** 63, nb=2 ** 63), "bounds"),
                      (patched(0, off=ent.unpack_from(blob, 16)[6] + 2), "bounds"),
                      (patched(0, d0=d0 + 1), "byte count"), (patched(0, nb=nb - 4), "byte count")):
        st = stage(sim_program, workdir, bad)
        assert st["status"] == REFUSED and text in st["error"], (text, st["error"])
