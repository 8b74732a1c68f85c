"""The configuration's way into the library, and the reference answers tests/test_gpu_config.py leans on (no GPU).

  * include/truely_hip.h against the ctypes binding: trl_config field by field (name, order, C type) and every prototype's
    return and argument classes against _lib._SIGNATURES -- test_header_symbols_exported_by_library compares names only, and a
    float field out of order would put thr1 into thr2 without a sound.  The same for the oracle's parameter struct.
  * list_ref.probs at both ends of its range: one float for every logit difference at or below the exponent clamp, and 1.0f from
    one difference on.
  * oracle.detect loses exactly one stage-2 (stage-3) row when thr1 (thr2) moves from one float below a row's probability onto it."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import truely_amd
from truely_amd import _lib
import list_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ---- a small C declaration parser: enough for the two headers ----------------------------------------------------------------
def _strip(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return "\n".join(l for l in text.split("\n") if not l.lstrip().startswith("#"))


def _c_class(decl):
    """the class of a C return or parameter declaration: "ptr", "i32", "i64", "size_t", "f32", "f64" or "void\""""
    if "*" in decl or "[" in decl:
        return "ptr"
    words = [w for w in re.findall(r"[A-Za-z_]\w*", decl) if w not in ("const", "unsigned", "signed", "struct")]
    if words[:2] == ["long", "long"]:
        return "i64"
    return {"int": "i32", "int32_t": "i32", "uint32_t": "i32", "int64_t": "i64", "uint64_t": "i64", "long": "i64", "size_t": "size_t",
            "float": "f32", "double": "f64", "void": "void"}.get(words[0], words[0])      # (a struct by value: its own name)


def _ctypes_class(t):
    if t is None:
        return "void"
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return "ptr"
    if t is C.c_size_t:
        return "size_t"
    if t is C.c_float:
        return "f32"
    if t is C.c_double:
        return "f64"
    assert issubclass(t, C._SimpleCData) and t._type_ in "iIlLqQ", t
    return {4: "i32", 8: "i64"}[C.sizeof(t)]


def parse_struct(text, name):
    """[(field, class)] of `typedef struct { ... } name;` (scalar fields, several declarators per line allowed)"""
    m = re.search(r"typedef\s+struct\s*(?:\w+\s*)?\{([^{}]*)\}\s*" + name + r"\s*;", _strip(text))
    assert m, f"struct {name} not found"
    fields = []
    for stmt in m.group(1).split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        typ, names = re.match(r"((?:const\s+|unsigned\s+)*(?:long\s+long|\w+))\s+(.*)$", stmt, flags=re.S).groups()
        for n in names.split(","):
            fields.append((n.strip(), _c_class(typ + (" *" if "*" in n else ""))))
    return fields


def parse_prototypes(text, prefix):
    """{function: (return class, [argument classes])} of every prototype whose name starts with `prefix`"""
    flat = re.sub(r"\{[^{}]*\}", " ", _strip(text))              # struct and enum bodies hold no prototypes
    out = {}
    for m in re.finditer(r"([\w\s\*]+?)\b(" + prefix + r"\w+)\s*\(([^()]*)\)\s*;", flat):
        ret, name, args = m.groups()
        ret = ret.split(";")[-1].replace("extern", " ").strip()
        args = [] if args.strip() in ("", "void") else [_c_class(a) for a in args.split(",")]
        assert name not in out, name
        out[name] = (_c_class(ret + " "), args)
    return out


def struct_mismatches(parsed, fields):
    want = [(n, _ctypes_class(t)) for n, t in fields]
    return [(a, b) for a, b in itertools.zip_longest(parsed, want) if a != b]


def signature_mismatches(parsed, table):
    bad = [(n, "missing") for n in set(parsed) ^ set(table)]
    for n in set(parsed) & set(table):
        res, args = table[n]
        got = (_ctypes_class(res), [_ctypes_class(a) for a in args])
        if got != parsed[n]:
            bad.append((n, parsed[n], got))
    return bad


@pytest.fixture(scope="module")
def header():
    return open(os.path.join(ROOT, "include", "truely_hip.h")).read()


def test_trl_config_fields_equal_the_ctypes_struct(header):
    parsed = parse_struct(header, "trl_config")
    assert [n for n, _ in parsed] == ["device", "min_face_size", "thr0", "thr1", "thr2", "factor", "cap_level", "cap_frame", "max_faces",
                                      "pnet_mode", "embed_mode", "embed_precision"]
    fields = list(_lib.TrlConfig._fields_)
    assert struct_mismatches(parsed, fields) == []
    # the comparison can fail: two floats swapped, a float read as an int, a field dropped
    i1, i2 = [n for n, _ in fields].index("thr1"), [n for n, _ in fields].index("thr2")
    swapped = list(fields); swapped[i1], swapped[i2] = swapped[i2], swapped[i1]
    assert struct_mismatches(parsed, swapped)
    assert struct_mismatches(parsed, [(n, C.c_int if n == "thr2" else t) for n, t in fields])
    assert struct_mismatches(parsed, [(n, C.c_float if n == "factor" else t) for n, t in fields])
    assert struct_mismatches(parsed, fields[:-1])
    # and the layout the library sees is the one ctypes writes: the defaults arrive in their own fields
    cfg = _lib.TrlConfig()
    assert _lib.load().trl_default_config(C.byref(cfg)) == 0
    assert (cfg.min_face_size, F32(cfg.thr0), F32(cfg.thr1), F32(cfg.thr2), cfg.factor, cfg.max_faces) == (20, F32(0.6), F32(0.7), F32(0.7), 0.709, 64)


def test_other_header_structs_equal_their_ctypes_structs(header):
    for name, cls in (("trl_jpegd_info", _lib.TrlJpegdInfo), ("trl_jpeg_options", _lib.TrlJpegOptions)):
        assert struct_mismatches(parse_struct(header, name), list(cls._fields_)) == [], name


def test_every_prototype_equals_its_ctypes_signature(header):
    parsed = parse_prototypes(header, "trl_")
    assert len(parsed) >= 95 and set(parsed) == set(_lib._SIGNATURES)
    assert parsed["trl_select_faces"] == ("i32", ["ptr", "i32", "ptr", "ptr", "ptr", "i32", "i32", "i32", "f32", "f64", "ptr", "ptr"])
    assert parsed["trl_draw_workspace"] == ("size_t", ["i32", "i32"])
    assert parsed["trl_last_error"] == ("ptr", [])
    assert signature_mismatches(parsed, _lib._SIGNATURES) == []
    # the comparison can fail: float and double swapped, an int widened, an argument dropped, a return class changed
    table = dict(_lib._SIGNATURES)
    res, args = table["trl_select_faces"]
    mut = list(args); mut[8], mut[9] = mut[9], mut[8]
    assert [b[0] for b in signature_mismatches(parsed, {**table, "trl_select_faces": (res, mut)})] == ["trl_select_faces"]
    res, args = table["trl_debug_batch_capacity"]
    assert signature_mismatches(parsed, {**table, "trl_debug_batch_capacity": (res, [args[0], C.c_double] + list(args[2:]))})
    res, args = table["trl_debug_redzone"]
    assert signature_mismatches(parsed, {**table, "trl_debug_redzone": (res, [args[0], C.c_int, args[2]])})
    assert signature_mismatches(parsed, {**table, "trl_destroy": (C.c_int, [])})
    assert signature_mismatches(parsed, {**table, "trl_draw_workspace": (C.c_int, table["trl_draw_workspace"][1])})
    assert signature_mismatches(parsed, {k: v for k, v in table.items() if k != "trl_create"})


def test_oracle_params_equal_the_ctypes_struct():
    from oracle import oracle as O
    text = open(os.path.join(ROOT, "oracle", "trl_oracle.h")).read()
    parsed = parse_struct(text, "orc_params")
    assert [n for n, _ in parsed] == ["min_face_size", "thr0", "thr1", "thr2", "factor"]
    fields = list(O.Params._fields_)
    assert struct_mismatches(parsed, fields) == []
    swapped = [fields[0], fields[1], fields[3], fields[2], fields[4]]
    assert struct_mismatches(parsed, swapped)
    protos = parse_prototypes(text, "orc_")
    assert protos["orc_expf"] == ("f32", ["f32"]) and protos["orc_detect"][1][4] == "ptr"


# ---- reference known answers ---------------------------------------------------------------------------------------------------
def _p1(oracle, d, a0=0.0):
    return R.probs(oracle.expf, np.array([[a0, F32(a0) + F32(d)]], F32))[0]


def test_reference_softmax_clamps_and_saturates(oracle):
    low = [_p1(oracle, d) for d in (-87.0, -104.0, -200.0, -3e38)]
    assert all(v == R.CLAMP_PROB for v in low) and R.CLAMP_PROB > 0
    assert R.probs(oracle.expf, np.array([[3e38, -3e38]], F32))[0] == R.CLAMP_PROB        # the difference itself is -inf
    assert _p1(oracle, -86.9) > R.CLAMP_PROB
    # 1.0f from one difference on: bisect to adjacent floats, then look two floats to either side
    lo, hi = F32(16.0), F32(17.0)
    assert _p1(oracle, lo) < 1 and _p1(oracle, hi) == 1
    while np.nextafter(lo, F32(np.inf)) < hi:
        mid = F32((lo + hi) / F32(2))
        lo, hi = (lo, mid) if _p1(oracle, mid) == 1 else (mid, hi)
    assert F32(16.6) < hi < F32(16.7)                        # (tests/list_ref.py RANGE_DIFFS stands on both sides of it)
    below = np.nextafter(np.nextafter(lo, F32(0)), F32(0))
    above = np.nextafter(np.nextafter(hi, F32(np.inf)), F32(np.inf))
    assert [_p1(oracle, d) == 1 for d in (below, np.nextafter(lo, F32(0)), lo, hi, np.nextafter(hi, F32(np.inf)), above)] == [False] * 3 + [True] * 3
    assert _p1(oracle, 200.0) == 1 and _p1(oracle, 1e4) == 1 and R.probs(oracle.expf, np.array([[-3e38, 3e38]], F32))[0] == 1
    # the list the GPU test walks reaches both ends and the middle
    p = R.probs(oracle.expf, R.range_logits())
    assert (p == 1).any() and (p == R.CLAMP_PROB).any() and len(np.unique(p[(p > F32(0.01)) & (p < F32(0.99))])) >= 50


@pytest.fixture(scope="module")
def orc(blob):
    from oracle.oracle import Oracle
    return Oracle(blob)                                       # its params are changed below; the session's oracle keeps the defaults


def _counts(orc, frame, thr):
    orc.params.thr0, orc.params.thr1, orc.params.thr2 = (float(t) for t in thr)
    tr = orc.detect(frame, trace=True, max_trace=1 << 14)[2]
    return tr, (len(tr["boxes2"]), len(tr["boxes3"]))


def test_oracle_counts_at_stage_thresholds(orc):
    """the per-frame (stage-2, stage-3) counts tests/test_gpu_config.py pins for its clip"""
    from test_gpu_config import TRIPLES
    clip = truely_amd.synthetic.synthetic_frames(2, 180, 320, seed=11, faces=-1)
    for triple, want in [((0.6, 0.7, 0.7), [(15, 3), (13, 4)])] + TRIPLES:
        assert [_counts(orc, f, triple)[1] for f in clip] == want, triple


def test_oracle_threshold_on_a_rows_probability(orc):
    frame = truely_amd.synthetic.synthetic_frames(2, 180, 320, seed=11, faces=-1)[0]
    tr, n = _counts(orc, frame, (0.6, 0.0, 0.0))
    assert n == (30, 8)
    p2, p3 = (np.sort(tr[k][:, 4])[len(tr[k]) // 2] for k in ("boxes2", "boxes3"))
    assert (p2, p3) == (F32(0.7162569), F32(0.6642022))
    for stage, p, want in ((2, p2, [15, 14]), (3, p3, [4, 3])):
        got = []
        for t in (np.nextafter(p, F32(0)), p):
            tr, n = _counts(orc, frame, (0.6, t, 0.0) if stage == 2 else (0.6, 0.0, t))
            got.append(n[stage - 2])
            assert (tr[f"boxes{stage}"][:, 4] == p).any() == (len(got) == 1)      # strict: the row ON the threshold goes
        assert got == want
