"""The cascade's list kernels -- k_nms_level, k_nms_frame, k_stage2_post, k_stage3_post, k_select -- on lists built to sit on
their edges, against tests/list_ref.py (detect_face's post-processing restated in numpy / torch float32).

trl_debug_lists runs them through the cascade's own launch code on the lists it is given.  Every case runs at the default
LDS tiers (512 / 2048), at (16, 64) and at the non-power-of-two tiers (100, 300) and (500, 3072), with list lengths at the small
and full tier -1 / = / +1, at power-of-two edges, at the spill chunk C, C + 1 and 2 C + 1 (kept counts that cross the 'Min'
tile TK and 2 TK).  Checked: counts, rows in order, keep indices, landmarks, and k_select's boxes / probs / points / rect /
valid.  Score ties are fed in two append orders; the largest cases run once more over 0xFF and 0x7F workspaces."""
import numpy as np
import pytest

import list_ref as R

pytestmark = pytest.mark.gpu

TIERS = [(512, 2048), (16, 64), (100, 300), (500, 3072)]
FAMILIES = ("dup", "cell", "chain", "special")
MAX_FACES = 64               # trl_default_config


_REF = {}


def _ref(oracle, kind, fam, n, part):
    key = (kind, fam, n, part)
    if key not in _REF:
        case = R.build_case(kind, fam, n, part=part)
        _REF[key] = (case, R.reference(case, oracle.expf, max_faces=MAX_FACES))
    return _REF[key]


def _run(eng, case, order=None):
    caps, counts, rows, logits, sent = R.hook_args(case, order)
    got = eng.lists(case["kind"], case["H"], case["W"], caps, counts, rows, logits)
    got["sent"] = sent
    return got


def _check(case, ref, got, tag):
    kind = case["kind"]
    for f, rf in enumerate(ref):
        if kind == 1:
            for l, rec in enumerate(got["sent"][f]):
                cells = rec["cell"][got["keep"][f][l]]
                assert np.array_equal(cells, rf["keep_cells"][l]), f"{tag} level {l}: keep list ({len(cells)} vs {len(rf['keep_cells'][l])})"
        k = f"rows{kind}"
        a, b = got[k][f], rf[k]
        assert a.shape == b.shape, f"{tag} frame {f}: {k} count {len(a)} vs {len(b)}"
        assert np.array_equal(a, b), f"{tag} frame {f}: {k} first differing row {np.flatnonzero((a != b).any(1))[:3]}"
        if kind == 3:
            assert np.array_equal(got["pts3"][f], rf["pts3"]), f"{tag} frame {f}: landmarks"
            s = rf["sel"]
            c = s["count"]
            assert got["counts"][f] == c, f"{tag} frame {f}: selected count"
            assert np.array_equal(got["boxes"][f, :c], s["boxes"]), f"{tag} frame {f}: selected boxes (area order)"
            assert np.array_equal(got["probs"][f, :c], s["probs"]), f"{tag} frame {f}: selected probs"
            assert np.array_equal(got["points"][f, :c], s["points"]), f"{tag} frame {f}: selected points"
            assert np.array_equal(got["box0"][f], s["box0"]) and got["prob0"][f] == s["prob0"], f"{tag} frame {f}: box0"
            assert np.array_equal(got["rect"][f], s["rect"]), f"{tag} frame {f}: rect {got['rect'][f]} vs {s['rect']}"
            assert got["valid"][f] == s["valid"], f"{tag} frame {f}: valid"


def _expect_spill(case, ref, tiers):
    """(lists, bytes): the lists that the routing restatement sends to the spill tier and the pool bytes they request
    (list_stats reports both)."""
    lv, fr = R.list_lengths(case, ref)
    ll = R.launch(tiers[0], tiers[1], case["caps"][:-1], case["caps"][-1])
    W, H, kind = case["W"], case["H"], case["kind"]
    spilled = [R.spill_bytes(1, "level", c, W, H) for c in lv if R.route(ll, c, True)[0] == "spill"]
    spilled += [R.spill_bytes(kind, "frame", c, W, H) for c in fr if c > 0 and R.route(ll, c, False)[0] == "spill"]
    return len(spilled), sum(spilled)


@pytest.fixture(scope="module")
def list_engine(blob):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from truely_amd.engine import Engine
    eng = Engine(blob)
    assert eng.cfg.max_faces == MAX_FACES
    return eng


@pytest.mark.parametrize("tiers", TIERS, ids=lambda t: f"{t[0]}-{t[1]}")
@pytest.mark.parametrize("kind", ["1-level", "1-frame", "2", "3"])
def test_list_kernels_at_edges(list_engine, oracle, tiers, kind):
    eng = list_engine
    eng.nms_tiers(*tiers)
    k, part = (1, kind[2:]) if kind.startswith("1") else (int(kind), "level")
    try:
        for n in R.edges(*tiers):
            for fam in FAMILIES:
                case, ref = _ref(oracle, k, fam, n, part)
                got = _run(eng, case, order=1 if k == 1 else None)
                _check(case, ref, got, f"tiers {tiers} kind {kind} {fam} n={n}")
                st = eng.list_stats()
                assert (st["spill_lists"], st["spill_used"]) == _expect_spill(case, ref, tiers), (tiers, kind, fam, n, st)
    finally:
        eng.nms_tiers(512, 2048)


def test_ties_do_not_depend_on_append_order(list_engine, oracle):
    """Exact score ties at one level (the special list) and whole lists fed in three append orders: the picks are the same cells."""
    eng = list_engine
    for tiers in ((512, 2048), (16, 64)):
        eng.nms_tiers(*tiers)
        for fam in FAMILIES:
            for n in (17, 65, 600):
                case, ref = _ref(oracle, 1, fam, n, "level")
                for order in (None, 2, 3):
                    _check(case, ref, _run(eng, case, order), f"tiers {tiers} {fam} n={n} order {order}")
    eng.nms_tiers(512, 2048)


@pytest.mark.parametrize("byte", [0xFF, 0x7F])
def test_largest_lists_over_poisoned_workspaces(blob, oracle, byte):
    """The largest cases over workspaces (and record slots past the counts) filled with NaN (0xFF) / huge-float (0x7F) bytes."""
    from truely_amd.engine import Engine
    eng = Engine(blob)
    eng.poison_workspaces(byte)
    for tiers in ((512, 2048), (16, 64)):
        eng.nms_tiers(*tiers)
        for kind, part in ((1, "level"), (1, "frame"), (2, "level"), (3, "level")):
            for fam in FAMILIES:
                case, ref = _ref(oracle, kind, fam, 4097, part)
                _check(case, ref, _run(eng, case), f"poison {byte:#x} tiers {tiers} kind {kind} {fam}")
