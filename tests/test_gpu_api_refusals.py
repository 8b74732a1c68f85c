"""The context-bound entry points on a context: what each answers on a context without weights, on an idle one to every argument
it refuses, and while a call is queued -- status and message, against tests/golden/api_refusals.json (tests/api_refusal_cases.py
has the table and says how the golden file was recorded).  Raw ctypes, one context per state, one 32 x 32 frame; the queued
trl_detect_embed_begin is the only call that launches a kernel.

And the device rule of the inspection hooks: they select the context's device before they synchronise and copy."""
import json

import numpy as np
import pytest
import torch

from api_refusal_cases import GOLDEN, NOT_IN_FLIGHT, context_bound, names_of, run, text

pytestmark = pytest.mark.gpu
TRL_ERR_STATE = -5
IN_FLIGHT_TEXT = "the context has a call in flight: trl_detect_embed_end() first"


@pytest.fixture(scope="module")
def answers():
    return run(("no_weights", "idle", "in_flight"))


@pytest.mark.parametrize("section", ["no_weights", "idle", "in_flight"])
def test_answers_equal_the_recorded_ones(answers, section):
    got, want = answers[section], json.load(open(GOLDEN))[section]
    labels = [c[0] for c in got]
    assert len(set(labels)) == len(labels)
    for g, w in zip(got, want):
        assert g == w
    assert text(got) == text(want)                                         # ... and nothing missing or added


def test_every_entry_meets_a_queued_call(answers):
    """all context-bound names but trl_create, trl_default_config and trl_destroy are called between _begin and _end; an entry
    that refuses the queued call does so with TRL_ERR_STATE and the one text, the others answer as on an idle context"""
    rows = answers["in_flight"]
    assert names_of(rows) == set(context_bound()) - NOT_IN_FLIGHT
    assert rows[0][1:] == [0, ""] and rows[-1][1:] == [0, ""]             # the queued call itself, and its end
    host_only = {"trl_debug_timings", "trl_debug_pnet_run", "trl_debug_stage_totals", "trl_debug_list_stats", "trl_debug_pnet_kernel_ms",
                 "trl_debug_pnet_screen_bound", "trl_debug_pnet_screen_weights", "trl_debug_pnet_defer", "trl_debug_batch_capacity",
                 "trl_facenet_num_classes"}
    # never refused a queued call, and would launch: called with what they refuse or with the empty batch (api_refusal_cases.py)
    unchecked = {"trl_load_weights", "trl_drift_score", "trl_drift_update", "trl_ingest_nv12", "trl_ingest_i420", "trl_debug_crop_resize",
                 "trl_debug_crop_aligned", "trl_debug_crop_area"}
    for label, status, message in rows[1:-1]:
        name = label.split("(")[0]
        if name in host_only or label.startswith("trl_debug_option(key="):         # (the two process-wide keys)
            assert (status, message) == (0, ""), label
        elif name in unchecked:
            assert message != IN_FLIGHT_TEXT and status in (0, -1), label
        else:
            assert (status, message) == (TRL_ERR_STATE, IN_FLIGHT_TEXT), label


def test_inspection_hooks_select_the_contexts_device():
    """stage_boxes, level_counts, level_cands and level_keep of a context on device 1, read with device 0 current, equal the same
    reads with device 1 current"""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible GPUs: the context lives on device 1 while device 0 is current")
    import truely_amd
    from truely_amd.engine import Engine
    eng = Engine(truely_amd.weights.synthetic_blob(0), device=1)
    try:
        eng.detect_embed(truely_amd.synthetic.synthetic_frames(2, 97, 131, seed=3))

        def read():
            out = []
            for f in range(2):
                cand, keep = eng.level_counts(f)
                out += [np.asarray(cand), np.asarray(keep)] + [eng.stage_boxes(s, f) for s in (1, 2, 3)]
                for l in range(len(cand)):
                    rec, idx = eng.level_keep(f, l)
                    out += [eng.level_cands(f, l), rec, idx]
            return out
        torch.cuda.set_device(1)
        want = read()
        torch.cuda.set_device(0)
        got = read()
        assert len(got) == len(want) and sum(len(a) for a in want) > 0
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()
    finally:
        torch.cuda.set_device(0)
        eng.close()
