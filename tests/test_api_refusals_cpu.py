"""The context-bound entry points without a GPU: what each answers to a null context, trl_create to every bad trl_config field and
to null arguments, trl_default_config(NULL) and trl_debug_option to a null key and to its two process-wide keys -- status and
message, against the "null" section of tests/golden/api_refusals.json.  tests/api_refusal_cases.py has the table and says how the
golden file was recorded; tests/test_gpu_api_refusals.py reads the sections that need a context."""
import json

from api_refusal_cases import GOLDEN, context_bound, names_of, run, text


def test_no_context_bound_entry_is_missing_from_the_table():
    """every name of _lib._SIGNATURES outside the context-free families has a null-context (trl_create, trl_default_config: a null
    argument) case -- here and in the golden file, so an entry added later cannot be forgotten"""
    bound = context_bound()
    assert len(bound) == 61 and len(set(bound)) == 61, bound            # 2 + 21 product entries + 38 hooks (ABI 7)
    assert names_of(run(("null",))["null"]) == set(bound)
    assert names_of(json.load(open(GOLDEN))["null"]) == set(bound)


def test_null_context_answers_equal_the_recorded_ones():
    got, want = run(("null",))["null"], json.load(open(GOLDEN))["null"]
    labels = [c[0] for c in got]
    assert len(set(labels)) == len(labels)
    assert all(status in (0, -1, -5) for _l, status, _m in got)          # TRL_OK, TRL_ERR_INVALID, TRL_ERR_STATE: no case reached HIP
    for g, w in zip(got, want):
        assert g == w
    assert text(got) == text(want)                                         # ... and nothing missing or added
