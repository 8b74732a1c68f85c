"""k_extract_plan / k_extract (csrc/trl_extract.hip) on extract_ref.TABLE: every resampler path, LDS tap chunk count, output size
from 1 to 1024, fast-area form, margin and frame edge that the C ABI accepts (test_extract_cpu.py checks that the table reaches
them).  trl_extract_faces is called directly on buffers prefilled with NaN and followed by NaN guards: every row must equal
extract_ref.extract bit for bit, the statuses must be equal and no cell outside the rows may change.  The largest cases run again
over poisoned workspaces, on a side stream, and with a small S after a large one on the same context; trl_area_pixel's sum is
checked on a bin of more than 2^32 / 255 pixels."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import extract_ref as R
from truely_amd import _lib
from truely_amd.engine import RESAMPLERS

pytestmark = pytest.mark.gpu
GUARD = 4096                                     # guard words behind the faces and behind the statuses
NAN_BITS = np.float32(np.nan).view(np.int32)
BY_NAME = {c["name"]: c for c in R.TABLE}


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _extract(eng, frames, rows, S, margin, resample, post):
    """trl_extract_faces on the current stream -> (faces [m, S, S, 3], face guard, statuses [m], status guard) on the host"""
    dev = eng.device
    fr = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(frames).to(dev)
    n, H, W, _ = fr.shape
    m = len(rows)
    frame_of = torch.tensor([f for f, _b in rows], dtype=torch.int32, device=dev)
    boxes = torch.tensor([b for _f, b in rows], dtype=torch.float32, device=dev).reshape(-1, 4)
    out = torch.full((m * S * S * 3 + GUARD,), float("nan"), dtype=torch.float32, device=dev)
    status = torch.full((m + GUARD,), float("nan"), dtype=torch.float32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(eng.lib.trl_extract_faces(eng._h, _ptr(fr), n, H, W, _ptr(frame_of), _ptr(boxes), m, S, margin, RESAMPLERS[resample],
                                         int(post), _ptr(out), _ptr(status), stream))
    torch.cuda.current_stream(dev).synchronize()
    o, s = out.cpu().numpy(), status.view(torch.int32).cpu().numpy()
    return o[:m * S * S * 3].reshape(m, S, S, 3), o[m * S * S * 3:], s[:m], s[m:]


def _run_case(eng, case, resample, what=""):
    faces, fguard, status, sguard = _extract(eng, R.case_frames(case), case["rows"], case["S"], case["margin"], resample, case["post"])
    ref_faces, ref_status = R.expected(case, resample)
    tag = (what, case["name"], resample)
    assert np.array_equal(status, ref_status), (tag, status.tolist(), ref_status.tolist())
    assert np.isnan(fguard).all() and (sguard == NAN_BITS).all(), tag
    for r in range(len(case["rows"])):
        assert np.array_equal(faces[r], ref_faces[r]), (tag, r, int((faces[r] != ref_faces[r]).sum()))


@pytest.mark.parametrize("resample", R.RESAMPLERS)
@pytest.mark.parametrize("name", list(BY_NAME))
def test_table_case_equals_restatement(engine, name, resample):
    _run_case(engine, BY_NAME[name], resample)


@pytest.mark.parametrize("resample", R.RESAMPLERS)
def test_largest_cases_over_poisoned_workspaces(engine, resample):
    """The plan lives in the context's scratch arena: NaN bytes in it (and in LDS) may not reach a face."""
    eng = engine.clone()
    try:
        eng.poison_workspaces(0xFF)
        for name in ("tall200", "taps171", "tall1024", "vfirst87s160"):
            _run_case(eng, BY_NAME[name], resample, "poisoned")
    finally:
        eng.close()


@pytest.mark.parametrize("resample", R.RESAMPLERS)
def test_side_stream_and_small_size_after_large(engine, resample):
    """A call on a non-default stream; then, on the same context, S = 7 and S = 160 after S = 1024: a plan left in the arena by
    the larger call may not show in the smaller one's rows."""
    side = torch.cuda.Stream(engine.device)
    with torch.cuda.stream(side):
        _run_case(engine, BY_NAME["tall1024"], resample, "side stream")
        _run_case(engine, BY_NAME["edges7m3"], resample, "side stream, after S = 1024")
    side.synchronize()
    _run_case(engine, BY_NAME["order160"], resample, "after S = 1024")
    _run_case(engine, BY_NAME["fast86"], resample, "after S = 160")


def test_area_sum_of_a_bin_past_32_bits(engine):
    """torch resampler, S = 1 on a 4105 x 4104 crop of 255s: the bin sums to 255 * 16 846 920 > 2^32.  S = 2 stays below it."""
    fr = torch.full((1, 4105, 4104, 3), 255, dtype=torch.uint8, device=engine.device)
    rows = [(0, (0.0, 0.0, 4104.0, 4105.0))]
    for S in (2, 1):
        t0 = time.perf_counter()
        faces, fguard, status, sguard = _extract(engine, fr, rows, S, 0, "torch", False)
        print(f"S = {S}: {time.perf_counter() - t0:.3f} s")
        assert status.tolist() == [1] and np.isnan(fguard).all() and (sguard == NAN_BITS).all()
        assert np.array_equal(faces, np.full((1, S, S, 3), 255, np.float32)), (S, faces.ravel()[:12].tolist())
