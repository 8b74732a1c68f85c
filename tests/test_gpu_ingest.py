"""The 4:2:0 ingest path on the GPU (csrc/trl_ingest.hip: k_nv12_to_bgr<PLANAR> behind trl_ingest_nv12 / trl_ingest_i420,
Engine.ingest_nv12, ingest.Nv12Uploader) against the plain restatement tests/ingest_ref.py.  Every comparison is byte equality
with ingest_ref.yuv420_to_bgr of the bytes the kernel was given, in both layouts (NV12, I420):

  A  the whole (Y, U, V) cube in one 4096 x 4096 frame
  B  shapes from 2x4 to 4K x every (n_in, step) pair x every content kind
  C  production batches: the grid-stride loop's first (ragged) wrap and the benchmark's 256 x 720p, and 4K batches whose input
     and output byte offsets pass 2^32
  D  the C ABI's refusals (status, message, output untouched), guard bytes around the output, input unmodified, a non-default
     stream, Engine.ingest_nv12's input handling
  E  the empty batch
  F  Nv12Uploader: upload() and prefetch() / convert() over batches that share neither content nor length

E found a defect: trl_ingest_* refused a NULL buffer before it looked at n_in, and a 0-frame tensor's pointer is NULL, so
Engine.ingest_nv12 of an empty batch raised TrlError("bad argument").  Fixed in the LIBRARY (csrc/trl_ingest.hip, ingest_420:
the empty batch returns before the buffers are looked at; NULL context / n_out and a NULL buffer of a non-empty batch are
refused as before), so C callers get the same answer as Engine's.

Run against deliberately wrong builds (a constant off by one, a rounding term dropped, the luma floor dropped, U and V swapped in
the planar branch, one pass instead of the grid-stride loop, a skipped store, the other slot's count in Nv12Uploader.convert),
every one turns tests here red.  Two of those builds were red for a reason of their own: with the loop or the store changed, the
compiler's v_ashr_pk_u8_i32 packing left stray bits in bytes 2 and 3 of every output dword.  sat8 in csrc/trl_ingest.hip now
keeps the compiler from forming that instruction; test_colour_cube and the shape tests are what would catch its return.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ingest_ref as R
import truely_amd
from truely_amd import _lib
from truely_amd._lib import TrlError
from truely_amd.ingest import Nv12Uploader, bgr_to_nv12

pytestmark = pytest.mark.gpu

# csrc/trl_ingest.hip, ingest_420: the launch is capped at 256 * 32 blocks of 256 threads, one thread per 4x2-pixel quad per pass
MAX_THREADS = 256 * 32 * 256
TRL_OK, TRL_ERR_INVALID = 0, -1
LAYOUTS = pytest.mark.parametrize("planar", [False, True], ids=["nv12", "i420"])
STEP_PAIRS = [(1, 1), (5, 1), (9, 4), (7, 3), (3, 5), (8, 8), (17, 16)]                # (n_in, step)


def _pattern(nbytes, dev):
    """a byte pattern with no period that divides a row, a pixel or a store"""
    base = (torch.arange(min(nbytes, 1 << 24), device=dev, dtype=torch.int32) % 251).to(torch.uint8)
    return base if nbytes <= base.numel() else base.repeat((nbytes + base.numel() - 1) // base.numel())[:nbytes]


def _layout(nv12, H, W, planar):
    return R.nv12_to_i420(nv12, H, W) if planar else nv12


def _raw(engine, in_ptr, n_in, H, W, step, planar, out_ptr, k=None, stream=0):
    """trl_ingest_nv12 / _i420 through the ctypes handle: (status, n_out) with n_out = -7 if the call did not write it"""
    lib = _lib.load()
    fn = lib.trl_ingest_i420 if planar else lib.trl_ingest_nv12
    k = C.c_int(-7) if k is None else k
    st = fn(engine._h, C.c_void_p(in_ptr), n_in, H, W, step, C.c_void_p(out_ptr), C.byref(k), C.c_void_p(stream))
    return st, k.value


def _convert(engine, d_in, H, W, step, planar):
    """the raw call into an output pre-filled with a pattern (so a byte the kernel skips cannot be right by accident)"""
    n_in = int(d_in.shape[0])
    n_out = (n_in + step - 1) // step
    out = _pattern(n_out * H * W * 3, d_in.device).view(n_out, H, W, 3)
    st, k = _raw(engine, d_in.data_ptr(), n_in, H, W, step, planar, out.data_ptr())
    assert (st, k) == (TRL_OK, n_out), (st, k, _lib.load().trl_last_error())
    return out


def _first_diff(got, ref):
    y, x, c = (int(v[0]) for v in np.nonzero(got != ref))
    return y, x, c


# ---- A: every (Y, U, V) ------------------------------------------------------------------------------------------------------
@LAYOUTS
def test_colour_cube(engine, planar):
    n = R.CUBE
    frame = R.colour_cube_nv12()[int(planar)]
    ref = R.yuv420_to_bgr(frame, n, n, planar)
    out = _convert(engine, torch.from_numpy(frame[None]).to(engine.device), n, n, 1, planar)
    got = out[0].cpu().numpy()
    if not np.array_equal(got, ref):
        y, x, c = _first_diff(got, ref)
        bad = int((got != ref).any(axis=2).sum())
        pytest.fail(f"(Y, U, V) = {tuple(int(t) for t in R.cube_triple(y, x))} channel {'BGR'[c]}: kernel {got[y, x, c]}, reference {ref[y, x, c]}"
                    f" (pixel {y}, {x}; {bad} of {n * n} triples differ)")


# ---- B: shapes x steps x content ---------------------------------------------------------------------------------------------
SMALL = [(2, 4), (2, 8), (4, 4), (38, 52), (48, 64), (6, 1284), (1080, 4)]       # every step pair x every kind
LARGE = {(360, 640): [("noise", (17, 16)), ("edges", (5, 1)), ("flat", (7, 3)), ("ramp", (8, 8))],
         (720, 1280): [("ramp", (9, 4)), ("noise", (3, 5)), ("edges", (1, 1))],
         (1080, 1920): [("edges", (8, 8)), ("noise", (7, 3)), ("flat", (1, 1))],
         (2160, 3840): [("noise", (3, 5)), ("ramp", (9, 4)), ("edges", (1, 1))]}


def _shape_cases(H, W):
    if (H, W) in LARGE:
        return LARGE[(H, W)]
    return [(kind, pair) for kind in R.KINDS for pair in STEP_PAIRS]


def test_shape_table_keeps_every_pair_and_kind():
    """the thinned table of the large shapes alone still has every (n_in, step) pair and every content kind"""
    assert {p for cs in LARGE.values() for _, p in cs} == set(STEP_PAIRS) and {k for cs in LARGE.values() for k, _ in cs} == set(R.KINDS)
    assert all(len(_shape_cases(*hw)) == len(R.KINDS) * len(STEP_PAIRS) for hw in SMALL)


@LAYOUTS
@pytest.mark.parametrize("H,W", SMALL + list(LARGE), ids=lambda v: str(v))
def test_shapes_and_steps(engine, H, W, planar):
    for kind, (n_in, step) in _shape_cases(H, W):
        tag = f"{H}x{W} {kind} n_in={n_in} step={step}"
        frames = _layout(R.content(kind, n_in, H, W, seed=n_in * 100 + step), H, W, planar)
        n_out = (n_in + step - 1) // step
        out = _convert(engine, torch.from_numpy(frames).to(engine.device), H, W, step, planar)
        api = engine.ingest_nv12(frames, H, W, step, planar=planar)                      # the Python entry point: shape, type, bytes
        assert tuple(api.shape) == (n_out, H, W, 3) and api.dtype == torch.uint8 and api.device == engine.device, tag
        got = out.cpu().numpy()
        for j in range(n_out):
            ref = R.yuv420_to_bgr(frames[j * step], H, W, planar)
            if not np.array_equal(got[j], ref):
                y, x, c = _first_diff(got[j], ref)
                pytest.fail(f"{tag}: output {j} (input {j * step}) differs first at pixel ({y}, {x}) channel {c}: {got[j, y, x, c]} != {ref[y, x, c]}")
        assert torch.equal(api, out), tag


# ---- C: production batches ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pool(H, W, K, planar):
    """K distinct source frames of mixed content in the given layout, and their references"""
    kinds = ("noise", "edges", "noise", "ramp")
    nv12 = np.stack([R.content(kinds[k % 4], 1, H, W, seed=1000 + k)[0] for k in range(K)])
    frames = _layout(nv12, H, W, planar)
    refs = np.stack([R.yuv420_to_bgr(f, H, W, planar) for f in frames])
    return frames, refs


def _src_of(i, K):
    """which pool frame input i is: neighbours differ, and so do inputs K apart (asserted for the step in use)"""
    return (3 * i + i // K) % K


def _batch_from_pool(engine, H, W, n_in, step, K, planar):
    """n_in frames built on the device from K host frames; every output compared on the device with the reference of the pool
    frame it must be.  Returns the indices of the outputs that differ."""
    dev = engine.device
    for i in range(n_in - 1):
        assert _src_of(i, K) != _src_of(i + 1, K) and _src_of(i, K) != _src_of(i + step, K), (i, step)
    frames, refs = _pool(H, W, K, planar)
    n_out = (n_in + step - 1) // step
    src = torch.from_numpy(frames).to(dev)
    idx = torch.tensor([_src_of(i, K) for i in range(n_in)], device=dev)
    d_in = src.index_select(0, idx)
    keep = d_in.clone() if d_in.numel() < (1 << 30) else None
    out = _convert(engine, d_in, H, W, step, planar)
    d_ref = torch.from_numpy(refs).to(dev)
    bad = [j for j in range(n_out) if not torch.equal(out[j], d_ref[_src_of(j * step, K)])]
    if keep is not None:
        assert torch.equal(keep, d_in), "the input was modified"
    return bad


def _release():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@LAYOUTS
@pytest.mark.parametrize("n", [20, 256])
def test_720p_batches_wrap_the_grid_stride_loop(engine, n, planar):
    """20 frames: the first wrap, ragged (2,304,000 quads on 2,097,152 threads); 256 frames: the benchmark's call (14 wraps)."""
    H, W = 720, 1280
    quads = n * (H // 2) * (W // 4)
    assert quads > MAX_THREADS and quads % MAX_THREADS != 0
    assert quads // MAX_THREADS == {20: 1, 256: 14}[n]
    try:
        bad = _batch_from_pool(engine, H, W, n, 1, 16, planar)
        assert not bad, f"{len(bad)} of {n} output frames differ, first {bad[:8]}"
    finally:
        _release()


@LAYOUTS
def test_4k_input_offsets_pass_4gib(engine, planar):
    """n_in = 360, step = 8: the last sampled frame starts 352 * 12,441,600 B = 4.38 GB into the input."""
    H, W, n_in, step = 2160, 3840, 360, 8
    assert (n_in - 1) // step * step * (H * W * 3 // 2) > 2 ** 32 and (n_in + step - 1) // step == 45
    try:
        bad = _batch_from_pool(engine, H, W, n_in, step, 8, planar)
        assert not bad, f"{len(bad)} of 45 output frames differ, first {bad[:8]} (inputs {[j * step for j in bad[:8]]})"
    finally:
        _release()


@LAYOUTS
def test_4k_output_offsets_pass_4gib(engine, planar):
    """n_in = 176, step = 1: the output is 4.38 GB; its last two frames start past 2^32."""
    H, W, n_in = 2160, 3840, 176
    assert (n_in - 1) * H * W * 3 > 2 ** 32 and (n_in - 1) * (H * W * 3 // 2) > 2 ** 31     # where the last frame starts: output, input
    try:
        bad = _batch_from_pool(engine, H, W, n_in, 1, 8, planar)
        assert not bad, f"{len(bad)} of {n_in} output frames differ, first {bad[:8]}"
    finally:
        _release()


# ---- D: the ABI contract -----------------------------------------------------------------------------------------------------
REFUSALS = [("W=6", dict(W=6), b"4:2:0 ingest needs"), ("W=2", dict(W=2), b"4:2:0 ingest needs"), ("H=3", dict(H=3), b"4:2:0 ingest needs"),
            ("H=0", dict(H=0), b"4:2:0 ingest needs"), ("step=0", dict(step=0), b"bad argument"), ("n_in=-1", dict(n_in=-1), b"bad argument"),
            ("in+1", dict(in_off=1), b"4-byte aligned"), ("in+2", dict(in_off=2), b"4-byte aligned"), ("out+2", dict(out_off=2), b"4-byte aligned"),
            ("in=NULL", dict(null_in=True), b"bad argument"), ("out=NULL", dict(null_out=True), b"bad argument"),
            ("n_out=NULL", dict(null_k=True), b"bad argument")]


@LAYOUTS
@pytest.mark.parametrize("name,change,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_leave_the_output_untouched(engine, name, change, msg, planar):
    """Each of these is refused by the host code before any launch (ingest_420's three checks): TRL_ERR_INVALID, its message,
    neither the output nor *n_out written."""
    lib = _lib.load()
    dev = engine.device
    a = dict(H=4, W=8, n_in=2, step=1, in_off=0, out_off=0, null_in=False, null_out=False, null_k=False)
    a.update(change)
    d_in = torch.full((4096,), 7, dtype=torch.uint8, device=dev)
    out = _pattern(4096, dev)
    fn = lib.trl_ingest_i420 if planar else lib.trl_ingest_nv12
    k = C.c_int(-7)
    torch.cuda.synchronize()
    st = fn(engine._h, C.c_void_p(0 if a["null_in"] else d_in.data_ptr() + a["in_off"]), a["n_in"], a["H"], a["W"], a["step"],
            C.c_void_p(0 if a["null_out"] else out.data_ptr() + a["out_off"]), None if a["null_k"] else C.byref(k), None)
    err = lib.trl_last_error()
    torch.cuda.synchronize()
    assert st == TRL_ERR_INVALID and msg in err, (name, st, err)
    assert k.value == -7
    assert torch.equal(out, _pattern(4096, dev)) and bool((d_in == 7).all())
    # the context works afterwards
    ok = _convert(engine, torch.from_numpy(R.content("noise", 1, 2, 4, seed=9)).to(dev), 2, 4, 1, False)
    assert np.array_equal(ok[0].cpu().numpy(), R.yuv420_to_bgr(R.content("noise", 1, 2, 4, seed=9)[0], 2, 4))


def test_null_context_is_refused(engine):
    d = torch.zeros(4096, dtype=torch.uint8, device=engine.device)
    k = C.c_int(-7)
    for fn in (_lib.load().trl_ingest_nv12, _lib.load().trl_ingest_i420):
        assert fn(None, C.c_void_p(d.data_ptr()), 0, 4, 8, 1, C.c_void_p(d.data_ptr()), C.byref(k), None) == TRL_ERR_INVALID
        assert fn(None, C.c_void_p(d.data_ptr()), 1, 4, 8, 1, C.c_void_p(d.data_ptr()), C.byref(k), None) == TRL_ERR_INVALID
    assert k.value == -7 and not d.any()


GUARD = 4096


@LAYOUTS
@pytest.mark.parametrize("step", [1, 3])
@pytest.mark.parametrize("H,W", [(38, 52), (2, 4), (720, 1280)], ids=lambda v: str(v))
def test_guard_bytes_and_input_intact(engine, H, W, step, planar):
    dev = engine.device
    n_in = 7
    n_out = (n_in + step - 1) // step
    frames = _layout(R.content("noise", n_in, H, W, seed=77), H, W, planar)
    d_in = torch.from_numpy(frames).to(dev)
    payload = n_out * H * W * 3
    buf = _pattern(GUARD + payload + GUARD, dev)
    st, k = _raw(engine, d_in.data_ptr(), n_in, H, W, step, planar, buf.data_ptr() + GUARD)
    torch.cuda.synchronize()
    assert (st, k) == (TRL_OK, n_out)
    pat = _pattern(GUARD + payload + GUARD, dev)
    assert torch.equal(buf[:GUARD], pat[:GUARD]), "bytes before the output were written"
    assert torch.equal(buf[GUARD + payload:], pat[GUARD + payload:]), "bytes after the output were written"
    got = buf[GUARD:GUARD + payload].view(n_out, H, W, 3).cpu().numpy()
    for j in range(n_out):
        assert np.array_equal(got[j], R.yuv420_to_bgr(frames[j * step], H, W, planar)), j
    assert np.array_equal(d_in.cpu().numpy(), frames), "the input was modified"


@LAYOUTS
def test_non_default_stream_and_back_to_back_calls(engine, planar):
    dev = engine.device
    H, W, n_in, step = 360, 640, 12, 2
    frames = _layout(R.content("noise", n_in, H, W, seed=31), H, W, planar)
    ref = np.stack([R.yuv420_to_bgr(f, H, W, planar) for f in frames[::step]])
    d_in = torch.from_numpy(frames).to(dev)
    outs = [_pattern(ref.size, dev).view(ref.shape) for _ in range(3)]
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    ra = _raw(engine, d_in.data_ptr(), n_in, H, W, step, planar, outs[0].data_ptr(), stream=side.cuda_stream)
    rb = _raw(engine, d_in.data_ptr(), n_in, H, W, step, planar, outs[1].data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    with torch.cuda.stream(side):                                       # Engine takes torch's current stream
        outs[2] = engine.ingest_nv12(d_in, H, W, step, planar=planar)
    side.synchronize()
    assert ra == rb == (TRL_OK, n_in // step)
    for o in outs:
        assert np.array_equal(o.cpu().numpy(), ref)
    assert np.array_equal(d_in.cpu().numpy(), frames)


@LAYOUTS
def test_engine_ingest_input_handling(engine, planar):
    dev = engine.device
    H, W, n = 38, 52, 10
    frames = _layout(R.content("noise", n, H, W, seed=8), H, W, planar)
    ref = np.stack([R.yuv420_to_bgr(f, H, W, planar) for f in frames])
    d = torch.from_numpy(frames).to(dev)
    call = lambda x, step=1: engine.ingest_nv12(x, H, W, step, planar=planar).cpu().numpy()
    assert np.array_equal(call(frames), ref)                                                  # numpy
    assert np.array_equal(call(torch.from_numpy(frames)), ref)                                # CPU tensor
    assert np.array_equal(call(d, 3), ref[::3])                                               # device tensor
    assert not d[::2].is_contiguous() and np.array_equal(call(d[::2]), ref[::2])              # row-strided: every second frame
    assert np.array_equal(call(d[::2], 2), ref[::4])
    assert np.array_equal(call(frames[::-1]), ref[::-1])                                      # negative numpy stride
    wide = torch.zeros((n, H * W * 3 // 2 + 4), dtype=torch.uint8, device=dev)
    wide[:, :-4] = d
    assert np.array_equal(call(wide[:, :-4]), ref)                                            # padded rows
    with pytest.raises(ValueError, match="uint8"):
        engine.ingest_nv12(d.to(torch.int8), H, W, 1, planar=planar)                          # wrong dtype
    with pytest.raises(ValueError, match="uint8"):
        engine.ingest_nv12(frames.astype(np.float32), H, W, 1, planar=planar)
    with pytest.raises(ValueError, match=r"H\*W\*3/2"):
        engine.ingest_nv12(d[:, :-3], H, W, 1, planar=planar)                                 # wrong row length
    with pytest.raises(ValueError):
        engine.ingest_nv12(d.view(n, H * 3 // 2, W), H, W, 1, planar=planar)                  # not (n, bytes)
    with pytest.raises(TrlError, match="4:2:0 ingest needs") as e:                            # a shape only the library refuses
        engine.ingest_nv12(torch.zeros((2, 6 * 6 * 3 // 2), dtype=torch.uint8), 6, 6, 1, planar=planar)
    assert e.value.status == TRL_ERR_INVALID


# ---- E: the empty batch ------------------------------------------------------------------------------------------------------
@LAYOUTS
def test_empty_batch(engine, planar):
    dev = engine.device
    H, W = 38, 52
    for empty in (np.zeros((0, H * W * 3 // 2), np.uint8), torch.zeros((0, H * W * 3 // 2), dtype=torch.uint8),
                  torch.zeros((0, H * W * 3 // 2), dtype=torch.uint8, device=dev)):
        for step in (1, 4):
            out = engine.ingest_nv12(empty, H, W, step, planar=planar)
            assert tuple(out.shape) == (0, H, W, 3) and out.dtype == torch.uint8 and out.device == dev
    d_in = torch.full((4096,), 7, dtype=torch.uint8, device=dev)
    out = _pattern(4096, dev)
    assert _raw(engine, d_in.data_ptr(), 0, H, W, 1, planar, out.data_ptr()) == (TRL_OK, 0)
    assert _raw(engine, 0, 0, H, W, 5, planar, 0) == (TRL_OK, 0)                          # what Engine passes: no buffers at all
    torch.cuda.synchronize()
    assert torch.equal(out, _pattern(4096, dev))
    # the shape is still checked, and a null n_out still refused
    assert _raw(engine, d_in.data_ptr(), 0, H, W + 2, 1, planar, out.data_ptr()) == (TRL_ERR_INVALID, -7)
    fn = _lib.load().trl_ingest_i420 if planar else _lib.load().trl_ingest_nv12
    assert fn(engine._h, C.c_void_p(d_in.data_ptr()), 0, H, W, 1, C.c_void_p(out.data_ptr()), None, None) == TRL_ERR_INVALID


# ---- F: Nv12Uploader ---------------------------------------------------------------------------------------------------------
BATCH_SIZES = [24, 1, 23, 24, 2, 24, 24, 5, 24]
POOL = 32


@functools.lru_cache(maxsize=None)
def _clip_pool(H, W):
    """POOL distinct decoder-like frames with a face each (so the cascade has work), as NV12, and their references"""
    seed = {360: 41, 720: 0}[H]          # clips in which the synthetic-weight cascade finds the face (720p: the benchmark's clip)
    nv12 = bgr_to_nv12(truely_amd.synthetic.synthetic_frames(POOL, H, W, seed=seed))
    assert len({f.tobytes() for f in nv12}) == POOL
    return nv12, np.stack([R.yuv420_to_bgr(f, H, W) for f in nv12])


def _batches(H, W):
    """Nine batches; frame f of batch b is pool frame (f + 3 b) % POOL, so at no position do two batches hold the same frame,
    and no two neighbouring batches have the same length.  Sources: pageable numpy, pageable tensor, pinned tensor in turn."""
    nv12, _ = _clip_pool(H, W)
    idx = [[(f + 3 * b) % POOL for f in range(n)] for b, n in enumerate(BATCH_SIZES)]
    for b in range(len(idx)):
        for c in range(b):
            assert all(x != y for x, y in zip(idx[b], idx[c]))
    srcs = []
    for b, ix in enumerate(idx):
        a = np.ascontiguousarray(nv12[ix])
        srcs.append(a if b % 3 == 0 else torch.from_numpy(a.copy()) if b % 3 == 1 else torch.from_numpy(a).pin_memory())
    assert not srcs[1].is_pinned() and srcs[2].is_pinned()
    return idx, srcs


def _check_batches(engine, H, W, idx, outs, step):
    _, refs = _clip_pool(H, W)
    d_ref = torch.from_numpy(refs).to(engine.device)
    torch.cuda.synchronize()
    for b, (ix, out) in enumerate(zip(idx, outs)):
        want = ix[::step]
        assert tuple(out.shape) == (len(want), H, W, 3), f"batch {b}: {tuple(out.shape)} for {len(ix)} frames at step {step}"
        bad = [j for j, p in enumerate(want) if not torch.equal(out[j], d_ref[p])]
        assert not bad, f"batch {b} (n = {len(ix)}): outputs {bad[:8]} are not the conversion of this batch's own frames"
    assert len({o.data_ptr() for o in outs}) == len(outs)               # fresh tensors: none of them aliases another


SIZES = pytest.mark.parametrize("H,W", [(360, 640), (720, 1280)], ids=lambda v: str(v))


@SIZES
@pytest.mark.parametrize("step", [1, 4])
def test_uploader_upload(engine, H, W, step):
    """Every returned batch is the conversion of its own input, checked after all nine calls were issued with no
    synchronisation in between; the returned tensors stay valid (they are fresh, not slots)."""
    idx, srcs = _batches(H, W)
    up = Nv12Uploader(engine, H, W, max_frames=24)
    outs = [up.upload(s, step) for s in srcs]
    _check_batches(engine, H, W, idx, outs, step)


def _same_result(a, b):
    assert a.keys() == b.keys()
    for key in a:
        assert torch.equal(a[key], b[key]), key


@SIZES
@pytest.mark.parametrize("slots,step", [(2, 1), (3, 1), (2, 4), (3, 4)])
def test_uploader_prefetch_convert_in_bench_order(engine, H, W, slots, step):
    """bench.py's --ingest nv12 order: convert batch k, start the copy of batch k + 1 on the copy stream, then run the cascade on
    batch k (the engine's stream is busy while the copy runs)."""
    idx, srcs = _batches(H, W)
    _, refs = _clip_pool(H, W)
    up = Nv12Uploader(engine, H, W, max_frames=24, slots=slots)
    outs, results = [], []
    pending = up.prefetch(srcs[0])
    for k in range(len(srcs)):
        out = up.convert(pending, step)
        pending = up.prefetch(srcs[k + 1]) if k + 1 < len(srcs) else None
        results.append(engine.detect_embed(out))
        outs.append(out)
    _check_batches(engine, H, W, idx, outs, step)
    faces = 0
    for k, ix in enumerate(idx):
        direct = engine.detect_embed(torch.from_numpy(refs[ix[::step]]).to(engine.device))
        _same_result(results[k], direct)
        faces += int(direct["valid"].sum())
    assert faces > 0                                                    # the cascade had something to find


@SIZES
def test_uploader_refuses_oversized_batches(engine, H, W):
    up = Nv12Uploader(engine, H, W, max_frames=4, slots=3)
    nv12, refs = _clip_pool(H, W)
    up.upload(nv12[:2])
    assert up.i == 1
    for big in (nv12[:5], torch.from_numpy(nv12[:5])):
        with pytest.raises(ValueError, match="exceeds"):
            up.upload(big)
        with pytest.raises(ValueError, match="exceeds"):
            up.prefetch(big)
        assert up.i == 1
    out = up.convert(up.prefetch(nv12[1:5]), 3)                         # still usable, and on the next slot
    assert up.i == 2 and np.array_equal(out.cpu().numpy(), refs[[1, 4]])
