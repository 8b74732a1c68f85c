"""The table behind tests/test_api_refusals_cpu.py and tests/test_gpu_api_refusals.py: what every context-bound entry point of
libtruely_hip.so -- the product calls of csrc/trl_api.hip, trl_extract.hip, trl_ingest.hip and trl_weights.hip, the hooks of
csrc/trl_hooks.hip and trl_redzone.hip -- answers where it refuses a call or has nothing to run, as [case, status, message] rows
against tests/golden/api_refusals.json.

The golden file was recorded from the library of the commit BEFORE the hooks and the red zones left trl_api.hip; a status or a
message that differs is a change of behaviour.  `python tests/api_refusal_cases.py --record [FILE]` (on a machine with a GPU)
writes it from whatever library TRUELY_HIP_LIB selects: record it from the library the change is held against, never from the
tree under test.

Four sections, one context state each:
  null        every entry with a null context, trl_create with each bad trl_config field and with null arguments,
              trl_default_config(NULL), trl_debug_option with a null key and with the two process-wide keys.  All of it is
              answered before the library's first HIP call.  No entry dereferences a null context (read off the code: each one
              starts with trl_check_idle, or a null check of its own, or -- trl_debug_option -- reaches the context only behind
              one), so none is left out.
  no_weights  a context without weights: every entry that requires them.
  idle        weights loaded, nothing queued, no call made yet: null outputs, counts at 0, -1 and one past their limit, bad
              enumerators, a frame pointer off by 2 bytes, tier / option / red-zone values just outside their ranges, the hooks
              that need cascade state, trl_detect_embed_end with nothing queued.  A count at 0 is left out where the entry
              accepts it and would launch (trl_drift_score, trl_debug_stage_net, trl_debug_front).
  in_flight   between trl_detect_embed_begin on one 32 x 32 frame and trl_detect_embed_end: every entry that takes a context but
              trl_destroy.  Those that refuse answer TRL_ERR_STATE; the host-only hooks answer as ever.  Seven entries neither
              check for a queued call nor stay on the host (trl_drift_score, trl_drift_update, trl_ingest_nv12, trl_ingest_i420
              and the three crop hooks): they are called with an argument they refuse, or with the empty batch, so that the
              queued call stays the only kernel work of the test.  trl_load_weights would reload: called with a null blob.

A refusal that sets no message (trl_default_config(NULL), trl_debug_timings) leaves the last error as it was, so every case
starts from the same one: trl_debug_option(NULL key) -> "null key"."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "api_refusals.json")
SECTIONS = ("null", "no_weights", "idle", "in_flight")
# the families of include/truely_hip.h that take no context (tests/test_host_layer_cpu.py and their own tests hold those)
CONTEXT_FREE = ("trl_abi_version", "trl_last_error", "trl_jpeg", "trl_jpegd_", "trl_draw", "trl_gallery_", "trl_cluster_", "trl_track_", "trl_pool_",
                "trl_quality_", "trl_face_quality", "trl_best_", "trl_shots_", "trl_frame_signatures", "trl_signature_distance")
NOT_IN_FLIGHT = {"trl_default_config", "trl_create", "trl_destroy"}

_HOST = (C.c_longlong * 1024)()         # what a hook that answers writes into
_ZERO = (C.c_longlong * 64)()           # the host rows a hook reads: never written, so frame 0 and an empty box / window / list
HP, HZ = C.addressof(_HOST), C.addressof(_ZERO)
NAN = float("nan")


def context_bound():
    """Every name of _lib._SIGNATURES that takes a context, trl_default_config and trl_create"""
    from truely_amd._lib import _SIGNATURES
    return [n for n in _SIGNATURES if not n.startswith(CONTEXT_FREE)]


class _Entry:
    """One exported function with an argument list that it accepts; __call__ gives the case that changes some of them."""

    def __init__(self, lib, name, show, ctx, **base):
        self.fn, self.name, self.show, self.ctx, self.base = getattr(lib, name), name, show, ctx, base

    def __call__(self, note="", **changed):
        """note: told apart from the same call in another state of the context"""
        assert set(changed) <= set(self.base), (self.name, changed)
        args = [self.ctx] + list(dict(self.base, **changed).values())
        args = [C.cast(v, t) if isinstance(v, int) and isinstance(t, type) and issubclass(t, C._Pointer) else v for v, t in zip(args, self.fn.argtypes)]
        label = f"{self.name}({', '.join(f'{k}={self.show(v)}' for k, v in changed.items())}){note}"
        return label, lambda: self.fn(*args)

    def each(self, **values):
        """One case per value: each(m=(-1, 5), k=(0,)) -> m=-1, m=5, k=0"""
        return [self(**{k: v}) for k, vs in values.items() for v in vs]


def entries(lib, ctx, D):
    """name -> _Entry of every entry that takes a context, on `ctx`.  D: a 64 KB device buffer, zero, 256-byte aligned (the null
    section, where nothing is read: any address).  Frames are 32 x 32, batches 1."""
    def show(v):
        if v is None:
            return "null"
        if isinstance(v, int) and D <= v < D + 65536:
            return "d" if v == D else f"d+{v - D}"
        if isinstance(v, int) and HP <= v < HP + C.sizeof(_HOST):
            return "h" if v == HP else f"h+{v - HP}"
        if v == HZ:
            return "z"
        return repr(v)

    E = lambda name, **base: (name, _Entry(lib, name, show, ctx, **base))
    frames = dict(frames=D, n=1, H=32, W=32)
    embed = dict(frames, box=D + 4096, prob=D + 4160, rect=D + 4224, valid=D + 4288)
    crop_hook = dict(frames, rows=D + 4224, valid=D + 4288)
    return dict([
        E("trl_destroy"),
        E("trl_load_weights", blob=b"TRLW", nbytes=4),
        E("trl_mtcnn_detect", **frames, boxes=D + 8192, probs=D + 12288, counts=D + 4352, stream=None),
        E("trl_mtcnn_detect_landmarks", **frames, boxes=D + 8192, probs=D + 12288, points=D + 16384, counts=D + 4352, stream=None),
        E("trl_mtcnn_detect_ordered", **frames, order=0, boxes=D + 8192, probs=D + 12288, points=None, counts=D + 4352, stream=None),
        E("trl_select_faces", n=1, boxes=D + 8192, probs=D + 12288, counts=D + 4352, H=32, W=32, method=0, threshold=0.9, center_weight=2.0,
          pick=D + 4416, stream=None),
        E("trl_extract_faces", **frames, frame_of=D + 4352, boxes=D + 4096, m=1, S=160, margin=0, resample=0, post_process=1, out=D + 8192,
          status=D + 4416, stream=None),
        E("trl_facenet_embed", faces=D, n=1, h=80, w=80, emb=D + 8192, stream=None),
        E("trl_facenet_num_classes", C=HP),
        E("trl_facenet_features", faces=D, valid=None, n=1, h=80, w=80, feat=D + 8192, stream=None),
        E("trl_facenet_logits", feat=D, n=1, logits=D + 8192, ld=1 << 20, stream=None),
        E("trl_detect_embed", **embed, emb=D + 8192, stream=None),
        E("trl_detect_crop", **embed, faces=D + 8192, stream=None),
        E("trl_detect_embed_begin", **embed, emb=D + 8192, stream=None),
        E("trl_detect_crop_begin", **embed, faces=D + 8192, stream=None),
        E("trl_detect_embed_end"),
        E("trl_facenet_embed_masked", faces=D, valid=D + 4288, n=1, h=80, w=80, emb=D + 8192, stream=None),
        E("trl_drift_score", emb=D + 8192, valid=D + 4288, n=1, frame_count=16, fps=30, sims=D + 4160, flags=D + 4480, result=D + 4544, stream=None),
        E("trl_ingest_nv12", nv12=D, n_in=1, H=32, W=32, step=1, bgr=D + 8192, n_out=HP, stream=None),
        E("trl_ingest_i420", i420=D, n_in=1, H=32, W=32, step=1, bgr=D + 8192, n_out=HP, stream=None),
        E("trl_drift_update", state=D + 16384, emb=D + 8192, valid=D + 4288, n=1, frame_count=16, fps=30, sims=D + 4160, flags=D + 4480,
          result=D + 4544, stream=None),
        E("trl_debug_stage_boxes", stage=1, frame=0, boxes=HP, max_rows=1, n_out=HP + 4096),
        E("trl_debug_level_counts", frame=0, cand=HP, keep=HP + 1024, n_levels=HP + 4096),
        E("trl_debug_level_cands", frame=0, level=0, rows=HP, max_rows=1, n_out=HP + 4096),
        E("trl_debug_level_keep", frame=0, level=0, idx=HP, max_rows=1, n_out=HP + 4096),
        E("trl_debug_batch_capacity", t2=0.0, t3=0.0, last_attempts=HP),
        E("trl_debug_nms_tiers", small=0, full=0),
        E("trl_debug_option", key=b"rnet_chunk", value=49152),
        E("trl_debug_list_stats", out8=HP),
        E("trl_debug_poison", byte=0xFF),
        E("trl_debug_pyramid_level", frame=D, H=32, W=32, level=0, out=D + 16384, h=HP, w=HP + 8, stream=None),
        E("trl_debug_pyramid_batch", **frames, out=None, pyr_stride=HP, levels=HP + 64, max_levels=16, n_levels=HP + 4096, stream=None),
        E("trl_debug_pyramid_plan", rows=HP, max_levels=16, n_levels=HP + 4096),
        E("trl_debug_facenet_plan", rows=HP, max_rows=1, n_rows=HP + 4096),
        E("trl_debug_facenet_capture", conv_index=-1),
        E("trl_debug_facenet_capture_read", view=0, dst=None, max_bytes=0, dims5=HP),
        E("trl_debug_pnet_level", frame=D, H=32, W=32, level=0, prob=D + 16384, reg=D + 32768, oh=HP, ow=HP + 8, stream=None),
        E("trl_debug_rnet", crops=D, n=1, out=D + 8192, stream=None),
        E("trl_debug_onet", crops=D, n=1, out=D + 8192, stream=None),
        E("trl_debug_front_net", frame=D, H=32, W=32, boxes=HZ, nb=1, net=24, out=D + 8192, stream=None),
        E("trl_debug_stage_net", **frames, recs=HZ, nb=1, net=24, capacity=1, out=D + 8192, stream=None),
        E("trl_debug_front", **frames, win=HZ, nb=1, net=24, capacity=1, pool=D + 16384, stream=None),
        E("trl_debug_mtcnn_plan", rows=HP, max_rows=1, n_rows=HP + 4096),
        E("trl_debug_lists", kind=1, n=1, H=32, W=32, caps=HZ, n_levels=1, counts=HZ, rows=HZ, logits=None, pts=None, boxes=None,
          probs=None, points=None, dcounts=None, box0=None, prob0=None, rect=None, valid=None, stream=None),
        E("trl_debug_crop_resize", **crop_hook, faces=D + 8192, stream=None),
        E("trl_debug_crop_aligned", **crop_hook, S=160, rgb=1, faces=D + 8192, stream=None),
        E("trl_debug_crop_area", **crop_hook, S=160, rgb=0, faces=D + 8192, stream=None),
        E("trl_debug_timings", out4=HP),
        E("trl_debug_workspace", what=0, n=0, h=0, w=0, out6=HP),
        E("trl_debug_redzone", guard=0, byte=0xA5),
        E("trl_debug_redzone_report", flags=0, out4=HP, hits=HP + 64, max_hits=1),
        E("trl_debug_redzone_poke", arena=0, block=-1, offset=0, value=0x3C),
        E("trl_debug_stage_totals", out2=HP),
        E("trl_debug_pnet_run", run=0),
        E("trl_debug_pnet_kernel_ms", ms=HP),
        E("trl_debug_pnet_span", reset=0, ms_sum=HP, launches=HP + 8),
        E("trl_debug_pnet_screen_bound", A=HP, B=HP + 8, on=HP + 16),
        E("trl_debug_pnet_screen_weights", g16=HP),
        E("trl_debug_pnet_defer", out4=HP),
    ])


def null_cases(lib):
    from truely_amd._lib import TrlConfig
    out = [e() for e in entries(lib, None, 1 << 20).values()]

    def create(label, cfg, h):
        return f"trl_create({label})", lambda: lib.trl_create(cfg, h)

    def config(**kw):
        cfg = TrlConfig()
        assert lib.trl_default_config(C.byref(cfg)) == 0
        for k, v in kw.items():
            setattr(cfg, k, v)
        return C.byref(cfg)
    h = C.c_void_p()
    out += [create("cfg=null", None, C.byref(h)), create("out=null", config(), None)]
    bad = dict(cap_level=(63, (1 << 24) + 4, 66), cap_frame=(63, (1 << 24) + 4, 66), min_face_size=(11,), max_faces=(0,), factor=(0.1, 0.99, NAN),
               embed_mode=(-1, 4), embed_precision=(-1, 3))
    out += [create(f"{k}={v!r}", config(**{k: v}), C.byref(h)) for k, vs in bad.items() for v in vs]
    out.append(("trl_default_config(null)", lambda: lib.trl_default_config(None)))
    out += [(f"trl_debug_option(null context, key={k!r})", (lambda k=k: lib.trl_debug_option(None, k, 0))) for k in (None, b"no_fnconv", b"pnet_gate", b"tail_pool")]
    return out


def no_weights_cases(lib, ctx, D):
    e = entries(lib, ctx, D)
    names = ("trl_mtcnn_detect", "trl_mtcnn_detect_landmarks", "trl_mtcnn_detect_ordered", "trl_detect_embed", "trl_detect_crop",
             "trl_detect_embed_begin", "trl_detect_crop_begin", "trl_facenet_embed", "trl_facenet_embed_masked", "trl_facenet_features",
             "trl_facenet_num_classes", "trl_facenet_logits", "trl_debug_pyramid_level", "trl_debug_pyramid_batch", "trl_debug_pnet_level",
             "trl_debug_rnet", "trl_debug_onet", "trl_debug_front_net", "trl_debug_stage_net", "trl_debug_front")
    return [e[n]() for n in names] + [e["trl_debug_workspace"](what=w, n=1, h=80, w=80) for w in (1, 24, 48)]


def idle_cases(lib, ctx, D):
    e = entries(lib, ctx, D)
    out = []
    batch = dict(frames=(None, D + 2), n=(0, -1, 65536), H=(11, 16384), W=(11, 16384))
    one = dict(frame=(None, D + 2), H=(11, 16384), W=(11, 16384))
    nulls = lambda *names: {k: (None,) for k in names}
    out += e["trl_mtcnn_detect"].each(**batch, **nulls("boxes", "probs", "counts"))
    out += e["trl_mtcnn_detect_landmarks"].each(**batch, **nulls("boxes", "probs", "points", "counts"))
    out += e["trl_mtcnn_detect_ordered"].each(**batch, order=(-1, 2), **nulls("boxes", "probs", "counts"))
    for n in ("trl_detect_embed", "trl_detect_embed_begin"):
        out += e[n].each(**batch, **nulls("box", "prob", "rect", "valid", "emb"))
    for n in ("trl_detect_crop", "trl_detect_crop_begin"):
        out += e[n].each(**batch, **nulls("box", "prob", "rect", "valid", "faces"))
    out.append(e["trl_detect_embed_end"]())
    out += e["trl_select_faces"].each(n=(0, -1, 65536), H=(0,), W=(0,), method=(-1, 4), **nulls("boxes", "probs", "counts", "pick"))
    x = e["trl_extract_faces"]
    out += x.each(n=(0, -1, 65536), H=(0, 16384), W=(0, 16384), m=(-1, 65536), S=(0, 1025), margin=(-1, 160), resample=(-1, 3), post_process=(2,),
                  **nulls("frames", "frame_of", "boxes", "out")) + [x(m=0), x(m=0, frame_of=None, boxes=None, out=None)]
    out += e["trl_facenet_embed"].each(n=(0, -1), h=(74,), w=(74,), **nulls("faces", "emb"))
    out += e["trl_facenet_embed_masked"].each(n=(0, -1), h=(74,), w=(74,), **nulls("faces", "valid", "emb"))
    out += e["trl_facenet_features"].each(n=(0, -1), h=(74,), w=(74,), **nulls("faces", "feat"))
    out += e["trl_facenet_num_classes"].each(C=(None,)) + [e["trl_facenet_num_classes"]()]
    out += e["trl_facenet_logits"].each(n=(0, -1), ld=(0,), **nulls("feat", "logits"))
    out += e["trl_drift_score"].each(n=(-1,), **nulls("emb", "valid", "result"))
    out += e["trl_drift_update"].each(n=(-1,), state=(None, D + 16386), **nulls("emb", "valid", "result"))
    for n, src in (("trl_ingest_nv12", "nv12"), ("trl_ingest_i420", "i420")):
        x = e[n]
        out += x.each(n_in=(-1,), step=(0,), W=(0, 30), H=(0, 31), n_out=(None,), bgr=(None, D + 8194), **{src: (None, D + 2)})
        out += [x(n_in=0), x(n_in=0, bgr=None, **{src: None})]
    # the hooks that read the state a call left: none yet
    for n in ("trl_debug_stage_boxes", "trl_debug_level_counts", "trl_debug_level_cands", "trl_debug_level_keep"):
        out.append(e[n]())
    out += e["trl_debug_stage_boxes"].each(stage=(0, 4), frame=(-1,), n_out=(None,))
    out += e["trl_debug_batch_capacity"].each(last_attempts=(None,)) + [e["trl_debug_batch_capacity"]()]
    out += e["trl_debug_nms_tiers"].each(small=(15, 3076, 18, -4), full=(15, 3076, 18, -4)) + [e["trl_debug_nms_tiers"]()]
    x = e["trl_debug_option"]
    out += [x(key=b"no_such_option"), x(key=None), x(key=b"rnet_chunk", value=15), x(key=b"onet_chunk", value=15), x(key=b"pnet_screen", value=2),
            x(key=b"pnet_screen", value=-1), x(key=b"pnet_defer", value=2), x(key=b"pnet_defer", value=-1), x(key=b"pnet_defer_cap", value=-1),
            x(key=b"pyr_row_bands", value=-1), x(key=b"tail_pool", value=2), x(key=b"tail_pool", value=-1), x()]
    out += e["trl_debug_list_stats"].each(out8=(None,)) + [e["trl_debug_list_stats"]()]
    out += e["trl_debug_pyramid_level"].each(**one)
    out += e["trl_debug_pyramid_batch"].each(**batch, **nulls("pyr_stride", "levels", "n_levels"))
    for n, rows, mx, cnt in (("trl_debug_pyramid_plan", "rows", "max_levels", "n_levels"), ("trl_debug_facenet_plan", "rows", "max_rows", "n_rows"),
                             ("trl_debug_mtcnn_plan", "rows", "max_rows", "n_rows")):
        out += e[n].each(**nulls(rows, cnt)) + [e[n](), e[n](**{rows: None, mx: 0})]
    out.append(e["trl_debug_facenet_capture"]())
    out += e["trl_debug_facenet_capture_read"].each(view=(-1, 3), dims5=(None,)) + [e["trl_debug_facenet_capture_read"]()]
    out += e["trl_debug_pnet_level"].each(**one, level=(-1, 99))
    for n in ("trl_debug_rnet", "trl_debug_onet"):
        out += e[n].each(n=(0, -1), **nulls("crops", "out"))
    out += e["trl_debug_front_net"].each(**one, nb=(0, -1, (1 << 20) + 1), net=(12, 0), **nulls("boxes", "out"))
    out += e["trl_debug_stage_net"].each(**batch, nb=(-1, (1 << 24) + 1), capacity=(-1, (1 << 24) + 1), net=(12, 25), **nulls("recs", "out"))
    out += e["trl_debug_front"].each(**batch, nb=(-1, (1 << 20) + 1), capacity=(-1, (1 << 20) + 1), net=(12, 25), **nulls("win", "pool"))
    # rows the two stage hooks refuse one by one (the host rows are zero: frame 0, an empty box / window)
    out += [e["trl_debug_stage_net"](), e["trl_debug_front"](), e["trl_debug_front_net"]()]
    x = e["trl_debug_lists"]
    out += x.each(kind=(0, 4), n=(0, -1, 65536), H=(11, 16384), W=(11, 16384), n_levels=(0, 33, -1), **nulls("caps", "counts"))
    out += [x(kind=3, n_levels=0), x()]                                   # kind 3 without outputs; caps[0] = 0: "capacity 0"
    for n, nmax in (("trl_debug_crop_resize", None), ("trl_debug_crop_aligned", 65536), ("trl_debug_crop_area", 65536)):
        vals = dict(n=(0, -1) + ((nmax,) if nmax else ()), H=(0,), W=(0,), **nulls("frames", "rows", "valid", "faces"))
        if nmax:
            vals["S"] = (0, 4097)
        out += e[n].each(**vals)
    out += e["trl_debug_timings"].each(out4=(None,)) + [e["trl_debug_timings"]()]
    x = e["trl_debug_workspace"]
    out += x.each(what=(2, -1), out6=(None,)) + [x(what=1, n=0, h=80, w=80), x(what=1, n=1, h=74, w=80), x(what=1, n=1, h=80, w=74), x(what=24), x()]
    out += e["trl_debug_redzone"].each(guard=(-256, 255, (1 << 20) + 256), byte=(-1, 256)) + [e["trl_debug_redzone"]()]
    out += e["trl_debug_redzone_report"].each(**nulls("out4", "hits")) + [e["trl_debug_redzone_report"](), e["trl_debug_redzone_report"](hits=None, max_hits=0)]
    out.append(e["trl_debug_redzone_poke"]())                                  # red zones are off
    out.append(e["trl_debug_redzone"](guard=256))                              # ... on: both workspaces start over, nothing is launched
    out.append(e["trl_debug_poison"]())
    out += e["trl_debug_redzone_poke"].each(arena=(-1, 2), value=(-1, 256, 0xA5)) + [e["trl_debug_redzone_poke"](" with red zones on")]   # no workspace yet
    out.append(e["trl_debug_redzone"](" with red zones on"))                   # off again
    out += e["trl_debug_stage_totals"].each(out2=(None,)) + [e["trl_debug_stage_totals"]()]
    out += e["trl_debug_pnet_run"].each(run=(-1, 65)) + [e["trl_debug_pnet_run"]()]
    out += e["trl_debug_pnet_kernel_ms"].each(ms=(None,)) + [e["trl_debug_pnet_kernel_ms"]()]
    out += e["trl_debug_pnet_span"].each(**nulls("ms_sum", "launches")) + [e["trl_debug_pnet_span"]()]
    out += e["trl_debug_pnet_screen_bound"].each(**nulls("A", "B", "on")) + [e["trl_debug_pnet_screen_bound"]()]
    out += e["trl_debug_pnet_screen_weights"].each(g16=(None,)) + [e["trl_debug_pnet_screen_weights"]()]
    out += e["trl_debug_pnet_defer"].each(out4=(None,)) + [e["trl_debug_pnet_defer"]()]
    return out


def in_flight_cases(lib, ctx, D):
    """The calls between trl_detect_embed_begin and trl_detect_embed_end (both made by run())"""
    e = entries(lib, ctx, D)
    changed = {"trl_load_weights": dict(blob=None), "trl_drift_score": dict(emb=None), "trl_drift_update": dict(state=None),
               "trl_ingest_nv12": dict(n_in=0), "trl_ingest_i420": dict(n_in=0), "trl_debug_crop_resize": dict(n=0),
               "trl_debug_crop_aligned": dict(n=0), "trl_debug_crop_area": dict(n=0)}
    out = [x(**changed.get(n, {})) for n, x in e.items() if n not in NOT_IN_FLIGHT and n != "trl_detect_embed_end"]
    out += [e["trl_debug_option"](key=k, value=0) for k in (b"no_fnconv", b"pnet_gate")]
    return out


def _run(lib, cases):
    rows = []
    for label, call in cases:
        assert lib.trl_debug_option(None, None, 0) == -1                      # the last error every case starts from: "null key"
        status = call()
        rows.append([label, status, lib.trl_last_error().decode() if status else ""])
    return rows


def run(sections):
    """{section: [[case, status, message]]}: the message of a refusal, "" for a success.  "null" needs no GPU; the other three make
    one context each on device 0."""
    from truely_amd import _lib
    from truely_amd._lib import TrlConfig
    lib = _lib.load()
    out = {}
    if "null" in sections:
        out["null"] = _run(lib, null_cases(lib))
    if set(sections) - {"null"}:
        import torch
        from truely_amd import weights
        buf = torch.zeros(65536 + 256, dtype=torch.uint8, device="cuda:0")
        D = (buf.data_ptr() + 255) & ~255
        torch.cuda.synchronize()
        blob = weights.synthetic_blob(0)
        for section, cases in (("no_weights", no_weights_cases), ("idle", idle_cases), ("in_flight", in_flight_cases)):
            if section not in sections:
                continue
            cfg, ctx = TrlConfig(), C.c_void_p()
            assert lib.trl_default_config(C.byref(cfg)) == 0 and lib.trl_create(C.byref(cfg), C.byref(ctx)) == 0
            try:
                if section != "no_weights":
                    assert lib.trl_load_weights(ctx, blob, len(blob)) == 0, lib.trl_last_error()
                e = entries(lib, ctx, D)
                if section == "in_flight":
                    rows = _run(lib, [("trl_detect_embed_begin(the queued call)", e["trl_detect_embed_begin"]()[1])])
                    assert rows[0][1] == 0, rows
                    rows += _run(lib, cases(lib, ctx, D)) + _run(lib, [("trl_detect_embed_end(the queued call)", e["trl_detect_embed_end"]()[1])])
                else:
                    rows = _run(lib, cases(lib, ctx, D))
                out[section] = rows
            finally:
                lib.trl_destroy(ctx)
        del buf
    return out


def names_of(rows):
    return {r[0].split("(")[0] for r in rows}


def text(data) -> str:
    return json.dumps(data, indent=0, allow_nan=False) + "\n"


if __name__ == "__main__":
    assert sys.argv[1:2] == ["--record"] and len(sys.argv) <= 3, __doc__
    sys.path.insert(0, ROOT)
    import truely_amd  # noqa: F401
    open(sys.argv[2] if len(sys.argv) == 3 else GOLDEN, "w").write(text(run(SECTIONS)))
