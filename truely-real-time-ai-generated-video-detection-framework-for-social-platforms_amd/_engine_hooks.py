"""The inspection and test hooks of an :class:`~truely_amd.engine.Engine`: every method that calls a ``trl_debug_*`` entry of
libtruely_hip.so (csrc/trl_hooks.hip, csrc/trl_redzone.hip).  The parity tests call them on the engine; no production path does.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class EngineHooks:
    """Base class of Engine, which provides ``lib``, ``_h``, ``cfg``, ``device``, ``_frames`` and ``_stream``."""


    def stage_boxes(self, stage: int, frame: int, max_rows: int | None = None) -> np.ndarray:
        k = C.c_int()
        if max_rows is None:                              # every row the stage produced
            _lib.check(self.lib.trl_debug_stage_boxes(self._h, stage, frame, None, 0, C.byref(k)))
            max_rows = max(1, k.value)
        buf = np.zeros((max_rows, 5), np.float32)
        _lib.check(self.lib.trl_debug_stage_boxes(self._h, stage, frame, buf.ctypes.data_as(C.c_void_p), max_rows, C.byref(k)))
        return buf[:min(k.value, max_rows)].copy()

    def pyramid_level(self, frame, level: int) -> torch.Tensor:
        """Test hook: pyramid level of one frame as the fused PNet kernel reads it, (h, w, 3) float32."""
        fr = self._frames(frame[None] if getattr(frame, "ndim", 4) == 3 else frame)
        _, H, W, _ = fr.shape
        m = 12.0 / self.cfg.min_face_size
        out = torch.empty((int(H * m + 1) * int(W * m + 1) * 3,), dtype=torch.float32, device=self.device)
        h, w = C.c_int(), C.c_int()
        _lib.check(self.lib.trl_debug_pyramid_level(self._h, _ptr(fr), H, W, int(level), _ptr(out), C.byref(h), C.byref(w), self._stream()))
        return out[:h.value * w.value * 3].view(h.value, w.value, 3)

    def pyramid_batch(self, frames):
        """Test hook: the pyramid of an n-frame batch through the production pyramid pass, as the raw workspace
        (n, pyr_stride, 3) float32 -- frame f, level l at [f, pix0:pix0 + h*w], the level's padding up to pix0 + pix_pad -- and the
        per-level layout, a list of dicts {pix0, h, w, pix_pad}."""
        fr = self._frames(frames)
        n, H, W, _ = fr.shape
        stride, L = C.c_longlong(), C.c_int()
        lv = np.zeros((16, 4), np.int32)
        _lib.check(self.lib.trl_debug_pyramid_batch(self._h, _ptr(fr), n, H, W, None, C.byref(stride), lv.ctypes.data_as(C.c_void_p), 16,
                                                    C.byref(L), self._stream()))
        out = torch.empty((n, stride.value, 3), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.trl_debug_pyramid_batch(self._h, _ptr(fr), n, H, W, _ptr(out), C.byref(stride), lv.ctypes.data_as(C.c_void_p), 16,
                                                    C.byref(L), self._stream()))
        levels = [dict(zip(("pix0", "h", "w", "pix_pad"), (int(v) for v in lv[l]))) for l in range(L.value)]
        return out, levels

    PYR_KERNELS = {1: "F", 2: "S4", 3: "S8", 4: "SW4", 5: "SW8", 6: "L0-3", 7: "L0-4", 8: "L0-5", 9: "L1", 10: "L2"}   # TRL_PYR_*

    def pyramid_plan(self):
        """Test hook: what the last pyramid pass of this context chose per level, a list of dicts {kernel ("F", "S4", "S8", "SW4",
        "SW8", "L0-3", "L0-4", "L0-5", "L1", "L2"), row_bands, col_bands, cols_per_band, frames_per_launch, khmax}; [] after a
        refused call."""
        rows = np.zeros((16, 6), np.int32)
        L = C.c_int()
        _lib.check(self.lib.trl_debug_pyramid_plan(self._h, rows.ctypes.data_as(C.c_void_p), 16, C.byref(L)))
        keys = ("row_bands", "col_bands", "cols_per_band", "frames_per_launch", "khmax")
        return [dict(kernel=self.PYR_KERNELS[int(r[0])], **dict(zip(keys, (int(v) for v in r[1:])))) for r in rows[:L.value]]

    FN_FAMILIES = {1: "fn_conv", 2: "fn_conv_split4", 3: "conv_tap", 4: "conv_igemm_vec", 5: "conv_igemm_scalar",
                   6: "conv_splitk4", 7: "conv_splitk4_tap", 8: "conv_tap48", 9: "conv_bf16"}   # TRL_FNK_*
    FN_PLAN_DTYPE = np.dtype([(k, np.int32) for k in ("conv", "family", "bm", "bn", "bk", "pad", "nz", "m", "cout", "k", "precision",
                                                      "has_res")] + [("layer", "S48")])

    def facenet_plan(self):
        """Test hook: one dict per conv launch of this context's last embedder call, in walk order: conv (index), layer, family
        ("fn_conv", "fn_conv_split4", "conv_tap", "conv_igemm_vec", "conv_igemm_scalar", "conv_splitk4", "conv_splitk4_tap",
        "conv_tap48", "conv_bf16"), bm, bn, bk, pad, nz (convs sharing the launch), m, cout, k, precision (0 f32 / 1 bf16 / 2 fp16),
        has_res."""
        return self._plan_rows(self.lib.trl_debug_facenet_plan)

    def mtcnn_plan(self):
        """Test hook: one dict per R-/O-Net tail conv launch of this context's last stage_net() call, chunk after chunk, with the
        keys of facenet_plan (layer = "rnet.conv2", ..., "onet.heads"; conv = row index)."""
        return self._plan_rows(self.lib.trl_debug_mtcnn_plan)

    def _plan_rows(self, fn):
        n = C.c_int()
        _lib.check(fn(self._h, None, 0, C.byref(n)))
        rows = np.zeros(n.value, self.FN_PLAN_DTYPE)
        _lib.check(fn(self._h, rows.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        out = []
        for r in rows:
            d = {k: int(r[k]) for k in self.FN_PLAN_DTYPE.names if k != "layer"}
            d["family"] = self.FN_FAMILIES[d["family"]]
            d["layer"] = r["layer"].decode()
            out.append(d)
        return out

    def facenet_capture(self, conv_index: int):
        """Test hook: the next embedder call on this context copies conv ``conv_index``'s input, residual and output views
        (walk order of facenet_plan; -1 disarms); read them with facenet_captured()."""
        _lib.check(self.lib.trl_debug_facenet_capture(self._h, int(conv_index)))

    def facenet_captured(self):
        """(input, residual or None, output) of the last armed capture: dense NHWC numpy arrays, float32, or uint16 holding the
        bf16 / fp16 bits in reduced-precision mode."""
        out = []
        for v in range(3):
            dims = np.zeros(5, np.int32)
            _lib.check(self.lib.trl_debug_facenet_capture_read(self._h, v, None, 0, dims.ctypes.data_as(C.c_void_p)))
            if dims[3] == 0:
                out.append(None)
                continue
            a = np.empty(tuple(int(d) for d in dims[:4]), np.float32 if dims[4] == 4 else np.uint16)
            _lib.check(self.lib.trl_debug_facenet_capture_read(self._h, v, a.ctypes.data_as(C.c_void_p), a.nbytes,
                                                               dims.ctypes.data_as(C.c_void_p)))
            out.append(a)
        return tuple(out)

    def batch_capacity(self, t2_per_frame: float = 0.0, t3_per_frame: float = 0.0) -> int:
        """Test hook: set the optimistic R-/O-Net candidate capacities (per frame) and return the attempts the last call took."""
        k = C.c_int()
        _lib.check(self.lib.trl_debug_batch_capacity(self._h, float(t2_per_frame), float(t3_per_frame), C.byref(k)))
        return k.value

    def option(self, key: str, value: int):
        """Test hook (``trl_debug_option``): "rnet_chunk" / "onet_chunk" / "pnet_screen" / "pnet_defer" / "pnet_defer_cap" / "pyr_row_bands" /
        "tail_pool" (this context), "no_fnconv" (process-wide)."""
        _lib.check(self.lib.trl_debug_option(self._h, key.encode(), int(value)))

    def nms_tiers(self, small: int = 0, full: int = 0):
        """Test hook: LDS tiers (candidates per list) of the sort + NMS kernels; lists longer than ``full`` take the
        global-memory spill tier.  Results never depend on the tiers."""
        _lib.check(self.lib.trl_debug_nms_tiers(self._h, int(small), int(full)))

    def list_stats(self) -> dict:
        """Candidate-list statistics of the last call (attempts, lists in the spill tier, capacities, largest counts)."""
        t = (C.c_longlong * 8)()
        _lib.check(self.lib.trl_debug_list_stats(self._h, t))
        keys = ("attempts", "spill_lists", "spill_used", "spill_cap", "cap_frame", "slots_per_frame", "max_level_count", "max_frame_total")
        return dict(zip(keys, (int(v) for v in t)))

    def pnet_screen_bound(self):
        """Test hook: (A, B, on) of the fused PNet's fp16 conv3 screen, |d_screen - d_exact| <= A X + B."""
        A, B, on = C.c_float(), C.c_float(), C.c_int()
        _lib.check(self.lib.trl_debug_pnet_screen_bound(self._h, C.byref(A), C.byref(B), C.byref(on)))
        return float(A.value), float(B.value), bool(on.value)

    def pnet_screen_weights(self):
        """Test hook: the sixteen per-channel error weights g of the screen's bound, E = sum of g[channel] |x| over a cell's
        3 x 3 x 16 conv2 inputs + B."""
        g = (C.c_float * 16)()
        _lib.check(self.lib.trl_debug_pnet_screen_weights(self._h, g))
        return [float(v) for v in g]

    def pnet_defer(self) -> dict:
        """Test hook: the fused PNet's confirm queue in the last attempt of the last call -- ``slots`` (0: the exact conv3 chain ran
        inline), ``queued`` M-tiles that asked for a slot, ``mtiles`` of the launch, ``hold`` calls the inline path is kept for."""
        t = (C.c_longlong * 4)()
        _lib.check(self.lib.trl_debug_pnet_defer(self._h, t))
        return dict(zip(("slots", "queued", "mtiles", "hold"), (int(v) for v in t)))

    def pnet_run(self, run: int = 0):
        """Test / tuning hook: tiles per cursor fetch of the fused PNet launch (0 = automatic); > 1 exercises the halo carry."""
        _lib.check(self.lib.trl_debug_pnet_run(self._h, int(run)))

    def stage_totals(self):
        """(boxes that entered R-Net, boxes that entered O-Net) over the whole batch of the last call."""
        t = (C.c_int32 * 2)()
        _lib.check(self.lib.trl_debug_stage_totals(self._h, t))
        return int(t[0]), int(t[1])

    def workspace(self, what: int = 0, n: int = 0, h: int = 0, w: int = 0) -> dict:
        """Test hook (``trl_debug_workspace``): the two workspaces of the context in bytes -- ``scratch_cap``, ``scratch_high`` (the
        high-water offset of the last call that used the scratch), ``arena_cap``, ``arena_off``, ``arena_need`` -- and ``need``, the
        dry-run count of a call that is not run: what=1 facenet_embed on n faces of h x w, what=24 / 48 rnet() / onet() on n crops."""
        o = (C.c_longlong * 6)()
        _lib.check(self.lib.trl_debug_workspace(self._h, int(what), int(n), int(h), int(w), o))
        return dict(zip(("scratch_cap", "scratch_high", "arena_cap", "arena_off", "arena_need", "need"), (int(v) for v in o)))

    def poison_workspaces(self, byte: int = 0xFF):
        """Test hook: fill the activation workspaces with a byte pattern (0xFF = NaNs)."""
        _lib.check(self.lib.trl_debug_poison(self._h, int(byte)))

    def redzone(self, guard: int, byte: int = 0xA5):
        """Test hook (``trl_debug_redzone``): follow every block of the context's two workspaces with ``guard`` bytes of red zone
        (a multiple of 256; 0 = off) filled with ``byte``, and sweep them at every rewind and at the end of every call."""
        _lib.check(self.lib.trl_debug_redzone(self._h, int(guard), int(byte)))

    def redzone_report(self, clear: bool = False, sweep: bool = False) -> dict:
        """``sweeps`` made, guard ``bytes`` checked and ``hits`` (dicts: arena, site, block, block_bytes, gap_off, gap_bytes, first,
        last, count; ``nhits`` counts those past the first 256 too) since ``redzone()`` or the last ``clear``.  ``sweep``: sweep
        both workspaces first (site "report")."""
        o = (C.c_longlong * 4)()
        hits = (_lib.TrlRzHit * 256)()
        _lib.check(self.lib.trl_debug_redzone_report(self._h, (1 if clear else 0) | (2 if sweep else 0), o, hits, 256))
        rows = [dict(arena=int(h.arena), site=h.site.decode(), block=int(h.block), block_bytes=int(h.block_bytes), gap_off=int(h.gap_off),
                     gap_bytes=int(h.gap_bytes), first=int(h.first), last=int(h.last), count=int(h.count)) for h in hits[:int(o[3])]]
        return dict(sweeps=int(o[0]), bytes=int(o[1]), nhits=int(o[2]), hits=rows)

    def redzone_poke(self, arena: int, block: int, offset: int, value: int = 0x3C):
        """Self-test of the sweep: one byte ``value`` at ``offset`` of the gap behind block ``block`` (-1: the tail) of workspace
        ``arena`` (0 = cascade lists, 1 = scratch).  The next sweep reports exactly that byte."""
        _lib.check(self.lib.trl_debug_redzone_poke(self._h, int(arena), int(block), int(offset), int(value)))

    def level_counts(self, frame: int):
        a = np.zeros(32, np.int32); b = np.zeros(32, np.int32)
        L = C.c_int()
        _lib.check(self.lib.trl_debug_level_counts(self._h, frame, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), C.byref(L)))
        return a[:L.value].tolist(), b[:L.value].tolist()

    CAND_DTYPE = np.dtype([("box", np.float32, 4), ("score", np.float32), ("reg", np.float32, 4), ("cell", np.int32)])

    def level_keep(self, frame: int, level: int):
        """Test hook: (records in APPEND order, pick list) of one (frame, level) of the last call: the pick list holds indices into
        the records, in pick order (descending score) -- the per-level batched_nms(0.5) of detect_face()."""
        k = C.c_int()
        _lib.check(self.lib.trl_debug_level_cands(self._h, int(frame), int(level), None, 0, C.byref(k)))
        rec = np.zeros((max(1, k.value),), self.CAND_DTYPE)
        _lib.check(self.lib.trl_debug_level_cands(self._h, int(frame), int(level), rec.ctypes.data_as(C.c_void_p), len(rec), C.byref(k)))
        rec = rec[:k.value]
        _lib.check(self.lib.trl_debug_level_keep(self._h, int(frame), int(level), None, 0, C.byref(k)))
        idx = np.zeros((max(1, k.value),), np.int32)
        _lib.check(self.lib.trl_debug_level_keep(self._h, int(frame), int(level), idx.ctypes.data_as(C.c_void_p), len(idx), C.byref(k)))
        return rec, idx[:k.value]

    def level_cands(self, frame: int, level: int) -> np.ndarray:
        """Test hook: the candidate records the PNet kernel appended for (frame, level) in the last call, sorted by cell."""
        k = C.c_int()
        _lib.check(self.lib.trl_debug_level_cands(self._h, int(frame), int(level), None, 0, C.byref(k)))
        buf = np.zeros((max(1, k.value),), self.CAND_DTYPE)
        _lib.check(self.lib.trl_debug_level_cands(self._h, int(frame), int(level), buf.ctypes.data_as(C.c_void_p), len(buf), C.byref(k)))
        rows = buf[:min(k.value, len(buf))]
        return rows[np.argsort(rows["cell"], kind="stable")].copy()

    def pnet_level(self, frame, level: int):
        fr = self._frames(frame[None] if frame.ndim == 3 else frame)
        _, H, W, _ = fr.shape
        prob = torch.empty((H * W,), dtype=torch.float32, device=self.device)
        reg = torch.empty((H * W * 4,), dtype=torch.float32, device=self.device)
        oh, ow = C.c_int(), C.c_int()
        _lib.check(self.lib.trl_debug_pnet_level(self._h, _ptr(fr), H, W, level, _ptr(prob), _ptr(reg), C.byref(oh), C.byref(ow), self._stream()))
        k = oh.value * ow.value
        return prob[:k].reshape(oh.value, ow.value), reg[:4 * k].reshape(oh.value, ow.value, 4)

    def rnet(self, crops: torch.Tensor) -> torch.Tensor:
        crops = crops.to(self.device, torch.float32).contiguous()
        out = torch.empty((crops.shape[0], 6), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.trl_debug_rnet(self._h, _ptr(crops), crops.shape[0], _ptr(out), self._stream()))
        return out

    def onet(self, crops: torch.Tensor) -> torch.Tensor:
        crops = crops.to(self.device, torch.float32).contiguous()
        out = torch.empty((crops.shape[0], 16), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.trl_debug_onet(self._h, _ptr(crops), crops.shape[0], _ptr(out), self._stream()))
        return out

    def front_net(self, frame, boxes: np.ndarray, net: int) -> torch.Tensor:
        """Test hook: R-Net (net=24 -> [nb, 6]) or O-Net (net=48 -> [nb, 16]) through the production front kernel + tail on the
        given boxes (x1, y1, x2, y2) of one frame."""
        fr = self._frames(frame[None] if getattr(frame, "ndim", 4) == 3 else frame)
        _, H, W, _ = fr.shape
        b = np.ascontiguousarray(boxes, np.float32).reshape(-1, 4)
        out = torch.empty((len(b), 6 if net == 24 else 16), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.trl_debug_front_net(self._h, _ptr(fr), H, W, b.ctypes.data_as(C.c_void_p), len(b), int(net), _ptr(out), self._stream()))
        return out

    def stage_net(self, frames, recs: np.ndarray, net: int, capacity: int, fill: float | None = None) -> torch.Tensor:
        """Test hook: the production stage-2 / stage-3 loop (chunked front kernel + tail, trl_stage_net) over ``capacity``
        candidate slots, ``len(recs)`` of them live: recs rows (frame, x1, y1, x2, y2).  Returns [capacity, 6] (net=24) or
        [capacity, 16] (net=48); rows past len(recs) are not defined (``fill``, if given, is what the output held before)."""
        fr = self._frames(frames)
        nf, H, W, _ = fr.shape
        r = np.ascontiguousarray(recs, np.float32).reshape(-1, 5)
        shape = (int(capacity), 6 if net == 24 else 16)
        out = torch.empty(shape, dtype=torch.float32, device=self.device) if fill is None else \
            torch.full(shape, fill, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.trl_debug_stage_net(self._h, _ptr(fr), nf, H, W, r.ctypes.data_as(C.c_void_p), len(r), int(net),
                                                int(capacity), _ptr(out), self._stream()))
        return out

    def front_pool(self, frames, win: np.ndarray, net: int, capacity: int | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
        """Test hook (``trl_debug_front``): the front kernel's own output.  ``win`` rows are int32 (frame, y0, x0, ih, iw), the
        crop window itself; the launch covers ``capacity`` slots (default len(win)).  Returns the pooled maps [capacity, 11, 11, 28]
        (net=24) or [capacity, 23, 23, 32] (net=48); maps past len(win) keep what ``out`` held.  A device tensor is passed on as it
        is; its address must be a multiple of 4, as for every call that takes frames."""
        fr = self._frames(frames)
        nf, H, W, _ = fr.shape
        w = np.ascontiguousarray(win, np.int32).reshape(-1, 5)
        cap = len(w) if capacity is None else int(capacity)
        shape = (cap, 11, 11, 28) if net == 24 else (cap, 23, 23, 32)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != self.device or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous float32 {shape} tensor on {self.device}")
        _lib.check(self.lib.trl_debug_front(self._h, _ptr(fr), nf, H, W, w.ctypes.data_as(C.c_void_p), len(w), int(net), cap, _ptr(out),
                                            self._stream()))
        return out

    def lists(self, kind: int, H: int, W: int, caps, counts, rows: np.ndarray, logits: np.ndarray | None = None) -> dict:
        """Test hook (``trl_debug_lists``): the cascade's list kernels on caller-built lists of frames H x W, launched as the
        cascade launches them.  ``caps`` = level capacities then the per-frame capacity.
        kind 1: ``rows`` = CAND_DTYPE records of every (frame, level) in append order, ``counts`` [n][L] -> {"keep": [n][L] pick
        lists (indices into that list's records), "rows1": [n] stage-1 rows}.
        kind 2: ``rows`` = stage-1 rows [total][5] (frame-major), ``counts`` [n], ``logits`` [total][6] -> {"rows2": [n]}.
        kind 3: stage-2 rows, ``logits`` [total][16] -> {"rows3", "pts3": [n] per frame, and the k_select outputs "boxes",
        "probs", "points", "counts", "box0", "prob0", "rect", "valid" as numpy arrays}."""
        caps = np.ascontiguousarray(caps, np.int32)
        counts = np.ascontiguousarray(counts, np.int32)
        n = counts.shape[0]
        L = counts.shape[1] if kind == 1 else 0
        assert len(caps) == L + 1
        rows = np.ascontiguousarray(rows, self.CAND_DTYPE if kind == 1 else np.float32)
        lg = None if logits is None else np.ascontiguousarray(logits, np.float32)
        capF = int(caps[-1])
        out = {}
        if kind == 3:
            mf = self.cfg.max_faces
            dev = dict(boxes=torch.empty((n, mf, 4), dtype=torch.float32, device=self.device),
                       probs=torch.empty((n, mf), dtype=torch.float32, device=self.device),
                       points=torch.empty((n, mf, 10), dtype=torch.float32, device=self.device),
                       counts=torch.empty((n,), dtype=torch.int32, device=self.device),
                       box0=torch.empty((n, 4), dtype=torch.float32, device=self.device),
                       prob0=torch.empty((n,), dtype=torch.float32, device=self.device),
                       rect=torch.empty((n, 4), dtype=torch.int32, device=self.device),
                       valid=torch.empty((n,), dtype=torch.uint8, device=self.device))
            pts = np.zeros((n, capF, 10), np.float32)
        else:
            dev = dict.fromkeys(("boxes", "probs", "points", "counts", "box0", "prob0", "rect", "valid"))
            pts = None
        _lib.check(self.lib.trl_debug_lists(self._h, int(kind), n, int(H), int(W), caps.ctypes.data_as(C.c_void_p), L,
                                            counts.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p),
                                            None if lg is None else lg.ctypes.data_as(C.c_void_p),
                                            None if pts is None else pts.ctypes.data_as(C.c_void_p),
                                            *(_ptr(dev[k]) for k in ("boxes", "probs", "points", "counts", "box0", "prob0", "rect", "valid")),
                                            self._stream()))
        torch.cuda.synchronize(self.device)
        if kind == 1:
            out["keep"] = [[self.level_keep(f, l)[1] for l in range(L)] for f in range(n)]
        out[f"rows{kind}"] = [self.stage_boxes(kind, f) for f in range(n)]
        if kind == 3:
            out["pts3"] = [pts[f, :len(out["rows3"][f])].copy() for f in range(n)]
            out.update({k: v.cpu().numpy() for k, v in dev.items()})
        return out

    def _faces_out(self, out: torch.Tensor | None, n: int, S: int) -> torch.Tensor:
        """The destination of a crop hook: a new tensor, or the caller's (e.g. pre-filled, to see what the kernel wrote)."""
        if out is None:
            return torch.empty((n, S, S, 3), dtype=torch.float32, device=self.device)
        if out.shape != (n, S, S, 3) or out.dtype != torch.float32 or out.device != self.device or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous float32 ({n}, {S}, {S}, 3) tensor on {self.device}")
        return out

    def crop_resize(self, frames, rect: torch.Tensor, valid: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """The default crop alone (model.py:55-58): each frame's rectangle (rect [n,4] = x0, y0, x1, y1) -> 80 x 80, / 255."""
        fr = self._frames(frames)
        n, H, W, _ = fr.shape
        rect = rect.to(self.device, torch.int32).contiguous(); valid = valid.to(self.device, torch.uint8).contiguous()
        if rect.shape != (n, 4) or valid.shape != (n,):
            raise ValueError("rect must be (n, 4) and valid (n,)")
        out = self._faces_out(out, n, 80)
        _lib.check(self.lib.trl_debug_crop_resize(self._h, _ptr(fr), n, H, W, _ptr(rect), _ptr(valid), _ptr(out), self._stream()))
        return out

    def crop_aligned(self, frames, pts: torch.Tensor, valid: torch.Tensor, S: int = 160, rgb: bool = True,
                     out: torch.Tensor | None = None) -> torch.Tensor:
        """Embedding mode 3's crop alone: five-point similarity alignment of each frame's face (pts [n,10] = x0..x4, y0..y4)."""
        fr = self._frames(frames)
        n, H, W, _ = fr.shape
        pts = pts.to(self.device, torch.float32).contiguous(); valid = valid.to(self.device, torch.uint8).contiguous()
        if pts.shape != (n, 10) or valid.shape != (n,):
            raise ValueError("pts must be (n, 10) and valid (n,)")
        out = self._faces_out(out, n, int(S))
        _lib.check(self.lib.trl_debug_crop_aligned(self._h, _ptr(fr), n, H, W, _ptr(pts), _ptr(valid), int(S), int(bool(rgb)), _ptr(out),
                                                   self._stream()))
        return out

    def crop_area(self, frames, rect: torch.Tensor, valid: torch.Tensor, S: int = 160, rgb: bool = False,
                  out: torch.Tensor | None = None) -> torch.Tensor:
        """Embedding mode 1 / 2's crop alone: each frame's rectangle (rect [n,4] = x0, y0, x1, y1) area-pooled to S x S,
        truncated to bytes, (v - 127.5) / 128, channels reversed when ``rgb``."""
        fr = self._frames(frames)
        n, H, W, _ = fr.shape
        rect = rect.to(self.device, torch.int32).contiguous(); valid = valid.to(self.device, torch.uint8).contiguous()
        if rect.shape != (n, 4) or valid.shape != (n,):
            raise ValueError("rect must be (n, 4) and valid (n,)")
        out = self._faces_out(out, n, int(S))
        _lib.check(self.lib.trl_debug_crop_area(self._h, _ptr(fr), n, H, W, _ptr(rect), _ptr(valid), int(S), int(bool(rgb)), _ptr(out),
                                                self._stream()))
        return out

    def pnet_span(self, reset: bool = False):
        """(milliseconds, launches): execution spans of the fused PNet launches of this context since the last reset, summed on
        the device (first workgroup start to last workgroup end: the duration rocprofv3 reports for the kernel)."""
        ms, k = C.c_double(), C.c_int32()
        _lib.check(self.lib.trl_debug_pnet_span(self._h, 1 if reset else 0, C.byref(ms), C.byref(k)))
        return float(ms.value), int(k.value)

    def timings(self):
        t = (C.c_float * 4)()
        _lib.check(self.lib.trl_debug_timings(self._h, t))
        k = C.c_float()
        _lib.check(self.lib.trl_debug_pnet_kernel_ms(self._h, C.byref(k)))
        return {"pnet_ms": t[0], "call_ms": t[1], "pnet_launches": int(t[2]), "pyramid_ms": t[3], "pnet_kernel_ms": float(k.value)}
