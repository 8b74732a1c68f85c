"""``DeviceJpeg`` and ``DeviceJpegDecoder``: the Motion-JPEG encoder of ``trl_jpeg.hip`` and the decoder of ``trl_jpegd.hip``, each
behind a small Python object.

Each frame's file is byte-identical to Pillow's ``Image.save(format="JPEG", quality=q, subsampling=s, restart_marker_rows=r |
restart_marker_blocks=b, optimize=o)`` of the RGB frame (defaults: 4:2:0, no restart markers, standard tables), which is what
``AviMjpegWriter`` writes with its Pillow encoder: the device encoder changes how fast ``run()``'s annotated output is
written, not what is written.  The encoder owns its device workspace and its own stream, independent of the cascade contexts
(run()'s contexts are busy while the writer thread encodes)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib


class DeviceJpeg:
    """``encode(frames)``: a uint8 BGR batch (n, H, W, 3) -- host array or device tensor, any stride between frames -- to a list of
    n JPEG files (bytes).  ``max_frames`` bounds one call's batch (larger batches are split).  ``subsampling`` 0 / 1 / 2 = 4:4:4 /
    4:2:2 / 4:2:0, ``restart_rows`` / ``restart_blocks`` (an interval in MCU rows / in MCUs; rows win) and ``optimize`` (per-frame
    Huffman tables) mean what they mean to Pillow's ``Image.save``; a stream with ``restart_rows=1`` is the kind
    ``DeviceJpegDecoder`` reads fastest."""

    def __init__(self, W: int, H: int, quality: int = 80, device=None, max_frames: int = 32, subsampling: int = 2,
                 restart_rows: int = 0, restart_blocks: int = 0, optimize: bool = False):
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"DeviceJpeg needs a GPU device, got {self.device}")
        self.W, self.H, self.quality, self.max_frames = int(W), int(H), int(quality), int(max_frames)
        self.subsampling, self.restart_rows, self.restart_blocks = int(subsampling), int(restart_rows), int(restart_blocks)
        self.optimize = bool(optimize)
        self.lib = _lib.load()
        self.stream = torch.cuda.Stream(self.device)
        h = C.c_void_p()
        opt = _lib.TrlJpegOptions(self.quality, self.subsampling, self.restart_rows, self.restart_blocks, int(self.optimize))
        _lib.check(self.lib.trl_jpeg_create_ex(self.device.index or 0, self.H, self.W, C.byref(opt), self.max_frames, C.byref(h)))
        self.h = h
        n = C.c_int(0)
        self.lib.trl_jpeg_header_ex(self.H, self.W, C.byref(opt), None, 0, C.byref(n))      # (no buffer: the length only)
        self.header_len = n.value                         # (optimize: an upper bound on every frame's header)
        # start capacity: a generous guess for ordinary content -- a third of a byte per sample (4:2:0 has 1.5 samples per pixel,
        # 4:2:2 2, 4:4:4 3) and the restart markers; the first batch that needs more grows it (grow and re-run)
        mw, mh = (8, 8) if self.subsampling == 0 else (16, 8) if self.subsampling == 1 else (16, 16)
        mcux, mcuy = -(-self.W // mw), -(-self.H // mh)
        interval = min(self.restart_rows * mcux, 65535) if self.restart_rows > 0 else self.restart_blocks
        markers = 2 * (-(-mcux * mcuy // interval) - 1) if interval > 0 else 0
        samples6 = (6, 4, 3)[self.subsampling]            # samples per pixel x 2
        self.capacity = self.max_frames * (self.header_len + 2 + self.H * self.W * samples6 // 6 + markers + 4096)
        self.out = torch.empty(self.capacity, dtype=torch.uint8, device=self.device)
        self.host = torch.empty(self.capacity, dtype=torch.uint8).pin_memory()
        self.sizes = np.zeros(self.max_frames, np.int64)
        self.staging = None                               # device copy of host batches
        self.reruns = 0                                   # grow-and-re-run count (tests)

    def __del__(self):
        h = getattr(self, "h", None)
        if h is not None and h.value:
            self.lib.trl_jpeg_destroy(h)
            self.h = None

    def _grow(self, need: int):
        self.capacity = int(need * 1.25) + 4096
        self.out = torch.empty(self.capacity, dtype=torch.uint8, device=self.device)
        self.host = torch.empty(self.capacity, dtype=torch.uint8).pin_memory()

    def encode_device(self, frames: torch.Tensor):
        """Device batch -> (device buffer, sizes): the n files lie back to back at the start of the returned buffer.  Work is
        ordered after everything already queued on the current stream."""
        n = frames.shape[0]
        if frames.dtype != torch.uint8 or frames.dim() != 4 or tuple(frames.shape[1:]) != (self.H, self.W, 3):
            raise ValueError(f"expected uint8 frames (n, {self.H}, {self.W}, 3), got {tuple(frames.shape)} {frames.dtype}")
        if frames.device != self.device:
            raise ValueError(f"frames on {frames.device}, encoder on {self.device}")
        if n and tuple(frames.stride()[1:]) != (self.W * 3, 3, 1):
            frames = frames.contiguous()
        if n > self.max_frames:
            raise ValueError(f"batch of {n} frames > max_frames {self.max_frames}")
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        sizes = self.sizes[:n]
        stride = frames.stride(0) if n > 1 else self.H * self.W * 3
        while True:
            _lib.check(self.lib.trl_jpeg_encode(self.h, C.c_void_p(frames.data_ptr()), n, stride, C.c_void_p(self.out.data_ptr()),
                                                self.capacity, sizes.ctypes.data_as(C.c_void_p), C.c_void_p(self.stream.cuda_stream)))
            need = int(sizes.sum())
            if need <= self.capacity:
                break
            self._grow(need)
            self.reruns += 1
        frames.record_stream(self.stream)
        return self.out, sizes.copy()

    def encode(self, frames) -> list:
        """A batch of n frames -> n JPEG files.  Host frames go through a pinned staging copy on the encoder's stream."""
        if isinstance(frames, torch.Tensor) and frames.is_cuda:
            out = []
            for k in range(0, frames.shape[0], self.max_frames):
                out += self._encode_chunk(frames[k:k + self.max_frames])
            return out
        a = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frames, np.uint8))
        out = []
        for k in range(0, a.shape[0], self.max_frames):
            part = a[k:k + self.max_frames].contiguous()
            if not part.is_pinned():
                part = part.pin_memory()
            if self.staging is None:
                self.staging = torch.empty((self.max_frames, self.H, self.W, 3), dtype=torch.uint8, device=self.device)
            dev = self.staging[:part.shape[0]]
            with torch.cuda.stream(self.stream):
                dev.copy_(part, non_blocking=True)
                out += self._encode_chunk(dev)
        return out

    def _encode_chunk(self, frames: torch.Tensor) -> list:
        buf, sizes = self.encode_device(frames)
        total = int(sizes.sum())
        with torch.cuda.stream(self.stream):
            self.host[:total].copy_(buf[:total], non_blocking=True)
        self.stream.synchronize()
        data = self.host[:total].numpy()
        ends = np.cumsum(sizes)
        return [data[e - s:e].tobytes() for s, e in zip(sizes, ends)]


class DeviceJpegDecoder:
    """The baseline-JPEG decoder of ``trl_jpegd.hip`` behind a small Python object: Motion-JPEG frames to BGR on the GPU, byte for
    byte what ``np.asarray(Image.open(f).convert("RGB"))[:, :, ::-1]`` gives.

    ``decode(files)``: a list of n JPEG files (``bytes``) -> ``(frames, status)``: a uint8 device tensor (n, H, W, 3) in BGR and a
    numpy array of n statuses -- 0 decoded on the device, 1 not attempted (progressive, grayscale, another size, ...), 2 the
    entropy decoder met something irregular or a block lies outside the IDCT's gate (coefficients no encoder makes from pixels).  A frame whose status is not 0 is left unwritten (zero here): the caller decodes it
    with Pillow.  The object has its own stream, workspace and pinned staging; batches above ``max_frames`` are split.

    ``decode_into(h_arena, d_arena, offsets, sizes, out)`` is the form ``run()`` uses: the files already lie in a pinned host
    arena and in its device copy; the work is queued on the current stream and the call returns after one synchronisation."""

    def __init__(self, W: int, H: int, device=None, max_frames: int = 32):
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"DeviceJpegDecoder needs a GPU device, got {self.device}")
        self.W, self.H, self.max_frames = int(W), int(H), int(max_frames)
        self.lib = _lib.load()
        self.stream = torch.cuda.Stream(self.device)
        self.h = None
        self.max_bytes = 0
        self._create(self.max_frames * (self.H * self.W * 3 + 65536))
        self.host = self.dev = None                       # staging of decode(): pinned arena and its device copy
        self.status = np.zeros(self.max_frames, np.int32)

    def _create(self, max_bytes: int):
        h = C.c_void_p()
        _lib.check(self.lib.trl_jpegd_create(self.device.index or 0, self.H, self.W, self.max_frames, int(max_bytes), C.byref(h)))
        if self.h is not None:
            self.lib.trl_jpegd_destroy(self.h)
        self.h, self.max_bytes = h, int(max_bytes)

    def __del__(self):
        h = getattr(self, "h", None)
        if h is not None and h.value:
            self.lib.trl_jpegd_destroy(h)
            self.h = None

    def decode_into(self, h_arena: torch.Tensor, d_arena: torch.Tensor, offsets, sizes, out: torch.Tensor) -> np.ndarray:
        """Files k = sizes[k] bytes at offsets[k] of ``h_arena`` (host uint8, read during the call) and of ``d_arena`` (its device
        copy, whose upload is queued on the current stream or finished) -> ``out[k]`` (uint8 device (n, H, W, 3), any stride
        between frames).  Returns the statuses; frames whose status is not 0 are untouched."""
        offsets = np.ascontiguousarray(offsets, np.int64)
        sizes = np.ascontiguousarray(sizes, np.int64)
        n = len(offsets)
        if len(sizes) != n or out.shape[0] != n:
            raise ValueError(f"{n} offsets, {len(sizes)} sizes, {out.shape[0]} output frames")
        if out.dtype != torch.uint8 or out.dim() != 4 or tuple(out.shape[1:]) != (self.H, self.W, 3) or out.device != self.device:
            raise ValueError(f"expected uint8 frames (n, {self.H}, {self.W}, 3) on {self.device}, got {tuple(out.shape)} {out.dtype} on {out.device}")
        if n and tuple(out.stride()[1:]) != (self.W * 3, 3, 1):
            raise ValueError("output frames must be dense")
        if h_arena.dtype != torch.uint8 or d_arena.dtype != torch.uint8 or h_arena.is_cuda or d_arena.device != self.device:
            raise ValueError("arenas: uint8, one on the host and its copy on the decoder's device")
        nbytes = min(h_arena.numel(), d_arena.numel())
        if nbytes > self.max_bytes:
            self._create(nbytes)
        status = np.zeros(n, np.int32)
        stream = torch.cuda.current_stream(self.device)
        stride = out.stride(0) if n > 1 else self.H * self.W * 3
        for k in range(0, n, self.max_frames):
            m = min(self.max_frames, n - k)
            st = self.status[:m]
            _lib.check(self._decode(h_arena, d_arena, nbytes, offsets[k:k + m], sizes[k:k + m], m, out[k:k + m], stride, st, stream))
            status[k:k + m] = st
        return status

    def _decode(self, h_arena, d_arena, nbytes, offsets, sizes, m, out, stride, st, stream):
        if m and (int((offsets + sizes).max()) > nbytes or int(offsets.min()) < 0 or int(sizes.min()) < 0):
            raise ValueError(f"a file lies outside the arena of {nbytes} bytes")     # (the library checks against max_bytes >= nbytes)
        return self.lib.trl_jpegd_decode(self.h, C.c_void_p(h_arena.data_ptr()), C.c_void_p(d_arena.data_ptr()),
                                         offsets.ctypes.data_as(C.c_void_p), sizes.ctypes.data_as(C.c_void_p), m,
                                         C.c_void_p(out.data_ptr()), stride, st.ctypes.data_as(C.c_void_p), C.c_void_p(stream.cuda_stream))

    def decode(self, files):
        files = list(files)
        n = len(files)
        frames = torch.zeros((n, self.H, self.W, 3), dtype=torch.uint8, device=self.device)
        status = np.zeros(n, np.int32)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        for k in range(0, n, self.max_frames):
            part = files[k:k + self.max_frames]
            sizes = np.array([len(f) for f in part], np.int64)
            offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
            total = int(sizes.sum())
            if self.host is None or self.host.numel() < max(total, 1):
                cap = max(total + total // 4, 1 << 16)
                self.host = torch.empty(cap, dtype=torch.uint8).pin_memory()
                self.dev = torch.empty(cap, dtype=torch.uint8, device=self.device)
            hn = self.host.numpy()
            for o, f in zip(offsets, part):
                hn[o:o + len(f)] = np.frombuffer(f, np.uint8)
            with torch.cuda.stream(self.stream):
                self.dev[:total].copy_(self.host[:total], non_blocking=True)
                status[k:k + len(part)] = self.decode_into(self.host, self.dev, offsets, sizes, frames[k:k + len(part)])
        frames.record_stream(self.stream)
        return frames, status


def jpeg_info(data: bytes) -> dict:
    """What the decoder's marker parser finds in one JPEG file (host only, no GPU): ``trl_jpegd_parse`` as a dict."""
    info = _lib.TrlJpegdInfo()
    buf = (C.c_ubyte * max(len(data), 1)).from_buffer_copy(data if data else b"\0")
    _lib.check(_lib.load().trl_jpegd_parse(buf, len(data), C.byref(info)))
    return {n: getattr(info, n) for n, _ in info._fields_}
