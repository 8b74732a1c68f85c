"""``DeviceJpeg``: the Motion-JPEG encoder of ``trl_jpeg.hip`` behind a small Python object.

Each frame's file is byte-identical to Pillow's ``Image.save(format="JPEG", quality=q, subsampling=2)`` of the RGB frame, which is
what ``AviMjpegWriter`` writes with its Pillow encoder: the device encoder changes how fast ``run()``'s annotated output is
written, not what is written.  The encoder owns its device workspace and its own stream, independent of the cascade contexts
(run()'s contexts are busy while the writer thread encodes)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib


class DeviceJpeg:
    """``encode(frames)``: a uint8 BGR batch (n, H, W, 3) -- host array or device tensor, any stride between frames -- to a list of
    n JPEG files (bytes).  ``max_frames`` bounds one call's batch (larger batches are split)."""

    def __init__(self, W: int, H: int, quality: int = 80, device=None, max_frames: int = 32):
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"DeviceJpeg needs a GPU device, got {self.device}")
        self.W, self.H, self.quality, self.max_frames = int(W), int(H), int(quality), int(max_frames)
        self.lib = _lib.load()
        self.stream = torch.cuda.Stream(self.device)
        h = C.c_void_p()
        _lib.check(self.lib.trl_jpeg_create(self.device.index or 0, self.H, self.W, self.quality, self.max_frames, C.byref(h)))
        self.h = h
        n = C.c_int(0)
        self.lib.trl_jpeg_header(self.H, self.W, self.quality, None, 0, C.byref(n))
        self.header_len = n.value
        # start capacity: a generous guess for ordinary content; the first batch that needs more grows it (grow and re-run)
        self.capacity = self.max_frames * (self.header_len + 2 + self.H * self.W // 2 + 4096)
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
