"""Frame sources / sinks for ``model.run``.

The reference decodes with ``cv2.VideoCapture`` and re-encodes every frame with
``cv2.VideoWriter(fourcc "H264")`` (server/model.py:23,35-36,43,77).  OpenCV is not installed in
the build environment, so two back-ends exist behind the same tiny interface:

* ``cv2`` when importable (real .mp4 in, annotated .mp4 out, like the reference);
* the raw "TRLV" container (fps header + uint8 frames, BGR or -- what a hardware decoder hands over -- NV12) used by the
  tests and the benchmark.  NV12 clips take the device ingest path of ``model.run``;
* Motion-JPEG in AVI (``AviMjpegWriter`` / ``AviMjpegReader``): the annotated OUTPUT when OpenCV is absent -- a bounded standard
  file instead of raw frames, encoded by Pillow's libjpeg or, byte-identical, by the HIP encoder (jpeg.DeviceJpeg) -- and the one
  compressed INPUT this build decodes by itself: ``run()`` reads the chunks of the frames it needs by position and decodes them
  on the GPU (jpeg.DeviceJpegDecoder: baseline 4:2:0 / 4:2:2 / 4:4:4, byte-identical to Pillow), with Pillow for any frame
  the device decoder does not attempt and for ``cap.read()``;
* YUV4MPEG2 (``.y4m``, 4:2:0 progressive): the uncompressed interchange format every decoder can emit
  (``ffmpeg -i clip.mp4 -pix_fmt yuv420p clip.y4m``).  Planes are repacked to NV12 on the fly and take the same device ingest.
``AsyncWriter`` is the decoupled, skippable annotated-output stage: drawing and encoding run on their
own thread behind a bounded queue, so the analysis loop never waits for the encoder (the reference draws and encodes inline,
server/model.py:67-77).
"""
from __future__ import annotations

import os
import struct
import threading

import numpy as np

from . import annotate as _annotate

_MAGIC = b"TRLV0001"

try:  # pragma: no cover - not available offline
    import cv2  # type: ignore
except Exception:  # noqa: BLE001
    cv2 = None


class RawReader:
    def __init__(self, path):
        self.f = open(path, "rb")
        head = self.f.read(32)
        if len(head) < 32 or head[:8] != _MAGIC:
            self.f.close()
            raise ValueError("not a TRLV file")
        self.n, self.height, self.width = struct.unpack("<III", head[8:20])
        (self.fps_f,) = struct.unpack("<d", head[20:28])
        (fmt,) = struct.unpack("<I", head[28:32])
        self.pixfmt = "nv12" if fmt == 1 else "bgr"
        self.frame_bytes = self.height * self.width * 3 // (2 if fmt == 1 else 1)
        self.i = 0
        self.data0, self.stride = 32, self.frame_bytes    # random access (model.run's reader reads only what it needs, in parallel)
        self.raw_pixfmt = self.pixfmt                     # layout of the bytes at frame_offset()
        avail = max(0, (os.path.getsize(path) - 32) // self.frame_bytes) if self.frame_bytes else 0
        self.n = min(self.n, avail)                       # a truncated file ends where its bytes end

    def frame_offset(self, i: int) -> int:
        return self.data0 + i * self.stride

    def isOpened(self):
        return True

    def read(self):
        """(ok, frame): BGR (H, W, 3) for a BGR clip, the flat NV12 frame (H*W*3/2,) for an NV12 clip."""
        if self.i >= self.n:
            return False, None
        buf = self.f.read(self.frame_bytes)
        if len(buf) < self.frame_bytes:
            return False, None
        self.i += 1
        a = np.frombuffer(buf, np.uint8)
        return True, (a.copy() if self.pixfmt == "nv12" else a.reshape(self.height, self.width, 3).copy())

    def release(self):
        self.f.close()


class Y4MReader:
    """YUV4MPEG2 4:2:0 progressive.  ``read()`` yields flat NV12 frames (Y plane, then interleaved U/V) like an NV12 TRLV clip."""
    pixfmt = "nv12"

    def __init__(self, path):
        self.f = open(path, "rb")
        line = self.f.readline(256)
        if not line.startswith(b"YUV4MPEG2 ") or not line.endswith(b"\n"):
            self.f.close()
            raise ValueError("not a YUV4MPEG2 file")
        self.width = self.height = 0
        self.fps_f = 0.0
        chroma, interlace = "420jpeg", "p"
        for tok in line[10:].split():
            t, v = chr(tok[0]), tok[1:].decode("ascii", "replace")
            if t == "W":
                self.width = int(v)
            elif t == "H":
                self.height = int(v)
            elif t == "F":
                num, _, den = v.partition(":")
                self.fps_f = int(num) / max(1, int(den or 1))
            elif t == "C":
                chroma = v
            elif t == "I":
                interlace = v
        if not chroma.startswith("420") or chroma.startswith("420p1") or interlace not in ("p", "?"):
            self.f.close()
            raise ValueError(f"unsupported YUV4MPEG2 stream (chroma {chroma}, interlace {interlace}): 8-bit 4:2:0 progressive only")
        if self.width <= 0 or self.height <= 0 or self.width % 4 or self.height % 2:
            self.f.close()
            raise ValueError(f"YUV4MPEG2 {self.width}x{self.height}: the NV12 ingest needs W % 4 == 0 and even H")
        self.header = len(line)
        self.ysize, self.csize = self.width * self.height, (self.width // 2) * (self.height // 2)
        self.frame_bytes = self.ysize + 2 * self.csize
        self.n = max(0, (os.path.getsize(path) - self.header) // (6 + self.frame_bytes))   # "FRAME\n" + planes (no frame params)
        self.i = 0
        # random access to the planar frames as stored (I420: the device ingest takes them without repacking).  Only when every
        # frame header is the bare "FRAME\n" (checked on the first two); otherwise model.run falls back to sequential read()
        self.data0, self.stride, self.raw_pixfmt = self.header + 6, 6 + self.frame_bytes, "i420"
        ok = True
        for k in range(min(self.n, 2)):
            self.f.seek(self.header + k * self.stride)
            ok = ok and self.f.read(6) == b"FRAME\n"
        self.f.seek(self.header)
        if not ok:
            self.stride = 0

    def frame_offset(self, i: int) -> int:
        return self.data0 + i * self.stride

    def isOpened(self):
        return True

    def read(self):
        tag = self.f.readline(256)
        if not tag.startswith(b"FRAME"):
            return False, None
        buf = self.f.read(self.frame_bytes)
        if len(buf) < self.frame_bytes:
            return False, None
        self.i += 1
        a = np.frombuffer(buf, np.uint8)
        out = np.empty(self.frame_bytes, np.uint8)
        out[:self.ysize] = a[:self.ysize]
        out[self.ysize::2] = a[self.ysize:self.ysize + self.csize]          # U
        out[self.ysize + 1::2] = a[self.ysize + self.csize:]                # V
        return True, out

    def release(self):
        self.f.close()


def write_y4m(path, nv12_frames: np.ndarray, fps: int, size):
    """Test / tooling helper: flat NV12 frames -> a YUV4MPEG2 file (planar 4:2:0)."""
    w, h = size
    ys = w * h
    with open(path, "wb") as f:
        f.write(f"YUV4MPEG2 W{w} H{h} F{int(fps)}:1 Ip A1:1 C420jpeg\n".encode())
        for fr in nv12_frames:
            fr = np.asarray(fr, np.uint8).reshape(-1)
            f.write(b"FRAME\n")
            f.write(fr[:ys].tobytes()); f.write(fr[ys::2].tobytes()); f.write(fr[ys + 1::2].tobytes())


class RawWriter:
    def __init__(self, path, fps, size, pixfmt: str = "bgr"):
        self.path, self.w, self.h, self.n = path, size[0], size[1], 0
        self.f = open(path, "wb")
        self.f.write(_MAGIC + struct.pack("<IIIdI", 0, self.h, self.w, float(fps), 1 if pixfmt == "nv12" else 0))

    def write(self, frame):
        self.f.write(np.ascontiguousarray(frame, np.uint8).tobytes())
        self.n += 1

    def release(self):
        self.f.seek(8)
        self.f.write(struct.pack("<I", self.n))
        self.f.close()


def write_raw(path, frames: np.ndarray, fps: float, pixfmt: str = "bgr", size=None):
    """BGR clip: frames (n, H, W, 3).  NV12 clip: frames (n, H*W*3/2) plus size=(W, H)."""
    w = RawWriter(path, fps, size or (frames.shape[2], frames.shape[1]), pixfmt)
    for fr in frames:
        w.write(fr)
    w.release()


class AviMjpegWriter:
    """Motion-JPEG in an AVI 1.0 container (RIFF 'AVI ': hdrl / movi with '00dc' chunks / idx1), frames encoded with Pillow's
    libjpeg on the writer thread.  The output stage of ``run()`` when OpenCV is absent: a bounded, standard file any player opens
    (a 10-minute 720p clip is ~1.5 GB instead of the ~50 GB of raw frames).  The reference writes H.264 through
    ``cv2.VideoWriter`` (server/model.py:35-36,77); H.264 needs OpenCV -- see INTEGRATION.md.  AVI 1.0 sizes are 32-bit: frames
    past ~3.9 GB are dropped with a warning and the file is still closed properly."""
    LIMIT = 0xE8000000

    BATCH = 32                                       # frames per device encoder call

    def __init__(self, path, fps, size, quality: int = 80, threads: int | None = None, encoder: str = "pillow", device=None,
                 subsampling: int = 2, restart_rows: int = 0, optimize: bool = False):
        """``encoder="device"``: frames are collected into a pinned batch of ``BATCH``, encoded on the GPU ``device`` by
        jpeg.DeviceJpeg (byte-identical files) and appended in order; ``"pillow"``: Pillow's libjpeg on the calling thread.
        ``subsampling`` (0 / 1 / 2 = 4:4:4 / 4:2:2 / 4:2:0), ``restart_rows`` (a restart marker every that many MCU rows) and
        ``optimize`` (per-frame Huffman tables) go to whichever encoder writes: the file does not depend on it."""
        from PIL import Image                        # noqa: F401  (fail at open time, not on the writer thread)
        import collections
        import concurrent.futures
        if encoder not in ("pillow", "device"):
            raise ValueError(f"encoder must be 'pillow' or 'device', not {encoder!r}")
        self.path, self.w, self.h, self.fps, self.quality = path, int(size[0]), int(size[1]), max(1, int(round(fps))), int(quality)
        if subsampling not in (0, 1, 2) or int(restart_rows) < 0:
            raise ValueError(f"subsampling must be 0, 1 or 2 and restart_rows >= 0, not {subsampling!r} / {restart_rows!r}")
        self.subsampling, self.restart_rows, self.optimize = int(subsampling), int(restart_rows), bool(optimize)
        self.encoder = encoder
        self.dev_enc = self.batch = None
        self.pending = 0
        if encoder == "device":
            import torch
            from .jpeg import DeviceJpeg
            self.dev_enc = DeviceJpeg(self.w, self.h, self.quality, device=device, max_frames=self.BATCH, subsampling=self.subsampling,
                                      restart_rows=self.restart_rows, optimize=self.optimize)
            self.batch = torch.empty((self.BATCH, self.h, self.w, 3), dtype=torch.uint8).pin_memory()
            self.batch_np = self.batch.numpy()
            threads = 1
        self.threads = int(os.environ.get("TRUELY_ENCODE_THREADS", "1")) if threads is None else int(threads)
        self.pool = concurrent.futures.ThreadPoolExecutor(self.threads, thread_name_prefix="truely-jpeg") if self.threads > 1 else None
        self.inflight = collections.deque()
        self.f = open(path, "wb")
        self.index: list = []                        # (offset relative to 'movi', size)
        self.n = self.dropped = 0
        self.max_chunk = 0
        self.f.write(self._header(0, 0, 0))
        self.movi_start = self.f.tell() - 4          # position of the 'movi' fourcc
        self.pos = 4                                 # bytes of the movi list written so far ('movi' itself)

    def _header(self, nframes, movi_bytes, max_chunk):
        w, h, fps = self.w, self.h, self.fps
        avih = struct.pack("<IIIIIIIIII4I", 1000000 // fps, max_chunk * fps, 0, 0x10, nframes, 0, 1, max_chunk, w, h, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIIIhhhh", b"vids", b"MJPG", 0, 0, 0, 0, 1, fps, 0, nframes, max_chunk, 0xFFFFFFFF, 0, 0, 0, w, h)
        strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", w * h * 3, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        head = b"LIST" + struct.pack("<I", len(hdrl)) + hdrl
        idx_bytes = 8 + 16 * nframes
        riff_size = 4 + len(head) + 8 + movi_bytes + idx_bytes
        return b"RIFF" + struct.pack("<I", riff_size & 0xFFFFFFFF) + b"AVI " + head + b"LIST" + struct.pack("<I", movi_bytes) + b"movi"

    def _encode(self, frame) -> bytes:
        from PIL import Image
        import io
        a = np.ascontiguousarray(np.asarray(frame, np.uint8)[:, :, ::-1])      # BGR (cap.read()) -> RGB
        buf = io.BytesIO()
        more = {"restart_marker_rows": self.restart_rows} if self.restart_rows else {}
        if self.optimize:
            from PIL import ImageFile
            more["optimize"] = True
            # Pillow hands libjpeg's second pass one buffer of w * h bytes (2 w h from quality 95) and fails on a larger file
            # (noise at 4:4:4); MAXBLOCK is that buffer's lower bound
            ImageFile.MAXBLOCK = max(ImageFile.MAXBLOCK, a.size + 65536)
        Image.fromarray(a, "RGB").save(buf, format="JPEG", quality=self.quality, subsampling=self.subsampling, **more)
        return buf.getvalue()

    def _append(self, data: bytes):
        if self.pos > self.LIMIT:
            if not self.dropped:
                print(f"Warning: {self.path} reached the 4 GB AVI limit; further frames are not written")
            self.dropped += 1
            return
        pad = len(data) & 1
        self.f.write(b"00dc" + struct.pack("<I", len(data)) + data + (b"\0" if pad else b""))
        self.index.append((self.pos, len(data)))
        self.pos += 8 + len(data) + pad
        self.max_chunk = max(self.max_chunk, len(data))
        self.n += 1

    def encode_frame(self, frame) -> bytes:
        """One BGR frame -> the JPEG file this writer's Pillow encoder makes of it (nothing is appended)."""
        return self._encode(frame)

    def append_encoded(self, data: bytes):
        """Append one already encoded JPEG file as the next frame's chunk (tools and tests that build clips from files of their
        own: restart markers, progressive or damaged frames)."""
        self._append(data)

    def _flush_device(self):
        if self.pending:
            for data in self.dev_enc.encode(self.batch[:self.pending]):
                self._append(data)
            self.pending = 0

    def write_device(self, frames):
        """Encode + append a device batch (n, H, W, 3) uint8 BGR of any length, in chunks of ``BATCH``; device encoder only.
        Frames handed to ``write()`` before it come first.  Nothing but the files crosses to the host.  The encoder's work is
        ordered after what is queued on the current stream."""
        if self.dev_enc is None:
            raise ValueError("write_device needs the device encoder (encoder='device')")
        self._flush_device()
        for data in self.dev_enc.encode(frames):
            self._append(data)

    def write(self, frame):
        """Encode + append.  TRUELY_ENCODE_THREADS > 1 encodes on a small pool and appends in call order (at most 2 x threads
        encoded frames wait in memory); measured here Pillow's encoder holds the GIL for most of a frame (x1.3 with four
        threads, ~750 frames/s of 360p per core), so the default is the writer thread alone.  The device encoder copies the frame
        into its pinned batch and encodes every ``BATCH`` frames."""
        if self.dev_enc is not None:
            self.batch_np[self.pending] = frame
            self.pending += 1
            if self.pending == self.BATCH:
                self._flush_device()
            return
        if self.pool is None:
            self._append(self._encode(frame))
            return
        self.inflight.append(self.pool.submit(self._encode, np.array(frame, np.uint8, copy=True)))
        while len(self.inflight) > 2 * self.threads:
            self._append(self.inflight.popleft().result())

    def release(self):
        if self.dev_enc is not None:
            self._flush_device()
            self.dev_enc = None
        while self.inflight:
            self._append(self.inflight.popleft().result())
        if self.pool is not None:
            self.pool.shutdown(wait=True)
        idx = b"".join(b"00dc" + struct.pack("<III", 0x10, off, size) for off, size in self.index)
        self.f.write(b"idx1" + struct.pack("<I", len(idx)) + idx)
        self.f.seek(0)
        self.f.write(self._header(self.n, self.pos, self.max_chunk))
        self.f.close()


class AviMjpegReader:
    """Reads the Motion-JPEG AVI files ``AviMjpegWriter`` (or any encoder: ``ffmpeg -c:v mjpeg out.avi``) produces: walks the
    'movi' list, decodes each '00dc' / '00db' chunk with Pillow -> BGR frames like ``cap.read()``.  The one COMPRESSED input
    this build can decode without OpenCV.  JPEG frames are independent of each other: ``frames`` indexes the chunks,
    ``read_chunk(i)`` reads one by position, and ``run()`` decodes them on the GPU (jpeg.DeviceJpegDecoder, the same bytes as
    Pillow's) -- only the frames it needs; ``decode_host`` is the Pillow decoder for the frames the device does not attempt."""
    pixfmt = "bgr"
    compressed = "mjpeg"                             # frames are independently decodable compressed chunks

    def __init__(self, path):
        self.f = open(path, "rb")
        head = self.f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"AVI ":
            self.f.close()
            raise ValueError("not an AVI file")
        fsize = os.path.getsize(path)
        self.width = self.height = 0
        self.fps_f, self.n, self.codec = 0.0, 0, b""
        self.frames: list = []                       # (file offset, size)
        pos, top = 12, 0
        while pos + 8 <= fsize and top < 65536:      # (a sane file has a handful of top-level chunks: a hostile one cannot make this spin)
            top += 1
            self.f.seek(pos)
            cid, csz = struct.unpack("<4sI", self.f.read(8))
            if cid == b"LIST":
                ltype = self.f.read(4)
                if ltype == b"hdrl":
                    self._parse_hdrl(self.f.read(max(0, min(csz - 4, 1 << 20))))
                elif ltype == b"movi":
                    self._walk_movi(pos + 12, min(pos + 8 + csz, fsize))
            pos += 8 + csz + (csz & 1)
        if self.codec.upper() not in (b"MJPG", b"JPEG") or self.width <= 0 or self.height <= 0:
            self.f.close()
            raise ValueError(f"AVI video codec {self.codec!r}: only Motion-JPEG can be decoded without OpenCV")
        self.n = len(self.frames)
        self.i = 0

    def _parse_hdrl(self, b):
        p = 0
        while p + 8 <= len(b):
            cid, csz = struct.unpack_from("<4sI", b, p)
            if cid == b"LIST":
                p += 12
                continue
            body = b[p + 8:p + 8 + csz]
            if cid == b"strh" and len(body) >= 32 and body[:4] == b"vids":
                self.codec = body[4:8]
                scale, rate = struct.unpack_from("<II", body, 20)
                self.fps_f = rate / scale if scale else 0.0
            elif cid == b"strf" and len(body) >= 20 and not self.width:
                self.width, self.height = struct.unpack_from("<ii", body, 4)
                self.height = abs(self.height)
                if not self.codec.strip(b"\0"):
                    self.codec = body[16:20]
            p += 8 + csz + (csz & 1)

    def _walk_movi(self, pos, end):
        while pos + 8 <= end and len(self.frames) < 4_000_000:      # (37 h at 30 fps: anything longer is a damaged or hostile file)
            self.f.seek(pos)
            cid, csz = struct.unpack("<4sI", self.f.read(8))
            if cid == b"LIST":                       # 'rec ' groups
                pos += 12
                continue
            if cid[2:4] in (b"dc", b"db") and csz > 0 and pos + 8 + csz <= end:
                self.frames.append((pos + 8, csz))
            pos += 8 + csz + (csz & 1)

    def isOpened(self):
        return True

    def read_chunk(self, i: int, dst=None):
        """Frame i's compressed chunk by a positioned read (thread-safe, independent of ``read()``'s position): the bytes, or with
        ``dst`` (a writable buffer of at least the chunk's size) the number of bytes read into it."""
        off, size = self.frames[i]
        fd = self.f.fileno()
        if dst is None:
            return os.pread(fd, size, off)
        mv, got = memoryview(dst)[:size], 0
        while got < size:
            k = os.preadv(fd, [mv[got:]], off + got)
            if k <= 0:
                break
            got += k
        return got

    def decode_host(self, data, i: int):
        """Frame i's chunk -> BGR frame with Pillow, or None (with a warning) for a chunk that cannot be decoded or whose size
        is not the header's: the clip ends there."""
        from PIL import Image
        import io
        try:
            im = Image.open(io.BytesIO(data)).convert("RGB")
        except Exception as e:  # noqa: BLE001 - a damaged frame ends the clip like a failed cap.read() -- but not silently
            print(f"Warning: frame {i} of {self.n} cannot be decoded ({e}): the clip is analysed up to it")
            return None
        a = np.asarray(im, np.uint8)
        if a.shape[0] != self.height or a.shape[1] != self.width:
            print(f"Warning: frame {i} of {self.n} is {a.shape[1]}x{a.shape[0]}, the header says {self.width}x{self.height}: "
                  f"the clip is analysed up to it")
            return None
        return np.ascontiguousarray(a[:, :, ::-1])

    def read(self):
        if self.i >= self.n:
            return False, None
        off, size = self.frames[self.i]
        self.f.seek(off)
        frame = self.decode_host(self.f.read(size), self.i)
        if frame is None:
            return False, None
        self.i += 1
        return True, frame

    def release(self):
        self.f.close()


class AsyncWriter:
    """Decoupled annotated-output stage.  ``put(frame, note)`` hands a frame (and, for sampled frames that were compared with
    their predecessor, ``note = (frame_index, rect, flagged)``) to a worker thread that draws (annotate.py) and encodes;
    ``put_batch(frames, notes)`` hands over a whole device batch, drawn on (``trl_draw``) and encoded where it lies.
    ``annotate=False`` skips the drawing, ``sink=None`` skips the stage altogether (benchmarks); the queue is bounded -- by
    ``depth`` FRAMES, whether they arrive one by one or in batches -- so a slow encoder applies back-pressure instead of
    growing memory."""

    def __init__(self, sink, annotate: bool = True, depth: int = 64):
        import collections
        self.sink, self.annotate, self.frames = sink, annotate, 0
        self.err = None
        self.depth, self.queued = max(1, int(depth)), 0   # frames the queue may hold / holds
        self.items = collections.deque()                  # (item, frames in it)
        self.cv = threading.Condition()
        self.th = threading.Thread(target=self._work, name="truely-writer", daemon=True) if sink is not None else None
        if self.th:
            self.th.start()

    def _push(self, item, n: int):
        with self.cv:
            while self.queued and self.queued + n > self.depth:      # (a batch larger than the whole queue goes in alone)
                self.cv.wait()
            self.items.append((item, n))
            self.queued += n
            self.cv.notify_all()

    def _pop(self):
        with self.cv:
            while not self.items:
                self.cv.wait()
            item, n = self.items.popleft()
            self.queued -= n
            self.cv.notify_all()
        return item

    def _work(self):
        while True:
            item = self._pop()
            if item is None:
                return
            if self.err is not None:
                continue                                  # keep draining so the producer never blocks on a dead stage
            try:
                if len(item) == 3:
                    self._write_batch(*item)
                    continue
                frame, note = item
                if note is not None and self.annotate:
                    _annotate.annotate(frame, *note)
                self.sink.write(frame)
            except BaseException as e:                    # surfaced by close()
                self.err = e

    def _write_batch(self, frames, notes, ready):
        import torch
        stream = self.sink.dev_enc.stream                 # drawing and encoding are ordered on the encoder's stream
        with torch.cuda.stream(stream):
            if ready is not None:
                stream.wait_event(ready)                  # the producer has finished with these frames
            if notes and self.annotate:
                _annotate.annotate_device(frames, notes, stream=stream)
            self.sink.write_device(frames)

    def put(self, frame, note=None):
        self.frames += 1
        if self.th:
            self._push((frame, note), 1)

    def put_batch(self, frames, notes=(), ready=None):
        """A device batch (n, H, W, 3) for a sink with ``write_device``; notes = (row, frame_index, rect, flagged) for the rows to
        annotate; ``ready``: an event recorded once the producer's work on these frames was queued (the writer's stream waits
        for it).  The frames are drawn on in place: they are the writer's from here on."""
        n = int(frames.shape[0])
        self.frames += n
        if self.th and n:
            self._push((frames, list(notes), ready), n)

    def close(self):
        if self.th:
            self._push(None, 0)
            self.th.join()
        if self.sink is not None:
            self.sink.release()
        if self.err is not None:
            raise self.err


def open_reader(path):
    """Returns (reader, fps:int, width, height) or None if the file cannot be opened (model.py:23-29)."""
    with open(path, "rb") as f:
        magic = f.read(8)
    if magic == _MAGIC:
        r = RawReader(path)
        return r, int(r.fps_f), r.width, r.height
    if magic == b"YUV4MPEG":
        try:
            r = Y4MReader(path)
        except ValueError as e:
            print(f"Error: {e}")
            return None
        return r, int(r.fps_f), r.width, r.height
    if magic[:4] == b"RIFF" and cv2 is None:
        try:
            r = AviMjpegReader(path)
        except (ValueError, struct.error, OSError) as e:
            print(f"Error: {e}")
            return None
        return r, int(r.fps_f), r.width, r.height
    if cv2 is not None:  # pragma: no cover
        cap = cv2.VideoCapture(path)
        if not cap.isOpened():
            return None
        return cap, int(cap.get(cv2.CAP_PROP_FPS)), int(cap.get(cv2.CAP_PROP_FRAME_WIDTH)), int(cap.get(cv2.CAP_PROP_FRAME_HEIGHT))
    return None


def describe(path) -> str:
    """One line about a clip this build cannot decode (no OpenCV): what the container says it is."""
    from . import mp4probe
    try:
        i = mp4probe.probe(path)
    except Exception:  # noqa: BLE001 - a damaged container is simply "unknown"
        i = None
    if i is None:
        return "unknown container"
    prof = {66: "Baseline", 77: "Main", 88: "Extended", 100: "High"}.get(i.profile_idc, str(i.profile_idc))
    return (f"H.264 {prof}@L{i.level_idc / 10:.1f} {i.width}x{i.height}, {i.fps:.3f} fps, {i.frame_count} frames"
            f"{' (fragmented mp4)' if i.fragmented else ''}: decoding needs opencv-python (cv2.VideoCapture), or hand run() decoder output as an NV12 TRLV clip")


def open_writer(path, fps, size, like_raw: bool = False, device=None):
    """The sink of ``run()``'s annotated output (server/model.py:35-36).  ``*.trlv``: the raw container (tests, byte-exact
    read-back).  Otherwise OpenCV's H.264 writer when importable, like the reference; without OpenCV a Motion-JPEG AVI stream
    (bounded size, plays anywhere -- but it is MJPEG/AVI whatever the file is called: H.264 needs OpenCV), encoded on the GPU
    ``device`` when one is given (byte-identical to Pillow's encoder, which is used otherwise)."""
    if str(path).lower().endswith(".trlv"):
        return RawWriter(path, fps, size)
    if cv2 is not None:  # pragma: no cover
        return cv2.VideoWriter(path, cv2.VideoWriter_fourcc(*"H264"), fps, size)
    if not str(path).lower().endswith(".avi"):       # the server names the file *.mp4 and serves it as video/mp4: say what it really is
        print(f"Note: OpenCV is not installed, {os.path.basename(str(path))} is written as Motion-JPEG in an AVI container (not H.264)")
    opts = jpeg_options_from_env()
    if device is not None:
        return AviMjpegWriter(path, fps, size, encoder="device", device=device, **opts)
    return AviMjpegWriter(path, fps, size, **opts)


def jpeg_options_from_env() -> dict:
    """``AviMjpegWriter``'s JPEG options from the environment: ``TRUELY_JPEG_SUBSAMPLING`` (``420``, ``422``, ``444``),
    ``TRUELY_JPEG_RESTART_ROWS`` (MCU rows per restart interval) and ``TRUELY_JPEG_OPTIMIZE`` (``1``: per-frame Huffman tables).
    Unset (or empty) variables leave the writer's defaults, and with them every byte of the file, as they are."""
    opts = {}
    sub = os.environ.get("TRUELY_JPEG_SUBSAMPLING", "")
    if sub:
        if sub not in ("420", "422", "444"):
            raise ValueError(f"TRUELY_JPEG_SUBSAMPLING must be 420, 422 or 444, not {sub!r}")
        opts["subsampling"] = {"444": 0, "422": 1, "420": 2}[sub]
    rows = os.environ.get("TRUELY_JPEG_RESTART_ROWS", "")
    if rows:
        if not rows.isdigit():
            raise ValueError(f"TRUELY_JPEG_RESTART_ROWS must be a number of MCU rows, not {rows!r}")
        opts["restart_rows"] = int(rows)
    opt = os.environ.get("TRUELY_JPEG_OPTIMIZE", "")
    if opt:
        if opt not in ("0", "1"):
            raise ValueError(f"TRUELY_JPEG_OPTIMIZE must be 0 or 1, not {opt!r}")
        opts["optimize"] = opt == "1"
    return opts


def encodes_on_device(path, device) -> bool:
    """Whether ``open_writer(path, ..., device=device)`` gives a sink that encodes on the GPU (``AviMjpegWriter.write_device``)."""
    return device is not None and cv2 is None and not str(path).lower().endswith(".trlv")


def _on_device(frame):
    return hasattr(frame, "is_cuda") and frame.is_cuda


def draw_box(frame, x0, y0, x1, y1, color, thickness=2):
    """A rectangle on a host frame (H, W, 3) -- or, in place, on a frame that lies on a GPU (a uint8 tensor: ``trl_draw``)."""
    if _on_device(frame):
        dl = _annotate.DrawList()
        dl.rectangle(0, (x0, y0), (x1, y1), color, thickness)
        _annotate.draw_device(frame.unsqueeze(0), *dl.arrays())
        return
    _annotate.rectangle(frame, (x0, y0), (x1, y1), color, thickness)


def put_text(frame, text, org, scale, color, thickness):
    """Text on a host frame -- or, in place, on a frame that lies on a GPU (this module's own glyphs)."""
    if _on_device(frame):
        dl = _annotate.DrawList()
        dl.put_text(0, text, org, scale, color, thickness)
        _annotate.draw_device(frame.unsqueeze(0), *dl.arrays())
        return
    _annotate.put_text(frame, text, org, scale, color, thickness)
