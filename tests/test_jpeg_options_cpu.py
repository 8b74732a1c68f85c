"""CPU tests of the Motion-JPEG encoder's options (no GPU): 4:4:4 / 4:2:2 / 4:2:0, restart intervals and optimised Huffman tables.

``jpeg_options_ref.encode`` restates the rules in numpy; these tests pin it to Pillow's bytes over a grid of sizes, samplings,
qualities, content and intervals, pin ``trl_jpeg_header_ex`` (host-only C ABI) to Pillow's headers, the exported table builder
(``trl_jpeg_optimal_table``, the function the device runs per frame and table) to the restatement's over seeded histograms -- also
in a stand-alone program under the address and undefined-behaviour sanitizers --, and ``AviMjpegWriter``'s options to Pillow."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_options_ref as R
from test_jpeg_cpu import make_frame
from truely_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.dirname(_lib.LIB_PATH) + "/csrc"

SIZES = [(1, 1), (7, 5), (8, 8), (9, 9), (16, 16), (17, 15), (33, 31), (64, 48), (100, 75), (320, 180)]     # (W, H)
SAMPLINGS = [0, 1, 2]
QUALITIES = [1, 50, 80, 100]
KINDS = ["noise", "gradient", "constant", "saturated"]


def mcus(W, H, s):
    _, _, mx, my = R.geometry(H, W, s)
    return mx, my


def interval_variants(W, H, s):
    """(restart_rows, restart_blocks) worth a case at this size: none, a row, one MCU, three MCUs (crossing rows where a row is
    no multiple of 3), exactly the MCU count, and beyond it (a DRI segment and no marker)."""
    mx, my = mcus(W, H, s)
    return [(0, 0), (1, 0), (0, 1), (0, 3), (0, mx * my), (0, mx * my + 5), (2, 7)]


def _table():
    """The grid: every size x sampling x quality x content x optimize, each with one interval variant; the variants cycle with a
    period (7) coprime to every axis, so each meets every sampling, quality, content kind and both optimize settings."""
    out, k = [], 0
    for (W, H) in SIZES:
        for s in SAMPLINGS:
            for q in QUALITIES:
                for kind in KINDS:
                    for opt in (False, True):
                        rr, rb = interval_variants(W, H, s)[k % 7]
                        out.append((W, H, s, q, kind, opt, rr, rb))
                        k += 1
    return out


TABLE = _table()
# frames of 4 x 2 MCUs at each sampling: an interval of 3 MCUs crosses the MCU rows and divides neither the row nor the frame
FOUR_BY_TWO = {0: (32, 16), 1: (64, 16), 2: (64, 32)}


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("s", SAMPLINGS)
def test_reference_rules_equal_pillow(W, H, s):
    for (w, h, ss, q, kind, opt, rr, rb) in TABLE:
        if (w, h, ss) != (W, H, s):
            continue
        frame = make_frame(kind, H, W)
        assert R.encode(frame, q, s, rr, rb, opt) == R.pillow(frame, q, s, rr, rb, opt), (q, kind, opt, rr, rb)


@pytest.mark.parametrize("s", SAMPLINGS)
@pytest.mark.parametrize("opt", [False, True])
def test_every_interval_kind_at_every_sampling(s, opt):
    """Each interval kind the grid cycles through, here at every sampling and optimize setting on one ragged size, and the
    interval of 3 on 4 MCUs per row."""
    W, H = 33, 31
    for kind in ("noise", "saturated"):
        frame = make_frame(kind, H, W)
        for rr, rb in interval_variants(W, H, s):
            assert R.encode(frame, 80, s, rr, rb, opt) == R.pillow(frame, 80, s, rr, rb, opt), (kind, rr, rb)
    W, H = FOUR_BY_TWO[s]
    assert mcus(W, H, s) == (4, 2)
    frame = make_frame("noise", H, W)
    info = {}
    assert R.encode(frame, 80, s, 0, 3, opt, info) == R.pillow(frame, 80, s, 0, 3, opt)
    assert info["intervals"] == 3                           # 3 + 3 + 2 MCUs


def test_table_reaches_every_interval_kind_and_edge():
    """What the grid is there for is in it, held by assertion: every interval kind at every sampling with and without optimize;
    a frame of more than eight intervals (RST7 followed by RST0); interval padding that comes out as 0xFF and is stuffed directly
    in front of a marker; an optimize case whose unadjusted code lengths exceed 16, so libjpeg's limiting step runs."""
    for s in SAMPLINGS:
        for opt in (False, True):
            kinds = set()
            for (W, H, ss, q, kind, o, rr, rb) in TABLE:
                if (ss, o) != (s, opt):
                    continue
                mx, my = mcus(W, H, s)
                n = mx * my
                kinds.add("none" if (rr, rb) == (0, 0) else "rows" if rr else "one" if rb == 1 else "three" if rb == 3
                          else "all" if rb == n else "beyond")
                if rr == 0 and rb == 1 and n > 8:
                    kinds.add("rst7-rst0")
            assert kinds == {"none", "rows", "one", "three", "all", "beyond", "rst7-rst0"}, (s, opt, kinds)
    stuffed = limited = wrapped = 0
    for (W, H, s, q, kind, opt, rr, rb) in TABLE:
        if (W, H) != (320, 180) or q != 100 or kind not in ("noise", "saturated") or (rr, rb) == (0, 0):
            continue
        info = {}
        data = R.encode(make_frame(kind, H, W), q, s, rr, rb, opt, info)
        stuffed += info["stuffed_pad"] > 0 and any(b"\xff\x00" + bytes([0xFF, 0xD0 + k]) in data for k in range(8))
        limited += opt and info["maxlen"] > 16
        wrapped += info["intervals"] > 9 and b"\xff\xd7" in data
    assert stuffed >= 1 and limited >= 1 and wrapped >= 1, (stuffed, limited, wrapped)


# ---- trl_jpeg_header_ex -------------------------------------------------------------------------------------------------------
def _header_ex(H, W, q, s, rr, rb, opt=0, cap=1024):
    lib = _lib.load()
    o = _lib.TrlJpegOptions(q, s, rr, rb, opt)
    buf = (ctypes.c_uint8 * max(cap, 1))()
    n = ctypes.c_int(0)
    st = lib.trl_jpeg_header_ex(H, W, ctypes.byref(o), buf if cap else None, cap, ctypes.byref(n))
    return st, bytes(buf[:n.value]) if st == 0 else b"", n.value


@pytest.mark.parametrize("W,H", SIZES)
def test_trl_jpeg_header_ex_equals_pillow(W, H):
    frame = make_frame("gradient", H, W)
    for s in SAMPLINGS:
        for q in QUALITIES:
            for rr, rb in interval_variants(W, H, s) + [(1, 3), (3, 1)]:      # (both given: the rows win, as in libjpeg)
                st, hdr, _ = _header_ex(H, W, q, s, rr, rb)
                assert st == 0
                dri = R.restart_interval(H, W, s, rr, rb)
                assert hdr == R.header(H, W, q, s, dri)
                data = R.pillow(frame, q, s, rr, rb)
                assert data[:len(hdr)] == hdr, (s, q, rr, rb)


def test_header_ex_defaults_are_trl_jpeg_header():
    lib = _lib.load()
    for (W, H) in SIZES + [(1280, 720)]:
        for q in (0, 1, 80, 100, 101):
            buf = (ctypes.c_uint8 * 1024)()
            n = ctypes.c_int(0)
            assert lib.trl_jpeg_header(H, W, q, buf, 1024, ctypes.byref(n)) == 0
            assert _header_ex(H, W, q, 2, 0, 0)[1] == bytes(buf[:n.value])


def test_header_ex_interval_clamp_is_libjpegs():
    """rows x MCUs-per-row above 65535 becomes 65535 (tried on Pillow: an 80-row 4:4:4 frame of 8187 MCUs per row, 9 rows)."""
    H, W = 80, 65496
    st, hdr, _ = _header_ex(H, W, 80, 0, 9, 0)
    assert st == 0 and hdr[-20:-16] == b"\xff\xdd\x00\x04" and hdr[-16:-14] == b"\xff\xff"
    data = R.pillow(np.zeros((H, W, 3), np.uint8), 80, 0, 9, 0)
    assert data[:len(hdr)] == hdr


def test_header_ex_optimize_is_the_standard_header_and_an_upper_bound():
    for (W, H) in ((64, 48), (100, 75)):
        for s in SAMPLINGS:
            st, hdr, n = _header_ex(H, W, 100, s, 1, 0, opt=1)
            assert st == 0 and hdr == _header_ex(H, W, 100, s, 1, 0)[1]
            for kind in KINDS:
                data = R.pillow(make_frame(kind, H, W), 100, s, 1, 0, True)
                assert data.index(b"\xff\xda") + 14 <= n


def test_header_ex_refusals_and_capacity():
    lib = _lib.load()
    st, _, need = _header_ex(360, 640, 80, 0, 1, 0, cap=10)
    assert st == -4 and need == len(R.header(360, 640, 80, 0, 80))
    st, _, need2 = _header_ex(360, 640, 80, 0, 1, 0, cap=0)
    assert st == -4 and need2 == need
    assert _header_ex(360, 640, 80, 0, 1, 0, cap=need)[0] == 0
    for s, rr, rb in ((-1, 0, 0), (3, 0, 0), (2, -1, 0), (2, 0, -1), (0, 0, 65536)):
        st, _, _ = _header_ex(48, 64, 80, s, rr, rb)
        assert st == -1 and b"trl_jpeg_header_ex" in lib.trl_last_error(), (s, rr, rb)
    for H, W in ((0, 8), (8, 0), (65536, 8)):
        assert _header_ex(H, W, 80, 0, 0, 0)[0] == -1
    n = ctypes.c_int(0)
    assert lib.trl_jpeg_header_ex(48, 64, None, None, 0, ctypes.byref(n)) == -1
    # optimize on a frame whose histograms libjpeg itself could fail on (a code deeper than 32 bits): refused
    assert _header_ex(4000, 4000, 80, 2, 0, 0, opt=1)[0] == -1
    assert _header_ex(4000, 4000, 80, 2, 0, 0, opt=0)[0] == 0
    assert _header_ex(1080, 1920, 80, 0, 0, 0, opt=1)[0] == 0


def test_jpeg_option_symbols_exported():
    names = {"trl_jpeg_create_ex", "trl_jpeg_header_ex", "trl_jpeg_optimal_table"}
    hdr = open(os.path.join(ROOT, "include", "truely_hip.h")).read()
    assert names <= set(re.findall(r"\b(trl_[a-z0-9_]+)\s*\(", hdr)) and "trl_jpeg_options" in hdr
    assert names <= set(_lib.EXPORTS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert names <= set(re.findall(r"\bT (trl_[a-z0-9_]+)", out))
    assert b"getenv" not in subprocess.check_output(["nm", "-D", "--undefined-only", _lib.LIB_PATH])   # options come by argument


# ---- the table builder ----------------------------------------------------------------------------------------------------------
def histograms():
    """Seeded histograms, 256 counts each: the named families, then 10,000 random ones (mostly as sparse as a frame's, some
    dense, with flat, wide and exponentially spread counts)."""
    rng = np.random.default_rng(20240607)
    out = []

    def put(idx, counts):
        h = np.zeros(256, np.uint32)
        h[np.asarray(idx)] = counts
        out.append(h)
    for s in (0, 5, 255):
        put([s], 1)                                         # a single symbol: one 1-bit code (a constant frame's 20-byte DHT)
        put([s], 1_000_000)
    put([3, 200], [1, 1])                                   # two symbols
    put([0, 255], [7, 900])
    for n in (2, 3, 4, 11, 12, 64, 162, 255, 256):          # all equal
        put(np.arange(n), 1)
        put(np.arange(256 - n, 256), 1000)
    for n in (18, 20, 24, 30):                              # geometric: the unadjusted lengths reach n - 1 > 16
        put(np.arange(n), 2 ** np.arange(n))
        put(np.arange(n)[::-1] * 8, 2 ** np.arange(n))
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    put(np.arange(30), fib[:30])                            # Fibonacci counts: the deepest tree for the fewest symbols
    put(np.arange(256), np.arange(1, 257))                  # all 256 symbols
    put(np.arange(256), 1)
    put(np.arange(256), (np.arange(256) % 7 + 1) ** 6)
    put(np.arange(256), np.minimum(2 ** (np.arange(256) // 9), 2 ** 20))
    for k in range(10_000):
        n = int(rng.integers(1, 41)) if k % 10 else int(rng.integers(41, 257))
        idx = rng.choice(256, n, replace=False)
        mode = k % 4
        if mode == 0:
            c = rng.integers(1, 4, n)                       # many ties
        elif mode == 1:
            c = rng.integers(1, 100_000, n)
        elif mode == 2:
            c = 2 ** rng.integers(0, 30, n)                 # wide spread, ties among powers of two
        else:
            c = np.maximum(1, (rng.exponential(1.0, n) ** 4 * 50).astype(np.int64))
        put(idx, np.minimum(c, 10 ** 9 // (2 * n)))           # (libjpeg never merges counts above 10^9: a frame has fewer symbols)
    return out


@pytest.fixture(scope="module")
def expected_tables():
    hs = histograms()
    return hs, [R.optimal_table(h) for h in hs]


def test_histogram_families(expected_tables):
    hs, exp = expected_tables
    assert len(hs) >= 10_000
    longest = [m for _, _, m in exp]
    assert max(longest) > 16 and sum(m > 16 for m in longest) > 100      # the limiting step runs, and often
    assert any(len(v) == 256 for _, v, _ in exp) and any(len(v) == 1 for _, v, _ in exp)
    bits, vals, _ = exp[0]
    assert bits == [1] + [0] * 15 and vals == [0]           # a single symbol: one 1-bit code


def test_exported_builder_equals_restatement(expected_tables):
    hs, exp = expected_tables
    lib = _lib.load()
    bits = (ctypes.c_uint8 * 16)()
    vals = (ctypes.c_uint8 * 256)()
    n, m = ctypes.c_int(0), ctypes.c_int(0)
    for h, (eb, ev, em) in zip(hs, exp):
        assert lib.trl_jpeg_optimal_table(h.ctypes.data_as(ctypes.c_void_p), bits, vals, ctypes.byref(n), ctypes.byref(m)) == 0
        assert (list(bits), list(vals[:n.value]), m.value) == (eb, ev, em), h.nonzero()
    assert lib.trl_jpeg_optimal_table(None, bits, vals, ctypes.byref(n), None) == -1


def test_exported_builder_on_an_empty_histogram():
    lib = _lib.load()
    bits = (ctypes.c_uint8 * 16)(*([9] * 16))
    vals = (ctypes.c_uint8 * 256)()
    n = ctypes.c_int(-1)
    h = np.zeros(256, np.uint32)
    assert lib.trl_jpeg_optimal_table(h.ctypes.data_as(ctypes.c_void_p), bits, vals, ctypes.byref(n), None) == 0
    assert n.value == 0 and list(bits) == [0] * 16


@pytest.fixture(scope="module")
def hufftab_program(tmp_path_factory):
    """tests/jpeg_hufftab_main.cpp built for the host with the address and undefined-behaviour sanitizers (without them where
    their runtime is not installed: the program then still checks every table)."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("jpeg_hufftab") / "jpeg_hufftab_main")
    base = [cxx, "-O1", "-g", "-std=c++17", "-I", CSRC, os.path.join(ROOT, "tests", "jpeg_hufftab_main.cpp"), "-o", out]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(base + san, capture_output=True, text=True)
    if r.returncode != 0:
        subprocess.run(base, check=True)
    return out


def test_builder_stand_alone_under_sanitizers(hufftab_program, expected_tables, tmp_path):
    hs, exp = expected_tables
    path = str(tmp_path / "hist.bin")
    np.stack(hs).astype("<u4").tofile(path)
    r = subprocess.run([hufftab_program, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(hs)
    for line, (eb, ev, em) in zip(lines, exp):
        m, b, *v = line.split(" ")
        assert (int(m), list(bytes.fromhex(b)), list(bytes.fromhex(v[0] if v else ""))) == (em, eb, ev)


# ---- AviMjpegWriter and open_writer ---------------------------------------------------------------------------------------------
def _avi_frames(path):
    from truely_amd import video_io
    r = video_io.AviMjpegReader(path)
    out = []
    for off, size in r.frames:
        r.f.seek(off)
        out.append(r.f.read(size))
    r.release()
    return out


@pytest.mark.parametrize("s,rows,opt", [(0, 0, False), (1, 1, False), (2, 2, True), (0, 1, True), (2, 0, False)])
def test_writer_options_with_pillow_encoder(tmp_path, s, rows, opt):
    from truely_amd import video_io
    frames = [make_frame(k, 75, 100, seed=3) for k in KINDS]
    w = video_io.AviMjpegWriter(str(tmp_path / "o.avi"), 30, (100, 75), quality=80, subsampling=s, restart_rows=rows, optimize=opt)
    for f in frames:
        w.write(f)
    assert w.encode_frame(frames[0]) == R.pillow(frames[0], 80, s, rows, 0, opt)
    w.release()
    assert _avi_frames(str(tmp_path / "o.avi")) == [R.pillow(f, 80, s, rows, 0, opt) for f in frames]


def test_writer_refuses_bad_options(tmp_path):
    from truely_amd import video_io
    for kw in ({"subsampling": 3}, {"subsampling": -1}, {"restart_rows": -1}):
        with pytest.raises(ValueError):
            video_io.AviMjpegWriter(str(tmp_path / "p.avi"), 30, (64, 48), **kw)


def test_open_writer_reads_the_environment(tmp_path, monkeypatch):
    from truely_amd import video_io
    if video_io.cv2 is not None:
        pytest.skip("OpenCV present: open_writer gives cv2's H.264 writer")
    frame = make_frame("noise", 48, 64)
    for v in ("TRUELY_JPEG_SUBSAMPLING", "TRUELY_JPEG_RESTART_ROWS", "TRUELY_JPEG_OPTIMIZE"):
        monkeypatch.delenv(v, raising=False)
    assert video_io.jpeg_options_from_env() == {}
    monkeypatch.setenv("TRUELY_JPEG_SUBSAMPLING", "444")
    monkeypatch.setenv("TRUELY_JPEG_RESTART_ROWS", "1")
    monkeypatch.setenv("TRUELY_JPEG_OPTIMIZE", "1")
    assert video_io.jpeg_options_from_env() == {"subsampling": 0, "restart_rows": 1, "optimize": True}
    w = video_io.open_writer(str(tmp_path / "e.avi"), 30, (64, 48))
    w.write(frame)
    w.release()
    assert _avi_frames(str(tmp_path / "e.avi")) == [R.pillow(frame, 80, 0, 1, 0, True)]
    monkeypatch.setenv("TRUELY_JPEG_SUBSAMPLING", "422")
    monkeypatch.setenv("TRUELY_JPEG_OPTIMIZE", "0")
    assert video_io.jpeg_options_from_env() == {"subsampling": 1, "restart_rows": 1, "optimize": False}
    for var, bad in (("TRUELY_JPEG_SUBSAMPLING", "411"), ("TRUELY_JPEG_RESTART_ROWS", "-1"), ("TRUELY_JPEG_OPTIMIZE", "yes")):
        monkeypatch.setenv(var, bad)
        with pytest.raises(ValueError):
            video_io.jpeg_options_from_env()
        monkeypatch.delenv(var)
