"""CPU tests of the Motion-JPEG encoder's rules (no GPU).

``encode_reference`` restates, in numpy, what ``Image.save(format="JPEG", quality=q, subsampling=2)`` does through libjpeg-turbo's
baseline path: jccolor's 16-bit colour conversion, edge replication and h2v2 downsampling, the islow integer FDCT, quantisation by
division, libjpeg's dummy blocks, Annex K Huffman coding with 0xFF stuffing, and Pillow's marker sequence.  The device encoder
(csrc/trl_jpeg.hip) implements the same rules; these tests pin the rules to Pillow's bytes, and ``trl_jpeg_header`` (host-only
C ABI) to Pillow's headers, over sizes, qualities and content chosen to reach every edge case."""
import ctypes
import io
import os
import re
import subprocess

import numpy as np
import pytest

from truely_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the rules ----------------------------------------------------------------------------------------------------------------
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
                   47, 55, 62, 63])          # zigzag position -> natural index
STD_LUMA_Q = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29,
                       51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121,
                       120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
STD_CHROMA_Q = np.full(64, 99)
STD_CHROMA_Q[[0, 1, 2, 3, 8, 9, 10, 11, 16, 17, 18, 24, 25]] = [17, 18, 24, 47, 18, 21, 26, 66, 24, 26, 56, 47, 66]
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43444546"
    "4748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8"
    "b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"))
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445"
    "464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6"
    "b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))


def quant_tables(quality):
    q = min(100, max(1, int(quality)))
    s = 5000 // q if q < 50 else 200 - 2 * q
    return [np.clip((t * s + 50) // 100, 1, 255) for t in (STD_LUMA_Q, STD_CHROMA_Q)]


def huff_codes(table):
    bits, vals = table
    code, out = 0, {}
    k = 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            k += 1
            code += 1
        code <<= 1
    return out


def jpeg_header(H, W, quality):
    """Pillow's marker sequence up to and including SOS."""
    def seg(marker, body):
        return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body
    ql, qc = quant_tables(quality)
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += seg(0xDB, bytes([0]) + bytes(ql[ZIGZAG].astype(np.uint8))) + seg(0xDB, bytes([1]) + bytes(qc[ZIGZAG].astype(np.uint8)))
    out += seg(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for cls_id, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += seg(0xC4, bytes([cls_id]) + bytes(bits) + bytes(vals))
    return out + seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def _fix(x):
    return int(x * 65536 + 0.5)


def color_convert(rgb):
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (_fix(0.299) * r + _fix(0.587) * g + _fix(0.114) * b + (1 << 15)) >> 16
    cb = (-_fix(0.16874) * r - _fix(0.33126) * g + _fix(0.5) * b + (128 << 16) + (1 << 15) - 1) >> 16
    cr = (_fix(0.5) * r - _fix(0.41869) * g - _fix(0.08131) * b + (128 << 16) + (1 << 15) - 1) >> 16
    return y, cb, cr


def _pad_to(a, rows, cols):
    return np.pad(a, ((0, rows - a.shape[0]), (0, cols - a.shape[1])), mode="edge")


def _blocks(plane):
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(h // 8, w // 8, 64)


def fdct_islow(blocks):
    """jfdctint islow on (..., 64) centred samples: rows, then columns.  Output is scaled by 8 like libjpeg's."""
    CB, P1 = 13, 2
    F = dict(f0298=2446, f0390=3196, f0541=4433, f0765=6270, f0899=7373, f1175=9633, f1501=12299, f1847=15137, f1961=16069,
             f2053=16819, f2562=20995, f3072=25172)

    def desc(x, n):
        return (x + (1 << (n - 1))) >> n

    def pass1d(d, first):
        t0, t7 = d[0] + d[7], d[0] - d[7]
        t1, t6 = d[1] + d[6], d[1] - d[6]
        t2, t5 = d[2] + d[5], d[2] - d[5]
        t3, t4 = d[3] + d[4], d[3] - d[4]
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        sh = CB - P1 if first else CB + P1
        o = [None] * 8
        o[0] = (t10 + t11) << P1 if first else desc(t10 + t11, P1)
        o[4] = (t10 - t11) << P1 if first else desc(t10 - t11, P1)
        z1 = (t12 + t13) * F["f0541"]
        o[2] = desc(z1 + t13 * F["f0765"], sh)
        o[6] = desc(z1 - t12 * F["f1847"], sh)
        z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
        z5 = (z3 + z4) * F["f1175"]
        t4, t5, t6, t7 = t4 * F["f0298"], t5 * F["f2053"], t6 * F["f3072"], t7 * F["f1501"]
        z1, z2 = -z1 * F["f0899"], -z2 * F["f2562"]
        z3, z4 = -z3 * F["f1961"] + z5, -z4 * F["f0390"] + z5
        o[7] = desc(t4 + z1 + z3, sh)
        o[5] = desc(t5 + z2 + z4, sh)
        o[3] = desc(t6 + z2 + z3, sh)
        o[1] = desc(t7 + z1 + z4, sh)
        return o

    b = blocks.astype(np.int64).reshape(blocks.shape[:-1] + (8, 8))
    rows = pass1d([b[..., :, i] for i in range(8)], True)
    b = np.stack(rows, axis=-1)
    cols = pass1d([b[..., i, :] for i in range(8)], False)
    return np.stack(cols, axis=-2).reshape(blocks.shape)


def quantize(coef, qt):
    d = (qt.astype(np.int64) * 8)
    a = (np.abs(coef) + (d >> 1)) // d
    return np.where(coef < 0, -a, a)


def encode_reference(bgr, quality):
    """A complete baseline 4:2:0 JPEG file of one BGR frame, byte for byte what Pillow writes for the RGB frame."""
    H, W = bgr.shape[:2]
    y, cb, cr = color_convert(np.asarray(bgr)[:, :, ::-1])
    ql, qc = quant_tables(quality)
    bw, bh = -(-W // 8), -(-H // 8)                     # Y blocks with real samples
    mx, my = -(-W // 16), -(-H // 16)                   # MCUs
    cw, ch = -(-W // 2), -(-H // 2)
    Y = _pad_to(y, bh * 8, bw * 8)
    chroma = []
    for p in (cb, cr):
        full = _pad_to(p, 2 * ch, 16 * mx)
        s = full[0::2, 0::2] + full[0::2, 1::2] + full[1::2, 0::2] + full[1::2, 1::2]
        bias = np.where(np.arange(s.shape[1]) & 1, 2, 1)
        chroma.append(_pad_to((s + bias) >> 2, 8 * my, 8 * mx))
    qY = quantize(fdct_islow(_blocks(Y) - 128), ql)                         # (bh, bw, 64) natural order
    qC = [quantize(fdct_islow(_blocks(c) - 128), qc) for c in chroma]       # (my, mx, 64)
    # the Y block grid of whole MCUs, with libjpeg's dummy blocks at the right and bottom
    full = np.zeros((2 * my, 2 * mx, 64), np.int64)
    full[:bh, :bw] = qY
    if bw & 1:                                          # right dummy: DC of its left neighbour
        full[:, bw, 0] = full[:, bw - 1, 0]
    if bh & 1:                                          # bottom dummy: DC of the MCU's Y01
        full[bh, :, 0] = full[bh - 1, 1::2, 0].repeat(2)
    zz = [huff_codes(t) for t in (DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA)]
    pieces = []                                         # (code, length)

    def block(coefs, dc_t, ac_t, pred):
        z = coefs[ZIGZAG]
        diff = int(z[0]) - pred
        n = abs(diff).bit_length()
        pieces.append(dc_t[n])
        if n:
            pieces.append(((diff if diff >= 0 else diff - 1) & ((1 << n) - 1), n))
        r = 0
        for k in range(1, 64):
            v = int(z[k])
            if v == 0:
                r += 1
                continue
            while r > 15:
                pieces.append(ac_t[0xF0])
                r -= 16
            n = abs(v).bit_length()
            pieces.append(ac_t[(r << 4) | n])
            pieces.append(((v if v >= 0 else v - 1) & ((1 << n) - 1), n))
            r = 0
        if r:
            pieces.append(ac_t[0x00])
        return int(z[0])

    pY = pCb = pCr = 0
    for j in range(my):
        for i in range(mx):
            for by, bx in ((0, 0), (0, 1), (1, 0), (1, 1)):
                pY = block(full[2 * j + by, 2 * i + bx], zz[0], zz[1], pY)
            pCb = block(qC[0][j, i], zz[2], zz[3], pCb)
            pCr = block(qC[1][j, i], zz[2], zz[3], pCr)
    bits = "".join(format(code, f"0{length}b") for code, length in pieces)
    bits += "1" * (-len(bits) % 8)                      # pad the last byte with 1-bits
    data = int(bits, 2).to_bytes(len(bits) // 8, "big") if bits else b""
    return jpeg_header(H, W, quality) + data.replace(b"\xff", b"\xff\x00") + b"\xff\xd9"


def pillow_jpeg(bgr, quality):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1]), "RGB").save(buf, format="JPEG", quality=quality, subsampling=2)
    return buf.getvalue()


def make_frame(kind, H, W, seed=0):
    rng = np.random.default_rng(seed + 7919 * H + W)
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "gradient":
        yy, xx = np.mgrid[0:H, 0:W]
        return np.stack([(xx * 255 // max(1, W - 1)), (yy * 255 // max(1, H - 1)), ((xx + yy) * 3) % 256], -1).astype(np.uint8)
    if kind == "constant":
        return np.full((H, W, 3), (37, 201, 118), np.uint8)
    if kind == "saturated":     # saturated primaries in blocks of random size: large DC steps and AC values, many 0xFF bytes
        pal = np.array([[0, 0, 255], [0, 255, 0], [255, 0, 0], [255, 255, 255], [0, 0, 0], [255, 0, 255]], np.uint8)
        cells = rng.integers(0, len(pal), (H // 3 + 1, W // 5 + 1))
        return pal[cells.repeat(3, 0).repeat(5, 1)[:H, :W]]
    raise ValueError(kind)


SIZES = [(1, 1), (8, 8), (9, 9), (1, 17), (16, 18), (16, 24), (53, 37), (30, 100), (7, 119), (321, 183), (17, 33), (31, 47),
         (180, 320), (270, 480), (360, 640)]
QUALITIES = [1, 30, 80, 95, 100]
KINDS = ["noise", "gradient", "constant", "saturated"]
CASES = [(H, W, q, k) for (H, W) in SIZES for q in QUALITIES for k in KINDS
         if not (H * W > 100_000 and (q, k) not in ((80, "noise"), (80, "gradient"), (100, "saturated"), (1, "noise")))]


@pytest.mark.parametrize("H,W,q,kind", CASES)
def test_reference_rules_equal_pillow(H, W, q, kind):
    frame = make_frame(kind, H, W)
    assert encode_reference(frame, q) == pillow_jpeg(frame, q)


def test_reference_rules_equal_pillow_1080p():
    frame = make_frame("noise", 1080, 1920)[:, :, :]
    frame[::7] = 255                                    # saturated rows among the noise: stuffing in every block row
    assert encode_reference(frame, 95) == pillow_jpeg(frame, 95)


def test_saturated_content_stuffs_often():
    """The 'saturated' frames really exercise 0xFF stuffing (the byte pattern the scatter pass has to get right)."""
    data = pillow_jpeg(make_frame("saturated", 180, 320), 100)
    hdr = len(jpeg_header(180, 320, 100))
    assert data[hdr:-2].count(b"\xff\x00") > 100


# ---- the host-only header entry point and the symbol table ------------------------------------------------------------------
def _header_bytes(H, W, q, cap=1024):
    lib = _lib.load()
    buf = (ctypes.c_uint8 * cap)()
    n = ctypes.c_int(0)
    st = lib.trl_jpeg_header(H, W, q, buf, cap, ctypes.byref(n))
    return st, bytes(buf[:n.value]), n.value


@pytest.mark.parametrize("H,W", SIZES + [(720, 1280), (1080, 1920), (2160, 3840), (65535, 65535)])
@pytest.mark.parametrize("q", QUALITIES + [0, 50, 101])
def test_trl_jpeg_header_equals_pillow(H, W, q):
    st, hdr, _ = _header_bytes(H, W, q)
    assert st == 0
    assert hdr == jpeg_header(H, W, q)
    if H * W <= 640 * 360 and 1 <= q <= 100:
        data = pillow_jpeg(make_frame("gradient", H, W), q)
        assert data[:len(hdr)] == hdr


def test_trl_jpeg_header_capacity_and_arguments():
    st, _, need = _header_bytes(360, 640, 80, cap=10)
    assert st == -4 and need == len(jpeg_header(360, 640, 80))
    for H, W in ((0, 8), (8, 0), (65536, 8), (8, -1)):
        st, _, _ = _header_bytes(H, W, 80)
        assert st == -1
        assert b"trl_jpeg" in _lib.load().trl_last_error()


def test_jpeg_symbols_exported():
    names = {"trl_jpeg_create", "trl_jpeg_encode", "trl_jpeg_destroy", "trl_jpeg_header"}
    hdr = open(os.path.join(ROOT, "include", "truely_hip.h")).read()
    assert names <= set(re.findall(r"\b(trl_[a-z0-9_]+)\s*\(", hdr))
    assert names <= set(_lib.EXPORTS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert names <= set(re.findall(r"\bT (trl_[a-z0-9_]+)", out))


def test_writer_keeps_pillow_without_device(tmp_path):
    from truely_amd import video_io
    w = video_io.open_writer(str(tmp_path / "o.avi"), 30, (64, 48))
    assert isinstance(w, video_io.AviMjpegWriter) and w.encoder == "pillow"
    w.write(make_frame("noise", 48, 64))
    w.release()
    r = video_io.AviMjpegReader(str(tmp_path / "o.avi"))
    assert r.n == 1
    r.f.seek(r.frames[0][0])
    assert r.f.read(r.frames[0][1]) == pillow_jpeg(make_frame("noise", 48, 64), 80)
    r.release()
    with pytest.raises(ValueError):
        video_io.AviMjpegWriter(str(tmp_path / "p.avi"), 30, (64, 48), encoder="h264")
