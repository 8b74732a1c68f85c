"""Inputs shared by the JPEG decoder's CPU and GPU tests: frame content, the size x subsampling x option table of good files (all
written by Pillow, all inside what the device decoder attempts), the unsupported kinds, and the fixed, seeded table of damaged
streams that the stand-alone fuzz program (tests/jpegd_fuzz.cpp) processes before any of them reaches a kernel."""
import io
import os

import numpy as np
from PIL import Image

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_ODD = np.load(os.path.join(GOLDEN, "clip_odd.npz"))
ODD = (int(_ODD["W"]), int(_ODD["H"]))                   # (W, H) of the golden odd clip

SIZES = [(1, 1), (7, 5), (8, 8), (16, 16), (17, 17), (37, 51), (48, 32), (64, 48), ODD, (320, 180)]   # (W, H)
QUALITIES = [1, 50, 80, 100]
CONTENT = ["noise", "gradient", "constant", "checker"]


def content(kind, W, H, seed=0):
    """An RGB frame (H, W, 3)."""
    rng = np.random.default_rng([seed, W, H])
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "gradient":
        y, x = np.mgrid[0:H, 0:W]
        return np.stack([(x * 255) // max(W - 1, 1), (y * 255) // max(H - 1, 1), ((x + y) * 255) // max(W + H - 2, 1)], -1).astype(np.uint8)
    if kind == "constant":
        return np.full((H, W, 3), (200, 30, 90), np.uint8)
    if kind == "checker":
        y, x = np.mgrid[0:H, 0:W]
        return np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], 3, -1)
    raise ValueError(kind)


def stuffed_file(W, H, quality, sub):
    """A noise frame whose scan holds a stuffed 0xFF byte: the first seed that gives one (a byte in 256 is 0xFF)."""
    for seed in range(100, 4000):
        data = encode(content("noise", W, H, seed), quality, sub)
        if b"\xff\x00" in data[scan_offset(data):]:
            return data
    raise AssertionError("no seed gives a stuffed byte")


def encode(rgb, quality=80, subsampling=2, **kw):
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "JPEG", quality=quality, subsampling=subsampling, **kw)
    return b.getvalue()


def pillow_bgr(data):
    """The reference: what AviMjpegReader.read() yields for this file."""
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[:, :, ::-1])


def good_files(W, H, sub):
    """[(label, file)] for one size and subsampling: every quality on noise, every other content at quality 80, and at a subset of
    the sizes the encoder options (optimised tables, a restart marker per block / per MCU row, an interval of 2 MCUs; a frame of more
    than 8 intervals wraps from RST7 to RST0)."""
    out = [(f"noise-q{q}", encode(content("noise", W, H, q), q, sub)) for q in QUALITIES]
    out += [(f"{k}-q80", encode(content(k, W, H), 80, sub)) for k in CONTENT[1:]]
    if W * H >= 64:            # (the scan of a smaller frame is a handful of bytes)
        out += [("stuffed-q80", stuffed_file(W, H, 80, sub)), ("stuffed-q100", stuffed_file(W, H, 100, sub))]
    if (W, H) in ((7, 5), (17, 17), (37, 51), (64, 48), ODD):
        rgb = content("noise", W, H, 7)
        out += [("optimize", encode(rgb, 80, sub, optimize=True)),
                ("rst-blocks1", encode(rgb, 80, sub, restart_marker_blocks=1)),
                ("rst-rows1", encode(rgb, 80, sub, restart_marker_rows=1)),
                ("rst-blocks2", encode(rgb, 90, sub, restart_marker_blocks=2)),
                ("rst-optimize", encode(rgb, 60, sub, restart_marker_blocks=3, optimize=True))]
    return out


def strip_segments(data, marker):
    """The file without its segments of this marker (before SOS)."""
    out, p = bytearray(data[:2]), 2
    while data[p + 1] != 0xDA:
        L = (data[p + 2] << 8) | data[p + 3]
        if data[p + 1] != marker:
            out += data[p:p + 2 + L]
        p += 2 + L
    return bytes(out + data[p:])


def unsupported_files(W=48, H=32):
    """[(label, file)]: kinds the device decoder does not attempt, made with Pillow."""
    rgb = content("gradient", W, H)
    base = encode(rgb)
    b = io.BytesIO(); Image.fromarray(rgb).convert("L").save(b, "JPEG"); gray = b.getvalue()
    b = io.BytesIO(); Image.fromarray(rgb).convert("CMYK").save(b, "JPEG"); cmyk = b.getvalue()
    return [("progressive", encode(rgb, progressive=True)), ("grayscale", gray), ("cmyk", cmyk), ("cut-in-headers", base[:300]),
            ("no-dht", strip_segments(base, 0xC4)), ("empty", b""), ("not-jpeg", b"RIFF" + base[4:])]


def scan_offset(data):
    p = 2
    while data[p + 1] != 0xDA:
        p += 2 + ((data[p + 2] << 8) | data[p + 3])
    return p + 2 + ((data[p + 2] << 8) | data[p + 3])


def damaged_files(W=64, H=48):
    """[(label, file)]: the fixed, seeded table of damaged streams.  Each is a Pillow file of W x H with bytes cut, overwritten or
    flipped; the decoder must report status 1 or 2 for it, or else decode exactly what tests/jpegd_ref.py decodes."""
    rng = np.random.default_rng(20240607)
    plain = encode(content("noise", W, H, 3), 80, 2)
    rst = encode(content("noise", W, H, 4), 80, 2, restart_marker_blocks=1)
    out = []
    s = scan_offset(plain)
    dht = plain.index(b"\xff\xc4")
    dqt = plain.index(b"\xff\xdb")
    for label, cut in (("cut-soi", 1), ("cut-app0", 10), ("cut-dqt", dqt + 20), ("cut-dht", dht + 30), ("cut-sos", s - 3), ("cut-scan-start", s),
                       ("cut-scan-1", s + 1), ("cut-scan-mid", (s + len(plain)) // 2), ("cut-before-eoi", len(plain) - 2), ("cut-in-eoi", len(plain) - 1)):
        out.append((label, plain[:cut]))
    half = (s + len(plain)) // 2
    out.append(("zero-tail", plain[:half] + bytes(len(plain) - half)))
    out.append(("ff-tail", plain[:half] + b"\xff" * (len(plain) - half)))
    out.append(("ff00-tail", plain[:half] + b"\xff\x00" * ((len(plain) - half) // 2)))
    for k in range(24):
        pos = int(rng.integers(s, len(plain) - 2))
        bit = 1 << int(rng.integers(0, 8))
        b = bytearray(plain); b[pos] ^= bit
        out.append((f"flip-{pos}-{bit}", bytes(b)))
    for k in range(8):
        pos = int(rng.integers(s, len(rst) - 2))
        b = bytearray(rst); b[pos] ^= 1 << int(rng.integers(0, 8))
        out.append((f"rst-flip-{pos}", bytes(b)))
    marks = [i for i in range(scan_offset(rst), len(rst) - 1) if rst[i] == 0xFF and 0xD0 <= rst[i + 1] <= 0xD7]
    b = bytearray(rst); b[marks[3] + 1] = 0xD0 + ((rst[marks[3] + 1] - 0xD0 + 1) & 7)
    out.append(("wrong-rst-number", bytes(b)))
    out.append(("rst-removed", rst[:marks[2]] + rst[marks[2] + 2:]))
    out.append(("rst-extra", rst[:marks[2]] + rst[marks[2]:marks[2] + 2] + rst[marks[2]:]))
    out.append(("rst-cut-at-marker", rst[:marks[5] + 1]))
    out.append(("rst-eoi-early", rst[:marks[4]] + b"\xff\xd9"))
    b = bytearray(plain); b[dht + 4 + 16] = 0xFF                      # one count of the first DHT: the table no longer fits its segment
    out.append(("dht-over-long", bytes(b)))
    b = bytearray(plain); b[dht + 2:dht + 4] = (0xFFFF).to_bytes(2, "big")
    out.append(("dht-length-past-file", bytes(b)))
    b = bytearray(plain); b[dht + 5:dht + 7] = b"\xff\xff"            # far more short codes than bits allow
    out.append(("dht-code-overflow", bytes(b)))
    b = bytearray(plain); b[dqt + 4] = 0x10
    out.append(("dqt-16bit", bytes(b)))
    sof = plain.index(b"\xff\xc0")
    b = bytearray(plain); b[sof + 5:sof + 9] = (H * 4).to_bytes(2, "big") + (W * 4).to_bytes(2, "big")
    out.append(("sof-larger-than-scan", bytes(b)))
    b = bytearray(plain); b[s:s + 40] = b"\xff" * 40
    out.append(("ff-run-at-scan-start", bytes(b)))
    b = bytearray(plain); b[half:half + 64] = bytes(rng.integers(0, 256, 64, dtype=np.uint8))
    out.append(("noise-in-scan", bytes(b)))
    out.append(("garbage-after-scan", plain[:-2] + b"\x12\x34\x56" + plain[-2:]))
    out.append(("second-scan", plain[:-2] + plain[s - 14:]))
    return out
