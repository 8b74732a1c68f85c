"""Inputs shared by the JPEG decoder's CPU and GPU tests: frame content, the size x subsampling x option table of good files (all
written by Pillow, all inside what the device decoder attempts), the unsupported kinds, the fixed, seeded table of damaged
streams that the stand-alone fuzz program (tests/jpegd_fuzz.cpp) processes before any of them reaches a kernel, and the synthetic
table: regular baseline streams that no encoder writes from pixels (edited headers, hand-coded scans, coefficients of chosen size),
each with what the decoder owes for it -- Pillow's bytes, or the frame reported irregular."""
import io
import os

import functools

import numpy as np
from PIL import Image

import jpegd_ref

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


# ---- streams no encoder writes from pixels ----------------------------------------------------------------------------------------
# Two builders: a header editor, which takes a Pillow file apart up to SOS and puts it together again after edits that leave the scan
# alone, and a baseline writer, which entropy-codes coefficient blocks given to it.  synthetic_files() is the table both feed.
SYN_SIZES = [(8, 8), (16, 16), (17, 17), (37, 51), (64, 48)]              # (W, H)
SUB_HV = {0: (1, 1), 1: (2, 1), 2: (2, 2)}                                # Pillow's subsampling -> luma (h, v)
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35,
          42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def split_header(data):
    """A Pillow file -> (items, scan).  items, in file order up to SOS: ["APP", marker, body], ["DQT", [[id, 64 bytes in zigzag
    order]]], ["DHT", [[class, id, 16 counts, symbols]]], ["SOF", H, W, [[id, hv, tq]]], ["DRI", interval],
    ["SOS", [[id, td, ta]]]; scan: the entropy-coded bytes and EOI."""
    items, p = [], 2
    while True:
        m, L = data[p + 1], (data[p + 2] << 8) | data[p + 3]
        body = data[p + 4:p + 2 + L]
        p += 2 + L
        if m == 0xDB:
            items.append(["DQT", [[body[q], bytes(body[q + 1:q + 65])] for q in range(0, len(body), 65)]])
        elif m == 0xC4:
            tabs, q = [], 0
            while q < len(body):
                n = sum(body[q + 1:q + 17])
                tabs.append([body[q] >> 4, body[q] & 15, bytes(body[q + 1:q + 17]), bytes(body[q + 17:q + 17 + n])])
                q += 17 + n
            items.append(["DHT", tabs])
        elif m == 0xC0:
            items.append(["SOF", (body[1] << 8) | body[2], (body[3] << 8) | body[4], [[body[6 + 3 * i], body[7 + 3 * i], body[8 + 3 * i]] for i in range(3)]])
        elif m == 0xDD:
            items.append(["DRI", (body[0] << 8) | body[1]])
        elif m == 0xDA:
            items.append(["SOS", [[body[1 + 2 * i], body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15] for i in range(3)]])
            return items, data[p:]
        else:
            items.append(["APP", m, bytes(body)])


def join_header(items, scan, fill=None):
    """The file of these items; fill(i) 0xFF fill bytes go in front of the i-th marker after SOI."""
    out = bytearray(b"\xff\xd8")
    for i, it in enumerate(items):
        kind = it[0]
        if kind == "APP":
            m, body = it[1], it[2]
        elif kind == "DQT":
            m, body = 0xDB, b"".join(bytes([t[0]]) + t[1] for t in it[1])
        elif kind == "DHT":
            m, body = 0xC4, b"".join(bytes([t[0] << 4 | t[1]]) + t[2] + t[3] for t in it[1])
        elif kind == "SOF":
            m, body = 0xC0, bytes([8]) + it[1].to_bytes(2, "big") + it[2].to_bytes(2, "big") + bytes([3]) + b"".join(bytes(c) for c in it[3])
        elif kind == "DRI":
            m, body = 0xDD, it[1].to_bytes(2, "big")
        else:
            m, body = 0xDA, bytes([3]) + b"".join(bytes([c[0], c[1] << 4 | c[2]]) for c in it[1]) + bytes([0, 63, 0])
        out += b"\xff" * (fill(i) if fill else 0) + bytes([0xFF, m]) + (len(body) + 2).to_bytes(2, "big") + body
    return bytes(out + scan)


def _item(items, kind):
    return next(it for it in items if it[0] == kind)


def _tables(items, kind):
    return [t for it in items if it[0] == kind for t in it[1]]


def set_component_ids(items, ids):
    for part in (_item(items, "SOF")[3], _item(items, "SOS")[1]):
        for c, i in zip(part, ids):
            c[0] = i


def drop_app0(items):
    items[:] = [it for it in items if not (it[0] == "APP" and it[1] == 0xE0)]


def renumber_tables(items, q, dc, ac):
    """Table ids old -> new (dicts) in DQT and DHT, with SOF's Tq and SOS's Td / Ta following."""
    for t in _tables(items, "DQT"):
        t[0] = q[t[0]]
    for t in _tables(items, "DHT"):
        t[1] = (ac if t[0] else dc)[t[1]]
    for c in _item(items, "SOF")[3]:
        c[2] = q[c[2]]
    for c in _item(items, "SOS")[1]:
        c[1], c[2] = dc[c[1]], ac[c[2]]


def regroup_tables(items, merged):
    """All tables in one DQT and one DHT segment, or one table per segment, at the place of the first segment of each kind."""
    for kind in ("DQT", "DHT"):
        tabs = _tables(items, kind)
        at = items.index(_item(items, kind))
        items[:] = [it for it in items if it[0] != kind]
        items[at:at] = [[kind, tabs]] if merged else [[kind, [t]] for t in tabs]


def cr_own_tables(items):
    """Cr gets a third quantisation table (other contents than Cb's) and a third Huffman pair (Cb's codes: the scan is untouched)."""
    q = _tables(items, "DQT")[1]
    items.insert(items.index(_item(items, "SOF")), ["DQT", [[2, bytes(min(255, 2 * b + 1) for b in q[1])]]])
    items.insert(items.index(_item(items, "SOS")), ["DHT", [[t[0], 2, t[2], t[3]] for t in _tables(items, "DHT") if t[1] == 1]])
    _item(items, "SOF")[3][2][2] = 2
    _item(items, "SOS")[1][2][1:] = [2, 2]


def define_twice(items):
    """The luma quantiser and the luma DC table are first defined wrong (the chroma ones' contents), then right."""
    q, h = _tables(items, "DQT"), _tables(items, "DHT")
    wrong_dc = next(t for t in h if t[0] == 0 and t[1] == 1)
    items[1:1] = [["DQT", [[0, q[1][1]]]], ["DHT", [[0, 0, wrong_dc[2], wrong_dc[3]]]]]


def define_unused(items):
    q, h = _tables(items, "DQT"), _tables(items, "DHT")
    items[1:1] = [["DQT", [[3, bytes(range(1, 65))]]], ["DHT", [[1, 3, h[1][2], h[1][3]], [0, 3, h[0][2], h[0][3]]]]]


def add_marker_like_segments(items):
    """COM, APP1 and APP13 segments whose bodies hold EOI, SOS, a stuffed 0xFF and a restart marker."""
    body = b"\xff\xd9 \xff\xda\x00\x0c\x03\x01\x00 \xff\x00 \xff\xd0 \xff\xd8\xff"
    items[1:1] = [["APP", 0xFE, body]]
    at = items.index(_item(items, "SOF"))
    items[at:at] = [["APP", 0xE1, b"Exif\xff\xd9" + body], ["APP", 0xED, body + b"Photoshop\xff\xda"]]
    items.insert(items.index(_item(items, "SOS")), ["APP", 0xFE, body[::-1]])


def rescale_dqt(items, fn):
    """Every quantiser q of table t at zigzag position k becomes fn(t, k, q), clamped to 1..255."""
    for t in _tables(items, "DQT"):
        t[1] = bytes(max(1, min(255, int(fn(t[0], k, q)))) for k, q in enumerate(t[1]))


def edited(data, *edits, fill=None):
    items, scan = split_header(data)
    for e in edits:
        e(items)
    return join_header(items, scan, fill)


def rescaled(data, fn):
    return edited(data, lambda it: rescale_dqt(it, fn))


RGB_IDS = b"RGB"
COMPONENT_IDS = [(0, 1, 2), (3, 2, 1), tuple(b"YCc"), (255, 0, 7), tuple(b"rgb")]


def header_edit_files(W, H, sub):
    """[(label, file)]: Pillow files whose headers were edited; every one is regular baseline JPEG that the decoder attempts."""
    plain = encode(content("noise", W, H, 11), 80, sub)
    opt = encode(content("gradient", W, H), 90, sub, optimize=True)
    rst = encode(content("noise", W, H, 12), 80, sub, restart_marker_blocks=1)
    hv = SUB_HV[sub]
    mcus = ((W + 8 * hv[0] - 1) // (8 * hv[0])) * ((H + 8 * hv[1] - 1) // (8 * hv[1]))
    out = [(f"ids-{'-'.join(map(str, ids))}", edited(plain, lambda it, ids=ids: set_component_ids(it, ids))) for ids in COMPONENT_IDS]
    out += [("ids-255-0-7-no-app0", edited(plain, drop_app0, lambda it: set_component_ids(it, (255, 0, 7)))),
            ("no-app0", edited(plain, drop_app0)),
            ("tables-2-3", edited(plain, lambda it: renumber_tables(it, {0: 2, 1: 3}, {0: 2, 1: 3}, {0: 3, 1: 2}))),
            ("tables-swapped", edited(opt, lambda it: renumber_tables(it, {0: 1, 1: 0}, {0: 1, 1: 0}, {0: 1, 1: 0}))),
            ("dc-ac-ids-differ", edited(plain, lambda it: renumber_tables(it, {0: 3, 1: 0}, {0: 0, 1: 2}, {0: 1, 1: 3}))),
            ("cr-own-tables", edited(plain, cr_own_tables)),
            ("cr-own-tables-merged", edited(opt, cr_own_tables, lambda it: regroup_tables(it, True))),
            ("merged", edited(plain, lambda it: regroup_tables(it, True))),
            ("split", edited(opt, lambda it: regroup_tables(it, True), lambda it: regroup_tables(it, False))),
            ("defined-twice", edited(plain, define_twice)),
            ("unused-table", edited(opt, define_unused)),
            ("fill-bytes", edited(plain, fill=lambda i: 1 + i % 3)),
            ("fill-bytes-rst", edited(rst, fill=lambda i: 3 - i % 3)),
            ("marker-like-segments", edited(plain, add_marker_like_segments)),
            ("marker-like-segments-fill", edited(rst, add_marker_like_segments, define_unused, fill=lambda i: 1 + (i & 1))),
            ("dri-twice", edited(rst, lambda it: it.insert(1, ["DRI", 7]))),
            ("dri-then-0", edited(plain, lambda it: it.insert(2, ["DRI", max(1, mcus // 2)]),
                                  lambda it: it.insert(it.index(_item(it, "SOS")), ["DRI", 0]))),
            ("dqt-x2", rescaled(plain, lambda t, k, q: 2 * q)),
            ("dqt-by-index", rescaled(opt, lambda t, k, q: q + (k * 7 + t * 3) % 5))]
    return out


def rgb_id_files(W=48, H=32):
    """[(label, file)]: component ids 'R' 'G' 'B', with and without APP0: libjpeg may read such a file as RGB; never attempted."""
    plain = encode(content("gradient", W, H), 80, 2)
    return [("rgb-ids", edited(plain, lambda it: set_component_ids(it, RGB_IDS))),
            ("rgb-ids-no-app0", edited(plain, drop_app0, lambda it: set_component_ids(it, RGB_IDS)))]


# ---- the baseline writer ----
def std_huff():
    """{(class, id): (16 counts, symbols)}: the tables of Annex K, as Pillow writes them into a file that is not optimised."""
    return {(t[0], t[1]): (t[2], t[3]) for t in _tables(split_header(encode(content("constant", 8, 8)))[0], "DHT")}


def flat_huff():
    """Tables whose codes are 4 (DC) or 8 and 9 (AC) bits long except the last four symbols of each, which get 16-bit codes: the
    DC categories 0, 11, 10, 9 and the AC symbols EOB, ZRL, 0/10 and 15/10."""
    dc_syms = bytes([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 0])
    dc_counts = bytes([0, 0, 0, 8] + [0] * 11 + [4])
    last = [0x00, 0xF0, 0x0A, 0xFA]
    ac_syms = [r << 4 | s for r in range(16) for s in range(1, 11) if (r << 4 | s) not in last] + last      # 162 symbols
    ac_counts = bytes([0] * 7 + [128, len(ac_syms) - 132] + [0] * 6 + [4])
    tabs = {}
    for i in range(2):
        tabs[(0, i)] = (dc_counts, dc_syms)
        tabs[(1, i)] = (ac_counts, bytes(ac_syms))
    return tabs


def _codes(counts, syms):
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[syms[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, length):
        self.acc, self.n = (self.acc << length) | code, self.n + length
        while self.n >= 8:
            self.n -= 8
            b = (self.acc >> self.n) & 255
            self.out += b"\xff\x00" if b == 255 else bytes([b])
        self.acc &= (1 << self.n) - 1

    def align(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _put_value(bits, code, v):
    s = abs(v).bit_length()
    bits.put(*code)
    if s:
        bits.put(v if v >= 0 else v + (1 << s) - 1, s)


def write_baseline(coefs, quant, huff, hs, vs, W, H, ri=0, tq=(0, 1, 1), td=(0, 1, 1), ta=(0, 1, 1), ids=(1, 2, 3), app0=True, seen=None):
    """A baseline file (SOF0, one interleaved scan) that codes these coefficients: coefs[c] (block rows, block columns, 64) int16 in
    natural order, whole MCUs; quant {id: 64 quantisers in natural order}; huff {(class, id): (16 counts, symbols)}; component c uses
    quantiser tq[c] and the Huffman tables td[c] / ta[c].  ri: restart interval in MCUs (0: none).  seen, a dict of sets, collects what
    was coded: "dc" categories, "ac" symbols, "zrl" zero runs in front of a coefficient, "len" code lengths, "rst" marker bytes."""
    items = [["APP", 0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0"]] if app0 else []
    items.append(["DQT", [[i, bytes(int(q[ZIGZAG[k]]) for k in range(64))] for i, q in sorted(quant.items())]])
    items.append(["SOF", H, W, [[ids[c], (hs << 4 | vs) if c == 0 else 0x11, tq[c]] for c in range(3)]])
    items.append(["DHT", [[k[0], k[1], bytes(t[0]), bytes(t[1])] for k, t in sorted(huff.items())]])
    if ri:
        items.append(["DRI", ri])
    items.append(["SOS", [[ids[c], td[c], ta[c]] for c in range(3)]])
    dc = [_codes(*huff[(0, td[c])]) for c in range(3)]
    ac = [_codes(*huff[(1, ta[c])]) for c in range(3)]
    mcux, mcuy = (W + 8 * hs - 1) // (8 * hs), (H + 8 * vs - 1) // (8 * vs)
    assert coefs[0].shape == (mcuy * vs, mcux * hs, 64) and coefs[1].shape == coefs[2].shape == (mcuy, mcux, 64)
    bits, pred, nrst = _Bits(), [0, 0, 0], 0
    seen = seen if seen is not None else {}
    for k in ("dc", "ac", "zrl", "len", "rst"):
        seen.setdefault(k, set())
    for m in range(mcux * mcuy):
        if ri and m and m % ri == 0:
            bits.align()
            bits.out += bytes([0xFF, 0xD0 + (nrst & 7)])
            seen["rst"].add(0xD0 + (nrst & 7))
            nrst, pred = nrst + 1, [0, 0, 0]
        my, mx = divmod(m, mcux)
        for c in range(3):
            ch, cv = (hs, vs) if c == 0 else (1, 1)
            for v in range(cv):
                for h in range(ch):
                    blk = [int(x) for x in coefs[c][my * cv + v, mx * ch + h]]
                    d = blk[0] - pred[c]
                    pred[c] = blk[0]
                    _put_value(bits, dc[c][abs(d).bit_length()], d)
                    seen["dc"].add(abs(d).bit_length())
                    seen["len"].add(dc[c][abs(d).bit_length()][1])
                    run = 0
                    for k in range(1, 64):
                        x = blk[ZIGZAG[k]]
                        if x == 0:
                            run += 1
                            continue
                        seen["zrl"].add(run)
                        while run > 15:
                            bits.put(*ac[c][0xF0])
                            seen["ac"].add(0xF0)
                            seen["len"].add(ac[c][0xF0][1])
                            run -= 16
                        sym = run << 4 | abs(x).bit_length()
                        _put_value(bits, ac[c][sym], x)
                        seen["ac"].add(sym)
                        seen["len"].add(ac[c][sym][1])
                        run = 0
                    if run:
                        bits.put(*ac[c][0x00])
                        seen["ac"].add(0x00)
                        seen["len"].add(ac[c][0x00][1])
    bits.align()
    data = join_header(items, bytes(bits.out) + b"\xff\xd9")
    _WRITTEN[data] = np.concatenate([np.asarray(a, np.int16).reshape(-1) for a in coefs])
    return data


_WRITTEN = {}


def written_coefficients(data):
    """The coefficients write_baseline was given for this file (components one after the other, as the decoder's coefficient slot
    holds them), or None for a file it did not write."""
    return _WRITTEN.get(data)


# ---- the synthetic table ----
def gate_expectation(data):
    """"pillow" or "gated": the IDCT gate's conditions on this file's coefficients, evaluated in 64-bit
    arithmetic, in which nothing wraps: the specification that the kernel's and the restatement's 32-bit tests are held to."""
    info = jpegd_ref.parse(data)
    for coef, quant in zip(jpegd_ref.entropy_decode(data, info), info["quant"]):
        by, bx = coef.shape[:2]
        x = np.moveaxis((coef.astype(np.int64) * quant.astype(np.int64)).reshape(by, bx, 8, 8), 2, 0)
        for shift, axis, lo, hi in ((11, 3, -32768, 32767), (18, None, -512, 511)):
            a = np.abs(x)
            if max((a[0] + a[4]).max(), (a[2] + a[6]).max(), (a[1] + a[3] + a[5] + a[7]).max()) > 32767:
                return "gated"
            x = jpegd_ref._idct_1d(x, shift)
            assert x.dtype == np.int64
            if x.min() < lo or x.max() > hi:
                return "gated"
            if axis is not None:
                x = np.moveaxis(x, axis, 0)
    return "pillow"


def former_gate_trips(data):
    """The gate as it was before the IDCT gate: a dequantised value outside int16."""
    info = jpegd_ref.parse(data)
    return any(bool((np.abs(c.astype(np.int32) * q) > 32767).any()) for c, q in zip(jpegd_ref.entropy_decode(data, info), info["quant"]))


def table_set(data):
    """A key of the file's decode tables: files with equal keys share one (DQT, DHT) set in a decoder call."""
    info = jpegd_ref.parse(data)
    return hash(tuple(a.tobytes() for k in ("quant", "dc", "ac") for a in info[k]))


def blank(W, H, hs, vs):
    mcux, mcuy = (W + 8 * hs - 1) // (8 * hs), (H + 8 * vs - 1) // (8 * vs)
    return [np.zeros((mcuy * vs, mcux * hs, 64), np.int16), np.zeros((mcuy, mcux, 64), np.int16), np.zeros((mcuy, mcux, 64), np.int16)]


def coded_blocks(coefs, hs, vs):
    """Per component, its blocks (views of 64 coefficients) in the order the scan codes them."""
    mcuy, mcux = coefs[1].shape[:2]
    out = [[], [], []]
    for m in range(mcux * mcuy):
        my, mx = divmod(m, mcux)
        for c in range(3):
            ch, cv = (hs, vs) if c == 0 else (1, 1)
            out[c] += [coefs[c][my * cv + v, mx * ch + h] for v in range(cv) for h in range(ch)]
    return out


def _magnitude(s, top):
    return 0 if s == 0 else (1 << s) - 1 if top else 1 << (s - 1)


def entropy_contents(W, H, hs, vs):
    """[(label, coefficients)]: what the entropy coder can be made to write, whatever the frame's content then looks like.  The
    smallest frames hold three blocks, so a kind is spread over the components and over consecutive blocks as far as they go."""
    out = []
    co = blank(W, H, hs, vs)                                 # DC differences of every category 0..11, both signs, smallest and largest
    j = 0
    for c, blocks in enumerate(coded_blocks(co, hs, vs)):
        dc = 0
        for b in blocks:
            mag = _magnitude((j * 5 + c) % 12, j & 1)
            dc += -mag if dc > 0 else mag
            b[0] = dc
            j += 1
    out.append(("dc-categories", co))
    co = blank(W, H, hs, vs)                                 # AC categories 1..10 at every zigzag position
    j = 0
    for blocks in coded_blocks(co, hs, vs):
        for b in blocks:
            b[ZIGZAG[1 + (j * 11) % 63]] = _magnitude(1 + j % 10, j & 1) * (1 if j & 2 else -1)
            j += 1
    out.append(("ac-categories", co))
    co = blank(W, H, hs, vs)                                 # runs of 16, 32 and 47 zeros (ZRL chains), blocks without EOB
    j = 0
    for blocks in coded_blocks(co, hs, vs):
        for b in blocks:
            for k in ((17,), (33,), (48,), (1, 49), (16, 63), (63,), (2, 19, 52), ())[j % 8]:
                b[ZIGZAG[k]] = 3 - 5 * (k & 1)
            b[0] = 20 * (j % 5) - 40
            j += 1
    out.append(("zrl-and-no-eob", co))
    for seed in range(400):                                  # every coefficient non-zero, and a stuffed 0xFF byte in the scan
        rng = np.random.default_rng([seed, W, H, hs, vs])
        co = blank(W, H, hs, vs)
        for a in co:
            a[...] = rng.integers(1, 24, a.shape) * rng.choice([-1, 1], a.shape)
        data = write_baseline(co, {0: np.ones(64, int), 1: np.ones(64, int)}, std_huff(), hs, vs, W, H)
        if b"\xff\x00" in data[jpegd_ref.parse(data)["scan"]:]:
            break
    else:
        raise AssertionError("no seed gives a stuffed byte")
    out.append(("dense-stuffed", co))
    return out


def entropy_files(W, H, sub, seen=None):
    """[(label, file)]: the entropy contents under the standard tables, the flat ones (16-bit codes) and a pair whose DC and AC ids
    differ per component, with restart intervals of 0, 1, one that does not divide the MCU count and one larger than it."""
    hs, vs = SUB_HV[sub]
    mcus = ((W + 8 * hs - 1) // (8 * hs)) * ((H + 8 * vs - 1) // (8 * vs))
    odd = next((r for r in range(2, mcus) if mcus % r), None)
    std, flat = std_huff(), flat_huff()
    crossed = {(0, 0): std[(0, 0)], (0, 2): std[(0, 1)], (1, 3): std[(1, 0)], (1, 1): std[(1, 1)]}
    kinds = {"std": dict(huff=std), "flat": dict(huff=flat), "crossed": dict(huff=crossed, td=(0, 2, 2), ta=(3, 1, 1), ids=(7, 8, 200), app0=False)}
    quant = {0: np.ones(64, int), 1: np.ones(64, int)}
    out = []
    for label, co in entropy_contents(W, H, hs, vs):
        for kind, kw in kinds.items():
            for ri in (0, 1, odd, mcus + 3):
                if ri is None or (ri and kind == "crossed" and label != "dense-stuffed"):
                    continue
                out.append((f"{label}-{kind}-ri{ri}", write_baseline(co, quant, hs=hs, vs=vs, W=W, H=H, ri=ri, seen=seen, **kw)))
    return out


def _dc_only(W, H, hs, vs, c, q, coef):
    co = blank(W, H, hs, vs)
    co[c][..., 0] = coef
    quant = {0: np.ones(64, int), 1: np.ones(64, int)}
    quant[min(c, 1)][0] = q
    return write_baseline(co, quant, std_huff(), hs, vs, W, H)


# A DC-only block's output is (dc + 4) >> 3 everywhere (pass 1: dc << 2, pass 2: (4 dc 2^13 + 2^17) >> 18), so the first value
# the range-limit mask wraps is reached at dc = 4092 (-> 512) and dc = -4101 (-> -513).  (quantiser, coefficient, expectation):
DC_EDGES = [(2, 2045, "pillow"),      # 4090 -> 511 (4091, the last, is prime: no quantiser x coefficient gives it)
            (4, 1023, "gated"),       # 4092 -> 512
            (4, -1025, "pillow"),     # -4100 -> -512
            (3, -1367, "gated"),      # -4101 -> -513
            (8, 511, "pillow"), (8, -512, "pillow"), (1, 2047, "pillow"), (1, -2047, "pillow"),
            # pass 1 writes dc << 2 into a 16-bit workspace: 32760 | 32768 and -32768 | -32776.  No block has a workspace value
            # past int16 and all its outputs inside [-512, 511], so both sides of these pairs are gated already.
            (6, 1365, "gated"), (8, 1024, "gated"), (8, -1024, "gated"), (17, -482, "gated")]
AC_POSITIONS = [1, 8, 9, 36, 63]                                              # natural index of the single AC coefficient


def _single_ac(W, H, hs, vs, pos, q, coef):
    co = blank(W, H, hs, vs)
    co[0][..., pos] = coef
    co[2][0, 0, pos] = -coef
    return write_baseline(co, {0: np.full(64, q), 1: np.full(64, q)}, std_huff(), hs, vs, W, H)


@functools.lru_cache(maxsize=None)
def _ac_edge(pos, q=16):
    """The largest coefficient c for which a block holding only q x c at this position passes the gate (bisection on an 8 x 8 frame:
    the outputs grow with |c|)."""
    lo, hi = 1, 1023
    assert gate_expectation(_single_ac(8, 8, 1, 1, pos, q, lo)) == "pillow" and gate_expectation(_single_ac(8, 8, 1, 1, pos, q, hi)) == "gated"
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if gate_expectation(_single_ac(8, 8, 1, 1, pos, q, mid)) == "pillow" else (lo, mid)
    return lo


def magnitude_files(W, H, sub):
    """[(label, file, expectation)]: coefficients of chosen size.  The expectation of a DC-only block is written down above; the
    others are what gate_expectation computes.  None trips the former gate (|coefficient x quantiser| <= 32767) except the three
    named int16."""
    hs, vs = SUB_HV[sub]
    out = [(f"dc-c{c}-{q}x{coef}", _dc_only(W, H, hs, vs, c, q, coef), e) for c in range(3) for q, coef, e in DC_EDGES]
    for pos in AC_POSITIONS:
        edge = _ac_edge(pos)
        for coef in (edge // 2, edge, edge + 1, -edge, -edge - 1):
            out.append((f"ac{pos}-16x{coef}", _single_ac(W, H, hs, vs, pos, 16, coef), None))
    for amp in (256, 1024, 2048, 3072, 4096, 8192, 16384, 32767):             # sparse blocks: 1..4 coefficients of up to +-amp
        q = -(-amp // 1023)
        for seed in range(2):
            rng = np.random.default_rng([amp, seed, W, H, sub])
            co = blank(W, H, hs, vs)
            for a in co:
                for blk in a.reshape(-1, 64):
                    idx = rng.choice(64, int(rng.integers(1, 5)), replace=False)
                    blk[idx] = rng.integers(-(amp // q), amp // q + 1, len(idx))
            out.append((f"sparse-{amp}-{seed}", write_baseline(co, {0: np.full(64, q), 1: np.full(64, q)}, std_huff(), hs, vs, W, H), None))
    for kind in ("white", "noise", "checker"):                                # Pillow files at quality 100 with other quantisers
        rgb = np.full((H, W, 3), 255, np.uint8) if kind == "white" else content(kind, W, H, 5)
        base = encode(rgb, 100, sub)
        for label, fn in (("dc8", lambda t, k, q: 8 if k == 0 else q), ("x2", lambda t, k, q: 2), ("x4", lambda t, k, q: 4),
                          ("x16", lambda t, k, q: 16), ("ac3", lambda t, k, q: 3 if k else q)):
            out.append((f"{kind}-q100-{label}", rescaled(base, fn), None))
    co = blank(W, H, hs, vs)
    co[0][0, 0, 1] = 1023
    out.append(("int16-ac", write_baseline(co, {0: np.full(64, 255), 1: np.full(64, 255)}, std_huff(), hs, vs, W, H), "gated"))
    out.append(("int16-dc", _dc_only(W, H, hs, vs, 1, 255, -2047), "gated"))
    # 112 x 1171 = 2^17 + 80: in 32 bits pass 2's dc << 15 wraps to 80 << 15 and every output to (80 + 4) >> 3 = 10, well inside
    # [-512, 511]: a gate that looked at the outputs only, after they have wrapped, would let this frame through
    out.append(("int16-dc-wraps-into-range", _dc_only(W, H, hs, vs, 0, 112, 1171), "gated"))
    return [(label, data, e or gate_expectation(data)) for label, data, e in out]


@functools.lru_cache(maxsize=None)
def synthetic_files(W, H, sub):
    """[(label, file, expectation)] for one size of SYN_SIZES and one subsampling: header edits of Pillow files, the baseline writer's
    entropy cases (both kinds hold coefficients of ordinary size: "pillow") and the coefficient-magnitude family ("pillow" where the
    decoder must give Pillow's bytes, "gated" where it must report the frame irregular and write nothing)."""
    out = [("edit-" + label, data, "pillow") for label, data in header_edit_files(W, H, sub)]
    out += [("entropy-" + label, data, "pillow") for label, data in entropy_files(W, H, sub)]
    out += [("magnitude-" + label, data, e) for label, data, e in magnitude_files(W, H, sub)]
    return out
