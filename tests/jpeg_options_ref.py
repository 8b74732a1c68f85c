"""The Motion-JPEG encoder's rules with its four options, restated in numpy (no GPU): what Pillow's
``Image.save(format="JPEG", quality=q, subsampling=s, restart_marker_rows=r | restart_marker_blocks=b, optimize=o)`` does through
libjpeg-turbo.  The colour conversion, FDCT, quantisation, Annex K tables and marker layout come from ``tests/test_jpeg_cpu.py``;
this file adds

* the 4:2:2 MCU (16 x 8: Y0 Y1 Cb Cr, h2v1 average with bias 0,1,0,1...) and the 4:4:4 MCU (8 x 8: Y Cb Cr),
* libjpeg's dummy blocks for any sampling: past the right edge zero AC and the DC of the block to the left; a block row past the
  bottom edge zero AC and the DC of the block before it in the MCU,
* restart intervals: a DRI segment after the DHTs; every R MCUs the DC predictors return to 0, the bits are padded with ones to
  a byte (stuffed like any other byte) and RSTn (n cycling 0..7) follows, but not after the last interval; rows win over blocks,
  and rows x MCUs-per-row is clamped to 65535,
* ``optimize``: the symbol counts of the scan (luma tables and chroma tables, Cb and Cr together) and jpeg_gen_optimal_table's
  procedure, one DHT segment per table in the order DC luma, AC luma, DC chroma, AC chroma.

``tests/test_jpeg_options_cpu.py`` pins all of it to Pillow's bytes; the GPU tests compare the device encoder with Pillow directly."""
import io

import numpy as np

from test_jpeg_cpu import (AC_CHROMA, AC_LUMA, DC_CHROMA, DC_LUMA, ZIGZAG, _blocks, _pad_to, color_convert, fdct_islow, huff_codes,
                           quant_tables, quantize)

SAMPLING = {0: (1, 1), 1: (2, 1), 2: (2, 2)}            # Pillow's subsampling -> luma sampling factors (h, v)


def geometry(H, W, subsampling):
    h, v = SAMPLING[subsampling]
    mx, my = -(-W // (8 * h)), -(-H // (8 * v))
    return h, v, mx, my


def restart_interval(H, W, subsampling, restart_rows=0, restart_blocks=0):
    """libjpeg's restart interval in MCUs (0: none) -- the value the DRI segment carries."""
    _, _, mx, _ = geometry(H, W, subsampling)
    if restart_rows > 0:
        return min(restart_rows * mx, 65535)
    return restart_blocks


def optimal_table(freq256):
    """jpeg_gen_optimal_table: 256 counts -> (bits[16], vals, longest unadjusted code length)."""
    freq = [int(x) for x in freq256] + [1]              # the pseudo-symbol 256 keeps the all-ones code free
    codesize = [0] * 257
    others = [-1] * 257
    while True:
        c1, v = -1, 1000000000
        for i in range(257):                            # the least frequent; of equals the larger symbol
            if freq[i] and freq[i] <= v:
                v, c1 = freq[i], i
        c2, v = -1, 1000000000
        for i in range(257):
            if freq[i] and freq[i] <= v and i != c1:
                v, c2 = freq[i], i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    bits = [0] * 33
    for cs in codesize:
        if cs:
            assert cs <= 32
            bits[cs] += 1
    longest = max((i for i in range(33) if bits[i]), default=0)
    if not longest:
        return [0] * 16, [], 0
    i = 32
    while i > 16:                                       # no code may be longer than 16 bits
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
        i -= 1
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                                        # the pseudo-symbol's code
    vals = [s for length in range(1, 33) for s in range(256) if codesize[s] == length]
    return bits[1:17], vals, longest


def header(H, W, quality, subsampling=2, dri=0, tables=None):
    """Pillow's marker sequence up to and including SOS.  tables: four (bits, vals), default Annex K."""
    def seg(marker, body):
        return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body
    ql, qc = quant_tables(quality)
    h, v = SAMPLING[subsampling]
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += seg(0xDB, bytes([0]) + bytes(ql[ZIGZAG].astype(np.uint8))) + seg(0xDB, bytes([1]) + bytes(qc[ZIGZAG].astype(np.uint8)))
    out += seg(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, 1, (h << 4) | v, 0, 2, 0x11, 1, 3, 0x11, 1]))
    tables = tables or (DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA)
    for cls_id, (bits, vals) in zip((0x00, 0x10, 0x01, 0x11), tables):
        out += seg(0xC4, bytes([cls_id]) + bytes(bits) + bytes(vals))
    if dri > 0:
        out += seg(0xDD, dri.to_bytes(2, "big"))
    return out + seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def component_blocks(bgr, quality, subsampling):
    """Quantised blocks in zigzag order per component, on the grid of whole MCUs, dummies included: [(rows, cols, 64)] x 3."""
    H, W = bgr.shape[:2]
    h, v, mx, my = geometry(H, W, subsampling)
    y, cb, cr = color_convert(np.asarray(bgr)[:, :, ::-1])
    ql, qc = quant_tables(quality)
    out = []
    for plane, qt, ch, cv in ((y, ql, h, v), (cb, qc, 1, 1), (cr, qc, 1, 1)):
        fh, fv = h // ch, v // cv                       # this component's downsampling factors
        cw, chh = -(-W * ch // h), -(-H * cv // v)      # its size in samples
        bw, bh = -(-cw // 8), -(-chh // 8)              # blocks that hold samples
        full = _pad_to(plane, chh * fv, 8 * bw * fh)    # rows to whole sample rows, columns to whole blocks, by replication
        if (fh, fv) == (2, 2):
            s = full[0::2, 0::2] + full[0::2, 1::2] + full[1::2, 0::2] + full[1::2, 1::2]
            s = (s + np.where(np.arange(s.shape[1]) & 1, 2, 1)) >> 2
        elif (fh, fv) == (2, 1):
            s = (full[:, 0::2] + full[:, 1::2] + (np.arange(full.shape[1] // 2) & 1)) >> 1
        else:
            s = full
        q = quantize(fdct_islow(_blocks(_pad_to(s, 8 * bh, 8 * bw)) - 128), qt)[..., ZIGZAG]
        grid = np.zeros((my * cv, mx * ch, 64), np.int64)
        grid[:bh, :bw] = q
        for bx in range(bw, mx * ch):                   # right dummies: the DC of the block to the left
            grid[:bh, bx, 0] = grid[:bh, bx - 1, 0]
        for by in range(bh, my * cv):                   # bottom dummy rows: the DC of the block before them in the MCU
            assert cv == 2 and by % 2 == 1
            grid[by, :, 0] = grid[by - 1, ch - 1::ch, 0].repeat(ch)
        out.append(grid)
    return out


def _block_symbols(z, pred):
    """One block -> [(table 0 = DC / 1 = AC, symbol, extra bits, their count)]."""
    diff = int(z[0]) - pred
    n = abs(diff).bit_length()
    out = [(0, n, (diff if diff >= 0 else diff - 1) & ((1 << n) - 1), n)]
    last = 0
    for k in np.flatnonzero(z[1:]) + 1:
        r = int(k) - last - 1
        while r > 15:
            out.append((1, 0xF0, 0, 0))
            r -= 16
        vv = int(z[k])
        n = abs(vv).bit_length()
        out.append((1, (r << 4) | n, (vv if vv >= 0 else vv - 1) & ((1 << n) - 1), n))
        last = int(k)
    if last != 63:
        out.append((1, 0x00, 0, 0))
    return out


def encode(bgr, quality, subsampling=2, restart_rows=0, restart_blocks=0, optimize=False, info=None):
    """A complete baseline JPEG file of one BGR frame, byte for byte what Pillow writes for the RGB frame with these options.
    info (a dict) receives what the table tests want to know: 'stuffed_pad' (intervals whose padded last byte came out as 0xFF in
    front of a marker), 'maxlen' (the longest unadjusted code length of the four optimal tables), 'intervals'."""
    H, W = bgr.shape[:2]
    h, v, mx, my = geometry(H, W, subsampling)
    comps = component_blocks(bgr, quality, subsampling)
    R = restart_interval(H, W, subsampling, restart_rows, restart_blocks)
    per = R if R > 0 else mx * my
    intervals, cur, pred = [], [], [0, 0, 0]
    for m in range(mx * my):
        if m and m % per == 0:
            intervals.append(cur)
            cur, pred = [], [0, 0, 0]
        j, i = divmod(m, mx)
        for c, (ch, cv) in enumerate(((h, v), (1, 1), (1, 1))):
            for by in range(cv):
                for bx in range(ch):
                    z = comps[c][j * cv + by, i * ch + bx]
                    cur += [(2 * (c > 0) + t, s, e, n) for t, s, e, n in _block_symbols(z, pred[c])]
                    pred[c] = int(z[0])
    intervals.append(cur)
    tables = (DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA)
    maxlen = 0
    if optimize:
        hist = np.zeros((4, 256), np.int64)
        for iv in intervals:
            for t, s, _, _ in iv:
                hist[t, s] += 1
        built = [optimal_table(hist[t]) for t in range(4)]
        tables = [(b, vals) for b, vals, _ in built]
        maxlen = max(longest for _, _, longest in built)
    codes = [huff_codes(t) for t in tables]
    scan, stuffed_pad = b"", 0
    for k, iv in enumerate(intervals):
        parts = []
        for t, s, e, n in iv:
            code, length = codes[t][s]
            parts.append(format(code, f"0{length}b"))
            if n:
                parts.append(format(e, f"0{n}b"))
        bits = "".join(parts)
        pad = -len(bits) % 8
        bits += "1" * pad
        data = int(bits, 2).to_bytes(len(bits) // 8, "big") if bits else b""
        scan += data.replace(b"\xff", b"\xff\x00")
        if k < len(intervals) - 1:
            stuffed_pad += pad > 0 and data.endswith(b"\xff")
            scan += bytes([0xFF, 0xD0 + (k & 7)])
    if info is not None:
        info.update(stuffed_pad=stuffed_pad, maxlen=maxlen, intervals=len(intervals))
    return header(H, W, quality, subsampling, R, tables) + scan + b"\xff\xd9"


def pillow(bgr, quality, subsampling=2, restart_rows=0, restart_blocks=0, optimize=False):
    from PIL import Image, ImageFile
    buf = io.BytesIO()
    more = {}
    if restart_rows:
        more["restart_marker_rows"] = restart_rows
    if restart_blocks:
        more["restart_marker_blocks"] = restart_blocks
    if optimize:
        more["optimize"] = True
        # Pillow gives libjpeg's second pass one output buffer of w * h bytes (2 w h from quality 95); a file larger than that
        # (noise at 4:4:4) fails with "Suspension not allowed here" unless MAXBLOCK, the buffer's lower bound, is raised
        ImageFile.MAXBLOCK = max(ImageFile.MAXBLOCK, bgr.size + 65536)
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1]), "RGB").save(buf, format="JPEG", quality=quality, subsampling=subsampling,
                                                                      **more)
    return buf.getvalue()
