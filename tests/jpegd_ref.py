"""The baseline-JPEG decoding rules of csrc/trl_jpegd.hip, restated in numpy (no GPU).

``decode(data)`` gives the BGR frame that ``np.asarray(Image.open(f).convert("RGB"))[:, :, ::-1]`` gives, byte for byte: libjpeg-turbo's
default decompression path (JDCT_ISLOW, fancy upsampling, no merged upsampling, RGB out).

* Markers up to SOS: ``parse`` accepts what the device decoder accepts (SOF0, 8 bit, three components in one interleaved scan,
  luma 2x2 / 2x1 / 1x1 over chroma 1x1, 8-bit DQT, any DHT, any DRI) and raises ``Unsupported`` with a reason for the rest.
* Entropy decoding: 0xFF00 unstuffing, DC prediction per component, reset and byte alignment at each restart, HUFF_EXTEND.  Anything
  irregular (invalid code, a run past coefficient 63, bytes running out, a marker other than the expected one, bytes left over)
  raises ``Irregular``: the decoder never imitates libjpeg's error recovery.
* jidctint.c's jpeg_idct_islow (CONST_BITS 13, PASS1_BITS 2, range limit), jdsample.c's h2v2 / h2v1 fancy upsampling on the
  component's downsampled_width x downsampled_height (plain replication when downsampled_width <= 2, as jinit_upsampler chooses),
  jdcolor.c's 16-bit-fixed YCbCr -> RGB tables.

The IDCT below is int32 arithmetic that wraps and a range-limit mask, which is what the kernel computes and what jidctint.c's C
code computes on a long as long as nothing wraps.  Pillow's libjpeg-turbo runs a SIMD IDCT instead: 16-bit products, 16-bit sums in
front of its multiplies, a saturated 16-bit workspace after pass 1 and a saturated 8-bit result.  The three agree only while no
value reaches a point where one of them wraps or saturates, and a dequantised value inside int16 does not ensure that (a white
frame whose DC quantiser is 8 has a DC of 8128 and an output of 1016 + 128: the mask wraps it, the SIMD code saturates it).  So
``idct_islow`` carries the kernel's gate ("The IDCT gate"), tested on exact values before anything can have
wrapped: in either pass the sums |x0| + |x4|, |x2| + |x6| and |x1| + |x3| + |x5| + |x7| of a column's / row's inputs stay within
32767 (that bounds the dequantised values too), every pass-1 output lies in int16, and every descaled result lies in
[-512, 511], the range the mask leaves alone.  A block outside any of these makes the frame ``Irregular`` here and on the device,
and Pillow decides what that frame is.  No encoder makes such a block from pixels."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
                   47, 55, 62, 63])          # zigzag position -> natural index

# reasons of trl_jpegd_parse (include/truely_hip.h)
OK, R_TRUNCATED, R_NOT_JPEG, R_PROCESS, R_PRECISION, R_COMPONENTS, R_SAMPLING, R_DQT, R_DHT, R_SCAN, R_ADOBE, R_MARKER, R_SIZE = range(13)


class Unsupported(Exception):
    def __init__(self, reason, what=""):
        super().__init__(f"reason {reason} {what}")
        self.reason = reason


class Irregular(Exception):
    pass


def _huff_table(counts, vals, is_dc):
    """(lookup of 65536 entries: (length << 8) | symbol, 0 = invalid code) or Unsupported, as jpeg_make_d_derived_tbl decides."""
    look = np.zeros(65536, np.uint16)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            if code >= (1 << length):
                raise Unsupported(R_DHT, "code overflow")
            if is_dc and vals[k] > 15:
                raise Unsupported(R_DHT, "DC symbol > 15")
            look[code << (16 - length):(code + 1) << (16 - length)] = (length << 8) | vals[k]
            code += 1
            k += 1
        code <<= 1
    return look


def parse(data):
    """Markers up to and including SOS -> dict(H, W, hs, vs, ri, scan, quant[3] (natural order), dc[3], ac[3] (lookups))."""
    n = len(data)
    if n < 4:
        raise Unsupported(R_TRUNCATED)
    if data[0] != 0xFF or data[1] != 0xD8:
        raise Unsupported(R_NOT_JPEG)
    p = 2
    qt, dht, sof, ri = {}, {}, None, 0
    while True:
        if p + 2 > n:
            raise Unsupported(R_TRUNCATED)
        if data[p] != 0xFF:
            raise Unsupported(R_MARKER, "no marker")
        while p < n and data[p] == 0xFF:
            p += 1
        if p >= n:
            raise Unsupported(R_TRUNCATED)
        m = data[p]
        p += 1
        if m in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
            raise Unsupported(R_PROCESS)
        if m not in (0xC0, 0xC4, 0xDB, 0xDD, 0xDA, 0xFE) and not 0xE0 <= m <= 0xEF:
            raise Unsupported(R_MARKER, hex(m))
        if p + 2 > n:
            raise Unsupported(R_TRUNCATED)
        L = (data[p] << 8) | data[p + 1]
        if L < 2:
            raise Unsupported(R_MARKER, "length")
        if p + L > n:
            raise Unsupported(R_TRUNCATED)
        body = data[p + 2:p + L]
        p += L
        if m == 0xEE:
            raise Unsupported(R_ADOBE)
        if m == 0xDB:
            q = 0
            while q < len(body):
                if body[q] >> 4:
                    raise Unsupported(R_DQT, "16-bit")
                if (body[q] & 15) > 3 or q + 65 > len(body):
                    raise Unsupported(R_DQT)
                t = np.zeros(64, np.int32)
                t[ZIGZAG] = np.frombuffer(body[q + 1:q + 65], np.uint8)
                qt[body[q] & 15] = t
                q += 65
        elif m == 0xC4:
            q = 0
            while q < len(body):
                if q + 17 > len(body) or (body[q] >> 4) > 1 or (body[q] & 15) > 3:
                    raise Unsupported(R_DHT)
                counts = list(body[q + 1:q + 17])
                total = sum(counts)
                if total > 256 or q + 17 + total > len(body):
                    raise Unsupported(R_DHT, "too long")
                dht[(body[q] >> 4, body[q] & 15)] = _huff_table(counts, body[q + 17:q + 17 + total], (body[q] >> 4) == 0)
                q += 17 + total
        elif m == 0xDD:
            if len(body) != 2:
                raise Unsupported(R_MARKER, "DRI")
            ri = (body[0] << 8) | body[1]
        elif m == 0xC0:
            if sof is not None or len(body) < 6:
                raise Unsupported(R_MARKER, "SOF")
            if body[0] != 8:
                raise Unsupported(R_PRECISION)
            H, W, nf = (body[1] << 8) | body[2], (body[3] << 8) | body[4], body[5]
            if nf != 3 or len(body) != 6 + 3 * nf:
                raise Unsupported(R_COMPONENTS)
            if H < 1 or W < 1:
                raise Unsupported(R_SIZE)
            comps = [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(3)]
            if bytes(c[0] for c in comps) == b"RGB":
                raise Unsupported(R_COMPONENTS, "RGB ids")
            if (comps[0][1], comps[0][2]) not in ((2, 2), (2, 1), (1, 1)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
                raise Unsupported(R_SAMPLING)
            if any(c[3] > 3 for c in comps):
                raise Unsupported(R_DQT)
            sof = (H, W, comps)
        elif m == 0xDA:
            if sof is None:
                raise Unsupported(R_SCAN, "SOS before SOF")
            H, W, comps = sof
            if len(body) != 10 or body[0] != 3:
                raise Unsupported(R_SCAN, "not one interleaved scan")
            dc, ac, quant = [], [], []
            for i in range(3):
                if body[1 + 2 * i] != comps[i][0]:
                    raise Unsupported(R_SCAN, "component order")
                td, ta = body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15
                if td > 3 or ta > 3 or (0, td) not in dht or (1, ta) not in dht:
                    raise Unsupported(R_DHT, "missing")
                if comps[i][3] not in qt:
                    raise Unsupported(R_DQT, "missing")
                dc.append(dht[(0, td)]); ac.append(dht[(1, ta)]); quant.append(qt[comps[i][3]])
            if tuple(body[7:10]) != (0, 63, 0):
                raise Unsupported(R_SCAN, "spectral selection")
            return dict(H=H, W=W, hs=comps[0][1], vs=comps[0][2], ri=ri, scan=p, quant=quant, dc=dc, ac=ac)


def _decode_segment(data, p, info, mcu0, nmcu, expect, coefs):
    """One restart interval: nmcu MCUs from byte p; the marker 0xFF `expect` must follow.  Returns the marker's position."""
    n = len(data)
    acc, nb, stop = 0, 0, False       # nb bits in acc (a Python int used as a queue)
    hs, vs = info["hs"], info["vs"]
    mcux = (info["W"] + 8 * hs - 1) // (8 * hs)
    pred = [0, 0, 0]
    for m in range(mcu0, mcu0 + nmcu):
        my, mx = divmod(m, mcux)
        for c in range(3):
            ch, cv = (hs, vs) if c == 0 else (1, 1)
            for v in range(cv):
                for h in range(ch):
                    blk = coefs[c][my * cv + v, mx * ch + h]
                    k = 0
                    while k < 64:
                        while nb <= 48 and not stop:
                            if p >= n:
                                stop = True
                            elif data[p] != 0xFF:
                                acc = (acc << 8) | data[p]; nb += 8; p += 1
                            elif p + 1 < n and data[p + 1] == 0:
                                acc = (acc << 8) | 0xFF; nb += 8; p += 2
                            else:
                                stop = True
                        peek = ((acc << 16) >> nb) & 0xFFFF if nb else 0
                        e = int((info["dc"] if k == 0 else info["ac"])[c][peek])
                        ln, sym = e >> 8, e & 255
                        if e == 0 or ln > nb:
                            raise Irregular("invalid code or out of bytes")
                        nb -= ln
                        r, s = (0, sym) if k == 0 else (sym >> 4, sym & 15)
                        if s > nb:
                            raise Irregular("out of bytes")
                        val = 0
                        if s:
                            nb -= s
                            val = (acc >> nb) & ((1 << s) - 1)
                            if val < (1 << (s - 1)):
                                val += 1 - (1 << s)
                        acc &= (1 << nb) - 1
                        if k == 0:
                            pred[c] += val
                            blk[0] = np.int32(pred[c]).astype(np.int16)
                            k = 1
                        elif s:
                            k += r
                            if k > 63:
                                raise Irregular("run past 63")
                            blk[ZIGZAG[k]] = val
                            k += 1
                        elif r == 15:
                            k += 16
                            if k > 63:
                                raise Irregular("run past 63")
                        else:
                            break
    if nb >= 8:
        raise Irregular("bytes left over")
    if p + 1 >= n or data[p] != 0xFF or data[p + 1] != expect:
        raise Irregular("unexpected marker")
    return p


def entropy_decode(data, info):
    hs, vs = info["hs"], info["vs"]
    mcux = (info["W"] + 8 * hs - 1) // (8 * hs)
    mcuy = (info["H"] + 8 * vs - 1) // (8 * vs)
    coefs = [np.zeros((mcuy * vs, mcux * hs, 64), np.int16), np.zeros((mcuy, mcux, 64), np.int16), np.zeros((mcuy, mcux, 64), np.int16)]
    total = mcux * mcuy
    ri = info["ri"] or total
    p, k = info["scan"], 0
    for m0 in range(0, total, ri):
        cnt = min(ri, total - m0)
        last = m0 + cnt == total
        p = _decode_segment(data, p, info, m0, cnt, 0xD9 if last else 0xD0 + (k & 7), coefs) + 2
        k += 1
    return coefs


def _mul(a, c):
    return a * np.int32(c)


def _idct_1d(x, shift):
    """jpeg_idct_islow's butterfly on axis 0 of x (8, ...), int32 that wraps."""
    z2, z3 = x[2], x[6]
    z1 = _mul(z2 + z3, 4433)
    tmp2 = z1 + _mul(z3, -15137)
    tmp3 = z1 + _mul(z2, 6270)
    tmp0 = (x[0] + x[4]) << 13
    tmp1 = (x[0] - x[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = _mul(z3 + z4, 9633)
    tmp0, tmp1, tmp2, tmp3 = _mul(tmp0, 2446), _mul(tmp1, 16819), _mul(tmp2, 25172), _mul(tmp3, 12299)
    z1, z2, z3, z4 = _mul(z1, -7373), _mul(z2, -20995), _mul(z3, -16069) + z5, _mul(z4, -3196) + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    rnd = np.int32(1 << (shift - 1))
    out = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
    return np.stack([(o + rnd) >> shift for o in out])


def _pass_wide(x):
    """The kernel's jd_pass_wide on axis 0 of x (8, ...): a 16-bit sum in front of a multiply may leave int16."""
    a = np.abs(x)
    return bool(((a[0] + a[4] > 32767) | (a[2] + a[6] > 32767) | (a[1] + a[3] + a[5] + a[7] > 32767)).any())


def idct_islow(coef, quant, gate=True):
    """(by, bx, 64) int16 natural order, quant (64,) -> u8 plane (by*8, bx*8).  gate=False: the arithmetic alone, as it was before
    the gate (for counting what the gate turns away)."""
    by, bx = coef.shape[:2]
    v = coef.astype(np.int32) * quant.astype(np.int32)                # |int16 x u8| < 2^23: exact
    with np.errstate(over="ignore"):
        x = np.moveaxis(v.reshape(by, bx, 8, 8), 2, 0)                # [row, by, bx, col]: columns are transformed first
        if gate and _pass_wide(x):
            raise Irregular("pass 1: a 16-bit input sum outside int16")
        ws = _idct_1d(x, 11)                                          # (8 rows, by, bx, col)
        if gate and ((ws < -32768) | (ws > 32767)).any():
            raise Irregular("pass 1: workspace outside int16")
        x = np.moveaxis(ws, 3, 0)                                     # [col, row, by, bx]
        if gate and _pass_wide(x):
            raise Irregular("pass 2: a 16-bit input sum outside int16")
        out = _idct_1d(x, 18)                                         # (8 cols, 8 rows, by, bx)
    if gate and ((out < -512) | (out > 511)).any():
        raise Irregular("descaled value outside [-512, 511]")
    s = out & 1023
    s = np.where(s >= 512, s - 1024, s)
    px = np.clip(s + 128, 0, 255).astype(np.uint8)                    # [col, row, by, bx]
    return px.transpose(2, 1, 3, 0).reshape(by * 8, bx * 8)


def upsample_h2v2(P, dw, dh):
    """jdsample.c h2v2_fancy_upsample on the component's dw x dh samples -> (2*dh, 2*dw)."""
    P = P[:dh].astype(np.int32)
    if dw <= 2:
        return np.repeat(np.repeat(P[:, :dw], 2, 0), 2, 1)
    up = np.concatenate([P[:1], P[:-1]]); dn = np.concatenate([P[1:], P[-1:]])
    out = np.zeros((2 * dh, 2 * dw), np.int32)
    for v, other in ((0, up), (1, dn)):
        s = 3 * P + other                                             # column sums, all padded columns
        this, left = s[:, :dw], np.concatenate([s[:, :1], s[:, :dw - 1]], 1)
        right = np.concatenate([s[:, 1:dw], s[:, dw - 1:dw]], 1)
        ev = (this * 3 + left + 8) >> 4
        od = (this * 3 + right + 7) >> 4
        ev[:, 0] = (this[:, 0] * 4 + 8) >> 4
        od[:, dw - 1] = (this[:, dw - 1] * 4 + 7) >> 4
        out[v::2, 0::2] = ev
        out[v::2, 1::2] = od
    return out


def upsample_h2v1(P, dw, dh):
    P = P[:dh].astype(np.int32)
    if dw <= 2:
        return np.repeat(P[:, :dw], 2, 1)
    this = P[:, :dw]
    left = np.concatenate([this[:, :1], this[:, :-1]], 1)
    right = np.concatenate([this[:, 1:], this[:, -1:]], 1)
    ev = (3 * this + left + 1) >> 2
    od = (3 * this + right + 2) >> 2
    ev[:, 0] = this[:, 0]
    od[:, -1] = this[:, -1]
    out = np.zeros((dh, 2 * dw), np.int32)
    out[:, 0::2] = ev
    out[:, 1::2] = od
    return out


def _fix(x):
    return int(x * 65536 + 0.5)


def color_bgr(y, cb, cr):
    y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((_fix(1.40200) * cr + 32768) >> 16)
    g = y + ((-_fix(0.34414) * cb + 32768 - _fix(0.71414) * cr) >> 16)
    b = y + ((_fix(1.77200) * cb + 32768) >> 16)
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def decode(data, gate=True):
    """A JPEG file -> BGR u8 (H, W, 3); Unsupported / Irregular where the device decoder reports status 1 / 2."""
    info = parse(data)
    H, W, hs, vs = info["H"], info["W"], info["hs"], info["vs"]
    coefs = entropy_decode(data, info)
    planes = [idct_islow(coefs[c], info["quant"][c], gate) for c in range(3)]
    dw, dh = (W + hs - 1) // hs, (H + vs - 1) // vs
    if (hs, vs) == (2, 2):
        cb, cr = (upsample_h2v2(planes[c], dw, dh) for c in (1, 2))
    elif (hs, vs) == (2, 1):
        cb, cr = (upsample_h2v1(planes[c], dw, dh) for c in (1, 2))
    else:
        cb, cr = planes[1], planes[2]
    return color_bgr(planes[0][:H, :W], cb[:H, :W], cr[:H, :W])
