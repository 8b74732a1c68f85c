"""CPU audit of the fused PNet kernel's fp16 screen ("conv3 screened on the fp16 matrix cores").

The fused kernel computes conv3 (3x3, 16 -> 32) of every 32-cell M-tile (2 output rows x 16 columns of a 16 x 16-cell tile)
first with fp16 operands, and recomputes the M-tile with the exact f32 chain only when some valid cell could pass the threshold:

    d_screen + E >= dthr,   E = sum over the cell's 3 x 3 x 16 conv2 inputs of ghat[channel] * |x| + B,

ghat and B the error bound of the screened logit difference (screen_weights below; the library computes the same in
trl_pnet_prepare).  The rule it replaced was E = A * X_cell + B, X_cell = max |conv2 activation| over the same receptive field
(screen_bound; the library still reports A).  This tool estimates, on the CPU, the share of M-tiles the screen confirms for the
seeded weights and the clips bench.py builds for configs 0, 1, 2 and 4: it evaluates PNet in float32 with torch (the pyramid by
adaptive average pooling), takes d = logit1 - logit0 of every cell and counts the M-tiles with some valid cell at d + E >= dthr,
under the kernel's rule (confirmed_share) and the replaced one (confirmed_share_max_rule).  The E = 0 column is the kernel's older
prefilter alone.

    python tools/pnet_screen_audit.py [--frames 8] [--out profiles/pnet_screen_audit.json]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

U32 = 2.0 ** -24      # f32 unit roundoff
U16 = 2.0 ** -11      # fp16 unit roundoff
TINY16 = 2.0 ** -14   # smallest normal fp16: absolute operand error of a subnormal kept or flushed
FP16_MAX = 65504.0


def _gamma(n, u=U32):
    return n * u / (1.0 - n * u)


def screen_bound(t):
    """(A, B, ok): |d_screen - d_exact| <= A * X + B for every cell whose conv2 inputs satisfy |x| <= X <= 65504.

    t: canonical PNet tensors (weights.unpack_tensors).  Float64 throughout, A and B rounded up to float32.  ok = False when a
    conv3 weight does not fit fp16 (the screen is then off)."""
    w3 = t["pnet.conv3.w"].astype(np.float64)            # [144][32]
    b3 = t["pnet.conv3.b"].astype(np.float64)
    s3 = t["pnet.prelu3"].astype(np.float64)
    wl = t["pnet.conv4_1.w"].astype(np.float64)          # [32][2]
    bl = t["pnet.conv4_1.b"].astype(np.float64)
    if not np.all(np.abs(w3) <= FP16_MAX):
        return math.inf, math.inf, False
    aw = np.abs(w3)
    h = w3.astype(np.float32).astype(np.float16).astype(np.float64)
    dw = np.where(aw < TINY16, aw, np.abs(h - w3))      # per-weight rounding error (flushed subnormals: the whole weight)
    W1, D = aw.sum(0), dw.sum(0)
    ge, gs = _gamma(145), _gamma(145, 2 * U32)          # exact fmaf chain; MFMA sum in any order, roundings of up to 2u
    # conv3 output c: |v_screen - v_exact| <= a3 X + b3e
    a3 = D * (1 + U16) + W1 * U16 + gs * (W1 + D) * (1 + U16) + ge * W1
    b3e = D * TINY16 + W1 * TINY16 + gs * (np.abs(b3) + (W1 + D) * TINY16) + ge * np.abs(b3)
    # |v_exact| <= aM X + bM; PReLU is Lipschitz with L = max(1, |slope|); both sides round s * v once
    aM, bM = W1 * (1 + ge), np.abs(b3) * (1 + ge)
    L = np.maximum(1.0, np.abs(s3))
    ap = L * (1 + U32) * a3 + 2 * U32 * L * aM          # |p_screen - p_exact| <= ap X + bp
    bp = L * (1 + U32) * b3e + 2 * U32 * L * bM
    aP, bP = L * (1 + U32) * aM, L * (1 + U32) * bM     # |p_exact| <= aP X + bP
    # exact heads: two fmaf chains of 33 terms, then logit1 - logit0 in f32
    S_a = (np.abs(wl[:, 0]) + np.abs(wl[:, 1])) @ aP
    S_b = abs(bl[0]) + abs(bl[1]) + (np.abs(wl[:, 0]) + np.abs(wl[:, 1])) @ bP
    ae, be = _gamma(35) * S_a, _gamma(35) * S_b
    # screened difference head: wd = f32(w1 - w0) (one rounding), a 16-term chain per half, the halves and the bias added
    wd = np.abs(wl[:, 1] - wl[:, 0])
    bd = abs(bl[1] - bl[0])
    ad = wd @ ap + _gamma(36) * (1 + U32) * (wd @ (aP + ap))
    bdd = wd @ bp + _gamma(36) * (1 + U32) * (bd + wd @ (bP + bp))
    A, B = (ae + ad) * (1 + 2.0 ** -10), (be + bdd) * (1 + 2.0 ** -10)
    up = lambda v: float(np.nextafter(np.float32(v), np.float32(np.inf))) if np.float32(v) < v else float(np.float32(v))
    return up(A), up(B), True


def screen_weights(t):
    """(g [9][16], ghat [16], B, ok): the same bound with A's terms kept per input k = (tap, channel),

        |d_screen - d_exact| <= sum_k g_k |x_k| + B,   sum_k g_k = A (before A's inflation),

    every term of A in screen_bound being a sum over k of a non-negative coefficient times the bound X of |x_k|.  ghat[channel] =
    max over the nine taps of g, multiplied by 1 + 2^-10 and rounded up to float32 like A and B: the weights the kernel applies
    (one number per conv2 cell and channel half, nine cells added).  The factor also covers the kernel's f32 roundings of its sum:
    at most 18 per term (8 fmaf of a cell half, 8 additions over the taps, the two halves, + B), all on non-negative terms.
    g is returned without the inflation (float64)."""
    w3 = t["pnet.conv3.w"].astype(np.float64)
    s3 = t["pnet.prelu3"].astype(np.float64)
    wl = t["pnet.conv4_1.w"].astype(np.float64)
    _A, B, ok = screen_bound(t)
    if not ok:
        return np.full((9, 16), math.inf), [math.inf] * 16, B, False
    aw = np.abs(w3)                                      # [144][32]: the per-input (|w_k|, D_k) in place of (W1, D)
    h = w3.astype(np.float32).astype(np.float16).astype(np.float64)
    dw = np.where(aw < TINY16, aw, np.abs(h - w3))
    ge, gs = _gamma(145), _gamma(145, 2 * U32)
    a3 = dw * (1 + U16) + aw * U16 + gs * (aw + dw) * (1 + U16) + ge * aw
    aM = aw * (1 + ge)
    L = np.maximum(1.0, np.abs(s3))
    ap = L * (1 + U32) * a3 + 2 * U32 * L * aM
    aP = L * (1 + U32) * aM
    wd = np.abs(wl[:, 1] - wl[:, 0])
    g = _gamma(35) * (aP @ (np.abs(wl[:, 0]) + np.abs(wl[:, 1]))) + ap @ wd + _gamma(36) * (1 + U32) * ((aP + ap) @ wd)
    g = g.reshape(9, 16)
    up = lambda v: float(np.nextafter(np.float32(v), np.float32(np.inf))) if np.float32(v) < v else float(np.float32(v))
    return g, [up(v * (1 + 2.0 ** -10)) for v in g.max(0)], B, True


def pnet_maps(lvl, t, ghat=None):
    """float32 PNet of one level [h][w][3] -> (d = logit1 - logit0 [oh][ow], X_cell [oh][ow]) and, given ghat, the per-input error
    sum of every cell, sum over its 3 x 3 x 16 conv2 inputs of ghat[channel] |x|, as a third map."""
    import torch
    import torch.nn.functional as F

    def conv(x, w, b, cin):
        co = w.shape[1]
        wt = torch.from_numpy(w.reshape(3, 3, cin, co).transpose(3, 2, 0, 1).copy())
        return F.conv2d(x, wt, torch.from_numpy(b))

    def prelu(x, s):
        s = torch.from_numpy(s).view(1, -1, 1, 1)
        return torch.where(x >= 0, x, x * s)

    x = torch.from_numpy(np.ascontiguousarray(lvl.transpose(2, 0, 1)))[None]
    y = prelu(conv(x, t["pnet.conv1.w"], t["pnet.conv1.b"], 3), t["pnet.prelu1"])
    y = F.max_pool2d(y, 2, 2, ceil_mode=True)
    a2 = prelu(conv(y, t["pnet.conv2.w"], t["pnet.conv2.b"], 10), t["pnet.prelu2"])
    y = prelu(conv(a2, t["pnet.conv3.w"], t["pnet.conv3.b"], 16), t["pnet.prelu3"])
    wl = torch.from_numpy(t["pnet.conv4_1.w"].T.copy())[:, :, None, None]
    lg = F.conv2d(y, wl, torch.from_numpy(t["pnet.conv4_1.b"]))[0]
    X = F.max_pool2d(a2.abs().amax(1, keepdim=True), 3, 1)[0, 0]
    if ghat is None:
        return (lg[1] - lg[0]).numpy(), X.numpy()
    m = (a2.abs().double() * torch.tensor(ghat, dtype=torch.float64).view(1, -1, 1, 1)).sum(1, keepdim=True)
    return (lg[1] - lg[0]).numpy(), X.numpy(), (9.0 * F.avg_pool2d(m, 3, 1))[0, 0].numpy()


def mtile_hits(ok):
    """ok [oh][ow] bool -> (M-tiles holding a valid cell, M-tiles with some ok cell): 16 x 16 tiles, 2-row M-tiles."""
    oh, ow = ok.shape
    ty, tx = (oh + 15) // 16, (ow + 15) // 16
    p = np.zeros((ty * 16, tx * 16), bool)
    p[:oh, :ow] = ok
    v = np.zeros_like(p)
    v[:oh, :ow] = True
    hit = p.reshape(ty * 8, 2, tx, 16).any(axis=(1, 3))
    val = v.reshape(ty * 8, 2, tx, 16).any(axis=(1, 3))
    return int(val.sum()), int(hit.sum())


def audit(cfg_id, frames, t, A, B, ghat, thr=0.6):
    import torch
    import torch.nn.functional as F
    import bench
    from oracle.oracle import Oracle
    from truely_amd import weights

    cfg = bench.CONFIGS[cfg_id]
    clip = bench.make_clip(cfg, min(frames, cfg["batch"]), seed=0)
    orc = Oracle(weights.pack_tensors(t))
    dthr = math.log(thr / (1 - thr)) - 0.05
    tot = hit_s = hit_m = hit_0 = cells = 0
    for f in clip:
        src = torch.from_numpy(f.astype(np.float32).transpose(2, 0, 1).copy())[None]
        for _s, h, w in orc.scales(cfg["H"], cfg["W"], cfg["min_face"], 0.709):
            lvl = ((F.adaptive_avg_pool2d(src, (h, w))[0] - 127.5) * 0.0078125).permute(1, 2, 0).contiguous().numpy()
            d, X, S = pnet_maps(lvl, t, ghat)
            n, k = mtile_hits(d + (S + B) >= dthr)           # the kernel's rule: per-input weights
            _, kx = mtile_hits(d + (A * X + B) >= dthr)      # the rule it replaced: E = A X + B
            _, k0 = mtile_hits(d >= dthr)
            tot += n; hit_s += k; hit_m += kx; hit_0 += k0; cells += int((d + (S + B) >= dthr).sum())
    return dict(config=cfg_id, frames=len(clip), shape=[cfg["H"], cfg["W"]], min_face=cfg["min_face"], mtiles=tot,
                confirmed_screen=hit_s, confirmed_share=hit_s / tot, confirmed_max_rule=hit_m, confirmed_share_max_rule=hit_m / tot,
                flagged_cells=cells, prefilter_only=hit_0, prefilter_share=hit_0 / tot)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=8, help="frames of each config's clip (from its start)")
    ap.add_argument("--configs", default="1,0,2,4")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from truely_amd import weights
    t = weights.unpack_tensors(weights.synthetic_blob(0))
    A, B, ok = screen_bound(t)
    _g, ghat, _B, _ok = screen_weights(t)
    res = dict(A=A, B=B, ghat=ghat, screen_on=ok, dthr_thr0_0p6=math.log(1.5) - 0.05, results=[])
    for c in (int(v) for v in args.configs.split(",")):
        r = audit(c, args.frames, t, A, B, ghat)
        print(json.dumps(r), flush=True)
        res["results"].append(r)
    print(f"A = {A:.6g}  B = {B:.6g}")
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
