"""PReLU slope classes of the seeded weights, shared by the GPU and CPU tests that run every kernel instantiation the slopes select."""
import numpy as np


def slope_variant_blob(variant):
    from truely_amd import weights
    sds = [dict(sd) for sd in weights.synthetic_state_dicts(0)]
    if variant == "generalise_prelu":                           # what bench.py --prelu general runs
        weights.generalise_prelu(sds)
        return weights.pack_state_dicts(*sds)
    for net, keys in ((sds[0], ("prelu1.weight", "prelu2.weight", "prelu3.weight")), (sds[1], ("prelu1.weight",)),
                      (sds[2], ("prelu1.weight",))):          # PNet (fused kernel) and the R-/O-Net front kernels
        for key in keys:
            w = np.array(net[key], np.float32, copy=True)
            if variant == "slopes_above_one":                   # k_pnet_fused<false, false>, front MODE 1
                w[::2] = 1.25
            elif variant == "negative_slopes":                  # all <= 1, some negative: k_pnet_fused<true, true>, front MODE 0
                w[1::3] = -0.2
            elif variant == "mixed_signs":                      # every class in one layer: k_pnet_fused<false, true>, front MODE 0
                w[0::4] = 1.5; w[1::4] = -0.35; w[2::4] = 0.0; w[3::4] = 1.0
            elif variant == "negative_deep_only":               # conv1 slopes stay in [0, 1]: k_pnet_fused<true, false> with negative conv2/3 slopes
                if key != "prelu1.weight":
                    w[::2] = -0.15
            net[key] = w
    return weights.pack_state_dicts(*sds)
