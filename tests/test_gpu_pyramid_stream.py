"""GPU tests of the streaming pyramid pass (k_pyramid_stream, csrc/trl_pyramid.hip) at the edges of its running column sum.

The pass keeps ONE packed 16-bit running sum of the source rows a unit has walked and, per level, the sum's value before the current
bin's first row; a bin's column sums are the difference.  The fields wrap once a unit has walked more than 257 rows of 255s, which is
harmless while no bin is taller than 256 rows.  The cases below make the sum wrap, take snapshots on both sides of a wrap, force
row bands from one per frame down to bands shorter than a bin (trl_debug_option "pyr_row_bands"), and run the wave-local form with its
16-bit strip.  Shapes are the smallest that still have coarse levels (bins wider than 5 px: short side >= 80).  Every level of every
frame, padding included, is compared bit for bit with the oracle's imresample over a poisoned workspace; the plan is asserted, so a
dispatch change cannot silently drop a case."""
import numpy as np
import pytest

from test_gpu_pyramid import check_pixels

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(blob):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from truely_amd.engine import Engine
    e = Engine(blob)
    yield e
    e.close()


def noise(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def run(eng, oracle, frames, bands, kind, n_streamed):
    """One pyramid pass with `bands` forced row bands (0: the pass's policy) over a poisoned workspace, against the oracle."""
    n, H, W, _ = frames.shape
    eng.poison_workspaces(0xFF)
    eng.option("pyr_row_bands", bands)
    try:
        raw, levels = eng.pyramid_batch(frames)
        plan = eng.pyramid_plan()
    finally:
        eng.option("pyr_row_bands", 0)
    streamed = [p for p in plan if p["kernel"] == kind]
    assert len(streamed) == n_streamed and not [p for p in plan if p["kernel"].startswith("S") and p["kernel"] != kind], plan
    if bands:
        rows = -(-H // min(bands, H))
        assert {p["row_bands"] for p in streamed} == {-(-H // rows)}, (bands, plan)      # clamped: every band has a row
    check_pixels(oracle, (H, W, n, 20, 0.709), frames, raw.cpu().numpy(), levels)
    return streamed


@pytest.fixture(scope="module")
def frames_300x96():
    return np.stack([np.full((300, 96, 3), 255, np.uint8), noise(300, 96, 11)])


@pytest.mark.parametrize("bands", [1, 2, 3, 7, 40])
def test_running_sum_wraps_at_every_band_count(eng, oracle, frames_300x96, bands):
    """300 x 96: two levels stream as S4 (bins of 5-6 and 7-8 rows).  One band walks all 300 rows (300 x 255 > 65,535: the running
    sum wraps); 40 forced bands become 38 of 8 rows, about a bin tall: most own one bin start of a level or none, and a band reads
    on past its end for almost as long as it is tall."""
    run(eng, oracle, frames_300x96, bands, "S4", 2)


@pytest.mark.parametrize("bands", [0, 2])
def test_odd_row_pitch_block_wide(eng, oracle, bands):
    """300 x 97: rows of 291 bytes, the byte phase of a row's first dword changes every row.  The noise frame comes last: its last
    rows are the only ones whose lanes move their load window back from the end of the frame buffer and shift the dwords up again
    (k_pyramid_stream: fix_tail), here at a byte phase other than 0."""
    fr = np.stack([np.full((300, 97, 3), 255, np.uint8), noise(300, 97, 12)])
    run(eng, oracle, fr, bands, "S4", 2)


@pytest.mark.parametrize("bands", [0, 1])
@pytest.mark.parametrize("fill", ["255", "noise"])
def test_wave_local_strip(eng, oracle, bands, fill):
    """300 x 1366: the narrowest frame of the wave-local pass, five levels as SW8, through the 16-bit strip; one band walks 300 rows."""
    fr = (np.full((1, 300, 1366, 3), 255, np.uint8) if fill == "255" else noise(300, 1366, 13)[None])
    run(eng, oracle, fr, bands, "SW8", 5)


def test_snapshots_on_both_sides_of_a_wrap(eng, oracle):
    """255 in the top 260 rows, noise below, one band: the sum wraps in row 257; bins start before it, across it and after it."""
    fr = noise(300, 96, 14)
    fr[:260] = 255
    run(eng, oracle, fr[None], 1, "S4", 2)
