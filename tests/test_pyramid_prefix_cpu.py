"""The streaming pyramid pass (k_pyramid_stream) keeps one running column sum per byte column in a 16-bit field that wraps, and
takes a bin's column sum as the difference of the running sum after the bin's last row and before its first, modulo 2^16.  A numpy
uint16 restatement: the difference is the true sum for every bin of at most 256 rows wherever it starts, and no longer at 258 rows
of 255s -- the precondition launch_coarse enforces (khmax <= 256; 257 x 255 = 65,535 still fits)."""
import numpy as np

ROWS = 600


def wrapped_prefix(col):
    """P[y] = sum of rows [0, y) in a 16-bit field, as v_pk_add_u16 leaves it."""
    p = np.zeros(len(col) + 1, np.uint16)
    p[1:] = np.cumsum(col.astype(np.uint64)).astype(np.uint16)          # the low 16 bits of the true sum
    return p


def bin_sums(p, kh):
    """P[s + kh] - P[s] in 16-bit arithmetic for every start row s."""
    return (p[kh:] - p[:-kh]).astype(np.uint16)


def test_wrapped_difference_is_exact_up_to_256_rows():
    cols = [np.full(ROWS, 255, np.uint8), np.random.default_rng(5).integers(0, 256, ROWS, dtype=np.uint8)]
    for col in cols:
        p = wrapped_prefix(col)
        assert int(p.max()) < 65536 and np.cumsum(col.astype(np.int64))[-1] > 65535          # the walk does wrap
        true = np.concatenate([[0], np.cumsum(col.astype(np.int64))])
        for kh in range(1, 257):
            assert np.array_equal(bin_sums(p, kh).astype(np.int64), true[kh:] - true[:-kh]), kh


def test_wrapped_difference_fails_at_258_rows_of_255():
    p = wrapped_prefix(np.full(ROWS, 255, np.uint8))
    assert (bin_sums(p, 257) == 257 * 255).all()                           # 65,535: the last sum a field holds
    got = bin_sums(p, 258).astype(np.int64)
    assert (got != 258 * 255).all() and (got == 258 * 255 - 65536).all()
