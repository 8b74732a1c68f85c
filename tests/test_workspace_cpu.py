"""The embedder's activation workspace, restated on the CPU from the walk's allocation rule -- the independent reference of
tests/test_gpu_workspace.py, which asks the library (whose sizes are dry runs of its own carving code) for the same numbers.

The rule: the walk takes one block per activation it materialises, n * h * w * c * element size + 64 bytes, each on a 256-byte
boundary, in walk order.  A conv whose output is a channel slice of a concat buffer takes none; the concat buffer is taken when its
block starts.  Built on facenet_geometry() (tests/test_facenet_sizes_cpu.py), which is checked against torch's module shapes."""
import pytest

from test_facenet_sizes_cpu import _out, facenet_geometry

# convs that write a channel slice of their block's concat buffer (trl_nets.hip: the `into` destinations)
_INTO = {"repeat_1": ("fused", "branch1.1", "branch2.2"), "repeat_2": ("fused", "branch1.2"), "repeat_3": ("fused", "branch1.2"),
         "block8": ("fused", "branch1.2"), "mixed_6a": ("branch0", "branch1.2"), "mixed_7a": ("branch0.1", "branch1.1", "branch2.2")}
_CONCAT = {"repeat_2": 256, "repeat_3": 384, "block8": 384}
GROUPED_MAX_ROWS = 16384          # block35_grouped: f32, faces x map pixels of the block35 map up to this


def _split(name):
    """'repeat_1.3.branch2.1' -> ('repeat_1', 'branch2.1'); 'mixed_6a.branch0' -> ('mixed_6a', 'branch0'); 'conv2d_2a' -> ('conv2d_2a', '')"""
    parts = name.split(".")
    return parts[0], ".".join(parts[2:] if parts[0].startswith("repeat_") else parts[1:])


def block35_grouped(n, h, w, es=4, no_fnconv=False):
    r = [q for q in facenet_geometry(h, w) if q.layer == "facenet.conv2d_4b"][0]
    return es == 4 and not no_fnconv and n * r.OH * r.OW <= GROUPED_MAX_ROWS


def embedder_bytes(n, h, w, es=4, no_fnconv=False, guard=0):
    """Bytes the embedder's walk takes for n faces of h x w: es = 4 (f32) or 2 (bf16 / fp16: every activation behind the stem conv).
    guard: the red zone behind every block (csrc/trl_arena.h; 0 = off, the shipped library)."""
    rows = facenet_geometry(h, w)
    geo = {r.layer[len("facenet."):]: r for r in rows}
    grouped = block35_grouped(n, h, w, es, no_fnconv)
    off = 0

    def block(H, W, c, e):
        nonlocal off
        off = (off + 255) // 256 * 256 + n * H * W * c * e + 64 + guard

    for r in rows:
        name = r.layer[len("facenet."):]
        blk, leaf = _split(name)
        if name == "conv2d_1a":                               # the stem runs in f32; a 16-bit copy follows
            block(r.OH, r.OW, r.cout, 4)
            if es == 2:
                block(r.OH, r.OW, r.cout, 2)
            continue
        if name == "last_linear":                             # avgpool_1a's output (a 1x1 f32 map is its own average), then the linear
            b8 = geo["block8.conv2d"]
            if not (es == 4 and b8.OH * b8.OW == 1):
                block(1, 1, b8.cout, 4)
            block(1, 1, r.cout, 4)
            continue
        if leaf == "fused" and blk == "repeat_1":             # [branch0 | branch1 | branch2], + a free slot in the grouped form
            block(r.OH, r.OW, 128 if grouped else 96, es)
        elif leaf == "fused" and blk in _CONCAT:
            block(r.OH, r.OW, _CONCAT[blk], es)
        elif name == "mixed_6a.branch0":
            block(r.OH, r.OW, 896, es)
        elif name == "mixed_7a.fused":
            q = geo["mixed_7a.branch0.1"]
            block(q.OH, q.OW, 1792, es)
        if leaf in _INTO.get(blk, ()):
            continue
        block(r.OH, r.OW, r.cout, es)
        if name == "conv2d_2b":                               # maxpool_3a
            block(_out(r.OH, 3, 2, 0), _out(r.OW, 3, 2, 0), r.cout, es)
    return off


def old_formula(n, h, w):
    """The per-face budget rule n (h w 110 + 400000) 4 + 8 MiB (tests/test_gpu_embedder_sizes.py chooses its cases by it), and a
    block of that size with the head-room trl_ensure adds on a grow."""
    f = n * (h * w * 110 + 400000) * 4 + (8 << 20)
    return f, f + f // 8 + (32 << 20)


def test_restatement_gives_the_recorded_sizes():
    assert embedder_bytes(2048, 80, 80) == 4_508_372_032
    assert embedder_bytes(1, 75, 75) == 2_132_544
    assert embedder_bytes(24, 300, 300) == 1_241_926_464


def test_the_old_formula_was_no_bound():
    """The walk's need is not a multiple of h x w per face: 24 faces of 300 x 300 need more than the budget rule with trl_ensure's
    head-room on top, 64 of 224 x 224 more than the rule, 2048 of 80 x 80 less than half of it.  Only a count of the walk sizes it."""
    assert embedder_bytes(24, 300, 300) > old_formula(24, 300, 300)[1]
    assert old_formula(2048, 80, 80)[0] > 2 * embedder_bytes(2048, 80, 80)
    assert embedder_bytes(64, 224, 224) > old_formula(64, 224, 224)[0]


def test_block35_threshold_and_concat_width():
    """334 / 335 faces of 75 x 75 (7 x 7 block35 maps) lie on the two sides of the grouped form; its concat buffer is 128 wide, not
    96: five blocks of n * 49 * 32 * 4 bytes more (the 256-byte rounding aside)."""
    assert block35_grouped(334, 75, 75) and not block35_grouped(335, 75, 75)
    assert not block35_grouped(1, 75, 75, es=2) and not block35_grouped(1, 75, 75, no_fnconv=True)
    d = embedder_bytes(1, 75, 75) - embedder_bytes(1, 75, 75, no_fnconv=True)
    assert abs(d - 5 * 49 * 32 * 4) < 5 * 256


@pytest.mark.parametrize("n,h,w", [(1, 75, 75), (3, 160, 160), (2, 75, 107)], ids=str)
def test_16_bit_walk_is_smaller_but_keeps_the_f32_ends(n, h, w):
    """The 16-bit walk halves every activation but the stem's f32 output and the f32 tail (average pool, linear), and adds the
    stem's 16-bit copy."""
    f32, lo = embedder_bytes(n, h, w, 4, no_fnconv=True), embedder_bytes(n, h, w, 2)
    stem = facenet_geometry(h, w)[0]
    assert f32 // 2 < lo < f32 // 2 + n * stem.OH * stem.OW * 32 * 4 + n * (1792 + 512) * 4 + 80 * 256
