"""The workspace allocator (csrc/trl_arena.h) and its red zones, without a GPU.

``tests/arena_sim.cpp`` includes the header alone (it is plain C++17, no HIP) and is built for the host like
``tests/capacity_sim.cpp``: with ``-fsanitize=address,undefined`` where the toolchain links it, else without.  It runs scripts of
``alloc n / reset / rewind k / counter / blocks`` and prints what the arena did; ``Model`` below restates the rule:

  a block starts at the next multiple of 256 at or behind ``off``; ``off`` then moves to its end plus the guard; ``high`` is the
  largest ``off`` seen; a real arena hands out nothing (and changes nothing) when the block and its guard do not fit its capacity;
  a rewind moves ``off`` back and forgets the blocks that start at or behind the mark.

With guard 0 that is the allocator the library has always had: ``off = align256(off) + bytes``."""
import os
import random
import shutil
import subprocess

import pytest

from truely_amd import jpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(jpeg.__file__), "csrc")
GUARDS = (0, 256, 4096, 65536)
SIZES = (0, 1, 255, 256, 257, 3 << 30, (5 << 30) + 1)


@pytest.fixture(scope="module")
def sim_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("arena_sim") / "arena_sim")
    base = [cxx, "-O1", "-g", "-std=c++17", "-I", CSRC, os.path.join(ROOT, "tests", "arena_sim.cpp"), "-o", out]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(base + san, capture_output=True, text=True).returncode != 0:
        subprocess.run(base, check=True)
    return out


def test_the_header_is_plain_cpp():
    with open(os.path.join(CSRC, "trl_arena.h")) as f:
        src = f.read()
    includes = [ln.split()[1] for ln in src.split("\n") if ln.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes)
    with open(os.path.join(CSRC, "trl_common.h")) as f:
        common = f.read()
    assert '#include "trl_arena.h"' in common and "struct Arena {" not in common


class Model:
    def __init__(self, guard, cap=None):
        self.guard, self.cap, self.off, self.high, self.blocks, self.marks = guard, cap, 0, 0, [], [0]

    def alloc(self, n):
        a = (self.off + 255) // 256 * 256
        if self.cap is not None and a + n + self.guard > self.cap:
            self.marks.append(self.off)
            return None
        self.off = a + n + self.guard
        self.high = max(self.high, self.off)
        self.blocks.append((a, n))
        self.marks.append(self.off)
        return a

    def rewind(self, k):
        mark = self.marks[k]
        self.blocks = [b for b in self.blocks if b[0] < mark]
        del self.marks[k + 1:]
        self.off = mark


def run(program, guard, cap, script):
    """-> the output lines of arena_sim for ``script`` (a list of op strings)"""
    p = subprocess.run([program, str(guard), "count" if cap is None else str(cap)], input="\n".join(script) + "\n", capture_output=True,
                       text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    return p.stdout.split("\n")[:-1]


def random_script(rng, steps):
    script = []
    allocs = 0
    for _ in range(steps):
        r = rng.random()
        if r < 0.08:
            script.append("reset")
            allocs = 0
        elif r < 0.2 and allocs:
            k = rng.randrange(allocs + 1)
            script.append(f"rewind {k}")
            allocs = k
        else:
            n = rng.choice(SIZES) if rng.random() < 0.7 else rng.randrange(1, 1 << 20)
            script.append(f"alloc {n}")
            allocs += 1
        if rng.random() < 0.3:
            script.append("blocks")
    script.append("blocks")
    return script


def replay(script, guard, cap, lines, recording):
    """Checks every output line of a script against the model; -> (model, offsets of the allocs)"""
    m = Model(guard, cap)
    offs = []
    it = iter(lines)
    for op in script:
        word, _, arg = op.partition(" ")
        if word == "alloc":
            a = m.alloc(int(arg))
            offs.append(a)
            want = "null" if a is None else ("count" if cap is None else str(a))
            assert next(it) == f"a {want} {m.off} {m.high}", op
        elif word in ("reset", "rewind"):
            k = 0 if word == "reset" else int(arg)
            if recording:                     # the callback runs before the offset moves and sees the blocks of the old layout
                assert next(it) == f"w {m.marks[k]} {word} {len(m.blocks)}"
            m.rewind(k)
            assert next(it) == f"r {m.off} {m.high}"
        elif word == "blocks":
            rec = m.blocks if recording else []
            assert next(it) == " ".join([f"b {len(rec)}"] + [f"{o}:{n}" for o, n in rec])
    assert next(it, None) is None
    return m, offs


@pytest.mark.parametrize("guard", GUARDS)
def test_random_scripts_follow_the_rule(sim_program, guard):
    """Sizes 0, 1, 255, 256, 257 and multi-GiB, resets and partial rewinds: offsets, off, high and the recorded blocks.  The real
    arena is given exactly the capacity the counting one counted, so it never returns null and carves the same offsets."""
    rng = random.Random(1000 + guard)
    for _ in range(12):
        script = random_script(rng, 60)
        counted, offs_c = replay(script, guard, None, run(sim_program, guard, None, script), recording=False)
        real, offs_r = replay(script, guard, counted.high, run(sim_program, guard, counted.high, script), recording=guard != 0)
        assert offs_c == offs_r and None not in offs_r
        assert (real.off, real.high) == (counted.off, counted.high)
        # every gap between consecutive live blocks: >= guard, < guard + 256; blocks start on 256-byte boundaries
        blocks = real.blocks
        assert all(o % 256 == 0 for o, _ in blocks)
        for (o0, n0), (o1, _) in zip(blocks, blocks[1:]):
            assert guard <= o1 - (o0 + n0) < guard + 256
        if blocks:                            # ... and the last block's guard lies inside what was counted
            assert real.off - (blocks[-1][0] + blocks[-1][1]) == guard


@pytest.mark.parametrize("guard", GUARDS)
def test_one_byte_short_fails_exactly_at_the_block_that_does_not_fit(sim_program, guard):
    rng = random.Random(2000 + guard)
    for _ in range(8):
        script = ["alloc 1000"] + [f"alloc {rng.choice(SIZES[:5]) if rng.random() < 0.6 else rng.randrange(1, 1 << 16)}" for _ in range(rng.randrange(30))]
        counted, offs = replay(script, guard, None, run(sim_program, guard, None, script), recording=False)
        sizes = [int(s.split()[1]) for s in script]
        cap = counted.high - 1
        _, short = replay(script, guard, cap, run(sim_program, guard, cap, script), recording=guard != 0)
        # without rewinds `off` only grows: the first block whose end (guard included) is the count is the first that does not fit
        expected = next(i for i in range(len(script)) if offs[i] + sizes[i] + guard > cap)
        assert offs[expected] + sizes[expected] + guard == counted.high
        assert short.index(None) == expected and short[:expected] == offs[:expected]


def test_guard_zero_is_the_old_rule(sim_program):
    """off = align256(off) + bytes, high = max off, reset keeps high -- and nothing is recorded, no callback runs."""
    rng = random.Random(7)
    script = random_script(rng, 200)
    lines = run(sim_program, 0, 1 << 62, script)
    off = high = 0
    marks = [0]
    it = iter(lines)
    for op in script:
        word, _, arg = op.partition(" ")
        if word == "alloc":
            a = (off + 255) & ~255
            off = a + int(arg)
            high = max(high, off)
            marks.append(off)
            assert next(it) == f"a {a} {off} {high}"
        elif word == "blocks":
            assert next(it) == "b 0"
        else:
            k = 0 if word == "reset" else int(arg)
            off = marks[k]
            del marks[k + 1:]
            assert next(it) == f"r {off} {high}"
    assert next(it, None) is None


@pytest.mark.parametrize("guard", GUARDS[1:])
def test_partial_rewind_keeps_the_blocks_below_the_mark(sim_program, guard):
    """The R-/O-Net chunk loop: blocks, a mark, a chunk's blocks, back to the mark, the next chunk's blocks at the same offsets."""
    script = ["alloc 1000", "alloc 77", "alloc 5000", "alloc 300", "blocks", "rewind 2", "blocks", "alloc 5000", "alloc 300", "blocks",
              "rewind 2", "rewind 2", "blocks", "rewind 0", "blocks"]
    lines = run(sim_program, guard, 1 << 40, script)
    m, offs = replay(script, guard, 1 << 40, lines, recording=True)
    assert offs[2:4] == offs[4:6]
    b = [ln for ln in lines if ln.startswith("b ")]
    assert b[0].split()[1] == "4" and b[1].split()[1] == "2" and b[2] == b[0] and b[3] == b[1] and b[4] == "b 0"
    assert b[1].split()[2:] == b[0].split()[2:4]


@pytest.mark.parametrize("guard", GUARDS)
def test_counter_carries_the_guard(sim_program, guard):
    assert run(sim_program, guard, 4096, ["counter"]) == [f"c {guard} 1"]
    assert run(sim_program, guard, None, ["counter"]) == [f"c {guard} 1"]


def test_over_a_callers_workspace(sim_program):
    """Arena::over: a real arena, guard off, with the workspace's size as its capacity -- and capacity 0 over a null workspace,
    whatever size the caller claims, so that nothing is ever carved from a null pointer."""
    script = ["over 1 1000 1000", "over 1 1000 1001", "over 1 0 1", "over 0 1000 1", "over 0 1000 0", "over 0 0 0", "over 1 %d %d" % (5 << 30, 5 << 30)]
    assert run(sim_program, 256, 4096, script) == ["o 1000 0 0 0", "o 1000 0 0 null", "o 0 0 0 null", "o 0 0 0 null", "o 0 0 0 null",
                                                   "o 0 0 0 null", "o %d 0 0 0" % (5 << 30)]
