"""CPU tests of the fused PNet's confirm-queue capacity (csrc/trl_capacity.h: DeferCaps, trl_defer_plan, trl_defer_check inside
trl_caps_check) and of its block in the workspace (csrc/trl_arena.h).  ``tests/defer_sim.cpp`` includes the two headers alone, is
built for the host with ``-ffp-contract=off`` like the library (and the address / undefined-behaviour sanitizers where their runtime
exists) and reads calls from stdin; nothing is loaded into Python.  The expectations below restate the policy in numpy float32:

* start: ``int(0.25 * mtiles) + 64`` slots, at least the 13,617 that fit 64 MiB, never more than the launch has M-tiles
  (DESIGN.md section 4): a small launch gets a slot per M-tile and cannot overflow;
* growth: an overflow measures the need N (the slot counter keeps counting), the re-run gets ``int(1.25 N / mtiles * mtiles) + 64``;
* bound: N above half of the M-tiles (or a queue beyond 4 GiB) puts the next 256 PNet attempts (the re-run is the first) on the inline path;
* a call that fitted lets the hint follow the need: grow at once, decay by 3 % per call;
* the dry run (a counting arena) and the carve agree to the byte, with red zones, and the red zone behind the queue stays intact."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from truely_amd import jpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(jpeg.__file__), "csrc")
F = np.float32
SLOT = 32 + 72 * 17 * 4
MAX_SLOTS = (4 << 30) // SLOT
FULL_SLOTS = (64 << 20) // SLOT
HOLD = 256


@pytest.fixture(scope="module")
def sim_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("defer_sim") / "defer_sim")
    base = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "tests", "defer_sim.cpp"), "-o", out]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(base + san, capture_output=True, text=True).returncode != 0:
        subprocess.run(base, check=True)
    return out


def bits(v):
    return int(np.array(v, np.float32).view(np.uint32))


class Policy:
    """the restatement"""

    def __init__(self, forced=0):
        self.frac, self.hold, self.forced = F(0.0), 0, forced

    def plan(self, mtiles, applicable):
        if not applicable or mtiles <= 0 or self.hold > 0:
            return 0
        want = self.forced if self.forced > 0 else max(int(F(0.25) * F(mtiles)) + 64, FULL_SLOTS)
        if self.frac > 0:
            want = max(want, int(self.frac * F(mtiles)) + 64)
        return min(want, mtiles, MAX_SLOTS)

    def call(self, mtiles, applicable, need):
        """[(cap, bytes, retry, hold, frac bits)] of the attempts of one call"""
        rows = []
        while True:
            cap = self.plan(mtiles, applicable)
            retry = 0
            if cap > 0:
                over = need > cap
                if F(need) > F(0.5) * F(mtiles) or int(F(1.25) * F(need)) + 64 > MAX_SLOTS:
                    self.hold = HOLD
                else:
                    want = F(1.25) * F(need) / F(mtiles) + F(0.0)
                    d = F(0.97) * self.frac
                    self.frac = want if over or want > d else (d if d > 0 else min(self.frac, F(0.0)))
                retry = int(over)
            elif self.hold > 0:
                self.hold -= 1
            rows.append((cap, cap * SLOT, retry, self.hold, bits(self.frac)))
            if not retry:
                return rows


def run(program, script):
    r = subprocess.run([program], input=script, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return iter(r.stdout.splitlines())


def play(program, forced, calls, guard=4096):
    """calls: [(mtiles, applicable, need)] -> the attempts of every call, checked against the restatement"""
    got = run(program, f"new {forced}\n" + "".join(f"call {m} {int(a)} {n} {guard}\n" for m, a, n in calls))
    ref, out = Policy(forced), []
    for m, a, n in calls:
        want = ref.call(m, a, n)
        for w in want:
            line = next(got).split()
            assert line[0] == "attempt" and tuple(int(v) for v in line[1:]) == w, ((m, a, n), line, w)
        assert next(got).split() == ["done", str(len(want))]
        out.append(want)
    assert next(got, None) is None
    return out


def start(m):
    return Policy().plan(m, True)


def test_start_size(sim_program):
    assert FULL_SLOTS == 13_617
    for m in (1, 63, 64, 100, 5213, 13_617, 13_618, 54_211, 54_213, 1_303_250, 40_000_000):
        (rows,) = play(sim_program, 0, [(m, True, 0)])
        cap = min(m, max(m // 4 + 64, FULL_SLOTS), MAX_SLOTS)
        assert rows == [(cap, cap * SLOT, 0, 0, 0)]
    assert start(13_618) == 13_617 and start(54_212) == 13_617 and start(54_216) == 13_618 and start(1_303_250) == 325_876
    # not applicable (screen off, a net without the instantiation, thr0 outside the prefilter): no queue, no block, no state
    (rows,) = play(sim_program, 0, [(5213, False, 4000)])
    assert rows == [(0, 0, 0, 0, 0)]


def test_growth_and_settling(sim_program):
    m = 100_000                                                       # (a launch past the slot-per-M-tile region)
    calls = [(m, True, 6_700)] * 3 + [(m, True, 40_000)] + [(m, True, 40_000)] + [(m, True, 6_700)] * 60
    out = play(sim_program, 0, calls)
    assert [len(r) for r in out[:5]] == [1, 1, 1, 2, 1]              # 40 % overflows the 25 % start once; the next call fits
    assert out[3][0][2] == 1 and out[3][1][0] >= 40_000 and out[3][1][0] == int(F(1.25) * F(40_000) / F(m) * F(m)) + 64
    caps = [r[0][0] for r in out[5:]]
    assert all(a >= b for a, b in zip(caps, caps[1:])) and caps[-1] == m // 4 + 64      # decays back to the start, never below
    # a forced start of one slot: one overflow, then 1.25 N + 64
    out = play(sim_program, 1, [(m, True, 6_700), (m, True, 6_700)])
    assert [r[0] for r in out[0]] == [1, int(F(1.25) * F(6_700) / F(m) * F(m)) + 64] and len(out[1]) == 1
    # need - 1 slots overflow, need slots fit
    assert len(play(sim_program, 6_699, [(m, True, 6_700)])[0]) == 2
    assert len(play(sim_program, 6_700, [(m, True, 6_700)])[0]) == 1


def test_bound_selects_the_inline_path_and_holds_it(sim_program):
    m = 100_000
    for need in (50_001, 99_999, 100_000):
        out = play(sim_program, 0, [(m, True, need)] * (HOLD + 3))
        assert [r[0] for r in out[0]] == [m // 4 + 64, 0] and out[0][0][2:4] == (1, HOLD)     # overflow, then inline
        assert all(len(r) == 1 and r[0][0] == 0 for r in out[1:HOLD])                         # no oscillation: one attempt, inline
        assert [r[0] for r in out[HOLD]] == [m // 4 + 64, 0]                                  # one probe per HOLD calls
    # exactly half is still queued
    out = play(sim_program, 0, [(m, True, 50_000)] * 2)
    assert [r[0] for r in out[0]] == [m // 4 + 64, 50_000 * 5 // 4 + 64] and len(out[1]) == 1
    # a small launch has a slot per M-tile: content past the bound fits, and the next HOLD calls are inline all the same
    out = play(sim_program, 0, [(5_000, True, 4_000)] * (HOLD + 2))
    assert out[0] == [(5_000, 5_000 * SLOT, 0, HOLD, 0)]
    assert all(r == [(0, 0, 0, HOLD - 1 - i, 0)] for i, r in enumerate(out[1:HOLD + 1])) and out[HOLD + 1][0][0] == 5_000
    # a queue beyond 4 GiB is past the bound whatever the fraction
    big = 40_000_000
    out = play(sim_program, 0, [(big, True, MAX_SLOTS + 1)] * 2, guard=256)
    assert [r[0] for r in out[0]] == [MAX_SLOTS, 0] and out[1][0][0] == 0


def test_dry_run_and_carve_agree(sim_program):
    """every attempt of the calls above carved its block from an arena of exactly the counted size; here across guards"""
    for guard in (0, 256, 4096):
        play(sim_program, 0, [(m, True, n) for m in (1, 7, 300, 5213) for n in (0, 1, m // 8, m // 3, m)], guard=guard)
        play(sim_program, 3, [(5213, True, 700), (5213, True, 2)], guard=guard)
