"""CPU tests of the cascade's capacity policy (csrc/trl_capacity.h; no GPU).

``tests/capacity_sim.cpp`` includes the header alone and is built for the host with ``-ffp-contract=off`` like the library, and with
the address and undefined-behaviour sanitizers where their runtime exists.  It reads attempts from stdin -- geometry, then the
flag words the kernels would have written -- and prints after each the plan, the capacity struct, ``retry`` and ``resume_stage``.
Nothing is loaded into Python.

Equivalence: ``Parent`` below restates, in numpy ``float32`` with the same operation order, ``plan_lists()``, the ``cap_t2`` /
``cap_t3`` part of ``size_scratch()`` and ``trl_cascade_check()`` as they stood in ``trl_cascade.hip`` before the header existed
(written from that text, not from the header).  Over hand-made sequences, one per branch, and 200 seeded random ones, every float
must be equal as bits and every integer equal.  The program does not handle the ``L == 0`` shortcut of ``trl_cascade_detect``
(no scale at all: every count is zeroed and no kernel reports): with ``L = 0`` it plans and checks like for any other geometry.

Convergence: a model device holds true needs and reports the flag words as the kernels do (``trl_cascade.hip`` / ``trl_pnet.hip``):

* ``FLG_LEVEL_MAX`` carries the true per-level maximum even when the list overflowed: the slot counter keeps counting
  (``atomicAdd`` on ``lvl_cnt`` in ``k_pnet_collect``, trl_cascade.hip:511, and in ``k_pnet_fused``'s candidate write,
  trl_pnet.hip:826; the ``slot >= cap`` test comes after it) and ``k_nms_level`` takes
  ``atomicMax(&flags[FLG_LEVEL_MAX + l], cnt)`` in front of ``if (cnt > cap)`` (trl_cascade.hip:552-553).
* ``FLG_FRAME_MAX`` carries the true per-frame total even when the list overflowed: ``k_nms_frame`` takes
  ``atomicMax(&flags[FLG_FRAME_MAX], run)`` in front of ``if (run > capF) flags[FLG_FRAME] = 1`` (trl_cascade.hip:585-586).
* The spill cursor keeps counting past the pool: ``spill_alloc`` adds the bytes to ``FLG_SPILL_CUR`` first and raises
  ``FLG_SPILL`` when ``off_s + bytes > sp.cap`` (trl_cascade.hip:198-200).
* ``FLG_T2N`` / ``FLG_T3N`` carry true totals: ``k_scan_counts`` writes ``flags[FLG_T2N + slot] = total`` in front of
  ``if (total > cap_total) flags[FLG_T2 + slot] = 1`` (trl_cascade.hip:629).
* Every word behind the first overflowing stage is unreliable (it was computed from truncated or dropped lists).  One exception
  is by design and is modelled as such: a spill overflow drops lists, so the per-frame total ``k_nms_frame`` reports is a lower
  bound of the true one, and ``FLG_FRAME`` with it is still a true overflow -- the check reads both in that branch.

For the unreliable words the model writes zeros, ``INT_MAX`` and the true value into three instances of the program that run in
lockstep; their structs must stay equal.  The largest attempt count seen is printed: it is the figure in the comment on
``TRL_MAX_ATTEMPTS`` (``trl_api.hip``)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from truely_amd import jpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(jpeg.__file__), "csrc")
F = np.float32
INT_MAX = 2**31 - 1
U64 = 2**64 - 1
NFLAGS = 64
FLG_LEVEL, FLG_FRAME, FLG_T2, FLG_T3, FLG_T2N, FLG_T3N, FLG_FRAME_MAX, FLG_SPILL, FLG_SPILL_CUR, FLG_SPILL_LISTS, FLG_LEVEL_MAX = 0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 16
TRL_MAX_ATTEMPTS = 12


@pytest.fixture(scope="module")
def sim_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("capacity_sim") / "capacity_sim")
    base = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "tests", "capacity_sim.cpp"), "-o", out]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(base + san, capture_output=True, text=True).returncode != 0:
        subprocess.run(base, check=True)
    return out


def test_max_attempts_constant_is_the_librarys():
    with open(os.path.join(CSRC, "trl_api.hip")) as f:
        assert f"enum {{ TRL_MAX_ATTEMPTS = {TRL_MAX_ATTEMPTS} }};" in f.read()


# ---- the parent commit's arithmetic, restated ------------------------------------------------------------------------------------
def bits(v):
    return int(np.array(v, np.float32).view(np.uint32))


def i32(v):
    """(int) of a long long, as the hardware truncates it"""
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v & 0x80000000 else v


class Parent:
    def __init__(self, cap_level, cap_frame):
        self.cap_level, self.cap_frame = cap_level, cap_frame
        self.t2, self.t3 = F(160.0), F(48.0)
        self.lvl = [F(0.0)] * 32
        self.frame = F(0.0)
        self.spill = 0
        self.capl = []

    def plan(self, n, cells):
        self.n = n
        capl, rec0, S, total = [], [], 0, 0
        for l, c in enumerate(cells):                  # plan_lists()
            want = self.cap_level
            if int(self.lvl[l]) > want:
                want = int(self.lvl[l])
            if want > c:
                want = c
            if want < 4:
                want = 4
            capl.append(i32((want + 3) & ~3))
            rec0.append(S)
            S += capl[-1]
            total += c
        want = self.cap_frame
        if int(self.frame) > want:
            want = int(self.frame)
        if want > total:
            want = total
        if want < 4:
            want = 4
        capF = i32((want + 3) & ~3)
        c2, c3 = int(self.t2 * F(n)) + 64, int(self.t3 * F(n)) + 64     # size_scratch()
        lim = n * capF
        self.capl = capl
        return [len(cells), S, capF, i32(min(c2, lim)), i32(min(c3, lim))] + capl + rec0

    def check(self, f):                                # trl_cascade_check()
        n, L = self.n, len(self.capl)
        retry = resume = 0
        used = (f[FLG_SPILL_CUR] & 0xFFFFFFFF) | ((f[FLG_SPILL_CUR + 1] & 0xFFFFFFFF) << 32)
        if f[FLG_LEVEL]:
            s = 0
            for l in range(L):
                want = F(1.25) * F(f[FLG_LEVEL_MAX + l]) + F(4.0)
                if f[FLG_LEVEL_MAX + l] > self.capl[l] and want > self.lvl[l]:
                    self.lvl[l] = want
                s += f[FLG_LEVEL_MAX + l]
            if F(s) > self.frame and float(s) * 132.0 * float(n) < 8e9:
                self.frame = F(s)
            return self.state(1, 0)
        if f[FLG_SPILL]:
            self.spill = (used * 2 + (16 << 20)) & U64
            if f[FLG_FRAME]:
                self.frame = F(1.25) * F(f[FLG_FRAME_MAX]) + F(4.0)
            return self.state(1, 0)
        if f[FLG_FRAME]:
            self.frame = F(1.25) * F(f[FLG_FRAME_MAX]) + F(4.0)
            return self.state(1, 0)
        want2 = F(1.25) * F(f[FLG_T2N]) / F(n) + F(1.0)
        want3 = F(1.25) * F(f[FLG_T3N]) / F(n) + F(1.0)
        if f[FLG_T2]:
            self.t2, retry, resume = want2, 1, 2
        elif f[FLG_T3]:
            self.t3, retry, resume = want3, 1, 3
        if not retry:
            d2, d3 = F(0.97) * self.t2, F(0.97) * self.t3
            self.t2 = want2 if want2 > d2 else (d2 if d2 > F(160.0) else (self.t2 if self.t2 < F(160.0) else F(160.0)))
            self.t3 = want3 if want3 > d3 else (d3 if d3 > F(48.0) else (self.t3 if self.t3 < F(48.0) else F(48.0)))
            for l in range(L):
                want, d = F(1.25) * F(f[FLG_LEVEL_MAX + l]) + F(4.0), F(0.97) * self.lvl[l]
                self.lvl[l] = want if want > d else d
            want, d = F(1.25) * F(f[FLG_FRAME_MAX]) + F(4.0), F(0.97) * self.frame
            self.frame = want if want > d else d
            want, d = (used + (used >> 2)) & U64, self.spill - (self.spill >> 5)
            self.spill = max(want, d) if used else (d if d > (1 << 20) else 0)
        return self.state(retry, resume)

    def state(self, retry, resume):
        return [retry, resume, bits(self.t2), bits(self.t3), bits(self.frame), self.spill] + [bits(v) for v in self.lvl]


def words(level=0, frame=0, t2=0, t3=0, t2n=0, t3n=0, frame_max=0, spill=0, spill_cur=0, spill_lists=0, level_max=()):
    f = [0] * NFLAGS
    f[FLG_LEVEL], f[FLG_FRAME], f[FLG_T2], f[FLG_T3], f[FLG_T2N], f[FLG_T3N] = level, frame, t2, t3, t2n, t3n
    f[FLG_FRAME_MAX], f[FLG_SPILL], f[FLG_SPILL_LISTS] = frame_max, spill, spill_lists
    f[FLG_SPILL_CUR], f[FLG_SPILL_CUR + 1] = i32(spill_cur & 0xFFFFFFFF), i32(spill_cur >> 32)
    for l, v in enumerate(level_max):
        f[FLG_LEVEL_MAX + l] = v
    return f


def hand_sequences():
    """(name, cap_level, cap_frame, (t2, t3) hint or None, [(n, cells, flag words)])"""
    geo = [4000, 1000, 250]
    settled = words(t2n=300, t3n=40, frame_max=50, level_max=[30, 20, 10])
    seqs = [
        ("level overflow with the frame jump", 64, 64, None, [
            (2, geo, words(level=1, level_max=[500, 300, 20], frame=1, frame_max=INT_MAX, t2=1, t3n=7)),
            (2, geo, settled), (2, geo, settled)]),
        ("level overflow without the jump: the sum is under the frame hint", 64, 64, None, [
            (2, geo, words(frame_max=2000, level_max=[30, 20, 10])),
            (2, geo, words(level=1, level_max=[500, 300, 20])), (2, geo, settled)]),
        ("level overflow on both sides of the 8e9 test", 64, 64, None, [
            (65535, geo, words(level=1, level_max=[500, 404, 20])),      # 924 * 132 * 65535 < 8e9: jump
            (65535, geo, words(level=1, level_max=[501, 404, 20])),      # 925: no jump
            (65535, [10**7, 10**6], words(level=1, level_max=[9 * 10**6, 10**6])), (65535, geo, settled)]),
        ("spill overflow without FLG_FRAME", 64, 64, None, [
            (3, geo, words(spill=1, spill_cur=(5 << 30) + 12345, spill_lists=9, frame_max=50, t2=1, t2n=INT_MAX, level_max=[30, 20, 10])),
            (3, geo, words(spill_cur=(5 << 30) + 12345, spill_lists=9, t2n=300, t3n=40, frame_max=50, level_max=[30, 20, 10]))]),
        ("spill overflow with FLG_FRAME", 64, 64, None, [
            (3, geo, words(spill=1, spill_cur=77777, spill_lists=2, frame=1, frame_max=900, t3=1, level_max=[30, 20, 10])),
            (3, geo, settled)]),
        ("frame overflow alone", 64, 64, None, [
            (3, geo, words(frame=1, frame_max=333, t2=1, t3=1, t2n=5, level_max=[60, 60, 60])), (3, geo, settled)]),
        ("T2 overflow (and T3 behind it)", 2048, 2048, None, [
            (4, geo, words(t2=1, t3=1, t2n=5000, t3n=3, frame_max=50, level_max=[30, 20, 10])),
            (4, geo, words(t3=1, t2n=5000, t3n=2000, frame_max=50, level_max=[30, 20, 10])),
            (4, geo, words(t2n=5000, t3n=2000, frame_max=50, level_max=[30, 20, 10]))]),
        ("T3 overflow", 2048, 2048, None, [
            (4, geo, words(t3=1, t2n=100, t3n=999, frame_max=50, level_max=[30, 20, 10])), (4, geo, settled)]),
        ("a settled call grows every hint", 64, 64, None, [
            (2, geo, words(t2n=100000, t3n=50000, frame_max=3000, spill_cur=1 << 33, level_max=[2500, 900, 200])),
            (2, geo, words(t2n=100001, t3n=50001, frame_max=3001, spill_cur=(1 << 33) + 1, level_max=[2501, 901, 201]))]),
        ("settled calls decay every hint to its floor", 64, 64, None,
            [(2, geo, words(t2n=100000, t3n=50000, frame_max=3000, spill_cur=1 << 33, level_max=[2500, 900, 200]))]
            + [(2, geo, words())] * 420),
        ("hints below the configured start", 2048, 2048, (0.25, 0.25), [
            (4, geo, words(t2n=0, t3n=0)), (4, geo, words(t2n=1, t3n=0, frame_max=3, level_max=[2, 1])),
            (4, geo, words(t2=1, t2n=70, t3n=0)), (4, geo, words(t2n=70, t3n=3))]),
        ("a level with fewer than 4 cells", 64, 64, None, [
            (2, [100, 3, 2, 1], words(level=1, level_max=[90, 3, 2, 1])), (2, [100, 3, 2, 1], words(frame_max=80, level_max=[90, 3, 2, 1])),
            (1, [3], words(level_max=[3], frame_max=3)), (1, [1], words())]),
        ("n = 1", 64, 64, None, [(1, geo, words(t2=1, t2n=1000, level_max=[10])), (1, geo, words(t2n=1000, t3n=10, level_max=[10]))]),
        ("n = 65535", 2048, 2048, None, [
            (65535, geo, words(t2=1, t2n=INT_MAX, frame_max=2048, level_max=[2048, 1000, 250])),
            (65535, geo, words(t3=1, t2n=INT_MAX, t3n=10**9, frame_max=2048, level_max=[2048, 1000, 250])),
            (65535, geo, words(t2n=10**9, t3n=10**9, frame_max=2048, level_max=[2048, 1000, 250]))]),
        ("L = 0", 64, 64, None, [(3, [], words()), (3, [], words(t2=1, t2n=50))]),
        ("L = 32", 64, 64, None, [
            (2, [2**26 >> l for l in range(32)], words(level=1, level_max=[min(2**26 >> l, 70 + l) for l in range(32)])),
            (2, [2**26 >> l for l in range(32)], words(frame_max=500, level_max=[min(2**26 >> l, 70 + l) for l in range(32)])),
            (2, [2**26 >> l for l in range(32)], words(level=1, level_max=[INT_MAX] * 32))]),
    ]
    return seqs


def random_sequences():
    rng = np.random.default_rng(20261019)

    def count(scale):
        k = int(rng.integers(0, 6))
        return [0, int(rng.integers(0, 8)), int(rng.integers(0, max(2, scale))), int(rng.integers(0, max(2, 4 * scale))),
                int(rng.integers(0, 2**24)), int(rng.integers(2**30, 2**31))][k]
    seqs = []
    for t in range(200):
        cap_level, cap_frame = (int(rng.choice([4, 64, 2048, 3072, 2**24])) for _ in range(2))
        hint = (float(F(rng.uniform(0.1, 400))), float(F(rng.uniform(0.1, 400)))) if t % 5 == 0 else None
        steps = []
        L = int(rng.integers(0, 33))
        top = int(rng.integers(1, 2**26))
        cells = [max(1, top >> l) for l in range(L)]
        n = int(rng.choice([1, 2, 16, 256, 65535]))
        for a in range(8):
            if a and rng.random() < 0.15:              # another geometry, as a new clip would bring
                L = int(rng.integers(0, 33))
                cells = [max(1, top >> l) for l in range(L)]
                n = int(rng.choice([1, 3, 64, 65535]))
            flag = [int(rng.random() < p) for p in (0.25, 0.25, 0.3, 0.3, 0.2)]
            steps.append((n, cells, words(level=flag[0], frame=flag[1], t2=flag[2], t3=flag[3], spill=flag[4], t2n=count(200 * n), t3n=count(50 * n),
                                          frame_max=count(cap_frame), spill_cur=int(rng.integers(0, 2**40)) if rng.random() < 0.6 else 0,
                                          spill_lists=int(rng.integers(0, 99)), level_max=[count(cap_level) for _ in range(L)])))
        seqs.append((f"random {t}", cap_level, cap_frame, hint, steps))
    return seqs


def script_of(seqs):
    lines = []
    for _name, cap_level, cap_frame, hint, steps in seqs:
        lines.append(f"new {cap_level} {cap_frame}")
        if hint:
            lines.append(f"hint {bits(F(hint[0]))} {bits(F(hint[1]))}")
        for n, cells, f in steps:
            lines.append(" ".join(map(str, ["plan", n, len(cells)] + cells)))
            lines.append(" ".join(map(str, ["check"] + f)))
    return "\n".join(lines) + "\n"


def test_header_equals_the_parent_commits_arithmetic(sim_program):
    seqs = hand_sequences() + random_sequences()
    r = subprocess.run([sim_program], input=script_of(seqs), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    got = iter(r.stdout.splitlines())
    branches = set()
    for name, cap_level, cap_frame, hint, steps in seqs:
        ref = Parent(cap_level, cap_frame)
        if hint:
            ref.t2, ref.t3 = F(hint[0]), F(hint[1])
        for k, (n, cells, f) in enumerate(steps):
            line = next(got).split()
            assert line[0] == "plan" and [int(v) for v in line[1:]] == ref.plan(n, cells), (name, k, "plan")
            line = next(got).split()
            want = ref.check(f)
            assert line[0] == "caps" and [int(v) for v in line[1:]] == want, (name, k, "check")
            branches.add((want[0], want[1], bool(f[FLG_LEVEL]), bool(f[FLG_SPILL]) and not f[FLG_LEVEL]))
    assert next(got, None) is None
    assert {(0, 0, False, False), (1, 0, True, False), (1, 0, False, True), (1, 0, False, False), (1, 2, False, False), (1, 3, False, False)} <= branches


def test_decay_reaches_the_floors():
    """The hand-made decay sequence does what its name says in the restatement (so the equivalence test covers that branch)."""
    name, cap_level, cap_frame, _hint, steps = [s for s in hand_sequences() if s[0].startswith("settled calls decay")][0]
    ref = Parent(cap_level, cap_frame)
    for n, cells, f in steps:
        ref.plan(n, cells)
        ref.check(f)
    assert ref.t2 == F(160.0) and ref.t3 == F(48.0) and ref.spill == 0
    assert ref.frame == F(4.0) and all(v == F(4.0) for v in ref.lvl[:3])


# ---- convergence on a model device -----------------------------------------------------------------------------------------------
class Device:
    """True needs of one batch and the flag words the kernels report for a plan (see the module docstring)."""
    SPILL_BOUND = 64          # bytes per entry the up-front pool reserves for a list that can spill (+ 256 per list)

    def __init__(self, rng, t):
        kind = t % 5
        self.nms_full = int(rng.choice([64, 2048]))
        if kind == 0:                                   # empty content
            self.n, L, top = int(rng.choice([1, 16, 65535])), int(rng.integers(0, 17)), int(rng.integers(1, 2**16))
        elif kind == 1:                                 # geometry limits: a 16383 px frame, PNet map 8187 x 8187 at the finest level
            self.n, L, top = 1, int(rng.integers(20, 33)), 8187 * 8187
        else:
            self.n, L, top = int(rng.choice([1, 2, 16, 256, 4096, 65535])), int(rng.integers(1, 20)), int(rng.integers(1, 2**22))
        self.cells = [max(1, top >> l) for l in range(L)]
        fill = 0.0 if kind == 0 else float(rng.random()) ** 3
        self.level = [int(round(c * fill * rng.random())) for c in self.cells]
        if kind == 1 and t % 2:
            self.level = list(self.cells)               # every cell of every level a candidate
        total = sum(self.level)
        self.frame = int(total * (1.0 if t % 7 == 0 else rng.random()))          # stage-1 rows of the fullest frame (NMS keeps a subset)
        self.t2 = min(int(self.frame * self.n * (1.0 if t % 3 == 0 else rng.random())), 10**9)
        self.t3 = int(self.t2 * (1.0 if t % 4 == 0 else rng.random()))
        self.spill_per_entry = int(rng.choice([16, 64, 200, 4000]))              # above SPILL_BOUND: the up-front pool is too small
        self.cap_level, self.cap_frame = (int(rng.choice([4, 64, 2048, 2**24])) for _ in range(2))

    def pool(self, spill_hint, capl, capF):             # spill_pool(): the hint, or the bounded up-front estimate
        per_frame = sum(c * self.SPILL_BOUND + 256 for c in capl if c > self.nms_full)
        if capF > self.nms_full:
            per_frame += 3 * (capF * self.SPILL_BOUND + 256)
        return max(spill_hint, min(per_frame * self.n, 8 << 30))

    def report(self, capl, capF, cap_t, pool, junk):
        """The words of an attempt; `junk(true)` fills every word behind the first overflowing stage."""
        f = words(level_max=self.level)
        over = [need > cap for need, cap in zip(self.level, capl)]
        kept = [min(need, cap) for need, cap in zip(self.level, capl)]
        used = sum(self.n * (k * self.spill_per_entry + 256) for k in kept if k > self.nms_full)
        lists = sum(self.n for k in kept if k > self.nms_full)
        frame_fits = self.frame <= capF
        if frame_fits and self.frame > self.nms_full:   # the frame lists of stages 1-3
            used += 3 * self.n * (self.frame * self.spill_per_entry + 256)
            lists += 3 * self.n
        true = dict(frame=int(not frame_fits), frame_max=self.frame, spill=int(used > pool), spill_cur=used, spill_lists=lists,
                    t2=int(self.t2 > cap_t[0]), t2n=self.t2, t3=int(self.t3 > cap_t[1]), t3n=self.t3)
        if any(over):
            keys, true["level"] = list(true), 1
        elif true["spill"]:
            keys = ["t2", "t2n", "t3", "t3n"]
            true["frame_max"] = self.frame // 2 if frame_fits else capF + 1 + (self.frame - capF - 1) // 2   # a lower bound (lists were dropped)
        elif true["frame"]:
            keys = ["t2", "t2n", "t3", "t3n"]
        elif true["t2"]:
            keys = ["t3", "t3n"]
        else:
            keys = []
        for k in keys:
            true[k] = junk(true[k]) if k.endswith("n") or k in ("frame_max", "spill_cur", "spill_lists") else int(junk(true[k]) != 0)
        return words(level_max=self.level, **true)


class Sims:
    """Three instances of the program in lockstep, one per way of filling the unreliable words"""
    JUNK = (lambda v: 0, lambda v: INT_MAX, lambda v: v)

    def __init__(self, program):
        self.p = [subprocess.Popen([program], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, bufsize=1) for _ in self.JUNK]

    def ask(self, lines, reply=True):
        for p, line in zip(self.p, lines):
            p.stdin.write(line + "\n")
            p.stdin.flush()
        if not reply:
            return None
        got = [p.stdout.readline() for p in self.p]
        assert got[0] and got.count(got[0]) == len(got), ("the struct depends on a word behind the first overflow", lines, got)
        return [int(v) for v in got[0].split()[1:]]

    def close(self):
        for p in self.p:
            p.stdin.close()
            assert p.wait(timeout=30) == 0, p.stderr


def run_call(sims, dev):
    """One call: attempts until the check asks for no re-run.  Returns the attempt count."""
    for attempt in range(1, TRL_MAX_ATTEMPTS + 1):
        plan = sims.ask([" ".join(map(str, ["plan", dev.n, len(dev.cells)] + dev.cells))] * 3)
        L = plan[0]
        capF, cap_t, capl = plan[2], plan[3:5], plan[5:5 + L]
        pool = dev.pool(dev.spill_hint, capl, capF)
        caps = sims.ask([" ".join(map(str, ["check"] + dev.report(capl, capF, cap_t, pool, junk))) for junk in Sims.JUNK])
        dev.spill_hint = caps[5]
        if not caps[0]:
            return attempt
    return TRL_MAX_ATTEMPTS + 1


def test_every_call_converges_and_the_next_fits(sim_program):
    rng = np.random.default_rng(45)
    sims = Sims(sim_program)
    worst, histogram = 0, {}
    try:
        for t in range(500):
            dev = Device(rng, t)
            dev.spill_hint = 0
            sims.ask([f"new {dev.cap_level} {dev.cap_frame}"] * 3, reply=False)
            if t % 6 == 0:                              # batch hints put far below the need by hand
                sims.ask([f"hint {bits(F(0.25))} {bits(F(0.25))}"] * 3, reply=False)
            first = run_call(sims, dev)
            assert first <= TRL_MAX_ATTEMPTS, (t, vars(dev))
            assert run_call(sims, dev) == 1, (t, vars(dev))
            worst = max(worst, first)
            histogram[first] = histogram.get(first, 0) + 1
    finally:
        sims.close()
    print(f"largest attempt count over 500 need sets: {worst}; calls by attempts: {dict(sorted(histogram.items()))}")
    assert worst >= 5                                   # the model reaches the long chains, not only easy calls
