"""CPU tests of the Motion-JPEG decoder's rules (no GPU).

``jpegd_ref.decode`` restates in numpy what ``Image.open(f).convert("RGB")`` does through libjpeg-turbo's default decompression
path; these tests pin it to Pillow's bytes over sizes, subsamplings, qualities, content and encoder options chosen to reach every
edge case (partial edge MCUs, one-sample chroma, stuffed 0xFF bytes, optimised tables, restart intervals with RST7 -> RST0), pin
``trl_jpegd_parse`` (host-only C ABI) to what Pillow reads from the same headers, and run the decoder's parser and its shared
entropy-decode function in a stand-alone, sanitized host program over a fixed table of damaged streams.

The synthetic table (``jpegd_cases.synthetic_files``) holds what Pillow's encoder never writes: edited headers, scans coded by the
tests' own baseline writer, and coefficients large enough to reach the IDCT gate.  Its "pillow" streams must decode to Pillow's
bytes, its "gated" streams must be refused."""
import io
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

import jpegd_cases as cases
import jpegd_ref
from truely_amd import jpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(jpeg.__file__), "csrc")


@pytest.mark.parametrize("sub", [0, 1, 2])
@pytest.mark.parametrize("size", cases.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_reference_decoder_equals_pillow(size, sub):
    W, H = size
    for label, data in cases.good_files(W, H, sub):
        if label.startswith("stuffed"):
            assert b"\xff\x00" in data[cases.scan_offset(data):], "the stuffed frame has no stuffed byte"
        got = jpegd_ref.decode(data)
        assert got.shape == (H, W, 3)
        assert np.array_equal(got, cases.pillow_bgr(data)), f"{W}x{H} subsampling {sub} {label}"


@pytest.mark.parametrize("sub", [0, 1, 2])
def test_restart_numbers_wrap(sub):
    """The marker-per-MCU files of the decode table hold more than eight restart markers: RST7 is followed by RST0."""
    data = dict(cases.good_files(64, 48, sub))["rst-blocks1"]
    s = cases.scan_offset(data)
    marks = [data[i + 1] for i in range(s, len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]
    assert len(marks) > 8 and marks[7] == 0xD7 and marks[8] == 0xD0


def _pillow_sampling(im):
    (_, h, v, _) = im.layer[0]
    return h, v


@pytest.mark.parametrize("sub", [0, 1, 2])
def test_parse_equals_pillow(sub):
    """trl_jpegd_parse on the files of the decode table: size, sampling, restart interval and scan offset."""
    for W, H in cases.SIZES:
        for label, data in cases.good_files(W, H, sub):
            info = jpeg.jpeg_info(data)
            im = Image.open(io.BytesIO(data))
            assert info["supported"] == 1 and info["reason"] == 0, (W, H, label, info)
            assert (info["width"], info["height"]) == im.size
            assert (info["h_samp"], info["v_samp"]) == _pillow_sampling(im)
            assert all(tuple(layer[1:3]) == (1, 1) for layer in im.layer[1:])
            assert info["scan_offset"] == cases.scan_offset(data)
            ref = jpegd_ref.parse(data)
            assert info["restart_interval"] == ref["ri"]
            assert (info["restart_interval"] != 0) == label.startswith("rst")


def test_parse_reports_unsupported_kinds():
    want = {"progressive": jpegd_ref.R_PROCESS, "grayscale": jpegd_ref.R_COMPONENTS, "cmyk": jpegd_ref.R_ADOBE,
            "cut-in-headers": jpegd_ref.R_TRUNCATED, "no-dht": jpegd_ref.R_DHT, "empty": jpegd_ref.R_TRUNCATED,
            "not-jpeg": jpegd_ref.R_NOT_JPEG}
    files = cases.unsupported_files()
    assert {label for label, _ in files} == set(want)
    for label, data in files:
        info = jpeg.jpeg_info(data)
        assert info["supported"] == 0 and info["reason"] == want[label], (label, info)
        with pytest.raises(jpegd_ref.Unsupported) as e:
            jpegd_ref.parse(data)
        assert e.value.reason == want[label]


def test_parse_agrees_with_reference_on_damaged_headers():
    for label, data in cases.damaged_files():
        info = jpeg.jpeg_info(data)
        try:
            jpegd_ref.parse(data)
            reason = 0
        except jpegd_ref.Unsupported as e:
            reason = e.reason
        assert info["reason"] == reason, (label, info, reason)


@pytest.fixture(scope="module")
def fuzz_program(tmp_path_factory):
    """tests/jpegd_fuzz.cpp built for the host with the address and undefined-behaviour sanitizers (without them where their
    runtime is not installed: the program then still checks statuses and coefficients)."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("jpegd_fuzz") / "jpegd_fuzz")
    base = [cxx, "-O1", "-g", "-std=c++17", "-I", CSRC, os.path.join(ROOT, "tests", "jpegd_fuzz.cpp"), "-o", out]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(base + san, capture_output=True, text=True)
    sanitized = r.returncode == 0
    if not sanitized:
        subprocess.run(base, check=True)
    return out, sanitized


def run_fuzz(program, files, folder):
    """[(status, coefficients | None)] of the stand-alone program for these files."""
    names = []
    for k, data in enumerate(files):
        names.append(os.path.join(folder, f"{k}.jpg"))
        with open(names[-1], "wb") as f:
            f.write(data)
    r = subprocess.run([program] + names, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(files)
    out = []
    for name, line in zip(names, lines):
        status = int(line.split()[0])
        out.append((status, np.fromfile(name + ".coef", np.int16) if status == 0 else None))
    return out


def ref_coefficients(data):
    info = jpegd_ref.parse(data)
    return np.concatenate([c.reshape(-1) for c in jpegd_ref.entropy_decode(data, info)])


def test_fuzz_program_good_files(fuzz_program, tmp_path):
    """The shared entropy-decode function, built for the CPU, gives the reference's coefficients for good files."""
    program, _ = fuzz_program
    files = [d for size in ((7, 5), (37, 51), (64, 48)) for sub in (0, 1, 2) for _, d in cases.good_files(*size, sub)]
    for data, (status, coef) in zip(files, run_fuzz(program, files, str(tmp_path))):
        assert status == 0
        assert np.array_equal(coef, ref_coefficients(data))


def test_fuzz_program_damaged_files(fuzz_program, tmp_path):
    """Every damaged stream: the program exits clean (no sanitizer report) and reports status 1 or 2 exactly where the reference
    raises Unsupported / Irregular from its parser and entropy decoder, or else decodes the reference's coefficients."""
    program, sanitized = fuzz_program
    table = cases.damaged_files() + cases.unsupported_files()
    seen = set()
    for (label, data), (status, coef) in zip(table, run_fuzz(program, [d for _, d in table], str(tmp_path))):
        try:
            want, ref = 0, ref_coefficients(data)
        except jpegd_ref.Unsupported:
            want = 1
        except jpegd_ref.Irregular:
            want = 2
        assert status == want, (label, status, want)
        if status == 0:
            assert np.array_equal(coef, ref), label
        seen.add(status)
    assert {1, 2} <= seen
    print("sanitized" if sanitized else "built without sanitizers")


# ---- the synthetic table ---------------------------------------------------------------------------------------------------------
SYN = pytest.mark.parametrize("size,sub", [(s, sub) for s in cases.SYN_SIZES for sub in (0, 1, 2)], ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else f"sub{v}")


@SYN
def test_writer_round_trip(size, sub):
    """The reference's entropy decoder returns from every written file the coefficients the writer was given."""
    n = 0
    for label, data, _ in cases.synthetic_files(*size, sub):
        want = cases.written_coefficients(data)
        if want is not None:
            assert np.array_equal(ref_coefficients(data), want), label
            n += 1
    assert n >= 40


@pytest.mark.parametrize("sub", [0, 1, 2])
def test_writer_covers_the_entropy_cases(sub):
    """At 64 x 48 the written scans hold every DC category 0..11, AC categories 1..10, zero runs of 16, 32 and 47, blocks without
    EOB and blocks of a DC alone, 16-bit codes, stuffed bytes, and more than eight restart intervals (RST7 -> RST0)."""
    seen = {}
    table = cases.entropy_files(64, 48, sub, seen)
    assert seen["dc"] == set(range(12))
    assert {s & 15 for s in seen["ac"]} >= set(range(1, 11)) and {0x00, 0xF0} <= seen["ac"]
    assert {16, 32, 47} <= seen["zrl"]
    assert min(seen["len"]) == 2 and max(seen["len"]) == 16
    assert seen["rst"] == set(range(0xD0, 0xD8))
    files = dict(table)
    contents = dict(cases.entropy_contents(64, 48, *cases.SUB_HV[sub]))
    assert any(b[63] != 0 for blocks in cases.coded_blocks(contents["zrl-and-no-eob"], *cases.SUB_HV[sub]) for b in blocks)
    assert any(not b[1:].any() for blocks in cases.coded_blocks(contents["zrl-and-no-eob"], *cases.SUB_HV[sub]) for b in blocks)
    for label, data in table:
        info = jpegd_ref.parse(data)
        scan = data[info["scan"]:]
        if label == "dense-stuffed-std-ri0":                       # (the content was chosen for this file; others stuff by chance)
            assert b"\xff\x00" in scan, label
        marks = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]
        mcus = 8 * 6 // (info["hs"] * info["vs"])
        assert len(marks) == ((mcus - 1) // info["ri"] if info["ri"] else 0), label
        if label.endswith("-ri1"):
            assert len(marks) > 8 and marks[7:9] == [0xD7, 0xD0]
    intervals = {jpegd_ref.parse(d)["ri"] for d in files.values()}
    mcus = 8 * 6 // (cases.SUB_HV[sub][0] * cases.SUB_HV[sub][1])
    assert {0, 1} <= intervals and any(r > mcus for r in intervals) and any(1 < r < mcus and mcus % r for r in intervals)


@SYN
def test_synthetic_files_in_the_reference(size, sub):
    """Every "pillow" stream decodes in the restatement to Pillow's bytes, every "gated" stream raises Irregular; neither half of
    the magnitude family is a token one, and all but a handful of its streams passed the former gate."""
    W, H = size
    table = cases.synthetic_files(W, H, sub)
    count = {"pillow": 0, "gated": 0}
    differ = former = 0
    for label, data, expect in table:
        pil = cases.pillow_bgr(data)
        assert pil.shape == (H, W, 3)
        if expect == "pillow":
            assert np.array_equal(jpegd_ref.decode(data), pil), label
        else:
            with pytest.raises(jpegd_ref.Irregular):
                jpegd_ref.decode(data)
            differ += not np.array_equal(jpegd_ref.decode(data, gate=False), pil)
        if label.startswith("magnitude-"):
            count[expect] += 1
            former += cases.former_gate_trips(data)
            assert cases.gate_expectation(data) == expect, label      # the expectations written by hand follow from the conditions
        else:
            assert expect == "pillow" and cases.gate_expectation(data) == "pillow", label
    total = sum(count.values())
    assert 3 * count["pillow"] >= total and 3 * count["gated"] >= total, count
    assert former <= 3
    # evidence, not a contract: it depends on whether this Pillow's libjpeg-turbo runs a SIMD IDCT
    print(f"{W}x{H} subsampling {sub}: the arithmetic without the gate decodes {differ} of {count['gated']} gated streams to other bytes than Pillow")


def test_gate_edges_of_a_dc_only_block():
    """(dc + 4) >> 3 is a DC-only block's output: the streams on either side of 511 | 512 and -512 | -513 are in the table, the inner
    ones owed to Pillow and the outer ones gated; single AC coefficients have their pairs too."""
    by_value = {q * c: e for q, c, e in cases.DC_EDGES}
    assert [(v, (v + 4) >> 3, by_value[v]) for v in (4090, 4092, -4100, -4101)] == [
        (4090, 511, "pillow"), (4092, 512, "gated"), (-4100, -512, "pillow"), (-4101, -513, "gated")]
    table = {label: e for label, _, e in cases.synthetic_files(17, 17, 2)}
    for pos in cases.AC_POSITIONS:
        edge = cases._ac_edge(pos)
        assert [table[f"magnitude-ac{pos}-16x{c}"] for c in (edge, edge + 1, -edge, -edge - 1)] == ["pillow", "gated", "pillow", "gated"]


@pytest.mark.parametrize("sub", [0, 1, 2])
def test_parse_on_edited_headers(sub):
    """trl_jpegd_parse agrees with the reference parser and with what Pillow reads on every header edit."""
    for W, H in cases.SYN_SIZES:
        for label, data in cases.header_edit_files(W, H, sub):
            info = jpeg.jpeg_info(data)
            ref = jpegd_ref.parse(data)
            im = Image.open(io.BytesIO(data))
            assert info["supported"] == 1 and info["reason"] == 0, (W, H, label, info)
            assert (info["width"], info["height"]) == im.size == (ref["W"], ref["H"]) == (W, H), label
            assert (info["h_samp"], info["v_samp"]) == _pillow_sampling(im) == (ref["hs"], ref["vs"]) == cases.SUB_HV[sub], label
            assert info["restart_interval"] == ref["ri"] and info["scan_offset"] == ref["scan"], label
            assert (ref["ri"] != 0) == (label in ("fill-bytes-rst", "marker-like-segments-fill", "dri-twice")), label


def test_rgb_component_ids_stay_unsupported():
    for label, data in cases.rgb_id_files():
        info = jpeg.jpeg_info(data)
        assert info["supported"] == 0 and info["reason"] == jpegd_ref.R_COMPONENTS, (label, info)
        with pytest.raises(jpegd_ref.Unsupported) as e:
            jpegd_ref.parse(data)
        assert e.value.reason == jpegd_ref.R_COMPONENTS


@pytest.mark.parametrize("sub", [0, 1, 2])
def test_fuzz_program_synthetic_files(fuzz_program, tmp_path, sub):
    """The shared entropy-decode function, built for the CPU: the coefficients the writer was given, and for edited Pillow files
    the reference's (the IDCT gate is not its business: gated streams decode here too)."""
    program, _ = fuzz_program
    table = [row for size in cases.SYN_SIZES for row in cases.synthetic_files(*size, sub)]
    for (label, data, _), (status, coef) in zip(table, run_fuzz(program, [d for _, d, _ in table], str(tmp_path))):
        assert status == 0, label
        want = cases.written_coefficients(data)
        assert np.array_equal(coef, ref_coefficients(data) if want is None else want), label


def test_damaged_files_that_decode_equal_pillow():
    """Wherever the restatement decodes a damaged stream, it decodes what Pillow decodes."""
    n = 0
    for label, data in cases.damaged_files():
        try:
            got = jpegd_ref.decode(data)
        except (jpegd_ref.Unsupported, jpegd_ref.Irregular):
            continue
        assert np.array_equal(got, cases.pillow_bgr(data)), label
        n += 1
    assert n >= 10
