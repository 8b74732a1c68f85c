"""CPU tests of the Motion-JPEG decoder's rules (no GPU).

``jpegd_ref.decode`` restates in numpy what ``Image.open(f).convert("RGB")`` does through libjpeg-turbo's default decompression
path; these tests pin it to Pillow's bytes over sizes, subsamplings, qualities, content and encoder options chosen to reach every
edge case (partial edge MCUs, one-sample chroma, stuffed 0xFF bytes, optimised tables, restart intervals with RST7 -> RST0), pin
``trl_jpegd_parse`` (host-only C ABI) to what Pillow reads from the same headers, and run the decoder's parser and its shared
entropy-decode function in a stand-alone, sanitized host program over a fixed table of damaged streams."""
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
