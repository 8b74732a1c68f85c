"""Writes tests/golden/sample_clip_skeleton.mp4.gz from the reference project's sample clip (a fragmented 640x360 30 fps H.264 mp4,
BASELINE configs[0]).  Run:  python tests/golden/make_mp4_skeleton.py <path to the sample .mp4>

The skeleton is the clip with its pictures taken out and nothing else changed: every byte outside the mdat boxes (ftyp, moov,
moof/trun, mfra) is kept, as are the mdat headers and, inside each video sample, every NAL unit's length prefix and header byte
(its nal_unit_type).  All other bytes -- the coded slices and the audio samples -- become zero.  File size, box layout, sample
offsets and sizes are those of the original, so mp4probe sees the same container; gzip shrinks the zeros to a few kB."""
import gzip
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import truely_amd  # noqa: E402,F401  (import shim for the hyphenated package directory)
from truely_amd import mp4probe  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sample_clip_skeleton.mp4.gz")


def skeleton(buf: bytes) -> bytes:
    info = mp4probe._probe(buf)
    assert info is not None and info.nal_length_size == 4
    out = bytearray(buf)
    for typ, a, b, _ in mp4probe._boxes(buf, 0, len(buf)):
        if typ == b"mdat":
            out[a:b] = bytes(b - a)
    for off, size in info.sample_ranges:
        q = off
        while q + 5 <= off + size:
            ln = int.from_bytes(buf[q:q + 4], "big")
            out[q:q + 5] = buf[q:q + 5]
            q += 4 + ln
        assert q == off + size
    return bytes(out)


def main():
    src = sys.argv[1]
    data = skeleton(open(src, "rb").read())
    with open(OUT, "wb") as f:
        f.write(gzip.compress(data, compresslevel=9, mtime=0))
    print(f"{OUT}: {os.path.getsize(OUT)} bytes ({len(data)} uncompressed)")


if __name__ == "__main__":
    main()
