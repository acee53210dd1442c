"""Writes tests/golden/g8_jpeg_entropy.npz: the JPEG files (bytes and names only, no pixels) that take the parallel entropy
decode (hpmvs_amd/csrc/kernel_jpeg_entropy.hip) down each of its paths.  Needs Pillow; no test imports Pillow.  The truth
for every file is the host decoder, which tests/golden/g7_jpeg.npz pins to libjpeg.

    python tests/golden/make_golden_jpeg_entropy.py
"""
import io
import os

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
SUBSEQ_BYTES, SUBS_PER_GROUP = 64, 64   # jpeg.hpp: kSubseqBits / 8, kSubsPerGroup


def encode(arr, **kw):
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG", **kw)
    return buf.getvalue()


def scan_of(data):
    """the entropy-coded bytes: behind the SOS header, up to EOI"""
    i = 2
    while True:
        assert data[i] == 0xFF
        m, ln = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        i += 2 + ln
        if m == 0xDA:
            return data[i:data.rindex(b"\xff\xd9")]


def longest_code(data):
    """longest Huffman code length any DHT segment of the file defines"""
    i, longest = 2, 0
    while data[i + 1] != 0xDA:
        m, ln = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        if m == 0xC4:
            k = i + 4
            while k < i + 2 + ln:
                counts = data[k + 1:k + 17]
                longest = max(longest, max(l + 1 for l in range(16) if counts[l]))
                k += 17 + sum(counts)
        i += 2 + ln
    return longest


def main():
    rng = np.random.default_rng(8)
    files = {}

    noise = rng.integers(0, 256, (96, 112, 3), dtype=np.uint8)
    files["noise112x96_420_q95"] = encode(noise, quality=95, subsampling=2)
    assert len(scan_of(files["noise112x96_420_q95"])) > 3 * SUBS_PER_GROUP * SUBSEQ_BYTES   # three workgroups and more

    y, x = np.mgrid[0:256, 0:256]
    grad = np.stack([x, y, (x + y) // 2], -1).astype(np.uint8)
    files["gradient256_420_q1"] = encode(grad, quality=1, subsampling=2)
    n_blocks = (256 // 8) ** 2 * 3 // 2
    per_subseq = n_blocks * SUBSEQ_BYTES / len(scan_of(files["gradient256_420_q1"]))
    print("gradient256_420_q1: %.0f blocks per subsequence" % per_subseq)
    assert per_subseq >= 90           # (a block takes 4 bits at the least: 128 is the most 512 bits can hold; this file reaches 92)

    files["noise64_444_q100_opt"] = encode(rng.integers(0, 256, (64, 64, 3), dtype=np.uint8), quality=100, subsampling=0, optimize=True)
    assert longest_code(files["noise64_444_q100_opt"]) > 9                                  # beyond the 9-bit look-ahead
    assert scan_of(files["noise64_444_q100_opt"]).count(b"\xff\x00") >= 20                  # stuffed FFs

    smooth = (127 + 100 * np.sin(x[:65, :97] / 7.0)[..., None] * np.array([1.0, 0.6, -0.8])).astype(np.uint8)
    smooth = (smooth.astype(int) + rng.integers(-12, 13, smooth.shape)).clip(0, 255).astype(np.uint8)
    files["c96x64_420_rst1"] = encode(smooth[:64, :96], quality=75, subsampling=2, restart_marker_blocks=1)
    rst = [m for m in range(0xD0, 0xD8) for _ in range(scan_of(files["c96x64_420_rst1"]).count(bytes([0xFF, m])))]
    assert len(rst) == 23 and rst.count(0xD7) == 2   # 24 MCUs, a marker between any two: RST7 passed twice, into a third round
    files["c97x65_422_rst5"] = encode(smooth, quality=80, subsampling=1, restart_marker_blocks=5)
    gray = smooth[:64, :64, 0]
    files["g64_norst"] = encode(gray, quality=85)
    files["g40_rst2"] = encode(gray[:40, :40], quality=85, restart_marker_blocks=2)
    for name in ("c96x64_420_rst1", "c97x65_422_rst5", "g40_rst2"):
        assert b"\xff\xdd" in files[name], name                                             # a DRI segment

    names = sorted(files)
    out = {"pillow_version": np.array(PIL.__version__), "names": np.array(names)}
    for n in names:
        out[n + "_jpg"] = np.frombuffer(files[n], np.uint8)
    path = os.path.join(HERE, "g8_jpeg_entropy.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {n: len(files[n]) for n in names})


if __name__ == "__main__":
    main()
