"""Writes tests/golden/g8_jpeg_enc.npz: seeded RGB inputs and, per (input, quality), the file Pillow (libjpeg-turbo) writes
for it with quality=q, subsampling=2 (4:2:0), optimize=False -- what CImg's save_jpeg amounts to -- plus Pillow's decode of
two of the files.  Run on a machine with Pillow:  python tests/golden/make_golden_jpeg_enc.py
(--dump PATH also writes the raw cases for the stand-alone program of tests/jpeg_enc_host.cpp.)
No test imports Pillow; the versions used are recorded in the file.  The asserts keep the set covering the paths the
encoder has: the counts come from the host restatement walking the very files it reproduced."""
import io
import os
import struct
import sys
import tempfile

import numpy as np
import PIL
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from jpeg_enc_ref import HostJpegEnc  # noqa: E402

SIZES = [(16, 16), (8, 8), (24, 40), (17, 9), (40, 24), (33, 10), (250, 130), (9, 33)]   # (W, H)
QUALITIES = [100, 90, 50, 10]
DECODED = ["noise_17x9_q90", "smooth_250x130_q100"]


def noise(rng, w, h):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def smooth(rng, w, h):
    y, x = np.mgrid[0:h, 0:w]
    ph = rng.uniform(0, 6.28, 3)
    a = np.stack([127 + 120 * np.sin(x / 9.1 + y / 15.0 + ph[0]), 127 + 120 * np.cos(x / 14.7 - y / 7.3 + ph[1]),
                  127 + 100 * np.sin((x + 2 * y) / 23.0 + ph[2])], -1)
    return np.clip(a, 0, 255).astype(np.uint8)


def encode(a, q):
    f = io.BytesIO()
    Image.fromarray(a).save(f, "JPEG", quality=q, subsampling=2, optimize=False)
    return f.getvalue()


def main():
    rng = np.random.default_rng(8)
    out = {"pillow_version": np.array(PIL.__version__), "libjpeg_version": np.array(str(features.version("jpg")))}
    inputs, cases = [], []   # cases: (name, input index, quality)
    for w, h in SIZES:
        for kind, make in (("noise", noise), ("smooth", smooth)):
            inputs.append(make(rng, w, h))
            cases += [("%s_%dx%d_q%d" % (kind, w, h, q), len(inputs) - 1, q) for q in QUALITIES]
    yy, xx = np.mgrid[0:40, 0:56]
    inputs.append(np.repeat((((yy // 8 + xx // 8) & 1) * 255).astype(np.uint8)[..., None], 3, -1))   # 8x8-block checkerboard
    cases.append(("checker_56x40_q100", len(inputs) - 1, 100))
    inputs.append(np.full((21, 35, 3), (200, 30, 90), np.uint8))
    cases.append(("constant_35x21_q100", len(inputs) - 1, 100))
    cases.append(("constant_35x21_q50", len(inputs) - 1, 50))

    host = HostJpegEnc(tempfile.mkdtemp())
    seen = dict(stuffed=0, zrl=0, dc10=0, pad=0, right=0, bottom=0, even_h=0, odd_h=0)
    for name, i, q in cases:
        a = inputs[i]
        b = encode(a, q)
        rc, mine, st, msg, intact = host.encode(a, q)
        assert rc == 0 and intact and mine == b, "%s: the host restatement does not reproduce Pillow's file (%d %s)" % (name, rc, msg)
        assert b.count(b"\xff\x00") >= st["stuffed"]
        out[name + "_jpg"] = np.frombuffer(b, np.uint8)
        h = a.shape[0]
        seen["stuffed"] += st["stuffed"] > 0
        seen["zrl"] += st["zrl"] > 0
        seen["dc10"] += st["dc_category"] >= 10
        seen["pad"] += st["pad_bits"] > 0
        seen["right"] += st["right_dummies"] > 0
        seen["bottom"] += st["bottom_dummies"] > 0
        seen["even_h"] += h % 16 != 0 and h % 2 == 0
        seen["odd_h"] += h % 2 == 1
    for k, v in seen.items():
        assert v > 0, "no case covers " + k
    for i, a in enumerate(inputs):
        out["%d_rgb" % i] = a
    out["names"] = np.array([c[0] for c in cases])
    out["input_of"] = np.array([c[1] for c in cases], np.int32)
    out["quality"] = np.array([c[2] for c in cases], np.int32)
    for name in DECODED:
        out[name + "_dec"] = np.asarray(Image.open(io.BytesIO(out[name + "_jpg"].tobytes())).convert("RGB"))
    out["decoded_names"] = np.array(DECODED)

    path = os.path.join(HERE, "g8_jpeg_enc.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(cases), "cases; Pillow", PIL.__version__, "libjpeg", features.version("jpg"), seen)
    assert os.path.getsize(path) < 900 * 1024
    if "--dump" in sys.argv:
        with open(sys.argv[sys.argv.index("--dump") + 1], "wb") as f:
            for name, i, q in cases:
                a = inputs[i]
                f.write(struct.pack("<iii", a.shape[1], a.shape[0], q))
                f.write(a.tobytes())


if __name__ == "__main__":
    main()
