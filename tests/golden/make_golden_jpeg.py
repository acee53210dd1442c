"""Writes tests/golden/g7_jpeg.npz: JPEG files encoded with Pillow (libjpeg-turbo) from seeded numpy images, Pillow's
own decode of each as the expected pixels, files the decoder must refuse, and the three views of a synthetic scene as
JPEG bytes.  Run on a machine with Pillow:  python tests/golden/make_golden_jpeg.py
No test imports Pillow; the versions used are recorded in the file."""
import io
import os
import sys
import tempfile

import numpy as np
import PIL
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hpmvs_amd import synth  # noqa: E402
from jpeg_ref import HPMVS_ERR_ARG, HPMVS_ERR_UNSUPPORTED, HostJpeg  # noqa: E402

# name: (W, H, Pillow subsampling (0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0, None = grayscale), quality, save options)
ENTRIES = [
    ("c16x16_444_q90", 16, 16, 0, 90, {}),
    ("c37x29_420_q75", 37, 29, 2, 75, {}),
    ("c37x29_422_q75", 37, 29, 1, 75, {}),
    ("c41x23_420_q5", 41, 23, 2, 5, {}),
    ("c33x17_420_q100", 33, 17, 2, 100, {}),
    ("c17x33_420_q50", 17, 33, 2, 50, {}),
    ("c64x48_420_q1", 64, 48, 2, 1, {}),
    ("c40x24_420_q80_rst3", 40, 24, 2, 80, dict(restart_marker_blocks=3)),
    ("c49x31_422_q30_rstrow", 49, 31, 1, 30, dict(restart_marker_rows=1)),
    ("c40x24_444_q80_opt", 40, 24, 0, 80, dict(optimize=True)),
    ("c8x8_420_q95", 8, 8, 2, 95, {}),
    ("g19x21_q85", 19, 21, None, 85, {}),
    ("c200x136_420_q85", 200, 136, 2, 85, {}),
]
SAMPLING = {0: (1, 1), 1: (2, 1), 2: (2, 2), None: (1, 1)}


def image(rng, w, h, noise):
    """smooth waves plus noise: low and high frequencies, values up to both ends of the range"""
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([127 + 120 * np.sin(x / 3.1 + y / 5.0), 127 + 120 * np.cos(x / 4.7 - y / 2.3), (x * 7 + y * 13) % 256], -1)
    return np.clip(a + rng.normal(0, noise, (h, w, 3)), 0, 255).astype(np.uint8)


def encode(a, sub, q, kw):
    f = io.BytesIO()
    if sub is None:
        Image.fromarray(a[..., 0]).save(f, "JPEG", quality=q, **kw)
    else:
        Image.fromarray(a).save(f, "JPEG", quality=q, subsampling=sub, **kw)
    return f.getvalue()


def pillow_rgb(b):
    return np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))


def main():
    rng = np.random.default_rng(7)
    out = {"pillow_version": np.array(PIL.__version__), "libjpeg_version": np.array(str(features.version("jpg")))}
    host = HostJpeg(tempfile.mkdtemp())
    names, info, ac_seen = [], [], np.zeros(64, bool)
    for k, (name, w, h, sub, q, kw) in enumerate(ENTRIES):
        b = encode(image(rng, w, h, 20 + 35 * (k % 3)), sub, q, kw)
        rgb = pillow_rgb(b)
        assert rgb.shape == (h, w, 3)
        names.append(name)
        info.append((w, h, 1 if sub is None else 3) + SAMPLING[sub])
        out[name + "_jpg"] = np.frombuffer(b, np.uint8)
        out[name + "_rgb"] = rgb
        ac_seen |= host.nonzero_positions(b) > 0
        if "rst" in name:
            assert any(bytes([0xFF, 0xD0 + r]) in b for r in range(8)), name
            assert b"\xff\xdd" in b, name
        if name == "c64x48_420_q1":
            assert rgb.min() == 0 and rgb.max() == 255, "the q1 entry must reach both clamps"
    assert ac_seen[1:].all(), "every AC position must occur in some entry"
    out["names"] = np.array(names)
    out["info"] = np.array(info, np.int32)

    base = out["c37x29_420_q75_jpg"].tobytes()
    refuse = []
    f = io.BytesIO()
    Image.fromarray(image(rng, 32, 24, 30)).save(f, "JPEG", quality=80, progressive=True)
    refuse.append(("progressive", f.getvalue(), HPMVS_ERR_UNSUPPORTED, "progressive"))
    f = io.BytesIO()
    Image.fromarray(np.dstack([image(rng, 24, 16, 30), image(rng, 24, 16, 30)[..., :1]]), "CMYK").save(f, "JPEG", quality=80)
    refuse.append(("cmyk", f.getvalue(), HPMVS_ERR_UNSUPPORTED, "four components"))
    sos = base.index(b"\xff\xda")
    refuse.append(("cut_in_entropy_data", base[: sos + 14 + (len(base) - sos - 14) // 2], HPMVS_ERR_ARG, "truncated"))
    sof = base.index(b"\xff\xc0")
    zero_h = bytearray(base)
    zero_h[sof + 5] = zero_h[sof + 6] = 0
    refuse.append(("height_zero", bytes(zero_h), HPMVS_ERR_ARG, "zero width or height"))
    refuse.append(("random_after_soi", b"\xff\xd8" + rng.integers(0, 256, 64, dtype=np.uint8).tobytes(), HPMVS_ERR_ARG, "marker"))
    for name, b, _, _ in refuse:
        out[name + "_jpg"] = np.frombuffer(b, np.uint8)
    out["refuse_names"] = np.array([r[0] for r in refuse])
    out["refuse_codes"] = np.array([r[2] for r in refuse], np.int32)
    out["refuse_words"] = np.array([r[3] for r in refuse])   # a word the error message carries
    # Pillow itself refuses or pads these only in part: nothing of its output is recorded for them

    W, H = 640, 480   # the tests' tiny_scene size
    sc = synth.make_scene(3, W, H, n_waves=24)
    for i, v in enumerate(sc.views):
        out["scene_view%d_jpg" % i] = np.frombuffer(encode(np.ascontiguousarray(v.rgb), 2, 90, {}), np.uint8)
    out["scene_size"] = np.array([W, H, 3], np.int32)

    path = os.path.join(HERE, "g7_jpeg.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; Pillow", PIL.__version__, "libjpeg", features.version("jpg"))
    assert os.path.getsize(path) < 700 * 1024


if __name__ == "__main__":
    main()
