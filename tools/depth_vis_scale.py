#!/usr/bin/env python3
"""Depth maps as jet-coloured JPEG files at production size: one 3840x2160 view's maps (level 0: 1920x1080 cells), filled by
set_depths_batch from seeded patches of every pyramid level.  Times Scene.depth_jpeg for the combined map and for level 0 (the
cells and the pixels stay in HBM; wall clock, median of repeated calls after warm-up), Scene.depth_image alone, and what they
replace: the maps fetched with depth_get_level and coloured on the host by the numpy restatement the tests pin to CImg
(tests/depth_vis_ref.py), then encoded by Pillow when it imports -- else the fetch and the colouring are reported alone.  Also
checks the device's image against the restatement's, and its file against Pillow's, byte for byte.  No threshold rests on the
numbers.  Prints one JSON object and writes it to --out.

    python tools/depth_vis_scale.py [--width 3840 --height 2160] [--out profiles/depth_vis_scale.json]
"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(ts):
    return {"min": float(min(ts)), "median": float(np.median(ts))}


def wall_ms(fn):
    t = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--patches", type=int, default=400000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_vis_scale.json"))
    a = ap.parse_args()
    import torch
    import depth_vis_ref as ref
    from hpmvs_amd import api, synth

    w, h = a.width, a.height
    syn = ref.make_scene(sizes=[(w, h), (w, h)], max_level=5, seed=0xD5)   # (the depth entries read no pixel: random bytes)
    sc = api.Scene(syn, device=0)
    api.depth_reset(sc)
    levels = sc.view_levels[0]
    for l in range(levels):
        seeds = synth.make_seeds(syn, a.patches >> l, start_level=l, seed=synth.SEED + 41 + l)
        batch = api.Batch.from_seeds(seeds)
        batch.ok[:] = 1
        api.set_depths_batch(sc, batch)
    lut = api.depth_colormap()
    res = {"build_id": api.build_id(), "device": torch.cuda.get_device_name(0), "w": w, "h": h, "levels": levels,
           "map_cells": [int(api.depth_level(sc, 0, l).size) for l in range(levels)],
           "filled_cells": [int((api.depth_level(sc, 0, l) < ref.MAX_DEPTH).sum()) for l in range(levels)],
           "reps": a.reps, "warmup": a.warmup, "images": {}}
    try:
        import PIL
        from PIL import Image, features
        res["host_encoder"] = "Pillow %s over libjpeg %s" % (PIL.__version__, features.version("jpg"))

        def host_encode(px):
            f = io.BytesIO()
            Image.fromarray(px).save(f, "JPEG", quality=100, subsampling=2, optimize=False)
            return f.getvalue()
    except ImportError:
        res["host_encoder"] = None
        host_encode = None

    def host_image(level):
        if level is None:
            return ref.image(ref.combined([api.depth_level(sc, 0, l) for l in range(levels)]), lut)[0]
        return ref.image(api.depth_level(sc, 0, level), lut)[0]

    def fetch(level):
        return [api.depth_level(sc, 0, l) for l in (range(levels) if level is None else [level])]

    try:
        for name, level in (("combined", None), ("level0", 0)):
            r = {}
            for _ in range(a.warmup):
                sc.depth_jpeg(0, level)
                sc.depth_image(0, level)
                host_image(level)
            # alternating, so that what else runs on the host falls on all alike
            t = {k: [] for k in ("depth_jpeg_ms", "depth_image_ms", "fetch_ms", "fetch_colour_ms", "fetch_colour_encode_ms")}
            for _ in range(a.reps):
                ms, dev_file = wall_ms(lambda: sc.depth_jpeg(0, level))
                t["depth_jpeg_ms"].append(ms)
                ms, dev_img = wall_ms(lambda: sc.depth_image(0, level))
                t["depth_image_ms"].append(ms)
                t["fetch_ms"].append(wall_ms(lambda: fetch(level))[0])
                ms, img = wall_ms(lambda: host_image(level))
                t["fetch_colour_ms"].append(ms)
                if host_encode:
                    ms, host_file = wall_ms(lambda: host_encode(host_image(level)))
                    t["fetch_colour_encode_ms"].append(ms)
            for k, v in t.items():
                if v:
                    r[k] = stats(v)
            r["file_bytes"] = len(dev_file)
            r["device_image_equals_restatement"] = bool(np.array_equal(dev_img, img))
            if host_encode:
                r["device_file_equals_host_file"] = bool(dev_file == host_file)
            res["images"][name] = r
    finally:
        sc.close()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
