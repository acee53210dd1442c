"""Scene::visualizeDepths of the C++ host layer on BASELINE.json configs[0] ("tiny nvm scene"): tests/native/visualize_depths_cpp.cpp
builds the scene from an NVM model with PPM views, refines the seeds, enters their depths (seedTree) and writes the folder; it
also dumps every depth map.  Here the folder must hold exactly the expected files, overview.html must equal the reference's
markup (src/hpmvs/Scene.cpp:436-513) with <cols>x<rows> in the cells of images under 8 pixels on a side, and every .jpg must
equal what Scene.depth_jpeg / Scene.level_jpeg give for a Python scene that holds the same maps."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_gpu_nvm_files import write_nvm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_visualize_depths_writes_the_folder(tiny_scene, tmp_path):
    from hpmvs_amd import api, synth
    # the program is built here, against the host layer build() made (as test_gpu_cpp_save_as_nvm.py builds its own)
    exe = str(tmp_path / "visualize_depths_cpp")
    lib = os.path.join(ROOT, "hpmvs_amd")
    subprocess.run(["g++", "-O2", "-std=c++14", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "visualize_depths_cpp.cpp"),
                    "-o", exe, "-L" + lib, "-lhpmvs_host", "-lhpmvs_amd", "-Wl,-rpath," + lib], check=True, capture_output=True)
    xyz, off, img = synth.make_nvm_points(tiny_scene, 300, start_level=2, noise=1.0)
    for i, v in enumerate(tiny_scene.views):
        with open(tmp_path / ("view%02d.ppm" % i), "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (v.width, v.height) + np.ascontiguousarray(v.rgb).tobytes())
    nvm = tmp_path / "scene.nvm"
    write_nvm(nvm, tiny_scene, xyz, off, img)
    folder, dump = tmp_path / "depths", tmp_path / "maps"
    dump.mkdir()
    run = subprocess.run([exe, str(nvm), str(folder), str(dump), "2"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr
    print("\n" + run.stdout.strip())
    m = re.search(r"views (\d+) levels (\d+) patches (\d+) cells (\d+) filled (\d+)", run.stdout)
    assert m, run.stdout
    n_views, levels, n_patches, filled = int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(5))
    assert n_views == tiny_scene.n_views and n_patches >= 50 and filled >= n_patches
    assert "hpmvs_scene_depth_reset" in run.stderr and "below_a_file" in run.stderr   # the two refusals left their reasons

    # a scene of this test's own with the same maps
    sc = api.Scene(tiny_scene, device=0)
    try:
        assert sc.view_levels == [levels] * n_views
        api.depth_reset(sc)
        shapes = {}
        for v in range(n_views):
            for l in range(levels):
                raw = open(dump / ("%d_%d.f32" % (v, l)), "rb").read()
                rows, cols = np.frombuffer(raw[:8], np.int32)
                data = np.frombuffer(raw[8:], np.float32).reshape(cols, rows)
                assert api.depth_level(sc, v, l).shape == (cols, rows)
                api.depth_set_level(sc, v, l, data)
                shapes[(v, l)] = (int(cols), int(rows))
        assert any(min(s) < 8 for s in shapes.values()) and any(min(s) >= 8 for s in shapes.values())
        # the reference's markup and column order
        html = "<!DOCTYPE html><html><head>"
        html += "<style>table, th, td {border: 1px solid black;border-collapse: collapse;}"
        html += "img { height: auto; width: 100%;}"
        html += "th, td {padding: 5px;text-align: left;}</style>"
        html += "</head><body>"
        html += "<h2>Depth Images:</h2>"
        html += "<table style=\"width:100%\">"
        html += "<tr><th>Color</th><th>Combined</th>" + "".join("<th>L%d</th>" % l for l in range(levels)) + "</tr>"
        files = {}
        for v in range(n_views):
            html += "<tr>"
            col = sc.level(v, 1)
            cells = [("%d_col" % v, (col.shape[1], col.shape[0]), lambda v=v: sc.level_jpeg(v, 1, 100)),
                     ("%d_all" % v, shapes[(v, 0)], lambda v=v: sc.depth_jpeg(v, None, 100))]
            cells += [("%d_%d" % (v, l), shapes[(v, l)], lambda v=v, l=l: sc.depth_jpeg(v, l, 100)) for l in range(levels)]
            for name, (w, h), make in cells:
                if w < 8 or h < 8:
                    html += "<td>%dx%d</td>" % (w, h)
                else:
                    html += "<td><img src=\"%s.jpg\"/></td>" % name
                    files[name + ".jpg"] = make()
            html += "</tr>"
        html += "</table></body></html>"
        assert sorted(os.listdir(folder)) == sorted(list(files) + ["overview.html"])
        assert open(folder / "overview.html", "rb").read() == html.encode()
        for name, data in files.items():
            assert open(folder / name, "rb").read() == data, name
        # the images are not blank: the combined map of view 0 shows the patches' depths
        assert len(np.unique(sc.depth_image(0).reshape(-1, 3), axis=0)) > 10
    finally:
        sc.close()
