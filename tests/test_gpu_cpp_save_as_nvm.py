"""Scene::saveAsNVM of the C++ host layer on BASELINE.json configs[0] ("tiny nvm scene"): tests/native/save_as_nvm_cpp.cpp builds
the scene from an NVM model with PPM views, refines the seeds, writes the folder and checks project.nvm itself (read back
through NVMReader::readFile: counts, r == 0, unit quaternions, rotation rows, points, measurements, and that the written
folder loads as a scene); here every imgs/<i>.jpg is compared with Scene.level_jpeg of the Python scene built from the same
inputs, and the counts with the file."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_gpu_nvm_files import read_nvm, write_nvm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_save_as_nvm_writes_the_scene_and_it_loads_again(tiny_scene, gpu_scene, tmp_path):
    from hpmvs_amd import synth
    # the program is built here, against the host layer build() made (as tests/jpeg_ref.py builds its restatement)
    exe = str(tmp_path / "save_as_nvm_cpp")
    lib = os.path.join(ROOT, "hpmvs_amd")
    subprocess.run(["g++", "-O2", "-std=c++14", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "save_as_nvm_cpp.cpp"),
                    "-o", exe, "-L" + lib, "-lhpmvs_host", "-lhpmvs_amd", "-Wl,-rpath," + lib], check=True, capture_output=True)
    xyz, off, img = synth.make_nvm_points(tiny_scene, 300, start_level=2, noise=1.0)
    for i, v in enumerate(tiny_scene.views):
        with open(tmp_path / ("view%02d.ppm" % i), "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (v.width, v.height) + np.ascontiguousarray(v.rgb).tobytes())
    nvm = tmp_path / "scene.nvm"
    write_nvm(nvm, tiny_scene, xyz, off, img)
    folder = tmp_path / "saved"
    run = subprocess.run([exe, str(nvm), str(folder), "2"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr
    print("\n" + run.stdout.strip())
    m = re.search(r"cameras (\d+) points (\d+) measurements (\d+) quaternion_norm_error (\S+) row_error (\S+) reloaded (\d+)", run.stdout)
    assert m, run.stdout
    n_cams, n_points, n_meas, reloaded = int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(6))
    assert n_cams == reloaded == tiny_scene.n_views and n_points >= 50 and n_meas >= n_points
    assert float(m.group(4)) <= 1e-12 and float(m.group(5)) <= 1e-6
    # the views: the undistorted level 0 as the library encodes it where it lies
    for i in range(tiny_scene.n_views):
        data = open(folder / "imgs" / ("%d.jpg" % i), "rb").read()
        assert data == gpu_scene.level_jpeg(i, 0), f"view {i}"
    # Image::saveJpeg of view 0's pixels: k1 == 0, so they are level 0 (the refused quality left a message, no crash)
    assert open(folder / "view0_pixels.jpg", "rb").read() == gpu_scene.level_jpeg(0, 0)
    assert "quality" in run.stderr
    # project.nvm as a plain reader sees it: the model and the empty one behind it
    cams, pts = read_nvm(folder / "project.nvm")
    assert len(cams) == n_cams and len(pts) == n_points
    for i, (name, par) in enumerate(cams):
        assert name == "imgs/%d.jpg" % i and par[8] == 0.0                    # r
        assert abs(np.linalg.norm(par[1:5]) - 1.0) <= 1e-12
        assert np.allclose(par[5:8], tiny_scene.views[i].c, rtol=0, atol=1e-5)   # the float32 centre
    assert open(folder / "project.nvm").read().split()[-2:] == ["0", "0"]
