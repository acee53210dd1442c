"""Scene::toExtPly of the C++ host layer: tests/native/to_ext_ply_cpp.cpp writes 300 patches with Scene::toExtPly (the GPU) and
with the unchanged mo3d::writeExtPly (the host's iostream loop, the pin), for the reference's default arguments (ASCII,
normals, scale, visibility) and for main's "light" set (binary, nothing else; src/main.cpp:164-168).  The files must be
identical; a path that cannot be written returns false, which the program checks itself."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_to_ext_ply_equals_write_ext_ply(tmp_path):
    # the program is built here, against the host layer build() made (as test_gpu_cpp_visualize_depths.py builds its own)
    exe = str(tmp_path / "to_ext_ply_cpp")
    lib = os.path.join(ROOT, "hpmvs_amd")
    subprocess.run(["g++", "-O2", "-std=c++14", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "to_ext_ply_cpp.cpp"),
                    "-o", exe, "-L" + lib, "-lhpmvs_host", "-lhpmvs_amd", "-Wl,-rpath," + lib], check=True, capture_output=True)
    folder = tmp_path / "ply"
    folder.mkdir()
    run = subprocess.run([exe, str(folder)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert "patches 300" in run.stdout and "cannot write" in run.stderr   # (the refused path left its reason)
    for name in ("default", "light", "empty"):
        gpu, host = (folder / f"gpu_{name}.ply").read_bytes(), (folder / f"host_{name}.ply").read_bytes()
        assert gpu == host, name
    text = (folder / "gpu_default.ply").read_bytes()
    assert text.startswith(b"ply\nformat ascii 1.0\nelement vertex 300\n") and b"element point_visibility 300\n" in text
    assert b" 4294967295 " in text and b"e+" in text and b"e-" in text   # an id of -1, both scientific forms
    light = (folder / "gpu_light.ply").read_bytes()
    assert len(light) == len(light.split(b"end_header\n", 1)[0]) + len(b"end_header\n") + 300 * 15
