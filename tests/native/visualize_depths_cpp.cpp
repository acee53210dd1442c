// Scene::visualizeDepths end to end (BASELINE.json configs[0], "tiny nvm scene"): read an NVM_V3 model whose cameras point at
// binary PPM images, build the Scene as run_nvm_scene does, refine the seeds, enter their depths with seedTree and write the
// folder with visualizeDepths.  Every depth map is also written raw (int32 rows, cols, then rows * cols floats, column-major)
// into <dump folder>/<view>_<level>.f32, so that the Python test can plant the same maps into a scene of its own and compare
// the files' bytes.  The refusals are checked here: no depth maps yet, and a folder that cannot be created.
//   visualize_depths_cpp <in.nvm> <out folder> <dump folder> <start_level>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <hpmvs/HpmvsOptions.h>
#include <hpmvs/NVMReader.h>
#include <hpmvs/Scene.h>
#include <hpmvs_amd.h>

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    std::vector<mo3d::NVM_Model> models;
    mo3d::NVMReader::readFile(argv[1], models, true);
    if (models.empty()) { fprintf(stderr, "no model\n"); return 3; }
    mo3d::HpmvsOptions options;
    options.START_LEVEL = atoi(argv[4]);
    mo3d::Scene scene;
    if (!scene.addCameras(models[0], options)) { fprintf(stderr, "addCameras failed\n"); return 4; }
    if (!scene.extractCoVisiblilty(models[0], options)) return 5;
    const std::string folder(argv[2]), dump(argv[3]);

    // before the maps exist: false, and the library names the missing call
    if (scene.visualizeDepths(folder.c_str())) { fprintf(stderr, "visualizeDepths ran without depth maps\n"); return 6; }
    if (!strstr(hpmvs_last_error(), "hpmvs_scene_depth_reset")) { fprintf(stderr, "unexpected error text: %s\n", hpmvs_last_error()); return 6; }

    std::vector<mo3d::Ppatch3d> patches;
    if (!scene.initPatches(models[0], options, patches)) { fprintf(stderr, "initPatches failed\n"); return 7; }
    mo3d::Scene::SeedTree tree;
    if (!scene.resetDepths() || !scene.seedTree(patches, options, tree, true)) { fprintf(stderr, "seedTree failed\n"); return 7; }

    // a folder below a regular file cannot be created
    const std::string below = std::string(argv[1]) + "/below_a_file";
    if (scene.visualizeDepths(below.c_str())) {
        fprintf(stderr, "visualizeDepths wrote below a regular file\n");
        return 8;
    }
    if (!scene.visualizeDepths(folder.c_str())) { fprintf(stderr, "visualizeDepths failed\n"); return 9; }

    hpmvs_scene* dev = scene.deviceScene();
    const int levels = scene.cameras_[0].getLevels();
    size_t cells = 0, filled = 0;
    std::vector<float> map;
    for (int v = 0; v < (int)scene.cameras_.size(); v++)
        for (int l = 0; l < levels; l++) {
            int rows = 0, cols = 0;
            if (hpmvs_scene_depth_get_level(dev, v, l, nullptr, 0, &rows, &cols) != HPMVS_OK) { fprintf(stderr, "%s\n", hpmvs_last_error()); return 10; }
            map.assign((size_t)rows * cols, 0.0f);
            if (!map.empty() && hpmvs_scene_depth_get_level(dev, v, l, map.data(), map.size(), &rows, &cols) != HPMVS_OK) { fprintf(stderr, "%s\n", hpmvs_last_error()); return 10; }
            for (float d : map) { cells++; filled += d != 1000.0f; }
            const std::string path = dump + "/" + std::to_string(v) + "_" + std::to_string(l) + ".f32";
            FILE* f = fopen(path.c_str(), "wb");
            const int32_t hd[2] = {rows, cols};
            if (!f || fwrite(hd, 4, 2, f) != 2 || fwrite(map.data(), 4, map.size(), f) != map.size() || fclose(f) != 0) { fprintf(stderr, "cannot write %s\n", path.c_str()); return 11; }
        }
    printf("views %zu levels %d patches %zu cells %zu filled %zu\n", scene.cameras_.size(), levels, patches.size(), cells, filled);
    return 0;
}
