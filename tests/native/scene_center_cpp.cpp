// Scene::getSceneCenter and the gated forms of Scene::initPatches (the C++ host layer) on an NVM model read from files, for
// tests/test_gpu_cpp_scene_center.py, which makes the same calls through hpmvs_amd.api and compares the bytes.  Built by that
// test with g++ against libhpmvs_host.so.
//   scene_center_cpp <in.nvm> <out.bin> <start_level>
// Out (binary): int32 valid, double center[3], double radius of getSceneCenter, then four runs of initPatches:
//   0  the explicit overload at (0, 0, 0; 5), with its stage vector
//   1  initPatches(model, options, out) with FILTER_SCENE_CENTER = true
//   2  the explicit overload at getSceneCenter's values, with its stage vector
//   3  initPatches(model, options, out) with FILTER_SCENE_CENTER = false
// Each run: int32 ok, int32 S and int32 stage[S] (S = 0 where no stage vector was asked for), int32 P, then per patch
// float center[4], normal[4], scale, ncc, color[3], int32 n, int32 images[n].
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <hpmvs/HpmvsOptions.h>
#include <hpmvs/NVMReader.h>
#include <hpmvs/Scene.h>

template <typename T> static void wr(FILE* f, const T& v) { if (fwrite(&v, sizeof(T), 1, f) != 1) { perror("write"); exit(2); } }

static void write_run(FILE* g, bool ok, const std::vector<int>* stage, const std::vector<mo3d::Ppatch3d>& patches) {
    wr(g, (int32_t)ok);
    wr(g, (int32_t)(stage ? stage->size() : 0));
    if (stage) for (int s : *stage) wr(g, (int32_t)s);
    wr(g, (int32_t)patches.size());
    for (const mo3d::Ppatch3d& p : patches) {
        for (int k = 0; k < 4; k++) wr(g, (float)p->center_[k]);
        for (int k = 0; k < 4; k++) wr(g, (float)p->normal_[k]);
        wr(g, (float)p->scale_3dx_); wr(g, (float)p->ncc_);
        for (int k = 0; k < 3; k++) wr(g, (float)p->color_[k]);
        wr(g, (int32_t)p->images_.size());
        for (int id : p->images_) wr(g, (int32_t)id);
    }
}

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: %s <in.nvm> <out.bin> <start_level>\n", argv[0]); return 2; }
    std::vector<mo3d::NVM_Model> models;
    mo3d::NVMReader::readFile(argv[1], models, true);
    if (models.empty()) { fprintf(stderr, "no model\n"); return 3; }
    const mo3d::NVM_Model& model = models[0];
    mo3d::HpmvsOptions options;
    options.START_LEVEL = atoi(argv[3]);
    mo3d::Scene scene;
    if (!scene.addCameras(model, options)) { fprintf(stderr, "addCameras failed\n"); return 4; }
    if (!scene.extractCoVisiblilty(model, options)) return 5;
    FILE* g = fopen(argv[2], "wb");
    if (!g) return 2;

    Eigen::Vector3d center(0.0, 0.0, 0.0);
    double radius = 0.0;
    const bool valid = scene.getSceneCenter(center, radius);
    wr(g, (int32_t)valid);
    for (int k = 0; k < 3; k++) wr(g, (double)center[k]);
    wr(g, radius);

    {
        std::vector<mo3d::Ppatch3d> out;
        std::vector<int> stage;
        const bool ok = scene.initPatches(model, options, out, Eigen::Vector3d(0.0, 0.0, 0.0), 5.0, &stage);
        write_run(g, ok, &stage, out);
    }
    {
        std::vector<mo3d::Ppatch3d> out;
        options.FILTER_SCENE_CENTER = true;
        const bool ok = scene.initPatches(model, options, out);
        write_run(g, ok, nullptr, out);
    }
    {
        std::vector<mo3d::Ppatch3d> out;
        std::vector<int> stage;
        options.FILTER_SCENE_CENTER = false;  // the explicit sphere gates whatever the option says
        const bool ok = valid && scene.initPatches(model, options, out, center, radius, &stage);
        write_run(g, ok, &stage, out);
    }
    {
        std::vector<mo3d::Ppatch3d> out;
        options.FILTER_SCENE_CENTER = false;
        const bool ok = scene.initPatches(model, options, out);
        write_run(g, ok, nullptr, out);
    }
    fclose(g);
    return 0;
}
