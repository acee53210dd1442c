// Scene::seedTree (the C++ host layer) on a dumped state, for tests/test_gpu_cpp_seed_tree.py, which runs hpmvs_amd.frontier's
// seed_tree on the same state and compares the bytes.  Built by that test with g++ against libhpmvs_host.so.
//   seed_tree_cpp <dump> <out>
// Dump: the scene and patches of tests/test_gpu_cpp_interface.py (_dump_scene), then int32 PATCH_INIT_MAXLEVEL.
// Out (binary), after resetDepths + seedTree(patches, options, tree, true): float rootCenter[3], rootWidth, scaleFloor,
// float scale_3dx_[n], int32 R, int32 L, int32 rows[R], int32 cellStart[L + 1], float cellCenter[L][3], float cellWidth[L],
// int32 cellLevel[L], float patchCenter[L][3], the maps: per view, per pyramid level, int32 rows, int32 cols,
// float depth[rows * cols] (hpmvs_scene_depth_get_level's order).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <hpmvs/HpmvsOptions.h>
#include <hpmvs/Scene.h>
#include <hpmvs_amd.h>

template <typename T> static T rd(FILE* f) { T v; if (fread(&v, sizeof(T), 1, f) != 1) { perror("read"); exit(2); } return v; }
template <typename T> static void wr(FILE* f, const T& v) { if (fwrite(&v, sizeof(T), 1, f) != 1) { perror("write"); exit(2); } }
template <typename T> static void wrv(FILE* f, const std::vector<T>& v) { if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { perror("write"); exit(2); } }

static bool write_maps(FILE* g, const mo3d::Scene& scene) {
    hpmvs_scene* dev = scene.deviceScene();
    if (!dev) return false;
    for (size_t v = 0; v < scene.cameras_.size(); v++)
        for (int l = 0; l < scene.cameras_[v].getLevels(); l++) {
            int rows = 0, cols = 0;
            if (hpmvs_scene_depth_get_level(dev, (int)v, l, nullptr, 0, &rows, &cols) != HPMVS_OK) return false;
            std::vector<float> d((size_t)rows * cols);
            if (hpmvs_scene_depth_get_level(dev, (int)v, l, d.data(), d.size(), &rows, &cols) != HPMVS_OK) return false;
            wr(g, (int32_t)rows); wr(g, (int32_t)cols); wrv(g, d);
        }
    return true;
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s <dump> <out>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    mo3d::HpmvsOptions options;
    mo3d::Scene scene;
    mo3d::NVM_Model model;
    const int nv = rd<int>(f);
    std::vector<std::vector<unsigned char> > pix(nv);
    std::vector<int> W(nv), H(nv);
    for (int i = 0; i < nv; i++) {
        mo3d::NVM_Camera cam;
        cam.filename = "view" + std::to_string(i);
        W[i] = rd<int>(f); H[i] = rd<int>(f);
        cam.f = rd<double>(f);
        for (int k = 0; k < 4; k++) cam.rq[k] = rd<double>(f);
        for (int k = 0; k < 3; k++) cam.c[k] = rd<double>(f);
        cam.r = 0.0;
        pix[i].resize((size_t)W[i] * H[i] * 3);
        if (fread(pix[i].data(), 1, pix[i].size(), f) != pix[i].size()) return 2;
        model.cameras.push_back(cam);
    }
    for (int i = 0; i < nv; i++) {
        scene.cameras_.emplace_back();
        scene.images_.emplace_back();
        scene.dict_[model.cameras[i].filename] = i;
        scene.images_[i].init(&model.cameras[i], options.MAXLEVEL);
        scene.images_[i].setPixels(W[i], H[i], pix[i].data());
        scene.cameras_[i].init(&model.cameras[i], scene.images_[i].getWidth(), scene.images_[i].getHeight(), options.MAXLEVEL);
    }
    scene.covis_.resize(nv);
    for (int i = 0; i < nv; i++) {
        const int m = rd<int>(f);
        for (int k = 0; k < m; k++) scene.covis_[i].push_back(rd<int>(f));
    }
    const int n = rd<int>(f);
    std::vector<mo3d::Ppatch3d> patches(n);
    for (int i = 0; i < n; i++) {
        patches[i].reset(new mo3d::Patch3d);
        mo3d::Patch3d& p = *patches[i];
        for (int k = 0; k < 4; k++) p.center_[k] = rd<float>(f);
        for (int k = 0; k < 4; k++) p.normal_[k] = rd<float>(f);
        p.scale_3dx_ = rd<float>(f);
        const int m = rd<int>(f);
        for (int k = 0; k < m; k++) p.images_.push_back(rd<int>(f));
        p.expanded_ = false;
    }
    options.PATCH_INIT_MAXLEVEL = rd<int32_t>(f);
    fclose(f);

    FILE* g = fopen(argv[2], "wb");
    if (!g) return 2;
    mo3d::Scene::SeedTree t;
    if (!scene.resetDepths() || !scene.seedTree(patches, options, t, true)) { fprintf(stderr, "seedTree failed\n"); return 1; }
    for (int k = 0; k < 3; k++) wr(g, t.rootCenter[k]);
    wr(g, t.rootWidth); wr(g, t.scaleFloor);
    for (int i = 0; i < n; i++) wr(g, patches[i]->scale_3dx_);
    wr(g, (int32_t)t.rows.size()); wr(g, (int32_t)t.leaves());
    wrv(g, t.rows); wrv(g, t.cellStart); wrv(g, t.cellCenter); wrv(g, t.cellWidth); wrv(g, t.cellLevel); wrv(g, t.patchCenter);
    if (!write_maps(g, scene)) { fprintf(stderr, "maps failed\n"); return 1; }
    fclose(g);
    return 0;
}
