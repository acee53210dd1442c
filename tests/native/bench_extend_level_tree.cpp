// One extend level at PRODUCTION size through the C++ host layer, against the real octree and beside the grid keys:
// PatchOptimizer::extendLevelTree (ONE hpmvs_extend_tree_batch, then the walk) and PatchOptimizer::extendLevel (candidate
// centres, LeafKeyFn per point, one expandBatch, then the same walk) on the same parents, each from resetDepths +
// setDepths(parents), timed.  Run with HPMVS_LEVEL_TIMES=1 for both breakdowns (stderr).  tools/extend_level_tree_scale.py
// builds it, writes its input and reads the JSON line it prints.
//   bench_extend_level_tree <dump>
// Dump: the format of tests/test_gpu_cpp_interface.py (_dump_scene) -- its patches are the level's parents, leaves of ONE node
// level in the scheduler's order --, then float width, float root[4] (c_, width_), int32 nb, uint64 branchKeys[nb], int32 nl,
// uint64 leafKeys[nl].  The two loops decide different things by design (tests/test_gpu_extend_level_tree.py): only their times
// stand beside each other.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <unordered_set>
#include <vector>

#include <hpmvs/HpmvsOptions.h>
#include <hpmvs/PatchOptimizer.h>
#include <hpmvs/Scene.h>

template <typename T> static T rd(FILE* f) { T v; if (fread(&v, sizeof(T), 1, f) != 1) { perror("read"); exit(2); } return v; }
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s <dump>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    mo3d::HpmvsOptions options;
    mo3d::Scene scene;
    mo3d::NVM_Model model;
    const int nv = rd<int>(f);
    model.cameras.reserve(nv);   // (an Image keeps a pointer to its NVM camera)
    std::vector<unsigned char> pix;
    for (int i = 0; i < nv; i++) {
        mo3d::NVM_Camera cam;
        cam.filename = "view" + std::to_string(i);
        const int w = rd<int>(f), h = rd<int>(f);
        cam.f = rd<double>(f);
        for (int k = 0; k < 4; k++) cam.rq[k] = rd<double>(f);
        for (int k = 0; k < 3; k++) cam.c[k] = rd<double>(f);
        cam.r = 0.0;
        model.cameras.push_back(cam);
        pix.resize((size_t)w * h * 3);
        if (fread(pix.data(), 1, pix.size(), f) != pix.size()) return 2;
        scene.cameras_.emplace_back();
        scene.images_.emplace_back();
        scene.dict_[cam.filename] = i;
        scene.images_[i].init(&model.cameras[i], options.MAXLEVEL);
        scene.images_[i].setPixels(w, h, pix.data());   // (copies)
        scene.cameras_[i].init(&model.cameras[i], scene.images_[i].getWidth(), scene.images_[i].getHeight(), options.MAXLEVEL);
    }
    scene.covis_.resize(nv);
    for (int i = 0; i < nv; i++) {
        const int m = rd<int>(f);
        for (int k = 0; k < m; k++) scene.covis_[i].push_back(rd<int>(f));
    }
    const int n = rd<int>(f);
    std::vector<mo3d::Patch3d> base(n);
    for (int i = 0; i < n; i++) {
        mo3d::Patch3d& p = base[i];
        for (int k = 0; k < 4; k++) p.center_[k] = rd<float>(f);
        for (int k = 0; k < 4; k++) p.normal_[k] = rd<float>(f);
        p.scale_3dx_ = rd<float>(f);
        const int m = rd<int>(f);
        for (int k = 0; k < m; k++) p.images_.push_back(rd<int>(f));
        p.expanded_ = false;
    }
    const float width = rd<float>(f);
    mo3d::OctreeIndex tree0;
    for (int k = 0; k < 3; k++) tree0.rootCenter[k] = rd<float>(f);
    tree0.rootWidth = rd<float>(f);
    tree0.branchKeys.resize(rd<int32_t>(f));
    for (uint64_t& k : tree0.branchKeys) k = rd<uint64_t>(f);
    tree0.leafKeys.resize(rd<int32_t>(f));
    for (uint64_t& k : tree0.leafKeys) k = rd<uint64_t>(f);
    fclose(f);

    mo3d::PatchOptimizer opt(options, &scene);
    std::vector<const mo3d::Patch3d*> parents(n);
    for (int i = 0; i < n; i++) parents[i] = &base[i];
    auto fresh = [&]() { return scene.resetDepths() && scene.setDepths(parents.data(), parents.size()); };
    auto grid = [&](const Eigen::Vector4f& p) {
        const long long ix = (long long)std::floor(p[0] / width), iy = (long long)std::floor(p[1] / width), iz = (long long)std::floor(p[2] / width);
        return (uint64_t)(((ix + (1 << 20)) << 42) | ((iy + (1 << 20)) << 21) | (iz + (1 << 20)));
    };
    double secs[2][2];
    size_t accepted[2][2], border = 0;
    int waves[2][2];
    for (int rep = 0; rep < 2; rep++) {   // (the first pass of each warms the pinned-memory cache and the workspaces)
        {
            if (!fresh()) { fprintf(stderr, "depth setup failed\n"); return 1; }
            std::unordered_set<uint64_t> occ;
            for (const mo3d::Patch3d& p : base) occ.insert(grid(p.center_));
            mo3d::PatchOptimizer::LevelResult L;
            const double t0 = now();
            if (!opt.extendLevel(parents.data(), parents.size(), width, occ, 1.0f, false, L)) { fprintf(stderr, "extendLevel failed\n"); return 1; }
            secs[rep][0] = now() - t0; accepted[rep][0] = L.accepted.size(); waves[rep][0] = L.waves;
        }
        {
            if (!fresh()) { fprintf(stderr, "depth setup failed\n"); return 1; }
            mo3d::OctreeIndex tree = tree0;
            mo3d::PatchOptimizer::LevelResult L;
            const double t0 = now();
            if (!opt.extendLevelTree(parents.data(), parents.size(), width, tree, 1.0f, false, L)) { fprintf(stderr, "extendLevelTree failed\n"); return 1; }
            secs[rep][1] = now() - t0; accepted[rep][1] = L.accepted.size(); waves[rep][1] = L.waves; border = L.border.size();
        }
    }
    printf("{\"parents\": %d, \"candidates\": %d, \"width\": %.9g, \"extendLevel_s\": [%.4f, %.4f], \"extendLevelTree_s\": [%.4f, %.4f], "
           "\"extendLevel_accepted\": %zu, \"extendLevelTree_accepted\": %zu, \"extendLevelTree_border\": %zu, \"extendLevel_waves\": %d, "
           "\"extendLevelTree_waves\": %d}\n", n, 6 * n, (double)width, secs[0][0], secs[1][0], secs[0][1], secs[1][1], accepted[1][0],
           accepted[1][1], border, waves[1][0], waves[1][1]);
    return 0;
}
