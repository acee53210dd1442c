// One extend level over ALL subtrees of a partition at PRODUCTION size through the C++ host layer: the per-tree loop of
// PatchOptimizer::extendLevelTree (one hpmvs_extend_tree_batch and one walk per subtree, in list order) beside ONE
// PatchOptimizer::extendLevelForest (one hpmvs_extend_forest_batch, one walk) on the same parents, each from resetDepths +
// setDepths(parents), timed.  Run with HPMVS_LEVEL_TIMES=1 for the breakdowns (stderr).  tools/extend_forest_scale.py builds it,
// writes its input and reads the JSON line it prints.
//   bench_extend_level_forest <dump>
// Dump: the format of tests/test_gpu_cpp_interface.py (_dump_scene) -- its patches are the level's parents, tree after tree --,
// then float width, int32 parentTree[n] (non-decreasing), int32 nTrees and per tree float root[4] (c_, width_), int32 nb,
// uint64 branchKeys[nb], int32 nl, uint64 leafKeys[nl].  The two must decide the same things: accepted, border and every stage
// are compared here, and the JSON says so.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
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
    std::vector<int32_t> parentTree(n);
    for (int32_t& t : parentTree) t = rd<int32_t>(f);
    mo3d::OctreeForest forest0;
    forest0.trees.resize(rd<int32_t>(f));
    for (mo3d::OctreeIndex& t : forest0.trees) {
        for (int k = 0; k < 3; k++) t.rootCenter[k] = rd<float>(f);
        t.rootWidth = rd<float>(f);
        t.branchKeys.resize(rd<int32_t>(f));
        for (uint64_t& k : t.branchKeys) k = rd<uint64_t>(f);
        t.leafKeys.resize(rd<int32_t>(f));
        for (uint64_t& k : t.leafKeys) k = rd<uint64_t>(f);
    }
    fclose(f);

    mo3d::PatchOptimizer opt(options, &scene);
    std::vector<const mo3d::Patch3d*> parents(n);
    for (int i = 0; i < n; i++) parents[i] = &base[i];
    auto fresh = [&]() { return scene.resetDepths() && scene.setDepths(parents.data(), parents.size()); };
    double secs[2][2];
    size_t accepted[2] = {0, 0}, border[2] = {0, 0};
    int waves[2] = {0, 0}, treesWithParents = 0;
    bool same = true;
    for (int rep = 0; rep < 2; rep++) {   // (the first pass of each warms the pinned-memory cache and the workspaces)
        std::vector<int> loopStage;
        {
            if (!fresh()) { fprintf(stderr, "depth setup failed\n"); return 1; }
            mo3d::OctreeForest forest = forest0;
            accepted[0] = border[0] = 0; waves[0] = 0; treesWithParents = 0;
            const double t0 = now();
            for (int a = 0; a < n;) {
                int b = a;
                while (b < n && parentTree[b] == parentTree[a]) b++;
                mo3d::PatchOptimizer::LevelResult L;
                if (!opt.extendLevelTree(parents.data() + a, (size_t)(b - a), width, forest.trees[(size_t)parentTree[a]], 1.0f, false, L)) {
                    fprintf(stderr, "extendLevelTree failed\n");
                    return 1;
                }
                accepted[0] += L.accepted.size(); border[0] += L.border.size(); waves[0] += L.waves; treesWithParents++;
                loopStage.insert(loopStage.end(), L.stage.begin(), L.stage.end());
                a = b;
            }
            secs[rep][0] = now() - t0;
        }
        {
            if (!fresh()) { fprintf(stderr, "depth setup failed\n"); return 1; }
            mo3d::OctreeForest forest = forest0;
            mo3d::PatchOptimizer::LevelResult L;
            const double t0 = now();
            if (!opt.extendLevelForest(parents.data(), parentTree.data(), (size_t)n, width, forest, 1.0f, false, L)) { fprintf(stderr, "extendLevelForest failed\n"); return 1; }
            secs[rep][1] = now() - t0;
            accepted[1] = L.accepted.size(); border[1] = L.border.size(); waves[1] = L.waves;
            same = same && L.stage == loopStage;
        }
    }
    printf("{\"parents\": %d, \"candidates\": %d, \"trees\": %zu, \"trees_with_parents\": %d, \"width\": %.9g, \"extendLevelTree_loop_s\": [%.4f, %.4f], "
           "\"extendLevelForest_s\": [%.4f, %.4f], \"loop_accepted\": %zu, \"forest_accepted\": %zu, \"loop_border\": %zu, \"forest_border\": %zu, "
           "\"loop_waves_sum\": %d, \"forest_waves\": %d, \"stages_equal\": %s}\n", n, 6 * n, forest0.trees.size(), treesWithParents, (double)width,
           secs[0][0], secs[1][0], secs[0][1], secs[1][1], accepted[0], accepted[1], border[0], border[1], waves[0], waves[1], same ? "true" : "false");
    return 0;
}
