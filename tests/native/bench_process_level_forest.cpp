// One regularize / settle sweep over ALL subtrees of a partition at PRODUCTION size through the C++ host layer: the per-tree loop
// of PatchOptimizer::processLevel (level_support, expand, depth_ops and regularize calls per subtree, in list order) beside ONE
// PatchOptimizer::processLevelForest (one hpmvs_process_forest_batch) on the same cells, each from resetDepths + setDepths(cells),
// timed.  tools/process_forest_scale.py builds it, writes its input and reads the JSON line it prints.
//   bench_process_level_forest <dump>
// Dump: the format of tests/test_gpu_cpp_interface.py (_dump_scene) -- its patches are the cells, tree after tree --, then per
// cell float flatness, int32 tree (non-decreasing), uint64 key, uint8 final, int32 leaf (the index of its leaf among its tree's);
// then int32 nTrees and per tree float root[4] (c_, width_), int32 nb, uint64 branchKeys[nb], int32 nl, uint64 leafKeys[nl], float
// cellCenter[3 nl], float cellWidth[nl], float patchCenter[3 nl].  The two must decide the same things: flatness bits, removed and
// split are compared here, and the JSON says so.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <hpmvs/HpmvsOptions.h>
#include <hpmvs/PatchOptimizer.h>
#include <hpmvs/Scene.h>

template <typename T> static T rd(FILE* f) { T v; if (fread(&v, sizeof(T), 1, f) != 1) { perror("read"); exit(2); } return v; }
template <typename T> static std::vector<T> rdv(FILE* f, size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, f) != n) { perror("read"); exit(2); } return v; }
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
        p.expanded_ = true;
    }
    std::vector<int32_t> tree(n), leaf(n);
    std::vector<uint64_t> key(n);
    std::vector<uint8_t> fin(n);
    for (int i = 0; i < n; i++) { base[i].flatness_ = rd<float>(f); tree[i] = rd<int32_t>(f); key[i] = rd<uint64_t>(f); fin[i] = rd<uint8_t>(f); leaf[i] = rd<int32_t>(f); }
    mo3d::OctreeForest forest;
    forest.trees.resize(rd<int32_t>(f));
    std::vector<mo3d::PatchOptimizer::LeafTable> tables(forest.trees.size());
    std::vector<float> patchCenter;
    for (size_t t = 0; t < forest.trees.size(); t++) {
        mo3d::OctreeIndex& ix = forest.trees[t];
        for (int k = 0; k < 3; k++) ix.rootCenter[k] = rd<float>(f);
        ix.rootWidth = rd<float>(f);
        ix.branchKeys = rdv<uint64_t>(f, (size_t)rd<int32_t>(f));
        const size_t nl = (size_t)rd<int32_t>(f);
        ix.leafKeys = rdv<uint64_t>(f, nl);
        mo3d::PatchOptimizer::LeafTable& T = tables[t];
        T.rootCenter = Eigen::Vector3f(ix.rootCenter[0], ix.rootCenter[1], ix.rootCenter[2]);
        T.rootWidth = ix.rootWidth;
        T.center = rdv<float>(f, 3 * nl); T.width = rdv<float>(f, nl); T.patch = rdv<float>(f, 3 * nl);
        T.born.assign(nl, -1); T.died.assign(nl, INT32_MAX);
        patchCenter.insert(patchCenter.end(), T.patch.begin(), T.patch.end());
    }
    fclose(f);

    mo3d::PatchOptimizer opt(options, &scene);
    std::vector<mo3d::Patch3d> cells;
    std::vector<mo3d::Patch3d*> cp(n);
    std::vector<const mo3d::Patch3d*> ccp(n);
    auto fresh = [&]() {
        cells = base;
        for (int i = 0; i < n; i++) { cp[i] = &cells[i]; ccp[i] = &cells[i]; }
        return scene.resetDepths() && scene.setDepths(ccp.data(), ccp.size());
    };
    double secs[2][2];
    int treesWithCells = 0;
    size_t removed[2] = {0, 0}, split[2] = {0, 0};
    bool same = true;
    for (int rep = 0; rep < 2; rep++) {   // (the first pass of each warms the pinned-memory cache and the workspaces)
        std::vector<float> loopFlat(n);
        std::vector<uint8_t> loopRemoved(n, 0), loopSplit(n, 0);
        {
            if (!fresh()) { fprintf(stderr, "depth setup failed\n"); return 1; }
            treesWithCells = 0;
            const double t0 = now();
            for (int a = 0; a < n;) {
                int b = a;
                while (b < n && tree[b] == tree[a]) b++;
                mo3d::PatchOptimizer::ProcessResult R;
                if (!opt.processLevel(cp.data() + a, leaf.data() + a, (size_t)(b - a), fin.data() + a, tables[(size_t)tree[a]], R)) { fprintf(stderr, "processLevel failed\n"); return 1; }
                for (size_t j = 0; j < R.settled.size(); j++) { loopRemoved[a + R.settled[j]] = R.settle.removed[j]; loopSplit[a + R.settled[j]] = R.settle.split[j]; }
                treesWithCells++;
                a = b;
            }
            secs[rep][0] = now() - t0;
            for (int i = 0; i < n; i++) loopFlat[i] = cells[i].flatness_;
        }
        {
            if (!fresh()) { fprintf(stderr, "depth setup failed\n"); return 1; }
            mo3d::PatchOptimizer::ForestProcessResult R;
            const double t0 = now();
            if (!opt.processLevelForest(cp.data(), tree.data(), key.data(), (size_t)n, fin.data(), forest, patchCenter, R)) { fprintf(stderr, "processLevelForest failed\n"); return 1; }
            secs[rep][1] = now() - t0;
            removed[0] = removed[1] = split[0] = split[1] = 0;
            for (int i = 0; i < n; i++) {
                removed[0] += loopRemoved[i]; removed[1] += R.removed[i]; split[0] += loopSplit[i]; split[1] += R.split[i];
                same = same && loopRemoved[i] == R.removed[i] && loopSplit[i] == R.split[i] && !memcmp(&loopFlat[i], &cells[i].flatness_, 4);
            }
        }
    }
    printf("{\"cells\": %d, \"trees\": %zu, \"trees_with_cells\": %d, \"processLevel_loop_s\": [%.4f, %.4f], \"processLevelForest_s\": [%.4f, %.4f], "
           "\"loop_removed\": %zu, \"forest_removed\": %zu, \"loop_split\": %zu, \"forest_split\": %zu, \"decisions_equal\": %s}\n", n,
           forest.trees.size(), treesWithCells, secs[0][0], secs[1][0], secs[0][1], secs[1][1], removed[0], removed[1], split[0], split[1],
           same ? "true" : "false");
    return 0;
}
