// PatchOptimizer::extendLevelForest / filterExtendLevelForest (the C++ host layer's levels over all subtrees of a partition) on a
// dumped state, for tests/test_gpu_cpp_extend_level_forest.py, which runs hpmvs_amd.frontier's extend_level_forest /
// filter_extend_level_forest on the same state and compares the bytes.  Built by that test with g++ against libhpmvs_host.so.
//   extend_level_forest_cpp <dump> <out>
// Dump: the scene and patches of tests/test_gpu_cpp_interface.py (_dump_scene), then int32 nTrees and per tree float root[4] (c_,
// width_), int32 nb, uint64 branchKeys[nb], int32 nl, uint64 leafKeys[nl]; then two levels, each float width, int32 np,
// int32 parent[np] (patch rows: the first patch of every leaf), int32 parentTree[np] (non-decreasing), then the leaves with all
// their patches: int32 cellStart[np + 1], int32 row[cellStart[np]]; then int32 one: a tree with parents on the first level.
// Out (binary), each part from resetDepths + setDepths(every patch) and the trees as dumped:
//   (1) extendLevelTree on tree `one` alone over its parents of the first level: the LEVEL record, the TREE;
//   (2) extendLevelForest over the first level, then filterExtendLevelForest over the second, the forest carried on: the LEVEL
//       record; int32 keep[np], float dist[rows], uint8 removed[rows], the LEVEL record, int32 losers whose images_ are empty; then
//       every TREE and the maps;
//   (3) part (1) again: the forest levels leave the one-tree level as it was.
// LEVEL: int32 stage[6 np], int32 counts[18 np], int32 A, int32 accepted[A], uint64 leafKey[A], int32 B, int32 border[B],
//        int32 waves, float center[6 np][4], float normal[6 np][4], int32 T, int32 tree[T] (T = 6 np for a forest level, else 0).
// TREE:  int32 nb, uint64 branchKeys[nb] sorted, int32 nl, uint64 leafKeys[nl] sorted.
// The maps: per view, per pyramid level, int32 rows, int32 cols, float depth[rows * cols] (hpmvs_scene_depth_get_level's order).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <hpmvs/HpmvsOptions.h>
#include <hpmvs/PatchOptimizer.h>
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
    struct Level { float width; std::vector<int32_t> parent, parentTree, row; std::vector<size_t> cellStart; };
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
    Level level[2];
    for (Level& l : level) {
        l.width = rd<float>(f);
        l.parent.resize(rd<int32_t>(f));
        for (int32_t& p : l.parent) p = rd<int32_t>(f);
        l.parentTree.resize(l.parent.size());
        for (int32_t& p : l.parentTree) p = rd<int32_t>(f);
        l.cellStart.resize(l.parent.size() + 1);
        for (size_t& c : l.cellStart) c = (size_t)rd<int32_t>(f);
        l.row.resize(l.cellStart.back());
        for (int32_t& p : l.row) p = rd<int32_t>(f);
    }
    const int32_t one = rd<int32_t>(f);
    fclose(f);

    mo3d::PatchOptimizer opt(options, &scene);
    FILE* g = fopen(argv[2], "wb");
    if (!g) return 2;
    auto fresh = [&](std::vector<mo3d::Patch3d>& cells) {
        cells = base;
        std::vector<const mo3d::Patch3d*> ccp(n);
        for (int i = 0; i < n; i++) ccp[i] = &cells[i];
        return scene.resetDepths() && scene.setDepths(ccp.data(), ccp.size());
    };
    auto write_level = [&](const mo3d::PatchOptimizer::LevelResult& L) {
        wrv(g, std::vector<int32_t>(L.stage.begin(), L.stage.end())); wrv(g, std::vector<int32_t>(L.counts.begin(), L.counts.end()));
        wr(g, (int32_t)L.accepted.size());
        for (size_t t : L.accepted) wr(g, (int32_t)t);
        wrv(g, L.leafKey);
        wr(g, (int32_t)L.border.size());
        for (size_t t : L.border) wr(g, (int32_t)t);
        wr(g, (int32_t)L.waves);
        for (const mo3d::Patch3d& p : L.candidates) for (int k = 0; k < 4; k++) wr(g, p.center_[k]);
        for (const mo3d::Patch3d& p : L.candidates) for (int k = 0; k < 4; k++) wr(g, p.normal_[k]);
        wr(g, (int32_t)L.tree.size()); wrv(g, L.tree);
    };
    auto write_tree = [&](const mo3d::OctreeIndex& t) {
        std::vector<uint64_t> b(t.branchKeys), l(t.leafKeys);
        std::sort(b.begin(), b.end()); std::sort(l.begin(), l.end());
        wr(g, (int32_t)b.size()); wrv(g, b); wr(g, (int32_t)l.size()); wrv(g, l);
    };
    auto one_tree = [&]() {   // extendLevelTree on tree `one` alone, first level
        std::vector<mo3d::Patch3d> cells;
        if (!fresh(cells)) { fprintf(stderr, "depth setup failed\n"); return false; }
        mo3d::OctreeIndex tree = forest0.trees[(size_t)one];
        std::vector<const mo3d::Patch3d*> parents;
        for (size_t i = 0; i < level[0].parent.size(); i++)
            if (level[0].parentTree[i] == one) parents.push_back(&cells[level[0].parent[i]]);
        mo3d::PatchOptimizer::LevelResult L;
        if (!opt.extendLevelTree(parents.data(), parents.size(), level[0].width, tree, 1.0f, false, L)) { fprintf(stderr, "extendLevelTree failed\n"); return false; }
        if (!L.tree.empty()) { fprintf(stderr, "extendLevelTree filled LevelResult::tree\n"); return false; }
        write_level(L);
        write_tree(tree);
        return true;
    };
    if (!one_tree()) return 1;
    {
        std::vector<mo3d::Patch3d> cells;
        if (!fresh(cells)) { fprintf(stderr, "depth setup failed\n"); return 1; }
        mo3d::OctreeForest forest = forest0;
        {
            const Level& l = level[0];
            std::vector<const mo3d::Patch3d*> parents;
            for (int32_t p : l.parent) parents.push_back(&cells[p]);
            mo3d::PatchOptimizer::LevelResult L;
            if (!opt.extendLevelForest(parents.data(), l.parentTree.data(), parents.size(), l.width, forest, 1.0f, false, L)) {
                fprintf(stderr, "extendLevelForest failed\n");
                return 1;
            }
            if (L.leafKey.size() != L.accepted.size() || L.tree.size() != L.stage.size()) { fprintf(stderr, "leafKey / tree have the wrong length\n"); return 1; }
            write_level(L);
        }
        {
            const Level& l = level[1];
            std::vector<mo3d::Patch3d*> cp;
            for (int32_t p : l.row) cp.push_back(&cells[p]);
            mo3d::PatchOptimizer::FilterResult R;
            mo3d::PatchOptimizer::LevelResult L;
            if (!opt.filterExtendLevelForest(cp.data(), l.cellStart.data(), l.parentTree.data(), l.cellStart.size() - 1, l.width, forest, 1.0f, false, R, L)) {
                fprintf(stderr, "filterExtendLevelForest failed\n");
                return 1;
            }
            wrv(g, std::vector<int32_t>(R.keep.begin(), R.keep.end())); wrv(g, R.dist); wrv(g, R.removed);
            write_level(L);
            int32_t clearedLosers = 0;
            for (size_t i = 0; i < cp.size(); i++) clearedLosers += R.removed[i] && cp[i]->images_.empty();
            wr(g, clearedLosers);
        }
        for (const mo3d::OctreeIndex& t : forest.trees) write_tree(t);
        if (!write_maps(g, scene)) { fprintf(stderr, "maps failed\n"); return 1; }
        // a queue that is not the trees' queues in list order is refused before anything changes
        std::vector<int32_t> backwards(level[0].parentTree.rbegin(), level[0].parentTree.rend());
        std::vector<const mo3d::Patch3d*> parents;
        for (int32_t p : level[0].parent) parents.push_back(&cells[p]);
        mo3d::PatchOptimizer::LevelResult L;
        if (backwards != level[0].parentTree && opt.extendLevelForest(parents.data(), backwards.data(), parents.size(), level[0].width, forest, 1.0f, false, L)) {
            fprintf(stderr, "extendLevelForest took a decreasing parentTree\n");
            return 1;
        }
    }
    if (!one_tree()) return 1;
    fclose(g);
    return 0;
}
