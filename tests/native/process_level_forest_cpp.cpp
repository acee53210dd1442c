// PatchOptimizer::processLevelForest and OctreeIndex::applySweep (the C++ host layer) on a dumped state, for
// tests/test_gpu_cpp_process_level_forest.py, which runs hpmvs_amd.frontier.process_level_forest on the same state and compares
// the bytes.  Built by that test with g++ against libhpmvs_host.so.
//   process_level_forest_cpp <dump> <out>
// Dump: the scene and the cells' patches as tests/test_gpu_cpp_interface.py writes them (_dump_scene), then per cell float
// flatness, int32 tree, uint64 key, uint8 final; then int32 nAll and the patches whose depths the maps start with (centre, normal,
// scale, list); then int32 nTrees and per tree float root[4], int32 nBranches, int32 nLeaves, uint64 branchKeys[], uint64
// leafKeys[], float patchCenter[3 nLeaves].
// Out (binary): float flatness[n], int32 priorityReduction[n], int32 images_.size()[n], int32 nNeighbours[n], int32 support[n],
// uint8 removed[n], split[n], child[4 n], uint64 childKey[4 n], the candidates' centre and normal (8 floats each, 4 n of them);
// per tree after applySweep int32 nBranches, nLeaves, uint64 branchKeys[], leafKeys[], float patchCenter[3 nLeaves] carried over
// through leafFrom; then depthGates(margin 1) of every cell: int32 visible[n], blocking[n], free[n].
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <hpmvs/HpmvsOptions.h>
#include <hpmvs/PatchOptimizer.h>
#include <hpmvs/Scene.h>

template <typename T> static T rd(FILE* f) { T v; if (fread(&v, sizeof(T), 1, f) != 1) { perror("read"); exit(2); } return v; }
template <typename T> static std::vector<T> rdv(FILE* f, size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, f) != n) { perror("read"); exit(2); } return v; }
template <typename T> static void wr(FILE* f, const T& v) { if (fwrite(&v, sizeof(T), 1, f) != 1) { perror("write"); exit(2); } }
template <typename T> static void wrv(FILE* f, const std::vector<T>& v) { if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { perror("write"); exit(2); } }

static void read_patches(FILE* f, std::vector<mo3d::Patch3d>& out) {
    const int n = rd<int>(f);
    out.resize(n);
    for (int i = 0; i < n; i++) {
        mo3d::Patch3d& p = out[i];
        for (int k = 0; k < 4; k++) p.center_[k] = rd<float>(f);
        for (int k = 0; k < 4; k++) p.normal_[k] = rd<float>(f);
        p.scale_3dx_ = rd<float>(f);
        const int m = rd<int>(f);
        for (int k = 0; k < m; k++) p.images_.push_back(rd<int>(f));
        p.expanded_ = true;
    }
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
    std::vector<mo3d::Patch3d> cells, all;
    read_patches(f, cells);
    const size_t n = cells.size();
    std::vector<int32_t> tree(n);
    std::vector<uint64_t> key(n);
    std::vector<uint8_t> fin(n);
    for (size_t i = 0; i < n; i++) { cells[i].flatness_ = rd<float>(f); tree[i] = rd<int32_t>(f); key[i] = rd<uint64_t>(f); fin[i] = rd<uint8_t>(f); cells[i].priorityReduction_ = 5; }
    read_patches(f, all);
    mo3d::OctreeForest forest;
    std::vector<std::vector<float> > centre;
    const int nt = rd<int32_t>(f);
    for (int t = 0; t < nt; t++) {
        mo3d::OctreeIndex ix;
        for (int k = 0; k < 3; k++) ix.rootCenter[k] = rd<float>(f);
        ix.rootWidth = rd<float>(f);
        const int nb = rd<int32_t>(f), nl = rd<int32_t>(f);
        ix.branchKeys = rdv<uint64_t>(f, nb);
        ix.leafKeys = rdv<uint64_t>(f, nl);
        centre.push_back(rdv<float>(f, 3 * (size_t)nl));
        forest.trees.push_back(ix);
    }
    fclose(f);
    std::vector<float> patchCenter;
    for (const std::vector<float>& c : centre) patchCenter.insert(patchCenter.end(), c.begin(), c.end());

    const std::vector<mo3d::Patch3d> dumped(cells);
    mo3d::PatchOptimizer opt(options, &scene);
    FILE* g = fopen(argv[2], "wb");
    if (!g) return 2;
    std::vector<mo3d::Patch3d*> cp(n);
    for (size_t i = 0; i < n; i++) cp[i] = &cells[i];
    std::vector<const mo3d::Patch3d*> ap(all.size());
    for (size_t i = 0; i < all.size(); i++) ap[i] = &all[i];
    if (!scene.resetDepths() || !scene.setDepths(ap.data(), ap.size())) { fprintf(stderr, "depth setup failed\n"); return 1; }
    // a decreasing cellTree is refused before anything happens
    if (n >= 2 && tree[0] != tree[n - 1]) {
        std::vector<int32_t> bad(tree);
        std::swap(bad[0], bad[n - 1]);
        mo3d::PatchOptimizer::ForestProcessResult X;
        if (opt.processLevelForest(cp.data(), bad.data(), key.data(), n, fin.data(), forest, patchCenter, X)) { fprintf(stderr, "a decreasing cellTree passed\n"); return 1; }
    }
    mo3d::PatchOptimizer::ForestProcessResult R;
    if (!opt.processLevelForest(cp.data(), tree.data(), key.data(), n, fin.data(), forest, patchCenter, R)) { fprintf(stderr, "processLevelForest failed\n"); return 1; }
    std::vector<float> fl(n);
    std::vector<int32_t> pr(n), ni(n);
    for (size_t i = 0; i < n; i++) { fl[i] = cells[i].flatness_; pr[i] = cells[i].priorityReduction_; ni[i] = (int32_t)cells[i].images_.size(); }
    wrv(g, fl); wrv(g, pr); wrv(g, ni);
    wrv(g, std::vector<int32_t>(R.nNeighbours.begin(), R.nNeighbours.end()));
    wrv(g, std::vector<int32_t>(R.support.begin(), R.support.end()));
    wrv(g, R.removed); wrv(g, R.split); wrv(g, R.child); wrv(g, R.childKey);
    for (const mo3d::Patch3d& q : R.candidates) {
        for (int k = 0; k < 4; k++) wr(g, (float)q.center_[k]);
        for (int k = 0; k < 4; k++) wr(g, (float)q.normal_[k]);
    }
    size_t first = 0;
    for (int t = 0; t < nt; t++) {   // every tree's share of the sweep: its cells are one run of the queue
        size_t last = first;
        while (last < n && tree[last] == t) last++;
        std::vector<int32_t> from;
        if (!forest.trees[t].applySweep(key.data() + first, R.removed.data() + first, R.split.data() + first, R.child.data() + 4 * first,
                                        R.childKey.data() + 4 * first, last - first, &from)) { fprintf(stderr, "applySweep failed on tree %d\n", t); return 1; }
        std::vector<float> pc;
        for (int32_t src : from)
            for (int d = 0; d < 3; d++)
                pc.push_back(src >= 0 ? centre[t][3 * (size_t)src + d] : (float)R.candidates[4 * first + (size_t)(-src - 1)].center_[d]);
        wr(g, (int32_t)forest.trees[t].branchKeys.size()); wr(g, (int32_t)forest.trees[t].leafKeys.size());
        wrv(g, forest.trees[t].branchKeys); wrv(g, forest.trees[t].leafKeys); wrv(g, pc);
        first = last;
    }
    std::vector<const mo3d::Patch3d*> gp(n);   // (the cells as dumped: the sweep cleared some lists)
    for (size_t i = 0; i < n; i++) gp[i] = &dumped[i];
    std::vector<int> v, b, fr;
    if (!scene.depthGates(gp.data(), gp.size(), 1.0f, v, b, fr, false)) { fprintf(stderr, "depthGates failed\n"); return 1; }
    wrv(g, std::vector<int32_t>(v.begin(), v.end())); wrv(g, std::vector<int32_t>(b.begin(), b.end())); wrv(g, std::vector<int32_t>(fr.begin(), fr.end()));
    fclose(g);
    return 0;
}
