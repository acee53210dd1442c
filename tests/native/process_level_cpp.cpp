// PatchOptimizer::regularizeLevel / settleLevel / processLevel (the C++ host layer) on a dumped state, for
// tests/test_gpu_cpp_process_level.py, which runs hpmvs_amd.frontier's regularize_level / process_level on the same state and compares
// the bytes.  Built by that test with g++ against libhpmvs_host.so.
//   process_level_cpp <dump> <out>
// Dump: the scene and patches of tests/test_gpu_cpp_interface.py (_dump_scene), then per patch float flatness, int32 leaf, uint8 final,
// then float root[3], float rootWidth, int32 L, float center[3 L], float width[L], float patch[3 L].
// Out (binary): (A) regularizeLevel on every cell (flatness_ -1, position = index, the table as given): float flatness[n],
// int32 nNeighbours[n], int32 cells with priorityReduction_ == 0; (B) processLevel after resetDepths + setDepths(all cells):
// float flatness[n], int32 nNeighbours[n], int32 S, per settled cell int32 index, uint8 removed, uint8 split, int32 support,
// uint8 child[4], int32 childOctant[4], int32 childLeaf[4]; int32 L2, float center[3 L2], width[L2], patch[3 L2], int32 born[L2],
// died[L2]; then depthGates(margin 1) of every cell: int32 visible[n], blocking[n], free[n].
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <hpmvs/HpmvsOptions.h>
#include <hpmvs/PatchOptimizer.h>
#include <hpmvs/Scene.h>

template <typename T> static T rd(FILE* f) { T v; if (fread(&v, sizeof(T), 1, f) != 1) { perror("read"); exit(2); } return v; }
template <typename T> static void wr(FILE* f, const T& v) { if (fwrite(&v, sizeof(T), 1, f) != 1) { perror("write"); exit(2); } }
template <typename T> static void wrv(FILE* f, const std::vector<T>& v) { if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { perror("write"); exit(2); } }

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
    std::vector<mo3d::Patch3d> cells(n);
    for (int i = 0; i < n; i++) {
        mo3d::Patch3d& p = cells[i];
        for (int k = 0; k < 4; k++) p.center_[k] = rd<float>(f);
        for (int k = 0; k < 4; k++) p.normal_[k] = rd<float>(f);
        p.scale_3dx_ = rd<float>(f);
        const int m = rd<int>(f);
        for (int k = 0; k < m; k++) p.images_.push_back(rd<int>(f));
        p.expanded_ = true;
    }
    std::vector<float> flat(n);
    std::vector<int32_t> leaf(n);
    std::vector<uint8_t> fin(n);
    for (int i = 0; i < n; i++) { flat[i] = rd<float>(f); leaf[i] = rd<int32_t>(f); fin[i] = rd<uint8_t>(f); }
    mo3d::PatchOptimizer::LeafTable T;
    for (int k = 0; k < 3; k++) T.rootCenter[k] = rd<float>(f);
    T.rootWidth = rd<float>(f);
    const int L = rd<int32_t>(f);
    T.center.resize(3 * L); T.width.resize(L); T.patch.resize(3 * L);
    for (float& v : T.center) v = rd<float>(f);
    for (float& v : T.width) v = rd<float>(f);
    for (float& v : T.patch) v = rd<float>(f);
    T.born.assign(L, -1);
    T.died.assign(L, INT32_MAX);
    fclose(f);

    mo3d::PatchOptimizer opt(options, &scene);
    FILE* g = fopen(argv[2], "wb");
    if (!g) return 2;
    std::vector<mo3d::Patch3d*> cp(n);
    for (int i = 0; i < n; i++) cp[i] = &cells[i];
    {   // (A) regularizeLevel alone
        std::vector<float> cw(n);
        std::vector<int32_t> pos(n);
        for (int i = 0; i < n; i++) { cells[i].flatness_ = -1.0f; cells[i].priorityReduction_ = 5; cw[i] = T.width[leaf[i]]; pos[i] = i; }
        std::vector<int> nn;
        if (!opt.regularizeLevel(cp.data(), n, cw.data(), pos.data(), T, &nn)) { fprintf(stderr, "regularizeLevel failed\n"); return 1; }
        std::vector<float> fl(n);
        int32_t reset = 0;
        for (int i = 0; i < n; i++) { fl[i] = cells[i].flatness_; reset += cells[i].priorityReduction_ == 0; }
        wrv(g, fl);
        wrv(g, std::vector<int32_t>(nn.begin(), nn.end()));
        wr(g, reset);
    }
    {   // (B) processLevel on the maps the leaves' patches wrote
        std::vector<const mo3d::Patch3d*> ccp(cp.begin(), cp.end());
        if (!scene.resetDepths() || !scene.setDepths(ccp.data(), ccp.size())) { fprintf(stderr, "depth setup failed\n"); return 1; }
        for (int i = 0; i < n; i++) cells[i].flatness_ = flat[i];
        mo3d::PatchOptimizer::ProcessResult R;
        if (!opt.processLevel(cp.data(), leaf.data(), n, fin.data(), T, R)) { fprintf(stderr, "processLevel failed\n"); return 1; }
        std::vector<float> fl(n);
        for (int i = 0; i < n; i++) fl[i] = cells[i].flatness_;
        wrv(g, fl);
        wrv(g, std::vector<int32_t>(R.nNeighbours.begin(), R.nNeighbours.end()));
        wr(g, (int32_t)R.settled.size());
        for (size_t j = 0; j < R.settled.size(); j++) {
            wr(g, (int32_t)R.settled[j]);
            wr(g, R.settle.removed[j]); wr(g, R.settle.split[j]); wr(g, (int32_t)R.settle.support[j]);
            for (int k = 0; k < 4; k++) wr(g, R.settle.child[4 * j + k]);
            for (int k = 0; k < 4; k++) wr(g, (int32_t)R.settle.childOctant[4 * j + k]);
            for (int k = 0; k < 4; k++) wr(g, (int32_t)R.childLeaf[4 * j + k]);
        }
        wr(g, (int32_t)R.table.size());
        wrv(g, R.table.center); wrv(g, R.table.width); wrv(g, R.table.patch); wrv(g, R.table.born); wrv(g, R.table.died);
        std::vector<int> v, b, fr;
        if (!scene.depthGates(ccp.data(), ccp.size(), 1.0f, v, b, fr, false)) { fprintf(stderr, "depthGates failed\n"); return 1; }
        wrv(g, std::vector<int32_t>(v.begin(), v.end())); wrv(g, std::vector<int32_t>(b.begin(), b.end())); wrv(g, std::vector<int32_t>(fr.begin(), fr.end()));
    }
    fclose(g);
    return 0;
}
