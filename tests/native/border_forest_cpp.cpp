// Scene::octreeBorderForest and PatchOptimizer::deliverBorderForest (the C++ host layer) on a dumped state, for
// tests/test_gpu_cpp_border_forest.py, which runs hpmvs_amd.api.border_forest_batch on the same state and compares the bytes.  Built
// by that test with g++ against libhpmvs_host.so.
//   border_forest_cpp <dump> <out>
// Dump: the scene and patches of tests/test_gpu_cpp_interface.py (_dump_scene) -- the patches are the border queue --, then int32
// nt, float roots[nt][4], int32 branchFirst[nt + 1], int32 leafFirst[nt + 1], uint64 branch keys, uint64 leaf keys.
// Out (binary): from octreeBorderForest without setDepths int32 tree[n], uint8 accepted[n], uint64 leafKey[n], int32 blocker[n]; the
// same four from deliverBorderForest (after resetDepths, every patch's flatness_ set to -1 before); float flatness_[n] after it;
// then per tree int32 nb, uint64 branchKeys[nb], int32 nl, uint64 leafKeys[nl] of the forest as deliverBorderForest leaves it.
// Exit status 3 when octreeBorderForest refuses, 4 when deliverBorderForest does.
#include <cstdint>
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

template <typename T> static std::vector<T> rdv(FILE* f, size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, f) != n) { perror("read"); exit(2); } return v; }

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
    const size_t nt = (size_t)rd<int32_t>(f);
    const std::vector<float> roots = rdv<float>(f, 4 * nt);
    const std::vector<int32_t> bf = rdv<int32_t>(f, nt + 1), lf = rdv<int32_t>(f, nt + 1);
    const std::vector<uint64_t> bk = rdv<uint64_t>(f, (size_t)bf[nt]), lk = rdv<uint64_t>(f, (size_t)lf[nt]);
    fclose(f);
    mo3d::OctreeForest forest;
    forest.trees.resize(nt);
    for (size_t k = 0; k < nt; k++) {
        mo3d::OctreeIndex& t = forest.trees[k];
        for (int c = 0; c < 3; c++) t.rootCenter[c] = roots[4 * k + c];
        t.rootWidth = roots[4 * k + 3];
        t.branchKeys.assign(bk.begin() + bf[k], bk.begin() + bf[k + 1]);
        t.leafKeys.assign(lk.begin() + lf[k], lk.begin() + lf[k + 1]);
    }
    std::vector<mo3d::Patch3d*> queue((size_t)n);
    for (int i = 0; i < n; i++) { queue[i] = patches[i].get(); queue[i]->flatness_ = -1.0f; }

    mo3d::BorderForestInsertion a, b;
    if (!scene.octreeBorderForest(forest, queue.data(), queue.size(), false, a)) return 3;
    mo3d::PatchOptimizer opt(options, &scene);
    if (!scene.resetDepths() || !opt.deliverBorderForest(queue.data(), queue.size(), forest, b)) return 4;
    FILE* g = fopen(argv[2], "wb");
    if (!g) return 2;
    wrv(g, a.tree); wrv(g, a.accepted); wrv(g, a.leafKey); wrv(g, a.blocker);
    wrv(g, b.tree); wrv(g, b.accepted); wrv(g, b.leafKey); wrv(g, b.blocker);
    for (int i = 0; i < n; i++) wr(g, (float)queue[i]->flatness_);
    for (const mo3d::OctreeIndex& t : forest.trees) {
        wr(g, (int32_t)t.branchKeys.size()); wrv(g, t.branchKeys);
        wr(g, (int32_t)t.leafKeys.size()); wrv(g, t.leafKeys);
    }
    fclose(g);
    return 0;
}
