// Scene::octreePartition (the C++ host layer) on a dumped state, for tests/test_gpu_cpp_octree_partition.py, which runs
// hpmvs_amd.api.octree_partition on the same state and compares the bytes.  Built by that test with g++ against libhpmvs_host.so.
//   octree_partition_cpp <dump> <out>
// Dump: the scene and patches of tests/test_gpu_cpp_interface.py (_dump_scene), then float root[4] (c_, width_), int32 nb,
// uint64 branch keys[nb], int32 nl, uint64 leaf keys[nl], int32 minTrees, int32 minSplitLeaves.
// Out (binary): int32 nTrees, nOrphans, nSplits, stop, histogram[22]; uint64 rootKey[nTrees], float rootCell[nTrees][4], int32
// treeFirst[nTrees], treeLeaves[nTrees], leafOrder[nl], leafTree[nl], uint64 leafSubKey[nl], int32 branchTree[nb], uint64
// branchSubKey[nb].  Exit status 3 when octreePartition refuses.
#include <cstdint>
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
    mo3d::OctreeIndex tree;
    for (int k = 0; k < 3; k++) tree.rootCenter[k] = rd<float>(f);
    tree.rootWidth = rd<float>(f);
    tree.branchKeys = rdv<uint64_t>(f, (size_t)rd<int32_t>(f));
    tree.leafKeys = rdv<uint64_t>(f, (size_t)rd<int32_t>(f));
    const int minTrees = rd<int32_t>(f);
    const int minSplitLeaves = rd<int32_t>(f);
    fclose(f);

    mo3d::OctreePartition r;
    if (!scene.octreePartition(tree, minTrees, r, minSplitLeaves)) return 3;
    FILE* g = fopen(argv[2], "wb");
    if (!g) return 2;
    wr<int32_t>(g, r.nTrees); wr<int32_t>(g, r.nOrphans); wr<int32_t>(g, r.nSplits); wr<int32_t>(g, r.stop);
    wrv(g, r.histogram); wrv(g, r.rootKey); wrv(g, r.rootCell); wrv(g, r.treeFirst); wrv(g, r.treeLeaves); wrv(g, r.leafOrder);
    wrv(g, r.leafTree); wrv(g, r.leafSubKey); wrv(g, r.branchTree); wrv(g, r.branchSubKey);
    fclose(g);
    return 0;
}
