// Scene::levelConflicts (the C++ host layer's face of hpmvs_level_conflicts_batch) on a dumped state, for
// tests/test_gpu_cpp_level_conflicts.py, which runs hpmvs_amd.api.level_conflicts on the same patches and compares the bytes.
// Built by that test with g++ against libhpmvs_host.so.
//   level_conflicts_cpp <dump> <out>
// Dump: the scene and patches of tests/test_gpu_cpp_interface.py (_dump_scene), then uint8 isEvent[n].
// Out (binary), twice -- all candidates (isEvent == nullptr), then with the events: int32 nFlow, uint32 flowOff[n + 1],
// uint32 flowAdj[nFlow], int32 nAnti, uint32 antiOff[n + 1], uint32 antiAdj[nAnti]; then the empty graph of n == 0 the same way.
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
    std::vector<uint8_t> isEvent(n);
    for (uint8_t& e : isEvent) e = rd<uint8_t>(f);
    fclose(f);

    std::vector<const mo3d::Patch3d*> pp(n);
    for (int i = 0; i < n; i++) pp[i] = &base[i];
    if (!scene.resetDepths() || !scene.setDepths(pp.data(), pp.size())) { fprintf(stderr, "depth setup failed\n"); return 1; }
    FILE* g = fopen(argv[2], "wb");
    if (!g) return 2;
    auto graph = [&](size_t count, const uint8_t* ev) {
        mo3d::Scene::LevelGraph G;
        if (!scene.levelConflicts(pp.data(), count, ev, G)) { fprintf(stderr, "levelConflicts failed\n"); return false; }
        if (G.flowOff.size() != count + 1 || G.antiOff.size() != count + 1 || G.flowOff[count] != G.flowAdj.size() || G.antiOff[count] != G.antiAdj.size()) {
            fprintf(stderr, "levelConflicts: offsets and lists disagree\n");
            return false;
        }
        wr(g, (int32_t)G.flowAdj.size()); wrv(g, G.flowOff); wrv(g, G.flowAdj);
        wr(g, (int32_t)G.antiAdj.size()); wrv(g, G.antiOff); wrv(g, G.antiAdj);
        return true;
    };
    if (!graph((size_t)n, nullptr) || !graph((size_t)n, isEvent.data()) || !graph(0, nullptr)) return 1;
    fclose(g);
    return 0;
}
