// PatchOptimizer::filterLevel / filterExtendLevel (the C++ host layer) on a dumped state, for tests/test_gpu_cpp_filter_level.py, which
// runs hpmvs_amd.frontier's filter_level / filter_extend_level on the same state and compares the bytes.  Built by that test with g++
// against libhpmvs_host.so.
//   filter_level_cpp <dump> <out>
// Dump: the scene and patches of tests/test_gpu_cpp_interface.py (_dump_scene; the patches are the cells' rows, cells contiguous),
// then int32 nCells, int32 cellStart[nCells + 1], float width, int32 absInt, int32 nOcc, uint64 occupied[nOcc].
// Out (binary), both after resetDepths + setDepths(every patch):
//   (A) filterLevel: int32 keep[nCells], float dist[n], uint8 removed[n], int32 losers whose images_ are empty, the maps;
//   (B) filterExtendLevel: int32 keep[nCells], float dist[n], uint8 removed[n], int32 stage[6 nCells], int32 counts[18 nCells],
//       int32 A, int32 accepted[A], int32 waves, int32 O, uint64 occupied[O] (sorted), float center[6 nCells][4],
//       float normal[6 nCells][4], int32 losers whose images_ are empty, the maps.
// The maps: per view, per pyramid level, int32 rows, int32 cols, float depth[rows * cols] (hpmvs_scene_depth_get_level's order).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <unordered_set>
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
    const int nCells = rd<int32_t>(f);
    std::vector<size_t> cs(nCells + 1);
    for (int c = 0; c <= nCells; c++) cs[c] = (size_t)rd<int32_t>(f);
    const float width = rd<float>(f);
    const int absInt = rd<int32_t>(f);
    const int nOcc = rd<int32_t>(f);
    std::unordered_set<uint64_t> occ0;
    for (int k = 0; k < nOcc; k++) occ0.insert(rd<uint64_t>(f));
    fclose(f);

    mo3d::PatchOptimizer opt(options, &scene);
    FILE* g = fopen(argv[2], "wb");
    if (!g) return 2;
    auto fresh = [&](std::vector<mo3d::Patch3d>& cells, std::vector<mo3d::Patch3d*>& cp) {
        cells = base;
        cp.resize(n);
        for (int i = 0; i < n; i++) cp[i] = &cells[i];
        std::vector<const mo3d::Patch3d*> ccp(cp.begin(), cp.end());
        return scene.resetDepths() && scene.setDepths(ccp.data(), ccp.size());
    };
    auto cleared = [&](const std::vector<mo3d::Patch3d>& cells, const std::vector<uint8_t>& removed) {
        int32_t c = 0;
        for (int i = 0; i < n; i++) c += removed[i] && cells[i].images_.empty();
        return c;
    };
    {   // (A) filterLevel
        std::vector<mo3d::Patch3d> cells;
        std::vector<mo3d::Patch3d*> cp;
        if (!fresh(cells, cp)) { fprintf(stderr, "depth setup failed\n"); return 1; }
        mo3d::PatchOptimizer::FilterResult R;
        if (!opt.filterLevel(cp.data(), cs.data(), nCells, R)) { fprintf(stderr, "filterLevel failed\n"); return 1; }
        wrv(g, std::vector<int32_t>(R.keep.begin(), R.keep.end())); wrv(g, R.dist); wrv(g, R.removed);
        wr(g, cleared(cells, R.removed));
        if (!write_maps(g, scene)) { fprintf(stderr, "maps failed\n"); return 1; }
    }
    {   // (B) filterExtendLevel
        std::vector<mo3d::Patch3d> cells;
        std::vector<mo3d::Patch3d*> cp;
        if (!fresh(cells, cp)) { fprintf(stderr, "depth setup failed\n"); return 1; }
        std::unordered_set<uint64_t> occ = occ0;
        mo3d::PatchOptimizer::FilterResult R;
        mo3d::PatchOptimizer::LevelResult L;
        if (!opt.filterExtendLevel(cp.data(), cs.data(), nCells, width, occ, 1.0f, absInt != 0, R, L)) { fprintf(stderr, "filterExtendLevel failed\n"); return 1; }
        wrv(g, std::vector<int32_t>(R.keep.begin(), R.keep.end())); wrv(g, R.dist); wrv(g, R.removed);
        wrv(g, std::vector<int32_t>(L.stage.begin(), L.stage.end())); wrv(g, std::vector<int32_t>(L.counts.begin(), L.counts.end()));
        wr(g, (int32_t)L.accepted.size());
        for (size_t t : L.accepted) wr(g, (int32_t)t);
        wr(g, (int32_t)L.waves);
        std::vector<uint64_t> ok(occ.begin(), occ.end());
        std::sort(ok.begin(), ok.end());
        wr(g, (int32_t)ok.size()); wrv(g, ok);
        for (const mo3d::Patch3d& p : L.candidates) for (int k = 0; k < 4; k++) wr(g, p.center_[k]);
        for (const mo3d::Patch3d& p : L.candidates) for (int k = 0; k < 4; k++) wr(g, p.normal_[k]);
        wr(g, cleared(cells, R.removed));
        if (!write_maps(g, scene)) { fprintf(stderr, "maps failed\n"); return 1; }
    }
    fclose(g);
    return 0;
}
