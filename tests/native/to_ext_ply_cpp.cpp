// Scene::toExtPly against mo3d::writeExtPly, the unchanged host loop: 300 patches made here (coordinates of every size, the
// values whose text sits on a rounding or notation boundary, colours with fractions, lists of 0 .. 300 ids with -1 among them)
// written by both, with the reference's default arguments into <folder>/{gpu,host}_default.ply and with main's "light" set
// (binary, no normal, no scale, no visibility; src/main.cpp:164-168) into <folder>/{gpu,host}_light.ply.  The Python test
// compares the files; the refusal of a path that cannot be written is checked here.
//   to_ext_ply_cpp <folder>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include <hpmvs/Patch3d.h>
#include <hpmvs/PlyWriter.h>
#include <hpmvs/Scene.h>

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string folder(argv[1]);
    const float special[] = {1234565.f, 1234575.f, 1024.125f, 1024.375f, 999999.5f, 999999.4f, 9.9999995f, 0.0001f, 1e-5f, -0.0f, 0.0f,
                             1e-45f, -1.17549435e-38f, 3.4028235e38f, -0.000123457f, 100000.f, 0.5f, -1.f};
    const int n_special = (int)(sizeof(special) / sizeof(special[0]));
    uint64_t state = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(state >> 33); };
    auto value = [&]() -> float {
        const uint32_t r = next();
        if (r % 4 == 0) return special[next() % n_special];
        float scale = 1.0f;
        for (uint32_t k = next() % 12; k > 0; k--) scale *= (r & 8) ? 10.0f : 0.1f;
        return ((float)(next() % 2000001) / 1000000.0f - 1.0f) * scale;
    };
    std::vector<mo3d::Ppatch3d> patches;
    for (int i = 0; i < 300; i++) {
        mo3d::Ppatch3d p(new mo3d::Patch3d);
        for (int k = 0; k < 3; k++) { p->center_[k] = value(); p->normal_[k] = value(); }
        p->center_[3] = 1.0f; p->normal_[3] = 0.0f;
        p->scale_3dx_ = value();
        for (int k = 0; k < 3; k++) p->color_[k] = (float)(next() % 25600) / 100.0f;   // [0, 256): where both conversions are defined
        const int n_ids = i == 7 ? 300 : (int)(next() % 5 == 0 ? 0 : next() % 12);
        for (int k = 0; k < n_ids; k++) p->images_.push_back(next() % 9 == 0 ? -1 : (int)(next() % 1000));
        patches.push_back(p);
    }
    mo3d::Scene scene;
    const std::string gd = folder + "/gpu_default.ply", hd = folder + "/host_default.ply", gl = folder + "/gpu_light.ply", hl = folder + "/host_light.ply";
    if (!scene.toExtPly(gd.c_str(), patches)) { fprintf(stderr, "toExtPly (defaults) failed\n"); return 3; }
    if (!mo3d::writeExtPly(hd.c_str(), patches, false, true, true, true)) { fprintf(stderr, "writeExtPly failed\n"); return 4; }
    if (!scene.toExtPly(gl.c_str(), patches, true, false, false, false)) { fprintf(stderr, "toExtPly (light) failed\n"); return 5; }
    if (!mo3d::writeExtPly(hl.c_str(), patches, true, false, false, false)) { fprintf(stderr, "writeExtPly failed\n"); return 6; }
    // a path below a regular file cannot be written
    const std::string below = gd + "/below_a_file.ply";
    if (scene.toExtPly(below.c_str(), patches)) { fprintf(stderr, "toExtPly wrote below a regular file\n"); return 7; }
    // no patches: the header alone
    const std::string ge = folder + "/gpu_empty.ply", he = folder + "/host_empty.ply";
    if (!scene.toExtPly(ge.c_str(), std::vector<mo3d::Ppatch3d>()) || !mo3d::writeExtPly(he.c_str(), std::vector<mo3d::Ppatch3d>(), false)) return 8;
    printf("patches %zu\n", patches.size());
    return 0;
}
