// The host side of tools/ply_ext_scale.py: mo3d::writeExtPly, the unchanged iostream loop, timed on patches read from a raw file
// (int32 n, m; then center [n][4], normal [n][4], scale [n], color [n][3] as float32; n_images [n], images [n][m] as int32).
//   bench_ply_ext_host <patches.raw> <out.ply> <binary 0|1> <reps>
// prints one line per repetition: "ms <wall clock of the call>".
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <hpmvs/Patch3d.h>
#include <hpmvs/PlyWriter.h>

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    FILE* f = fopen(argv[1], "rb");
    int32_t hd[2];
    if (!f || fread(hd, 4, 2, f) != 2) return 3;
    const size_t n = (size_t)hd[0], m = (size_t)hd[1];
    std::vector<float> center(4 * n), normal(4 * n), scale(n), color(3 * n);
    std::vector<int32_t> nimg(n), images(n * m);
    if (fread(center.data(), 4, 4 * n, f) != 4 * n || fread(normal.data(), 4, 4 * n, f) != 4 * n || fread(scale.data(), 4, n, f) != n ||
        fread(color.data(), 4, 3 * n, f) != 3 * n || fread(nimg.data(), 4, n, f) != n || fread(images.data(), 4, n * m, f) != n * m)
        return 3;
    fclose(f);
    std::vector<mo3d::Ppatch3d> patches;
    patches.reserve(n);
    for (size_t i = 0; i < n; i++) {
        mo3d::Ppatch3d p(new mo3d::Patch3d);
        for (int k = 0; k < 4; k++) { p->center_[k] = center[4 * i + k]; p->normal_[k] = normal[4 * i + k]; }
        for (int k = 0; k < 3; k++) p->color_[k] = color[3 * i + k];
        p->scale_3dx_ = scale[i];
        p->images_.assign(images.begin() + (long)(i * m), images.begin() + (long)(i * m) + nimg[i]);
        patches.push_back(p);
    }
    const bool binary = atoi(argv[3]) != 0;
    for (int r = 0; r < atoi(argv[4]); r++) {
        const auto t0 = std::chrono::steady_clock::now();
        if (!mo3d::writeExtPly(argv[2], patches, binary, true, true, true)) return 4;
        printf("ms %.3f\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    return 0;
}
