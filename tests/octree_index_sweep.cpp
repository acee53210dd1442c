// mo3d::OctreeIndex::applySweep (include/hpmvs/Scene.h, header only) as a stand-alone program, for
// tests/test_cpu_octree_index_sweep.py, which applies the same sweeps to hpmvs_amd.frontier.Octree and compares the sets.
// Build: g++ -std=c++14 -O2 -I include octree_index_sweep.cpp (no library)
//   octree_index_sweep <in> <out>
// In:  int32 nBranches, int32 nLeaves, uint64 branchKeys[], uint64 leafKeys[], int32 nSweeps, then per sweep int32 n,
//      uint64 cellKey[n], uint8 removed[n], uint8 split[n], uint8 child[4 n], uint64 childKey[4 n].
// Out: per sweep int32 ok, int32 nBranches, int32 nLeaves, uint64 branchKeys[], uint64 leafKeys[], int32 leafFrom[nLeaves].
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <hpmvs/Scene.h>

template <typename T> static T rd(FILE* f) { T v; if (fread(&v, sizeof(T), 1, f) != 1) { perror("read"); exit(2); } return v; }
template <typename T> static std::vector<T> rdv(FILE* f, size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, f) != n) { perror("read"); exit(2); } return v; }
template <typename T> static void wr(FILE* f, const T& v) { if (fwrite(&v, sizeof(T), 1, f) != 1) { perror("write"); exit(2); } }
template <typename T> static void wrv(FILE* f, const std::vector<T>& v) { if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { perror("write"); exit(2); } }

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    FILE* g = fopen(argv[2], "wb");
    if (!f || !g) return 2;
    mo3d::OctreeIndex t;
    t.rootCenter[0] = t.rootCenter[1] = t.rootCenter[2] = 0.0f;
    t.rootWidth = 8.0f;
    const int nb = rd<int32_t>(f), nl = rd<int32_t>(f);
    t.branchKeys = rdv<uint64_t>(f, nb);
    t.leafKeys = rdv<uint64_t>(f, nl);
    const int sweeps = rd<int32_t>(f);
    for (int s = 0; s < sweeps; s++) {
        const size_t n = (size_t)rd<int32_t>(f);
        const std::vector<uint64_t> key = rdv<uint64_t>(f, n);
        const std::vector<uint8_t> removed = rdv<uint8_t>(f, n), split = rdv<uint8_t>(f, n), child = rdv<uint8_t>(f, 4 * n);
        const std::vector<uint64_t> childKey = rdv<uint64_t>(f, 4 * n);
        std::vector<int32_t> from;
        const bool ok = t.applySweep(key.data(), removed.data(), split.data(), child.data(), childKey.data(), n, &from);
        if (!ok) from.assign(t.leafKeys.size(), 0);
        wr(g, (int32_t)ok); wr(g, (int32_t)t.branchKeys.size()); wr(g, (int32_t)t.leafKeys.size());
        wrv(g, t.branchKeys); wrv(g, t.leafKeys); wrv(g, from);
    }
    fclose(f);
    fclose(g);
    return 0;
}
