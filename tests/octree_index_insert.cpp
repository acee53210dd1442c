// mo3d::OctreeIndex::insertLeaf / levelDepth (include/hpmvs/Scene.h, header only) as a stand-alone program, for
// tests/test_cpu_octree_index_insert.py, which runs hpmvs_amd.frontier.Octree.insert on the same keys and compares the sets.
// Build: g++ -std=c++14 -O2 -I include octree_index_insert.cpp (no library)
//   octree_index_insert <in> <out>
// In:  float rootWidth, int32 nKeys, uint64 key[nKeys], int32 nWidths, float width[nWidths].
// Out: after every hundredth insertion and after the last one a snapshot -- int32 step, int32 nBranches, int32 nLeaves,
//      uint64 branchKeys[], uint64 leafKeys[] in the vectors' order --, then int32 levelDepth(width[i]) for every width.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <hpmvs/Scene.h>

template <typename T> static T rd(FILE* f) { T v; if (fread(&v, sizeof(T), 1, f) != 1) { perror("read"); exit(2); } return v; }
template <typename T> static void wr(FILE* f, const T& v) { if (fwrite(&v, sizeof(T), 1, f) != 1) { perror("write"); exit(2); } }
template <typename T> static void wrv(FILE* f, const std::vector<T>& v) { if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { perror("write"); exit(2); } }

static void snapshot(FILE* g, int step, const mo3d::OctreeIndex& t) {
    wr(g, (int32_t)step); wr(g, (int32_t)t.branchKeys.size()); wr(g, (int32_t)t.leafKeys.size());
    wrv(g, t.branchKeys); wrv(g, t.leafKeys);
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    FILE* g = fopen(argv[2], "wb");
    if (!f || !g) return 2;
    mo3d::OctreeIndex t;
    t.rootCenter[0] = t.rootCenter[1] = t.rootCenter[2] = 0.0f;
    t.rootWidth = rd<float>(f);
    const int n = rd<int32_t>(f);
    for (int i = 0; i < n; i++) {
        t.insertLeaf(rd<uint64_t>(f));
        if (i % 100 == 99 || i == n - 1) snapshot(g, i, t);
    }
    const int nw = rd<int32_t>(f);
    for (int i = 0; i < nw; i++) wr(g, (int32_t)t.levelDepth(rd<float>(f)));
    fclose(f);
    fclose(g);
    return 0;
}
