// Host restatement of CellProcessor::regularize (reference src/hpmvs/CellProcessor.cpp:309-367) for the timing leg of
// tools/branch_level_scale.py: a pointer octree built from a leaf table (Cell(parent, idx) / Branch::at recurrences), then per cell the
// 24 probes, a std::set<const Node*> of the nonempty leaves found and the RMS sum in set order, as the reference runs it; OpenMP over
// the cells.  Built by the tool: g++ -O2 -std=c++14 -fopenmp -ffp-contract=off -shared -fPIC.
#include <omp.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <set>
#include <vector>

namespace {
struct Node {
    float c[3];
    float w;
    Node* ch[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int patch = -1;   // leaf: index of data[0] (-1: empty)
    bool branch = false;
};
int octant(const float* c, const float* p) { return ((p[2] > c[2]) << 2) | ((p[1] > c[1]) << 1) | (p[0] > c[0]); }
void make_branch(Node* b, std::vector<Node*>& pool) {
    b->branch = true;
    const float cw = (float)(b->w / 2.0);
    for (int i = 0; i < 8; i++) {
        Node* n = new Node();
        pool.push_back(n);
        n->w = cw;
        for (int k = 0; k < 3; k++) n->c[k] = (float)(b->c[k] + ((i >> k) & 1 ? 1.0 : -1.0) * cw / 2.0);
        b->ch[i] = n;
    }
}
const Node* at(const Node* b, const float* p) {
    while (true) {
        const Node* n = b->ch[octant(b->c, p)];
        if (!n->branch) return n;
        b = n;
    }
}
float dot(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
void cross(const float* a, const float* b, float* r) {
    const float r0 = a[1] * b[2] - a[2] * b[1], r1 = a[2] * b[0] - a[0] * b[2], r2 = a[0] * b[1] - a[1] * b[0];
    r[0] = r0; r[1] = r1; r[2] = r2;
}
void normalized(const float* a, float* r) {
    const float n2 = dot(a, a);
    if (n2 > 0.0f) { const float n = std::sqrt(n2); for (int k = 0; k < 3; k++) r[k] = a[k] / n; }
    else for (int k = 0; k < 3; k++) r[k] = a[k];
}
}  // namespace

// flatness[n], n_neighbours[n] out; returns the seconds of the cell loop (the tree build is not timed)
extern "C" double regularize_host(const float* root, int L, const float* leaf_c, const float* leaf_w, const float* leaf_p, int n,
                                  const float* center, const float* normal, const float* xaxis, const float* width, int threads,
                                  float* flatness, int32_t* n_neighbours) {
    std::vector<Node*> pool;
    Node* r = new Node();
    pool.push_back(r);
    for (int k = 0; k < 3; k++) r->c[k] = root[k];
    r->w = root[3];
    make_branch(r, pool);
    for (int j = 0; j < L; j++) {   // descend to the leaf's centre, splitting leaves on the way, until the width matches
        Node* b = r;
        Node* n = b->ch[octant(b->c, leaf_c + 3 * j)];
        while (n->w != leaf_w[j]) {
            if (!n->branch) make_branch(n, pool);
            b = n;
            n = b->ch[octant(b->c, leaf_c + 3 * j)];
        }
        n->patch = j;
    }
    const auto t0 = std::chrono::steady_clock::now();
#pragma omp parallel for num_threads(threads) schedule(dynamic, 256)
    for (int i = 0; i < n; i++) {
        const float* pn = normal + 4 * i;
        const float* x0 = center + 4 * i;
        float t[3], ya[3], xa[3];
        cross(pn, xaxis + 3 * i, t);
        normalized(t, ya);
        cross(ya, pn, xa);
        std::set<const Node*> found;
        for (int yy = -2; yy <= 2; yy++)
            for (int xx = -2; xx <= 2; xx++) {
                if (xx == 0 && yy == 0) continue;
                float p[3];
                for (int k = 0; k < 3; k++) p[k] = x0[k] + ((float)xx * xa[k] + (float)yy * ya[k]) * width[i];
                const Node* l = at(r, p);
                if (l->patch >= 0) found.insert(l);
            }
        const int k = (int)found.size();
        n_neighbours[i] = k;
        if (k < 1) { flatness[i] = 2.6f; continue; }
        if (k < 4) { flatness[i] = 2.5f; continue; }
        float nn[3];
        normalized(pn, nn);
        float dist = 0.0f;
        for (const Node* l : found) {
            const float* pb = leaf_p + 3 * l->patch;
            const float d[3] = {pb[0] - x0[0], pb[1] - x0[1], pb[2] - x0[2]};
            const float e = dot(nn, d);
            dist += e * e;
        }
        flatness[i] = std::sqrt(dist / k) / width[i];
    }
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (Node* p : pool) delete p;
    return s;
}
