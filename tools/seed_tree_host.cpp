// The second half of Scene::initPatches (reference src/hpmvs/Scene.cpp:183-199) as the reference runs it, for the timing leg of
// tools/seed_tree_scale.py: one thread, a pointer octree, DynOctTree::add(e, width) element by element (descend, split while
// leaf width / 2.0 > width, redistribute, append), then the flattening a caller of the level calls needs (nonempty leaves in
// Leaf_iterator order with their data).  Built by the tool: g++ -O2 -std=c++14 -ffp-contract=off -shared -fPIC.
#include <cfloat>
#include <chrono>
#include <cstdint>
#include <vector>

namespace {
struct Node {
    float c[3];
    float w;
    int level;
    Node* ch[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // a Branch has all eight
    std::vector<int32_t> data;
    bool branch() const { return ch[0] != nullptr; }
};
int octant(const float* c, const float* p) { return ((p[2] > c[2]) << 2) | ((p[1] > c[1]) << 1) | (p[0] > c[0]); }
void make_branch(Node* b, std::vector<Node*>& pool) {
    const float cw = (float)((double)b->w / 2.0);
    for (int i = 0; i < 8; i++) {
        Node* n = new Node();
        pool.push_back(n);
        n->w = cw;
        n->level = b->level + 1;
        for (int k = 0; k < 3; k++) n->c[k] = (float)((double)b->c[k] + ((i >> k) & 1 ? 1.0 : -1.0) * (double)cw / 2.0);
        b->ch[i] = n;
    }
}
Node* at(Node* b, const float* p) {
    while (true) {
        Node* n = b->ch[octant(b->c, p)];
        if (!n->branch()) return n;
        b = n;
    }
}
struct Flat {
    int32_t *rows, *cell_start, *cell_level;
    float *cell_center, *cell_width;
    int n_rows = 0, n_leaves = 0;
};
void flatten(const Node* n, Flat& f) {
    if (n->branch()) {
        for (int i = 0; i < 8; i++) flatten(n->ch[i], f);
        return;
    }
    if (n->data.empty()) return;
    f.cell_start[f.n_leaves] = f.n_rows;
    for (int k = 0; k < 3; k++) f.cell_center[3 * f.n_leaves + k] = n->c[k];
    f.cell_width[f.n_leaves] = n->w;
    f.cell_level[f.n_leaves] = n->level;
    for (int32_t e : n->data) f.rows[f.n_rows++] = e;
    f.n_leaves++;
}
}  // namespace

// center [n][4], scale [n] in/out; root [5] out: centre, width, floor; counts [2] out: rows, leaves.  Returns the seconds of
// bounding box + insertion + flattening (freeing the tree is not timed).
extern "C" double seed_tree_host(int n, const float* center, float* scale, int patch_init_maxlevel, float* root, int32_t* counts,
                                 int32_t* rows, int32_t* cell_start, float* cell_center, float* cell_width, int32_t* cell_level) {
    const auto t0 = std::chrono::steady_clock::now();
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {FLT_MIN, FLT_MIN, FLT_MIN};
    if (n == 0)
        for (int k = 0; k < 3; k++) { mn[k] = -1.0f; mx[k] = 1.0f; }
    for (int i = 0; i < n; i++)
        for (int k = 0; k < 3; k++) {
            const float x = center[4 * (size_t)i + k];
            mn[k] = x < mn[k] ? x : mn[k];
            mx[k] = mx[k] < x ? x : mx[k];
        }
    std::vector<Node*> pool;
    Node* r = new Node();
    pool.push_back(r);
    float dist[3];
    for (int k = 0; k < 3; k++) { dist[k] = mx[k] - mn[k]; r->c[k] = (mn[k] + mx[k]) / 2.0f; }
    const float inner = dist[1] < dist[2] ? dist[2] : dist[1];
    r->w = dist[0] < inner ? inner : dist[0];
    r->level = 0;
    make_branch(r, pool);
    const float floor = r->w / (float)(1 << (patch_init_maxlevel + 1));
    std::vector<int32_t> buf;
    for (int i = 0; i < n; i++) {
        const float* p = center + 4 * (size_t)i;
        scale[i] = scale[i] < floor ? floor : scale[i];
        Node* leaf = at(r, p);
        while ((double)leaf->w / 2.0 > (double)scale[i]) {
            buf.clear();
            buf.swap(leaf->data);
            make_branch(leaf, pool);
            for (int32_t e : buf) at(leaf, center + 4 * (size_t)e)->data.push_back(e);
            leaf = at(leaf, p);
        }
        leaf->data.push_back(i);
    }
    Flat f;
    f.rows = rows; f.cell_start = cell_start; f.cell_level = cell_level; f.cell_center = cell_center; f.cell_width = cell_width;
    flatten(r, f);
    cell_start[f.n_leaves] = f.n_rows;
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (int k = 0; k < 3; k++) root[k] = r->c[k];
    root[3] = r->w; root[4] = floor;
    counts[0] = f.n_rows; counts[1] = f.n_leaves;
    for (Node* p : pool) delete p;
    return s;
}
