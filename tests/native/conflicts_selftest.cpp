// Stand-alone check of hpmvs_amd/csrc/conflicts.hpp's conflicts_sequential, built with -fsanitize=address,undefined and run as a
// program (tests/test_cpu_conflicts.py): random footprints with blocks beyond the image corners, short rows, bad views and levels,
// events every third node, against a definition of its own -- every node's read and written cells as std::set, every pair of
// nodes tested by intersection.  Prints "<k> failures"; exit status 0 only for k == 0.
#include "../../hpmvs_amd/csrc/conflicts.hpp"

#include <cstdio>
#include <set>
#include <tuple>

namespace {
typedef std::tuple<int, int, int, int> Cell;

unsigned long long state = 0x9E3779B97F4A7C15ull;
int rnd(int m) { state = state * 6364136223846793005ull + 1442695040888963407ull; return (int)((state >> 33) % (unsigned long long)m); }

void block(std::set<Cell>& s, int V, int L, int view, int ix0, int iy0) {
    if (view < 0 || view >= V || ix0 < -2 || iy0 < -2 || ix0 >= (1 << 24) || iy0 >= (1 << 24)) return;
    const int x1 = ix0 + 2, y1 = iy0 + 2, x0 = ix0 < 0 ? 0 : ix0, y0 = iy0 < 0 ? 0 : iy0;
    for (int l = 0; l < L; l++)
        for (int x = x0 >> (1 + l); x <= x1 >> (1 + l); x++)
            for (int y = y0 >> (1 + l); y <= y1 >> (1 + l); y++) s.insert(Cell(view, l, x, y));
}
bool cell(int V, int L, const int32_t* e, Cell& c) {
    if (e[0] < 0 || e[0] >= V || e[1] < 0 || e[1] >= L || e[2] < 0 || e[2] >= (1 << 24) || e[3] < 0 || e[3] >= (1 << 24)) return false;
    c = Cell(e[0], e[1], e[2], e[3]);
    return true;
}
bool meets(const std::set<Cell>& a, const std::set<Cell>& b) {
    for (const Cell& c : a) if (b.count(c)) return true;
    return false;
}

int run(int n, int M, int V, int L, int event_every, int window) {
    std::vector<int32_t> ni(n), wr((size_t)n * M * 4, -1), fr((size_t)n * M * 4, -1), at((size_t)n * M * 3, -1), vb((size_t)n * V * 3, 0);
    std::vector<uint8_t> ev(n, 0);
    const int W = 640, H = 480;
    for (int i = 0; i < n; i++) {
        if (event_every) ev[i] = (i % event_every) == event_every - 1;
        const int m = rnd(10) == 0 ? rnd(M + 1) : 1 + rnd(M);
        ni[i] = rnd(20) == 0 ? m + 3 : m;   // (beyond M now and then: clamped)
        const int corner = rnd(4), bx = (corner & 1) ? W - window - 1 : -2, by = (corner & 2) ? H - window - 1 : -2;
        for (int k = 0; k < M; k++) {   // (all M entries are filled: those past n_images must not count)
            const int view = rnd(V + 1) - (rnd(16) == 0), px = bx + rnd(window + 3), py = by + rnd(window + 3);
            int32_t* a = &at[((size_t)i * M + k) * 3];
            if (rnd(8)) { a[0] = view; a[1] = px - 1 - rnd(3); a[2] = py - 1 - rnd(3); }
            const int l = rnd(L + 1), lf = rnd(L + 1);
            int32_t* w = &wr[((size_t)i * M + k) * 4];
            if (rnd(6)) { w[0] = view; w[1] = l; w[2] = ((px < 0 ? 0 : px) >> (1 + l)) + rnd(2); w[3] = ((py < 0 ? 0 : py) >> (1 + l)) + rnd(2); }
            int32_t* f = &fr[((size_t)i * M + k) * 4];
            if (rnd(6)) { f[0] = view; f[1] = lf; f[2] = ((px < 0 ? 0 : px) >> (1 + lf)) + rnd(2); f[3] = ((py < 0 ? 0 : py) >> (1 + lf)) + rnd(2); }
        }
        for (int v = 0; v < V; v++)
            if (rnd(3) == 0) { int32_t* b = &vb[((size_t)i * V + v) * 3]; b[0] = 1; b[1] = bx + rnd(window + 3) - 3; b[2] = by + rnd(window + 3) - 3; }
    }
    conflicts::Footprints F;
    F.n = n; F.M = M; F.V = V; F.n_levels = L;
    F.n_images = ni.data(); F.wr = wr.data(); F.fr = fr.data(); F.at = at.data(); F.vb = vb.data(); F.is_event = event_every ? ev.data() : nullptr;
    std::vector<uint32_t> fo, fa, ao, aa;
    if (!conflicts::conflicts_sequential(F, fo, fa, ao, aa)) return 1;
    std::vector<std::set<Cell> > R(n), Wc(n);
    for (int i = 0; i < n; i++) {
        const int m = ni[i] < 0 ? 0 : (ni[i] > M ? M : ni[i]);
        for (int k = 0; k < m; k++) {
            Cell c;
            if (cell(V, L, &wr[((size_t)i * M + k) * 4], c)) Wc[i].insert(c);
            if (ev[i]) continue;
            if (cell(V, L, &fr[((size_t)i * M + k) * 4], c)) R[i].insert(c);
            const int32_t* a = &at[((size_t)i * M + k) * 3];
            block(R[i], V, L, a[0], a[1], a[2]);
        }
        if (!ev[i])
            for (int v = 0; v < V; v++) { const int32_t* b = &vb[((size_t)i * V + v) * 3]; if (b[0]) block(R[i], V, L, v, b[1], b[2]); }
    }
    int bad = 0;
    for (int i = 0; i < n; i++) {
        std::vector<uint32_t> wf, wa;
        for (int j = 0; j < i; j++) {
            if (ev[i]) {
                if (!ev[j] && meets(Wc[j], Wc[i])) wf.push_back((uint32_t)j);
                if (!ev[j] && meets(R[j], Wc[i])) wa.push_back((uint32_t)j);
            } else {
                if (meets(Wc[j], R[i])) wf.push_back((uint32_t)j);
                if (ev[j] ? meets(Wc[j], Wc[i]) : meets(R[j], Wc[i])) wa.push_back((uint32_t)j);
            }
        }
        const std::vector<uint32_t> gf(fa.begin() + fo[i], fa.begin() + fo[i + 1]), ga(aa.begin() + ao[i], aa.begin() + ao[i + 1]);
        if (gf != wf || ga != wa) bad++;
    }
    if (fo[n] != fa.size() || ao[n] != aa.size()) bad++;
    std::printf("n %d M %d V %d levels %d events 1/%d: %zu flow, %zu anti edges, %d nodes differ\n", n, M, V, L, event_every, fa.size(), aa.size(), bad);
    return bad;
}
}  // namespace

int main() {
    int bad = 0;
    bad += run(1, 1, 1, 1, 0, 24);
    bad += run(2, 3, 2, 2, 0, 24);
    bad += run(300, 7, 3, 4, 3, 40);
    bad += run(200, 70, 5, 8, 3, 60);
    bad += run(400, 2, 50, 6, 0, 24);
    bad += run(150, 5, 1, 7, 2, 24);
    std::printf("%d failures\n", bad);
    return bad ? 1 : 0;
}
