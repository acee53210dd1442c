// Host restatement of the parallel entropy decode (kernel_jpeg_entropy.hip): the product's prescan and its shared
// subsequence step (hpmvs_amd/csrc/jpeg.hpp: prescan, decode_subseq, segment_ok) compiled by g++, with everything the
// kernels do around the step -- the guess, the synchronisation rounds inside a workgroup and across workgroups, the
// check, the scan of the block counts and DC sums, the write -- run as plain loops in the kernels' order, so that the
// round count is the device's.  The truth is decode_file.
// Build: g++ -std=c++14 -O2 -fPIC -shared jpeg_entropy_host.cpp; with -DJE_MAIN a stand-alone program (for sanitizers)
// that runs the scheme over a file of [u32 length][bytes] records and compares every outcome with decode_file.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../hpmvs_amd/csrc/jpeg.hpp"

using namespace hpmvs::jpg;

namespace {

struct Chain {
    std::vector<SubState> entry, exit;
    std::vector<SubCount> cnt;
    std::vector<uint32_t> seg_of;
};

SubState run_step(const Prescan& ps, const Huff* tabs, const ScanInfo& si, uint32_t S, size_t j, uint32_t seg, SubState in, SubCount* cnt) {
    const Segment& g = ps.segs[seg];
    const uint32_t i = (uint32_t)j - g.first_sub;
    const uint64_t e = (uint64_t)(i + 1) * S;
    return decode_subseq(ps.bytes.data() + g.first_byte, g.bits, e < g.bits ? (uint32_t)e : g.bits, tabs, si, kZigzag, in, cnt, nullptr, 0, 0,
                         0, nullptr);
}

// steps 1 and 2: -> false when the rounds ran out; *rounds: the sum over the passes of a pass's slowest workgroup
bool synchronise(const Prescan& ps, const Huff* tabs, const ScanInfo& si, uint32_t S, int cap, Chain& ch, int* rounds) {
    const size_t n = ps.n_subs, G = kSubsPerGroup, n_wg = (n + G - 1) / G;
    ch.entry.assign(n, SubState{0, 0});
    ch.exit.assign(n, SubState{0, 0});
    ch.cnt.assign(n, SubCount{0, {0, 0, 0}});
    ch.seg_of.assign(n, 0);
    for (size_t s = 0; s < ps.segs.size(); s++)
        for (uint32_t i = 0; i < ps.segs[s].n_subs; i++) ch.seg_of[ps.segs[s].first_sub + i] = (uint32_t)s;
    std::vector<SubState> wg_exit[2] = {std::vector<SubState>(n_wg, SubState{0, 0}), std::vector<SubState>(n_wg, SubState{0, 0})};
    int total = 0;
    for (int pass = 0;; pass++) {
        const int budget = cap - total;
        int slowest = 0;
        bool overflow = false;
        for (size_t w = 0; w < n_wg; w++) {
            const size_t j0 = w * G, j1 = j0 + G < n ? j0 + G : n;
            if (pass == 0)
                for (size_t j = j0; j < j1; j++) {
                    const uint32_t i = (uint32_t)j - ps.segs[ch.seg_of[j]].first_sub;
                    ch.entry[j] = guess_state(i, S);
                    ch.exit[j] = run_step(ps, tabs, si, S, j, ch.seg_of[j], ch.entry[j], &ch.cnt[j]);
                }
            int r = 0;
            for (;;) {
                std::vector<SubState> seen(ch.exit.begin() + j0, ch.exit.begin() + j1);  // the exits of the round before
                std::vector<size_t> need;
                std::vector<SubState> from;
                for (size_t j = j0; j < j1; j++) {
                    if (j == ps.segs[ch.seg_of[j]].first_sub) continue;  // a segment's first: its entry is no guess
                    SubState pred;
                    if (j > j0) pred = handed_on(seen[j - 1 - j0]);
                    else if (pass == 0) continue;
                    else pred = wg_exit[(pass - 1) & 1][w - 1];
                    if (!same_state(pred, ch.entry[j])) { need.push_back(j); from.push_back(pred); }
                }
                if (need.empty()) break;
                if (r == budget) { overflow = true; break; }
                for (size_t q = 0; q < need.size(); q++) {
                    const size_t j = need[q];
                    ch.entry[j] = from[q];
                    ch.exit[j] = run_step(ps, tabs, si, S, j, ch.seg_of[j], ch.entry[j], &ch.cnt[j]);
                }
                r++;
            }
            if (j1 == j0 + G) wg_exit[pass & 1][w] = handed_on(ch.exit[j1 - 1]);
            if (r > slowest) slowest = r;
        }
        total += slowest;
        *rounds = total;
        if (overflow) return false;
        if (pass > 0 && slowest == 0) return true;
    }
}

// steps 3 to 6 (the scan carries the DC sums with the block counts: the write stores predictions at once)
bool check_and_write(const Prescan& ps, const Huff* tabs, const ScanInfo& si, uint32_t S, const Chain& ch, int16_t* coef) {
    const size_t n = ps.n_subs;
    std::vector<SubCount> incl(n);  // inclusive sums over all subsequences, mod 2^32
    SubCount run = {0, {0, 0, 0}};
    for (size_t j = 0; j < n; j++) {
        run.nblk += ch.cnt[j].nblk;
        for (int c = 0; c < 3; c++) run.dc[c] += ch.cnt[j].dc[c];
        incl[j] = run;
    }
    const SubCount zero = {0, {0, 0, 0}};
    for (size_t s = 0; s < ps.segs.size(); s++) {
        const Segment& g = ps.segs[s];
        const SubCount base = g.first_sub ? incl[g.first_sub - 1] : zero;
        for (uint32_t i = 0; i < g.n_subs; i++) {
            const size_t j = g.first_sub + i;
            const SubState want = i == 0 ? SubState{0, 0} : handed_on(ch.exit[j - 1]);
            if (!same_state(ch.entry[j], want) || (ch.exit[j].bk & kStateErr)) return false;
        }
        const size_t last = g.first_sub + g.n_subs - 1;
        if (!segment_ok(g, ch.exit[last], incl[last].nblk - base.nblk, si.bpm, s + 1 == ps.segs.size())) return false;
    }
    for (size_t s = 0; s < ps.segs.size(); s++) {
        const Segment& g = ps.segs[s];
        const SubCount base = g.first_sub ? incl[g.first_sub - 1] : zero;
        for (uint32_t i = 0; i < g.n_subs; i++) {
            const size_t j = g.first_sub + i;
            const SubCount before = j ? incl[j - 1] : zero;
            const uint32_t dc_in[3] = {before.dc[0] - base.dc[0], before.dc[1] - base.dc[1], before.dc[2] - base.dc[2]};
            const uint64_t e = (uint64_t)(i + 1) * S;
            decode_subseq(ps.bytes.data() + g.first_byte, g.bits, e < g.bits ? (uint32_t)e : g.bits, tabs, si, kZigzag, ch.entry[j], nullptr,
                          coef, before.nblk - base.nblk, g.first_mcu, g.n_mcus * (uint32_t)si.bpm, dc_in);
        }
    }
    return true;
}

void put_err(const std::string& e, char* err, int cap) {
    if (err && cap > 0) snprintf(err, (size_t)cap, "%s", e.c_str());
}

}  // namespace

extern "C" {

// number of coefficients of the file's frame (0: the headers are refused)
size_t je_n_coef(const uint8_t* bytes, size_t n) {
    Frame fr;
    std::vector<Huff> huff(8);
    size_t start = 0;
    return parse_headers(bytes, n, fr, huff.data(), &start, nullptr) == kOk ? fr.n_blocks * 64 : 0;
}

// decode_file's coefficients: the truth
int je_host(const uint8_t* bytes, size_t n, int16_t* coef, size_t cap, char* err, int errcap) {
    Frame fr;
    std::string e;
    const int rc = decode_file(bytes, n, fr, true, &e);
    put_err(e, err, errcap);
    if (rc != kOk) return rc;
    if (cap < fr.coef.size()) return kErrArg;
    for (size_t i = 0; i < fr.coef.size(); i++) coef[i] = fr.coef[i];
    return kOk;
}

// The scheme with its fallback, as the library runs it.  subseq_bits 0: the shipped size; round_cap 0: the shipped cap.
// *used: 1 the parallel decode was accepted, 0 decode_scan ran; *rounds: synchronisation rounds (0 without a prescan).
int je_decode(const uint8_t* bytes, size_t n, int subseq_bits, int round_cap, int16_t* coef, size_t cap, int* used, int* rounds, char* err,
              int errcap) {
    *used = 0;
    *rounds = 0;
    Frame fr;
    std::string e;
    std::vector<Huff> huff(8);
    size_t start = 0;
    int rc = parse_headers(bytes, n, fr, huff.data(), &start, &e);
    put_err(e, err, errcap);
    if (rc != kOk) return rc;
    if (cap < fr.n_blocks * 64) return kErrArg;
    const uint32_t S = subseq_bits ? (uint32_t)subseq_bits : (uint32_t)kSubseqBits;
    Prescan ps;
    if (prescan(bytes, n, start, fr, ps)) {
        plan_subsequences(ps, S);
        std::vector<Huff> tabs(6);
        scan_tables(fr, huff.data(), tabs.data());
        const ScanInfo si = make_scan_info(fr);
        Chain ch;
        std::vector<int16_t> out(fr.n_blocks * 64, 0);
        if (synchronise(ps, tabs.data(), si, S, round_cap ? round_cap : sync_round_cap(S), ch, rounds) &&
            check_and_write(ps, tabs.data(), si, S, ch, out.data())) {
            for (size_t i = 0; i < out.size(); i++) coef[i] = out[i];
            *used = 1;
            return kOk;
        }
    }
    rc = decode_scan(bytes, n, start, fr, huff.data(), true, &e);
    put_err(e, err, errcap);
    if (rc != kOk) return rc;
    for (size_t i = 0; i < fr.coef.size(); i++) coef[i] = fr.coef[i];
    return kOk;
}

}  // extern "C"

#ifdef JE_MAIN
// records of [u32 little-endian length][bytes]; every record is decoded at every subsequence size given and compared with
// decode_file.  Prints "records accepted_by_host parallel fallbacks mismatches"; exit status 1 on a mismatch.
int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int> sizes;
    for (int a = 2; a < argc; a++) sizes.push_back(atoi(argv[a]));
    size_t records = 0, host_ok = 0, parallel = 0, fallbacks = 0, mismatches = 0;
    for (;;) {
        uint8_t l[4];
        if (fread(l, 1, 4, f) != 4) break;
        const size_t n = (size_t)l[0] | (size_t)l[1] << 8 | (size_t)l[2] << 16 | (size_t)l[3] << 24;
        std::vector<uint8_t> bytes(n);
        if (n && fread(bytes.data(), 1, n, f) != n) return 2;
        records++;
        const size_t nc = je_n_coef(bytes.data(), n);
        std::vector<int16_t> a(nc + 1), b(nc + 1);
        char ea[256] = "", eb[256] = "";
        const int ra = je_host(bytes.data(), n, a.data(), nc, ea, 256);
        host_ok += ra == kOk;
        for (int S : sizes) {
            int used = 0, rounds = 0;
            const int rb = je_decode(bytes.data(), n, S, 0, b.data(), nc, &used, &rounds, eb, 256);
            if (ra == kOk) (used ? parallel : fallbacks)++;
            bool same = ra == rb && std::string(ea) == std::string(eb);
            if (same && ra == kOk)
                for (size_t i = 0; i < nc; i++) same = same && a[i] == b[i];
            if (!same) {
                mismatches++;
                fprintf(stderr, "record %zu, %d bits: host %d '%s', scheme %d '%s' (used %d)\n", records - 1, S, ra, ea, rb, eb, used);
            }
        }
    }
    fclose(f);
    printf("%zu %zu %zu %zu %zu\n", records, host_ok, parallel, fallbacks, mismatches);
    return mismatches ? 1 : 0;
}
#endif
