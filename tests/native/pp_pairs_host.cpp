// pp_pairs_host.cpp -- the ping-pong kernel's row pairing and in-register schedule
// (graph.h pp_pair_rows, build_pp_inreg_schedule) checked on the host: a stand-alone
// program over graph.cpp, built with -fsanitize=address,undefined by
// tests/test_pp_pairs_host.py and run directly.
//   usage: pp_pairs_host 80211n_1944_r12.alist 80211n_1296_r12.alist
#include "graph.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace ldpc;

static int g_fail = 0;
#define EXPECT(cond, ...)                                 \
    do {                                                  \
        if (!(cond)) {                                    \
            ++g_fail;                                     \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
        }                                                 \
    } while (0)

static int row_of(const ldpc_graph &g, int v, int e) { return (int)(g.col_refs[g.col_ptr[v] + e] >> kRefShift); }

// The properties every pairing has, whatever the code.
static void check_pairing(const ldpc_graph &g, int threads, int dc_low, int dc, const PPPairing &pr)
{
    const int half = threads / 2;
    std::vector<int> seen(g.M, 0);
    for (int sl = 0; sl < 2 * threads; ++sl) {
        const int j = pr.row_of_slot[sl];
        if (j < 0) continue;
        EXPECT(j < g.M, "slot %d holds row %d", sl, j);
        if (j < g.M) ++seen[j];
        const bool capped = sl < threads || sl - threads >= half;
        EXPECT(g.row_deg[j] <= (capped ? dc_low : dc), "slot %d (capped %d) holds a row of degree %d", sl, (int)capped,
               (int)g.row_deg[j]);
    }
    for (int j = 0; j < g.M; ++j) EXPECT(seen[j] == 1, "row %d placed %d times", j, seen[j]);
    int pairs = 0;
    std::vector<char> bit_used(g.N, 0);
    for (int t = 0; t < threads; ++t) {
        const int v = pr.bit_of_thread[t];
        if (v < 0) continue;
        ++pairs;
        EXPECT(g.col_deg[v] == 2 && !bit_used[v], "thread %d: bit %d of degree %d (used %d)", t, v, (int)g.col_deg[v],
               (int)bit_used[v]);
        bit_used[v] = 1;
        const int r0 = pr.row_of_slot[t], r1 = pr.row_of_slot[threads + t];
        const int a = row_of(g, v, 0), b = row_of(g, v, 1);
        EXPECT((r0 == a && r1 == b) || (r0 == b && r1 == a), "thread %d: rows %d,%d are not bit %d's neighbours %d,%d", t,
               r0, r1, v, a, b);
        EXPECT((pr.first_r[t] ? r1 : r0) == a, "thread %d: first flag %d but nlist starts at row %d (r0 %d, r1 %d)", t,
               (int)pr.first_r[t], a, r0, r1);
        EXPECT(t < half || !pr.first_r[t], "thread %d of the capped half has its first row at r = 1", t);
    }
    EXPECT(pairs == pr.pairs, "pairs %d but %d threads hold a bit", pr.pairs, pairs);
}

// The schedule over it: the in-register edge at the last position of both rows, every other
// edge of every row present once, no bit slot for the in-register bits.
static void check_schedule(const ldpc_graph &g, int threads, int dc_low, int dc, const PPPairing &pr, const RowSchedule &s,
                           const std::vector<uint8_t> &fl)
{
    const int half = threads / 2, dcs = g.maxdc > 0 ? g.maxdc : 1;
    EXPECT(fl.size() == (size_t)threads + threads / 64, "flags size %zu", fl.size());
    for (int t = 0; t < threads; ++t) {
        const int v = pr.bit_of_thread[t];
        EXPECT((fl[t] & 1) == (v >= 0) && ((fl[t] >> 1) & 1) == (v >= 0 && pr.first_r[t]), "thread %d flags %d", t, (int)fl[t]);
        for (int r = 0; r < 2; ++r) {
            const int sl = r * threads + t, j = pr.row_of_slot[sl], last = (r == 1 && t < half ? dc : dc_low) - 1;
            const uint16_t *cols = &s.cn_cols[(size_t)sl * dc], *pos = &s.cn_pos[(size_t)sl * dc];
            if (j < 0) continue;
            const int d = g.row_deg[j];
            std::vector<int> want(g.row_cols.begin() + (size_t)j * dcs, g.row_cols.begin() + (size_t)j * dcs + d), got;
            for (int k = 0; k <= last; ++k) {
                if (cols[k] == g.N) {
                    EXPECT(pos[k] >= s.e_pad && pos[k] < s.e_pad + 64, "slot %d padding edge %d scatters to %d", sl, k, (int)pos[k]);
                    continue;
                }
                got.push_back(cols[k]);
                if (v >= 0 && cols[k] == v) {
                    EXPECT(k == last, "slot %d: in-register bit at position %d, not %d", sl, k, last);
                    EXPECT(pos[k] >= s.e_pad && pos[k] < s.e_pad + 64, "slot %d: in-register edge scatters to %d", sl, (int)pos[k]);
                } else {
                    EXPECT(pos[k] < s.e_pad, "slot %d edge %d scatters to %d (e_pad %d)", sl, k, (int)pos[k], s.e_pad);
                }
            }
            std::sort(want.begin(), want.end());
            std::sort(got.begin(), got.end());
            EXPECT(want == got, "slot %d does not hold row %d's bits", sl, j);
            if (v >= 0) EXPECT(cols[last] == v, "slot %d: last position holds %d, not bit %d", sl, (int)cols[last], v);
        }
    }
    std::vector<char> slot_bit(g.N, 0);
    for (uint16_t c : s.vn_col)
        if (c != 0xffff) {
            EXPECT(c < g.N && !slot_bit[c], "bit slot of %d", (int)c);
            if (c < g.N) slot_bit[c] = 1;
        }
    for (int v = 0; v < g.N; ++v) {
        bool inreg = false;
        for (int t = 0; t < threads; ++t) inreg |= pr.bit_of_thread[t] == v;
        EXPECT(slot_bit[v] != inreg, "bit %d: bit slot %d, in-register %d", v, (int)slot_bit[v], (int)inreg);
    }
}

// M rows joined into one path by M - 1 degree-2 bits (deg2) or not at all, plus degree-3 bits
// over rows (i, i + 1, i + 3 mod M): row degree 3, or up to 5 on the path.
static ldpc_graph synthetic(int M, bool deg2)
{
    std::vector<std::vector<int>> nl, ml(M);
    auto add_bit = [&](std::vector<int> rows) {
        for (int j : rows) ml[j].push_back((int)nl.size() + 1);
        for (int &j : rows) ++j;
        nl.push_back(rows);
    };
    if (deg2)
        for (int i = 0; i + 1 < M; ++i) add_bit(i & 1 ? std::vector<int>{i + 1, i} : std::vector<int>{i, i + 1});
    for (int i = 0; i < M; ++i) add_bit({i, (i + 1) % M, (i + 3) % M});
    const int N = (int)nl.size();
    std::vector<int> wn(N), wm(M);
    std::vector<const int *> np(N), mp(M);
    for (int i = 0; i < N; ++i) { wn[i] = (int)nl[i].size(); np[i] = nl[i].data(); }
    for (int j = 0; j < M; ++j) { wm[j] = (int)ml[j].size(); mp[j] = ml[j].data(); }
    ldpc_graph g;
    const std::string err = build_graph(N, M, wn.data(), np.data(), wm.data(), mp.data(), g);
    EXPECT(err.empty(), "synthetic graph: %s", err.c_str());
    return g;
}

int main(int argc, char **argv)
{
    if (argc != 3) {
        std::fprintf(stderr, "usage: pp_pairs_host 80211n_1944_r12.alist 80211n_1296_r12.alist\n");
        return 2;
    }
    {   // the bench code: Z = 81, 12 block rows, block rows 6 and 11 of degree 8
        ldpc_graph g;
        const std::string err = load_alist(argv[1], g);
        EXPECT(err.empty(), "%s", err.c_str());
        if (!err.empty()) return 1;
        PPPairing pr;
        const bool ok = pp_pair_rows(g, 512, 7, 8, pr);
        EXPECT(ok && pr.pairs == 486, "bench code: ok %d, %d pairs", (int)ok, pr.pairs);
        if (!ok) return 1;
        check_pairing(g, 512, 7, 8, pr);
        int blockpair[12] = {}, first1[12] = {}, first0[12] = {};
        for (int t = 0; t < 512; ++t) {
            if (pr.bit_of_thread[t] < 0) continue;
            const int r0 = pr.row_of_slot[t], r1 = pr.row_of_slot[512 + t], lo = std::min(r0, r1), hi = std::max(r0, r1);
            EXPECT(hi == lo + 81 && (lo / 81) % 2 == 0, "thread %d pairs rows %d and %d", t, r0, r1);
            ++blockpair[lo / 81];
            ++(pr.first_r[t] ? first1 : first0)[lo / 81];
            if (lo / 81 == 6) EXPECT(r1 == lo && t < 256, "thread %d: the degree-8 row %d of block row 6 is not at r = 1", t, lo);
            if (lo / 81 == 10) EXPECT(r1 == hi && t < 256, "thread %d: the degree-8 row %d of block row 11 is not at r = 1", t, hi);
        }
        for (int b = 0; b < 12; b += 2) EXPECT(blockpair[b] == 81, "block pair (%d,%d): %d pairs", b, b + 1, blockpair[b]);
        // block row 6 (degree 8) sits at r = 1 and comes first in its bits' nlist (lower row index first)
        EXPECT(first1[6] == 81 && first0[6] == 0, "block pair (6,7): %d first at r = 1, %d at r = 0", first1[6], first0[6]);
        EXPECT(first0[10] == 81 && first1[10] == 0, "block pair (10,11): %d first at r = 0, %d at r = 1", first0[10], first1[10]);
        std::printf("bench code: %d pairs; (6,7) first at r=1: %d, (10,11) first at r=0: %d\n", pr.pairs, first1[6], first0[10]);
        RowSchedule s;
        std::vector<uint8_t> fl;
        const std::string e2 = build_pp_inreg_schedule(g, 512, 4, 8, 7, pr, s, fl);
        EXPECT(e2.empty(), "%s", e2.c_str());
        if (e2.empty()) {
            check_schedule(g, 512, 7, 8, pr, s, fl);
            int pure = 0;
            for (int w = 0; w < 8; ++w) pure += fl[512 + w];
            EXPECT(s.e_pad == 6208 && pure == 8, "bench code: e_pad %d, %d waves without LDS at the last positions", s.e_pad, pure);
            std::printf("bench code: e_pad %d, pure waves %d\n", s.e_pad, pure);
        }
    }
    {   // Z = 54 (N = 1296, M = 648) on 512 check threads: 324 pairs, 188 threads without one, block rows
        // of 54 rows so that runs of pairs straddle the 64-lane wave boundaries
        ldpc_graph g;
        const std::string err = load_alist(argv[2], g);
        EXPECT(err.empty(), "%s", err.c_str());
        PPPairing pr;
        const bool ok = err.empty() && pp_pair_rows(g, 512, 7, 8, pr);
        EXPECT(ok && pr.pairs == 324, "Z = 54: ok %d, %d pairs", (int)ok, pr.pairs);
        if (ok) {
            check_pairing(g, 512, 7, 8, pr);
            int none = 0;
            for (int t = 0; t < 512; ++t) none += pr.bit_of_thread[t] < 0 && pr.row_of_slot[t] < 0 && pr.row_of_slot[512 + t] < 0;
            RowSchedule s;
            std::vector<uint8_t> fl;
            const std::string e2 = build_pp_inreg_schedule(g, 512, 4, 8, 7, pr, s, fl);
            EXPECT(e2.empty(), "%s", e2.c_str());
            int pure = 0;
            if (e2.empty()) {
                check_schedule(g, 512, 7, 8, pr, s, fl);
                for (int w = 0; w < 8; ++w) pure += fl[512 + w];
            }
            EXPECT(none == 188 && pure == 8, "Z = 54: %d empty threads, %d waves without LDS at the last positions", none, pure);
            std::printf("Z=54: %d pairs, %d empty threads, pure waves %d\n", pr.pairs, none, pure);
        }
    }
    {   // no degree-2 bit: no schedule
        const ldpc_graph g = synthetic(200, false);
        PPPairing pr;
        EXPECT(!pp_pair_rows(g, 128, 7, 8, pr) && pr.pairs == 0 && pr.row_of_slot.empty(), "a code without degree-2 bits paired");
    }
    {   // a path of odd length: one row stays alone
        const ldpc_graph g = synthetic(201, true);
        PPPairing pr;
        const bool ok = pp_pair_rows(g, 128, 7, 8, pr);
        EXPECT(ok && pr.pairs == 100, "odd path: ok %d, %d pairs", (int)ok, pr.pairs);
        if (ok) {
            check_pairing(g, 128, 7, 8, pr);
            RowSchedule s;
            std::vector<uint8_t> fl;
            const std::string e2 = build_pp_inreg_schedule(g, 128, 4, 8, 7, pr, s, fl);
            EXPECT(e2.empty(), "%s", e2.c_str());
            if (e2.empty()) check_schedule(g, 128, 7, 8, pr, s, fl);
        }
        std::printf("odd path: %d pairs of 201 rows\n", pr.pairs);
    }
    std::printf("%s (%d failures)\n", g_fail ? "FAILED" : "ok", g_fail);
    return g_fail ? 1 : 0;
}
