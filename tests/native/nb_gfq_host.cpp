// nb_gfq_host.cpp -- the host side of the GF(4) / GF(8) EMS kernels without a GPU, built with
// AddressSanitizer and UBSan by tests/test_ems_gfq_host.py: the message layout (nb_layout.h) for
// q = 4, 8 and 16, the GF products of nb_graph.cpp against shift-and-reduce, the packed schedule
// tables, and the kernel choice (nb_plan). Prints one "plan N M E q maxdc -> kind lds slot" line per
// queried shape (stdin-free: the shapes are arguments, five numbers each) and exits 0, or prints
// the failed check and exits 1.
#include "nb_graph.h"
#include "nb_layout.h"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

static int failures = 0;
#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            std::printf("FAILED %s: ", #cond);    \
            std::printf(__VA_ARGS__);             \
            std::printf("\n");                    \
            ++failures;                           \
        }                                         \
    } while (0)

// q = 16 as it was before the smaller fields: lambda(p, 10) and chunk strides
static const int kLambda16K10[16] = {0,     4,     8,     12,    16400, 16404, 16408, 16412,
                                     32800, 32804, 32808, 32812, 49200, 49204, 49208, 49212};
static const int kEp[][3] = {{2, 1, 4}, {4, 500, 2048}, {8, 40, 512}, {5, 600, 4096}, {4, 8200, 65536}, {4, 6000, 32768}};

static int slow_mul(int q, int poly, int a, int b)
{
    int r = 0;
    for (int i = 0; (1 << i) < q; ++i)
        if ((b >> i) & 1) r ^= a << i;
    int m = 0;
    while ((1 << m) < q) ++m;
    for (int bit = 2 * m - 2; bit >= m; --bit)   // the carry-less product, reduced from the top
        if ((r >> bit) & 1) r ^= poly << (bit - m);
    return r;
}

static void layout(int q, int maxdc, int M)
{
    const int Ep = ldpc::nb_ep(maxdc, M), k = ldpc::nb_ep_log2(Ep);
    const long bytes = (long)Ep * q * 4;
    CHECK((1 << k) == Ep && Ep >= maxdc * M, "q=%d Ep=%d", q, Ep);
    // a slot's q entries: distinct, 4-byte aligned, inside the array
    for (int s = 0; s < Ep; s += (s < 70 || s > Ep - 70) ? 1 : 37) {
        std::set<long> seen;
        for (int p = 0; p < q; ++p) {
            const long a = ((long)s << 4) ^ ldpc::nb_lambda(p, k);
            CHECK(a >= 0 && a + 4 <= bytes && (a & 3) == 0, "q=%d slot %d entry %d at %ld of %ld", q, s, p, a, bytes);
            seen.insert(a);
        }
        CHECK((int)seen.size() == q, "q=%d slot %d: %zu addresses", q, s, seen.size());
    }
    // a wave's 64 consecutive slots: chunk c of each in a 16-byte unit of its own, all inside chunk c's region
    for (int s0 = 0; s0 + 64 <= Ep; s0 += 64) {
        for (int c = 0; c < q / 4; ++c) {
            std::set<long> units;
            for (int s = s0; s < s0 + 64; ++s) {
                const long a = ((long)s << 4) ^ ldpc::nb_lambda(4 * c, k);
                CHECK((a & 15) == 0 && a / 16 / Ep == c, "q=%d slot %d chunk %d at %ld", q, s, c, a);
                for (int i = 1; i < 4; ++i)
                    CHECK((((long)s << 4) ^ ldpc::nb_lambda(4 * c + i, k)) == a + 4 * i, "q=%d slot %d chunk %d entry %d", q, s, c, i);
                units.insert(a / 16);
            }
            CHECK(units.size() == 64, "q=%d slots %d..: chunk %d in %zu units", q, s0, c, units.size());
        }
    }
}

int main(int argc, char **argv)
{
    for (int p = 0; p < 16; ++p) CHECK(ldpc::nb_lambda(p, 10) == kLambda16K10[p], "lambda(%d, 10) = %d", p, ldpc::nb_lambda(p, 10));
    for (const auto &e : kEp) CHECK(ldpc::nb_ep(e[0], e[1]) == e[2], "nb_ep(%d, %d) = %d", e[0], e[1], ldpc::nb_ep(e[0], e[1]));
    CHECK(ldpc::nb_q_supported(4) && ldpc::nb_q_supported(8) && ldpc::nb_q_supported(16), "supported sizes");
    CHECK(!ldpc::nb_q_supported(2) && !ldpc::nb_q_supported(32) && !ldpc::nb_q_supported(64) && !ldpc::nb_q_supported(12), "refused sizes");
    for (int q : {4, 8, 16}) {
        layout(q, 4, 48);
        layout(q, 5, 600);
        layout(q, 2, 1);
    }
    // GF(4) over x^2+x+1, GF(8) over x^3+x+1, GF(16) over x^4+x+1
    const int polys[][2] = {{4, 0x7}, {8, 0xB}, {16, 0x13}};
    for (const auto &f : polys) {
        const int q = f[0];
        CHECK(ldpc::gf_poly(q) == f[1], "gf_poly(%d)", q);
        for (int a = 0; a < q; ++a)
            for (int b = 0; b < q; ++b) {
                const int want = slow_mul(q, f[1], a, b), got = ldpc::gf_mul(q, a, b);
                CHECK(got == want && got < q, "GF(%d): %d * %d = %d, want %d", q, a, b, got, want);
                // the kernels' product: h * 2^i by xtime (top power -> x + 1), xor over the bits of b
                int hp = a, acc = 0;
                for (int i = 0; (1 << i) < q; ++i) {
                    if ((b >> i) & 1) acc ^= hp;
                    hp = ((hp << 1) & (q - 1)) ^ ((hp & (q >> 1)) ? 3 : 0);
                }
                CHECK(acc == want, "GF(%d) by xtime: %d * %d = %d, want %d", q, a, b, acc, want);
            }
    }
    // the packed schedule and the swizzle of a small GF(8) graph: f = 0 below GF(16)
    {
        ldpc::NbLists cols(6), rows(3);
        const int h[3][4] = {{1, 5, 7, 2}, {3, 3, 6, 4}, {2, 1, 1, 7}};
        const int c[3][4] = {{0, 1, 2, 3}, {2, 3, 4, 5}, {4, 5, 0, 1}};
        for (int j = 0; j < 3; ++j)
            for (int k = 0; k < 4; ++k) {
                rows[j].push_back({c[j][k], h[j][k]});
                cols[c[j][k]].push_back({j, h[j][k]});
            }
        ldpc_nb_graph g;
        std::string msg;
        CHECK(ldpc::nb_build_graph(6, 3, 8, cols, rows, g, msg) == 0, "%s", msg.c_str());
        ldpc::NbTables t;
        ldpc::nb_tables(g, t);
        CHECK(t.cn_d.size() == 3 && t.vn.size() == 6 && t.vslot.size() == 12 && t.colh_swz == t.colh, "table sizes");
        for (int j = 0; j < 3; ++j) CHECK(t.cn_d[j] == 4, "cn_d[%d]", j);
        for (int v = 0; v < 6; ++v) CHECK(t.vn[v] == (((uint32_t)g.col_ptr[v] << 8) | 2u), "vn[%d] = %u", v, t.vn[v]);
        for (int e = 0; e < 12; ++e) CHECK(t.vslot[e] == t.pslot[e] && t.vslot[e] < 12 && (t.colh[e] >> 3) == 0, "edge %d", e);
    }
    static const char *const names[] = {"-", "ems_lds", "ems_global", "ems_global_sched"};
    for (int i = 1; i + 4 < argc; i += 5) {
        const int N = std::atoi(argv[i]), M = std::atoi(argv[i + 1]), E = std::atoi(argv[i + 2]), q = std::atoi(argv[i + 3]),
                  maxdc = std::atoi(argv[i + 4]);
        int m = 0;
        while ((1 << m) < q) ++m;
        const ldpc::NbPlan p = ldpc::nb_plan(N, M, E, q, m, maxdc);
        std::printf("plan %d %d %d %d %d -> %s %zu %zu\n", N, M, E, q, maxdc, names[p.kind], p.lds_bytes, p.slot_bytes);
    }
    return failures ? 1 : 0;
}
