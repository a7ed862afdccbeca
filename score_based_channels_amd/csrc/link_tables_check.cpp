// Stand-alone host program for `make check-link`: builds the generator and edge tables of link_tables.h under the address and
// undefined-behaviour sanitizers -- the 802.11n (648, 324) code of the reference and its base at Z = 56, a small code with uneven check degrees
// at three sizes, one with check degrees 2, 5, 6 and 7, and every refusal -- and checks what link.hip relies on: H c = 0 for encoded payloads, every edge listed once per side, sorted lists.
#include "link_tables.h"
#include <stdio.h>
#include <stdlib.h>
#include <numeric>

using namespace sbc;

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static const int32_t REF_BASE[12 * 24] = {
    0, -1, -1, -1, 0, 0, -1, -1, 0, -1, -1, 0, 1, 0, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    22, 0, -1, -1, 17, -1, 0, 0, 12, -1, -1, -1, -1, 0, 0, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    6, -1, 0, -1, 10, -1, -1, -1, 24, -1, 0, -1, -1, -1, 0, 0, -1, -1, -1, -1, -1, -1, -1, -1,
    2, -1, -1, 0, 20, -1, -1, -1, 25, 0, -1, -1, -1, -1, -1, 0, 0, -1, -1, -1, -1, -1, -1, -1,
    23, -1, -1, -1, 3, -1, -1, -1, 0, -1, 9, 11, -1, -1, -1, -1, 0, 0, -1, -1, -1, -1, -1, -1,
    24, -1, 23, 1, 17, -1, 3, -1, 10, -1, -1, -1, -1, -1, -1, -1, -1, 0, 0, -1, -1, -1, -1, -1,
    25, -1, -1, -1, 8, -1, -1, -1, 7, 18, -1, -1, 0, -1, -1, -1, -1, -1, 0, 0, -1, -1, -1, -1,
    13, 24, -1, -1, 0, -1, 8, -1, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 0, -1, -1, -1,
    7, 20, -1, 16, 22, 10, -1, -1, 23, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 0, -1, -1,
    11, -1, -1, -1, 19, -1, -1, -1, 13, -1, 3, 17, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 0, -1,
    25, -1, 8, -1, 23, 18, -1, 14, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 0,
    3, -1, -1, -1, 16, -1, -1, 2, 25, 5, -1, -1, 1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0};
static const int32_t SMALL_BASE[3 * 6] = {0, 1, -1, 0, -1, -1, 2, -1, 3, 0, 0, -1, -1, 4, 1, -1, 0, 0};
// check degrees 2, 5, 6, 7 and variable degrees 1 .. 4 (tests/link_cases.py)
static const int32_t MIXED_BASE[4 * 8] = {3, -1, -1, -1, 0, -1, -1, -1, 1, 2, 0, -1, 4, 0, -1, -1, 0, 4, 1, 2, -1, 3, 0, -1, 2, 0, 3, 1, 1, -1, 2, 0};

static std::vector<int32_t> reversed_interleaver(int N) {
    std::vector<int32_t> p(N);
    std::iota(p.begin(), p.end(), 0);
    for (int i = 0; i < N / 2; ++i) std::swap(p[i], p[N - 1 - i]);
    return p;
}

// encode pseudo-random payloads with the generator and check every parity equation on the edge lists
static void check_code(const int32_t* base, int rows, int cols, int Z, int want_edges, int want_dc, int want_dv) {
    LinkTables t;
    std::string why;
    const std::vector<int32_t> P = reversed_interleaver(cols * Z);
    EXPECT(build_link_tables(base, rows, cols, Z, P.data(), t, why) == 0);
    EXPECT(t.E == want_edges && t.dc_max == want_dc && t.dv_max == want_dv);
    EXPECT(t.cptr[t.M] == t.E && t.vptr[t.N] == t.E && (int)t.gen.size() == t.M * t.Kw);
    std::vector<int> seen(t.E, 0);
    for (int v = 0; v < t.N; ++v)
        for (int q = t.vptr[v]; q < t.vptr[v + 1]; ++q) {
            EXPECT(t.evar[t.vedge[q]] == v);
            EXPECT(q == t.vptr[v] || t.vedge[q] > t.vedge[q - 1]);
            ++seen[t.vedge[q]];
        }
    for (int e = 0; e < t.E; ++e) EXPECT(seen[e] == 1);
    for (int m = 0; m < t.M; ++m)
        for (int q = t.cptr[m] + 1; q < t.cptr[m + 1]; ++q) EXPECT(t.evar[q] > t.evar[q - 1]);
    uint32_t state = 12345u;
    for (int trial = 0; trial < 20; ++trial) {
        std::vector<uint32_t> u(t.Kw, 0u);
        std::vector<uint8_t> cw(t.N, 0);
        for (int k = 0; k < t.K; ++k) {
            state = state * 1664525u + 1013904223u;
            cw[k] = (state >> 16) & 1u;
            u[k >> 5] |= (uint32_t)cw[k] << (k & 31);
        }
        for (int j = 0; j < t.M; ++j) {
            uint32_t acc = 0;
            for (int w = 0; w < t.Kw; ++w) acc ^= t.gen[(size_t)j * t.Kw + w] & u[w];
            cw[t.K + j] = __builtin_popcount(acc) & 1;
        }
        int bad = 0;
        for (int m = 0; m < t.M; ++m) {
            int x = 0;
            for (int q = t.cptr[m]; q < t.cptr[m + 1]; ++q) x ^= cw[t.evar[q]];
            bad += x;
        }
        EXPECT(bad == 0);
    }
}

static void check_refusal(const int32_t* base, int rows, int cols, int Z, const int32_t* P, int want) {
    LinkTables t;
    std::string why;
    EXPECT(build_link_tables(base, rows, cols, Z, P, t, why) == want);
    EXPECT(!why.empty());
}

int main() {
    check_code(REF_BASE, 12, 24, 27, 2376, 8, 12);
    check_code(SMALL_BASE, 3, 6, 5, 55, 4, 2);
    check_code(SMALL_BASE, 3, 6, 10, 110, 4, 2);
    check_code(MIXED_BASE, 4, 8, 7, 140, 7, 4);
    check_code(REF_BASE, 12, 24, 56, 4928, 8, 12);                               // one codeword per decoder workgroup
    check_code(SMALL_BASE, 3, 6, 120, 1320, 4, 2);
    const std::vector<int32_t> P30 = reversed_interleaver(30);
    std::vector<int32_t> twice = P30;
    twice[3] = twice[4];
    check_refusal(nullptr, 3, 6, 5, P30.data(), 1);
    check_refusal(SMALL_BASE, 3, 6, 5, nullptr, 1);
    check_refusal(SMALL_BASE, 3, 6, 5, twice.data(), 1);                         // not a permutation
    check_refusal(SMALL_BASE, 3, 6, 4, P30.data(), 1);                           // a shift of 4 with Z = 4
    check_refusal(SMALL_BASE, 6, 3, 5, P30.data(), 1);                           // no payload columns
    const int32_t singular[2 * 4] = {0, 0, 0, 0, 1, 2, 0, 0};                   // two equal parity block columns
    const std::vector<int32_t> P20 = reversed_interleaver(20);
    check_refusal(singular, 2, 4, 5, P20.data(), 2);
    const int32_t wide[1 * 10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};                // check degree 10
    check_refusal(wide, 1, 10, 2, P20.data(), 2);
    const int32_t lonely[2 * 3] = {0, -1, 0, -1, -1, 0};                        // a check with one edge
    const std::vector<int32_t> P15 = reversed_interleaver(15);
    check_refusal(lonely, 2, 3, 5, P15.data(), 2);
    std::vector<int32_t> big(2 * 24, 0);
    const std::vector<int32_t> Pbig = reversed_interleaver(24 * 400);
    check_refusal(big.data(), 2, 24, 400, Pbig.data(), 2);                       // more than 8192 bits
    if (failures) { printf("%d check(s) failed\n", failures); return 1; }
    printf("link tables: 6 codes and 9 refusals built and freed clean\n");
    return 0;
}
