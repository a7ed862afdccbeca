// Host tables of a quasi-cyclic LDPC code for the coded link simulation (link.hip): the bit-packed generator B^-1 A of the systematic
// encoder and the edge lists of the decoder, built from the descriptor's base matrix of circulant shifts and lifting size.  Host code
// only (no HIP header): link.hip uploads the tables, link_tables_check.cpp builds them under the sanitizers (`make check-link`).
#pragma once
#include <stdint.h>
#include <string>
#include <vector>

namespace sbc {

constexpr int LINK_MAX_N = 8192;        // edge and bit indices are stored in 16 bits and a codeword lives in LDS
constexpr int LINK_MAX_DC = 8;          // a check's messages live in registers during its update
constexpr int LINK_MAX_EDGES = 32768;

struct LinkTables {
    int rows = 0, cols = 0, Z = 0;      // base matrix and lifting size
    int M = 0, N = 0, K = 0, E = 0;     // checks, bits, payload bits, edges
    int Kw = 0;                         // 32-bit words of a packed payload
    int dc_max = 0, dv_max = 0;
    std::vector<uint32_t> gen;          // [M][Kw]: parity bit j = parity of (gen[j] & payload)
    std::vector<uint16_t> cptr, vptr;   // [M + 1], [N + 1]: a check's / a variable's first edge
    std::vector<uint16_t> evar;         // [E]: the variable of edge e (edges check by check, ascending column)
    std::vector<uint16_t> vedge;        // [E]: a variable's edges, by ascending check
    std::vector<int32_t> P;             // [N]: interleaver, bitsInt[i] = bitsEnc[P[i]]
};

// 0: built; 1: invalid descriptor; 2: unsupported (sizes, degrees, singular parity part).  `why` says which.
inline int build_link_tables(const int32_t* base, int rows, int cols, int Z, const int32_t* interleaver, LinkTables& t, std::string& why) {
    if (!base || !interleaver) { why = "NULL base matrix or interleaver"; return 1; }
    if (rows < 1 || cols <= rows || Z < 1) { why = "need rows >= 1, cols > rows and Z >= 1"; return 1; }
    if ((int64_t)cols * Z > LINK_MAX_N) { why = "more than " + std::to_string(LINK_MAX_N) + " code bits"; return 2; }
    t.rows = rows; t.cols = cols; t.Z = Z;
    t.M = rows * Z; t.N = cols * Z; t.K = t.N - t.M; t.Kw = (t.K + 31) / 32;
    for (int i = 0; i < rows * cols; ++i)
        if (base[i] < -1 || base[i] >= Z) { why = "a shift outside [-1, Z)"; return 1; }
    // the interleaver must be a permutation of 0 .. N - 1
    std::vector<uint8_t> seen(t.N, 0);
    t.P.assign(interleaver, interleaver + t.N);
    for (int i = 0; i < t.N; ++i) {
        const int32_t p = t.P[i];
        if (p < 0 || p >= t.N || seen[p]) { why = "the interleaver is not a permutation of 0 .. N - 1"; return 1; }
        seen[p] = 1;
    }
    // edges: row i of block (r, c) with shift s has its one in column (i + s) mod Z  (circshift(eye(Z), [0 s]))
    std::vector<std::vector<int>> row_cols(t.M);
    std::vector<int> col_deg(t.N, 0);
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) {                 // ascending c: a check's columns come out sorted
            const int s = base[r * cols + c];
            if (s < 0) continue;
            for (int i = 0; i < Z; ++i) {
                const int col = c * Z + (i + s) % Z;
                row_cols[r * Z + i].push_back(col);
                ++col_deg[col];
            }
        }
    t.E = 0; t.dc_max = 0; t.dv_max = 0;
    for (int m = 0; m < t.M; ++m) {
        const int d = (int)row_cols[m].size();
        if (d < 2) { why = "a check with fewer than two edges"; return 2; }
        if (d > t.dc_max) t.dc_max = d;
        t.E += d;
    }
    for (int v = 0; v < t.N; ++v) {
        if (col_deg[v] < 1) { why = "a code bit in no check"; return 2; }
        if (col_deg[v] > t.dv_max) t.dv_max = col_deg[v];
    }
    if (t.dc_max > LINK_MAX_DC) { why = "check degree above " + std::to_string(LINK_MAX_DC); return 2; }
    if (t.E > LINK_MAX_EDGES) { why = "more than " + std::to_string(LINK_MAX_EDGES) + " edges"; return 2; }
    t.cptr.assign(t.M + 1, 0); t.vptr.assign(t.N + 1, 0);
    t.evar.resize(t.E); t.vedge.resize(t.E);
    int e = 0;
    for (int m = 0; m < t.M; ++m) {
        t.cptr[m] = (uint16_t)e;
        for (int col : row_cols[m]) t.evar[e++] = (uint16_t)col;
    }
    t.cptr[t.M] = (uint16_t)e;
    int acc = 0;
    for (int v = 0; v < t.N; ++v) { t.vptr[v] = (uint16_t)acc; acc += col_deg[v]; }
    t.vptr[t.N] = (uint16_t)acc;
    std::vector<int> fill(t.N, 0);
    for (e = 0; e < t.E; ++e) {                          // ascending edge = ascending check
        const int v = t.evar[e];
        t.vedge[t.vptr[v] + fill[v]++] = (uint16_t)e;
    }
    // Gaussian elimination over GF(2) on the bit-packed rows of [B | A]  ->  [I | B^-1 A]   (H = [A | B], A the K payload columns)
    const int W = (t.N + 31) / 32;
    std::vector<uint32_t> aug((size_t)t.M * W, 0u);
    auto flip = [&](int m, int bit) { aug[(size_t)m * W + (bit >> 5)] ^= 1u << (bit & 31); };
    for (int m = 0; m < t.M; ++m)
        for (int col : row_cols[m]) flip(m, col >= t.K ? col - t.K : t.M + col);
    for (int col = 0; col < t.M; ++col) {
        int piv = -1;
        for (int m = col; m < t.M && piv < 0; ++m)
            if ((aug[(size_t)m * W + (col >> 5)] >> (col & 31)) & 1u) piv = m;
        if (piv < 0) { why = "the parity part of the check matrix is singular over GF(2)"; return 2; }
        if (piv != col)
            for (int w = 0; w < W; ++w) std::swap(aug[(size_t)piv * W + w], aug[(size_t)col * W + w]);
        for (int m = 0; m < t.M; ++m)
            if (m != col && ((aug[(size_t)m * W + (col >> 5)] >> (col & 31)) & 1u))
                for (int w = 0; w < W; ++w) aug[(size_t)m * W + w] ^= aug[(size_t)col * W + w];
    }
    t.gen.assign((size_t)t.M * t.Kw, 0u);
    for (int m = 0; m < t.M; ++m)
        for (int k = 0; k < t.K; ++k) {
            const int bit = t.M + k;
            if ((aug[(size_t)m * W + (bit >> 5)] >> (bit & 31)) & 1u) t.gen[(size_t)m * t.Kw + (k >> 5)] |= 1u << (k & 31);
        }
    return 0;
}

}  // namespace sbc
