// Host check of the index bookkeeping of the vertical momentum pass's tile forms (csrc/mvmix_index.hpp: mv_span, mv_slot, mv_magic,
// mv_tile_lds) at the set counts in use -- 3 (forward, with or without a viscosity field), 4 (transposed pass) and 5 (transposed pass
// of a step that ran with a field: both tile widths, every K up to 64).  Stand-alone; meant for the host sanitizers:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I mpas-ocean.jl_amd/csrc tools/mvmix_index_check.cpp -o /tmp/mvmix_index_check
//     /tmp/mvmix_index_check
// For every K and a few edge counts it walks every tile as the kernels do: each element of the span goes to its slot of each column
// set of a heap buffer of exactly mv_tile_lds bytes (a slot out of range is an out-of-bounds write the sanitizer reports), every slot
// of a column's K rows is hit exactly once, the span stays inside the (K, nE) field, and the record array behind the sets is 16-byte
// aligned.  The tile widths are vmix_kernel's, restated.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mvmix_index.hpp"

using namespace moka;

static int tile_columns(int K, int sets)
{
    const size_t cu = 160 * 1024;
    const int cs = K | 1;
    if (K >= 2)
        for (int tc : {64, 32}) {
            const size_t lds = (size_t)sets * tc * cs * 8 + (size_t)tc * 4;
            if (lds * (tc == 64 ? 4 : 2) <= cu) return tc;
        }
    return 0;
}

int main()
{
    long tiles = 0, elems = 0;
    if (tile_columns(15, 5) != 64 || tile_columns(16, 5) != 32 || tile_columns(63, 5) != 32 || tile_columns(64, 5) != 0 ||
        mv_tile_lds(5, 32, 63) != 81152) { std::printf("the five-set boundaries moved\n"); return 1; }
    for (int sets : {3, 4, 5})
        for (int K = 2; K <= 110; ++K) {
            const int te = tile_columns(K, sets);
            if (!te) continue;
            const unsigned cs = (unsigned)K | 1u, magic = mv_magic((unsigned)K);
            const size_t lds = mv_tile_lds(sets, te, K);
            if (lds > 80 * 1024) { std::printf("K %d sets %d: %zu bytes of LDS exceed the 80 KiB the launchers raise to\n", K, sets, lds); return 1; }
            if (((size_t)sets * te * cs * 8) % 16) { std::printf("K %d sets %d: records off the 16-byte grid\n", K, sets); return 1; }
            for (int nE : {1, te - 1, te, te + 1, 3 * te + 7}) {
                std::vector<double> field((size_t)nE * K, 1.0);
                for (int t = 0; t < (nE + te - 1) / te; ++t, ++tiles) {
                    const MvSpan sp = mv_span(t, te, nE, K);
                    if (sp.ncol < 1 || sp.ncol > te || sp.base + sp.nEl > field.size()) { std::printf("K %d nE %d tile %d: span out of the field\n", K, nE, t); return 1; }
                    double *smem = static_cast<double *>(std::malloc(lds));      // exactly the tile's bytes: the sanitizer guards both ends
                    for (size_t i = 0; i < lds / 8; ++i) smem[i] = 0.0;
                    for (unsigned e = 0; e < sp.nEl; ++e, ++elems) {
                        unsigned col;
                        const unsigned q = mv_slot(e, magic, (unsigned)K, cs, col);
                        if (col != e / (unsigned)K || q != col * cs + e % (unsigned)K) { std::printf("K %d: element %u -> column %u slot %u\n", K, e, col, q); return 1; }
                        for (int s = 0; s < sets; ++s) smem[(size_t)s * te * cs + q] += field[sp.base + e];
                    }
                    for (int s = 0; s < sets; ++s)
                        for (int c = 0; c < sp.ncol; ++c)
                            for (int k = 0; k < K; ++k)
                                if (smem[(size_t)s * te * cs + (size_t)c * cs + k] != 1.0) { std::printf("K %d set %d column %d row %d hit %g times\n", K, s, c, k, smem[(size_t)s * te * cs + (size_t)c * cs + k]); return 1; }
                    std::free(smem);
                }
            }
        }
    std::printf("mvmix index check: %ld tiles, %ld elements, no finding\n", tiles, elems);
    return 0;
}
