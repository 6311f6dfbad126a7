// mvmix_index.hpp -- the index bookkeeping of the tile forms of the vertical momentum pass and of its transpose (momentum_vmix.hip), in
// a form that also compiles for the host: tools/mvmix_index_check.cpp walks it under the host sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define MV_HD __host__ __device__ __forceinline__
#else
#define MV_HD inline
#endif

namespace moka {

// element e of a tile's span -> its place in a column set (magic = 2^32 / K + 1: exact while e * K < 2^32)
MV_HD unsigned mv_slot(unsigned e, unsigned magic, unsigned K, unsigned cs, unsigned &col)
{
#if defined(__HIP_DEVICE_COMPILE__)
    col = __umulhi(e, magic);
#else
    col = (unsigned)(((uint64_t)e * magic) >> 32);
#endif
    return col * cs + (e - col * K);
}
MV_HD unsigned mv_magic(unsigned K) { return (unsigned)((1ull << 32) / K) + 1u; }

// tile `t` of te edge columns of an (K, nE) field: its first edge, its columns, the elements and the offset of its contiguous span
struct MvSpan {
    int e0, ncol;
    unsigned nEl;
    size_t base;
};
MV_HD MvSpan mv_span(int t, int te, int nE, int K)
{
    MvSpan s;
    s.e0 = t * te;
    s.ncol = te < nE - s.e0 ? te : nE - s.e0;
    s.nEl = (unsigned)s.ncol * (unsigned)K;
    s.base = (size_t)s.e0 * K;
    return s;
}
// dynamic LDS of a tile: `sets` column sets of cs = K | 1 doubles and a 16-byte record per column
MV_HD size_t mv_tile_lds(int sets, int te, int K) { return (size_t)sets * te * (K | 1) * 8 + 16 * (size_t)te; }

}  // namespace moka
