// tracer_patch.hpp -- the row cache of the patch-form tracer kernels, written once: k_tracer_patch and k_tracer_lap_patch (tracers.hip) and
// k_tracer_adj_patch (tracer_adjoint.hip) differ in what a slot contributes and in their epilogues, not in any line of this file.
#pragma once
#include <type_traits>

#include "kernels_common.hpp"

namespace moka {

constexpr int TR_NT = 256;            // threads of a patch-form workgroup
constexpr int TR_NG = TR_NT / 32;     // ... and its half-waves: the cells it works on at a time
constexpr int TR_TJ = 4;              // tracers whose sums a lane of a generic-form kernel carries at once (a slot's factor is formed once per TR_TJ)

// ------------------------------------------------------------------------------------------------
// Patch form (even 34 <= K <= 64, hexagon-width byte-offset records): one workgroup per patch, half a wave per cell, a lane owns levels
// 2l and 2l + 1 (16 bytes).  The patch's cRec records, slot weights, invArea and maxLevelEdgeTop entries and `rowSets` row sets of its
// own cells -- set 0 the ph rows, the others a gathered field each -- are staged in LDS; a cell then reads its neighbours' cached rows in
// one burst of ds_read_b128 and overwrites the lanes of foreign rows with exec-masked global loads by 32-bit byte offset (k_nl_prep5's
// row cache).  The layout, in the order of the carve:
//     rows [rowSets][maxOwnC][K] | sdv [maxOwnC][ME] (hasSdv) | dvdc [maxOwnC][ME] (hasDvdc) | invArea [maxOwnC] | cRec [maxOwnC][CI] |
//     maxLevelEdgeTop of the slot's edge [maxOwnC][ME]
// tracer_patch_lds is its byte count for 1 + chunk row sets (bih: 1 + 2 chunk) with the sdv slice always there: the Laplacian kernel
// keeps dvdc where the others keep sdv and is launched with the size of (diff, bih) = (false, false).
// ------------------------------------------------------------------------------------------------
inline size_t tracer_patch_lds(const MeshDev &m, int chunk, bool diff, bool bih)
{
    return (size_t)(1 + (bih ? 2 : 1) * chunk) * m.maxOwnC * m.K * 8 + (size_t)m.maxOwnC * (m.ME + 1) * 8 +
           (size_t)m.maxOwnC * (m.CI + m.ME) * 4 + (diff ? (size_t)m.maxOwnC * m.ME * 8 : 0);
}

// what a workgroup knows of its patch and a lane of its place in it
struct TracerPatch {
    double *rows, *sd, *dd, *ia;      // the LDS arrays, as carved
    uint32_t *rec;
    int *ml;
    int tid, grp, l, K, CI, mC;       // half-wave grp, lane l of it; maxOwnC
    int c0, nc;                       // the patch's cells [c0, c0 + nc)
    bool act;                         // the lane owns levels of the column
    unsigned rowB, lo;                // bytes of a row; of the lane's levels in it
    unsigned ownB, ownN;              // byte offset of row c0 in a (K, nC) array, bytes of the patch's rows
    uint32_t ldsH;                    // LDS address of the lane's levels in row 0 of set 0
};

// the carve and the geometry of local patch pl_ = patch_of_block(m.nPatches) < m.nPatches (the grid is rounded up to the XCD count: a kernel
// returns on a block without a patch before it comes here)
template <int ME_>
__device__ __forceinline__ TracerPatch tracer_patch_open(const MeshDev &m, unsigned char *smem, int pl_, int rowSets, bool hasSdv, bool hasDvdc)
{
    TracerPatch P;
    P.tid = threadIdx.x, P.grp = P.tid >> 5, P.l = P.tid & 31, P.K = m.K, P.CI = m.CI, P.mC = m.maxOwnC;
    P.act = 2 * P.l < P.K;
    P.rowB = (unsigned)P.K * 8u, P.lo = (unsigned)P.l * 16u;
    P.rows = reinterpret_cast<double *>(smem);
    P.sd = P.rows + (size_t)rowSets * P.mC * P.K;
    P.dd = P.sd + (hasSdv ? (size_t)P.mC * ME_ : 0);
    P.ia = P.dd + (hasDvdc ? (size_t)P.mC * ME_ : 0);
    P.rec = reinterpret_cast<uint32_t *>(P.ia + P.mC);
    P.ml = reinterpret_cast<int *>(P.rec + (size_t)P.mC * P.CI);
    const int p = pl_ + m.patchBegin;
    P.c0 = m.patchCellStart[p], P.nc = m.patchCellStart[p + 1] - P.c0;
    P.ownB = (unsigned)P.c0 * P.rowB, P.ownN = (unsigned)P.nc * P.rowB;
    P.ldsH = (uint32_t)(size_t)P.rows + P.lo;
    return P;
}

// the lane's levels of own cell ci in row set ty
__device__ __forceinline__ double2 tracer_own_row(const TracerPatch &P, int ty, int ci)
{
    return reinterpret_cast<const double2 *>(P.rows + ((size_t)ty * P.mC + ci) * P.K)[P.l];
}

// rows [rb * nc, (1 + cj) * nc) of the cache from global memory: row set 0 = ph, 1 + jj = field jj of the cj that lie `stride` apart from
// `field` on; eight in flight per half-wave
__device__ __forceinline__ void tracer_stage_rows(const TracerPatch &P, int rb, int cj, const double *ph, const double *field, int64_t stride)
{
    if (!P.act) return;
    const int nc = P.nc, nrows = (1 + cj) * nc;
    for (int q0 = rb * nc + P.grp; q0 < nrows; q0 += 8 * TR_NG) {
        double2 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int q = q0 + j * TR_NG;
            v[j] = make_double2(0.0, 0.0);
            if (q < nrows) {
                const int ty = q / nc, ci = q - ty * nc;
                const double *src = ty == 0 ? ph : field + (size_t)(ty - 1) * stride;
                v[j] = *reinterpret_cast<const double2 *>(reinterpret_cast<const char *>(src) + (P.ownB + (unsigned)ci * P.rowB + P.lo));
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int q = q0 + j * TR_NG;
            if (q < nrows) {
                const int ty = q / nc, ci = q - ty * nc;
                reinterpret_cast<double2 *>(P.rows + ((size_t)ty * P.mC + ci) * P.K)[P.l] = v[j];
            }
        }
    }
}

// row set ty of the cache from global memory, the patch's own cells of the (K, nC) array `base`
__device__ __forceinline__ void tracer_stage_set(const TracerPatch &P, int ty, const double *base)
{
    if (!P.act) return;
    const char *src = reinterpret_cast<const char *>(base);
    double *dst = P.rows + (size_t)ty * P.mC * P.K;
    for (int ci = P.grp; ci < P.nc; ci += TR_NG)
        reinterpret_cast<double2 *>(dst + (size_t)ci * P.K)[P.l] = *reinterpret_cast<const double2 *>(src + (P.ownB + (unsigned)ci * P.rowB + P.lo));
}

// The records of the forward and the reverse kernel (cRec, sdv, dvdc with DD, maxLevelEdgeTop, invArea): the first TR_NT entries of each list
// go through registers, and rows() -- the kernel's row staging -- runs between their loads and the first LDS write, so that every global
// load of the phase is issued before that write; lists longer than TR_NT (large patch_cells) finish in plain loops.
template <int ME_, bool DD, class Rows>
__device__ __forceinline__ void tracer_stage_records(const TracerPatch &P, const MeshDev &m, const double *dvdc, Rows rows)
{
    const int tid = P.tid, c0 = P.c0, nc = P.nc, nRec = nc * P.CI, nSd = nc * ME_;
    const uint32_t r0 = tid < nRec ? m.cRec[(size_t)c0 * P.CI + tid] : 0u;
    const double sd0 = tid < nSd ? m.sdv[(size_t)c0 * ME_ + tid] : 0.0;
    const double dd0 = DD && tid < nSd ? dvdc[(size_t)c0 * ME_ + tid] : 0.0;
    const int ml0 = tid < nSd ? m.mltc[(size_t)c0 * ME_ + tid] : 0;
    const double ia0 = tid < nc ? m.invArea[c0 + tid] : 0.0;
    rows();
    if (tid < nRec) P.rec[tid] = r0;
    if (tid < nSd) { P.sd[tid] = sd0; P.ml[tid] = ml0; }
    if (DD && tid < nSd) P.dd[tid] = dd0;
    if (tid < nc) P.ia[tid] = ia0;
    for (int i = tid + TR_NT; i < nRec; i += TR_NT) P.rec[i] = m.cRec[(size_t)c0 * P.CI + i];
    for (int i = tid + TR_NT; i < nSd; i += TR_NT) { P.sd[i] = m.sdv[(size_t)c0 * ME_ + i]; P.ml[i] = m.mltc[(size_t)c0 * ME_ + i]; }
    if (DD)
        for (int i = tid + TR_NT; i < nSd; i += TR_NT) P.dd[i] = dvdc[(size_t)c0 * ME_ + i];
    for (int i = tid + TR_NT; i < nc; i += TR_NT) P.ia[i] = m.invArea[c0 + i];
}

// The neighbour rows of a cell from its record: per slot, whether the row is cached (ch), its byte offset in a row set (aoff: row 0 for a
// foreign row, whose lanes tracer_gather then overwrites) and the lane's byte offset in a (K, nC) array (gh).
template <int ME_>
__device__ __forceinline__ void tracer_slots(const TracerPatch &P, const uint32_t *rec, bool (&ch)[ME_], uint32_t (&aoff)[ME_], uint32_t (&gh)[ME_])
{
#pragma unroll
    for (int i = 0; i < ME_; ++i) {
        const unsigned ho = rec[ME_ + i], loc = ho - P.ownB;
        ch[i] = loc < P.ownN;
        aoff[i] = ch[i] ? loc : 0u;
        gh[i] = ho + P.lo;
        asm("" : "+v"(gh[i]));             // the offset stays in a VGPR (see k_nl_prep5)
    }
}

// the lane's levels of the slots' rows of one field: row set ty of the cache in one burst, then foreign rows from `field` by masked global loads
template <int ME_>
__device__ __forceinline__ void tracer_gather(const TracerPatch &P, int ty, const double *field, const bool (&ch)[ME_], const uint32_t (&aoff)[ME_],
                                              const uint32_t (&gh)[ME_], double2 (&v)[ME_])
{
    const glb_bytes_t G = (glb_bytes_t)field;
    const uint32_t lds = P.ldsH + (uint32_t)ty * (uint32_t)P.mC * P.rowB;
    uint32_t ad[ME_];
    v4u_t r[ME_];
#pragma unroll
    for (int i = 0; i < ME_; ++i) ad[i] = lds + aoff[i];
    lds_burst<ME_>(r, ad);
#pragma unroll
    for (int i = 0; i < ME_; ++i) {
        v[i] = __builtin_bit_cast(double2, r[i]);
        if (!ch[i]) v[i] = glb_row2(G + gh[i]);
    }
}

// does slot i of own cell ci contribute to the lane's level 2l (okx) and 2l + 1 (oky): the record's slot mask and maxLevelEdgeTop of the edge
template <int ME_>
__device__ __forceinline__ void tracer_level_masks(const TracerPatch &P, int ci, unsigned mask, bool (&okx)[ME_], bool (&oky)[ME_])
{
#pragma unroll
    for (int i = 0; i < ME_; ++i) {
        const int ml = P.ml[ci * ME_ + i];
        const bool valid = (mask >> i) & 1u;
        okx[i] = valid && 2 * P.l < ml;
        oky[i] = valid && 2 * P.l + 1 < ml;
    }
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
// a patch-form kernel over the patches of m, with k.lds bytes of dynamic LDS (raised above the default 64 KB at the kernel's first large launch)
template <class Args>
static hipError_t launch_tracer_patch_form(void (*kern)(MeshDev, Args, int), const MeshDev &m, const Args &a, const TracerKernel &k, hipStream_t s)
{
    if (k.lds > 64 * 1024)
        if (hipError_t e = raise_dyn_lds({reinterpret_cast<const void *>(kern)}, 80 * 1024); e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(patch_grid(m)), dim3(TR_NT), k.lds, s, m, a, k.chunk);
    return hipGetLastError();
}

// a generic-form kernel of LPC = lpc lanes per column over the cells of m
template <class Args>
static hipError_t launch_tracer_cell_form(void (*kern)(MeshDev, Args), int lpc, const MeshDev &m, const Args &a, hipStream_t s)
{
    const int ng = BLOCK / lpc;
    const int grid = std::min(std::max((m.nC + ng - 1) / ng, 1), 65536);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(BLOCK), 0, s, m, a);
    return hipGetLastError();
}

// f(DIFF, X, BIH) with the three switches of a forward (X = SRC) or reverse (X = SG) launch as std::bool_constant values: the six
// instantiations that exist.  BIH instantiates only together with DIFF.
template <class F>
static hipError_t pick_tracer_instance(bool diff, bool x, bool bih, F f)
{
    constexpr std::true_type T{};
    constexpr std::false_type N{};
    if (bih && !diff) return hipErrorInvalidValue;
    return bih    ? (x ? f(T, T, T) : f(T, N, T))
           : diff ? (x ? f(T, T, N) : f(T, N, N))
                  : (x ? f(N, T, N) : f(N, N, N));
}

}  // namespace moka
