// vmix_closure.hip -- the Richardson-number closure of the two implicit vertical passes (gfx950; moka_set_richardson_mixing, NOT in the
// reference): the viscosity F per interface and edge and the diffusivity G per interface and cell, in the Pacanowski-Philander form,
// from the new level as stage 4 of an RK4 step and the tracers' stage 4 left it.  Two launches behind stage 4, in front of the tracer
// pass (which takes G through its field instances) and the momentum pass (which takes F through its FIELD instances).
//
// include/moka_hip.h states the recipe; the two kernels below are it, once each.  Every operation is rounded once (-ffp-contract=off)
// in the order written there, so the numpy twin of the tests agrees bit for bit.  Both kernels are elementwise in k apart from the
// k+1 neighbour, and the arrays are level-fastest, so the lanes run along k: LPC = min(64, the power of two >= K) lanes own one edge
// (cell) column and take the interfaces k = l, l + LPC, ... < n - 1; the loads of u, h and b and the stores of F and G are then
// contiguous 8-byte lanes of one column.
// The k+1 operand is a second load of the same lines, not a lane shift.  In the ISA hipcc fuses the two adjacent 8-byte loads of an
// operand pair into ONE global_load_dwordx4 per lane (8-byte aligned; neighbouring lanes overlap by one double): five of them per
// interface in the edge kernel, issued back to back ahead of counted s_waitcnt vmcnt(3..0); two for h and b plus one per passing slot
// in the cell kernel, under one s_waitcnt vmcnt(0).  The second operand therefore costs no further instruction and no further line, only
// bytes through the vector L1.  A shift would take a DPP move per 16-lane row with a fix-up of each row's edge lane (or two
// ds_bpermute_b32 per double), an extra load for the last lane of a group whenever K > LPC, and selects around both -- more
// instructions than it saves, in kernels that wait on HBM for u, F and G (profiles/richardson_summary.txt).
// Levels no active element reads are never loaded: u[k,e] at k >= n_e, h and b at k >= nLev[c]; the edge kernel reads b[k+1,c] and
// h[k+1,c] only for k+1 <= n_e - 1 < nLev[c].  Rows k >= n - 1 of F and G are never written.  No LDS, no atomics, any K, any
// maxEdges <= RC_ME, every kernel variant.
// DIAG (moka_richardson_diagnose): the same arithmetic also stores Ri, and F / G only where their pointer is non-null; the step's
// launches are the instances without it.
#include "kernels_common.hpp"

namespace moka {

constexpr int RC_ME = 8;                // the slots of a cell the gfx950 kernels support (moka_mesh_create refuses more)
constexpr double RC_EPS = 1e-20;        // EPS of the recipe

// Ri > 0:  t = 1 + alpha * Ri;  m = nu0 / (t * t);  the edge value nuB + m, the cell value kB + (nuB + m) / t
// else:    nuB + nu0 (kB + (nuB + nu0)), plus conv where db < 0
template <bool CELL>
__device__ __forceinline__ double rich_coefficient(const RichArgs &a, const double Ri, const double db)
{
    double out;
    if (Ri > 0.0) {
        const double t = 1.0 + a.alpha * Ri;
        const double m = a.nu0 / (t * t);
        out = CELL ? a.kB + (a.nuB + m) / t : a.nuB + m;
    } else {
        out = CELL ? a.kB + (a.nuB + a.nu0) : a.nuB + a.nu0;
        if (db < 0.0) out = out + a.conv;
    }
    return out;
}

template <bool DIAG>
__global__ __launch_bounds__(BLOCK) void k_rich_edge(const RichArgs a, const int lpc)
{
    const size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t e = t / (unsigned)lpc;
    const int l = (int)(t - e * (unsigned)lpc);
    if (e >= (size_t)a.nE) return;
    const int4 r = *reinterpret_cast<const int4 *>(a.ehdr + e * 4);
    asm volatile("" ::"v"(r.x), "v"(r.y), "v"(r.w));      // the whole record before the exit below: one 16-byte load, not the depth first and the cells behind it
    const int n = min(r.w, a.K);
    if (n < 2) return;                               // (the cells of such an edge are not read)
    const double *u = a.u + e * a.K;
    const double *h1 = a.h + (size_t)r.x * a.K, *h2 = a.h + (size_t)r.y * a.K;
    const double *b1 = a.b + (size_t)r.x * a.K, *b2 = a.b + (size_t)r.y * a.K;
    for (int k = l; k < n - 1; k += lpc) {
        const double h1k = h1[k], h1n = h1[k + 1], h2k = h2[k], h2n = h2[k + 1];
        const double b1k = b1[k], b1n = b1[k + 1], b2k = b2[k], b2n = b2[k + 1];
        const double uk = u[k], un = u[k + 1];
        const double hEk = 0.5 * (h1k + h2k), hEn = 0.5 * (h1n + h2n);
        const double hm = 0.5 * (hEk + hEn);
        const double db = 0.5 * ((b1k - b1n) + (b2k - b2n));
        const double du = uk - un;
        const double Ri = (db * hm) / (du * du + RC_EPS);
        const double f = rich_coefficient<false>(a, Ri, db);
        if (DIAG) {
            if (a.riE) a.riE[e * a.K + k] = Ri;
            if (a.F) a.F[e * a.K + k] = f;
        } else {
            a.F[e * a.K + k] = f;
        }
    }
}

// The slot loop is that of k_mvmix_bottom_speed: the cell's eoc / mltc rows and kc of its edges first (the same addresses in every
// lane of the column: one request each), the depth test from mltc without a dependent read of the edge's header, every u load of the
// passing slots in flight before the sum, the sum in slot order in registers.
template <bool DIAG>
__global__ __launch_bounds__(BLOCK) void k_rich_cell(const RichArgs a, const int lpc)
{
    const size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t c = t / (unsigned)lpc;
    const int l = (int)(t - c * (unsigned)lpc);
    if (c >= (size_t)a.nC) return;
    const int n = min(a.nLev[c], a.K);
    // Every load below is unconditional, so that none waits for another: a slot past maxEdges re-reads the last one and is masked, an
    // empty slot (eoc -1, mltc 0) and an edge too shallow for the interface have their address replaced by the lane's own h[k], h[k+1]
    // -- u[.,e'] of such a slot is not read, and what is read in its place is dropped by the select in front of the sum.
    int ee[RC_ME], ml[RC_ME];
    double kc[RC_ME];
    const size_t row = c * a.ME;
#pragma unroll
    for (int i = 0; i < RC_ME; ++i) {
        const int ii = min(i, a.ME - 1);
        ee[i] = a.eoc[row + ii];
        ml[i] = a.mltc[row + ii];
    }
#pragma unroll
    for (int i = 0; i < RC_ME; ++i) asm volatile("" ::"v"(ee[i]), "v"(ml[i]));      // the rows go out beside nLev[c], not behind the exit below
    if (n < 2) return;
#pragma unroll
    for (int i = 0; i < RC_ME; ++i) {
        ml[i] = i < a.ME && ee[i] >= 0 ? min(ml[i], a.K) : 0;
        ee[i] = max(ee[i], 0);
    }
#pragma unroll
    for (int i = 0; i < RC_ME; ++i) kc[i] = a.keCoef[ee[i]];
    const double invA = a.invArea[c];
    const double *h = a.h + c * a.K, *b = a.b + c * a.K;
    for (int k = l; k < n - 1; k += lpc) {
        const double hk = h[k], hn = h[k + 1], bk = b[k], bn = b[k + 1];
        double xk[RC_ME], xn[RC_ME];
#pragma unroll
        for (int i = 0; i < RC_ME; ++i) {
            const double *x = ml[i] > k + 1 ? a.u + (size_t)ee[i] * a.K + k : h + k;
            xk[i] = x[0];
            xn[i] = x[1];
        }
        const double hm = 0.5 * (hk + hn);
        const double db = bk - bn;
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < RC_ME; ++i)
            if (ml[i] > k + 1) {
                const double du = xk[i] - xn[i];
                acc = acc + (kc[i] * du) * du;
            }
        const double S2 = 2.0 * (acc * invA);
        const double Ri = (db * hm) / (S2 + RC_EPS);
        const double g = rich_coefficient<true>(a, Ri, db);
        if (DIAG) {
            if (a.riC) a.riC[c * a.K + k] = Ri;
            if (a.G) a.G[c * a.K + k] = g;
        } else {
            a.G[c * a.K + k] = g;
        }
    }
}

// The step's form (F and G and neither Ri: both are written unconditionally) or the diagnostic one (any of the four outputs may be
// nullptr; a kernel none of whose outputs is wanted is not launched).  Nothing is launched for K < 2.
hipError_t launch_richardson(const RichArgs &a, hipStream_t s)
{
    if (a.K < 2 || a.nE <= 0 || a.nC <= 0) return hipSuccess;
    if (a.ME < 1 || a.ME > RC_ME ||!a.ehdr || !a.eoc || !a.mltc || !a.nLev || !a.keCoef || !a.invArea || !a.u || !a.h || !a.b) return hipErrorInvalidValue;
    const bool diag = a.riE || a.riC || !a.F || !a.G;
    int lpc = 1;
    while (lpc < a.K && lpc < 64) lpc *= 2;
    const size_t tE = (size_t)a.nE * lpc, tC = (size_t)a.nC * lpc;
    if (((tE > tC ? tE : tC) + BLOCK - 1) / BLOCK >= (1ull << 31)) return hipErrorInvalidValue;
    const dim3 gE((unsigned)((tE + BLOCK - 1) / BLOCK)), gC((unsigned)((tC + BLOCK - 1) / BLOCK));
    if (diag) {
        if (a.riE || a.F) hipLaunchKernelGGL(k_rich_edge<true>, gE, dim3(BLOCK), 0, s, a, lpc);
        if (a.riC || a.G) hipLaunchKernelGGL(k_rich_cell<true>, gC, dim3(BLOCK), 0, s, a, lpc);
    } else {
        hipLaunchKernelGGL(k_rich_edge<false>, gE, dim3(BLOCK), 0, s, a, lpc);
        hipLaunchKernelGGL(k_rich_cell<false>, gC, dim3(BLOCK), 0, s, a, lpc);
    }
    return hipGetLastError();
}

}  // namespace moka
