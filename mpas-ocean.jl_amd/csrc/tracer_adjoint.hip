// tracer_adjoint.hip -- reverse mode of the passive tracer transport over a frozen flow (gfx950; moka_tracer_tape_*, NOT in the reference).
#include "tracer_patch.hpp"

namespace moka {

// ------------------------------------------------------------------------------------------------
// The tracer step is linear in phi once the provisional states P_s = (pu_s, ph_s) are given, so its reverse mode is the transpose of a
// linear map and reads nothing but those states (include/moka_hip.h states the algebra).  The transposed tendency r = R(P, y) of a
// field y that already carries invArea is again a gather over the slots of edgesOnCell, in slot order, with the forward skip rules:
//     hE = 0.5 * (ph[k,c] + ph[k,c']);  F = pu[k,e] * hE                  (the forward bits)
//     r += ((0.5 * F) * sdv[c,i]) * (y[k,c] - y[k,c'])
//     DIFF:  r += ((kappa[j] * hE) * dvdc[c,i]) * (y[k,c'] - y[k,c])       a second, separate addition
// -- sdv of the edge seen from c' is -sdv[c,i] and the mask belongs to the edge, so the scatter of the forward sum folds into the
// difference; no atomics, the forward launch's streams.  What a reverse stage does with r: TracerAdjArgs (kernels.hpp).
// SG (moka_tracer_adjoint_want_source_gradient): the head kernel and the reverse stages 3, 2, 1 add tau, the value they multiply by
// invArea to form the next gathered field, to the accumulator of every tracer whose entry of TracerAdjArgs::G is not nullptr --
// one read and one write of the cell's own element, nothing staged; y = tau * invA keeps its bits.  SG == false is the code of a sweep
// that wants no gradient.
// BIH (some recorded kappa4_j != 0; only together with DIFF): the biharmonic term is self-adjoint under the area weight, so its
// transpose is the same two passes applied to y.  M_j = Lap(ph_s, y_j) comes from launch_tracer_lap (tracers.hip: the forward pass's
// kernel) ahead of the reverse stage, and after the harmonic addition of a slot
//     r -= ((kappa4[j] * hE) * dvdc[c,i]) * (M[k,c'] - M[k,c])              a third, separate addition
// skipped by a wave-uniform branch for the tracers with kappa4[j] == 0, whose M is never written and never read.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void tracer_adj_update(const TracerAdjArgs &a, double r, double hc, double invA, double g, double sIn,
                                                  double &sOut, double &out, double &tau)
{
    if (a.rs == 0) {
        sOut = sIn;
        out = hc * (g + sIn) + r;
        tau = 0.0;
        return;
    }
    const double v = r / hc;
    sOut = a.rs == 3 ? v : sIn + v;
    tau = a.cb * g + a.ca * v;
    out = tau * invA;
}

// g = X / hn and the first gathered field y = (b4 * g) * invArea of a reverse step: elementwise over (tracer, cell, level)
template <bool SG>
__global__ __launch_bounds__(BLOCK) void k_tracer_adj_seed(const double *X, const double *hn, const double *invArea, double *g, double *y,
                                                           double b4, int K, int64_t stride, int64_t n, double *const *G)
{
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
        const int64_t off = i % stride;
        const double gg = X[i] / hn[off];
        g[i] = gg;
        const double tau = b4 * gg;
        y[i] = tau * invArea[off / K];
        if (SG)
            if (double *G_ = G[i / stride]) G_[off] += tau;
    }
}

// Generic form: LPC lanes span a column, one cell per lane group, index records; any K, any maxEdges (the shape of k_tracer_cell).
template <int LPC, bool DIFF, bool SG, bool BIH>
__global__ __launch_bounds__(BLOCK) void k_tracer_adj_cell(const MeshDev m, const TracerAdjArgs a)
{
    constexpr int NG = BLOCK / LPC;
    const int grp = uniform_if_wave<LPC>(threadIdx.x / LPC), l = threadIdx.x % LPC;
    const int K = m.K, ME = m.ME;
    for (int c = blockIdx.x * NG + grp; c < m.nC; c += gridDim.x * NG) {
        const double invA = cptr(m.invArea)[c];
        for (int k = l; k < K; k += LPC) {
            const size_t off = (size_t)c * K + k;
            const double hc = a.ph[off];
            for (int j0 = 0; j0 < a.nT; j0 += TR_TJ) {
                const int nj = min(TR_TJ, a.nT - j0);
                double r[TR_TJ], yc[TR_TJ], kap[TR_TJ], k4[BIH ? TR_TJ : 1], mc[BIH ? TR_TJ : 1];
#pragma unroll
                for (int jj = 0; jj < TR_TJ; ++jj) {
                    r[jj] = 0.0;
                    yc[jj] = jj < nj ? a.y[(size_t)(j0 + jj) * a.stride + off] : 0.0;
                    kap[jj] = DIFF && jj < nj ? cptr(a.kappa)[j0 + jj] : 0.0;
                    if (BIH) {
                        k4[jj] = jj < nj ? cptr(a.kappa4)[j0 + jj] : 0.0;
                        mc[jj] = k4[jj] != 0.0 ? a.lapy[(size_t)(j0 + jj) * a.stride + off] : 0.0;
                    }
                }
                for (int i = 0; i < ME; ++i) {
                    const int e = cptr(m.eoc)[(size_t)c * ME + i];
                    if (e < 0 || k >= cptr(m.mltc)[(size_t)c * ME + i]) continue;
                    const size_t noff = (size_t)cptr(m.coc)[(size_t)c * ME + i] * K + k;
                    const double hE = 0.5 * (hc + a.ph[noff]);
                    const double F = a.pu[(size_t)e * K + k] * hE;
                    const double w = (0.5 * F) * cptr(m.sdv)[(size_t)c * ME + i];
                    const double dd = DIFF ? cptr(a.dvdc)[(size_t)c * ME + i] : 0.0;
#pragma unroll
                    for (int jj = 0; jj < TR_TJ; ++jj)
                        if (jj < nj) {
                            const double yn = a.y[(size_t)(j0 + jj) * a.stride + noff];
                            r[jj] += w * (yc[jj] - yn);
                            if (DIFF) r[jj] += ((kap[jj] * hE) * dd) * (yn - yc[jj]);
                            if (BIH)
                                if (k4[jj] != 0.0)
                                    r[jj] -= ((k4[jj] * hE) * dd) * (a.lapy[(size_t)(j0 + jj) * a.stride + noff] - mc[jj]);
                        }
                }
#pragma unroll
                for (int jj = 0; jj < TR_TJ; ++jj)
                    if (jj < nj) {
                        const size_t joff = (size_t)(j0 + jj) * a.stride + off;
                        double sOut, out, tau;
                        tracer_adj_update(a, r[jj], hc, invA, a.g[joff], a.rs == 3 ? 0.0 : a.S[joff], sOut, out, tau);
                        if (a.rs > 0) a.S[joff] = sOut;
                        a.out[joff] = out;
                        if (SG && a.rs > 0)
                            if (double *G_ = a.G[j0 + jj]) G_[off] += tau;
                    }
            }
        }
    }
}

// Patch form (tracer_patch.hpp): k_tracer_patch's shape and LDS layout, hence its LDS formula and its chunking (tracer_kernel) -- the
// patch's records and the ph rows and the y rows of `chunk` tracers of its own cells are staged in LDS.  The slot factors
// (0.5 * F) * sdv are formed once per cell and pass and reused by the tracer loop; v = r / ph_s and ph_0 * (g + S) use the staged own row.
// BIH: a resident tracer takes a second row set, for M (row set 1 + chunk + jj), as in k_tracer_patch.
template <int ME_, bool DIFF, bool SG, bool BIH>
__global__ __launch_bounds__(TR_NT, 2) void k_tracer_adj_patch(const MeshDev m, const TracerAdjArgs a, const int chunk)
{
    static_assert(ME_ == 6, "burst width");
    static_assert(DIFF || !BIH, "BIH instantiates only together with DIFF");
    extern __shared__ __align__(16) unsigned char tra_smem[];
    const int pl_ = patch_of_block(m.nPatches);
    if (pl_ >= m.nPatches) return;
    const TracerPatch P = tracer_patch_open<ME_>(m, tra_smem, pl_, 1 + (BIH ? 2 : 1) * chunk, true, DIFF);
    const glb_bytes_t uG = (glb_bytes_t)a.pu;

    // the rows of a pass: ph (rb == 0) and y of its cj tracers, then the M rows of those with kappa4 != 0
    auto stage_rows = [&](int rb, int j0, int cj) {
        tracer_stage_rows(P, rb, cj, a.ph, a.y + (size_t)j0 * a.stride, a.stride);
        if constexpr (BIH)
            for (int jj = 0; jj < cj; ++jj)
                if (a.kappa4[j0 + jj] != 0.0) tracer_stage_set(P, 1 + chunk + jj, a.lapy + (size_t)(j0 + jj) * a.stride);
    };

    tracer_stage_records<ME_, DIFF>(P, m, a.dvdc, [&] { stage_rows(0, 0, min(chunk, a.nT)); });
    for (int j0 = 0; j0 < a.nT; j0 += chunk) {
        const int cj = min(chunk, a.nT - j0);
        if (j0 > 0) {
            __syncthreads();                      // the previous pass has read its rows
            stage_rows(1, j0, cj);
        }
        __syncthreads();
        if (!P.act) continue;
        for (int ci = P.grp; ci < P.nc; ci += TR_NG) {
            const uint32_t *rec = P.rec + (size_t)ci * P.CI;
            double2 w[ME_], hE[DIFF ? ME_ : 1];
            bool ch[ME_], okx[ME_], oky[ME_];
            uint32_t aoff[ME_], gh[ME_];
            const double *sd = P.sd + ci * ME_, *dd = P.dd + ci * ME_;
            const double2 hc = tracer_own_row(P, 0, ci);
            double2 uu[ME_], hh[ME_];
#pragma unroll
            for (int i = 0; i < ME_; ++i) uu[i] = glb_row2(uG + (rec[i] + P.lo));
            tracer_slots<ME_>(P, rec, ch, aoff, gh);
            tracer_gather<ME_>(P, 0, a.ph, ch, aoff, gh, hh);
            tracer_level_masks<ME_>(P, ci, rec[2 * ME_], okx, oky);
#pragma unroll
            for (int i = 0; i < ME_; ++i) {
                const double2 he = make_double2(0.5 * (hc.x + hh[i].x), 0.5 * (hc.y + hh[i].y));
                const double2 F = make_double2(uu[i].x * he.x, uu[i].y * he.y);
                w[i] = make_double2((0.5 * F.x) * sd[i], (0.5 * F.y) * sd[i]);
                if constexpr (DIFF) hE[i] = he;
            }
            const double invA = P.ia[ci];
            const unsigned orow = P.ownB + (unsigned)ci * P.rowB + P.lo;       // the cell's own row in every (K, nC) array
            for (int jj = 0; jj < cj; ++jj) {
                const size_t jo = (size_t)(j0 + jj) * a.stride;
                const double kap = DIFF ? a.kappa[j0 + jj] : 0.0;
                double2 yy[ME_];
                tracer_gather<ME_>(P, 1 + jj, a.y + jo, ch, aoff, gh, yy);
                const double2 yc = tracer_own_row(P, 1 + jj, ci);
                double2 r = make_double2(0.0, 0.0);
                const double kap4 = BIH ? a.kappa4[j0 + jj] : 0.0;
                const bool b4 = BIH && kap4 != 0.0;             // wave-uniform
                double2 mm[BIH ? ME_ : 1], mc = make_double2(0.0, 0.0);
                if constexpr (BIH) {
#pragma unroll
                    for (int i = 0; i < ME_; ++i) mm[i] = make_double2(0.0, 0.0);
                    if (b4) {                                   // M gathered as y is, from its own row set
                        tracer_gather<ME_>(P, 1 + chunk + jj, a.lapy + jo, ch, aoff, gh, mm);
                        mc = tracer_own_row(P, 1 + chunk + jj, ci);
                    }
                }
#pragma unroll
                for (int i = 0; i < ME_; ++i) {
                    double rx = r.x + w[i].x * (yc.x - yy[i].x), ry = r.y + w[i].y * (yc.y - yy[i].y);
                    if constexpr (DIFF) {
                        rx += ((kap * hE[i].x) * dd[i]) * (yy[i].x - yc.x);
                        ry += ((kap * hE[i].y) * dd[i]) * (yy[i].y - yc.y);
                    }
                    if constexpr (BIH)
                        if (b4) {
                            rx -= ((kap4 * hE[i].x) * dd[i]) * (mm[i].x - mc.x);
                            ry -= ((kap4 * hE[i].y) * dd[i]) * (mm[i].y - mc.y);
                        }
                    r.x = okx[i] ? rx : r.x;
                    r.y = oky[i] ? ry : r.y;
                }
                const double2 g = gload2(a.g + jo, orow);
                const double2 sIn = a.rs == 3 ? make_double2(0.0, 0.0) : gload2(a.S + jo, orow);
                double2 sOut, out, tau;
                tracer_adj_update(a, r.x, hc.x, invA, g.x, sIn.x, sOut.x, out.x, tau.x);
                tracer_adj_update(a, r.y, hc.y, invA, g.y, sIn.y, sOut.y, out.y, tau.y);
                if (a.rs > 0) gstore2(a.S + jo, orow, sOut);
                gstore2(a.out + jo, orow, out);
                if (SG && a.rs > 0)
                    if (double *G_ = a.G[j0 + jj]) {
                        const double2 G0 = gload2(G_, orow);
                        gstore2(G_, orow, make_double2(G0.x + tau.x, G0.y + tau.y));
                    }
            }
        }
    }
}



hipError_t launch_tracer_adj_seed(const MeshDev &m, const double *X, const double *hn, double *g, double *y, double b4, int nT,
                                  double *const *G, hipStream_t s)
{
    if (nT <= 0) return hipSuccess;
    const int64_t stride = (int64_t)m.K * m.nC, n = stride * nT;
    const int grid = (int)std::min<int64_t>(std::max<int64_t>((n + BLOCK - 1) / BLOCK, 1), 65536);
    if (G) hipLaunchKernelGGL(k_tracer_adj_seed<true>, dim3(grid), dim3(BLOCK), 0, s, X, hn, m.invArea, g, y, b4, m.K, stride, n, G);
    else hipLaunchKernelGGL(k_tracer_adj_seed<false>, dim3(grid), dim3(BLOCK), 0, s, X, hn, m.invArea, g, y, b4, m.K, stride, n, G);
    return hipGetLastError();
}

template <bool DIFF, bool SG, bool BIH>
static hipError_t launch_tracer_adj_generic(const MeshDev &m, const TracerAdjArgs &a, int lpc, hipStream_t s)
{
#define CALL(L) launch_tracer_cell_form(k_tracer_adj_cell<L, DIFF, SG, BIH>, L, m, a, s)
    DISPATCH_LPC(lpc, CALL)
#undef CALL
}

hipError_t launch_tracer_adjoint(const MeshDev &m, const TracerAdjArgs &a, int lpc, bool generic, hipStream_t s)
{
    if (a.nT <= 0) return hipSuccess;
    const bool diff = a.kappa != nullptr;       // (then a.dvdc is set too: moka_tracer_adjoint_sweep)
    const bool sg = a.G != nullptr;             // (some tracer's source gradient is wanted: moka_tracer_adjoint_sweep)
    const bool bih = a.kappa4 != nullptr;       // (then a.lapy, a.kappa and a.dvdc are set too: moka_tracer_adjoint_sweep)
    const TracerKernel k = tracer_adjoint_kernel(m, lpc, a.nT, generic, diff, bih);
    return pick_tracer_instance(diff, sg, bih, [&](auto D, auto S, auto B) {
        if (k.form == 1) return launch_tracer_patch_form(k_tracer_adj_patch<6, D.value, S.value, B.value>, m, a, k, s);
        return launch_tracer_adj_generic<D.value, S.value, B.value>(m, a, lpc, s);
    });
}

// ------------------------------------------------------------------------------------------------
// d J / d kappa_j and d J / d kappa4_j (TracerKgradArgs, kernels.hpp: the algebra and the summation order).  An elementwise stream with a
// column sum: no gather, so one form serves every K and every cell order -- k_tracer_adj_cell's lanes per cell, the strided loop for
// K > 64.  ph of a lane's first level is read once and kept across the groups of TR_TJ flagged tracers (for K <= 64 that is every
// element); p = ph * L is formed once and serves both products.  No atomics, no LDS: the lanes meet in group_sum's shuffles.
// ------------------------------------------------------------------------------------------------
template <int LPC>
__global__ __launch_bounds__(BLOCK) void k_tracer_kgrad(const MeshDev m, const TracerKgradArgs a)
{
    constexpr int NG = BLOCK / LPC;
    const int grp = uniform_if_wave<LPC>(threadIdx.x / LPC), l = threadIdx.x % LPC;
    const int K = m.K;
    for (int c = blockIdx.x * NG + grp; c < m.nC; c += gridDim.x * NG) {
        const double area = cptr(m.areaCell)[c];
        const size_t row = (size_t)c * K;
        const double h0 = l < K ? a.ph[row + l] : 0.0;
        for (int f0 = 0; f0 < a.nF; f0 += TR_TJ) {
            const int nf = min(TR_TJ, a.nF - f0);
            double sk[TR_TJ], s4[TR_TJ], wk0[TR_TJ], w40[TR_TJ];
            double *Wk[TR_TJ], *W4[TR_TJ];
            size_t jo[TR_TJ];
#pragma unroll
            for (int jj = 0; jj < TR_TJ; ++jj) {
                sk[jj] = 0.0;
                s4[jj] = 0.0;
                Wk[jj] = jj < nf ? cptr(a.W)[2 * (f0 + jj)] : nullptr;      // wave-uniform; the tables are kernel-invariant
                W4[jj] = jj < nf ? cptr(a.W)[2 * (f0 + jj) + 1] : nullptr;
                jo[jj] = jj < nf ? (size_t)cptr(a.tracer)[f0 + jj] * a.stride : 0;
                // lane 0 fetches the densities' old values beside the streams, not behind the shuffles
                wk0[jj] = l == 0 && Wk[jj] ? Wk[jj][c] : 0.0;
                w40[jj] = l == 0 && W4[jj] ? W4[jj][c] : 0.0;
            }
            for (int k = l; k < K; k += LPC) {
                const size_t off = row + k;
                const double hc = k == l ? h0 : a.ph[off];
#pragma unroll
                for (int jj = 0; jj < TR_TJ; ++jj)
                    if (jj < nf) {
                        const double p = hc * a.L[(size_t)(f0 + jj) * a.stride + off];
                        if (Wk[jj]) sk[jj] += p * a.y[jo[jj] + off];
                        if (W4[jj]) s4[jj] += p * a.M[jo[jj] + off];
                    }
            }
#pragma unroll
            for (int jj = 0; jj < TR_TJ; ++jj)
                if (jj < nf) {
                    if (Wk[jj]) {
                        const double t = group_sum<LPC>(sk[jj]);
                        if (l == 0) Wk[jj][c] = wk0[jj] + area * t;
                    }
                    if (W4[jj]) {
                        const double t = group_sum<LPC>(s4[jj]);
                        if (l == 0) W4[jj][c] = w40[jj] - area * t;
                    }
                }
        }
    }
}

hipError_t launch_tracer_kgrad(const MeshDev &m, const TracerKgradArgs &a, int lpc, hipStream_t s)
{
    if (a.nF <= 0) return hipSuccess;
#define CALL(L) launch_tracer_cell_form(k_tracer_kgrad<L>, L, m, a, s)
    DISPATCH_LPC(lpc, CALL)
#undef CALL
}

}  // namespace moka
