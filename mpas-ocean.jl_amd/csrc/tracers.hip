// tracers.hip -- passive tracer transport beside the RK4 stages of libmoka_hip (gfx950; moka_set_tracers, NOT in the reference).
#include "tracer_patch.hpp"

namespace moka {

// ------------------------------------------------------------------------------------------------
// Conservative flux form d(h phi)/dt = -div(F phi_e) with the thickness flux F = u * h_e of the thickness equation and the centred
// edge value phi_e = (phi_c + phi_c') / 2.  Per cell c and level k the tendency accumulates from 0.0 over the slots of edgesOnCell
// in slot order (empty slots and slots with k >= maxLevelEdgeTop of the edge skipped):
//     hE = 0.5 * (ph[k,c] + ph[k,c']);  F = pu[k,e] * hE;  pE = 0.5 * (pphi[k,c] + pphi[k,c']);  T += ((F * pE) * sdv[c,i]) * invArea[c]
// -- the thickness tendency of k_stage_nl with F * pE for F, so that a tracer that is 1 everywhere reproduces tendLayerThickness,
// and then the provisional and the new thickness, bit for bit: it stays exactly 1.0.  One launch serves every tracer of the state:
// F of a slot is formed once and reused by the tracer loop.  What a stage does with T: TracerArgs (kernels.hpp).
// DIFF (moka_set_tracer_diffusion: some kappa_j != 0) adds the harmonic term div(kappa_j h_e grad phi): after the advective addition
// of a slot, a second, separate one,
//     G = pphi[k,c'] - pphi[k,c];  T += ((((kappa[j] * hE) * G) * dvdc[c,i]) * invArea[c]),   dvdc = dvEdge[e] / dcEdge[e] (plan.cpp)
// -- G == 0 for a constant tracer, the product antisymmetric between the two cells of an edge, and +-0.0 for kappa[j] == 0, which
// leaves the bits of T alone.  DIFF == false is the code of a state that never set a diffusivity.
// SRC (moka_tracer_source_upload: some tracer has a source q_j) adds, behind the whole slot loop, T = T + q_j[k,c] with a rounding of its
// own, for the tracers whose entry of TracerArgs::src is not nullptr; the others read no source byte and add nothing.  T is never -0.0
// there (it starts at +0.0 and x + (-x) = +0.0), so a source of +-0.0 leaves its bits alone.  The source element is the cell's own,
// read from global memory beside hnext, cphi and qn: nothing of it is staged.  SRC == false is the code of a state without sources.
// BIH (moka_set_tracer_biharmonic: some kappa4_j != 0; only together with DIFF) adds -div(kappa4_j h_e grad L_j) with
// L_j = Lap(ph, pphi_j) of launch_tracer_lap (further down): after the harmonic addition of a slot, a third, separate one,
//     T -= ((((kappa4[j] * hE) * (L[k,c'] - L[k,c])) * dvdc[c,i]) * invArea[c])
// skipped by a wave-uniform branch for the tracers with kappa4[j] == 0, whose L is never written and never read (an uninitialised NaN
// times zero would be NaN).  A constant tracer has L == 0 exactly; the product is antisymmetric between the two cells of an edge.
// BIH == false is the code of a state that never set a kappa4.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void tracer_update(const TracerArgs &a, double t, double cphi, double hcur, double hnext, double qnIn,
                                              double &pOut, double &qOut)
{
    const double qc = cphi * hcur;
    pOut = (qc + a.a * t) / hnext;
    const double qn = (a.stage == 1 ? qc : qnIn) + a.b * t;
    qOut = a.stage == 4 ? qn / hnext : qn;
}

// Generic form: LPC lanes span a column, one cell per lane group, index records; any K, any maxEdges (the shape of k_nl_cell).
template <int LPC, bool DIFF, bool SRC, bool BIH>
__global__ __launch_bounds__(BLOCK) void k_tracer_cell(const MeshDev m, const TracerArgs a)
{
    constexpr int NG = BLOCK / LPC;
    const int grp = uniform_if_wave<LPC>(threadIdx.x / LPC), l = threadIdx.x % LPC;
    const int K = m.K, ME = m.ME;
    const bool s1 = a.stage == 1, s4 = a.stage == 4;
    for (int c = blockIdx.x * NG + grp; c < m.nC; c += gridDim.x * NG) {
        const double invA = cptr(m.invArea)[c];
        for (int k = l; k < K; k += LPC) {
            const size_t off = (size_t)c * K + k;
            const double hc = a.ph[off], hnext = a.hnext[off], hcur = s4 ? 0.0 : a.hcur[off];
            for (int j0 = 0; j0 < a.nT; j0 += TR_TJ) {
                const int nj = min(TR_TJ, a.nT - j0);
                double t[TR_TJ], pc[TR_TJ], kap[TR_TJ], k4[BIH ? TR_TJ : 1], lc[BIH ? TR_TJ : 1];
#pragma unroll
                for (int jj = 0; jj < TR_TJ; ++jj) {
                    t[jj] = 0.0;
                    pc[jj] = jj < nj ? a.pphi[(size_t)(j0 + jj) * a.stride + off] : 0.0;
                    kap[jj] = DIFF && jj < nj ? cptr(a.kappa)[j0 + jj] : 0.0;
                    if (BIH) {
                        k4[jj] = jj < nj ? cptr(a.kappa4)[j0 + jj] : 0.0;
                        lc[jj] = k4[jj] != 0.0 ? a.lap[(size_t)(j0 + jj) * a.stride + off] : 0.0;
                    }
                }
                for (int i = 0; i < ME; ++i) {
                    const int e = cptr(m.eoc)[(size_t)c * ME + i];
                    if (e < 0 || k >= cptr(m.mltc)[(size_t)c * ME + i]) continue;
                    const size_t noff = (size_t)cptr(m.coc)[(size_t)c * ME + i] * K + k;
                    const double hE = 0.5 * (hc + a.ph[noff]);
                    const double F = a.pu[(size_t)e * K + k] * hE;
                    const double sd = cptr(m.sdv)[(size_t)c * ME + i];
                    const double dd = DIFF ? cptr(a.dvdc)[(size_t)c * ME + i] : 0.0;
#pragma unroll
                    for (int jj = 0; jj < TR_TJ; ++jj)
                        if (jj < nj) {
                            const double pn = a.pphi[(size_t)(j0 + jj) * a.stride + noff];
                            const double pE = 0.5 * (pc[jj] + pn);
                            t[jj] += ((F * pE) * sd) * invA;
                            if (DIFF) t[jj] += (((kap[jj] * hE) * (pn - pc[jj])) * dd) * invA;
                            if (BIH)
                                if (k4[jj] != 0.0)
                                    t[jj] -= (((k4[jj] * hE) * (a.lap[(size_t)(j0 + jj) * a.stride + noff] - lc[jj])) * dd) * invA;
                        }
                }
#pragma unroll
                for (int jj = 0; jj < TR_TJ; ++jj)
                    if (jj < nj) {
                        const size_t joff = (size_t)(j0 + jj) * a.stride + off;
                        const double cphi = s1 ? pc[jj] : s4 ? 0.0 : a.cphi[joff];
                        double pOut, qOut;
                        if (SRC)
                            if (const double *q = a.src[j0 + jj]) t[jj] += q[off];
                        tracer_update(a, t[jj], cphi, hcur, hnext, s1 ? 0.0 : a.qn[joff], pOut, qOut);
                        if (!s4) a.pphi_out[joff] = pOut;
                        a.qn[joff] = qOut;
                    }
            }
        }
    }
}

// Patch form (tracer_patch.hpp: the workgroup shape, the LDS layout, the row cache): the patch's records and the ph and pphi rows of its
// own cells are staged in LDS in one phase.  `chunk` tracers' rows are resident at a time: a state with more takes further passes over the
// patch (the pphi rows re-staged, F re-formed once per pass).
// DIFF: the patch's dvdc entries are staged beside sdv, and a cell keeps hE of its slots beside F.  SRC: one more own-row load per
// sourced tracer, not staged (the LDS layout and the chunking do not know about sources).  BIH: a resident tracer takes a second row
// set, for L (row set 1 + chunk + jj), staged and gathered as pphi is -- for the tracers with kappa4 != 0 only.
template <int ME_, bool DIFF, bool SRC, bool BIH>
__global__ __launch_bounds__(TR_NT, 2) void k_tracer_patch(const MeshDev m, const TracerArgs a, const int chunk)
{
    static_assert(ME_ == 6, "burst width");
    static_assert(DIFF || !BIH, "BIH instantiates only together with DIFF");
    extern __shared__ __align__(16) unsigned char tr_smem[];
    const int pl_ = patch_of_block(m.nPatches);
    if (pl_ >= m.nPatches) return;
    const TracerPatch P = tracer_patch_open<ME_>(m, tr_smem, pl_, 1 + (BIH ? 2 : 1) * chunk, true, DIFF);
    const bool s1 = a.stage == 1, s4 = a.stage == 4;
    const glb_bytes_t uG = (glb_bytes_t)a.pu;

    // the rows of a pass: ph (rb == 0) and pphi of its cj tracers, then the L rows of those with kappa4 != 0
    auto stage_rows = [&](int rb, int j0, int cj) {
        tracer_stage_rows(P, rb, cj, a.ph, a.pphi + (size_t)j0 * a.stride, a.stride);
        if constexpr (BIH)
            for (int jj = 0; jj < cj; ++jj)
                if (a.kappa4[j0 + jj] != 0.0) tracer_stage_set(P, 1 + chunk + jj, a.lap + (size_t)(j0 + jj) * a.stride);
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
            double2 F[ME_], hE[DIFF ? ME_ : 1];
            bool ch[ME_], okx[ME_], oky[ME_];
            uint32_t aoff[ME_], gh[ME_];
            double2 uu[ME_], hh[ME_];
#pragma unroll
            for (int i = 0; i < ME_; ++i) uu[i] = glb_row2(uG + (rec[i] + P.lo));
            tracer_slots<ME_>(P, rec, ch, aoff, gh);
            tracer_gather<ME_>(P, 0, a.ph, ch, aoff, gh, hh);
            tracer_level_masks<ME_>(P, ci, rec[2 * ME_], okx, oky);
            const double2 hc = tracer_own_row(P, 0, ci);
#pragma unroll
            for (int i = 0; i < ME_; ++i) {
                const double2 he = make_double2(0.5 * (hc.x + hh[i].x), 0.5 * (hc.y + hh[i].y));
                F[i] = make_double2(uu[i].x * he.x, uu[i].y * he.y);   // Operators.jl:217, DiagnosticVars.jl:165
                if constexpr (DIFF) hE[i] = he;
            }
            const double *sd = P.sd + ci * ME_, *dd = P.dd + ci * ME_;
            const double invA = P.ia[ci];
            const unsigned orow = P.ownB + (unsigned)ci * P.rowB + P.lo;       // the cell's own row in every (K, nC) array
            const double2 hnext = gload2(a.hnext, orow);
            const double2 hcur = s1 ? hc : s4 ? make_double2(0.0, 0.0) : gload2(a.hcur, orow);
            for (int jj = 0; jj < cj; ++jj) {
                const size_t jo = (size_t)(j0 + jj) * a.stride;
                const double kap = DIFF ? a.kappa[j0 + jj] : 0.0;
                double2 pp[ME_];
                tracer_gather<ME_>(P, 1 + jj, a.pphi + jo, ch, aoff, gh, pp);
                const double2 pc = tracer_own_row(P, 1 + jj, ci);
                double2 t = make_double2(0.0, 0.0);
                const double kap4 = BIH ? a.kappa4[j0 + jj] : 0.0;
                const bool b4 = BIH && kap4 != 0.0;             // wave-uniform
                double2 ll[BIH ? ME_ : 1], lc = make_double2(0.0, 0.0);
                if constexpr (BIH) {
#pragma unroll
                    for (int i = 0; i < ME_; ++i) ll[i] = make_double2(0.0, 0.0);
                    if (b4) {                                   // L gathered as pphi is, from its own row set
                        tracer_gather<ME_>(P, 1 + chunk + jj, a.lap + jo, ch, aoff, gh, ll);
                        lc = tracer_own_row(P, 1 + chunk + jj, ci);
                    }
                }
#pragma unroll
                for (int i = 0; i < ME_; ++i) {
                    const double ex = 0.5 * (pc.x + pp[i].x), ey = 0.5 * (pc.y + pp[i].y);
                    double tx = t.x + ((F[i].x * ex) * sd[i]) * invA, ty = t.y + ((F[i].y * ey) * sd[i]) * invA;
                    if constexpr (DIFF) {
                        tx += (((kap * hE[i].x) * (pp[i].x - pc.x)) * dd[i]) * invA;
                        ty += (((kap * hE[i].y) * (pp[i].y - pc.y)) * dd[i]) * invA;
                    }
                    if constexpr (BIH)
                        if (b4) {
                            tx -= (((kap4 * hE[i].x) * (ll[i].x - lc.x)) * dd[i]) * invA;
                            ty -= (((kap4 * hE[i].y) * (ll[i].y - lc.y)) * dd[i]) * invA;
                        }
                    t.x = okx[i] ? tx : t.x;
                    t.y = oky[i] ? ty : t.y;
                }
                const double2 cphi = s1 ? pc : s4 ? make_double2(0.0, 0.0) : gload2(a.cphi + jo, orow);
                const double2 qnIn = s1 ? make_double2(0.0, 0.0) : gload2(a.qn + jo, orow);
                double2 pOut, qOut;
                if (SRC)
                    if (const double *q = a.src[j0 + jj]) {
                        const double2 qq = gload2(q, orow);
                        t.x += qq.x;
                        t.y += qq.y;
                    }
                tracer_update(a, t.x, cphi.x, hcur.x, hnext.x, qnIn.x, pOut.x, qOut.x);
                tracer_update(a, t.y, cphi.y, hcur.y, hnext.y, qnIn.y, pOut.y, qOut.y);
                if (!s4) gstore2(a.pphi_out + jo, orow, pOut);
                gstore2(a.qn + jo, orow, qOut);
            }
        }
    }
}

TracerKernel tracer_kernel(const MeshDev &m, int lpc, int nT, bool generic, bool diff, bool bih)
{
    if (!generic && lpc == 64 && m.K >= 34 && m.K <= 64 && !(m.K & 1) && m.ME == 6 && m.cRec && m.maxOwnC > 0) {
        // as many tracers' rows resident as 80 KB hold (two workgroups per CU), at least one; with bih a resident tracer takes two row
        // sets (pphi and L), so half as many fit, and the generic form serves when not even one tracer's two sets do
        const size_t budget = 80 * 1024, fixed = tracer_patch_lds(m, 0, diff, bih), perT = (size_t)m.maxOwnC * m.K * 8 * (bih ? 2 : 1);
        if (fixed + perT <= budget) {
            const int chunk = (int)std::min<size_t>((size_t)std::max(nT, 1), (budget - fixed) / perT);
            return {1, tracer_patch_lds(m, chunk, diff, bih), chunk};
        }
    }
    return {2, 0, 0};
}

template <bool DIFF, bool SRC, bool BIH>
static hipError_t launch_tracer_generic(const MeshDev &m, const TracerArgs &a, int lpc, hipStream_t s)
{
#define CALL(L) launch_tracer_cell_form(k_tracer_cell<L, DIFF, SRC, BIH>, L, m, a, s)
    DISPATCH_LPC(lpc, CALL)
#undef CALL
}

hipError_t launch_tracers(const MeshDev &m, const TracerArgs &a, int lpc, bool generic, hipStream_t s)
{
    if (a.nT <= 0) return hipSuccess;
    const bool diff = a.kappa != nullptr;       // (then a.dvdc is set too: tracer_stage)
    const bool src = a.src != nullptr;          // (some tracer of the state has a source: tracer_stage)
    const bool bih = a.kappa4 != nullptr;       // (then a.lap, a.kappa and a.dvdc are set too: tracer_stage)
    const TracerKernel k = tracer_kernel(m, lpc, a.nT, generic, diff, bih);
    return pick_tracer_instance(diff, src, bih, [&](auto D, auto S, auto B) {
        if (k.form == 1) return launch_tracer_patch_form(k_tracer_patch<6, D.value, S.value, B.value>, m, a, k, s);
        return launch_tracer_generic<D.value, S.value, B.value>(m, a, lpc, s);
    });
}

// ------------------------------------------------------------------------------------------------
// The Laplacian pass (TracerLapArgs, kernels.hpp): out_j = Lap(ph, x_j) for every field with kappa4[j] != 0, one launch.  One kernel
// with two callers: the forward step hands it (ph_s, pphi), the reverse sweep (ph_s, y).  It does not read u.
// ------------------------------------------------------------------------------------------------
// Generic form: k_tracer_cell's shape.
template <int LPC>
__global__ __launch_bounds__(BLOCK) void k_tracer_lap_cell(const MeshDev m, const TracerLapArgs a)
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
                double s[TR_TJ], xc[TR_TJ];
                bool on[TR_TJ];
                bool any = false;
#pragma unroll
                for (int jj = 0; jj < TR_TJ; ++jj) {
                    on[jj] = jj < nj && cptr(a.kappa4)[j0 + jj] != 0.0;      // wave-uniform
                    any = any || on[jj];
                    s[jj] = 0.0;
                    xc[jj] = on[jj] ? a.x[(size_t)(j0 + jj) * a.stride + off] : 0.0;
                }
                if (!any) continue;
                for (int i = 0; i < ME; ++i) {
                    const int e = cptr(m.eoc)[(size_t)c * ME + i];
                    if (e < 0 || k >= cptr(m.mltc)[(size_t)c * ME + i]) continue;
                    const size_t noff = (size_t)cptr(m.coc)[(size_t)c * ME + i] * K + k;
                    const double hE = 0.5 * (hc + a.ph[noff]);
                    const double dd = cptr(a.dvdc)[(size_t)c * ME + i];
#pragma unroll
                    for (int jj = 0; jj < TR_TJ; ++jj)
                        if (on[jj]) s[jj] += (hE * (a.x[(size_t)(j0 + jj) * a.stride + noff] - xc[jj])) * dd;
                }
#pragma unroll
                for (int jj = 0; jj < TR_TJ; ++jj)
                    if (on[jj]) a.out[(size_t)(j0 + jj) * a.stride + off] = (s[jj] * invA) / hc;
            }
        }
    }
}

// Patch form: k_tracer_patch's shape and LDS layout (tracer_patch.hpp) with dvdc where that one keeps sdv -- the patch's cRec records, dvdc,
// invArea and maxLevelEdgeTop entries, the ph rows and the x rows of `chunk` fields of its own cells in LDS; neighbours' rows in one burst,
// foreign rows by masked global loads at 32-bit byte offsets.  Fields with kappa4 == 0 are not staged, not gathered, not written.
template <int ME_>
__global__ __launch_bounds__(TR_NT, 2) void k_tracer_lap_patch(const MeshDev m, const TracerLapArgs a, const int chunk)
{
    static_assert(ME_ == 6, "burst width");
    extern __shared__ __align__(16) unsigned char trl_smem[];
    const int pl_ = patch_of_block(m.nPatches);
    if (pl_ >= m.nPatches) return;
    const TracerPatch P = tracer_patch_open<ME_>(m, trl_smem, pl_, 1 + chunk, false, true);
    const int tid = P.tid, c0 = P.c0, nc = P.nc;

    auto stage_fields = [&](int j0, int cj) {
        for (int jj = 0; jj < cj; ++jj)
            if (a.kappa4[j0 + jj] != 0.0) tracer_stage_set(P, 1 + jj, a.x + (size_t)(j0 + jj) * a.stride);
    };

    {
        const int nRec = nc * P.CI, nSd = nc * ME_;
        tracer_stage_set(P, 0, a.ph);
        stage_fields(0, min(chunk, a.nT));
        for (int i = tid; i < nRec; i += TR_NT) P.rec[i] = m.cRec[(size_t)c0 * P.CI + i];
        for (int i = tid; i < nSd; i += TR_NT) { P.dd[i] = a.dvdc[(size_t)c0 * ME_ + i]; P.ml[i] = m.mltc[(size_t)c0 * ME_ + i]; }
        for (int i = tid; i < nc; i += TR_NT) P.ia[i] = m.invArea[c0 + i];
    }
    for (int j0 = 0; j0 < a.nT; j0 += chunk) {
        const int cj = min(chunk, a.nT - j0);
        if (j0 > 0) {
            __syncthreads();                      // the previous pass has read its rows
            stage_fields(j0, cj);
        }
        __syncthreads();
        if (!P.act) continue;
        for (int ci = P.grp; ci < nc; ci += TR_NG) {
            const uint32_t *rec = P.rec + (size_t)ci * P.CI;
            double2 hE[ME_];
            bool ch[ME_], okx[ME_], oky[ME_];
            uint32_t aoff[ME_], gh[ME_];
            const double2 hc = tracer_own_row(P, 0, ci);
            {
                double2 hh[ME_];
                tracer_slots<ME_>(P, rec, ch, aoff, gh);
                tracer_gather<ME_>(P, 0, a.ph, ch, aoff, gh, hh);
                tracer_level_masks<ME_>(P, ci, rec[2 * ME_], okx, oky);
#pragma unroll
                for (int i = 0; i < ME_; ++i) hE[i] = make_double2(0.5 * (hc.x + hh[i].x), 0.5 * (hc.y + hh[i].y));
            }
            const double *dd = P.dd + ci * ME_;
            const double invA = P.ia[ci];
            const unsigned orow = P.ownB + (unsigned)ci * P.rowB + P.lo;       // the cell's own row in every (K, nC) array
            for (int jj = 0; jj < cj; ++jj) {
                if (a.kappa4[j0 + jj] == 0.0) continue;                  // wave-uniform
                const size_t jo = (size_t)(j0 + jj) * a.stride;
                double2 xx[ME_];
                tracer_gather<ME_>(P, 1 + jj, a.x + jo, ch, aoff, gh, xx);
                const double2 xc = tracer_own_row(P, 1 + jj, ci);
                double2 s = make_double2(0.0, 0.0);
#pragma unroll
                for (int i = 0; i < ME_; ++i) {
                    const double sx = s.x + (hE[i].x * (xx[i].x - xc.x)) * dd[i], sy = s.y + (hE[i].y * (xx[i].y - xc.y)) * dd[i];
                    s.x = okx[i] ? sx : s.x;
                    s.y = oky[i] ? sy : s.y;
                }
                gstore2(a.out + jo, orow, make_double2((s.x * invA) / hc.x, (s.y * invA) / hc.y));
            }
        }
    }
}

hipError_t launch_tracer_lap(const MeshDev &m, const TracerLapArgs &a, int lpc, bool generic, hipStream_t s)
{
    if (a.nT <= 0) return hipSuccess;
    // k_tracer_patch's layout without the harmonic extras (dvdc takes the place of sdv): the size and the chunk of the plain tracer kernel
    const TracerKernel k = tracer_kernel(m, lpc, a.nT, generic, false, false);
    if (k.form == 1) return launch_tracer_patch_form(k_tracer_lap_patch<6>, m, a, k, s);
#define CALL(L) launch_tracer_cell_form(k_tracer_lap_cell<L>, L, m, a, s)
    DISPATCH_LPC(lpc, CALL)
#undef CALL
}

}  // namespace moka
