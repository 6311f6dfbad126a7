// api_state.hip -- C ABI, continued: the state, the lazily pending arrays, the Forward-Euler and RK4 steps, the momentum setters.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <climits>
#include <cstdint>
#include <mutex>
#include <new>
#include <string>
#include <unordered_set>
#include <utility>
#include <vector>

#include "kernels_common.hpp"
#include "state.hpp"
#include "tapes.hpp"

namespace mk {

static std::mutex g_liveMutex;
static std::unordered_set<const moka_state *> g_liveStates;
void state_attach(moka_state *st, bool halo)
{
    std::lock_guard<std::mutex> lk(g_liveMutex);
    if (g_liveStates.count(st)) { ++st->attached; st->halos += halo; }
}
bool state_detach(moka_state *st, bool halo)
{
    std::lock_guard<std::mutex> lk(g_liveMutex);
    const bool alive = g_liveStates.count(st) != 0;
    if (alive) { --st->attached; st->halos -= halo; }
    return alive;
}

int ensure_rk_bufs(moka_state *st)
{
    if (st->rk[1].ssh) return MOKA_OK;       // the last of the six: set only when all of them exist
    const Plan &p = st->mesh->plan;
    LevelBufs tmp[2];
    const size_t mark = st->mem.mark();
    const size_t sb = st->f32 ? 4 : 8;
    int rc = MOKA_OK;
    for (auto &r : tmp) {
        if (rc == MOKA_OK) rc = st->mem.alloc(&r.u, (size_t)p.K * p.nE, sb);
        if (rc == MOKA_OK) rc = st->mem.alloc(&r.h, (size_t)p.K * p.nC, sb);
        if (rc == MOKA_OK) rc = st->mem.alloc(&r.ssh, (size_t)p.nC, sb);
    }
    // the code arrays of the stage 1 -> 2 hand-off (rk_handoff_usable) come with them, behind them: Float64 states only
    signed char *codeU = nullptr, *codeH = nullptr;
    if (!st->f32) {
        if (rc == MOKA_OK) rc = st->mem.alloc(&codeU, (size_t)p.K * p.nE);
        if (rc == MOKA_OK) rc = st->mem.alloc(&codeH, (size_t)p.K * p.nC);
    }
    if (rc != MOKA_OK) {                     // free what a partial failure left behind: a later call starts over
        st->mem.rollback(mark);
        return rc;
    }
    st->hoCodeU = codeU; st->hoCodeH = codeH;
    st->rk[0] = tmp[0]; st->rk[1] = tmp[1];
    st->phys[2] = tmp[0]; st->phys[3] = tmp[1];
    return MOKA_OK;
}

int ensure_spare(moka_state *st)
{
    if (st->spare.ssh) return MOKA_OK;
    const Plan &p = st->mesh->plan;
    LevelBufs tmp;
    const size_t mark = st->mem.mark();
    const size_t sb = st->f32 ? 4 : 8;
    int rc = st->mem.alloc(&tmp.u, (size_t)p.K * p.nE, sb);
    if (rc == MOKA_OK) rc = st->mem.alloc(&tmp.h, (size_t)p.K * p.nC, sb);
    if (rc == MOKA_OK) rc = st->mem.alloc(&tmp.ssh, (size_t)p.nC, sb);
    if (rc != MOKA_OK) {
        st->mem.rollback(mark);
        return rc;
    }
    st->spare = tmp;
    st->phys[4] = tmp;
    return MOKA_OK;
}

// Where a Forward-Euler step writes its new level: the spare set when it exists (the step may then read the previous level
// while it runs), else the previous level's buffers (which the new level replaces anyway).
LevelBufs &fe_new_level(moka_state *st) { return st->spare.ssh ? st->spare : st->lev[0]; }

// prev <- cur <- new (<- old prev becomes the spare).  Without a spare set: the plain swap.
void fe_rotate_levels(moka_state *st)
{
    if (st->spare.ssh) {
        const LevelBufs oldPrev = st->lev[0];
        st->lev[0] = st->lev[1];
        st->lev[1] = st->spare;
        st->spare = oldPrev;
    } else {
        std::swap(st->lev[0], st->lev[1]);
    }
}

struct FieldRef {
    double *ptr;
    int kind;     // MOKA_CELL / EDGE / VERTEX
    int64_t n;
    int K;
    bool f32 = false;   // ptr is a float array (prognostic field of an fp32-storage state)
};

int field_ref(moka_state *st, int field, int level, FieldRef *r)
{
    const Plan &p = st->mesh->plan;
    if (level != 0 && level != 1) return fail(st->ctx, MOKA_ERR_ARG, "time_level must be 0 (previous) or 1 (current)");
    switch (field) {
        case MOKA_F_SSH: *r = {st->lev[level].ssh, MOKA_CELL, p.nC, 1}; break;
        case MOKA_F_NORMAL_VELOCITY: *r = {st->lev[level].u, MOKA_EDGE, p.nE, p.K}; break;
        case MOKA_F_LAYER_THICKNESS: *r = {st->lev[level].h, MOKA_CELL, p.nC, p.K}; break;
        case MOKA_F_LAYER_THICKNESS_EDGE: *r = {st->hEdge[0], MOKA_EDGE, p.nE, p.K}; break;
        case MOKA_F_THICKNESS_FLUX: *r = {st->F, MOKA_EDGE, p.nE, p.K}; break;
        case MOKA_F_VELOCITY_DIV_CELL: *r = {st->div, MOKA_CELL, p.nC, p.K}; break;
        case MOKA_F_RELATIVE_VORTICITY: *r = {st->vort, MOKA_VERTEX, p.nV, p.K}; break;
        case MOKA_F_TEND_NORMAL_VELOCITY: *r = {st->tendU, MOKA_EDGE, p.nE, p.K}; break;
        case MOKA_F_TEND_LAYER_THICKNESS: *r = {st->tendH, MOKA_CELL, p.nC, p.K}; break;
        default: return fail(st->ctx, MOKA_ERR_ARG, "unknown field id");
    }
    r->f32 = st->f32;     // every field of an fp32-storage state is a float array
    if (!r->ptr) return fail(st->ctx, MOKA_ERR_ARG, "field not allocated");
    return MOKA_OK;
}

int nlev_of(const moka_state *st, int flags) { return (flags & MOKA_FE_LEVEL1_ONLY) ? 1 : st->mesh->plan.K; }

FeArgs fe_args(moka_state *st, int ops, int flags, double dt)
{
    FeArgs a{};
    a.ops = ops;
    a.flags = flags;
    a.nlev = nlev_of(st, flags);
    a.dt = dt;
    a.u = st->lev[1].u; a.h = st->lev[1].h; a.ssh = st->lev[1].ssh;
    a.hEdgeOld = st->hEdge[0]; a.hEdgeNew = st->hEdge[1];
    a.Fin = st->F; a.F = st->F; a.div = st->div; a.vort = st->vort;
    a.tendU = st->tendU; a.tendH = st->tendH;
    const LevelBufs &nw = fe_new_level(st);
    a.u_new = nw.u; a.h_new = nw.h; a.ssh_new = nw.ssh;
    return a;
}

// One fused tendency / RK-stage launch over patches [pBegin, pBegin + pCount) (default: all) on the compute stream (or `on`).
// variant 0 (auto): k_stage_rec2c, then rec2 / rec / col / generic as the mesh allows; fp32-storage and nonlinear states have
// their own kernels.
hipError_t run_stage(moka_state *st, const StageArgs &g_in, int pBegin, int pCount, hipStream_t on, int tail)
{
    const StageArgs &g = g_in;
    const moka_mesh *m = st->mesh;
    MeshDev dev = m->dev;                 // the launch covers patches [pBegin, pBegin + pCount) (+ the patch `tail`)
    dev.tailPatch = -1;
    hipStream_t s = on ? on : st->ctx->stream;
    if (tail >= 0) {
        // One extra, non-adjacent patch in the same launch: only the default kernels can carry it.  Anything else
        // (explicit variants, fallbacks for other K, the nonlinear path) gets a launch of its own for it.
        hipError_t e = hipErrorNotSupported;
        if (pCount > 0 && !st->nonlinear && (st->f32 || default_stage_kernels(st))) {
            const moka::Plan &p = m->plan;
            dev.patchBegin = pBegin; dev.nPatches = pCount; dev.tailPatch = tail;
            int mE = p.patchEdgeStart[tail + 1] - p.patchEdgeStart[tail], mC = p.patchCellStart[tail + 1] - p.patchCellStart[tail];
            for (int q = pBegin; q < pBegin + pCount; ++q) {
                mE = std::max(mE, p.patchEdgeStart[q + 1] - p.patchEdgeStart[q]);
                mC = std::max(mC, p.patchCellStart[q + 1] - p.patchCellStart[q]);
            }
            dev.maxOwnE = mE; dev.maxOwnC = mC;
            e = st->f32 ? launch_stage_rec2c_f32(dev, g, s) : launch_stage_rec2c(dev, g, s);
        }
        if (e != hipErrorNotSupported) return e;
        e = run_stage(st, g_in, pBegin, pCount, on);
        return e != hipSuccess ? e : run_stage(st, g_in, tail, 1, on);
    }
    if (pCount >= 0) {
        dev.patchBegin = pBegin; dev.nPatches = pCount;
        if (pCount > 0) {
            auto &cache = st->mesh->rangeMax;
            auto it = cache.find({pBegin, pCount});
            if (it == cache.end()) {
                const moka::Plan &p = m->plan;
                int mE = 1, mC = 1;
                for (int q = pBegin; q < pBegin + pCount; ++q) {
                    mE = std::max(mE, p.patchEdgeStart[q + 1] - p.patchEdgeStart[q]);
                    mC = std::max(mC, p.patchCellStart[q + 1] - p.patchCellStart[q]);
                }
                it = cache.emplace(std::make_pair(pBegin, pCount), std::make_pair(mE, mC)).first;
            }
            dev.maxOwnE = it->second.first; dev.maxOwnC = it->second.second;
        }
    }
    if (dev.nPatches <= 0) return hipSuccess;
    if ((g.codeU || g.codeH) && (st->nonlinear || st->f32)) return hipErrorNotSupported;   // (rk_handoff_usable saw to it)
    if (st->nonlinear) {
        // vector-invariant form: potential vorticity at vertices -> edges, kinetic energy at cells, thickness flux at edges
        // (whole mesh: the stencil of the edge pass reaches two cells deep), then the generic stage kernel's nonlinear twin
        const bool del2 = st->viscDel2 != 0.0, del4 = st->viscDel4 != 0.0;
        NlArgs nl{st->nlQv, st->nlQe, st->nlKe, del2 ? st->nlZv : nullptr, del2 ? st->nlDiv : nullptr, st->viscDel2};
        const int form = nl_form(st->ctx);          // tests run every form against the oracle
        // a patch range (partitioned meshes: moka_rk4_dist_stage) is served by the patch forms only
        if (pCount >= 0 && !nl_patch_forms(dev, m->lpc, form)) return hipErrorNotSupported;
        // Del4: whole-mesh stages only (its stencil reaches three cell rings; moka_halo_create refuses such states)
        if (del4 && (pCount >= 0 || st->nlPhase != 0)) return hipErrorNotSupported;
        if (st->nlPhase != 2) {
            NlArgs np = nl;                       // Del4 needs velocityDivCell / relativeVorticity even without Del2
            if (del4) { np.zv = st->nlZv; np.divc = st->nlDiv; }
            hipError_t e = launch_nl_prepare(dev, g.pu, g.ph, np, m->lpc, form, s);
            if (e != hipSuccess) return e;
        }
        if (st->nlPhase == 1) return hipSuccess;
        if (del4) {                               // div4 / curl4 of L(u), then the stage kernels' Del4 instances
            const int path = del4_path(dev, m->d4, m->lpc, form);
            hipError_t e = launch_del4(dev, m->d4, st->nlDiv, st->nlZv, st->nlDiv4, st->nlCurl4, path, s);
            if (e != hipSuccess) return e;
            st->del4Path = path;
            nl.div4 = st->nlDiv4; nl.curl4 = st->nlCurl4; nl.coef4 = st->coef4;
        }
        return launch_stage_nl(dev, g, nl, m->lpc, m->plan.ldsOk, form, s);
    }
    if (st->f32) {   // the one fp32-storage kernel (checked at state creation against the patches that are ever launched)
        if (pCount < 0 && m->plan.nPatchesLaunch < m->plan.nPatches) {
            // whole-mesh launch on a partitioned mesh: the halo-only patches are skipped (their rows arrive by exchange)
            dev = launch_bounds(m);
            dev.tailPatch = -1; dev.nPatches = m->plan.nPatchesLaunch;
        }
        return launch_stage_rec2c_f32(dev, g, s);
    }
    const int v = st->ctx->variant;
    // 0 = auto: rec2c (even 34 <= K <= 64, patches whose records + own rows fit the LDS), else the plain column kernel (K >= 33),
    // else the generic index kernel.  11 rec2c, 4 column, 3 generic.  (The other execution shapes measured in rounds 1-3 -- pipelined
    // and 16-byte-lane column kernels, LDS-tiled and LDS-DMA forms, persistent double-buffered tiles -- lost and are gone; their
    // numbers are in profiles/r01_variants.txt ... r03_variants.txt.)
    if (default_stage_kernels(st)) {                          // default: 16-byte lanes + own-edge u rows cached in LDS
        hipError_t e = launch_stage_rec2c(dev, g, s);
        if (e != hipErrorNotSupported) return e;
    }
    if (g.codeU || g.codeH) return hipErrorNotSupported;      // the hand-off exists in that kernel only (rk_handoff_usable saw to it)
    if (v != 3 && m->lpc == 64 && m->colOk) return launch_stage_col(dev, g, s);
    return launch_stage(dev, g, m->lpc, s);
}

// Forward-Euler step in the stage kernels (k_stage_rec2c* modes 4 / 5 / 6): all levels, the default kernel choice, a mesh the
// kernels can carry.  (MOKA_FE_LEVEL1_ONLY, odd or large K, explicit kernel variants take the generic one-launch kernel k_fe.)
bool fe_stage_path(const moka_state *st, int flags)
{
    const moka_mesh *mm = st->mesh;
    if (flags & MOKA_FE_LEVEL1_ONLY) return false;
    if (st->f32) return true;                                  // checked when the state was created
    return default_stage_kernels(st) && rec2c_supported(launch_bounds(mm));
}

// A LEAN step stores the new level and relativeVorticity only (moka_state.feLazy).  It needs the stage-kernel path, the spare
// level set, and -- with the reference's stale flux thickness -- that thickness to be derivable from the previous level.
bool fe_lean(const moka_state *st, int flags)
{
    return tuning(TUNE_FE_LEAN) && !st->feForceEager && fe_stage_path(st, flags) && st->spare.ssh &&
           (!(flags & MOKA_FE_STALE_HEDGE) || (st->hEdgePrev && tuning(TUNE_FE_PREV)));
}

// What a Forward-Euler step does about lazily pending arrays before its first launch.  A lean step reads none of them and
// supersedes them -- except relativeVorticity when it accumulates onto a value an RK4 step left pending; anything else needs
// them in memory.  Idempotent: the parts of a distributed step all call it.
int fe_begin(moka_state *st, int flags)
{
    // an fp32-storage state after an RK4 step has no current DiagnosticVars: a step that carries none over (flags 0) may follow
    if (st->f32 && st->diagDirty && !(flags & (MOKA_FE_STALE_HEDGE | MOKA_FE_ACCUM_VORT))) st->diagDirty = false;
    if (fe_lean(st, flags) && !(st->diagDirty && (flags & MOKA_FE_ACCUM_VORT))) {
        st->diagDirty = st->tendDirty = false;
        st->lazyPu = st->lazyPh = nullptr; st->lazyOwner = nullptr;
        return MOKA_OK;
    }
    return flush_lazy(st, true, true);
}

void fe_end(moka_state *st, int flags, bool stageKernel, bool lean, bool prevMode)
{
    fe_rotate_levels(st);
    if (!lean) std::swap(st->hEdge[0], st->hEdge[1]);          // a lean step has not written layerThicknessEdge
    st->feFast = stageKernel ? (prevMode ? 2 : 1) : 0;
    st->feLazy = lean;
    st->feLazyCount = -1;              // (a distributed step with a direct halo narrows it: moka_fe_dist_end)
    st->feLazyStale = lean && (flags & MOKA_FE_STALE_HEDGE);
    // the stage kernel interpolated (or, lean, will interpolate) layerThicknessEdge of every computed edge from the level that is
    // the previous one now: the next step may form the reference's stale flux thickness from that level (mode 6)
    st->hEdgePrev = stageKernel;
}

// Argument block of a Forward-Euler launch of the stage kernels from the generic kernel's.  MOKA_FE_STALE_HEDGE: the stored
// layerThicknessEdge is gathered (mode 4) unless it is known to be the interpolation of the previous level's layerThickness and
// that level survives the step (the spare set takes the new level): then it is formed from those rows (mode 6).  A lean step
// passes no TendencyVars / DiagnosticVars outputs.
StageArgs fe_stage_args(moka_state *st, const FeArgs &a, int flags)
{
    StageArgs s{};
    s.pu = a.u; s.ph = a.h; s.ssh = a.ssh;
    s.pu_out = a.u_new; s.ph_out = a.h_new; s.ssh_out = a.ssh_new;
    s.a = a.dt;
    const bool stale = flags & MOKA_FE_STALE_HEDGE;
    const bool prev = stale && st->hEdgePrev && st->spare.ssh && a.h_new != st->lev[0].h && tuning(TUNE_FE_PREV);
    s.hEdgeOld = stale && !prev ? a.hEdgeOld : nullptr;
    s.hPrev = prev ? st->lev[0].h : nullptr;
    s.feMode = prev ? 6 : stale ? 4 : 5;
    s.areaCell = st->mesh->dev.areaCell;
    if (!fe_lean(st, flags)) {
        s.tendU = a.tendU; s.tendH = a.tendH;
        s.hEdgeNew = a.hEdgeNew; s.F = a.F; s.div = a.div;
    }
    // relativeVorticity by the same launch (the vertices of the launched patches) where the stage kernels can carry it
    if (stage_curl_fits(launch_bounds(st->mesh), st->f32)) { s.vort = a.vort; s.accumVort = (flags & MOKA_FE_ACCUM_VORT) ? 1 : 0; }
    return s;
}

// The arrays a lean Forward-Euler step left pending (moka_state.feLazy), produced now: the same launch over the same patches
// with the new-level outputs switched off and the diagnostic outputs on, from the level the step started from (the previous
// one now) and, for the stale flux thickness, the level before it (`spare`).
static int materialize_fe(moka_state *st)
{
    const moka_mesh *mm = st->mesh;
    StageArgs g{};
    g.pu = st->lev[0].u; g.ph = st->lev[0].h; g.ssh = st->lev[0].ssh;
    g.feMode = st->feLazyStale ? 6 : 5;
    g.hPrev = st->feLazyStale ? st->spare.h : nullptr;
    g.tendU = st->tendU; g.tendH = st->tendH; g.F = st->F; g.div = st->div;
    g.hEdgeNew = st->hEdge[0];                                  // mode 6 reads no stored layerThicknessEdge: written in place
    g.areaCell = mm->dev.areaCell;
    MeshDev dev = launch_bounds(mm);
    dev.tailPatch = -1;
    dev.patchBegin = 0; dev.nPatches = mm->plan.nPatchesLaunch;
    if (st->feLazyCount >= 0) {                                 // a distributed step with a direct halo: the interior patches only
        dev.patchBegin = st->feLazyBegin; dev.nPatches = st->feLazyCount;
    }
    if (dev.nPatches > 0)
        HIPCHK(st->ctx, st->f32 ? launch_stage_rec2c_f32(dev, g, st->ctx->stream) : launch_stage_rec2c(dev, g, st->ctx->stream));
    st->feLazy = false;
    st->feLazyCount = -1;
    return MOKA_OK;
}

int flush_lazy(moka_state *st, bool diag, bool tend)
{
    if ((diag || tend) && st->feLazy)
        if (int rc = materialize_fe(st)) return rc;
    if (diag && st->diagDirty && st->f32)   // no diagnostics-only kernel for float arrays: they come out of Forward-Euler steps
        return fail(st->ctx, MOKA_ERR_UNSUPPORTED,
                    "fp32-storage state: DiagnosticVars exist after Forward-Euler steps only (not after RK4 steps or uploads)");
    if (diag && st->diagDirty) {
        // clean diagnostics of the current state: hEdge = interp(h); F = u*hEdge; div; vort zeroed + curl
        FeArgs a = fe_args(st, FE_FLUX | FE_DIV | FE_CURL | FE_HEDGE, 0, 0.0);
        a.nlev = st->mesh->plan.K;
        HIPCHK(st->ctx, launch_fe(st->mesh->dev, a, st->mesh->lpc, st->ctx->stream));
        std::swap(st->hEdge[0], st->hEdge[1]);
        st->diagDirty = false;
        st->hEdgePrev = false;            // layerThicknessEdge now belongs to the CURRENT level
    }
    if (tend && st->tendDirty) {
        StageArgs g{};
        g.pu = st->lazyPu ? st->lazyPu : st->rk[0].u; g.ph = st->lazyPh ? st->lazyPh : st->rk[0].h; g.ssh = st->rk[0].ssh;
        g.tendU = st->tendU; g.tendH = st->tendH;
        HIPCHK(st->ctx, run_stage(st, g));
        st->tendDirty = false;
        st->lazyPu = st->lazyPh = nullptr; st->lazyOwner = nullptr;
    }
    return MOKA_OK;
}

bool is_diag_field(int f) { return f >= MOKA_F_LAYER_THICKNESS_EDGE && f <= MOKA_F_RELATIVE_VORTICITY; }
bool is_tend_field(int f) { return f == MOKA_F_TEND_NORMAL_VELOCITY || f == MOKA_F_TEND_LAYER_THICKNESS; }

static int make_ssh_consistent(moka_state *st, double *dst)
{
    const Plan &p = st->mesh->plan;
    if (st->f32)
        HIPCHK(st->ctx, launch_update_ssh_f32(st->mesh->dev, reinterpret_cast<const float *>(st->lev[1].h),
                                              reinterpret_cast<float *>(dst), p.K, st->mesh->lpc, st->ctx->stream));
    else
        HIPCHK(st->ctx, launch_update_ssh(st->mesh->dev, st->lev[1].h, dst, p.K, st->mesh->lpc, st->ctx->stream));
    return MOKA_OK;
}

// Argument block of RK4 stage s (1..4).  A = Curr (current level), B = New accumulator (the previous
// level's buffers, becomes the current level at the end), R1/R2 = provisional states.
StageArgs rk4_stage_args(moka_state *st, int s, double dt, const double *ssh0)
{
    const double a[3] = {dt / 2., dt / 2., dt};                         // time_integration.jl:77
    const double b[4] = {dt / 6., dt / 3., dt / 3., dt / 6.};           // :78
    LevelBufs &A = st->lev[1], &B = st->lev[0], &R1 = st->rk[0], &R2 = st->rk[1];
    StageArgs g{};
    g.nu_out = B.u; g.nh_out = B.h; g.b = b[s - 1];
    if (s == 1) {          // Provis == Curr == A;  New = Curr + b1*k1 -> B;  Provis' = Curr + a1*k1 -> R1
        g.pu = A.u; g.ph = A.h; g.ssh = ssh0;
        g.pu_out = R1.u; g.ph_out = R1.h; g.ssh_out = R1.ssh; g.a = a[0];
        // New as one-byte codes beside B (escapes in B itself): every stage-1 launch of the step, and then its stage-2 launches
        st->hoLive = st->hoRan = rk_handoff_usable(st);
        st->hoRho = a[0] != 0.0 ? b[0] / a[0] : 0.0;
        if (st->hoLive) { g.codeU = st->hoCodeU; g.codeH = st->hoCodeH; g.rho = st->hoRho; }
    } else if (s == 2) {   // Provis = R1 -> R2
        g.pu = R1.u; g.ph = R1.h; g.ssh = R1.ssh; g.cu = A.u; g.ch = A.h; g.nu_in = B.u; g.nh_in = B.h;
        g.pu_out = R2.u; g.ph_out = R2.h; g.ssh_out = R2.ssh; g.a = a[1];
        if (st->hoLive) { g.codeU = st->hoCodeU; g.codeH = st->hoCodeH; g.rho = st->hoRho; }   // what stage 1 of this step stored
    } else if (s == 3) {   // Provis = R2 -> R1
        st->hoLive = false;
        g.pu = R2.u; g.ph = R2.h; g.ssh = R2.ssh; g.cu = A.u; g.ch = A.h; g.nu_in = B.u; g.nh_in = B.h;
        g.pu_out = R1.u; g.ph_out = R1.h; g.ssh_out = R1.ssh; g.a = a[2];
    } else {               // Provis = R1; New += b4*k4; ssh of New
        g.pu = R1.u; g.ph = R1.h; g.ssh = R1.ssh; g.cu = A.u; g.ch = A.h; g.nu_in = B.u; g.nh_in = B.h;
        g.ssh_out = B.ssh; g.a = 0.0;
    }
    return g;
}

// buffers a stage writes that other ranks gather from next: stage 1,3 -> R1; 2 -> R2; 4 -> B; 0 -> current level
// 5 = the new level of a distributed Forward-Euler step before its levels rotate
LevelBufs &rk4_stage_output(moka_state *st, int s)
{
    return s == 0 ? st->lev[1] : s == 5 ? fe_new_level(st) : s == 4 ? st->lev[0] : s == 2 ? st->rk[1] : st->rk[0];
}

int rk4_begin(moka_state *st, const double **ssh0)
{
    int rc = ensure_rk_bufs(st);
    if (rc) return rc;
    st->feLazy = false;              // the arrays a lean Forward-Euler step left pending are superseded by this step's (rk4_end)
    *ssh0 = st->lev[1].ssh;
    if (!st->sshConsistent) {    // the tendency of stage 1 uses ssh computed from layerThickness
        if ((rc = make_ssh_consistent(st, st->rk[1].ssh))) return rc;
        *ssh0 = st->rk[1].ssh;
    }
    return MOKA_OK;
}

void rk4_end(moka_state *st)
{
    std::swap(st->lev[0], st->lev[1]);
    std::swap(st->trPhi[0], st->trPhi[1]);       // the tracers' time levels rotate with the state's
    st->sshConsistent = true;
    st->diagDirty = true;
    st->tendDirty = true;
    st->hEdgePrev = false;
    st->lazyPu = st->lazyPh = nullptr; st->lazyOwner = nullptr;
}

// ---- the RK4 step with 13 instead of 16 state streams (opt-in: moka_set_tuning key 7) -----------------------------------------
// The reference accumulates New += b_s k_s through the four stages (time_integration.jl:134-135): New is written by stage 1 and
// read + written by stages 2-4 = 7 of the step's 16 state streams.  The provisional states carry the same information:
// P2 - C = dt/2 k1, P3 - C = dt/2 k2, P4 - C = dt k3, so New = C + ((P2 - C) + 2 (P3 - C) + (P4 - C)) / 3 + dt/6 k4 can be formed by
// stage 4 alone from OWN rows (no gathers): streams per stage 2 / 3 / 3 / 5 = 13.  Same four buffer sets: P2 -> R1, P3 -> R2,
// P4 -> the previous level's set, New over P2 in place; the sets then rotate (current <- R1, previous <- old current, R1 <- old
// previous holding P4, which the lazily produced stage-4 tendencies read).  Round-off differs from the running sum (a few
// units in the last place of the state per step), hence opt-in; Float64 states on whole meshes through the default stage kernel
// (with the nonlinear terms: through k_stage_nl5, twin oracle_step_rk4_nonlinear_s13).
bool rk13_usable(const moka_state *st)
{
    if (!tuning(TUNE_RK13) || st->f32) return false;
    if (st->nTracers > 0) return false;                          // tracers: the running sum (their stage launch follows its buffers)
    if (st->nonlinear && st->viscDel4 != 0.0) return false;     // Del4: the reference's running sum (no 13-stream twin)
    const moka_mesh *mm = st->mesh;
    if (mm->plan.nPatchesLaunch != mm->plan.nPatches) return false;
    if (st->nonlinear)             // nonlinear terms: k_stage_nl5 carries the form (StageArgs.rkMode 9), the plainer kernels do not
        return nl_stage_is_nl5(mm->dev, mm->lpc, mm->plan.ldsOk, nl_form(st->ctx));
    return default_stage_kernels(st) && rec2c_supported(launch_bounds(mm));
}

// ---- New from RK4 stage 1 to stage 2 as one-byte codes (moka_set_tuning key 12) -------------------------------------------------
// Only stage 1 starts from Provis == Curr == New, so its two results P = C + a t and N = C + b t (time_integration.jl:124-125, 134-135)
// determine each other up to a few units in the last place: stage 1 stores a checked signed byte per value instead of N (an escape
// keeps N itself in the New array), stage 2 rebuilds N from the own rows of Curr and Provis it reads anyway (rk_handoff_* in
// kernels_common.hpp; k_stage_rec2c modes 12 / 13) and stores New in full.  Bit for bit: 7/8 of a state stream less in each of the
// two stages.  On only where BOTH stages run through launch_stage_rec2c, whole-mesh launches and patch ranges alike (own rows only):
// a Float64 state, the reference's 16-stream form, no nonlinear terms, the default kernel choice, a mesh that kernel carries in
// every launch shape.  Nothing reads New between the two stages: the tracer stage, the tapes' recording copies and the halo push
// take Provis (New only behind stage 4).
bool rk_handoff_usable(const moka_state *st)
{
    if (!tuning(TUNE_RK_HANDOFF) || st->f32 || st->nonlinear || !st->hoCodeU || !st->hoCodeH) return false;
    if (rk13_usable(st)) return false;
    const moka_mesh *mm = st->mesh;
    return default_stage_kernels(st) && rec2c_supported(launch_bounds(mm)) && rec2c_supported(mm->dev);
}

StageArgs rk13_stage_args(moka_state *st, int s, double dt, const double *ssh0)
{
    LevelBufs &A = st->lev[1], &B = st->lev[0], &R1 = st->rk[0], &R2 = st->rk[1];
    StageArgs g{};
    if (s == 1) {          // P2 = C + dt/2 k1 -> R1
        g.pu = A.u; g.ph = A.h; g.ssh = ssh0;
        g.pu_out = R1.u; g.ph_out = R1.h; g.ssh_out = R1.ssh; g.a = dt / 2.; g.rkMode = 7;
    } else if (s == 2) {   // P3 = C + dt/2 k2 -> R2
        g.pu = R1.u; g.ph = R1.h; g.ssh = R1.ssh; g.cu = A.u; g.ch = A.h;
        g.pu_out = R2.u; g.ph_out = R2.h; g.ssh_out = R2.ssh; g.a = dt / 2.; g.rkMode = 8;
    } else if (s == 3) {   // P4 = C + dt k3 -> B
        g.pu = R2.u; g.ph = R2.h; g.ssh = R2.ssh; g.cu = A.u; g.ch = A.h;
        g.pu_out = B.u; g.ph_out = B.h; g.ssh_out = B.ssh; g.a = dt; g.rkMode = 8;
    } else {               // New over P2 (R1), ssh of New
        g.pu = B.u; g.ph = B.h; g.ssh = B.ssh; g.cu = A.u; g.ch = A.h;
        g.nu_in = R1.u; g.nh_in = R1.h; g.q3u = R2.u; g.q3h = R2.h;
        g.nu_out = R1.u; g.nh_out = R1.h; g.ssh_out = R1.ssh; g.b = dt / 6.; g.rkMode = 9;
    }
    return g;
}

void rk13_end(moka_state *st)
{
    const LevelBufs A = st->lev[1], B = st->lev[0], R1 = st->rk[0];
    st->lev[1] = R1;             // New
    st->lev[0] = A;              // the level the step started from
    st->rk[0] = B;               // P4: the provisional state of stage 4 (lazily produced tendencies read it, like rk4_end's rk[0])
    st->sshConsistent = true;
    st->diagDirty = true;
    st->tendDirty = true;
    st->hEdgePrev = false;
    st->lazyPu = st->lazyPh = nullptr; st->lazyOwner = nullptr;
}

// keCoef on the device: meshes with the nonlinear arrays upload it when they are created, the others when a state first asks
int ensure_ke_coef(moka_mesh *m)
{
    if (m->dev.keCoef) return MOKA_OK;
    return m->mem.upload(m->plan.keCoef, &m->dev.keCoef);
}

// the bottom-speed launch over the whole mesh: u a (K, nE) field, sp nE doubles (keCoef is on the device: ensure_ke_coef)
MomSpeedArgs bottom_speed_args(const moka_state *st, const double *u, double *sp)
{
    const Plan &p = st->mesh->plan;
    const MeshDev &d = st->mesh->dev;
    MomSpeedArgs a{};
    a.nE = p.nE; a.K = p.K; a.ME = p.ME;
    a.ehdr = d.ehdr; a.eoc = d.eoc; a.mltc = d.mltc; a.keCoef = d.keCoef; a.invArea = d.invArea;
    a.u = u; a.sp = sp;
    return a;
}

// The vertical pass of the flow (implicit vertical mixing of momentum with a surface stress and a bottom drag, include/moka_hip.h): behind
// stage 4 on the new level's normalVelocity and layerThickness, through the same two pointers in the 16- and the 13-stream form; with
// Cd != 0 the bottom-speed launch goes in front of it.  The
// caller skips it while the pass is off and when dt == 0.0.  Launches only: nothing is allocated, synchronised or read back, so a
// captured step replays it.
int momentum_vmix(moka_state *st, double *u, const double *h, double dt)
{
    const Plan &p = st->mesh->plan;
    MomVmixArgs a{};
    a.nE = p.nE; a.K = p.K; a.ehdr = st->mesh->dev.ehdr; a.u = u; a.h = h;
    a.tau = st->momTau && st->momTauOn ? st->momTau : nullptr;
    a.dt = dt; a.nu = mom_vmix_nu(st); a.drag = st->momDrag; a.scratch = st->momScratch;
    a.fld = mom_vmix_field(st);
    if (st->rich && p.K >= 2) { a.nu = 0.0; a.fld = st->richF; }      // the Richardson closure: F of this step, the caller's nuV and field set aside
    const bool qd = st->momCd != 0.0;
    if (p.K < 2 && a.drag == 0.0 && !qd && !a.tau) return MOKA_OK;      // one level and the viscosity alone: no column has anything to do
    const bool generic = st->ctx->variant == 3;
    if (qd) {       // the quadratic drag: the bottom speed of u*, before the pass overwrites u
        HIPCHK(st->ctx, launch_momentum_bottom_speed(bottom_speed_args(st, u, st->momSpeed), st->ctx->stream));
        a.speed = st->momSpeed; a.cd = st->momCd;
    }
    st->momSpeedUsed = qd;
    HIPCHK(st->ctx, launch_momentum_vmix(a, generic, st->ctx->stream));
    st->momVmixPath = momentum_vmix_form(p.K, generic);
    return MOKA_OK;
}

// moka_step_rk4, and the same step recorded on `rec`: each stage's provisional state is copied behind that stage's launches, before a
// later stage overwrites the ping-pong buffer; the new thickness behind stage 4.  Copies only: the step's launches are untouched.
int step_rk4(moka_state *st, double dt, moka_tracer_tape *rec)
{
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    const bool rich = st->rich;             // the Richardson closure: both vertical passes are on and take the coefficients it computes
    if (rich && dt < 0.0) return fail(st->ctx, MOKA_ERR_ARG, "Richardson closure: dt must be >= 0 (the implicit solves are not reversible in time)");
    const bool vmix = st->nTracers > 0 && (rich || st->trKappaVDev != nullptr);      // (non-null exactly while some kappaV != 0 or some diffusivity field is on)
    if (vmix && dt < 0.0) return fail(st->ctx, MOKA_ERR_ARG, "vertical tracer diffusion: dt must be >= 0 (the implicit solve is not reversible in time)");
    const bool mvmix = mom_vmix_on(st);
    if (mvmix && dt < 0.0) return fail(st->ctx, MOKA_ERR_ARG, "vertical momentum mixing: dt must be >= 0 (the implicit solve is not reversible in time)");
    const double *ssh0 = nullptr;
    int rc = rk4_begin(st, &ssh0);
    if (rc) return rc;
    moka_ctx *c = st->ctx;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(c->stream, &cap);
    const bool timed = c->stageTiming && cap == hipStreamCaptureStatusNone;
    auto stamp = [&]() -> hipError_t {
        if (c->evUsed == c->evPool.size()) {
            hipEvent_t e = nullptr;
            if (hipError_t er = hipEventCreate(&e); er != hipSuccess) return er;
            c->evPool.push_back(e);
        }
        return hipEventRecord(c->evPool[c->evUsed++], c->stream);
    };
    const bool s13 = rk13_usable(st);
    if (s13) st->hoLive = st->hoRan = false;      // (no New travels through stages 1-3 of that form: nothing to hand over)
    for (int s = 1; s <= 4; ++s) {
        if (timed) HIPCHK(c, stamp());
        const StageArgs g = s13 ? rk13_stage_args(st, s, dt, ssh0) : rk4_stage_args(st, s, dt, ssh0);
        HIPCHK(c, run_stage(st, g));
        if (st->nTracers > 0) HIPCHK(c, tracer_stage(st, s, g));
        if (s == 4) {       // the closure: F and G from the new level as stage 4 and the tracers' stage 4 left it, in front of both passes
            st->richRan = rich && st->mesh->plan.K >= 2 && dt != 0.0;
            if (st->richRan)
                HIPCHK(c, launch_richardson(rich_args(st, g.nu_out, g.nh_out, st->trPhi[0] + (size_t)st->mesh->plan.K * st->mesh->plan.nC * st->richP.buoyancyTracer), c->stream));
        }
        if (s == 4 && vmix && st->mesh->plan.K >= 2 && dt != 0.0)       // the split step: the new tracers (still in the previous level's array) over the new thickness
            if ((rc = tracer_vmix(st->mesh, c, st->nTracers, g.nh_out, st->trPhi[0], rich ? st->richKvDev : st->trKappaVDev, rich ? st->richVfDev : st->trVfDev, dt,
                                  st->trVmixScratch, false, &st->vmixPath))) return rc;
        if (s == 4 && mvmix && dt != 0.0)       // the split step of the flow: the new normalVelocity over the new thickness (the tracers' stage 4 has read the provisional flow)
            if ((rc = momentum_vmix(st, g.nu_out, g.nh_out, dt))) return rc;
        if (rec) {
            const Plan &p = st->mesh->plan;
            const size_t nEK = (size_t)p.K * p.nE, nCK = (size_t)p.K * p.nC;
            HIPCHK(c, hipMemcpyAsync(rec->pu + nEK * (4 * rec->n + s - 1), g.pu, nEK * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(rec->ph + nCK * (4 * rec->n + s - 1), g.ph, nCK * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
            if (s == 4) HIPCHK(c, hipMemcpyAsync(rec->hn + nCK * rec->n, g.nh_out, nCK * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
            // pphi_{s-1} of the tracers flagged for a diffusivity gradient: what tracer_stage handed the stage's launches
            const double *pphi = s == 1 ? st->trPhi[1] : st->trProv[s == 3 ? 1 : 0];
            const size_t nF = rec->kgTracer.size();
            for (size_t f = 0; f < nF; ++f)
                HIPCHK(c, hipMemcpyAsync(rec->kgP + nCK * ((4 * rec->n + s - 1) * nF + f), pphi + nCK * rec->kgTracer[f], nCK * sizeof(double),
                                         hipMemcpyDeviceToDevice, c->stream));
            // phi_new of the tracers flagged for the vertical gradient: behind the vertical pass where one ran, else what stage 4 formed
            const size_t nV = rec->vgTracer.size();
            for (size_t f = 0; s == 4 && f < nV; ++f)
                HIPCHK(c, hipMemcpyAsync(rec->vgP + nCK * (rec->n * nV + f), st->trPhi[0] + nCK * rec->vgTracer[f], nCK * sizeof(double),
                                         hipMemcpyDeviceToDevice, c->stream));
        }
    }
    if (timed) HIPCHK(c, stamp());
    if (s13) rk13_end(st);
    else rk4_end(st);
    return MOKA_OK;
}


}  // namespace mk

using namespace mk;

extern "C" {

// ---------------------------------------------------------------------------------------------
// state
// ---------------------------------------------------------------------------------------------
int moka_state_create(moka_ctx *ctx, moka_mesh *mesh, moka_state **out)
{
    if (!ctx || !mesh || !out) return fail(ctx, MOKA_ERR_ARG, "NULL argument");
    *out = nullptr;
    moka_state *st = new (std::nothrow) moka_state();
    if (!st) return fail(ctx, MOKA_ERR_ALLOC, "out of host memory");
    st->ctx = ctx;
    st->mem.ctx = ctx;
    st->mesh = mesh;
    const Plan &p = mesh->plan;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nEK = (size_t)p.K * p.nE, nCK = (size_t)p.K * p.nC, nVK = (size_t)p.K * p.nV;
    st->f32 = p.stateBytes == 4;
    const MeshDev launchDev = launch_bounds(mesh);
    if (st->f32 && !stage_f32_supported(launchDev)) {
        delete st;
        return fail(ctx, MOKA_ERR_UNSUPPORTED,
                    "fp32-storage state: needs nVertLevels % 4 == 0, nVertLevels <= 128, fields below 4 GiB and patches whose "
                    "records + own u rows fit 64 KB of LDS (smaller patch_cells)");
    }
    const size_t sb = st->f32 ? 4 : 8;
    int rc = MOKA_OK;
    auto A = [&](double **q, size_t n, size_t eb = 8) { if (rc == MOKA_OK) rc = st->mem.alloc(q, n, eb); };
    for (auto &l : st->lev) { A(&l.ssh, p.nC, sb); A(&l.u, nEK, sb); A(&l.h, nCK, sb); }
    A(&st->hEdge[0], nEK, sb); A(&st->hEdge[1], nEK, sb);     // DiagnosticVars arrays have the state's storage type
    A(&st->F, nEK, sb); A(&st->div, nCK, sb); A(&st->vort, nVK, sb);
    A(&st->tendU, nEK, sb); A(&st->tendH, nCK, sb);       // fp32-storage states store their tendencies fp32 as well
    A(&st->scalar, 2);
    if (rc != MOKA_OK) { moka_state_destroy(st); return rc; }
    st->phys[0] = st->lev[0]; st->phys[1] = st->lev[1];
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    {
        std::lock_guard<std::mutex> lk(g_liveMutex);
        g_liveStates.insert(st);
    }
    *out = st;
    return MOKA_OK;
}

void moka_state_destroy(moka_state *st)
{
    if (!st) return;
    {
        std::lock_guard<std::mutex> lk(g_liveMutex);
        g_liveStates.erase(st);
    }
    (void)hipSetDevice(st->ctx->device);
    (void)hipStreamSynchronize(st->ctx->stream);
    st->mem.release_all();
    delete st;
}

int moka_state_upload(moka_state *st, int field, int time_level, const double *host)
{
    if (!st || !host) return fail(st ? st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    FieldRef r;
    int rc = field_ref(st, field, time_level, &r);
    if (rc) return rc;
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    // the arrays of a lean Forward-Euler step are derived from the previous level (and the one before): whatever the caller
    // overwrites, they are produced from the values the step saw
    if (st->feLazy && !(field <= MOKA_F_LAYER_THICKNESS && time_level == 1))
        if ((rc = flush_lazy(st, true, true))) return rc;
    const bool prog1 = field <= MOKA_F_LAYER_THICKNESS && time_level == 1;   // pending lazy results refer to the old state
    // (an fp32-storage state cannot materialise pending diagnostics: they stay pending, i.e. unavailable)
    if ((rc = flush_lazy(st, (prog1 && !st->f32) || is_diag_field(field), prog1 || is_tend_field(field)))) return rc;
    if ((rc = field_ref(st, field, time_level, &r))) return rc;   // flush may have swapped buffers
    if (time_level == 1 && (field == MOKA_F_SSH || field == MOKA_F_LAYER_THICKNESS)) st->sshConsistent = false;
    if ((field == MOKA_F_LAYER_THICKNESS && time_level == 0) || field == MOKA_F_LAYER_THICKNESS_EDGE) st->hEdgePrev = false;
    return put_rows(st->mesh, r.ptr, host, r.kind, r.n, r.K, r.f32);
}

int moka_state_download(moka_state *st, int field, int time_level, double *host)
{
    if (!st || !host) return fail(st ? st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    FieldRef r;
    int rc = field_ref(st, field, time_level, &r);
    if (rc) return rc;
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    if ((rc = flush_lazy(st, is_diag_field(field), is_tend_field(field)))) return rc;
    if ((rc = field_ref(st, field, time_level, &r))) return rc;   // flush may have swapped buffers
    return get_rows(st->mesh, host, r.ptr, r.kind, r.n, r.K, r.f32);
}

int moka_advance_time_levels(moka_state *st, int flags)
{
    if (!st) return fail(nullptr, MOKA_ERR_ARG, "state is NULL");
    const Plan &p = st->mesh->plan;
    hipStream_t s = st->ctx->stream;
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    if (int rcl = flush_lazy(st, st->feLazy, st->feLazy)) return rcl;      // a lean step's arrays derive from the level overwritten now
    st->hEdgePrev = false;                 // the previous level changes under the stored layerThicknessEdge
    // advance_2d_array / advance_3d_array (time_integration.jl:42-59): prev <- next.
    // Level-1-only copies (K > 1) go through the FE kernel's carry-over path instead.
    if ((flags & MOKA_FE_LEVEL1_ONLY) && p.K > 1)
        return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "level-1-only advanceTimeLevels! is only available inside moka_step_fe");
    if (st->f32) {   // float arrays: plain device copies
        HIPCHK(st->ctx, hipMemcpyAsync(st->lev[0].ssh, st->lev[1].ssh, (size_t)p.nC * 4, hipMemcpyDeviceToDevice, s));
        HIPCHK(st->ctx, hipMemcpyAsync(st->lev[0].u, st->lev[1].u, (size_t)p.K * p.nE * 4, hipMemcpyDeviceToDevice, s));
        HIPCHK(st->ctx, hipMemcpyAsync(st->lev[0].h, st->lev[1].h, (size_t)p.K * p.nC * 4, hipMemcpyDeviceToDevice, s));
        return MOKA_OK;
    }
    HIPCHK(st->ctx, launch_copy(st->lev[0].ssh, st->lev[1].ssh, p.nC, s));
    HIPCHK(st->ctx, launch_copy(st->lev[0].u, st->lev[1].u, (int64_t)p.K * p.nE, s));
    HIPCHK(st->ctx, launch_copy(st->lev[0].h, st->lev[1].h, (int64_t)p.K * p.nC, s));
    if (st->nTracers > 0) HIPCHK(st->ctx, launch_copy(st->trPhi[0], st->trPhi[1], (int64_t)st->nTracers * p.K * p.nC, s));
    return MOKA_OK;
}

int moka_diagnostic_compute(moka_state *st, int flags)
{
    if (!st) return fail(nullptr, MOKA_ERR_ARG, "state is NULL");
    if (st->nonlinear) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "nonlinear terms: moka_tendencies / RK4 only");
    if (st->f32) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "fp32-storage state: moka_step_fe, moka_step_rk4 and moka_tendencies only (the piecewise reference calls are Float64)");
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    if (int rcl = flush_lazy(st, true, false)) return rcl;
    FeArgs a = fe_args(st, FE_FLUX | FE_DIV | FE_CURL | FE_HEDGE, flags, 0.0);
    HIPCHK(st->ctx, launch_fe(st->mesh->dev, a, st->mesh->lpc, st->ctx->stream));
    std::swap(st->hEdge[0], st->hEdge[1]);
    st->hEdgePrev = false;
    return MOKA_OK;
}

int moka_compute_normal_velocity_tendency(moka_state *st, int flags)
{
    if (!st) return fail(nullptr, MOKA_ERR_ARG, "state is NULL");
    if (st->nonlinear) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "nonlinear terms: moka_tendencies / RK4 only");
    if (st->f32) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "fp32-storage state: moka_step_fe, moka_step_rk4 and moka_tendencies only (the piecewise reference calls are Float64)");
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    if (int rcl = flush_lazy(st, false, true)) return rcl;
    FeArgs a = fe_args(st, FE_TENDU, flags, 0.0);
    HIPCHK(st->ctx, launch_fe(st->mesh->dev, a, st->mesh->lpc, st->ctx->stream));
    return MOKA_OK;
}

int moka_compute_layer_thickness_tendency(moka_state *st, int flags)
{
    if (!st) return fail(nullptr, MOKA_ERR_ARG, "state is NULL");
    if (st->nonlinear) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "nonlinear terms: moka_tendencies / RK4 only");
    if (st->f32) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "fp32-storage state: moka_step_fe, moka_step_rk4 and moka_tendencies only (the piecewise reference calls are Float64)");
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    if (int rcl = flush_lazy(st, true, true)) return rcl;
    FeArgs a = fe_args(st, FE_TENDH | FE_TENDH_FROM_F, flags, 0.0);
    HIPCHK(st->ctx, launch_fe(st->mesh->dev, a, st->mesh->lpc, st->ctx->stream));
    return MOKA_OK;
}

int moka_tendencies(moka_state *st)
{
    if (!st) return fail(nullptr, MOKA_ERR_ARG, "state is NULL");
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    int rc;
    if (!st->sshConsistent) {
        if ((rc = make_ssh_consistent(st, st->lev[1].ssh))) return rc;
        st->sshConsistent = true;
    }
    if (st->feLazy && (rc = flush_lazy(st, true, true))) return rc;        // (it would overwrite the tendencies written here later)
    StageArgs a{};
    a.pu = st->lev[1].u; a.ph = st->lev[1].h; a.ssh = st->lev[1].ssh;
    a.tendU = st->tendU; a.tendH = st->tendH;
    HIPCHK(st->ctx, run_stage(st, a));
    st->tendDirty = false;
    return MOKA_OK;
}

int moka_step_fe(moka_state *st, double dt, int flags)
{
    if (!st) return fail(nullptr, MOKA_ERR_ARG, "state is NULL");
    if (st->rich) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "Richardson closure: applied by RK4 steps only (no Forward Euler)");
    if (st->nonlinear) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "nonlinear terms: moka_tendencies / RK4 only");
    if (st->nTracers > 0) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "tracers: transported by RK4 steps only (no Forward Euler)");
    if (mom_vmix_on(st)) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "vertical momentum mixing: applied by RK4 steps only (no Forward Euler)");
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    const moka_mesh *mm = st->mesh;
    const bool whole = mm->plan.nPatchesLaunch == mm->plan.nPatches;
    if (st->f32 && ((flags & MOKA_FE_LEVEL1_ONLY) || !whole))
        return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "fp32-storage state: Forward Euler steps all levels of a whole mesh (no MOKA_FE_LEVEL1_ONLY, no partitions)");
    // All levels on a whole mesh with the default kernel choice: the step runs in the stage kernels (modes 4 / 5 / 6 of
    // k_stage_rec2c*), relativeVorticity in the same launch where the vertex records fit.  Anything else -- MOKA_FE_LEVEL1_ONLY, odd
    // or large K, explicit kernel variants, local meshes of a partition outside the halo API -- takes the generic one-launch kernel.
    const bool stagePath = whole && fe_stage_path(st, flags);
    if (stagePath)
        if (int rcs = ensure_spare(st)) return rcs;            // the new level goes to the spare set; the previous one stays readable
    const bool lean = stagePath && fe_lean(st, flags);
    if (int rcl = fe_begin(st, flags)) return rcl;
    // advanceTimeLevels! + diagnostic_compute! + both tendencies + updates (time_integration.jl:163-189) in one launch: the new
    // level is written into the spare set (or, without one, over the previous level), then the levels rotate.
    FeArgs a = fe_args(st, FE_FLUX | FE_DIV | FE_CURL | FE_HEDGE | FE_TENDU | FE_TENDH | FE_UPDATE, flags, dt);
    bool fast = false, prevMode = false;
    if (stagePath) {
        StageArgs g = fe_stage_args(st, a, flags);
        MeshDev dev = launch_bounds(mm);
        dev.tailPatch = -1;
        auto launch = [&]() { return st->f32 ? launch_stage_rec2c_f32(dev, g, st->ctx->stream) : launch_stage_rec2c(dev, g, st->ctx->stream); };
        hipError_t e = launch();
        if (e == hipErrorNotSupported && g.vort) {             // vertex records do not fit beside the rows after all: own launch
            g.vort = nullptr;
            e = launch();
        }
        if (e == hipSuccess) {
            fast = true;
            prevMode = g.hPrev != nullptr;
            if (!g.vort) {                                     // ssh as stored, relativeVorticity of the OLD state
                if (st->f32) {
                    HIPCHK(st->ctx, launch_curl_f32(dev, reinterpret_cast<const float *>(a.u), reinterpret_cast<float *>(a.vort),
                                                    flags & MOKA_FE_ACCUM_VORT, st->ctx->stream));
                } else {
                    const hipError_t ec = launch_curl2(mm->dev, a.u, a.vort, flags & MOKA_FE_ACCUM_VORT, st->ctx->stream);
                    if (ec == hipErrorNotSupported) {
                        a.ops = FE_CURL;
                        HIPCHK(st->ctx, launch_fe(mm->dev, a, mm->lpc, st->ctx->stream));
                    } else {
                        HIPCHK(st->ctx, ec);
                    }
                }
            }
        } else if (e != hipErrorNotSupported || st->f32 || lean) {
            HIPCHK(st->ctx, e);                                // (fp32 storage and lean steps have no generic form behind them)
            return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "internal: the stage kernel refused a Forward-Euler launch it was selected for");
        }
    }
    if (!fast) HIPCHK(st->ctx, launch_fe(mm->dev, a, mm->lpc, st->ctx->stream));
    fe_end(st, flags, fast, fast && lean, prevMode);
    st->sshConsistent = !(flags & MOKA_FE_LEVEL1_ONLY) || mm->plan.K == 1;
    return MOKA_OK;
}

int moka_fe_lazy_pending(const moka_state *st) { return st && st->feLazy ? 1 : 0; }

int moka_state_rk4_streams(const moka_state *st) { return !st ? 0 : rk13_usable(st) ? 13 : 16; }

// the host build of the codec the stage kernels run (kernels_common.hpp, under the library's -ffp-contract=off): no GPU is touched
int moka_rk_handoff_codec(const double *C, const double *P, const double *N, double rho, int64_t n, int8_t *code_out, double *decoded_out)
{
    if (n < 0 || (n > 0 && (!C || !P || !N || !code_out || !decoded_out))) return fail(nullptr, MOKA_ERR_ARG, "moka_rk_handoff_codec: NULL argument");
    for (int64_t i = 0; i < n; ++i) {
        const int8_t c = moka::rk_handoff_encode(C[i], P[i], N[i], rho);
        code_out[i] = c;
        decoded_out[i] = c == (int8_t)moka::RK_HANDOFF_ESCAPE ? N[i] : moka::rk_handoff_decode(C[i], P[i], (int)c, rho);
    }
    return MOKA_OK;
}

// a test aid, off the step path: the code arrays of the last hand-off step, copied to the host and counted
int moka_state_rk_handoff_escapes(moka_state *st, int64_t *cells, int64_t *edges)
{
    if (!st || !cells || !edges) return fail(st ? st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    *cells = *edges = 0;
    if (!st->hoRan || !st->hoCodeU || !st->hoCodeH)
        return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "the last RK4 step of this state did not hand New over as codes (moka_set_tuning key 12)");
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    const Plan &p = st->mesh->plan;
    std::vector<signed char> host;
    auto count = [&](const signed char *dev, size_t n, int64_t *out) -> int {
        host.resize(n);
        HIPCHK(st->ctx, hipMemcpyAsync(host.data(), dev, n, hipMemcpyDeviceToHost, st->ctx->stream));
        HIPCHK(st->ctx, hipStreamSynchronize(st->ctx->stream));
        *out = (int64_t)std::count(host.begin(), host.end(), (signed char)moka::RK_HANDOFF_ESCAPE);
        return MOKA_OK;
    };
    if (int rc = count(st->hoCodeH, (size_t)p.K * p.nC, cells)) return rc;
    return count(st->hoCodeU, (size_t)p.K * p.nE, edges);
}

int moka_step_rk4(moka_state *st, double dt)
{
    if (!st) return fail(nullptr, MOKA_ERR_ARG, "state is NULL");
    return step_rk4(st, dt, nullptr);
}

// Per-stage kernel durations of moka_step_rk4 from HIP events on the compute stream (bench.py's per-mode roofline lines).
// enable != 0: forget earlier samples and start recording 5 events per step; enable == 0: stop.
int moka_stage_timing(moka_ctx *ctx, int enable)
{
    if (!ctx) return fail(nullptr, MOKA_ERR_ARG, "ctx is NULL");
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->stageTiming = enable != 0;
    if (enable) ctx->evUsed = 0;
    return MOKA_OK;
}

// ms[s-1] = mean duration of the stage-s launch over the recorded steps; *steps = how many steps were recorded
int moka_stage_timing_read(moka_ctx *ctx, double ms[4], int64_t *steps)
{
    if (!ctx || !ms || !steps) return fail(ctx, MOKA_ERR_ARG, "NULL argument");
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const size_t n = ctx->evUsed / 5;
    for (int s = 0; s < 4; ++s) ms[s] = 0.0;
    for (size_t i = 0; i < n; ++i)
        for (int s = 0; s < 4; ++s) {
            float t = 0.f;
            HIPCHK(ctx, hipEventElapsedTime(&t, ctx->evPool[5 * i + s], ctx->evPool[5 * i + s + 1]));
            ms[s] += t;
        }
    for (int s = 0; s < 4; ++s) ms[s] = n ? ms[s] / (double)n : 0.0;
    *steps = (int64_t)n;
    return MOKA_OK;
}

int moka_run(moka_state *st, int integrator, double dt, int64_t nsteps, int flags)
{
    if (!st) return fail(nullptr, MOKA_ERR_ARG, "state is NULL");
    if (nsteps < 0) return fail(st->ctx, MOKA_ERR_ARG, "nsteps must be >= 0");
    if (integrator != MOKA_FORWARD_EULER && integrator != MOKA_RUNGE_KUTTA_4) return fail(st->ctx, MOKA_ERR_ARG, "unknown integrator");
    if (integrator == MOKA_RUNGE_KUTTA_4 && dt < 0.0 && st->rich)
        return fail(st->ctx, MOKA_ERR_ARG, "Richardson closure: dt must be >= 0 (the implicit solves are not reversible in time)");
    if (integrator == MOKA_FORWARD_EULER && st->rich)
        return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "Richardson closure: applied by RK4 steps only (no Forward Euler)");
    if (integrator == MOKA_RUNGE_KUTTA_4 && dt < 0.0 && st->nTracers > 0 && st->trKappaVDev)
        return fail(st->ctx, MOKA_ERR_ARG, "vertical tracer diffusion: dt must be >= 0 (the implicit solve is not reversible in time)");
    if (integrator == MOKA_RUNGE_KUTTA_4 && dt < 0.0 && mom_vmix_on(st))
        return fail(st->ctx, MOKA_ERR_ARG, "vertical momentum mixing: dt must be >= 0 (the implicit solve is not reversible in time)");
    if (integrator == MOKA_FORWARD_EULER && mom_vmix_on(st))
        return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "vertical momentum mixing: applied by RK4 steps only (no Forward Euler)");
    auto one = [&]() { return integrator == MOKA_FORWARD_EULER ? moka_step_fe(st, dt, flags) : moka_step_rk4(st, dt); };
    int64_t done = 0;
    int rc;
    // Launch-bound regime (small meshes): capture one PERIOD of consecutive steps into a hipGraph and replay it.  The
    // pointer pattern of a step repeats after 2 steps when the two time-level sets swap (RK4; Forward Euler without a spare
    // set) and after 6 when a Forward-Euler step rotates three level sets (period 3) while layerThicknessEdge's two buffers
    // swap (period 2).  The first step runs eagerly: it may have to make ssh consistent and allocate the RK buffers or the
    // spare set, none of which may happen during capture -- and it brings the state into the steady regime every later step
    // is launched in (e.g. layerThicknessEdge formed from the previous level from the second step on).
    if (nsteps >= 6) {
        if ((rc = one())) return rc;
        ++done;
        if (integrator == MOKA_FORWARD_EULER && st->spare.ssh && nsteps - done >= 2) {   // one more: the regime settles with step 2
            if ((rc = one())) return rc;
            ++done;
        }
    }
    // (the 13-stream RK4 form rotates three buffer sets: period 3; 6 serves it too)
    const int period = ((integrator == MOKA_FORWARD_EULER && st->spare.ssh) || (integrator == MOKA_RUNGE_KUTTA_4 && rk13_usable(st))) ? 6 : 2;
    if (done > 0 && nsteps - done >= period) {
        HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
        // nothing lazy may fire inside the capture (pending diagnostics of an fp32-storage state cannot be produced: they
        // stay pending -- an RK4 run leaves them pending anyway, a Forward-Euler step has none)
        if ((rc = flush_lazy(st, !st->f32, true))) return rc;
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        hipStream_t s = st->ctx->stream;
        if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            const bool d0 = st->diagDirty, t0 = st->tendDirty;
            int rc2 = MOKA_OK;
            for (int i = 0; i < period && rc2 == MOKA_OK; ++i) {
                st->diagDirty = st->tendDirty = false;         // keep flush_lazy inside the steps a no-op while capturing
                rc2 = one();
            }
            hipError_t ec = hipStreamEndCapture(s, &graph);
            if (rc2 || ec != hipSuccess || !graph) {
                if (graph) (void)hipGraphDestroy(graph);
                st->diagDirty = d0; st->tendDirty = t0;
                return rc2 ? rc2 : fail(st->ctx, MOKA_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ec));
            }
            // the capture recorded the launches but executed nothing: the host-side swaps / rotations of one period cancel
            if (hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess) {
                hipError_t el = hipSuccess;
                while (nsteps - done >= period && (el = hipGraphLaunch(exec, s)) == hipSuccess) done += period;
                (void)hipGraphExecDestroy(exec);
                if (el != hipSuccess) {
                    (void)hipGraphDestroy(graph);
                    return fail(st->ctx, MOKA_ERR_HIP, std::string("hipGraphLaunch: ") + hipGetErrorString(el));
                }
            }
            (void)hipGraphDestroy(graph);
            st->diagDirty = st->tendDirty = (integrator == MOKA_RUNGE_KUTTA_4);
        }
    }
    for (; done < nsteps; ++done)
        if ((rc = one())) return rc;
    return MOKA_OK;
}

int moka_sum_sq(moka_state *st, int field, int time_level, double *out)
{
    if (!st || !out) return fail(st ? st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    FieldRef r;
    int rc = field_ref(st, field, time_level, &r);
    if (rc) return rc;
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    if ((rc = flush_lazy(st, is_diag_field(field), is_tend_field(field)))) return rc;     // lazily pending arrays are produced on a read
    if ((rc = field_ref(st, field, time_level, &r))) return rc;                            // (the flush may have swapped buffers)
    if ((rc = ensure_op_bufs(st->mesh))) return rc;
    hipStream_t s = st->ctx->stream;
    // caller's numbering, then the strictly serial order of sumArray (run_loop.jl:47-51)
    if (r.f32) HIPCHK(st->ctx, launch_permute_rows_f32(st->mesh->opBuf[2], r.ptr, perm_of(st->mesh, r.kind), r.n, r.K, 0, s));
    else HIPCHK(st->ctx, launch_permute_rows(st->mesh->opBuf[2], r.ptr, perm_of(st->mesh, r.kind), r.n, r.K, 0, s));
    HIPCHK(st->ctx, launch_sum_sq_serial(st->mesh->opBuf[2], r.n * r.K, st->scalar, s));
    HIPCHK(st->ctx, hipMemcpyAsync(out, st->scalar, sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(st->ctx, hipStreamSynchronize(s));
    return MOKA_OK;
}

int moka_last_fe_path(const moka_state *st) { return st ? st->feFast : -1; }

int moka_set_nonlinear(moka_state *st, int on)
{
    if (!st) return fail(nullptr, MOKA_ERR_ARG, "state is NULL");
    if (!on) {
        if (st->nonlinear) {           // the stage-4 tendencies an RK4 step left pending belong to the terms they were computed with
            HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
            if (int rc = flush_lazy(st, false, true)) return rc;
        }
        st->nonlinear = false;
        return MOKA_OK;
    }
    const Plan &p = st->mesh->plan;
    if (st->f32) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "nonlinear terms: Float64 states only");
    if (st->dycoreTapes > 0)
        return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "nonlinear terms: not while a moka_tape of this state exists (reverse mode covers the linear terms only)");
    if (st->forcedTapes > 0)
        return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "nonlinear terms: not while a moka_forced_tape of this state exists (reverse mode covers the linear terms only)");
    if (!p.nlOk)
        return fail(st->ctx, MOKA_ERR_UNSUPPORTED,
                    "nonlinear terms need kiteAreasOnVertex, fVertex, verticesOnEdge and cellsOnVertex in the mesh descriptor");
    // (a rank-local mesh is fine when its halo is two cells deep -- moka_hip.parallel.build_local(rings = 2) -- and every stage
    //  is launched over the whole local mesh: moka_rk4_dist_stage(h, s, 2); what its rim computes is never read by an owned entity)
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    int rc = flush_lazy(st, true, true);
    if (rc) return rc;
    if (!st->nlQv) {
        if ((rc = st->mem.alloc(&st->nlQv, (size_t)p.K * p.nV))) return rc;
        if ((rc = st->mem.alloc(&st->nlQe, 2 * (size_t)p.K * p.nE))) return rc;   // {F, q_e} pairs
        if ((rc = st->mem.alloc(&st->nlKe, (size_t)p.K * p.nC))) return rc;
    }
    st->nonlinear = true;
    return MOKA_OK;
}

int moka_set_viscosity_del2(moka_state *st, double viscDel2)
{
    if (!st) return fail(nullptr, MOKA_ERR_ARG, "state is NULL");
    if (!(viscDel2 >= 0.0)) return fail(st->ctx, MOKA_ERR_ARG, "viscDel2 must be >= 0");
    if (viscDel2 != 0.0 && !st->nonlinear)
        return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "Del2 mixing rides on the nonlinear tendencies: call moka_set_nonlinear first");
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    int rc;
    // pending stage-4 tendencies belong to the coefficient they were computed with (as in moka_set_viscosity_del4)
    if (viscDel2 != st->viscDel2 && (rc = flush_lazy(st, false, true))) return rc;
    if (viscDel2 != 0.0 && !st->nlZv) {
        const Plan &p = st->mesh->plan;
        if ((rc = st->mem.alloc(&st->nlZv, (size_t)p.K * p.nV))) return rc;
        if ((rc = st->mem.alloc(&st->nlDiv, (size_t)p.K * p.nC))) return rc;
    }
    st->viscDel2 = viscDel2;
    return MOKA_OK;
}

// the per-patch edge rows of k_d4_patch: the distinct edges of the patch's own cells and own vertices, and per cell / vertex slot the
// patch-local row of its edge.  Once per mesh.
static int ensure_d4_rows(moka_mesh *mm)
{
    if (mm->d4.start) return MOKA_OK;
    const Plan &p = mm->plan;
    const int ME = p.ME, VD = p.VD;
    std::vector<int32_t> start(p.nPatches + 1, 0), rows, local(p.nE, -1);
    std::vector<uint16_t> locC((size_t)p.nC * ME, 0), locV((size_t)p.nV * VD, 0);
    int maxRows = 0;
    for (int q = 0; q < p.nPatches; ++q) {
        const size_t base = rows.size();
        auto lid = [&](int e) {
            if (local[e] < 0) { local[e] = (int32_t)(rows.size() - base); rows.push_back(e); }
            return (uint16_t)std::min(local[e], 65535);
        };
        for (int c = p.patchCellStart[q]; c < p.patchCellStart[q + 1]; ++c)
            for (int i = 0; i < ME; ++i)
                if (const int e = p.eoc[(size_t)c * ME + i]; e >= 0) locC[(size_t)c * ME + i] = lid(e);
        for (int v = p.patchVertStart[q]; v < p.patchVertStart[q + 1]; ++v)
            for (int j = 0; j < VD; ++j)
                if (const int e = p.eov[(size_t)v * VD + j]; e >= 0) locV[(size_t)v * VD + j] = lid(e);
        const int n = (int)(rows.size() - base);
        maxRows = std::max(maxRows, n);
        for (size_t j = base; j < rows.size(); ++j) local[rows[j]] = -1;
        start[q + 1] = (int32_t)rows.size();
    }
    rows.push_back(0);
    D4Rows d{};
    d.maxRows = maxRows > 65535 ? INT32_MAX / 2 : maxRows;    // (a patch beyond 16-bit row ids never fits the LDS: entity kernels)
    int rc;
    if ((rc = mm->mem.upload(rows, &d.row)) || (rc = mm->mem.upload(locC, &d.locC)) || (rc = mm->mem.upload(locV, &d.locV))) return rc;
    if ((rc = mm->mem.upload(start, &d.start))) return rc;
    mm->d4 = d;
    return MOKA_OK;
}

int moka_set_viscosity_del4(moka_state *st, double viscDel4, const double *meshScalingDel4)
{
    if (!st) return fail(nullptr, MOKA_ERR_ARG, "state is NULL");
    if (!(viscDel4 >= 0.0)) return fail(st->ctx, MOKA_ERR_ARG, "viscDel4 must be >= 0");
    const Plan &p = st->mesh->plan;
    if (viscDel4 != 0.0) {
        if (st->f32) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "Del4 mixing: Float64 states only");
        if (!st->nonlinear)
            return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "Del4 mixing rides on the nonlinear tendencies: call moka_set_nonlinear first");
        if (st->halos > 0)
            return fail(st->ctx, MOKA_ERR_UNSUPPORTED,
                        "Del4 mixing: not on a state with a halo (its stencil reaches three cell rings, the nonlinear halo two)");
        if (meshScalingDel4)
            for (int e = 0; e < p.nE; ++e)
                if (!(meshScalingDel4[e] >= 0.0)) return fail(st->ctx, MOKA_ERR_ARG, "meshScalingDel4 entries must be >= 0");
    }
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    int rc = flush_lazy(st, true, true);       // pending tendencies belong to the coefficients they were computed with
    if (rc) return rc;
    if (viscDel4 == 0.0) { st->viscDel4 = 0.0; return MOKA_OK; }
    if (!st->nlZv) {
        if ((rc = st->mem.alloc(&st->nlZv, (size_t)p.K * p.nV))) return rc;
        if ((rc = st->mem.alloc(&st->nlDiv, (size_t)p.K * p.nC))) return rc;
    }
    if (!st->nlDiv4) {
        if ((rc = st->mem.alloc(&st->nlDiv4, (size_t)p.K * p.nC))) return rc;
        if ((rc = st->mem.alloc(&st->nlCurl4, (size_t)p.K * p.nV))) return rc;
        if ((rc = st->mem.alloc(&st->coef4, (size_t)p.nE))) return rc;
    }
    if ((rc = ensure_d4_rows(st->mesh))) return rc;
    std::vector<double> coef(p.nE, viscDel4);  // viscDel4 * meshScalingDel4[e], in double, in plan order
    if (meshScalingDel4)
        for (int e = 0; e < p.nE; ++e) coef[e] = viscDel4 * meshScalingDel4[p.edgeN2O[e]];
    if ((rc = h2d(st->ctx, st->coef4, coef.data(), coef.size() * sizeof(double)))) return rc;
    st->viscDel4 = viscDel4;
    return MOKA_OK;
}

int moka_state_del4_path(const moka_state *st) { return st ? st->del4Path : 0; }

// ---- implicit vertical mixing of momentum (include/moka_hip.h: the recipe; momentum_vmix.hip: the kernels) ----
// what a state must be for the pass to be switched on (checked only when a call asks for something other than zero / NULL)
static int mom_vmix_supported(moka_state *st)
{
    const Plan &p = st->mesh->plan;
    if (st->f32) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "vertical momentum mixing: Float64 states only");
    if (st->halos > 0) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "vertical momentum mixing: not on a state with a halo");
    if (p.nPatchesLaunch != p.nPatches) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "vertical momentum mixing: whole (unpartitioned) meshes only");
    if (st->dycoreTapes > 0)
        return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "vertical momentum mixing: not while a moka_tape of this state exists (reverse mode does not cover the pass)");
    return MOKA_OK;
}

// the scratch of the column form, allocated by the first call that turns the pass on (never by a step) and kept
static int mom_vmix_scratch(moka_state *st)
{
    if (st->momScratch) return MOKA_OK;
    const Plan &p = st->mesh->plan;
    if (int rc = st->mem.alloc(&st->momScratch, 2 * (size_t)p.K * p.nE)) return rc;
    HIPCHK(st->ctx, hipStreamSynchronize(st->ctx->stream));
    return MOKA_OK;
}

int moka_set_vertical_viscosity(moka_state *st, double nuV, double bottomDrag)
{
    if (!st) return fail(nullptr, MOKA_ERR_ARG, "state is NULL");
    if (!(nuV >= 0.0) || !std::isfinite(nuV) || !(bottomDrag >= 0.0) || !std::isfinite(bottomDrag))
        return fail(st->ctx, MOKA_ERR_ARG, "vertical momentum mixing: the viscosity and the bottom drag must be finite and >= 0");
    if (nuV != 0.0 || bottomDrag != 0.0) {
        if (int rc = mom_vmix_supported(st)) return rc;
        HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
        if (int rc = mom_vmix_scratch(st)) return rc;
    }
    st->momNuV = nuV; st->momDrag = bottomDrag;      // (kernel arguments of the next step's launch: nothing on the device changes)
    return MOKA_OK;
}

int moka_vertical_viscosity(const moka_state *st, double *nuV, double *bottomDrag)
{
    if (!st || !nuV || !bottomDrag) return fail(st ? st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    *nuV = st->momNuV; *bottomDrag = st->momDrag;
    return MOKA_OK;
}

int moka_surface_stress_upload(moka_state *st, const double *host)
{
    if (!st) return fail(nullptr, MOKA_ERR_ARG, "state is NULL");
    const Plan &p = st->mesh->plan;
    bool on = false;                     // the host scan: a nonzero entry at an edge with an active level
    for (int e = 0; host && e < p.nE; ++e) {
        const double v = host[p.edgeN2O[e]];
        if (!std::isfinite(v))
            return fail(st->ctx, MOKA_ERR_ARG, "surface stress: every value must be finite");
        on = on || (v != 0.0 && p.ehdr[(size_t)e * 4 + 3] >= 1 && p.K >= 1);
    }
    if (host)
        if (int rc = mom_vmix_supported(st)) return rc;
    if (st->forcedSteps > 0)             // the reverse pass reads the stress the recorded steps ran with, and G_tau is the gradient of one field
        return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "surface stress: not while a moka_forced_tape of this state holds recorded steps");
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    HIPCHK(st->ctx, hipStreamSynchronize(st->ctx->stream));      // no launch is reading the old array
    if (!host) {
        st->mem.release(st->momTau);
        st->momTauOn = false;
        return MOKA_OK;
    }
    if (on)
        if (int rc = mom_vmix_scratch(st)) return rc;
    double *fresh = nullptr;             // the new stress goes into an array of its own: a failure leaves the old one in force
    if (int rc = st->mem.alloc(&fresh, (size_t)p.nE)) return rc;
    if (int rc = put_rows(st->mesh, fresh, host, MOKA_EDGE, p.nE, 1)) {
        (void)hipStreamSynchronize(st->ctx->stream);
        st->mem.release(fresh);
        return rc;
    }
    st->mem.release(st->momTau);
    st->momTau = fresh; st->momTauOn = on;
    return MOKA_OK;
}

int moka_surface_stress_download(moka_state *st, double *host)
{
    if (!st || !host) return fail(st ? st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    const Plan &p = st->mesh->plan;
    if (!st->momTau) {
        std::fill(host, host + (size_t)p.nE, 0.0);
        return MOKA_OK;
    }
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    return get_rows(st->mesh, host, st->momTau, MOKA_EDGE, p.nE, 1);
}

int moka_has_surface_stress(const moka_state *st, int *out)
{
    if (!st || !out) return fail(st ? st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    *out = st->momTau ? 1 : 0;
    return MOKA_OK;
}

int moka_vertical_viscosity_field_upload(moka_state *st, const double *host)
{
    if (!st) return fail(nullptr, MOKA_ERR_ARG, "state is NULL");
    const Plan &p = st->mesh->plan;
    bool on = false;                     // the host scan: the interfaces k < n_e - 1 of every edge column, and nothing else
    for (int e = 0; host && e < p.nE; ++e) {
        const double *col = host + (size_t)p.edgeN2O[e] * p.K;
        const int n = std::min(p.ehdr[(size_t)e * 4 + 3], p.K);
        for (int k = 0; k < n - 1; ++k) {
            if (!(col[k] >= 0.0) || !std::isfinite(col[k]))
                return fail(st->ctx, MOKA_ERR_ARG, "vertical viscosity field: every value at an active interface must be finite and >= 0");
            on = on || col[k] != 0.0;
        }
    }
    if (!host && !st->momVf) return MOKA_OK;      // nothing to remove: the call of a state that never had a field does nothing at all
    // a removal lets the scalar act again: with nuV != 0 it asks for what moka_set_vertical_viscosity(nuV != 0) asks for (a field whose
    // active entries are all zero had set that nuV aside, and a moka_tape or a halo may have been created meanwhile)
    if (host || st->momNuV != 0.0)
        if (int rc = mom_vmix_supported(st)) return rc;
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    HIPCHK(st->ctx, hipStreamSynchronize(st->ctx->stream));      // no launch is reading the old array
    if (!host) {
        st->mem.release(st->momVf);
        st->momVfOn = false;
        ++st->momVfGen;
        return MOKA_OK;
    }
    if (on)
        if (int rc = mom_vmix_scratch(st)) return rc;
    double *fresh = nullptr;             // the new field goes into an array of its own: a failure leaves the old one in force
    if (int rc = st->mem.alloc(&fresh, (size_t)p.K * p.nE)) return rc;
    if (int rc = put_rows(st->mesh, fresh, host, MOKA_EDGE, p.nE, p.K)) {
        (void)hipStreamSynchronize(st->ctx->stream);
        st->mem.release(fresh);
        return rc;
    }
    st->mem.release(st->momVf);
    st->momVf = fresh; st->momVfOn = on;
    ++st->momVfGen;
    return MOKA_OK;
}

int moka_vertical_viscosity_field_download(moka_state *st, double *host)
{
    if (!st || !host) return fail(st ? st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    const Plan &p = st->mesh->plan;
    if (!st->momVf) {
        std::fill(host, host + (size_t)p.K * p.nE, 0.0);
        return MOKA_OK;
    }
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    return get_rows(st->mesh, host, st->momVf, MOKA_EDGE, p.nE, p.K);
}

int moka_has_vertical_viscosity_field(const moka_state *st, int *out)
{
    if (!st || !out) return fail(st ? st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    *out = st->momVf ? 1 : 0;
    return MOKA_OK;
}

// ---- the quadratic bottom drag (include/moka_hip.h: the recipe; momentum_vmix.hip: k_mvmix_bottom_speed and the QD instances) ----
int moka_set_quadratic_bottom_drag(moka_state *st, double cd)
{
    if (!st) return fail(nullptr, MOKA_ERR_ARG, "state is NULL");
    if (!(cd >= 0.0) || !std::isfinite(cd))
        return fail(st->ctx, MOKA_ERR_ARG, "vertical momentum mixing: the quadratic drag coefficient must be finite and >= 0");
    if (cd != 0.0) {
        if (int rc = mom_vmix_supported(st)) return rc;
        if (st->forcedPlainTapes > 0)     // (a tape of moka_forced_tape_create_quadratic carries Cd: it is counted in forcedTapes alone)
            return fail(st->ctx, MOKA_ERR_UNSUPPORTED,
                        "vertical momentum mixing: no quadratic drag while a moka_forced_tape of this state exists (reverse mode does not cover it)");
        HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
        if (int rc = mom_vmix_scratch(st)) return rc;
        if (int rc = ensure_ke_coef(st->mesh)) return rc;
        if (!st->momSpeed) {
            if (int rc = st->mem.alloc(&st->momSpeed, (size_t)st->mesh->plan.nE)) return rc;
            HIPCHK(st->ctx, hipStreamSynchronize(st->ctx->stream));
        }
    }
    st->momCd = cd;      // (a kernel argument of the next step's launches: moka_run captures its graph anew in every call)
    return MOKA_OK;
}

int moka_quadratic_bottom_drag(const moka_state *st, double *cd)
{
    if (!st || !cd) return fail(st ? st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    *cd = st->momCd;
    return MOKA_OK;
}

int moka_bottom_speed_download(moka_state *st, double *host)
{
    if (!st || !host) return fail(st ? st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    const Plan &p = st->mesh->plan;
    if (!st->momSpeed || !st->momSpeedUsed) {
        std::fill(host, host + (size_t)p.nE, 0.0);
        return MOKA_OK;
    }
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    return get_rows(st->mesh, host, st->momSpeed, MOKA_EDGE, p.nE, 1);
}

int moka_bottom_speed(moka_state *st, int time_level, double *host)
{
    if (!st || !host) return fail(st ? st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    const Plan &p = st->mesh->plan;
    if (time_level != 0 && time_level != 1) return fail(st->ctx, MOKA_ERR_ARG, "time_level must be 0 (previous) or 1 (current)");
    if (st->f32) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "bottom speed: Float64 states only");
    if (st->halos > 0 || p.nPatchesLaunch != p.nPatches) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "bottom speed: whole (unpartitioned) meshes only");
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    if (int rc = ensure_ke_coef(st->mesh)) return rc;
    if (int rc = ensure_op_bufs(st->mesh)) return rc;
    double *sp = st->mesh->opBuf[0];         // operator scratch; get_rows stages through opBuf[2]
    HIPCHK(st->ctx, launch_momentum_bottom_speed(bottom_speed_args(st, st->lev[time_level].u, sp), st->ctx->stream));
    return get_rows(st->mesh, host, sp, MOKA_EDGE, p.nE, 1);
}

int moka_state_momentum_vmix_path(const moka_state *st) { return st ? st->momVmixPath : 0; }

}  // extern "C"
