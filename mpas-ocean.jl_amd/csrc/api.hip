// api.hip -- C ABI of libmoka_hip.so (include/moka_hip.h): context, device mesh, state, steps.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <unordered_set>
#include <utility>
#include <vector>

#include <mutex>
#include <unordered_set>

#include "state.hpp"

namespace moka {

void fill_mesh_info(const Plan &p, moka_mesh_info *info);

// Process-wide launch-shape switches (moka_set_tuning / moka_get_tuning; include/moka_hip.h lists the keys, kernels.hpp names them):
// the default, and either a bit mask whose bits each name kernel instances (mask != 0) or the largest value accepted (from 0).
struct TuningEntry {
    int mask, max;
    std::atomic<int> value;
    TuningEntry(int def, int m, int x) : mask(m), max(x), value(def) {}
    bool accepts(int v) const { return mask ? (v & ~mask) == 0 : v >= 0 && v <= max; }
};
static TuningEntry g_tuning[] = {
    {0, 0, -1},                                              // (no key 0)
    {1 << 0, 0x7f | 1 << 10 | 1 << 11, 0},                   // 1 TUNE_F32_WIDE: fp32 modes 0-6, lean 10 / 11 (launch_rec2c_f32)
    {1, 0, 1},                                               // 2 TUNE_FE_PREV
    {1, 0, 1},                                               // 3 TUNE_CURL_FUSED
    {1, 0, 1},                                               // 4 TUNE_FE_LEAN
    {0, 0, 3},                                               // 5 TUNE_NL_SHAPE: shapes 0-3 (nl_stage_kernel)
    {0, 0, INT_MAX},                                         // 6 TUNE_NL_CAP: vertex rows, 0 = no limit
    {0, 0, 1},                                               // 7 TUNE_RK13
    {1 << 0 | 1 << 1 | 1 << 7, 0xf | 7 << 7 | 1 << 16, 0},   // 8 TUNE_PAIR: pair instances 0-3, 7-9; bit 16 test hook (launch_rec2c_pair)
    {1, 0, 1},                                               // 9 TUNE_FE_LEAN_INST
};
constexpr int N_TUNING = sizeof(g_tuning) / sizeof(g_tuning[0]);

int tuning(TuningKey key) { return g_tuning[key].value.load(); }

}  // namespace moka

namespace mk {

static std::mutex g_liveMutex;
static std::unordered_set<const moka_state *> g_liveStates;
void state_attach(moka_state *st, bool halo)
{
    std::lock_guard<std::mutex> lk(g_liveMutex);
    if (g_liveStates.count(st)) { ++st->attached; st->halos += halo; }
}
void state_detach(moka_state *st, bool halo)
{
    std::lock_guard<std::mutex> lk(g_liveMutex);
    if (g_liveStates.count(st)) { --st->attached; st->halos -= halo; }
}

int fail(moka_ctx *ctx, int code, const std::string &msg)
{
    set_error(msg);
    if (ctx) ctx->err = msg;
    return code;
}

int lanes_per_column(int K)
{
    int l = 1;
    while (l < K && l < 64) l <<= 1;
    return l;
}

// Rule of this file: no null-stream hipMemcpy / hipMemset after context creation.  The context's streams are non-blocking,
// i.e. NOT ordered against the null stream, so a null-stream copy can overtake (or be overtaken by) a hipMemsetAsync queued
// on the context stream (the tape-list race of round 1).  Every host->device copy goes through h2d(): on the context's
// stream, then synchronised (the source is usually a temporary).  tools/check_streams.sh greps for offenders.
int h2d(moka_ctx *ctx, void *dst, const void *src, size_t bytes)
{
    if (!bytes) return MOKA_OK;
    HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return MOKA_OK;
}

template <class T>
int upload_vec(moka_mesh *m, const std::vector<T> &v, const T **out)
{
    void *d = nullptr;
    const size_t bytes = std::max<size_t>(v.size() * sizeof(T), 16);
    HIPCHK(m->ctx, hipMalloc(&d, bytes));
    m->allocs.push_back(d);
    if (int rc = h2d(m->ctx, d, v.data(), v.size() * sizeof(T))) return rc;
    *out = static_cast<const T *>(d);
    return MOKA_OK;
}

int ensure_op_bufs(moka_mesh *m)
{
    const Plan &p = m->plan;
    const size_t need = (size_t)p.K * std::max(p.nE, std::max(p.nC, p.nV));
    if (m->opBufElems >= need) return MOKA_OK;
    for (auto &b : m->opBuf) {
        if (b) HIPCHK(m->ctx, hipFree(b));
        b = nullptr;
    }
    for (auto &b : m->opBuf) HIPCHK(m->ctx, hipMalloc((void **)&b, need * sizeof(double)));
    m->opBufElems = need;
    return MOKA_OK;
}

int alloc_field(moka_state *st, double **out, size_t elems, size_t elemBytes)
{
    void *d = nullptr;
    HIPCHK(st->ctx, hipMalloc(&d, std::max<size_t>(elems * elemBytes, 16)));
    st->allocs.push_back(d);
    HIPCHK(st->ctx, hipMemsetAsync(d, 0, elems * elemBytes, st->ctx->stream));   // KA.zeros
    *out = static_cast<double *>(d);
    return MOKA_OK;
}

int ensure_rk_bufs(moka_state *st)
{
    if (st->rk[1].ssh) return MOKA_OK;       // the last of the six: set only when all of them exist
    const Plan &p = st->mesh->plan;
    LevelBufs tmp[2];
    const size_t mark = st->allocs.size();
    const size_t sb = st->f32 ? 4 : 8;
    int rc = MOKA_OK;
    for (auto &r : tmp) {
        if (rc == MOKA_OK) rc = alloc_field(st, &r.u, (size_t)p.K * p.nE, sb);
        if (rc == MOKA_OK) rc = alloc_field(st, &r.h, (size_t)p.K * p.nC, sb);
        if (rc == MOKA_OK) rc = alloc_field(st, &r.ssh, (size_t)p.nC, sb);
    }
    if (rc != MOKA_OK) {                     // free what a partial failure left behind: a later call starts over
        (void)hipStreamSynchronize(st->ctx->stream);
        while (st->allocs.size() > mark) { (void)hipFree(st->allocs.back()); st->allocs.pop_back(); }
        return rc;
    }
    st->rk[0] = tmp[0]; st->rk[1] = tmp[1];
    st->phys[2] = tmp[0]; st->phys[3] = tmp[1];
    return MOKA_OK;
}

int ensure_spare(moka_state *st)
{
    if (st->spare.ssh) return MOKA_OK;
    const Plan &p = st->mesh->plan;
    LevelBufs tmp;
    const size_t mark = st->allocs.size();
    const size_t sb = st->f32 ? 4 : 8;
    int rc = alloc_field(st, &tmp.u, (size_t)p.K * p.nE, sb);
    if (rc == MOKA_OK) rc = alloc_field(st, &tmp.h, (size_t)p.K * p.nC, sb);
    if (rc == MOKA_OK) rc = alloc_field(st, &tmp.ssh, (size_t)p.nC, sb);
    if (rc != MOKA_OK) {
        (void)hipStreamSynchronize(st->ctx->stream);
        while (st->allocs.size() > mark) { (void)hipFree(st->allocs.back()); st->allocs.pop_back(); }
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

const int32_t *perm_of(const moka_mesh *m, int kind)
{
    return kind == MOKA_CELL ? m->dev.cellN2O : kind == MOKA_EDGE ? m->dev.edgeN2O : m->dev.vertN2O;
}

// host (caller numbering) -> device field (device numbering)
int put_rows(moka_mesh *m, double *dst, const double *host, int kind, int64_t n, int K, bool f32 = false)
{
    int rc = ensure_op_bufs(m);
    if (rc) return rc;
    hipStream_t s = m->ctx->stream;
    HIPCHK(m->ctx, hipMemcpyAsync(m->opBuf[2], host, (size_t)n * K * sizeof(double), hipMemcpyHostToDevice, s));
    if (f32) HIPCHK(m->ctx, launch_permute_rows_f32(dst, m->opBuf[2], perm_of(m, kind), n, K, 1, s));   // rounds to fp32
    else HIPCHK(m->ctx, launch_permute_rows(dst, m->opBuf[2], perm_of(m, kind), n, K, 1, s));
    HIPCHK(m->ctx, hipStreamSynchronize(s));
    return MOKA_OK;
}

int get_rows(moka_mesh *m, double *host, const double *src, int kind, int64_t n, int K, bool f32 = false)
{
    int rc = ensure_op_bufs(m);
    if (rc) return rc;
    hipStream_t s = m->ctx->stream;
    if (f32) HIPCHK(m->ctx, launch_permute_rows_f32(m->opBuf[2], src, perm_of(m, kind), n, K, 0, s));
    else HIPCHK(m->ctx, launch_permute_rows(m->opBuf[2], src, perm_of(m, kind), n, K, 0, s));
    HIPCHK(m->ctx, hipMemcpyAsync(host, m->opBuf[2], (size_t)n * K * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(m->ctx, hipStreamSynchronize(s));
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

}  // namespace mk

using namespace mk;

extern "C" {

const char *moka_version(void) { return "moka-hip 0.1.0 (gfx950)"; }

const char *moka_last_error(const moka_ctx *ctx) { return ctx ? ctx->err.c_str() : moka::get_error(); }

int moka_ctx_create(int device, moka_ctx **out)
{
    if (!out) return fail(nullptr, MOKA_ERR_ARG, "out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, MOKA_ERR_NO_DEVICE,
                    std::string("no HIP device available (libmoka_hip has no CPU fallback): ") +
                        (e != hipSuccess ? hipGetErrorString(e) : "device count is 0"));
    if (device < 0 || device >= ndev) return fail(nullptr, MOKA_ERR_ARG, "device index out of range");
    HIPCHK(nullptr, hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(nullptr, hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, MOKA_ERR_NO_DEVICE,
                    std::string("device is ") + prop.gcnArchName + ", this library carries gfx950 code objects only");
    moka_ctx *c = new (std::nothrow) moka_ctx();
    if (!c) return fail(nullptr, MOKA_ERR_ALLOC, "out of host memory");
    c->device = device;
    c->nCUs = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    hipError_t e1 = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    hipError_t e2 = hipEventCreate(&c->ev0);
    hipError_t e3 = hipEventCreate(&c->ev1);
    if (e1 == hipSuccess) {
        // the comm stream carries the boundary patches, pack / unpack and the halo transport: highest priority, so that its
        // few workgroups are dispatched ahead of the thousands the interior launch has queued
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        e1 = hipStreamCreateWithPriority(&c->comm, hipStreamNonBlocking, hi);
    }
    if (e2 == hipSuccess) e2 = hipEventCreateWithFlags(&c->evBoundary, hipEventDisableTiming);
    if (e2 == hipSuccess) e2 = hipEventCreateWithFlags(&c->evInterior, hipEventDisableTiming);
    if (e3 == hipSuccess) e3 = hipEventCreateWithFlags(&c->evHalo, hipEventDisableTiming);
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) {
        moka_ctx_destroy(c);                  // destroys whatever was created
        return fail(nullptr, MOKA_ERR_HIP, "failed to create stream/events");
    }
    *out = c;
    return MOKA_OK;
}

void moka_ctx_destroy(moka_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->comm) { (void)hipStreamSynchronize(ctx->comm); (void)hipStreamDestroy(ctx->comm); }
    for (hipEvent_t e : {ctx->evBoundary, ctx->evInterior, ctx->evHalo}) if (e) (void)hipEventDestroy(e);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    for (hipEvent_t e : ctx->evPool) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->marks) (void)hipEventDestroy(e);
    if (ctx->bwBuf) (void)hipFree(ctx->bwBuf);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int moka_sync(moka_ctx *ctx)
{
    if (!ctx) return fail(nullptr, MOKA_ERR_ARG, "ctx is NULL");
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->comm));
    return MOKA_OK;
}

int moka_ctx_streams(moka_ctx *ctx, void **compute, void **comm)
{
    if (!ctx) return fail(nullptr, MOKA_ERR_ARG, "ctx is NULL");
    if (compute) *compute = (void *)ctx->stream;
    if (comm) *comm = (void *)ctx->comm;
    return MOKA_OK;
}

int moka_timer_start(moka_ctx *ctx)
{
    if (!ctx) return fail(nullptr, MOKA_ERR_ARG, "ctx is NULL");
    HIPCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    return MOKA_OK;
}

int moka_timer_stop(moka_ctx *ctx, float *elapsed_ms)
{
    if (!ctx || !elapsed_ms) return fail(ctx, MOKA_ERR_ARG, "NULL argument");
    HIPCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    HIPCHK(ctx, hipEventSynchronize(ctx->ev1));
    HIPCHK(ctx, hipEventElapsedTime(elapsed_ms, ctx->ev0, ctx->ev1));
    return MOKA_OK;
}

// PCI bus id ("0000:c5:00.0") of the context's device: lets a caller find the device's clock / power files in sysfs
// (/sys/bus/pci/devices/<id>/pp_dpm_sclk ...) and count distinct devices among the ranks of a launch.
int moka_ctx_pci_bus_id(moka_ctx *ctx, char *buf, int32_t len)
{
    if (!ctx || !buf || len < 16) return fail(ctx, MOKA_ERR_ARG, "buf is NULL or shorter than 16 bytes");
    HIPCHK(ctx, hipDeviceGetPCIBusId(buf, len, ctx->device));
    return MOKA_OK;
}

// Per-step statistics of a timed region (bench.py: median / min / max of the step times).  moka_mark records one event on the
// compute stream; n marks give n - 1 intervals.  moka_marks_reset forgets them (the events are kept for reuse).
int moka_mark(moka_ctx *ctx)
{
    if (!ctx) return fail(nullptr, MOKA_ERR_ARG, "ctx is NULL");
    if (ctx->marksUsed == ctx->marks.size()) {
        hipEvent_t e = nullptr;
        HIPCHK(ctx, hipEventCreate(&e));
        ctx->marks.push_back(e);
    }
    HIPCHK(ctx, hipEventRecord(ctx->marks[ctx->marksUsed++], ctx->stream));
    return MOKA_OK;
}

int moka_marks_reset(moka_ctx *ctx)
{
    if (!ctx) return fail(nullptr, MOKA_ERR_ARG, "ctx is NULL");
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->marksUsed = 0;
    return MOKA_OK;
}

// ms[i] = time between mark i and mark i + 1 (at most `capacity` intervals); *n = number of intervals available
int moka_marks_read(moka_ctx *ctx, int64_t capacity, double *ms, int64_t *n)
{
    if (!ctx || !n || (capacity > 0 && !ms)) return fail(ctx, MOKA_ERR_ARG, "NULL argument");
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const int64_t have = ctx->marksUsed > 0 ? (int64_t)ctx->marksUsed - 1 : 0;
    *n = have;
    for (int64_t i = 0; i < have && i < capacity; ++i) {
        float t = 0.f;
        HIPCHK(ctx, hipEventElapsedTime(&t, ctx->marks[i], ctx->marks[i + 1]));
        ms[i] = t;
    }
    return MOKA_OK;
}

// Same-run bandwidth calibration: what this device, in the state it is in NOW, moves with a plain 16-byte-per-lane copy and a
// read-only sweep (MI355X_MICROARCH.md quotes 6.29 TB/s for the copy).  `bytes` = total footprint (two halves: source and
// destination); every launch is timed on its own with HIP events on the compute stream, the best of `iters` is reported
// (the first launch also faults the pages in).  gbs[0] = copy, bytes read + written per second; gbs[1] = read-only sweep of both
// halves; gbs[2] = mean copy rate over the launches; gbs[3] = gather of 480-byte rows in a scattered order, a half-wave per
// row (the access pattern of the stage kernels at 60 layers).  bytes = 0 releases the buffers.
int moka_bw_probe(moka_ctx *ctx, int64_t bytes, int iters, double gbs[4])
{
    if (!ctx) return fail(nullptr, MOKA_ERR_ARG, "ctx is NULL");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (bytes <= 0) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->bwBuf) HIPCHK(ctx, hipFree(ctx->bwBuf));
        ctx->bwBuf = nullptr; ctx->bwBytes = 0;
        return MOKA_OK;
    }
    if (!gbs || iters < 1) return fail(ctx, MOKA_ERR_ARG, "gbs is NULL or iters < 1");
    const size_t half = ((size_t)bytes / 2) & ~(size_t)4095;
    if (half < ((size_t)1 << 20)) return fail(ctx, MOKA_ERR_ARG, "bandwidth probe: at least 2 MiB");
    hipStream_t s = ctx->stream;
    if (ctx->bwBytes != 2 * half) {
        if (ctx->bwBuf) { HIPCHK(ctx, hipStreamSynchronize(s)); HIPCHK(ctx, hipFree(ctx->bwBuf)); ctx->bwBuf = nullptr; ctx->bwBytes = 0; }
        hipError_t e = hipMalloc(&ctx->bwBuf, 2 * half + 64);
        if (e != hipSuccess) return fail(ctx, MOKA_ERR_ALLOC, std::string("bandwidth probe: hipMalloc: ") + hipGetErrorString(e));
        ctx->bwBytes = 2 * half;
        HIPCHK(ctx, hipMemsetAsync(ctx->bwBuf, 0x5A, 2 * half + 64, s));
    }
    unsigned char *a = static_cast<unsigned char *>(ctx->bwBuf), *b = a + half;
    uint32_t *sink = reinterpret_cast<uint32_t *>(a + 2 * half);
    double bestCopy = 0.0, bestRead = 0.0, sumCopy = 0.0, bestGather = 0.0;
    const uint32_t rowB = 480;
    for (int pass = 0; pass < 3; ++pass)
        for (int i = 0; i < iters; ++i) {
            HIPCHK(ctx, hipEventRecord(ctx->ev0, s));
            if (pass == 0) HIPCHK(ctx, launch_bw_copy(b, a, (int64_t)half, ctx->nCUs, s));
            else if (pass == 1) HIPCHK(ctx, launch_bw_read(a, (int64_t)(2 * half), sink, ctx->nCUs, s));
            else HIPCHK(ctx, launch_bw_gather(a, (int64_t)(2 * half), rowB, sink, ctx->nCUs, s));
            HIPCHK(ctx, hipEventRecord(ctx->ev1, s));
            HIPCHK(ctx, hipEventSynchronize(ctx->ev1));
            float ms = 0.f;
            HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
            const double r = (double)(2 * half) / ((double)ms * 1e-3) / 1e9;
            if (pass == 0) { bestCopy = std::max(bestCopy, r); sumCopy += r; }
            else if (pass == 1) bestRead = std::max(bestRead, r);
            else bestGather = std::max(bestGather, (double)((2 * half) / rowB * rowB) / ((double)ms * 1e-3) / 1e9);
        }
    gbs[0] = bestCopy; gbs[1] = bestRead; gbs[2] = sumCopy / iters; gbs[3] = bestGather;
    return MOKA_OK;
}

// A fifth figure for the same calibration: three streams read and two written at once (k_bw_streams) over the buffer moka_bw_probe
// allocated (call that first); GB/s of all five, best of `iters` launches.
int moka_bw_probe_streams(moka_ctx *ctx, int iters, double *gbs)
{
    if (!ctx || !gbs || iters < 1) return fail(ctx, MOKA_ERR_ARG, "NULL argument or iters < 1");
    if (!ctx->bwBuf || ctx->bwBytes < ((size_t)5 << 20)) return fail(ctx, MOKA_ERR_ARG, "moka_bw_probe first: it owns the buffer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int64_t n = (int64_t)(ctx->bwBytes / 5 / 16);
    double best = 0.0;
    for (int i = 0; i < iters; ++i) {
        HIPCHK(ctx, hipEventRecord(ctx->ev0, s));
        HIPCHK(ctx, launch_bw_streams(ctx->bwBuf, (int64_t)ctx->bwBytes, s));
        HIPCHK(ctx, hipEventRecord(ctx->ev1, s));
        HIPCHK(ctx, hipEventSynchronize(ctx->ev1));
        float ms = 0.f;
        HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        best = std::max(best, (double)(5 * 16 * n) / ((double)ms * 1e-3) / 1e9);
    }
    // the probes XOR the pattern away: restore it, the read probe's sentinel test relies on it
    HIPCHK(ctx, hipMemsetAsync(ctx->bwBuf, 0x5A, ctx->bwBytes + 64, s));
    *gbs = best;
    return MOKA_OK;
}

// A sixth figure: `region` bytes (more than the 32 MB of L2s, less than the 256 MB Infinity Cache: 128 MiB) read `reps` times back
// to back, GB/s over all passes, best of `iters` -- the rate at which re-read data comes back.  The stage kernels fetch a fifth
// to a quarter of their bytes a second time (rows of neighbouring patches, profiles/r03_traffic_attribution.txt); the streaming
// probes above never read anything twice.
int moka_bw_probe_reread(moka_ctx *ctx, int64_t region, int reps, int iters, double *gbs)
{
    if (!ctx || !gbs || iters < 1 || reps < 1) return fail(ctx, MOKA_ERR_ARG, "NULL argument or iters / reps < 1");
    if (!ctx->bwBuf || region < ((int64_t)1 << 20) || (size_t)region > ctx->bwBytes) return fail(ctx, MOKA_ERR_ARG, "moka_bw_probe first: it owns the buffer (region must fit it)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    unsigned char *a = static_cast<unsigned char *>(ctx->bwBuf);
    uint32_t *sink = reinterpret_cast<uint32_t *>(a + ctx->bwBytes);
    region &= ~(int64_t)4095;
    double best = 0.0;
    HIPCHK(ctx, launch_bw_read(a, region, sink, ctx->nCUs, s));          // first touch: from HBM
    for (int i = 0; i < iters; ++i) {
        HIPCHK(ctx, hipEventRecord(ctx->ev0, s));
        for (int r = 0; r < reps; ++r) HIPCHK(ctx, launch_bw_read(a, region, sink, ctx->nCUs, s));
        HIPCHK(ctx, hipEventRecord(ctx->ev1, s));
        HIPCHK(ctx, hipEventSynchronize(ctx->ev1));
        float ms = 0.f;
        HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        best = std::max(best, (double)region * reps / ((double)ms * 1e-3) / 1e9);
    }
    *gbs = best;
    return MOKA_OK;
}

// A seventh: the scattered row gather over a LARGE footprint of its own (`bytes`, e.g. 32 GiB: what a state with all its arrays
// spans), a quarter of the rows fetched once each -- consecutive half-waves land ~19 MB apart, so nearly every fetch needs an
// address translation the TLBs do not hold.  The 4 GiB gather of moka_bw_probe fits them.
int moka_bw_probe_gather_big(moka_ctx *ctx, int64_t bytes, int iters, double *gbs)
{
    if (!ctx || !gbs || iters < 1 || bytes < ((int64_t)1 << 24)) return fail(ctx, MOKA_ERR_ARG, "NULL argument, iters < 1 or less than 16 MiB");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    void *buf = nullptr;
    hipError_t e = hipMalloc(&buf, (size_t)bytes + 64);
    if (e != hipSuccess) return fail(ctx, MOKA_ERR_ALLOC, std::string("big gather probe: hipMalloc: ") + hipGetErrorString(e));
    const uint32_t rowB = 480;
    const int64_t nRows = bytes / rowB, nFetch = nRows / 4;
    uint32_t *sink = reinterpret_cast<uint32_t *>(static_cast<unsigned char *>(buf) + bytes);
    double best = 0.0;
    hipError_t rc = hipMemsetAsync(buf, 0x5A, (size_t)bytes + 64, s);
    for (int i = 0; i < iters && rc == hipSuccess; ++i) {
        if ((rc = hipEventRecord(ctx->ev0, s)) != hipSuccess) break;
        if ((rc = launch_bw_gather_n(buf, nRows, rowB, nFetch, sink, ctx->nCUs, s)) != hipSuccess) break;
        if ((rc = hipEventRecord(ctx->ev1, s)) != hipSuccess) break;
        if ((rc = hipEventSynchronize(ctx->ev1)) != hipSuccess) break;
        float ms = 0.f;
        if ((rc = hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1)) != hipSuccess) break;
        best = std::max(best, (double)nFetch * rowB / ((double)ms * 1e-3) / 1e9);
    }
    (void)hipStreamSynchronize(s);
    (void)hipFree(buf);
    HIPCHK(ctx, rc);
    *gbs = best;
    return MOKA_OK;
}

int moka_set_tuning(int key, int value)
{
    if (key < 1 || key >= N_TUNING) return fail(nullptr, MOKA_ERR_ARG, "unknown tuning key");
    if (!g_tuning[key].accepts(value)) return fail(nullptr, MOKA_ERR_ARG, "tuning key " + std::to_string(key) + ": value names no kernel instance");
    g_tuning[key].value.store(value);
    return MOKA_OK;
}

int moka_get_tuning(int key, int *value)
{
    if (!value) return fail(nullptr, MOKA_ERR_ARG, "value is NULL");
    if (key < 1 || key >= N_TUNING) return fail(nullptr, MOKA_ERR_ARG, "unknown tuning key");
    *value = g_tuning[key].value.load();
    return MOKA_OK;
}

int moka_kernel_variant_available(int variant)
{
    return variant == 0 || variant == 3 || variant == 4 || variant == 11;
}

int moka_set_kernel_variant(moka_ctx *ctx, int variant)
{
    if (!ctx) return fail(nullptr, MOKA_ERR_ARG, "ctx is NULL");
    if (variant < 0 || variant > 14) return fail(ctx, MOKA_ERR_ARG, "variant must be 0..14");
    if (!moka_kernel_variant_available(variant))
        return fail(ctx, MOKA_ERR_UNSUPPORTED, "this kernel variant was an experiment of rounds 1-3 and no longer exists (0, 3, 4, 11 do)");
    ctx->variant = variant;
    return MOKA_OK;
}

// ---------------------------------------------------------------------------------------------
// mesh
// ---------------------------------------------------------------------------------------------
int moka_mesh_create(moka_ctx *ctx, const moka_mesh_desc *desc, moka_mesh **out)
{
    if (!ctx || !out) return fail(ctx, MOKA_ERR_ARG, "NULL argument");
    *out = nullptr;
    moka_mesh *m = new (std::nothrow) moka_mesh();
    if (!m) return fail(ctx, MOKA_ERR_ALLOC, "out of host memory");
    m->ctx = ctx;
    int rc;
    try {
        rc = build_plan(desc, m->plan);
    } catch (const std::bad_alloc &) {
        rc = fail(ctx, MOKA_ERR_ALLOC, "out of host memory while building the mesh plan");
    }
    if (rc != MOKA_OK) {
        ctx->err = moka::get_error();
        delete m;
        return rc;
    }
    const Plan &p = m->plan;
    if (p.ME > 8 || p.ME2 > 14) {
        delete m;
        return fail(ctx, MOKA_ERR_UNSUPPORTED, "cells with more than 8 edges are not supported by the gfx950 kernels");
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    MeshDev &d = m->dev;
    d.nC = p.nC; d.nE = p.nE; d.nV = p.nV; d.K = p.K; d.ME = p.ME; d.ME2 = p.ME2; d.VD = p.VD; d.nPatches = p.nPatches;
    d.tailPatch = -1;      // no extra patch rides in a launch of this view (0, the zero-initialised value, would name patch 0: a
                           // whole-mesh Forward-Euler launch then ran patch 0 twice -- harmless while every result was a pure
                           // function of the inputs, wrong once relativeVorticity accumulates in the same launch)
    m->lpc = lanes_per_column(p.K);
#define UP(field)                                                \
    if ((rc = upload_vec(m, p.field, &d.field)) != MOKA_OK) {    \
        moka_mesh_destroy(m);                                    \
        return rc;                                               \
    }
    UP(patchCellStart) UP(patchEdgeStart) UP(patchVertStart)
    UP(eoc) UP(coc) UP(mltc) UP(sdv) UP(invArea) UP(areaCell) UP(rsum)
    UP(ehdr) UP(eoe) UP(woe) UP(gInvDc) UP(dcEdge) UP(dvEdge) UP(fEdge)
    UP(eov) UP(cv) UP(cellN2O) UP(edgeN2O) UP(vertN2O)
    UP(leoe) UP(cRec) UP(eRec) UP(feoe) UP(vRec) UP(rowStart) UP(rowEdge)
    if (p.nlOk) { UP(voe) UP(cov) UP(kite) UP(invAreaTri) UP(fVertex) UP(keCoef) UP(invDc) UP(keoc) UP(rowVoe) }
    if (p.nl5Ok) { UP(pvStart) UP(pvList) UP(lvoe) }
#undef UP
    d.maxPV = p.nl5Ok ? p.maxPV : 0;
    if (!p.nl5Ok) { d.pvStart = nullptr; d.pvList = nullptr; d.lvoe = nullptr; }
    d.CI = p.CI; d.EI = p.EI;
    m->colOk = p.colOk;

    d.maxRows = p.maxRows; d.maxOwnE = p.maxOwnE; d.maxOwnC = p.maxOwnC;
    d.maxOwnV = p.maxOwnV;
    if (p.vRec.empty()) d.vRec = nullptr;       // (upload_vec hands out a dummy allocation for an empty vector)
    *out = m;
    return MOKA_OK;
}

void moka_mesh_destroy(moka_mesh *mesh)
{
    if (!mesh) return;
    (void)hipSetDevice(mesh->ctx->device);
    (void)hipStreamSynchronize(mesh->ctx->stream);
    for (void *q : mesh->allocs) (void)hipFree(q);
    for (auto b : mesh->opBuf)
        if (b) (void)hipFree(b);
    delete mesh;
}

int moka_mesh_permutation(const moka_mesh *mesh, int kind, int32_t *new_to_old)
{
    if (!mesh || !new_to_old) return fail(nullptr, MOKA_ERR_ARG, "NULL argument");
    const Plan &p = mesh->plan;
    const std::vector<int32_t> *v = kind == MOKA_CELL ? &p.cellN2O : kind == MOKA_EDGE ? &p.edgeN2O : kind == MOKA_VERTEX ? &p.vertN2O : nullptr;
    if (!v) return fail(mesh->ctx, MOKA_ERR_ARG, "kind must be MOKA_CELL, MOKA_EDGE or MOKA_VERTEX");
    std::copy(v->begin(), v->end(), new_to_old);
    return MOKA_OK;
}

int moka_mesh_class_ranges(const moka_mesh *mesh, int32_t capacity, int32_t *nClasses, int32_t *patchStart, int32_t *cellStart,
                           int32_t *edgeStart)
{
    if (!mesh || !nClasses) return fail(nullptr, MOKA_ERR_ARG, "NULL argument");
    const Plan &p = mesh->plan;
    const int n = (int)p.classPatchStart.size() - 1;
    *nClasses = n;
    for (int k = 0; k <= n && k < capacity; ++k) {
        if (patchStart) patchStart[k] = p.classPatchStart[k];
        if (cellStart) cellStart[k] = p.classCellStart[k];
        if (edgeStart) edgeStart[k] = p.classEdgeStart[k];
    }
    return MOKA_OK;
}

int moka_mesh_info_get(const moka_mesh *mesh, moka_mesh_info *info)
{
    if (!mesh || !info) return fail(nullptr, MOKA_ERR_ARG, "NULL argument");
    fill_mesh_info(mesh->plan, info);
    return MOKA_OK;
}

// ---------------------------------------------------------------------------------------------
// operators on host arrays
// ---------------------------------------------------------------------------------------------
static int run_operator(moka_mesh *m, int op, int nlev, const double *in, int inKind, double *out, int outKind,
                        bool out_is_inout)
{
    if (!m || !in || !out) return fail(m ? m->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    const Plan &p = m->plan;
    auto count = [&](int kind) -> int64_t { return kind == MOKA_CELL ? p.nC : kind == MOKA_EDGE ? p.nE : p.nV; };
    int rc = ensure_op_bufs(m);
    if (rc) return rc;
    hipStream_t s = m->ctx->stream;
    HIPCHK(m->ctx, hipSetDevice(m->ctx->device));
    if ((rc = put_rows(m, m->opBuf[0], in, inKind, count(inKind), p.K))) return rc;
    if (out_is_inout) {
        if ((rc = put_rows(m, m->opBuf[1], out, outKind, count(outKind), p.K))) return rc;
    } else {
        // untouched levels (interpolate, nlev < K) must come back as the caller had them
        if (op == OP_INTERP && nlev < p.K) {
            if ((rc = put_rows(m, m->opBuf[1], out, outKind, count(outKind), p.K))) return rc;
        }
    }
    OpArgs a{op, nlev, m->opBuf[0], m->opBuf[1]};
    HIPCHK(m->ctx, launch_operator(m->dev, a, m->lpc, s));
    return get_rows(m, out, m->opBuf[1], outKind, count(outKind), p.K);
}

int moka_gradient_on_edge(moka_mesh *mesh, const double *scalarCell, double *gradEdge)
{
    return run_operator(mesh, OP_GRADIENT, 0, scalarCell, MOKA_CELL, gradEdge, MOKA_EDGE, false);
}

int moka_interpolate_cell2edge(moka_mesh *mesh, const double *cellValue, double *edgeValue, int nlev)
{
    if (mesh && (nlev < 1 || nlev > mesh->plan.K)) return fail(mesh->ctx, MOKA_ERR_ARG, "nlev out of range");
    return run_operator(mesh, OP_INTERP, nlev, cellValue, MOKA_CELL, edgeValue, MOKA_EDGE, false);
}

int moka_curl_on_vertex(moka_mesh *mesh, const double *vecEdge, double *curlVertex)
{
    return run_operator(mesh, OP_CURL, 0, vecEdge, MOKA_EDGE, curlVertex, MOKA_VERTEX, true);
}

// ---------------------------------------------------------------------------------------------
// reverse and forward mode of the stand-alone operators (test/enzyme/test_Enzyme_Operators.jl:42-131, 137-225).
// The operators are linear: forward mode is the operator applied to the tangent, reverse mode its transpose applied to the
// cotangent.  Shadow conventions are Enzyme's for in-place kernels with Duplicated arguments: the shadow of an input is
// accumulated into, the shadow of an output the kernel overwrites is zero afterwards, the shadow of the (accumulated-into)
// curl output stays.  Transposes are gathers with a fixed order (oracle twins: oracle_*_vjp).
// ---------------------------------------------------------------------------------------------
static int ensure_op_transposes(moka_mesh *m)
{
    if (m->opESign) return MOKA_OK;
    const Plan &p = m->plan;
    std::vector<std::vector<std::pair<std::pair<int32_t, int32_t>, int32_t>>> lists(p.nE);     // ((caller's vertex, slot), new vertex)
    for (int v = 0; v < p.nV; ++v)
        for (int j = 0; j < p.VD; ++j) {
            const int e = p.eov[(size_t)v * p.VD + j];
            if (e >= 0) lists[e].push_back({{p.vertN2O[v], j}, v});
        }
    int W = 1;
    for (auto &l : lists) { std::sort(l.begin(), l.end()); W = std::max(W, (int)l.size()); }
    std::vector<int32_t> tv((size_t)p.nE * W, -1);
    std::vector<double> tc((size_t)p.nE * W, 0.0), es((size_t)p.nE * 2, 0.0);
    for (int e = 0; e < p.nE; ++e) {
        for (size_t q = 0; q < lists[e].size(); ++q) {
            const int v = lists[e][q].second, j = lists[e][q].first.second;
            tv[(size_t)e * W + q] = v;
            tc[(size_t)e * W + q] = p.cv[(size_t)v * p.VD + j];
        }
        for (int q = 0; q < 2; ++q) {
            const int c = p.ehdr[(size_t)e * 4 + q];
            for (int i = 0; i < p.ME; ++i)
                if (p.eoc[(size_t)c * p.ME + i] == e) { es[(size_t)e * 2 + q] = p.sdv[(size_t)c * p.ME + i] < 0.0 ? -1.0 : 1.0; break; }
        }
    }
    int rc;
    if ((rc = upload_vec(m, tv, &m->opTVert)) || (rc = upload_vec(m, tc, &m->opTCoef))) return rc;
    if ((rc = upload_vec(m, es, &m->opESign))) return rc;
    m->opTW = W;
    return MOKA_OK;
}

int moka_gradient_on_edge_vjp(moka_mesh *m, double *dGradEdge, double *dScalarCell)
{
    if (!m || !dGradEdge || !dScalarCell) return fail(m ? m->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    const Plan &p = m->plan;
    int rc = ensure_op_bufs(m);
    if (rc) return rc;
    HIPCHK(m->ctx, hipSetDevice(m->ctx->device));
    if ((rc = put_rows(m, m->opBuf[0], dGradEdge, MOKA_EDGE, p.nE, p.K))) return rc;
    if ((rc = put_rows(m, m->opBuf[1], dScalarCell, MOKA_CELL, p.nC, p.K))) return rc;
    OpArgs a{OP_GRAD_T, 0, m->opBuf[0], m->opBuf[1]};
    HIPCHK(m->ctx, launch_operator(m->dev, a, m->lpc, m->ctx->stream));
    if ((rc = get_rows(m, dScalarCell, m->opBuf[1], MOKA_CELL, p.nC, p.K))) return rc;
    std::memset(dGradEdge, 0, sizeof(double) * (size_t)p.K * p.nE);       // the overwritten output's shadow
    return MOKA_OK;
}

int moka_gradient_on_edge_jvp(moka_mesh *m, const double *dScalarCell, double *dGradEdge)
{
    return moka_gradient_on_edge(m, dScalarCell, dGradEdge);              // linear: the tangent map is the operator
}

int moka_divergence_on_cell_vjp(moka_mesh *m, double *dDivCell, double *dVecEdge, double *dTempEdge)
{
    if (!m || !dDivCell || !dVecEdge) return fail(m ? m->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    const Plan &p = m->plan;
    int rc = ensure_op_bufs(m);
    if (rc) return rc;
    HIPCHK(m->ctx, hipSetDevice(m->ctx->device));
    if ((rc = ensure_op_transposes(m))) return rc;
    if ((rc = put_rows(m, m->opBuf[0], dDivCell, MOKA_CELL, p.nC, p.K))) return rc;
    if ((rc = put_rows(m, m->opBuf[1], dVecEdge, MOKA_EDGE, p.nE, p.K))) return rc;
    if (dTempEdge && (rc = put_rows(m, m->opBuf[3], dTempEdge, MOKA_EDGE, p.nE, p.K))) return rc;
    OpArgs a{OP_DIV_T, 0, m->opBuf[0], m->opBuf[1]};
    a.in2 = dTempEdge ? m->opBuf[3] : nullptr;
    a.auxD = m->opESign;
    HIPCHK(m->ctx, launch_operator(m->dev, a, m->lpc, m->ctx->stream));
    if ((rc = get_rows(m, dVecEdge, m->opBuf[1], MOKA_EDGE, p.nE, p.K))) return rc;
    std::memset(dDivCell, 0, sizeof(double) * (size_t)p.K * p.nC);
    if (dTempEdge) std::memset(dTempEdge, 0, sizeof(double) * (size_t)p.K * p.nE);
    return MOKA_OK;
}

int moka_divergence_on_cell_jvp(moka_mesh *m, const double *dVecEdge, double *dTempEdge, double *dDivCell)
{
    return moka_divergence_on_cell(m, dVecEdge, dTempEdge, dDivCell);
}

int moka_curl_on_vertex_vjp(moka_mesh *m, const double *dCurlVertex, double *dVecEdge)
{
    if (!m || !dCurlVertex || !dVecEdge) return fail(m ? m->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    const Plan &p = m->plan;
    int rc = ensure_op_bufs(m);
    if (rc) return rc;
    HIPCHK(m->ctx, hipSetDevice(m->ctx->device));
    if ((rc = ensure_op_transposes(m))) return rc;
    if ((rc = put_rows(m, m->opBuf[0], dCurlVertex, MOKA_VERTEX, p.nV, p.K))) return rc;
    if ((rc = put_rows(m, m->opBuf[1], dVecEdge, MOKA_EDGE, p.nE, p.K))) return rc;
    OpArgs a{OP_CURL_T, 0, m->opBuf[0], m->opBuf[1]};
    a.auxI = m->opTVert; a.auxD = m->opTCoef; a.auxW = m->opTW;
    HIPCHK(m->ctx, launch_operator(m->dev, a, m->lpc, m->ctx->stream));
    return get_rows(m, dVecEdge, m->opBuf[1], MOKA_EDGE, p.nE, p.K);       // the curl shadow stays: the primal accumulates
}

int moka_curl_on_vertex_jvp(moka_mesh *m, const double *dVecEdge, double *dCurlVertex)
{
    return moka_curl_on_vertex(m, dVecEdge, dCurlVertex);                 // accumulates, like the primal
}

int moka_divergence_on_cell(moka_mesh *m, const double *vecEdge, double *tempEdge, double *divCell)
{
    if (!m || !vecEdge || !divCell) return fail(m ? m->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    const Plan &p = m->plan;
    int rc = ensure_op_bufs(m);
    if (rc) return rc;
    hipStream_t s = m->ctx->stream;
    HIPCHK(m->ctx, hipSetDevice(m->ctx->device));
    if ((rc = put_rows(m, m->opBuf[0], vecEdge, MOKA_EDGE, p.nE, p.K))) return rc;
    OpArgs a1{OP_DIV_P1, 0, m->opBuf[0], m->opBuf[1]};      // temp = V*dvEdge (Operators.jl:60)
    HIPCHK(m->ctx, launch_operator(m->dev, a1, m->lpc, s));
    if (tempEdge && (rc = get_rows(m, tempEdge, m->opBuf[1], MOKA_EDGE, p.nE, p.K))) return rc;
    OpArgs a2{OP_DIV_P2, 0, m->opBuf[0], m->opBuf[1]};      // second pass reads V, folds dvEdge*sign exactly
    HIPCHK(m->ctx, launch_operator(m->dev, a2, m->lpc, s));
    return get_rows(m, divCell, m->opBuf[1], MOKA_CELL, p.nC, p.K);
}

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
    auto A = [&](double **q, size_t n, size_t eb = 8) { if (rc == MOKA_OK) rc = alloc_field(st, q, n, eb); };
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
    for (void *q : st->allocs) (void)hipFree(q);
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

// Argument block of RK4 stage s (1..4).  A = Curr (current level), B = New accumulator (the previous
// level's buffers, becomes the current level at the end), R1/R2 = provisional states.
}  // extern "C"
namespace mk {
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
    } else if (s == 2) {   // Provis = R1 -> R2
        g.pu = R1.u; g.ph = R1.h; g.ssh = R1.ssh; g.cu = A.u; g.ch = A.h; g.nu_in = B.u; g.nh_in = B.h;
        g.pu_out = R2.u; g.ph_out = R2.h; g.ssh_out = R2.ssh; g.a = a[1];
    } else if (s == 3) {   // Provis = R2 -> R1
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
}  // namespace mk
// The tracer launch of RK4 stage s, behind the dycore's launch g on the compute stream (it reads the thickness that launch wrote:
// the next provisional one, the new level's at stage 4; the stage's own provisional state is never written by its launch).  Buffers
// follow rk4_stage_args: provisional tracers current level -> trProv[0] -> trProv[1] -> trProv[0]; the running content sum Qn lives in
// the previous level's array, as New does, and stage 4 leaves the new tracers there (rk4_end swaps the levels).  Qc = phi * h of the
// current level is formed on the fly by every stage that needs it (the same product, the same bits as a stored one).
static hipError_t tracer_stage(moka_state *st, int s, const StageArgs &g)
{
    const moka_mesh *mm = st->mesh;
    const Plan &p = mm->plan;
    TracerArgs t{};
    t.nT = st->nTracers; t.stage = s; t.stride = (int64_t)p.K * p.nC;
    t.pu = g.pu; t.ph = g.ph; t.hcur = st->lev[1].h; t.hnext = s < 4 ? g.ph_out : g.nh_out;
    t.pphi = s == 1 ? st->trPhi[1] : st->trProv[s == 3 ? 1 : 0];
    t.pphi_out = s == 4 ? nullptr : st->trProv[s == 2 ? 1 : 0];
    t.cphi = st->trPhi[1]; t.qn = st->trPhi[0];
    t.a = g.a; t.b = g.b;
    const bool bih = st->trKappa4Dev != nullptr;
    t.kappa = st->trKappaDev ? st->trKappaDev : bih ? st->trKappa4Dev + t.nT : nullptr;      // (bih alone: the array of zeros)
    t.dvdc = t.kappa ? mm->dvdc : nullptr;
    t.src = st->trSrcDev;
    t.kappa4 = st->trKappa4Dev; t.lap = bih ? st->trLap : nullptr;
    const MeshDev dev = launch_bounds(mm);
    const bool generic = st->ctx->variant == 3;
    st->tracerPath = tracer_kernel(dev, mm->lpc, t.nT, generic, t.kappa != nullptr, bih).form;
    if (bih) {          // L = Lap(ph_s, pphi) of the tracers with kappa4 != 0, behind the dycore's launch and ahead of the tracer launch
        TracerLapArgs q{};
        q.nT = t.nT; q.stride = t.stride; q.ph = t.ph; q.x = t.pphi; q.kappa4 = t.kappa4; q.dvdc = t.dvdc; q.out = st->trLap;
        if (hipError_t e = launch_tracer_lap(dev, q, mm->lpc, generic, st->ctx->stream); e != hipSuccess) return e;
    }
    return launch_tracers(dev, t, mm->lpc, generic, st->ctx->stream);
}

// The vertical pass (implicit vertical diffusion, include/moka_hip.h): forwards behind the stage-4 tracer launch on the new tracers with
// the new thickness, backwards at the head of a reversed step on X with the recorded hn.  The callers skip it when K < 2, when dt == 0.0
// and while every kappaV is zero and no tracer has a diffusivity field that is on.  *path takes the form that served it.  fld: the
// device table of the diffusivity fields (nullptr: none -- the scalar instances).  gslot (reverse only): the gradient instances, with the
// step's recorded phi_new in p and the densities in D (moka_tracer_adjoint_want_vertical_gradient).
static int tracer_vmix(moka_mesh *mm, moka_ctx *ctx, int nT, const double *h, double *x, const double *kv, const double *const *fld, double dt,
                       double *scratch,
                       bool reverse, int *path, const int32_t *gslot = nullptr, const double *p_new = nullptr, double *D = nullptr)
{
    const Plan &p = mm->plan;
    if (!mm->nLev)
        if (int rc = upload_vec(mm, p.nLev, &mm->nLev)) return rc;
    VmixArgs a{};
    a.nT = nT; a.nC = p.nC; a.K = p.K; a.stride = (int64_t)p.K * p.nC;
    a.h = h; a.x = x; a.kv = kv; a.fld = fld; a.dt = dt; a.nLev = mm->nLev; a.scratch = scratch;
    a.gslot = gslot; a.p = p_new; a.D = D;
    const bool generic = ctx->variant == 3;
    *path = vmix_kernel(p.K, generic, gslot ? 4 : 3).form;
    HIPCHK(ctx, launch_tracer_vmix(a, reverse, generic, ctx->stream));
    return MOKA_OK;
}

// The vertical pass of the flow (implicit vertical mixing of momentum with a surface stress and a bottom drag, include/moka_hip.h): behind
// stage 4 on the new level's normalVelocity and layerThickness, through the same two pointers in the 16- and the 13-stream form.  The
// caller skips it while the pass is off and when dt == 0.0.  Launches only: nothing is allocated, synchronised or read back, so a
// captured step replays it.
static int momentum_vmix(moka_state *st, double *u, const double *h, double dt)
{
    const Plan &p = st->mesh->plan;
    MomVmixArgs a{};
    a.nE = p.nE; a.K = p.K; a.ehdr = st->mesh->dev.ehdr; a.u = u; a.h = h;
    a.tau = st->momTau && st->momTauOn ? st->momTau : nullptr;
    a.dt = dt; a.nu = st->momNuV; a.drag = st->momDrag; a.scratch = st->momScratch;
    if (p.K < 2 && a.drag == 0.0 && !a.tau) return MOKA_OK;      // one level and the viscosity alone: no column has anything to do
    const bool generic = st->ctx->variant == 3;
    HIPCHK(st->ctx, launch_momentum_vmix(a, generic, st->ctx->stream));
    st->momVmixPath = momentum_vmix_form(p.K, generic);
    return MOKA_OK;
}

// Tape of the tracer reverse mode (moka_tracer_tape_*, further down).  Per recorded step: the four provisional states the stage launches
// read, the new level's thickness and the diffusivities in force -- K * (4 nEdges + 5 nCells) doubles and nTracers more.
struct moka_tracer_tape {
    moka_state *st = nullptr;
    moka_ctx *ctx = nullptr;
    int nT = 0;
    int64_t capacity = 0, n = 0;
    double *pu = nullptr, *ph = nullptr;             // capacity x 4 x (K, nE) / (K, nC): pu_s, ph_s of stage s = 0..3
    double *hn = nullptr;                            // capacity x (K, nC): layerThickness of the new level
    double *kap = nullptr, *kap4 = nullptr;          // capacity x nT each: the diffusivities and the biharmonic coefficients on the device
    std::vector<double> kappa, kappa4, dts;          // ... and on the host (n * nT values each); dt of each step
    double *kv = nullptr;                            // capacity x nT: the vertical diffusivities on the device ...
    std::vector<double> kappaV;                      // ... and on the host
    bool kvUsed = false;                             // some recorded step had a nonzero kappaV: slots of kv may hold old values
    double *vmScratch = nullptr;                     // 2 x (K, nC): the column form's g and y, allocated by the first sweep that has a vertical pass
    int vmixPath = 0;                                // moka_tracer_adjoint_vmix_path
    // the diffusivity fields the recorded steps ran with (moka_tracer_vertical_field_upload).  A step copies a tracer's field only when
    // the state's generation of it differs from that of the tape's newest copy; all of this is allocated by the first recorded step
    // that sees a field that is on, and the copies are released when a sweep has emptied the tape.
    std::vector<double *> vfCopies;                  // (K, nC) each
    std::vector<int32_t> vfNewest;                   // nT: a tracer's newest copy in vfCopies, -1 none
    std::vector<uint64_t> vfGen;                     // nT: ... and the generation it was taken at
    std::vector<int32_t> vfStep;                     // n x nT once vfTab exists: the copy a recorded step ran with, -1 the scalar
    double **vfTab = nullptr;                        // capacity x nT on the device: vfStep as the pointers the field instances read
    double *M = nullptr;                             // nT x (K, nC): Lap(ph_s, y) of a reverse stage (biharmonic term)
    double *X = nullptr, *g = nullptr, *S = nullptr, *y[2] = {nullptr, nullptr};   // nT x (K, nC) each: the adjoint state and the sweep's work arrays
    // gradient with respect to the sources (moka_tracer_adjoint_want_source_gradient): the (K, nC) accumulator of every tracer that was
    // ever flagged (nullptr otherwise), whether it is wanted now, and the device table of the wanted ones that the sweep's launches read
    std::vector<double *> G;
    std::vector<char> wantG;
    double **Gdev = nullptr;
    // gradient with respect to kappa_j and kappa4_j (moka_tracer_adjoint_want_diffusivity_gradient): the bit set of every tracer and the
    // nF flagged ones in ascending order.  All of the following is allocated by a flag, never by moka_tracer_tape_create, and replaced
    // as a whole when the set of flagged tracers changes (only an empty tape may change it).
    std::vector<int> wantK;                          // nT bit sets of MOKA_TRACER_GRAD_*
    std::vector<int32_t> kgTracer;                   // nF
    double *kgP = nullptr;                           // capacity x 4 x nF x (K, nC): pphi_s of the flagged tracers
    double *kgL = nullptr;                           // nF x (K, nC): Lap(ph_rs, pphi_rs) of a reverse stage
    double *kgW = nullptr;                           // 2 nF x nC: the densities Wk_f, Wk4_f (both rows exist; a row not wanted stays zero)
    double *kgOnes = nullptr;                        // nF ones: launch_tracer_lap's filter for the pass over the flagged tracers
    double *kgMOn = nullptr;                         // capacity x nT: the filter of the sweep's M pass (recorded kappa4, or 1 where M is wanted)
    int32_t *kgTracerDev = nullptr;                  // nF
    double **kgWdev = nullptr;                       // 2 nF
    // gradient with respect to kappaV_j (moka_tracer_adjoint_want_vertical_gradient): the nV flagged tracers in ascending order.  Allocated
    // by a flag, never by moka_tracer_tape_create, and replaced as a whole when the set changes (only an empty tape may change it).
    std::vector<char> wantV;                         // nT
    std::vector<int32_t> vgTracer;                   // nV
    double *vgP = nullptr;                           // capacity x nV x (K, nC): phi_new of the flagged tracers as each step left it
    double *vgD = nullptr;                           // nV x (K, nC): the densities D_f
    int32_t *vgSlot = nullptr;                       // nT on the device: a tracer's slot in vgP / vgD, -1 when it is not flagged
    bool seeded = false;
    bool pending = false;                            // seeded and not yet swept
    int path = 0;                                    // moka_tracer_adjoint_path
    std::vector<void *> allocs;
    bool counted = false;                            // st->attached includes this tape
};

// moka_step_rk4, and the same step recorded on `rec`: each stage's provisional state is copied behind that stage's launches, before a
// later stage overwrites the ping-pong buffer; the new thickness behind stage 4.  Copies only: the step's launches are untouched.
static int step_rk4(moka_state *st, double dt, moka_tracer_tape *rec)
{
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    const bool vmix = st->nTracers > 0 && st->trKappaVDev != nullptr;      // (non-null exactly while some kappaV != 0 or some diffusivity field is on)
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
    for (int s = 1; s <= 4; ++s) {
        if (timed) HIPCHK(c, stamp());
        const StageArgs g = s13 ? rk13_stage_args(st, s, dt, ssh0) : rk4_stage_args(st, s, dt, ssh0);
        HIPCHK(c, run_stage(st, g));
        if (st->nTracers > 0) HIPCHK(c, tracer_stage(st, s, g));
        if (s == 4 && vmix && st->mesh->plan.K >= 2 && dt != 0.0)       // the split step: the new tracers (still in the previous level's array) over the new thickness
            if ((rc = tracer_vmix(st->mesh, c, st->nTracers, g.nh_out, st->trPhi[0], st->trKappaVDev, st->trVfDev, dt, st->trVmixScratch, false, &st->vmixPath))) return rc;
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

extern "C" {

int moka_state_rk4_streams(const moka_state *st) { return !st ? 0 : rk13_usable(st) ? 13 : 16; }

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
        if ((rc = alloc_field(st, &st->nlQv, (size_t)p.K * p.nV))) return rc;
        if ((rc = alloc_field(st, &st->nlQe, 2 * (size_t)p.K * p.nE))) return rc;   // {F, q_e} pairs
        if ((rc = alloc_field(st, &st->nlKe, (size_t)p.K * p.nC))) return rc;
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
        if ((rc = alloc_field(st, &st->nlZv, (size_t)p.K * p.nV))) return rc;
        if ((rc = alloc_field(st, &st->nlDiv, (size_t)p.K * p.nC))) return rc;
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
    if ((rc = upload_vec(mm, rows, &d.row)) || (rc = upload_vec(mm, locC, &d.locC)) || (rc = upload_vec(mm, locV, &d.locV))) return rc;
    if ((rc = upload_vec(mm, start, &d.start))) return rc;
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
        if ((rc = alloc_field(st, &st->nlZv, (size_t)p.K * p.nV))) return rc;
        if ((rc = alloc_field(st, &st->nlDiv, (size_t)p.K * p.nC))) return rc;
    }
    if (!st->nlDiv4) {
        if ((rc = alloc_field(st, &st->nlDiv4, (size_t)p.K * p.nC))) return rc;
        if ((rc = alloc_field(st, &st->nlCurl4, (size_t)p.K * p.nV))) return rc;
        if ((rc = alloc_field(st, &st->coef4, (size_t)p.nE))) return rc;
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

// ---- tracer sources: d(h phi_j)/dt gains q_j[k,c], constant in time until changed (include/moka_hip.h) ----
static void state_free(moka_state *st, void *q)
{
    st->allocs.erase(std::remove(st->allocs.begin(), st->allocs.end(), q), st->allocs.end());
    (void)hipFree(q);
}

// the caller has synchronised the stream: no launch reads the table or a source
static void drop_sources(moka_state *st)
{
    for (double *q : st->trSrc)
        if (q) state_free(st, q);
    st->trSrc.clear();
    if (st->trSrcDev) state_free(st, st->trSrcDev);
    st->trSrcDev = nullptr;
}

// likewise for the diffusivity fields of the vertical pass (moka_tracer_vertical_field_upload, further down)
static void drop_vfields(moka_state *st)
{
    for (double *q : st->trVf)
        if (q) state_free(st, q);
    st->trVf.clear();
    st->trVfOn.clear();
    st->trVfGen.clear();                 // (trVfClock goes on counting)
    if (st->trVfDev) state_free(st, st->trVfDev);
    st->trVfDev = nullptr;
}

int moka_tracer_source_upload(moka_state *st, int32_t j, const double *host)
{
    if (!st) return fail(nullptr, MOKA_ERR_ARG, "state is NULL");
    if (j < 0 || j >= st->nTracers) return fail(st->ctx, MOKA_ERR_ARG, "tracer index out of range (moka_set_tracers)");
    const Plan &p = st->mesh->plan;
    const size_t nCK = (size_t)p.K * p.nC;
    for (size_t i = 0; host && i < nCK; ++i)
        if (!std::isfinite(host[i])) return fail(st->ctx, MOKA_ERR_ARG, "tracer source: every value must be finite");
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    HIPCHK(st->ctx, hipStreamSynchronize(st->ctx->stream));      // no launch is reading the old table or the old values
    const bool had = !st->trSrc.empty() && st->trSrc[j];
    if (!host) {
        if (!had) return MOKA_OK;
        state_free(st, st->trSrc[j]);
        st->trSrc[j] = nullptr;
        if (std::all_of(st->trSrc.begin(), st->trSrc.end(), [](double *q) { return !q; })) {
            drop_sources(st);
            return MOKA_OK;
        }
    } else {
        if (!had) {
            double *d = nullptr;
            if (int rc = alloc_field(st, &d, nCK)) return rc;
            if (!st->trSrcDev)
                if (int rc = alloc_field(st, reinterpret_cast<double **>(&st->trSrcDev), (size_t)st->nTracers, sizeof(double *))) {
                    (void)hipStreamSynchronize(st->ctx->stream);
                    state_free(st, d);
                    return rc;
                }
            st->trSrc.resize((size_t)st->nTracers, nullptr);
            st->trSrc[j] = d;
        }
        if (int rc = put_rows(st->mesh, st->trSrc[j], host, MOKA_CELL, p.nC, p.K)) return rc;
    }
    return h2d(st->ctx, st->trSrcDev, st->trSrc.data(), st->trSrc.size() * sizeof(double *));
}

int moka_tracer_source_download(moka_state *st, int32_t j, double *host)
{
    if (!st || !host) return fail(st ? st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    if (j < 0 || j >= st->nTracers) return fail(st->ctx, MOKA_ERR_ARG, "tracer index out of range (moka_set_tracers)");
    const Plan &p = st->mesh->plan;
    if (st->trSrc.empty() || !st->trSrc[j]) {
        std::fill(host, host + (size_t)p.K * p.nC, 0.0);
        return MOKA_OK;
    }
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    return get_rows(st->mesh, host, st->trSrc[j], MOKA_CELL, p.nC, p.K);
}

int moka_tracer_has_source(const moka_state *st, int32_t j, int *out)
{
    if (!st || !out) return fail(st ? st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    if (j < 0 || j >= st->nTracers) return fail(st->ctx, MOKA_ERR_ARG, "tracer index out of range (moka_set_tracers)");
    *out = !st->trSrc.empty() && st->trSrc[j] ? 1 : 0;
    return MOKA_OK;
}

int moka_set_tracers(moka_state *st, int32_t nTracers)
{
    if (!st) return fail(nullptr, MOKA_ERR_ARG, "state is NULL");
    if (nTracers < 0) return fail(st->ctx, MOKA_ERR_ARG, "nTracers must be >= 0");
    const Plan &p = st->mesh->plan;
    if (nTracers > 0) {
        if (st->f32) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "tracers: Float64 states only");
        if (st->attached > 0 || st->halos > 0)
            return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "tracers: not on a state with a halo or a tape");
        if (p.nPatchesLaunch != p.nPatches) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "tracers: whole (unpartitioned) meshes only");
    }
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    HIPCHK(st->ctx, hipStreamSynchronize(st->ctx->stream));
    double **arr[9] = {&st->trPhi[0], &st->trPhi[1], &st->trProv[0], &st->trProv[1], &st->trKappaDev, &st->trKappa4Dev, &st->trLap,
                       &st->trKappaVDev, &st->trVmixScratch};
    auto release = [&]() {
        drop_sources(st);                // every source goes with the tracers
        drop_vfields(st);                // ... and every diffusivity field
        for (double **q : arr) {
            if (!*q) continue;
            st->allocs.erase(std::remove(st->allocs.begin(), st->allocs.end(), (void *)*q), st->allocs.end());
            (void)hipFree(*q);
            *q = nullptr;
        }
        st->nTracers = 0;
        st->tracerPath = 0;
        st->trKappa.clear();             // every diffusivity back to zero
        st->trKappa4.clear();            // ... and every biharmonic coefficient
        st->trKappaV.clear();            // ... and every vertical diffusivity
        st->vmixPath = 0;
    };
    release();
    if (nTracers == 0) return MOKA_OK;
    for (double **q : arr)
        if (q == &st->trKappaDev || q == &st->trKappa4Dev || q == &st->trLap || q == &st->trKappaVDev || q == &st->trVmixScratch) continue;      // allocated by their setters
        else if (int rc = alloc_field(st, q, (size_t)nTracers * p.K * p.nC)) {
            (void)hipStreamSynchronize(st->ctx->stream);
            release();
            return rc;
        }
    HIPCHK(st->ctx, hipStreamSynchronize(st->ctx->stream));
    st->nTracers = nTracers;
    return MOKA_OK;
}

static int tracer_ref(moka_state *st, int32_t j, int time_level, const void *host, double **out)
{
    if (!st || !host) return fail(st ? st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    if (j < 0 || j >= st->nTracers) return fail(st->ctx, MOKA_ERR_ARG, "tracer index out of range (moka_set_tracers)");
    if (time_level != 0 && time_level != 1) return fail(st->ctx, MOKA_ERR_ARG, "time_level must be 0 (previous) or 1 (current)");
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    const Plan &p = st->mesh->plan;
    *out = st->trPhi[time_level] + (size_t)j * p.K * p.nC;
    return MOKA_OK;
}

int moka_tracer_upload(moka_state *st, int32_t j, int time_level, const double *host)
{
    double *d = nullptr;
    if (int rc = tracer_ref(st, j, time_level, host, &d)) return rc;
    return put_rows(st->mesh, d, host, MOKA_CELL, st->mesh->plan.nC, st->mesh->plan.K);
}

int moka_tracer_download(moka_state *st, int32_t j, int time_level, double *host)
{
    double *d = nullptr;
    if (int rc = tracer_ref(st, j, time_level, host, &d)) return rc;
    return get_rows(st->mesh, host, d, MOKA_CELL, st->mesh->plan.nC, st->mesh->plan.K);
}

int moka_state_tracer_path(const moka_state *st) { return st ? st->tracerPath : 0; }

int moka_set_tracer_diffusion(moka_state *st, const double *kappa)
{
    if (!st) return fail(nullptr, MOKA_ERR_ARG, "state is NULL");
    const int nT = st->nTracers;
    if (kappa && nT == 0) return fail(st->ctx, MOKA_ERR_ARG, "tracer diffusion: the state has no tracers (moka_set_tracers)");
    bool any = false;
    for (int j = 0; kappa && j < nT; ++j) {
        if (!(kappa[j] >= 0.0) || !std::isfinite(kappa[j]))
            return fail(st->ctx, MOKA_ERR_ARG, "tracer diffusion: every diffusivity must be finite and >= 0");
        any = any || kappa[j] != 0.0;
    }
    moka_mesh *mm = st->mesh;
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    HIPCHK(st->ctx, hipStreamSynchronize(st->ctx->stream));      // no launch is reading the old values
    if (!any) {
        if (st->trKappaDev) {
            st->allocs.erase(std::remove(st->allocs.begin(), st->allocs.end(), (void *)st->trKappaDev), st->allocs.end());
            (void)hipFree(st->trKappaDev);
            st->trKappaDev = nullptr;
        }
        st->trKappa.clear();
        return MOKA_OK;
    }
    if (!mm->dvdc)
        if (int rc = upload_vec(mm, mm->plan.dvdc, &mm->dvdc)) return rc;
    if (!st->trKappaDev)
        if (int rc = alloc_field(st, &st->trKappaDev, (size_t)nT)) return rc;
    if (int rc = h2d(st->ctx, st->trKappaDev, kappa, (size_t)nT * sizeof(double))) return rc;
    st->trKappa.assign(kappa, kappa + nT);
    return MOKA_OK;
}

int moka_tracer_diffusion(const moka_state *st, int32_t j, double *out)
{
    if (!st || !out) return fail(st ? st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    if (j < 0 || j >= st->nTracers) return fail(st->ctx, MOKA_ERR_ARG, "tracer index out of range (moka_set_tracers)");
    *out = st->trKappa.empty() ? 0.0 : st->trKappa[j];
    return MOKA_OK;
}

int moka_set_tracer_biharmonic(moka_state *st, const double *kappa4)
{
    if (!st) return fail(nullptr, MOKA_ERR_ARG, "state is NULL");
    const int nT = st->nTracers;
    if (kappa4 && nT == 0) return fail(st->ctx, MOKA_ERR_ARG, "tracer biharmonic diffusion: the state has no tracers (moka_set_tracers)");
    bool any = false;
    for (int j = 0; kappa4 && j < nT; ++j) {
        if (!(kappa4[j] >= 0.0) || !std::isfinite(kappa4[j]))
            return fail(st->ctx, MOKA_ERR_ARG, "tracer biharmonic diffusion: every coefficient must be finite and >= 0");
        any = any || kappa4[j] != 0.0;
    }
    moka_mesh *mm = st->mesh;
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    HIPCHK(st->ctx, hipStreamSynchronize(st->ctx->stream));      // no launch is reading the old values
    auto drop = [&](double **q) {
        if (!*q) return;
        st->allocs.erase(std::remove(st->allocs.begin(), st->allocs.end(), (void *)*q), st->allocs.end());
        (void)hipFree(*q);
        *q = nullptr;
    };
    if (!any) {
        drop(&st->trKappa4Dev);
        drop(&st->trLap);
        st->trKappa4.clear();
        return MOKA_OK;
    }
    const Plan &p = mm->plan;
    if (!mm->dvdc)
        if (int rc = upload_vec(mm, mm->plan.dvdc, &mm->dvdc)) return rc;
    if (!st->trLap)
        if (int rc = alloc_field(st, &st->trLap, (size_t)nT * p.K * p.nC)) return rc;
    if (!st->trKappa4Dev)           // (alloc_field zero-fills: the second half stays the array of zeros)
        if (int rc = alloc_field(st, &st->trKappa4Dev, 2 * (size_t)nT)) {
            (void)hipStreamSynchronize(st->ctx->stream);
            drop(&st->trLap);
            return rc;
        }
    if (int rc = h2d(st->ctx, st->trKappa4Dev, kappa4, (size_t)nT * sizeof(double))) return rc;
    st->trKappa4.assign(kappa4, kappa4 + nT);
    return MOKA_OK;
}

int moka_tracer_biharmonic(const moka_state *st, int32_t j, double *out)
{
    if (!st || !out) return fail(st ? st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    if (j < 0 || j >= st->nTracers) return fail(st->ctx, MOKA_ERR_ARG, "tracer index out of range (moka_set_tracers)");
    *out = st->trKappa4.empty() ? 0.0 : st->trKappa4[j];
    return MOKA_OK;
}

// ---- what the vertical pass is to take for every tracer: its scalar, or its diffusivity field (include/moka_hip.h) ----
static bool vfield_on(const moka_state *st, int j) { return !st->trVf.empty() && st->trVf[j] && st->trVfOn[j]; }

// the coefficient the pass and a tape take for tracer j while the scalars are kv (empty = all zero): a field whose active entries are
// all zero makes it 0.0; beside a field that is on it is not read
static double vmix_coefficient(const moka_state *st, const std::vector<double> &kv, int j)
{
    if (!st->trVf.empty() && st->trVf[j] && !st->trVfOn[j]) return 0.0;
    return kv.empty() ? 0.0 : kv[j];
}

// Brings the device side in line with the scalars kv (empty = all zero) and the fields as they stand: the coefficient array, the table of
// the fields that are on, nLev and the scratch of the column form exist exactly while the pass is on.  The caller has synchronised the
// stream.  The scalars are taken over once nothing can fail any more.
static int vmix_commit(moka_state *st, std::vector<double> kv)
{
    const int nT = st->nTracers;
    moka_mesh *mm = st->mesh;
    std::vector<double> eff((size_t)nT, 0.0);
    std::vector<double *> tab((size_t)nT, nullptr);
    bool any = false, anyField = false;
    for (int j = 0; j < nT; ++j) {
        eff[j] = vmix_coefficient(st, kv, j);
        if (vfield_on(st, j)) { tab[j] = st->trVf[j]; anyField = true; }
        any = any || tab[j] || eff[j] != 0.0;
    }
    auto drop = [&](double **q) {
        if (!*q) return;
        st->allocs.erase(std::remove(st->allocs.begin(), st->allocs.end(), (void *)*q), st->allocs.end());
        (void)hipFree(*q);
        *q = nullptr;
    };
    if (std::all_of(kv.begin(), kv.end(), [](double k) { return k == 0.0; })) kv.clear();
    if (!anyField) drop(reinterpret_cast<double **>(&st->trVfDev));
    if (!any) {
        drop(&st->trKappaVDev);
        drop(&st->trVmixScratch);
        st->trKappaV = std::move(kv);
        return MOKA_OK;
    }
    const Plan &p = mm->plan;
    if (!mm->nLev)
        if (int rc = upload_vec(mm, p.nLev, &mm->nLev)) return rc;
    if (!st->trVmixScratch)
        if (int rc = alloc_field(st, &st->trVmixScratch, 2 * (size_t)p.K * p.nC)) return rc;
    if (!st->trKappaVDev)
        if (int rc = alloc_field(st, &st->trKappaVDev, (size_t)nT)) {
            (void)hipStreamSynchronize(st->ctx->stream);
            drop(&st->trVmixScratch);
            return rc;
        }
    if (anyField && !st->trVfDev)
        if (int rc = alloc_field(st, reinterpret_cast<double **>(&st->trVfDev), (size_t)nT, sizeof(double *))) return rc;
    if (int rc = h2d(st->ctx, st->trKappaVDev, eff.data(), (size_t)nT * sizeof(double))) return rc;
    if (anyField)
        if (int rc = h2d(st->ctx, st->trVfDev, tab.data(), (size_t)nT * sizeof(double *))) return rc;
    st->trKappaV = std::move(kv);
    return MOKA_OK;
}

int moka_set_tracer_vertical_diffusion(moka_state *st, const double *kappaV)
{
    if (!st) return fail(nullptr, MOKA_ERR_ARG, "state is NULL");
    const int nT = st->nTracers;
    if (kappaV && nT == 0) return fail(st->ctx, MOKA_ERR_ARG, "vertical tracer diffusion: the state has no tracers (moka_set_tracers)");
    for (int j = 0; kappaV && j < nT; ++j)
        if (!(kappaV[j] >= 0.0) || !std::isfinite(kappaV[j]))
            return fail(st->ctx, MOKA_ERR_ARG, "vertical tracer diffusion: every diffusivity must be finite and >= 0");
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    HIPCHK(st->ctx, hipStreamSynchronize(st->ctx->stream));      // no launch is reading the old values
    return vmix_commit(st, kappaV ? std::vector<double>(kappaV, kappaV + nT) : std::vector<double>());
}

int moka_tracer_vertical_field_upload(moka_state *st, int32_t j, const double *host)
{
    if (!st) return fail(nullptr, MOKA_ERR_ARG, "state is NULL");
    if (st->nTracers == 0) return fail(st->ctx, MOKA_ERR_ARG, "vertical diffusivity field: the state has no tracers (moka_set_tracers)");
    if (j < 0 || j >= st->nTracers) return fail(st->ctx, MOKA_ERR_ARG, "tracer index out of range (moka_set_tracers)");
    const Plan &p = st->mesh->plan;
    const size_t nCK = (size_t)p.K * p.nC;
    bool on = false;                     // the host scan: the interfaces k < nLev[c] - 1 of every column, and nothing else
    for (int i = 0; host && i < p.nC; ++i) {
        const double *col = host + (size_t)p.cellN2O[i] * p.K;
        for (int k = 0; k < p.nLev[i] - 1; ++k) {
            if (!(col[k] >= 0.0) || !std::isfinite(col[k]))
                return fail(st->ctx, MOKA_ERR_ARG, "vertical diffusivity field: every value at an active interface must be finite and >= 0");
            on = on || col[k] != 0.0;
        }
    }
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    HIPCHK(st->ctx, hipStreamSynchronize(st->ctx->stream));      // no launch is reading the old table or the old values
    const bool had = !st->trVf.empty() && st->trVf[j];
    if (!host && !had) return MOKA_OK;
    // The new field goes into an array of its own and the old one stays until the device side has been brought in line: a failure
    // on the way leaves the tracer with the field, the table and the generation it had.
    double *fresh = nullptr;
    if (host) {
        if (int rc = alloc_field(st, &fresh, nCK)) return rc;
        if (int rc = put_rows(st->mesh, fresh, host, MOKA_CELL, p.nC, p.K)) {
            (void)hipStreamSynchronize(st->ctx->stream);
            state_free(st, fresh);
            return rc;
        }
    }
    const std::vector<double *> vf0 = st->trVf;
    const std::vector<char> on0 = st->trVfOn;
    const std::vector<uint64_t> gen0 = st->trVfGen;
    st->trVf.resize((size_t)st->nTracers, nullptr);
    st->trVfOn.resize((size_t)st->nTracers, 0);
    st->trVfGen.resize((size_t)st->nTracers, 0);
    double *const old = st->trVf[j];
    st->trVf[j] = fresh;
    st->trVfOn[j] = fresh && on ? 1 : 0;
    st->trVfGen[j] = st->trVfClock + 1;
    if (std::all_of(st->trVf.begin(), st->trVf.end(), [](double *q) { return !q; })) {
        st->trVf.clear();
        st->trVfOn.clear();
    }
    if (int rc = vmix_commit(st, st->trKappaV)) {
        (void)hipStreamSynchronize(st->ctx->stream);
        st->trVf = vf0;
        st->trVfOn = on0;
        st->trVfGen = gen0;
        if (fresh) state_free(st, fresh);
        (void)vmix_commit(st, st->trKappaV);     // the table and the coefficients of the fields as they were
        return rc;
    }
    ++st->trVfClock;
    if (old) state_free(st, old);
    return MOKA_OK;
}

int moka_tracer_vertical_field_download(moka_state *st, int32_t j, double *host)
{
    if (!st || !host) return fail(st ? st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    if (j < 0 || j >= st->nTracers) return fail(st->ctx, MOKA_ERR_ARG, "tracer index out of range (moka_set_tracers)");
    const Plan &p = st->mesh->plan;
    if (st->trVf.empty() || !st->trVf[j]) {
        std::fill(host, host + (size_t)p.K * p.nC, 0.0);
        return MOKA_OK;
    }
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    return get_rows(st->mesh, host, st->trVf[j], MOKA_CELL, p.nC, p.K);
}

int moka_tracer_has_vertical_field(const moka_state *st, int32_t j, int *out)
{
    if (!st || !out) return fail(st ? st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    if (j < 0 || j >= st->nTracers) return fail(st->ctx, MOKA_ERR_ARG, "tracer index out of range (moka_set_tracers)");
    *out = !st->trVf.empty() && st->trVf[j] ? 1 : 0;
    return MOKA_OK;
}

int moka_tracer_vertical_diffusion(const moka_state *st, int32_t j, double *out)
{
    if (!st || !out) return fail(st ? st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    if (j < 0 || j >= st->nTracers) return fail(st->ctx, MOKA_ERR_ARG, "tracer index out of range (moka_set_tracers)");
    *out = st->trKappaV.empty() ? 0.0 : st->trKappaV[j];
    return MOKA_OK;
}

int moka_state_tracer_vmix_path(const moka_state *st) { return st ? st->vmixPath : 0; }

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
    if (int rc = alloc_field(st, &st->momScratch, 2 * (size_t)p.K * p.nE)) return rc;
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
        if (st->momTau) state_free(st, st->momTau);
        st->momTau = nullptr; st->momTauOn = false;
        return MOKA_OK;
    }
    if (on)
        if (int rc = mom_vmix_scratch(st)) return rc;
    double *fresh = nullptr;             // the new stress goes into an array of its own: a failure leaves the old one in force
    if (int rc = alloc_field(st, &fresh, (size_t)p.nE)) return rc;
    if (int rc = put_rows(st->mesh, fresh, host, MOKA_EDGE, p.nE, 1)) {
        (void)hipStreamSynchronize(st->ctx->stream);
        state_free(st, fresh);
        return rc;
    }
    if (st->momTau) state_free(st, st->momTau);
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

int moka_state_momentum_vmix_path(const moka_state *st) { return st ? st->momVmixPath : 0; }

// ---------------------------------------------------------------------------------------------
// reverse mode of the tracer transport over a frozen flow (include/moka_hip.h: the algebra; tracer_adjoint.hip: the kernels).  A handle of
// its own, separate from moka_tape: the tracer step is linear in phi, so its transpose needs the recorded provisional states only.
// ---------------------------------------------------------------------------------------------
static int ttape_alloc(moka_tracer_tape *t, double **out, size_t elems)
{
    void *d = nullptr;
    const size_t bytes = elems * sizeof(double);
    hipError_t e = hipMalloc(&d, std::max<size_t>(bytes, 16));
    if (e != hipSuccess)
        return fail(t->ctx, MOKA_ERR_ALLOC, std::string("tracer tape: hipMalloc of ") + std::to_string(bytes) + " bytes: " + hipGetErrorString(e));
    t->allocs.push_back(d);
    HIPCHK(t->ctx, hipMemsetAsync(d, 0, bytes, t->ctx->stream));
    *out = static_cast<double *>(d);
    return MOKA_OK;
}

int moka_tracer_tape_create(moka_state *st, int64_t capacity_steps, moka_tracer_tape **out)
{
    if (!st || !out || capacity_steps < 0) return fail(st ? st->ctx : nullptr, MOKA_ERR_ARG, "bad argument");
    *out = nullptr;
    if (st->nTracers == 0) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "tracer reverse mode: the state has no tracers (moka_set_tracers)");
    const Plan &p = st->mesh->plan;
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    moka_tracer_tape *t = new (std::nothrow) moka_tracer_tape();
    if (!t) return fail(st->ctx, MOKA_ERR_ALLOC, "out of host memory");
    t->st = st; t->ctx = st->ctx;
    t->nT = st->nTracers;
    t->G.assign((size_t)t->nT, nullptr);
    t->wantG.assign((size_t)t->nT, 0);
    t->wantK.assign((size_t)t->nT, 0);
    t->wantV.assign((size_t)t->nT, 0);
    t->capacity = capacity_steps;
    const size_t nEK = (size_t)p.K * p.nE, nCK = (size_t)p.K * p.nC, cap = (size_t)capacity_steps;
    int rc = MOKA_OK;
    auto A = [&](double **q, size_t n) { if (rc == MOKA_OK) rc = ttape_alloc(t, q, n); };
    A(&t->pu, nEK * 4 * cap); A(&t->ph, nCK * 4 * cap); A(&t->hn, nCK * cap); A(&t->kap, (size_t)t->nT * cap); A(&t->kap4, (size_t)t->nT * cap); A(&t->kv, (size_t)t->nT * cap);
    A(&t->X, nCK * t->nT); A(&t->g, nCK * t->nT); A(&t->S, nCK * t->nT); A(&t->y[0], nCK * t->nT); A(&t->y[1], nCK * t->nT); A(&t->M, nCK * t->nT);
    if (rc != MOKA_OK) { moka_tracer_tape_destroy(t); return rc; }
    HIPCHK(st->ctx, hipStreamSynchronize(st->ctx->stream));
    state_attach(st);
    t->counted = true;
    *out = t;
    return MOKA_OK;
}

void moka_tracer_tape_destroy(moka_tracer_tape *t)
{
    if (!t) return;
    bool alive;
    {
        std::lock_guard<std::mutex> lk(g_liveMutex);
        alive = g_liveStates.count(t->st) != 0;
    }
    if (t->counted) state_detach(t->st);
    if (alive) {                         // a state that went first synchronised its stream when it did: nothing of this tape is in flight
        (void)hipSetDevice(t->ctx->device);
        (void)hipStreamSynchronize(t->ctx->stream);
    }
    for (void *q : t->allocs) (void)hipFree(q);
    delete t;
}

int moka_step_rk4_tracer_taped(moka_tracer_tape *t, double dt)
{
    if (!t) return fail(nullptr, MOKA_ERR_ARG, "tracer tape is NULL");
    moka_state *st = t->st;
    if (t->n >= t->capacity) return fail(t->ctx, MOKA_ERR_ARG, "tracer tape is full");
    if (st->nTracers != t->nT) return fail(t->ctx, MOKA_ERR_ARG, "tracer tape: the state's tracer count has changed since the tape was created");
    HIPCHK(t->ctx, hipSetDevice(t->ctx->device));
    if (dt < 0.0 && (st->trKappaVDev || mom_vmix_on(st))) return step_rk4(st, dt, t);      // (refused there, before any launch)
    // the diffusivity fields the step is about to run with: a copy of every one the tape does not hold yet, allocated ahead of the
    // step's first launch -- a failure leaves the state and the tape as they were
    const Plan &p = st->mesh->plan;
    const size_t nCK = (size_t)p.K * p.nC;
    std::vector<int> fresh;
    bool fields = false;
    for (int j = 0; j < t->nT; ++j) {
        if (!vfield_on(st, j)) continue;
        fields = true;
        if (t->vfNewest.empty() || t->vfNewest[j] < 0 || t->vfGen[j] != st->trVfGen[j]) fresh.push_back(j);
    }
    if (fields && !t->vfTab) {
        if (int rc = ttape_alloc(t, reinterpret_cast<double **>(&t->vfTab), (size_t)t->capacity * t->nT * sizeof(double *) / sizeof(double))) return rc;
        t->vfStep.assign((size_t)t->n * t->nT, -1);
        t->vfNewest.assign((size_t)t->nT, -1);
        t->vfGen.assign((size_t)t->nT, 0);
    }
    if (!fresh.empty()) {
        std::vector<void *> got;
        for (size_t i = 0; i < fresh.size(); ++i) {
            void *d = nullptr;
            if (hipError_t e = hipMalloc(&d, std::max<size_t>(nCK * sizeof(double), 16)); e != hipSuccess) {
                for (void *q : got) (void)hipFree(q);
                return fail(t->ctx, MOKA_ERR_ALLOC, std::string("tracer tape: hipMalloc of a diffusivity field: ") + hipGetErrorString(e));
            }
            got.push_back(d);
        }
        for (size_t i = 0; i < fresh.size(); ++i) {
            const int j = fresh[i];
            t->allocs.push_back(got[i]);
            t->vfCopies.push_back(static_cast<double *>(got[i]));
            t->vfNewest[j] = (int32_t)t->vfCopies.size() - 1;
            t->vfGen[j] = st->trVfGen[j];
            HIPCHK(t->ctx, hipMemcpyAsync(got[i], st->trVf[j], nCK * sizeof(double), hipMemcpyDeviceToDevice, t->ctx->stream));
        }
    }
    if (int rc = step_rk4(st, dt, t)) return rc;
    if (t->vfTab) {                  // which copy the step ran with, per tracer
        std::vector<double *> row((size_t)t->nT, nullptr);
        for (int j = 0; j < t->nT; ++j) {
            const int32_t i = vfield_on(st, j) ? t->vfNewest[j] : -1;
            t->vfStep.push_back(i);
            if (i >= 0) row[j] = t->vfCopies[i];
        }
        if (int rc = h2d(t->ctx, t->vfTab + (size_t)t->n * t->nT, row.data(), row.size() * sizeof(double *))) {
            t->vfStep.resize((size_t)t->n * t->nT);
            return rc;
        }
    }
    // the diffusivities the step's launches read (every copy on the context's stream, device to device: no host buffer to keep alive)
    double *kd = t->kap + (size_t)t->n * t->nT;
    if (st->trKappaDev) HIPCHK(t->ctx, hipMemcpyAsync(kd, st->trKappaDev, (size_t)t->nT * sizeof(double), hipMemcpyDeviceToDevice, t->ctx->stream));
    else HIPCHK(t->ctx, hipMemsetAsync(kd, 0, (size_t)t->nT * sizeof(double), t->ctx->stream));
    for (int j = 0; j < t->nT; ++j) t->kappa.push_back(st->trKappa.empty() ? 0.0 : st->trKappa[j]);
    double *k4d = t->kap4 + (size_t)t->n * t->nT;
    if (st->trKappa4Dev) HIPCHK(t->ctx, hipMemcpyAsync(k4d, st->trKappa4Dev, (size_t)t->nT * sizeof(double), hipMemcpyDeviceToDevice, t->ctx->stream));
    else HIPCHK(t->ctx, hipMemsetAsync(k4d, 0, (size_t)t->nT * sizeof(double), t->ctx->stream));
    for (int j = 0; j < t->nT; ++j) t->kappa4.push_back(st->trKappa4.empty() ? 0.0 : st->trKappa4[j]);
    double *kvd = t->kv + (size_t)t->n * t->nT;
    if (st->trKappaVDev) {
        HIPCHK(t->ctx, hipMemcpyAsync(kvd, st->trKappaVDev, (size_t)t->nT * sizeof(double), hipMemcpyDeviceToDevice, t->ctx->stream));
        t->kvUsed = true;
    } else if (t->kvUsed)            // (the array is created zeroed: a tape that never saw a kappaV issues nothing here)
        HIPCHK(t->ctx, hipMemsetAsync(kvd, 0, (size_t)t->nT * sizeof(double), t->ctx->stream));
    for (int j = 0; j < t->nT; ++j) t->kappaV.push_back(vmix_coefficient(st, st->trKappaV, j));
    t->dts.push_back(dt);
    ++t->n;
    t->seeded = false;
    t->pending = false;
    return MOKA_OK;
}

int moka_tracer_tape_steps(const moka_tracer_tape *t, int64_t *n)
{
    if (!t || !n) return fail(t ? t->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    *n = t->n;
    return MOKA_OK;
}

static int ttape_field(moka_tracer_tape *t, int32_t j, double **out)
{
    if (!t) return fail(nullptr, MOKA_ERR_ARG, "tracer tape is NULL");
    if (j < 0 || j >= t->nT) return fail(t->ctx, MOKA_ERR_ARG, "tracer index out of range (moka_tracer_tape_create)");
    HIPCHK(t->ctx, hipSetDevice(t->ctx->device));
    const Plan &p = t->st->mesh->plan;
    *out = t->X + (size_t)j * p.K * p.nC;
    return MOKA_OK;
}

int moka_tracer_adjoint_seed(moka_tracer_tape *t, int32_t j, const double *host)
{
    double *d = nullptr;
    if (int rc = ttape_field(t, j, &d)) return rc;
    const Plan &p = t->st->mesh->plan;
    const size_t nCK = (size_t)p.K * p.nC;
    if (!t->seeded) {
        HIPCHK(t->ctx, hipMemsetAsync(t->X, 0, nCK * t->nT * sizeof(double), t->ctx->stream));
        for (double *G : t->G)
            if (G) HIPCHK(t->ctx, hipMemsetAsync(G, 0, nCK * sizeof(double), t->ctx->stream));
        if (t->kgW) HIPCHK(t->ctx, hipMemsetAsync(t->kgW, 0, 2 * t->kgTracer.size() * (size_t)p.nC * sizeof(double), t->ctx->stream));
        if (t->vgD) HIPCHK(t->ctx, hipMemsetAsync(t->vgD, 0, t->vgTracer.size() * nCK * sizeof(double), t->ctx->stream));
    }
    t->seeded = true;
    t->pending = true;
    if (!host) {
        HIPCHK(t->ctx, hipMemsetAsync(d, 0, nCK * sizeof(double), t->ctx->stream));
        return MOKA_OK;
    }
    return put_rows(t->st->mesh, d, host, MOKA_CELL, p.nC, p.K);
}

static void ttape_free(moka_tracer_tape *t, void *q);

int moka_tracer_adjoint_sweep(moka_tracer_tape *t)
{
    if (!t) return fail(nullptr, MOKA_ERR_ARG, "tracer tape is NULL");
    if (!t->seeded) return fail(t->ctx, MOKA_ERR_ARG, "tracer tape: seed first (moka_tracer_adjoint_seed)");
    moka_state *st = t->st;
    moka_mesh *mm = st->mesh;
    const Plan &p = mm->plan;
    HIPCHK(t->ctx, hipSetDevice(t->ctx->device));
    hipStream_t s = t->ctx->stream;
    bool diff = false, bih = false;
    for (double k : t->kappa4) bih = bih || k != 0.0;
    for (double k : t->kappa) diff = diff || k != 0.0;
    diff = diff || bih;                 // the BIH kernels exist only together with DIFF (a step without diffusivities recorded zeros)
    const int nF = (int)t->kgTracer.size();         // tracers flagged for d J / d kappa, d J / d kappa4: their passes need dvdc as well
    if ((diff || nF > 0) && !mm->dvdc)
        if (int rc = upload_vec(mm, mm->plan.dvdc, &mm->dvdc)) return rc;
    // M of a tracer whose d J / d kappa4 is wanted and whose recorded kappa4 is zero: the sweep's own pass skips it, so the pass takes a
    // filter in which such a tracer counts -- its M lands in its own slot of t->M, which no reverse kernel reads for kappa4_j == 0
    bool kgM = false;
    for (int w : t->wantK) kgM = kgM || (w & MOKA_TRACER_GRAD_KAPPA4) != 0;
    if (kgM && t->n > 0) {
        std::vector<double> on(t->kappa4.begin(), t->kappa4.begin() + (size_t)t->n * t->nT);
        for (size_t i = 0; i < on.size(); ++i)
            if (on[i] == 0.0 && (t->wantK[i % t->nT] & MOKA_TRACER_GRAD_KAPPA4)) on[i] = 1.0;
        if (int rc = h2d(t->ctx, t->kgMOn, on.data(), on.size() * sizeof(double))) return rc;
    }
    const MeshDev dev = launch_bounds(mm);
    const bool generic = t->ctx->variant == 3;
    const size_t nEK = (size_t)p.K * p.nE, nCK = (size_t)p.K * p.nC;
    // the vertical pass of a recorded step (its kappaV, its dt): skipped as in the forward step, unless some tracer is flagged for the
    // vertical gradient -- then the gradient instances run, for a step whose kappaV are all zero the gradient alone.  A step that ran
    // with a diffusivity field takes the field instances and its row of the table of copies.
    const size_t nV = t->vgTracer.size();
    auto fields_of = [&](int64_t n) {
        return !t->vfStep.empty() && std::any_of(t->vfStep.begin() + n * t->nT, t->vfStep.begin() + (n + 1) * t->nT, [](int32_t i) { return i >= 0; });
    };
    auto vmix_of = [&](int64_t n) {
        return p.K >= 2 && t->dts[n] != 0.0 &&
               (nV > 0 || fields_of(n) ||
                std::any_of(t->kappaV.begin() + n * t->nT, t->kappaV.begin() + (n + 1) * t->nT, [](double k) { return k != 0.0; }));
    };
    for (int64_t n = 0; n < t->n && !t->vmScratch; ++n)
        if (vmix_of(n))
            if (int rc = ttape_alloc(t, &t->vmScratch, 2 * nCK)) return rc;
    double *const *G = std::any_of(t->wantG.begin(), t->wantG.end(), [](char w) { return w != 0; }) ? t->Gdev : nullptr;
    t->pending = false;
    while (t->n > 0) {
        const int64_t n = t->n - 1;
        const double dt = t->dts[n];
        const double a[3] = {dt / 2., dt / 2., dt};
        const double b[4] = {dt / 6., dt / 3., dt / 3., dt / 6.};
        int cur = 0;
        if (vmix_of(n))             // S^T = diag(h) A^-1 on X, ahead of g = X / hn
            if (int rc = tracer_vmix(mm, t->ctx, t->nT, t->hn + nCK * n, t->X, t->kv + (size_t)n * t->nT,
                                     fields_of(n) ? t->vfTab + (size_t)n * t->nT : nullptr, dt, t->vmScratch, true, &t->vmixPath,
                                     nV > 0 ? t->vgSlot : nullptr, nV > 0 ? t->vgP + nCK * ((size_t)n * nV) : nullptr, t->vgD)) return rc;
        HIPCHK(t->ctx, launch_tracer_adj_seed(dev, t->X, t->hn + nCK * n, t->g, t->y[cur], b[3], t->nT, G, s));
        for (int rs = 3; rs >= 0; --rs) {
            TracerAdjArgs q{};
            q.nT = t->nT; q.rs = rs; q.stride = (int64_t)nCK;
            q.pu = t->pu + nEK * (4 * n + rs); q.ph = t->ph + nCK * (4 * n + rs);
            q.y = t->y[cur]; q.g = t->g; q.S = t->S;
            q.out = rs > 0 ? t->y[cur ^ 1] : t->X;
            q.cb = rs > 0 ? b[rs - 1] : 0.0; q.ca = rs > 0 ? a[rs - 1] : 0.0;
            q.kappa = diff ? t->kap + (size_t)n * t->nT : nullptr;
            q.dvdc = diff ? mm->dvdc : nullptr;
            q.G = rs > 0 ? G : nullptr;         // reverse stage 0 does not touch G
            q.kappa4 = bih ? t->kap4 + (size_t)n * t->nT : nullptr;
            q.lapy = bih ? t->M : nullptr;
            if (kgM || (bih && std::any_of(t->kappa4.begin() + n * t->nT, t->kappa4.begin() + (n + 1) * t->nT, [](double k) { return k != 0.0; }))) {
                TracerLapArgs w{};          // M = Lap(ph_s, y) of the tracers whose recorded kappa4 is not zero (kgM: or whose d J / d kappa4 is wanted)
                w.nT = q.nT; w.stride = q.stride; w.ph = q.ph; w.x = q.y; w.kappa4 = kgM ? t->kgMOn + (size_t)n * t->nT : q.kappa4;
                w.dvdc = mm->dvdc; w.out = t->M;
                HIPCHK(t->ctx, launch_tracer_lap(dev, w, mm->lpc, generic, s));
            }
            if (nF > 0) {                   // L = Lap(ph_rs, pphi_rs) of the flagged tracers, then the products against y and M
                TracerLapArgs w{};
                w.nT = nF; w.stride = q.stride; w.ph = q.ph; w.x = t->kgP + nCK * ((size_t)(4 * n + rs) * nF); w.kappa4 = t->kgOnes;
                w.dvdc = mm->dvdc; w.out = t->kgL;
                HIPCHK(t->ctx, launch_tracer_lap(dev, w, mm->lpc, generic, s));
                TracerKgradArgs kg{};
                kg.nF = nF; kg.stride = q.stride; kg.ph = q.ph; kg.L = t->kgL; kg.y = q.y; kg.M = t->M;
                kg.tracer = t->kgTracerDev; kg.W = t->kgWdev;
                HIPCHK(t->ctx, launch_tracer_kgrad(dev, kg, mm->lpc, s));
            }
            t->path = tracer_adjoint_kernel(dev, mm->lpc, q.nT, generic, diff, bih).form;
            HIPCHK(t->ctx, launch_tracer_adjoint(dev, q, mm->lpc, generic, s));
            cur ^= 1;
        }
        t->n = n;
        t->dts.pop_back();
        t->kappa.resize((size_t)n * t->nT);
        t->kappa4.resize((size_t)n * t->nT);
        t->kappaV.resize((size_t)n * t->nT);
        if (!t->vfStep.empty()) t->vfStep.resize((size_t)n * t->nT);
    }
    if (!t->vfCopies.empty()) {         // the tape is empty: its copies of the diffusivity fields go once the sweep has read them
        HIPCHK(t->ctx, hipStreamSynchronize(s));
        for (double *q : t->vfCopies) ttape_free(t, q);
        t->vfCopies.clear();
        t->vfNewest.assign((size_t)t->nT, -1);
    }
    return MOKA_OK;
}

int moka_tracer_adjoint_download(moka_tracer_tape *t, int32_t j, double *host)
{
    double *d = nullptr;
    if (int rc = ttape_field(t, j, &d)) return rc;
    if (!host) return fail(t->ctx, MOKA_ERR_ARG, "NULL argument");
    const Plan &p = t->st->mesh->plan;
    return get_rows(t->st->mesh, host, d, MOKA_CELL, p.nC, p.K);
}

int moka_tracer_adjoint_want_source_gradient(moka_tracer_tape *t, int32_t j, int on)
{
    if (!t) return fail(nullptr, MOKA_ERR_ARG, "tracer tape is NULL");
    if (j < 0 || j >= t->nT) return fail(t->ctx, MOKA_ERR_ARG, "tracer index out of range (moka_tracer_tape_create)");
    if (t->pending) return fail(t->ctx, MOKA_ERR_ARG, "tracer tape: not between a seed and its sweep");
    HIPCHK(t->ctx, hipSetDevice(t->ctx->device));
    const Plan &p = t->st->mesh->plan;
    if (on && !t->G[j])
        if (int rc = ttape_alloc(t, &t->G[j], (size_t)p.K * p.nC)) return rc;
    if (!t->Gdev)
        if (int rc = ttape_alloc(t, reinterpret_cast<double **>(&t->Gdev), (size_t)t->nT * sizeof(double *) / sizeof(double))) return rc;
    t->wantG[j] = on ? 1 : 0;
    std::vector<double *> tab((size_t)t->nT, nullptr);
    for (int i = 0; i < t->nT; ++i) tab[i] = t->wantG[i] ? t->G[i] : nullptr;
    HIPCHK(t->ctx, hipStreamSynchronize(t->ctx->stream));        // no launch is reading the old table
    return h2d(t->ctx, t->Gdev, tab.data(), tab.size() * sizeof(double *));
}

int moka_tracer_adjoint_source_download(moka_tracer_tape *t, int32_t j, double *host)
{
    if (!t) return fail(nullptr, MOKA_ERR_ARG, "tracer tape is NULL");
    if (j < 0 || j >= t->nT) return fail(t->ctx, MOKA_ERR_ARG, "tracer index out of range (moka_tracer_tape_create)");
    if (!host) return fail(t->ctx, MOKA_ERR_ARG, "NULL argument");
    if (!t->G[j]) return fail(t->ctx, MOKA_ERR_ARG, "tracer tape: no source gradient was asked for this tracer (moka_tracer_adjoint_want_source_gradient)");
    HIPCHK(t->ctx, hipSetDevice(t->ctx->device));
    const Plan &p = t->st->mesh->plan;
    return get_rows(t->st->mesh, host, t->G[j], MOKA_CELL, p.nC, p.K);
}

int moka_tracer_adjoint_path(const moka_tracer_tape *t) { return t ? t->path : 0; }
int moka_tracer_adjoint_vmix_path(const moka_tracer_tape *t) { return t ? t->vmixPath : 0; }

// ---- d J / d kappa_j, d J / d kappa4_j (include/moka_hip.h: the algebra; k_tracer_kgrad) ----
static void ttape_free(moka_tracer_tape *t, void *q)
{
    if (!q) return;
    t->allocs.erase(std::remove(t->allocs.begin(), t->allocs.end(), q), t->allocs.end());
    (void)hipFree(q);
}

int moka_tracer_adjoint_want_diffusivity_gradient(moka_tracer_tape *t, int32_t j, int what, int on)
{
    if (!t) return fail(nullptr, MOKA_ERR_ARG, "tracer tape is NULL");
    if (j < 0 || j >= t->nT) return fail(t->ctx, MOKA_ERR_ARG, "tracer index out of range (moka_tracer_tape_create)");
    if (what == 0 || (what & ~(MOKA_TRACER_GRAD_KAPPA | MOKA_TRACER_GRAD_KAPPA4)))
        return fail(t->ctx, MOKA_ERR_ARG, "tracer tape: what must be a nonempty set of MOKA_TRACER_GRAD_KAPPA | MOKA_TRACER_GRAD_KAPPA4");
    if (t->n > 0) return fail(t->ctx, MOKA_ERR_ARG, "tracer tape: the diffusivity gradients may be chosen only while the tape holds no recorded step");
    if (t->pending) return fail(t->ctx, MOKA_ERR_ARG, "tracer tape: not between a seed and its sweep");
    HIPCHK(t->ctx, hipSetDevice(t->ctx->device));
    const Plan &p = t->st->mesh->plan;
    std::vector<int> want = t->wantK;
    want[j] = on ? (want[j] | what) : (want[j] & ~what);
    std::vector<int32_t> tr;
    for (int i = 0; i < t->nT; ++i)
        if (want[i]) tr.push_back(i);
    const size_t nF = tr.size(), nCK = (size_t)p.K * p.nC, cap = (size_t)t->capacity;
    HIPCHK(t->ctx, hipStreamSynchronize(t->ctx->stream));        // no launch is reading what goes
    if (nF > 0 && tr == t->kgTracer) {          // the same tracers, other bits: the arrays stay; the table of wanted densities changes
        std::vector<double *> tab(2 * nF, nullptr);
        for (size_t f = 0; f < nF; ++f) {
            if (want[tr[f]] & MOKA_TRACER_GRAD_KAPPA) tab[2 * f] = t->kgW + (2 * f) * (size_t)p.nC;
            if (want[tr[f]] & MOKA_TRACER_GRAD_KAPPA4) tab[2 * f + 1] = t->kgW + (2 * f + 1) * (size_t)p.nC;
        }
        HIPCHK(t->ctx, hipMemsetAsync(t->kgW, 0, 2 * nF * (size_t)p.nC * sizeof(double), t->ctx->stream));
        if (int rc = h2d(t->ctx, t->kgWdev, tab.data(), tab.size() * sizeof(double *))) return rc;
        t->wantK = want;
        return MOKA_OK;
    }
    // the new arrays first (each zeroed): a failure leaves the tape as it was
    double *P = nullptr, *Lk = nullptr, *W = nullptr, *ones = nullptr, *mOn = nullptr, *trDev = nullptr, *wDev = nullptr;
    int rc = MOKA_OK;
    if (nF > 0) {
        auto A = [&](double **q, size_t n) { if (rc == MOKA_OK) rc = ttape_alloc(t, q, n); };
        A(&P, nCK * 4 * nF * cap); A(&Lk, nCK * nF); A(&W, 2 * nF * (size_t)p.nC); A(&ones, nF); A(&mOn, cap * t->nT);
        A(&trDev, (nF * sizeof(int32_t) + sizeof(double) - 1) / sizeof(double)); A(&wDev, 2 * nF * sizeof(double *) / sizeof(double));
        if (rc == MOKA_OK) {
            std::vector<double> one(nF, 1.0);
            std::vector<double *> tab(2 * nF, nullptr);
            for (size_t f = 0; f < nF; ++f) {
                if (want[tr[f]] & MOKA_TRACER_GRAD_KAPPA) tab[2 * f] = W + (2 * f) * (size_t)p.nC;
                if (want[tr[f]] & MOKA_TRACER_GRAD_KAPPA4) tab[2 * f + 1] = W + (2 * f + 1) * (size_t)p.nC;
            }
            rc = h2d(t->ctx, ones, one.data(), nF * sizeof(double));
            if (rc == MOKA_OK) rc = h2d(t->ctx, trDev, tr.data(), nF * sizeof(int32_t));
            if (rc == MOKA_OK) rc = h2d(t->ctx, wDev, tab.data(), tab.size() * sizeof(double *));
        }
        if (rc != MOKA_OK) {
            (void)hipStreamSynchronize(t->ctx->stream);
            for (double *q : {P, Lk, W, ones, mOn, trDev, wDev}) ttape_free(t, q);
            return rc;
        }
    }
    for (void *q : {(void *)t->kgP, (void *)t->kgL, (void *)t->kgW, (void *)t->kgOnes, (void *)t->kgMOn, (void *)t->kgTracerDev, (void *)t->kgWdev})
        ttape_free(t, q);
    t->kgP = P; t->kgL = Lk; t->kgW = W; t->kgOnes = ones; t->kgMOn = mOn;
    t->kgTracerDev = reinterpret_cast<int32_t *>(trDev); t->kgWdev = reinterpret_cast<double **>(wDev);
    t->wantK = want;
    t->kgTracer = tr;
    return MOKA_OK;
}

// the row of kgW that holds the density `what` of tracer j, or an error
static int kgrad_row(moka_tracer_tape *t, int32_t j, int what, const void *out, const double **row)
{
    if (!t) return fail(nullptr, MOKA_ERR_ARG, "tracer tape is NULL");
    if (j < 0 || j >= t->nT) return fail(t->ctx, MOKA_ERR_ARG, "tracer index out of range (moka_tracer_tape_create)");
    if (!out) return fail(t->ctx, MOKA_ERR_ARG, "NULL argument");
    if (what != MOKA_TRACER_GRAD_KAPPA && what != MOKA_TRACER_GRAD_KAPPA4)
        return fail(t->ctx, MOKA_ERR_ARG, "tracer tape: what must be exactly one of MOKA_TRACER_GRAD_KAPPA, MOKA_TRACER_GRAD_KAPPA4");
    if (!(t->wantK[j] & what))
        return fail(t->ctx, MOKA_ERR_ARG, "tracer tape: this gradient was not asked for (moka_tracer_adjoint_want_diffusivity_gradient)");
    const size_t f = std::lower_bound(t->kgTracer.begin(), t->kgTracer.end(), j) - t->kgTracer.begin();
    *row = t->kgW + (2 * f + (what == MOKA_TRACER_GRAD_KAPPA4 ? 1 : 0)) * (size_t)t->st->mesh->plan.nC;
    return MOKA_OK;
}

int moka_tracer_adjoint_diffusivity_density_download(moka_tracer_tape *t, int32_t j, int what, double *host)
{
    const double *row = nullptr;
    if (int rc = kgrad_row(t, j, what, host, &row)) return rc;
    HIPCHK(t->ctx, hipSetDevice(t->ctx->device));
    return get_rows(t->st->mesh, host, row, MOKA_CELL, t->st->mesh->plan.nC, 1);
}

int moka_tracer_adjoint_diffusivity_gradient(moka_tracer_tape *t, int32_t j, int what, double *out)
{
    const double *row = nullptr;
    if (int rc = kgrad_row(t, j, what, out, &row)) return rc;
    HIPCHK(t->ctx, hipSetDevice(t->ctx->device));
    std::vector<double> w((size_t)t->st->mesh->plan.nC);
    if (int rc = get_rows(t->st->mesh, w.data(), row, MOKA_CELL, (int64_t)w.size(), 1)) return rc;
    long double sum = 0.0L;            // the caller's cell numbering, ascending, one rounding at the end: independent of the plan's order
    for (double v : w) sum += (long double)v;
    *out = (double)sum;
    return MOKA_OK;
}

// ---- d J / d kappaV_j (include/moka_hip.h: the algebra; the gradient instances of tracer_vmix.hip) ----
int moka_tracer_adjoint_want_vertical_gradient(moka_tracer_tape *t, int32_t j, int on)
{
    if (!t) return fail(nullptr, MOKA_ERR_ARG, "tracer tape is NULL");
    if (j < 0 || j >= t->nT) return fail(t->ctx, MOKA_ERR_ARG, "tracer index out of range (moka_tracer_tape_create)");
    if (t->n > 0) return fail(t->ctx, MOKA_ERR_ARG, "tracer tape: the vertical gradient may be chosen only while the tape holds no recorded step");
    if (t->pending) return fail(t->ctx, MOKA_ERR_ARG, "tracer tape: not between a seed and its sweep");
    HIPCHK(t->ctx, hipSetDevice(t->ctx->device));
    std::vector<char> want = t->wantV;
    want[j] = on ? 1 : 0;
    if (want == t->wantV) return MOKA_OK;
    const Plan &p = t->st->mesh->plan;
    std::vector<int32_t> tr, slot((size_t)t->nT, -1);
    for (int i = 0; i < t->nT; ++i)
        if (want[i]) { slot[i] = (int32_t)tr.size(); tr.push_back(i); }
    const size_t nV = tr.size(), nCK = (size_t)p.K * p.nC, cap = (size_t)t->capacity;
    HIPCHK(t->ctx, hipStreamSynchronize(t->ctx->stream));        // no launch is reading what goes
    // the new arrays first (each zeroed): a failure leaves the tape as it was
    double *P = nullptr, *D = nullptr, *sl = nullptr;
    if (nV > 0) {
        int rc = MOKA_OK;
        auto A = [&](double **q, size_t n) { if (rc == MOKA_OK) rc = ttape_alloc(t, q, n); };
        A(&P, nCK * nV * cap); A(&D, nCK * nV); A(&sl, ((size_t)t->nT * sizeof(int32_t) + sizeof(double) - 1) / sizeof(double));
        if (rc == MOKA_OK) rc = h2d(t->ctx, sl, slot.data(), slot.size() * sizeof(int32_t));
        if (rc != MOKA_OK) {
            (void)hipStreamSynchronize(t->ctx->stream);
            for (double *q : {P, D, sl}) ttape_free(t, q);
            return rc;
        }
    }
    for (void *q : {(void *)t->vgP, (void *)t->vgD, (void *)t->vgSlot}) ttape_free(t, q);
    t->vgP = P; t->vgD = D; t->vgSlot = reinterpret_cast<int32_t *>(sl);
    t->wantV = want;
    t->vgTracer = tr;
    return MOKA_OK;
}

// the density of tracer j in the caller's cell numbering, (K, nC) as every field, or an error
static int vgrad_density(moka_tracer_tape *t, int32_t j, const void *out, std::vector<double> &d)
{
    if (!t) return fail(nullptr, MOKA_ERR_ARG, "tracer tape is NULL");
    if (j < 0 || j >= t->nT) return fail(t->ctx, MOKA_ERR_ARG, "tracer index out of range (moka_tracer_tape_create)");
    if (!out) return fail(t->ctx, MOKA_ERR_ARG, "NULL argument");
    if (!t->wantV[j]) return fail(t->ctx, MOKA_ERR_ARG, "tracer tape: this gradient was not asked for (moka_tracer_adjoint_want_vertical_gradient)");
    HIPCHK(t->ctx, hipSetDevice(t->ctx->device));
    const Plan &p = t->st->mesh->plan;
    const size_t f = std::lower_bound(t->vgTracer.begin(), t->vgTracer.end(), j) - t->vgTracer.begin();
    d.resize((size_t)p.K * p.nC);
    return get_rows(t->st->mesh, d.data(), t->vgD + f * d.size(), MOKA_CELL, p.nC, p.K);
}

int moka_tracer_adjoint_vertical_density_download(moka_tracer_tape *t, int32_t j, int view, double *host)
{
    if (t && view != MOKA_VGRAD_INTERFACE && view != MOKA_VGRAD_CELL && view != MOKA_VGRAD_PROFILE)
        return fail(t->ctx, MOKA_ERR_ARG, "tracer tape: view must be MOKA_VGRAD_INTERFACE, MOKA_VGRAD_CELL or MOKA_VGRAD_PROFILE");
    std::vector<double> d;
    if (int rc = vgrad_density(t, j, host, d)) return rc;
    const int64_t K = t->st->mesh->plan.K, nC = t->st->mesh->plan.nC;
    if (view == MOKA_VGRAD_INTERFACE) {
        std::copy(d.begin(), d.end(), host);
    } else if (view == MOKA_VGRAD_CELL) {         // ascending k, long double, one rounding
        for (int64_t c = 0; c < nC; ++c) {
            long double sum = 0.0L;
            for (int64_t k = 0; k < K; ++k) sum += (long double)d[(size_t)(c * K + k)];
            host[c] = (double)sum;
        }
    } else {                                      // ascending over the caller's cells
        for (int64_t k = 0; k < K; ++k) {
            long double sum = 0.0L;
            for (int64_t c = 0; c < nC; ++c) sum += (long double)d[(size_t)(c * K + k)];
            host[k] = (double)sum;
        }
    }
    return MOKA_OK;
}

int moka_tracer_adjoint_vertical_gradient(moka_tracer_tape *t, int32_t j, double *out)
{
    std::vector<double> d;
    if (int rc = vgrad_density(t, j, out, d)) return rc;
    long double sum = 0.0L;            // cell-major over the caller's numbering, one rounding at the end: independent of the plan's order
    for (double v : d) sum += (long double)v;
    *out = (double)sum;
    return MOKA_OK;
}

// ---------------------------------------------------------------------------------------------
// reverse mode of the Forward-Euler loop.  The reference differentiates
// ocn_run_loop with Enzyme (ext/MPASEnzymeExt.jl; test/enzyme/test_Enzyme_end2end.jl: d sum(ssh^2) / d initial
// layerThickness, normalVelocity); here the tape and the transposed kernels are written by hand.
// ---------------------------------------------------------------------------------------------
struct moka_tape {
    moka_state *st = nullptr;
    int64_t capacity = 0, n = 0;
    double *uTape = nullptr, *hTape = nullptr;      // capacity x (K, nE): u_n and the hEdge the flux of step n used
    std::vector<double> dts;
    std::vector<int> flags;
    double *lamU[2] = {nullptr, nullptr}, *lamH[2] = {nullptr, nullptr}, *lamS[2] = {nullptr, nullptr}, *lamE[2] = {nullptr, nullptr};
    double *Enew = nullptr, *csum = nullptr;
    // RK4: per step the four provisional states the tendencies were evaluated at; work arrays of the reverse step
    double *rkU = nullptr, *rkH = nullptr;          // capacity x 4 x (K, nE) / (K, nC), allocated at the first RK4 step
    double *kbU = nullptr, *kbH = nullptr, *pbU = nullptr, *pbH = nullptr;
    int kind = -1;                                   // -1 empty, 0 Forward Euler, 1 RK4 (one integrator per tape)
    int cur = 0;                                     // index of the adjoint state that is current
    int revNext = 4;                                 // stage-wise reverse RK4 step (moka_adjoint_rk4_stage): the stage that comes next
    int revPart = 0;                                 // ... and, part by part (moka_adjoint_rk4_stage_part), which part of it
    int recMask = 0;                                 // piecewise taping (moka_tape_record_rk4): slots of the open step already filled
    bool seeded = false;
    moka::AdjMesh am{};
    std::vector<void *> allocs;
    bool counted = false;                            // st->attached includes this tape
    bool forced = false;                             // the tape a moka_forced_tape embeds: counted in st->forcedTapes
};

static int tape_alloc(moka_tape *t, void **out, size_t bytes)
{
    void *d = nullptr;
    hipError_t e = hipMalloc(&d, std::max<size_t>(bytes, 16));
    if (e != hipSuccess)
        return fail(t->st->ctx, MOKA_ERR_ALLOC, std::string("tape: hipMalloc of ") + std::to_string(bytes) + " bytes: " + hipGetErrorString(e));
    t->allocs.push_back(d);
    HIPCHK(t->st->ctx, hipMemsetAsync(d, 0, bytes, t->st->ctx->stream));
    *out = d;
    return MOKA_OK;
}

extern "C++" {
template <class T>
static int tape_upload(moka_tape *t, const std::vector<T> &v, const T **out)
{
    void *d = nullptr;
    int rc = tape_alloc(t, &d, v.size() * sizeof(T));
    if (rc) return rc;
    // on the context's stream, behind tape_alloc's memset: a plain hipMemcpy runs on the null stream, which the (non-blocking)
    // context stream does not order against -- once in ~1500 tapes the zero fill landed after the copy and wiped the lists
    if ((rc = h2d(t->st->ctx, d, v.data(), v.size() * sizeof(T)))) return rc;     // v is a temporary of the caller
    *out = static_cast<const T *>(d);
    return MOKA_OK;
}
}  // extern "C++"

// forced: the tape inside a moka_forced_tape, which transposes the vertical momentum pass itself
static int tape_create(moka_state *st, int64_t capacity_steps, moka_tape **out, bool forced)
{
    if (!st || !out || capacity_steps < 0) return fail(st ? st->ctx : nullptr, MOKA_ERR_ARG, "bad argument");
    *out = nullptr;
    if (st->f32) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "reverse mode: Float64 states only");
    if (st->nonlinear) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "reverse mode covers the reference's linear terms only");
    if (st->nTracers > 0) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "tracers: no reverse mode (moka_set_tracers(st, 0) first)");
    if (!forced && mom_vmix_on(st)) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "vertical momentum mixing: no reverse mode (moka_set_vertical_viscosity(st, 0, 0) and a NULL stress first)");
    if (st->forcedTapes > 0) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "reverse mode: a moka_forced_tape of this state exists");
    const Plan &p = st->mesh->plan;
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    // transposed Coriolis stencil, sources sorted by (caller's edge id, slot): the oracle's summation order
    const int nE = p.nE, nC = p.nC, ME = p.ME, ME2 = p.ME2;
    std::vector<std::vector<std::pair<std::pair<int32_t, int32_t>, int32_t>>> lists(nE);   // ((orig src, slot), new src)
    for (int s = 0; s < nE; ++s)
        for (int i = 0; i < ME2; ++i) {
            const int tgt = p.eoe[(size_t)s * ME2 + i];
            if (tgt >= 0) lists[tgt].push_back({{p.edgeN2O[s], i}, s});
        }
    int W = 1;
    for (auto &l : lists) { std::sort(l.begin(), l.end()); W = std::max(W, (int)l.size()); }
    std::vector<int32_t> teoe((size_t)nE * W, -1), csgn((size_t)nC * ME, 0);
    std::vector<double> tw((size_t)nE * W, 0.0), sd((size_t)nE * 2, 0.0);
    for (int e = 0; e < nE; ++e)
        for (size_t j = 0; j < lists[e].size(); ++j) {
            const int s = lists[e][j].second, i = lists[e][j].first.second;
            teoe[(size_t)e * W + j] = s;
            tw[(size_t)e * W + j] = p.woe[(size_t)s * ME2 + i];
        }
    for (int c = 0; c < nC; ++c)
        for (int i = 0; i < ME; ++i)
            if (p.eoc[(size_t)c * ME + i] >= 0) csgn[(size_t)c * ME + i] = p.sdv[(size_t)c * ME + i] < 0.0 ? -1 : 1;
    for (int e = 0; e < nE; ++e) {
        const int cc[2] = {p.ehdr[(size_t)e * 4], p.ehdr[(size_t)e * 4 + 1]};
        // (cc[0] == cc[1]: an outermost edge of a rank-local mesh, both sides set to the inside halo cell.  Its adjoint is never
        //  computed here -- it arrives by exchange, like its forward value -- so its factors may be anything finite.)
        for (int q = 0; q < 2; ++q) {
            double sgn = 0.0;
            for (int i = 0; i < ME; ++i)
                if (p.eoc[(size_t)cc[q] * ME + i] == e) { sgn = (double)csgn[(size_t)cc[q] * ME + i]; break; }
            sd[(size_t)e * 2 + q] = p.dvEdge[e] * sgn * p.invArea[cc[q]];
        }
    }
    moka_tape *t = new (std::nothrow) moka_tape();
    if (!t) return fail(st->ctx, MOKA_ERR_ALLOC, "out of host memory");
    t->st = st;
    t->capacity = capacity_steps;
    const size_t nEK = (size_t)p.K * nE, nCK = (size_t)p.K * nC;
    int rc = MOKA_OK;
    auto A = [&](double **q, size_t n) { if (rc == MOKA_OK) { void *d = nullptr; rc = tape_alloc(t, &d, n * sizeof(double)); *q = static_cast<double *>(d); } };
    A(&t->uTape, nEK * (size_t)capacity_steps); A(&t->hTape, nEK * (size_t)capacity_steps);
    for (int b = 0; b < 2; ++b) { A(&t->lamU[b], nEK); A(&t->lamH[b], nCK); A(&t->lamS[b], nC); A(&t->lamE[b], nEK); }
    A(&t->Enew, nEK); A(&t->csum, nE);
    moka::AdjMesh &am = t->am;
    am.nC = nC; am.nE = nE; am.K = p.K; am.ME = ME; am.W = W;
    am.eBegin = 0; am.eCount = nE; am.cBegin = 0; am.cCount = nC;
    am.eoc = st->mesh->dev.eoc; am.ehdr = st->mesh->dev.ehdr; am.fEdge = st->mesh->dev.fEdge; am.gInvDc = st->mesh->dev.gInvDc;
    if (rc == MOKA_OK) rc = tape_upload(t, teoe, &am.teoe);
    if (rc == MOKA_OK) rc = tape_upload(t, tw, &am.tw);
    if (rc == MOKA_OK) rc = tape_upload(t, sd, &am.sd);
    if (rc == MOKA_OK) rc = tape_upload(t, csgn, &am.csgn);
    {   // regular edges (everything but the neighbourhood of the 12 pentagons on a sphere without land): mask-free path
        std::vector<int32_t> efull(nE, 0);
        for (int e = 0; e < nE; ++e) {
            bool full = p.ehdr[(size_t)e * 4 + 3] >= p.K;
            for (int j = 0; j < W && full; ++j) {
                const int sidx = teoe[(size_t)e * W + j];
                full = sidx >= 0 && p.ehdr[(size_t)sidx * 4 + 3] >= p.K;
            }
            efull[e] = full ? 1 : 0;
        }
        if (rc == MOKA_OK) rc = tape_upload(t, efull, &am.efull);
    }
    if (rc != MOKA_OK) { moka_tape_destroy(t); return rc; }
    HIPCHK(st->ctx, hipStreamSynchronize(st->ctx->stream));
    state_attach(st);
    t->counted = true;
    t->forced = forced;
    ++(forced ? st->forcedTapes : st->dycoreTapes);
    *out = t;
    return MOKA_OK;
}

int moka_tape_create(moka_state *st, int64_t capacity_steps, moka_tape **out) { return tape_create(st, capacity_steps, out, false); }

void moka_tape_destroy(moka_tape *t)
{
    if (!t) return;
    if (t->counted) { state_detach(t->st); --(t->forced ? t->st->forcedTapes : t->st->dycoreTapes); }
    (void)hipSetDevice(t->st->ctx->device);
    if (t->st->lazyOwner == t) {        // the stage-4 tendencies of the last taped step would be produced from a slot of this tape
        if (t->st->tendDirty) (void)flush_lazy(t->st, false, true);
        t->st->lazyPu = t->st->lazyPh = nullptr; t->st->lazyOwner = nullptr;
    }
    (void)hipStreamSynchronize(t->st->ctx->stream);
    for (void *q : t->allocs) (void)hipFree(q);
    delete t;
}

int moka_step_fe_taped(moka_tape *t, double dt, int flags)
{
    if (!t) return fail(nullptr, MOKA_ERR_ARG, "tape is NULL");
    moka_state *st = t->st;
    const Plan &p = st->mesh->plan;
    if (t->n >= t->capacity) return fail(st->ctx, MOKA_ERR_ARG, "tape is full");
    if ((flags & MOKA_FE_LEVEL1_ONLY) && p.K != 1)
        return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "reverse mode: level-1-only stepping is supported for nVertLevels = 1 only");
    if (t->n > 0 && t->kind != 0) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "reverse mode: one integrator per tape");
    t->kind = 0;
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    int rc = flush_lazy(st, true, true);
    if (rc) return rc;
    hipStream_t s = st->ctx->stream;
    const size_t nEK = (size_t)p.K * p.nE, bytes = nEK * sizeof(double);
    HIPCHK(st->ctx, hipMemcpyAsync(t->uTape + nEK * t->n, st->lev[1].u, bytes, hipMemcpyDeviceToDevice, s));
    const bool stale = flags & MOKA_FE_STALE_HEDGE;
    if (stale) HIPCHK(st->ctx, hipMemcpyAsync(t->hTape + nEK * t->n, st->hEdge[0], bytes, hipMemcpyDeviceToDevice, s));
    st->feForceEager = true;            // the tape copies DiagnosticVars around the step: it stores all of its arrays
    rc = moka_step_fe(st, dt, flags);
    st->feForceEager = false;
    if (rc) return rc;
    // a refreshed layerThicknessEdge (= interp of the pre-step thickness) is what the flux used: it is Diag's after the step
    if (!stale) HIPCHK(st->ctx, hipMemcpyAsync(t->hTape + nEK * t->n, st->hEdge[0], bytes, hipMemcpyDeviceToDevice, s));
    t->dts.push_back(dt);
    t->flags.push_back(flags);
    ++t->n;
    t->seeded = false;
    return MOKA_OK;
}

int moka_step_rk4_taped(moka_tape *t, double dt)
{
    if (!t) return fail(nullptr, MOKA_ERR_ARG, "tape is NULL");
    moka_state *st = t->st;
    const Plan &p = st->mesh->plan;
    if (t->n >= t->capacity) return fail(st->ctx, MOKA_ERR_ARG, "tape is full");
    if (t->n > 0 && t->kind != 1) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "reverse mode: one integrator per tape");
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    const size_t nEK = (size_t)p.K * p.nE, nCK = (size_t)p.K * p.nC;
    int rc = MOKA_OK;
    if (!t->rkU) {
        auto A = [&](double **q, size_t n) { if (rc == MOKA_OK) { void *d = nullptr; rc = tape_alloc(t, &d, n * sizeof(double)); *q = static_cast<double *>(d); } };
        A(&t->rkU, nEK * 4 * (size_t)t->capacity); A(&t->rkH, nCK * 4 * (size_t)t->capacity);
        A(&t->kbU, nEK); A(&t->kbH, nCK); A(&t->pbU, nEK); A(&t->pbH, nCK);
        if (rc) return rc;
    }
    const double *ssh0 = nullptr;       // like moka_step_rk4: pending lazy diagnostics / tendencies of the previous step are simply superseded
    if ((rc = rk4_begin(st, &ssh0))) return rc;
    hipStream_t s = st->ctx->stream;
    double *tu = t->rkU + nEK * 4 * t->n, *th = t->rkH + nCK * 4 * t->n;
    // The tape needs the provisional states P1..P4 the four tendencies are evaluated at.  P1 (the current level) is copied;
    // P2, P3 and P4 are written by stages 1, 2 and 3 straight into their tape slots and read from there by the next stage
    // (and, P4, by the lazily produced stage-4 tendencies: moka_state.lazyPu / lazyPh).
    auto slotU = [&](int i) { return tu + nEK * i; };
    auto slotH = [&](int i) { return th + nCK * i; };
    HIPCHK(st->ctx, hipMemcpyAsync(slotU(0), st->lev[1].u, nEK * sizeof(double), hipMemcpyDeviceToDevice, s));
    HIPCHK(st->ctx, hipMemcpyAsync(slotH(0), st->lev[1].h, nCK * sizeof(double), hipMemcpyDeviceToDevice, s));
    for (int sg = 1; sg <= 4; ++sg) {
        StageArgs g = rk4_stage_args(st, sg, dt, ssh0);
        if (sg >= 2) { g.pu = slotU(sg - 1); g.ph = slotH(sg - 1); }
        if (sg <= 3) { g.pu_out = slotU(sg); g.ph_out = slotH(sg); }
        HIPCHK(st->ctx, run_stage(st, g));
    }
    rk4_end(st);
    st->lazyPu = slotU(3); st->lazyPh = slotH(3); st->lazyOwner = t;
    t->kind = 1;
    t->dts.push_back(dt);
    t->flags.push_back(0);
    ++t->n;
    t->seeded = false;
    return MOKA_OK;
}

// Piecewise taping for a step the caller runs itself (the distributed RK4 step, whose stages are separated by halo
// exchanges): slot 0..3 of the step being recorded := (normalVelocity, layerThickness) of buffer set `what` (0 = the current
// level, 1..3 = the output of RK stage `what`), halo rows included; moka_tape_commit_rk4 closes the step.
int moka_tape_record_rk4(moka_tape *t, int slot, int what)
{
    if (!t) return fail(nullptr, MOKA_ERR_ARG, "tape is NULL");
    moka_state *st = t->st;
    const Plan &p = st->mesh->plan;
    if (slot < 0 || slot > 3 || what < 0 || what > 3) return fail(st->ctx, MOKA_ERR_ARG, "slot and what must be 0..3");
    if (t->n >= t->capacity) return fail(st->ctx, MOKA_ERR_ARG, "tape is full");
    if (t->n > 0 && t->kind != 1) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "reverse mode: one integrator per tape");
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    const size_t nEK = (size_t)p.K * p.nE, nCK = (size_t)p.K * p.nC;
    int rc = MOKA_OK;
    if (!t->rkU) {
        auto A = [&](double **q, size_t n) { if (rc == MOKA_OK) { void *d = nullptr; rc = tape_alloc(t, &d, n * sizeof(double)); *q = static_cast<double *>(d); } };
        A(&t->rkU, nEK * 4 * (size_t)t->capacity); A(&t->rkH, nCK * 4 * (size_t)t->capacity);
        A(&t->kbU, nEK); A(&t->kbH, nCK); A(&t->pbU, nEK); A(&t->pbH, nCK);
        if (rc) return rc;
    }
    if ((rc = ensure_rk_bufs(st))) return rc;
    const LevelBufs &o = rk4_stage_output(st, what);
    hipStream_t s = st->ctx->stream;
    // the rows may have been produced on either stream (boundary patches, halo unpack): the copy waits for both
    HIPCHK(st->ctx, hipEventRecord(st->ctx->evHalo, st->ctx->comm));
    HIPCHK(st->ctx, hipStreamWaitEvent(s, st->ctx->evHalo, 0));
    HIPCHK(st->ctx, hipMemcpyAsync(t->rkU + nEK * (4 * t->n + slot), o.u, nEK * sizeof(double), hipMemcpyDeviceToDevice, s));
    HIPCHK(st->ctx, hipMemcpyAsync(t->rkH + nCK * (4 * t->n + slot), o.h, nCK * sizeof(double), hipMemcpyDeviceToDevice, s));
    t->recMask |= 1 << slot;
    return MOKA_OK;
}

// The same for a Forward-Euler step the caller runs itself (moka_fe_dist_step): after = 0 before the step (normalVelocity and,
// with MOKA_FE_STALE_HEDGE, the carried layerThicknessEdge the flux is about to use), after = 1 behind it (without the flag:
// the refreshed layerThicknessEdge the flux used, Diag's after the step); moka_tape_commit_fe closes the step.
int moka_tape_record_fe(moka_tape *t, int flags, int after)
{
    if (!t) return fail(nullptr, MOKA_ERR_ARG, "tape is NULL");
    moka_state *st = t->st;
    const Plan &p = st->mesh->plan;
    if (t->n >= t->capacity) return fail(st->ctx, MOKA_ERR_ARG, "tape is full");
    if ((flags & MOKA_FE_LEVEL1_ONLY) && p.K != 1)
        return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "reverse mode: level-1-only stepping is supported for nVertLevels = 1 only");
    if (t->n > 0 && t->kind != 0) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "reverse mode: one integrator per tape");
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    hipStream_t s = st->ctx->stream;
    const size_t nEK = (size_t)p.K * p.nE, bytes = nEK * sizeof(double);
    const bool stale = flags & MOKA_FE_STALE_HEDGE;
    HIPCHK(st->ctx, hipEventRecord(st->ctx->evHalo, st->ctx->comm));       // rows produced on either stream
    HIPCHK(st->ctx, hipStreamWaitEvent(s, st->ctx->evHalo, 0));
    if (!after) {
        if (int rc = flush_lazy(st, true, true)) return rc;
        st->feForceEager = true;        // until moka_tape_commit_fe: the recorded step stores all of its arrays
        HIPCHK(st->ctx, hipMemcpyAsync(t->uTape + nEK * t->n, st->lev[1].u, bytes, hipMemcpyDeviceToDevice, s));
        if (stale) HIPCHK(st->ctx, hipMemcpyAsync(t->hTape + nEK * t->n, st->hEdge[0], bytes, hipMemcpyDeviceToDevice, s));
        t->recMask = 1;
    } else {
        if (t->recMask != 1) return fail(st->ctx, MOKA_ERR_ARG, "moka_tape_record_fe: record before the step first");
        if (!stale) HIPCHK(st->ctx, hipMemcpyAsync(t->hTape + nEK * t->n, st->hEdge[0], bytes, hipMemcpyDeviceToDevice, s));
        t->recMask = 3;
    }
    return MOKA_OK;
}

int moka_tape_commit_fe(moka_tape *t, double dt, int flags)
{
    if (!t) return fail(nullptr, MOKA_ERR_ARG, "tape is NULL");
    if (t->recMask != 3) return fail(t->st->ctx, MOKA_ERR_ARG, "moka_tape_commit_fe: record before and after the step first");
    t->st->feForceEager = false;
    t->recMask = 0;
    t->kind = 0;
    t->dts.push_back(dt);
    t->flags.push_back(flags);
    ++t->n;
    t->seeded = false;
    return MOKA_OK;
}

int moka_tape_commit_rk4(moka_tape *t, double dt)
{
    if (!t) return fail(nullptr, MOKA_ERR_ARG, "tape is NULL");
    if (t->recMask != 15) return fail(t->st->ctx, MOKA_ERR_ARG, "moka_tape_commit_rk4: record the four provisional states first");
    t->recMask = 0;
    t->kind = 1;
    t->dts.push_back(dt);
    t->flags.push_back(0);
    ++t->n;
    t->seeded = false;
    return MOKA_OK;
}

int moka_adjoint_seed_sum_sq_ssh(moka_tape *t)
{
    if (!t) return fail(nullptr, MOKA_ERR_ARG, "tape is NULL");
    moka_state *st = t->st;
    const Plan &p = st->mesh->plan;
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    hipStream_t s = st->ctx->stream;
    const size_t nEK = (size_t)p.K * p.nE, nCK = (size_t)p.K * p.nC;
    t->cur = 0;
    HIPCHK(st->ctx, hipMemsetAsync(t->lamU[0], 0, nEK * sizeof(double), s));
    HIPCHK(st->ctx, hipMemsetAsync(t->lamH[0], 0, nCK * sizeof(double), s));
    HIPCHK(st->ctx, hipMemsetAsync(t->lamE[0], 0, nEK * sizeof(double), s));
    if (t->kind == 1) {
        // RK4: ssh is recomputed from layerThickness inside every tendency, so the objective lives on h: every level gets 2 ssh
        for (int b = 0; b < 2; ++b) {   // the RK4 sweep never writes the ssh / layerThicknessEdge adjoints: both stay zero
            HIPCHK(st->ctx, hipMemsetAsync(t->lamS[b], 0, (size_t)p.nC * sizeof(double), s));
            HIPCHK(st->ctx, hipMemsetAsync(t->lamE[b], 0, nEK * sizeof(double), s));
        }
        HIPCHK(st->ctx, launch_bcast_rows(t->lamH[0], st->lev[1].ssh, 2.0, p.nC, p.K, s));
    } else {
        HIPCHK(st->ctx, launch_scale_copy(t->lamS[0], st->lev[1].ssh, 2.0, p.nC, s));      // d sum(ssh^2) = 2 ssh
    }
    t->seeded = true;
    return MOKA_OK;
}

// one stage (sg = 4, 3, 2, 1) of one RK4 step backwards (time_integration.jl:61-148 transposed):
//   kb4 = b4*X; Pb = T'(P4)^T kb4; acc = X + Pb;  for s = 3,2,1: kb = b_s*X + a_s*Pb; Pb = T'(P_s)^T kb; acc += Pb;  X = acc
// sg == 1 completes the step (the adjoint states swap, the step is popped).  Between two stages the host layer of a partitioned
// run exchanges the halo rows of the k-bar the next stage gathers from (rk4_reverse_fields).
static void rk4_reverse_fields(moka_tape *t, int sg, double **fU, double **fH)
{
    double *kU[2] = {t->kbU, t->pbU}, *kH[2] = {t->kbH, t->pbH};
    const int kc = (4 - sg) & 1;                      // stage 4 reads k-bar 0 (or X itself), 3 reads 1, 2 reads 0, 1 reads 1
    *fU = sg == 4 ? t->lamU[t->cur] : kU[kc];
    *fH = sg == 4 ? t->lamH[t->cur] : kH[kc];
}

// part < 0: every local entity; 0 / 1: the edges and cells of cell class 0 (boundary: what other ranks gather from) / 1 (interior)
static int rk4_reverse_stage(moka_tape *t, int sg, int part = -1)
{
    moka_state *st = t->st;
    const Plan &p = st->mesh->plan;
    hipStream_t s = st->ctx->stream;
    const size_t nEK = (size_t)p.K * p.nE, nCK = (size_t)p.K * p.nC;
    const int64_t i = t->n - 1;
    const double dt = t->dts[i];
    const double ca[3] = {dt / 2., dt / 2., dt}, cb[4] = {dt / 6., dt / 3., dt / 3., dt / 6.};
    const int in = t->cur, o = 1 - t->cur;
    const double *XU = t->lamU[in], *XH = t->lamH[in];
    double *accU = t->lamU[o], *accH = t->lamH[o];
    // every k-bar after the first, and the running sum X + Pb4 + Pb3 + ..., come out of the two transposed kernels themselves
    // (fused epilogues: AdjArgs.accOut / kNext), k-bar double-buffered because the current one is being gathered while the
    // next one is written
    double *kU[2] = {t->kbU, t->pbU}, *kH[2] = {t->kbH, t->pbH};
    // chunk kernels (even K <= 64, hexagon-width lists): stage 4 reads X scaled on the fly (kb4 is never stored) and
    // u*Fbar is recomputed by the cell kernel instead of travelling through memory
    const bool fused = moka::adj_fused_available(t->am, st->mesh->lpc);
    moka::AdjMesh am = t->am;
    if (part >= 0) {
        if (!fused) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "reverse RK4 stages part by part need the chunk kernels (even 34 <= K <= 64, hexagon-width lists)");
        if ((int)p.classCellStart.size() < 3) return fail(st->ctx, MOKA_ERR_ARG, "the mesh has no cell classes (moka_mesh_desc.cellClass)");
        am.cBegin = p.classCellStart[part]; am.cCount = p.classCellStart[part + 1] - am.cBegin;
        am.eBegin = p.classEdgeStart[part]; am.eCount = p.classEdgeStart[part + 1] - am.eBegin;
    }
    if (sg == 4 && !fused) {
        HIPCHK(st->ctx, launch_scale_copy(kU[0], XU, cb[3], (int64_t)nEK, s));
        HIPCHK(st->ctx, launch_scale_copy(kH[0], XH, cb[3], (int64_t)nCK, s));
    }
    const int kc = (4 - sg) & 1;
    moka::AdjArgs a{};
    a.tt = 1; a.dt = 1.0;
    a.u = t->rkU + nEK * (4 * i + (sg - 1)); a.h = t->rkH + nCK * (4 * i + (sg - 1));
    a.lamU1 = kU[kc]; a.lamH1 = kH[kc];
    a.lamScale = 1.0; a.fuseE = fused ? 1 : 0;
    if (fused && sg == 4) { a.lamU1 = XU; a.lamH1 = XH; a.lamScale = cb[3]; }
    a.Enew = t->Enew; a.csum = t->csum;
    a.xU = XU; a.xH = XH;
    a.accInU = sg == 4 ? nullptr : accU; a.accInH = sg == 4 ? nullptr : accH;
    a.accOutU = accU; a.accOutH = accH;
    if (sg > 1) {
        a.kNextU = kU[1 - kc]; a.kNextH = kH[1 - kc];
        a.cbNext = cb[sg - 2]; a.caNext = ca[sg - 2];
    }
    HIPCHK(st->ctx, launch_adj_edge(am, a, st->mesh->lpc, s));     // the cell kernel reads csum of the cells' edges: written by the edge
    HIPCHK(st->ctx, launch_adj_cell(am, a, st->mesh->lpc, s));     // kernel of the same part or (interior cells) of the boundary part
    if (part == 0) return MOKA_OK;                                 // the step's bookkeeping moves with the last part
    if (sg == 1) {
        t->cur = o;
        t->dts.pop_back(); t->flags.pop_back();
        --t->n;
    }
    return MOKA_OK;
}

// one Forward-Euler step backwards (the transposition of oracle_step_fe: see oracle_step_fe_adjoint)
static int fe_reverse_step(moka_tape *t)
{
    moka_state *st = t->st;
    const Plan &p = st->mesh->plan;
    hipStream_t s = st->ctx->stream;
    const size_t nEK = (size_t)p.K * p.nE;
    const int64_t i = t->n - 1;
    const int in = t->cur, o = 1 - t->cur;
    moka::AdjArgs a{};
    a.dt = t->dts[i];
    a.stale = (t->flags[i] & MOKA_FE_STALE_HEDGE) ? 1 : 0;
    a.u = t->uTape + nEK * i; a.hEuse = t->hTape + nEK * i;
    a.lamU1 = t->lamU[in]; a.lamH1 = t->lamH[in]; a.lamS1 = t->lamS[in]; a.lamE1 = t->lamE[in];
    a.lamU0 = t->lamU[o]; a.lamH0 = t->lamH[o]; a.lamS0 = t->lamS[o];
    a.Enew = a.stale ? t->lamE[o] : t->Enew;        // stale: u*Fbar IS the adjoint of the carried hEdge
    a.csum = t->csum;
    HIPCHK(st->ctx, launch_adj_edge(t->am, a, st->mesh->lpc, s));
    HIPCHK(st->ctx, launch_adj_cell(t->am, a, st->mesh->lpc, s));
    if (!a.stale) HIPCHK(st->ctx, hipMemsetAsync(t->lamE[o], 0, nEK * sizeof(double), s));
    t->cur = o;
    t->dts.pop_back(); t->flags.pop_back();
    --t->n;
    return MOKA_OK;
}

int moka_adjoint_fe_step_fields(moka_tape *t, void **fieldU, void **fieldH, void **fieldS)
{
    if (!t || !fieldU || !fieldH || !fieldS) return fail(t ? t->st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    if (t->kind != 0 || t->n <= 0) return fail(t->st->ctx, MOKA_ERR_ARG, "no recorded Forward-Euler step");
    *fieldU = t->lamU[t->cur]; *fieldH = t->lamH[t->cur]; *fieldS = t->lamS[t->cur];
    return MOKA_OK;
}

int moka_adjoint_fe_step(moka_tape *t)
{
    if (!t) return fail(nullptr, MOKA_ERR_ARG, "tape is NULL");
    moka_state *st = t->st;
    if (!t->seeded) return fail(st->ctx, MOKA_ERR_ARG, "seed the adjoint first (moka_adjoint_seed_sum_sq_ssh)");
    if (t->kind != 0 || t->n <= 0) return fail(st->ctx, MOKA_ERR_ARG, "no recorded Forward-Euler step");
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    return fe_reverse_step(t);
}

int moka_adjoint_rk4_stage_fields(moka_tape *t, int sg, void **fieldU, void **fieldH, void **scratchS)
{
    if (!t || !fieldU || !fieldH) return fail(t ? t->st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    if (sg < 1 || sg > 4 || t->kind != 1 || t->n <= 0) return fail(t->st->ctx, MOKA_ERR_ARG, "no recorded RK4 step / stage must be 4..1");
    double *fU, *fH;
    rk4_reverse_fields(t, sg, &fU, &fH);
    *fieldU = fU; *fieldH = fH;
    if (scratchS) *scratchS = t->lamS[1 - t->cur];     // an (nCells) array nothing reads: stands in for ssh in the exchange maps
    return MOKA_OK;
}

int moka_adjoint_rk4_stage(moka_tape *t, int sg)
{
    if (!t) return fail(nullptr, MOKA_ERR_ARG, "tape is NULL");
    moka_state *st = t->st;
    if (!t->seeded) return fail(st->ctx, MOKA_ERR_ARG, "seed the adjoint first (moka_adjoint_seed_sum_sq_ssh)");
    if (sg < 1 || sg > 4 || t->kind != 1 || t->n <= 0) return fail(st->ctx, MOKA_ERR_ARG, "no recorded RK4 step / stage must be 4..1");
    if (sg != t->revNext || t->revPart != 0) return fail(st->ctx, MOKA_ERR_ARG, "reverse RK4 stages run 4, 3, 2, 1");
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    if (int rc = rk4_reverse_stage(t, sg)) return rc;
    t->revNext = sg == 1 ? 4 : sg - 1;
    return MOKA_OK;
}

// The same stage in two launches on a partitioned mesh: part 0 = the entities of the boundary class (whose rows other ranks
// gather from in the next transposed stage), part 1 = the interior class.  Between the two the caller starts the exchange of
// the rows part 0 produced (moka_adjoint_rk4_stage_out_fields + moka_halo_pack_fields); it then overlaps part 1, which reads and
// writes owned rows only.  Halo entities are not computed at all (moka_adjoint_rk4_stage computes them redundantly).
int moka_adjoint_rk4_stage_part(moka_tape *t, int sg, int part)
{
    if (!t) return fail(nullptr, MOKA_ERR_ARG, "tape is NULL");
    moka_state *st = t->st;
    if (!t->seeded) return fail(st->ctx, MOKA_ERR_ARG, "seed the adjoint first (moka_adjoint_seed_sum_sq_ssh)");
    if (sg < 1 || sg > 4 || t->kind != 1 || t->n <= 0) return fail(st->ctx, MOKA_ERR_ARG, "no recorded RK4 step / stage must be 4..1");
    if (part < 0 || part > 1) return fail(st->ctx, MOKA_ERR_ARG, "part must be 0 (boundary class) or 1 (interior class)");
    if (sg != t->revNext || part != t->revPart) return fail(st->ctx, MOKA_ERR_ARG, "reverse RK4 stages run 4, 3, 2, 1, each as part 0 then part 1");
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    if (int rc = rk4_reverse_stage(t, sg, part)) return rc;
    t->revPart = 1 - part;
    if (part == 1) t->revNext = sg == 1 ? 4 : sg - 1;
    return MOKA_OK;
}

// 1: this tape's transposed RK4 stages can run class by class (the chunk kernels serve the mesh and the mesh has cell classes)
int moka_adjoint_rk4_parts_available(const moka_tape *t)
{
    if (!t) return 0;
    const moka_state *st = t->st;
    return moka::adj_fused_available(t->am, st->mesh->lpc) && (int)st->mesh->plan.classCellStart.size() >= 3 ? 1 : 0;
}

// The arrays stage `sg` of the reverse step in progress WRITES and the next transposed stage gathers from (stage sg - 1's k-bar;
// after stage 1: the adjoint state handed to the previous recorded step): what has to be exchanged behind part 0 of the stage.
int moka_adjoint_rk4_stage_out_fields(moka_tape *t, int sg, void **fieldU, void **fieldH, void **scratchS)
{
    if (!t || !fieldU || !fieldH) return fail(t ? t->st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    if (sg < 1 || sg > 4 || t->kind != 1 || t->n <= 0) return fail(t->st->ctx, MOKA_ERR_ARG, "no recorded RK4 step / stage must be 4..1");
    double *kU[2] = {t->kbU, t->pbU}, *kH[2] = {t->kbH, t->pbH};
    const int kc = (4 - sg) & 1, o = 1 - t->cur;
    *fieldU = sg == 1 ? t->lamU[o] : kU[1 - kc];
    *fieldH = sg == 1 ? t->lamH[o] : kH[1 - kc];
    if (scratchS) *scratchS = t->lamS[o];              // an (nCells) array nothing reads here: stands in for ssh in the exchange maps
    return MOKA_OK;
}

int moka_adjoint_sweep(moka_tape *t)
{
    if (!t) return fail(nullptr, MOKA_ERR_ARG, "tape is NULL");
    moka_state *st = t->st;
    if (!t->seeded) return fail(st->ctx, MOKA_ERR_ARG, "seed the adjoint first (moka_adjoint_seed_sum_sq_ssh)");
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    if (t->kind == 1 && t->revNext != 4) return fail(st->ctx, MOKA_ERR_ARG, "a stage-wise reverse step is in progress");
    while (t->n > 0 && t->kind == 1)
        for (int sg = 4; sg >= 1; --sg)
            if (int rc = rk4_reverse_stage(t, sg)) return rc;
    while (t->n > 0)
        if (int rc = fe_reverse_step(t)) return rc;
    return MOKA_OK;
}

int moka_adjoint_download(moka_tape *t, int field, double *host)
{
    if (!t || !host) return fail(t ? t->st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    moka_state *st = t->st;
    const Plan &p = st->mesh->plan;
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    switch (field) {
        case MOKA_F_SSH: return get_rows(st->mesh, host, t->lamS[t->cur], MOKA_CELL, p.nC, 1);
        case MOKA_F_NORMAL_VELOCITY: return get_rows(st->mesh, host, t->lamU[t->cur], MOKA_EDGE, p.nE, p.K);
        case MOKA_F_LAYER_THICKNESS: return get_rows(st->mesh, host, t->lamH[t->cur], MOKA_CELL, p.nC, p.K);
        case MOKA_F_LAYER_THICKNESS_EDGE: return get_rows(st->mesh, host, t->lamE[t->cur], MOKA_EDGE, p.nE, p.K);
        default: return fail(st->ctx, MOKA_ERR_ARG, "adjoint fields: ssh, normalVelocity, layerThickness, layerThicknessEdge");
    }
}


// ---------------------------------------------------------------------------------------------
// reverse mode through the forced RK4 step (include/moka_hip.h: the recipe; momentum_vmix.hip: the transposed pass).  A handle of its
// own, separate from moka_tape: it embeds one -- built without the check for the pass, counted in moka_state.forcedTapes -- for the
// four transposed RK stages, and puts the transposed vertical pass in front of them.
// ---------------------------------------------------------------------------------------------
struct ForcedStep {
    bool rec, on, stress;        // u_new / h_new were recorded; the pass ran; with the stress
    double nu, drag;
};

struct moka_forced_tape {
    moka_state *st = nullptr;
    moka_tape *inner = nullptr;
    int64_t capacity = 0;
    double *unRec = nullptr, *hnRec = nullptr;       // capacity x (K, nE) / (K, nC): the new level of every step that recorded it
    double *hbar = nullptr, *scratch = nullptr;      // (K, nE); 2 x (K, nE): the column form's g and y.  All four come with the first step that records.
    double *dens[3] = {nullptr, nullptr, nullptr};   // G_tau, D_nu, D_r (nE each), allocated by the flag
    int want = 0;                                    // MOKA_FORCED_GRAD_* bits
    std::vector<ForcedStep> steps;
    int path = 0;                                    // moka_forced_tape_vmix_path
    std::vector<void *> allocs;
};

static int forced_alloc(moka_forced_tape *ft, std::initializer_list<std::pair<double **, size_t>> what)
{
    moka_ctx *ctx = ft->st->ctx;
    std::vector<void *> got;
    for (auto &w : what) {
        void *d = nullptr;
        hipError_t e = hipMalloc(&d, std::max<size_t>(w.second * sizeof(double), 16));
        if (e == hipSuccess) e = hipMemsetAsync(d, 0, w.second * sizeof(double), ctx->stream);
        if (e != hipSuccess) {                       // nothing changes: what this call took goes back
            if (d) got.push_back(d);
            (void)hipStreamSynchronize(ctx->stream);
            for (void *q : got) (void)hipFree(q);
            return fail(ctx, MOKA_ERR_ALLOC, std::string("forced tape: hipMalloc of ") + std::to_string(w.second * sizeof(double)) + " bytes: " + hipGetErrorString(e));
        }
        got.push_back(d);
    }
    size_t i = 0;
    for (auto &w : what) { *w.first = static_cast<double *>(got[i]); ft->allocs.push_back(got[i++]); }
    return MOKA_OK;
}

int moka_forced_tape_create(moka_state *st, int64_t capacity_steps, moka_forced_tape **out)
{
    if (!st || !out || capacity_steps < 0) return fail(st ? st->ctx : nullptr, MOKA_ERR_ARG, "bad argument");
    *out = nullptr;
    const Plan &p = st->mesh->plan;
    if (st->halos > 0) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "forced tape: not on a state with a halo");
    if (p.nPatchesLaunch != p.nPatches) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "forced tape: whole (unpartitioned) meshes only");
    if (st->dycoreTapes > 0) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "forced tape: a moka_tape of this state exists");
    moka_forced_tape *ft = new (std::nothrow) moka_forced_tape();
    if (!ft) return fail(st->ctx, MOKA_ERR_ALLOC, "out of host memory");
    if (int rc = tape_create(st, capacity_steps, &ft->inner, true)) { delete ft; return rc; }     // fp32, nonlinear, tracers, a forced tape
    ft->inner->kind = 1;                             // RK4 only: a seed of the empty tape is an RK4 seed
    ft->st = st;
    ft->capacity = capacity_steps;
    *out = ft;
    return MOKA_OK;
}

void moka_forced_tape_destroy(moka_forced_tape *ft)
{
    if (!ft) return;
    moka_state *st = ft->st;
    st->forcedSteps -= (int64_t)ft->steps.size();
    moka_tape_destroy(ft->inner);                    // synchronises the stream
    for (void *q : ft->allocs) (void)hipFree(q);
    delete ft;
}

int moka_step_rk4_forced_taped(moka_forced_tape *ft, double dt)
{
    if (!ft) return fail(nullptr, MOKA_ERR_ARG, "forced tape is NULL");
    moka_state *st = ft->st;
    const Plan &p = st->mesh->plan;
    if ((int64_t)ft->steps.size() >= ft->capacity) return fail(st->ctx, MOKA_ERR_ARG, "forced tape is full");
    const bool on = mom_vmix_on(st);
    if (on && dt < 0.0) return fail(st->ctx, MOKA_ERR_ARG, "vertical momentum mixing: dt must be >= 0 (the implicit solve is not reversible in time)");
    const bool rec = on || ft->want != 0;
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    const size_t nEK = (size_t)p.K * p.nE, nCK = (size_t)p.K * p.nC;
    if (rec && !ft->unRec)
        if (int rc = forced_alloc(ft, {{&ft->unRec, nEK * (size_t)ft->capacity}, {&ft->hnRec, nCK * (size_t)ft->capacity}, {&ft->hbar, nEK}, {&ft->scratch, 2 * nEK}}))
            return rc;
    if (int rc = moka_step_rk4_taped(ft->inner, dt)) return rc;
    hipStream_t s = st->ctx->stream;
    if (on && dt != 0.0)         // the split step of moka_step_rk4, on the same two arrays (rk4_end has made them the current level)
        if (int rc = momentum_vmix(st, st->lev[1].u, st->lev[1].h, dt)) return rc;
    const size_t i = ft->steps.size();
    if (rec) {
        HIPCHK(st->ctx, hipMemcpyAsync(ft->unRec + nEK * i, st->lev[1].u, nEK * sizeof(double), hipMemcpyDeviceToDevice, s));
        HIPCHK(st->ctx, hipMemcpyAsync(ft->hnRec + nCK * i, st->lev[1].h, nCK * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    ft->steps.push_back({rec, on, st->momTau && st->momTauOn, st->momNuV, st->momDrag});
    ++st->forcedSteps;
    return MOKA_OK;
}

static int forced_zero_densities(moka_forced_tape *ft)
{
    for (double *d : ft->dens)
        if (d) HIPCHK(ft->st->ctx, hipMemsetAsync(d, 0, (size_t)ft->st->mesh->plan.nE * sizeof(double), ft->st->ctx->stream));
    return MOKA_OK;
}

int moka_forced_adjoint_seed_sum_sq_ssh(moka_forced_tape *ft)
{
    if (!ft) return fail(nullptr, MOKA_ERR_ARG, "forced tape is NULL");
    if (int rc = moka_adjoint_seed_sum_sq_ssh(ft->inner)) return rc;
    return forced_zero_densities(ft);
}

int moka_forced_adjoint_seed(moka_forced_tape *ft, const double *hostU, const double *hostH)
{
    if (!ft || !hostU || !hostH) return fail(ft ? ft->st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    moka_state *st = ft->st;
    moka_tape *t = ft->inner;
    const Plan &p = st->mesh->plan;
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    hipStream_t s = st->ctx->stream;
    const size_t nEK = (size_t)p.K * p.nE;
    t->cur = 0;
    for (int b = 0; b < 2; ++b) {       // as the RK4 seed of moka_tape: the sweep never writes the ssh / layerThicknessEdge adjoints
        HIPCHK(st->ctx, hipMemsetAsync(t->lamS[b], 0, (size_t)p.nC * sizeof(double), s));
        HIPCHK(st->ctx, hipMemsetAsync(t->lamE[b], 0, nEK * sizeof(double), s));
    }
    if (int rc = put_rows(st->mesh, t->lamU[0], hostU, MOKA_EDGE, p.nE, p.K)) return rc;
    if (int rc = put_rows(st->mesh, t->lamH[0], hostH, MOKA_CELL, p.nC, p.K)) return rc;
    t->seeded = true;
    return forced_zero_densities(ft);
}

int moka_forced_adjoint_sweep(moka_forced_tape *ft)
{
    if (!ft) return fail(nullptr, MOKA_ERR_ARG, "forced tape is NULL");
    moka_state *st = ft->st;
    moka_tape *t = ft->inner;
    if (!t->seeded) return fail(st->ctx, MOKA_ERR_ARG, "seed the adjoint first (moka_forced_adjoint_seed_sum_sq_ssh, moka_forced_adjoint_seed)");
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    const Plan &p = st->mesh->plan;
    const size_t nEK = (size_t)p.K * p.nE, nCK = (size_t)p.K * p.nC;
    const bool generic = st->ctx->variant == 3;
    while (!ft->steps.empty()) {
        const ForcedStep r = ft->steps.back();
        const size_t i = ft->steps.size() - 1;
        const double dt = t->dts[i];
        if (r.rec && dt != 0.0) {       // the transposed pass, at the head of the reversed step
            MomVmixAdjArgs a{};
            a.nE = p.nE; a.K = p.K; a.nC = p.nC; a.ME = p.ME;
            a.ehdr = st->mesh->dev.ehdr; a.eoc = st->mesh->dev.eoc;
            a.xu = t->lamU[t->cur]; a.xh = t->lamH[t->cur];
            a.un = ft->unRec + nEK * i; a.hn = ft->hnRec + nCK * i;
            a.tau = r.stress ? st->momTau : nullptr;
            a.dt = dt; a.nu = r.nu; a.drag = r.drag; a.on = r.on ? 1 : 0;
            a.hbar = ft->hbar; a.scratch = ft->scratch;
            a.Gtau = (ft->want & MOKA_FORCED_GRAD_STRESS) ? ft->dens[0] : nullptr;
            a.Dnu = (ft->want & MOKA_FORCED_GRAD_VISCOSITY) ? ft->dens[1] : nullptr;
            a.Dr = (ft->want & MOKA_FORCED_GRAD_DRAG) ? ft->dens[2] : nullptr;
            const bool launched = ft->want != 0 || (r.on && !(p.K < 2 && r.drag == 0.0 && !a.tau));
            HIPCHK(st->ctx, launch_momentum_vmix_adjoint(a, generic, st->ctx->stream));
            HIPCHK(st->ctx, launch_momentum_vmix_gather(a, st->ctx->stream));
            if (launched) ft->path = momentum_vmix_adjoint_form(p.K, generic);
        }
        for (int sg = 4; sg >= 1; --sg)
            if (int rc = rk4_reverse_stage(t, sg)) return rc;
        ft->steps.pop_back();
        --st->forcedSteps;
    }
    return MOKA_OK;
}

int moka_forced_adjoint_download(moka_forced_tape *ft, int field, double *host)
{
    if (!ft || !host) return fail(ft ? ft->st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    if (field != MOKA_F_NORMAL_VELOCITY && field != MOKA_F_LAYER_THICKNESS)
        return fail(ft->st->ctx, MOKA_ERR_ARG, "forced adjoint fields: normalVelocity, layerThickness");
    return moka_adjoint_download(ft->inner, field, host);
}

static int forced_bit(int what) { return what == MOKA_FORCED_GRAD_STRESS ? 0 : what == MOKA_FORCED_GRAD_VISCOSITY ? 1 : what == MOKA_FORCED_GRAD_DRAG ? 2 : -1; }

int moka_forced_adjoint_want_gradient(moka_forced_tape *ft, int what, int on)
{
    if (!ft) return fail(nullptr, MOKA_ERR_ARG, "forced tape is NULL");
    moka_state *st = ft->st;
    const int all = MOKA_FORCED_GRAD_STRESS | MOKA_FORCED_GRAD_VISCOSITY | MOKA_FORCED_GRAD_DRAG;
    if (what == 0 || (what & ~all)) return fail(st->ctx, MOKA_ERR_ARG, "forced tape: what must be a nonempty set of MOKA_FORCED_GRAD_* bits");
    if (!ft->steps.empty()) return fail(st->ctx, MOKA_ERR_ARG, "forced tape: gradients are flagged while no step is recorded");
    if (on) {
        HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
        double *fresh[3] = {nullptr, nullptr, nullptr};
        for (int b = 0; b < 3; ++b)
            if ((what >> b & 1) && !ft->dens[b]) {
                if (int rc = forced_alloc(ft, {{&fresh[b], (size_t)st->mesh->plan.nE}})) {
                    for (int c = 0; c < b; ++c)     // nothing changes: the densities this call took go back
                        if (fresh[c]) { ft->allocs.erase(std::find(ft->allocs.begin(), ft->allocs.end(), (void *)fresh[c])); (void)hipFree(fresh[c]); }
                    return rc;
                }
            }
        for (int b = 0; b < 3; ++b)
            if (fresh[b]) ft->dens[b] = fresh[b];
        HIPCHK(st->ctx, hipStreamSynchronize(st->ctx->stream));
        ft->want |= what;
    } else {
        ft->want &= ~what;
    }
    return MOKA_OK;
}

int moka_forced_adjoint_density_download(moka_forced_tape *ft, int what, double *host)
{
    if (!ft || !host) return fail(ft ? ft->st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    const int b = forced_bit(what);
    if (b < 0 || !(ft->want & what)) return fail(ft->st->ctx, MOKA_ERR_ARG, "forced tape: what must be one flagged MOKA_FORCED_GRAD_* bit");
    HIPCHK(ft->st->ctx, hipSetDevice(ft->st->ctx->device));
    return get_rows(ft->st->mesh, host, ft->dens[b], MOKA_EDGE, ft->st->mesh->plan.nE, 1);
}

int moka_forced_adjoint_gradient(moka_forced_tape *ft, int what, double *out)
{
    if (!ft || !out) return fail(ft ? ft->st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    std::vector<double> w((size_t)ft->st->mesh->plan.nE);
    if (int rc = moka_forced_adjoint_density_download(ft, what, w.data())) return rc;
    long double sum = 0.0L;            // the caller's edge numbering, ascending, one rounding at the end: independent of the plan's order
    for (double v : w) sum += (long double)v;
    *out = (double)sum;
    return MOKA_OK;
}

int moka_forced_tape_vmix_path(const moka_forced_tape *ft) { return ft ? ft->path : 0; }

}  // extern "C"
