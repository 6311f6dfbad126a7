// api_tape.hip -- C ABI, continued: the moka_tape entry points.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "state.hpp"
#include "tapes.hpp"

// ---------------------------------------------------------------------------------------------
// reverse mode of the Forward-Euler loop.  The reference differentiates
// ocn_run_loop with Enzyme (ext/MPASEnzymeExt.jl; test/enzyme/test_Enzyme_end2end.jl: d sum(ssh^2) / d initial
// layerThickness, normalVelocity); here the tape and the transposed kernels are written by hand.
// ---------------------------------------------------------------------------------------------
namespace mk {

// forced: the tape inside a moka_forced_tape, which transposes the vertical momentum pass itself
int tape_create(moka_state *st, int64_t capacity_steps, moka_tape **out, bool forced)
{
    if (!st || !out || capacity_steps < 0) return fail(st ? st->ctx : nullptr, MOKA_ERR_ARG, "bad argument");
    *out = nullptr;
    if (st->rich) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "Richardson closure: no reverse mode through or beside it (moka_set_richardson_mixing(st, NULL) first)");
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
    t->mem.ctx = st->ctx; t->mem.owner = "tape";
    t->capacity = capacity_steps;
    const size_t nEK = (size_t)p.K * nE, nCK = (size_t)p.K * nC;
    int rc = MOKA_OK;
    auto A = [&](double **q, size_t n) { if (rc == MOKA_OK) rc = t->mem.alloc(q, n); };
    A(&t->uTape, nEK * (size_t)capacity_steps); A(&t->hTape, nEK * (size_t)capacity_steps);
    for (int b = 0; b < 2; ++b) { A(&t->lamU[b], nEK); A(&t->lamH[b], nCK); A(&t->lamS[b], nC); A(&t->lamE[b], nEK); }
    A(&t->Enew, nEK); A(&t->csum, nE);
    moka::AdjMesh &am = t->am;
    am.nC = nC; am.nE = nE; am.K = p.K; am.ME = ME; am.W = W;
    am.eBegin = 0; am.eCount = nE; am.cBegin = 0; am.cCount = nC;
    am.eoc = st->mesh->dev.eoc; am.ehdr = st->mesh->dev.ehdr; am.fEdge = st->mesh->dev.fEdge; am.gInvDc = st->mesh->dev.gInvDc;
    if (rc == MOKA_OK) rc = t->mem.upload(teoe, &am.teoe);
    if (rc == MOKA_OK) rc = t->mem.upload(tw, &am.tw);
    if (rc == MOKA_OK) rc = t->mem.upload(sd, &am.sd);
    if (rc == MOKA_OK) rc = t->mem.upload(csgn, &am.csgn);
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
        if (rc == MOKA_OK) rc = t->mem.upload(efull, &am.efull);
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

// false: the state had gone before the tape (the forced tape around this one then leaves its counters alone too)
bool tape_destroy(moka_tape *t)
{
    moka_ctx *ctx = t->mem.ctx;
    const bool alive = !t->counted || state_detach(t->st);      // (not counted: inside a failed tape_create)
    if (alive && t->counted) --(t->forced ? t->st->forcedTapes : t->st->dycoreTapes);
    (void)hipSetDevice(ctx->device);
    if (alive && t->st->lazyOwner == t) {   // the stage-4 tendencies of the last taped step would be produced from a slot of this tape
        if (t->st->tendDirty) (void)flush_lazy(t->st, false, true);
        t->st->lazyPu = t->st->lazyPh = nullptr; t->st->lazyOwner = nullptr;
    }
    (void)hipStreamSynchronize(ctx->stream);
    t->mem.release_all();
    delete t;
    return alive;
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
int rk4_reverse_stage(moka_tape *t, int sg, int part)
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

}  // namespace mk

using namespace mk;

extern "C" {

int moka_tape_create(moka_state *st, int64_t capacity_steps, moka_tape **out) { return tape_create(st, capacity_steps, out, false); }

void moka_tape_destroy(moka_tape *t)
{
    if (t) (void)tape_destroy(t);
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
        auto A = [&](double **q, size_t n) { if (rc == MOKA_OK) rc = t->mem.alloc(q, n); };
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
        auto A = [&](double **q, size_t n) { if (rc == MOKA_OK) rc = t->mem.alloc(q, n); };
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

}  // extern "C"
