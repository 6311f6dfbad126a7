// api_closure.hip -- C ABI, continued: the Richardson-number closure that computes the coefficients of the two vertical passes on the
// device (include/moka_hip.h: the recipe; vmix_closure.hip: the kernels; step_rk4 in api_state.hip: where it is launched).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "state.hpp"

namespace mk {

RichArgs rich_args(const moka_state *st, const double *u, const double *h, const double *b)
{
    const Plan &p = st->mesh->plan;
    const MeshDev &d = st->mesh->dev;
    const moka_richardson_params &q = st->richP;
    RichArgs a{};
    a.nE = p.nE; a.nC = p.nC; a.K = p.K; a.ME = p.ME;
    a.ehdr = d.ehdr; a.eoc = d.eoc; a.mltc = d.mltc; a.nLev = st->mesh->nLev; a.keCoef = d.keCoef; a.invArea = d.invArea;
    a.u = u; a.h = h; a.b = b;
    a.nu0 = q.nu0; a.alpha = q.alpha; a.nuB = q.nuBackground; a.kB = q.kappaBackground; a.conv = q.convective;
    a.F = st->richF; a.G = st->richG;
    return a;
}

// What the tracer pass takes while the closure is on: G for a tracer of the set, else the tracer's own field that is on, else its
// scalar (0.0 under a field whose active entries are all zero).  The caller has synchronised the stream.
int rich_commit(moka_state *st, const std::vector<double> &kv)
{
    if (!st->rich) return MOKA_OK;
    const int nT = st->nTracers;
    std::vector<double> eff((size_t)nT, 0.0);
    std::vector<double *> tab((size_t)nT, nullptr);
    for (int j = 0; j < nT; ++j) {
        if (st->richMask[j]) { tab[j] = st->richG; continue; }
        eff[j] = vmix_coefficient(st, kv, j);
        if (vfield_on(st, j)) tab[j] = st->trVf[j];
    }
    if (int rc = h2d(st->ctx, st->richKvDev, eff.data(), (size_t)nT * sizeof(double))) return rc;
    return h2d(st->ctx, st->richVfDev, tab.data(), (size_t)nT * sizeof(double *));
}

// off, and everything the closure owns freed; the scratch of the tracer pass goes too when nothing else keeps that pass on.  The caller
// has synchronised the stream.
void rich_drop(moka_state *st)
{
    st->rich = false;
    st->richRan = false;
    st->richMask.clear();
    st->richP = moka_richardson_params{};
    st->mem.release(st->richF);
    st->mem.release(st->richG);
    st->mem.release(st->richKvDev);
    st->mem.release(st->richVfDev);
    if (!st->trKappaVDev) st->mem.release(st->trVmixScratch);
}

}  // namespace mk

using namespace mk;

// what a state must be for the closure to be switched on: what the two passes ask for, and no tape of any kind
static int rich_supported(moka_state *st)
{
    const Plan &p = st->mesh->plan;
    if (st->f32) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "Richardson closure: Float64 states only");
    if (st->halos > 0) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "Richardson closure: not on a state with a halo");
    if (p.nPatchesLaunch != p.nPatches) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "Richardson closure: whole (unpartitioned) meshes only");
    if (st->dycoreTapes > 0 || st->forcedTapes > 0 || st->attached > 0)
        return fail(st->ctx, MOKA_ERR_UNSUPPORTED,
                    "Richardson closure: not while a moka_tape, a moka_forced_tape or a moka_tracer_tape of this state exists (the closure makes the "
                    "coefficients depend on the flow and on the buoyancy tracer: reverse mode does not cover it)");
    return MOKA_OK;
}

extern "C" {

int moka_set_richardson_mixing(moka_state *st, const moka_richardson_params *p)
{
    if (!st) return fail(nullptr, MOKA_ERR_ARG, "state is NULL");
    if (!p) {
        if (!st->rich) return MOKA_OK;
        HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
        HIPCHK(st->ctx, hipStreamSynchronize(st->ctx->stream));      // no launch is reading F, G or the tables
        rich_drop(st);
        return MOKA_OK;
    }
    for (double v : {p->nu0, p->alpha, p->nuBackground, p->kappaBackground, p->convective})
        if (!(v >= 0.0) || !std::isfinite(v)) return fail(st->ctx, MOKA_ERR_ARG, "Richardson closure: every parameter must be finite and >= 0");
    if (int rc = rich_supported(st)) return rc;      // (ahead of the tracer count: such a state cannot have tracers either, and this is the reason that lasts)
    const int nT = st->nTracers;
    if (nT == 0) return fail(st->ctx, MOKA_ERR_ARG, "Richardson closure: the state has no tracers (moka_set_tracers): one of them is the buoyancy");
    if (p->buoyancyTracer < 0 || p->buoyancyTracer >= nT) return fail(st->ctx, MOKA_ERR_ARG, "Richardson closure: buoyancyTracer out of range (moka_set_tracers)");
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    HIPCHK(st->ctx, hipStreamSynchronize(st->ctx->stream));          // no launch is reading the old tables
    moka_mesh *mm = st->mesh;
    const Plan &pl = mm->plan;
    const bool was = st->rich;
    if (!was) {          // everything a step with the closure needs, now: F, G, kc, nLev, both column forms' scratch, the tables
        if (int rc = ensure_ke_coef(mm)) return rc;
        if (!mm->nLev)
            if (int rc = mm->mem.upload(pl.nLev, &mm->nLev)) return rc;
        const size_t nEK = (size_t)pl.K * pl.nE, nCK = (size_t)pl.K * pl.nC, m = st->mem.mark();
        double *F = nullptr, *G = nullptr, *kvd = nullptr, *ms = st->momScratch, *ts = st->trVmixScratch;
        double **tab = nullptr;
        int rc = st->mem.alloc(&F, nEK);
        if (!rc) rc = st->mem.alloc(&G, nCK);
        if (!rc) rc = st->mem.alloc(&kvd, (size_t)nT);
        if (!rc) rc = st->mem.alloc(&tab, (size_t)nT);
        if (!rc && !ms) rc = st->mem.alloc(&ms, 2 * nEK);
        if (!rc && !ts) rc = st->mem.alloc(&ts, 2 * nCK);
        if (rc) { st->mem.rollback(m); return rc; }
        if (hipError_t e = hipStreamSynchronize(st->ctx->stream); e != hipSuccess) {      // (the zero fills)
            st->mem.rollback(m);
            return fail(st->ctx, MOKA_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
        }
        st->richF = F; st->richG = G; st->richKvDev = kvd; st->richVfDev = tab; st->momScratch = ms; st->trVmixScratch = ts;
    }
    const moka_richardson_params p0 = st->richP;
    const std::vector<int32_t> mask0 = st->richMask;
    st->richP = *p;
    st->richP.tracerMask = nullptr;
    st->richMask.assign((size_t)nT, 1);
    for (int j = 0; p->tracerMask && j < nT; ++j) st->richMask[j] = p->tracerMask[j] != 0;
    st->rich = true;
    if (int rc = rich_commit(st, st->trKappaV)) {
        (void)hipStreamSynchronize(st->ctx->stream);
        if (was) { st->richP = p0; st->richMask = mask0; (void)rich_commit(st, st->trKappaV); }
        else rich_drop(st);
        return rc;
    }
    return MOKA_OK;
}

int moka_richardson_mixing(const moka_state *st, int *on, moka_richardson_params *out, int32_t *maskOut)
{
    if (!st || !on || !out) return fail(st ? st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    *on = st->rich ? 1 : 0;
    *out = st->richP;            // (all zero while the closure is off; tracerMask is never handed back: maskOut takes the flags)
    for (int j = 0; maskOut && j < st->nTracers; ++j) maskOut[j] = st->rich ? st->richMask[j] : 0;
    return MOKA_OK;
}

int moka_richardson_fields_download(moka_state *st, double *viscEdge, double *diffCell)
{
    if (!st) return fail(nullptr, MOKA_ERR_ARG, "state is NULL");
    const Plan &p = st->mesh->plan;
    if (!st->rich || !st->richRan) {
        if (viscEdge) std::fill(viscEdge, viscEdge + (size_t)p.K * p.nE, 0.0);
        if (diffCell) std::fill(diffCell, diffCell + (size_t)p.K * p.nC, 0.0);
        return MOKA_OK;
    }
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    if (viscEdge)
        if (int rc = get_rows(st->mesh, viscEdge, st->richF, MOKA_EDGE, p.nE, p.K)) return rc;
    if (diffCell)
        if (int rc = get_rows(st->mesh, diffCell, st->richG, MOKA_CELL, p.nC, p.K)) return rc;
    return MOKA_OK;
}

int moka_richardson_diagnose(moka_state *st, int time_level, double *riEdge, double *riCell, double *viscEdge, double *diffCell)
{
    if (!st) return fail(nullptr, MOKA_ERR_ARG, "state is NULL");
    if (time_level != 0 && time_level != 1) return fail(st->ctx, MOKA_ERR_ARG, "time_level must be 0 (previous) or 1 (current)");
    if (!st->rich) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "Richardson closure: off (moka_set_richardson_mixing names the buoyancy tracer and the parameters)");
    const Plan &p = st->mesh->plan;
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    const size_t nEK = (size_t)p.K * p.nE, nCK = (size_t)p.K * p.nC, m = st->mem.mark();
    double *host[4] = {riEdge, riCell, viscEdge, diffCell}, *dev[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < 4; ++i)          // zero-filled work arrays: rows no interface reaches come back 0.0, as in F and G
        if (host[i])
            if (int rc = st->mem.alloc(&dev[i], i % 2 ? nCK : nEK)) { st->mem.rollback(m); return rc; }
    RichArgs a = rich_args(st, st->lev[time_level].u, st->lev[time_level].h, st->trPhi[time_level] + nCK * (size_t)st->richP.buoyancyTracer);
    a.riE = dev[0]; a.riC = dev[1]; a.F = dev[2]; a.G = dev[3];
    int rc = MOKA_OK;
    if (hipError_t e = launch_richardson(a, st->ctx->stream); e != hipSuccess)
        rc = fail(st->ctx, MOKA_ERR_HIP, std::string("launch_richardson: ") + hipGetErrorString(e));
    for (int i = 0; i < 4 && rc == MOKA_OK; ++i)
        if (host[i]) rc = get_rows(st->mesh, host[i], dev[i], i % 2 ? MOKA_CELL : MOKA_EDGE, i % 2 ? p.nC : p.nE, p.K);
    st->mem.rollback(m);             // (synchronises, then frees the work arrays)
    return rc;
}

}  // extern "C"
