// api_tracers.hip -- C ABI, continued: passive tracers of a state -- their sources, diffusivities and diffusivity fields, and the launches of an RK4 stage.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "state.hpp"

namespace mk {

// The tracer launch of RK4 stage s, behind the dycore's launch g on the compute stream (it reads the thickness that launch wrote:
// the next provisional one, the new level's at stage 4; the stage's own provisional state is never written by its launch).  Buffers
// follow rk4_stage_args: provisional tracers current level -> trProv[0] -> trProv[1] -> trProv[0]; the running content sum Qn lives in
// the previous level's array, as New does, and stage 4 leaves the new tracers there (rk4_end swaps the levels).  Qc = phi * h of the
// current level is formed on the fly by every stage that needs it (the same product, the same bits as a stored one).
hipError_t tracer_stage(moka_state *st, int s, const StageArgs &g)
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
int tracer_vmix(moka_mesh *mm, moka_ctx *ctx, int nT, const double *h, double *x, const double *kv, const double *const *fld, double dt,
                double *scratch, bool reverse, int *path, const int32_t *gslot, const double *p_new, double *D)
{
    const Plan &p = mm->plan;
    if (!mm->nLev)
        if (int rc = mm->mem.upload(p.nLev, &mm->nLev)) return rc;
    VmixArgs a{};
    a.nT = nT; a.nC = p.nC; a.K = p.K; a.stride = (int64_t)p.K * p.nC;
    a.h = h; a.x = x; a.kv = kv; a.fld = fld; a.dt = dt; a.nLev = mm->nLev; a.scratch = scratch;
    a.gslot = gslot; a.p = p_new; a.D = D;
    const bool generic = ctx->variant == 3;
    *path = vmix_kernel(p.K, generic, gslot ? 4 : 3).form;
    HIPCHK(ctx, launch_tracer_vmix(a, reverse, generic, ctx->stream));
    return MOKA_OK;
}

// ---- what the vertical pass is to take for a tracer: its scalar, or its diffusivity field (include/moka_hip.h) ----
bool vfield_on(const moka_state *st, int j) { return !st->trVf.empty() && st->trVf[j] && st->trVfOn[j]; }

// the coefficient the pass and a tape take for tracer j while the scalars are kv (empty = all zero): a field whose active entries are
// all zero makes it 0.0; beside a field that is on it is not read
double vmix_coefficient(const moka_state *st, const std::vector<double> &kv, int j)
{
    if (!st->trVf.empty() && st->trVf[j] && !st->trVfOn[j]) return 0.0;
    return kv.empty() ? 0.0 : kv[j];
}

}  // namespace mk

using namespace mk;

extern "C" {

// ---- tracer sources: d(h phi_j)/dt gains q_j[k,c], constant in time until changed (include/moka_hip.h) ----
// the caller has synchronised the stream: no launch reads the table or a source
static void drop_sources(moka_state *st)
{
    for (double *&q : st->trSrc) st->mem.release(q);
    st->trSrc.clear();
    st->mem.release(st->trSrcDev);
}

// likewise for the diffusivity fields of the vertical pass (moka_tracer_vertical_field_upload, further down)
static void drop_vfields(moka_state *st)
{
    for (double *&q : st->trVf) st->mem.release(q);
    st->trVf.clear();
    st->trVfOn.clear();
    st->trVfGen.clear();                 // (trVfClock goes on counting)
    st->mem.release(st->trVfDev);
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
        st->mem.release(st->trSrc[j]);
        if (std::all_of(st->trSrc.begin(), st->trSrc.end(), [](double *q) { return !q; })) {
            drop_sources(st);
            return MOKA_OK;
        }
    } else {
        if (!had) {
            double *d = nullptr;
            if (int rc = st->mem.alloc(&d, nCK)) return rc;
            if (!st->trSrcDev)
                if (int rc = st->mem.alloc(&st->trSrcDev, (size_t)st->nTracers)) {
                    (void)hipStreamSynchronize(st->ctx->stream);
                    st->mem.release(d);
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
        rich_drop(st);                   // the Richardson closure reads a tracer: off, and G (and F) freed
        drop_sources(st);                // every source goes with the tracers
        drop_vfields(st);                // ... and every diffusivity field
        for (double **q : arr) st->mem.release(*q);
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
        else if (int rc = st->mem.alloc(q, (size_t)nTracers * p.K * p.nC)) {
            (void)hipStreamSynchronize(st->ctx->stream);
            release();
            return rc;
        }
    HIPCHK(st->ctx, hipStreamSynchronize(st->ctx->stream));
    st->nTracers = nTracers;
    return MOKA_OK;
}

int moka_tracer_count(const moka_state *st, int32_t *out)
{
    if (!st || !out) return fail(st ? st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    *out = st->nTracers;
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
        st->mem.release(st->trKappaDev);
        st->trKappa.clear();
        return MOKA_OK;
    }
    if (!mm->dvdc)
        if (int rc = mm->mem.upload(mm->plan.dvdc, &mm->dvdc)) return rc;
    if (!st->trKappaDev)
        if (int rc = st->mem.alloc(&st->trKappaDev, (size_t)nT)) return rc;
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
    if (!any) {
        st->mem.release(st->trKappa4Dev);
        st->mem.release(st->trLap);
        st->trKappa4.clear();
        return MOKA_OK;
    }
    const Plan &p = mm->plan;
    if (!mm->dvdc)
        if (int rc = mm->mem.upload(mm->plan.dvdc, &mm->dvdc)) return rc;
    if (!st->trLap)
        if (int rc = st->mem.alloc(&st->trLap, (size_t)nT * p.K * p.nC)) return rc;
    if (!st->trKappa4Dev)           // (alloc zero-fills: the second half stays the array of zeros)
        if (int rc = st->mem.alloc(&st->trKappa4Dev, 2 * (size_t)nT)) {
            (void)hipStreamSynchronize(st->ctx->stream);
            st->mem.release(st->trLap);
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
    if (std::all_of(kv.begin(), kv.end(), [](double k) { return k == 0.0; })) kv.clear();
    if (!anyField) st->mem.release(st->trVfDev);
    if (!any) {
        st->mem.release(st->trKappaVDev);
        if (!st->rich) st->mem.release(st->trVmixScratch);      // (the Richardson closure runs the pass too and keeps the scratch)
        if (int rc = rich_commit(st, kv)) return rc;
        st->trKappaV = std::move(kv);
        return MOKA_OK;
    }
    const Plan &p = mm->plan;
    if (!mm->nLev)
        if (int rc = mm->mem.upload(p.nLev, &mm->nLev)) return rc;
    if (!st->trVmixScratch)
        if (int rc = st->mem.alloc(&st->trVmixScratch, 2 * (size_t)p.K * p.nC)) return rc;
    if (!st->trKappaVDev)
        if (int rc = st->mem.alloc(&st->trKappaVDev, (size_t)nT)) {
            (void)hipStreamSynchronize(st->ctx->stream);
            st->mem.release(st->trVmixScratch);
            return rc;
        }
    if (anyField && !st->trVfDev)
        if (int rc = st->mem.alloc(&st->trVfDev, (size_t)nT)) return rc;
    if (int rc = h2d(st->ctx, st->trKappaVDev, eff.data(), (size_t)nT * sizeof(double))) return rc;
    if (anyField)
        if (int rc = h2d(st->ctx, st->trVfDev, tab.data(), (size_t)nT * sizeof(double *))) return rc;
    if (int rc = rich_commit(st, kv)) return rc;      // what the pass takes while the Richardson closure is on follows the set-aside values
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
        if (int rc = st->mem.alloc(&fresh, nCK)) return rc;
        if (int rc = put_rows(st->mesh, fresh, host, MOKA_CELL, p.nC, p.K)) {
            (void)hipStreamSynchronize(st->ctx->stream);
            st->mem.release(fresh);
            return rc;
        }
    }
    const std::vector<double *> vf0 = st->trVf;
    const std::vector<char> on0 = st->trVfOn;
    const std::vector<uint64_t> gen0 = st->trVfGen;
    st->trVf.resize((size_t)st->nTracers, nullptr);
    st->trVfOn.resize((size_t)st->nTracers, 0);
    st->trVfGen.resize((size_t)st->nTracers, 0);
    double *old = st->trVf[j];
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
        st->mem.release(fresh);
        (void)vmix_commit(st, st->trKappaV);     // the table and the coefficients of the fields as they were
        return rc;
    }
    ++st->trVfClock;
    st->mem.release(old);
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

}  // extern "C"
