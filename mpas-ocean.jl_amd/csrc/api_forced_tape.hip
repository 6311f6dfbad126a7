// api_forced_tape.hip -- C ABI, continued: the moka_forced_tape entry points.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <new>
#include <string>
#include <vector>

#include "state.hpp"
#include "tapes.hpp"

// ---------------------------------------------------------------------------------------------
// reverse mode through the forced RK4 step (include/moka_hip.h: the recipe; momentum_vmix.hip: the transposed pass).  A handle of its
// own, separate from moka_tape: it embeds one -- built without the check for the pass, counted in moka_state.forcedTapes -- for the
// four transposed RK stages, and puts the transposed vertical pass in front of them.
// ---------------------------------------------------------------------------------------------
using namespace mk;

// quadratic: the tape of moka_forced_tape_create_quadratic, which carries the quadratic drag; a plain one refuses a state with Cd != 0
// and is counted in forcedPlainTapes, where moka_set_quadratic_bottom_drag looks
static int forced_tape_create(moka_state *st, int64_t capacity_steps, moka_forced_tape **out, bool quadratic)
{
    if (!st || !out || capacity_steps < 0) return fail(st ? st->ctx : nullptr, MOKA_ERR_ARG, "bad argument");
    *out = nullptr;
    const Plan &p = st->mesh->plan;
    if (st->rich) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "Richardson closure: no reverse mode through or beside it (moka_set_richardson_mixing(st, NULL) first)");
    if (st->halos > 0) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "forced tape: not on a state with a halo");
    if (p.nPatchesLaunch != p.nPatches) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "forced tape: whole (unpartitioned) meshes only");
    if (st->dycoreTapes > 0) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "forced tape: a moka_tape of this state exists");
    if (!quadratic && st->momCd != 0.0)
        return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "forced tape: no reverse mode through the quadratic bottom drag (moka_set_quadratic_bottom_drag(st, 0) first)");
    moka_forced_tape *ft = new (std::nothrow) moka_forced_tape();
    if (!ft) return fail(st->ctx, MOKA_ERR_ALLOC, "out of host memory");
    if (int rc = tape_create(st, capacity_steps, &ft->inner, true)) { delete ft; return rc; }     // fp32, nonlinear, tracers, a forced tape
    ft->inner->kind = 1;                             // RK4 only: a seed of the empty tape is an RK4 seed
    ft->st = st;
    ft->mem.ctx = st->ctx; ft->mem.owner = "forced tape";
    ft->capacity = capacity_steps;
    ft->quadratic = quadratic;
    if (!quadratic) { ++st->forcedPlainTapes; ft->countedPlain = true; }
    *out = ft;
    return MOKA_OK;
}

extern "C" {

int moka_forced_tape_create(moka_state *st, int64_t capacity_steps, moka_forced_tape **out)
{
    return forced_tape_create(st, capacity_steps, out, false);
}

int moka_forced_tape_create_quadratic(moka_state *st, int64_t capacity_steps, moka_forced_tape **out)
{
    return forced_tape_create(st, capacity_steps, out, true);
}

void moka_forced_tape_destroy(moka_forced_tape *ft)
{
    if (!ft) return;
    if (tape_destroy(ft->inner)) {                   // synchronises the stream
        ft->st->forcedSteps -= (int64_t)ft->steps.size();
        if (ft->countedPlain) --ft->st->forcedPlainTapes;
    }
    ft->mem.release_all();
    delete ft;
}

int moka_step_rk4_forced_taped(moka_forced_tape *ft, double dt)
{
    if (!ft) return fail(nullptr, MOKA_ERR_ARG, "forced tape is NULL");
    moka_state *st = ft->st;
    const Plan &p = st->mesh->plan;
    if ((int64_t)ft->steps.size() >= ft->capacity) return fail(st->ctx, MOKA_ERR_ARG, "forced tape is full");
    if (!ft->quadratic && st->momCd != 0.0)      // (the setter refuses a nonzero value beside a plain forced tape: kept for a state that gains another path to it)
        return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "forced tape: no reverse mode through the quadratic bottom drag");
    const bool on = mom_vmix_on(st);
    if (on && dt < 0.0) return fail(st->ctx, MOKA_ERR_ARG, "vertical momentum mixing: dt must be >= 0 (the implicit solve is not reversible in time)");
    const bool rec = on || ft->want != 0 || ft->wantF || ft->wantCd;
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    const size_t nEK = (size_t)p.K * p.nE, nCK = (size_t)p.K * p.nC;
    if (rec && !ft->unRec)
        if (int rc = ft->mem.alloc_all({{&ft->unRec, nEK * (size_t)ft->capacity}, {&ft->hnRec, nCK * (size_t)ft->capacity}, {&ft->hbar, nEK}, {&ft->scratch, 2 * nEK}}))
            return rc;
    // the quadratic drag: sp of a step whose pass runs with Cd != 0 or whose density of Cd is wanted, u* of a step with Cd != 0 --
    // allocated ahead of the step's first launch, by the first step that needs each (a plain tape has qd == wsp == false)
    const bool qd = ft->quadratic && st->momCd != 0.0 && dt != 0.0, wsp = qd || (ft->wantCd && dt != 0.0);
    if (wsp && !ft->spRec)
        if (int rc = ft->mem.alloc(&ft->spRec, (size_t)p.nE * (size_t)ft->capacity)) return rc;
    if (qd && !ft->usRec)
        if (int rc = ft->mem.alloc_all({{&ft->usRec, nEK * (size_t)ft->capacity}, {&ft->M, (size_t)p.nE}})) return rc;
    // the viscosity field the step is about to run with: a copy of its own when the tape's newest one is of another generation,
    // allocated and taken ahead of the step's first launch (a step that fails afterwards leaves a copy the next step uses)
    const double *fld = on ? mom_vmix_field(st) : nullptr;
    hipStream_t s = st->ctx->stream;
    if (fld && (ft->vfCopies.empty() || ft->vfGen != st->momVfGen)) {
        double *copy = nullptr;
        if (int rc = ft->mem.alloc(&copy, nEK)) return rc;
        ft->vfCopies.push_back(copy);
        ft->vfGen = st->momVfGen;
        HIPCHK(st->ctx, hipMemcpyAsync(copy, fld, nEK * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    if (int rc = moka_step_rk4_taped(ft->inner, dt)) return rc;
    const size_t i = ft->steps.size();
    if (qd)                      // u*, before the pass overwrites it
        HIPCHK(st->ctx, hipMemcpyAsync(ft->usRec + nEK * i, st->lev[1].u, nEK * sizeof(double), hipMemcpyDeviceToDevice, s));
    else if (wsp)                // Cd == 0 and the density of Cd wanted: sp of u* straight into the record (no state memory is written)
        HIPCHK(st->ctx, launch_momentum_bottom_speed(bottom_speed_args(st, st->lev[1].u, ft->spRec + (size_t)p.nE * i), s));
    if (on && dt != 0.0)         // the split step of moka_step_rk4, on the same two arrays (rk4_end has made them the current level)
        if (int rc = momentum_vmix(st, st->lev[1].u, st->lev[1].h, dt)) return rc;
    if (qd)                      // the sp the pass used
        HIPCHK(st->ctx, hipMemcpyAsync(ft->spRec + (size_t)p.nE * i, st->momSpeed, (size_t)p.nE * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (rec) {
        HIPCHK(st->ctx, hipMemcpyAsync(ft->unRec + nEK * i, st->lev[1].u, nEK * sizeof(double), hipMemcpyDeviceToDevice, s));
        HIPCHK(st->ctx, hipMemcpyAsync(ft->hnRec + nCK * i, st->lev[1].h, nCK * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    ForcedStep fs{rec, on, st->momTau && st->momTauOn, mom_vmix_nu(st), st->momDrag, fld ? (int32_t)ft->vfCopies.size() - 1 : -1};
    fs.cd = qd ? st->momCd : 0.0;
    fs.sp = wsp;
    ft->steps.push_back(fs);
    ++st->forcedSteps;
    return MOKA_OK;
}

static int forced_zero_densities(moka_forced_tape *ft)
{
    for (double *d : ft->dens)
        if (d) HIPCHK(ft->st->ctx, hipMemsetAsync(d, 0, (size_t)ft->st->mesh->plan.nE * sizeof(double), ft->st->ctx->stream));
    if (ft->wantF) {
        const Plan &p = ft->st->mesh->plan;
        HIPCHK(ft->st->ctx, hipMemsetAsync(ft->densF, 0, (size_t)p.K * p.nE * sizeof(double), ft->st->ctx->stream));
    }
    if (ft->densCd) HIPCHK(ft->st->ctx, hipMemsetAsync(ft->densCd, 0, (size_t)ft->st->mesh->plan.nE * sizeof(double), ft->st->ctx->stream));
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
            a.fld = r.vf >= 0 ? ft->vfCopies[(size_t)r.vf] : nullptr;
            a.DF = ft->wantF ? ft->densF : nullptr;
            if (r.sp) {                 // a quadratic tape: the step's sp, its Cd, and the density of Cd while it is flagged
                a.speed = ft->spRec + (size_t)p.nE * i; a.cd = r.cd;
                a.Dcd = ft->wantCd ? ft->densCd : nullptr;
                if (r.cd != 0.0) {      // M: 0.0 at the edges with no active level, which no lane writes
                    a.M = ft->M;
                    HIPCHK(st->ctx, hipMemsetAsync(ft->M, 0, (size_t)p.nE * sizeof(double), st->ctx->stream));
                }
            }
            const bool launched = ft->want != 0 || ft->wantF || (a.speed && a.Dcd) || (r.on && !(p.K < 2 && r.drag == 0.0 && r.cd == 0.0 && !a.tau));
            HIPCHK(st->ctx, launch_momentum_vmix_adjoint(a, generic, st->ctx->stream));
            HIPCHK(st->ctx, launch_momentum_vmix_gather(a, st->ctx->stream));
            if (r.cd != 0.0) {          // the transpose of the bottom-speed stencil, on the adjoint of u* the pass has just left
                const MeshDev &d = st->mesh->dev;
                MomSpeedAdjArgs g{};
                g.nE = p.nE; g.K = p.K; g.ME = p.ME;
                g.ehdr = d.ehdr; g.eoc = d.eoc; g.mltc = d.mltc; g.keCoef = d.keCoef; g.invArea = d.invArea;
                g.M = ft->M; g.us = ft->usRec + nEK * i; g.xu = a.xu;
                HIPCHK(st->ctx, launch_momentum_speed_adjoint(g, st->ctx->stream));
            }
            if (launched) ft->path = momentum_vmix_adjoint_form(p.K, generic, a.fld != nullptr);
        }
        for (int sg = 4; sg >= 1; --sg)
            if (int rc = rk4_reverse_stage(t, sg)) return rc;
        ft->steps.pop_back();
        --st->forcedSteps;
    }
    if (!ft->vfCopies.empty()) {        // the tape is empty: the field copies go once the last launch that reads one has finished
        HIPCHK(st->ctx, hipStreamSynchronize(st->ctx->stream));
        for (double *&c : ft->vfCopies) ft->mem.release(c);
        ft->vfCopies.clear();
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
        const size_t mark = ft->mem.mark();
        for (int b = 0; b < 3; ++b)
            if ((what >> b & 1) && !ft->dens[b])
                if (int rc = ft->mem.alloc(&fresh[b], (size_t)st->mesh->plan.nE)) {
                    ft->mem.rollback(mark);         // nothing changes: the densities this call took go back
                    return rc;
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

int moka_forced_adjoint_want_viscosity_field_gradient(moka_forced_tape *ft, int on)
{
    if (!ft) return fail(nullptr, MOKA_ERR_ARG, "forced tape is NULL");
    moka_state *st = ft->st;
    if (!ft->steps.empty()) return fail(st->ctx, MOKA_ERR_ARG, "forced tape: gradients are flagged while no step is recorded");
    if (on && !ft->densF) {
        HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
        const Plan &p = st->mesh->plan;
        if (int rc = ft->mem.alloc(&ft->densF, (size_t)p.K * p.nE)) return rc;
        HIPCHK(st->ctx, hipStreamSynchronize(st->ctx->stream));
    }
    ft->wantF = on != 0;
    return MOKA_OK;
}

int moka_forced_adjoint_viscosity_field_density_download(moka_forced_tape *ft, double *host)
{
    if (!ft || !host) return fail(ft ? ft->st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    if (!ft->wantF) return fail(ft->st->ctx, MOKA_ERR_ARG, "forced tape: the viscosity field gradient is not flagged");
    const Plan &p = ft->st->mesh->plan;
    HIPCHK(ft->st->ctx, hipSetDevice(ft->st->ctx->device));
    return get_rows(ft->st->mesh, host, ft->densF, MOKA_EDGE, p.nE, p.K);
}

int moka_forced_adjoint_want_quadratic_drag_gradient(moka_forced_tape *ft, int on)
{
    if (!ft) return fail(nullptr, MOKA_ERR_ARG, "forced tape is NULL");
    moka_state *st = ft->st;
    if (!ft->quadratic) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "forced tape: the gradient of Cd needs a tape of moka_forced_tape_create_quadratic");
    if (!ft->steps.empty()) return fail(st->ctx, MOKA_ERR_ARG, "forced tape: gradients are flagged while no step is recorded");
    if (on && !ft->densCd) {
        HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
        if (int rc = ensure_ke_coef(st->mesh)) return rc;       // a step with Cd == 0 launches the bottom speed for the record
        if (int rc = ft->mem.alloc(&ft->densCd, (size_t)st->mesh->plan.nE)) return rc;
        HIPCHK(st->ctx, hipStreamSynchronize(st->ctx->stream));
    }
    ft->wantCd = on != 0;
    return MOKA_OK;
}

int moka_forced_adjoint_quadratic_drag_density_download(moka_forced_tape *ft, double *host)
{
    if (!ft || !host) return fail(ft ? ft->st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    if (!ft->wantCd) return fail(ft->st->ctx, MOKA_ERR_ARG, "forced tape: the gradient of Cd is not flagged");
    HIPCHK(ft->st->ctx, hipSetDevice(ft->st->ctx->device));
    return get_rows(ft->st->mesh, host, ft->densCd, MOKA_EDGE, ft->st->mesh->plan.nE, 1);
}

// the caller's edge numbering, ascending, one rounding at the end: independent of the plan's order
static double host_sum(const std::vector<double> &w)
{
    long double sum = 0.0L;
    for (double v : w) sum += (long double)v;
    return (double)sum;
}

int moka_forced_adjoint_quadratic_drag_gradient(moka_forced_tape *ft, double *out)
{
    if (!ft || !out) return fail(ft ? ft->st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    std::vector<double> w((size_t)ft->st->mesh->plan.nE);
    if (int rc = moka_forced_adjoint_quadratic_drag_density_download(ft, w.data())) return rc;
    *out = host_sum(w);
    return MOKA_OK;
}

int moka_forced_adjoint_gradient(moka_forced_tape *ft, int what, double *out)
{
    if (!ft || !out) return fail(ft ? ft->st->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    std::vector<double> w((size_t)ft->st->mesh->plan.nE);
    if (int rc = moka_forced_adjoint_density_download(ft, what, w.data())) return rc;
    *out = host_sum(w);
    return MOKA_OK;
}

int moka_forced_tape_vmix_path(const moka_forced_tape *ft) { return ft ? ft->path : 0; }

int64_t moka_forced_tape_device_arrays(const moka_forced_tape *ft) { return ft ? (int64_t)ft->mem.ptrs.size() : 0; }

}  // extern "C"
