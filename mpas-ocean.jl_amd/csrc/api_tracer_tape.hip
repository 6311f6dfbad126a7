// api_tracer_tape.hip -- C ABI, continued: the moka_tracer_tape entry points.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <new>
#include <string>
#include <vector>

#include "state.hpp"
#include "tapes.hpp"

// ---------------------------------------------------------------------------------------------
// reverse mode of the tracer transport over a frozen flow (include/moka_hip.h: the algebra; tracer_adjoint.hip: the kernels).  A handle of
// its own, separate from moka_tape: the tracer step is linear in phi, so its transpose needs the recorded provisional states only.
// ---------------------------------------------------------------------------------------------
using namespace mk;

extern "C" {

int moka_tracer_tape_create(moka_state *st, int64_t capacity_steps, moka_tracer_tape **out)
{
    if (!st || !out || capacity_steps < 0) return fail(st ? st->ctx : nullptr, MOKA_ERR_ARG, "bad argument");
    *out = nullptr;
    if (st->nTracers == 0) return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "tracer reverse mode: the state has no tracers (moka_set_tracers)");
    if (st->rich)      // (the step is no longer linear in the buoyancy tracer, and the diffusivity depends on the flow)
        return fail(st->ctx, MOKA_ERR_UNSUPPORTED, "Richardson closure: no reverse mode through or beside it (moka_set_richardson_mixing(st, NULL) first)");
    const Plan &p = st->mesh->plan;
    HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
    moka_tracer_tape *t = new (std::nothrow) moka_tracer_tape();
    if (!t) return fail(st->ctx, MOKA_ERR_ALLOC, "out of host memory");
    t->st = st; t->ctx = st->ctx;
    t->mem.ctx = st->ctx; t->mem.owner = "tracer tape";
    t->nT = st->nTracers;
    t->G.assign((size_t)t->nT, nullptr);
    t->wantG.assign((size_t)t->nT, 0);
    t->wantK.assign((size_t)t->nT, 0);
    t->wantV.assign((size_t)t->nT, 0);
    t->capacity = capacity_steps;
    const size_t nEK = (size_t)p.K * p.nE, nCK = (size_t)p.K * p.nC, cap = (size_t)capacity_steps;
    int rc = MOKA_OK;
    auto A = [&](double **q, size_t n) { if (rc == MOKA_OK) rc = t->mem.alloc(q, n); };
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
    const bool alive = !t->counted || state_detach(t->st);      // (not counted: inside a failed moka_tracer_tape_create)
    if (alive) {                         // a state that went first synchronised its stream when it did: nothing of this tape is in flight
        (void)hipSetDevice(t->ctx->device);
        (void)hipStreamSynchronize(t->ctx->stream);
    }
    t->mem.release_all();
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
        if (int rc = t->mem.alloc(&t->vfTab, (size_t)t->capacity * t->nT)) return rc;
        t->vfStep.assign((size_t)t->n * t->nT, -1);
        t->vfNewest.assign((size_t)t->nT, -1);
        t->vfGen.assign((size_t)t->nT, 0);
    }
    if (!fresh.empty()) {
        std::vector<double *> got(fresh.size(), nullptr);
        const size_t mark = t->mem.mark();
        for (double *&d : got)
            if (int rc = t->mem.alloc(&d, nCK)) { t->mem.rollback(mark); return rc; }
        for (size_t i = 0; i < fresh.size(); ++i) {
            const int j = fresh[i];
            t->vfCopies.push_back(got[i]);
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
        if (int rc = mm->mem.upload(mm->plan.dvdc, &mm->dvdc)) return rc;
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
            if (int rc = t->mem.alloc(&t->vmScratch, 2 * nCK)) return rc;
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
        for (double *&q : t->vfCopies) t->mem.release(q);
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
        if (int rc = t->mem.alloc(&t->G[j], (size_t)p.K * p.nC)) return rc;
    if (!t->Gdev)
        if (int rc = t->mem.alloc(&t->Gdev, (size_t)t->nT)) return rc;
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
    double *P = nullptr, *Lk = nullptr, *W = nullptr, *ones = nullptr, *mOn = nullptr;
    int32_t *trDev = nullptr;
    double **wDev = nullptr;
    int rc = MOKA_OK;
    if (nF > 0) {
        const size_t mark = t->mem.mark();
        auto A = [&](double **q, size_t n) { if (rc == MOKA_OK) rc = t->mem.alloc(q, n); };
        A(&P, nCK * 4 * nF * cap); A(&Lk, nCK * nF); A(&W, 2 * nF * (size_t)p.nC); A(&ones, nF); A(&mOn, cap * t->nT);
        if (rc == MOKA_OK) rc = t->mem.alloc(&trDev, nF);
        if (rc == MOKA_OK) rc = t->mem.alloc(&wDev, 2 * nF);
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
            t->mem.rollback(mark);
            return rc;
        }
    }
    for (double **q : {&t->kgP, &t->kgL, &t->kgW, &t->kgOnes, &t->kgMOn}) t->mem.release(*q);
    t->mem.release(t->kgTracerDev);
    t->mem.release(t->kgWdev);
    t->kgP = P; t->kgL = Lk; t->kgW = W; t->kgOnes = ones; t->kgMOn = mOn;
    t->kgTracerDev = trDev; t->kgWdev = wDev;
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
    double *P = nullptr, *D = nullptr;
    int32_t *sl = nullptr;
    if (nV > 0) {
        const size_t mark = t->mem.mark();
        int rc = t->mem.alloc(&P, nCK * nV * cap);
        if (rc == MOKA_OK) rc = t->mem.alloc(&D, nCK * nV);
        if (rc == MOKA_OK) rc = t->mem.alloc(&sl, (size_t)t->nT);
        if (rc == MOKA_OK) rc = h2d(t->ctx, sl, slot.data(), slot.size() * sizeof(int32_t));
        if (rc != MOKA_OK) {
            t->mem.rollback(mark);
            return rc;
        }
    }
    t->mem.release(t->vgP);
    t->mem.release(t->vgD);
    t->mem.release(t->vgSlot);
    t->vgP = P; t->vgD = D; t->vgSlot = sl;
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

}  // extern "C"
