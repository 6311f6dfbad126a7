// state.hpp -- the objects behind the opaque handles of include/moka_hip.h and the helpers the api*.hip files share with each other
// and with halo.hip (the three tapes: tapes.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <initializer_list>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "kernels.hpp"
#include "moka_internal.hpp"

struct moka_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t comm = nullptr;                       // halo pack / transport / unpack
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t evBoundary = nullptr, evInterior = nullptr, evHalo = nullptr;
    int variant = 0;
    int nCUs = 256;
    std::string err;
    // per-stage HIP-event timing of moka_step_rk4 (moka_stage_timing): 5 events per recorded step, read back on request
    bool stageTiming = false;
    std::vector<hipEvent_t> evPool;          // events owned by the context (reused between measurements)
    size_t evUsed = 0;
    // per-step statistics of a timed region (moka_mark / moka_marks_read): one event per mark on the compute stream
    std::vector<hipEvent_t> marks;
    size_t marksUsed = 0;
    // same-run bandwidth calibration (moka_bw_probe): two halves of one allocation, kept between the probes of a run
    void *bwBuf = nullptr;
    size_t bwBytes = 0;
};

namespace mk {

int fail(moka_ctx *ctx, int code, const std::string &msg);
// every host->device copy of the library: on the context's stream, then synchronised (see api.hip)
int h2d(moka_ctx *ctx, void *dst, const void *src, size_t bytes);

#define HIPCHK(ctx, call)                                                                          \
    do {                                                                                           \
        hipError_t _e = (call);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return mk::fail(ctx, MOKA_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_e)); \
    } while (0)

// The device memory a handle owns: every hipMalloc / hipFree of a mesh, a state, a tape or a halo happens here (the mesh's opBuf, the
// context's probe buffers, placement.hip and inspect.hip manage transient memory of another kind).  A list of pointers, not a pool:
// nothing is cached or reused.  Only rollback() synchronises: a caller that releases memory a launch may still read synchronises first.
struct DeviceAllocs {
    moka_ctx *ctx = nullptr;         // device and stream, set when the handle is created: a tape or halo reaches them after its state has gone
    const char *owner = nullptr;     // "tape", ...: a failed hipMalloc is MOKA_ERR_ALLOC "<owner>: hipMalloc of N bytes: ..."; nullptr (mesh, state, halo): MOKA_ERR_HIP
    std::vector<void *> ptrs;

    int take(void **out, size_t bytes, bool zero)
    {
        void *d = nullptr;
        const hipError_t e = hipMalloc(&d, std::max<size_t>(bytes, 16));
        if (e != hipSuccess)
            return fail(ctx, owner ? MOKA_ERR_ALLOC : MOKA_ERR_HIP,
                        (owner ? std::string(owner) + ": " : std::string()) + "hipMalloc of " + std::to_string(bytes) + " bytes: " + hipGetErrorString(e));
        ptrs.push_back(d);
        if (zero) HIPCHK(ctx, hipMemsetAsync(d, 0, bytes, ctx->stream));
        *out = d;
        return MOKA_OK;
    }
    // elems elements (at least 16 bytes), zeroed on the context's stream (KA.zeros).  elemBytes: the float arrays of an fp32-storage state
    // sit behind double pointers
    template <class T>
    int alloc(T **out, size_t elems, size_t elemBytes = sizeof(T))
    {
        void *d = nullptr;
        if (int rc = take(&d, elems * elemBytes, true)) return rc;
        *out = static_cast<T *>(d);
        return MOKA_OK;
    }
    // a copy of v (at least 16 bytes, no zero fill) through h2d; U is T or const T
    template <class T, class U>
    int upload(const std::vector<T> &v, U **out)
    {
        void *d = nullptr;
        if (int rc = take(&d, v.size() * sizeof(T), false)) return rc;
        if (int rc = h2d(ctx, d, v.data(), v.size() * sizeof(T))) return rc;
        *out = static_cast<U *>(d);
        return MOKA_OK;
    }
    size_t mark() const { return ptrs.size(); }
    // back to mark(): the stream is synchronised (the zero fills), then what came since is freed, newest first
    void rollback(size_t mark)
    {
        (void)hipStreamSynchronize(ctx->stream);
        while (ptrs.size() > mark) { (void)hipFree(ptrs.back()); ptrs.pop_back(); }
    }
    // several arrays of doubles, all of them or none
    int alloc_all(std::initializer_list<std::pair<double **, size_t>> what)
    {
        const size_t m = mark();
        std::vector<double *> got;
        for (auto &w : what) {
            double *d = nullptr;
            if (int rc = alloc(&d, w.second)) { rollback(m); return rc; }
            got.push_back(d);
        }
        size_t i = 0;
        for (auto &w : what) *w.first = got[i++];
        return MOKA_OK;
    }
    // frees p and sets it to nullptr; a null p is left alone
    template <class T>
    void release(T *&p)
    {
        if (!p) return;
        ptrs.erase(std::remove(ptrs.begin(), ptrs.end(), (void *)p), ptrs.end());
        (void)hipFree((void *)p);
        p = nullptr;
    }
    void release_all()
    {
        for (void *q : ptrs) (void)hipFree(q);
        ptrs.clear();
    }
};

}  // namespace mk

struct moka_mesh {
    moka_ctx *ctx = nullptr;
    moka::Plan plan;          // host copy (permutations, sizes)
    moka::MeshDev dev{};
    mk::DeviceAllocs mem;
    int lpc = 1;
    bool colOk = false;       // byte-offset records exist (every field < 4 GiB)
    double *opBuf[4] = {nullptr, nullptr, nullptr, nullptr};   // operator scratch [0], [1], [3] / transfer staging [2], lazily sized
    size_t opBufElems = 0;
    // transposed lists of the operator reverse mode (moka_*_vjp), built at first use
    const int32_t *opTVert = nullptr;     // (opTW, nE) vertices naming the edge, sorted by (caller's vertex id, slot); -1 = none
    const double *opTCoef = nullptr;      // (opTW, nE) their CurlOnVertex coefficients
    const double *opESign = nullptr;      // (2, nE) edgeSignOnCell of the edge in cellsOnEdge[1], [2] (0: not listed there)
    int opTW = 0;
    // (maxOwnE, maxOwnC) of a launched patch sub-range: a partition's halo-only patches own up to 6 edges per cell
    // and are never launched, so the LDS carve of a boundary / interior launch is sized by the patches it covers
    std::map<std::pair<int, int>, std::pair<int, int>> rangeMax;
    const double *dvdc = nullptr;         // plan.dvdc on the device, uploaded by the first moka_set_tracer_diffusion with a nonzero value
    const int32_t *nLev = nullptr;        // plan.nLev on the device, uploaded when the vertical tracer diffusion first needs it
    moka::D4Rows d4{};      // Del4 mixing: per-patch edge rows of k_d4_patch, built at the first moka_set_viscosity_del4 (start == nullptr: not yet)
};

struct LevelBufs {
    double *ssh = nullptr, *u = nullptr, *h = nullptr;
};

struct moka_state {
    moka_ctx *ctx = nullptr;
    moka_mesh *mesh = nullptr;
    LevelBufs lev[2];                 // [0] previous, [1] current   (reference Vector index 1 / end)
    double *hEdge[2] = {nullptr, nullptr};   // [0] is Diag.layerThicknessEdge, [1] the write target of the next step
    double *F = nullptr, *div = nullptr, *vort = nullptr, *tendU = nullptr, *tendH = nullptr;
    LevelBufs rk[2];                  // RK4 provisional states (lazily allocated)
    // RK4 stage 1 -> stage 2 hand-off of New as one-byte codes (mk::rk_handoff_usable; Float64 states): (K, nE) and (K, nC) bytes,
    // allocated with rk[].  hoLive: the stage-1 launches of the step under way stored codes, formed with hoRho (b1 / a1 of that step),
    // and its stage-2 launches read them; cleared when stage 3 begins.  hoRan: the same of the last step begun, kept for
    // moka_state_rk_handoff_escapes.
    signed char *hoCodeU = nullptr, *hoCodeH = nullptr;
    bool hoLive = false, hoRan = false;
    double hoRho = 0.0;
    LevelBufs spare;                  // third time-level set of the tuned Forward-Euler step (lazily allocated): the step writes
                                      // the new level here, so the PREVIOUS level's layerThickness stays readable while it runs
                                      // (k_stage_rec2c mode 6), and the three sets rotate: prev <- cur <- new <- old prev
    static constexpr int NPHYS = 5;
    LevelBufs phys[NPHYS];            // the same buffer sets by allocation: [0],[1] the time levels as created (lev[] swaps /
                                      // rotates), [2],[3] = rk[], [4] = the Forward-Euler spare: what a neighbour rank addresses
                                      // when it pushes halo rows (halo.hip)
    // Diag.layerThicknessEdge (hEdge[0]) is, bit for bit, the interpolation of lev[0].layerThickness on every edge a launch
    // of this state computes: true after a Forward-Euler step of all levels through the stage kernel, false after anything
    // else that writes either array (uploads, RK4 steps, the piecewise reference calls, lazily produced diagnostics)
    bool hEdgePrev = false;
    // The last Forward-Euler step was LEAN: it stored the new time level (and relativeVorticity) only.  Its TendencyVars and
    // DiagnosticVars (tendNormalVelocity, tendLayerThickness, thicknessFlux, velocityDivCell, layerThicknessEdge) are pending:
    // produced on the first read (flush_lazy) from the level the step started from -- the previous level now -- and, for the
    // reference's stale flux thickness, the level before it, which the rotation of three level sets has kept in `spare`.
    // Same arithmetic, same bits as a step that stores everything; the next lean step reads none of those arrays and
    // supersedes them, exactly as an RK4 step supersedes its lazily produced diagnostics.
    bool feLazy = false, feLazyStale = false;
    bool feForceEager = false;        // a tape is recording: every step stores all of its arrays
    bool feLeanInteriorOnly = false;  // a direct (peer-store) halo is connected: a lean distributed step stores every array of its
                                      // BOUNDARY patches at once and leaves only the interior patches' pending (halo.hip header)
    int feLazyBegin = 0, feLazyCount = -1;   // the patch range whose arrays are pending (-1: every launched patch)
    double *scalar = nullptr;         // 1 double (sum_sq result)
    bool sshConsistent = false;       // lev[1].ssh == ksum(lev[1].h) - restingThicknessSum
    // moka_step_rk4 ends with diagnostic_compute! of the new state and leaves the stage-4 tendencies in
    // Tend (time_integration.jl:114-147).  Neither is needed by the next RK4 step, so they are produced
    // lazily -- on the first read (download, Forward-Euler step, reference-sequenced calls) -- with
    // results identical to computing them at the end of the step.
    bool diagDirty = false;
    bool tendDirty = false;           // stage-4 provisional state still sits in rk[0] -- or, after a taped step, in the tape:
    const double *lazyPu = nullptr, *lazyPh = nullptr;   // where (nullptr: rk[0]); ssh of it is rk[0].ssh either way
    const void *lazyOwner = nullptr;                     // the tape those rows belong to (it materialises them before it goes away)
    // fp32 storage of the prognostic fields (mesh stateBytes == 4): lev[] / rk[] then point at float arrays
    // (the pointer type stays double* so that one StageArgs block serves both), Diag arrays do not exist.
    bool f32 = false;
    // optional nonlinear terms (moka_set_nonlinear): scratch of the three preparation passes
    bool nonlinear = false;
    int nlPhase = 0;                  // what run_stage launches for a nonlinear state: 0 preparation + stage, 1 preparation only, 2 stage only
    double *nlQv = nullptr, *nlQe = nullptr, *nlKe = nullptr;
    int feFast = -1;                            // moka_last_fe_path
    double *nlZv = nullptr, *nlDiv = nullptr;   // Del2 mixing (moka_set_viscosity_del2); Del4 reads them too
    double viscDel2 = 0.0;
    double *nlDiv4 = nullptr, *nlCurl4 = nullptr, *coef4 = nullptr;   // Del4 mixing (moka_set_viscosity_del4): div4, curl4, viscDel4 * scaling
    double viscDel4 = 0.0;
    int del4Path = 0;                 // moka_state_del4_path
    int halos = 0;                    // live moka_halo objects on this state (Del4 refuses them)
    // passive tracers (moka_set_tracers): nTracers arrays of (K, nC) doubles, K * nC apart, per buffer.  trPhi[] are the two time
    // levels and swap with lev[] (during an RK4 step trPhi[0] carries the running content sum Qn, as lev[0] carries New); trProv[] are
    // the provisional tracers beside rk[].  nullptr without tracers.
    int nTracers = 0;
    double *trPhi[2] = {nullptr, nullptr}, *trProv[2] = {nullptr, nullptr};
    int tracerPath = 0;               // moka_state_tracer_path
    // harmonic tracer diffusion (moka_set_tracer_diffusion): the host copy (nTracers values, empty = all zero) and the device array the
    // tracer launches read -- nullptr while every value is zero: the launches are then those of a state that never set any
    std::vector<double> trKappa;
    double *trKappaDev = nullptr;
    // biharmonic tracer diffusion (moka_set_tracer_biharmonic): the host copy beside trKappa (empty = all zero); the device array of
    // 2 * nTracers doubles -- the coefficients, then nTracers zeros that stand in for the diffusivities while those are all zero (the
    // BIH kernels exist only together with DIFF) -- and the scratch of L = Lap(ph, pphi), nTracers x (K, nC).  Both are allocated when a
    // nonzero value is first set, never inside a step, and nullptr while every value is zero.
    std::vector<double> trKappa4;
    double *trKappa4Dev = nullptr, *trLap = nullptr;
    // implicit vertical tracer diffusion (moka_set_tracer_vertical_diffusion): the host copy (empty = all zero), the device array the
    // vertical pass reads and the scratch of its column form (2 * K * nC doubles).  Both are allocated when a nonzero value is first set
    // and nullptr while every value is zero: a step then launches what a state that never set one launches.
    std::vector<double> trKappaV;
    double *trKappaVDev = nullptr, *trVmixScratch = nullptr;
    int vmixPath = 0;                 // moka_state_tracer_vmix_path
    // diffusivity fields (moka_tracer_vertical_field_upload): only a tracer with a field owns a (K, nC) device array.  trVf holds nTracers
    // pointers (nullptr = the scalar) and is empty while no tracer has a field; trVfOn[j]: the field has a nonzero value at an active
    // interface (the host scan of the upload) -- one that has none counts as kappaV_j == 0.  trVfDev is the device table of the fields
    // that are on, the one the field instances of the vertical pass read, nullptr while there is none: the pass is then the scalar
    // one.  With fields, trKappaVDev holds what the pass is to take for a tracer -- 0.0 for one whose field is all zero -- and is
    // non-null exactly while some such value is nonzero or some field is on.  trVfGen[j] takes the next value of trVfClock with every
    // upload and removal (empty until the first upload): a tape compares it with that of its newest copy.
    std::vector<double *> trVf;
    std::vector<char> trVfOn;
    std::vector<uint64_t> trVfGen;
    uint64_t trVfClock = 0;
    double **trVfDev = nullptr;
    // tracer sources (moka_tracer_source_upload): only a sourced tracer owns a (K, nC) device array.  trSrc holds nTracers pointers
    // (nullptr = no source) and is empty while no tracer has a source; trSrcDev is its copy on the device, the table the tracer
    // launches read -- nullptr while trSrc is empty: the launches are then those of a state that never had a source.  Sources do
    // not rotate with the time levels.
    std::vector<double *> trSrc;
    double **trSrcDev = nullptr;
    // implicit vertical mixing of momentum (moka_set_vertical_viscosity, moka_surface_stress_upload): the two scalars; the surface
    // stress in device edge numbering (nullptr: none) and whether it has a nonzero entry at an edge with an active level (the host scan
    // of the upload; one that has none counts as absent); the scratch of the column form (2 * K * nE doubles), allocated by the first
    // call that turns the pass on and kept.  mk::mom_vmix_on says whether the pass is on.
    double momNuV = 0.0, momDrag = 0.0;
    double *momTau = nullptr, *momScratch = nullptr;
    bool momTauOn = false;
    // the viscosity field (moka_vertical_viscosity_field_upload): (K, nE) in device edge numbering, nullptr: none, and the pass takes
    // momNuV; momVfOn: it has a nonzero value at an active interface (the host scan of the upload) -- one that has none counts as
    // nuV == 0.  momVfGen takes a new value with every upload and removal: a forced tape compares it with that of its newest copy.
    double *momVf = nullptr;
    bool momVfOn = false;
    uint64_t momVfGen = 0;
    int momVmixPath = 0;              // moka_state_momentum_vmix_path
    // the quadratic bottom drag (moka_set_quadratic_bottom_drag): the coefficient; the bottom speed sp[e] in device edge numbering,
    // allocated by the first call that sets Cd != 0 and kept (nullptr: never set); momSpeedUsed: the last pass ran with it
    // (moka_bottom_speed_download hands out zeros otherwise)
    double momCd = 0.0;
    double *momSpeed = nullptr;
    bool momSpeedUsed = false;
    // the Richardson-number closure (moka_set_richardson_mixing): on or off, the parameters (tracerMask is not kept: richMask holds
    // nTracers flags), F (K, nE) and G (K, nC) in device numbering, and what the tracer pass takes while the closure is on in the place
    // of trKappaVDev / trVfDev -- richKvDev: nTracers coefficients, 0.0 for a tracer of the set, else vmix_coefficient; richVfDev:
    // nTracers pointers, G for a tracer of the set, else its own field that is on, else nullptr.  All of it is allocated when the
    // closure is switched on (never by a step), brought in line by rich_commit whenever a set-aside coefficient changes, and freed when
    // it is switched off.  richRan: the last step launched the closure (moka_richardson_fields_download hands out zeros otherwise).
    bool rich = false;
    moka_richardson_params richP{};
    std::vector<int32_t> richMask;
    double *richF = nullptr, *richG = nullptr, *richKvDev = nullptr;
    double **richVfDev = nullptr;
    bool richRan = false;
    mk::DeviceAllocs mem;
    // objects that hold or have exported the addresses of this state's arrays (halos, tapes): while any exists the arrays stay
    // where they are (moka_state_optimize_placement refuses)
    int attached = 0;
    int dycoreTapes = 0;              // live moka_tape objects on this state (moka_set_nonlinear refuses while one exists)
    // a live moka_forced_tape on this state (at most one; the moka_tape it embeds is counted here, not in dycoreTapes: the setters of the
    // vertical momentum pass keep working beside it) and the steps it holds (moka_surface_stress_upload refuses while there are any)
    int forcedTapes = 0;
    int64_t forcedSteps = 0;
    // ... and how many of them are plain (moka_forced_tape_create, not moka_forced_tape_create_quadratic): moka_set_quadratic_bottom_drag
    // refuses a nonzero Cd while this is nonzero
    int forcedPlainTapes = 0;
    std::vector<moka_placement_trial> placementLog;   // what the last moka_state_optimize_placement tried
    int64_t placementLaunches = 0;                    // ... and how many stage launches it issued (measurement bookkeeping)
};

namespace mk {

using namespace moka;

// Halos and tapes count themselves in moka_state.attached while they hold the state's addresses.  Handles may be destroyed in
// any order (garbage-collected callers: a state can go before its tape), so the count is only touched while the state is alive.
// halo = true: the object is a moka_halo (counted in moka_state.halos too)
void state_attach(moka_state *st, bool halo = false);
// false: the state has gone -- the caller skips every access to it and works with the context it cached (DeviceAllocs.ctx)
bool state_detach(moka_state *st, bool halo = false);

// The kernel choice of the linear stage launches.  The default stage kernels (launch_stage_rec2c*) may serve a Float64 state's
// launches: kernel variant 0 (auto) or 11, 64 lanes per column, byte-offset records.  Whether they do depends on the patches too
// (rec2c_supported / stage_curl_fits of launch_bounds); run_stage falls back to the column or the generic kernel.
inline bool default_stage_kernels(const moka_state *st)
{
    const int v = st->ctx->variant;
    return (v == 0 || v == 11) && st->mesh->lpc == 64 && st->mesh->colOk;
}
// the mesh as every whole-mesh stage launch sees it: maxima over the patches that are ever computed (at least 1)
inline MeshDev launch_bounds(const moka_mesh *mm)
{
    MeshDev dev = mm->dev;
    dev.maxOwnE = std::max(mm->plan.maxOwnELaunch, 1); dev.maxOwnC = std::max(mm->plan.maxOwnCLaunch, 1);
    return dev;
}
// is the vertical momentum pass on: some coefficient nonzero, Cd included (a field sets nuV aside and counts when an active entry is nonzero), or a
// stress with a nonzero entry at an edge that has an active level; or the Richardson closure, which supplies the viscosity field
inline bool mom_vmix_on(const moka_state *st)
{
    return st->rich || (st->momVf ? st->momVfOn : st->momNuV != 0.0) || st->momDrag != 0.0 || st->momCd != 0.0 || (st->momTau && st->momTauOn);
}
// what the pass takes for the viscosity: the field that is on, else the scalar -- 0.0 under a field whose active entries are all zero
inline const double *mom_vmix_field(const moka_state *st) { return st->momVf && st->momVfOn ? st->momVf : nullptr; }
inline double mom_vmix_nu(const moka_state *st) { return st->momVf ? 0.0 : st->momNuV; }
// `form` of the nonlinear launchers: kernel variants 4 / 3 select the plainer forms of the nonlinear kernels too
inline int nl_form(const moka_ctx *ctx) { return ctx->variant == 4 ? 1 : ctx->variant == 3 ? 3 : 0; }

// api.hip: the mesh's transfer staging and the row permutation between the caller's numbering and the device's
int ensure_op_bufs(moka_mesh *m);
const int32_t *perm_of(const moka_mesh *m, int kind);
int put_rows(moka_mesh *m, double *dst, const double *host, int kind, int64_t n, int K, bool f32 = false);
int get_rows(moka_mesh *m, double *host, const double *src, int kind, int64_t n, int K, bool f32 = false);
// api_state.hip
int ensure_rk_bufs(moka_state *st);
int ensure_spare(moka_state *st);
// the set a Forward-Euler step writes its new level to / the rotation that makes it the current level
LevelBufs &fe_new_level(moka_state *st);
void fe_rotate_levels(moka_state *st);
int flush_lazy(moka_state *st, bool diag, bool tend);
// one fused tendency / RK-stage launch over patches [pBegin, pBegin + pCount) (default: all) on the compute stream (or `on`)
hipError_t run_stage(moka_state *st, const StageArgs &g, int pBegin = 0, int pCount = -1, hipStream_t on = nullptr, int tail = -1);
StageArgs rk4_stage_args(moka_state *st, int s, double dt, const double *ssh0);
LevelBufs &rk4_stage_output(moka_state *st, int s);
int rk4_begin(moka_state *st, const double **ssh0);
void rk4_end(moka_state *st);
bool rk13_usable(const moka_state *st);       // the 13-stream RK4 form (moka_set_tuning key 7), see api_state.hip
bool rk_handoff_usable(const moka_state *st); // New from RK4 stage 1 to stage 2 as one-byte codes (moka_set_tuning key 12), see api_state.hip
StageArgs rk13_stage_args(moka_state *st, int s, double dt, const double *ssh0);
void rk13_end(moka_state *st);
FeArgs fe_args(moka_state *st, int ops, int flags, double dt);
StageArgs fe_stage_args(moka_state *st, const FeArgs &a, int flags);
// Forward-Euler step in the stage kernels: is that path open to this state / these flags; will the step be lean (see
// moka_state.feLazy); what a step has to do about lazily pending arrays before its launches (idempotent within a step)
bool fe_stage_path(const moka_state *st, int flags);
bool fe_lean(const moka_state *st, int flags);
int fe_begin(moka_state *st, int flags);
void fe_end(moka_state *st, int flags, bool stageKernel, bool lean, bool prevMode);
// moka_step_rk4, and the same step recorded on `rec` (nullptr: not recorded); the vertical pass of the flow behind stage 4
int step_rk4(moka_state *st, double dt, moka_tracer_tape *rec);
int momentum_vmix(moka_state *st, double *u, const double *h, double dt);
// keCoef on the device (uploaded when a state first asks); the bottom-speed launch over the whole mesh: u a (K, nE) field, sp nE doubles
int ensure_ke_coef(moka_mesh *m);
MomSpeedArgs bottom_speed_args(const moka_state *st, const double *u, double *sp);
// api_tracers.hip: the tracer launch of RK4 stage s; the vertical pass, forwards and backwards; what it takes for tracer j
hipError_t tracer_stage(moka_state *st, int s, const StageArgs &g);
int tracer_vmix(moka_mesh *mm, moka_ctx *ctx, int nT, const double *h, double *x, const double *kv, const double *const *fld, double dt,
                double *scratch, bool reverse, int *path, const int32_t *gslot = nullptr, const double *p_new = nullptr, double *D = nullptr);
bool vfield_on(const moka_state *st, int j);
double vmix_coefficient(const moka_state *st, const std::vector<double> &kv, int j);
// api_closure.hip: the Richardson closure.  rich_commit brings richKvDev / richVfDev in line with the mask, the scalars kv and the
// fields as they stand (the caller has synchronised the stream; a no-op while the closure is off); rich_drop switches the closure off
// and frees what it owns (likewise synchronised); rich_args: the launch over the whole mesh from u (K, nE), h and b (K, nC)
int rich_commit(moka_state *st, const std::vector<double> &kv);
void rich_drop(moka_state *st);
RichArgs rich_args(const moka_state *st, const double *u, const double *h, const double *b);

}  // namespace mk
