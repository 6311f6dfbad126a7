// kernels.hpp -- argument blocks and launchers of the gfx950 kernels (kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>

#include "moka_internal.hpp"

namespace moka {

// Fused tendency / RK-stage kernel.  NULL pointers switch the corresponding read/write off.
struct StageArgs {
    const double *pu, *ph;        // provisional state: the gather source of the tendency
    const double *ssh;            // ssh of the provisional state (nC)
    const double *cu, *ch;        // Curr (NULL: Curr == Provis, e.g. RK stage 1 / Forward Euler)
    const double *nu_in, *nh_in;  // New accumulator in (NULL: start from Curr)
    double *nu_out, *nh_out;      // New accumulator out
    double *pu_out, *ph_out;      // next provisional state  Curr + a*tend
    double *ssh_out;              // ssh of ph_out (or of nh_out when ph_out == NULL)
    double *tendU, *tendH;        // tendencies
    double a, b;
    // Forward-Euler step in the default stage kernel (k_stage_rec2c modes 4 / 5; every other kernel ignores these):
    // pu/ph/ssh = current level, pu_out/ph_out/ssh_out = new level, a = dt, tendU/tendH, and the diagnostics below
    // feMode != 0 marks a Forward-Euler launch and names its kernel mode (4 / 5 / 6).  Every OUTPUT group of such a launch is
    // optional: {pu_out, ph_out, ssh_out} = the new level; {tendU, tendH, F, div, hEdgeNew} = the step's TendencyVars /
    // DiagnosticVars; vort.  A lean step passes the first (and vort), the launch that materialises a lean step's arrays on
    // demand passes the second.
    int feMode;
    const double *hEdgeOld;       // previous step's layerThicknessEdge (mode 4: MOKA_FE_STALE_HEDGE) or NULL (modes 5, 6)
    const double *hPrev;          // mode 6: the previous time level's layerThickness, which hEdgeOld is the interpolation of
    double *hEdgeNew, *F, *div;   // layerThicknessEdge, thicknessFlux, velocityDivCell
    const double *areaCell;
    // relativeVorticity of the OLD state (CurlOnVertex, Operators.jl:137-146) by the same launch: the vertices of the launched
    // patches, normalVelocity rows from the patch's LDS row cache where it has them.  NULL: the caller launches the vertex
    // pass itself (k_curl3 / k_fe).  vertexDegree 3 meshes with byte-offset records only (stage_curl_fused()).
    double *vort;
    int accumVort;                // MOKA_FE_ACCUM_VORT: on top of what the array holds (Operators.jl:135,142)
    // 13-stream RK4 form (k_stage_rec2c modes 7 / 8 / 9; Float64 states): rkMode names the mode.  7: pu/ph -> pu_out/ph_out/ssh_out;
    // 8: + cu/ch; 9: pu/ph = P4 (gathered), own rows cu/ch = Curr, nu_in/nh_in = P2, q3u/q3h = P3 -> nu_out/nh_out (may alias
    // nu_in/nh_in: every entity reads its own row of P2 before it writes there), ssh_out = ssh of New, b = dt/6
    int rkMode;
    const double *q3u, *q3h;
    // RK4 stage 1 -> stage 2 hand-off of New as one-byte codes (k_stage_rec2c modes 12 / 13; rk_handoff_* in kernels_common.hpp;
    // mk::rk_handoff_usable): (K, nE) / (K, nC) bytes beside New, NULL = New travels in full.  rho = b1 / a1 of the step, the same
    // double in both launches.
    signed char *codeU, *codeH;
    double rho;
};

// the slice of MeshDev the column kernel reads (kept small: kernel arguments live in SGPRs)
struct ColMesh {
    int32_t nC, nE, K, nPatches, patchBegin, CI, EI;
    const int32_t *patchCellStart, *patchEdgeStart;
    const uint32_t *cRec, *eRec;
    const int32_t *mltc;
    const double *sdv, *invArea, *rsum, *woe, *feoe, *gInvDc;
    int32_t tailPlus1;   // != 0: the launch's last workgroup takes patch tailPlus1 - 1 instead of patchBegin + nPatches - 1
    // vertex pass of the Forward-Euler modes (StageArgs.vort): the patches' vertex ranges, u-row offsets and coefficients
    const int32_t *patchVertStart;
    const uint32_t *vRec;
    const double *cv;
    int32_t maxOwnV;
    // > 0: every workgroup of this launch takes TWO consecutive patches (2 * block, 2 * block + 1 of the launched range, the last one
    // alone when their number is odd) as one unit -- one staging phase, one row cache over both patches' own edges -- and pairEnd
    // is the end of the launched patch range (absolute).  k_stage_rec2c, 512 threads; see launch_stage_rec2c.
    int32_t pairEnd;
};

enum : int {
    FE_FLUX = 1, FE_DIV = 2, FE_CURL = 4, FE_HEDGE = 8, FE_TENDU = 16, FE_TENDH = 32, FE_UPDATE = 64,
    FE_TENDH_FROM_F = 128
};

struct FeArgs {
    int ops, flags, nlev;
    double dt;
    const double *u, *h, *ssh;    // current time level
    const double *hEdgeOld;       // layerThicknessEdge as the previous step left it
    const double *Fin;            // stored thicknessFlux (FE_TENDH_FROM_F)
    double *hEdgeNew, *F, *div, *vort, *tendU, *tendH;
    double *u_new, *h_new, *ssh_new;
};

// OP_*_T: the transposes (reverse mode of the stand-alone operators, moka_*_vjp), gather form, fixed summation order
enum : int { OP_GRADIENT = 0, OP_INTERP = 1, OP_DIV_P1 = 2, OP_DIV_P2 = 3, OP_CURL = 4, OP_GRAD_T = 5, OP_DIV_T = 6, OP_CURL_T = 7 };

struct OpArgs {
    int op, nlev;
    const double *in;
    double *out;
    // transposes only
    const double *in2 = nullptr;       // OP_DIV_T: the shadow of temp (added in before the multiplication by dvEdge)
    const int32_t *auxI = nullptr;     // OP_CURL_T: (W, nE) vertices whose edgesOnVertex lists name the edge, by (caller's vertex id, slot); -1 = none
    const double *auxD = nullptr;      // OP_CURL_T: (W, nE) their coefficients; OP_DIV_T: (2, nE) edgeSignOnCell of the edge in c1, c2
    int auxW = 0;
};

// the product's stage kernels: default (kernels.hip) and the two fallbacks (stage_fallback.hip)
hipError_t launch_stage(const MeshDev &m, const StageArgs &a, int lpc, hipStream_t s);          // generic index kernel
hipError_t launch_stage_col(const MeshDev &m, const StageArgs &a, hipStream_t s);               // plain column kernel
hipError_t launch_stage_rec2c(const MeshDev &m, const StageArgs &a, hipStream_t s);
bool rec2c_supported(const MeshDev &m);
// can the Forward-Euler modes of the stage kernels carry the relativeVorticity pass of this mesh (StageArgs.vort)
bool stage_curl_fused(const MeshDev &m);
bool stage_curl_fits(const MeshDev &m, bool f32);      // ... with patches of m.maxOwnE / m.maxOwnC own edges / cells
// fp32-state form (state pointers of StageArgs are float arrays); stage_f32_supported: can this mesh carry one
bool stage_f32_supported(const MeshDev &m);
hipError_t launch_stage_rec2c_f32(const MeshDev &m, const StageArgs &a, hipStream_t s);

// Process-wide launch-shape switches: the keys of moka_set_tuning / moka_get_tuning (include/moka_hip.h).  One table in api.hip
// holds each key's default and accepted values; launchers read the current value through tuning().
enum TuningKey : int {
    TUNE_F32_WIDE = 1,       // bit mask: modes of the fp32-storage kernel run as 512-thread workgroups (4 waves per SIMD)
    TUNE_FE_PREV = 2,        // 0 = never form the stale layerThicknessEdge from the previous level (mode 6)
    TUNE_CURL_FUSED = 3,     // 0 = the Forward-Euler vertex pass always gets a launch of its own
    TUNE_FE_LEAN = 4,        // 0 = Forward-Euler steps always store every array (no lean steps)
    TUNE_NL_SHAPE = 5,       // launch shape of the nonlinear stage kernel's patch form (nonlinear.hip, nl_stage_kernel)
    TUNE_NL_CAP = 6,         // test hook: upper limit of the vertex rows k_stage_nl5 keeps resident (0 = none)
    TUNE_RK13 = 7,           // 1 = RK4 steps in the 13-stream form where mk::rk13_usable (NOT result-neutral)
    TUNE_PAIR = 8,           // bit mask: modes of the Float64 stage kernel that take two patches per 512-thread workgroup
    TUNE_FE_LEAN_INST = 9,   // 0 = lean Forward-Euler launches through the general instances (modes 5 / 6) instead of 10 / 11
    TUNE_RK_HANDOFF = 12,    // 1 = RK4 stage 1 hands New to stage 2 as one-byte codes where mk::rk_handoff_usable (10, 11: no such keys)
};
int tuning(TuningKey key);

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) of each kernel in `fns` to `bytes`, once per device and kernel (the attribute is
// a per-device property of a kernel; a process may drive several devices, e.g. LocalCluster over a device list).  Called by the
// launchers ahead of their first large launch, never inside a stream capture: moka_run steps eagerly before it captures.
hipError_t raise_dyn_lds(std::initializer_list<const void *> fns, int bytes);
hipError_t launch_update_ssh_f32(const MeshDev &m, const float *h, float *ssh, int nlev, int lpc, hipStream_t s);
hipError_t launch_permute_rows_f32(void *dst, const void *src, const int32_t *n2o, int64_t n, int K, int to_device,
                                   hipStream_t s);
hipError_t launch_halo_map_f32(float *buf, float *h, float *ssh, float *u, const uint32_t *map, int64_t n, int unpack,
                               hipStream_t s);
hipError_t launch_fe(const MeshDev &m, const FeArgs &a, int lpc, hipStream_t s);
hipError_t launch_curl2(const MeshDev &m, const double *u, double *vort, bool accum, hipStream_t s);
hipError_t launch_curl_f32(const MeshDev &m, const float *u, float *vort, bool accum, hipStream_t s);   // fp32-storage states
hipError_t launch_operator(const MeshDev &m, const OpArgs &a, int lpc, hipStream_t s);
hipError_t launch_update_ssh(const MeshDev &m, const double *h, double *ssh, int nlev, int lpc, hipStream_t s);
hipError_t launch_permute_rows(double *dst, const double *src, const int32_t *n2o, int64_t n, int K, int to_device,
                               hipStream_t s);
hipError_t launch_sum_sq_serial(const double *a, int64_t n, double *out, hipStream_t s);
hipError_t launch_copy(double *dst, const double *src, int64_t n, hipStream_t s);
// bandwidth probes of the same-run calibration (moka_bw_probe): 16-byte-per-lane copy / read-only sweep of `bytes`
hipError_t launch_bw_copy(void *dst, const void *src, int64_t bytes, int nCUs, hipStream_t s);
hipError_t launch_bw_streams(void *buf, int64_t bytes, hipStream_t s);
hipError_t launch_bw_gather_n(const void *src, int64_t nRows, uint32_t rowB, int64_t nFetch, uint32_t *sink, int nCUs, hipStream_t s);
hipError_t launch_bw_read(const void *src, int64_t bytes, uint32_t *sink, int nCUs, hipStream_t s);
hipError_t launch_bw_gather(const void *src, int64_t bytes, uint32_t rowB, uint32_t *sink, int nCUs, hipStream_t s);
// halo pack / unpack: rows of (K doubles) gathered into / scattered from a contiguous buffer
hipError_t launch_halo_map(double *buf, double *h, double *ssh, double *u, const uint32_t *map, int64_t n, int unpack,
                           hipStream_t s);
hipError_t launch_pack_rows(double *buf, const double *field, const int32_t *rows, int64_t n, int K, int unpack, hipStream_t s);

// ---- optional nonlinear terms (not in the reference): scratch arrays of the preparation passes ----
struct NlArgs {
    double *qv;     // (K, nV) potential vorticity at vertices
    double *fq;     // (K, nE) pairs {thickness flux u * layerThicknessEdge, potential vorticity averaged to the edge}
    double *ke;     // (K, nC) kinetic energy at cells
    // Del2 momentum mixing (moka_set_viscosity_del2; horizontal_momentum_mixing.jl:53-80): nullptr / 0 = term absent
    double *zv;     // (K, nV) relativeVorticity
    double *divc;   // (K, nC) velocityDivCell
    double visc;
    // Del4 momentum mixing (moka_set_viscosity_del4): read by the stage kernels' Del4 instances only (launch_stage_nl picks them
    // when coef4 != nullptr).  div4 / curl4 = DivergenceOnCell / CurlOnVertex of L(u), the Del2 bracket of zv / divc (launch_del4)
    const double *div4;    // (K, nC)
    const double *curl4;   // (K, nV)
    const double *coef4;   // (nE) viscDel4 * meshScalingDel4
};
// form: 0 = best available, 1 = patch kernels without the LDS q_e rows, 2 = 16-byte-lane entity kernels, 3 = generic lane-group kernels
// (prepare and stage must be called with the same form: forms 0 / 1 keep F alone in NlArgs.fq, forms 2 / 3 {F, q_e} pairs)
bool nl_stage_is_nl5(const MeshDev &m, int lpc, bool rowsOk, int form);  // the nonlinear stage launch of this mesh is k_stage_nl5 (knows StageArgs.rkMode 9)
bool nl_patch_forms(const MeshDev &m, int lpc, int form);   // do the nonlinear launches of this mesh go through the per-patch kernels (which serve patch ranges)
hipError_t launch_nl_prepare(const MeshDev &m, const double *u, const double *h, const NlArgs &nl, int lpc, int form, hipStream_t s);
// rowsOk: the plan built the patch row lists (rowStart / rowEdge / leoe; Plan.ldsOk)
hipError_t launch_stage_nl(const MeshDev &m, const StageArgs &a, const NlArgs &nl, int lpc, bool rowsOk, int form, hipStream_t s);
// Del4 momentum mixing: div4 / curl4 of d2u = L(u) from divc / zv of the preparation pass (which must have run on the same stream).
// D4Rows: per-patch lists of the edges whose d2u the patch's own cells and vertices read (built once per mesh, plan order).
struct D4Rows {
    const int32_t *start;   // nPatches + 1: rows of patch q are row[start[q] .. start[q+1])
    const int32_t *row;     // edge ids
    const uint16_t *locC;   // (ME, nC): patch-local row of the edge in slot i of the cell (0 for empty slots)
    const uint16_t *locV;   // (VD, nV): patch-local row of the edge in slot j of the vertex
    int32_t maxRows;
};
// 1 = the fused patch kernel k_d4_patch serves this mesh / form (the nonlinear path runs its patch preparation pass and the rows of
// the largest patch fit the LDS budget), 2 = the entity kernels k_d4_cell / k_d4_vertex
int del4_path(const MeshDev &m, const D4Rows &r, int lpc, int form);
hipError_t launch_del4(const MeshDev &m, const D4Rows &r, const double *divc, const double *zv, double *div4, double *curl4, int path,
                       hipStream_t s);

// ---- passive tracers (moka_set_tracers; tracers.hip): one launch per RK4 stage behind the dycore's stage launch, all tracers ----
// Arrays of nT tracers lie `stride` doubles apart.  With T the flux-form tendency of include/moka_hip.h, per tracer and element:
//   Qc = cphi * hcur;  stage < 4: pphi_out = (Qc + a * T) / hnext;  Qn = (stage 1 ? Qc : qn) + b * T;  qn = stage 4 ? Qn / hnext : Qn
struct TracerArgs {
    int nT, stage;                // stage 1..4
    int64_t stride;               // K * nC
    const double *pu, *ph;        // the stage's provisional normalVelocity / layerThickness (gathered)
    const double *hcur;           // the current level's layerThickness (stage 1: == ph)
    const double *hnext;          // the next provisional layerThickness (stages 1-3) / the new level's (stage 4)
    const double *pphi;           // the stage's provisional tracers (stage 1: the current level's; gathered)
    const double *cphi;           // the current level's tracers
    double *pphi_out;             // the next provisional tracers (stage 4: unused)
    double *qn;                   // the running content sum: written by stage 1, read + written by 2 and 3; stage 4 leaves the new level's tracers there
    double a, b;
    // harmonic diffusion (moka_set_tracer_diffusion): nT diffusivities and the plan's (nC, ME) dvEdge / dcEdge per slot; both nullptr
    // while every diffusivity of the state is zero (the launch is then the one of a state that never set any)
    const double *kappa, *dvdc;
    // sources (moka_tracer_source_upload): nT device pointers, tracer j's (K, nC) source or nullptr for a tracer without one; the
    // table itself is nullptr while no tracer of the state has a source (the launch is then the one of a state that never had any).
    // After the slot loop T = T + q[k,c], the cell's own element, read from global memory.
    const double *const *src;
    // biharmonic diffusion (moka_set_tracer_biharmonic): nT coefficients kappa4 and the base of L = Lap(ph, pphi) (nT fields `stride`
    // apart, written by launch_tracer_lap on the same stream); both nullptr while every kappa4 of the state is zero (the launch is then
    // the one of a state that never set any).  L of a tracer with kappa4[j] == 0 is never written and never read.  Set only together
    // with kappa and dvdc (a state whose diffusivities are all zero passes an array of zeros).
    const double *kappa4, *lap;
};
// The kernel that serves a tracer launch, chosen in one place for the launcher and for moka_state_tracer_path.  form 1: k_tracer_patch
// (even 34 <= K <= 64, hexagon-width byte-offset records, which exist only where every field's rows stay below 4 GiB; `chunk` tracers'
// rows resident in `lds` bytes of dynamic LDS per pass), form 2: k_tracer_cell.  generic: the caller asks for form 2 (kernel variant 3).
// diff: the DIFF instantiations (the patch form then stages dvdc too: more LDS, possibly a smaller chunk).
// bih: the BIH instantiations (a resident tracer takes a second row set, for L: half as many tracers per pass; form 2 when not even
// one tracer's two row sets fit).
struct TracerKernel {
    int form;
    size_t lds;
    int chunk;
};
TracerKernel tracer_kernel(const MeshDev &m, int lpc, int nT, bool generic, bool diff, bool bih);
hipError_t launch_tracers(const MeshDev &m, const TracerArgs &a, int lpc, bool generic, hipStream_t s);

// The Laplacian pass of the biharmonic term (tracers.hip), one launch for every field j with kappa4[j] != 0; the others are neither
// read nor written.  Per cell c and level k, from s = 0.0 over the slots of edgesOnCell in slot order with the tendency's skip rules:
//   hE = 0.5 * (ph[k,c] + ph[k,c']);  s += (hE * (x[k,c'] - x[k,c])) * dvdc[c,i];      out[k,c] = (s * invArea[c]) / ph[k,c]
// Two callers: the forward step on (ph_s, pphi) ahead of the tracer launch, the reverse sweep on (ph_s, y) ahead of a reverse stage.
struct TracerLapArgs {
    int nT;
    int64_t stride;               // K * nC: fields of x and of out lie this far apart
    const double *ph;             // the thickness (gathered)
    const double *x;              // the fields (gathered)
    const double *kappa4, *dvdc;  // nT coefficients (only their being zero or not matters here); the plan's (nC, ME) dvEdge / dcEdge
    double *out;
};
// The kernel that serves the pass: k_tracer_patch's layout without the harmonic extras (dvdc takes the place of sdv), so
// tracer_kernel(m, lpc, nT, generic, false, false) decides.  form 1: k_tracer_lap_patch, form 2: k_tracer_lap_cell.
hipError_t launch_tracer_lap(const MeshDev &m, const TracerLapArgs &a, int lpc, bool generic, hipStream_t s);

// ---- reverse mode of the tracer step over a frozen flow (moka_tracer_tape_*; tracer_adjoint.hip): one launch per reverse stage ----
// With r = R(P_rs, y) the transposed tendency of include/moka_hip.h, per tracer and element (hc = ph[k,c], invA = invArea[c]):
//   rs > 0:  v = r / hc;  S = (rs == 3 ? v : S + v);  out = (cb * g + ca * v) * invA      the next gathered field
//   rs == 0: out = hc * (g + S) + r                                                        the adjoint of the current level's tracers
// y is gathered while out is written: the two never alias.
struct TracerAdjArgs {
    int nT, rs;                   // reverse stage 3, 2, 1, 0 = the forward stage whose provisional state is read
    int64_t stride;               // K * nC
    const double *pu, *ph;        // the recorded provisional normalVelocity / layerThickness of forward stage rs (gathered)
    const double *y;              // the adjoint of the stage's tendency times invArea (gathered)
    const double *g;              // X / hn of the step
    double *S;                    // the running sum of v: written by rs 3, read + written by 2 and 1, read by 0
    double *out;
    double cb, ca;                // b[rs - 1], a[rs - 1] (unused by rs 0)
    const double *kappa, *dvdc;   // as in TracerArgs; both nullptr in a sweep whose recorded steps all have every diffusivity zero
    // gradient with respect to the sources (moka_tracer_adjoint_want_source_gradient): nT device pointers, tracer j's (K, nC)
    // accumulator or nullptr where none is wanted; the table is nullptr in a sweep that wants none.  rs > 0 adds tau = cb * g + ca * v,
    // the value `out` multiplies by invA, to the cell's own element: G = G + tau.  rs == 0 does not touch G.
    double *const *G;
    // biharmonic diffusion: the recorded nT coefficients of the step and the base of M = Lap(ph, y) (launch_tracer_lap on the same
    // stream); both nullptr in a sweep whose recorded steps all have every kappa4 zero.  As in TracerArgs: only together with kappa and
    // dvdc, and M of a tracer with kappa4[j] == 0 is never read.
    const double *kappa4, *lapy;
};
// The kernel that serves a reverse stage, for the launcher and for moka_tracer_adjoint_path.  The reverse kernels stage what the forward
// ones do (ph rows and one gathered row set per resident tracer, two with bih, the same records), so the form, the LDS size and the chunk
// are tracer_kernel's: one decision for both directions.
inline TracerKernel tracer_adjoint_kernel(const MeshDev &m, int lpc, int nT, bool generic, bool diff, bool bih)
{
    return tracer_kernel(m, lpc, nT, generic, diff, bih);
}
hipError_t launch_tracer_adjoint(const MeshDev &m, const TracerAdjArgs &a, int lpc, bool generic, hipStream_t s);
// g = X / hn and y = (b4 * g) * invArea, elementwise over nT fields: the head of a reverse step
// G: TracerAdjArgs::G (nullptr: no gradient wanted); the head adds tau_3 = b4 * g, the value y multiplies by invArea
hipError_t launch_tracer_adj_seed(const MeshDev &m, const double *X, const double *hn, double *g, double *y, double b4, int nT,
                                  double *const *G, hipStream_t s);

// ---- gradient of a tracer objective with respect to kappa_j and kappa4_j (moka_tracer_adjoint_want_diffusivity_gradient) ----
// One launch ahead of a reverse stage, over the nF flagged tracers only.  With L_f = Lap(ph_rs, pphi_rs) of flagged tracer f (nF fields
// `stride` apart, launch_tracer_lap on the same stream), y = tau_rs * invArea and M = Lap(ph_rs, y) of the sweep (nT fields `stride`
// apart, indexed by the tracer tracer[f]), per element (k, c):
//   p = ph[k,c] * L_f[k,c];   dk = p * y[k,c];   dk4 = p * M[k,c]
// colsum: lane l of the LPC = lanes_per_column(K) lanes of a cell adds its levels k = l, l + LPC, ... in ascending order onto 0.0, then
// the XOR butterfly of group_sum (offsets LPC/2, ..., 1) adds the lanes; lane 0 holds the sum.  Then, one read and one write per cell:
//   Wk_f[c] = Wk_f[c] + areaCell[c] * colsum(dk);      Wk4_f[c] = Wk4_f[c] - areaCell[c] * colsum(dk4)
// W holds 2 nF device pointers: W[2f] = Wk_f, W[2f+1] = Wk4_f, each nC doubles or nullptr where that derivative is not wanted (then
// its factor -- y, or M -- is not read).  Reads ph, L, y, M; writes W only.
struct TracerKgradArgs {
    int nF;
    int64_t stride;               // K * nC
    const double *ph, *L, *y, *M;
    const int32_t *tracer;        // nF: the tracer index of flagged tracer f
    double *const *W;
};
hipError_t launch_tracer_kgrad(const MeshDev &m, const TracerKgradArgs &a, int lpc, hipStream_t s);

// ---- implicit vertical diffusion of the tracers (moka_set_tracer_vertical_diffusion; tracer_vmix.hip) ----
// One launch over every column and every field j with kv[j] != 0 (the others are neither read nor written): forward behind the stage-4
// tracer launch, x = the new tracers and h the new thickness; reverse at the head of a reversed step, x = X and h the recorded hn.
// Per column c with n = nLev[c] >= 2 and s = dt * kv[j] (the recipe of include/moka_hip.h):
//   forward:  x = x + Solve(Lv(x))        reverse:  x = x + Lv(Solve(x))
// fld != nullptr: the field instances.  A tracer j with fld[j] != nullptr takes s[k] = dt * fld[j][k,c] per interface and its kv[j] is
// not read; one with fld[j] == nullptr takes dt * kv[j] as above (moka_tracer_vertical_field_upload).
struct VmixArgs {
    int nT, nC, K;
    int64_t stride;               // K * nC: the fields of x lie this far apart
    const double *h;              // (K, nC) thickness
    double *x;                    // nT fields, updated in place
    const double *kv;             // nT coefficients kappaV
    double dt;
    const int32_t *nLev;          // (nC) active depth of a cell (Plan.nLev)
    double *scratch;              // 2 * K * nC doubles: g and y of the column form (the tile form keeps them in LDS)
    // the gradient instances of the reverse pass only (moka_tracer_adjoint_want_vertical_gradient; nullptr otherwise):
    const int32_t *gslot;         // nT: the slot f of a flagged tracer in p and D, -1 for an unflagged one
    const double *p;              // nF fields `stride` apart: the recorded phi_new of this step
    double *D;                    // nF fields `stride` apart: the densities, D[k,c] = D[k,c] - e
    // the field instances only (moka_tracer_vertical_field_upload; nullptr otherwise):
    const double *const *fld;     // nullptr, or nT device pointers: (K, nC) diffusivity per interface and cell, nullptr = the scalar kv[j]
};
// The kernel that serves the pass (tracer_vmix.hip holds the LDS formula): form 1 = k_vmix_tile over tiles of `tc` columns with `lds`
// bytes of dynamic LDS, form 2 = k_vmix_column.  generic: the caller asks for form 2 (kernel variant 3).  sets: the column sets a
// resident column takes in LDS, 3 for the forward and the plain reverse pass, 4 for the gradient instances (and the transposed momentum
// pass), 5 for the transposed momentum pass of a step that ran with a viscosity field.
struct VmixKernel {
    int form;
    size_t lds;
    int tc;
};
VmixKernel vmix_kernel(int K, bool generic, int sets = 3);
// a.gslot != nullptr (reverse only): the gradient instances, which also serve the unflagged tracers of the step
hipError_t launch_tracer_vmix(const VmixArgs &a, bool reverse, bool generic, hipStream_t s);

// ---- implicit vertical mixing of momentum (moka_set_vertical_viscosity / moka_surface_stress_upload; momentum_vmix.hip) ----
// One launch over every edge column behind stage 4 of an RK4 step: u = the new normalVelocity, updated in place, h = the new
// layerThickness, from which a column's thickness 0.5 * (h[k,c1] + h[k,c2]) is gathered.  Per edge with n = min(maxLevelEdgeTop[e], K)
// (the recipe of include/moka_hip.h): u = u + Solve(R), R = Lv(u) (+ dt * tau[e] in row 0) (- dt * drag * u[n-1] in row n-1).
// Columns with n >= 2 are computed, columns with n == 1 only when drag != 0 or tau != nullptr.
struct MomVmixArgs {
    int nE, K;
    const int32_t *ehdr;          // (4, nE) c1, c2, -, maxLevelEdgeTop
    double *u;                    // (K, nE), updated in place
    const double *h;              // (K, nC)
    const double *tau;            // (nE) surface stress over rho0 in device edge numbering; nullptr: none (the instances without it)
    double dt, nu, drag;          // drag == 0.0: the instances without it
    double *scratch;              // 2 * K * nE doubles: g and y of the column form (the tile form keeps them in LDS)
    const double *fld;            // (K, nE) viscosity per interface and edge (moka_vertical_viscosity_field_upload): the FIELD instances,
                                  // s[k] = dt * fld[k,e] and nu is not read; nullptr: the scalar instances
    const double *speed;          // (nE) bottom speed sp[e] of u* (launch_momentum_bottom_speed) and the quadratic drag coefficient: with
    double cd;                    // speed != nullptr && cd != 0.0 the QD instances, q = dt * (drag + cd * speed[e]) per lane and the drag
                                  // lines are on whatever drag is; else the instances with the one q = dt * drag
};
// the form vmix_kernel(K, generic, 3) gives the pass: 1 = k_mvmix_tile, 2 = k_mvmix_column
int momentum_vmix_form(int K, bool generic);
hipError_t launch_momentum_vmix(const MomVmixArgs &a, bool generic, hipStream_t s);

// ---- the bottom speed of the quadratic drag (moka_set_quadratic_bottom_drag, moka_bottom_speed; momentum_vmix.hip) ----
// One lane per edge, a launch of its own in front of the pass (which overwrites u tile by tile while an edge's stencil reaches into
// other tiles).  Per edge with n = min(maxLevelEdgeTop[e], K) >= 1 and kb = n - 1 (the recipe of include/moka_hip.h):
//   KE_c = (the sum, from 0.0, over the slots i of edgesOnCell[c] in slot order whose edge e' has min(maxLevelEdgeTop[e'], K) > kb, of
//          (keCoef[e'] * u[kb,e']) * u[kb,e']) * invArea[c];     sp[e] = sqrt(KE_c1 + KE_c2)
// sp[e] = 0.0 for n == 0.  u[kb,e'] of a slot that fails the depth test is not read.
struct MomSpeedArgs {
    int nE, K, ME;
    const int32_t *ehdr;          // (4, nE) c1, c2, -, maxLevelEdgeTop
    const int32_t *eoc, *mltc;    // (ME, nC) edges of a cell, -1 = none; maxLevelEdgeTop of that edge, 0 = none
    const double *keCoef;         // (nE) 0.25 * dcEdge * dvEdge
    const double *invArea;        // (nC)
    const double *u;              // (K, nE)
    double *sp;                   // (nE)
};
hipError_t launch_momentum_bottom_speed(const MomSpeedArgs &a, hipStream_t s);

// ---- the Richardson-number closure of the two vertical passes (moka_set_richardson_mixing; vmix_closure.hip) ----
// Two launches behind stage 4 of an RK4 step and the tracers' stage 4, in front of both vertical passes: k_rich_edge writes the
// viscosity F[k,e] of the interfaces k < min(maxLevelEdgeTop[e], K) - 1, k_rich_cell the diffusivity G[k,c] of the interfaces
// k < nLev[c] - 1 (the recipe of include/moka_hip.h).  LPC lanes run along the contiguous column of an edge / a cell.  Rows at and
// below those bounds are never written; u, h and b at levels no active element reads are never loaded.
struct RichArgs {
    int nE, nC, K, ME;
    const int32_t *ehdr;          // (4, nE) c1, c2, -, maxLevelEdgeTop
    const int32_t *eoc, *mltc;    // (ME, nC) edges of a cell, -1 = none; maxLevelEdgeTop of that edge, 0 = none
    const int32_t *nLev;          // (nC) active depth of a cell (Plan.nLev)
    const double *keCoef;         // (nE) 0.25 * dcEdge * dvEdge
    const double *invArea;        // (nC)
    const double *u, *h, *b;      // (K, nE) normalVelocity, (K, nC) layerThickness, (K, nC) the buoyancy tracer
    double nu0, alpha, nuB, kB, conv;
    double *F, *G;                // (K, nE), (K, nC)
    // the diagnostic instances (moka_richardson_diagnose): Ri of the edge / the cell recipe, (K, nE) / (K, nC).  With either non-null
    // F and G are optional too, and a kernel none of whose outputs is wanted is not launched.  Both nullptr: the step's instances.
    double *riE, *riC;
};
hipError_t launch_richardson(const RichArgs &a, hipStream_t s);

// ---- the transposed pass (moka_forced_tape; momentum_vmix.hip) ----
// At the head of a reversed step, per edge column the forward pass computed with these switches (the recipe of include/moka_hip.h):
// z = Solve_A(xu), xu = h o z in place, hbar to its own (K, nE) array, active levels only; then launch_momentum_vmix_gather adds
// 0.5 * (the sum of hbar over a cell's computed edges, slot order) to xh.  Gtau / Dnu / Dr (nE each; nullptr: not wanted): with any of
// them the gradient instances run, which also solve the columns with n >= 1 the forward pass skipped, for the densities alone.
struct MomVmixAdjArgs {
    int nE, K, nC, ME;
    const int32_t *ehdr;          // (4, nE) c1, c2, -, maxLevelEdgeTop
    const int32_t *eoc;           // (ME, nC) edges of a cell, -1 = none
    double *xu, *xh;              // the adjoint state (K, nE), (K, nC), updated in place
    const double *un, *hn;        // the recorded u_new (K, nE) and h_new (K, nC) of the step
    const double *tau;            // the stress of the step (nullptr: it had none)
    double dt, nu, drag;          // the step's
    int on;                       // 0: the step ran without the pass (gradient instances only: no column writes xu or hbar)
    double *hbar;                 // (K, nE) work array
    double *scratch;              // 2 * K * nE doubles: g and y of the column form
    double *Gtau, *Dnu, *Dr;
    const double *fld;            // the field the step ran with (nullptr: the scalar nu): the FIELD instances, five column sets a tile
    double *DF;                   // (K, nE) density of the field, rows k < n - 1 of a solved column (nullptr: not wanted)
    // the quadratic drag (a quadratic moka_forced_tape): speed != nullptr selects the QD instances -- the recorded sp[e] (nE) of the
    // step, q = dt * (drag + cd * speed[e]) per lane when cd != 0.0 (the forward's bits; the drag lines are then on whatever drag is)
    // and the one q = dt * drag when cd == 0.0.  M (nE; needed when cd != 0.0): the lane's sp-bar / sp for launch_momentum_speed_adjoint;
    // Dcd (nE; nullptr: not wanted): the density of Cd.  speed == nullptr: the instances without any of it.
    const double *speed;
    double cd;
    double *M, *Dcd;
};
int momentum_vmix_adjoint_form(int K, bool generic, bool field);            // vmix_kernel(K, generic, field ? 5 : 4).form
hipError_t launch_momentum_vmix_adjoint(const MomVmixAdjArgs &a, bool generic, hipStream_t s);
hipError_t launch_momentum_vmix_gather(const MomVmixAdjArgs &a, hipStream_t s);

// ---- the transpose of the bottom-speed stencil (a quadratic moka_forced_tape; momentum_vmix.hip: k_mvadj_bottom_speed) ----
// Behind the transposed pass of a step with Cd != 0, one lane per edge e' with n' = min(maxLevelEdgeTop[e'], K) >= 1 (the recipe of
// include/moka_hip.h): for every level k that is the bottom level kb_e = n_e - 1 < n' of an edge e in a slot of e''s two cells,
//   a_j = (the sum, from 0.0, over the slots of cell c_j in slot order with kb_e == k, of M[e]);   g = a_1 * invArea[c1] + a_2 * invArea[c2]
//   xu[k,e'] = xu[k,e'] + (keCoef[e'] * us[k,e']) * g
// Rows k >= n' of xu and us are never touched; M and us of a slot that fails the test are not read.
struct MomSpeedAdjArgs {
    int nE, K, ME;
    const int32_t *ehdr;          // (4, nE) c1, c2, -, maxLevelEdgeTop
    const int32_t *eoc, *mltc;    // (ME, nC) edges of a cell, -1 = none; maxLevelEdgeTop of that edge, 0 = none
    const double *keCoef;         // (nE)
    const double *invArea;        // (nC)
    const double *M;              // (nE) sp-bar[e] / sp[e] of the transposed pass, 0.0 where sp[e] == 0 and where n_e == 0
    const double *us;             // (K, nE) the recorded u* of the step
    double *xu;                   // (K, nE) the adjoint of u*, updated in place
};
hipError_t launch_momentum_speed_adjoint(const MomSpeedAdjArgs &a, hipStream_t s);

// ---- reverse mode of one Forward-Euler step: gather form, the oracle's summation order ----
struct AdjMesh {
    int32_t nC, nE, K, ME, W;          // W = width of the transposed Coriolis lists
    const int32_t *eoc;                // (ME, nC) edges of a cell, -1 = none
    const int32_t *csgn;               // (ME, nC) edgeSignOnCell
    const int32_t *ehdr;               // (4, nE) c1, c2, -, maxLevelEdgeTop
    const int32_t *teoe;               // (W, nE) source edges s with edgesOnEdge[i,s] == e, sorted by (original s, i); -1 = none
    const double *tw;                  // (W, nE) weightsOnEdge[i,s]
    const double *sd;                  // (2, nE) dvEdge*edgeSign*invArea for c1, c2
    const double *fEdge, *gInvDc;      // (nE)
    const int32_t *efull;              // (nE) 1: all W sources exist and the edge and every source are active on all levels
    // the entities a launch of the chunk kernels (k_adj_edge3 / k_adj_cell3) covers: edges [eBegin, eBegin + eCount), cells
    // [cBegin, cBegin + cCount) -- everything by default, one cell class of a partitioned mesh in moka_adjoint_rk4_stage_part
    int32_t eBegin, eCount, cBegin, cCount;
};
struct AdjArgs {
    double dt;
    int stale;                         // MOKA_FE_STALE_HEDGE
    int tt;                            // 1: transpose of the tendency evaluation only (RK4 stages); 0: of a Forward-Euler step
    const double *u, *hEuse;           // forward values of the step (tape)
    const double *h;                   // tt: layerThickness of the stage (layerThicknessEdge is recomputed from it)
    const double *lamU1, *lamH1, *lamS1, *lamE1;
    double *lamU0, *lamH0, *lamS0;
    double *Enew, *csum;               // u*Fbar (K, nE); ksum_k dt*lamU1 (nE)
    // RK4 reverse sweep (tt = 1): the element-wise steps around T'(P)^T fused into the two kernels.  With accOut set the
    // result Pb = T'(P)^T k is not stored (lamU0 / lamH0 unused); instead, row by row,
    //   accOut = (accIn ? accIn : x) + Pb          X + Pb4, then (...) + Pb3 ...   (time_integration.jl:61-148 transposed)
    //   kNext  = cbNext * x + caNext * Pb          the next stage's k-bar (nullptr after the last stage)
    const double *xU, *xH, *accInU, *accInH;
    double *accOutU, *accOutH, *kNextU, *kNextH;
    double cbNext, caNext;
    // tt only.  lamScale: the k-bar actually used is lamScale * lamU1 / lamH1 (stage 4 reads X itself: kb4 = b4 * X is never
    // stored).  fuseE: u*Fbar is not stored by the edge kernel; the cell kernel recomputes it from the stage's u rows and the
    // k-bar rows of the edge's two cells (same products, same order) -- set only when adj_fused_available() says so.
    double lamScale;
    int fuseE;
};
// both fused forms (lamScale != 1, fuseE) need the 16-byte-lane chunk kernels: even K <= 64, hexagon-width lists
bool adj_fused_available(const AdjMesh &m, int lpc);
hipError_t launch_adj_edge(const AdjMesh &m, const AdjArgs &a, int lpc, hipStream_t s);
hipError_t launch_adj_cell(const AdjMesh &m, const AdjArgs &a, int lpc, hipStream_t s);
hipError_t launch_scale_copy(double *dst, const double *src, double f, int64_t n, hipStream_t s);   // dst = f*src
hipError_t launch_axpby(double *dst, double a, const double *x, double b, const double *y, int64_t n, hipStream_t s);
hipError_t launch_add(double *dst, const double *x, const double *y, int64_t n, hipStream_t s);       // dst = x + y
hipError_t launch_bcast_rows(double *dst, const double *src, double f, int64_t n, int K, hipStream_t s);   // dst[c][k] = f*src[c]

}  // namespace moka
