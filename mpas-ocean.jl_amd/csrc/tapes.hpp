// tapes.hpp -- the three tape handles (moka_tracer_tape, moka_tape, moka_forced_tape) and the helpers their files share.  Only the
// api*.hip files include this: the forced tape embeds a moka_tape and reads inner->kind, step_rk4 records on the tracer tape.
#pragma once
#include "state.hpp"

// Tape of the tracer reverse mode (moka_tracer_tape_*, api_tracer_tape.hip).  Per recorded step: the four provisional states the stage launches
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
    mk::DeviceAllocs mem;
    bool counted = false;                            // st->attached includes this tape
};

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
    mk::DeviceAllocs mem;
    bool counted = false;                            // st->attached includes this tape
    bool forced = false;                             // the tape a moka_forced_tape embeds: counted in st->forcedTapes
};

struct ForcedStep {
    bool rec, on, stress;        // u_new / h_new were recorded; the pass ran; with the stress
    double nu, drag;             // nu: what the pass took (0.0 under a field)
    int32_t vf;                  // the copy in moka_forced_tape.vfCopies of the field the step ran with, -1: the scalar nu
    double cd = 0.0;             // a quadratic tape: the Cd the step ran with (its u* sits in usRec when it is nonzero) ...
    bool sp = false;             // ... and whether the step's slot of spRec holds its bottom speed
};

struct moka_forced_tape {
    moka_state *st = nullptr;
    moka_tape *inner = nullptr;
    int64_t capacity = 0;
    double *unRec = nullptr, *hnRec = nullptr;       // capacity x (K, nE) / (K, nC): the new level of every step that recorded it
    double *hbar = nullptr, *scratch = nullptr;      // (K, nE); 2 x (K, nE): the column form's g and y.  All four come with the first step that records.
    double *dens[3] = {nullptr, nullptr, nullptr};   // G_tau, D_nu, D_r (nE each), allocated by the flag
    // the viscosity field: DF (K, nE), allocated by its flag; one (K, nE) copy per field the recorded steps ran with, taken when the
    // state's generation differs from that of the newest copy, released when a sweep has emptied the tape and at destroy
    double *densF = nullptr;
    bool wantF = false;
    std::vector<double *> vfCopies;
    uint64_t vfGen = 0;
    int want = 0;                                    // MOKA_FORCED_GRAD_* bits
    // the quadratic drag (moka_forced_tape_create_quadratic): spRec capacity x nE, the sp of every step with Cd != 0 or the flag;
    // usRec capacity x (K, nE), u* of every step with Cd != 0, and M (nE), the transposed pass's sp-bar / sp -- each allocated by
    // the first step that needs it; densCd (nE), the density of Cd, by its flag.  A plain tape never touches any of them.
    bool quadratic = false, wantCd = false;
    bool countedPlain = false;                       // st->forcedPlainTapes includes this tape
    double *spRec = nullptr, *usRec = nullptr, *M = nullptr, *densCd = nullptr;
    std::vector<ForcedStep> steps;
    int path = 0;                                    // moka_forced_tape_vmix_path
    mk::DeviceAllocs mem;
};

namespace mk {

// api_tape.hip.  forced: the tape inside a moka_forced_tape; tape_destroy returns false when the state had gone before the tape
int tape_create(moka_state *st, int64_t capacity_steps, moka_tape **out, bool forced);
bool tape_destroy(moka_tape *t);
int rk4_reverse_stage(moka_tape *t, int sg, int part = -1);

}  // namespace mk
