/* moka_hip.h -- C ABI of libmoka_hip.so: the MI355X-native (gfx950, HIP) implementation of the
 * MOKA.jl (jlk9/MPAS-Ocean.jl) shallow-water hot path: TRiSK tendency operators of src/ocn and
 * the Forward-Euler / RK4 step loop of src/forward.
 *
 * This is the drop-in boundary.  The reference has no FFI; its seam is Julia dispatch on the
 * `backend` keyword + `Adapt.adapt_structure` (src/Architectures.jl:12, MPASMesh.jl:26,
 * HorzMesh.jl:53,357,373,388, VertMesh.jl:119,124, PrognosticVars.jl:108, DiagnosticVars.jl:101).
 * A Julia shim (mpas-ocean.jl_amd/julia/MokaHIP.jl) overloads those methods for a `MokaHIP`
 * backend tag and `ccall`s the functions below; INTEGRATION.md shows the binding.  Each entry
 * point cites the reference method it replaces.
 *
 * Conventions
 *   - Plain C types only.  All host arrays are exactly what Julia holds in memory: Float64 /
 *     Int32, column-major, 1-based connectivity (0 = "no neighbour" in edgesOnEdge), the slot
 *     index fastest for connectivity ((maxEdges,nCells)...), the level index fastest for fields
 *     ((nVertLevels,n)).
 *   - Host pointers are borrowed for the duration of a call only.  The library owns all device
 *     memory, its reordered copies of the mesh and the permutations; uploads/downloads present
 *     the caller's original numbering.
 *   - Every function returns 0 (MOKA_OK) or a negative moka_status; the message is available from
 *     moka_last_error().  Nothing aborts, nothing prints.
 *   - One context = one device = one owning host thread (not thread-safe).
 *   - Operator entry points are synchronous on return (the reference ends every operator with
 *     KA.synchronize: Operators.jl:72,119,176,198).  moka_step_ / moka_run are asynchronous on the
 *     context's compute stream; download, sum_sq, timer_stop and sync are completion points.
 *   - There is no CPU fallback: without a usable HIP device moka_ctx_create fails.
 */
#ifndef MOKA_HIP_H
#define MOKA_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct moka_ctx   moka_ctx;
typedef struct moka_plan  moka_plan;   /* host-side reordered mesh (no GPU needed) */
typedef struct moka_mesh  moka_mesh;   /* plan resident on a device                */
typedef struct moka_state moka_state;  /* Prog + Diag + Tend on a device           */

typedef enum {
    MOKA_OK = 0,
    MOKA_ERR_ARG = -1,       /* bad argument / inconsistent mesh (Julia: error("..."))  */
    MOKA_ERR_HIP = -2,       /* a HIP runtime call failed (message has hipGetErrorString) */
    MOKA_ERR_NO_DEVICE = -3, /* no usable gfx950 device: there is no CPU fallback         */
    MOKA_ERR_ALLOC = -4,
    MOKA_ERR_UNSUPPORTED = -5,
    MOKA_ERR_COMM = -6
} moka_status;

/* cell ordering applied at mesh upload (north_star: "re-laid out SoA and RCM-reordered") */
typedef enum {
    MOKA_ORDER_DEFAULT = 0,  /* RCB patches when coordinates are given, else RCM */
    MOKA_ORDER_NONE = 1,     /* keep the caller's numbering                      */
    MOKA_ORDER_RCM = 2,      /* reverse Cuthill-McKee on the cell graph          */
    MOKA_ORDER_RCB = 3       /* recursive coordinate bisection into compact patches */
} moka_ordering;

/* Mesh as the reference holds it: Edges (HorzMesh.jl:64-95), PrimaryCells (:102-132),
 * DualCells (:135-162), VerticalMesh (VertMesh.jl:3-26).  Pointers marked (opt) may be NULL. */
typedef struct moka_mesh_desc {
    int32_t nCells, nEdges, nVertices;
    int32_t maxEdges, maxEdges2, vertexDegree;
    int32_t nVertLevels;
    int32_t edgeSignOnVertexLD;      /* leading dim of edgeSignOnVertex (= maxEdges, HorzMesh.jl:234); 0 -> vertexDegree */
    /* PrimaryCells */
    const double  *xCell, *yCell, *zCell;            /* (opt) only used to order cells          */
    const int32_t *nEdgesOnCell;                     /* (nCells)                                */
    const int32_t *edgesOnCell;                      /* (maxEdges, nCells)                      */
    const int32_t *edgeSignOnCell;                   /* (maxEdges, nCells)  signIndexField! :292 */
    const double  *areaCell;                         /* (nCells)                                */
    /* Edges */
    const int32_t *cellsOnEdge;                      /* (2, nEdges)                             */
    const int32_t *verticesOnEdge;                   /* (opt) (2, nEdges)                       */
    const int32_t *nEdgesOnEdge;                     /* (nEdges)                                */
    const int32_t *edgesOnEdge;                      /* (maxEdges2, nEdges), 0 = none           */
    const double  *weightsOnEdge;                    /* (maxEdges2, nEdges)                     */
    const double  *dvEdge, *dcEdge, *fEdge;          /* (nEdges)                                */
    /* DualCells */
    const int32_t *edgesOnVertex;                    /* (vertexDegree, nVertices)               */
    const int32_t *cellsOnVertex;                    /* (opt) (vertexDegree, nVertices)         */
    const int32_t *edgeSignOnVertex;                 /* (edgeSignOnVertexLD, nVertices) :313    */
    const double  *areaTriangle;                     /* (nVertices)                             */
    /* VerticalMesh */
    const int32_t *maxLevelEdgeTop;                  /* (opt) (nEdges); NULL -> all ones (VertMesh.jl:32).  Skipped means
                                                      * never read: normalVelocity, tracers and adjoint seeds at levels no active
                                                      * element reads may hold anything (NaN, infinities: fill values below the
                                                      * sea floor) and never reach an active element (tests/test_gpu_poison.py);
                                                      * layerThickness must be finite on every level (ssh sums all of them) */
    const double  *restingThicknessSum;              /* (nCells) (VertMesh.jl:73,100)           */
    /* layout controls */
    int32_t ordering;                                /* moka_ordering                            */
    int32_t patch_cells;                             /* cells per patch (0 = library default)    */
    /* (opt) (nCells) small non-negative class per cell; cells are ordered by class first, then by `ordering`
     * inside a class.  The multi-GPU layer passes 0 = owned & needed by another rank, 1 = owned interior,
     * 2 = halo, so that patch ranges [0,pb) / [pb,po) / [po,nPatches) are boundary / interior / halo. */
    const int32_t *cellClass;
    /* bytes per real of the prognostic state this mesh will carry: 0 or 8 = Float64 (the reference,
     * PrognosticVars.jl:91-93); 4 = fp32 STORAGE of every array of PrognosticVars (every time level and RK provisional
     * state), DiagnosticVars and TendencyVars, with fp64 arithmetic: an element is accumulated in fp64 and rounded once
     * when it is stored (BASELINE config 5; not a reference feature).
     * It fixes the byte offsets baked into the gather records, so a mesh serves states of one storage type. */
    int32_t stateBytes;
    /* (opt) only for the optional nonlinear terms (moka_set_nonlinear): MPAS mesh files carry both, the reference
     * reads neither.  With them verticesOnEdge and cellsOnVertex are required too. */
    const double *kiteAreasOnVertex;                 /* (vertexDegree, nVertices) */
    const double *fVertex;                           /* (nVertices)               */
} moka_mesh_desc;

typedef struct moka_mesh_info {
    int32_t nCells, nEdges, nVertices, nVertLevels;
    int32_t ordering, patch_cells, nPatches;
    int32_t maxEdgesUsed, maxEdges2Used;             /* record widths after compaction           */
    int32_t lanesPerColumn;                          /* wavefront lanes that span one k-column   */
    int64_t meshBytesDevice;                         /* reordered mesh resident in HBM           */
    int64_t cellBandwidth;                           /* max |new(c1)-new(c2)| over edges         */
    int32_t maxPatchRows;                            /* most u-rows (own + halo edges) any patch stages in LDS */
    int32_t ldsBytesPerBlock;                        /* dynamic LDS of the LDS-tiled stage kernel (0: not applicable) */
    int32_t maxPatchCells, maxPatchEdges;            /* largest own cell / edge range of any patch (sizes the record staging) */
} moka_mesh_info;

/* entity kinds for permutations */
enum { MOKA_CELL = 0, MOKA_EDGE = 1, MOKA_VERTEX = 2 };

/* state fields (PrognosticVars.jl:6-57, DiagnosticVars.jl:6-73, TendencyVars.jl:7-49) */
typedef enum {
    MOKA_F_SSH = 0,                  /* (nCells)            time levels 0,1 */
    MOKA_F_NORMAL_VELOCITY = 1,      /* (K, nEdges)         time levels 0,1 */
    MOKA_F_LAYER_THICKNESS = 2,      /* (K, nCells)         time levels 0,1 */
    MOKA_F_LAYER_THICKNESS_EDGE = 3, /* (K, nEdges)                         */
    MOKA_F_THICKNESS_FLUX = 4,       /* (K, nEdges)                         */
    MOKA_F_VELOCITY_DIV_CELL = 5,    /* (K, nCells)                         */
    MOKA_F_RELATIVE_VORTICITY = 6,   /* (K, nVertices)                      */
    MOKA_F_TEND_NORMAL_VELOCITY = 7, /* (K, nEdges)                         */
    MOKA_F_TEND_LAYER_THICKNESS = 8  /* (K, nCells)                         */
} moka_field;

/* Forward-Euler order-of-evaluation switches; all set = the live reference step */
#define MOKA_FE_STALE_HEDGE      1  /* flux uses previous step's layerThicknessEdge (DiagnosticVars.jl:113-116) */
#define MOKA_FE_ACCUM_VORT       2  /* relativeVorticity accumulates (Operators.jl:135,142)                      */
#define MOKA_FE_LEVEL1_ONLY      4  /* "[1,j]" kernels touch level 1 only (Operators.jl:207,228 ...)             */
#define MOKA_FE_REFERENCE_COMPAT 7

typedef enum { MOKA_FORWARD_EULER = 0, MOKA_RUNGE_KUTTA_4 = 1 } moka_integrator;

/* ---- library / context ---------------------------------------------------------------- */
const char *moka_version(void);
/* replaces the `backend = CUDABackend()` choice, src/driver/mpas_ocean.jl:28 */
int  moka_ctx_create(int device, moka_ctx **out);
void moka_ctx_destroy(moka_ctx *ctx);
const char *moka_last_error(const moka_ctx *ctx);   /* ctx may be NULL: last error of the calling thread */
int  moka_sync(moka_ctx *ctx);                      /* KA.synchronize(backend) */
/* HIP-event timer on the compute stream (used by bench.py for the roofline figure) */
int  moka_timer_start(moka_ctx *ctx);
int  moka_timer_stop(moka_ctx *ctx, float *elapsed_ms);

/* ---- mesh ------------------------------------------------------------------------------ */
/* Host-only: validate, convert to 0-based, order cells (RCB patches / RCM), renumber edges and
 * vertices by first-touching cell, build per-entity records.  Needs no GPU. */
int  moka_plan_create(const moka_mesh_desc *desc, moka_plan **out);
void moka_plan_destroy(moka_plan *plan);
int  moka_plan_info(const moka_plan *plan, moka_mesh_info *info);
/* new_to_old[new] = caller's 0-based index; kind = MOKA_CELL / MOKA_EDGE / MOKA_VERTEX */
int  moka_plan_permutation(const moka_plan *plan, int kind, int32_t *new_to_old);
/* first cell / edge / vertex of every patch, nPatches+1 entries each */
int  moka_plan_patch_ranges(const moka_plan *plan, int32_t *cellStart, int32_t *edgeStart, int32_t *vertexStart);
/* patch / cell / edge range of every cell class (see moka_mesh_class_ranges) */
int  moka_plan_class_ranges(const moka_plan *plan, int32_t capacity, int32_t *nClasses, int32_t *patchStart,
                            int32_t *cellStart, int32_t *edgeStart);

/* Read-only view of one of the plan's per-entity record arrays (device layout, new numbering):
 * lets host tests check the reordered mesh without a GPU.  `data` stays valid until plan destroy. */
enum {
    MOKA_PA_EOC = 0, MOKA_PA_COC, MOKA_PA_MLTC, MOKA_PA_SDV, MOKA_PA_INVAREA, MOKA_PA_AREACELL, MOKA_PA_RSUM,
    MOKA_PA_EHDR, MOKA_PA_EOE, MOKA_PA_WOE, MOKA_PA_GINVDC, MOKA_PA_DCEDGE, MOKA_PA_DVEDGE, MOKA_PA_FEDGE,
    MOKA_PA_EOV, MOKA_PA_CV, MOKA_PA_HALO_START, MOKA_PA_HALO_EDGE, MOKA_PA_LEOC, MOKA_PA_LEOE,
    MOKA_PA_CREC, MOKA_PA_EREC, MOKA_PA_FEOE, MOKA_PA_PVSTART, MOKA_PA_PVLIST, MOKA_PA_LVOE,
    MOKA_PA_NLEV     /* (nCells) int32: active depth of a cell, see moka_set_tracer_vertical_diffusion */
};
int  moka_plan_array(const moka_plan *plan, int which, const void **data, int64_t *count);

/* replaces Adapt.adapt_structure(backend, ::Mesh) (MPASMesh.jl:26; HorzMesh.jl:354) */
int  moka_mesh_create(moka_ctx *ctx, const moka_mesh_desc *desc, moka_mesh **out);
void moka_mesh_destroy(moka_mesh *mesh);
int  moka_mesh_info_get(const moka_mesh *mesh, moka_mesh_info *info);

/* ---- operators on host arrays (synchronous) -------------------------------------------- */
/* GradientOnEdge!(grad, h, Mesh)            src/ocn/Operators.jl:102-120 */
int moka_gradient_on_edge(moka_mesh *mesh, const double *scalarCell, double *gradEdge);
/* DivergenceOnCell!(div, V, temp, Mesh)     src/ocn/Operators.jl:46-74; temp (opt) receives V*dvEdge */
int moka_divergence_on_cell(moka_mesh *mesh, const double *vecEdge, double *tempEdge, double *divCell);
/* CurlOnVertex!(curl, V, Mesh)              src/ocn/Operators.jl:151-177; ACCUMULATES into curlVertex */
int moka_curl_on_vertex(moka_mesh *mesh, const double *vecEdge, double *curlVertex);
/* interpolateCell2Edge!(e, c, Mesh)         src/ocn/Operators.jl:179-222; nlev = 1 is the reference (level 1 only) */
int moka_interpolate_cell2edge(moka_mesh *mesh, const double *cellValue, double *edgeValue, int nlev);

/* Reverse (vjp) and forward (jvp) mode of the three operators -- what the reference obtains from Enzyme in
 * test/enzyme/test_Enzyme_Operators.jl:42-131 (gradient) and :137-225 (divergence); the rules a maintainer registers are in
 * julia/MokaHIPEnzymeExt.jl.  Host arrays of the primal's shapes.  Shadow conventions are Enzyme's for in-place kernels with
 * Duplicated arguments: vjp ACCUMULATES into the shadow of the input and ZEROES the shadow of an output the primal overwrites
 * (grad; div and temp); the shadow of the curl output, which the primal accumulates into, is left as it is.  The operators
 * are linear, so jvp is the operator applied to the tangent of the input (curl: accumulated onto the tangent of the output).
 * Transposes are gathers with a fixed summation order (oracle twins: oracle_*_vjp, bit-identical). */
int moka_gradient_on_edge_vjp(moka_mesh *mesh, double *dGradEdge /* in, zeroed */, double *dScalarCell /* += */);
int moka_gradient_on_edge_jvp(moka_mesh *mesh, const double *dScalarCell, double *dGradEdge);
int moka_divergence_on_cell_vjp(moka_mesh *mesh, double *dDivCell /* in, zeroed */, double *dVecEdge /* += */,
                                double *dTempEdge /* (opt) in, zeroed */);
int moka_divergence_on_cell_jvp(moka_mesh *mesh, const double *dVecEdge, double *dTempEdge /* (opt) */, double *dDivCell);
int moka_curl_on_vertex_vjp(moka_mesh *mesh, const double *dCurlVertex, double *dVecEdge /* += */);
int moka_curl_on_vertex_jvp(moka_mesh *mesh, const double *dVecEdge, double *dCurlVertex /* += */);

/* ---- state ----------------------------------------------------------------------------- */
/* PrognosticVars/DiagnosticVars/TendencyVars constructors with KA.zeros on the backend
 * (PrognosticVars.jl:59-106, DiagnosticVars.jl:75-99, TendencyVars.jl:51-67); nTimeLevels = 2 */
/* A mesh created with stateBytes = 4 yields an fp32-STORAGE state: host arrays stay double (upload rounds to fp32,
 * download widens); moka_tendencies / moka_step_rk4 / moka_step_fe / moka_run / moka_sum_sq / the halo API work on it.
 * moka_step_fe steps all levels of a whole mesh (no MOKA_FE_LEVEL1_ONLY; on a partitioned mesh: moka_fe_dist_step).  DiagnosticVars come out of
 * Forward-Euler steps only: after an RK4 step they are unavailable (MOKA_ERR_UNSUPPORTED on download, moka_sum_sq and upload of a
 * DiagnosticVars field; the state is unchanged), and the next
 * Forward-Euler step must carry none over (flags 0).  The piecewise calls (moka_diagnostic_compute, moka_compute_*_tendency,
 * moka_advance_time_levels with level-1-only flags) stay Float64-only.  Needs nVertLevels % 4 == 0 and <= 128. */
int  moka_state_create(moka_ctx *ctx, moka_mesh *mesh, moka_state **out);
void moka_state_destroy(moka_state *st);
/* Adapt.adapt(backend, array) / Adapt.adapt_structure(KA.CPU(), x) (OutPut.jl:122-124).
 * time_level: 0 = previous, 1 = current (reference indices 1 and end); ignored for Diag/Tend. */
int  moka_state_upload(moka_state *st, int field, int time_level, const double *host);
int  moka_state_download(moka_state *st, int field, int time_level, double *host);

/* Selected rows of a field (caller's 0-based ids; any order, repeats allowed) into host (nVertLevels, nRows) -- (1, nRows) for
 * ssh -- widened to double: what a row-sampled check of a full-size state needs without moving the whole field across PCIe.
 * time_level 0 / 1 as moka_state_download; 2 / 3 = the two RK4 provisional states as the last stage launches left them
 * (inspection only: prognostic fields; they exist after the first RK4 step). */
int  moka_state_download_rows(moka_state *st, int field, int time_level, int64_t nRows, const int32_t *rows, double *host);

/* Device address of a prognostic array (inspection; time_level as above, 0 when the array does not exist yet). */
int  moka_state_array_address(moka_state *st, int field, int time_level, uint64_t *address);

/* Placement of the state's arrays in device memory.  Where the allocator puts the four buffer sets an RK4 step streams through
 * (current level, previous level = New accumulator, two provisional states) decides 5-14 % of every stage launch (DESIGN.md
 * section 5): a stable property of the memory behind an array, not visible in its address.  The reference's driver only ever
 * calls ocn_init and the step (src/driver/mpas_ocean.jl:28-39), so the choice is made here, behind the boundary: the four
 * launches of an RK4 step are timed with the library's own events (dt = 0), then up to max_tries times ONE array is given a
 * second allocation while the first is still alive, the launches that array takes part in are timed again, and the faster
 * allocation is kept (the loser is held back, within a quarter of the free memory, so that it is not handed out again; all
 * are released on return).  Peak extra memory: the previous level (saved / restored) + one candidate + the held-back losers.
 * The state's observable contents are unchanged (every array of Prog / Diag / Tend, both time levels, what is lazily
 * pending); only the provisional RK states, which every RK4 step overwrites before reading, are clobbered.
 * *ms_before / *ms_after (opt): sum of the four stage launches' median times before / with the kept layout.
 * max_tries <= 0 measures only.  Stops early after 12 consecutive trials without a gain (every array tried once: normalVelocity,
 * layerThickness and ssh of the four buffer sets).
 * MOKA_ERR_UNSUPPORTED once a halo or a tape of the state exists (they export / hold addresses): call it right after
 * moka_state_create (+ uploads), which is what julia/MokaHIP.jl, moka_hip.shim and moka_hip.parallel do. */
int  moka_state_optimize_placement(moka_state *st, int max_tries, double *ms_before, double *ms_after);
/* What the last moka_state_optimize_placement tried: field = 3 * set + (0 normalVelocity, 1 layerThickness, 2 ssh), set 0 = current
 * level, 1 = previous level, 2 / 3 = RK provisional states; ms_old / ms_new = summed median times of the stage launches the
 * array takes part in with the old / the candidate allocation; kept = 1 when the candidate replaced the old one.
 * *n = number of trials; out receives min(*n, capacity) of them (may be NULL). */
typedef struct { int32_t field; double ms_old, ms_new; int32_t kept; } moka_placement_trial;
int  moka_state_placement_log(const moka_state *st, int32_t capacity, moka_placement_trial *out, int32_t *n);
/* stage launches the last search issued (bookkeeping for whoever lines a kernel trace up with a timed region) */
int64_t moka_state_placement_launches(const moka_state *st);

/* advanceTimeLevels!(Prog)                  src/forward/time_integration.jl:10-40 */
int moka_advance_time_levels(moka_state *st, int flags);
/* diagnostic_compute!(Mesh, Diag, Prog)     src/ocn/DiagnosticVars.jl:108-117 (flags: MOKA_FE_*) */
int moka_diagnostic_compute(moka_state *st, int flags);
/* computeNormalVelocityTendency!            src/ocn/Tendencies/normalVelocity/normalVelocity.jl:21-53 */
int moka_compute_normal_velocity_tendency(moka_state *st, int flags);
/* computeLayerThicknessTendency!            src/ocn/Tendencies/layerThickness/layerThickness.jl:14-28 */
int moka_compute_layer_thickness_tendency(moka_state *st, int flags);
/* Fused tendency evaluation (u,h) -> (tendU,tendH) with consistent diagnostics:
 * the kernel the roofline figure is quoted on. */
int moka_tendencies(moka_state *st);
/* ocn_timestep(timestep, Prog, Diag, Tend, S, ForwardEuler)   time_integration.jl:150-193 */
int moka_step_fe(moka_state *st, double dt, int flags);
/* ocn_timestep(Prog, Diag, Tend, S, RungeKutta4)              time_integration.jl:61-148 (spec) */
int moka_step_rk4(moka_state *st, double dt);
/* the body of ocn_run_loop                   src/forward/run_loop.jl:8-22 : nsteps x ocn_timestep */
int moka_run(moka_state *st, int integrator, double dt, int64_t nsteps, int flags);
/* sumArray                                   src/forward/run_loop.jl:39-51 : sum_j a[j]^2 */
int moka_sum_sq(moka_state *st, int field, int time_level, double *out);

/* ---- multi-GPU (one process per GPU; the reference has no distributed code) -----------------
 * The mesh handed to moka_mesh_create is the rank's LOCAL mesh: owned cells + a one-cell-deep halo, with
 * cellClass = 0 (owned, needed by another rank) / 1 (owned interior) / 2 + i (halo cells owned by the rank's i-th
 * neighbour; plain 2 for all of them also works, but then only the buffered transport is available).  The plan orders
 * cells class-major and never lets a patch straddle a class: moka_mesh_class_ranges reports the patch / cell / edge range
 * of every class, moka_mesh_permutation the library's numbering (new -> caller's), which is the order in which a rank
 * has to list the halo cells / edges it receives for the direct transport.
 *
 * Two transports, per neighbour and stage the rows [layerThickness | ssh | normalVelocity] of the listed cells / edges:
 *   buffered: moka_halo_pack -> one contiguous device buffer -> the host layer moves it (torch.distributed on RCCL over
 *     xGMI in bench.py; gloo in the tests; MPI.jl from Julia) -> moka_halo_unpack.  Buffer layout, per neighbour i:
 *     [K reals of layerThickness for cells[off[i]..off[i+1])] [ssh of the same cells] [K reals of normalVelocity for
 *      edges[off[i]..off[i+1])]   (reals = double, or float for an fp32-storage state; sizes in elements)
 *   direct: after moka_halo_export / moka_halo_connect with every neighbour, moka_halo_push_begin stores the rows straight
 *     into the neighbours' fields (peer-mapped memory over xGMI: hipIpcOpenMemHandle between processes, plain pointers
 *     inside one process), moka_halo_push_signal / _wait complete the exchange through flag words in host (shared)
 *     memory.  No send buffer, no unpack, no collective library, no kernel that spins on the device.
 * Entity ids are in the caller's (local mesh) numbering; the *Off arrays have nNeighbors+1 entries. */
typedef struct moka_halo moka_halo;
int  moka_ctx_streams(moka_ctx *ctx, void **compute_stream, void **comm_stream);   /* hipStream_t handles */
int  moka_mesh_permutation(const moka_mesh *mesh, int kind, int32_t *new_to_old);
/* class k covers patches [patchStart[k], patchStart[k+1]), cells [cellStart[k], ...), edges [edgeStart[k], ...) of the
 * library's numbering; the arrays take min(nClasses + 1, capacity) entries (any of them may be NULL) */
int  moka_mesh_class_ranges(const moka_mesh *mesh, int32_t capacity, int32_t *nClasses, int32_t *patchStart,
                            int32_t *cellStart, int32_t *edgeStart);
/* nPatchesBoundary / nPatchesOwned: patchStart[1] / patchStart[2] of moka_mesh_class_ranges */
int  moka_halo_create(moka_state *st, int32_t nNeighbors, const int32_t *sendCells, const int64_t *sendCellOff,
                      const int32_t *sendEdges, const int64_t *sendEdgeOff, const int32_t *recvCells,
                      const int64_t *recvCellOff, const int32_t *recvEdges, const int64_t *recvEdgeOff,
                      int32_t nPatchesBoundary, int32_t nPatchesOwned, moka_halo **out);
void moka_halo_destroy(moka_halo *h);
int  moka_halo_buffer_elems(const moka_halo *h, int64_t *sendElems, int64_t *recvElems);
/* what: 0 = current time level, 1..4 = output of RK4 stage `what`, 5 = the new level of a distributed Forward-Euler step
 * (before moka_fe_dist_end rotates the levels).  pack runs on the comm stream after the work already queued on the compute
 * stream; unpack makes later compute-stream work wait for it. */
int  moka_halo_pack(moka_halo *h, int what, void *sendbuf_device);
int  moka_halo_unpack(moka_halo *h, int what, const void *recvbuf_device);

/* direct transport.  What a rank tells neighbour `nbr` so that the neighbour can push to it (moka_halo_export), to be
 * carried to that neighbour by the host layer (any byte transport: it is plain data) and given to moka_halo_connect
 * there.  shared = 1: the two ranks are different processes (IPC handles + a POSIX shared-memory flag block);
 * shared = 0: same process (raw pointers; several devices are mapped with hipDeviceEnablePeerAccess). */
typedef struct {
    unsigned char ipc[15][64];   /* hipIpcMemHandle_t of the five buffer sets (two time levels, two RK provisional states, the
                                    Forward-Euler spare level) x (normalVelocity, layerThickness, ssh) */
    uint64_t ptr[15];            /* the same allocations as raw device pointers */
    uint64_t flagPtr;            /* the rank's flag block as a raw host pointer */
    char     shmName[64];        /* ... and as a POSIX shared-memory object (shared = 1) */
    int32_t  dstCell, dstEdge;   /* first cell / edge (library numbering) of the ranges the neighbour's rows go to */
    int32_t  nCells, nEdges;     /* their lengths: must equal what the neighbour lists as its send cells / edges */
    int32_t  slot;               /* the neighbour's slot in the flag block */
    int32_t  nNeighbors, pid, device, stateBytes, nVertLevels;
} moka_halo_peer_info;
/* How a distributed RK4 stage queues its two launches.  0: boundary patches, then interior patches, on the compute stream
 * (the exchange starts behind the first).  1: boundary patches on the high-priority communication stream, interior patches
 * on the compute stream, in flight together (a small boundary launch no longer leaves the chip idle).  -1 (default):
 * chosen from the size of the interior launch.  Takes effect at the next moka_rk4_dist_begin.  Results are identical. */
int  moka_halo_set_overlap(moka_halo *h, int mode);
/* on != 0: a system-scope acquire (cache invalidate on every XCD) is launched in front of every launch that reads received
 * rows (the boundary patches of a stage, the Forward-Euler vertex pass).  Default off: the acquire of a kernel dispatch makes
 * peer-written rows visible (csrc/halo.hip header); the transport selection falls back to this form ("ipc-acq") when whole steps
 * over the plain direct transport do not reproduce the host-staged exchange bit for bit. */
int  moka_halo_set_acquire(moka_halo *h, int on);
/* the same exchange for arbitrary device fields of the state's shapes and storage type (u-like, h-like, ssh-like), library
 * numbering: pack waits for the compute stream, unpack makes the compute stream wait for the received rows */
int  moka_halo_pack_fields(moka_halo *h, const void *uField, const void *hField, const void *sField, void *sendbuf);
int  moka_halo_unpack_fields(moka_halo *h, void *uField, void *hField, void *sField, const void *recvbuf);
int  moka_halo_direct_available(const moka_halo *h);   /* 1: the receive lists are contiguous ranges (see above) */
int  moka_halo_export(moka_halo *h, int32_t nbr, int32_t shared, moka_halo_peer_info *out);
int  moka_halo_connect(moka_halo *h, int32_t nbr, const moka_halo_peer_info *peer, int32_t shared);
int  moka_halo_push_begin(moka_halo *h, int what);        /* queue the push behind the work on the compute stream */
int  moka_halo_push_signal(moka_halo *h);                 /* host: wait for the own push, then signal the neighbours */
int  moka_halo_push_wait(moka_halo *h, double timeout_s); /* host: wait for every neighbour's signal (MOKA_ERR_COMM on timeout) */

/* Experiment: the direct transport's handshake as stream memory operations (hipStreamWriteValue64 behind the push kernel,
 * hipStreamWaitValue64 in front of the next boundary launch) instead of a host thread that waits for the push event, stores the
 * flags and polls the neighbours': a distributed step becomes enqueue-only.  Call after every neighbour is connected.  A stream
 * wait has no timeout (a dead neighbour blocks the queue until the process ends), so this is a transport CANDIDATE ("ipc-smo" in
 * moka_hip.parallel), qualified like the others; MOKA_ERR_UNSUPPORTED where the device or the flag memory does not allow it. */
int  moka_halo_set_stream_flags(moka_halo *h, int on);

/* Measurement: where a distributed step spends its time on this rank.  moka_halo_stats_enable(h, 1) forgets earlier samples and
 * starts recording, (h, 0) stops; moka_halo_stats_read synchronises the rank's two streams and returns the sums:
 *   steps / host_step_ms              moka_rk4_dist_step calls and the host time spent inside them
 *   exchanges                         direct exchanges signalled
 *   host_signal_wait_ms               host time in moka_halo_push_signal waiting for the rank's own push kernel (its event)
 *   host_flag_store_ms                ... and from that event to the last flag store (event -> flag)
 *   host_wait_ms                      host time in moka_halo_push_wait polling the neighbours' flags
 *   boundary_ / interior_launch_ms    device time of the boundary / interior stage launches (HIP events around each launch, on the
 *   boundary_ / interior_launches     stream it was queued to; at most 2048 launches are recorded) and how many were recorded */
typedef struct {
    int64_t steps, exchanges, boundary_launches, interior_launches;
    double host_step_ms, host_signal_wait_ms, host_flag_store_ms, host_wait_ms, boundary_launch_ms, interior_launch_ms;
} moka_halo_stats;
int  moka_halo_stats_enable(moka_halo *h, int on);
int  moka_halo_stats_read(moka_halo *h, moka_halo_stats *out);

/* distributed form of moka_step_rk4, piecewise: begin; for stage 1..4 { stage(s,0) boundary patches; pack(s) or
 * push_begin(s); stage(s,1) interior patches (overlaps the exchange); transport + unpack(s), or push_signal + push_wait };
 * end.  moka_rk4_dist_stage_launch(s) = stage(s,0) + push_begin(s) + stage(s,1).
 * part = 2: the whole local mesh in one launch, halo entities included (redundantly), exchange behind it.
 * States with the optional nonlinear terms (their stencil needs a halo two cells deep: build_local(rings = 2)) split a stage
 * into its preparation pass and its stage kernel: part 3 = preparation over the boundary and halo patches (after the previous
 * stage's exchange has arrived), part 4 = preparation over the interior patches (owned rows only: may be queued as soon as the
 * previous stage's launches are, and then overlaps that stage's exchange), parts 0 / 1 = the stage kernel over the boundary /
 * interior patches.  moka_rk4_dist_step orders them so; part 2 remains for the kernel variants without per-patch kernels
 * (moka_rk4_dist_parts_available == 0). */
int  moka_rk4_dist_begin(moka_halo *h, double dt);
int  moka_rk4_dist_stage(moka_halo *h, int stage, int part);
int  moka_rk4_dist_parts_available(const moka_halo *h);
int  moka_rk4_dist_stage_launch(moka_halo *h, int stage);
int  moka_rk4_dist_end(moka_halo *h);
/* ... and as ONE call per step.  transport == NULL: the direct exchange (every neighbour must be connected, MOKA_ERR_ARG
 * otherwise); a callback, when given, is always used, connected or not: it moves the packed send buffer of a stage to the
 * neighbours and fills the receive buffer (stream-ordered on the comm stream, or synchronously; returns 0 on success).
 * timeout_s bounds every wait of the direct form. */
typedef int (*moka_transport_fn)(void *user, int what, void *sendbuf_device, void *recvbuf_device);
int  moka_rk4_dist_step(moka_halo *h, double dt, moka_transport_fn transport, void *user, void *sendbuf_device,
                        void *recvbuf_device, double timeout_s);
/* distributed form of moka_step_fe (ocn_timestep(..., ForwardEuler), time_integration.jl:150-193) with the same flags:
 * part 0 boundary patches, 1 interior patches, 2 relativeVorticity; the new level is exchanged as `what` = 5 between
 * part 0 and the end; moka_fe_dist_end rotates the time levels (previous <- current <- new: a third level set takes the new
 * level, so the step can form the reference's stale layerThicknessEdge from the previous level's layerThickness).  Order with the direct transport: part 2 FIRST (it reads
 * old-level rows of halo edges, which a neighbour's next step overwrites once this rank's push has been signalled), then
 * part 0, push, part 1.  moka_fe_dist_step does all of it in one call, in that order. */
int  moka_fe_dist_launch(moka_halo *h, double dt, int flags, int part);
int  moka_fe_dist_end(moka_halo *h);
int  moka_fe_dist_step(moka_halo *h, double dt, int flags, moka_transport_fn transport, void *user, void *sendbuf_device,
                       void *recvbuf_device, double timeout_s);

/* kernel variant selection for measurement (all variants give identical results): 0 = auto [default: 11 when the mesh
 * allows it (even 34 <= nVertLevels <= 64), else 4 (nVertLevels >= 33), else 3]; 11 = record-staged, 16-byte lanes, two
 * entities per wave, own u rows cached in LDS; 4 = plain column kernel; 3 = generic index kernel.  The other design points
 * measured in rounds 1-3 (1, 2, 5-10, 12-14) lost and were removed in round 4 (their numbers: profiles/r0*_variants.txt);
 * moka_set_kernel_variant returns MOKA_ERR_UNSUPPORTED for them. */
int moka_kernel_variant_available(int variant);
int moka_set_kernel_variant(moka_ctx *ctx, int variant);
/* Process-wide launch-shape switches for A/B measurements (every setting gives identical results).  key 1: bit mask of the
 * modes (0 tendency, 1..3 RK4 stages, 4..6 Forward Euler, 10 / 11 lean Forward Euler) of the fp32-storage stage kernel that run as 512-thread workgroups
 * bounded to 128 registers = 4 waves per SIMD instead of 3 (default: mode 0, the tendency launch).  key 2: 0 = Forward-Euler
 * steps always gather the stored layerThicknessEdge (mode 4); 1 (default) = formed from the previous level when valid (mode 6).
 * key 3: relativeVorticity of a Forward-Euler step inside the stage launches (1, default) or as a launch of its own (0).
 * key 4: lean Forward-Euler steps (1, default) or every array stored every step (0).  key 5: launch shape of the nonlinear
 * stage kernel's patch form (0 default: potential vorticity of the patch's vertices in LDS, three workgroups per CU; 1: q_e of
 * its edge rows in LDS, two workgroups; 2 / 3: other shapes of the default).  key 6 (test hook): upper limit of the vertex rows
 * that form keeps resident (0 = what the LDS budget holds).
 * key 8: bit mask of the modes of the Float64 stage kernel whose large whole-range launches take two consecutive patches per
 * 512-thread workgroup, one row cache over both (default: the tendency launch and RK stage 1, modes 0 / 1, and the
 * 13-stream stage 1, mode 7; 0 = one patch per workgroup everywhere).
 * key 9: lean Forward-Euler launches through their own kernel instances (1, default: stage-kernel modes 10 / 11, the optional
 * DiagnosticVars / TendencyVars outputs compiled out) or through the general Forward-Euler instances (0; measurement).
 * key 7 is NOT result-neutral and therefore off by default: 1 = moka_step_rk4 / moka_run step Float64 states on whole meshes
 * with 13 instead of 16 state streams per step.  The reference accumulates New += b_s k_s through the stages
 * (time_integration.jl:134-135); here stages 1-3 store only the provisional states and stage 4 forms
 * New = C + ((P2 - C) + 2 (P3 - C) + (P4 - C)) / 3 + dt/6 k4 from own rows -- the same Runge-Kutta step up to round-off (a
 * few units in the last place of the state per step; oracle twin oracle_step_rk4_s13, tests/test_oracle_igw.py holds the
 * tolerance against the reference form).  With the nonlinear terms on: the same where the stage launch is the default patch
 * kernel (even 34 <= nVertLevels <= 64; twin oracle_step_rk4_nonlinear_s13).  Distributed, taped and fp32-storage steps keep
 * the reference's form.  moka_state_rk4_streams tells which form the next moka_step_rk4 of a state takes.
 * key 12 (keys 10 and 11 do not exist): 1 (default) = RK4 stage 1 hands New to stage 2 as one checked byte per value instead of the
 * value; 0 = New travels in full.  Stage 1 forms Provis' = C + a t and New = C + b t from one tendency, so stage 2 can rebuild New
 * from the own rows of Curr and Provis it reads anyway, C + (P - C) * (b / a), corrected by the stored distance of the bit patterns;
 * a value the byte cannot carry is an escape and travels in the New array as before.  Bit for bit the same step with 7/8 of a state
 * stream less in each of the two stages; Float64 states in the 16-stream form without the nonlinear terms whose stage launches all
 * run through the default stage kernel, whole and partitioned meshes, taped steps included.  The pair mask of key 8 applies to the
 * two launches as to modes 1 and 2.
 * Accepted values (anything else, and a key outside 1-9 and 12, is MOKA_ERR_ARG and changes nothing): key 1 a mask of modes 0-6, 10 and
 * 11; key 8 a mask of modes 0-3 and 7-9 plus bit 16 (test hook: small launches too); key 5 0-3; key 6 >= 0; keys 2, 3, 4, 7, 9 and
 * 12 0 or 1.  moka_get_tuning returns the value last set (or the default). */
int moka_set_tuning(int key, int value);
int moka_get_tuning(int key, int *value);
/* The codec of key 12 as the host runs it, over n values (no GPU is touched; a test aid): code_out[i] is the byte stage 1 would
 * store for New N[i] given Curr C[i], Provis' P[i] and rho = b / a (-128 = escape), decoded_out[i] what stage 2 would rebuild (an
 * escape: N[i], which it reads from the New array). */
int moka_rk_handoff_codec(const double *C, const double *P, const double *N, double rho, int64_t n, int8_t *code_out, double *decoded_out);
/* How many escapes the codes of the last RK4 step hold, over all levels of the state's cells / edges (a test aid: copies the code
 * arrays to the host).  MOKA_ERR_UNSUPPORTED when that step did not hand New over as codes. */
int moka_state_rk_handoff_escapes(moka_state *st, int64_t *cells, int64_t *edges);
/* 13 = the next moka_step_rk4 / moka_run of this state runs in the 13-stream form (key 7 set and the state qualifies), 16 = the
 * reference's running sum (time_integration.jl:134-135); 0 for NULL. */
int moka_state_rk4_streams(const moka_state *st);
/* Per-stage durations of moka_step_rk4 from HIP events on the compute stream (measurement: bench.py's per-mode roofline
 * lines).  moka_stage_timing(ctx, 1) forgets earlier samples and records 5 events per step from now on; (ctx, 0) stops.
 * moka_stage_timing_read: ms[s-1] = mean duration of the stage-s launch over the *steps recorded steps. */
int moka_stage_timing(moka_ctx *ctx, int enable);
int moka_stage_timing_read(moka_ctx *ctx, double ms[4], int64_t *steps);
/* PCI bus id of the context's device ("0000:c5:00.0"; buf of >= 16 bytes): the key to its clock / power files in sysfs and to
 * counting the distinct devices the ranks of a launch really use (measurement). */
int moka_ctx_pci_bus_id(moka_ctx *ctx, char *buf, int32_t len);
/* Per-step statistics of a timed region (measurement: bench.py's median / min / max): moka_mark records one HIP event on the
 * compute stream, n marks give n - 1 intervals; moka_marks_read: ms[i] = time between marks i and i + 1 (at most `capacity`
 * of them), *n = how many exist; moka_marks_reset forgets them. */
int moka_mark(moka_ctx *ctx);
int moka_marks_reset(moka_ctx *ctx);
int moka_marks_read(moka_ctx *ctx, int64_t capacity, double *ms, int64_t *n);
/* Same-run bandwidth calibration (measurement): a plain 16-byte-per-lane copy and a read-only sweep over a buffer of `bytes`
 * (two halves), each launch timed with HIP events on the compute stream; gbs[0] = best copy rate (bytes read + written, GB/s),
 * gbs[1] = best read-only rate, gbs[2] = mean copy rate over the `iters` launches, gbs[3] = best rate of a scattered gather of
 * 480-byte rows, a half-wave per row (the stage kernels' access pattern).  The buffer is kept for the next probe;
 * bytes = 0 frees it.  (MI355X_MICROARCH.md quotes 6.29 TB/s for such a copy; SURVEY.md 8d asks for the copy and read figures.) */
int moka_bw_probe(moka_ctx *ctx, int64_t bytes, int iters, double gbs[4]);
/* ... and a fifth figure: three streams read and two written at once (the mix of the RK stage launches), over the buffer
 * moka_bw_probe allocated: GB/s of all five streams, best of `iters` launches */
int moka_bw_probe_streams(moka_ctx *ctx, int iters, double *gbs);
/* ... and a sixth: `region` bytes of that buffer (between the L2s' 32 MB and the Infinity Cache's 256 MB) read `reps` times back to
 * back -- the rate at which re-read data returns; GB/s over all passes, best of `iters` */
int moka_bw_probe_reread(moka_ctx *ctx, int64_t region, int reps, int iters, double *gbs);
/* ... and a seventh: the scattered row gather over a footprint of its own of `bytes` (allocated and freed here; e.g. 32 GiB, the span
 * of a state with all its arrays), a quarter of the rows once each: nearly every fetch needs an address translation the TLBs do not hold */
int moka_bw_probe_gather_big(moka_ctx *ctx, int64_t bytes, int iters, double *gbs);
/* which kernel the last moka_step_fe of this state used: 1 = the tuned stage kernel (+ vertex pass), 2 = the same with the
 * stale layerThicknessEdge formed from the previous level's layerThickness instead of gathered (every MOKA_FE_STALE_HEDGE
 * step after the first of a run), 0 = the generic one-launch kernel, -1 = no Forward-Euler step yet.  For tests and
 * measurement; results are identical either way. */
int moka_last_fe_path(const moka_state *st);
/* 1 while the TendencyVars / DiagnosticVars of the last Forward-Euler step are pending.  With the default kernel choice a
 * Forward-Euler step of all levels is LEAN: it stores the new time level and relativeVorticity; tendNormalVelocity,
 * tendLayerThickness, thicknessFlux, velocityDivCell and layerThicknessEdge of the step are produced on the first read
 * (download, sum_sq, upload, the piecewise reference calls, a taped step ...), from the level the step started from -- same
 * arithmetic, same bits -- and superseded by the next step otherwise, like the DiagnosticVars an RK4 step leaves pending.
 * The first step of a run with MOKA_FE_STALE_HEDGE, steps on a tape, MOKA_FE_LEVEL1_ONLY steps and moka_set_tuning(4, 0)
 * store everything at once. */
int moka_fe_lazy_pending(const moka_state *st);

/* ---- optional nonlinear terms (extension; NOT in the reference, parity unpinned) ---------------------------------
 * north_star names potential-vorticity Coriolis over edgesOnEdge, the KE + ssh gradient over cellsOnEdge and vertex
 * relativeVorticity; the reference has only the linear f*u_perp term (horizontal_advection_and_coriolis.jl:61-73,
 * SURVEY.md N4).  on = 1 switches moka_tendencies / moka_step_rk4 / moka_run(RK4) of this state to the
 * vector-invariant TRiSK form (Ringler et al. 2010):  q = (fVertex + zeta)/h_vertex at vertices, averaged to edges;
 *   tendU = sum_i w[i,e] F[eoe_i] (q_e + q_eoe_i)/2 - g grad(ssh) - grad(KE),  KE = sum_e dc dv u^2 / (4 areaCell).
 * Default off.  Needs the optional mesh arrays above; Float64 states on whole meshes; no Forward Euler, no tape: on = 1 is
 * MOKA_ERR_UNSUPPORTED while a moka_tape of the state exists, as moka_tape_create is on a nonlinear state.
 * Order of calls: the toggles below and this one take effect with the next tendency evaluation.  What a finished step left in
 * TendencyVars (also where it is produced on the first read) was computed with the terms and coefficients in force during that
 * step, whatever is switched afterwards. */
int  moka_set_nonlinear(moka_state *st, int on);
/* Del2 momentum mixing on top of the nonlinear terms -- the reference's sketch (never called there, and not runnable:
 * src/ocn/Tendencies/normalVelocity/horizontal_momentum_mixing.jl:53-80, with viscDel2 hard-wired to 1.0 at :30):
 *   tendU[k,e] += ((div[k,c2] - div[k,c1]) / dcEdge[e] - (relVort[k,v2] - relVort[k,v1]) / dvEdge[e]) * viscDel2
 * with div = velocityDivCell and relVort = relativeVorticity of the stage's provisional velocity.  0 (default) = off.
 * MOKA_ERR_UNSUPPORTED unless moka_set_nonlinear(st, 1) came first. */
int  moka_set_viscosity_del2(moka_state *st, double viscDel2);
/* Del4 (biharmonic) momentum mixing on top of the nonlinear terms (the reference declares Del2 and Del4,
 * horizontal_momentum_mixing.jl:6-9, and sketches Del2 only).  With L the Del2 bracket above,
 *   L(u)[k,e] = (div(u)[k,c2] - div(u)[k,c1]) * (1/dcEdge[e]) - (curl(u)[k,v2] - curl(u)[k,v1]) * (1/dvEdge[e])   (0 above maxLevelEdgeTop)
 * with div = velocityDivCell, curl = relativeVorticity of the stage's provisional velocity, each tendency evaluation forms d2u = L(u),
 * then div4 = div(d2u), curl4 = curl(d2u) (the same operators, the same operand order), and finishes
 *   tendU[k,e] = <nonlinear tendency, Del2 term included> - ((div4[k,c2] - div4[k,c1]) * (1/dcEdge[e]) - (curl4[k,v2] - curl4[k,v1]) * (1/dvEdge[e])) * coef4[e]
 * for k <= maxLevelEdgeTop[e]: the last operation on the tendency.  coef4[e] = viscDel4 * meshScalingDel4[e] in double, formed here
 * (meshScalingDel4 NULL: coef4 = viscDel4).  A positive viscDel4 damps (MPAS-Ocean's hmix_del4 convention).
 * meshScalingDel4: NULL or nEdges values >= 0 in the caller's edge numbering.  viscDel4 < 0: MOKA_ERR_ARG; 0 (default) = off, and the
 * arithmetic is then that of the nonlinear (+ Del2) form, bit for bit.  MOKA_ERR_UNSUPPORTED unless moka_set_nonlinear(st, 1) came
 * first, and for fp32-storage states and states with a halo (the stencil reaches three cell rings; moka_halo_create and the
 * moka_rk4_dist_* calls refuse a state with Del4 on in turn).  With moka_set_tuning key 7 a Del4 state keeps the reference's running sum
 * (moka_state_rk4_streams: 16). */
int  moka_set_viscosity_del4(moka_state *st, double viscDel4, const double *meshScalingDel4);
/* which kernels formed div4 / curl4 in the last Del4 stage of this state: 1 the fused patch kernel (even K <= 64, hexagon meshes,
 * the default and variant-4 forms), 2 the entity kernels, 0 no Del4 stage yet */
int  moka_state_del4_path(const moka_state *st);

/* ---- passive tracers (extension; the reference has none, parity unpinned, default off) ---------------------------
 * nTracers >= 0 cell-centred tracers phi_j[k,c] ride with the RK4 step in the conservative flux form
 *   d(h phi)/dt = -div(F phi_e),  F = u * h_e the thickness flux of the thickness equation,  phi_e = (phi_c + phi_c') / 2.
 * For a provisional state (pu, ph, pphi), cell c and level k the tendency T accumulates from 0.0 over the slots i of edgesOnCell in
 * slot order, skipping empty slots and slots with k >= maxLevelEdgeTop[e] (levels counted from 0; c' = the cell across slot i):
 *   hE = 0.5 * (ph[k,c] + ph[k,c']);  F = pu[k,e] * hE;  pE = 0.5 * (pphi[k,c] + pphi[k,c']);
 *   T += ((F * pE) * (dvEdge[e] * edgeSignOnCell[i,c])) * (1/areaCell[c])
 * -- the thickness tendency with F * pE for F: a tracer that is 1 everywhere reproduces tendLayerThickness and stays exactly 1.0.
 * Harmonic diffusion (moka_set_tracer_diffusion; default off).  With a diffusivity kappa_j >= 0 (m^2/s) per tracer the scheme is
 *   d(h phi)/dt = -div(F phi_e) + div(kappa_j h_e grad phi).
 * Per cell, level and slot the skip rules are those above, for both terms; after the advective addition of a slot a second,
 * separate addition follows, with the slot's hE and one rounding per operation (no contraction):
 *   G = pphi[k,c'] - pphi[k,c];  T += ((((kappa_j * hE) * G) * dvdc[c,i]) * (1/areaCell[c])),  dvdc[c,i] = dvEdge[e] / dcEdge[e]
 * (dvdc: one double division when the mesh is created; unsigned, so both cells of an edge see the same value).  The RK4 recipe below
 * is untouched: only T gains the term.  Hence: a constant tracer has G == 0 exactly and the unit tracer stays exactly 1.0 for any
 * kappa; (kappa * hE) * G * dvdc is exactly antisymmetric between the two cells of an edge, so the content sum_c A_c sum_k phi h is
 * conserved to round-off as by the advective flux; and adding +-0.0 never changes the bits of T (it starts at +0.0 and cannot become
 * -0.0 under round-to-nearest), so a tracer with kappa_j == 0 beside diffused ones equals the undiffused result bit for bit.
 * Biharmonic diffusion (moka_set_tracer_biharmonic; default off).  With a coefficient kappa4_j >= 0 (m^4/s) per tracer the scheme is
 *   d(h phi)/dt = -div(F phi_e) + div(kappa_j h_e grad phi) - div(kappa4_j h_e grad L_j) + q_j,
 *   L_j = (1/(A h)) sum_e h_e (dv/dc) (phi_c' - phi_c)          the thickness-weighted Laplacian of phi_j.
 * Laplacian pass.  For a cell field x over the thickness ph, per cell c and level k: start from s = 0.0 and run over the slots of
 * edgesOnCell in slot order with the skip rules above (empty slots, slots with k >= maxLevelEdgeTop[e]); per slot
 *   hE = 0.5 * (ph[k,c] + ph[k,c']);  s += (hE * (x[k,c'] - x[k,c])) * dvdc[c,i];
 * and Lap(ph, x)[k,c] = (s * (1/areaCell[c])) / ph[k,c].  One rounding per operation, no contraction.
 * Forward, per stage: L_j = Lap(ph_s, pphi_j) for the tracers with kappa4_j != 0; in the tendency's slot loop a third, separate
 * addition follows the advective and the harmonic ones:
 *   T = T - ((((kappa4_j * hE) * (L_j[k,c'] - L_j[k,c])) * dvdc[c,i]) * (1/areaCell[c]))
 * The source addition and the RK4 recipe are untouched.  Hence: a constant tracer has L == 0 exactly, so the unit tracer stays exactly
 * 1.0; the product is exactly antisymmetric between the two cells of an edge, so content is conserved to round-off; a tracer with
 * kappa4_j == 0 keeps the bits it has without the term, also beside tracers that do have kappa4 != 0, forwards and backwards (T is
 * never -0.0, so the added term would be +-0.0 and change nothing; the library skips it, and never reads L of such a tracer);
 * tracer variance decays by exactly -kappa4 sum_c A_c h_c L_c^2 (sum_c A_c phi_c T4_c, the operator being self-adjoint under the area
 * weight).  The explicit limit is kappa4 dt / dcEdge_min^4 <~ 0.043: RK4 reaches -2.78 on the real axis and the hexagon Laplacian
 * reaches 8 / dc^2, so (kappa 8/dc^2 + kappa4 64/dc^4) dt, the sum of the harmonic and the biharmonic parts, must stay inside 2.78.  It
 * is not checked, as for kappa.
 * One RK4 step, per tracer, with a = (dt/2, dt/2, dt), b = (dt/6, dt/3, dt/3, dt/6) and (pu_s, ph_s), ph_{s+1}, h_new the step's own
 * provisional and new states, whatever terms are switched on (linear, nonlinear, Del2, Del4):
 *   Qc = phi_cur * h_cur;  Qn = Qc;  pphi = phi_cur
 *   s = 0..3:  t = T(pu_s, ph_s, pphi);  s < 3: pphi = (Qc + a[s] * t) / ph_{s+1};  Qn = Qn + b[s] * t
 *   phi_new = Qn / h_new
 * The library stores phi per time level (upload then download is exact; re-uploading layerThickness between steps leaves nothing
 * stale: the contents Q exist inside a step only); layerThickness must be nonzero.  The tracers' time levels rotate with the state's
 * (moka_step_rk4, moka_run(MOKA_RUNGE_KUTTA_4), moka_advance_time_levels).  Tracers never feed back: the dycore's fields are, bit for bit,
 * those of a state without tracers, and moka_tendencies is unchanged.
 * Sources (moka_tracer_source_upload; default none).  Tracer j may carry a source q_j[k,c] in tracer * m/s, the rate of change of the
 * content h phi, constant in time until it is changed:
 *   d(h phi)/dt = -div(F phi_e) + div(kappa_j h_e grad phi) + q_j.
 * For every stage tendency, after the whole slot loop (advective and diffusive additions), one more addition follows with a rounding
 * of its own:   T = T + q_j[k,c].   The RK4 recipe below is untouched, and all four stages see the same q.  Hence: T is never -0.0
 * before that addition, so a source that is zero everywhere (+0.0 or -0.0) leaves every bit of the tracer unchanged; a tracer without a
 * source beside sourced ones has the bits of a state that never had a source (it reads no source and adds nothing); the dycore never
 * sees tracers, so the flow is unchanged bit for bit; and the unit tracer stays exactly 1.0 while it has no source.
 * moka_set_tracers allocates the arrays (zeros; any earlier tracers are dropped); 0 frees them and restores the behaviour of a state
 * that never had any.  MOKA_ERR_ARG for a negative count; MOKA_ERR_UNSUPPORTED for fp32-storage states, partitioned meshes and states
 * that have a halo or a tape.  While nTracers > 0, moka_step_fe, moka_run(MOKA_FORWARD_EULER), moka_tape_create, moka_halo_create and
 * the moka_rk4_dist_* calls return MOKA_ERR_UNSUPPORTED, and moka_set_tuning key 7 leaves the state on the running sum
 * (moka_state_rk4_streams: 16).  moka_state_optimize_placement neither times nor moves the tracer arrays.
 * Out of scope: upwind, FCT and higher-order edge values, a spatially varying kappa or kappa4 or a mesh scaling per edge, anisotropic
 * mixing, Forward Euler,
 * fp32 storage, partitioned meshes, reverse mode with respect to the flow (with respect to the tracers themselves, to the sources and
 * to kappa_j and kappa4_j: moka_tracer_tape_* below), time-dependent sources, point-source convenience calls, the 13-stream form, YAML keys and NetCDF I/O of tracers, and fusing the tracer sum into the dycore's stage
 * kernels. */
int  moka_set_tracers(moka_state *st, int32_t nTracers);
/* *out = the number of tracers as it stands (0: none); MOKA_ERR_ARG for a NULL out */
int  moka_tracer_count(const moka_state *st, int32_t *out);
/* tracer j (0-based) at time_level 0 (previous) / 1 (current): (nVertLevels, nCells) doubles in the caller's cell numbering, like
 * layerThickness */
int  moka_tracer_upload(moka_state *st, int32_t j, int time_level, const double *host);
int  moka_tracer_download(moka_state *st, int32_t j, int time_level, double *host);
/* which kernel served the last tracer stage of this state: 1 the patch form (even 34 <= nVertLevels <= 64, hexagon-width byte-offset
 * records, the default kernel choice), 2 the generic form (everything else, and kernel variant 3), 0 no tracer stage yet */
int  moka_state_tracer_path(const moka_state *st);
/* Harmonic tracer diffusion (algebra above).  kappa: nTracers diffusivities in m^2/s, NULL = all zero; the values take effect with
 * the next RK4 step or moka_run.  MOKA_ERR_ARG, with nothing changed, for a negative, NaN or infinite value and for a non-NULL kappa
 * on a state without tracers.  While every value is zero the tracer launches are those of a state that never set a diffusivity.
 * moka_set_tracers (any count, 0 included) resets every diffusivity to zero.  The explicit stability limit is not checked (as for
 * visc_del2).  Rule of thumb: RK4 is stable on the negative real axis down to about -2.78 and the largest eigenvalue of the hexagon
 * Laplacian is about 8 / dcEdge^2, so kappa dt / dcEdge_min^2 <~ 0.35.  Tracers still never feed back. */
int  moka_set_tracer_diffusion(moka_state *st, const double *kappa);
/* the diffusivity of tracer j (0-based) into *out; MOKA_ERR_ARG for j out of range */
int  moka_tracer_diffusion(const moka_state *st, int32_t j, double *out);
/* Biharmonic tracer diffusion (algebra above).  kappa4: nTracers coefficients in m^4/s, NULL = all zero; the values take effect with
 * the next RK4 step or moka_run.  MOKA_ERR_ARG, with nothing changed, for a negative, NaN or infinite value and for a non-NULL kappa4
 * on a state without tracers.  The first nonzero value allocates the coefficient array and the scratch of L (nTracers * nVertLevels *
 * nCells doubles); every stage then has one more launch, the Laplacian pass, ahead of the tracer launch.  While every value is zero
 * the launches are those of a state that never set one.  moka_set_tracers (any count, 0 included) resets every coefficient to zero.
 * moka_state_tracer_path: the patch form keeps two row sets per resident tracer then (phi and L) and gives way to the generic form
 * when not even one tracer's two fit. */
int  moka_set_tracer_biharmonic(moka_state *st, const double *kappa4);
/* the biharmonic coefficient of tracer j (0-based) into *out; MOKA_ERR_ARG for j out of range */
int  moka_tracer_biharmonic(const moka_state *st, int32_t j, double *out);
/* Tracer sources (algebra above).  host: the source of tracer j, (nVertLevels, nCells) doubles in the caller's cell numbering like
 * moka_tracer_upload (any cell ordering of the mesh); NULL removes tracer j's source.  It takes effect with the next RK4 step or
 * moka_run and stays until changed: the state's time levels rotate, sources do not.  MOKA_ERR_ARG for j out of range and, with nothing
 * changed, for a NaN or infinite value.  Only sourced tracers own a device array; while no tracer has a source the tracer launches are
 * those of a state that never had one.  moka_set_tracers (any count, 0 included) drops every source, as it resets the diffusivities.
 * moka_state_tracer_path answers as without sources: a source is read from global memory, never staged. */
int  moka_tracer_source_upload(moka_state *st, int32_t j, const double *host);
/* the source of tracer j into host (zeros when tracer j has none); MOKA_ERR_ARG for j out of range or a NULL host */
int  moka_tracer_source_download(moka_state *st, int32_t j, double *host);
/* *out = 1 when tracer j has a source, else 0; MOKA_ERR_ARG for j out of range or a NULL out */
int  moka_tracer_has_source(const moka_state *st, int32_t j, int *out);
/* Implicit vertical diffusion (moka_set_tracer_vertical_diffusion; default off).  One coefficient kappaV_j >= 0 (m^2/s) per tracer.  After the
 * RK4 step above has formed phi* = Qn / h_new (stage 4, unchanged), the step is split:
 *   (h_new phi_new)[k] - dt d/dz(kappaV_j d/dz phi_new)[k] = (h_new phi*)[k]
 * -- backward Euler in the vertical, unconditionally stable: layers are metres thick where cells are kilometres wide, and an explicit
 * term would cap dt by h^2 / kappaV.
 * Active depth.  nLev[c] = the maximum of maxLevelEdgeTop[e] over the non-empty slots of edgesOnCell, at most nVertLevels: exactly the
 * levels at which some active element reads the cell (moka_plan_array: MOKA_PA_NLEV).  Levels k >= nLev[c] are neither read into
 * arithmetic nor changed; a column with nLev[c] < 2 is left alone.
 * Arithmetic.  For tracer j with kappaV_j != 0 and a column with n = nLev[c] >= 2, every operation below rounded once, nothing
 * contracted; x[k] = phi*[k,c], h[k] = h_new[k,c], s = dt * kappaV_j:
 *   w[k]  = s / (0.5 * (h[k] + h[k+1]))                         k = 0 .. n-2
 *   d[0]  = h[0] + w[0];   d[k] = (h[k] + w[k-1]) + w[k];   d[n-1] = h[n-1] + w[n-2]
 *   Lv(v)[0] = w[0]*(v[1]-v[0]);   Lv(v)[n-1] = w[n-2]*(v[n-2]-v[n-1])
 *   Lv(v)[k] = w[k-1]*(v[k-1]-v[k]) + w[k]*(v[k+1]-v[k])        0 < k < n-1
 *   Solve(r):  beta = d[0];  y[0] = r[0]/beta
 *              k = 1..n-1:  g[k-1] = w[k-1]/beta;  beta = d[k] - w[k-1]*g[k-1];  y[k] = (r[k] + w[k-1]*y[k-1])/beta
 *              z[n-1] = y[n-1];   k = n-2..0:  z[k] = y[k] + g[k]*z[k+1]
 *   forward:   phi_new = x + Solve(Lv(x))
 *   reverse:   X      <- X + Lv(Solve(X))
 * This is the increment form of A phi_new = h o phi* with A = diag(h) + s W, W the interface-flux matrix of weights 1 / hm.  A is
 * symmetric and strictly diagonally dominant for h > 0: no pivoting.  h > 0 on active levels is required and, like the explicit limits,
 * not checked.  The reverse line is S^T = diag(h) A^-1 = I - s W A^-1, applied to X_j at the head of a reversed step, ahead of
 * g = X / hn, with the recorded hn, dt and kappaV_j of that step; tau_s, G, Wk and Wk4 keep their definitions (sources and horizontal
 * mixing act inside the RK stages, before the solve).  The reverse mode uses the factorisation of the forward pass and stays an exact
 * transpose; the tape records nTracers doubles more per step.
 * Hence: a tracer that is constant over a column has Lv(x) == 0 exactly, so the unit tracer stays exactly 1.0; a tracer with
 * kappaV_j == 0 is skipped by a wave-uniform branch (nothing is added to it) and keeps every bit, also beside mixed tracers, forwards
 * and backwards; the column content sum_k h phi is conserved to round-off; A^-1 diag(h) is row-stochastic and non-negative, so every
 * active value of a column stays inside that column's former range up to round-off (the limiter-free centred horizontal scheme has no
 * such property).  The launch is skipped when nVertLevels < 2, when dt == 0.0 and while every kappaV is zero.
 * moka_step_rk4, moka_run and moka_step_rk4_tracer_taped return MOKA_ERR_ARG before any launch when dt < 0 and some kappaV != 0.
 * kappaV: nTracers values, NULL = all zero; they take effect with the next RK4 step or moka_run.  MOKA_ERR_ARG, with nothing changed,
 * for a negative, NaN or infinite value and for a non-NULL kappaV on a state without tracers.  The first nonzero value allocates the
 * coefficient array and the scratch of the column form (2 * nVertLevels * nCells doubles); while every value is zero a step launches,
 * allocates and records what a state that never set one does.  moka_set_tracers (any count, 0 included) resets every value to zero.
 * Gradient with respect to kappaV_j (moka_tracer_adjoint_want_vertical_gradient, with the tracer tape below).  d J / d kappaV_j =
 * -dt sum over columns and k of (z[k] - z[k+1]) (phi_new[k] - phi_new[k+1]) / hm[k] with z = A^-1 X and hm[k] = 0.5 (h[k] + h[k+1]);
 * the unsummed term is, per interface and cell, d J / d kappaV(k+1/2, c): the sensitivity to a depth-dependent diffusivity, at the
 * diffusivity the run used -- the uniform kappaV_j, or the field f_j of moka_tracer_vertical_field_upload below, for which D_j is
 * d J / d f_j[k,c] itself.  The product keeps that density.  Consider a recorded step with its own dt, hn (h below) and
 * kappaV_j; X_j the adjoint of phi_new as it stands at the head of the reversed step, BEFORE S^T is applied; p = phi_new,j, tracer j at
 * the new level as the step left it (after the vertical pass where one ran, otherwise what stage 4 formed), recorded behind the step by
 * a copy.  For a flagged tracer j and a column with n = nLev[c] >= 2, every operation rounded once, nothing contracted:
 *   z = Solve(X)            the bits the reverse pass forms (y, g downwards; z upwards), when kappaV_j != 0 in that step
 *   z[k] = X[k] / h[k]      when kappaV_j == 0 in that step (A = diag(h); a derivative at zero is legitimate, as for kappa4)
 *   k = 0 .. n-2:   q = dt / (0.5 * (h[k] + h[k+1]));   c = (p[k] - p[k+1]) * q;   e = (z[k] - z[k+1]) * c;   D_j[k,c] = D_j[k,c] - e
 * D_j is (nVertLevels, nCells) doubles; row k belongs to the interface between levels k and k+1; rows k >= nLev[c] - 1, row
 * nVertLevels - 1 included, are never written and stay 0.0.  Like G and Wk, D_j accumulates over every recorded step and is zeroed
 * where they are, at the first seed after a recorded step.  A recorded step with dt == 0.0, or a mesh with nVertLevels < 2, contributes
 * nothing and launches nothing; flagging is still allowed there and every view is zeros.  No column reduction happens on the device, so
 * the device leaves no summation order to pin.  Host views, over the caller's numbering in ascending order, in long double, rounded once:
 *   cell:     Wv_j[c] = sum_k D_j[k,c]        profile:  Pv_j[k] = sum_c D_j[k,c]        scalar:  d J / d kappaV_j = sum_c sum_k D_j[k,c]
 * (the scalar cell-major); independent of the mesh's cell ordering because D is elementwise per column.
 * Hence: asking for the gradient changes no bit of X, G, Wk, Wk4, the state or the tracers; a flagged tracer with kappaV_j == 0 keeps
 * every bit of its X (only z is formed, nothing is added to X); an unflagged tracer is neither recorded, read nor written; a tracer
 * that is constant over a column has c == 0 exactly, so the unit tracer's density is exactly 0.0; a zero seed gives exactly zero; the
 * map is linear in the seed; values at levels >= nLev[c] of p and X (NaN fill under the sea floor) never reach D.  The derivative is
 * with respect to a coefficient acting identically in every recorded step (the values the steps ran with may differ from step to
 * step), the flow held as it ran.
 * Out of scope: a kappaV that varies in time other than by a new call between steps, a per-step split of D, second derivatives,
 * vertical advection, vertical mixing of momentum, Forward Euler, fp32 storage, partitioned meshes, YAML keys and NetCDF I/O, the
 * 13-stream form. */
int  moka_set_tracer_vertical_diffusion(moka_state *st, const double *kappaV);
/* the vertical diffusivity of tracer j (0-based) into *out; MOKA_ERR_ARG for j out of range */
int  moka_tracer_vertical_diffusion(const moka_state *st, int32_t j, double *out);
/* which kernel served the last vertical pass of this state: 1 the tile form (column tiles staged in LDS, a lane per column; nVertLevels
 * <= 105), 2 the column form (a lane per column from global memory: deeper columns, and kernel variant 3), 0 no vertical pass yet */
/* moka_set_tracers (any count, 0 included) puts this answer, like that of moka_state_tracer_path, back to 0. */
int  moka_state_tracer_vmix_path(const moka_state *st);
/* A vertical diffusivity per interface and cell (default: none).  Tracer j may carry a field f_j >= 0 (m^2/s), laid out as every tracer
 * field and as D_j are: (nVertLevels, nCells) doubles, row k of a column the interface between levels k and k+1.  Rows
 * k >= nLev[c] - 1, row nVertLevels - 1 included, are never read and may hold anything, NaN included.  For such a tracer the recipe
 * above changes in one operand,
 *   s[k] = dt * f_j[k,c]                          (one product, rounded once)
 *   w[k] = s[k] / (0.5 * (h[k] + h[k+1]))         k = 0 .. n-2
 * and stays as it is, letter for letter, in d, Lv, Solve, the forward line x + Solve(Lv(x)), the reverse line X + Lv(Solve(X)) and the
 * gradient lines q, c, e and D = D - e, with z from the field's solve.  While tracer j has a field its kappaV_j is not read for it (the
 * scalar is kept and acts again once the field is removed).
 * Hence: a field that equals kappa at every active interface gives the bits of the scalar kappa, forwards, backwards and in D (dt *
 * kappa is the same product); an interface with f == 0 decouples the column there (w == 0, g == 0, no pivot is lost: beta >= h > 0);
 * A stays symmetric and strictly diagonally dominant for f >= 0, h > 0; the unit tracer stays exactly 1.0, the column content stays
 * conserved and every active value stays inside its column's former range, as above; D_j[k,c] is d J / d f_j[k,c] for a field that
 * acts in every recorded step, and the scalar view is the directional derivative along the all-ones field.
 * A field whose active entries are all zero (found by the host scan of the upload) counts as kappaV_j == 0: the tracer is skipped by
 * the wave-uniform branch and keeps every bit, and a gradient takes z[k] = X[k] / h[k].
 * "The pass is on" -- nLev and the scratch of the column form exist, dt < 0 is refused, the launch is skipped only for nVertLevels < 2
 * and dt == 0.0 -- now reads: some kappaV_j != 0 that is not set aside by a field, or some tracer has a field with a nonzero active
 * entry.  A state that never uploads a field launches, allocates and records exactly what it did before.
 * The tile form stages s[k] into the column set that y[k] overwrites once s[k] is read: the same LDS, the same tiles, the same paths
 * (moka_state_tracer_vmix_path, moka_tracer_adjoint_vmix_path), one more field read per tracer with a field.
 * host: (nCells, nVertLevels) in the caller's numbering like moka_tracer_upload; NULL removes the field and the tracer returns to its
 * scalar.  MOKA_ERR_ARG, with nothing changed, for j out of range, a state without tracers, and a negative, NaN or infinite value at an
 * active row, k < nLev[c] - 1 by the plan's nLev (MOKA_PA_NLEV); inactive rows are not inspected.  The call synchronises the stream
 * before it replaces a field a launch may still read, and takes effect with the next RK4 step or moka_run.  moka_set_tracers frees
 * every field; moka_set_tracer_vertical_diffusion leaves them alone.
 * Tape: moka_step_rk4_tracer_taped keeps, per tracer, a copy of the field the step ran with -- K * nCells doubles, taken device to
 * device on the context's stream ahead of the step's first launch, and only when the field was uploaded or removed since the tape's
 * newest copy of it -- so that the reverse pass and the gradient instances of a recorded step use the field of that step.  The copies
 * are released when a sweep has emptied the tape and when the tape is destroyed.  A tape whose steps never saw a field allocates,
 * records and launches what it did before.
 * Out of scope: a field shared across tracers (upload the same array per tracer; the Richardson-number closure further down computes
 * one field for a set of tracers), KPP, vertical mixing of momentum, and everything listed above. */
int  moka_tracer_vertical_field_upload(moka_state *st, int32_t j, const double *host);
/* the diffusivity field of tracer j into host (zeros when tracer j has none); MOKA_ERR_ARG for j out of range or a NULL host */
int  moka_tracer_vertical_field_download(moka_state *st, int32_t j, double *host);
/* *out = 1 when tracer j has a diffusivity field, else 0; MOKA_ERR_ARG for j out of range or a NULL out */
int  moka_tracer_has_vertical_field(const moka_state *st, int32_t j, int *out);

/* ---- implicit vertical mixing of momentum with a surface stress and a bottom drag (extension; default off) -----------
 * The other half of what MPAS-Ocean's vmix does, and the first forcing of this model.  nuV >= 0 (m^2/s) and a linear bottom drag
 * r >= 0 (m/s) are one scalar each per state; tau_e (m^2/s^2: wind stress over rho0 along the edge normal) is an optional field of
 * nEdges doubles.  After stage 4 of the RK4 step has formed the new level (u*, h_new) the step is split, per edge column:
 *   (h_e u_new)[k] - dt d/dz(nuV d/dz u_new)[k] = (h_e u*)[k],      top flux = tau_e,   bottom flux = -r * u_new[n-1]
 * -- backward Euler, unconditionally stable; nothing else in the step changes.
 * Arithmetic.  For edge e with n = maxLevelEdgeTop[e] (at most nVertLevels) and c1, c2 = cellsOnEdge, every operation below rounded
 * once, nothing contracted; x[k] = u*[k,e]; h[k] = 0.5 * (h_new[k,c1] + h_new[k,c2]), the hE of the tracer recipe; s = dt * nuV,
 * q = dt * r, b = dt * tau[e], one product each; Lv and Solve those of the tracer recipe above:
 *   w[k]  = s / (0.5 * (h[k] + h[k+1]))                      k = 0 .. n-2
 *   d[0]  = h[0] + w[0];  d[k] = (h[k] + w[k-1]) + w[k];  d[n-1] = h[n-1] + w[n-2]      (n == 1: d[0] = h[0])
 *   drag on (r != 0):     d[n-1] = d[n-1] + q
 *   R     = Lv(x)                                             (n == 1: R[0] = 0.0)
 *   stress present:       R[0]   = R[0] + b
 *   drag on:              R[n-1] = R[n-1] - q * x[n-1]        (after the stress addition when n == 1)
 *   u_new = x + Solve(R)                                      (Solve with this d; n == 1: y[0] = R[0] / d[0])
 * This is the increment form of A u_new = h o u* + b e_0 with A = diag(h) + s W + q e_{n-1} e_{n-1}^T; A is symmetric and strictly
 * diagonally dominant for h > 0: no pivoting.  h > 0 on active levels is required and not checked.
 * The stress and drag lines are wave-uniform switches, not added zeros: a state with r == 0 and no stress runs the nuV-only
 * arithmetic.  A stress that is zero at every edge with n >= 1 (found by the host scan of the upload) counts as absent.
 * Which columns: a column is computed when n >= 2, or when n == 1 and drag or stress is on.  Edges with n == 0 are never touched and
 * their cells never read; the same for n == 1 with only nuV on.  Levels k >= n of u and of both cells' h are neither read into
 * arithmetic nor written.
 * Hence: without drag and stress a depth-uniform column has Lv(x) == 0 exactly and comes back bit for bit; the column momentum obeys
 * sum_k h u_new - sum_k h u* = dt tau - dt r u_new[n-1] to round-off; without stress sum_k h u_new^2 does not grow, and without stress
 * and drag every value stays inside the column's former range (A^-1 diag(h) is row-stochastic and non-negative); the profile
 * u[n-1] = tau / r, u[k] - u[k+1] = tau hm[k] / nuV is a fixed point.
 * "The pass is on": nuV != 0, or r != 0, or a stress is present with a nonzero entry at an edge with n >= 1.  While it is off a step
 * launches, allocates and records exactly what it does without this extension.  The launch is skipped for dt == 0.0 (and for
 * nVertLevels == 1 with only nuV on); dt < 0 with the pass on is MOKA_ERR_ARG before any launch (moka_step_rk4, moka_run,
 * moka_step_rk4_tracer_taped).  The pass runs behind stage 4 of moka_step_rk4 in the 16- and the 13-stream form, over the linear, the
 * nonlinear, the Del2 and the Del4 dycore, inside the graph moka_run replays (the step allocates nothing, synchronises nothing and
 * reads nothing back); ssh of the new level depends on h only and stays valid; the lazily produced stage-4 tendencies are those of the
 * provisional state and are untouched; the diagnostics of the new level come from the mixed u.  Tracers never see the pass inside a
 * step -- their stage 4 reads the provisional flow -- so their launches, their tape and the tracer vertical pass keep their arithmetic;
 * they see a different flow from the next step on.
 * Values take effect with the next RK4 step or moka_run.  MOKA_ERR_ARG, with nothing changed, for a negative, NaN or infinite nuV or r,
 * a NaN or infinite stress value and NULL out-pointers.  MOKA_ERR_UNSUPPORTED, for a call that asks for a nonzero value or uploads a
 * stress, on fp32-storage states, states with a halo or on a partitioned mesh, and states that have a moka_tape.  While the pass is on
 * moka_step_fe, moka_run(MOKA_FORWARD_EULER), moka_tape_create, moka_halo_create and the moka_rk4_dist_* calls return
 * MOKA_ERR_UNSUPPORTED.  The first call that turns the pass on allocates the column form's scratch of 2 * nVertLevels * nEdges doubles;
 * no step allocates anything.  moka_state_optimize_placement neither times nor moves the new arrays.
 * Out of scope: reverse mode through the pass by a moka_tape handle (the operator depends on h_new, so the flow adjoint gains thickness
 * terms; the moka_forced_tape handle, below, carries them), closures other than the Richardson-number one further down (KPP), Forward Euler, fp32
 * storage, partitioned meshes, YAML keys and NetCDF I/O, a time-dependent stress other than by a new upload between steps. */
int  moka_set_vertical_viscosity(moka_state *st, double nuV, double bottomDrag);
/* the two scalars as they stand; MOKA_ERR_ARG for a NULL out-pointer */
int  moka_vertical_viscosity(const moka_state *st, double *nuV, double *bottomDrag);
/* host: nEdges doubles in the caller's edge numbering; NULL removes the stress.  The call synchronises the stream before it replaces an
 * array a launch may still read. */
int  moka_surface_stress_upload(moka_state *st, const double *host);
/* the stress into host (nEdges doubles; zeros when there is none); MOKA_ERR_ARG for a NULL host */
int  moka_surface_stress_download(moka_state *st, double *host);
/* *out = 1 when a stress is present (all-zero ones included), else 0; MOKA_ERR_ARG for a NULL out */
int  moka_has_surface_stress(const moka_state *st, int *out);
/* which kernel served the last momentum pass of this state: 1 the tile form (tiles of edge columns staged in LDS, the edge thickness
 * gathered from the two cell columns; nVertLevels <= 105), 2 the column form (a lane per edge from global memory: deeper columns,
 * nVertLevels == 1 and kernel variant 3), 0 no pass yet */
int  moka_state_momentum_vmix_path(const moka_state *st);
/* A vertical viscosity per interface and edge (default: none; MPAS-Ocean's vertViscTopOfEdge).  The state may carry a field f >= 0
 * (m^2/s) in place of the one nuV: (nEdges, nVertLevels) doubles in the caller's numbering, like a normalVelocity upload; row k of an
 * edge column is the interface between levels k and k+1.  With n_e = min(maxLevelEdgeTop[e], nVertLevels), rows k >= n_e - 1, row
 * nVertLevels - 1 included, are never read -- by the host scan or on the device -- and may hold anything, NaN included.  The recipe
 * of moka_set_vertical_viscosity changes in one operand,
 *   s[k] = dt * f[k,e]                            (one product, rounded once)
 *   w[k] = s[k] / (0.5 * (h[k] + h[k+1]))         k = 0 .. n-2
 * and stays as it is, letter for letter, in d, R, the stress and drag lines, Solve and u_new = x + Solve(R).  While a field is present
 * nuV is not read (the scalar is kept and acts again once the field is removed).
 * Hence: a field that equals nuV at every active interface gives the bits of the scalar, forwards and backwards (dt * nuV is the same
 * product); an interface with f == 0 decouples the column there (w == 0, g == 0, no pivot is lost: beta >= h > 0); A stays symmetric
 * and strictly diagonally dominant for f >= 0, h > 0; the momentum budget, the contraction and the range property hold as stated
 * above.
 * A field whose active entries are all zero (found by the host scan of the upload) counts as nuV == 0.  "The pass is on" now reads:
 * nuV != 0 that is not set aside by a field, or a field with a nonzero active entry, or r != 0, or a stress present in the sense above.
 * Which columns are computed does not change.  A state that never uploads a field launches, allocates and records exactly what it did
 * before.
 * Kernels: the FIELD instances of both forms.  The tile form stages the tile's span of f into the column set that y[k] overwrites
 * once s[k] is read: the same LDS, the same tiles, the same boundary (nVertLevels 105 / 106) and the same path values, one more
 * coalesced read of nVertLevels * nEdges doubles.  The column form reads f from the edge's own column.
 * host: NULL removes the field; on a state without one the call does nothing.  MOKA_ERR_ARG, with nothing changed, for a negative, NaN
 * or infinite value at an active row (k < n_e - 1; inactive rows are not inspected).  MOKA_ERR_UNSUPPORTED where
 * moka_set_vertical_viscosity returns it for a nonzero value (fp32 storage, a halo, a partitioned mesh, an existing moka_tape) -- a
 * removal included when it would let a nuV != 0 act again (an all-zero field had set it aside while such an object was created): the
 * field then stays --, and everything that is refused while the pass is on is refused when a field turned it on.  The call synchronises
 * the stream before it replaces an array a launch may still read, and takes effect with the next RK4 step or moka_run -- a moka_run
 * after the call never replays launches captured before it.  A field costs nVertLevels * nEdges doubles of device memory; the upload
 * that turns the pass on allocates the column form's scratch.
 * Out of scope: closures that would compute the field other than the Richardson-number one further down (KPP), fp32 storage, partitioned meshes, YAML keys and NetCDF
 * I/O, and everything listed above. */
int  moka_vertical_viscosity_field_upload(moka_state *st, const double *host);
/* the field into host, (nEdges, nVertLevels) doubles (zeros when there is none); MOKA_ERR_ARG for a NULL host */
int  moka_vertical_viscosity_field_download(moka_state *st, double *host);
/* *out = 1 when a field is present (all-zero ones included), else 0; MOKA_ERR_ARG for a NULL out */
int  moka_has_vertical_viscosity_field(const moka_state *st, int *out);
/* Quadratic bottom drag (default: off; MPAS-Ocean's config_use_implicit_bottom_drag).  One more scalar per state, Cd >= 0
 * (dimensionless): the drag coefficient of an edge becomes r + Cd * sp[e], sp[e] the speed sqrt(KE[c1] + KE[c2]) of u* at the edge's
 * bottom level, KE the kinetic-energy stencil of the nonlinear dycore.  For an edge e the pass computes, with
 * n = min(maxLevelEdgeTop[e], nVertLevels) >= 1, kb = n - 1, x = u* (the new level's normalVelocity as stage 4 left it),
 * (c1, c2) = cellsOnEdge[e], kc[e'] = 0.25 * dcEdge[e'] * dvEdge[e'] (two products, left to right) and invArea[c] = 1 / areaCell[c]
 * (MOKA_PA_INVAREA), every operation rounded once, nothing contracted:
 *   for c in (c1, c2):
 *       acc = 0.0
 *       for slot i of edgesOnCell[:, c] in slot order, e' = edgesOnCell[i, c]:
 *           if min(maxLevelEdgeTop[e'], nVertLevels) > kb:         (else the term is omitted and u[kb,e'] is NOT read)
 *               acc = acc + (kc[e'] * x[kb,e']) * x[kb,e']
 *       KE_c = acc * invArea[c]
 *   sp[e] = sqrt(KE_c1 + KE_c2)                                     (correctly rounded)
 *   rq    = r + Cd * sp[e]
 *   q_e   = dt * rq
 * and the recipe of moka_set_vertical_viscosity runs letter for letter with q_e where it has q:
 *   d[n-1] = d[n-1] + q_e;      R[n-1] = R[n-1] - q_e * x[n-1]
 * "Drag on" now reads r != 0 or Cd != 0: that decides the drag lines, the n == 1 columns and "the pass is on".
 * Hence: Cd == 0 launches, allocates and records exactly what the state did before -- no speed launch, no new array; with Cd != 0
 * and u* == 0 in the stencil sp == 0 and r + 0.0 gives the bits of the linear pass; q_e >= 0, so symmetry, diagonal dominance, the
 * contraction and the range property hold as stated above; the column momentum obeys sum_k h u_new - sum_k h u* = dt tau -
 * q_e u_new[n-1] to round-off; levels k >= n of any edge are still never read, the gather of the speed included.  On a uniform flow U
 * over a flat bottom of depth h with nuV == 0, r == 0 and one level, sp == |U| and 1 / u_new = 1 / u* + dt Cd / h (for u* > 0): the
 * steps sample the exact solution of du/dt = -Cd |u| u / h.
 * Kernels: sp comes from a launch of its own in front of the pass (the pass overwrites u in place, tile by tile, and the stencil of an
 * edge reaches into other tiles): one lane per edge, the sums in slot order in registers, no atomics; any nVertLevels, any maxEdges,
 * every kernel variant.  sp[e] = 0.0 for edges with n == 0.  The pass runs its QD instances, which read sp[e] where the others take the
 * one q; tiles, LDS, the 105 / 106 boundary and the path values are those of the linear drag.  Both launches are issued by the step on
 * its stream and replayed by moka_run's graph; a moka_run after the call never replays launches captured before it.  The first call
 * with Cd != 0 allocates nEdges doubles for sp (and the column form's scratch, and uploads kc where the mesh has not); no step
 * allocates anything.
 * MOKA_ERR_ARG, with nothing changed, for a negative, NaN or infinite Cd and NULL pointers.  MOKA_ERR_UNSUPPORTED for Cd != 0 where
 * moka_set_vertical_viscosity returns it for a nonzero value (fp32 storage, a halo, a partitioned mesh, an existing moka_tape) and
 * while a moka_forced_tape made by moka_forced_tape_create exists; everything that is refused while the pass is on is refused when Cd
 * turned it on, and moka_forced_tape_create, and moka_step_rk4_forced_taped on such a tape, return MOKA_ERR_UNSUPPORTED while Cd != 0.
 * Reverse mode of the flow through this drag is the business of a tape made by moka_forced_tape_create_quadratic (below), beside
 * which any Cd is accepted at any time.  The tracer tape is unaffected.
 * Out of scope: reverse mode of the flow through this drag, a Cd field per edge or cell, Forward Euler, fp32 storage, partitioned
 * meshes, YAML keys and NetCDF I/O -- "reverse mode" meaning moka_tape and a tape of moka_forced_tape_create here: the one tape that
 * differentiates the flow through this drag is that of moka_forced_tape_create_quadratic. */
int  moka_set_quadratic_bottom_drag(moka_state *st, double cd);
/* Cd as it stands; MOKA_ERR_ARG for a NULL out-pointer */
int  moka_quadratic_bottom_drag(const moka_state *st, double *cd);
/* the sp the last pass of this state used into host, nEdges doubles in the caller's edge numbering; zeros when that pass ran without
 * Cd or none has run; MOKA_ERR_ARG for a NULL host */
int  moka_bottom_speed_download(moka_state *st, double *host);
/* sp of the recipe above from normalVelocity of time level 0 (previous) or 1 (current) into host (nEdges doubles, the caller's
 * numbering), synchronously and without a step, by the kernel the step launches: a diagnostic of the bottom stress Cd * sp * u.  Any
 * Float64 state on a whole mesh, whatever Cd is; MOKA_ERR_UNSUPPORTED for fp32 storage, a halo or a partitioned mesh; MOKA_ERR_ARG for
 * another time level or a NULL host. */
int  moka_bottom_speed(moka_state *st, int time_level, double *host);
/* The Richardson-number closure (default: off; MPAS-Ocean's config_use_rich_visc / config_use_rich_diff, the Pacanowski-Philander
 * form): the coefficients of both vertical passes computed on the device, behind stage 4 of every RK4 step, from the state the step
 * has just formed, and handed to the passes through the field operands above -- F (nVertLevels, nEdges) is the viscosity field of the
 * momentum pass, G (nVertLevels, nCells) the diffusivity field of the tracer pass; row k is the interface between levels k and k+1.
 * One tracer jb of the state is designated as buoyancy b (m/s^2, b = -g (rho - rho0) / rho0: a larger b above means stable).
 * Parameters, all >= 0: nu0 (m^2/s; config_rich_mix, 0.005), alpha (5), nuBackground nuB (m^2/s; 1e-4), kappaBackground kB (m^2/s;
 * 1e-5), convective conv (m^2/s; 1.0), added to both coefficients where the column is statically unstable; tracerMask: nTracers flags,
 * nonzero = the tracer takes the closure's diffusivity (NULL: every tracer).  EPS = 1e-20 is a constant of the recipe.
 * Arithmetic.  Every operation below rounded once, nothing contracted.  The inputs are those of the new level as stage 4 and the
 * tracers' stage 4 left them, before either vertical pass runs: u = u*, h = h_new, b = phi*_jb.  kc, invArea, nLev and the
 * maxLevelEdgeTop of a cell's slots are the ones the bottom-speed kernel and the vertical passes use.
 * Edge e, n = min(maxLevelEdgeTop[e], nVertLevels), (c1, c2) = cellsOnEdge[e], for the interfaces k = 0 .. n-2:
 *   hE[k]  = 0.5 * (h[k,c1] + h[k,c2])                                (the hE of the momentum recipe)
 *   hm     = 0.5 * (hE[k] + hE[k+1])
 *   db     = 0.5 * ((b[k,c1] - b[k+1,c1]) + (b[k,c2] - b[k+1,c2]))
 *   du     = u[k,e] - u[k+1,e]
 *   Ri     = (db * hm) / (du * du + EPS)
 *   Ri > 0 :  t = 1.0 + alpha * Ri;  m = nu0 / (t * t);   F[k,e] = nuB + m
 *   else   :  F[k,e] = nuB + nu0;    if db < 0:  F[k,e] = F[k,e] + conv
 * Cell c, n = nLev[c], for k = 0 .. n-2:
 *   hm  = 0.5 * (h[k,c] + h[k+1,c]);   db = b[k,c] - b[k+1,c]
 *   acc = 0.0;  for slot i of edgesOnCell[:,c] in slot order, e' = edgesOnCell[i,c]:
 *                  if min(maxLevelEdgeTop[e'], nVertLevels) > k+1:    (else the slot is omitted and NEITHER level of u[.,e'] is read)
 *                      du = u[k,e'] - u[k+1,e'];   acc = acc + (kc[e'] * du) * du
 *   S2  = 2.0 * (acc * invArea[c])
 *   Ri  = (db * hm) / (S2 + EPS)
 *   Ri > 0 :  t = 1.0 + alpha * Ri;  m = nu0 / (t * t);   G[k,c] = kB + (nuB + m) / t
 *   else   :  G[k,c] = kB + (nuB + nu0);   if db < 0:  G[k,c] = G[k,c] + conv
 * Rows k >= n-1 of F and G are never written: they stay 0.0 from allocation and are never read.  Levels that no active element reads
 * -- u at k >= n_e, b and h at k >= nLev[c] -- may hold anything, NaN included, and never reach F or G (nLev[c] is the largest n_e of
 * the cell's edges, so the edge recipe reads b[k+1,c] only for k+1 <= n_e - 1 < nLev[c]).
 * While the closure is on the momentum pass runs its FIELD instances with F where it would take the uploaded field or nuV, and every
 * tracer of the set runs the field instances of the tracer pass with G where it would take its own field or kappaV_j.  The caller's
 * nuV, viscosity field, kappaV_j and per-tracer fields are kept: they are set aside and act again when the closure is switched off,
 * and their setters and uploads keep working, with their own validation, meanwhile.  Drag, quadratic drag and stress are untouched;
 * tracers outside the set keep their own coefficient.  Both passes count as on whenever the closure is on (an all-zero F or G is
 * legitimate: it decouples the columns, as f == 0 does above); dt < 0 is MOKA_ERR_ARG before any launch; with dt == 0.0 or
 * nVertLevels < 2 the closure launches nothing, like the passes, and the momentum pass of a one-level state is the one it was.
 * Hence: a buoyancy that is constant over every column gives db == 0, Ri == 0, F = nuB + nu0 and G = kB + (nuB + nu0) everywhere, and
 * such a step has the bits of a step with the scalars nuV = fl(nuB + nu0) and kappaV_j = fl(kB + fl(nuB + nu0)); alpha == 0 gives the
 * same where db >= 0.  nuB <= F <= (nuB + nu0) + conv, and kB <= G <= (kB + (nuB + nu0)) + conv.  The sign of db decides the branch
 * exactly (a difference of doubles is zero only for equal operands; the edge's db is a sum of two of them and its sign is that of the
 * rounded sum).  No operation cancels after the differences du and db, so F and G carry a small counted multiple of 2^-53 of relative
 * error against exact arithmetic on the same du and db.  The unit tracer stays exactly 1.0, the column content is conserved and the
 * momentum budget holds as stated for the passes: F >= 0 and G >= 0 are all they ask.
 * Kernels (csrc/vmix_closure.hip): k_rich_edge and k_rich_cell, two launches in front of the tracer pass and the momentum pass, the
 * lanes along k so that loads and stores are contiguous, the k+1 operand a second load of the same lines, the cell's sum in slot
 * order in registers; no atomics, no LDS, any nVertLevels, every kernel variant.  The same launches over every dycore, in the 16-stream
 * form of the step: the 13-stream form never carries tracers, and the closure needs one, so a state with the closure on takes the
 * 16-stream step whatever moka_set_tuning key 7 says.  The step issues launches only: F, G, kc, nLev, both column forms' scratch and the table the tracer pass reads
 * are allocated by the call that switches the closure on (nVertLevels * (nEdges + nCells) doubles, plus the scratch where the passes
 * had none), nothing is allocated, synchronised or read back inside a step, and moka_run's graph replays the closure; a moka_run after
 * a switch never replays launches captured before it.  A state that never switches the closure on launches, allocates and records
 * exactly what it did before.
 * p == NULL switches the closure off and frees F and G.  MOKA_ERR_ARG, with nothing changed, for a negative, NaN or infinite
 * parameter, buoyancyTracer out of range, a state without tracers, NULL out-pointers and another time level.  MOKA_ERR_UNSUPPORTED
 * where moka_set_vertical_viscosity returns it for a nonzero value (fp32 storage, a halo, a partitioned mesh, an existing moka_tape)
 * and while a moka_forced_tape of either kind or a moka_tracer_tape of this state exists: the closure makes the step nonlinear in the
 * buoyancy tracer and the coefficients depend on the flow, so the tapes' transposes would no longer be exact.  While the closure is on
 * moka_tape_create, moka_forced_tape_create, moka_forced_tape_create_quadratic, moka_tracer_tape_create, moka_halo_create, the
 * moka_rk4_dist_* calls, moka_step_fe and moka_run(MOKA_FORWARD_EULER) return MOKA_ERR_UNSUPPORTED with a message that names the
 * closure.  moka_set_tracers (any count) switches the closure off and frees G.
 * Out of scope: KPP and any non-local closure, an equation of state (the caller supplies buoyancy as a tracer), reverse mode of the flow
 * or of the tracers through or beside the closure, Forward Euler, fp32 storage, partitioned meshes, YAML keys and NetCDF I/O, smoothing of Ri in space or time, and
 * fusion into the pass kernels. */
typedef struct {
    int32_t buoyancyTracer;
    double nu0, alpha, nuBackground, kappaBackground, convective;
    const int32_t *tracerMask;      /* (opt) nTracers flags; NULL = every tracer */
} moka_richardson_params;
int  moka_set_richardson_mixing(moka_state *st, const moka_richardson_params *p);
/* *on = 1 while the closure is on, else 0; *out the parameters as they stand (zeros while it is off; tracerMask is always NULL);
 * maskOut (opt): nTracers flags, nTracers by moka_tracer_count */
int  moka_richardson_mixing(const moka_state *st, int *on, moka_richardson_params *out, int32_t *maskOut);
/* F and G the last step of this state computed, (nEdges, nVertLevels) and (nCells, nVertLevels) doubles in the caller's numbering;
 * zeros when that step ran without the closure or launched nothing; either may be NULL */
int  moka_richardson_fields_download(moka_state *st, double *viscEdge, double *diffCell);
/* Ri, F and G of the recipe from normalVelocity, layerThickness and the buoyancy tracer of time level 0 (previous) or 1 (current),
 * synchronously and without a step, by the kernels the step launches (their instances that also store Ri): any of the four outputs may
 * be NULL; rows no interface reaches come back 0.0.  MOKA_ERR_UNSUPPORTED while the closure is off (it names the buoyancy tracer and
 * the parameters). */
int  moka_richardson_diagnose(moka_state *st, int time_level, double *riEdge, double *riCell, double *viscEdge, double *diffCell);

/* ---- reverse mode of passive tracer transport over a frozen flow (extension) ---------------------------------------
 * Once the flow is given the tracer step above is linear in phi, so d J(phi_N) / d phi_0 is the exact transpose of a linear map.  It
 * needs no adjoint of the dycore, only the provisional states the step forms anyway, and therefore works over the linear, nonlinear,
 * Del2 and Del4 dycores alike.  A handle of its own, separate from moka_tape: moka_tape_create still refuses a state with tracers, and
 * moka_set_tracers a state with a tape of either kind.
 * Notation as above: a = (dt/2, dt/2, dt), b = (dt/6, dt/3, dt/3, dt/6); P_s = (pu_s, ph_s), s = 0..3, the provisional states the four
 * stage launches read (ph_0 = h_cur); hn the new level's thickness; kappa_j the diffusivities in force during the step; sdv, dvdc,
 * invArea and the skip rules (empty slots, slots with k >= maxLevelEdgeTop[e]) those of the forward scheme; c' the cell across slot i.
 * The transposed tendency r = R(P, y) at (k, c) of a field y accumulates from 0.0 over the slots i of edgesOnCell in slot order, one
 * rounding per operation, no contraction:
 *   hE = 0.5 * (ph[k,c] + ph[k,c']);  F = pu[k,e] * hE                  (the forward bits)
 *   r += ((0.5 * F) * sdv[c,i]) * (y[k,c] - y[k,c'])
 *   with diffusion, a second, separate addition:   r += ((kappa_j * hE) * dvdc[c,i]) * (y[k,c'] - y[k,c])
 * -- sdv of the edge seen from c' is -sdv[c,i] and the mask belongs to the edge, so the transposed scatter folds into the difference
 * y[c] - y[c'] with y = w * invArea; the diffusion operator is self-adjoint under the area weight.  A gather over the forward stencil:
 * the forward launch's traffic, no atomics.
 * Biharmonic diffusion is self-adjoint under the area weight too: the reverse mode applies the same two passes to y.  Per reverse
 * stage s, with the recorded kappa4_j of the step and y carrying invArea already:  M_j = Lap(ph_s, y_j)  (the Laplacian pass above,
 * the same kernel forwards and backwards), and in R(P_s, y), after the harmonic addition of a slot, a third, separate one:
 *   r = r - ((kappa4_j * hE) * dvdc[c,i]) * (M_j[k,c'] - M_j[k,c])
 * Nothing else in the reverse step changes: tau_s, and therefore G below, keep their definitions.  A sweep whose recorded steps all
 * have every kappa4 == 0 launches what it launches without the term.
 * One step backwards, per tracer j and element (k, c); X the adjoint of phi_new, S a scratch field, invA = invArea[c]:
 *   g = X / hn
 *   y = (b[3] * g) * invA
 *   s = 3, 2, 1:   r = R(P_s, y);  v = r / ph_s;  S = (s == 3 ? v : S + v);  y = (b[s-1] * g + a[s-1] * v) * invA
 *   r = R(P_0, y);  X_prev = ph_0 * (g + S) + r
 * X_prev is the adjoint of phi_cur.  The recipe never reads phi.  Hence: a zero seed stays exactly zero; a tracer with kappa_j == 0
 * beside diffused tracers has the bits of the undiffused sweep (adding +-0.0 never changes r, by the forward argument); and a sweep
 * whose recorded steps all have every kappa == 0 launches the instances without diffusion.
 * The result is the gradient with respect to the tracer fields at the start of the first recorded step, the flow held as it ran.
 * Gradient with respect to the sources (moka_tracer_adjoint_want_source_gradient).  Let tau_3 = b[3] * g and, for s = 3, 2, 1,
 * tau_{s-1} = b[s-1] * g + a[s-1] * v: exactly the values the lines above multiply by invA (y = tau * invA keeps its bits; no
 * contraction, no reordering).  tau_s is the adjoint of stage s's tendency and, since T = (slot sum) + q, of q.  Per recorded step, in
 * this order, for every tracer whose gradient is wanted, each addition with its own rounding:
 *   G = G + tau_3  (with g);   G = G + tau_2  (reverse stage 3);   G = G + tau_1  (reverse stage 2);   G = G + tau_0  (reverse stage 1)
 * -- reverse stage 0 does not touch G.  After the sweep G_j = d J / d q_j: the derivative with respect to a source that acts
 * identically in every recorded step, the flow held as it ran.  Hence: G depends neither on the sources the forward run had nor on
 * phi (the tape records nothing new), so two runs that differ only in q give the same G and the same X bit for bit; asking for G
 * changes no bit of X; a zero seed gives G == 0 exactly; and the map is affine in q, so
 *   <X, phi_N(phi_0, q) - phi_N(phi_0, 0)> = <G, q>   up to round-off.
 * Gradient with respect to the mixing coefficients (moka_tracer_adjoint_want_diffusivity_gradient).  The step is linear in phi and
 * affine in (kappa_j, kappa4_j): stage s of tracer j forms T = A(P_s) pphi_s + kappa_j * D_s - kappa4_j * B_s (+ q) with
 *   D_s[k,c] = sum over the slots of ((hE * (pphi_s[k,c'] - pphi_s[k,c])) * dvdc[c,i]) * invArea[c]
 * and B_s the same sum with L_s = Lap(ph_s, pphi_s) in the place of pphi_s.  tau_s above is the adjoint of T, hence
 *   d J / d kappa_j  =   sum over the recorded steps, s = 0..3 and (k, c) of tau_s[k,c] * D_s[k,c]
 *   d J / d kappa4_j = - sum over the recorded steps, s = 0..3 and (k, c) of tau_s[k,c] * B_s[k,c]
 * Two identities make both a dot product of fields the sweep holds: D_s = ph_s * L_s, and, Lap being self-adjoint under the weight
 * areaCell[c] * ph_s[k,c], sum tau_s B_s = sum over (k, c) of areaCell[c] ph_s[k,c] L_s[k,c] M[k,c] with M = Lap(ph_s, y), y = tau_s * invA.
 * A flagged tracer's pphi_0..pphi_3 (pphi_0 = phi_cur) are recorded beside P_s by copies behind the stage launches: 4 * nVertLevels *
 * nCells doubles more per flagged tracer and step.  In the sweep, ahead of each reverse stage rs = 3, 2, 1, 0 (when y holds tau_rs * invA),
 * for the flagged tracers only: L = Lap(ph_rs, pphi_rs) by the Laplacian pass above, M = Lap(ph_rs, y) also for a tracer whose d J / d
 * kappa4 is wanted while its recorded kappa4 is zero (a derivative at zero is legitimate; the reverse stages never read that M), and
 * per element, one rounding per operation, no contraction:
 *   p = ph_rs[k,c] * L[k,c];     dk = p * y[k,c];     dk4 = p * M[k,c]
 * colsum(d)[c], the sum over the column: with LPC the smallest power of two >= nVertLevels, at most 64, partial l = 0..LPC-1 starts
 * at 0.0 and adds d[k,c] for k = l, l + LPC, l + 2 LPC, ... in ascending order; then for o = LPC/2, LPC/4, ..., 1 every partial l
 * becomes partial[l] + partial[l xor o] (all at once); colsum = partial[0].  The order depends on nVertLevels alone.
 * Two sensitivity densities per flagged tracer, nCells doubles each, take one addition per reverse stage, each with its own rounding:
 *   Wk_j[c]  = Wk_j[c]  + areaCell[c] * colsum(dk)[c]
 *   Wk4_j[c] = Wk4_j[c] - areaCell[c] * colsum(dk4)[c]
 * They accumulate over the four stages and over every recorded step, as G does, and are zeroed where G is: at the first seed after a
 * recorded step.  d J / d kappa_j = sum over c of Wk_j[c] and d J / d kappa4_j = sum over c of Wk4_j[c], taken on the host over the
 * caller's cell numbering, ascending, in long double and rounded once: independent of the mesh's cell ordering.  The density shows
 * where J feels the mixing.  The derivative is with respect to a coefficient that acts identically in every recorded step (the values
 * the steps ran with may differ from step to step), the flow held as it ran.  Hence: asking for these changes no bit of X, of G, of the
 * state or of the tracers (the new launches read ph, y and M and write arrays of their own); the tracer that is 1 everywhere stays exactly 1.0, so its L == 0
 * and both its gradients are exactly 0.0; a zero seed gives densities that are exactly zero; an unflagged tracer is neither recorded, read nor written.
 * Usage: tracer_tape_create -> n x step_rk4_tracer_taped -> seed (per tracer) -> sweep -> download (per tracer).
 * Out of scope: sensitivities of the tracers to the flow (d phi_N / d (u, h)), a spatially varying or time-dependent kappa and a
 * per-step split of its gradient, second derivatives, time-dependent sources and a per-step
 * split of G, coupling to moka_tape, Forward Euler, partitioned meshes, fp32 storage. */
typedef struct moka_tracer_tape moka_tracer_tape;
/* MOKA_ERR_UNSUPPORTED on a state without tracers, MOKA_ERR_ARG for NULL arguments or a negative capacity.  The tape remembers the
 * state's tracer count and counts as a tape of the state: while it lives, moka_state_optimize_placement and moka_set_tracers(st, n > 0)
 * refuse.  K * (4 nEdges + 5 nCells) doubles per step of capacity (the four P_s and hn), nTracers more for the diffusivities, nTracers
 * for the biharmonic coefficients and nTracers for the vertical diffusivities, and six work arrays of nTracers * K * nCells doubles (the sixth holds M).
 * A tracer flagged by moka_tracer_adjoint_want_vertical_gradient adds K * nCells doubles per step of capacity (its phi_new) and one
 * K * nCells density; that call allocates them, not this one.  State and tape may be destroyed in either order. */
int  moka_tracer_tape_create(moka_state *st, int64_t capacity_steps, moka_tracer_tape **out);
void moka_tracer_tape_destroy(moka_tracer_tape *t);
/* exactly moka_step_rk4 on the tape's state -- state and tracers end up bit for bit as after the untaped call -- with P_0..P_3, hn and
 * the diffusivities and biharmonic coefficients recorded by copies behind the stage launches (and phi_new of the tracers flagged for the vertical gradient).  MOKA_ERR_ARG when the tape is full or the state's tracer count is no
 * longer the tape's.  A recorded step un-seeds the tape. */
int  moka_step_rk4_tracer_taped(moka_tracer_tape *t, double dt);
int  moka_tracer_tape_steps(const moka_tracer_tape *t, int64_t *n);                /* recorded and not yet reversed */
/* X_j := host, (nVertLevels, nCells) doubles in the caller's numbering like moka_tracer_upload; NULL = zeros.  The first seed after a
 * recorded step zeroes the other tracers' X.  MOKA_ERR_ARG for j out of range. */
int  moka_tracer_adjoint_seed(moka_tracer_tape *t, int32_t j, const double *host);
/* reverse over (and pop) every recorded step; the tape is then empty and reusable.  MOKA_ERR_ARG when unseeded. */
int  moka_tracer_adjoint_sweep(moka_tracer_tape *t);
int  moka_tracer_adjoint_download(moka_tracer_tape *t, int32_t j, double *host);    /* X_j as it stands */
/* which kernel served the last reverse stage: 1 the patch form, 2 the generic form (the conditions of moka_state_tracer_path), 0 none yet */
int  moka_tracer_adjoint_path(const moka_tracer_tape *t);
/* which kernel served the vertical pass of the last reverse step that had one: as moka_state_tracer_vmix_path; 0 none yet.  A sweep whose
 * recorded steps all have every kappaV == 0 launches what it launches without the term.  While a tracer is flagged for the vertical
 * gradient the pass runs in every reversed step with nVertLevels >= 2 and dt != 0.0, also one whose kappaV are all zero, and its
 * gradient instances keep four column sets in LDS: the tile form then serves nVertLevels <= 79, the column form deeper columns. */
int  moka_tracer_adjoint_vmix_path(const moka_tracer_tape *t);
/* on != 0: the next sweeps also accumulate G_j (algebra above); 0: they no longer do (the accumulator stays readable).  May be called
 * whenever the tape is not between a seed and its sweep (MOKA_ERR_ARG there, and for j out of range); the first call for a tracer
 * allocates its (nVertLevels, nCells) accumulator.  The first seed after a recorded step zeroes every G, as it zeroes X.  A sweep in
 * which no gradient is wanted launches the kernels of a tape that never asked for one. */
int  moka_tracer_adjoint_want_source_gradient(moka_tracer_tape *t, int32_t j, int on);
/* G_j as it stands, in the caller's cell numbering; MOKA_ERR_ARG for j out of range, a NULL host, or a tracer that was never flagged */
int  moka_tracer_adjoint_source_download(moka_tracer_tape *t, int32_t j, double *host);
/* Gradient with respect to kappa_j and kappa4_j (algebra above).  what: a nonempty set of the two bits; on != 0 adds them to tracer
 * j's set, 0 removes them.  Only while the tape holds no recorded step and is not between a seed and its sweep: MOKA_ERR_ARG there, for
 * j out of range and for an empty or unknown `what`.  moka_tracer_tape_create sizes nothing for this: a call that changes the set of
 * flagged tracers allocates the record of their provisional tracers (capacity * 4 * nVertLevels * nCells doubles each), one scratch
 * field and two densities per flagged tracer -- MOKA_ERR_ALLOC, with nothing changed, when that fails -- and drops what earlier
 * sweeps accumulated.  While any tracer is flagged moka_step_rk4_tracer_taped records more (state and tracers keep their bits) and the
 * sweep has up to three more launches per reverse stage; a tape without a flag records, allocates and launches what it always did. */
enum { MOKA_TRACER_GRAD_KAPPA = 1, MOKA_TRACER_GRAD_KAPPA4 = 2 };
int  moka_tracer_adjoint_want_diffusivity_gradient(moka_tracer_tape *t, int32_t j, int what, int on);
/* what: exactly one bit.  *out = d J / d kappa_j (d J / d kappa4_j) as the densities stand; host: the density itself, nCells doubles in
 * the caller's cell numbering.  MOKA_ERR_ARG for j out of range, NULL arguments, a `what` that is not one bit, and a tracer or bit
 * that is not flagged. */
int  moka_tracer_adjoint_diffusivity_gradient(moka_tracer_tape *t, int32_t j, int what, double *out);
int  moka_tracer_adjoint_diffusivity_density_download(moka_tracer_tape *t, int32_t j, int what, double *host);
/* Gradient with respect to kappaV_j (algebra at moka_set_tracer_vertical_diffusion).  on != 0 flags tracer j, 0 unflags it.  Only while
 * the tape holds no recorded step and is not between a seed and its sweep: MOKA_ERR_ARG there and for j out of range.  A call that
 * changes the flagged set allocates each flagged tracer's record of phi_new (capacity * nVertLevels * nCells doubles) and its D --
 * MOKA_ERR_ALLOC, with nothing changed, when that fails -- and drops what earlier sweeps accumulated.  While any tracer is flagged
 * moka_step_rk4_tracer_taped copies each flagged tracer's new-level field behind the step (state and tracers keep their bits), and a
 * reversed step runs the gradient instances of the vertical pass for all its tracers: an unflagged tracer with kappaV != 0 takes the
 * plain reverse column, a flagged one with kappaV == 0 the gradient alone, an unflagged one with kappaV == 0 is skipped.  A tape
 * without a flag records, allocates and launches what it always did. */
int  moka_tracer_adjoint_want_vertical_gradient(moka_tracer_tape *t, int32_t j, int on);
/* *out = d J / d kappaV_j as D_j stands (the scalar view).  MOKA_ERR_ARG for NULL arguments, j out of range or a tracer that is not
 * flagged; a flagged tracer that has not been swept reads zero. */
int  moka_tracer_adjoint_vertical_gradient(moka_tracer_tape *t, int32_t j, double *out);
/* host: D_j itself, (nVertLevels, nCells) doubles (MOKA_VGRAD_INTERFACE), Wv_j, nCells doubles (MOKA_VGRAD_CELL), or Pv_j, nVertLevels
 * doubles (MOKA_VGRAD_PROFILE), in the caller's cell numbering.  MOKA_ERR_ARG as above and for an unknown view. */
enum { MOKA_VGRAD_INTERFACE = 0, MOKA_VGRAD_CELL = 1, MOKA_VGRAD_PROFILE = 2 };
int  moka_tracer_adjoint_vertical_density_download(moka_tracer_tape *t, int32_t j, int view, double *host);

/* ---- reverse mode of the Forward-Euler loop ----------------------------------------------------------------
 * The reference gets d sum(ssh^2) / d (initial normalVelocity, layerThickness) from Enzyme over ocn_run_loop
 * (ext/MPASEnzymeExt.jl, test/enzyme/test_Enzyme_end2end.jl:62-96; on CUDA it yields NaNs there, :183-186).
 * Here: a tape of the forward values each step's transpose needs, and hand-written transposed kernels in gather
 * form (no atomics).  Float64 states on whole (unpartitioned) meshes; flags without MOKA_FE_LEVEL1_ONLY unless
 * nVertLevels = 1.  Usage: tape_create -> n x step_fe_taped -> seed -> sweep -> download. */
typedef struct moka_tape moka_tape;
int  moka_tape_create(moka_state *st, int64_t capacity_steps, moka_tape **out);   /* 2*K*nEdges doubles per step */
void moka_tape_destroy(moka_tape *t);
int  moka_step_fe_taped(moka_tape *t, double dt, int flags);                        /* records, then moka_step_fe */
/* RK4 (time_integration.jl:61-148): records the four provisional states, 4*K*(nEdges+nCells) doubles per step.
 * One integrator per tape.  The RK4 map's state is (normalVelocity, layerThickness): the ssh gradient is zero. */
int  moka_step_rk4_taped(moka_tape *t, double dt);
/* lambda := d sum(ssh^2) / d state at the current state (the objective of run_loop.jl:26-45) */
int  moka_adjoint_seed_sum_sq_ssh(moka_tape *t);
int  moka_adjoint_sweep(moka_tape *t);                                              /* reverse over (and pop) every recorded step */
/* Reverse mode of a PARTITIONED RK4 run (one rank's part; the host layer moves the halo rows between the calls):
 *   taping   -- the caller runs the distributed step itself and records, halo rows included, the four provisional states:
 *               slot 0 := the current level before the step (what = 0), slot s := the output of stage s after its exchange
 *               (what = s = 1..3); moka_tape_commit_rk4 closes the step.
 *   reversal -- per recorded step, for sg = 4, 3, 2, 1: exchange the halo rows of the fields moka_adjoint_rk4_stage_fields
 *               names (moka_halo_pack_fields / unpack_fields; sg = 4: the adjoint state itself), then moka_adjoint_rk4_stage.
 * The transposed lists are sorted by the caller's edge ids: a local mesh whose edges keep the order of their global ids
 * (moka_hip.parallel.build_local) reproduces the single-domain sums bit for bit. */
int  moka_tape_record_rk4(moka_tape *t, int slot, int what);
int  moka_tape_commit_rk4(moka_tape *t, double dt);
int  moka_adjoint_rk4_stage_fields(moka_tape *t, int stage, void **fieldU, void **fieldH, void **scratchS);
int  moka_adjoint_rk4_stage(moka_tape *t, int stage);
/* ... and with the exchange overlapped: moka_adjoint_rk4_stage_part(t, sg, 0) transposes the entities of the boundary cell class
 * (what other ranks gather from), the caller starts the exchange of the rows that produced (moka_adjoint_rk4_stage_out_fields names
 * the arrays stage sg writes for the next transposed stage; after sg = 1: the adjoint state itself), part 1 = the interior class
 * runs meanwhile (owned rows only), then the exchange completes.  Halo entities are not computed.  Chunk kernels only
 * (even 34 <= nVertLevels <= 64), MOKA_ERR_UNSUPPORTED otherwise. */
int  moka_adjoint_rk4_stage_part(moka_tape *t, int stage, int part);
int  moka_adjoint_rk4_parts_available(const moka_tape *t);   /* 1: moka_adjoint_rk4_stage_part serves this tape's mesh */
int  moka_adjoint_rk4_stage_out_fields(moka_tape *t, int stage, void **fieldU, void **fieldH, void **scratchS);
/* Forward-Euler runs on a partitioned mesh: record before (after = 0) and behind (after = 1) the distributed step, commit;
 * reversal per recorded step: exchange the halo rows of the three fields moka_adjoint_fe_step_fields names (the adjoints of
 * normalVelocity, layerThickness and ssh; that of the carried layerThicknessEdge needs none), then moka_adjoint_fe_step. */
int  moka_tape_record_fe(moka_tape *t, int flags, int after);
int  moka_tape_commit_fe(moka_tape *t, double dt, int flags);
int  moka_adjoint_fe_step_fields(moka_tape *t, void **fieldU, void **fieldH, void **fieldS);
int  moka_adjoint_fe_step(moka_tape *t);
/* field: MOKA_F_SSH, MOKA_F_NORMAL_VELOCITY, MOKA_F_LAYER_THICKNESS (d_Prog of the reference test) or
 * MOKA_F_LAYER_THICKNESS_EDGE (the carried diagnostic of the reference_compat sequence); caller's numbering */
int  moka_adjoint_download(moka_tape *t, int field, double *host);

/* ---- reverse mode through the forced RK4 step: gradients of wind stress, viscosity and drag (extension) -------------------
 * A handle of its own, separate from moka_tape, which keeps every answer it gave (it still refuses a state whose vertical momentum
 * pass is on, and the pass setters a state that has one).  A moka_forced_tape records RK4 steps of a Float64 state on a whole mesh
 * with the linear dycore, the pass on or off, and its sweep runs, per recorded step backwards, first the transposed pass and then the
 * four transposed RK stages of moka_adjoint_sweep (the same launches).
 * The transposed pass.  Notation of the forward recipe (moka_set_vertical_viscosity): for an edge column of depth n, h[k] = 0.5 *
 * (hn[k,c1] + hn[k,c2]) from the recorded new thickness hn, un the recorded mixed velocity, s = dt * nuV, q = dt * r, b = dt * tau[e]
 * (the step's values), A = diag(h) + s W + q e_{n-1} e_{n-1}^T, symmetric.  Differentiating A(h) u_new = h o u* + b e_0, and using
 * h o (u_new - u*) = R(u_new), which holds exactly, gives, with X = (XU, XH) the adjoint of (u_new, h_new), every operation rounded once,
 * nothing contracted, in this order:
 *   z      = Solve_A(XU[0..n-1])              w, d, and the sweep (g = w[k-1] / beta, beta = d[k] - w[k-1] * g, y = (XU[k] + w[k-1] * y)
 *                                             / beta; z[k] = y[k] + g[k] * z[k+1]) exactly as the forward pass forms them; n == 1: XU[0] / d[0]
 *   then for k = 0 .. n-1 ascending, hm[k] = 0.5 * (h[k] + h[k+1]), w[k] = s / hm[k]:
 *   de[k]  = (z[k] - z[k+1]) * (un[k] - un[k+1]);   P[k] = (w[k] / hm[k]) * de[k]                       k = 0 .. n-2
 *   Rn     = R(un): w[k-1] * (un[k-1] - un[k]) + w[k] * (un[k+1] - un[k]) (end rows: the one term; n == 1: 0.0), then + b in row 0
 *            with a stress, then - q * un[n-1] in row n-1 with drag: the forward's right-hand side formed from x := un
 *   hbar[k]= 0.5 * (P[k-1] + P[k]) - z[k] * (Rn[k] / h[k])      (end rows: 0.5 * the one P; n == 1: 0.0 - z[0] * (Rn[0] / h[0]))
 *   XU[k]  = h[k] * z[k]                                         the adjoint of u*
 * and then, per cell c and level k, S = 0.0; for the slots i of edgesOnCell[c] in ascending order whose edge e is a computed column
 * with k < n_e: S = S + hbar[k,e]; when at least one slot took part: XH[k,c] = XH[k,c] + 0.5 * S (a gather: no atomics; rows of hbar at
 * or below an edge's depth are never read).
 * Computed columns are exactly those the forward pass computed in that step (n >= 2, or n == 1 with drag or stress; none in a step
 * that ran without the pass); every other element of XU and XH keeps its bits.  A step recorded with dt == 0.0 skips the pass both ways.
 * Parameter sensitivities (moka_forced_adjoint_want_gradient): three densities of nEdges doubles take, per reversed step with
 * dt != 0.0 and per edge with n >= 1, each operation rounded once:
 *   G_tau[e] = G_tau[e] + dt * z[0]
 *   D_nu[e]  = D_nu[e]  - dt * sum,   sum = 0.0; sum = sum + de[k] / hm[k] for k = 0 .. n-2 ascending   (n == 1: D_nu[e] is left alone)
 *   D_r[e]   = D_r[e]   - dt * (z[n-1] * un[n-1])
 * While any is flagged, z is also computed in the columns with n >= 1 the forward pass skipped -- n == 1 with only nuV on, and every
 * column of a step that ran without the pass, where A = diag(h) and the result is the derivative at zero -- for the densities alone:
 * such a column writes neither XU nor hbar, so X after a flagged sweep has the bits of an unflagged one.  d J / d nuV = sum_e D_nu[e]
 * and d J / d r = sum_e D_r[e], summed on the host over the caller's edge numbering, ascending, in long double and rounded once; G_tau
 * itself is d J / d tau_e for a stress that acts in every recorded step.  The densities show where J feels each parameter.  Every
 * seed zeroes them.
 * Kernels: the edge columns run in the forward's two forms with one device function behind both -- the tile form with four column
 * sets in LDS (vmix_kernel(K, generic, 4): tiles of 64 columns for nVertLevels <= 19, of 32 for <= 79), the column form deeper, for
 * nVertLevels == 1 and with kernel variant 3 -- then the cell gather.  Both forms and the numpy twin of the tests agree bit for bit.
 * The tape: moka_step_rk4_forced_taped leaves state and diagnostics with the bits of moka_step_rk4 and records what
 * moka_step_rk4_taped records; when the pass is on in that step, or any gradient is flagged, also u_new and h_new (K * (nEdges +
 * nCells) doubles more) and the step's nuV, r and whether the stress was on.  Allocations happen at create (those of moka_tape_create),
 * at the first taped step (those of moka_step_rk4_taped; with the first step that records the new level, capacity * K * (nEdges + nCells)
 * + 3 * K * nEdges doubles more) and at moka_forced_adjoint_want_gradient (nEdges doubles a bit); MOKA_ERR_ALLOC leaves nothing changed.
 * MOKA_ERR_UNSUPPORTED at create: fp32 storage, the nonlinear terms, tracers, a state with a halo, a partitioned mesh, an existing
 * moka_tape or moka_forced_tape.  While a forced tape exists moka_tape_create, moka_set_tracers(st, n > 0), moka_set_nonlinear,
 * moka_halo_create and moka_state_optimize_placement return MOKA_ERR_UNSUPPORTED; moka_set_vertical_viscosity is allowed at any time
 * (the values are recorded per step); moka_surface_stress_upload returns MOKA_ERR_UNSUPPORTED while the tape holds recorded steps (the
 * reverse pass reads the stress the steps ran with, and G_tau is the gradient of one stress field).  MOKA_ERR_ARG: dt < 0 with the pass
 * on, a full tape, NULL arguments, a sweep without a seed, a `what` that is not flagged (or not one bit where one is asked for),
 * moka_forced_adjoint_want_gradient with recorded steps.  The state must outlive the tape.
 * Usage: forced_tape_create -> [want_gradient] -> n x step_rk4_forced_taped -> seed -> sweep -> download / density_download / gradient.
 * Out of scope: the nonlinear, Del2 and Del4 dycores (no moka_tape covers them either), Forward Euler, the piecewise, partitioned
 * taping calls, fp32 storage, a time-dependent stress and a per-step split of the densities, second derivatives, the quadratic drag
 * on a tape of this call (moka_forced_tape_create and moka_step_rk4_forced_taped return MOKA_ERR_UNSUPPORTED while Cd != 0, and
 * moka_set_quadratic_bottom_drag refuses a nonzero Cd while such a tape exists: moka_forced_tape_create_quadratic, below, is the tape
 * that carries it), coupling to the tracer tape, the 13-stream form for taped steps, YAML keys and NetCDF I/O. */
typedef struct moka_forced_tape moka_forced_tape;
int  moka_forced_tape_create(moka_state *st, int64_t capacity_steps, moka_forced_tape **out);
void moka_forced_tape_destroy(moka_forced_tape *t);
int  moka_step_rk4_forced_taped(moka_forced_tape *t, double dt);
/* X := d sum(ssh^2) / d (normalVelocity, layerThickness) at the current state, as moka_adjoint_seed_sum_sq_ssh for an RK4 tape */
int  moka_forced_adjoint_seed_sum_sq_ssh(moka_forced_tape *t);
/* X := the caller's (nEdges, nVertLevels) and (nCells, nVertLevels) doubles, caller's numbering */
int  moka_forced_adjoint_seed(moka_forced_tape *t, const double *hostU, const double *hostH);
int  moka_forced_adjoint_sweep(moka_forced_tape *t);            /* reverse over (and pop) every recorded step */
/* field: MOKA_F_NORMAL_VELOCITY or MOKA_F_LAYER_THICKNESS; X as it stands */
int  moka_forced_adjoint_download(moka_forced_tape *t, int field, double *host);
enum { MOKA_FORCED_GRAD_STRESS = 1, MOKA_FORCED_GRAD_VISCOSITY = 2, MOKA_FORCED_GRAD_DRAG = 4 };
/* what: a nonempty set of the bits; on != 0 adds them, 0 removes them.  Only while no step is recorded. */
int  moka_forced_adjoint_want_gradient(moka_forced_tape *t, int what, int on);
/* what: exactly one flagged bit.  host: the density, nEdges doubles in the caller's edge numbering; *out: the host sum (for
 * MOKA_FORCED_GRAD_STRESS: the sum of G_tau, the derivative with respect to a uniform offset of the stress) */
int  moka_forced_adjoint_density_download(moka_forced_tape *t, int what, double *host);
int  moka_forced_adjoint_gradient(moka_forced_tape *t, int what, double *out);
/* which kernel served the last transposed pass: 1 the tile form, 2 the column form, 0 none yet */
int  moka_forced_tape_vmix_path(const moka_forced_tape *t);
/* The viscosity field in reverse mode.  A step recorded while a field (moka_vertical_viscosity_field_upload) was in force is
 * reversed with that field: w[k] = s[k] / hm[k], s[k] = dt * f[k,e], in both places where the transposed recipe forms w -- the
 * elimination, and the ascending P / Rn lines; everything else is as written above.  G_tau, D_r and D_nu keep their formulas, with z
 * from the field's solve; with a field in force D_nu and its host sum are the directional derivative along the all-ones field.
 * The density DF (flagged by moka_forced_adjoint_want_viscosity_field_gradient, a call of its own: `what` of
 * moka_forced_adjoint_want_gradient keeps its three bits) has the layout of the field.  Per reversed step with dt != 0.0, per edge
 * with n >= 2 and per k = 0 .. n-2, each operation rounded once:
 *   DF[k,e] = DF[k,e] - dt * (de[k] / hm[k])
 * Rows k >= n_e - 1 of DF are never written: they keep the zeros of the seed.  DF[k,e] is d J / d f[k,e] for a field that acts in
 * every recorded step; at a scalar nuV it is the sensitivity to a depth-dependent viscosity at the uniform value the run used, and
 * sum_k DF[k,e] equals D_nu[e] up to the order of summation; without the pass it is the derivative at zero.  As for the other
 * densities, columns the forward pass skipped are then solved for the densities alone and write neither XU nor hbar: X after a sweep
 * with DF flagged has the bits of an unflagged one.  The flag may change only while no step is recorded (MOKA_ERR_ARG otherwise);
 * the first flag allocates nVertLevels * nEdges doubles; a download without the flag is MOKA_ERR_ARG; every seed zeroes DF.
 * Tape: moka_step_rk4_forced_taped keeps a device copy of the field a step ran with -- nVertLevels * nEdges doubles, taken device
 * to device on the context's stream ahead of the step's first launch, and only when the field was uploaded or removed since the
 * tape's newest copy.  The copies are released when a sweep has emptied the tape and when the tape is destroyed.  Unlike the stress,
 * a field upload is therefore allowed while steps are recorded.  A tape whose steps never saw a field and never flags DF allocates,
 * records and launches what it did before.
 * Kernels: steps recorded with a field run the FIELD instances, which keep f in a fifth column set for the whole column
 * (vmix_kernel(K, generic, 5): tiles of 64 columns for nVertLevels <= 15, of 32 for <= 63 -- 81,152 bytes at most -- the column form
 * from 64); steps recorded without one keep the four-set instances and their boundary at 79 / 80, with DF flagged or not.
 * moka_forced_tape_vmix_path reports the form that ran.  DF in the tile form: the lane leaves dt * (de[k] / hm[k]) in the slot of h[k],
 * free by then, and the rows k < n - 1 of every solved column are taken off the tile's span of DF, coalesced; in the column form the
 * lane updates its own rows k < n - 1.  No other row of DF is read or written.  Both forms and the numpy twin agree bit for bit.
 * host: (nEdges, nVertLevels) doubles in the caller's numbering. */
int  moka_forced_adjoint_want_viscosity_field_gradient(moka_forced_tape *t, int on);
int  moka_forced_adjoint_viscosity_field_density_download(moka_forced_tape *t, double *host);
/* The quadratic bottom drag in reverse mode.  moka_forced_tape_create_quadratic behaves as moka_forced_tape_create, every refusal
 * included (a halo, a partitioned mesh, an existing moka_tape or moka_forced_tape, fp32 storage, the nonlinear terms, tracers), except
 * that it accepts a state with any Cd and marks the tape "quadratic": moka_step_rk4_forced_taped on it accepts Cd != 0 and records
 * the step's Cd beside nuV and r, so Cd may change between recorded steps, and moka_set_quadratic_bottom_drag accepts a nonzero Cd
 * beside it (a state has at most one forced tape: the setter refuses beside a plain one, with the error text it always had).  A
 * quadratic tape on a state whose Cd stays 0, without the flag below, allocates, records and launches what a plain one does.
 * The transposed recipe, for a recorded step with Cd != 0 and dt != 0.0, notation as above, us the recorded u*, sp the recorded
 * bottom speed of the step, kb_e = n_e - 1, every operation rounded once, nothing contracted, in this order:
 *   q_e    = dt * (r + Cd * sp[e])            the forward's expression on the recorded sp: its bits; it stands for q in d[n-1] and Rn[n-1],
 *                                             and the drag lines are on whatever r is (every column with n >= 1 is a computed column)
 *   z, hbar, XU, the cell gather, G_tau, D_nu, D_r, DF   as written above, with q_e
 *   t      = z[n-1] * un[n-1]                 once per column, n == 1 included                    (q-bar_e = -t)
 *   M[e]   = (0.0 - (dt * Cd) * t) / sp[e]    where sp[e] > 0, else 0.0;  0.0 for edges with n == 0   (sp-bar_e / sp_e)
 * and then, per edge e' with n' = n_e' >= 1 and per level k that is the bottom level kb_e of some edge e in a slot of edgesOnCell of
 * c1 or c2 of e' with n_e >= 1 and kb_e < n':
 *   a_j    = 0.0; for the slots i of cell c_j in ascending order with kb_e == k: a_j = a_j + M[e]            j = 1, 2
 *   g      = a_1 * invArea[c1] + a_2 * invArea[c2]
 *   XU[k,e'] = XU[k,e'] + (kc[e'] * us[k,e']) * g
 * which is the transpose of the bottom-speed stencil: sp_e^2 = KE_c1[kb_e] + KE_c2[kb_e] has d sp_e / d u*[k,e'] = kc[e'] u*[k,e']
 * (invArea[c1] [e' in c1] + invArea[c2] [e' in c2]) / sp_e for k == kb_e < n_e'.  The edge e' sits in both its cells' slot lists and
 * is counted in both, as in the forward.  sp does not depend on h: XH gets no new term.  sp_e == 0 is the kink of the square root,
 * where the speed has no derivative: M[e] = 0.0 there, the subgradient that keeps a resting bottom layer at rest; with it a state
 * whose bottom flow is exactly zero gives XU the bits of the linear-drag transpose with r alone.  Rows k >= n_e' of XU and us are
 * never read or written, and M and us of a slot that fails the test are not read: NaN there does not travel.
 * The density of Cd (moka_forced_adjoint_want_quadratic_drag_gradient, a call of its own: `what` of
 * moka_forced_adjoint_want_gradient keeps its three bits; MOKA_ERR_UNSUPPORTED on a tape of moka_forced_tape_create, MOKA_ERR_ARG with
 * recorded steps; the first flag allocates nEdges doubles and uploads kc where the mesh has not): per reversed step with dt != 0.0
 * and per edge with n >= 1,
 *   D_cd[e] = D_cd[e] - (dt * t) * sp[e]
 * also in steps recorded with Cd == 0, where q = dt * r, the switches are the step's own, no M is formed and the stencil's
 * transpose is not launched: the derivative at zero.  As for the other densities, the columns the forward pass skipped are then
 * solved for the density alone.  d J / d Cd = sum_e D_cd[e], summed as the other scalar gradients are; every seed zeroes D_cd.
 * The tape records, device to device on the state's stream: sp (nEdges doubles) of a step with Cd != 0 -- a copy of the sp the pass
 * used -- or with the flag set -- then moka's bottom-speed launch runs on u* straight into the tape's record and writes no state
 * memory; and u* (nVertLevels * nEdges doubles) of a step with Cd != 0, taken between stage 4 and the pass.  Each array is allocated
 * by the first step that needs it, ahead of that step's first launch: capacity * (nVertLevels + 1) * nEdges doubles more than a
 * plain tape in all, and nEdges for M.
 * Kernels: the transposed pass runs QD instances of its two forms (M and sp are per-lane scalars: tiles, LDS, the 79 / 80 and 63 / 64
 * boundaries and the path values do not change); the stencil's transpose is a gather with the bottom-speed kernel's shape, one lane
 * per edge e', the grouping by level a predicate scan in registers, distinct levels distinct elements of the lane's own column: no
 * atomics, one summation order; any nVertLevels, any maxEdges, every kernel variant.  Both forms and the numpy twin agree bit for bit.
 * host: nEdges doubles in the caller's numbering; *out: the host sum.  A download or gradient without the flag is MOKA_ERR_ARG.
 * Out of scope: a Cd field, a per-step split of the density, second derivatives, a smoothed square root at sp == 0. */
int  moka_forced_tape_create_quadratic(moka_state *st, int64_t capacity_steps, moka_forced_tape **out);
int  moka_forced_adjoint_want_quadratic_drag_gradient(moka_forced_tape *t, int on);
int  moka_forced_adjoint_quadratic_drag_density_download(moka_forced_tape *t, double *host);
int  moka_forced_adjoint_quadratic_drag_gradient(moka_forced_tape *t, double *out);
/* how many device arrays the handle owns itself (those of the moka_tape it embeds not counted), 0 for NULL: what the lazy allocations
 * above can be checked by -- a quadratic tape whose steps saw no Cd and no flag reports what a plain one does */
int64_t moka_forced_tape_device_arrays(const moka_forced_tape *t);

#ifdef __cplusplus
}
#endif
#endif /* MOKA_HIP_H */
