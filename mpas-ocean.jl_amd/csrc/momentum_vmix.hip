// momentum_vmix.hip -- implicit vertical mixing of momentum with a surface stress and a linear and a quadratic bottom drag (gfx950;
// moka_set_vertical_viscosity / moka_surface_stress_upload / moka_set_quadratic_bottom_drag, NOT in the reference): one tridiagonal
// solve per edge column behind stage 4 of an RK4 step, on the new normalVelocity over the new layerThickness, the bottom speed of the
// quadratic drag gathered by a launch in front of it.  Second half of the file: the transpose of that pass for
// moka_forced_tape (reverse mode through the forced step), in the same two forms, the cell gather of its thickness terms, and the
// transpose of the bottom-speed stencil for a tape that carries the quadratic drag.
#include "kernels_common.hpp"
#include "mvmix_index.hpp"

namespace moka {

// ------------------------------------------------------------------------------------------------
// include/moka_hip.h states the recipe; this is it, once, for one edge column of n = min(maxLevelEdgeTop[e], K) >= 1 active levels,
// s = dt * nuV, q = dt * bottomDrag, b = dt * tau[e], h[k] = 0.5 * (h_new[k,c1] + h_new[k,c2]):
//     w[k] = s / (0.5 * (h[k] + h[k+1]));   d[k] = (h[k] + w[k-1]) + w[k]  (end rows: one w);   DRAG: d[n-1] = d[n-1] + q
//     R = Lv(x);   STRESS: R[0] = R[0] + b;   DRAG: R[n-1] = R[n-1] - q * x[n-1];   u_new = x + Solve(R)
// with Solve and Lv those of the tracer pass (tracer_vmix.hip).  Every operation is rounded once (-ffp-contract=off), in the order
// written in the header, so the two forms below and the numpy twin of the tests agree bit for bit.  DRAG and STRESS are compile-time
// switches chosen per launch (wave-uniform): an instance without them holds none of their operations, not added zeros.
// One lane owns one column; the accessor C hides where it keeps it:
//     h(k), x(k)             the edge thickness and u*, read once each, in ascending k
//     putG / g, putY / y     the sweep's two work columns
//     emit(k, inc)           u[k] = u[k] + inc
//     s(k)                   FIELD only: dt * f[k,e], read once, before putY(k) (the tile keeps f in the set y overwrites)
// n == 1 (instances with DRAG or STRESS only): y[0] = R[0] / d[0] with d[0] = h[0] (+ q) and R[0] = 0.0 (+ b) (- q * x[0]).
// Levels k >= n are never touched.  FIELD (moka_vertical_viscosity_field_upload): s[k] = dt * f[k,e] per interface k <= n - 2 in place
// of the one s; rows k >= n - 1 of f are never read.  An instance without it is the scalar one, operation for operation.
// ------------------------------------------------------------------------------------------------
template <bool DRAG, bool STRESS, bool FIELD, class C>
__device__ __forceinline__ void mvmix_column(C &c, const int n, const double s, const double q, const double b)
{
    double hk = c.h(0), xk = c.x(0);
    if (n == 1) {
        double d = hk, r = 0.0;
        if (DRAG) d = d + q;
        if (STRESS) r = r + b;
        if (DRAG) r = r - q * xk;
        c.emit(0, r / d);
        return;
    }
    double hn = c.h(1), xn = c.x(1), xm = 0.0;
    double w = (FIELD ? c.s(0) : s) / (0.5 * (hk + hn));      // w[0]
    double beta = hk + w;                           // d[0]
    double r = w * (xn - xk);
    if (STRESS) r = r + b;
    double y = r / beta;
    c.putY(0, y);
    for (int k = 1; k < n; ++k) {
        const double wp = w;                        // w[k-1]
        xm = xk; xk = xn; hk = hn;
        const double g = wp / beta;
        c.putG(k - 1, g);
        double d;
        if (k < n - 1) {
            hn = c.h(k + 1); xn = c.x(k + 1);
            w = (FIELD ? c.s(k) : s) / (0.5 * (hk + hn));
            d = (hk + wp) + w;
            r = wp * (xm - xk) + w * (xn - xk);
        } else {
            d = hk + wp;
            if (DRAG) d = d + q;
            r = wp * (xm - xk);
            if (DRAG) r = r - q * xk;
        }
        beta = d - wp * g;
        y = (r + wp * y) / beta;
        c.putY(k, y);
    }
    double z = y;                                   // z[n-1]
    c.emit(n - 1, z);
    for (int k = n - 2; k >= 0; --k) {
        z = c.y(k) + c.g(k) * z;
        c.emit(k, z);
    }
}

// the active depth of an edge column as a launch sees it: 0 = the column is left alone (and its cells are not read)
template <bool DRAG, bool STRESS>
__device__ __forceinline__ int mvmix_depth(const int mlt, const int K)
{
    const int n = min(mlt, K);
    return n >= 2 || (n == 1 && (DRAG || STRESS)) ? n : 0;
}

// ------------------------------------------------------------------------------------------------
// Form 1, tile.  A workgroup of one wave takes te consecutive edges (device numbering): their te * K doubles of u are one contiguous
// span, staged as the tracer tile stages a field -- 16-byte lanes, MV_U loads in flight per lane -- into set 1 of three column sets in
// LDS, a column cs = K | 1 doubles apart (odd: the lanes of a ds_read_b64 / ds_write_b64 group hit distinct banks):
//     set 0: h_e, its slot k taking g[k] once h[k] and h[k+1] sit in registers | set 1: u | set 2: y (FIELD: f, its slot k taking y[k]
//     once s[k] is read -- one more coalesced read of the span, no LDS beyond the scalar tile's)
// Set 0 does not exist as an array: for every element (column, k) of the tile with k < n a lane reads h_new[k,c1] and h_new[k,c2] and
// stores 0.5 * (a + b).  The edges' ehdr records {c1, c2, -, maxLevelEdgeTop} come in with one 16-byte load per edge and stay in LDS
// behind the sets (16 bytes per column, where the tracer tile keeps 4: the tile's LDS is vmix_kernel's plus 12 * te bytes, which no
// limit of that function feels -- at cs = 105 two tiles of 81,152 B still share a CU).  A pair of elements (k, k + 1) of one column
// takes a 16-byte load per cell where both cell addresses are 16-byte aligned -- always for even K -- and 8-byte loads otherwise (odd
// K: every second pair of a cell column).  A cell column is K contiguous doubles shared by the ~6 edges of a patch around it: the
// gather costs requests, hardly HBM bytes.  Lane l < te sweeps column l; u goes back the way it came, active levels only.
// vmix_kernel(K, generic, 3) of tracer_vmix.hip holds the LDS formula and the choice of te.
// ------------------------------------------------------------------------------------------------
constexpr int MV_NT = 64;             // threads of a tile-form workgroup: one wave
constexpr int MV_U = 8;               // 16-byte loads a lane has in flight per array while it stages

struct MvmixTileCol {
    double *hs, *xs, *ys;             // the lane's column in the sets
    double dt;
    __device__ __forceinline__ double s(int k) const { return dt * ys[k]; }        // FIELD: f[k] sits in the slot y[k] takes next
    __device__ __forceinline__ double h(int k) const { return hs[k]; }
    __device__ __forceinline__ double x(int k) const { return xs[k]; }
    __device__ __forceinline__ void putG(int k, double v) { hs[k] = v; }
    __device__ __forceinline__ double g(int k) const { return hs[k]; }
    __device__ __forceinline__ void putY(int k, double v) { ys[k] = v; }
    __device__ __forceinline__ double y(int k) const { return ys[k]; }
    __device__ __forceinline__ void emit(int k, double inc) { xs[k] = xs[k] + inc; }
};

// The staging of a tile, shared by the forward pass and its transpose (mvmix_index.hpp holds mv_slot and the span arithmetic).
// mv_stage_span: the nEl doubles of a tile's span of an (K, nE) field into a column set, as they lie.
__device__ __forceinline__ void mv_stage_span(double *const S, const double *const G, const unsigned nEl, const int tid, const unsigned magic,
                                              const unsigned K, const unsigned cs)
{
    const bool vec = (reinterpret_cast<uintptr_t>(G) & 15) == 0;
    for (unsigned i0 = 2u * tid; i0 < nEl; i0 += 2u * MV_NT * MV_U) {
        double2 vx[MV_U];
#pragma unroll
        for (int u = 0; u < MV_U; ++u) {
            const unsigned e = i0 + 2u * MV_NT * u;
            vx[u] = make_double2(0.0, 0.0);
            if (vec && e + 1 < nEl) vx[u] = *reinterpret_cast<const double2 *>(G + e);
            else if (e < nEl) {
                vx[u].x = G[e];
                if (e + 1 < nEl) vx[u].y = G[e + 1];
            }
        }
#pragma unroll
        for (int u = 0; u < MV_U; ++u) {
            const unsigned e = i0 + 2u * MV_NT * u;
            unsigned cc;
            if (e < nEl) S[mv_slot(e, magic, K, cs, cc)] = vx[u].x;
            if (e + 1 < nEl) S[mv_slot(e + 1, magic, K, cs, cc)] = vx[u].y;
        }
    }
}

// mv_gather_h: h_e of every element (column, k) with k < hd[column].w from the two cell columns {hd.x, hd.y} of the edge
__device__ __forceinline__ void mv_gather_h(double *const H, const double *const hG, const int4 *const hd, const unsigned nEl, const int tid,
                                            const unsigned magic, const unsigned K, const unsigned cs)
{
    const bool vecH = (reinterpret_cast<uintptr_t>(hG) & 15) == 0;
    for (unsigned i0 = 2u * tid; i0 < nEl; i0 += 2u * MV_NT * MV_U) {
        double2 v1[MV_U], v2[MV_U];
        unsigned qa[MV_U], qb[MV_U];
        bool okA[MV_U], okB[MV_U];
#pragma unroll
        for (int u = 0; u < MV_U; ++u) {
            const unsigned e = i0 + 2u * MV_NT * u;
            v1[u] = v2[u] = make_double2(0.0, 0.0);
            qa[u] = qb[u] = 0;
            okA[u] = okB[u] = false;
            if (e >= nEl) continue;
            unsigned ca, cb = 0;
            qa[u] = mv_slot(e, magic, K, cs, ca);
            const int4 ra = hd[ca];
            const unsigned ka = e - ca * K;
            okA[u] = (int)ka < ra.w;
            const size_t a1 = (size_t)ra.x * K + ka, a2 = (size_t)ra.y * K + ka;
            int4 rb = ra;
            unsigned kb = ka + 1;
            if (e + 1 < nEl) {
                qb[u] = mv_slot(e + 1, magic, K, cs, cb);
                if (cb != ca) { rb = hd[cb]; kb = 0; }
                okB[u] = (int)kb < rb.w;
            }
            if (okA[u] && okB[u] && cb == ca && vecH && ((a1 | a2) & 1) == 0) {
                v1[u] = *reinterpret_cast<const double2 *>(hG + a1);
                v2[u] = *reinterpret_cast<const double2 *>(hG + a2);
            } else {
                if (okA[u]) { v1[u].x = hG[a1]; v2[u].x = hG[a2]; }
                if (okB[u]) { v1[u].y = hG[(size_t)rb.x * K + kb]; v2[u].y = hG[(size_t)rb.y * K + kb]; }
            }
        }
#pragma unroll
        for (int u = 0; u < MV_U; ++u) {
            if (okA[u]) H[qa[u]] = 0.5 * (v1[u].x + v2[u].x);
            if (okB[u]) H[qb[u]] = 0.5 * (v1[u].y + v2[u].y);
        }
    }
}

// mv_store_span: a column set back into the span, the rows k < depth of a column only (depth = hd.w, or hd.z with WZ: the transpose
// keeps the depth it writes apart from the depth it stages)
template <bool WZ>
__device__ __forceinline__ void mv_store_span(const double *const S, double *const G, const int4 *const hd, const unsigned nEl, const int tid,
                                              const unsigned magic, const unsigned K, const unsigned cs)
{
    const bool vec = (reinterpret_cast<uintptr_t>(G) & 15) == 0;
    for (unsigned i0 = 2u * tid; i0 < nEl; i0 += 2u * MV_NT) {
        const unsigned e = i0;
        unsigned ca, cb = 0;
        const unsigned qA = mv_slot(e, magic, K, cs, ca);
        const bool okA = (int)(e - ca * K) < (WZ ? hd[ca].z : hd[ca].w);
        bool okB = false;
        double2 o = make_double2(0.0, 0.0);
        if (okA) o.x = S[qA];
        if (e + 1 < nEl) {
            const unsigned qB = mv_slot(e + 1, magic, K, cs, cb);
            okB = (int)(e + 1 - cb * K) < (WZ ? hd[cb].z : hd[cb].w);
            if (okB) o.y = S[qB];
        }
        if (vec && okA && okB) *reinterpret_cast<double2 *>(G + e) = o;
        else {
            if (okA) G[e] = o.x;
            if (okB) G[e + 1] = o.y;
        }
    }
}

// mv_sub_span: G[k,e] = G[k,e] - S[k,e] for the rows k < hd.w - 1 of a column (the interfaces of the solved rows); no other row of the
// span is read or written
__device__ __forceinline__ void mv_sub_span(const double *const S, double *const G, const int4 *const hd, const unsigned nEl, const int tid,
                                            const unsigned magic, const unsigned K, const unsigned cs)
{
    const bool vec = (reinterpret_cast<uintptr_t>(G) & 15) == 0;
    for (unsigned i0 = 2u * tid; i0 < nEl; i0 += 2u * MV_NT) {
        const unsigned e = i0;
        unsigned ca, cb = 0;
        const unsigned qA = mv_slot(e, magic, K, cs, ca);
        const bool okA = (int)(e - ca * K) < hd[ca].w - 1;
        bool okB = false;
        unsigned qB = 0;
        if (e + 1 < nEl) {
            qB = mv_slot(e + 1, magic, K, cs, cb);
            okB = (int)(e + 1 - cb * K) < hd[cb].w - 1;
        }
        if (vec && okA && okB) {
            double2 o = *reinterpret_cast<const double2 *>(G + e);
            o.x = o.x - S[qA]; o.y = o.y - S[qB];
            *reinterpret_cast<double2 *>(G + e) = o;
        } else {
            if (okA) G[e] = G[e] - S[qA];
            if (okB) G[e + 1] = G[e + 1] - S[qB];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The bottom speed of the quadratic drag (moka_set_quadratic_bottom_drag; the recipe of include/moka_hip.h): a launch of its own in
// front of the pass, which overwrites u tile by tile while the stencil of an edge reaches into other tiles.  One lane per edge in
// device numbering: the edges of a patch are numbered together, so the lanes of a wave share their cells' eoc / mltc rows and most of
// the u[kb,e'] they gather -- about one new line of u per edge, element-granular 8-byte requests served from L2.  A lane loads its two
// cells' eoc and mltc rows (mltc[c,i] = maxLevelEdgeTop of the edge in slot i, 0 for an empty slot: the depth test without a dependent
// read of that edge's ehdr), then keCoef[e'] and u[kb,e'] of the slots that pass the test, all in flight together; the two sums run
// afterwards in slot order, in registers: no atomics, no shuffles, one summation order.  u[kb,e'] of a slot that fails the test is
// not read.  Any K, any maxEdges <= MS_ME, every kernel variant.
// ------------------------------------------------------------------------------------------------
constexpr int MS_ME = 8;              // the slots of a cell the gfx950 kernels support (moka_mesh_create refuses more)

__global__ __launch_bounds__(BLOCK) void k_mvmix_bottom_speed(const MomSpeedArgs a)
{
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= a.nE) return;
    const int4 r = *reinterpret_cast<const int4 *>(a.ehdr + (size_t)e * 4);
    const int n = min(r.w, a.K);
    if (n < 1) {
        a.sp[e] = 0.0;
        return;
    }
    const int kb = n - 1;
    int ee[2][MS_ME];
    bool ok[2][MS_ME];
    double kc[2][MS_ME], x[2][MS_ME];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const size_t row = (size_t)(j ? r.y : r.x) * a.ME;
#pragma unroll
        for (int i = 0; i < MS_ME; ++i) {
            ee[j][i] = i < a.ME ? a.eoc[row + i] : -1;
            ok[j][i] = i < a.ME && ee[j][i] >= 0 && min(a.mltc[row + i], a.K) > kb;
        }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < MS_ME; ++i) {
            kc[j][i] = ok[j][i] ? a.keCoef[ee[j][i]] : 0.0;
            x[j][i] = ok[j][i] ? a.u[(size_t)ee[j][i] * a.K + kb] : 0.0;
        }
    double ke[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < MS_ME; ++i)
            if (ok[j][i]) acc = acc + (kc[j][i] * x[j][i]) * x[j][i];
        ke[j] = acc * a.invArea[j ? r.y : r.x];
    }
    a.sp[e] = sqrt(ke[0] + ke[1]);       // (llvm.sqrt.f64: correctly rounded on gfx950 -- v_rsq_f64, two Goldschmidt steps, two fma corrections)
}

hipError_t launch_momentum_bottom_speed(const MomSpeedArgs &a, hipStream_t s)
{
    if (a.nE <= 0 || a.K < 1) return hipSuccess;
    if (a.ME > MS_ME || !a.ehdr || !a.eoc || !a.mltc || !a.keCoef || !a.invArea || !a.u || !a.sp) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mvmix_bottom_speed, dim3((a.nE + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, a);
    return hipGetLastError();
}

// QD (the quadratic drag): q = dt * (drag + cd * speed[e]) per lane where the other instances take the one q = dt * drag; DRAG is on
// with it, and mvmix_column is what it is.
template <bool QD>
__device__ __forceinline__ double mvmix_q(const MomVmixArgs &a, const int e)
{
    return QD ? a.dt * (a.drag + a.cd * a.speed[e]) : a.dt * a.drag;
}

template <bool DRAG, bool STRESS, bool FIELD, bool QD>
__global__ __launch_bounds__(MV_NT) void k_mvmix_tile(const MomVmixArgs a, const int te, const int cs, const unsigned magic)
{
    extern __shared__ __align__(16) unsigned char mv_smem[];
    double *const H = reinterpret_cast<double *>(mv_smem), *const X = H + (size_t)te * cs, *const Y = X + (size_t)te * cs;
    int4 *const hd = reinterpret_cast<int4 *>(Y + (size_t)te * cs);        // {c1, c2, -, n}: (3 te cs) doubles in, te even: 16-byte aligned
    const int tid = threadIdx.x, K = a.K;
    const MvSpan sp = mv_span(blockIdx.x, te, a.nE, K);
    int n = 0;
    double b = 0.0, q = mvmix_q<false>(a, 0);
    if (tid < te) {
        int4 r = make_int4(0, 0, 0, 0);
        if (tid < sp.ncol) {
            r = *reinterpret_cast<const int4 *>(a.ehdr + (size_t)(sp.e0 + tid) * 4);
            n = mvmix_depth<DRAG, STRESS>(r.w, K);
            if (STRESS && n > 0) b = a.dt * a.tau[sp.e0 + tid];
            if (QD && n > 0) q = mvmix_q<true>(a, sp.e0 + tid);
        }
        r.w = n;
        hd[tid] = r;
    }
    double *const uG = a.u + sp.base;
    mv_stage_span(X, uG, sp.nEl, tid, magic, K, cs);            // u: the span as it lies
    if (FIELD) mv_stage_span(Y, a.fld + sp.base, sp.nEl, tid, magic, K, cs);       // f into the set of y: rows k >= n - 1 lie there unread
    __syncthreads();                                            // the records are in place
    mv_gather_h(H, a.h, hd, sp.nEl, tid, magic, K, cs);         // h_e: gathered from the two cell columns of every edge, active levels only
    __syncthreads();
    if (n > 0) {
        MvmixTileCol col{H + (size_t)tid * cs, X + (size_t)tid * cs, Y + (size_t)tid * cs, a.dt};
        mvmix_column<DRAG, STRESS, FIELD>(col, n, a.dt * a.nu, q, b);
    }
    __syncthreads();
    mv_store_span<false>(X, uG, hd, sp.nEl, tid, magic, K, cs); // back: the rows k < n of a column only
}

// ------------------------------------------------------------------------------------------------
// Form 2, column.  One lane per edge straight from global memory; h_e formed on the fly from the two cell columns; g and y in a global
// scratch of 2 * K * nE doubles laid out level-major (the lanes of a wave store side by side).  Any K, any mesh, kernel variant 3.
// ------------------------------------------------------------------------------------------------
struct MvmixGlobalCol {
    const double *h1, *h2;            // the two cell columns
    double *uc;                       // the edge's column of u
    double *gs, *ys;                  // scratch: element k at [k * nE]
    size_t nE;
    const double *fc;                 // FIELD: the edge's column of f
    double dt;
    __device__ __forceinline__ double s(int k) const { return dt * fc[k]; }
    __device__ __forceinline__ double h(int k) const { return 0.5 * (h1[k] + h2[k]); }
    __device__ __forceinline__ double x(int k) const { return uc[k]; }
    __device__ __forceinline__ void putG(int k, double v) { gs[k * nE] = v; }
    __device__ __forceinline__ double g(int k) const { return gs[k * nE]; }
    __device__ __forceinline__ void putY(int k, double v) { ys[k * nE] = v; }
    __device__ __forceinline__ double y(int k) const { return ys[k * nE]; }
    __device__ __forceinline__ void emit(int k, double inc) { uc[k] = uc[k] + inc; }
};

template <bool DRAG, bool STRESS, bool FIELD, bool QD>
__global__ __launch_bounds__(BLOCK) void k_mvmix_column(const MomVmixArgs a)
{
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= a.nE) return;
    const int4 r = *reinterpret_cast<const int4 *>(a.ehdr + (size_t)e * 4);
    const int n = mvmix_depth<DRAG, STRESS>(r.w, a.K);
    if (n == 0) return;
    const size_t nEK = (size_t)a.nE * a.K;
    MvmixGlobalCol col{a.h + (size_t)r.x * a.K, a.h + (size_t)r.y * a.K, a.u + (size_t)e * a.K, a.scratch + e, a.scratch + nEK + e, (size_t)a.nE,
                       FIELD ? a.fld + (size_t)e * a.K : nullptr, a.dt};
    mvmix_column<DRAG, STRESS, FIELD>(col, n, a.dt * a.nu, mvmix_q<QD>(a, e), STRESS ? a.dt * a.tau[e] : 0.0);
}

template <bool DRAG, bool STRESS, bool FIELD, bool QD>
static hipError_t launch_mvmix_with(const MomVmixArgs &a, const VmixKernel &k, hipStream_t s)
{
    if (k.form == 1) {
        const size_t lds = k.lds + 12 * (size_t)k.tc;       // the records take 16 bytes a column where vmix_kernel counts 4
        if (lds > 64 * 1024)
            if (hipError_t e = raise_dyn_lds({reinterpret_cast<const void *>(k_mvmix_tile<DRAG, STRESS, FIELD, QD>)}, 80 * 1024); e != hipSuccess) return e;
        const unsigned magic = mv_magic((unsigned)a.K);
        hipLaunchKernelGGL((k_mvmix_tile<DRAG, STRESS, FIELD, QD>), dim3((a.nE + k.tc - 1) / k.tc), dim3(MV_NT), lds, s, a, k.tc, a.K | 1, magic);
    } else {
        hipLaunchKernelGGL((k_mvmix_column<DRAG, STRESS, FIELD, QD>), dim3((a.nE + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, a);
    }
    return hipGetLastError();
}

int momentum_vmix_form(int K, bool generic) { return vmix_kernel(K, generic, 3).form; }

template <bool STRESS, bool FIELD>
static hipError_t launch_mvmix_drag(const MomVmixArgs &a, const VmixKernel &k, hipStream_t s)
{
    if (a.speed && a.cd != 0.0) return launch_mvmix_with<true, STRESS, FIELD, true>(a, k, s);
    return a.drag != 0.0 ? launch_mvmix_with<true, STRESS, FIELD, false>(a, k, s) : launch_mvmix_with<false, STRESS, FIELD, false>(a, k, s);
}

hipError_t launch_momentum_vmix(const MomVmixArgs &a, bool generic, hipStream_t s)
{
    const bool drag = a.drag != 0.0 || (a.speed && a.cd != 0.0), stress = a.tau != nullptr;
    if (a.nE <= 0 || a.K < 1 || (a.K < 2 && !drag && !stress)) return hipSuccess;
    if ((uint64_t)a.K * 64u >= (1ull << 32)) return hipErrorInvalidValue;
    const VmixKernel k = vmix_kernel(a.K, generic, 3);
    if (k.form == 2 && !a.scratch) return hipErrorInvalidValue;
    if (a.fld) return stress ? launch_mvmix_drag<true, true>(a, k, s) : launch_mvmix_drag<false, true>(a, k, s);
    return stress ? launch_mvmix_drag<true, false>(a, k, s) : launch_mvmix_drag<false, false>(a, k, s);
}

// ================================================================================================
// The transposed pass (moka_forced_tape): include/moka_hip.h states the recipe; this is it, once, for one edge column of n >= 1 levels.
// A = diag(h) + s W + q e_{n-1} e_{n-1}^T is symmetric, so z = Solve_A(xu) takes the forward's factorisation and sweep with xu as the
// right-hand side; then, ascending, hm[k] = 0.5 * (h[k] + h[k+1]), w[k] = s / hm[k] (the forward's bits), D = z[k] - z[k+1],
// E = un[k] - un[k+1], P[k] = (w[k] / hm[k]) * (D * E), Rn = R(un) as mvmix_column forms R, hbar[k] = 0.5 * (P[k-1] + P[k]) - z[k] *
// (Rn[k] / h[k]) (end rows: 0.5 * the one P; n == 1: 0.0 - z[0] * (Rn[0] / h[0])), xu[k] = h[k] * z[k].  GRAD: the three densities.
// The accessor C:
//     h(k), xu(k), un(k)     edge thickness, the adjoint's right-hand side (read once, before putY(k)), the recorded u_new
//     putG / g, putY / y     the sweep's two work columns; y[k] takes z[k]
//     putHbar, putXU         the results (an accessor of a column the forward pass skipped drops them)
//     s(k)                   FIELD only: dt * f[k,e] of the recorded step's field, read in both sweeps (the tile keeps f in a set of its own)
//     putDF(k, v)            GRAD with wdf only: DF[k,e] = DF[k,e] - v, v = dt * (de[k] / hm[k]), k <= n - 2, called once h(k + 1) is read
// FIELD: s[k] = dt * f[k,e] in both places where w is formed; everything else as written.
// QD (a step of a quadratic tape whose sp was recorded): q is the lane's own, and mvadj_speed_bar runs once at the end of the column;
// an instance without it holds none of its operations.
// ================================================================================================
// QD (a quadratic moka_forced_tape; the lane's q comes from the recorded sp[e], see mvadj_q): with t = z[n-1] * un[n-1], formed once
// per column, q-bar = -t, hence sp-bar = dt * Cd * q-bar and, for the transpose of the bottom-speed stencil, M = sp-bar / sp -- 0.0 at
// sp == 0, the kink of the square root -- and the density of Cd takes dt * sp * q-bar.  mo: M[e] (nullptr: the step ran with Cd == 0),
// dc: Dcd[e] (nullptr: not wanted).
__device__ __forceinline__ void mvadj_speed_bar(const double t, const double sp, const double dt, const double dtcd, double *const mo,
                                                double *const dc)
{
    if (mo) *mo = sp > 0.0 ? (0.0 - dtcd * t) / sp : 0.0;
    if (dc) *dc = *dc - (dt * t) * sp;
}

// the q of a lane in the QD instances: the forward's mvmix_q<true> expression on the recorded sp for a step with Cd != 0, the one
// q = dt * drag for a step with Cd == 0 whose sp was recorded for the density alone
__device__ __forceinline__ double mvadj_q(const MomVmixAdjArgs &a, const double sp)
{
    return a.cd != 0.0 ? a.dt * (a.drag + a.cd * sp) : a.dt * a.drag;
}

template <bool DRAG, bool STRESS, bool GRAD, bool FIELD, bool QD, class C>
__device__ __forceinline__ void mvadj_column(C &c, const int n, const double s, const double q, const double b, const double dt,
                                             double *const gt, double *const dn, double *const dr, const bool wdf, const double sp = 0.0,
                                             const double dtcd = 0.0, double *const mo = nullptr, double *const dc = nullptr)
{
    double hk = c.h(0);
    if (n == 1) {
        double d = hk, r = 0.0;
        if (DRAG) d = d + q;
        const double z = c.xu(0) / d, uk = c.un(0);
        if (STRESS) r = r + b;
        if (DRAG) r = r - q * uk;
        c.putHbar(0, 0.0 - z * (r / hk));
        c.putXU(0, hk * z);
        if (GRAD) {                                 // (the sum of D_nu is empty: the density is left alone)
            if (gt) *gt = *gt + dt * z;
            if (dr) *dr = *dr - dt * (z * uk);
        }
        if (QD) mvadj_speed_bar(z * uk, sp, dt, dtcd, mo, dc);
        return;
    }
    double hn = c.h(1);
    double w = (FIELD ? c.s(0) : s) / (0.5 * (hk + hn));      // w[0]
    double beta = hk + w;                           // d[0]
    double y = c.xu(0) / beta;
    c.putY(0, y);
    for (int k = 1; k < n; ++k) {
        const double wp = w;                        // w[k-1]
        hk = hn;
        const double g = wp / beta;
        c.putG(k - 1, g);
        double d;
        if (k < n - 1) {
            hn = c.h(k + 1);
            w = (FIELD ? c.s(k) : s) / (0.5 * (hk + hn));
            d = (hk + wp) + w;
        } else {
            d = hk + wp;
            if (DRAG) d = d + q;
        }
        beta = d - wp * g;
        y = (c.xu(k) + wp * y) / beta;
        c.putY(k, y);
    }
    double z = y;                                   // z[n-1] already sits in y[n-1]
    for (int k = n - 2; k >= 0; --k) {
        z = c.y(k) + c.g(k) * z;
        c.putY(k, z);
    }
    const double z0 = z;
    // ascending: hbar and h o z
    hk = c.h(0); hn = c.h(1);
    double zk = z0, zn = c.y(1), uk = c.un(0), un = c.un(1), um = 0.0;
    double hm = 0.5 * (hk + hn);
    w = (FIELD ? c.s(0) : s) / hm;
    double de = (zk - zn) * (uk - un);
    double P = (w / hm) * de, sum = 0.0;
    if (GRAD) sum = sum + de / hm;
    if (GRAD && wdf) c.putDF(0, dt * (de / hm));
    double r = w * (un - uk);
    if (STRESS) r = r + b;
    c.putHbar(0, 0.5 * P - zk * (r / hk));
    c.putXU(0, hk * zk);
    for (int k = 1; k < n; ++k) {
        const double Pp = P, wp = w;
        um = uk; uk = un; hk = hn; zk = zn;
        double hb;
        if (k < n - 1) {
            hn = c.h(k + 1); un = c.un(k + 1); zn = c.y(k + 1);
            hm = 0.5 * (hk + hn);
            w = (FIELD ? c.s(k) : s) / hm;
            de = (zk - zn) * (uk - un);
            P = (w / hm) * de;
            if (GRAD) sum = sum + de / hm;
            if (GRAD && wdf) c.putDF(k, dt * (de / hm));
            r = wp * (um - uk) + w * (un - uk);
            hb = 0.5 * (Pp + P) - zk * (r / hk);
        } else {
            r = wp * (um - uk);
            if (DRAG) r = r - q * uk;
            hb = 0.5 * Pp - zk * (r / hk);
        }
        c.putHbar(k, hb);
        c.putXU(k, hk * zk);
    }
    if (GRAD) {
        if (gt) *gt = *gt + dt * z0;
        if (dn) *dn = *dn - dt * sum;
        if (dr) *dr = *dr - dt * (zk * uk);         // row n - 1
    }
    if (QD) mvadj_speed_bar(zk * uk, sp, dt, dtcd, mo, dc);
}

// the two depths of a column in a launch of the transpose: nw, the rows whose xu and hbar it writes -- the forward's mvmix_depth, 0
// for a step that ran without the pass -- and n >= nw, the rows it solves: with GRAD every column that has an active level
template <bool DRAG, bool STRESS, bool GRAD>
__device__ __forceinline__ int mvadj_depth(const int mlt, const int K, const int on, int &nw)
{
    nw = on ? mvmix_depth<DRAG, STRESS>(mlt, K) : 0;
    return GRAD ? max(min(mlt, K), 0) : nw;
}

// ------------------------------------------------------------------------------------------------
// Form 1, tile: the forward tile with four column sets --
//     set 0: h_e | set 1: xu, its slot k taking y[k], then z[k], then h[k] * z[k] | set 2: g, its slot k taking hbar[k] | set 3: un
// -- and the record {c1, c2, nw, n}.  xu and un are staged as spans, h_e gathered for the rows k < n, xu and hbar go back as spans,
// rows k < nw only.  vmix_kernel(K, generic, 4) holds the choice of te: at most 32 * 79 * 8 * 4 + 16 * 32 = 81,408 bytes a tile.
// FIELD: w is formed in two sweeps and every slot of the four sets is rewritten in between, so f of the recorded step is staged into
// a fifth set and stays there: vmix_kernel(K, generic, 5), 64-column tiles to K = 15, 32-column tiles to K = 63 (81,152 bytes).
// DF (a.DF != nullptr, with or without FIELD): the lane leaves dt * (de[k] / hm[k]) in slot k of set 0 -- free once the ascending sweep
// holds h[k] and h[k+1] in registers -- and mv_sub_span takes the rows k < n - 1 of the set off the span of DF, coalesced, as xu and
// hbar go back.  A lane that wrote its own column of DF would issue one 8-byte store per level, K doubles apart from its neighbour's.
// ------------------------------------------------------------------------------------------------
struct MvadjTileCol {
    double *hs, *xs, *gs, *us;
    const double *fs;                 // FIELD: the fifth set
    double dt;
    __device__ __forceinline__ double s(int k) const { return dt * fs[k]; }
    __device__ __forceinline__ void putDF(int k, double v) { hs[k] = v; }          // h[k] and h[k+1] sit in registers: mv_sub_span takes it from here
    __device__ __forceinline__ double h(int k) const { return hs[k]; }
    __device__ __forceinline__ double xu(int k) const { return xs[k]; }
    __device__ __forceinline__ double un(int k) const { return us[k]; }
    __device__ __forceinline__ void putG(int k, double v) { gs[k] = v; }
    __device__ __forceinline__ double g(int k) const { return gs[k]; }
    __device__ __forceinline__ void putY(int k, double v) { xs[k] = v; }
    __device__ __forceinline__ double y(int k) const { return xs[k]; }
    __device__ __forceinline__ void putHbar(int k, double v) { gs[k] = v; }
    __device__ __forceinline__ void putXU(int k, double v) { xs[k] = v; }
};

template <bool DRAG, bool STRESS, bool GRAD, bool FIELD, bool QD>
__global__ __launch_bounds__(MV_NT) void k_mvadj_tile(const MomVmixAdjArgs a, const int te, const int cs, const unsigned magic)
{
    extern __shared__ __align__(16) unsigned char mv_smem[];
    const size_t set = (size_t)te * cs;
    double *const H = reinterpret_cast<double *>(mv_smem), *const X = H + set, *const Gs = X + set, *const U = Gs + set;
    double *const Fs = FIELD ? U + set : nullptr;                          // FIELD only: the fifth set
    int4 *const hd = reinterpret_cast<int4 *>(U + (FIELD ? 2 : 1) * set);  // (4 or 5 te cs) doubles in, te even: 16-byte aligned
    const int tid = threadIdx.x, K = a.K;
    const MvSpan sp = mv_span(blockIdx.x, te, a.nE, K);
    int n = 0;
    double b = 0.0, spd = 0.0;
    if (tid < te) {
        int4 r = make_int4(0, 0, 0, 0);
        if (tid < sp.ncol) {
            r = *reinterpret_cast<const int4 *>(a.ehdr + (size_t)(sp.e0 + tid) * 4);
            int nw;
            n = mvadj_depth<DRAG, STRESS, GRAD>(r.w, K, a.on, nw);
            if (STRESS && n > 0) b = a.dt * a.tau[sp.e0 + tid];
            if (QD && n > 0) spd = a.speed[sp.e0 + tid];
            r.z = nw;
        }
        r.w = n;
        hd[tid] = r;
    }
    mv_stage_span(X, a.xu + sp.base, sp.nEl, tid, magic, K, cs);
    mv_stage_span(U, a.un + sp.base, sp.nEl, tid, magic, K, cs);
    if (FIELD) mv_stage_span(Fs, a.fld + sp.base, sp.nEl, tid, magic, K, cs);
    __syncthreads();
    mv_gather_h(H, a.hn, hd, sp.nEl, tid, magic, K, cs);
    __syncthreads();
    if (n > 0) {
        const size_t o = (size_t)tid * cs;
        const int e = sp.e0 + tid;
        MvadjTileCol col{H + o, X + o, Gs + o, U + o, FIELD ? Fs + o : nullptr, a.dt};
        if (QD)
            mvadj_column<DRAG, STRESS, GRAD, FIELD, true>(col, n, a.dt * a.nu, mvadj_q(a, spd), b, a.dt, GRAD && a.Gtau ? a.Gtau + e : nullptr,
                                                          GRAD && a.Dnu ? a.Dnu + e : nullptr, GRAD && a.Dr ? a.Dr + e : nullptr, GRAD && a.DF, spd,
                                                          a.dt * a.cd, a.cd != 0.0 ? a.M + e : nullptr, GRAD && a.Dcd ? a.Dcd + e : nullptr);
        else
            mvadj_column<DRAG, STRESS, GRAD, FIELD, false>(col, n, a.dt * a.nu, a.dt * a.drag, b, a.dt, GRAD && a.Gtau ? a.Gtau + e : nullptr,
                                                           GRAD && a.Dnu ? a.Dnu + e : nullptr, GRAD && a.Dr ? a.Dr + e : nullptr, GRAD && a.DF);
    }
    __syncthreads();
    mv_store_span<true>(X, a.xu + sp.base, hd, sp.nEl, tid, magic, K, cs);
    mv_store_span<true>(Gs, a.hbar + sp.base, hd, sp.nEl, tid, magic, K, cs);
    if (GRAD && a.DF) mv_sub_span(H, a.DF + sp.base, hd, sp.nEl, tid, magic, K, cs);
}

// ------------------------------------------------------------------------------------------------
// Form 2, column: a lane per edge from global memory, g and y in the level-major scratch of the forward's column form.
// ------------------------------------------------------------------------------------------------
struct MvadjGlobalCol {
    const double *h1, *h2, *uc;
    double *xc, *hb, *gs, *ys;
    size_t nE;
    bool wr;                          // the forward pass computed this column: its xu and hbar are written
    const double *fc;                 // FIELD: the edge's column of f
    double *df;                       // ... and of DF (nullptr: not wanted)
    double dt;
    __device__ __forceinline__ double s(int k) const { return dt * fc[k]; }
    __device__ __forceinline__ void putDF(int k, double v) { df[k] = df[k] - v; }
    __device__ __forceinline__ double h(int k) const { return 0.5 * (h1[k] + h2[k]); }
    __device__ __forceinline__ double xu(int k) const { return xc[k]; }
    __device__ __forceinline__ double un(int k) const { return uc[k]; }
    __device__ __forceinline__ void putG(int k, double v) { gs[k * nE] = v; }
    __device__ __forceinline__ double g(int k) const { return gs[k * nE]; }
    __device__ __forceinline__ void putY(int k, double v) { ys[k * nE] = v; }
    __device__ __forceinline__ double y(int k) const { return ys[k * nE]; }
    __device__ __forceinline__ void putHbar(int k, double v) { if (wr) hb[k] = v; }
    __device__ __forceinline__ void putXU(int k, double v) { if (wr) xc[k] = v; }
};

template <bool DRAG, bool STRESS, bool GRAD, bool FIELD, bool QD>
__global__ __launch_bounds__(BLOCK) void k_mvadj_column(const MomVmixAdjArgs a)
{
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= a.nE) return;
    const int4 r = *reinterpret_cast<const int4 *>(a.ehdr + (size_t)e * 4);
    int nw;
    const int n = mvadj_depth<DRAG, STRESS, GRAD>(r.w, a.K, a.on, nw);
    if (n == 0) return;
    const size_t nEK = (size_t)a.nE * a.K, o = (size_t)e * a.K;
    MvadjGlobalCol col{a.hn + (size_t)r.x * a.K, a.hn + (size_t)r.y * a.K, a.un + o, a.xu + o, a.hbar + o, a.scratch + e, a.scratch + nEK + e,
                       (size_t)a.nE, nw > 0, FIELD ? a.fld + o : nullptr, GRAD && a.DF ? a.DF + o : nullptr, a.dt};
    if (QD) {
        const double spd = a.speed[e];
        mvadj_column<DRAG, STRESS, GRAD, FIELD, true>(col, n, a.dt * a.nu, mvadj_q(a, spd), STRESS ? a.dt * a.tau[e] : 0.0, a.dt,
                                                      GRAD && a.Gtau ? a.Gtau + e : nullptr, GRAD && a.Dnu ? a.Dnu + e : nullptr,
                                                      GRAD && a.Dr ? a.Dr + e : nullptr, GRAD && a.DF, spd, a.dt * a.cd,
                                                      a.cd != 0.0 ? a.M + e : nullptr, GRAD && a.Dcd ? a.Dcd + e : nullptr);
    } else {
        mvadj_column<DRAG, STRESS, GRAD, FIELD, false>(col, n, a.dt * a.nu, a.dt * a.drag, STRESS ? a.dt * a.tau[e] : 0.0, a.dt,
                                                       GRAD && a.Gtau ? a.Gtau + e : nullptr, GRAD && a.Dnu ? a.Dnu + e : nullptr,
                                                       GRAD && a.Dr ? a.Dr + e : nullptr, GRAD && a.DF);
    }
}

// ------------------------------------------------------------------------------------------------
// The cell gather: xh[k,c] = xh[k,c] + 0.5 * (the sum, from 0.0, over the slots i of edgesOnCell[c] in ascending order whose edge the
// forward pass computed and has k < n_e, of hbar[k,e]).  LPC lanes run along the contiguous column of a cell; an element no slot
// reaches is not written; rows of hbar at and below an edge's depth are never read.  No atomics.
// ------------------------------------------------------------------------------------------------
template <bool DRAG, bool STRESS>
__global__ __launch_bounds__(BLOCK) void k_mvadj_gather(const MomVmixAdjArgs a, const int lpc)
{
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    const int c = t / lpc, l = t - c * lpc;
    if (c >= a.nC) return;
    for (int k = l; k < a.K; k += lpc) {
        double sum = 0.0;
        bool any = false;
        for (int i = 0; i < a.ME; ++i) {
            const int e = a.eoc[(size_t)c * a.ME + i];
            if (e < 0) continue;
            if (k < mvmix_depth<DRAG, STRESS>(a.ehdr[(size_t)e * 4 + 3], a.K)) {
                sum = sum + a.hbar[(size_t)e * a.K + k];
                any = true;
            }
        }
        if (any) a.xh[(size_t)c * a.K + k] = a.xh[(size_t)c * a.K + k] + 0.5 * sum;
    }
}

// ------------------------------------------------------------------------------------------------
// The transpose of the bottom-speed stencil (a quadratic moka_forced_tape; the recipe of include/moka_hip.h), behind the transposed
// pass of a step with Cd != 0 and in front of the four reverse RK stages.  k_mvmix_bottom_speed turned round: where its lane e gathers
// u[kb_e,e'] over the slots e' of its two cells, the lane e' here gathers M[e] = sp-bar[e] / sp[e] over the same slots -- every edge
// whose stencil holds e' shares a cell with it -- and adds (kc[e'] * us[k,e']) * g to the rows k of its own column of xu that are some
// neighbour's bottom level kb_e < n_e'.  One lane per edge in device numbering; it loads its ehdr record, its two cells' eoc and
// mltc rows (the neighbour's depth without a dependent read of its ehdr), invArea of both cells, kc[e'], then M[e] of every slot that
// passes e >= 0, n_e >= 1, n_e - 1 < n_e', all in flight together; then us[k,e'] and xu[k,e'] of the distinct levels.  The grouping
// by level is a predicate scan over the 2 * MS_ME slots in registers: a slot is the first of its level when no earlier passing slot
// has its kb; the first slot of a level sums M over the slots of that level, cell by cell in slot order, and stores the one element.
// Distinct levels are distinct elements of the lane's column: no atomics, no shuffles, no read-modify-write chain on an address,
// one summation order.  The edge e' sits in both its cells' rows and is counted in both, as in the forward.  Rows k >= n_e' of xu and
// us are never touched; M and us of a slot that fails the test are not read.  Any K, any maxEdges <= MS_ME, every kernel variant.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_mvadj_bottom_speed(const MomSpeedAdjArgs a)
{
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= a.nE) return;
    const int4 r = *reinterpret_cast<const int4 *>(a.ehdr + (size_t)e * 4);
    const int n = min(r.w, a.K);
    if (n < 1) return;
    int ee[2][MS_ME], kb[2][MS_ME];
    bool ok[2][MS_ME], first[2][MS_ME];
    double m[2][MS_ME], us[2][MS_ME], xo[2][MS_ME];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const size_t row = (size_t)(j ? r.y : r.x) * a.ME;
#pragma unroll
        for (int i = 0; i < MS_ME; ++i) {
            ee[j][i] = i < a.ME ? a.eoc[row + i] : -1;
            const int ml = i < a.ME ? min(a.mltc[row + i], a.K) : 0;
            kb[j][i] = ml - 1;
            ok[j][i] = i < a.ME && ee[j][i] >= 0 && ml >= 1 && ml - 1 < n;
        }
    }
    const double inv0 = a.invArea[r.x], inv1 = a.invArea[r.y], kc = a.keCoef[e];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < MS_ME; ++i) m[j][i] = ok[j][i] ? a.M[ee[j][i]] : 0.0;
    const size_t col = (size_t)e * a.K;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < MS_ME; ++i) {
            bool f = ok[j][i];
#pragma unroll
            for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                for (int ii = 0; ii < MS_ME; ++ii)
                    if ((jj < j || (jj == j && ii < i)) && ok[jj][ii] && kb[jj][ii] == kb[j][i]) f = false;
            first[j][i] = f;
            us[j][i] = f ? a.us[col + kb[j][i]] : 0.0;
            xo[j][i] = f ? a.xu[col + kb[j][i]] : 0.0;
        }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < MS_ME; ++i)
            if (first[j][i]) {
                const int k = kb[j][i];
                double acc[2];
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    double s = 0.0;
#pragma unroll
                    for (int ii = 0; ii < MS_ME; ++ii)
                        if (ok[jj][ii] && kb[jj][ii] == k) s = s + m[jj][ii];
                    acc[jj] = s;
                }
                const double g = acc[0] * inv0 + acc[1] * inv1;
                a.xu[col + k] = xo[j][i] + (kc * us[j][i]) * g;
            }
}

hipError_t launch_momentum_speed_adjoint(const MomSpeedAdjArgs &a, hipStream_t s)
{
    if (a.nE <= 0 || a.K < 1) return hipSuccess;
    if (a.ME > MS_ME || !a.ehdr || !a.eoc || !a.mltc || !a.keCoef || !a.invArea || !a.M || !a.us || !a.xu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mvadj_bottom_speed, dim3((a.nE + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, a);
    return hipGetLastError();
}

template <bool DRAG, bool STRESS, bool GRAD, bool FIELD, bool QD>
static hipError_t launch_mvadj_with(const MomVmixAdjArgs &a, const VmixKernel &k, hipStream_t s)
{
    if (k.form == 1) {
        const size_t lds = mv_tile_lds(FIELD ? 5 : 4, k.tc, a.K);        // k.lds + 12 * k.tc: the records take 16 bytes a column where vmix_kernel counts 4
        if (lds > 64 * 1024)
            if (hipError_t e = raise_dyn_lds({reinterpret_cast<const void *>(k_mvadj_tile<DRAG, STRESS, GRAD, FIELD, QD>)}, 80 * 1024); e != hipSuccess) return e;
        hipLaunchKernelGGL((k_mvadj_tile<DRAG, STRESS, GRAD, FIELD, QD>), dim3((a.nE + k.tc - 1) / k.tc), dim3(MV_NT), lds, s, a, k.tc, a.K | 1,
                           mv_magic((unsigned)a.K));
    } else {
        hipLaunchKernelGGL((k_mvadj_column<DRAG, STRESS, GRAD, FIELD, QD>), dim3((a.nE + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, a);
    }
    return hipGetLastError();
}

// the QD instances run when the step's sp is at hand and something reads it: Cd != 0 (q and M) or the density of Cd (then among the
// gradient instances).  The drag lines are on with Cd != 0 whatever drag is, as in the forward; a step with Cd == 0 keeps the
// switches it ran with.
static bool mvadj_qd(const MomVmixAdjArgs &a) { return a.speed && (a.cd != 0.0 || a.Dcd); }
static bool mvadj_drag(const MomVmixAdjArgs &a) { return a.drag != 0.0 || (a.speed && a.cd != 0.0); }

template <bool GRAD, bool FIELD>
static hipError_t launch_mvadj_grad(const MomVmixAdjArgs &a, const VmixKernel &k, hipStream_t s)
{
    const bool drag = mvadj_drag(a), stress = a.tau != nullptr;
    if (mvadj_qd(a)) {
        if (drag) return stress ? launch_mvadj_with<true, true, GRAD, FIELD, true>(a, k, s) : launch_mvadj_with<true, false, GRAD, FIELD, true>(a, k, s);
        if constexpr (GRAD)         // Cd == 0 and no linear drag: the density of Cd alone, at zero
            return stress ? launch_mvadj_with<false, true, true, FIELD, true>(a, k, s) : launch_mvadj_with<false, false, true, FIELD, true>(a, k, s);
        return hipErrorInvalidValue;
    }
    return drag ? (stress ? launch_mvadj_with<true, true, GRAD, FIELD, false>(a, k, s) : launch_mvadj_with<true, false, GRAD, FIELD, false>(a, k, s))
                : (stress ? launch_mvadj_with<false, true, GRAD, FIELD, false>(a, k, s) : launch_mvadj_with<false, false, GRAD, FIELD, false>(a, k, s));
}

// the one place that decides the kernel of a transposed pass: four column sets, five when the step ran with a field
static VmixKernel mvadj_kernel(int K, bool generic, bool field) { return vmix_kernel(K, generic, field ? 5 : 4); }
int momentum_vmix_adjoint_form(int K, bool generic, bool field) { return mvadj_kernel(K, generic, field).form; }

hipError_t launch_momentum_vmix_adjoint(const MomVmixAdjArgs &a, bool generic, hipStream_t s)
{
    const bool drag = mvadj_drag(a), stress = a.tau != nullptr, grad = a.Gtau || a.Dnu || a.Dr || a.DF || (a.speed && a.Dcd);
    if (a.nE <= 0 || a.K < 1 || (!grad && (!a.on || (a.K < 2 && !drag && !stress)))) return hipSuccess;
    if ((uint64_t)a.K * 64u >= (1ull << 32)) return hipErrorInvalidValue;
    if (!a.xu || !a.un || !a.hn || !a.hbar) return hipErrorInvalidValue;
    if (a.speed && a.cd != 0.0 && !a.M) return hipErrorInvalidValue;
    const VmixKernel k = mvadj_kernel(a.K, generic, a.fld != nullptr);
    if (k.form == 2 && !a.scratch) return hipErrorInvalidValue;
    if (a.fld) return grad ? launch_mvadj_grad<true, true>(a, k, s) : launch_mvadj_grad<false, true>(a, k, s);
    return grad ? launch_mvadj_grad<true, false>(a, k, s) : launch_mvadj_grad<false, false>(a, k, s);
}

hipError_t launch_momentum_vmix_gather(const MomVmixAdjArgs &a, hipStream_t s)
{
    const bool drag = mvadj_drag(a), stress = a.tau != nullptr;
    if (a.nC <= 0 || a.K < 1 || !a.on || (a.K < 2 && !drag && !stress)) return hipSuccess;
    int lpc = 1;
    while (lpc < a.K && lpc < 64) lpc *= 2;
    const dim3 grid((unsigned)(((size_t)a.nC * lpc + BLOCK - 1) / BLOCK));
    if (drag) {
        if (stress) hipLaunchKernelGGL((k_mvadj_gather<true, true>), grid, dim3(BLOCK), 0, s, a, lpc);
        else hipLaunchKernelGGL((k_mvadj_gather<true, false>), grid, dim3(BLOCK), 0, s, a, lpc);
    } else {
        if (stress) hipLaunchKernelGGL((k_mvadj_gather<false, true>), grid, dim3(BLOCK), 0, s, a, lpc);
        else hipLaunchKernelGGL((k_mvadj_gather<false, false>), grid, dim3(BLOCK), 0, s, a, lpc);
    }
    return hipGetLastError();
}

}  // namespace moka
