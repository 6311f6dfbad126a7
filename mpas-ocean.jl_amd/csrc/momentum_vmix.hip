// momentum_vmix.hip -- implicit vertical mixing of momentum with a surface stress and a linear bottom drag (gfx950;
// moka_set_vertical_viscosity / moka_surface_stress_upload, NOT in the reference): one tridiagonal solve per edge column behind stage 4
// of an RK4 step, on the new normalVelocity over the new layerThickness.
#include "kernels_common.hpp"

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
// n == 1 (instances with DRAG or STRESS only): y[0] = R[0] / d[0] with d[0] = h[0] (+ q) and R[0] = 0.0 (+ b) (- q * x[0]).
// Levels k >= n are never touched.
// ------------------------------------------------------------------------------------------------
template <bool DRAG, bool STRESS, class C>
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
    double w = s / (0.5 * (hk + hn));               // w[0]
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
            w = s / (0.5 * (hk + hn));
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
//     set 0: h_e, its slot k taking g[k] once h[k] and h[k+1] sit in registers | set 1: u | set 2: y
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
    __device__ __forceinline__ double h(int k) const { return hs[k]; }
    __device__ __forceinline__ double x(int k) const { return xs[k]; }
    __device__ __forceinline__ void putG(int k, double v) { hs[k] = v; }
    __device__ __forceinline__ double g(int k) const { return hs[k]; }
    __device__ __forceinline__ void putY(int k, double v) { ys[k] = v; }
    __device__ __forceinline__ double y(int k) const { return ys[k]; }
    __device__ __forceinline__ void emit(int k, double inc) { xs[k] = xs[k] + inc; }
};

// element e of a tile's span -> its place in a column set (magic = 2^32 / K + 1: exact while e * K < 2^32)
__device__ __forceinline__ unsigned mv_slot(unsigned e, unsigned magic, unsigned K, unsigned cs, unsigned &col)
{
    col = __umulhi(e, magic);
    return col * cs + (e - col * K);
}

template <bool DRAG, bool STRESS>
__global__ __launch_bounds__(MV_NT) void k_mvmix_tile(const MomVmixArgs a, const int te, const int cs, const unsigned magic)
{
    extern __shared__ __align__(16) unsigned char mv_smem[];
    double *const H = reinterpret_cast<double *>(mv_smem), *const X = H + (size_t)te * cs, *const Y = X + (size_t)te * cs;
    int4 *const hd = reinterpret_cast<int4 *>(Y + (size_t)te * cs);        // {c1, c2, -, n}: (3 te cs) doubles in, te even: 16-byte aligned
    const int tid = threadIdx.x, K = a.K;
    const int e0 = blockIdx.x * te, ncol = min(te, a.nE - e0);
    const unsigned nEl = (unsigned)ncol * (unsigned)K;
    const size_t base = (size_t)e0 * K;
    int n = 0;
    double b = 0.0;
    if (tid < te) {
        int4 r = make_int4(0, 0, 0, 0);
        if (tid < ncol) {
            r = *reinterpret_cast<const int4 *>(a.ehdr + (size_t)(e0 + tid) * 4);
            n = mvmix_depth<DRAG, STRESS>(r.w, K);
            if (STRESS && n > 0) b = a.dt * a.tau[e0 + tid];
        }
        r.w = n;
        hd[tid] = r;
    }
    double *const uG = a.u + base;
    const double *const hG = a.h;
    const bool vec = (reinterpret_cast<uintptr_t>(uG) & 15) == 0, vecH = (reinterpret_cast<uintptr_t>(hG) & 15) == 0;
    // u: the span as it lies
    for (unsigned i0 = 2u * tid; i0 < nEl; i0 += 2u * MV_NT * MV_U) {
        double2 vx[MV_U];
#pragma unroll
        for (int u = 0; u < MV_U; ++u) {
            const unsigned e = i0 + 2u * MV_NT * u;
            vx[u] = make_double2(0.0, 0.0);
            if (vec && e + 1 < nEl) vx[u] = *reinterpret_cast<const double2 *>(uG + e);
            else if (e < nEl) {
                vx[u].x = uG[e];
                if (e + 1 < nEl) vx[u].y = uG[e + 1];
            }
        }
#pragma unroll
        for (int u = 0; u < MV_U; ++u) {
            const unsigned e = i0 + 2u * MV_NT * u;
            unsigned cc;
            if (e < nEl) X[mv_slot(e, magic, K, cs, cc)] = vx[u].x;
            if (e + 1 < nEl) X[mv_slot(e + 1, magic, K, cs, cc)] = vx[u].y;
        }
    }
    __syncthreads();                                // the records are in place
    // h_e: gathered from the two cell columns of every edge, active levels only
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
    __syncthreads();
    if (n > 0) {
        MvmixTileCol col{H + (size_t)tid * cs, X + (size_t)tid * cs, Y + (size_t)tid * cs};
        mvmix_column<DRAG, STRESS>(col, n, a.dt * a.nu, a.dt * a.drag, b);
    }
    __syncthreads();
    // back: the rows k < n of a column only
    for (unsigned i0 = 2u * tid; i0 < nEl; i0 += 2u * MV_NT) {
        const unsigned e = i0;
        unsigned ca, cb = 0;
        const unsigned qA = mv_slot(e, magic, K, cs, ca);
        const bool okA = (int)(e - ca * K) < hd[ca].w;
        bool okB = false;
        double2 o = make_double2(0.0, 0.0);
        if (okA) o.x = X[qA];
        if (e + 1 < nEl) {
            const unsigned qB = mv_slot(e + 1, magic, K, cs, cb);
            okB = (int)(e + 1 - cb * K) < hd[cb].w;
            if (okB) o.y = X[qB];
        }
        if (vec && okA && okB) *reinterpret_cast<double2 *>(uG + e) = o;
        else {
            if (okA) uG[e] = o.x;
            if (okB) uG[e + 1] = o.y;
        }
    }
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
    __device__ __forceinline__ double h(int k) const { return 0.5 * (h1[k] + h2[k]); }
    __device__ __forceinline__ double x(int k) const { return uc[k]; }
    __device__ __forceinline__ void putG(int k, double v) { gs[k * nE] = v; }
    __device__ __forceinline__ double g(int k) const { return gs[k * nE]; }
    __device__ __forceinline__ void putY(int k, double v) { ys[k * nE] = v; }
    __device__ __forceinline__ double y(int k) const { return ys[k * nE]; }
    __device__ __forceinline__ void emit(int k, double inc) { uc[k] = uc[k] + inc; }
};

template <bool DRAG, bool STRESS>
__global__ __launch_bounds__(BLOCK) void k_mvmix_column(const MomVmixArgs a)
{
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= a.nE) return;
    const int4 r = *reinterpret_cast<const int4 *>(a.ehdr + (size_t)e * 4);
    const int n = mvmix_depth<DRAG, STRESS>(r.w, a.K);
    if (n == 0) return;
    const size_t nEK = (size_t)a.nE * a.K;
    MvmixGlobalCol col{a.h + (size_t)r.x * a.K, a.h + (size_t)r.y * a.K, a.u + (size_t)e * a.K, a.scratch + e, a.scratch + nEK + e, (size_t)a.nE};
    mvmix_column<DRAG, STRESS>(col, n, a.dt * a.nu, a.dt * a.drag, STRESS ? a.dt * a.tau[e] : 0.0);
}

template <bool DRAG, bool STRESS>
static hipError_t launch_mvmix_with(const MomVmixArgs &a, const VmixKernel &k, hipStream_t s)
{
    if (k.form == 1) {
        const size_t lds = k.lds + 12 * (size_t)k.tc;       // the records take 16 bytes a column where vmix_kernel counts 4
        if (lds > 64 * 1024)
            if (hipError_t e = raise_dyn_lds({reinterpret_cast<const void *>(k_mvmix_tile<DRAG, STRESS>)}, 80 * 1024); e != hipSuccess) return e;
        const unsigned magic = (unsigned)((1ull << 32) / (unsigned)a.K) + 1u;
        hipLaunchKernelGGL((k_mvmix_tile<DRAG, STRESS>), dim3((a.nE + k.tc - 1) / k.tc), dim3(MV_NT), lds, s, a, k.tc, a.K | 1, magic);
    } else {
        hipLaunchKernelGGL((k_mvmix_column<DRAG, STRESS>), dim3((a.nE + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, a);
    }
    return hipGetLastError();
}

int momentum_vmix_form(int K, bool generic) { return vmix_kernel(K, generic, 3).form; }

hipError_t launch_momentum_vmix(const MomVmixArgs &a, bool generic, hipStream_t s)
{
    const bool drag = a.drag != 0.0, stress = a.tau != nullptr;
    if (a.nE <= 0 || a.K < 1 || (a.K < 2 && !drag && !stress)) return hipSuccess;
    if ((uint64_t)a.K * 64u >= (1ull << 32)) return hipErrorInvalidValue;
    const VmixKernel k = vmix_kernel(a.K, generic, 3);
    if (k.form == 2 && !a.scratch) return hipErrorInvalidValue;
    return drag ? (stress ? launch_mvmix_with<true, true>(a, k, s) : launch_mvmix_with<true, false>(a, k, s))
                : (stress ? launch_mvmix_with<false, true>(a, k, s) : launch_mvmix_with<false, false>(a, k, s));
}

}  // namespace moka
