// tracer_vmix.hip -- implicit vertical diffusion of the passive tracers of libmoka_hip (gfx950; moka_set_tracer_vertical_diffusion, NOT
// in the reference), forwards behind stage 4 of an RK4 step and backwards at the head of a reversed step.
#include "kernels_common.hpp"

namespace moka {

// ------------------------------------------------------------------------------------------------
// include/moka_hip.h states the recipe; this is it, once, for one column of n = nLev[c] >= 2 active levels and s = dt * kappaV_j:
//     w[k] = s / (0.5 * (h[k] + h[k+1]));   d[k] = (h[k] + w[k-1]) + w[k]  (end rows: one w);   A = diag(h) + tridiag(-w, d - h, -w)
//     forward:  phi_new = x + Solve(Lv(x))        reverse:  X = X + Lv(Solve(X))
// with Solve the Thomas sweep (beta, g, y downwards; z upwards) and Lv the interface-flux difference.  Every operation is rounded once
// (-ffp-contract=off), in the order written in the header, so the two forms below and the numpy twin of the tests agree bit for bit.
// The dependence runs along k and the parallelism across columns: one lane owns one column.  What differs between the forms is where a
// lane keeps its column, which the accessor C hides:
//     h(k), x(k)             the thickness and the field (forward: phi*; reverse: X), read once each, in ascending k
//     putG / g, putY / y     the sweep's two work columns
//     putW / w               reverse only: w[k] for the interface fluxes of the upward sweep
//     emit(k, inc)           field[k] = field[k] + inc
// Levels k >= n are never touched.
// ------------------------------------------------------------------------------------------------
template <bool REV, class C>
__device__ __forceinline__ void vmix_column(C &c, const int n, const double s)
{
    double hk = c.h(0), hn = c.h(1);
    double xm = 0.0, xk = c.x(0), xn = c.x(1);
    double w = s / (0.5 * (hk + hn));               // w[0]
    double beta = hk + w;                           // d[0]
    double y = (REV ? xk : w * (xn - xk)) / beta;
    c.putY(0, y);
    if (REV) c.putW(0, w);
    for (int k = 1; k < n; ++k) {
        const double wp = w;                        // w[k-1]
        xm = xk; xk = xn; hk = hn;
        const double g = wp / beta;
        c.putG(k - 1, g);
        double d, r;
        if (k < n - 1) {
            hn = c.h(k + 1); xn = c.x(k + 1);
            w = s / (0.5 * (hk + hn));
            d = (hk + wp) + w;
            r = REV ? xk : wp * (xm - xk) + w * (xn - xk);
            if (REV) c.putW(k, w);
        } else {
            d = hk + wp;
            r = REV ? xk : wp * (xm - xk);
        }
        beta = d - wp * g;
        y = (r + wp * y) / beta;
        c.putY(k, y);
    }
    if (!REV) {
        double z = y;                               // z[n-1]
        c.emit(n - 1, z);
        for (int k = n - 2; k >= 0; --k) {
            z = c.y(k) + c.g(k) * z;
            c.emit(k, z);
        }
    } else {
        double z1 = y, z2 = 0.0, w1 = 0.0;          // z[k+1], z[k+2], w[k+1]
        for (int k = n - 2; k >= 0; --k) {
            const double z0 = c.y(k) + c.g(k) * z1, w0 = c.w(k);
            c.emit(k + 1, k + 1 == n - 1 ? w0 * (z0 - z1) : w0 * (z0 - z1) + w1 * (z2 - z1));      // Lv(z)[k+1]
            z2 = z1; z1 = z0; w1 = w0;
        }
        c.emit(0, w1 * (z2 - z1));                  // Lv(z)[0] = w[0] * (z[1] - z[0])
    }
}

// ------------------------------------------------------------------------------------------------
// Form 1, tile.  A workgroup of one wave takes tc consecutive cells: their tc * K doubles of a (K, nC) array are one contiguous span,
// fetched with 16-byte lanes (eight loads in flight per lane, h and the field together) into three column sets in LDS,
//     set 0: h, its slot k taking g[k] once h[k] and h[k+1] sit in registers | set 1: the field | set 2: y, then z (forward) or Lv (reverse)
// a column `cs` doubles apart, cs = K | 1 odd: the 32 lanes of a ds_read_b64 group and the 16 of a ds_write_b64 group then hit distinct
// banks (MI355X_MICROARCH.md, LDS table).  Lane l < tc sweeps column l; the result goes back the way it came, active levels only.
// Reverse: w[k] takes the slot of X[k] once that is read, and the write-back adds Lv to the X it re-reads (the tile's own span, just
// fetched: an L2 hit), so that three sets serve both directions.  One tracer is resident at a time: h is fetched again for the next
// one (g has overwritten it; again an L2 hit), which keeps the HBM traffic at (1 + 2 nT) fields and a column at 3 cs doubles.
// vmix_kernel() holds the LDS formula and the choice of tc.
// ------------------------------------------------------------------------------------------------
constexpr int VM_NT = 64;             // threads of a tile-form workgroup: one wave
constexpr int VM_U = 8;               // 16-byte loads a lane has in flight per array while it stages

template <bool REV>
struct VmixTileCol {
    double *hs, *xs, *ys;             // the lane's column in the three sets
    __device__ __forceinline__ double h(int k) const { return hs[k]; }
    __device__ __forceinline__ double x(int k) const { return xs[k]; }
    __device__ __forceinline__ void putG(int k, double v) { hs[k] = v; }
    __device__ __forceinline__ double g(int k) const { return hs[k]; }
    __device__ __forceinline__ void putY(int k, double v) { ys[k] = v; }
    __device__ __forceinline__ double y(int k) const { return ys[k]; }
    __device__ __forceinline__ void putW(int k, double v) { xs[k] = v; }
    __device__ __forceinline__ double w(int k) const { return xs[k]; }
    __device__ __forceinline__ void emit(int k, double inc)
    {
        if (REV) ys[k] = inc;
        else xs[k] = xs[k] + inc;
    }
};

// element e of a tile's span -> its place in a column set (magic = 2^32 / K + 1: exact while e * K < 2^32)
__device__ __forceinline__ unsigned vm_slot(unsigned e, unsigned magic, unsigned K, unsigned cs, unsigned &col)
{
    col = __umulhi(e, magic);
    return col * cs + (e - col * K);
}

template <bool REV>
__global__ __launch_bounds__(VM_NT) void k_vmix_tile(const VmixArgs a, const int tc, const int cs, const unsigned magic)
{
    extern __shared__ __align__(16) unsigned char vm_smem[];
    double *const H = reinterpret_cast<double *>(vm_smem), *const X = H + (size_t)tc * cs, *const Y = X + (size_t)tc * cs;
    int *const nl = reinterpret_cast<int *>(Y + (size_t)tc * cs);
    const int tid = threadIdx.x, K = a.K;
    const int c0 = blockIdx.x * tc, ncol = min(tc, a.nC - c0);
    const unsigned nEl = (unsigned)ncol * (unsigned)K;
    const size_t base = (size_t)c0 * K;
    int n = 0;
    if (tid < ncol) {
        n = a.nLev[c0 + tid];
        if (n < 2) n = 0;                           // a column with fewer than two active levels is left alone
    }
    if (tid < tc) nl[tid] = n;
    VmixTileCol<REV> col{H + (size_t)tid * cs, X + (size_t)tid * cs, Y + (size_t)tid * cs};
    const double *hG = a.h + base;

    for (int j = 0; j < a.nT; ++j) {
        const double kv = a.kv[j];
        if (kv == 0.0) continue;                    // wave-uniform: such a tracer is neither read nor written
        double *fG = a.x + (size_t)j * a.stride + base;
        const bool vec = ((reinterpret_cast<uintptr_t>(hG) | reinterpret_cast<uintptr_t>(fG)) & 15) == 0;
        __syncthreads();                            // the previous tracer's write-back has read its sets
        for (unsigned e0 = 2u * tid; e0 < nEl; e0 += 2u * VM_NT * VM_U) {
            double2 vh[VM_U], vx[VM_U];
#pragma unroll
            for (int u = 0; u < VM_U; ++u) {
                const unsigned e = e0 + 2u * VM_NT * u;
                vh[u] = vx[u] = make_double2(0.0, 0.0);
                if (vec && e + 1 < nEl) {
                    vh[u] = *reinterpret_cast<const double2 *>(hG + e);
                    vx[u] = *reinterpret_cast<const double2 *>(fG + e);
                } else if (e < nEl) {
                    vh[u].x = hG[e]; vx[u].x = fG[e];
                    if (e + 1 < nEl) { vh[u].y = hG[e + 1]; vx[u].y = fG[e + 1]; }
                }
            }
#pragma unroll
            for (int u = 0; u < VM_U; ++u) {
                const unsigned e = e0 + 2u * VM_NT * u;
                unsigned cc;
                if (e < nEl) { const unsigned q = vm_slot(e, magic, K, cs, cc); H[q] = vh[u].x; X[q] = vx[u].x; }
                if (e + 1 < nEl) { const unsigned q = vm_slot(e + 1, magic, K, cs, cc); H[q] = vh[u].y; X[q] = vx[u].y; }
            }
        }
        __syncthreads();
        if (n >= 2) vmix_column<REV>(col, n, a.dt * kv);
        __syncthreads();
        // back: forward the field set, reverse X + Lv; only the active levels of a column are written
        for (unsigned e0 = 2u * tid; e0 < nEl; e0 += 2u * VM_NT * VM_U) {
            double2 vx[VM_U];
            if (REV) {
#pragma unroll
                for (int u = 0; u < VM_U; ++u) {
                    const unsigned e = e0 + 2u * VM_NT * u;
                    vx[u] = make_double2(0.0, 0.0);
                    if (vec && e + 1 < nEl) vx[u] = *reinterpret_cast<const double2 *>(fG + e);
                    else if (e < nEl) {
                        vx[u].x = fG[e];
                        if (e + 1 < nEl) vx[u].y = fG[e + 1];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < VM_U; ++u) {
                const unsigned e = e0 + 2u * VM_NT * u;
                if (e >= nEl) continue;
                unsigned ca, cb = 0;
                const unsigned qa = vm_slot(e, magic, K, cs, ca);
                const bool okA = (int)(e - ca * K) < nl[ca];
                bool okB = false;
                double2 o = make_double2(0.0, 0.0);
                if (okA) o.x = REV ? vx[u].x + Y[qa] : X[qa];
                if (e + 1 < nEl) {
                    const unsigned qb = vm_slot(e + 1, magic, K, cs, cb);
                    okB = (int)(e + 1 - cb * K) < nl[cb];
                    if (okB) o.y = REV ? vx[u].y + Y[qb] : X[qb];
                }
                if (vec && okA && okB) *reinterpret_cast<double2 *>(fG + e) = o;
                else {
                    if (okA) fG[e] = o.x;
                    if (okB) fG[e + 1] = o.y;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Form 2, column.  One lane per column straight from global memory; g and y in a global scratch of 2 * K * nC doubles laid out level-major
// ((K, nC) transposed: the lanes of a wave store side by side); the reverse sweep forms w again from h, the same division with the same
// operands.  Any K, any mesh; the tracers of a column one after the other, so one scratch serves them all.
// ------------------------------------------------------------------------------------------------
struct VmixGlobalCol {
    const double *hc;                 // the column's thickness
    double *fc;                       // ... and field
    double *gs, *ys;                  // scratch: element k at [k * nC]
    size_t nC;
    double s;
    __device__ __forceinline__ double h(int k) const { return hc[k]; }
    __device__ __forceinline__ double x(int k) const { return fc[k]; }
    __device__ __forceinline__ void putG(int k, double v) { gs[k * nC] = v; }
    __device__ __forceinline__ double g(int k) const { return gs[k * nC]; }
    __device__ __forceinline__ void putY(int k, double v) { ys[k * nC] = v; }
    __device__ __forceinline__ double y(int k) const { return ys[k * nC]; }
    __device__ __forceinline__ void putW(int, double) {}
    __device__ __forceinline__ double w(int k) const { return s / (0.5 * (hc[k] + hc[k + 1])); }
    __device__ __forceinline__ void emit(int k, double inc) { fc[k] = fc[k] + inc; }
};

template <bool REV>
__global__ __launch_bounds__(BLOCK) void k_vmix_column(const VmixArgs a)
{
    const int c = blockIdx.x * BLOCK + threadIdx.x;
    if (c >= a.nC) return;
    const int n = a.nLev[c];
    if (n < 2) return;
    const size_t off = (size_t)c * a.K, nCK = (size_t)a.nC * a.K;
    for (int j = 0; j < a.nT; ++j) {
        const double kv = a.kv[j];
        if (kv == 0.0) continue;
        const double s = a.dt * kv;
        VmixGlobalCol col{a.h + off, a.x + (size_t)j * a.stride + off, a.scratch + c, a.scratch + nCK + c, (size_t)a.nC, s};
        vmix_column<REV>(col, n, s);
    }
}

// The kernel that serves a vertical pass, chosen in one place for the launcher, moka_state_tracer_vmix_path and
// moka_tracer_adjoint_vmix_path.  A resident column takes three sets of cs = K | 1 doubles, so a CU's 160 KiB hold 163840 / (24 cs)
// columns at a time, whatever the tile: 111 at K = 60.  That number, not the tile, bounds the lanes that sweep at once, and the sweep is
// a chain of dependent divisions, so what matters is that the resident columns are spread over several waves: one per SIMD at least.
//   tc = 64 (full waves) while four such tiles fit a CU (cs <= 25);
//   tc = 32 (half the lanes of a wave sweep) while two such tiles fit (cs <= 105): at K = 60 three workgroups of 46,976 B share a CU;
//   form 2 beyond that -- fewer than a wave's worth of columns would be resident -- and for kernel variant 3 (generic).
// One tracer per pass (see k_vmix_tile).  lds = 3 * tc * cs * 8 + tc * 4 (the columns' active depths).
VmixKernel vmix_kernel(int K, bool generic)
{
    constexpr size_t cu = 160 * 1024;
    const int cs = K | 1;
    if (!generic && K >= 2)
        for (int tc : {64, 32}) {
            const size_t lds = (size_t)3 * tc * cs * 8 + (size_t)tc * 4;
            if (lds * (tc == 64 ? 4 : 2) <= cu) return {1, lds, tc};
        }
    return {2, 0, 0};
}

template <bool REV>
static hipError_t launch_vmix_dir(const VmixArgs &a, const VmixKernel &k, hipStream_t s)
{
    if (k.form == 1) {
        if (k.lds > 64 * 1024)
            if (hipError_t e = raise_dyn_lds({reinterpret_cast<const void *>(k_vmix_tile<REV>)}, 80 * 1024); e != hipSuccess) return e;
        const unsigned magic = (unsigned)((1ull << 32) / (unsigned)a.K) + 1u;
        hipLaunchKernelGGL(k_vmix_tile<REV>, dim3((a.nC + k.tc - 1) / k.tc), dim3(VM_NT), k.lds, s, a, k.tc, a.K | 1, magic);
    } else {
        hipLaunchKernelGGL(k_vmix_column<REV>, dim3((a.nC + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, a);
    }
    return hipGetLastError();
}

hipError_t launch_tracer_vmix(const VmixArgs &a, bool reverse, bool generic, hipStream_t s)
{
    if (a.nT <= 0 || a.nC <= 0 || a.K < 2) return hipSuccess;
    const VmixKernel k = vmix_kernel(a.K, generic);
    return reverse ? launch_vmix_dir<true>(a, k, s) : launch_vmix_dir<false>(a, k, s);
}

}  // namespace moka
