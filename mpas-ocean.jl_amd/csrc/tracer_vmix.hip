// tracer_vmix.hip -- implicit vertical diffusion of the passive tracers of libmoka_hip (gfx950; moka_set_tracer_vertical_diffusion, NOT
// in the reference), forwards behind stage 4 of an RK4 step and backwards at the head of a reversed step, where the gradient instances
// also form the density of d J / d kappaV (moka_tracer_adjoint_want_vertical_gradient).
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
// GRAD (reverse only): the column also yields e[k] = (z[k] - z[k+1]) * c[k], c[k] = (p[k] - p[k+1]) * (dt / (0.5 * (h[k] + h[k+1]))),
// for the interfaces k = 0 .. n-2, with p the recorded phi_new; X takes exactly the operations of the instance without the switch.
//     p(k)                   the recorded field, read once, in ascending k, beside h(k)
//     putC / c               c[k], formed on the way down where p[k], p[k+1], h[k], h[k+1] sit in registers
//     emitE(k, e)            D[k] = D[k] - e (the tile form defers the subtraction to its write-back)
// FLD (a tracer with a diffusivity field, moka_tracer_vertical_field_upload): s is not one number but s[k] = dt * f[k] per interface,
//     s(k)                   read once, in ascending k, beside h(k + 1) and before putY(k)
// and nothing else changes: where f is uniform the product is the scalar's, hence every bit is.
// Levels k >= n are never touched, and of the field no row k >= n - 1.
// ------------------------------------------------------------------------------------------------
template <bool REV, bool GRAD, bool FLD, class C>
__device__ __forceinline__ void vmix_column(C &c, const int n, const double s, const double dt)
{
    static_assert(REV || !GRAD, "the gradient belongs to the reverse pass");
    double hk = c.h(0), hn = c.h(1);
    double xm = 0.0, xk = c.x(0), xn = c.x(1);
    double pk = 0.0, pn = 0.0;
    double hm = 0.5 * (hk + hn);
    double w = (FLD ? c.s(0) : s) / hm;             // w[0]
    if (GRAD) {
        pk = c.p(0); pn = c.p(1);
        c.putC(0, (pk - pn) * (dt / hm));
    }
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
            hm = 0.5 * (hk + hn);
            w = (FLD ? c.s(k) : s) / hm;
            d = (hk + wp) + w;
            r = REV ? xk : wp * (xm - xk) + w * (xn - xk);
            if (REV) c.putW(k, w);
            if (GRAD) {
                pk = pn; pn = c.p(k + 1);
                c.putC(k, (pk - pn) * (dt / hm));
            }
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
            if (GRAD) c.emitE(k, (z0 - z1) * c.c(k));
            c.emit(k + 1, k + 1 == n - 1 ? w0 * (z0 - z1) : w0 * (z0 - z1) + w1 * (z2 - z1));      // Lv(z)[k+1]
            z2 = z1; z1 = z0; w1 = w0;
        }
        c.emit(0, w1 * (z2 - z1));                  // Lv(z)[0] = w[0] * (z[1] - z[0])
    }
}

// The gradient of a flagged tracer whose kappaV is zero in this step: A = diag(h), so z[k] = X[k] / h[k]; X is read and nothing is
// added to it (a derivative at zero, as for kappa4).
template <class C>
__device__ __forceinline__ void vgrad_column_at_zero(C &c, const int n, const double dt)
{
    double hk = c.h(0), pk = c.p(0);
    double zk = c.x(0) / hk;
    for (int k = 0; k < n - 1; ++k) {
        const double hn = c.h(k + 1), pn = c.p(k + 1);
        const double zn = c.x(k + 1) / hn;
        const double cc = (pk - pn) * (dt / (0.5 * (hk + hn)));
        c.emitE(k, (zk - zn) * cc);
        hk = hn; pk = pn; zk = zn;
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
// Gradient instances: a fourth set, staged with p beside h and X; its slot k takes c[k] on the way down (p[k] and p[k+1] are in
// registers by then) and e[k] on the way up; the tile's span of D is then read, reduced by e and written back the way X is, interface
// rows k < n - 1 only.  One field read and one read-modify-write more per flagged tracer, a column at 4 cs doubles.
// Field instances: s[k] = dt * f[k] of a tracer with a diffusivity field is staged into set 2 beside h and the field; the sweep reads
// slot k at iteration k, before it writes y[k] there, as g overwrites h -- no further set, the LDS formula and the choice of tc stand,
// and the pass moves one more field per such tracer.  A tracer without a field stages nothing there and sweeps with its dt * kv.
// vmix_kernel() holds the LDS formula and the choice of tc.
// ------------------------------------------------------------------------------------------------
constexpr int VM_NT = 64;             // threads of a tile-form workgroup: one wave
constexpr int VM_U = 8;               // 16-byte loads a lane has in flight per array while it stages

template <bool REV>
struct VmixTileCol {
    double *hs, *xs, *ys, *ps;        // the lane's column in the sets (ps: gradient instances only)
    __device__ __forceinline__ double h(int k) const { return hs[k]; }
    __device__ __forceinline__ double x(int k) const { return xs[k]; }
    __device__ __forceinline__ void putG(int k, double v) { hs[k] = v; }
    __device__ __forceinline__ double g(int k) const { return hs[k]; }
    __device__ __forceinline__ void putY(int k, double v) { ys[k] = v; }
    __device__ __forceinline__ double y(int k) const { return ys[k]; }
    __device__ __forceinline__ double s(int k) const { return ys[k]; }          // field instances: staged where y[k] goes once s[k] is read
    __device__ __forceinline__ void putW(int k, double v) { xs[k] = v; }
    __device__ __forceinline__ double w(int k) const { return xs[k]; }
    __device__ __forceinline__ void emit(int k, double inc)
    {
        if (REV) ys[k] = inc;
        else xs[k] = xs[k] + inc;
    }
    __device__ __forceinline__ double p(int k) const { return ps[k]; }
    __device__ __forceinline__ void putC(int k, double v) { ps[k] = v; }
    __device__ __forceinline__ double c(int k) const { return ps[k]; }
    __device__ __forceinline__ void emitE(int k, double e) { ps[k] = e; }
};

// element e of a tile's span -> its place in a column set (magic = 2^32 / K + 1: exact while e * K < 2^32)
__device__ __forceinline__ unsigned vm_slot(unsigned e, unsigned magic, unsigned K, unsigned cs, unsigned &col)
{
    col = __umulhi(e, magic);
    return col * cs + (e - col * K);
}

// A column set back into the tile's span dG, 16-byte lanes, the rows k < nl[column] - SHORT of a column only:
// MODE 0: dG = S (forward: the field set)    MODE 1: dG = dG + S (reverse: X + Lv)    MODE 2: dG = dG - S (the density: D - e)
template <int MODE, int SHORT>
__device__ __forceinline__ void vm_write_back(double *dG, const double *S, const int *nl, const bool vec, const int tid, const unsigned nEl,
                                              const unsigned magic, const unsigned K, const unsigned cs)
{
    for (unsigned e0 = 2u * tid; e0 < nEl; e0 += 2u * VM_NT * VM_U) {
        double2 vx[VM_U];
        if (MODE != 0) {
#pragma unroll
            for (int u = 0; u < VM_U; ++u) {
                const unsigned e = e0 + 2u * VM_NT * u;
                vx[u] = make_double2(0.0, 0.0);
                if (vec && e + 1 < nEl) vx[u] = *reinterpret_cast<const double2 *>(dG + e);
                else if (e < nEl) {
                    vx[u].x = dG[e];
                    if (e + 1 < nEl) vx[u].y = dG[e + 1];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < VM_U; ++u) {
            const unsigned e = e0 + 2u * VM_NT * u;
            if (e >= nEl) continue;
            unsigned ca, cb = 0;
            const unsigned qa = vm_slot(e, magic, K, cs, ca);
            const bool okA = (int)(e - ca * K) < nl[ca] - SHORT;
            bool okB = false;
            double2 o = make_double2(0.0, 0.0);
            if (okA) o.x = MODE == 0 ? S[qa] : MODE == 1 ? vx[u].x + S[qa] : vx[u].x - S[qa];
            if (e + 1 < nEl) {
                const unsigned qb = vm_slot(e + 1, magic, K, cs, cb);
                okB = (int)(e + 1 - cb * K) < nl[cb] - SHORT;
                if (okB) o.y = MODE == 0 ? S[qb] : MODE == 1 ? vx[u].y + S[qb] : vx[u].y - S[qb];
            }
            if (vec && okA && okB) *reinterpret_cast<double2 *>(dG + e) = o;
            else {
                if (okA) dG[e] = o.x;
                if (okB) dG[e + 1] = o.y;
            }
        }
    }
}

template <bool REV, bool GRAD, bool FLD>
__device__ __forceinline__ void vmix_tile(const VmixArgs &a, const int tc, const int cs, const unsigned magic)
{
    extern __shared__ __align__(16) unsigned char vm_smem[];
    double *const H = reinterpret_cast<double *>(vm_smem), *const X = H + (size_t)tc * cs, *const Y = X + (size_t)tc * cs;
    double *const P = Y + (size_t)tc * cs;          // the fourth set exists in the gradient instances only
    int *const nl = reinterpret_cast<int *>(GRAD ? P + (size_t)tc * cs : P);
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
    VmixTileCol<REV> col{H + (size_t)tid * cs, X + (size_t)tid * cs, Y + (size_t)tid * cs, P + (size_t)tid * cs};
    const double *hG = a.h + base;

    for (int j = 0; j < a.nT; ++j) {
        const double kv = a.kv[j];
        const int f = GRAD ? a.gslot[j] : -1;       // wave-uniform, like kv
        const double *const sF = FLD ? a.fld[j] : nullptr;      // ... and like the tracer's diffusivity field, which replaces kv
        if (!(FLD && sF) && kv == 0.0 && f < 0) continue;       // such a tracer is neither read nor written
        double *fG = a.x + (size_t)j * a.stride + base;
        const double *pG = f >= 0 ? a.p + (size_t)f * a.stride + base : hG;
        double *dG = f >= 0 ? a.D + (size_t)f * a.stride + base : fG;
        const double *sG = FLD && sF ? sF + base : hG;
        const bool vec = ((reinterpret_cast<uintptr_t>(hG) | reinterpret_cast<uintptr_t>(fG) | reinterpret_cast<uintptr_t>(pG) |
                           reinterpret_cast<uintptr_t>(dG) | reinterpret_cast<uintptr_t>(sG)) & 15) == 0;
        __syncthreads();                            // the previous tracer's write-back has read its sets
        for (unsigned e0 = 2u * tid; e0 < nEl; e0 += 2u * VM_NT * VM_U) {
            double2 vh[VM_U], vx[VM_U], vp[VM_U], vs[VM_U];
#pragma unroll
            for (int u = 0; u < VM_U; ++u) {
                const unsigned e = e0 + 2u * VM_NT * u;
                vh[u] = vx[u] = vp[u] = vs[u] = make_double2(0.0, 0.0);
                if (vec && e + 1 < nEl) {
                    vh[u] = *reinterpret_cast<const double2 *>(hG + e);
                    vx[u] = *reinterpret_cast<const double2 *>(fG + e);
                    if (GRAD && f >= 0) vp[u] = *reinterpret_cast<const double2 *>(pG + e);
                    if (FLD && sF) vs[u] = *reinterpret_cast<const double2 *>(sG + e);
                } else if (e < nEl) {
                    vh[u].x = hG[e]; vx[u].x = fG[e];
                    if (GRAD && f >= 0) vp[u].x = pG[e];
                    if (FLD && sF) vs[u].x = sG[e];
                    if (e + 1 < nEl) {
                        vh[u].y = hG[e + 1]; vx[u].y = fG[e + 1];
                        if (GRAD && f >= 0) vp[u].y = pG[e + 1];
                        if (FLD && sF) vs[u].y = sG[e + 1];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < VM_U; ++u) {
                const unsigned e = e0 + 2u * VM_NT * u;
                unsigned cc;
                if (e < nEl) {
                    const unsigned q = vm_slot(e, magic, K, cs, cc);
                    H[q] = vh[u].x; X[q] = vx[u].x;
                    if (GRAD && f >= 0) P[q] = vp[u].x;
                    if (FLD && sF) Y[q] = a.dt * vs[u].x;       // s[k] = dt * f[k], the one product
                }
                if (e + 1 < nEl) {
                    const unsigned q = vm_slot(e + 1, magic, K, cs, cc);
                    H[q] = vh[u].y; X[q] = vx[u].y;
                    if (GRAD && f >= 0) P[q] = vp[u].y;
                    if (FLD && sF) Y[q] = a.dt * vs[u].y;
                }
            }
        }
        __syncthreads();
        if (n >= 2) {
            if (GRAD && f >= 0) {
                if (FLD && sF) vmix_column<REV, GRAD, true>(col, n, 0.0, a.dt);
                else if (kv != 0.0) vmix_column<REV, GRAD, false>(col, n, a.dt * kv, a.dt);
                else vgrad_column_at_zero(col, n, a.dt);
            } else if (FLD && sF) vmix_column<REV, false, true>(col, n, 0.0, a.dt);
            else vmix_column<REV, false, false>(col, n, a.dt * kv, a.dt);
        }
        __syncthreads();
        // back: forward the field set, reverse X + Lv; only the active levels of a column are written
        if (!REV) vm_write_back<0, 0>(fG, X, nl, vec, tid, nEl, magic, K, cs);
        else if ((FLD && sF) || kv != 0.0) vm_write_back<1, 0>(fG, Y, nl, vec, tid, nEl, magic, K, cs);
        if (GRAD && f >= 0) vm_write_back<2, 1>(dG, P, nl, vec, tid, nEl, magic, K, cs);
    }
}

// the forward and the plain reverse pass, and the gradient instance of the reverse pass; FLD: their field instances (a.fld != nullptr)
template <bool REV, bool FLD>
__global__ __launch_bounds__(VM_NT) void k_vmix_tile(const VmixArgs a, const int tc, const int cs, const unsigned magic)
{
    vmix_tile<REV, false, FLD>(a, tc, cs, magic);
}

template <bool FLD>
__global__ __launch_bounds__(VM_NT) void k_vmix_tile_grad(const VmixArgs a, const int tc, const int cs, const unsigned magic)
{
    vmix_tile<true, true, FLD>(a, tc, cs, magic);
}

// ------------------------------------------------------------------------------------------------
// Form 2, column.  One lane per column straight from global memory; g and y in a global scratch of 2 * K * nC doubles laid out level-major
// ((K, nC) transposed: the lanes of a wave store side by side); the reverse sweep forms w again from h, the same division with the same
// operands, and the gradient instances c[k] again from p and h, likewise.  Any K, any mesh; the tracers of a column one after the
// other, so one scratch serves them all.  FLD: s[k] = dt * f[k] from the tracer's field column, the product formed again wherever w is.
// ------------------------------------------------------------------------------------------------
template <bool FLD>
struct VmixGlobalCol {
    const double *hc;                 // the column's thickness
    double *fc;                       // ... and field
    double *gs, *ys;                  // scratch: element k at [k * nC]
    size_t nC;
    double su;                        // dt * kappaV of a tracer without a field
    const double *pc;                 // gradient instances: the column's recorded phi_new
    double *dc;                       // ... and density
    double dt;
    const double *sc;                 // field instances: the column's diffusivity field
    __device__ __forceinline__ double h(int k) const { return hc[k]; }
    __device__ __forceinline__ double x(int k) const { return fc[k]; }
    __device__ __forceinline__ double s(int k) const { return dt * sc[k]; }
    __device__ __forceinline__ void putG(int k, double v) { gs[k * nC] = v; }
    __device__ __forceinline__ double g(int k) const { return gs[k * nC]; }
    __device__ __forceinline__ void putY(int k, double v) { ys[k * nC] = v; }
    __device__ __forceinline__ double y(int k) const { return ys[k * nC]; }
    __device__ __forceinline__ void putW(int, double) {}
    __device__ __forceinline__ double w(int k) const { return (FLD ? dt * sc[k] : su) / (0.5 * (hc[k] + hc[k + 1])); }
    __device__ __forceinline__ void emit(int k, double inc) { fc[k] = fc[k] + inc; }
    __device__ __forceinline__ double p(int k) const { return pc[k]; }
    __device__ __forceinline__ void putC(int, double) {}
    __device__ __forceinline__ double c(int k) const { return (pc[k] - pc[k + 1]) * (dt / (0.5 * (hc[k] + hc[k + 1]))); }
    __device__ __forceinline__ void emitE(int k, double e) { dc[k] = dc[k] - e; }
};

template <bool REV, bool GRAD, bool FLD>
__device__ __forceinline__ void vmix_columns(const VmixArgs &a)
{
    const int c = blockIdx.x * BLOCK + threadIdx.x;
    if (c >= a.nC) return;
    const int n = a.nLev[c];
    if (n < 2) return;
    const size_t off = (size_t)c * a.K, nCK = (size_t)a.nC * a.K;
    for (int j = 0; j < a.nT; ++j) {
        const double kv = a.kv[j];
        const int f = GRAD ? a.gslot[j] : -1;
        const double *const sF = FLD ? a.fld[j] : nullptr;
        if (FLD && sF) {
            VmixGlobalCol<true> col{a.h + off, a.x + (size_t)j * a.stride + off, a.scratch + c, a.scratch + nCK + c, (size_t)a.nC, 0.0,
                                    f >= 0 ? a.p + (size_t)f * a.stride + off : nullptr, f >= 0 ? a.D + (size_t)f * a.stride + off : nullptr, a.dt,
                                    sF + off};
            if (GRAD && f >= 0) vmix_column<REV, GRAD, true>(col, n, 0.0, a.dt);
            else vmix_column<REV, false, true>(col, n, 0.0, a.dt);
            continue;
        }
        if (kv == 0.0 && f < 0) continue;
        const double s = a.dt * kv;
        VmixGlobalCol<false> col{a.h + off, a.x + (size_t)j * a.stride + off, a.scratch + c, a.scratch + nCK + c, (size_t)a.nC, s,
                                 f >= 0 ? a.p + (size_t)f * a.stride + off : nullptr, f >= 0 ? a.D + (size_t)f * a.stride + off : nullptr, a.dt,
                                 nullptr};
        if (GRAD && f >= 0) {
            if (kv != 0.0) vmix_column<REV, GRAD, false>(col, n, s, a.dt);
            else vgrad_column_at_zero(col, n, a.dt);
        } else vmix_column<REV, false, false>(col, n, s, a.dt);
    }
}

template <bool REV, bool FLD>
__global__ __launch_bounds__(BLOCK) void k_vmix_column(const VmixArgs a)
{
    vmix_columns<REV, false, FLD>(a);
}

template <bool FLD>
__global__ __launch_bounds__(BLOCK) void k_vmix_column_grad(const VmixArgs a)
{
    vmix_columns<true, true, FLD>(a);
}

// The kernel that serves a vertical pass, chosen in one place for the launcher, moka_state_tracer_vmix_path and
// moka_tracer_adjoint_vmix_path.  A resident column takes `sets` sets of cs = K | 1 doubles -- three, or four in the gradient instances
// -- so a CU's 160 KiB hold 163840 / (8 sets cs) columns at a time, whatever the tile: 111 at K = 60 with three sets.  That number, not
// the tile, bounds the lanes that sweep at once, and the sweep is a chain of dependent divisions, so what matters is that the resident
// columns are spread over several waves: one per SIMD at least.
//   tc = 64 (full waves) while four such tiles fit a CU (three sets: cs <= 25; four: cs <= 19);
//   tc = 32 (half the lanes of a wave sweep) while two such tiles fit (three sets: cs <= 105, at K = 60 three workgroups of 46,976 B
//   share a CU; four: cs <= 79, a tile of 81,024 B at cs = 79 and two workgroups of 62,592 B at K = 60);
//   form 2 beyond that -- fewer than a wave's worth of columns would be resident -- and for kernel variant 3 (generic).
// One tracer per pass (see vmix_tile).  lds = sets * tc * cs * 8 + tc * 4 (the columns' active depths).
VmixKernel vmix_kernel(int K, bool generic, int sets)
{
    constexpr size_t cu = 160 * 1024;
    const int cs = K | 1;
    if (!generic && K >= 2)
        for (int tc : {64, 32}) {
            const size_t lds = (size_t)sets * tc * cs * 8 + (size_t)tc * 4;
            if (lds * (tc == 64 ? 4 : 2) <= cu) return {1, lds, tc};
        }
    return {2, 0, 0};
}

static hipError_t launch_vmix_with(void (*tile)(VmixArgs, int, int, unsigned), void (*column)(VmixArgs), const VmixArgs &a, const VmixKernel &k,
                                   hipStream_t s)
{
    if (k.form == 1) {
        if (k.lds > 64 * 1024)
            if (hipError_t e = raise_dyn_lds({reinterpret_cast<const void *>(tile)}, 80 * 1024); e != hipSuccess) return e;
        const unsigned magic = (unsigned)((1ull << 32) / (unsigned)a.K) + 1u;
        hipLaunchKernelGGL(tile, dim3((a.nC + k.tc - 1) / k.tc), dim3(VM_NT), k.lds, s, a, k.tc, a.K | 1, magic);
    } else {
        hipLaunchKernelGGL(column, dim3((a.nC + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, a);
    }
    return hipGetLastError();
}

hipError_t launch_tracer_vmix(const VmixArgs &a, bool reverse, bool generic, hipStream_t s)
{
    if (a.nT <= 0 || a.nC <= 0 || a.K < 2) return hipSuccess;
    if (a.gslot) {
        if (!reverse || !a.p || !a.D) return hipErrorInvalidValue;
        const VmixKernel k = vmix_kernel(a.K, generic, 4);
        return a.fld ? launch_vmix_with(k_vmix_tile_grad<true>, k_vmix_column_grad<true>, a, k, s)
                     : launch_vmix_with(k_vmix_tile_grad<false>, k_vmix_column_grad<false>, a, k, s);
    }
    const VmixKernel k = vmix_kernel(a.K, generic);       // (the field instances stage s into set 2: the same sets, the same tiles)
    if (a.fld)
        return reverse ? launch_vmix_with(k_vmix_tile<true, true>, k_vmix_column<true, true>, a, k, s)
                       : launch_vmix_with(k_vmix_tile<false, true>, k_vmix_column<false, true>, a, k, s);
    return reverse ? launch_vmix_with(k_vmix_tile<true, false>, k_vmix_column<true, false>, a, k, s)
                   : launch_vmix_with(k_vmix_tile<false, false>, k_vmix_column<false, false>, a, k, s);
}

}  // namespace moka
