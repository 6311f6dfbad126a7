// api.hip -- C ABI of libmoka_hip.so (include/moka_hip.h): version, errors and tuning, the context, the device mesh and the stand-alone
// operators.  The state and its steps: api_state.hip; tracers: api_tracers.hip; the three tapes: api_tracer_tape.hip, api_tape.hip,
// api_forced_tape.hip; the objects behind the handles: state.hpp, tapes.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "state.hpp"

namespace moka {

void fill_mesh_info(const Plan &p, moka_mesh_info *info);

// Process-wide launch-shape switches (moka_set_tuning / moka_get_tuning; include/moka_hip.h lists the keys, kernels.hpp names them):
// the default, and either a bit mask whose bits each name kernel instances (mask != 0) or the largest value accepted (from 0).
struct TuningEntry {
    int mask, max;
    std::atomic<int> value;
    TuningEntry(int def, int m, int x) : mask(m), max(x), value(def) {}
    bool exists() const { return mask != 0 || max >= 0; }
    bool accepts(int v) const { return mask ? (v & ~mask) == 0 : v >= 0 && v <= max; }
};
static TuningEntry g_tuning[] = {
    {0, 0, -1},                                              // (no key 0)
    {1 << 0, 0x7f | 1 << 10 | 1 << 11, 0},                   // 1 TUNE_F32_WIDE: fp32 modes 0-6, lean 10 / 11 (launch_rec2c_f32)
    {1, 0, 1},                                               // 2 TUNE_FE_PREV
    {1, 0, 1},                                               // 3 TUNE_CURL_FUSED
    {1, 0, 1},                                               // 4 TUNE_FE_LEAN
    {0, 0, 3},                                               // 5 TUNE_NL_SHAPE: shapes 0-3 (nl_stage_kernel)
    {0, 0, INT_MAX},                                         // 6 TUNE_NL_CAP: vertex rows, 0 = no limit
    {0, 0, 1},                                               // 7 TUNE_RK13
    {1 << 0 | 1 << 1 | 1 << 7, 0xf | 7 << 7 | 1 << 16, 0},   // 8 TUNE_PAIR: pair instances 0-3, 7-9; bit 16 test hook (launch_rec2c_pair)
    {1, 0, 1},                                               // 9 TUNE_FE_LEAN_INST
    {0, 0, -1},                                              // (no key 10)
    {0, 0, -1},                                              // (no key 11)
    {1, 0, 1},                                               // 12 TUNE_RK_HANDOFF
};
constexpr int N_TUNING = sizeof(g_tuning) / sizeof(g_tuning[0]);

int tuning(TuningKey key) { return g_tuning[key].value.load(); }

}  // namespace moka

namespace mk {

int fail(moka_ctx *ctx, int code, const std::string &msg)
{
    set_error(msg);
    if (ctx) ctx->err = msg;
    return code;
}

int lanes_per_column(int K)
{
    int l = 1;
    while (l < K && l < 64) l <<= 1;
    return l;
}

// Rule of this file: no null-stream hipMemcpy / hipMemset after context creation.  The context's streams are non-blocking,
// i.e. NOT ordered against the null stream, so a null-stream copy can overtake (or be overtaken by) a hipMemsetAsync queued
// on the context stream (the tape-list race of round 1).  Every host->device copy goes through h2d(): on the context's
// stream, then synchronised (the source is usually a temporary).  tests/test_source_rules.py
// (test_no_null_stream_copies_in_the_library) looks for offenders.
int h2d(moka_ctx *ctx, void *dst, const void *src, size_t bytes)
{
    if (!bytes) return MOKA_OK;
    HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return MOKA_OK;
}

int ensure_op_bufs(moka_mesh *m)
{
    const Plan &p = m->plan;
    const size_t need = (size_t)p.K * std::max(p.nE, std::max(p.nC, p.nV));
    if (m->opBufElems >= need) return MOKA_OK;
    for (auto &b : m->opBuf) {
        if (b) HIPCHK(m->ctx, hipFree(b));
        b = nullptr;
    }
    for (auto &b : m->opBuf) HIPCHK(m->ctx, hipMalloc((void **)&b, need * sizeof(double)));
    m->opBufElems = need;
    return MOKA_OK;
}

const int32_t *perm_of(const moka_mesh *m, int kind)
{
    return kind == MOKA_CELL ? m->dev.cellN2O : kind == MOKA_EDGE ? m->dev.edgeN2O : m->dev.vertN2O;
}

// host (caller numbering) -> device field (device numbering)
int put_rows(moka_mesh *m, double *dst, const double *host, int kind, int64_t n, int K, bool f32)
{
    int rc = ensure_op_bufs(m);
    if (rc) return rc;
    hipStream_t s = m->ctx->stream;
    HIPCHK(m->ctx, hipMemcpyAsync(m->opBuf[2], host, (size_t)n * K * sizeof(double), hipMemcpyHostToDevice, s));
    if (f32) HIPCHK(m->ctx, launch_permute_rows_f32(dst, m->opBuf[2], perm_of(m, kind), n, K, 1, s));   // rounds to fp32
    else HIPCHK(m->ctx, launch_permute_rows(dst, m->opBuf[2], perm_of(m, kind), n, K, 1, s));
    HIPCHK(m->ctx, hipStreamSynchronize(s));
    return MOKA_OK;
}

int get_rows(moka_mesh *m, double *host, const double *src, int kind, int64_t n, int K, bool f32)
{
    int rc = ensure_op_bufs(m);
    if (rc) return rc;
    hipStream_t s = m->ctx->stream;
    if (f32) HIPCHK(m->ctx, launch_permute_rows_f32(m->opBuf[2], src, perm_of(m, kind), n, K, 0, s));
    else HIPCHK(m->ctx, launch_permute_rows(m->opBuf[2], src, perm_of(m, kind), n, K, 0, s));
    HIPCHK(m->ctx, hipMemcpyAsync(host, m->opBuf[2], (size_t)n * K * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(m->ctx, hipStreamSynchronize(s));
    return MOKA_OK;
}

}  // namespace mk

using namespace mk;

extern "C" {

const char *moka_version(void) { return "moka-hip 0.1.0 (gfx950)"; }

const char *moka_last_error(const moka_ctx *ctx) { return ctx ? ctx->err.c_str() : moka::get_error(); }

int moka_ctx_create(int device, moka_ctx **out)
{
    if (!out) return fail(nullptr, MOKA_ERR_ARG, "out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, MOKA_ERR_NO_DEVICE,
                    std::string("no HIP device available (libmoka_hip has no CPU fallback): ") +
                        (e != hipSuccess ? hipGetErrorString(e) : "device count is 0"));
    if (device < 0 || device >= ndev) return fail(nullptr, MOKA_ERR_ARG, "device index out of range");
    HIPCHK(nullptr, hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(nullptr, hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, MOKA_ERR_NO_DEVICE,
                    std::string("device is ") + prop.gcnArchName + ", this library carries gfx950 code objects only");
    moka_ctx *c = new (std::nothrow) moka_ctx();
    if (!c) return fail(nullptr, MOKA_ERR_ALLOC, "out of host memory");
    c->device = device;
    c->nCUs = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    hipError_t e1 = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    hipError_t e2 = hipEventCreate(&c->ev0);
    hipError_t e3 = hipEventCreate(&c->ev1);
    if (e1 == hipSuccess) {
        // the comm stream carries the boundary patches, pack / unpack and the halo transport: highest priority, so that its
        // few workgroups are dispatched ahead of the thousands the interior launch has queued
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        e1 = hipStreamCreateWithPriority(&c->comm, hipStreamNonBlocking, hi);
    }
    if (e2 == hipSuccess) e2 = hipEventCreateWithFlags(&c->evBoundary, hipEventDisableTiming);
    if (e2 == hipSuccess) e2 = hipEventCreateWithFlags(&c->evInterior, hipEventDisableTiming);
    if (e3 == hipSuccess) e3 = hipEventCreateWithFlags(&c->evHalo, hipEventDisableTiming);
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) {
        moka_ctx_destroy(c);                  // destroys whatever was created
        return fail(nullptr, MOKA_ERR_HIP, "failed to create stream/events");
    }
    *out = c;
    return MOKA_OK;
}

void moka_ctx_destroy(moka_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->comm) { (void)hipStreamSynchronize(ctx->comm); (void)hipStreamDestroy(ctx->comm); }
    for (hipEvent_t e : {ctx->evBoundary, ctx->evInterior, ctx->evHalo}) if (e) (void)hipEventDestroy(e);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    for (hipEvent_t e : ctx->evPool) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->marks) (void)hipEventDestroy(e);
    if (ctx->bwBuf) (void)hipFree(ctx->bwBuf);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int moka_sync(moka_ctx *ctx)
{
    if (!ctx) return fail(nullptr, MOKA_ERR_ARG, "ctx is NULL");
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->comm));
    return MOKA_OK;
}

int moka_ctx_streams(moka_ctx *ctx, void **compute, void **comm)
{
    if (!ctx) return fail(nullptr, MOKA_ERR_ARG, "ctx is NULL");
    if (compute) *compute = (void *)ctx->stream;
    if (comm) *comm = (void *)ctx->comm;
    return MOKA_OK;
}

int moka_timer_start(moka_ctx *ctx)
{
    if (!ctx) return fail(nullptr, MOKA_ERR_ARG, "ctx is NULL");
    HIPCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    return MOKA_OK;
}

int moka_timer_stop(moka_ctx *ctx, float *elapsed_ms)
{
    if (!ctx || !elapsed_ms) return fail(ctx, MOKA_ERR_ARG, "NULL argument");
    HIPCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    HIPCHK(ctx, hipEventSynchronize(ctx->ev1));
    HIPCHK(ctx, hipEventElapsedTime(elapsed_ms, ctx->ev0, ctx->ev1));
    return MOKA_OK;
}

// PCI bus id ("0000:c5:00.0") of the context's device: lets a caller find the device's clock / power files in sysfs
// (/sys/bus/pci/devices/<id>/pp_dpm_sclk ...) and count distinct devices among the ranks of a launch.
int moka_ctx_pci_bus_id(moka_ctx *ctx, char *buf, int32_t len)
{
    if (!ctx || !buf || len < 16) return fail(ctx, MOKA_ERR_ARG, "buf is NULL or shorter than 16 bytes");
    HIPCHK(ctx, hipDeviceGetPCIBusId(buf, len, ctx->device));
    return MOKA_OK;
}

// Per-step statistics of a timed region (bench.py: median / min / max of the step times).  moka_mark records one event on the
// compute stream; n marks give n - 1 intervals.  moka_marks_reset forgets them (the events are kept for reuse).
int moka_mark(moka_ctx *ctx)
{
    if (!ctx) return fail(nullptr, MOKA_ERR_ARG, "ctx is NULL");
    if (ctx->marksUsed == ctx->marks.size()) {
        hipEvent_t e = nullptr;
        HIPCHK(ctx, hipEventCreate(&e));
        ctx->marks.push_back(e);
    }
    HIPCHK(ctx, hipEventRecord(ctx->marks[ctx->marksUsed++], ctx->stream));
    return MOKA_OK;
}

int moka_marks_reset(moka_ctx *ctx)
{
    if (!ctx) return fail(nullptr, MOKA_ERR_ARG, "ctx is NULL");
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->marksUsed = 0;
    return MOKA_OK;
}

// ms[i] = time between mark i and mark i + 1 (at most `capacity` intervals); *n = number of intervals available
int moka_marks_read(moka_ctx *ctx, int64_t capacity, double *ms, int64_t *n)
{
    if (!ctx || !n || (capacity > 0 && !ms)) return fail(ctx, MOKA_ERR_ARG, "NULL argument");
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const int64_t have = ctx->marksUsed > 0 ? (int64_t)ctx->marksUsed - 1 : 0;
    *n = have;
    for (int64_t i = 0; i < have && i < capacity; ++i) {
        float t = 0.f;
        HIPCHK(ctx, hipEventElapsedTime(&t, ctx->marks[i], ctx->marks[i + 1]));
        ms[i] = t;
    }
    return MOKA_OK;
}

// Same-run bandwidth calibration: what this device, in the state it is in NOW, moves with a plain 16-byte-per-lane copy and a
// read-only sweep (MI355X_MICROARCH.md quotes 6.29 TB/s for the copy).  `bytes` = total footprint (two halves: source and
// destination); every launch is timed on its own with HIP events on the compute stream, the best of `iters` is reported
// (the first launch also faults the pages in).  gbs[0] = copy, bytes read + written per second; gbs[1] = read-only sweep of both
// halves; gbs[2] = mean copy rate over the launches; gbs[3] = gather of 480-byte rows in a scattered order, a half-wave per
// row (the access pattern of the stage kernels at 60 layers).  bytes = 0 releases the buffers.
int moka_bw_probe(moka_ctx *ctx, int64_t bytes, int iters, double gbs[4])
{
    if (!ctx) return fail(nullptr, MOKA_ERR_ARG, "ctx is NULL");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (bytes <= 0) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->bwBuf) HIPCHK(ctx, hipFree(ctx->bwBuf));
        ctx->bwBuf = nullptr; ctx->bwBytes = 0;
        return MOKA_OK;
    }
    if (!gbs || iters < 1) return fail(ctx, MOKA_ERR_ARG, "gbs is NULL or iters < 1");
    const size_t half = ((size_t)bytes / 2) & ~(size_t)4095;
    if (half < ((size_t)1 << 20)) return fail(ctx, MOKA_ERR_ARG, "bandwidth probe: at least 2 MiB");
    hipStream_t s = ctx->stream;
    if (ctx->bwBytes != 2 * half) {
        if (ctx->bwBuf) { HIPCHK(ctx, hipStreamSynchronize(s)); HIPCHK(ctx, hipFree(ctx->bwBuf)); ctx->bwBuf = nullptr; ctx->bwBytes = 0; }
        hipError_t e = hipMalloc(&ctx->bwBuf, 2 * half + 64);
        if (e != hipSuccess) return fail(ctx, MOKA_ERR_ALLOC, std::string("bandwidth probe: hipMalloc: ") + hipGetErrorString(e));
        ctx->bwBytes = 2 * half;
        HIPCHK(ctx, hipMemsetAsync(ctx->bwBuf, 0x5A, 2 * half + 64, s));
    }
    unsigned char *a = static_cast<unsigned char *>(ctx->bwBuf), *b = a + half;
    uint32_t *sink = reinterpret_cast<uint32_t *>(a + 2 * half);
    double bestCopy = 0.0, bestRead = 0.0, sumCopy = 0.0, bestGather = 0.0;
    const uint32_t rowB = 480;
    for (int pass = 0; pass < 3; ++pass)
        for (int i = 0; i < iters; ++i) {
            HIPCHK(ctx, hipEventRecord(ctx->ev0, s));
            if (pass == 0) HIPCHK(ctx, launch_bw_copy(b, a, (int64_t)half, ctx->nCUs, s));
            else if (pass == 1) HIPCHK(ctx, launch_bw_read(a, (int64_t)(2 * half), sink, ctx->nCUs, s));
            else HIPCHK(ctx, launch_bw_gather(a, (int64_t)(2 * half), rowB, sink, ctx->nCUs, s));
            HIPCHK(ctx, hipEventRecord(ctx->ev1, s));
            HIPCHK(ctx, hipEventSynchronize(ctx->ev1));
            float ms = 0.f;
            HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
            const double r = (double)(2 * half) / ((double)ms * 1e-3) / 1e9;
            if (pass == 0) { bestCopy = std::max(bestCopy, r); sumCopy += r; }
            else if (pass == 1) bestRead = std::max(bestRead, r);
            else bestGather = std::max(bestGather, (double)((2 * half) / rowB * rowB) / ((double)ms * 1e-3) / 1e9);
        }
    gbs[0] = bestCopy; gbs[1] = bestRead; gbs[2] = sumCopy / iters; gbs[3] = bestGather;
    return MOKA_OK;
}

// A fifth figure for the same calibration: three streams read and two written at once (k_bw_streams) over the buffer moka_bw_probe
// allocated (call that first); GB/s of all five, best of `iters` launches.
int moka_bw_probe_streams(moka_ctx *ctx, int iters, double *gbs)
{
    if (!ctx || !gbs || iters < 1) return fail(ctx, MOKA_ERR_ARG, "NULL argument or iters < 1");
    if (!ctx->bwBuf || ctx->bwBytes < ((size_t)5 << 20)) return fail(ctx, MOKA_ERR_ARG, "moka_bw_probe first: it owns the buffer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int64_t n = (int64_t)(ctx->bwBytes / 5 / 16);
    double best = 0.0;
    for (int i = 0; i < iters; ++i) {
        HIPCHK(ctx, hipEventRecord(ctx->ev0, s));
        HIPCHK(ctx, launch_bw_streams(ctx->bwBuf, (int64_t)ctx->bwBytes, s));
        HIPCHK(ctx, hipEventRecord(ctx->ev1, s));
        HIPCHK(ctx, hipEventSynchronize(ctx->ev1));
        float ms = 0.f;
        HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        best = std::max(best, (double)(5 * 16 * n) / ((double)ms * 1e-3) / 1e9);
    }
    // the probes XOR the pattern away: restore it, the read probe's sentinel test relies on it
    HIPCHK(ctx, hipMemsetAsync(ctx->bwBuf, 0x5A, ctx->bwBytes + 64, s));
    *gbs = best;
    return MOKA_OK;
}

// A sixth figure: `region` bytes (more than the 32 MB of L2s, less than the 256 MB Infinity Cache: 128 MiB) read `reps` times back
// to back, GB/s over all passes, best of `iters` -- the rate at which re-read data comes back.  The stage kernels fetch a fifth
// to a quarter of their bytes a second time (rows of neighbouring patches, profiles/r03_traffic_attribution.txt); the streaming
// probes above never read anything twice.
int moka_bw_probe_reread(moka_ctx *ctx, int64_t region, int reps, int iters, double *gbs)
{
    if (!ctx || !gbs || iters < 1 || reps < 1) return fail(ctx, MOKA_ERR_ARG, "NULL argument or iters / reps < 1");
    if (!ctx->bwBuf || region < ((int64_t)1 << 20) || (size_t)region > ctx->bwBytes) return fail(ctx, MOKA_ERR_ARG, "moka_bw_probe first: it owns the buffer (region must fit it)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    unsigned char *a = static_cast<unsigned char *>(ctx->bwBuf);
    uint32_t *sink = reinterpret_cast<uint32_t *>(a + ctx->bwBytes);
    region &= ~(int64_t)4095;
    double best = 0.0;
    HIPCHK(ctx, launch_bw_read(a, region, sink, ctx->nCUs, s));          // first touch: from HBM
    for (int i = 0; i < iters; ++i) {
        HIPCHK(ctx, hipEventRecord(ctx->ev0, s));
        for (int r = 0; r < reps; ++r) HIPCHK(ctx, launch_bw_read(a, region, sink, ctx->nCUs, s));
        HIPCHK(ctx, hipEventRecord(ctx->ev1, s));
        HIPCHK(ctx, hipEventSynchronize(ctx->ev1));
        float ms = 0.f;
        HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        best = std::max(best, (double)region * reps / ((double)ms * 1e-3) / 1e9);
    }
    *gbs = best;
    return MOKA_OK;
}

// A seventh: the scattered row gather over a LARGE footprint of its own (`bytes`, e.g. 32 GiB: what a state with all its arrays
// spans), a quarter of the rows fetched once each -- consecutive half-waves land ~19 MB apart, so nearly every fetch needs an
// address translation the TLBs do not hold.  The 4 GiB gather of moka_bw_probe fits them.
int moka_bw_probe_gather_big(moka_ctx *ctx, int64_t bytes, int iters, double *gbs)
{
    if (!ctx || !gbs || iters < 1 || bytes < ((int64_t)1 << 24)) return fail(ctx, MOKA_ERR_ARG, "NULL argument, iters < 1 or less than 16 MiB");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    void *buf = nullptr;
    hipError_t e = hipMalloc(&buf, (size_t)bytes + 64);
    if (e != hipSuccess) return fail(ctx, MOKA_ERR_ALLOC, std::string("big gather probe: hipMalloc: ") + hipGetErrorString(e));
    const uint32_t rowB = 480;
    const int64_t nRows = bytes / rowB, nFetch = nRows / 4;
    uint32_t *sink = reinterpret_cast<uint32_t *>(static_cast<unsigned char *>(buf) + bytes);
    double best = 0.0;
    hipError_t rc = hipMemsetAsync(buf, 0x5A, (size_t)bytes + 64, s);
    for (int i = 0; i < iters && rc == hipSuccess; ++i) {
        if ((rc = hipEventRecord(ctx->ev0, s)) != hipSuccess) break;
        if ((rc = launch_bw_gather_n(buf, nRows, rowB, nFetch, sink, ctx->nCUs, s)) != hipSuccess) break;
        if ((rc = hipEventRecord(ctx->ev1, s)) != hipSuccess) break;
        if ((rc = hipEventSynchronize(ctx->ev1)) != hipSuccess) break;
        float ms = 0.f;
        if ((rc = hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1)) != hipSuccess) break;
        best = std::max(best, (double)nFetch * rowB / ((double)ms * 1e-3) / 1e9);
    }
    (void)hipStreamSynchronize(s);
    (void)hipFree(buf);
    HIPCHK(ctx, rc);
    *gbs = best;
    return MOKA_OK;
}

int moka_set_tuning(int key, int value)
{
    if (key < 1 || key >= N_TUNING || !g_tuning[key].exists()) return fail(nullptr, MOKA_ERR_ARG, "unknown tuning key");
    if (!g_tuning[key].accepts(value)) return fail(nullptr, MOKA_ERR_ARG, "tuning key " + std::to_string(key) + ": value names no kernel instance");
    g_tuning[key].value.store(value);
    return MOKA_OK;
}

int moka_get_tuning(int key, int *value)
{
    if (!value) return fail(nullptr, MOKA_ERR_ARG, "value is NULL");
    if (key < 1 || key >= N_TUNING || !g_tuning[key].exists()) return fail(nullptr, MOKA_ERR_ARG, "unknown tuning key");
    *value = g_tuning[key].value.load();
    return MOKA_OK;
}

int moka_kernel_variant_available(int variant)
{
    return variant == 0 || variant == 3 || variant == 4 || variant == 11;
}

int moka_set_kernel_variant(moka_ctx *ctx, int variant)
{
    if (!ctx) return fail(nullptr, MOKA_ERR_ARG, "ctx is NULL");
    if (variant < 0 || variant > 14) return fail(ctx, MOKA_ERR_ARG, "variant must be 0..14");
    if (!moka_kernel_variant_available(variant))
        return fail(ctx, MOKA_ERR_UNSUPPORTED, "this kernel variant was an experiment of rounds 1-3 and no longer exists (0, 3, 4, 11 do)");
    ctx->variant = variant;
    return MOKA_OK;
}

// ---------------------------------------------------------------------------------------------
// mesh
// ---------------------------------------------------------------------------------------------
int moka_mesh_create(moka_ctx *ctx, const moka_mesh_desc *desc, moka_mesh **out)
{
    if (!ctx || !out) return fail(ctx, MOKA_ERR_ARG, "NULL argument");
    *out = nullptr;
    moka_mesh *m = new (std::nothrow) moka_mesh();
    if (!m) return fail(ctx, MOKA_ERR_ALLOC, "out of host memory");
    m->ctx = ctx;
    m->mem.ctx = ctx;
    int rc;
    try {
        rc = build_plan(desc, m->plan);
    } catch (const std::bad_alloc &) {
        rc = fail(ctx, MOKA_ERR_ALLOC, "out of host memory while building the mesh plan");
    }
    if (rc != MOKA_OK) {
        ctx->err = moka::get_error();
        delete m;
        return rc;
    }
    const Plan &p = m->plan;
    if (p.ME > 8 || p.ME2 > 14) {
        delete m;
        return fail(ctx, MOKA_ERR_UNSUPPORTED, "cells with more than 8 edges are not supported by the gfx950 kernels");
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    MeshDev &d = m->dev;
    d.nC = p.nC; d.nE = p.nE; d.nV = p.nV; d.K = p.K; d.ME = p.ME; d.ME2 = p.ME2; d.VD = p.VD; d.nPatches = p.nPatches;
    d.tailPatch = -1;      // no extra patch rides in a launch of this view (0, the zero-initialised value, would name patch 0: a
                           // whole-mesh Forward-Euler launch then ran patch 0 twice -- harmless while every result was a pure
                           // function of the inputs, wrong once relativeVorticity accumulates in the same launch)
    m->lpc = lanes_per_column(p.K);
#define UP(field)                                                \
    if ((rc = m->mem.upload(p.field, &d.field)) != MOKA_OK) {   \
        moka_mesh_destroy(m);                                    \
        return rc;                                               \
    }
    UP(patchCellStart) UP(patchEdgeStart) UP(patchVertStart)
    UP(eoc) UP(coc) UP(mltc) UP(sdv) UP(invArea) UP(areaCell) UP(rsum)
    UP(ehdr) UP(eoe) UP(woe) UP(gInvDc) UP(dcEdge) UP(dvEdge) UP(fEdge)
    UP(eov) UP(cv) UP(cellN2O) UP(edgeN2O) UP(vertN2O)
    UP(leoe) UP(cRec) UP(eRec) UP(feoe) UP(vRec) UP(rowStart) UP(rowEdge)
    if (p.nlOk) { UP(voe) UP(cov) UP(kite) UP(invAreaTri) UP(fVertex) UP(keCoef) UP(invDc) UP(keoc) UP(rowVoe) }
    if (p.nl5Ok) { UP(pvStart) UP(pvList) UP(lvoe) }
#undef UP
    d.maxPV = p.nl5Ok ? p.maxPV : 0;
    if (!p.nl5Ok) { d.pvStart = nullptr; d.pvList = nullptr; d.lvoe = nullptr; }
    d.CI = p.CI; d.EI = p.EI;
    m->colOk = p.colOk;

    d.maxRows = p.maxRows; d.maxOwnE = p.maxOwnE; d.maxOwnC = p.maxOwnC;
    d.maxOwnV = p.maxOwnV;
    if (p.vRec.empty()) d.vRec = nullptr;       // (upload hands out a dummy allocation for an empty vector)
    *out = m;
    return MOKA_OK;
}

void moka_mesh_destroy(moka_mesh *mesh)
{
    if (!mesh) return;
    (void)hipSetDevice(mesh->ctx->device);
    (void)hipStreamSynchronize(mesh->ctx->stream);
    mesh->mem.release_all();
    for (auto b : mesh->opBuf)
        if (b) (void)hipFree(b);
    delete mesh;
}

int moka_mesh_permutation(const moka_mesh *mesh, int kind, int32_t *new_to_old)
{
    if (!mesh || !new_to_old) return fail(nullptr, MOKA_ERR_ARG, "NULL argument");
    const Plan &p = mesh->plan;
    const std::vector<int32_t> *v = kind == MOKA_CELL ? &p.cellN2O : kind == MOKA_EDGE ? &p.edgeN2O : kind == MOKA_VERTEX ? &p.vertN2O : nullptr;
    if (!v) return fail(mesh->ctx, MOKA_ERR_ARG, "kind must be MOKA_CELL, MOKA_EDGE or MOKA_VERTEX");
    std::copy(v->begin(), v->end(), new_to_old);
    return MOKA_OK;
}

int moka_mesh_class_ranges(const moka_mesh *mesh, int32_t capacity, int32_t *nClasses, int32_t *patchStart, int32_t *cellStart,
                           int32_t *edgeStart)
{
    if (!mesh || !nClasses) return fail(nullptr, MOKA_ERR_ARG, "NULL argument");
    const Plan &p = mesh->plan;
    const int n = (int)p.classPatchStart.size() - 1;
    *nClasses = n;
    for (int k = 0; k <= n && k < capacity; ++k) {
        if (patchStart) patchStart[k] = p.classPatchStart[k];
        if (cellStart) cellStart[k] = p.classCellStart[k];
        if (edgeStart) edgeStart[k] = p.classEdgeStart[k];
    }
    return MOKA_OK;
}

int moka_mesh_info_get(const moka_mesh *mesh, moka_mesh_info *info)
{
    if (!mesh || !info) return fail(nullptr, MOKA_ERR_ARG, "NULL argument");
    fill_mesh_info(mesh->plan, info);
    return MOKA_OK;
}

// ---------------------------------------------------------------------------------------------
// operators on host arrays
// ---------------------------------------------------------------------------------------------
static int run_operator(moka_mesh *m, int op, int nlev, const double *in, int inKind, double *out, int outKind,
                        bool out_is_inout)
{
    if (!m || !in || !out) return fail(m ? m->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    const Plan &p = m->plan;
    auto count = [&](int kind) -> int64_t { return kind == MOKA_CELL ? p.nC : kind == MOKA_EDGE ? p.nE : p.nV; };
    int rc = ensure_op_bufs(m);
    if (rc) return rc;
    hipStream_t s = m->ctx->stream;
    HIPCHK(m->ctx, hipSetDevice(m->ctx->device));
    if ((rc = put_rows(m, m->opBuf[0], in, inKind, count(inKind), p.K))) return rc;
    if (out_is_inout) {
        if ((rc = put_rows(m, m->opBuf[1], out, outKind, count(outKind), p.K))) return rc;
    } else {
        // untouched levels (interpolate, nlev < K) must come back as the caller had them
        if (op == OP_INTERP && nlev < p.K) {
            if ((rc = put_rows(m, m->opBuf[1], out, outKind, count(outKind), p.K))) return rc;
        }
    }
    OpArgs a{op, nlev, m->opBuf[0], m->opBuf[1]};
    HIPCHK(m->ctx, launch_operator(m->dev, a, m->lpc, s));
    return get_rows(m, out, m->opBuf[1], outKind, count(outKind), p.K);
}

int moka_gradient_on_edge(moka_mesh *mesh, const double *scalarCell, double *gradEdge)
{
    return run_operator(mesh, OP_GRADIENT, 0, scalarCell, MOKA_CELL, gradEdge, MOKA_EDGE, false);
}

int moka_interpolate_cell2edge(moka_mesh *mesh, const double *cellValue, double *edgeValue, int nlev)
{
    if (mesh && (nlev < 1 || nlev > mesh->plan.K)) return fail(mesh->ctx, MOKA_ERR_ARG, "nlev out of range");
    return run_operator(mesh, OP_INTERP, nlev, cellValue, MOKA_CELL, edgeValue, MOKA_EDGE, false);
}

int moka_curl_on_vertex(moka_mesh *mesh, const double *vecEdge, double *curlVertex)
{
    return run_operator(mesh, OP_CURL, 0, vecEdge, MOKA_EDGE, curlVertex, MOKA_VERTEX, true);
}

// ---------------------------------------------------------------------------------------------
// reverse and forward mode of the stand-alone operators (test/enzyme/test_Enzyme_Operators.jl:42-131, 137-225).
// The operators are linear: forward mode is the operator applied to the tangent, reverse mode its transpose applied to the
// cotangent.  Shadow conventions are Enzyme's for in-place kernels with Duplicated arguments: the shadow of an input is
// accumulated into, the shadow of an output the kernel overwrites is zero afterwards, the shadow of the (accumulated-into)
// curl output stays.  Transposes are gathers with a fixed order (oracle twins: oracle_*_vjp).
// ---------------------------------------------------------------------------------------------
static int ensure_op_transposes(moka_mesh *m)
{
    if (m->opESign) return MOKA_OK;
    const Plan &p = m->plan;
    std::vector<std::vector<std::pair<std::pair<int32_t, int32_t>, int32_t>>> lists(p.nE);     // ((caller's vertex, slot), new vertex)
    for (int v = 0; v < p.nV; ++v)
        for (int j = 0; j < p.VD; ++j) {
            const int e = p.eov[(size_t)v * p.VD + j];
            if (e >= 0) lists[e].push_back({{p.vertN2O[v], j}, v});
        }
    int W = 1;
    for (auto &l : lists) { std::sort(l.begin(), l.end()); W = std::max(W, (int)l.size()); }
    std::vector<int32_t> tv((size_t)p.nE * W, -1);
    std::vector<double> tc((size_t)p.nE * W, 0.0), es((size_t)p.nE * 2, 0.0);
    for (int e = 0; e < p.nE; ++e) {
        for (size_t q = 0; q < lists[e].size(); ++q) {
            const int v = lists[e][q].second, j = lists[e][q].first.second;
            tv[(size_t)e * W + q] = v;
            tc[(size_t)e * W + q] = p.cv[(size_t)v * p.VD + j];
        }
        for (int q = 0; q < 2; ++q) {
            const int c = p.ehdr[(size_t)e * 4 + q];
            for (int i = 0; i < p.ME; ++i)
                if (p.eoc[(size_t)c * p.ME + i] == e) { es[(size_t)e * 2 + q] = p.sdv[(size_t)c * p.ME + i] < 0.0 ? -1.0 : 1.0; break; }
        }
    }
    int rc;
    if ((rc = m->mem.upload(tv, &m->opTVert)) || (rc = m->mem.upload(tc, &m->opTCoef))) return rc;
    if ((rc = m->mem.upload(es, &m->opESign))) return rc;
    m->opTW = W;
    return MOKA_OK;
}

int moka_gradient_on_edge_vjp(moka_mesh *m, double *dGradEdge, double *dScalarCell)
{
    if (!m || !dGradEdge || !dScalarCell) return fail(m ? m->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    const Plan &p = m->plan;
    int rc = ensure_op_bufs(m);
    if (rc) return rc;
    HIPCHK(m->ctx, hipSetDevice(m->ctx->device));
    if ((rc = put_rows(m, m->opBuf[0], dGradEdge, MOKA_EDGE, p.nE, p.K))) return rc;
    if ((rc = put_rows(m, m->opBuf[1], dScalarCell, MOKA_CELL, p.nC, p.K))) return rc;
    OpArgs a{OP_GRAD_T, 0, m->opBuf[0], m->opBuf[1]};
    HIPCHK(m->ctx, launch_operator(m->dev, a, m->lpc, m->ctx->stream));
    if ((rc = get_rows(m, dScalarCell, m->opBuf[1], MOKA_CELL, p.nC, p.K))) return rc;
    std::memset(dGradEdge, 0, sizeof(double) * (size_t)p.K * p.nE);       // the overwritten output's shadow
    return MOKA_OK;
}

int moka_gradient_on_edge_jvp(moka_mesh *m, const double *dScalarCell, double *dGradEdge)
{
    return moka_gradient_on_edge(m, dScalarCell, dGradEdge);              // linear: the tangent map is the operator
}

int moka_divergence_on_cell_vjp(moka_mesh *m, double *dDivCell, double *dVecEdge, double *dTempEdge)
{
    if (!m || !dDivCell || !dVecEdge) return fail(m ? m->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    const Plan &p = m->plan;
    int rc = ensure_op_bufs(m);
    if (rc) return rc;
    HIPCHK(m->ctx, hipSetDevice(m->ctx->device));
    if ((rc = ensure_op_transposes(m))) return rc;
    if ((rc = put_rows(m, m->opBuf[0], dDivCell, MOKA_CELL, p.nC, p.K))) return rc;
    if ((rc = put_rows(m, m->opBuf[1], dVecEdge, MOKA_EDGE, p.nE, p.K))) return rc;
    if (dTempEdge && (rc = put_rows(m, m->opBuf[3], dTempEdge, MOKA_EDGE, p.nE, p.K))) return rc;
    OpArgs a{OP_DIV_T, 0, m->opBuf[0], m->opBuf[1]};
    a.in2 = dTempEdge ? m->opBuf[3] : nullptr;
    a.auxD = m->opESign;
    HIPCHK(m->ctx, launch_operator(m->dev, a, m->lpc, m->ctx->stream));
    if ((rc = get_rows(m, dVecEdge, m->opBuf[1], MOKA_EDGE, p.nE, p.K))) return rc;
    std::memset(dDivCell, 0, sizeof(double) * (size_t)p.K * p.nC);
    if (dTempEdge) std::memset(dTempEdge, 0, sizeof(double) * (size_t)p.K * p.nE);
    return MOKA_OK;
}

int moka_divergence_on_cell_jvp(moka_mesh *m, const double *dVecEdge, double *dTempEdge, double *dDivCell)
{
    return moka_divergence_on_cell(m, dVecEdge, dTempEdge, dDivCell);
}

int moka_curl_on_vertex_vjp(moka_mesh *m, const double *dCurlVertex, double *dVecEdge)
{
    if (!m || !dCurlVertex || !dVecEdge) return fail(m ? m->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    const Plan &p = m->plan;
    int rc = ensure_op_bufs(m);
    if (rc) return rc;
    HIPCHK(m->ctx, hipSetDevice(m->ctx->device));
    if ((rc = ensure_op_transposes(m))) return rc;
    if ((rc = put_rows(m, m->opBuf[0], dCurlVertex, MOKA_VERTEX, p.nV, p.K))) return rc;
    if ((rc = put_rows(m, m->opBuf[1], dVecEdge, MOKA_EDGE, p.nE, p.K))) return rc;
    OpArgs a{OP_CURL_T, 0, m->opBuf[0], m->opBuf[1]};
    a.auxI = m->opTVert; a.auxD = m->opTCoef; a.auxW = m->opTW;
    HIPCHK(m->ctx, launch_operator(m->dev, a, m->lpc, m->ctx->stream));
    return get_rows(m, dVecEdge, m->opBuf[1], MOKA_EDGE, p.nE, p.K);       // the curl shadow stays: the primal accumulates
}

int moka_curl_on_vertex_jvp(moka_mesh *m, const double *dVecEdge, double *dCurlVertex)
{
    return moka_curl_on_vertex(m, dVecEdge, dCurlVertex);                 // accumulates, like the primal
}

int moka_divergence_on_cell(moka_mesh *m, const double *vecEdge, double *tempEdge, double *divCell)
{
    if (!m || !vecEdge || !divCell) return fail(m ? m->ctx : nullptr, MOKA_ERR_ARG, "NULL argument");
    const Plan &p = m->plan;
    int rc = ensure_op_bufs(m);
    if (rc) return rc;
    hipStream_t s = m->ctx->stream;
    HIPCHK(m->ctx, hipSetDevice(m->ctx->device));
    if ((rc = put_rows(m, m->opBuf[0], vecEdge, MOKA_EDGE, p.nE, p.K))) return rc;
    OpArgs a1{OP_DIV_P1, 0, m->opBuf[0], m->opBuf[1]};      // temp = V*dvEdge (Operators.jl:60)
    HIPCHK(m->ctx, launch_operator(m->dev, a1, m->lpc, s));
    if (tempEdge && (rc = get_rows(m, tempEdge, m->opBuf[1], MOKA_EDGE, p.nE, p.K))) return rc;
    OpArgs a2{OP_DIV_P2, 0, m->opBuf[0], m->opBuf[1]};      // second pass reads V, folds dvEdge*sign exactly
    HIPCHK(m->ctx, launch_operator(m->dev, a2, m->lpc, s));
    return get_rows(m, divCell, m->opBuf[1], MOKA_CELL, p.nC, p.K);
}

}  // extern "C"
