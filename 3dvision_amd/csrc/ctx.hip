// Context, workspace arena, timers and the host helpers that are part of the path's semantics
// (RANSAC index stream, sqrt-free thresholds, pose composition).
#include "tdv_internal.hpp"
#include <cmath>
#include <cfloat>
#include <algorithm>
#include <cstring>
#include <vector>

namespace tdv {

int ws_reset(tdv_ctx* ctx) {
    // coalesce: if the previous call needed more than one block, replace them by one block
    if (ctx->blocks.size() > 1) {
        size_t total = 0;
        TDV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (auto& b : ctx->blocks) { total += b.cap; (void)hipFree(b.p); }
        ctx->blocks.clear();
        total = align_up(total + total / 4, (size_t)1 << 20);
        char* p = nullptr;
        TDV_HIP(ctx, hipMalloc((void**)&p, total));
        ctx->blocks.push_back({p, total});
    }
    ctx->cur_block = 0; ctx->cur_off = 0; ctx->used_total = 0;
    return TDV_OK;
}

int ws_alloc_bytes(tdv_ctx* ctx, size_t bytes, void** out) {
    bytes = align_up(bytes ? bytes : 1, 256);
    while (ctx->cur_block < ctx->blocks.size()) {
        auto& b = ctx->blocks[ctx->cur_block];
        if (ctx->cur_off + bytes <= b.cap) {
            *out = b.p + ctx->cur_off;
            ctx->cur_off += bytes; ctx->used_total += bytes;
            return TDV_OK;
        }
        ctx->cur_block++; ctx->cur_off = 0;
    }
    size_t cap = std::max(bytes, (size_t)64 << 20);
    if (!ctx->blocks.empty()) cap = std::max(cap, ctx->blocks.back().cap);
    char* p = nullptr;
    TDV_HIP(ctx, hipMalloc((void**)&p, cap));
    ctx->blocks.push_back({p, cap});
    ctx->cur_block = ctx->blocks.size() - 1;
    ctx->cur_off = bytes; ctx->used_total += bytes;
    *out = p;
    return TDV_OK;
}

int pin_reserve(tdv_ctx* ctx, size_t bytes) {
    if (bytes <= ctx->pin_cap) return TDV_OK;
    if (ctx->pin) { TDV_HIP(ctx, hipStreamSynchronize(ctx->stream)); (void)hipHostFree(ctx->pin); ctx->pin = nullptr; ctx->pin_cap = 0; }
    size_t cap = align_up(bytes, (size_t)1 << 16);
    // coherent (fine-grained), stated and not left to the environment's default: the host reads a RANSAC batch's record, and waits for
    // its sequence word, while the stream that wrote them is still running (ransac.hip: wait_batch)
    TDV_HIP(ctx, hipHostMalloc((void**)&ctx->pin, cap, hipHostMallocCoherent));
    ctx->pin_cap = cap;
    return TDV_OK;
}

// ---- the frame of a public call (entry.hpp)
int call_enter(tdv_ctx* ctx) {
    if (!ctx) return TDV_ERR_BAD_ARG;
    TDV_HIP(ctx, hipSetDevice(ctx->device));
    ctx->err[0] = 0;
    return TDV_OK;
}

int call_begin(tdv_ctx* ctx) {
    TDV_TRY(call_enter(ctx));
    return ws_reset(ctx);
}

int download_rows(tdv_ctx* ctx, size_t m, std::initializer_list<RowCopy> rows) {
    bool any = false;
    for (const RowCopy& r : rows) {
        if (m == 0 || !r.host || !r.dev) continue;
        TDV_HIP(ctx, hipMemcpyAsync(r.host, r.dev, m * r.row_bytes, hipMemcpyDeviceToHost, ctx->stream));
        any = true;
    }
    return any ? finish(ctx) : TDV_OK;
}

static hipEvent_t get_event(tdv_ctx* ctx) {
    if (!ctx->event_pool.empty()) { hipEvent_t e = ctx->event_pool.back(); ctx->event_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

hipEvent_t event_acquire(tdv_ctx* ctx) { return get_event(ctx); }
void event_release(tdv_ctx* ctx, hipEvent_t e) { if (e) ctx->event_pool.push_back(e); }

ScopedTimer::ScopedTimer(tdv_ctx* c, int s) : ctx(c), slot(s) {
    if (!ctx->timing || slot < 0) return;     // slot < 0: nothing to time here
    a = get_event(ctx); b = get_event(ctx);
    if (a) (void)hipEventRecord(a, ctx->stream);
}
ScopedTimer::~ScopedTimer() {
    if (!ctx->timing || slot < 0 || !a || !b) return;
    (void)hipEventRecord(b, ctx->stream);
    ctx->timers[slot].pending.emplace_back(a, b);
}

// ---- mt19937 + libstdc++-11 uniform_int_distribution<size_t> (Lemire's nearly-divisionless
// method on 32-bit draws when the range fits in 32 bits; for larger ranges libstdc++ composes
// two draws — clouds never reach 2^32 points, so that branch is rejected up front).
// Bulk form (round 6): the state is twisted a whole block of 624 words at a time - the twist split into its three index ranges,
// no modulo - and the block tempered at once; both loops vectorise.  Lemire's rejection loop is a per-word predicate: a word r is
// accepted iff (uint32)(r * range) >= (2^32 - range) mod range, and an accepted word gives the index (r * range) >> 32.  A draw
// of m indices therefore maps m words at a time (every word gives at most one index, so m words never overshoot), with a
// vectorised pass when none of them is rejected (about 8 words of a 65,536-hypothesis batch at 200k points are) and a
// branch-free compaction otherwise, until m indices have been produced: the same indices, from the same words, as the loop of
// std::uniform_int_distribution, and the stream continues exactly where that loop would.
namespace {
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
#define TDV_HOST_VECTOR __attribute__((target_clones("avx2", "default")))   // the two bulk loops below: 8 lanes where the host has them
#else
#define TDV_HOST_VECTOR
#endif
constexpr int MT_N = 624, MT_M = 397;
inline uint32_t mt_mix(uint32_t a, uint32_t b, uint32_t c) {   // mt[i] from mt[i] (a), mt[i + 1] (b) and mt[i + 397] (c)
    const uint32_t y = (a & 0x80000000u) | (b & 0x7fffffffu);
    return c ^ (y >> 1) ^ ((0u - (y & 1u)) & 0x9908b0dfu);
}
// the twist of a whole block, then its tempering into out[]
// (the sequential twist updates mt[i] in place in order i = 0..623; mt[i + 397] is still the old word for i < 227
// and already the new one from then on (index i - 227), mt[i + 1] is old except for i = 623 (mt[0], new))
TDV_HOST_VECTOR void mt_block(uint32_t* __restrict__ mt, uint32_t* __restrict__ out) {
    for (int i = 0; i < MT_N - MT_M; ++i) mt[i] = mt_mix(mt[i], mt[i + 1], mt[i + MT_M]);
    for (int i = MT_N - MT_M; i < MT_N - 1; ++i) mt[i] = mt_mix(mt[i], mt[i + 1], mt[i + MT_M - MT_N]);
    mt[MT_N - 1] = mt_mix(mt[MT_N - 1], mt[0], mt[MT_M - 1]);
    for (int i = 0; i < MT_N; ++i) {
        uint32_t y = mt[i];
        y ^= y >> 11; y ^= (y << 7) & 0x9d2c5680u; y ^= (y << 15) & 0xefc60000u; y ^= y >> 18;
        out[i] = y;
    }
}
// Lemire's index of every word (r * range) >> 32 into d; returns whether any word is rejected ((uint32)(r * range) < thr)
TDV_HOST_VECTOR uint32_t lemire_map(const uint32_t* __restrict__ w, int k, uint32_t range, uint32_t thr, uint32_t* __restrict__ d) {
    uint32_t rejected = 0;
    for (int i = 0; i < k; ++i) {
        const uint64_t p = (uint64_t)w[i] * range;
        d[i] = (uint32_t)(p >> 32);
        rejected |= (uint32_t)((uint32_t)p < thr);
    }
    return rejected;
}
struct Mt19937 {
    uint32_t mt[MT_N], out[MT_N]; int idx;
    explicit Mt19937(uint32_t seed) {
        mt[0] = seed;
        for (int i = 1; i < MT_N; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
        idx = MT_N;
    }
    void refill() { mt_block(mt, out); idx = 0; }   // the next 624 outputs into out[]
    uint32_t next() {
        if (idx >= MT_N) refill();
        return out[idx++];
    }
    // m uniform indices in [0, range) (range 0: 2^32, the raw words) into dst, in stream order
    void draw(uint32_t range, size_t m, uint32_t* dst) {
        const uint32_t thr = range ? (0u - range) % range : 0u;
        size_t got = 0;
        while (got < m) {
            if (idx >= MT_N) refill();
            const int k = (int)std::min((size_t)(MT_N - idx), m - got);
            const uint32_t* w = out + idx;
            uint32_t* d = dst + got;
            idx += k;
            if (!range) { std::memcpy(d, w, (size_t)k * 4); got += k; continue; }
            if (!lemire_map(w, k, range, thr, d)) { got += k; continue; }
            int j = 0;
            for (int i = 0; i < k; ++i) {
                const uint64_t p = (uint64_t)w[i] * range;
                d[j] = (uint32_t)(p >> 32);          // (j <= i < k: inside what this round may write)
                j += (uint32_t)p >= thr;
            }
            got += j;
        }
    }
};
}  // namespace

static void mt19937_lemire_triples(uint32_t seed, uint64_t n, int count, uint64_t* out) {
    Mt19937 g(seed);
    const uint32_t range = (uint32_t)n;      // n = 2^32 -> 0: the raw words
    uint32_t buf[3 * 1024];
    for (int i0 = 0; i0 < count; i0 += 1024) {
        const int c = std::min(1024, count - i0);
        g.draw(range, 3 * (size_t)c, buf);
        for (int k = 0; k < 3 * c; ++k) out[3 * (size_t)i0 + k] = buf[k];
    }
}

// the raw 32-bit outputs of mt19937(seed), for the device-side index sampler of the batched RANSAC (ransac.hip)
void mt19937_raw(uint32_t seed, size_t count, uint32_t* out) {
    Mt19937 g(seed);
    g.draw(0u, count, out);
}

struct TripleStream::Impl { Mt19937 g; std::vector<uint32_t> buf; explicit Impl(uint32_t seed) : g(seed) {} };
TripleStream::TripleStream(uint32_t seed, uint64_t n) : impl_(new Impl(seed)), n_(n) {}
TripleStream::~TripleStream() { delete impl_; }
void TripleStream::next(uint64_t* out3) {
    uint32_t d[3];
    impl_->g.draw((uint32_t)n_, 3, d);       // n = 2^32 -> range 0: one raw draw each
    for (int k = 0; k < 3; ++k) out3[k] = d[k];
}
void TripleStream::next_batch(int count, int* out4) {
    auto& b = impl_->buf;
    if (b.size() < 3 * (size_t)count) b.resize(3 * (size_t)count);
    impl_->g.draw((uint32_t)n_, 3 * (size_t)count, b.data());
    for (int k = 0; k < count; ++k) {
        const int a = (int)b[3 * k], c = (int)b[3 * k + 1], e = (int)b[3 * k + 2];
        out4[4 * k] = a; out4[4 * k + 1] = c; out4[4 * k + 2] = e;
        out4[4 * k + 3] = !(a == c || c == e || a == e);     // registration.cpp:240
    }
}
void TripleStream::next_batch_packed(int count, uint64_t* out) {
    auto& b = impl_->buf;
    if (b.size() < 3 * (size_t)count) b.resize(3 * (size_t)count);
    impl_->g.draw((uint32_t)n_, 3 * (size_t)count, b.data());
    for (int k = 0; k < count; ++k) out[k] = triple_pack(b[3 * k], b[3 * k + 1], b[3 * k + 2]);
}

float tau_le(float thr) {  // largest f with sqrtf(f) <= thr ; returns -1 if none (thr < 0 or NaN)
    if (!(thr >= 0.f)) return -1.f;
    if (std::isinf(thr)) return FLT_MAX;
    float c = thr * thr;
    if (std::isinf(c)) c = FLT_MAX;
    while (c > 0.f && std::sqrt(c) > thr) c = std::nextafterf(c, -1.f);
    while (c < FLT_MAX && std::sqrt(std::nextafterf(c, INFINITY)) <= thr) c = std::nextafterf(c, INFINITY);
    return c;
}
float tau_lt(float thr) {  // smallest f >= 0 with sqrtf(f) >= thr ; d2 < f <=> sqrtf(d2) < thr
    if (!(thr > 0.f)) return 0.f;  // nothing is < thr when thr <= 0 (d2 >= 0) ; NaN -> no inliers
    if (std::isinf(thr)) return INFINITY;
    float c = thr * thr;
    if (std::isinf(c)) c = FLT_MAX;
    while (c < FLT_MAX && std::sqrt(c) < thr) c = std::nextafterf(c, INFINITY);
    while (c > 0.f && std::sqrt(std::nextafterf(c, -1.f)) >= thr) c = std::nextafterf(c, -1.f);
    return c;
}

}  // namespace tdv

using namespace tdv;

extern "C" {

const char* tdv_version(void) { return "3dvision_amd 0.1 (gfx950)"; }

const char* tdv_status_string(int s) {
    switch (s) {
        case TDV_OK: return "ok";
        case TDV_ERR_NO_DEVICE: return "no HIP device";
        case TDV_ERR_BAD_ARG: return "bad argument";
        case TDV_ERR_OOM: return "out of memory";
        case TDV_ERR_LAUNCH: return "HIP launch/copy failure";
        default: return "internal error";
    }
}

int tdv_device_count(int* count) {
    if (!count) return TDV_ERR_BAD_ARG;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { (void)hipGetLastError(); n = 0; }
    *count = n;
    return TDV_OK;
}

int tdv_ctx_create(int device, tdv_ctx** out) {
    if (!out) return TDV_ERR_BAD_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { (void)hipGetLastError(); return TDV_ERR_NO_DEVICE; }
    if (device < 0 || device >= n) return TDV_ERR_BAD_ARG;
    if (hipSetDevice(device) != hipSuccess) return TDV_ERR_NO_DEVICE;
    tdv_ctx* c = new tdv_ctx();
    c->device = device;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return TDV_ERR_NO_DEVICE; }
    c->own_stream = true;
    // one persistent device word: the "last workgroup" ticket of the scans (reset by the kernel that uses it)
    // (cleared on the ctx's own stream and waited for: a null-stream memset is not ordered against a non-blocking stream)
    if (hipMalloc((void**)&c->scan_ticket, 64) != hipSuccess || hipMemsetAsync(c->scan_ticket, 0, 64, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
        (void)hipStreamDestroy(c->stream); delete c; return TDV_ERR_OOM;
    }
    if (const char* e = getenv("TDV_ICP_SEARCH")) {
        if (!strcmp(e, "brute")) c->icp_search = TDV_ICP_SEARCH_BRUTE;
        else if (!strcmp(e, "pruned")) c->icp_search = TDV_ICP_SEARCH_PRUNED;
        else if (!strcmp(e, "grid")) c->icp_search = TDV_ICP_SEARCH_GRID;
    }
    if (const char* e = getenv("TDV_ICP_ACCUMULATE")) {
        if (!strcmp(e, "reference")) c->icp_accumulate = TDV_ICP_ACCUMULATE_REFERENCE;
    }
    *out = c;
    return TDV_OK;
}

int tdv_ctx_set_icp_accumulation(tdv_ctx* ctx, int mode) {
    if (!ctx || (mode != TDV_ICP_ACCUMULATE_TREE && mode != TDV_ICP_ACCUMULATE_REFERENCE)) return TDV_ERR_BAD_ARG;
    ctx->icp_accumulate = mode;
    return TDV_OK;
}

int tdv_ctx_set_icp_launches(tdv_ctx* ctx, int mode) {
    if (!ctx || mode < TDV_ICP_LAUNCHES_AUTO || mode > TDV_ICP_LAUNCHES_ONE) return TDV_ERR_BAD_ARG;
    ctx->icp_launches = mode;
    return TDV_OK;
}
int tdv_ctx_last_icp_launches(tdv_ctx* ctx) { return ctx ? ctx->last_icp_launches : TDV_ERR_BAD_ARG; }

int tdv_ctx_set_icp_probe_cache(tdv_ctx* ctx, int mode) {
    if (!ctx || mode < TDV_ICP_PROBE_CACHE_AUTO || mode > TDV_ICP_PROBE_CACHE_ON) return TDV_ERR_BAD_ARG;
    ctx->icp_probe_cache = mode;
    return TDV_OK;
}
int tdv_ctx_last_icp_probe_misses(tdv_ctx* ctx) { return ctx ? ctx->last_icp_probe_misses : TDV_ERR_BAD_ARG; }

int tdv_ctx_set_icp_loss(tdv_ctx* ctx, int loss, float scale) {
    if (!ctx || loss < TDV_ICP_LOSS_L2 || loss > TDV_ICP_LOSS_CAUCHY) return TDV_ERR_BAD_ARG;
    if (loss != TDV_ICP_LOSS_L2 && !(std::isfinite(scale) && scale > 0.f)) return TDV_ERR_BAD_ARG;
    ctx->icp_loss = loss;
    ctx->icp_loss_scale = loss == TDV_ICP_LOSS_L2 ? 0.f : scale;
    return TDV_OK;
}

int tdv_ctx_get_icp_loss(tdv_ctx* ctx, int* loss, float* scale) {
    if (!ctx) return TDV_ERR_BAD_ARG;
    if (loss) *loss = ctx->icp_loss;
    if (scale) *scale = ctx->icp_loss_scale;
    return TDV_OK;
}

int tdv_ctx_set_icp_search(tdv_ctx* ctx, int mode) {
    if (!ctx || mode < TDV_ICP_SEARCH_AUTO || mode > TDV_ICP_SEARCH_GRID) return TDV_ERR_BAD_ARG;
    ctx->icp_search = mode;
    return TDV_OK;
}

int tdv_ctx_set_ransac_score(tdv_ctx* ctx, int mode) {
    if (!ctx || (mode != TDV_RANSAC_SCORE_FAST && mode != TDV_RANSAC_SCORE_EXACT && !(tdv::kStudyBuild && mode == TDV_RANSAC_SCORE_MATRIX))) return TDV_ERR_BAD_ARG;   // MATRIX: study build only
    ctx->ransac_score_mode = mode;
    return TDV_OK;
}

int tdv_ctx_set_ransac_leaf_order(tdv_ctx* ctx, int mode) {
    if (!ctx || mode < TDV_RANSAC_LEAVES_AUTO || mode > TDV_RANSAC_LEAVES_CLASSES) return TDV_ERR_BAD_ARG;
    ctx->ransac_leaf_order = mode;
    return TDV_OK;
}

int tdv_ctx_set_ransac_triples(tdv_ctx* ctx, int mode) {
    if (!ctx || mode < TDV_RANSAC_TRIPLES_AUTO || mode > TDV_RANSAC_TRIPLES_STAGED) return TDV_ERR_BAD_ARG;
    ctx->ransac_triples = mode;
    return TDV_OK;
}
int tdv_ctx_last_ransac_staged(tdv_ctx* ctx) { return ctx ? ctx->last_ransac_staged : 0; }

int tdv_ctx_set_fps_path(tdv_ctx* ctx, int mode) {
    if (!ctx || mode < TDV_FPS_AUTO || mode > TDV_FPS_GRID) return TDV_ERR_BAD_ARG;
    ctx->fps_path = mode;
    return TDV_OK;
}
int tdv_ctx_last_fps_path(tdv_ctx* ctx) { return ctx ? ctx->last_fps_path : 0; }

double tdv_ctx_last_ransac_rescore(tdv_ctx* ctx) { return ctx ? ctx->last_ransac_rescore : -1.0; }

double tdv_ctx_last_ransac_scored(tdv_ctx* ctx) { return ctx ? ctx->last_ransac_scored : 1.0; }
void tdv_ctx_last_ransac_bound(tdv_ctx* ctx, long long out[4]) { if (out) for (int e = 0; e < 4; ++e) out[e] = ctx ? ctx->last_ransac_bound[e] : 0; }

int tdv_ctx_last_icp_search(tdv_ctx* ctx) { return ctx ? ctx->last_icp_search : 0; }
int tdv_ctx_last_feature_match_path(tdv_ctx* ctx) { return ctx ? ctx->last_fm_path : 0; }
int tdv_ctx_last_voxel_grouping(tdv_ctx* ctx) { return ctx ? ctx->last_voxel_grouping : 0; }
int tdv_ctx_last_voxel_batch_redone(tdv_ctx* ctx) { return ctx ? ctx->last_voxel_batch_redone : TDV_ERR_BAD_ARG; }
int tdv_ctx_last_batch_lanes(tdv_ctx* ctx) { return ctx ? ctx->last_batch_lanes : 0; }
unsigned long long tdv_ctx_workspace_bytes(tdv_ctx* ctx) {
    unsigned long long total = 0;
    for (tdv_ctx* c = ctx; c; c = c->helper)
        for (auto& b : c->blocks) total += b.cap;
    return total;
}

// test aid (include/tdv_hip.h): arena blocks and pinned staging of the ctx and its lanes; scan_ticket and chain_status stay as they are
int tdv_ctx_workspace_fill(tdv_ctx* ctx, int byte) {
    if (!ctx || byte < 0 || byte > 255) return TDV_ERR_BAD_ARG;
    for (tdv_ctx* c = ctx; c; c = c->helper) {
        TDV_HIP(ctx, hipSetDevice(c->device));
        for (auto& b : c->blocks) TDV_HIP(ctx, hipMemsetAsync(b.p, byte, b.cap, c->stream));
        TDV_HIP(ctx, hipStreamSynchronize(c->stream));
        if (c->pin) memset(c->pin, byte, c->pin_cap);
    }
    return TDV_OK;
}

int tdv_ctx_set_stream(tdv_ctx* ctx, void* s) {
    if (!ctx) return TDV_ERR_BAD_ARG;
    if (ctx->own_stream && ctx->stream) { (void)hipStreamSynchronize(ctx->stream); (void)hipStreamDestroy(ctx->stream); }
    ctx->stream = (hipStream_t)s;
    ctx->own_stream = false;
    return TDV_OK;
}
void* tdv_ctx_get_stream(tdv_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int tdv_ctx_synchronize(tdv_ctx* ctx) {
    if (!ctx) return TDV_ERR_BAD_ARG;
    TDV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return TDV_OK;
}

void tdv_ctx_destroy(tdv_ctx* ctx) {
    if (!ctx) return;
    if (ctx->helper) { tdv_ctx_destroy(ctx->helper); ctx->helper = nullptr; }
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (auto& b : ctx->blocks) (void)hipFree(b.p);
    if (ctx->scan_ticket) (void)hipFree(ctx->scan_ticket);
    if (ctx->chain_status) (void)hipFree(ctx->chain_status);
    if (ctx->pin) (void)hipHostFree(ctx->pin);
    for (auto& t : ctx->timers) for (auto& p : t.pending) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    for (auto e : ctx->event_pool) (void)hipEventDestroy(e);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char* tdv_last_error(tdv_ctx* ctx) { return ctx ? ctx->err : ""; }

int tdv_timing_enable(tdv_ctx* ctx, int on) {
    if (!ctx) return TDV_ERR_BAD_ARG;
    ctx->timing = on != 0;
    return TDV_OK;
}

int tdv_timing_read(tdv_ctx* ctx, int slot, double* total_ms, int* launches) {
    if (!ctx || slot < 0 || slot >= TDV_TIMER_COUNT) return TDV_ERR_BAD_ARG;
    TDV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    auto& t = ctx->timers[slot];
    for (auto& p : t.pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) { t.total_ms += ms; t.launches++; }
        ctx->event_pool.push_back(p.first); ctx->event_pool.push_back(p.second);
    }
    t.pending.clear();
    if (ctx->helper) {   // the batched pipeline's second lane times its kernels on its own stream
        double hms = 0.0; int hl = 0;
        if (tdv_timing_read(ctx->helper, slot, &hms, &hl) == TDV_OK) { t.total_ms += hms; t.launches += hl; }
    }
    if (total_ms) *total_ms = t.total_ms;
    if (launches) *launches = t.launches;
    t.total_ms = 0.0; t.launches = 0;
    return TDV_OK;
}

int tdv_sample_triples(uint32_t seed, uint64_t n, int count, uint64_t* out) {
    if (!out || count < 0 || n == 0 || n > ((uint64_t)1 << 32)) return TDV_ERR_BAD_ARG;
    mt19937_lemire_triples(seed, n, count, out);
    return TDV_OK;
}

int tdv_sample_triples_batch(uint32_t seed, uint64_t n, int count, void* out, int* packed) {
    if (!out || !packed || count < 0 || n == 0 || n > ((uint64_t)1 << 31)) return TDV_ERR_BAD_ARG;
    TripleStream stream(seed, n);
    *packed = n <= kTriplePackMaxN;
    if (*packed) stream.next_batch_packed(count, static_cast<uint64_t*>(out));
    else stream.next_batch(count, static_cast<int*>(out));
    return TDV_OK;
}

// out = E * inverse(T), all column-major 4x4 (src/pipeline.cpp:136-137).  General inverse by
// the adjugate with double intermediates, rounded once to float.
int tdv_pose_compose(const float* E, const float* T, float* out) {
    if (!E || !T || !out) return TDV_ERR_BAD_ARG;
    double a[16], inv[16], cof[16];
    for (int i = 0; i < 16; ++i) a[i] = T[i];
    auto A = [&](int r, int c) { return a[c * 4 + r]; };
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            int rr[3], cc[3], k = 0;
            for (int i = 0; i < 4; ++i) if (i != r) rr[k++] = i;
            k = 0;
            for (int i = 0; i < 4; ++i) if (i != c) cc[k++] = i;
            double m = A(rr[0], cc[0]) * (A(rr[1], cc[1]) * A(rr[2], cc[2]) - A(rr[1], cc[2]) * A(rr[2], cc[1]))
                     - A(rr[0], cc[1]) * (A(rr[1], cc[0]) * A(rr[2], cc[2]) - A(rr[1], cc[2]) * A(rr[2], cc[0]))
                     + A(rr[0], cc[2]) * (A(rr[1], cc[0]) * A(rr[2], cc[1]) - A(rr[1], cc[1]) * A(rr[2], cc[0]));
            cof[c * 4 + r] = ((r + c) & 1) ? -m : m;
        }
    double det = 0;
    for (int c = 0; c < 4; ++c) det += A(0, c) * cof[c * 4 + 0];
    if (det == 0.0) return TDV_ERR_BAD_ARG;
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) inv[c * 4 + r] = cof[r * 4 + c] / det;
    float invf[16], res[16];
    for (int i = 0; i < 16; ++i) invf[i] = (float)inv[i];
    for (int j = 0; j < 4; ++j)
        for (int i = 0; i < 4; ++i) {
            float acc = E[0 * 4 + i] * invf[j * 4 + 0];
            for (int k = 1; k < 4; ++k) acc = E[k * 4 + i] * invf[j * 4 + k] + acc;
            res[j * 4 + i] = acc;
        }
    for (int i = 0; i < 16; ++i) out[i] = res[i];
    return TDV_OK;
}

}  // extern "C"
