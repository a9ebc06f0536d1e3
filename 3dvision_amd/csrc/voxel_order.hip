// The reference's voxel ORDER.  Registration::voxelDownsample groups with a std::unordered_map and emits the voxels in that container's
// iteration order (src/registration.cpp:38-58); voxel.hip groups in first-occurrence order, and TDV_VOXEL_ORDER_REFERENCE turns the
// one into the other here.  Only the first point of every voxel changes a container, so the order is a function of the LEADERS (cell +
// input index of each voxel's first point, in first-occurrence order), 16 B per voxel; the cloud stays in HBM.  Two ways to it:
//   the host replay     (voxel_reference_order)  the leaders go to the host, which replays the node-list manipulation of this libstdc++'s
//                       container on index arrays (LibstdcxxInsertionOrder; 22 ns per voxel + two copies) - or, with another
//                       standard library or TDV_VOXEL_REAL_MAP (study), inserts them into a real std::unordered_map;
//   the device periods  (voxel_reference_order_batch_dev)  the closed form of a rehash period, ~17 periods of small launches for all
//                       clouds of a batch at once; a cloud whose hash degenerates is finished by the host replay.
// voxel_finish_reference picks between them for one cloud (the measured cross-over is 10,000 voxels) and carries colours and normals
// through the permutation.
#include "voxel_rules.hpp"
#include <algorithm>
#include <chrono>
#include <mutex>
#include <unordered_map>

namespace tdv {

// out[p] = in[rank[order_first[p]]]
__global__ void k_voxel_permute(const float* __restrict__ in_xyz, const float* __restrict__ in_rgb, const int* __restrict__ rank, int rank_base,
                                const int* __restrict__ order_first, int v, float* __restrict__ out_xyz, float* __restrict__ out_rgb,
                                int* __restrict__ ref2first, int* __restrict__ first2ref, VoxelNormals nrm /* in: first-occurrence order; both NULL without normals */) {
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= v) return;
    int s = rank[order_first[p]] - rank_base;     // (rank_base: the cloud's first voxel when ranks count through several clouds)
    if (ref2first) { ref2first[p] = s; first2ref[s] = p; }
    copy_row3(out_xyz, (size_t)p, in_xyz, (size_t)s);
    copy_row3_opt(out_rgb, (size_t)p, in_rgb, (size_t)s);
    copy_row3_opt(nrm.out, (size_t)p, nrm.in, (size_t)s);
}

// out[p] = in[idx[p]] for rows of three floats
__global__ void k_gather_rows3(const float* __restrict__ in, const int* __restrict__ idx, int n, float* __restrict__ out) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    copy_row3(out, (size_t)p, in, (size_t)idx[p]);
}

namespace {
struct VoxelKey {
    int x, y, z;
    bool operator==(const VoxelKey& o) const { return x == o.x && y == o.y && z == o.z; }
};
struct VoxelKeyHash {  // the reference's combiner over THIS library's std::hash<int>: the real container's order is its library's by construction
    size_t operator()(const VoxelKey& k) const { return (size_t)voxel_key_combine(std::hash<int>()(k.x), std::hash<int>()(k.y), std::hash<int>()(k.z)); }
};
static_assert(sizeof(size_t) == 8, "the reference's hash is formed in a 64-bit size_t");

// The emulation below is tied to libstdc++'s <bits/hashtable.h> (it instantiates the library's own _Prime_rehash_policy):
// with any other standard library the real std::unordered_map is used instead (the TDV_VOXEL_REAL_MAP path), which is
// that library's order by construction.  tests/test_gpu_voxel.py holds the emulation against the real container, so a
// toolchain bump that changes the node-list manipulation is caught.
#ifdef __GLIBCXX__
#define TDV_HAVE_LIBSTDCXX_EMULATION 1
// Iteration order of a libstdc++ std::unordered_map (unique keys, std::__detail::_Mod_range_hashing, the library's own
// _Prime_rehash_policy object) after inserting DISTINCT keys in a given sequence — the same node-list manipulation as
// _Hashtable::_M_insert_unique_node / _M_insert_bucket_begin / _M_rehash_aux(unique) of <bits/hashtable.h>, on index
// arrays instead of heap nodes.  Only first occurrences change a container, so replaying the leaders (first point of
// every voxel, in input order) reproduces the reference's voxel order exactly, at a fraction of the cost of building
// the real map over all points; tests compare it with the real container.
class LibstdcxxInsertionOrder {
public:
    explicit LibstdcxxInsertionOrder(size_t expected) { next_.reserve(expected); code_.reserve(expected); buckets_.assign(1, EMPTY); }
    void insert(size_t code) {   // a key not inserted before
        const int node = (int)next_.size();
        next_.push_back(NONE); code_.push_back(code);
        const auto saved = policy_._M_state();
        const std::pair<bool, std::size_t> rh = policy_._M_need_rehash(buckets_.size(), (size_t)node, 1);
        if (rh.first) { try { rehash(rh.second); } catch (...) { policy_._M_reset(saved); throw; } }
        const size_t bkt = code % buckets_.size();
        if (buckets_[bkt] != EMPTY) {          // after the bucket's "before" node: the new node becomes the bucket's first
            int& after = link(buckets_[bkt]);
            next_[node] = after; after = node;
        } else {                               // at the very beginning of the list
            next_[node] = head_; head_ = node;
            if (next_[node] != NONE) buckets_[code_[next_[node]] % buckets_.size()] = node;
            buckets_[bkt] = BEFORE_BEGIN;
        }
    }
    template <class F> void for_each(F&& f) const { for (int p = head_; p != NONE; p = next_[p]) f(p); }   // p = insertion rank
private:
    static constexpr int NONE = -1, EMPTY = -1, BEFORE_BEGIN = -2;
    int& link(int before) { return before == BEFORE_BEGIN ? head_ : next_[before]; }
    void rehash(size_t n) {
        std::vector<int> nb(n, EMPTY);
        int p = head_; head_ = NONE;
        size_t bbegin_bkt = 0;
        while (p != NONE) {
            const int nxt = next_[p];
            const size_t bkt = code_[p] % n;
            if (nb[bkt] == EMPTY) {
                next_[p] = head_; head_ = p;
                nb[bkt] = BEFORE_BEGIN;
                if (next_[p] != NONE) nb[bbegin_bkt] = p;
                bbegin_bkt = bkt;
            } else {
                int& after = nb[bkt] == BEFORE_BEGIN ? head_ : next_[nb[bkt]];
                next_[p] = after; after = p;
            }
            p = nxt;
        }
        buckets_.swap(nb);
    }
    std::vector<int> next_; std::vector<size_t> code_; std::vector<int> buckets_;
    int head_ = NONE;
    std::__detail::_Prime_rehash_policy policy_;
};
#else
#define TDV_HAVE_LIBSTDCXX_EMULATION 0
#endif
}  // namespace

// The reference's container order for v voxels held in first-occurrence order (tmp_*): leaders (cell + input index of the first
// point of every voxel, at its first-occurrence rank) go to the host, which replays the container; d_rank[input index] =
// first-occurrence rank.  out[p] = tmp[rank[leader index of the p-th voxel of the container]].
int voxel_reference_order(tdv_ctx* ctx, int v, int n, const int4* d_leaders, const float* tmp_xyz, const float* tmp_rgb, const int* d_rank, int rank_base,
                          float* d_out_xyz, float* d_out_rgb, const VoxelBothOrders* both, VoxelNormals nrm /* in: the voxels' normals in first-occurrence order */) {
    hipStream_t s = ctx->stream;
    int* d_order;
    TDV_TRY(ws_alloc(ctx, (size_t)v, &d_order));
    // through pinned memory both ways (a pageable std::vector made these two copies staged ones: 2.3 MB + 0.6 MB per C4 instance)
    const size_t pin_order_off = align_up((size_t)v * sizeof(int4), 64);
    TDV_TRY(pin_reserve(ctx, pin_order_off + (size_t)v * 4));
    const int4* leaders = reinterpret_cast<const int4*>(ctx->pin);
    int* order_pinned = reinterpret_cast<int*>(ctx->pin + pin_order_off);
    TDV_HIP(ctx, hipMemcpyAsync(ctx->pin, d_leaders, (size_t)v * sizeof(int4), hipMemcpyDeviceToHost, s));
    TDV_HIP(ctx, hipStreamSynchronize(s));
    const bool real_map = !TDV_HAVE_LIBSTDCXX_EMULATION || voxel_knobs().real_map;
    const auto t_host0 = std::chrono::steady_clock::now();
    int n_first = 0;
    struct { int* p; int* n; void push_back(int x) { p[(*n)++] = x; } } order_first{order_pinned, &n_first};
    for (int r = 0; r < v; ++r)
        if (leaders[r].w < 0 || leaders[r].w >= n) { snprintf(ctx->err, sizeof(ctx->err), "voxel: bad leader index %d", leaders[r].w); return TDV_ERR_INTERNAL; }
    if (real_map) {
        // later members of a voxel never change the container (grid[key] finds the node), so inserting the first
        // occurrences in input order builds exactly the reference's table
        std::unordered_map<VoxelKey, int, VoxelKeyHash> grid;
        for (int r = 0; r < v; ++r) grid.emplace(VoxelKey{leaders[r].x, leaders[r].y, leaders[r].z}, leaders[r].w);
        if ((int)grid.size() != v) {
            snprintf(ctx->err, sizeof(ctx->err), "voxel: host replay found %zu voxels, device %d", grid.size(), v);
            return TDV_ERR_INTERNAL;
        }
        for (auto& kv : grid) order_first.push_back(kv.second);
    } else {
#if TDV_HAVE_LIBSTDCXX_EMULATION
        LibstdcxxInsertionOrder order((size_t)v);
        for (int r = 0; r < v; ++r) order.insert((size_t)voxel_key_code(leaders[r].x, leaders[r].y, leaders[r].z));
        order.for_each([&](int r) { order_first.push_back(leaders[r].w); });
#endif
    }
    if (study_env("TDV_DEBUG")) fprintf(stderr, "[tdv] voxel reference order: %d leaders replayed in %.3f ms (%s)\n", v,
                                   std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host0).count(), real_map ? "std::unordered_map" : "emulation");
    if (n_first != v) { snprintf(ctx->err, sizeof(ctx->err), "voxel: host replay listed %d voxels, device %d", n_first, v); return TDV_ERR_INTERNAL; }
    TDV_HIP(ctx, hipMemcpyAsync(d_order, order_pinned, (size_t)v * 4, hipMemcpyHostToDevice, s));
    k_voxel_permute<<<(v + 255) / 256, 256, 0, s>>>(tmp_xyz, tmp_rgb, d_rank, rank_base, d_order, v, d_out_xyz, d_out_rgb,
                                                    both ? both->ref2first : nullptr, both ? both->first2ref : nullptr, nrm);
    TDV_CHECK_LAUNCH(ctx);
    TDV_HIP(ctx, hipStreamSynchronize(s));  // the pinned staging is reused by the next call
    return TDV_OK;
}

// ---- the reference's container order ON THE DEVICE, for all clouds of a batch (round 3) ---------------------------------
// What the host replay above computes node by node has a closed form per rehash period.  Between two rehashes libstdc++ puts a
// new node at the FRONT of its bucket's run, and a bucket that was empty at the FRONT of the whole list (_M_insert_bucket_begin);
// a rehash walks the list front to back and re-inserts every node by the same rule (_M_rehash_aux).  So after a period with
// bucket count B the list is the REVERSE of: the period's insertion sequence - the previous list front to back, then the new
// keys in input order - grouped stably by bucket (code mod B), groups in order of first appearance.  With s(e) = position of
// element e in that sequence (its previous rank, or its own index if it is new: the previous list holds exactly the elements
// before it), first(b) = smallest s in bucket b, and F = the bucket sizes written at their first positions:
//     rank(e) = m - 1 - ( exclusive_scan(F)[first(bucket(e))] + #{x in bucket(e) : s(x) < s(e)} ),        m = elements so far
// One period = one memset + 3 small kernels + a scan over ALL clouds of the batch; ~17 periods reach 170k voxels (the bucket
// counts 13, 29, 59, 127 ... are libstdc++'s, taken from its own _Prime_rehash_policy on the host: they depend on the element
// count only).  Buckets hold their members' s in rows of RO_K; a fuller bucket (a degenerate hash) flags its cloud, which is then
// finished by the host replay.  No leader leaves the device, the lanes of the batch never wait for the host.
constexpr int RO_K = 16;
__global__ void k_ro_codes(const int4* __restrict__ leaders, int total_v, unsigned long long* __restrict__ code) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= total_v) return;
    const int4 l = leaders[p];
    code[p] = voxel_key_code(l.x, l.y, l.z);
}
// grid (ceil(n_next / 256), clouds).  A cloud takes part in the period while it has elements past n_k; m = its elements so far.
__global__ __launch_bounds__(256)
void k_ro_insert(const unsigned long long* __restrict__ code, const int* __restrict__ rank, const int* __restrict__ voff, int n_k, int n_next, unsigned nb,
                 int* __restrict__ fmax, int* __restrict__ cnt, int* __restrict__ rows, int* __restrict__ overflow) {
    const int b = blockIdx.y, v0 = voff[b], v = voff[b + 1] - v0;
    if (v <= n_k) return;
    const int m = min(v, n_next), e = blockIdx.x * 256 + threadIdx.x;
    if (e >= m) return;
    const size_t P = (size_t)v0 + e;
    const int s = e < n_k ? rank[P] : e;
    const size_t slot = (size_t)b * nb + (size_t)(code[P] % (unsigned long long)nb);
    atomicMax(&fmax[slot], 0x7fffffff - s);                // first(b) = 0x7fffffff - fmax: a zero fill initialises it
    const int pos = atomicAdd(&cnt[slot], 1);
    if (pos < RO_K) rows[slot * RO_K + pos] = s; else overflow[b] = 1;
}
__global__ __launch_bounds__(256)
void k_ro_first_sizes(const int* __restrict__ voff, int n_k, int n_next, unsigned nb, const int* __restrict__ fmax, const int* __restrict__ cnt, int* __restrict__ F) {
    const int b = blockIdx.y;
    if (voff[b + 1] - voff[b] <= n_k) return;
    const unsigned k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nb) return;
    const size_t slot = (size_t)b * nb + k;
    const int c = cnt[slot];
    if (c) F[(size_t)b * n_next + (0x7fffffff - fmax[slot])] = c;
}
__global__ __launch_bounds__(256)
void k_ro_rank(const unsigned long long* __restrict__ code, int* __restrict__ rank, const int* __restrict__ voff, int n_k, int n_next, unsigned nb,
               const int* __restrict__ fmax, const int* __restrict__ cnt, const int* __restrict__ rows, const int* __restrict__ S) {
    const int b = blockIdx.y, v0 = voff[b], v = voff[b + 1] - v0;
    if (v <= n_k) return;
    const int m = min(v, n_next), e = blockIdx.x * 256 + threadIdx.x;
    if (e >= m) return;
    const size_t P = (size_t)v0 + e;
    const int s = e < n_k ? rank[P] : e;
    const size_t slot = (size_t)b * nb + (size_t)(code[P] % (unsigned long long)nb);
    const int first = 0x7fffffff - fmax[slot], c = min(cnt[slot], RO_K);
    int before = S[(size_t)b * n_next + first] - S[(size_t)b * n_next];
    const int* row = rows + slot * RO_K;
    for (int q = 0; q < c; ++q) before += row[q] < s ? 1 : 0;
    rank[P] = m - 1 - before;                                // in place: a lane reads and writes only its own element's rank
}
// out[voff[b] + rank] = first-order voxel; the permutation both ways (positions local to the cloud)
__global__ __launch_bounds__(256)
void k_ro_permute(const float* __restrict__ first_xyz, const int* __restrict__ rank, const int* __restrict__ voff, const int* __restrict__ skip,
                  float* __restrict__ out_xyz, int* __restrict__ ref2first, int* __restrict__ first2ref) {
    const int b = blockIdx.y, v0 = voff[b], v = voff[b + 1] - v0, e = blockIdx.x * 256 + threadIdx.x;
    if (e >= v || skip[b]) return;
    const size_t P = (size_t)v0 + e, O = (size_t)v0 + rank[P];
    copy_row3(out_xyz, O, first_xyz, P);
    if (ref2first) { ref2first[O] = e; first2ref[P] = (int)(O - v0); }
}

#if TDV_HAVE_LIBSTDCXX_EMULATION
// (first element index, bucket count) of every rehash period a container of up to n_max elements goes through, from the
// library's own policy object
static void rehash_schedule(int n_max, std::vector<std::pair<int, unsigned>>& out) {
    static std::mutex mu; static std::vector<std::pair<int, unsigned>> cache; static int cached_to = 0;
    static std::__detail::_Prime_rehash_policy policy; static size_t buckets = 1;
    std::lock_guard<std::mutex> lock(mu);
    for (; cached_to < n_max; ++cached_to) {
        const auto rh = policy._M_need_rehash(buckets, (size_t)cached_to, 1);
        if (rh.first) { buckets = rh.second; cache.emplace_back(cached_to, (unsigned)buckets); }
    }
    out.clear();
    for (auto& p : cache) if (p.first < n_max) out.push_back(p);
}
#endif

// Reference order of every cloud of a batch on the device.  d_leaders / d_first_xyz / outputs are indexed by global first-
// occurrence position (cloud b at [h_voff[b], h_voff[b + 1])); d_voff: the same offsets on the device.  h_failed[b] = 1: a
// bucket of cloud b overflowed its row (or this build has no libstdc++): its slice of the outputs is untouched, the caller
// finishes it with voxel_reference_order.
int voxel_reference_order_batch_dev(tdv_ctx* ctx, int n_clouds, const int* h_voff, const int* d_voff, const int4* d_leaders, const float* d_first_xyz,
                                    float* d_out_xyz, int* d_ref2first, int* d_first2ref, int* h_failed) {
    for (int b = 0; b < n_clouds; ++b) h_failed[b] = TDV_HAVE_LIBSTDCXX_EMULATION ? 0 : 1;
#if TDV_HAVE_LIBSTDCXX_EMULATION
    const int total_v = h_voff[n_clouds];
    if (total_v == 0) return TDV_OK;
    int v_max = 0;
    for (int b = 0; b < n_clouds; ++b) v_max = std::max(v_max, h_voff[b + 1] - h_voff[b]);
    std::vector<std::pair<int, unsigned>> sched;
    rehash_schedule(v_max, sched);
    hipStream_t s = ctx->stream;
    unsigned long long* code; int *rank, *d_overflow;
    TDV_TRY(ws_alloc(ctx, (size_t)total_v, &code));
    TDV_TRY(ws_alloc(ctx, (size_t)total_v, &rank));
    TDV_TRY(ws_alloc(ctx, (size_t)n_clouds, &d_overflow));
    TDV_HIP(ctx, hipMemsetAsync(d_overflow, 0, (size_t)n_clouds * 4, s));
    k_ro_codes<<<(total_v + 255) / 256, 256, 0, s>>>(d_leaders, total_v, code);
    const WsMark mark = ws_mark(ctx);
    ScopedTimer tm(ctx, TDV_TIMER_VOXEL);
    for (size_t k = 0; k < sched.size(); ++k) {
        const int n_k = sched[k].first, n_next = std::min(k + 1 < sched.size() ? sched[k + 1].first : v_max, v_max);
        const unsigned nb = sched[k].second;
        ws_rewind(ctx, mark);                                  // every period reuses the same scratch (stream order keeps them apart)
        const size_t n_tab = (size_t)n_clouds * nb, n_F = (size_t)n_clouds * n_next;
        if (n_F + 1 > 0x7fffffffull) { for (int b = 0; b < n_clouds; ++b) h_failed[b] = 1; return TDV_OK; }   // (beyond the 32-bit scan: host replay)
        int *zero, *rows, *S, *d_tot;
        TDV_TRY(ws_alloc(ctx, 2 * n_tab + n_F, &zero));       // fmax | cnt | F: one fill
        TDV_TRY(ws_alloc(ctx, n_tab * RO_K, &rows));
        TDV_TRY(ws_alloc(ctx, n_F, &S));
        TDV_TRY(ws_alloc(ctx, 1, &d_tot));
        int *fmax = zero, *cnt = zero + n_tab, *F = zero + 2 * n_tab;
        TDV_HIP(ctx, hipMemsetAsync(zero, 0, (2 * n_tab + n_F) * 4, s));
        const dim3 ge((n_next + 255) / 256, n_clouds), gb((nb + 255) / 256, n_clouds);
        k_ro_insert<<<ge, 256, 0, s>>>(code, rank, d_voff, n_k, n_next, nb, fmax, cnt, rows, d_overflow);
        k_ro_first_sizes<<<gb, 256, 0, s>>>(d_voff, n_k, n_next, nb, fmax, cnt, F);
        TDV_TRY(exclusive_scan_dev(ctx, F, (int)n_F, S, d_tot));
        k_ro_rank<<<ge, 256, 0, s>>>(code, rank, d_voff, n_k, n_next, nb, fmax, cnt, rows, S);
        TDV_CHECK_LAUNCH(ctx);
    }
    k_ro_permute<<<dim3((v_max + 255) / 256, n_clouds), 256, 0, s>>>(d_first_xyz, rank, d_voff, d_overflow, d_out_xyz, d_ref2first, d_first2ref);
    TDV_CHECK_LAUNCH(ctx);
    TDV_TRY(pin_reserve(ctx, (size_t)n_clouds * 4));
    TDV_HIP(ctx, hipMemcpyAsync(ctx->pin, d_overflow, (size_t)n_clouds * 4, hipMemcpyDeviceToHost, s));
    TDV_HIP(ctx, hipStreamSynchronize(s));
    std::memcpy(h_failed, ctx->pin, (size_t)n_clouds * 4);
    ws_rewind(ctx, mark);
#endif
    return TDV_OK;
}

// One cloud's v voxels from first-occurrence order (first: rows of n, with the leaders' ranks and records) into the reference's order:
// on the device (the batch's way, ~17 rehash periods of small launches) when there are enough voxels for the host replay's 22 ns per
// voxel + two copies to cost more - measured cross-over around 10k voxels (tools/studies/voxel_probe.py); TDV_VOXEL_DEVICE_ORDER=0 / 1
// forces either.  Colours and normals ride along through the permutation.
int voxel_finish_reference(tdv_ctx* ctx, int n, int v, const VoxelFirst& first, float* d_out_xyz, float* d_out_rgb, float* d_out_nrm,
                           const VoxelBothOrders* both, const VoxelKnobs& knobs) {
    hipStream_t s = ctx->stream;
    if (TDV_HAVE_LIBSTDCXX_EMULATION && (knobs.device_order < 0 ? v >= 10000 : knobs.device_order != 0)) {
        int *r2f, *f2r; int failed = 1;
        if (both) { r2f = both->ref2first; f2r = both->first2ref; }
        else { TDV_TRY(ws_alloc(ctx, (size_t)v, &r2f)); TDV_TRY(ws_alloc(ctx, (size_t)v, &f2r)); }
        int* d_voff1;
        TDV_TRY(ws_alloc(ctx, 2, &d_voff1));
        const int h_voff1[2] = {0, v};
        TDV_HIP(ctx, hipMemcpyAsync(d_voff1, h_voff1, 8, hipMemcpyHostToDevice, s));
        TDV_TRY(voxel_reference_order_batch_dev(ctx, 1, h_voff1, d_voff1, first.leaders, first.xyz, d_out_xyz, r2f, f2r, &failed));
        if (!failed) {
            if (first.rgb && d_out_rgb) k_gather_rows3<<<(v + 255) / 256, 256, 0, s>>>(first.rgb, r2f, v, d_out_rgb);
            if (first.nrm) k_gather_rows3<<<(v + 255) / 256, 256, 0, s>>>(first.nrm, r2f, v, d_out_nrm);
            if ((first.rgb && d_out_rgb) || first.nrm) {
                TDV_CHECK_LAUNCH(ctx);
                TDV_HIP(ctx, hipStreamSynchronize(s));
            }
            return TDV_OK;
        }
    }
    return voxel_reference_order(ctx, v, n, first.leaders, first.xyz, first.rgb, first.rank, 0, d_out_xyz, d_out_rgb, both, VoxelNormals{first.nrm, d_out_nrm});
}

}  // namespace tdv
