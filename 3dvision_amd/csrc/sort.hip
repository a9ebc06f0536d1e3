// The generic device primitives: the radix sort of pairs (first), the bitonic sorts of 16-byte records and the exclusive scan (below).
// Each has a direct test: tests/test_gpu_sort.py (the radix sort against a stable argsort), tests/test_gpu_primitives_probe.py (the
// bitonic sorts at every shape of their launch chain and the scan up to three rounds of its last workgroup's loop, through probe.hip).
//
// Stable LSD radix sort of (64-bit key, 32-bit value) pairs on the low `end_bit` bits of the key, hand-written for gfx950 (round 4;
// rounds 2-3 called rocPRIM's device radix sort here).  Used by the descriptor index build (csrc/fmatch_index.hip: two sorts of ~150k
// (key, row) pairs once per model) - a launch-bound size, so the design goal is FEW launches of short kernels, not bandwidth:
//   per pass of up to 8 bits, two launches
//     k_rs_count    every workgroup (2,048 pairs) counts its digits into a digit-major table [256][workgroups]
//     k_rs_scatter  every workgroup ranks its pairs stably and writes them: a pair's place = the exclusive scan of the table (digit-major
//                   order IS the output order) at [digit][workgroup] + the pairs of the same digit before it in the workgroup.  Up to
//                   RS_SELF_SCAN_MAX workgroups each scatter workgroup works its 256 scan values out of the raw table itself (a quarter
//                   of a row per thread, all loads in flight: ~76 KB from L2 at 150k pairs); above that the LAST workgroup of k_rs_count
//                   to finish (a ticket) scans the table in place - the release / acquire fences of that hand-over write back and
//                   invalidate an XCD's L2 and cost 10-20 us per launch, which only a large sort amortises.  Pairs are held striped (pair r * 1024 + thread), so "before it" is
//                   (round, wave, lane) order: within a wave a match-any of the digit (8 ballots) gives the rank among the lanes and the
//                   group's count, the 32 (round, wave) groups are then chained per digit by 256 threads through LDS.
//   the digit width is end_bit / passes rounded up, so 33 bits are five passes of 7 bits and 42 bits six of 7.
// No look-back, no spinning.
// Measured against rocPRIM on the index build's two sorts: profiles/r4/history/radix_sort.md.
#include <cstring>
#include "tdv_internal.hpp"

namespace tdv {

constexpr int RS_THREADS = 1024, RS_WAVES = RS_THREADS / 64, RS_ROUNDS = 2, RS_TILE = RS_THREADS * RS_ROUNDS, RS_GROUPS = RS_ROUNDS * RS_WAVES;
constexpr int RS_BINS = 256;
constexpr int RS_SELF_SCAN_MAX = 1024;      // workgroups (2 M pairs) up to which k_rs_scatter scans the raw table itself

// the lanes of the wave that hold a pair (valid) with the same digit as this lane
__device__ __forceinline__ unsigned long long rs_peers(unsigned d, bool valid, int bits) {
    unsigned long long peers = __ballot(valid);
    for (int b = 0; b < bits; ++b) {
        const unsigned long long m = __ballot((d >> b) & 1u);
        peers &= ((d >> b) & 1u) ? m : ~m;
    }
    return peers;
}

template <bool SCAN>
__global__ __launch_bounds__(RS_THREADS)
void k_rs_count(const unsigned long long* __restrict__ keys, size_t n, int shift, unsigned mask, int bits, int nb, int* __restrict__ table, unsigned* __restrict__ ticket) {
    __shared__ int hist[RS_BINS];
    __shared__ bool is_last;
    __shared__ int wsum[RS_WAVES];
    if (threadIdx.x < RS_BINS) hist[threadIdx.x] = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * RS_TILE;
    const unsigned long long lt = (1ull << (threadIdx.x & 63)) - 1ull;
#pragma unroll
    for (int r = 0; r < RS_ROUNDS; ++r) {
        const size_t i = base + (size_t)r * RS_THREADS + threadIdx.x;
        const bool valid = i < n;
        const unsigned d = valid ? (unsigned)(keys[i] >> shift) & mask : 0u;
        const unsigned long long peers = rs_peers(d, valid, bits);      // one LDS atomic per digit and wave: the high digits of a key are a few values
        if (valid && (peers & lt) == 0ull) atomicAdd(&hist[d], (int)__popcll(peers));
    }
    __syncthreads();
    if (threadIdx.x < RS_BINS) table[(size_t)threadIdx.x * nb + blockIdx.x] = hist[threadIdx.x];
    if (!SCAN) return;
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");       // the counts are visible device-wide before the ticket moves
        is_last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!is_last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");           // acquire: the other workgroups' counts
    // exclusive scan of the whole table by this workgroup: a thread owns `per` consecutive entries - it adds them up (independent loads, all
    // in flight), the 1,024 sums are scanned through LDS, and a second walk writes the running prefix.  (First version: 1,024 entries per
    // round with a load, three barriers and a store in each - a memory latency per round, 16.7 us per launch at 37 workgroups.)
    // (relaxed device-scope atomic loads, not `volatile`: the compiler waits for every volatile access before it issues the next one -
    //  19 + 19 memory latencies per thread, 30 us per launch - while these stay in flight together)
    const int total = RS_BINS * nb;
    const int per = (total + RS_THREADS - 1) / RS_THREADS;
    const int i0 = min(threadIdx.x * per, total), i1 = min(i0 + per, total);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int sum = 0;
#pragma unroll 8
    for (int i = i0; i < i1; ++i) sum += __hip_atomic_load(&table[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const int t = __shfl_up(incl, off, 64); if (lane >= off) incl += t; }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int run = incl - sum;
    for (int w = 0; w < wave; ++w) run += wsum[w];
#pragma unroll 8
    for (int i = i0; i < i1; ++i) {
        const int v = __hip_atomic_load(&table[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        table[i] = run; run += v;
    }
    if (threadIdx.x == 0) *ticket = 0u;                           // ready for the next launch
}

template <bool SCANNED>
__global__ __launch_bounds__(RS_THREADS)
void k_rs_scatter(const unsigned long long* __restrict__ keys_in, const unsigned* __restrict__ vals_in, size_t n, int shift, unsigned mask, int bits, int nb,
                  const int* __restrict__ table, unsigned long long* __restrict__ keys_out, unsigned* __restrict__ vals_out) {
    __shared__ unsigned char cnt[RS_GROUPS][RS_BINS];          // pairs of a digit in a (round, wave) group: at most 64
    __shared__ unsigned short offs[RS_GROUPS][RS_BINS];        // ... in the groups before it
    __shared__ int gbase[RS_BINS];
    {
        unsigned* z = reinterpret_cast<unsigned*>(&cnt[0][0]);
#pragma unroll
        for (int k = 0; k < RS_GROUPS * RS_BINS / 4 / RS_THREADS; ++k) z[k * RS_THREADS + threadIdx.x] = 0u;
        static_assert(RS_GROUPS * RS_BINS / 4 % RS_THREADS == 0, "the count table is cleared in whole rounds");
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long lt = (1ull << lane) - 1ull;
    if (SCANNED) {
        if (threadIdx.x < RS_BINS) gbase[threadIdx.x] = table[(size_t)threadIdx.x * nb + blockIdx.x];
    } else {
        // this workgroup's 256 values of the table's exclusive scan, out of the raw counts: thread (part, digit) adds up a quarter of the
        // digit's row - all of it, and what lies before this workgroup's column
        __shared__ int part_all[RS_THREADS / RS_BINS][RS_BINS], part_pre[RS_THREADS / RS_BINS][RS_BINS];
        __shared__ int wtot[RS_BINS / 64];
        constexpr int PARTS = RS_THREADS / RS_BINS;
        const int d = threadIdx.x & (RS_BINS - 1), part = threadIdx.x / RS_BINS;
        const int per = (nb + PARTS - 1) / PARTS, b0 = min(part * per, nb), b1 = min(b0 + per, nb);
        const int* __restrict__ row = table + (size_t)d * nb;
        int all = 0, pre = 0;
#pragma unroll 8
        for (int b = b0; b < b1; ++b) { const int v = row[b]; all += v; pre += b < (int)blockIdx.x ? v : 0; }
        part_all[part][d] = all; part_pre[part][d] = pre;
        __syncthreads();
        if (threadIdx.x < RS_BINS) {
            int rowsum = 0, rowpre = 0;
#pragma unroll
            for (int q = 0; q < PARTS; ++q) { rowsum += part_all[q][d]; rowpre += part_pre[q][d]; }
            int incl = rowsum;                                    // exclusive scan of the 256 row sums: the pairs of all smaller digits
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) { const int t = __shfl_up(incl, off, 64); if (lane >= off) incl += t; }
            if (lane == 63) wtot[wave] = incl;
            part_all[0][d] = incl - rowsum + rowpre;              // (own slot: read above by this thread only)
        }
        __syncthreads();
        if (threadIdx.x < RS_BINS) {
            int before = 0;
            for (int w = 0; w < wave; ++w) before += wtot[w];
            gbase[d] = part_all[0][d] + before;
        }
    }
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * RS_TILE;
    unsigned long long key[RS_ROUNDS]; unsigned val[RS_ROUNDS]; int digit[RS_ROUNDS], rank[RS_ROUNDS];
#pragma unroll
    for (int r = 0; r < RS_ROUNDS; ++r) {
        const size_t i = base + (size_t)r * RS_THREADS + threadIdx.x;
        const bool valid = i < n;
        key[r] = valid ? keys_in[i] : 0ull; val[r] = valid ? vals_in[i] : 0u;
        const unsigned d = (unsigned)(key[r] >> shift) & mask;
        digit[r] = valid ? (int)d : -1;
        const unsigned long long peers = rs_peers(d, valid, bits);
        rank[r] = __popcll(peers & lt);
        if (valid && rank[r] == 0) cnt[r * RS_WAVES + wave][d] = (unsigned char)__popcll(peers);
    }
    __syncthreads();
    if (threadIdx.x < RS_BINS) {
        int run = 0;
#pragma unroll 8
        for (int g = 0; g < RS_GROUPS; ++g) { offs[g][threadIdx.x] = (unsigned short)run; run += cnt[g][threadIdx.x]; }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RS_ROUNDS; ++r) {
        if (digit[r] < 0) continue;
        const size_t dst = (size_t)gbase[digit[r]] + offs[r * RS_WAVES + wave][digit[r]] + rank[r];
        keys_out[dst] = key[r]; vals_out[dst] = val[r];
    }
}

int radix_sort_pairs_dev(tdv_ctx* ctx, const unsigned long long* d_keys_in, unsigned long long* d_keys_out,
                         const unsigned* d_vals_in, unsigned* d_vals_out, size_t n, int end_bit) {
    if (!ctx || end_bit < 1 || end_bit > 64 || (n > 0 && (!d_keys_in || !d_keys_out || !d_vals_in || !d_vals_out))) return TDV_ERR_BAD_ARG;
    if (n == 0) return TDV_OK;
    if (n > (size_t)1 << 30) return TDV_ERR_BAD_ARG;              // (places are 32-bit)
    const int passes = (end_bit + 7) / 8, bits = (end_bit + passes - 1) / passes;
    const int nb = (int)((n + RS_TILE - 1) / RS_TILE);
    int* table = nullptr; unsigned long long* tkeys = nullptr; unsigned* tvals = nullptr;
    TDV_TRY(ws_alloc(ctx, (size_t)RS_BINS * nb, &table));
    if (passes > 1) { TDV_TRY(ws_alloc(ctx, n, &tkeys)); TDV_TRY(ws_alloc(ctx, n, &tvals)); }
    hipStream_t s = ctx->stream;
    unsigned* ticket = ctx->scan_ticket + 9;
    const unsigned long long* kin = d_keys_in; const unsigned* vin = d_vals_in;
    for (int p = 0; p < passes; ++p) {
        // the last pass writes the caller's buffers; the passes before it alternate between them and the temporaries
        const bool to_out = ((passes - 1 - p) & 1) == 0;
        unsigned long long* kout = to_out ? d_keys_out : tkeys; unsigned* vout = to_out ? d_vals_out : tvals;
        const int shift = p * bits, width = std::min(bits, end_bit - shift);
        const unsigned mask = (1u << width) - 1u;
        if (nb <= RS_SELF_SCAN_MAX) {
            k_rs_count<false><<<nb, RS_THREADS, 0, s>>>(kin, n, shift, mask, width, nb, table, ticket);
            k_rs_scatter<false><<<nb, RS_THREADS, 0, s>>>(kin, vin, n, shift, mask, width, nb, table, kout, vout);
        } else {
            k_rs_count<true><<<nb, RS_THREADS, 0, s>>>(kin, n, shift, mask, width, nb, table, ticket);
            k_rs_scatter<true><<<nb, RS_THREADS, 0, s>>>(kin, vin, n, shift, mask, width, nb, table, kout, vout);
        }
        kin = kout; vin = vout;
    }
    TDV_CHECK_LAUNCH(ctx);
    return TDV_OK;
}

// ---- bitonic sorts of 16-byte records (the voxel grouping's full sort, knn.hip's Morton order, the columns of the descriptor index) ----
constexpr int BT_TILE = 2048;     // records per LDS tile (32 KB)
constexpr int BT_THREADS = 1024;  // one compare-exchange per thread per pass

__device__ __forceinline__ void cmpxchg(uint4& a, uint4& b, bool ascending) {
    bool sw = ascending ? rec_less(b, a) : rec_less(a, b);
    if (sw) { uint4 t = a; a = b; b = t; }
}

// full bitonic sort of each 2048-record tile (all k <= BT_TILE)
__global__ __launch_bounds__(BT_THREADS)
void k_bitonic_local_sort(uint4* __restrict__ rec) {
    __shared__ uint4 s[BT_TILE];
    const size_t base = (size_t)blockIdx.x * BT_TILE;
    const int t = threadIdx.x;
    s[t] = rec[base + t]; s[t + BT_THREADS] = rec[base + t + BT_THREADS];
    __syncthreads();
    for (int k = 2; k <= BT_TILE; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            int i = ((t / j) * (j << 1)) + (t % j);
            bool asc = (((base + i) & (size_t)k) == 0);
            cmpxchg(s[i], s[i + j], asc);
            __syncthreads();
        }
    }
    rec[base + t] = s[t]; rec[base + t + BT_THREADS] = s[t + BT_THREADS];
}

// one global compare-exchange pass (stride j >= BT_TILE)
__global__ __launch_bounds__(256)
void k_bitonic_global_step(uint4* __restrict__ rec, size_t n_pairs, unsigned k, unsigned j) {
    size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_pairs) return;
    size_t i = ((t / j) * ((size_t)j << 1)) + (t % j);
    uint4 a = rec[i], b = rec[i + j];
    bool asc = ((i & (size_t)k) == 0);
    bool sw = asc ? rec_less(b, a) : rec_less(a, b);
    if (sw) { rec[i] = b; rec[i + j] = a; }
}

// two global passes in one launch (strides j and j / 2, both >= BT_TILE): a thread holds the four records its two
// compare-exchanges per pass touch.  The sort of 131k-262k records is a chain of ~30 tiny launches; this removes a third.
__global__ __launch_bounds__(256)
void k_bitonic_global_step2(uint4* __restrict__ rec, size_t n_quads, unsigned k, unsigned j) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_quads) return;
    const size_t h = j >> 1;                                              // the second stride
    const size_t i = ((t / h) * ((size_t)j << 1)) + (t % h);              // bits j and h of i are clear
    uint4 a = rec[i], b = rec[i + h], c = rec[i + j], d = rec[i + j + h];
    const bool asc = ((i & (size_t)k) == 0);                              // k > j: the same for all four
    cmpxchg(a, c, asc); cmpxchg(b, d, asc);                               // stride j
    cmpxchg(a, b, asc); cmpxchg(c, d, asc);                               // stride j / 2
    rec[i] = a; rec[i + h] = b; rec[i + j] = c; rec[i + j + h] = d;
}

// all passes with stride < BT_TILE of merge stage k, inside LDS
__global__ __launch_bounds__(BT_THREADS)
void k_bitonic_local_merge(uint4* __restrict__ rec, unsigned k) {
    __shared__ uint4 s[BT_TILE];
    const size_t base = (size_t)blockIdx.x * BT_TILE;
    const int t = threadIdx.x;
    s[t] = rec[base + t]; s[t + BT_THREADS] = rec[base + t + BT_THREADS];
    __syncthreads();
    for (int j = BT_TILE >> 1; j > 0; j >>= 1) {
        int i = ((t / j) * (j << 1)) + (t % j);
        bool asc = (((base + i) & (size_t)k) == 0);
        cmpxchg(s[i], s[i + j], asc);
        __syncthreads();
    }
    rec[base + t] = s[t]; rec[base + t + BT_THREADS] = s[t + BT_THREADS];
}

// ascending bitonic sort of n_pow2 (power of two, >= BT_TILE) uint4 records by (x, y, z, w); also used by knn.hip
int sort_records_dev(tdv_ctx* ctx, uint4* rec, size_t n_pow2) {
    hipStream_t s = ctx->stream;
    const unsigned tiles = (unsigned)(n_pow2 / BT_TILE);
    k_bitonic_local_sort<<<tiles, BT_THREADS, 0, s>>>(rec);
    for (size_t k = (size_t)BT_TILE << 1; k <= n_pow2; k <<= 1) {
        for (size_t j = k >> 1; j >= BT_TILE; j >>= 1) {
            if ((j >> 1) >= BT_TILE) {
                k_bitonic_global_step2<<<(unsigned)((n_pow2 / 4 + 255) / 256), 256, 0, s>>>(rec, n_pow2 / 4, (unsigned)k, (unsigned)j);
                j >>= 1;
            } else {
                k_bitonic_global_step<<<(unsigned)((n_pow2 / 2 + 255) / 256), 256, 0, s>>>(rec, n_pow2 / 2, (unsigned)k, (unsigned)j);
            }
        }
        k_bitonic_local_merge<<<tiles, BT_THREADS, 0, s>>>(rec, (unsigned)k);
    }
    TDV_CHECK_LAUNCH(ctx);
    return TDV_OK;
}

// Every segment [seg_start[c], seg_start[c + 1]) of rec sorted on its own, one workgroup and one launch for all of them:
// for segments of at most BT_TILE records (the caller checks), e.g. the columns of the descriptor index, whose records
// only have to be ordered inside their column.
__global__ __launch_bounds__(BT_THREADS)
void k_bitonic_segment_sort(uint4* __restrict__ rec, const int* __restrict__ seg_start) {
    __shared__ uint4 s[BT_TILE];
    const int c0 = seg_start[blockIdx.x], m = seg_start[blockIdx.x + 1] - c0;
    if (m <= 1) return;
    const int t = threadIdx.x;
    const uint4 pad = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
    s[t] = t < m ? rec[(size_t)c0 + t] : pad;
    s[t + BT_THREADS] = t + BT_THREADS < m ? rec[(size_t)c0 + t + BT_THREADS] : pad;
    __syncthreads();
    int span = 2;
    while (span < m) span <<= 1;                      // the padded power of two that holds the segment
    for (int k = 2; k <= span; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int i = ((t / j) * (j << 1)) + (t % j);
            if (i + j < span) cmpxchg(s[i], s[i + j], (i & k) == 0);
            __syncthreads();
        }
    }
    if (t < m) rec[(size_t)c0 + t] = s[t];
    if (t + BT_THREADS < m) rec[(size_t)c0 + t + BT_THREADS] = s[t + BT_THREADS];
}
int segment_sort_records_dev(tdv_ctx* ctx, uint4* rec, const int* d_seg_start, int nseg) {
    if (nseg <= 0) return TDV_OK;
    k_bitonic_segment_sort<<<nseg, BT_THREADS, 0, ctx->stream>>>(rec, d_seg_start);
    TDV_CHECK_LAUNCH(ctx);
    return TDV_OK;
}
int segment_sort_max_len() { return BT_TILE; }

// exclusive scan of n ints in TWO launches: per-block (4096 items: 1024 threads x 4) reduce whose LAST workgroup (atomic
// ticket) scans the block sums, then the local scan.  (Round 1 used three launches; the scan sits on every grouping path —
// voxel x2, Morton order, descriptor buckets, batched depth — and each launch costs ~5 us on a path that is launch-bound
// anyway.  Four items per thread: a quarter of the workgroups, tickets and barriers for the 524k-bucket tables of the voxel
// hash, whose scan took 50 us with one item per thread.)
constexpr int SCAN_IPT = 4;
constexpr int SCAN_BLOCK_ITEMS = 1024 * SCAN_IPT;
__device__ __forceinline__ void scan_load4(const int* __restrict__ in, int n, int i0, int (&x)[SCAN_IPT]) {
    if (i0 + SCAN_IPT <= n && (((size_t)in & 15) == 0)) {
        const int4 q = *reinterpret_cast<const int4*>(in + i0);
        x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
    } else {
#pragma unroll
        for (int e = 0; e < SCAN_IPT; ++e) x[e] = i0 + e < n ? in[i0 + e] : 0;
    }
}
__global__ __launch_bounds__(1024)
void k_scan_reduce(const int* __restrict__ in, int n, int* __restrict__ sums, int* __restrict__ total, unsigned* __restrict__ ticket) {
    __shared__ int w[16];
    __shared__ int carry_s;
    __shared__ bool is_last;
    const int i0 = (blockIdx.x * 1024 + threadIdx.x) * SCAN_IPT;
    int x[SCAN_IPT];
    scan_load4(in, n, i0, x);
    int v = (x[0] + x[1]) + (x[2] + x[3]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int k = 0; k < 16; ++k) s += w[k];
        sums[blockIdx.x] = s;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");       // the sum is visible device-wide before the ticket moves (release only: __threadfence() would also invalidate the XCD's L2 under the workgroups still loading)
        is_last = atomicAdd(ticket, 1u) == gridDim.x - 1;
        carry_s = 0;
    }
    __syncthreads();
    if (!is_last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");           // acquire: the other workgroups' sums
    const int nblocks = gridDim.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    volatile int* vs = sums;                                    // written by other workgroups of this launch
    for (int b0 = 0; b0 < nblocks; b0 += 1024) {
        int k = b0 + threadIdx.x;
        int xs = k < nblocks ? vs[k] : 0;
        int incl = xs;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { int t = __shfl_up(incl, off, 64); if (lane >= off) incl += t; }
        if (lane == 63) w[wave] = incl;
        __syncthreads();
        int wbase = 0;
        for (int q = 0; q < wave; ++q) wbase += w[q];
        int carry = carry_s;
        if (k < nblocks) vs[k] = carry + wbase + incl - xs;
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = carry + wbase + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) { *total = carry_s; *ticket = 0u; }   // ready for the next launch (stream order)
}
__global__ __launch_bounds__(1024)
void k_scan_local(const int* __restrict__ in, int n, const int* __restrict__ sums, int* __restrict__ out) {
    __shared__ int wsum[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i0 = (blockIdx.x * 1024 + threadIdx.x) * SCAN_IPT;
    int x[SCAN_IPT];
    scan_load4(in, n, i0, x);
    const int v = (x[0] + x[1]) + (x[2] + x[3]);
    int incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { int t = __shfl_up(incl, off, 64); if (lane >= off) incl += t; }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int wbase = 0;
    for (int q = 0; q < wave; ++q) wbase += wsum[q];
    int run = sums[blockIdx.x] + wbase + incl - v;          // exclusive prefix of this thread's first item
#pragma unroll
    for (int e = 0; e < SCAN_IPT; ++e) { if (i0 + e < n) out[i0 + e] = run; run += x[e]; }
}

// exclusive scan of n ints on the ctx stream; *d_total receives the sum (device pointer)
int exclusive_scan_dev(tdv_ctx* ctx, const int* d_in, int n, int* d_out, int* d_total) {
    if (n <= 0) return TDV_OK;
    const int sblocks = (n + SCAN_BLOCK_ITEMS - 1) / SCAN_BLOCK_ITEMS;
    int* sums;
    TDV_TRY(ws_alloc(ctx, (size_t)sblocks, &sums));
    hipStream_t s = ctx->stream;
    k_scan_reduce<<<sblocks, 1024, 0, s>>>(d_in, n, sums, d_total, ctx->scan_ticket);
    k_scan_local<<<sblocks, 1024, 0, s>>>(d_in, n, sums, d_out);
    TDV_CHECK_LAUNCH(ctx);
    return TDV_OK;
}

size_t sort_pow2(size_t n) { size_t p = BT_TILE; while (p < n) p <<= 1; return p; }

}  // namespace tdv
