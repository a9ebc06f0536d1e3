// Study-build parts of csrc/fmatch.hip (-DTDV_STUDY only): the searches that lost their measurement and the statistics reports.
// Included by fmatch.hip inside namespace tdv, after the kernels, scan_splits, FmRun / LmRun, fm_scan_all and fm_walk; it is not a
// header for anything else.
// Round 1's key-ordered pruned scan (TDV_FM_KEYORDER); then, at the end: the scan without early exit (TDV_FM_NO_EARLY_EXIT), the walk
// with 1 or 4 sources per wave (TDV_FM_K), the second round of box tests (TDV_LM_ROUNDS=2) and the reports of TDV_FM_STATS.
#pragma once
#include <cstdio>

// ---- exact pruned descriptor match (large problems) -------------------------------------------------------------
// FPFH descriptors of a real part are strongly clustered (most of their variance lies along one direction), so both
// sides are ordered by a cheap scalar key (the three centre bins) with a counting sort, 33-D bounding boxes are built
// over runs of 64 ordered targets, and a wave of neighbouring sources skips every box whose lower bound exceeds all
// its lanes' current best.  The bound is the distance expression itself applied to the per-dimension gaps, summed in
// the same order: every term is <= the corresponding term of any target inside the box and float addition /
// multiplication are monotone, so lb <= fl(dist) holds exactly and no margin is needed.  Targets are visited
// inside-out from the wave's own key position; ties keep the lowest ORIGINAL target index, as the CPU scan does.
// The order only affects speed: any key (and the arbitrary order inside a bucket) gives the same correspondences.
constexpr int FMP_BOX = 64;
constexpr int FMP_TWO_KEYS_MAX_TARGETS = 32768;
__device__ __forceinline__ int fm_bucket(const float* __restrict__ f, int two_keys) {
    // key 1: the three centre bins (descriptors sum to 1, so it lies in [0, 1]); key 2: the first moment of the phi
    // sub-histogram (in [0, 10]).  two_keys: FMP_KEY_BITS bits each, interleaved (a 128 x 128 Morton grid) — measured
    // better against a small model (C4: 128k x 9.4k, 0.71 -> 0.60 ms); else key 1 alone at full resolution — better
    // when the target side is large (100k x 100k: 8.3 vs 9.6 ms).  An offline study on real descriptors
    // (tools/studies/feature_match_box_pruning.py) put this pair ahead of every other cheap pair.
    const float c1 = f[5] + (f[16] + f[27]);
    if (!two_keys) {
        const float k = c1 * (float)FMP_BUCKETS;
        return (k == k) ? (int)fminf(fmaxf(k, 0.f), (float)(FMP_BUCKETS - 1)) : 0;
    }
    constexpr float LEVELS = (float)(1 << FMP_KEY_BITS);
    const float k1 = c1 * LEVELS;
    float k2 = 0.f;
#pragma unroll
    for (int b = 1; b < 11; ++b) k2 += (float)b * f[11 + b];
    k2 *= LEVELS * 0.1f;
    const unsigned a = (k1 == k1) ? (unsigned)fminf(fmaxf(k1, 0.f), LEVELS - 1.f) : 0u;
    const unsigned c = (k2 == k2) ? (unsigned)fminf(fmaxf(k2, 0.f), LEVELS - 1.f) : 0u;
    unsigned m = 0;
#pragma unroll
    for (int i = 0; i < FMP_KEY_BITS; ++i) m |= (((a >> i) & 1u) << (2 * i + 1)) | (((c >> i) & 1u) << (2 * i));
    return (int)m;
}
// Real descriptors crowd a few buckets, so the histogram is counted in LDS first (as k_fm_scatter does in fmatch.hip).
__global__ __launch_bounds__(FMP_SORT_BLOCK)
void k_fm_hist(const float* __restrict__ f, int n, int two_keys, int* __restrict__ bucket_of, int* __restrict__ hist) {
    __shared__ int h[FMP_BUCKETS];
    for (int b = threadIdx.x; b < FMP_BUCKETS; b += FMP_SORT_BLOCK) h[b] = 0;
    __syncthreads();
    const int i = blockIdx.x * FMP_SORT_BLOCK + threadIdx.x;
    if (i < n) {
        const int b = fm_bucket(f + (size_t)i * FD, two_keys);
        bucket_of[i] = b;
        atomicAdd(&h[b], 1);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < FMP_BUCKETS; b += FMP_SORT_BLOCK) if (h[b]) atomicAdd(&hist[b], h[b]);
}
__global__ void k_fm_gather_targets(const float* __restrict__ ft, const int* __restrict__ perm, int nt, int nt_pad,
                                    float* __restrict__ T, int* __restrict__ torig) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)nt_pad * FD) return;
    const int row = (int)(e / FD), d = (int)(e % FD);
    T[e] = row < nt ? ft[(size_t)perm[row] * FD + d] : INFINITY;   // padding rows: distance +inf, never chosen
    if (d == 0) torig[row] = row < nt ? perm[row] : INT_MAX;
}
__global__ void k_fm_boxes(const float* __restrict__ T, int nt, int nbox, float* __restrict__ bmin, float* __restrict__ bmax) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nbox * FD) return;
    const int b = e / FD, d = e % FD;
    float mn = INFINITY, mx = -INFINITY;
    for (int r = b * FMP_BOX; r < min(nt, (b + 1) * FMP_BOX); ++r) { float v = T[(size_t)r * FD + d]; mn = fminf(mn, v); mx = fmaxf(mx, v); }
    bmin[e] = mn; bmax[e] = mx;
}

// box visited at position v of the inside-out order centred at box c (bijection onto [0, nbox))
__device__ __forceinline__ int visit_inside_out(int v, int c, int nbox) {
    const int L = c, R = nbox - 1 - c;
    const int m = min(L, R);
    if (v <= 2 * m) { int k = (v + 1) >> 1; return (v & 1) ? c + k : c - k; }
    return R > L ? c + (v - m) : c - (v - m);
}

template <int SPL>
__global__ __launch_bounds__(FM_BLOCK)
void k_feature_match_pruned(const float* __restrict__ fs, const int* __restrict__ sperm, int ns, int ns_pad,
                            const float* __restrict__ T, const int* __restrict__ torig, int nbox,
                            const float* __restrict__ bmin, const float* __restrict__ bmax, const int* __restrict__ tstart,
                            int two_keys, int nsplit, float* __restrict__ pd, int* __restrict__ pj) {
    const int split = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wbase = (blockIdx.x * (FM_BLOCK / 64) + wave) * (64 * SPL);   // the wave's 64*SPL consecutive ordered sources
    float f[SPL][FD];
    float best[SPL]; int bj[SPL]; int src[SPL];
#pragma unroll
    for (int s = 0; s < SPL; ++s) {
        const int t = wbase + s * 64 + lane;
        const int i = sperm[min(t, ns - 1)];
        src[s] = t < ns ? i : -1;   // padding lanes duplicate the last source and write nothing
#pragma unroll
        for (int d = 0; d < FD; ++d) f[s][d] = fs[(size_t)i * FD + d];
        best[s] = INFINITY; bj[s] = INT_MAX;
    }
    // start where the targets with the wave's own key begin
    const int c = min(nbox - 1, tstart[__builtin_amdgcn_readfirstlane(fm_bucket(f[0], two_keys))] / FMP_BOX);
    for (int v = split; v < nbox; v += nsplit) {
        const int b = visit_inside_out(v, c, nbox);
        const float* __restrict__ lo = bmin + (size_t)b * FD;   // wave-uniform -> scalar loads
        const float* __restrict__ hi = bmax + (size_t)b * FD;
        float lb[SPL];
#pragma unroll
        for (int s = 0; s < SPL; ++s) lb[s] = 0.f;
#pragma unroll
        for (int d = 0; d < FD; ++d) {
            const float l = lo[d], h = hi[d];
#pragma unroll
            for (int s = 0; s < SPL; ++s) { float g = fmaxf(fmaxf(l - f[s][d], f[s][d] - h), 0.f); lb[s] += g * g; }
        }
        bool alive = false;
#pragma unroll
        for (int s = 0; s < SPL; ++s) alive = alive || (lb[s] <= best[s]);   // <=: an equal distance with a lower index still wins
        if (!__any(alive)) continue;
#pragma unroll 1
        for (int t = 0; t < FMP_BOX; ++t) {
            const int j = b * FMP_BOX + t;
            const float* __restrict__ g = T + (size_t)j * FD;
            const int o = torig[j];
            float q[FD];
#pragma unroll
            for (int d = 0; d < FD; ++d) q[d] = g[d];
#pragma unroll
            for (int s = 0; s < SPL; ++s) {
                float dist = 0.f;
#pragma unroll
                for (int d = 0; d < FD; ++d) { float diff = f[s][d] - q[d]; dist += diff * diff; }
                const bool take = dist < best[s] || (dist == best[s] && o < bj[s]);
                best[s] = take ? dist : best[s];
                bj[s] = take ? o : bj[s];
            }
        }
    }
#pragma unroll
    for (int s = 0; s < SPL; ++s) {
        if (src[s] < 0) continue;
        const size_t o = (size_t)split * ns_pad + src[s];
        pd[o] = best[s]; pj[o] = bj[s];
    }
}

// partials of the pruned match: lexicographic (distance, original index) minimum, order-independent
__global__ void k_feature_match_combine_lex(int ns, int ns_pad, int nparts, const float* __restrict__ pd,
                                            const int* __restrict__ pj, int* __restrict__ corr) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns) return;
    float best = INFINITY; int bj = INT_MAX;
    for (int s = 0; s < nparts; ++s) {
        const float d = pd[(size_t)s * ns_pad + i]; const int j = pj[(size_t)s * ns_pad + i];
        if (d < best || (d == best && j < bj)) { best = d; bj = j; }
    }
    corr[i] = bj == INT_MAX ? 0 : bj;   // nothing finite: the CPU loop keeps its initial index 0
}

// counting sort of n descriptors by key bucket: perm (ordered position -> row) and, optionally, the bucket starts
static int fm_order(tdv_ctx* ctx, const float* d_f, int n, int two_keys, int* perm, int* start /* FMP_BUCKETS + 1 */) {
    hipStream_t s = ctx->stream;
    int *hist, *cursor, *d_total, *bucket_of;
    TDV_TRY(ws_alloc(ctx, (size_t)FMP_BUCKETS, &hist));
    TDV_TRY(ws_alloc(ctx, (size_t)FMP_BUCKETS, &cursor));
    TDV_TRY(ws_alloc(ctx, 1, &d_total));
    TDV_TRY(ws_alloc(ctx, (size_t)n, &bucket_of));
    TDV_HIP(ctx, hipMemsetAsync(hist, 0, (size_t)FMP_BUCKETS * 4, s));
    TDV_HIP(ctx, hipMemsetAsync(cursor, 0, (size_t)FMP_BUCKETS * 4, s));
    const int blocks = (n + FMP_SORT_BLOCK - 1) / FMP_SORT_BLOCK;
    k_fm_hist<<<blocks, FMP_SORT_BLOCK, 0, s>>>(d_f, n, two_keys, bucket_of, hist);
    TDV_TRY(exclusive_scan_dev(ctx, hist, FMP_BUCKETS, start, d_total));
    k_fm_scatter<<<blocks, FMP_SORT_BLOCK, 0, s>>>(bucket_of, n, start, cursor, perm);
    TDV_CHECK_LAUNCH(ctx);
    return TDV_OK;
}

constexpr int FMP_SPL = 1;   // 1 measured better than 2 (C4: 0.84 vs 0.93 ms)
static int feature_match_keyorder_dev(tdv_ctx* ctx, const float* d_fs, int ns, const float* d_ft, int nt, int* d_corr) {
    hipStream_t s = ctx->stream;
    const int nt_pad = (int)align_up((size_t)nt, FMP_BOX);
    const int nbox = nt_pad / FMP_BOX;
    constexpr int SRC_PER_BLOCK = FM_BLOCK * FMP_SPL;
    const int ns_pad = (int)align_up((size_t)ns, SRC_PER_BLOCK);
    const int blocks_x = ns_pad / SRC_PER_BLOCK;
    const int nsplit = scan_splits(blocks_x, nbox, 4096, 8, 32).asked;     // (the splits take the boxes in turn: every one of them holds something)
    int *sperm, *tperm, *tstart, *sstart, *torig; float *T, *bmin, *bmax, *pd; int* pj;
    TDV_TRY(ws_alloc(ctx, (size_t)ns, &sperm));
    TDV_TRY(ws_alloc(ctx, (size_t)nt, &tperm));
    TDV_TRY(ws_alloc(ctx, (size_t)FMP_BUCKETS + 1, &tstart));
    TDV_TRY(ws_alloc(ctx, (size_t)FMP_BUCKETS + 1, &sstart));
    TDV_TRY(ws_alloc(ctx, (size_t)nt_pad, &torig));
    TDV_TRY(ws_alloc(ctx, (size_t)nt_pad * FD, &T));
    TDV_TRY(ws_alloc(ctx, (size_t)nbox * FD, &bmin));
    TDV_TRY(ws_alloc(ctx, (size_t)nbox * FD, &bmax));
    TDV_TRY(ws_alloc(ctx, (size_t)nsplit * ns_pad, &pd));
    TDV_TRY(ws_alloc(ctx, (size_t)nsplit * ns_pad, &pj));
    ScopedTimer tm(ctx, TDV_TIMER_FEATURE_MATCH);
    const int two_keys = nt <= FMP_TWO_KEYS_MAX_TARGETS ? 1 : 0;
    TDV_TRY(fm_order(ctx, d_ft, nt, two_keys, tperm, tstart));
    TDV_TRY(fm_order(ctx, d_fs, ns, two_keys, sperm, sstart));
    k_fm_gather_targets<<<(unsigned)(((size_t)nt_pad * FD + 255) / 256), 256, 0, s>>>(d_ft, tperm, nt, nt_pad, T, torig);
    k_fm_boxes<<<(nbox * FD + 255) / 256, 256, 0, s>>>(T, nt, nbox, bmin, bmax);
    k_feature_match_pruned<FMP_SPL><<<dim3(blocks_x, nsplit), FM_BLOCK, 0, s>>>(d_fs, sperm, ns, ns_pad, T, torig, nbox, bmin, bmax, tstart,
                                                                               two_keys, nsplit, pd, pj);
    k_feature_match_combine_lex<<<(ns + 255) / 256, 256, 0, s>>>(ns, ns_pad, nsplit, pd, pj, d_corr);
    TDV_CHECK_LAUNCH(ctx);
    return TDV_OK;
}

// ---- the variants of the searches in fmatch.hip ------------------------------------------------------------------------
// TDV_FM_KEYORDER (for the sizes that would use the index) and TDV_FM_NO_EARLY_EXIT (for what the plain scan would answer)
static int fm_study_match(tdv_ctx* ctx, const float* d_fs, int ns, const float* d_ft, int nt, int* d_corr, bool* answered) {
    const FmKnobs k = fm_knobs();
    *answered = true;
    if (k.keyorder && !k.brute && fm_indexes_sources(ns) && nt >= FM_INDEX_MIN_TARGETS) return feature_match_keyorder_dev(ctx, d_fs, ns, d_ft, nt, d_corr);
    if (!k.early) return fm_scan_all<false>(ctx, d_fs, ns, d_ft, nt, d_corr);
    *answered = false;
    return TDV_OK;
}
// the walk with TDV_FM_K = 1 / 2 / 4 sources per wave, with or without TDV_FM_STATS
template <int K>
static int fm_study_walk_k(FmRun& r) { return r.knobs.stats ? fm_walk<K, true>(r) : fm_walk<K, false>(r); }
static int fm_study_walk(FmRun& r) {
    const int k = r.knobs.force_k ? r.knobs.force_k : 2;
    return k >= 4 ? fm_study_walk_k<4>(r) : k < 2 ? fm_study_walk_k<1>(r) : fm_study_walk_k<2>(r);
}
int fm_walk_report(tdv_ctx* ctx, const FmTables& t, int K, const unsigned long long* d_stats, int n_b, int n_scan) {
    unsigned long long h[12];
    TDV_HIP(ctx, hipMemcpyAsync(h, d_stats, 96, hipMemcpyDeviceToHost, ctx->stream));
    TDV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    fprintf(stderr, "[tdv] fm query: %d sources x %d leaves, %d groups, %d sources per wave, %llu waves: per wave %.1f group-chunk tests, "
            "%.1f groups visited, %.1f leaves opened (max %llu); wave time mean %.1f us max %.1f us; gave up: %d waves to pass B "
            "(%llu helper waves, %.1f leaves each, max %llu), %d waves to the plain scan\n",
            t.ns, t.nleaf, t.ngroup, K, h[0], (double)h[1] / h[0], (double)h[2] / h[0], (double)h[3] / h[0], h[4],
            (double)h[5] / h[0] * 0.01, (double)h[6] * 0.01, n_b, h[8], h[8] ? (double)h[9] / h[8] : 0.0, h[10], n_scan);
    return TDV_OK;
}
// TDV_LM_ROUNDS=2, second round: every group that is no home group, with the bounds the home groups' leaves left
static void lm_study_second_round(hipStream_t s, const FmTables& t, const FmIndex& ix, const LmLists& L, int waves, unsigned long long* d_stats) {
    k_lm_boxes<2><<<waves, 64 * LM_BOX_WAVES, 0, s>>>(t, ix.sleaf, ix.sgroup, L, d_stats ? d_stats + 8 : nullptr);
}
static int lm_study_report(const FmRun& r, const LmRun& m) {
    tdv_ctx* ctx = r.ctx;
    int h[2][LM_POOLS + 1];      // a round's entry cursors, then its overflow word
    long long pairs[2] = {0, 0};
    for (int b = 0; b < 2; ++b) {
        TDV_HIP(ctx, hipMemcpy(h[b], m.z.entry_cursor(b + 1), (LM_POOLS + 1) * 4, hipMemcpyDeviceToHost));
        for (int k = 0; k < LM_POOLS; ++k) pairs[b] += h[b][k];
    }
    fprintf(stderr, "[tdv] fm leaf-major: %d sources x %d leaves in %d groups: round 1 %lld entries (%.2f per source)%s, round 2 %lld entries (%.2f per source)%s\n",
            r.ns, r.ix.nleaf, r.ix.ngroup, pairs[0], (double)pairs[0] / r.ns, h[0][LM_POOLS] ? " OVERFLOW" : "", pairs[1], (double)pairs[1] / r.ns, h[1][LM_POOLS] ? " OVERFLOW" : "");
    unsigned long long st[16];
    TDV_HIP(ctx, hipMemcpy(st, m.d_stats, 128, hipMemcpyDeviceToHost));
    for (int b = 0; b < 2; ++b) {
        const unsigned long long* q = st + 8 * b; const double w = (double)std::max(1ull, q[0]);
        fprintf(stderr, "[tdv]   boxes round %d: %llu waves, per wave %.1f us (max %.1f), %.1f us until the source is loaded, %.1f us last flush; %.1f 3-D tests, %.1f 33-D tests, %.1f boxes emitted\n",
                b + 1, q[0], q[1] / w * 0.01, q[7] * 0.01, q[2] / w * 0.01, q[3] / w * 0.01, q[4] / w, q[5] / w, q[6] / w);
    }
    return TDV_OK;
}
