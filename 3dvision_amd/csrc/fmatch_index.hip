// The packed index of a target descriptor set (layouts: fmatch_layout.hpp; the searches over it: fmatch.hip).  A unit of its own:
// a single match builds it for its targets, a batch once for the model.  The order of rows, the principal directions and the host
// eigen-solver only decide WHICH rows a search looks at first; every search is exact whatever they are.
#include "tdv_internal.hpp"
#include "fmatch_layout.hpp"
#include <climits>
#include <algorithm>
#include <vector>

namespace tdv {

// ---- packed target index -----------------------------------------------------------------------------------------
// FPFH descriptors of a surface live close to a 3-D manifold of R^33 (96 % of their variance in three principal
// directions on the relief part).  The targets are therefore packed sort-tile-recursive along those directions:
// equal-count slabs along p0, equal-count columns along p1 inside every slab, rows sorted along p2 inside every column
// (two full sorts of 16-B records and one segmented sort inside the columns; slab / column counts proportional to the spread, chosen on the host from the
// eigenvalues).  Columns are padded to a multiple of 64 rows (+inf rows that never win), so a leaf = 64 consecutive
// rows never straddles two columns; group = 64 consecutive leaves.  Offline study on real descriptors
// (tools/studies/feature_match_pca_tree.py): a wave of 64 neighbouring sources has to open 2.3 % of the leaves with
// this packing against 17.8 % with round 1's scalar key.
constexpr int FX_MAX_S = 64;          // slabs / columns per slab at most
constexpr int FX_NMOM = 561 + 33;     // upper triangle of sum f f^T, then sum f

__device__ __forceinline__ unsigned sortable_bits(float v) {   // ascending float order as ascending unsigned order; NaN last
    if (v != v) return 0xffffffffu;
    unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// raw moments of the rows, per workgroup, in double; fixed order (deterministic basis -> deterministic packing)
constexpr int FX_MOM_BLOCK = 640;
constexpr int FX_MOM_TILE = 32;
__global__ __launch_bounds__(FX_MOM_BLOCK)
void k_fm_moments(const float* __restrict__ f, int n, int rows_per_block, double* __restrict__ partial) {
    __shared__ float tile[FX_MOM_TILE][FD + 1];
    const int t = threadIdx.x;
    int a = 0, b = 0;   // thread t < 561: pair (a <= b); 561 <= t < 594: column sum
    if (t < 561) { int r = t; a = 0; while (r >= FD - a) { r -= FD - a; ++a; } b = a + r; }
    const int r0 = blockIdx.x * rows_per_block, r1 = min(n, r0 + rows_per_block);
    double acc = 0.0;
    for (int base = r0; base < r1; base += FX_MOM_TILE) {
        const int m = min(FX_MOM_TILE, r1 - base);
        for (int e = t; e < m * FD; e += FX_MOM_BLOCK) tile[e / FD][e % FD] = f[(size_t)base * FD + e];
        __syncthreads();
        if (t < 561) { for (int r = 0; r < m; ++r) acc += (double)tile[r][a] * (double)tile[r][b]; }
        else if (t < FX_NMOM) { for (int r = 0; r < m; ++r) acc += (double)tile[r][t - 561]; }
        __syncthreads();
    }
    if (t < FX_NMOM) partial[(size_t)blockIdx.x * FX_NMOM + t] = acc;
}
// one wave per moment: the workgroups' partial sums in a fixed order (lane l takes blocks l, l + 64, ...; then a fixed tree)
__global__ __launch_bounds__(64)
void k_fm_moments_fold(const double* __restrict__ partial, int nblocks, double* __restrict__ out) {
    const int t = blockIdx.x;
    double s = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 64) s += partial[(size_t)b * FX_NMOM + t];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (threadIdx.x == 0) out[t] = s;
}

__global__ void k_fm_project(const float* __restrict__ f, int n, const float* __restrict__ basis, float* __restrict__ p0,
                             float* __restrict__ p1, float* __restrict__ p2, unsigned* __restrict__ amax) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, am = 0.f;
    if (i < n) { principal_coords(f + (size_t)i * FD, basis, a0, a1, a2, am); p0[i] = a0; p1[i] = a1; p2[i] = a2; }
    __shared__ unsigned s_max;
    if (threadIdx.x == 0) s_max = 0u;
    __syncthreads();
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) am = fmaxf(am, __shfl_xor(am, off, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(&s_max, __float_as_uint(am));
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(amax, s_max);
}

// Bit-identical target rows (the descriptor of a flat patch: a quarter of the relief model's rows are two such values)
// give bit-identical distances, and the tie rule hands the match to the lowest index among them: only that row can ever
// win, so the packed index holds it alone.  Without this every source on such a plateau has to open every leaf holding
// a copy.  Two levels of open addressing keyed by a hash of the row's bits, rows always compared in full (a hash
// collision costs a probe, never a row): a workgroup first folds its own 512 rows in LDS - a popular value would
// otherwise queue tens of thousands of atomics on one L2 address - and only the lowest row of every value it holds
// goes to the global table.  After the kernel table[slot_of[i]] == i exactly for the lowest row of every distinct value.
constexpr int FX_DD_ROWS = 512;
constexpr int FX_DD_SLOTS = 1024;
__device__ __forceinline__ unsigned row_hash(const float* x) {
    unsigned h = 0x9e3779b9u;
#pragma unroll
    for (int d = 0; d < FD; ++d) { h ^= __float_as_uint(x[d]); h *= 0x85ebca6bu; h ^= h >> 13; }
    h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}
__global__ __launch_bounds__(FX_DD_ROWS)
void k_fm_dedupe_insert(const float* __restrict__ f, int n, int* table, unsigned mask, int* __restrict__ slot_of, int* __restrict__ kept) {
    __shared__ float tile[FX_DD_ROWS * FD];          // row-major, stride 33 dwords: lanes = consecutive rows hit distinct banks
    __shared__ int ltab[FX_DD_SLOTS], lres[FX_DD_SLOTS];
    __shared__ int claimed;
    const int t = threadIdx.x, base = blockIdx.x * FX_DD_ROWS, m = min(FX_DD_ROWS, n - base);
    for (int e = t; e < m * FD; e += FX_DD_ROWS) tile[e] = f[(size_t)base * FD + e];
    for (int e = t; e < FX_DD_SLOTS; e += FX_DD_ROWS) ltab[e] = -1;
    if (t == 0) claimed = 0;
    __syncthreads();
    const float* x = tile + t * FD;
    unsigned h = 0, ls = 0;
    if (t < m) {
        h = row_hash(x);
        ls = h & (FX_DD_SLOTS - 1);
        for (;;) {
            int cur = atomicCAS(&ltab[ls], -1, t);
            if (cur < 0) break;
            const float* y = tile + cur * FD;
            bool same = true;
#pragma unroll
            for (int d = 0; d < FD; ++d) same = same && (__float_as_uint(x[d]) == __float_as_uint(y[d]));
            if (same) { if (t < cur) atomicMin(&ltab[ls], t); break; }
            ls = (ls + 1) & (FX_DD_SLOTS - 1);       // half full at most: the probe ends
        }
    }
    __syncthreads();
    bool claim = false;
    if (t < m && ltab[ls] == t) {                    // lowest row of its value in this workgroup
        const int i = base + t;
        unsigned slot = h & mask;
        for (;;) {
            // plain load: a stale owner is still a row with the slot's value, a stale "empty" is corrected by the CAS
            int cur = table[slot];
            if (cur < 0) { cur = atomicCAS(&table[slot], -1, i); if (cur < 0) { claim = true; break; } }
            const float* y = f + (size_t)cur * FD;
            bool same = true;
#pragma unroll
            for (int d = 0; d < FD; ++d) same = same && (__float_as_uint(x[d]) == __float_as_uint(y[d]));
            if (same) { if (i < cur) atomicMin(&table[slot], i); break; }
            slot = (slot + 1) & mask;
        }
        lres[ls] = (int)slot;
    }
    // every distinct value claims exactly one empty slot of the global table: the claims count the rows that stay
    const unsigned long long cm = __ballot(claim);
    if ((t & 63) == 0 && cm) atomicAdd(&claimed, __popcll(cm));
    __syncthreads();
    if (t < m) slot_of[base + t] = lres[ls];
    if (t == 0 && claimed) atomicAdd(kept, claimed);
}

// first key: p0 of the rows that stay; the others sort behind every real row together with the padding
// Keys of the three sorts of the packing.  The first two are stable radix sorts of (key, row) pairs: rows enter in index order,
// so equal keys keep the lower row first.
__global__ void k_fm_key_p0(const float* __restrict__ p0, int n, const int* __restrict__ table, const int* __restrict__ slot_of,
                            unsigned long long* __restrict__ key, unsigned* __restrict__ row) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool keep = table[slot_of[i]] == i;             // a bit-identical copy of an earlier row stays out of the index: it sorts last
    key[i] = keep ? (unsigned long long)sortable_bits(p0[i]) : (1ull << 32);
    row[i] = (unsigned)i;
}
// number of entries of the ascending array `starts` (m + 1 entries, starts[0] = 0) that are <= r, minus 1
__device__ __forceinline__ int segment_of(const int* __restrict__ starts, int m, int r) {
    int lo = 0, hi = m;   // invariant: starts[lo] <= r < starts[hi]
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (starts[mid] <= r) lo = mid; else hi = mid; }
    return lo;
}
// after the sort along p0: rank -> slab (equal counts); next key = (slab, p1); slab boundary values for locating
__global__ void k_fm_key_p1(const unsigned* __restrict__ row_in, int n, const int* __restrict__ slab_start, int S0, const float* __restrict__ p0,
                            const float* __restrict__ p1, float* __restrict__ b0, unsigned long long* __restrict__ key) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const unsigned idx = row_in[r];
    const int k = segment_of(slab_start, S0, r);
    if (r == slab_start[k]) b0[k] = p0[idx];
    key[r] = ((unsigned long long)(unsigned)k << 32) | sortable_bits(p1[idx]);
}
// after the sort along (slab, p1): rank -> column; last key = (column, p2, row), as 16-byte records for the per-column sort
__global__ void k_fm_rec_p2(const unsigned* __restrict__ row_in, int n, const int* __restrict__ col_start, int ncol, const float* __restrict__ p1,
                            const float* __restrict__ p2, float* __restrict__ b1, uint4* __restrict__ rec) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const unsigned idx = row_in[r];
    const int c = segment_of(col_start, ncol, r);
    if (r == col_start[c]) b1[c] = p1[idx];
    rec[r] = make_uint4((unsigned)c, sortable_bits(p2[idx]), idx, 0u);
}
__global__ void k_fm_fill_rows(float* __restrict__ T, int* __restrict__ torig, size_t n_rows) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n_rows * FD) T[e] = INFINITY;
    if (e < n_rows) torig[e] = INT_MAX;
}
// after the sort along (column, p2, row): rows to their padded positions
__global__ void k_fm_place_rows(const uint4* __restrict__ rec, int n, const int* __restrict__ col_start, const int* __restrict__ col_row0, int ncol,
                                const float* __restrict__ ft, const float* __restrict__ p0, const float* __restrict__ p1, const float* __restrict__ p2,
                                float* __restrict__ T, int* __restrict__ torig, float* __restrict__ leaf_p2, float* __restrict__ prow /* [3][rows] */, size_t rows) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)n * FD) return;
    const int r = (int)(e / FD), d = (int)(e % FD);
    const unsigned idx = rec[r].z;
    const int c = segment_of(col_start, ncol, r);
    const size_t row = (size_t)col_row0[c] + (size_t)(r - col_start[c]);
    T[row_elem(row, d)] = ft[(size_t)idx * FD + d];
    if (d == 0) {
        torig[row] = (int)idx;
        if (row % FX_LEAF == 0) leaf_p2[row / FX_LEAF] = p2[idx];
        prow[row] = p0[idx]; prow[rows + row] = p1[idx]; prow[2 * rows + row] = p2[idx];
    }
}
// Leaf boxes over the real rows of 64 padded rows (a leaf of padding gets the empty box), and beside the 33-D box of every leaf the
// 3-D box of its rows' principal coordinates: a leaf IS a cell of the packing in those coordinates, so this box is tight where the 33-D
// box (axis-aligned, the data are not) is loose; together they open 8 leaves per source where the 33-D box alone opens 19
// (tools/studies/feature_match_tail.py).
__global__ void k_fm_leaf_boxes(const float* __restrict__ T, const int* __restrict__ torig, const float* __restrict__ prow, size_t rows,
                                int nleaf, int ngroup, float* __restrict__ lbox, float* __restrict__ pbox) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ngroup * FX_GROUP * (FD + PD)) return;
    const int b = e / (FD + PD), d = e % (FD + PD);
    float mn = INFINITY, mx = -INFINITY;
    if (b < nleaf)
        for (int r = b * FX_LEAF; r < (b + 1) * FX_LEAF; ++r) {
            if (torig[r] == INT_MAX) continue;
            const float v = d < FD ? T[row_elem((size_t)r, d)] : prow[(size_t)(d - FD) * rows + r];
            mn = fminf(mn, v); mx = fmaxf(mx, v);
        }
    if (d < FD) {
        float* gb = lbox + (size_t)(b / FX_GROUP) * (2 * FD * FX_GROUP);
        gb[d * FX_GROUP + b % FX_GROUP] = mn; gb[(FD + d) * FX_GROUP + b % FX_GROUP] = mx;
    } else {
        float* gb = pbox + (size_t)(b / FX_GROUP) * (2 * PD * FX_GROUP);
        gb[(d - FD) * FX_GROUP + b % FX_GROUP] = mn; gb[(PD + d - FD) * FX_GROUP + b % FX_GROUP] = mx;
    }
}
// group boxes, same transposed layouts one level up: gbox[chunk of 64 groups][min | max][33][64], gpbox[chunk][min | max][3][64]
__global__ void k_fm_group_boxes(const float* __restrict__ lbox, const float* __restrict__ pbox, int ngroup, int nchunk,
                                 float* __restrict__ gbox, float* __restrict__ gpbox) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nchunk * 64 * (FD + PD)) return;
    const int g = e / (FD + PD), d = e % (FD + PD);
    float mn = INFINITY, mx = -INFINITY;
    if (g < ngroup) {
        const float* gb = d < FD ? lbox + (size_t)g * (2 * FD * FX_GROUP) : pbox + (size_t)g * (2 * PD * FX_GROUP);
        const int dd = d < FD ? d : d - FD, nd = d < FD ? FD : PD;
        for (int l = 0; l < FX_GROUP; ++l) { mn = fminf(mn, gb[dd * FX_GROUP + l]); mx = fmaxf(mx, gb[(nd + dd) * FX_GROUP + l]); }
    }
    if (d < FD) {
        float* cb = gbox + (size_t)(g / 64) * (2 * FD * 64);
        cb[d * 64 + g % 64] = mn; cb[(FD + d) * 64 + g % 64] = mx;
    } else {
        float* cb = gpbox + (size_t)(g / 64) * (2 * PD * 64);
        cb[(d - FD) * 64 + g % 64] = mn; cb[(PD + d - FD) * 64 + g % 64] = mx;
    }
}

// the boxes once more as the leaf-major search stages them: one box = LM_BOX consecutive floats (fmatch_layout.hpp)
__global__ void k_lm_box_layout(const float* __restrict__ lbox, const float* __restrict__ pbox, const float* __restrict__ gbox, const float* __restrict__ gpbox,
                                int nleaf, int ngroup, float* __restrict__ sleaf, float* __restrict__ sgroup) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (nleaf + ngroup) * LM_BOX) return;
    const int b = e / LM_BOX, f = e % LM_BOX;
    if (b < nleaf) {
        const int g = b / FX_GROUP, l = b % FX_GROUP;
        sleaf[e] = f < 2 * FD ? lbox[(size_t)g * (2 * FD * FX_GROUP) + f * FX_GROUP + l] : pbox[(size_t)g * (2 * PD * FX_GROUP) + (f - 2 * FD) * FX_GROUP + l];
    } else {
        const int gi = b - nleaf, c = gi / 64, k = gi % 64;
        sgroup[(size_t)gi * LM_BOX + f] = f < 2 * FD ? gbox[(size_t)c * (2 * FD * 64) + f * 64 + k] : gpbox[(size_t)c * (2 * PD * 64) + (f - 2 * FD) * 64 + k];
    }
}

namespace {

// cyclic Jacobi eigen-solver for a symmetric n x n matrix (host, double): eigenvalues descending, eigenvectors in rows
void jacobi_eigen_host(std::vector<double>& A, int n, std::vector<double>& evals, std::vector<double>& evecs) {
    std::vector<double> V((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) V[(size_t)i * n + i] = 1.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < n; ++p) for (int q = p + 1; q < n; ++q) off += A[(size_t)p * n + q] * A[(size_t)p * n + q];
        if (!(off > 1e-30)) break;
        for (int p = 0; p < n; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[(size_t)p * n + q];
                if (std::fabs(apq) < 1e-300) continue;
                const double theta = (A[(size_t)q * n + q] - A[(size_t)p * n + p]) / (2.0 * apq);
                const double tt = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(tt * tt + 1.0), s = tt * c;
                for (int k = 0; k < n; ++k) {
                    const double akp = A[(size_t)k * n + p], akq = A[(size_t)k * n + q];
                    A[(size_t)k * n + p] = c * akp - s * akq; A[(size_t)k * n + q] = s * akp + c * akq;
                }
                for (int k = 0; k < n; ++k) {
                    const double apk = A[(size_t)p * n + k], aqk = A[(size_t)q * n + k];
                    A[(size_t)p * n + k] = c * apk - s * aqk; A[(size_t)q * n + k] = s * apk + c * aqk;
                }
                for (int k = 0; k < n; ++k) {
                    const double vkp = V[(size_t)k * n + p], vkq = V[(size_t)k * n + q];
                    V[(size_t)k * n + p] = c * vkp - s * vkq; V[(size_t)k * n + q] = s * vkp + c * vkq;
                }
            }
    }
    std::vector<int> order(n);
    for (int i = 0; i < n; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return A[(size_t)a * n + a] > A[(size_t)b * n + b]; });
    evals.resize(n); evecs.assign((size_t)n * n, 0.0);
    for (int r = 0; r < n; ++r) {
        evals[r] = A[(size_t)order[r] * n + order[r]];
        for (int k = 0; k < n; ++k) evecs[(size_t)r * n + k] = V[(size_t)k * n + order[r]];
    }
}

// The build's pinned staging, one reservation: what comes down before the host step (the raw moments, the number of distinct
// rows) and what goes up after it (the basis; the cut tables slab_start | col_start | col_row0 | col_leaf0).  The host fills the
// upward part in place; the call ends with a synchronisation, so later calls may reuse the bytes.
constexpr size_t fx_cut_words(int S0, int S1) { return ((size_t)S0 + 1) + 3 * ((size_t)S0 * S1 + 1); }
constexpr size_t FX_PIN_BYTES = 64 * 1024;
struct FxStaging {
    double mom[FX_NMOM];
    int kept;
    float basis[4 * FD];
    int cuts[fx_cut_words(FX_MAX_S, FX_MAX_S)];
};
static_assert(sizeof(FxStaging) <= FX_PIN_BYTES, "the largest packing (S0 = S1 = FX_MAX_S) must fit the pinned reservation");

}  // namespace

int fm_index_build(tdv_ctx* ctx, const float* d_ft, int nt, FmIndex* ix) {
    if (!ctx || !d_ft || !ix || nt <= 0) return TDV_ERR_BAD_ARG;
    hipStream_t s = ctx->stream;
    ScopedTimer tm(ctx, TDV_TIMER_FM_INDEX);
    // 1. principal directions of the targets: raw moments on the device, 33 x 33 eigen-problem on the host
    const int mblocks = std::max(1, std::min(512, (nt + 255) / 256));
    const int rows_per_block = (nt + mblocks - 1) / mblocks;
    double *partial, *mom;
    TDV_TRY(ws_alloc(ctx, (size_t)mblocks * FX_NMOM, &partial));
    TDV_TRY(ws_alloc(ctx, (size_t)FX_NMOM, &mom));
    k_fm_moments<<<mblocks, FX_MOM_BLOCK, 0, s>>>(d_ft, nt, rows_per_block, partial);
    k_fm_moments_fold<<<FX_NMOM, 64, 0, s>>>(partial, mblocks, mom);
    // ... and, for the same round trip, which rows are copies of an earlier row (k_fm_dedupe_insert)
    const size_t table_size = sort_pow2((size_t)nt) * 2;
    int *table, *slot_of, *d_kept;
    TDV_TRY(ws_alloc(ctx, table_size, &table));
    TDV_TRY(ws_alloc(ctx, (size_t)nt, &slot_of));
    TDV_TRY(ws_alloc(ctx, 1, &d_kept));
    TDV_HIP(ctx, hipMemsetAsync(table, 0xff, table_size * 4, s));
    TDV_HIP(ctx, hipMemsetAsync(d_kept, 0, 4, s));
    k_fm_dedupe_insert<<<(unsigned)((nt + FX_DD_ROWS - 1) / FX_DD_ROWS), FX_DD_ROWS, 0, s>>>(d_ft, nt, table, (unsigned)(table_size - 1), slot_of, d_kept);
    TDV_CHECK_LAUNCH(ctx);
    TDV_TRY(pin_reserve(ctx, FX_PIN_BYTES));
    FxStaging* stage = reinterpret_cast<FxStaging*>(ctx->pin);
    const double* h_mom = stage->mom;
    TDV_HIP(ctx, hipMemcpyAsync(stage->mom, mom, sizeof(stage->mom), hipMemcpyDeviceToHost, s));
    TDV_HIP(ctx, hipMemcpyAsync(&stage->kept, d_kept, 4, hipMemcpyDeviceToHost, s));
    TDV_HIP(ctx, hipStreamSynchronize(s));
    const int nk = stage->kept;   // distinct rows: what the index packs
    if (nk <= 0 || nk > nt) return TDV_ERR_INTERNAL;
    std::vector<double> C((size_t)FD * FD), mean(FD), evals, evecs;
    bool finite = true;
    for (int d = 0; d < FD; ++d) { mean[d] = h_mom[561 + d] / nt; finite = finite && std::isfinite(mean[d]); }
    for (int a = 0, e = 0; a < FD; ++a)
        for (int b = a; b < FD; ++b, ++e) {
            const double c = h_mom[e] / nt - mean[a] * mean[b];
            finite = finite && std::isfinite(c);
            C[(size_t)a * FD + b] = C[(size_t)b * FD + a] = c;
        }
    float* h_basis = stage->basis;
    double e0 = 1, e1 = 1, e2 = 1;
    if (finite) {
        jacobi_eigen_host(C, FD, evals, evecs);
        for (int r = 0; r < 3; ++r) for (int d = 0; d < FD; ++d) h_basis[r * FD + d] = (float)evecs[(size_t)r * FD + d];
        for (int d = 0; d < FD; ++d) h_basis[3 * FD + d] = (float)mean[d];
        e0 = std::sqrt(std::max(evals[0], 0.0)); e1 = std::sqrt(std::max(evals[1], 0.0)); e2 = std::sqrt(std::max(evals[2], 0.0));
    } else {   // non-finite descriptors: any directions will do (the order only affects speed)
        for (int r = 0; r < 3; ++r) for (int d = 0; d < FD; ++d) h_basis[r * FD + d] = (d % 3 == r) ? 1.f : 0.f;
        for (int d = 0; d < FD; ++d) h_basis[3 * FD + d] = 0.f;
    }
    // how far the f32 directions are from orthonormal decides whether their boxes may be used (fmatch.hip: principal_bound_note)
    {
        double dev = 0.0;
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) {
                double g = 0.0;
                for (int d = 0; d < FD; ++d) g += (double)h_basis[a * FD + d] * (double)h_basis[b * FD + d];
                dev += (g - (a == b ? 1.0 : 0.0)) * (g - (a == b ? 1.0 : 0.0));
            }
        ix->pscale = (std::sqrt(dev) <= 1e-6) ? (1.0f - 1e-4f) : 0.0f;
    }
    // 2. slab / column counts: S0 * S1 * S2 = number of leaves with S_d proportional to the spread along p_d
    const double nleaf_t = std::max(1.0, (double)nk / FX_LEAF);
    const double tiny = 1e-6 * std::max(e0, 1e-30);
    e0 = std::max(e0, tiny); e1 = std::max(e1, tiny); e2 = std::max(e2, tiny);
    double g = std::cbrt(nleaf_t / (e0 * e1 * e2));
    double s0 = e0 * g, s1 = e1 * g, s2 = e2 * g;
    if (s2 < 1.0) { const double k = std::sqrt(s2); s0 *= k; s1 *= k; s2 = 1.0; }
    if (s1 < 1.0) { s0 *= s1; s1 = 1.0; }
    const int S0 = std::max(1, std::min(FX_MAX_S, (int)std::lround(s0)));
    const int S1 = std::max(1, std::min(FX_MAX_S, (int)std::lround(s1)));
    const int ncol = S0 * S1;
    // equal-count cuts by rank are known without looking at the data
    const size_t n_cuts = fx_cut_words(S0, S1);
    int* slab_start = stage->cuts; int* col_start = slab_start + S0 + 1; int* col_row0 = col_start + ncol + 1; int* col_leaf0 = col_row0 + ncol + 1;
    for (int k = 0; k <= S0; ++k) slab_start[k] = (int)((long long)nk * k / S0);
    for (int k = 0; k < S0; ++k) {
        const int c0 = slab_start[k], cnt = slab_start[k + 1] - c0;
        for (int j = 0; j < S1; ++j) col_start[k * S1 + j] = c0 + (int)((long long)cnt * j / S1);
    }
    col_start[ncol] = nk;
    size_t rows = 0;
    for (int c = 0; c < ncol; ++c) {
        col_row0[c] = (int)rows; col_leaf0[c] = (int)(rows / FX_LEAF);
        rows += align_up((size_t)(col_start[c + 1] - col_start[c]), FX_LEAF);
    }
    col_row0[ncol] = (int)rows; col_leaf0[ncol] = (int)(rows / FX_LEAF);
    if (rows == 0) rows = FX_LEAF;
    const int nleaf = (int)(rows / FX_LEAF), ngroup = (nleaf + FX_GROUP - 1) / FX_GROUP;
    // 3. device side
    float *basis, *p0, *p1, *p2; int* d_int; uint4* rec;
    size_t n_pow2 = sort_pow2((size_t)nt);
    TDV_TRY(ws_alloc(ctx, (size_t)4 * FD, &basis));
    TDV_TRY(ws_alloc(ctx, n_cuts, &d_int));
    TDV_TRY(ws_alloc(ctx, (size_t)S0 + 1, &ix->b0));
    TDV_TRY(ws_alloc(ctx, (size_t)ncol + 1, &ix->b1));
    TDV_TRY(ws_alloc(ctx, (size_t)nleaf, &ix->leaf_p2));
    TDV_TRY(ws_alloc(ctx, rows * FD, &ix->T));
    TDV_TRY(ws_alloc(ctx, rows, &ix->torig));
    const int nchunk = (ngroup + 63) / 64;
    TDV_TRY(ws_alloc(ctx, (size_t)ngroup * 2 * FD * FX_GROUP, &ix->lbox));
    TDV_TRY(ws_alloc(ctx, (size_t)nchunk * 2 * FD * 64, &ix->gbox));
    TDV_TRY(ws_alloc(ctx, (size_t)ngroup * 2 * PD * FX_GROUP, &ix->pbox));
    TDV_TRY(ws_alloc(ctx, (size_t)nchunk * 2 * PD * 64, &ix->gpbox));
    TDV_TRY(ws_alloc(ctx, 1, &ix->amax));
    TDV_TRY(ws_alloc(ctx, (size_t)nleaf * LM_BOX, &ix->sleaf));
    TDV_TRY(ws_alloc(ctx, (size_t)ngroup * LM_BOX, &ix->sgroup));
    const WsMark scratch = ws_mark(ctx);   // everything below is build scratch
    TDV_TRY(ws_alloc(ctx, (size_t)nt, &p0));
    TDV_TRY(ws_alloc(ctx, (size_t)nt, &p1));
    TDV_TRY(ws_alloc(ctx, (size_t)nt, &p2));
    TDV_TRY(ws_alloc(ctx, n_pow2, &rec));
    unsigned long long *key_a, *key_b; unsigned *row_a, *row_b;
    TDV_TRY(ws_alloc(ctx, (size_t)nt, &key_a));
    TDV_TRY(ws_alloc(ctx, (size_t)nt, &key_b));
    TDV_TRY(ws_alloc(ctx, (size_t)nt, &row_a));
    TDV_TRY(ws_alloc(ctx, (size_t)nt, &row_b));
    float* prow;
    TDV_TRY(ws_alloc(ctx, rows * PD, &prow));
    TDV_HIP(ctx, hipMemcpyAsync(basis, stage->basis, sizeof(stage->basis), hipMemcpyHostToDevice, s));
    TDV_HIP(ctx, hipMemcpyAsync(d_int, stage->cuts, n_cuts * 4, hipMemcpyHostToDevice, s));
    const int* d_slab_start = d_int; const int* d_col_start = d_int + S0 + 1; const int* d_col_row0 = d_col_start + ncol + 1;
    ix->col_leaf0 = d_col_row0 + ncol + 1;
    ix->ft = d_ft; ix->basis = basis; ix->nt = nt; ix->rows = (int)rows; ix->nleaf = nleaf; ix->ngroup = ngroup; ix->S0 = S0; ix->S1 = S1;
    TDV_HIP(ctx, hipMemsetAsync(ix->leaf_p2, 0, (size_t)nleaf * 4, s));
    TDV_HIP(ctx, hipMemsetAsync(ix->b0, 0, ((size_t)S0 + 1) * 4, s));
    TDV_HIP(ctx, hipMemsetAsync(ix->b1, 0, ((size_t)ncol + 1) * 4, s));
    const unsigned gn = (unsigned)((nt + 255) / 256);
    TDV_HIP(ctx, hipMemsetAsync(ix->amax, 0, 4, s));
    k_fm_project<<<gn, 256, 0, s>>>(d_ft, nt, basis, p0, p1, p2, ix->amax);
    // slabs along p0, columns along p1: two stable radix sorts of (key, row) pairs (csrc/sort.hip; two bitonic sorts of 16-byte records,
    // ~30 launches and 0.19 ms each at 150k rows, until the end of round 2)
    k_fm_key_p0<<<gn, 256, 0, s>>>(p0, nt, table, slot_of, key_a, row_a);
    TDV_TRY(radix_sort_pairs_dev(ctx, key_a, key_b, row_a, row_b, (size_t)nt, 33));   // the distinct rows lead; the copies follow
    k_fm_key_p1<<<gn, 256, 0, s>>>(row_b, nk, d_slab_start, S0, p0, p1, ix->b0, key_a);
    int slab_bits = 1;
    while ((1 << slab_bits) < S0) ++slab_bits;
    TDV_TRY(radix_sort_pairs_dev(ctx, key_a, key_b, row_b, row_a, (size_t)nk, 32 + slab_bits));
    k_fm_rec_p2<<<gn, 256, 0, s>>>(row_a, nk, d_col_start, ncol, p1, p2, ix->b1, rec);
    // the third key only orders the rows INSIDE their column: columns of up to 2,048 rows are sorted by one workgroup each,
    // all in one launch, instead of a third full sort
    int max_col = 0;
    for (int c = 0; c < ncol; ++c) max_col = std::max(max_col, col_start[c + 1] - col_start[c]);
    if (max_col <= segment_sort_max_len()) TDV_TRY(segment_sort_records_dev(ctx, rec, d_col_start, ncol));
    else {
        const size_t nk_pow2 = sort_pow2((size_t)nk);
        if (nk_pow2 > (size_t)nk) TDV_HIP(ctx, hipMemsetAsync(rec + nk, 0xff, (nk_pow2 - (size_t)nk) * sizeof(uint4), s));   // padding sorts last
        TDV_TRY(sort_records_dev(ctx, rec, nk_pow2));
    }
    k_fm_fill_rows<<<(unsigned)((rows * FD + 255) / 256), 256, 0, s>>>(ix->T, ix->torig, rows);
    k_fm_place_rows<<<(unsigned)(((size_t)nk * FD + 255) / 256), 256, 0, s>>>(rec, nk, d_col_start, d_col_row0, ncol, d_ft, p0, p1, p2, ix->T, ix->torig, ix->leaf_p2, prow, rows);
    k_fm_leaf_boxes<<<(ngroup * FX_GROUP * (FD + PD) + 255) / 256, 256, 0, s>>>(ix->T, ix->torig, prow, rows, nleaf, ngroup, ix->lbox, ix->pbox);
    k_fm_group_boxes<<<(nchunk * 64 * (FD + PD) + 255) / 256, 256, 0, s>>>(ix->lbox, ix->pbox, ngroup, nchunk, ix->gbox, ix->gpbox);
    k_lm_box_layout<<<((nleaf + ngroup) * LM_BOX + 255) / 256, 256, 0, s>>>(ix->lbox, ix->pbox, ix->gbox, ix->gpbox, nleaf, ngroup, ix->sleaf, ix->sgroup);
    TDV_CHECK_LAUNCH(ctx);
    TDV_HIP(ctx, hipStreamSynchronize(s));   // the pinned staging is reused by later calls; the scratch is released here
    ws_rewind(ctx, scratch);
    return TDV_OK;
}

}  // namespace tdv
