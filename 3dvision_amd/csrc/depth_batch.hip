// All instances of a frame in one pass (rules: depth_rules.hpp; the scalar kernels: depth_scalar.hpp).
// B masks (stacked u8 images, or one label image with label = b + 1) of ONE depth/colour frame -> B clouds stored
// back to back, each in row-major pixel order.  Grid = (pixel blocks, instances); the depth image is re-read from
// L2 / Infinity Cache by every instance, the masks and the output stream through HBM once.
#include "depth_scalar.hpp"
#include <cfloat>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

namespace tdv {

// ---- vectorised path (frame size a multiple of 16 pixels, 16-B aligned pointers): the masks cross HBM ONCE ----------
// Pass 1 (k_depth_bits): a wave owns 1,024 consecutive pixels (16 per lane).  It loads their depth once per frame, then
// walks DB_GROUP instances: one 16-B mask load per lane and instance -> 16 validity bits per lane, stored as a bitmap
// (2 B per lane, 1/8 of the mask's size) and counted per (instance, tile).  All DB_GROUP mask loads are issued before
// the first is used.  Pass 2 (k_depth_emit_bits) reads the bitmap instead of the masks, skips tiles without a valid
// pixel before touching anything else, recomputes depth only there, compacts through LDS and writes the cloud with
// coalesced stores.  HBM bytes for B stacked masks of one W x H frame with n valid pixels in total:
//   B W H (masks, once) + 2 B W H / 8 (bitmap out and in) + 12 n (points)        [round 1: 2 B W H + 12 n]
constexpr int DB_PX = 16;
constexpr int DB_TILE = 64 * DB_PX;       // pixels per wave
#ifndef DB_GROUP_VALUE
#define DB_GROUP_VALUE 8
#endif
constexpr int DB_GROUP = DB_GROUP_VALUE;  // instances per wave in pass 1 (8: the LDS transpose of the bitmap words assumes it)
static_assert(DB_GROUP == 8, "k_depth_bits stores 8 instances x 64 words as 64 x 16 B");

// mask_keeps (depth_rules.hpp) on four mask bytes at once (one dword, no per-byte extraction: the byte-by-byte form made pass 1
// VALU-bound at twice its memory time).  y = w, or w ^ label in every byte for the label rule; low 7 bits + `add` carry
// into bit 7 exactly when the byte exceeds the threshold (thresholds < 128; bytes >= 128 have bit 7 set themselves);
// the label rule is the exact zero-byte test of y, i.e. the complement.  Then the four bit-7 flags move to bits 0..3.
struct MaskRule { unsigned xor4, add4, inv, and4; };
__device__ __forceinline__ MaskRule mask_rule(int mode) {
    if (mode == TDV_MASK_THRESHOLD10) return {0u, (127u - 10u) * 0x01010101u, 0u, 0x80808080u};   // m > 10   (pipeline.cpp:51)
    if (mode == TDV_MASK_NONZERO) return {0u, 127u * 0x01010101u, 0u, 0x80808080u};             // m != 0   (depth_processing.cu:22)
    const int label = mode - TDV_MASK_LABEL_BASE;                                        // m == label
    if (label < 0 || label > 255) return {0u, 0u, 0u, 0u};                              // no byte can equal it: keeps nothing
    return {(unsigned)label * 0x01010101u, 127u * 0x01010101u, 0xffffffffu, 0x80808080u};
}
__device__ __forceinline__ unsigned keep_nibble(unsigned w, const MaskRule r) {
    const unsigned y = w ^ r.xor4;
    const unsigned f = (((((y & 0x7f7f7f7fu) + r.add4) | y) ^ r.inv) & r.and4) >> 7;   // flags at bits 0, 8, 16, 24
    return (f | (f >> 7) | (f >> 14) | (f >> 21)) & 0xfu;
}
__device__ __forceinline__ unsigned keep_bits16(const uint4 mv, const MaskRule r) {
    return keep_nibble(mv.x, r) | (keep_nibble(mv.y, r) << 4) | (keep_nibble(mv.z, r) << 8) | (keep_nibble(mv.w, r) << 12);
}

// z_valid(scaled_depth(raw)) (depth_rules.hpp; pipeline.cpp:47,71), `0 < z <= zmax` with z = (float)raw * inv_scale, is a test on the raw value itself: the product is
// monotone in raw, so the raw values that pass form one range [raw_lo, raw_hi], found on the host with the same float
// expression (depth_valid_range).  Sixteen pixels: the sign of (raw - lo) | (hi - raw) is shifted into the result, last
// pixel first.
__device__ __forceinline__ unsigned range_bits16(const uint4 r0, const uint4 r1, int lo, int hi) {
    const unsigned rw[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
    unsigned inv = 0u;
#pragma unroll
    for (int k = DB_PX - 1; k >= 0; --k) {
        const int a = (int)((rw[k >> 1] >> (16 * (k & 1))) & 0xffffu);
        inv = __builtin_amdgcn_alignbit(inv, (unsigned)((a - lo) | (hi - a)), 31);   // inv = inv << 1 | sign
    }
    return ~inv & 0xffffu;
}

// STACKED: one u8 mask per instance (else one label image, label = instance + 1).  PER_FRAME: instances read their own
// depth frame (frame_of), else all read frame 0 and its validity bits are computed once per wave.  The control flow is
// uniform: a ragged last group repeats its last instance and only skips the stores.
template <bool STACKED, bool PER_FRAME>
__global__ __launch_bounds__(DP_BLOCK)
void k_depth_bits(const uint16_t* __restrict__ raw0, const int* __restrict__ frame_of, const uint8_t* __restrict__ masks, size_t n, int n_inst,
                  int raw_lo, int raw_hi, int mask_mode, int ntiles, uint16_t* __restrict__ bits, int* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int tile = blockIdx.x * (DP_BLOCK / 64) + (threadIdx.x >> 6);
    if (tile >= ntiles) return;
    const size_t i0 = (size_t)tile * DB_TILE + (size_t)lane * DB_PX;
    const bool inside = i0 < n;                       // n is a multiple of 16: a lane is in or out as a whole
    const size_t il = inside ? i0 : 0;                // lanes past the end load pixel 0 and drop the result
    const int b0 = blockIdx.y * DB_GROUP, nb = min(DB_GROUP, n_inst - b0);
    uint4 mv[STACKED ? DB_GROUP : 1];
    if (STACKED) {
#pragma unroll
        for (int u = 0; u < DB_GROUP; ++u)            // all mask loads of the group in flight at once
            mv[u] = *reinterpret_cast<const uint4*>(masks + (size_t)(b0 + min(u, nb - 1)) * n + il);
    } else {
        mv[0] = *reinterpret_cast<const uint4*>(masks + il);
    }
    unsigned dvalid = 0u;
    if (!PER_FRAME) {
        const uint4 r0 = *reinterpret_cast<const uint4*>(raw0 + il), r1 = *reinterpret_cast<const uint4*>(raw0 + il + 8);
        dvalid = inside ? range_bits16(r0, r1, raw_lo, raw_hi) : 0u;
    }
    // The 16 validity bits of a lane are 2 bytes: stored lane by lane they would leave as 2-byte stores, the slowest shape
    // there is (per byte an order of magnitude above 16-B stores).  The wave therefore transposes its DB_GROUP x 64 words
    // through 1 KB of LDS and every lane stores 16 B: eight lanes cover one instance's 128-B row segment.
    __shared__ __attribute__((aligned(16))) uint16_t xpose[DP_BLOCK / 64][DB_GROUP][64];
    const int wave = threadIdx.x >> 6;
    const MaskRule stacked_rule = mask_rule(mask_mode);
#pragma unroll
    for (int u = 0; u < DB_GROUP; ++u) {
        const int b = b0 + min(u, nb - 1);
        if (PER_FRAME) {
            const uint16_t* __restrict__ raw = raw0 + (size_t)frame_of[b] * n + il;
            const uint4 r0 = *reinterpret_cast<const uint4*>(raw), r1 = *reinterpret_cast<const uint4*>(raw + 8);
            dvalid = inside ? range_bits16(r0, r1, raw_lo, raw_hi) : 0u;
        }
        // An instance's mask is zero over most of the frame, and a zero byte passes none of the rules (labels start at 1):
        // a wave whose 1 KB of mask is all zero - most waves - skips the bit arithmetic, which otherwise costs this
        // pass more than its memory traffic.
        const uint4 m = mv[STACKED ? u : 0];
        unsigned v = 0u; int c = 0;
        if (__any((m.x | m.y | m.z | m.w) != 0u)) {       // wave-uniform
            const MaskRule r = STACKED ? stacked_rule : mask_rule(TDV_MASK_LABEL_BASE + b + 1);
            v = keep_bits16(m, r) & dvalid;
            c = wave_sum_i32(__popc(v));
        }
        if (lane == 0 && u < nb) counts[(size_t)b * ntiles + tile] = c;
        xpose[wave][u][lane] = (uint16_t)v;
    }
    __builtin_amdgcn_wave_barrier();                       // a wave reads back only what it wrote itself
    const size_t words = n / DB_PX;                        // bitmap words per instance
    const int u2 = lane >> 3, seg = lane & 7;              // this lane stores words [seg*8, seg*8+8) of instance b0 + u2
    const size_t w0 = (size_t)tile * 64 + (size_t)seg * 8;
    if (u2 < nb && w0 < words) {
        uint16_t* dst = bits + (size_t)(b0 + u2) * words + w0;
        if (w0 + 8 <= words && (words % 8) == 0) *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(&xpose[wave][u2][seg * 8]);
        else for (int k = 0; k < 8 && w0 + k < words; ++k) dst[k] = xpose[wave][u2][seg * 8 + k];
    }
}

#ifndef DE_BLOCK_VALUE
#define DE_BLOCK_VALUE 256
#endif
constexpr int DE_BLOCK = DE_BLOCK_VALUE;
// Pass 2.  A wave owns the same 1,024 pixels as in pass 1 but walks them in 16 rounds of 64 CONSECUTIVE pixels (lane =
// pixel): the valid pixels of a round are consecutive points of the output, so a lane's slot is the round's base plus the
// number of valid lanes below it (one s_bcnt / v_mbcnt on the round's 64-bit mask) — no per-lane prefix sums, no
// compaction buffer, stores of neighbouring lanes are neighbours in memory.  (The first version let every lane own 16
// consecutive pixels and compacted through LDS: its 48 ds_write_b32 per lane hit 4 of the 64 banks — lane stride 48 dwords
// — and the pass ran at 3.8 TB/s.)  The round masks come from the bitmap words the lanes hold (4 v_readlane per round);
// the tile's raw depths are staged once in 2 KB of LDS so that a round reads them lane = pixel.
// UniformDiv: emit_point's two divisions (depth_rules.hpp) as a / d for a wave-uniform d, with the instructions the compiler emits for `a / d` (v_div_scale, v_rcp, two Newton steps on
// the reciprocal, three on the quotient, v_div_fmas, v_div_fixup) minus what does not depend on a - the reciprocal and its
// refinement, hoisted out of the loop - and minus the scaling, which is the identity (scale 1, VCC = 0) whenever d is
// normal, 1/d is normal, |a| >= 2^-102, the exponents of a and d differ by less than 96 and a / d is normal
// (V_DIV_SCALE_F32 in the CDNA ISA).  emit_fast_div_ok checks on the host that the call's camera parameters keep every
// pixel inside those conditions; otherwise the kernel divides the plain way.  Same quotient bit for bit: 6 instructions
// instead of 11 per division, and the pass is bound by instruction issue.
__device__ __forceinline__ float refined_rcp(float d) {
    const float r0 = __builtin_amdgcn_rcpf(d);
    return fmaf(fmaf(-d, r0, 1.0f), r0, r0);
}
__device__ __forceinline__ float div_by_uniform(float a, float d, float r) {
    const float q0 = a * r;
    const float q1 = fmaf(fmaf(-d, q0, a), r, q0);
    const float q2 = fmaf(fmaf(-d, q1, a), r, q1);
    return __builtin_amdgcn_div_fixupf(q2, d, a);
}
struct UniformDiv {
    float fx, fy, rfx, rfy;
    __device__ __forceinline__ UniformDiv(float fx_, float fy_) : fx(fx_), fy(fy_), rfx(refined_rcp(fx_)), rfy(refined_rcp(fy_)) {}
    __device__ __forceinline__ float by_fx(float a) const { return div_by_uniform(a, fx, rfx); }
    __device__ __forceinline__ float by_fy(float a) const { return div_by_uniform(a, fy, rfy); }
};
#ifndef DE_TPW_VALUE
#define DE_TPW_VALUE 4
#endif
constexpr int DE_TPW = DE_TPW_VALUE;   // tiles per wave
// Four of five tiles of an instance hold no valid pixel.  With one tile per wave the pass was bound by the rate at which
// workgroups can be launched (151k waves, most of them gone after one load; 19 % of the wave slots occupied — SQ counters
// in profiles/r2): a wave therefore takes DE_TPW tiles, strided by the number of waves of its instance so that every wave
// gets its share of the contiguous band of occupied tiles, and loads all their bitmap words before it looks at the first.
// ROWS (pixel count a multiple of 1,024: whole tiles only): the 64-bit validity mask of round j IS the j-th 8-byte word of
// the tile's 128-byte row of the bitmap, at a wave-uniform address — the wave reads the 16 masks of a tile with two
// scalar loads instead of assembling each from four v_readlane (the SQ counters showed 755 scalar next to 840 vector
// instructions per wave, most of them this assembling).
template <bool FAST_DIV, bool ROWS>
__global__ __launch_bounds__(DE_BLOCK)
void k_depth_emit_bits(const uint16_t* __restrict__ raw0, const int* __restrict__ frame_of, const uint8_t* __restrict__ bgr0, const uint16_t* __restrict__ bits,
                       int width, size_t n, float inv_scale, float fx, float fy, float cx, float cy, int ntiles,
                       const int* __restrict__ offsets, float* __restrict__ xyz, float* __restrict__ rgb) {
    __shared__ __attribute__((aligned(16))) uint16_t zraw[DE_BLOCK / 64][DB_TILE];
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int first = __builtin_amdgcn_readfirstlane(blockIdx.x * (DE_BLOCK / 64) + wave), stride = gridDim.x * (DE_BLOCK / 64);   // wave-uniform, and known as such
    const size_t frame = frame_of ? (size_t)frame_of[b] : 0;
    const uint16_t* __restrict__ raw = raw0 + frame * n;
    const uint8_t* __restrict__ bgr = (rgb && bgr0) ? bgr0 + frame * n * 3 : nullptr;
    const unsigned bit_lo = lane < 32 ? 1u << lane : 0u, bit_hi = lane < 32 ? 0u : 1u << (lane - 32);
    const typename std::conditional<FAST_DIV, UniformDiv, PlainDiv>::type div{fx, fy};
    unsigned words[DE_TPW];                                           // validity of pixels i0 .. i0 + 15 of each of the wave's tiles
#pragma unroll
    for (int k = 0; k < DE_TPW; ++k) {
        const int tile = first + k * stride;
        const size_t i0 = (size_t)tile * DB_TILE + (size_t)lane * DB_PX;
        words[k] = (tile < ntiles && i0 < n) ? (unsigned)bits[(size_t)b * (n / DB_PX) + i0 / DB_PX] : 0u;
    }
#pragma unroll
    for (int k = 0; k < DE_TPW; ++k) {
        const unsigned word = words[k];
        if (!__any(word != 0u)) continue;                             // most tiles of an instance: nothing else is read
        const int tile = first + k * stride;
        const size_t t0 = (size_t)tile * DB_TILE;                     // first pixel of the tile
        const size_t i0 = t0 + (size_t)lane * DB_PX;
        __builtin_amdgcn_wave_barrier();                              // the previous tile's rounds are done with zraw
        if (i0 < n) {                                                 // n is a multiple of 16: 32 B per lane, whole or not at all
            *reinterpret_cast<uint4*>(&zraw[wave][lane * DB_PX]) = *reinterpret_cast<const uint4*>(raw + i0);
            *reinterpret_cast<uint4*>(&zraw[wave][lane * DB_PX + 8]) = *reinterpret_cast<const uint4*>(raw + i0 + 8);
        }
        __builtin_amdgcn_wave_barrier();                              // a wave reads back only what it staged itself
        const size_t slot0 = (size_t)offsets[(size_t)b * ntiles + tile];    // output slot of the tile's first valid pixel
        float* __restrict__ tile_xyz = xyz + 3 * slot0;
        float* __restrict__ tile_rgb = bgr ? rgb + 3 * slot0 : nullptr;
        unsigned run = 0u;                                            // valid pixels of the tile's earlier rounds (32-bit offsets from here on)
        // (column, row) of this lane's pixel, advanced by 64 pixels per round: a division per pixel would be a third of
        // the loop's instructions
        unsigned row = (unsigned)(t0 / (size_t)width);
        unsigned col = (unsigned)(t0 - (size_t)row * (size_t)width) + (unsigned)lane;
        while (col >= (unsigned)width) { col -= (unsigned)width; ++row; }
        unsigned long long mrow[ROWS ? DB_PX : 1];
        if (ROWS) {
            const unsigned long long* __restrict__ mp = reinterpret_cast<const unsigned long long*>(bits + (size_t)b * (n / DB_PX)) + (size_t)tile * DB_PX;   // wave-uniform: scalar loads
#pragma unroll
            for (int j = 0; j < DB_PX; ++j) mrow[j] = mp[j];
        }
#pragma unroll ROWS ? DB_PX : 1
        for (int j = 0; j < DB_PX; ++j) {                             // round j: pixels t0 + 64 j .. + 63
            unsigned m_lo, m_hi;
            if (ROWS) { m_lo = (unsigned)mrow[ROWS ? j : 0]; m_hi = (unsigned)(mrow[ROWS ? j : 0] >> 32); }
            else {
                m_lo = (unsigned)__builtin_amdgcn_readlane((int)word, 4 * j) | ((unsigned)__builtin_amdgcn_readlane((int)word, 4 * j + 1) << 16);
                m_hi = (unsigned)__builtin_amdgcn_readlane((int)word, 4 * j + 2) | ((unsigned)__builtin_amdgcn_readlane((int)word, 4 * j + 3) << 16);
            }
            if (m_lo | m_hi) {                                        // wave-uniform
                if ((m_lo & bit_lo) | (m_hi & bit_hi)) {
                    const float z = scaled_depth(zraw[wave][64 * j + lane], inv_scale);
                    const unsigned slot = 3u * (run + __builtin_amdgcn_mbcnt_hi(m_hi, __builtin_amdgcn_mbcnt_lo(m_lo, 0u)));   // + valid lanes below this one
                    emit_point((float)col, (float)row, z, cx, cy, div, tile_xyz + slot, tile_rgb + slot, bgr, 0u, t0 + 64 * (size_t)j + lane);
                }
                run += __popc(m_lo) + __popc(m_hi);
            }
            col += 64u;
            while (col >= (unsigned)width) { col -= (unsigned)width; ++row; }
        }
    }
}

// ---- label images: every instance's cloud from ONE pass over the frame (round 3) ---------------------------------------------
// A label image assigns each pixel to at most one instance (label = instance + 1, u8 or u16), so the per-instance kernels above
// - a grid of (pixel blocks x instances), every instance re-reading the whole image: 1.7 ms for C5's 1,024 instances - are the
// wrong shape.  Here a wave owns a tile of 1,024 consecutive pixels and walks it in 16 rounds of 64 (lane = pixel).  The valid
// pixels of a round are grouped by label (one pass per distinct label: an object's pixels are neighbours, a round holds one to
// three labels): pass 1 adds the group's size to counts[instance][tile]; after the usual scan, pass 2 takes the group's base
// from the scanned entry with an atomic add of its size - only this wave ever touches (instance, tile), and it walks its rounds
// in order, so the bases it gets are the row-major ones - and every pixel writes at base + its rank among the group's lanes.
// Frame bytes are read twice (4 B per pixel and pass), the clouds written once.
template <bool L16>
__device__ __forceinline__ int label_at(const uint8_t* __restrict__ labels, size_t i) {
    return L16 ? (int)reinterpret_cast<const uint16_t*>(labels)[i] : (int)labels[i];
}
// the label of pixel i if it is one of the batch's and the pixel's depth (-> *z) is valid, else 0
template <bool L16>
__device__ __forceinline__ int valid_label_at(const uint16_t* __restrict__ raw, const uint8_t* __restrict__ labels, size_t n, int n_inst, float inv_scale,
                                              float zmax, size_t i, float* z) {
    int L = 0;
    if (i < n) {
        *z = scaled_depth(raw[i], inv_scale);
        const int l = label_at<L16>(labels, i);
        if (z_valid(*z, zmax) && l >= 1 && l <= n_inst) L = l;
    }
    return L;
}
// the lanes of a round grouped by label L (0: none): act(src, Ls, m) once per distinct label Ls, with the group's lanes m and its first lane src
template <class Act>
__device__ __forceinline__ void for_each_label_group(int L, Act act) {
    unsigned long long todo = __ballot(L != 0);
    while (todo) {                                                              // wave-uniform
        const int src = __builtin_ctzll(todo);
        const int Ls = __builtin_amdgcn_readlane(L, src);
        const unsigned long long m = __ballot(L == Ls);
        act(src, Ls, m);
        todo &= ~m;
    }
}
template <bool L16>
__global__ __launch_bounds__(256)
void k_label_count(const uint16_t* __restrict__ raw, const uint8_t* __restrict__ labels, size_t n, int n_inst, float inv_scale, float zmax, int ntiles,
                   int* __restrict__ counts) {
    const int lane = threadIdx.x & 63, tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= ntiles) return;
    for (int j = 0; j < 16; ++j) {
        const size_t i = (size_t)tile * 1024 + 64 * j + lane;
        float z = 0.f;
        const int L = valid_label_at<L16>(raw, labels, n, n_inst, inv_scale, zmax, i, &z);
        for_each_label_group(L, [&](int src, int Ls, unsigned long long m) {
            if (lane == src) atomicAdd(&counts[(size_t)(Ls - 1) * ntiles + tile], __popcll(m));
        });
    }
}
template <bool L16>
__global__ __launch_bounds__(256)
void k_label_emit(const uint16_t* __restrict__ raw, const uint8_t* __restrict__ labels, const uint8_t* __restrict__ bgr, int width, size_t n, int n_inst,
                  float inv_scale, float fx, float fy, float cx, float cy, float zmax, int ntiles, int* __restrict__ offsets,
                  float* __restrict__ xyz, float* __restrict__ rgb) {
    const int lane = threadIdx.x & 63, tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= ntiles) return;
    for (int j = 0; j < 16; ++j) {
        const size_t i = (size_t)tile * 1024 + 64 * j + lane;
        float z = 0.f;
        const int L = valid_label_at<L16>(raw, labels, n, n_inst, inv_scale, zmax, i, &z);
        int slot = 0;
        for_each_label_group(L, [&](int src, int Ls, unsigned long long m) {
            int base = 0;
            if (lane == src) base = atomicAdd(&offsets[(size_t)(Ls - 1) * ntiles + tile], __popcll(m));
            base = __builtin_amdgcn_readlane(base, src);
            if (L == Ls) slot = base + __popcll(m & ((1ull << lane) - 1ull));
        });
        if (L != 0) {
            const int v = (int)(i / width), u = (int)(i - (size_t)v * width);
            emit_point((float)u, (float)v, z, cx, cy, PlainDiv{fx, fy}, xyz, rgb, rgb ? bgr : nullptr, (size_t)slot, i);
        }
    }
}

__global__ void k_gather_instance_offsets(const int* __restrict__ offsets, const int* __restrict__ total, int blocks, int n_inst, int* __restrict__ out) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < n_inst) out[b] = offsets[(size_t)b * blocks];
    if (b == n_inst) out[b] = *total;
}

static bool batch_vectorisable(const uint16_t* d_raw, const uint8_t* d_masks, size_t n) {
    return n % 16 == 0 && ((uintptr_t)d_raw % 16 == 0) && ((uintptr_t)d_masks % 16 == 0);   // stacked masks and frames sit at multiples of n
}

// The raw values r with `z > 0 && z <= zmax`, z = (float)r * inv_scale, evaluated exactly as the kernels do (pipeline.cpp:47,71:
// `!(z <= 0 || z > zmax)`).  For a finite inv_scale >= 0 the product is monotone in r and never NaN, so the values form one
// range, found by two bisections; anything else (an infinite scale factor makes 0 * inf = NaN pass the test) is left to the
// per-pixel kernels.  An empty range comes back as [1, 0].
static bool depth_valid_range(float inv_scale, float zmax, int* lo, int* hi) {
    if (!(inv_scale >= 0.f) || !(inv_scale <= FLT_MAX)) return false;
    auto z = [inv_scale](int r) { volatile float v = (float)r * inv_scale; return (float)v; };
    int a = 0, b = 65536;                      // first r with z(r) > 0 (65536: none)
    while (a < b) { const int m = (a + b) / 2; if (z(m) > 0.f) b = m; else a = m + 1; }
    const int first = a;
    a = 0; b = 65536;                          // first r with z(r) > zmax (65536: none; NaN zmax: none, as in the test itself)
    while (a < b) { const int m = (a + b) / 2; if (z(m) > zmax) b = m; else a = m + 1; }
    *lo = first; *hi = a - 1;
    if (*lo > *hi) { *lo = 1; *hi = 0; }
    return true;
}

// Camera parameters for which div_by_uniform is `/` bit for bit on every pixel (see there).  a = (col - c) * z with
// integer col, row < 2^16: col - c is 0 or at least half an ulp of c in size, hence >= 2^-34 for |c| >= 2^-10, and at
// most 2^21; z = raw * inv_scale in [2^-30, 2^26]; so a is 0 (both forms return a signed zero through v_div_fixup) or
// 2^-64 <= |a| <= 2^47, and with 2^-10 <= |f| <= 2^30 the quotient stays within [2^-94, 2^57].
static bool emit_fast_div_ok(float fx, float fy, float cx, float cy, float inv_scale, int w, int h) {
    auto focal = [](float f) { const float a = std::fabs(f); return a >= 0x1p-10f && a <= 0x1p30f; };
    auto centre = [](float c) { const float a = std::fabs(c); return a == 0.f || (a >= 0x1p-10f && a <= 0x1p20f); };
    return focal(fx) && focal(fy) && centre(cx) && centre(cy) && inv_scale >= 0x1p-30f && inv_scale <= 0x1p10f && w <= 65536 && h <= 65536;
}

// Device copy of the instance -> frame map (nullptr when every instance reads frame 0).
int frame_map_dev(tdv_ctx* ctx, int n_inst, int n_frames, const int* h_frame_of, const int** d_frame_of) {
    *d_frame_of = nullptr;
    if (n_frames <= 1 || n_inst <= 0) return TDV_OK;
    std::vector<int> f((size_t)n_inst);
    for (int b = 0; b < n_inst; ++b) {
        f[b] = h_frame_of ? h_frame_of[b] : (int)((long long)b * n_frames / n_inst);
        if (f[b] < 0 || f[b] >= n_frames) return TDV_ERR_BAD_ARG;
    }
    int* d;
    TDV_TRY(ws_alloc(ctx, (size_t)n_inst, &d));
    TDV_HIP(ctx, hipMemcpyAsync(d, f.data(), (size_t)n_inst * 4, hipMemcpyHostToDevice, ctx->stream));
    TDV_HIP(ctx, hipStreamSynchronize(ctx->stream));   // f is a host temporary
    *d_frame_of = d;
    return TDV_OK;
}

static BatchSrc batch_src(const DepthFrames& f, const uint8_t* d_bgr) {
    return BatchSrc{f.raw, f.frame_of, f.masks, d_bgr, f.n, f.layout, f.inv_scale, f.mask_mode, f.zmax};
}

// pass 1 (bitmap + counts + scan): returns the per-instance start offsets (host, n_inst + 1 entries) and the plan - the device
// scan and the bitmap (ctx workspace) - for pass 2
int depth_to_cloud_batch_count(tdv_ctx* ctx, const DepthFrames& f, DepthBatchPlan* plan, int* h_offsets) {
    const size_t n = f.n;
    const int n_inst = f.n_inst;
    const bool label_image = f.layout != MaskLayout::Stacked;   // one u8 or u16 label image: the one-pass kernels
    if (label_image && f.frame_of) return TDV_ERR_BAD_ARG;      // a label image belongs to one frame
    int raw_lo = 1, raw_hi = 0;
    const bool vec = !label_image && batch_vectorisable(f.raw, f.masks, n) && depth_valid_range(f.inv_scale, f.zmax, &raw_lo, &raw_hi);
    const int blocks = vec ? (int)((n + DB_TILE - 1) / DB_TILE) : (int)((n + DP_PX_PER_BLOCK - 1) / DP_PX_PER_BLOCK);   // tiles resp. workgroups per instance (1,024 pixels either way)
    int *counts, *offsets, *d_total, *d_inst;
    uint16_t* bits = nullptr;
    TDV_TRY(ws_alloc(ctx, (size_t)blocks * n_inst, &counts));
    TDV_TRY(ws_alloc(ctx, (size_t)blocks * n_inst, &offsets));
    TDV_TRY(ws_alloc(ctx, 1, &d_total));
    TDV_TRY(ws_alloc(ctx, (size_t)n_inst + 1, &d_inst));
    if (vec) TDV_TRY(ws_alloc(ctx, (size_t)n_inst * (n / DB_PX), &bits));
    *plan = DepthBatchPlan{label_image ? DepthBatchPlan::LabelImage : vec ? DepthBatchPlan::TiledBitmap : DepthBatchPlan::Scalar, blocks, offsets, bits};
    hipStream_t s = ctx->stream;
    if (label_image) TDV_HIP(ctx, hipMemsetAsync(counts, 0, (size_t)blocks * n_inst * 4, s));
    {
        ScopedTimer tm(ctx, TDV_TIMER_DEPTH);
        if (label_image) {
            if (f.layout == MaskLayout::LabelU16) k_label_count<true><<<(blocks + 3) / 4, 256, 0, s>>>(f.raw, f.masks, n, n_inst, f.inv_scale, f.zmax, blocks, counts);
            else k_label_count<false><<<(blocks + 3) / 4, 256, 0, s>>>(f.raw, f.masks, n, n_inst, f.inv_scale, f.zmax, blocks, counts);
        } else if (vec) {
            const dim3 grid((blocks + DP_BLOCK / 64 - 1) / (DP_BLOCK / 64), (n_inst + DB_GROUP - 1) / DB_GROUP);
#define TDV_DEPTH_BITS(ST, PF) k_depth_bits<ST, PF><<<grid, DP_BLOCK, 0, s>>>(f.raw, f.frame_of, f.masks, n, n_inst, raw_lo, raw_hi, f.mask_mode, blocks, bits, counts)
            if (f.frame_of) TDV_DEPTH_BITS(true, true); else TDV_DEPTH_BITS(true, false);
#undef TDV_DEPTH_BITS
        } else k_count<BatchSrc><<<dim3(blocks, n_inst), DP_BLOCK, 0, s>>>(batch_src(f, nullptr), counts);
    }
    TDV_CHECK_LAUNCH(ctx);
    {
        ScopedTimer tm(ctx, TDV_TIMER_DEPTH);   // the scan belongs to the operator's kernel time
        TDV_TRY(exclusive_scan_dev(ctx, counts, blocks * n_inst, offsets, d_total));
        k_gather_instance_offsets<<<(n_inst + 256) / 256, 256, 0, s>>>(offsets, d_total, blocks, n_inst, d_inst);
    }
    TDV_CHECK_LAUNCH(ctx);
    TDV_TRY(pin_reserve(ctx, ((size_t)n_inst + 1) * 4));
    TDV_HIP(ctx, hipMemcpyAsync(ctx->pin, d_inst, ((size_t)n_inst + 1) * 4, hipMemcpyDeviceToHost, s));
    TDV_HIP(ctx, hipStreamSynchronize(s));
    std::memcpy(h_offsets, ctx->pin, ((size_t)n_inst + 1) * 4);
    return TDV_OK;
}

// pass 2 (emit) into buffers sized from pass 1, with the kernel family pass 1 took
int depth_to_cloud_batch_emit(tdv_ctx* ctx, const DepthFrames& f, const uint8_t* d_bgr, const Pinhole& cam, const DepthBatchPlan& plan,
                              float* d_xyz, float* d_rgb) {
    const size_t n = f.n;
    const int ntiles = plan.blocks;
    ScopedTimer tm(ctx, TDV_TIMER_DEPTH);
    if (plan.family == DepthBatchPlan::LabelImage) {             // the one-pass kernels (the scanned offsets serve as cursors)
        if (f.layout == MaskLayout::LabelU16) k_label_emit<true><<<(ntiles + 3) / 4, 256, 0, ctx->stream>>>(f.raw, f.masks, d_bgr, f.w, n, f.n_inst, f.inv_scale, cam.fx, cam.fy, cam.cx, cam.cy, f.zmax, ntiles, plan.offsets, d_xyz, d_rgb);
        else k_label_emit<false><<<(ntiles + 3) / 4, 256, 0, ctx->stream>>>(f.raw, f.masks, d_bgr, f.w, n, f.n_inst, f.inv_scale, cam.fx, cam.fy, cam.cx, cam.cy, f.zmax, ntiles, plan.offsets, d_xyz, d_rgb);
    } else if (plan.family == DepthBatchPlan::TiledBitmap) {
        const int tiles_per_block = (DE_BLOCK / 64) * DE_TPW;
        const dim3 grid((ntiles + tiles_per_block - 1) / tiles_per_block, f.n_inst);
        const bool fd = emit_fast_div_ok(cam.fx, cam.fy, cam.cx, cam.cy, f.inv_scale, f.w, f.h), rows = n % DB_TILE == 0;
#define TDV_EMIT(FD, RW) k_depth_emit_bits<FD, RW><<<grid, DE_BLOCK, 0, ctx->stream>>>(f.raw, f.frame_of, d_bgr, plan.bits, f.w, n, f.inv_scale, cam.fx, cam.fy, cam.cx, cam.cy, ntiles, plan.offsets, d_xyz, d_rgb)
        if (fd) { if (rows) TDV_EMIT(true, true); else TDV_EMIT(true, false); }
        else { if (rows) TDV_EMIT(false, true); else TDV_EMIT(false, false); }
#undef TDV_EMIT
    } else {
        k_emit<BatchSrc><<<dim3(ntiles, f.n_inst), DP_BLOCK, 0, ctx->stream>>>(batch_src(f, d_bgr), f.w, cam, plan.offsets, d_xyz, d_rgb);
    }
    TDV_CHECK_LAUNCH(ctx);
    return TDV_OK;
}

// Why an instance came out of the batched count pass with no point: does its masked depth image hold ANY non-zero value
// (cv::countNonZero(scaled_depth) of src/pipeline.cpp:57)?  If not the reference stops at :57-60 ("empty depth after
// masking"), else at :86-89 ("empty point cloud": every masked pixel lies beyond the z clip).  Run for the empty instances
// only - rare - so the count pass itself stays as it is.
__global__ __launch_bounds__(DP_BLOCK)
void k_masked_nonzero_any(const uint16_t* __restrict__ raw0, const int* __restrict__ frame_of, const uint8_t* __restrict__ masks, size_t n, MaskLayout layout,
                          float inv_scale, int mask_mode, const int* __restrict__ inst, int* __restrict__ flags) {
    const int b = inst[blockIdx.y];
    const uint16_t* __restrict__ raw = raw0 + (frame_of ? (size_t)frame_of[b] : 0) * n;
    bool any = false;
    for (int k = 0; k < DP_PX_PER_THREAD; ++k) {
        const size_t i = (size_t)blockIdx.x * DP_PX_PER_BLOCK + k * DP_BLOCK + threadIdx.x;
        if (i < n) any |= masked_depth(raw, masks, n, b, layout, i, inv_scale, mask_mode) != 0.f;
    }
    if (__any(any) && (threadIdx.x & 63) == 0) atomicOr(&flags[blockIdx.y], 1);
}

int depth_batch_nonzero_any(tdv_ctx* ctx, const DepthFrames& f, const int* h_inst, int n_list, int* h_flags) {
    if (n_list <= 0) return TDV_OK;
    int *d_inst, *d_flags;
    TDV_TRY(ws_alloc(ctx, (size_t)n_list, &d_inst));
    TDV_TRY(ws_alloc(ctx, (size_t)n_list, &d_flags));
    TDV_HIP(ctx, hipMemcpyAsync(d_inst, h_inst, (size_t)n_list * 4, hipMemcpyHostToDevice, ctx->stream));
    TDV_HIP(ctx, hipMemsetAsync(d_flags, 0, (size_t)n_list * 4, ctx->stream));
    const int blocks = (int)((f.n + DP_PX_PER_BLOCK - 1) / DP_PX_PER_BLOCK);
    k_masked_nonzero_any<<<dim3(blocks, n_list), DP_BLOCK, 0, ctx->stream>>>(f.raw, f.frame_of, f.masks, f.n, f.layout, f.inv_scale, f.mask_mode, d_inst, d_flags);
    TDV_CHECK_LAUNCH(ctx);
    TDV_HIP(ctx, hipMemcpyAsync(h_flags, d_flags, (size_t)n_list * 4, hipMemcpyDeviceToHost, ctx->stream));
    TDV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return TDV_OK;
}

}  // namespace tdv
