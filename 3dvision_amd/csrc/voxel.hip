// Voxel-grid downsample on gfx950 (HBM-bound: 24 B in + 24 B out per point, plus the grouping).
//
// Replaces Registration::voxelDownsample (src/registration.cpp:29-60 of the reference), which has no GPU entry point there
// (src/pipeline.cpp:92 calls the CPU static).  The rules - cell, mean, unit normal, key hash - are stated in voxel_rules.hpp; what this
// file adds is GROUPING: the members of a voxel have to be summed in ascending input index, and the voxels come out in FIRST-OCCURRENCE
// order (the order of their first points).  voxel_order.hip turns that into the reference's container order where it is asked for.
//
// Four ways to group, tried as a ladder (voxel_first_order): a rung that cannot cope says so with one word, and the next one starts over.
//   rung            default for                         hands over when                              cost
//   pixel windows   clouds handed over with the         VS_FAILED: a tile off the pixel grid, a      no atomics, no member rows, no limit on a voxel's
//   (k_vs_group)    intrinsics that unprojected them    window above VS_WIN_MAX (coarse voxels),     members; 73 KB of LDS per workgroup
//                   (registration batches, the          rows too long for the halo, points not in
//                   pinhole batch entry)                row-major pixel order
//   table           every other call: one cloud or      a voxel of more than VH_K = 16 points        memset + 2 launches for any number of clouds;
//   (k_vh_insert)   many (tdv_voxel_downsample*,        (the overflow word)                          bound by device-scope atomics (20 G/s)
//                   multi-scale levels, model prep)
//   counting sort   -  (TDV_VOXEL_LEGACY, study)        too_big: a hash bucket of more than          9 dependent launches, 0.10-0.12 ms for a cloud
//   (one cloud)                                         VX_MAX_BUCKET = 96 records                   that HBM moves in a microsecond
//   full sort       -  (TDV_VOXEL_SORT, study)          never                                        bitonic sort of (cell, index) records: 15 launches,
//   (one cloud)                                                                                      global passes for strides >= the 2,048-record tile
// The sorts take one cloud: a batch whose table overflows is redone cloud by cloud (voxel_downsample_batch_dev, or the caller's own
// lanes), each cloud starting again at the table.
#include "voxel_rules.hpp"
#include <type_traits>
#include <vector>

namespace tdv {

// the sort record of point i: its cell as unsigned words, then its index
__device__ __forceinline__ uint4 voxel_record(const float* __restrict__ xyz, int i, float inv) {
    const int4 c = voxel_cell(xyz, (size_t)i, inv, i);
    return make_uint4((unsigned)c.x, (unsigned)c.y, (unsigned)c.z, (unsigned)c.w);
}
__global__ void k_voxel_records(const float* __restrict__ xyz, int n, int n_pow2, float inv, uint4* __restrict__ rec) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pow2) return;
    rec[i] = i < n ? voxel_record(xyz, i, inv) : make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);  // padding sorts last
}

// ---- rungs 3 and 4: counting sort by cell hash, with the full bitonic sort (sort.hip) below it ---------------------------------
// Members of a voxel only have to become one run in ascending input index; the order of the runs is irrelevant
// (positions come from the leader scan).  So: bucket = hash(cell) into >= 2n buckets (counting sort, integer atomics),
// then every bucket — a handful of records, possibly of several colliding cells — is insertion-sorted by
// (cell, index) by one lane, which also emits the bucket's voxels (k_voxel_bucket_emit).  A bucket larger than VX_MAX_BUCKET (a very coarse grid) raises a flag and the call is
// redone with the full sort.
constexpr int VX_MAX_BUCKET = 96;
__device__ __forceinline__ unsigned voxel_hash(unsigned x, unsigned y, unsigned z) {
    unsigned h = x * 73856093u ^ y * 19349663u ^ z * 83492791u;
    h ^= h >> 15; h *= 0x2c1b3c6du; h ^= h >> 12;
    return h;
}
__global__ void k_voxel_hist(const float* __restrict__ xyz, int n, float inv, unsigned mask, uint4* __restrict__ rec_in, int* __restrict__ hist) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4 r = voxel_record(xyz, i, inv);
    rec_in[i] = r;
    atomicAdd(&hist[voxel_hash(r.x, r.y, r.z) & mask], 1);
}
__global__ void k_voxel_scatter(const uint4* __restrict__ rec_in, int n, unsigned mask, const int* __restrict__ start, int* __restrict__ cursor,
                                uint4* __restrict__ rec) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4 r = rec_in[i];
    const unsigned b = voxel_hash(r.x, r.y, r.z) & mask;
    rec[start[b] + atomicAdd(&cursor[b], 1)] = r;
}
// The hashed path's third kernel: every lane owns one bucket.  It sorts the bucket's few records by (cell, index); the
// members of a voxel then form a run INSIDE the bucket (a cell hashes to one bucket), so the same lane marks the run's
// leader (its smallest input index), sums the members in ascending index order and parks the mean at the leader's index.
// One launch instead of bucket sort + heads + means; the slot of a mean (its first-occurrence rank) comes from the scan of
// the leader flags, after which k_voxel_compact moves it there.
// The bucket's records sorted by (cell, index), its voxels emitted.  `a` points at the bucket's records - in LDS (the normal case:
// the workgroup's 256 buckets are one contiguous stretch of the record array, staged with coalesced loads) or in global memory.
template <bool NRM>
__device__ __forceinline__ void voxel_emit_bucket(uint4* a, int m, const float* __restrict__ xyz, const float* __restrict__ rgb,
                                                  int* __restrict__ leader, float* __restrict__ mean_xyz, float* __restrict__ mean_rgb, VoxelNormals nrm) {
    for (int e = 1; e < m; ++e) {   // insertion sort by (x, y, z, index)
        const uint4 key = a[e];
        int f = e - 1;
        while (f >= 0 && rec_less(key, a[f])) { a[f + 1] = a[f]; --f; }
        a[f + 1] = key;
    }
    for (int e = 0; e < m;) {
        const uint4 r = a[e];
        VoxelSum<NRM> sum;
        int cnt = 0;
        for (; e < m; ++e, ++cnt) {               // the run: ascending input index
            const uint4 q = a[e];
            if (!same_cell(q, r)) break;
            sum.add(xyz, rgb, nrm.in, (size_t)q.w);
        }
        leader[r.w] = 1;
        sum.emit(cnt, mean_xyz, mean_rgb, nrm.out, rgb != nullptr, (size_t)r.w);
    }
}
constexpr int VX_LDS_REC = 1024;   // records of a workgroup's 256 buckets staged in LDS (16 KB); a denser stretch sorts in global memory
template <bool NRM>
__global__ __launch_bounds__(256)
void k_voxel_bucket_emit(uint4* __restrict__ rec, const int* __restrict__ start, const int* __restrict__ hist, int nbuckets, int n_rec,
                         int* __restrict__ too_big, const float* __restrict__ xyz, const float* __restrict__ rgb,
                         int* __restrict__ leader, float* __restrict__ mean_xyz, float* __restrict__ mean_rgb, VoxelNormals nrm /* out: parked at the leader, like mean_rgb */) {
    // The insertion sort is a chain of dependent loads and stores: through global memory every step is a round trip of about a
    // microsecond and the kernel's time was that of its fullest bucket (42 us at 200k points with lanes alive for 3 us on
    // average); through LDS a step costs a hundred cycles: 25 us.  (Staging the records' points in LDS as well, so that the sums
    // run over LDS too, changed nothing; nor did a 12-comparator sorting network over registers for buckets of up to 6 records.)
    __shared__ uint4 s_rec[VX_LDS_REC];
    const int b0 = blockIdx.x * 256, b = b0 + threadIdx.x;
    const int base = start[b0];                                           // nbuckets is a multiple of 256
    const int end = b0 + 256 < nbuckets ? start[b0 + 256] : n_rec;
    const bool staged = end - base <= VX_LDS_REC;
    if (staged) for (int i = threadIdx.x; i < end - base; i += 256) s_rec[i] = rec[base + i];
    __syncthreads();
    const int m = hist[b];
    if (m == 0) return;
    if (m > VX_MAX_BUCKET) { *too_big = 1; return; }
    if (staged) voxel_emit_bucket<NRM>(s_rec + (start[b] - base), m, xyz, rgb, leader, mean_xyz, mean_rgb, nrm);
    else voxel_emit_bucket<NRM>(rec + start[b], m, xyz, rgb, leader, mean_xyz, mean_rgb, nrm);
}
// out[rank[i]] = mean parked at leader i
__global__ void k_voxel_compact(const int* __restrict__ leader, const int* __restrict__ rank, int n, const float* __restrict__ mean_xyz,
                                const float* __restrict__ mean_rgb, int capacity, float* __restrict__ out_xyz, float* __restrict__ out_rgb,
                                VoxelNormals nrm /* in: parked at the leaders; both NULL without normals */) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !leader[i]) return;
    const int slot = rank[i];
    if (slot >= capacity) return;
    copy_row3(out_xyz, (size_t)slot, mean_xyz, (size_t)i);
    copy_row3_opt(out_rgb, (size_t)slot, mean_rgb, (size_t)i);
    copy_row3_opt(nrm.out, (size_t)slot, nrm.in, (size_t)i);
}

// leader[idx] = 1 for the smallest input index of each voxel
__global__ void k_voxel_heads(const uint4* __restrict__ rec, int n, int* __restrict__ leader) {
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    uint4 r = rec[p];
    bool head = true;
    if (p > 0) head = !same_cell(rec[p - 1], r);
    if (head) leader[r.w] = 1;
}

// For every leader i (the first point of each voxel), at its first-occurrence rank: its input index and its integer
// cell — all the host needs to replay the reference's container (the cloud itself never leaves the device).
__global__ void k_voxel_leader_list(const int* __restrict__ leader, const int* __restrict__ rank, const float* __restrict__ xyz, float inv,
                                    int n, int4* __restrict__ leaders) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && leader[i]) leaders[rank[i]] = voxel_cell(xyz, (size_t)i, inv, i);
}

// one lane per run head: sequential sum over the run (ascending input index), mean -> out[rank]
template <bool NRM>
__global__ __launch_bounds__(256)
void k_voxel_means(const uint4* __restrict__ rec, int n, const float* __restrict__ xyz, const float* __restrict__ rgb,
                   const int* __restrict__ rank, int capacity, float* __restrict__ out_xyz, float* __restrict__ out_rgb, VoxelNormals nrm) {
    int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    uint4 r = rec[p];
    if (p > 0 && same_cell(rec[p - 1], r)) return;
    const int slot = rank[r.w];
    if (slot >= capacity) return;
    VoxelSum<NRM> sum;
    int cnt = 0;
    for (int e = p; e < n; ++e, ++cnt) {
        const uint4 m = rec[e];
        if (!same_cell(m, r)) break;
        sum.add(xyz, rgb, nrm.in, (size_t)m.w);
    }
    sum.emit(cnt, out_xyz, out_rgb, nrm.out, rgb != nullptr, (size_t)slot);
}


// ---- rung 2: grouping through a hash table, memset + 2 kernels for any number of clouds (round 3) ------------------------------
// The counting-sort path above is nine dependent launches whose waves wait >= 90 % of their cycles (profiles/r2: 0.10-0.12 ms
// for a cloud that HBM moves in a microsecond).  This path is three, and takes B clouds stored back to back at once:
//   memset            one fill (0x7f bytes) of [claim table | per-voxel count | scan descriptors | ticket | overflow flag]
//   k_vh_insert       one lane per point: find-or-claim the cell's slot of an open-addressing table (linear probing, 32-bit
//                     atomics).  The slot permanently holds the CLAIMER - the first point that got there; its index names the
//                     voxel: vcnt[claimer] counts the members down from 0x7f7f7f7f, members[claimer][arrival rank] lists them
//                     (VH_K per voxel; a fuller voxel raises a flag and the call is redone on the counting-sort path).  Lanes of
//                     a wave that share a cell go to the table once, through their lowest lane.  Which point claims a slot and
//                     the arrival order depend on the race; nothing that leaves the kernel pair does.
//   k_vh_finalize     one lane per point, 1,024 points per workgroup: every lane reads its voxel's member row; the smallest
//                     index in it is the voxel's leader (an atomic min per point in k_vh_insert did the same for 5 us more).
//                     Leader flags, workgroup scan, DECOUPLED LOOK-BACK over the workgroups' aggregates (single pass: no scan
//                     launches) -> the leader's first-occurrence rank; the leader sums its voxel's points in ascending index
//                     order (VoxelSum), divides and writes the mean at its rank.  Voxels of cloud b occupy
//                     [voff[b], voff[b + 1]).  Count and overflow flag go straight into pinned host memory (no copy kernel).
// Algorithmic bytes: 12 N in + 12 V out; the table adds 16 B per point of atomics and 4-68 B per voxel of member lists.
constexpr int VH_K = 16;                       // member slots per voxel (one 64-B row)
constexpr int VH_EMPTY = 0x7f7f7f7f;           // what the memset leaves; larger than any point index
constexpr int VH_BLOCK = 1024, VH_IPT = 1, VH_ITEMS = VH_BLOCK * VH_IPT;   // one point per lane: four per lane ran their gather chains one after the other
constexpr unsigned long long VH_ST_MASK = 3ull << 62, VH_ST_WAIT = 1ull << 62, VH_ST_AGG = 2ull << 62, VH_ST_PREFIX = 3ull << 62;   // 0x7f.. has status 01
static_assert((0x7f7f7f7f7f7f7f7full & VH_ST_MASK) == VH_ST_WAIT, "the memset pattern must read as 'not ready'");

__device__ __forceinline__ int vh_segment(const int* __restrict__ seg_off, int nseg, int g) {   // largest b with seg_off[b] <= g (b < nseg)
    int lo = 0, hi = nseg;
    while (hi - lo > 1) { const int m = (lo + hi) >> 1; if (seg_off[m] <= g) lo = m; else hi = m; }
    return lo;
}

__global__ __launch_bounds__(256)
void k_vh_insert(const float* __restrict__ xyz, int total, const int* __restrict__ seg_off, int nseg, float inv, unsigned mask,
                 int* __restrict__ claim, int* __restrict__ vcnt, int* __restrict__ members,
                 int* __restrict__ voxel_of, int* __restrict__ overflow) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    const bool active = g < total;
    const int lane = threadIdx.x & 63;
    int lo = 0, hi = total, b = 0;
    int cx = 0, cy = 0, cz = 0;
    if (active) {
        if (nseg > 1) { b = vh_segment(seg_off, nseg, g); lo = seg_off[b]; hi = seg_off[b + 1]; }
        const int3 c = voxel_cell(xyz, (size_t)g, inv);
        cx = c.x; cy = c.y; cz = c.z;
    }
    // Device-scope atomics are resolved beyond the XCDs' L2s and cost microseconds each; neighbouring points (one wave holds 64
    // consecutive ones, in image order neighbouring pixels) mostly share their voxels.  The wave therefore groups its lanes by
    // (cloud, cell) first - one pass per distinct cell, the cell of the lowest pending lane broadcast with readlane - and only the
    // lowest lane of a group goes to the table, for the whole group: one find-or-claim, one atomicMin, one atomicSub by the group's
    // size.  Lanes are in index order, so the group's lowest lane holds its smallest index.
    // (a cloud in random order has nothing to group: when no lane shares its cell with the lane before it, every lane goes alone)
    const bool dup = lane > 0 && cx == __shfl_up(cx, 1, 64) && cy == __shfl_up(cy, 1, 64) && cz == __shfl_up(cz, 1, 64) && b == __shfl_up(b, 1, 64);
    unsigned long long todo = __ballot(active), group = 1ull << lane;
    if (!__any(active && dup)) todo = 0ull;
    while (todo) {                                        // wave-uniform
        const int src = __builtin_ctzll(todo);
        const int rx = __builtin_amdgcn_readlane(cx, src), ry = __builtin_amdgcn_readlane(cy, src), rz = __builtin_amdgcn_readlane(cz, src),
                  rb = __builtin_amdgcn_readlane(b, src);
        const bool same = active && cx == rx && cy == ry && cz == rz && b == rb;
        const unsigned long long m = __ballot(same);
        if (same) group = m;
        todo &= ~m;
    }
    if (!active) return;
    const int head = __builtin_ctzll(group);
    const int rank = __popcll(group & ((1ull << lane) - 1ull)), size = __popcll(group);
    int j = 0, pos0 = 0;
    if (lane == head) {
        // (One table for all clouds, the cloud mixed into the hash.  Giving every cloud its OWN stretch of the table - two slots per
        //  point at [2 lo, 2 hi), so that the workgroups in flight touch a few MB instead of 512 - was measured in round 4 and LOST:
        //  k_vh_insert 2.2 -> 3.15 ms for the 256-cloud batch, 20 -> 39 us for one cloud.  The device-scope atomics of the ~2,000
        //  workgroups in flight then land on a few memory channels instead of all of them; spreading them is worth more than locality.)
        unsigned h = voxel_hash((unsigned)cx, (unsigned)cy, (unsigned)cz) + (unsigned)b * 0x9e3779b9u;
        for (;; ++h) {
            int* slot = claim + (h & mask);
            j = *slot;                                                  // (a plain load first: claiming with the CAS straight away - one round trip for the four
            if (j == VH_EMPTY) { const int prev = atomicCAS(slot, VH_EMPTY, g); j = prev == VH_EMPTY ? g : prev; }   // of five groups that find their slot empty - cost a batch 30 % more: a device-scope atomic is dearer than a load + an atomic that mostly succeeds)
            if (j == g) break;
            if (j >= lo && j < hi) {                        // the same cloud: same cell?
                const int3 q = voxel_cell(xyz, (size_t)j, inv);
                if (q.x == cx && q.y == cy && q.z == cz) break;
            }
        }
        // The claimer is a member by being the claimer: it neither counts itself nor writes itself into the row (round 4).  Four of five
        // voxels of a depth-camera cloud hold one point: for them the insertion is now the load + the claiming CAS and nothing else
        // (it was: + one more device-scope atomic and a scattered 4-byte store into a 64-byte row nobody reads).
        const int others = j == g ? size - 1 : size;
        if (others > 0) pos0 = VH_EMPTY - atomicSub(&vcnt[j], others);       // arrival ranks of the non-claimers pos0 .. pos0 + others - 1
    }
    const int g_head = __shfl(g, head, 64);
    j = __shfl(j, head, 64); pos0 = __shfl(pos0, head, 64);
    voxel_of[g] = j;
    if (j == g) return;                                  // the claimer itself
    const int pos = pos0 + (j == g_head ? rank - 1 : rank);
    if (pos < VH_K - 1) members[(size_t)j * VH_K + pos] = g;
    else *overflow = 1;                                 // (any value but the fill pattern)
}

// ---- rung 1: grouping WITHOUT the table, for clouds that come from a pinhole depth image (round 4) ------------------------------
// k_vh_insert is bound by the chip's rate of device-scope atomics (20 G/s: profiles/r4/history/voxel_batch.md).  A cloud
// unprojected from a depth image needs none: its points are in row-major pixel order, and all members of a voxel lie within a
// few pixels of each other - two points of one voxel differ by less than the voxel size s in x, y and z, hence by
//     |du| <= fx * (s / z) * (1 + |x / z|)        (u - cx = fx * x / z;  d(x / z) <= dx / z + |x / z| * dz / z)
// pixels in u, the same with fy in v.  So one workgroup takes a TILE of consecutive points of one cloud plus a HALO of whole
// rows before and after it, recovers every point's pixel (u = rint(cx + fx * x / z): the rounding error of the unprojection is
// 4e-4 pixel), enters the points into a pixel map in LDS, and every point looks its voxel's members up in the (2 win_v + 1) x
// (2 win_u + 1) window around its own pixel - 3 x 3 at the pipeline's 1.2-pixel voxels.  The window walk is in row-major order =
// ascending input index: the smallest member index is the voxel's LEADER, and the leader can add its voxel's points up in the
// reference's order right there.  The kernel writes voxel_of[g] = the leader (what k_vh_insert writes, with the leader as claimer)
// and the voxel's mean at the leader's index; k_vh_finalize then only ranks the leaders and moves the means to their ranks - no
// member rows, no counts, no limit on the members of a voxel, and nothing depends on a race.
// Anything the argument does not cover makes the tile raise *fail (the caller redoes the call through the table): a window
// above VS_WIN_MAX (coarse voxels), rows too long for the halo, a pixel map or a key range that does not fit, points that are not
// in row-major pixel order (the cloud is not what the caller said it was), non-positive depth, and points OFF THE PIXEL GRID.
// The window is a bound on continuous pixel distances, and the map holds rint'ed pixels: two members whose positions lie within
// VS_GRID_TOL of their pixels are at most 2 VS_GRID_TOL farther apart on the map than the bound, which the +0.01 of the windows'
// floors absorbs.  A cloud unprojected with other intrinsics than the caller's (another scale or principal point), or moved by a
// fraction of a pixel, can still be in row-major order, but its points sit up to half a pixel off their rint: a member would then
// fall one pixel outside its neighbour's window and the voxel would be split.  Such a point fails the tile.
struct VoxelPinhole { float fx, fy, cx, cy; };
// How far a recovered position cx + fx * x / z may lie from its pixel.  For a point the call's own intrinsics unprojected,
// x = (u - cx) * z / fx and a = x * rcp(z) carry ~5 roundings (2^-24 relative each: 3e-7 of |u - cx|, 2e-4 px at 640 px from the
// principal point), and cx + fx * a two more at the magnitude of the pixel (6e-5 px each below 2,048): 4e-4 px in all.
// VS_GRID_TOL is 10x that, and 2 VS_GRID_TOL = 0.008 stays inside the windows' 0.01 of slack, so on-grid clouds keep the windows
// they had.  The error grows with |u - cx| (3e-7 of it) and with the pixel's magnitude (half an ulp per rounding: 6e-5 px below
// 2,048, 4.9e-4 px from 8,192 to 16,383): the 10x margin holds within ~1,000 px of the principal point (frames up to ~2k px wide),
// and on-grid points stay within VS_GRID_TOL up to ~8k px from it.  Beyond that an on-grid cloud may be handed to the table: the
// same result, by the slower path.
constexpr float VS_GRID_TOL = 0.004f;
#ifndef VS_TILE_VALUE
#define VS_TILE_VALUE 4096
#endif
#ifndef VS_HALO_VALUE
#define VS_HALO_VALUE 2048
#endif
#ifndef VS_MAP_VALUE
#define VS_MAP_VALUE 20480
#endif
constexpr int VS_TILE = VS_TILE_VALUE, VS_HALO = VS_HALO_VALUE, VS_LOAD = VS_TILE + 2 * VS_HALO, VS_BLOCK = 1024, VS_PER = VS_LOAD / VS_BLOCK;
constexpr int VS_MAP = VS_MAP_VALUE;          // pixel map entries (u16: local index + 1)
constexpr int VS_WIN_MAX = 3;
constexpr int VS_FAILED = 2;           // value of the overflow word when a tile could not be grouped this way (written with atomicMin; the word starts as VH_EMPTY)

// LDS per loaded point: its cell relative to the tile's first point, packed into 32 bits (10 + 8 + 14: a tile spans a few hundred cells in
// x, a few dozen in y; a range that does not fit raises *fail), and its map entry: 73 KB per workgroup, two workgroups per CU.  (The
// first version kept three 16-bit cells and the pixels - 129 KB, one workgroup per CU: 1.39 ms for the 256-cloud batch; 16-bit tags
// with the neighbour's cell recomputed from memory on a match: 1.08 ms - the dependent loads of the checks, one after the other.)
constexpr int VS_KX = 10, VS_KY = 8, VS_KZ = 14;

__global__ __launch_bounds__(VS_BLOCK, 2)
void k_vs_group(const float* __restrict__ xyz, const int* __restrict__ seg_off, const int2* __restrict__ tiles /* (first owned point, cloud) */,
                float inv, float voxel, VoxelPinhole cam, float* __restrict__ mean_at /* [point][3]: a leader's voxel mean, at the leader's index */,
                int* __restrict__ voxel_of, int* __restrict__ overflow) {
    __shared__ unsigned key[VS_LOAD];
    __shared__ unsigned short map[VS_MAP];
    __shared__ unsigned edge[VS_PER][VS_BLOCK / 64];                      // pixel of every wave's last lane, per round (the order check across waves)
    __shared__ int s_umin, s_umax, s_vlast, s_vend, s_bad;
    __shared__ unsigned s_zmin, s_amax, s_bmax;
    const int2 tl = tiles[blockIdx.x];
    const int lo = seg_off[tl.y], hi = seg_off[tl.y + 1];
    const int g0 = tl.x, g1 = min(g0 + VS_TILE, hi);
    const int l0 = max(lo, g0 - VS_HALO), l1 = min(hi, g1 + VS_HALO), nl = l1 - l0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) { s_umin = INT_MAX; s_umax = INT_MIN; s_vlast = 0; s_vend = 0; s_bad = 0; s_zmin = 0x7f800000u; s_amax = 0u; s_bmax = 0u; }
    for (int e = threadIdx.x; e < VS_MAP / 2; e += VS_BLOCK) reinterpret_cast<unsigned*>(map)[e] = 0u;
    __syncthreads();
    // pass 1: pixel and tag of every loaded point (thread t holds points t, t + 1024, ...: the owned ones among them are its own in pass 3)
    unsigned pvu[VS_PER], pk[VS_PER];                                     // v << 16 | u; the cell relative to the first loaded point's, biased to the middle of its bit field
    const int3 c0 = voxel_cell(xyz, (size_t)l0, inv);
    const long long ox = (long long)c0.x - (1 << (VS_KX - 1)), oy = (long long)c0.y - (1 << (VS_KY - 1)), oz = (long long)c0.z - (1 << (VS_KZ - 1));   // (a poisoned first point has cell INT_MIN)
    int umin = INT_MAX, umax = INT_MIN;
    float zmin = INFINITY, amax = 0.f, bmax = 0.f; bool bad = false;
#pragma unroll
    for (int q = 0; q < VS_PER; ++q) {
        const int i = (int)threadIdx.x + q * VS_BLOCK;
        pvu[q] = 0u; pk[q] = 0u;
        if (i < nl) {
            const size_t g = (size_t)(l0 + i);
            const float x = xyz[3 * g], y = xyz[3 * g + 1], z = xyz[3 * g + 2];
            const int3 c = voxel_cell(xyz, g, inv);
            const long long rx = (long long)c.x - ox, ry = (long long)c.y - oy, rq = (long long)c.z - oz;
            if (rx < 0 || rx >= (1 << VS_KX) || ry < 0 || ry >= (1 << VS_KY) || rq < 0 || rq >= (1 << VS_KZ)) bad = true;     // a tile wider than the packed cell: the table
            pk[q] = (unsigned)rx | ((unsigned)ry << VS_KX) | ((unsigned)rq << (VS_KX + VS_KY));
            key[i] = pk[q];
            const float rz = __frcp_rn(z);                               // (a reciprocal is plenty: the pixel is recovered to 4e-4, VS_GRID_TOL is 4e-3)
            const float a = x * rz, b = y * rz;
            const float pu = cam.cx + cam.fx * a, pv = cam.cy + cam.fy * b;
            const float fu = rintf(pu), fv = rintf(pv);
            if (!(z > 0.f) || !(fu >= 0.f && fu < 65535.f && fv >= 0.f && fv < 65535.f)) bad = true;
            else if (!(fabsf(pu - fu) <= VS_GRID_TOL && fabsf(pv - fv) <= VS_GRID_TOL)) bad = true;      // off the pixel grid: the table
            else {
                const int u = (int)fu, v = (int)fv;
                pvu[q] = ((unsigned)v << 16) | (unsigned)u;
                umin = min(umin, u); umax = max(umax, u);
                zmin = fminf(zmin, z); amax = fmaxf(amax, fabsf(a)); bmax = fmaxf(bmax, fabsf(b));
                if (i == g1 - 1 - l0) s_vlast = v;
                if (i == nl - 1) s_vend = v;
            }
        }
        if (lane == 63) edge[q][wave] = pvu[q];
    }
    // (one LDS atomic per WAVE and value: an atomic per thread on a handful of addresses took longer than everything else here)
    unsigned zb = __float_as_uint(zmin), ab = __float_as_uint(amax), bb = __float_as_uint(bmax);      // (non-negative floats order like their bits)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        umin = min(umin, __shfl_xor(umin, o, 64)); umax = max(umax, __shfl_xor(umax, o, 64));
        zb = min(zb, (unsigned)__shfl_xor((int)zb, o, 64)); ab = max(ab, (unsigned)__shfl_xor((int)ab, o, 64)); bb = max(bb, (unsigned)__shfl_xor((int)bb, o, 64));
    }
    if (lane == 0) { atomicMin(&s_umin, umin); atomicMax(&s_umax, umax); atomicMin(&s_zmin, zb); atomicMax(&s_amax, ab); atomicMax(&s_bmax, bb); }
    if (bad) s_bad = 1;
    // row-major order inside the thread's rounds is checked against the lane before (the point before in memory); lane 0 looks at the wave before
    bool viol = false;
#pragma unroll
    for (int q = 0; q < VS_PER; ++q) {
        const unsigned prev = __shfl_up(pvu[q], 1, 64);
        const int i = (int)threadIdx.x + q * VS_BLOCK;
        if (lane > 0 && i < nl && !(pvu[q] > prev)) viol = true;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < VS_PER; ++q) {
        const int i = (int)threadIdx.x + q * VS_BLOCK;
        if (lane == 0 && i > 0 && i < nl) {
            const unsigned prev = wave > 0 ? edge[q][wave - 1] : edge[q > 0 ? q - 1 : 0][VS_BLOCK / 64 - 1];
            if (!(pvu[q] > prev)) viol = true;
        }
    }
    const int u0 = s_umin, ur = s_umax - s_umin + 1;
    const int qo = (g0 - l0) / VS_BLOCK;                                  // the thread's first owned round (g0 - l0 is 0 or VS_HALO: a multiple of the block)
    const int v0 = (int)(__shfl(pvu[0], 0, 64) >> 16);                    // (wave 0 only: the first loaded point's row) - broadcast below
    __shared__ int s_v0, s_vfirst;
    if (threadIdx.x == 0) { s_v0 = v0; s_vfirst = (int)((qo == 0 ? pvu[0] : pvu[VS_HALO / VS_BLOCK < VS_PER ? VS_HALO / VS_BLOCK : 0]) >> 16); }
    __syncthreads();
    const int vbase = s_v0, vr = s_vend - s_v0 + 1;
    const float z_min = __uint_as_float(s_zmin);
    // how far apart (in pixels) two members of one voxel can be: the bound of the header, for points that need not be among the loaded
    // ones (a member shares a voxel with a loaded point: its z is at most a voxel smaller, its |x| at most a voxel larger)
    const float z_eff = z_min - voxel, rze = 1.f / z_eff;
    const float reach = voxel * rze * 1.001f;
    const int win_u = (int)floorf(cam.fx * reach * (1.f + (__uint_as_float(s_amax) * z_min + voxel) * rze) + 0.01f);
    const int win_v = (int)floorf(cam.fy * reach * (1.f + (__uint_as_float(s_bmax) * z_min + voxel) * rze) + 0.01f);
    bool ok = !s_bad && nl > 0 && z_eff > 0.f && vr > 0 && (long long)ur * vr <= VS_MAP && win_u <= VS_WIN_MAX && win_v <= VS_WIN_MAX;
    // a halo of whole rows that covers the windows (the first and the last loaded row may be cut: they must lie outside every window)
    if (ok && threadIdx.x == 0) {
        if (l0 > lo && !(vbase < s_vfirst - win_v)) viol = true;
        if (l1 < hi && !(s_vend > s_vlast + win_v)) viol = true;
    }
    if (__syncthreads_or(viol || !ok)) { if (threadIdx.x == 0) atomicMin(overflow, VS_FAILED); return; }
    // pass 2: the pixel map
#pragma unroll
    for (int q = 0; q < VS_PER; ++q) {
        const int i = (int)threadIdx.x + q * VS_BLOCK;
        if (i < nl) map[((int)(pvu[q] >> 16) - vbase) * ur + ((int)(pvu[q] & 0xffffu) - u0)] = (unsigned short)(i + 1);
    }
    __syncthreads();
    // pass 3: every owned point walks its window in row-major order = ascending input index
#pragma unroll
    for (int q = 0; q < VS_PER; ++q) {
        const int li = (int)threadIdx.x + q * VS_BLOCK;
        if (q < qo || li < g0 - l0 || li >= g1 - l0) continue;
        const size_t gp = (size_t)(l0 + li);
        const unsigned mk = pk[q];
        // this point's own window: the bound with ITS depth and tangents - never larger than the tile's, which the halo was checked against
        const float pz = xyz[3 * gp + 2], prz = __frcp_rn(pz - voxel), pa = fabsf(xyz[3 * gp]) * prz, pb = fabsf(xyz[3 * gp + 1]) * prz;
        const float r0 = voxel * prz * 1.001f;
        const int wu = min(win_u, (int)floorf(cam.fx * r0 * (1.f + pa + r0) + 0.01f)), wv = min(win_v, (int)floorf(cam.fy * r0 * (1.f + pb + r0) + 0.01f));
        const int pu_ = (int)(pvu[q] & 0xffffu) - u0, pv_ = (int)(pvu[q] >> 16) - vbase;
        const int ua = max(pu_ - wu, 0), ub = min(pu_ + wu, ur - 1), va = max(pv_ - wv, 0), vb = min(pv_ + wv, vr - 1);
        auto member = [&](int m) -> bool { return m >= 0 && m != li && key[m] == mk; };
        int leader = li, others = 0;
        for (int vv = va; vv <= vb; ++vv)
            for (int uu = ua; uu <= ub; ++uu) {
                const int m = (int)map[vv * ur + uu] - 1;
                if (member(m)) { ++others; leader = min(leader, m); }
            }
        const int g = l0 + li;
        voxel_of[g] = l0 + leader;
        if (leader == li) {
            // the leader sums its voxel (VoxelSum, points only): itself, then the others as the window walk meets them - ascending input index
            VoxelSum<false> sum;
            sum.add_point(xyz[3 * gp], xyz[3 * gp + 1], pz);
            if (others > 0)
                for (int vv = va; vv <= vb; ++vv)
                    for (int uu = ua; uu <= ub; ++uu) {
                        const int m = (int)map[vv * ur + uu] - 1;
                        if (member(m)) sum.add(xyz, nullptr, nullptr, (size_t)(l0 + m));
                    }
            sum.emit(others + 1, mean_at, nullptr, nullptr, false, gp);
        }
    }
}

// MODE 0: single pass (tiles numbered by ticket, decoupled look-back).  MODE 1 / 2: the same split in two for large inputs - count
// the leaders per tile (tile_sums), [exclusive scan], emit with the scanned prefix (tile_prefix): with tens of thousands of tiles the
// look-back's polling (device-scope loads in a loop from every tile in flight) slows the whole memory system down - 61 us of waiting
// per tile and 51 us for a leader wave's gathers in a batch of 256 clouds, against 9 and 18 us for one cloud.
// (The parameters stay a scalar list: handed over as by-value descriptors - clouds, groups, scan state, VoxelFirst - the kernel kept its
// registers, LDS and occupancy but gained address arithmetic on the descriptors' kernarg bases and moves in front of its gathers, 1 to
// 6 instructions per instantiation: profiles/r28/voxel_rules.md.  The host side, voxel_group_hashed, takes the descriptors.)
template <int MODE, bool NRM>
__global__ __launch_bounds__(VH_BLOCK)
void k_vh_finalize(const float* __restrict__ xyz, const float* __restrict__ rgb, int total, const int* __restrict__ seg_off, int nseg, float inv,
                   const int* __restrict__ voxel_of, const int* __restrict__ vcnt, const int* __restrict__ members,
                   unsigned long long* __restrict__ desc, int* __restrict__ ticket, float* __restrict__ out_xyz, float* __restrict__ out_rgb,
                   int* __restrict__ rank_out /* per point: global first-occurrence rank of leaders */, int4* __restrict__ leaders /* optional */,
                   int* __restrict__ voff /* nseg + 2: the last entry receives the overflow flag */, int capacity /* voxels that fit out_xyz */,
                   const int* __restrict__ overflow_flag, int* __restrict__ host_result /* optional, pinned host memory: {voxels, overflow flag} */,
                   int* __restrict__ tile_sums /* MODE 1 */, const int* __restrict__ tile_prefix /* MODE 2 */,
                   int leader_known /* voxel_of[g] IS the voxel's smallest index (k_vs_group): only the leaders look at counts and rows */,
                   const float* __restrict__ mean_at /* with leader_known: the leaders' means are ready, at their own indices */,
                   VoxelNormals nrm /* NRM: the clouds' normals and their voxels' unit means, laid out like xyz and out_xyz (never with leader_known) */) {
    __shared__ int s_ticket, s_excl, s_wave[VH_BLOCK / 64];
    if (*overflow_flag == VS_FAILED) {          // k_vs_group gave up on a tile: voxel_of is not valid, nothing here may follow it - the caller redoes the call
        if (blockIdx.x == 0 && threadIdx.x == 0) { voff[nseg + 1] = VS_FAILED; if (host_result) { host_result[0] = 0; host_result[1] = VS_FAILED; __threadfence_system(); } }
        return;
    }
    if (MODE == 0) {
        if (threadIdx.x == 0) s_ticket = atomicAdd(ticket, 1) - VH_EMPTY;     // workgroups take their tiles in the order they start
        __syncthreads();
    }
    const int t = MODE == 0 ? s_ticket : (int)blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = t * VH_ITEMS + threadIdx.x;
    const bool inside = g < total;
    // this point's voxel: its member row (the indices of its points in arrival order).  The smallest is the voxel's leader.
    const int j = inside ? voxel_of[g] : 0;
    // members = the claimer j + the `others` that found j's slot taken (their indices in j's row, arrival order)
    const bool look = inside && !leader_known;
    const int others = look ? min(VH_EMPTY - vcnt[j], VH_K - 1) : 0;     // (an overflowing voxel: the call is redone, whatever is written here is dropped)
    const int cnt = inside ? others + 1 : 0;
    int m[VH_K];
    {
        const int4* row = reinterpret_cast<const int4*>(members + (size_t)j * VH_K);
#pragma unroll
        for (int q = 0; q < VH_K / 4; ++q) {
            int4 r = make_int4(VH_EMPTY, VH_EMPTY, VH_EMPTY, VH_EMPTY);
            if (4 * q < others) r = row[q];                  // (a voxel of one point - four of five in a depth-camera cloud - is that point: its row is never fetched)
            m[4 * q] = 4 * q < others ? r.x : VH_EMPTY; m[4 * q + 1] = 4 * q + 1 < others ? r.y : VH_EMPTY;
            m[4 * q + 2] = 4 * q + 2 < others ? r.z : VH_EMPTY; m[4 * q + 3] = 4 * q + 3 < others ? r.w : VH_EMPTY;
        }
        m[VH_K - 1] = inside ? j : VH_EMPTY;                 // (others <= VH_K - 1: the last entry of the row is never used)
    }
    int first_member = VH_EMPTY;
#pragma unroll
    for (int q = 0; q < VH_K; ++q) first_member = min(first_member, m[q]);
    const bool lead = inside && (leader_known ? j == g : first_member == g);
    const int mine = lead ? 1 : 0;
    // workgroup scan of the leader flags
    int incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const int v = __shfl_up(incl, off, 64); if (lane >= off) incl += v; }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int wbase = 0, agg = 0;
#pragma unroll
    for (int w = 0; w < VH_BLOCK / 64; ++w) { if (w < wave) wbase += s_wave[w]; agg += s_wave[w]; }
    if (MODE == 1) { if (threadIdx.x == 0) tile_sums[t] = agg; return; }
    if (MODE == 2) { if (threadIdx.x == 0) s_excl = tile_prefix[t]; }
    // decoupled look-back (wave 0): publish the aggregate, then add up the predecessors' aggregates back to the nearest
    // inclusive prefix, 64 tiles per step.  Tiles are numbered by ticket, so every predecessor has started and publishes its
    // aggregate without waiting for anybody: the wait below always ends.
    if (MODE == 0 && wave == 0) {
        if (lane == 0) __hip_atomic_store(&desc[t], (t == 0 ? VH_ST_PREFIX : VH_ST_AGG) | (unsigned long long)(unsigned)agg, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        int excl = 0;
        for (int look = t - 1; look >= 0; look -= 64) {
            const int idx = look - lane;
            unsigned long long d = VH_ST_PREFIX;                                  // tiles before the first: prefix 0
            if (idx >= 0) {
                d = __hip_atomic_load(&desc[idx], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
                while ((d & VH_ST_MASK) == VH_ST_WAIT) { __builtin_amdgcn_s_sleep(1); d = __hip_atomic_load(&desc[idx], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT); }
            }
            const unsigned long long pm = __ballot((d & VH_ST_MASK) == VH_ST_PREFIX);
            const int first = pm ? __builtin_ctzll(pm) : 64;                       // nearest tile that already holds an inclusive prefix
            int v = lane <= first ? (int)(unsigned)(d & 0xffffffffull) : 0;
            v = wave_sum_i32(v);
            excl += v;
            if (pm) break;
        }
        if (lane == 0) {
            if (t > 0) __hip_atomic_store(&desc[t], VH_ST_PREFIX | (unsigned long long)(unsigned)(excl + agg), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            s_excl = excl;
        }
    }
    __syncthreads();
    const int run = s_excl + wbase + incl - mine;        // global first-occurrence rank (of this lane's voxel if it leads one)
    const bool last_tile = (t + 1) * VH_ITEMS >= total;
    if (last_tile && threadIdx.x == VH_BLOCK - 1) {      // the grand total, and every cloud that starts at the very end (empty trailing clouds)
        const int total_v = s_excl + agg, ovf = *overflow_flag;   // (the flag was set by k_vh_insert, the launch before)
        voff[nseg] = total_v;
        voff[nseg + 1] = ovf;
        if (nseg > 1) for (int b = nseg - 1; b >= 0 && seg_off[b] >= total; --b) voff[b] = total_v;
        if (host_result) { host_result[0] = total_v; host_result[1] = ovf; __threadfence_system(); }   // straight into pinned host memory: no copy kernel
    }
    if (!inside) return;
    int lo = 0, b = 0;
    if (nseg > 1) { b = vh_segment(seg_off, nseg, g); lo = seg_off[b]; }
    if (g == lo) {                                        // first point of cloud b: its voxels start at this rank; so do the empty clouds right before it
        voff[b] = run;
        for (int bb = b - 1; bb >= 0 && seg_off[bb] == g; --bb) voff[bb] = run;
    }
    if (!lead) return;
    if (leader_known) {                                   // k_vs_group summed the voxel already: move its mean to its rank
        const size_t o = (size_t)run;
        if (rank_out) rank_out[g] = run;
        if (run >= capacity) return;
        copy_row3(out_xyz, o, mean_at, (size_t)g);
        if (leaders) leaders[o] = voxel_cell(xyz, (size_t)g, inv, g - lo);
        return;
    }
    // ascending index order without moving anything: cnt rounds of "smallest index above the last one"
    VoxelSum<NRM> sum;
    int last = -1;
    for (int r = 0; r < cnt; ++r) {
        int nxt = VH_EMPTY;
#pragma unroll
        for (int q = 0; q < VH_K; ++q) nxt = (m[q] > last && m[q] < nxt) ? m[q] : nxt;
        last = nxt;
        sum.add(xyz, rgb, nrm.in, (size_t)nxt);
    }
    const size_t o = (size_t)run;
    if (rank_out) rank_out[g] = run;
    if (run >= capacity) return;                          // the caller's buffer is too small: it learns the count and gets an error
    sum.emit(cnt, out_xyz, out_rgb, nrm.out, rgb != nullptr, o);
    if (leaders) leaders[o] = voxel_cell(xyz, (size_t)g, inv, g - lo);
}

// ---- the ladder -----------------------------------------------------------------------------------------------------------------
// What a rung is handed: one cloud (d_off null) or several stored back to back, with their optional companions.
struct VoxelInput {
    const float* xyz; const float* rgb; const float* nrm;   // rgb / nrm null: a cloud without that companion (nrm never with cam)
    int total; int n_clouds; const int* d_off; const int* h_off;   // cloud b = points [off[b], off[b + 1]), on the device and on the host
    const VoxelPinhole* cam;                                // the clouds are in row-major pixel order under these intrinsics, or null
};
enum VoxelRung { RUNG_PIXELS = 0, RUNG_TABLE, RUNG_COUNTING_SORT, RUNG_FULL_SORT, RUNG_CLOUD_BY_CLOUD };

// Rungs 1 and 2, the pixel windows (by_pixels) and the table: memset, k_vs_group or k_vh_insert, k_vh_finalize.  Voxels of cloud b at
// [h_voff[b], h_voff[b + 1]) of out.xyz.  *flag = the rung's overflow word: VH_EMPTY - grouped; VS_FAILED - a tile the pixel windows do
// not cover; anything else - a voxel of more than VH_K points (in both cases nothing of `out` is valid).  Synchronizes once.
static int voxel_group_hashed(tdv_ctx* ctx, const VoxelInput& in, float voxel, VoxelFirst out, bool by_pixels, int split_from, int* h_voff, int* flag) {
    hipStream_t s = ctx->stream;
    const int total = in.total, nseg = in.n_clouds;
    if (by_pixels && (in.nrm || !in.cam || !in.d_off || !in.h_off)) return TDV_ERR_BAD_ARG;      // (k_vs_group sums the points only)
    const float inv = 1.0f / voxel;  // registration.cpp:32
    const int tiles = (total + VH_ITEMS - 1) / VH_ITEMS;
    if (!out.d_voff) TDV_TRY(ws_alloc(ctx, (size_t)nseg + 2, &out.d_voff));
    // one cloud: the finalize kernel stores {voxel count, overflow flag} into pinned memory itself (a D2H copy of 8 bytes is a 9-us blit kernel)
    int* h_result = nullptr;
    if (!in.d_off) {
        TDV_TRY(pin_reserve(ctx, 64));
        h_result = reinterpret_cast<int*>(ctx->pin);
        h_result[0] = -1; h_result[1] = 0;
    }
    {
        ScopedTimer tm(ctx, TDV_TIMER_VOXEL);
        // one fill: claim[slots] | vcnt[total] | desc[tiles] (u64) | ticket | overflow.  Grouped by pixels: no table, no counts, no member rows -
        // only the scan descriptors, the ticket and the overflow word are filled, and the leaders' means take 12 B per point
        size_t slots = 0, n_cnt = 0;
        if (!by_pixels) { slots = 4096; while (slots < 2 * (size_t)total) slots <<= 1; n_cnt = (size_t)total; }
        const size_t desc_at = (slots + n_cnt + 1) & ~(size_t)1;
        const size_t n_fill = desc_at + 2 * (size_t)tiles + 2;
        int* fill;
        TDV_TRY(ws_alloc(ctx, n_fill, &fill));
        int* claim = fill; int* vcnt = claim + slots;
        unsigned long long* desc = reinterpret_cast<unsigned long long*>(fill + desc_at);
        int* ticket = reinterpret_cast<int*>(desc + tiles);
        int* overflow = ticket + 1;
        int *members = nullptr, *voxel_of; float* mean_at = nullptr;
        if (by_pixels) TDV_TRY(ws_alloc(ctx, (size_t)total * 3, &mean_at));
        else TDV_TRY(ws_alloc(ctx, (size_t)total * VH_K, &members));
        TDV_TRY(ws_alloc(ctx, (size_t)total, &voxel_of));
        if (by_pixels) {
            // tiles: consecutive VS_TILE-point stretches of every cloud (a tile never spans two clouds)
            size_t nt = 0;
            for (int b = 0; b < nseg; ++b) nt += (size_t)((in.h_off[b + 1] - in.h_off[b] + VS_TILE - 1) / VS_TILE);
            int2* d_tiles;
            TDV_TRY(ws_alloc(ctx, nt, &d_tiles));
            TDV_TRY(pin_reserve(ctx, nt * sizeof(int2) + 64 + ((size_t)nseg + 2) * 4));   // (+ what is staged afterwards: the buffer must not move while the copy below is in flight)
            int2* h_tiles = reinterpret_cast<int2*>(ctx->pin);
            size_t k = 0;
            for (int b = 0; b < nseg; ++b)
                for (int g = in.h_off[b]; g < in.h_off[b + 1]; g += VS_TILE) h_tiles[k++] = make_int2(g, b);
            TDV_HIP(ctx, hipMemcpyAsync(d_tiles, h_tiles, nt * sizeof(int2), hipMemcpyHostToDevice, s));
            TDV_HIP(ctx, hipMemsetAsync(fill, 0x7f, n_fill * 4, s));
            k_vs_group<<<(unsigned)nt, VS_BLOCK, 0, s>>>(in.xyz, in.d_off, d_tiles, inv, voxel, *in.cam, mean_at, voxel_of, overflow);
        } else {
            TDV_HIP(ctx, hipMemsetAsync(fill, 0x7f, n_fill * 4, s));
            k_vh_insert<<<(total + 255) / 256, 256, 0, s>>>(in.xyz, total, in.d_off, nseg, inv, (unsigned)(slots - 1), claim, vcnt, members, voxel_of, overflow);
        }
        // the finalize kernel of mode M, with the normals riding along (NRM) or not: the same grouping pass either way
        const auto finalize = [&](auto M, int* tile_sums, const int* tile_prefix) {
            constexpr int MODE = decltype(M)::value;
            const auto kernel = in.nrm ? k_vh_finalize<MODE, true> : k_vh_finalize<MODE, false>;
            kernel<<<tiles, VH_BLOCK, 0, s>>>(in.xyz, in.rgb, total, in.d_off, nseg, inv, voxel_of, vcnt, members, desc, ticket, out.xyz, out.rgb, out.rank, out.leaders,
                                              out.d_voff, out.capacity, overflow, h_result, tile_sums, tile_prefix, by_pixels ? 1 : 0, mean_at, VoxelNormals{in.nrm, out.nrm});
        };
        // (measured, us per call one pass / split: 184k points in pixel order 65 / 76; random order 250k 82 / 74, 500k 138 / 103, 1M 233 / 160, 4M 858 / 550;
        //  256 clouds of 184k 8,100 / 4,400 - tools/studies/voxel_split_threshold.py)
        if (tiles < split_from)
            finalize(std::integral_constant<int, 0>{}, nullptr, nullptr);
        else {      // large inputs (a batch): count, scan, emit - launches without a wait inside
            int *tile_sums, *tile_prefix, *d_tot;
            TDV_TRY(ws_alloc(ctx, (size_t)tiles, &tile_sums));
            TDV_TRY(ws_alloc(ctx, (size_t)tiles, &tile_prefix));
            TDV_TRY(ws_alloc(ctx, 1, &d_tot));
            finalize(std::integral_constant<int, 1>{}, tile_sums, nullptr);
            TDV_TRY(exclusive_scan_dev(ctx, tile_sums, tiles, tile_prefix, d_tot));
            finalize(std::integral_constant<int, 2>{}, nullptr, tile_prefix);
        }
        TDV_CHECK_LAUNCH(ctx);
    }
    if (h_result) {
        TDV_HIP(ctx, hipStreamSynchronize(s));
        if (h_result[0] < 0) { snprintf(ctx->err, sizeof(ctx->err), "voxel: the result did not reach the host"); return TDV_ERR_INTERNAL; }
        *flag = h_result[1];
        h_voff[0] = 0; h_voff[1] = h_result[0];
        return TDV_OK;
    }
    TDV_TRY(pin_reserve(ctx, ((size_t)nseg + 2) * 4));
    int* h = reinterpret_cast<int*>(ctx->pin);
    TDV_HIP(ctx, hipMemcpyAsync(h, out.d_voff, ((size_t)nseg + 2) * 4, hipMemcpyDeviceToHost, s));   // offsets, then the overflow flag
    TDV_HIP(ctx, hipStreamSynchronize(s));
    *flag = h[nseg + 1];
    if (*flag == VH_EMPTY) std::memcpy(h_voff, h, ((size_t)nseg + 1) * 4);
    return TDV_OK;
}

// Rungs 3 and 4, one cloud through the counting sort (buckets of up to VX_MAX_BUCKET records: a fuller one sets *too_big and nothing of
// `out` is valid) or the full bitonic sort (any cloud).  Both end in leader flags and their scan; the means are moved from where the
// bucket kernel parked them, or summed over the sorted runs.  Synchronizes twice.
static int voxel_group_sorted(tdv_ctx* ctx, const VoxelInput& in, float voxel, const VoxelFirst& out, bool full_sort, int* h_voff, int* too_big) {
    hipStream_t s = ctx->stream;
    const int n = in.total;
    const float inv = 1.0f / voxel;  // registration.cpp:32
    const size_t n_pow2 = sort_pow2((size_t)n);
    uint4* rec; int *leader, *rank = out.rank, *d_total;
    TDV_TRY(ws_alloc(ctx, n_pow2, &rec));
    if (!rank) TDV_TRY(ws_alloc(ctx, (size_t)n, &rank));
    TDV_TRY(ws_alloc(ctx, 1, &d_total));
    TDV_TRY(pin_reserve(ctx, 64));
    ScopedTimer tm(ctx, TDV_TIMER_VOXEL);
    int* d_too_big = nullptr;
    float *mean_xyz = nullptr, *mean_rgb = nullptr, *mean_nrm = nullptr;     // counting sort: means parked at their leader's input index
    if (!full_sort) {
        // 9 launches (round 1: 15): one memset, cell histogram, scan (2), scatter, bucket sort + leaders + means, scan (2), compact
        size_t nb = 4096;
        while (nb < 2 * (size_t)n) nb <<= 1;
        int *zeroed, *hist, *cursor, *start, *d_tot2; uint4* rec_in;
        TDV_TRY(ws_alloc(ctx, 2 * nb + 1 + (size_t)n, &zeroed));        // hist | cursor | too_big | leader: one memset
        hist = zeroed; cursor = zeroed + nb; d_too_big = zeroed + 2 * nb; leader = zeroed + 2 * nb + 1;
        TDV_TRY(ws_alloc(ctx, nb, &start));
        TDV_TRY(ws_alloc(ctx, 1, &d_tot2));
        TDV_TRY(ws_alloc(ctx, (size_t)n, &rec_in));
        TDV_TRY(ws_alloc(ctx, (size_t)n * 3, &mean_xyz));
        if (in.rgb) TDV_TRY(ws_alloc(ctx, (size_t)n * 3, &mean_rgb));
        if (in.nrm) TDV_TRY(ws_alloc(ctx, (size_t)n * 3, &mean_nrm));
        TDV_HIP(ctx, hipMemsetAsync(zeroed, 0, (2 * nb + 1 + (size_t)n) * 4, s));
        k_voxel_hist<<<(n + 255) / 256, 256, 0, s>>>(in.xyz, n, inv, (unsigned)(nb - 1), rec_in, hist);
        TDV_TRY(exclusive_scan_dev(ctx, hist, (int)nb, start, d_tot2));
        k_voxel_scatter<<<(n + 255) / 256, 256, 0, s>>>(rec_in, n, (unsigned)(nb - 1), start, cursor, rec);
        const auto emit = in.nrm ? k_voxel_bucket_emit<true> : k_voxel_bucket_emit<false>;
        emit<<<(unsigned)((nb + 255) / 256), 256, 0, s>>>(rec, start, hist, (int)nb, n, d_too_big, in.xyz, in.rgb, leader, mean_xyz, mean_rgb, VoxelNormals{in.nrm, mean_nrm});
    } else {
        TDV_TRY(ws_alloc(ctx, (size_t)n, &leader));
        k_voxel_records<<<(unsigned)((n_pow2 + 255) / 256), 256, 0, s>>>(in.xyz, n, (int)n_pow2, inv, rec);
        TDV_TRY(sort_records_dev(ctx, rec, n_pow2));
        TDV_HIP(ctx, hipMemsetAsync(leader, 0, (size_t)n * 4, s));
        k_voxel_heads<<<(n + 255) / 256, 256, 0, s>>>(rec, n, leader);
    }
    TDV_TRY(exclusive_scan_dev(ctx, leader, n, rank, d_total));
    int* h_total = reinterpret_cast<int*>(ctx->pin);
    h_total[1] = 0;
    TDV_HIP(ctx, hipMemcpyAsync(h_total, d_total, 4, hipMemcpyDeviceToHost, s));
    if (d_too_big) TDV_HIP(ctx, hipMemcpyAsync(h_total + 1, d_too_big, 4, hipMemcpyDeviceToHost, s));
    TDV_HIP(ctx, hipStreamSynchronize(s));
    *too_big = h_total[1];
    if (*too_big) return TDV_OK;   // a bucket too large for the per-lane sort (very coarse grid)
    h_voff[0] = 0; h_voff[1] = h_total[0];
    if (!full_sort) k_voxel_compact<<<(n + 255) / 256, 256, 0, s>>>(leader, rank, n, mean_xyz, mean_rgb, out.capacity, out.xyz, out.rgb, VoxelNormals{mean_nrm, out.nrm});
    else {
        const auto means = in.nrm ? k_voxel_means<true> : k_voxel_means<false>;
        means<<<(n + 255) / 256, 256, 0, s>>>(rec, n, in.xyz, in.rgb, rank, out.capacity, out.xyz, out.rgb, VoxelNormals{in.nrm, out.nrm});
    }
    // leaders (first point of every voxel: cell + input index) in first-occurrence order: all the reference order needs
    if (out.leaders) k_voxel_leader_list<<<(n + 255) / 256, 256, 0, s>>>(leader, rank, in.xyz, inv, n, out.leaders);
    TDV_CHECK_LAUNCH(ctx);
    TDV_HIP(ctx, hipStreamSynchronize(s));      // the device entry points return with their results in place (include/tdv_hip.h)
    return TDV_OK;
}

// The one owner of the rungs: the voxels of these clouds in first-occurrence order, by the first rung that can do it.  A rung's failure
// signal is read here and nowhere else; what a rung that handed over allocated is given back.  Several clouds have no rung below the
// table: *done = RUNG_CLOUD_BY_CLOUD tells the caller to climb down with one cloud at a time.  The study knobs start one cloud lower.
static int voxel_first_order(tdv_ctx* ctx, const VoxelInput& in, float voxel, const VoxelFirst& out, const VoxelKnobs& knobs, int* h_voff, VoxelRung* done) {
    int rung = in.cam && knobs.pixels ? RUNG_PIXELS : RUNG_TABLE;
    if (!in.d_off && knobs.counting_sort) rung = RUNG_COUNTING_SORT;
    if (!in.d_off && knobs.full_sort) rung = RUNG_FULL_SORT;
    const WsMark mark = ws_mark(ctx);
    for (;; ++rung) {
        ws_rewind(ctx, mark);
        if (rung >= RUNG_COUNTING_SORT && in.d_off) rung = RUNG_CLOUD_BY_CLOUD;
        int signal = 0;
        if (rung <= RUNG_TABLE) {
            TDV_TRY(voxel_group_hashed(ctx, in, voxel, out, rung == RUNG_PIXELS, knobs.split_from, h_voff, &signal));
            signal = signal != VH_EMPTY;      // VS_FAILED: a tile off the pixel grid, coarse voxels, rows too long; else a voxel of more than VH_K points
        } else if (rung <= RUNG_FULL_SORT)
            TDV_TRY(voxel_group_sorted(ctx, in, voxel, out, rung == RUNG_FULL_SORT, h_voff, &signal));      // too_big: a bucket of more than VX_MAX_BUCKET records
        if (!signal) break;
    }
    *done = (VoxelRung)rung;
    return TDV_OK;
}

VoxelKnobs voxel_knobs() {
    const auto live = [](const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; };
    const auto study = [](const char* name, int unset) { const char* e = study_env(name); return e ? atoi(e) : unset; };
    VoxelKnobs k;
    k.pixels = live("TDV_VOXEL_PIXELS", 1) != 0;
    k.device_order = live("TDV_VOXEL_DEVICE_ORDER", -1);
    k.batch = live("TDV_BATCH_VOXEL", 1) != 0;
    k.counting_sort = study_env("TDV_VOXEL_LEGACY") != nullptr;
    k.full_sort = study_env("TDV_VOXEL_SORT") != nullptr;
    k.real_map = study_env("TDV_VOXEL_REAL_MAP") != nullptr;
    k.split_from = study("TDV_VOXEL_SPLIT_FROM", 224);
    return k;
}

// ---- the entry points ----------------------------------------------------------------------------------------------------------
int voxel_downsample_dev(tdv_ctx* ctx, const float* d_xyz, const float* d_rgb, int n, float voxel, int order,
                         float* d_out_xyz, float* d_out_rgb, int capacity, int* n_out, const VoxelBothOrders* both, VoxelNormals nrm) {
    if (!ctx || !n_out || n < 0 || capacity < 0 || !(voxel > 0.f) || (n > 0 && !d_xyz)) return TDV_ERR_BAD_ARG;
    if (!nrm.in || !nrm.out) nrm = VoxelNormals{nullptr, nullptr};     // (as the colours: both arrays or no normals)
    if (!d_rgb || !d_out_rgb) { d_rgb = nullptr; d_out_rgb = nullptr; }
    if (order != TDV_VOXEL_ORDER_FIRST && order != TDV_VOXEL_ORDER_REFERENCE) return TDV_ERR_BAD_ARG;
    if (both && (order != TDV_VOXEL_ORDER_REFERENCE || !both->first_xyz || !both->ref2first || !both->first2ref)) return TDV_ERR_BAD_ARG;
    *n_out = 0;
    if (n == 0) return TDV_OK;
    const VoxelKnobs knobs = voxel_knobs();
    // first-occurrence order lands in the caller's buffers directly; the reference order goes through rows of their own
    VoxelFirst first{d_out_xyz, d_out_rgb, nrm.out, capacity};
    const bool ref = order == TDV_VOXEL_ORDER_REFERENCE;
    if (ref) {
        first.capacity = n;
        TDV_TRY(ws_alloc(ctx, (size_t)n, &first.rank));
        TDV_TRY(ws_alloc(ctx, (size_t)n, &first.leaders));
        if (both) first.xyz = both->first_xyz; else TDV_TRY(ws_alloc(ctx, (size_t)n * 3, &first.xyz));
        if (d_rgb) TDV_TRY(ws_alloc(ctx, (size_t)n * 3, &first.rgb));
        if (nrm.in) TDV_TRY(ws_alloc(ctx, (size_t)n * 3, &first.nrm));
    }
    int h_voff[2] = {0, 0};
    VoxelRung done;
    TDV_TRY(voxel_first_order(ctx, VoxelInput{d_xyz, d_rgb, nrm.in, n, 1, nullptr, nullptr, nullptr}, voxel, first, knobs, h_voff, &done));
    const int v = h_voff[1];
    *n_out = v;
    if (v > capacity) return TDV_ERR_BAD_ARG;
    if (!ref) return TDV_OK;
    return voxel_finish_reference(ctx, n, v, first, d_out_xyz, d_out_rgb, nrm.out, both, knobs);
}

int voxel_downsample_batch_dev(tdv_ctx* ctx, const float* d_xyz, const int* h_off, const int* d_off, int n_clouds, float voxel, const float* pinhole4,
                               const VoxelFirst& out, int* h_voff, const float* d_normals, int* overflowed, bool batched) {
    if (!ctx || n_clouds < 1 || !h_off || !h_voff || !(voxel > 0.f) || h_off[n_clouds] < 0) return TDV_ERR_BAD_ARG;
    const bool with_nrm = d_normals && out.nrm;
    if (with_nrm && pinhole4) return TDV_ERR_BAD_ARG;       // (the pixel windows sum the points only)
    const int total = h_off[n_clouds];
    if (overflowed) *overflowed = 0;
    for (int b = 0; b <= n_clouds; ++b) h_voff[b] = 0;
    if (batched) {
        VoxelRung done = RUNG_TABLE;
        if (total > 0) {
            // Clouds unprojected from a depth image with the given intrinsics are grouped through pixel windows, without the table
            // (k_vs_group); if a tile cannot be (coarse voxels, very long rows, a cloud that is not what the caller said) the table takes over.
            VoxelPinhole cam{};
            if (pinhole4) { cam.fx = pinhole4[0]; cam.fy = pinhole4[1]; cam.cx = pinhole4[2]; cam.cy = pinhole4[3]; }
            const bool has_cam = pinhole4 && cam.fx > 0.f && cam.fy > 0.f;
            const std::vector<int> off_copy(h_off, h_off + n_clouds + 1);          // (a copy: the pinned staging is reused by the tile table)
            VoxelFirst first = out;
            first.rgb = nullptr; first.nrm = with_nrm ? out.nrm : nullptr; first.capacity = total;
            TDV_TRY(voxel_first_order(ctx, VoxelInput{d_xyz, nullptr, with_nrm ? d_normals : nullptr, total, n_clouds, d_off, off_copy.data(), has_cam ? &cam : nullptr},
                                      voxel, first, voxel_knobs(), h_voff, &done));
            ctx->last_voxel_grouping = done == RUNG_PIXELS ? 2 : 1;
        }
        const int redo = done == RUNG_CLOUD_BY_CLOUD ? 1 : 0;
        ctx->last_voxel_batch_redone = redo;
        if (overflowed) *overflowed = redo;
        if (!redo || overflowed) return TDV_OK;
    }
    // one cloud on its own, or a voxel with more points than the table's member rows hold (a coarse grid): cloud by cloud down the
    // rest of the ladder, packed back to back as the batched pass leaves them
    const WsMark mark = ws_mark(ctx);
    int at = 0;
    for (int b = 0; b < n_clouds; ++b) {
        const int n = h_off[b + 1] - h_off[b];
        int v = 0;
        h_voff[b] = at;
        if (n > 0) {
            ws_rewind(ctx, mark);
            TDV_TRY(voxel_downsample_dev(ctx, d_xyz + (size_t)h_off[b] * 3, nullptr, n, voxel, TDV_VOXEL_ORDER_FIRST, out.xyz + (size_t)at * 3, nullptr, n, &v, nullptr,
                                         VoxelNormals{with_nrm ? d_normals + (size_t)h_off[b] * 3 : nullptr, with_nrm ? out.nrm + (size_t)at * 3 : nullptr}));
        }
        at += v;
    }
    h_voff[n_clouds] = at;
    return TDV_OK;
}

}  // namespace tdv
