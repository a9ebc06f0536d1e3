// The rules of the reference's voxel downsample (Registration::voxelDownsample, src/registration.cpp:29-60; key and hash :15-27),
// each stated once, for device and host code alike: every grouping path of voxel.hip, the reference order of voxel_order.hip and the
// host export tdv_voxel_rules (hostops.hip, held on the CPU by tests/test_voxel_rules.py) compile these statements.
#pragma once
#include "tdv_internal.hpp"

namespace tdv {

// 1. The cell of point i: (int)floor(p * inv) per axis, inv = 1 / voxel_size (:32), converted as x86 does (cvt_i32_x86: NaN and
// everything out of int range -> INT_MIN) ...
__host__ __device__ __forceinline__ int3 voxel_cell(const float* __restrict__ xyz, size_t i, float inv) {
    return make_int3(cvt_i32_x86(floorf(xyz[3 * i] * inv)), cvt_i32_x86(floorf(xyz[3 * i + 1] * inv)), cvt_i32_x86(floorf(xyz[3 * i + 2] * inv)));   // registration.cpp:33-36
}
// ... and the leader record of a voxel whose first point it is: the cell and the point's index (within its cloud) - all the reference
// order needs of a cloud
__host__ __device__ __forceinline__ int4 voxel_cell(const float* __restrict__ xyz, size_t i, float inv, int index) {
    const int3 c = voxel_cell(xyz, i, inv);
    return make_int4(c.x, c.y, c.z, index);
}
__host__ __device__ __forceinline__ bool same_cell(const uint4& a, const uint4& b) { return a.x == b.x && a.y == b.y && a.z == b.z; }   // of two sort records (cell, index)

// 2. The reference's key hash (registration.cpp:20-27) over the three per-axis hashes hx, hy, hz = std::hash<int> of the cell ...
__host__ __device__ __forceinline__ unsigned long long voxel_key_combine(unsigned long long hx, unsigned long long hy, unsigned long long hz) {
    unsigned long long h = hx;
    h ^= hy + 0x9e3779b9ull + (h << 6) + (h >> 2);
    h ^= hz + 0x9e3779b9ull + (h << 6) + (h >> 2);
    return h;
}
// ... with libstdc++'s std::hash<int>, which is static_cast<size_t>(value): the int sign-extended to 64 bits.  (The real
// std::unordered_map of voxel_order.hip calls std::hash<int> itself and so agrees with this wherever the library is libstdc++.)
__host__ __device__ __forceinline__ unsigned long long voxel_key_code(int x, int y, int z) {
    return voxel_key_combine((unsigned long long)(long long)x, (unsigned long long)(long long)y, (unsigned long long)(long long)z);
}

// 3. Rows of three floats: row s of src to row p of dst; null arrays (a cloud without that companion) are skipped
__host__ __device__ __forceinline__ void copy_row3(float* __restrict__ dst, size_t p, const float* __restrict__ src, size_t s) {
    dst[3 * p] = src[3 * s]; dst[3 * p + 1] = src[3 * s + 1]; dst[3 * p + 2] = src[3 * s + 2];
}
__host__ __device__ __forceinline__ void copy_row3_opt(float* __restrict__ dst, size_t p, const float* __restrict__ src, size_t s) {
    if (src && dst) copy_row3(dst, p, src, s);
}

// A voxel's normal (include/tdv_hip.h, tdv_voxel_downsample_normals): the mean of its members' normals - the colours' expression, f32
// sums in ascending input index divided by (float)count - brought to unit length in f32 without contraction, the squared length in the
// reference's three-term order (sorted_cloud.hpp: d2_sum<D2::REF>).  A mean of length 0 (normals that cancel) or of a length that is
// not finite (a NaN or infinite member, an overflowing square) stays as it is.
__host__ __device__ __forceinline__ void voxel_unit_normal(float& mx, float& my, float& mz) {
    const float l2 = mx * mx + (my * my + mz * mz);
    const float l = sqrtf(l2);
    if (l2 > 0.f && l <= 3.402823466e+38f /* FLT_MAX */) { mx = mx / l; my = my / l; mz = mz / l; }
}

// 4. A voxel's mean: f32 sums that start at 0 (a lone -0 becomes +0, as there) over the members IN ASCENDING INPUT INDEX, divided by
// (float)count (the caller's: every path knows or counts its members anyway).  Points always; colours when the cloud has them (rgb
// not null, and an array to receive them); normals when NRM, and then brought to unit length.  The caller adds the members in
// ascending index order - that order is what every grouping path exists for.
template <bool NRM>
struct VoxelSum {
    float ax = 0.f, ay = 0.f, az = 0.f, cr = 0.f, cg = 0.f, cb = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
    __host__ __device__ __forceinline__ void add_point(float x, float y, float z) { ax += x; ay += y; az += z; }   // registration.cpp:47-50
    __host__ __device__ __forceinline__ void add(const float* __restrict__ xyz, const float* __restrict__ rgb, const float* __restrict__ nrm, size_t idx) {
        add_point(xyz[3 * idx], xyz[3 * idx + 1], xyz[3 * idx + 2]);
        if (rgb) { cr += rgb[3 * idx]; cg += rgb[3 * idx + 1]; cb += rgb[3 * idx + 2]; }
        if (NRM) { nx += nrm[3 * idx]; ny += nrm[3 * idx + 1]; nz += nrm[3 * idx + 2]; }
    }
    // the mean of the `count` members added, into row `slot` of the outputs (rgb: whether colours were summed)
    __host__ __device__ __forceinline__ void emit(int count, float* __restrict__ out_xyz, float* __restrict__ out_rgb, float* __restrict__ out_nrm, bool rgb, size_t slot) const {
        const float fn = (float)count;
        out_xyz[3 * slot] = ax / fn; out_xyz[3 * slot + 1] = ay / fn; out_xyz[3 * slot + 2] = az / fn;   // registration.cpp:52-53
        if (rgb && out_rgb) { out_rgb[3 * slot] = cr / fn; out_rgb[3 * slot + 1] = cg / fn; out_rgb[3 * slot + 2] = cb / fn; }
        if (NRM) {
            float mx = nx / fn, my = ny / fn, mz = nz / fn;
            voxel_unit_normal(mx, my, mz);
            out_nrm[3 * slot] = mx; out_nrm[3 * slot + 1] = my; out_nrm[3 * slot + 2] = mz;
        }
    }
};

}  // namespace tdv
