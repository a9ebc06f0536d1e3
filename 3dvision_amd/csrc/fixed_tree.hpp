// The fixed f64 summation tree of include/tdv_hip.h (tdv_remove_statistical_outlier, rule 4; tdv_segment_planes; tdv_fgr's means), shared
// by the kernels that sum f64 terms per point of a cloud in index order: outlier.hip (cloud_mean, std_dev), iss.hip (the cloud's
// resolution), plane.hip (the inlier sums), fgr.hip (the clouds' means, first level) and odometry.hip (O7's 29 sums).  The term of point i belongs to workgroup
// i / 256, thread i % 256; a workgroup sum is the shuffle tree over each wave, then (w0 + w1) + (w2 + w3); one workgroup then adds the
// workgroup sums t, t + 256, ... into thread t and sums its 256 threads the same way.  One order, so two calls give the same bits.
// Device code for workgroups of 256 threads, compiled without contraction (the library's -ffp-contract=off).
// Held to that order bit for bit: tests/fixed_tree_restatement.py restates it from the header's text, tests/test_gpu_primitives_probe.py
// compares these functions with it through the study library's probe (probe.hip), tests/test_gpu_outlier.py and test_gpu_iss.py through
// the product entry points.
#pragma once
#include "tdv_internal.hpp"

namespace tdv {

namespace {   // per translation unit, as the kernels that use it

__device__ __forceinline__ double tree_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// f64 sum over the 256 threads of a workgroup in the fixed order (wave shuffles, then the four waves in order); valid in thread 0
__device__ __forceinline__ double tree_block_sum(double v, double* lds4) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
    __syncthreads();
    return (lds4[0] + lds4[1]) + (lds4[2] + lds4[3]);
}

// NV sums at once, each in tree_block_sum's order: the shuffles of all NV, then one trip through LDS (lds: 4 * NV doubles) instead of
// NV; sum k is returned in thread k (k < NV), the other threads get +0.0
template <int NV>
__device__ __forceinline__ double tree_block_sums(double* v, double* lds) {
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < NV; ++k) lds[(threadIdx.x >> 6) * NV + k] = v[k];
    __syncthreads();
    const int t = threadIdx.x;
    return t < NV ? (lds[t] + lds[NV + t]) + (lds[2 * NV + t] + lds[3 * NV + t]) : 0.0;
}

// the largest of a workgroup's 256 values (order-free; fmax: a NaN never wins); valid in thread 0
__device__ __forceinline__ double tree_block_max(double v, double* lds4) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmax(fmax(lds4[0], lds4[1]), fmax(lds4[2], lds4[3]));
}

__device__ __forceinline__ int tree_block_count(int v, int* lds4) {
    v = wave_sum_i32(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
    __syncthreads();
    return (lds4[0] + lds4[1]) + (lds4[2] + lds4[3]);
}

// the nb workgroup sums (counts) added by one workgroup: thread t takes t, t + 256, ... in order, then the block sum; valid in thread 0.
// width, a: workgroup b's sum is entry a of its `width` sums, part[width * b + a]
__device__ __forceinline__ double tree_partials_sum(const double* __restrict__ part, int nb, double* lds4, int width = 1, int a = 0) {
    double v = 0.0;
    for (int b = threadIdx.x; b < nb; b += 256) v += part[(size_t)width * b + a];
    return tree_block_sum(v, lds4);
}

__device__ __forceinline__ int tree_partials_count(const int* __restrict__ cnt, int nb, int* lds4) {
    int c = 0;
    for (int b = threadIdx.x; b < nb; b += 256) c += cnt[b];
    return tree_block_count(c, lds4);
}

}  // namespace

}  // namespace tdv
