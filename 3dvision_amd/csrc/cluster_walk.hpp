// The radius walk over a curve-ordered cloud (knn.hip: spatial_sort_cloud), one wave per query, shared by the kernels that count or
// visit the neighbours within eps of a point: cluster.hip (k_cluster_count, k_cluster_link) and outlier.hip (k_outlier_count).  The
// distance is rule 1 of tdv_cluster_dbscan (include/tdv_hip.h).  Device code only; include after `#pragma clang fp contract(off)`.
#pragma once
#include "tdv_internal.hpp"

namespace tdv {

namespace {   // per translation unit, as the kernels that use it

struct ClusterCloud { const float *sx, *sy, *sz; const int* orig; const float *lbox, *tbox; int n, n_leaf, n_top; };

// Lower bound of d2 = (dx*dx + dy*dy) + dz*dz between the query q and any point of box idx: per-axis gaps by one f32 subtraction each,
// then the same expression tree.  f32 subtraction, multiplication and addition are monotone under round-to-nearest, so the bound never
// exceeds the d2 of a point in the box.  NaN gaps count as 0 (fmaxf): such a box is looked at.
__device__ __forceinline__ float cluster_box_bound(const float* __restrict__ box, int count, int idx, float qx, float qy, float qz) {
    const float q[3] = {qx, qy, qz};
    float g[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float bmin = box[(size_t)a * count + idx], bmax = box[(size_t)(3 + a) * count + idx];
        g[a] = fmaxf(0.f, fmaxf(bmin - q[a], q[a] - bmax));
    }
    return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
}

// on_leaf(leaf) for every leaf whose box may hold a point within eps2 of q, until it returns true.  Wave-uniform control flow.
template <class F>
__device__ __forceinline__ void cluster_walk(const ClusterCloud& c, float qx, float qy, float qz, float eps2, int lane, F&& on_leaf) {
    for (int tb = 0; tb < c.n_top; tb += 64) {
        const int t = tb + lane;
        unsigned long long tmask = __ballot(t < c.n_top && cluster_box_bound(c.tbox, c.n_top, min(t, c.n_top - 1), qx, qy, qz) <= eps2);
        while (tmask) {
            const int bt = __ffsll((long long)tmask) - 1;
            tmask &= tmask - 1;
            const int u = (tb + bt) * 64 + lane;
            unsigned long long lmask = __ballot(u < c.n_leaf && cluster_box_bound(c.lbox, c.n_leaf, min(u, c.n_leaf - 1), qx, qy, qz) <= eps2);
            while (lmask) {
                const int bl = __ffsll((long long)lmask) - 1;
                lmask &= lmask - 1;
                if (on_leaf((tb + bt) * 64 + bl)) return;
            }
        }
    }
}

__device__ __forceinline__ float cluster_d2(float px, float py, float pz, float qx, float qy, float qz) {
    const float dx = px - qx, dy = py - qy, dz = pz - qz;
    return (dx * dx + dy * dy) + dz * dz;
}

}  // namespace

}  // namespace tdv
