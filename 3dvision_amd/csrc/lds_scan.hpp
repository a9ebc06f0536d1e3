// The brute-force nearest-target scan over a model staged in LDS, one lane per source point: what k_icp_small (icp.hip) searches with
// and what k_ppf_score (ppf.hip) scores a batch's poses with.  The scan's answer bit for bit: d2 = dx*dx + (dy*dy + dz*dz) with no
// contraction, targets in ascending order, strict <, the lowest index among equals.
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cmath>

namespace tdv {

__device__ __forceinline__ void transform_point(const float* __restrict__ T, float sx, float sy, float sz,
                                                float& px, float& py, float& pz) {
    // p = R*s + t with each row evaluated as r0*sx + (r1*sy + r2*sz), then + t (column-major T)
    px = (T[0] * sx + (T[4] * sy + T[8] * sz)) + T[12];
    py = (T[1] * sx + (T[5] * sy + T[9] * sz)) + T[13];
    pz = (T[2] * sx + (T[6] * sy + T[10] * sz)) + T[14];
}

// targets into LDS as structure-of-arrays (tx, ty, tz: 16-byte aligned, room for nt rounded up to four), in chunks of four, the last one
// padded with +inf (never a minimum); the caller's barrier follows
__device__ __forceinline__ void lds_stage_targets(const float* __restrict__ tgt, int nt, float* tx, float* ty, float* tz, int threads) {
    const int nt4 = (nt + 3) / 4;
    for (int j = threadIdx.x; j < nt4 * 4; j += threads) {
        const bool in = j < nt;
        tx[j] = in ? tgt[3 * j] : INFINITY; ty[j] = in ? tgt[3 * j + 1] : INFINITY; tz[j] = in ? tgt[3 * j + 2] : INFINITY;
    }
}

// nearest staged target of p: four targets per step (three 16-byte LDS reads at a wave-uniform address): the running minimum and the first
// CHUNK that reached it (strict <), then the lowest target of that chunk with that distance - the scan kernel's two-level argmin.
// best = FLT_MAX, index 0: none (no target, or none at a distance below FLT_MAX).
__device__ __forceinline__ void lds_nearest(float px, float py, float pz, const float* tx, const float* ty, const float* tz, int nt4,
                                            float& best_out, int& idx_out) {
    float best = FLT_MAX; int bc = 0;
    const float4* __restrict__ X4 = reinterpret_cast<const float4*>(tx);
    const float4* __restrict__ Y4 = reinterpret_cast<const float4*>(ty);
    const float4* __restrict__ Z4 = reinterpret_cast<const float4*>(tz);
#pragma unroll 2
    for (int c = 0; c < nt4; ++c) {
        const float4 X = X4[c], Y = Y4[c], Z = Z4[c];
        const float ax = px - X.x, ay = py - Y.x, az = pz - Z.x, bx = px - X.y, by = py - Y.y, bz = pz - Z.y;
        const float cx = px - X.z, cy = py - Y.z, cz = pz - Z.z, ex = px - X.w, ey = py - Y.w, ez = pz - Z.w;
        const float d0 = ax * ax + (ay * ay + az * az), d1 = bx * bx + (by * by + bz * bz);
        const float d2 = cx * cx + (cy * cy + cz * cz), d3 = ex * ex + (ey * ey + ez * ez);
        const float m = fminf(fminf(d0, d1), fminf(d2, d3));
        if (m < best) { best = m; bc = c; }
    }
    int bi = 0;
    if (best < FLT_MAX) {
        bi = 4 * bc;
#pragma unroll
        for (int t = 3; t >= 0; --t) {
            const int j = 4 * bc + t;
            const float dx = px - tx[j], dy = py - ty[j], dz = pz - tz[j];
            if (dx * dx + (dy * dy + dz * dz) == best) bi = j;
        }
    }
    best_out = best; idx_out = best < FLT_MAX ? bi : 0;
}

}  // namespace tdv
