// The pose and the pinhole as every stage that reads depth frames uses them (verify_common.hpp, tsdf.hip, tsdf_raycast.hip,
// odometry.hip), each form stated once with the parenthesisation include/tdv_hip.h writes: the 4 x 4 column-major pose, its two
// products and their rotation-only forms, which of them a pose_direction selects on the way into and out of the camera, rules 2 and 3
// (the projection) and the unprojection by depth_rules.hpp's rule.
#pragma once
#include "tdv_internal.hpp"
#include "depth_rules.hpp"

namespace tdv {

struct Pose16 { float T[16]; };

inline void pose_identity(float* T) { for (int k = 0; k < 16; ++k) T[k] = (k % 5 == 0) ? 1.f : 0.f; }
inline bool pose_direction_ok(int d) { return d == TDV_POSE_SOURCE_ONTO_TARGET || d == TDV_POSE_MODEL_TO_CAMERA; }

// O9's product C = A * B of two column-major poses: each entry the f64 sum of four f64 products in index order, rounded once to f32
inline void pose_chain_product(const float* A, const float* B, float* Cm) {
    for (int j = 0; j < 4; ++j)
        for (int i = 0; i < 4; ++i) {
            double acc = (double)A[i] * (double)B[4 * j];
            for (int q = 1; q < 4; ++q) acc = acc + (double)A[4 * q + i] * (double)B[4 * j + q];
            Cm[4 * j + i] = (float)acc;
        }
}

#ifdef __HIPCC__
__device__ __forceinline__ Pose16 load_pose(const float* __restrict__ poses, int pose) {
    Pose16 p;
    const float* T = poses + (size_t)pose * 16;
#pragma unroll
    for (int k = 0; k < 16; ++k) p.T[k] = T[k];
    return p;
}

// T x: ((T0 x + T4 y) + T8 z) + T12
__device__ __forceinline__ void pose_apply(const Pose16& P, float x, float y, float z, float& o0, float& o1, float& o2) {
    const float* T = P.T;
    o0 = ((T[0] * x + T[4] * y) + T[8] * z) + T[12];
    o1 = ((T[1] * x + T[5] * y) + T[9] * z) + T[13];
    o2 = ((T[2] * x + T[6] * y) + T[10] * z) + T[14];
}
// the rigid inverse R^T (x - t): (T0 d0 + T1 d1) + T2 d2 with d = x - t
__device__ __forceinline__ void pose_apply_inverse(const Pose16& P, float x, float y, float z, float& o0, float& o1, float& o2) {
    const float* T = P.T;
    const float d0 = x - T[12], d1 = y - T[13], d2 = z - T[14];
    o0 = (T[0] * d0 + T[1] * d1) + T[2] * d2;
    o1 = (T[4] * d0 + T[5] * d1) + T[6] * d2;
    o2 = (T[8] * d0 + T[9] * d1) + T[10] * d2;
}
// R g and R^T g: the same two without the translation
__device__ __forceinline__ void pose_rotate(const Pose16& P, float x, float y, float z, float& o0, float& o1, float& o2) {
    const float* T = P.T;
    o0 = (T[0] * x + T[4] * y) + T[8] * z;
    o1 = (T[1] * x + T[5] * y) + T[9] * z;
    o2 = (T[2] * x + T[6] * y) + T[10] * z;
}
__device__ __forceinline__ void pose_rotate_inverse(const Pose16& P, float x, float y, float z, float& o0, float& o1, float& o2) {
    const float* T = P.T;
    o0 = (T[0] * x + T[1] * y) + T[2] * z;
    o1 = (T[4] * x + T[5] * y) + T[6] * z;
    o2 = (T[8] * x + T[9] * y) + T[10] * z;
}

// The direction, read in one place.  TDV_POSE_SOURCE_ONTO_TARGET: the pose takes camera coordinates to the model's (the volume's),
// so a model point enters the camera by the inverse and a camera point leaves it by the product; TDV_POSE_MODEL_TO_CAMERA: the reverse.
// rule 1: the model point m in camera coordinates
__device__ __forceinline__ void pose_into_camera(const Pose16& P, int direction, float m0, float m1, float m2, float& xc, float& yc, float& zc) {
    if (direction == TDV_POSE_SOURCE_ONTO_TARGET) pose_apply_inverse(P, m0, m1, m2, xc, yc, zc);
    else pose_apply(P, m0, m1, m2, xc, yc, zc);
}
// T13: the camera point C in the model's coordinates
__device__ __forceinline__ void pose_out_of_camera(const Pose16& P, int direction, const float* C, float* p) {
    if (direction == TDV_POSE_SOURCE_ONTO_TARGET) pose_apply(P, C[0], C[1], C[2], p[0], p[1], p[2]);
    else pose_apply_inverse(P, C[0], C[1], C[2], p[0], p[1], p[2]);
}
// T18: a direction g of the model's frame in the camera's
__device__ __forceinline__ void rotate_into_camera(const Pose16& P, int direction, const float* g, float& n0, float& n1, float& n2) {
    if (direction == TDV_POSE_SOURCE_ONTO_TARGET) pose_rotate_inverse(P, g[0], g[1], g[2], n0, n1, n2);
    else pose_rotate(P, g[0], g[1], g[2], n0, n1, n2);
}

// rules 2 and 3 of include/tdv_hip.h, as written there, for the camera-space point (xc, yc, zc).  SUB 1: the pixel (u, v) =
// floorf(uf + 0.5f); SUB 16: the mesh's snapped position of rule M1, floorf(uf * 16.0f + 0.5f).  The point is taken by reference:
// by value hipcc orders rule 2's tests differently, and the verifier's tile kernels grow by 9 to 33 instructions (DESIGN.md 7,
// "Depth-frame stages").
template <int SUB>
__device__ __forceinline__ bool pinhole_project(const Pinhole& k, float zmax, const float& xc, const float& yc, const float& zc, int& u, int& v) {
    if (!(fabsf(xc) < INFINITY && fabsf(yc) < INFINITY && zc > 0.f && zc <= zmax && zc < INFINITY)) return false;
    const float uf = (xc * k.fx) / zc + k.cx, vf = (yc * k.fy) / zc + k.cy;
    if (!(fabsf(uf) < 1048576.f && fabsf(vf) < 1048576.f)) return false;          // (false for NaN too)
    if constexpr (SUB == 1) {
        u = (int)floorf(uf + 0.5f);
        v = (int)floorf(vf + 0.5f);
    } else {
        u = (int)floorf(uf * (float)SUB + 0.5f);             // |uf| < 2^20: within +-2^24 at SUB 16
        v = (int)floorf(vf * (float)SUB + 0.5f);
    }
    return true;
}

// O2: the camera-space point of pixel (u, v) at depth z, by depth_rules.hpp's rule with plain divisions
__device__ __forceinline__ void pinhole_vertex(int u, int v, float z, const Pinhole& k, float* out) {
    emit_point((float)u, (float)v, z, k.cx, k.cy, PlainDiv{k.fx, k.fy}, out, (float*)nullptr, (const uint8_t*)nullptr, 0, (size_t)0);
}
#endif

}  // namespace tdv
