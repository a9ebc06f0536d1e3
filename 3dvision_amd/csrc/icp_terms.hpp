// What point-to-plane ICP and the depth odometry share (icp.hip, odometry.hip), each stated once: the state record of a problem, the
// record of one correspondence (corr_jr, corr_rec), the tree sums' terms formed from it (rec_terms) and the update of one iteration
// from the folded sums (icp_update).  Device code, compiled without contraction (the library's -ffp-contract=off); every caller sees
// the same float steps, so their bits agree.
#pragma once
#include "tdv_internal.hpp"
#include "device_linalg.hpp"

namespace tdv {

// a robust loss as the kernels take it: TDV_ICP_LOSS_HUBER / _TUKEY / _CAUCHY and its scale k (include/tdv_hip.h)
struct IcpLoss { int kind; float scale; };

// the IRLS weight of an accepted correspondence with residual e (f32, no contraction: -ffp-contract=off)
__device__ __forceinline__ float loss_weight(IcpLoss L, float e) {
    const float a = fabsf(e), k = L.scale;
    if (L.kind == TDV_ICP_LOSS_HUBER) return a <= k ? 1.f : k / a;
    const float u = a / k;
    if (L.kind == TDV_ICP_LOSS_TUKEY) {
        const float t = 1.f - u * u;
        return a <= k ? t * t : 0.f;
    }
    return 1.f / (1.f + u * u);   // Cauchy
}

struct IcpState {
    float T[16];       // current transform, column-major
    float res_T[16];   // result.transformation
    float fitness, rmse;
    float rel_fitness, rel_rmse;   // the call's convergence criteria, written when the call initialises the state and never after; icp_update reads
                                   // them where the call's are not the defaults (ICP_RUN_CRITERIA)
    int n_corr;        // accepted correspondences of the last evaluated iteration
    int applied;       // iterations whose update was applied
    int done;          // loop finished (converged / n_corr < 3)
    int iter;          // iterations evaluated
    int last_n_corr_applied;
    int probe_misses;  // lanes that probed the hash table over the call's iterations (the probe cache: grid_nearest); 0 without the cache
};
// How a kernel's iteration ends (the kernels' `fixed_iterations` argument, which only icp_update looks at): bit 0 - run on whatever the
// rule says (benchmarking); bit 1 - the call's criteria are not the defaults, read them from the state.  A call with the default
// criteria takes the reference's rule as a constant and reads nothing more than it did: read in the tail of every iteration, the three
// words cost the one-launch iteration at 200k points 1.2 % (a round trip to memory before the solve's result can be judged); read
// before the block's slab goes out, 7 %; carried from the kernel's start, two SGPRs and with them an occupancy step of a robust
// k_icp_iterate (profiles/r23/icp_multiscale.md).
constexpr int ICP_RUN_FIXED = 1, ICP_RUN_CRITERIA = 2;

// The update of one iteration from the folded sums tot[] (thread 0 of the folding block): registration.cpp:361-411.
// (iter, prev_rmse, Tcur: the state as the kernel read it at its start - no other launch writes it in between - so that the
// tail of the iteration does not begin with another round trip to memory)
// REF (reference-order accumulation, below): tot[] holds float sums; in point-to-point mode tot[2..4] / tot[5..7] are the two
// MEANS (already divided, registration.cpp:380-381) and tot[8..16] the centred cross-covariance of :383-386.
// ROBUST (weighted sums, acc_terms): tot[acc_nv - 1] counts the correspondences of weight > 0, and point-to-point divides by the
// weight sum tot[17] instead of n_corr.
// MODE 3 (GICP) and MODE 4 (colored ICP) solve their systems as point-to-plane does.
// The stopping rule is Open3D's ICPConvergenceCriteria: done iff !fixed_iterations && iter > 0 && |prev_fitness - fitness| < rel_fitness
// && |prev_rmse - rmse| < rel_rmse, prev_* being what the previous applied iteration of this call wrote.  The two bounds are the state's
// (written by init_states, read here and nowhere else); rel_fitness = +inf with rel_rmse = 1e-6f is the reference's rule
// (registration.cpp:406: two finite fitness values always differ by less than +inf), and a call with exactly these runs without
// ICP_RUN_CRITERIA: the constant rule, nothing read.
template <int MODE, bool REF = false, bool ROBUST = false>
__device__ void icp_update(const double* tot, int ns, IcpState* st, int run /* ICP_RUN_* */, int iter, float prev_rmse, const float* Tcur, float* solve_ws /* LDS, 54 words */) {
    const bool fixed_iterations = (run & ICP_RUN_FIXED) != 0;
    static_assert(!(REF && ROBUST), "reference-order sums have no loss");
    static_assert(!(REF && MODE == 3), "reference-order sums have no GICP");
    static_assert(!(REF && MODE == 4), "reference-order sums have no colored ICP");
    const int n_corr = (int)(tot[0] + 0.5);
    st->iter = iter + 1;
    st->n_corr = n_corr;
    if (n_corr < 3 ||  // registration.cpp:361 — break, keeping the previous result
        (ROBUST && (int)(tot[(MODE == 0 || MODE >= 3) ? 29 : 18] + 0.5) < 3)) {   // (the same break when fewer than 3 have a weight: Tukey beyond its scale)
        if (!fixed_iterations) st->done = 1;
        return;
    }
    float delta[16];
    for (int i = 0; i < 16; ++i) delta[i] = 0.f;
    delta[0] = delta[5] = delta[10] = delta[15] = 1.f;
    if (MODE == 0 || MODE >= 3) {
        float ATA[36], nb[6], x[6];
        int k = 2;
        for (int a = 0; a < 6; ++a)
            for (int b = a; b < 6; ++b) { float val = (float)tot[k++]; ATA[a * 6 + b] = val; ATA[b * 6 + a] = val; }
        for (int a = 0; a < 6; ++a) nb[a] = -(float)tot[k++];
        dl::ldlt6_solve(ATA, nb, x, solve_ws);
        dl::Mat3 dR = dl::euler_xyz(x[0], x[1], x[2]);
        for (int c = 0; c < 3; ++c) for (int r = 0; r < 3; ++r) delta[c * 4 + r] = dl::el(dR, r, c);
        delta[12] = x[3]; delta[13] = x[4]; delta[14] = x[5];
    } else {
        const double n = ROBUST ? tot[17] : (double)n_corr;
        double sm[3] = {tot[2], tot[3], tot[4]};
        double tm[3] = {tot[5], tot[6], tot[7]};
        if (!REF) for (int a = 0; a < 3; ++a) { sm[a] /= n; tm[a] /= n; }
        dl::Mat3 H;
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) dl::el(H, a, b) = REF ? (float)tot[8 + a * 3 + b] : (float)(tot[8 + a * 3 + b] - n * sm[a] * tm[b]);
        dl::Mat3 dR = dl::kabsch_rotation(H);
        float smf[3] = {(float)sm[0], (float)sm[1], (float)sm[2]};
        float tmf[3] = {(float)tm[0], (float)tm[1], (float)tm[2]};
        float rx, ry, rz;
        dl::mulv3(dR, smf[0], smf[1], smf[2], rx, ry, rz);
        for (int c = 0; c < 3; ++c) for (int r = 0; r < 3; ++r) delta[c * 4 + r] = dl::el(dR, r, c);
        delta[12] = tmf[0] - rx; delta[13] = tmf[1] - ry; delta[14] = tmf[2] - rz;
    }
    float Tn[16];
    dl::mul44(delta, Tcur, Tn);
    for (int i = 0; i < 16; ++i) { st->T[i] = Tn[i]; st->res_T[i] = Tn[i]; }
    const float rmse = sqrtf((float)tot[1] / (float)n_corr);
    st->rmse = rmse;
    const float fitness = (float)n_corr / (float)ns;
    bool converged;
    if (run & ICP_RUN_CRITERIA) converged = fabsf(st->fitness - fitness) < st->rel_fitness && fabsf(prev_rmse - rmse) < st->rel_rmse;
    else converged = fabsf(prev_rmse - rmse) < 1e-6f;  // registration.cpp:406
    st->fitness = fitness;
    st->applied = iter + 1;
    st->last_n_corr_applied = n_corr;
    if (!fixed_iterations && iter > 0 && converged) st->done = 1;
}

// What a correspondence gathers from the target side, by the target's index: the point q, the normal n (point-to-plane, GICP,
// colored ICP) and colored ICP's (I, d).  icp.hip's corr_fetch fills it from a cloud, odometry.hip from the target frame's maps.
struct CorrTgt { float q[3], n[3]; float4 tc; };

// point-to-plane's J = [p x n | n] (registration.cpp:346-349) and r = (p - q) . n (:351) from the fetched target
__device__ __forceinline__ void corr_jr(float px, float py, float pz, const CorrTgt& G, float* J /* 6 */, float& r) {
    const float nx = G.n[0], ny = G.n[1], nz = G.n[2];
    J[0] = py * nz - pz * ny; J[1] = pz * nx - px * nz; J[2] = px * ny - py * nx; J[3] = nx; J[4] = ny; J[5] = nz;
    const float ex = px - G.q[0], ey = py - G.q[1], ez = pz - G.q[2];
    r = ex * nx + (ey * ny + ez * nz);
}

// The float record of one correspondence at squared distance d2, ref_record's fields: point-to-plane {d2, J0 .. J5, r}, point-to-point
// {d2, px, py, pz, qx, qy, qz, -}.  Everything the tree sums of MODE 0 and 1 need of a correspondence: k_icp_accumulate forms it in
// registers, k_icp_iterate hands it from the lane that searched to the lanes that sum through LDS.
constexpr int REC_WORDS = 8;
struct CorrRec { float f[REC_WORDS]; };
template <int MODE>
__device__ __forceinline__ void corr_rec(float px, float py, float pz, float d2, const CorrTgt& G, CorrRec& R) {
    static_assert(MODE == 0 || MODE == 1, "records exist for point-to-plane and point-to-point");
    R.f[0] = d2;
    if (MODE == 0) corr_jr(px, py, pz, G, R.f + 1, R.f[7]);
    else { R.f[1] = px; R.f[2] = py; R.f[3] = pz; R.f[4] = G.q[0]; R.f[5] = G.q[1]; R.f[6] = G.q[2]; R.f[7] = 0.f; }
}

// The tree sums' terms of MODE 0 and 1 (acc_terms_add below states them) from the record of an accepted correspondence: the one
// place their formulas stand.  A caller that wants a subset of the terms ignores the others in put (k is a constant after unrolling:
// the products nobody takes are not formed).
template <int MODE, bool ROBUST, class Put>
__device__ __forceinline__ void rec_terms(const CorrRec& R, IcpLoss L, Put put) {
    static_assert(MODE == 0 || MODE == 1, "records exist for point-to-plane and point-to-point");
    const float d2 = R.f[0];
    put(0, 1.0); put(1, (double)d2);
    float w = 1.f;
    if (ROBUST) w = loss_weight(L, MODE == 0 ? R.f[7] : sqrtf(d2));
    const double wd = w;
    if (MODE == 0) {
        const float* J = R.f + 1;
        const float r = R.f[7];
        int k = 2;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b) put(k++, ROBUST ? wd * (double)(J[a] * J[b]) : (double)(J[a] * J[b]));
#pragma unroll
        for (int a = 0; a < 6; ++a) put(k++, ROBUST ? wd * (double)(J[a] * r) : (double)(J[a] * r));
        if (ROBUST) put(29, w > 0.f ? 1.0 : 0.0);
    } else {
        const double P[3] = {R.f[1], R.f[2], R.f[3]}, Q[3] = {R.f[4], R.f[5], R.f[6]};
        if (ROBUST) {
            put(2, wd * P[0]); put(3, wd * P[1]); put(4, wd * P[2]);
            put(5, wd * Q[0]); put(6, wd * Q[1]); put(7, wd * Q[2]);
        } else {
            put(2, P[0]); put(3, P[1]); put(4, P[2]);
            put(5, Q[0]); put(6, Q[1]); put(7, Q[2]);
        }
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) put(8 + a * 3 + b, ROBUST ? wd * (P[a] * Q[b]) : P[a] * Q[b]);
        if (ROBUST) { put(17, wd); put(18, w > 0.f ? 1.0 : 0.0); }
    }
}

}  // namespace tdv
