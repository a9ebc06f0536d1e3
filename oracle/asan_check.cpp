// ORACLE — TEST INFRASTRUCTURE ONLY.  Sanitizer driver: exercises every oracle entry point on small random inputs
// in a binary built with -fsanitize=address,undefined (GPU sanitizers are not available on the pool; the CPU
// restatement is where memory/UB bugs in the checker itself would hide).  Run by tests/test_oracle_sanitizers.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <cmath>
extern "C" {
void orc_depth_preprocess(const uint16_t*, const uint8_t*, int, int, float, float*);
int orc_unproject(const float*, const uint8_t*, int, int, float, float, float, float, float, float*, float*);
int orc_voxel_downsample(const float*, const float*, int, float, float*, float*, int*, int);
void orc_estimate_normals(const float*, int, int, float*, int*);
void orc_compute_fpfh(const float*, const float*, int, float, float*, int*, int*);
void orc_feature_match(const float*, int, const float*, int, int*);
void orc_ransac(const float*, int, const float*, int, const float*, const float*, const int*, float, int, float, float*, float*, float*, int*, int*, int*, int*);
int orc_icp(const float*, int, const float*, const float*, int, const float*, float, int, int, float*, float*, float*, float*);
int orc_icp_criteria(const float*, int, const float*, const float*, int, const float*, float, int, int, float*, float*, float*, float*, int, int*, float, float);
void orc_bilateral_filter(const float*, float*, int, int, float, float);
int orc_filter_duplicates(const float*, int, float, float*);
void orc_demo_scene(int, int, float, uint16_t*, uint8_t*);
void orc_demo_mask(int, int, uint8_t*);
int orc_demo_model(float*, float*, int);
void orc_jacobi_svd3_batch(int, const float*, float*, float*, float*, int*);
void orc_kabsch_rotation_batch(int, const float*, float*);
void orc_self_adjoint_eig3_batch(int, const float*, float*, float*, int*, int*);
void orc_ldlt6_solve_batch(int, const float*, const float*, float*);
void orc_euler_xyz_matrix_batch(int, const float*, float*);
void orc_mul44_batch(int, const float*, const float*, float*);
void orc_hypothesis_from_pairs_batch(int, const float*, const float*, float*);
int orc_libm_f32_batch(int, long long, const float*, const float*, float*);
}
static float frand() { return (float)rand() / (float)RAND_MAX; }
int main() {
    srand(7);
    const int w = 64, h = 48;
    std::vector<uint16_t> raw(w * h); std::vector<uint8_t> mask(w * h), bgr(w * h * 3);
    orc_demo_scene(w, h, 1000.f, raw.data(), bgr.data()); orc_demo_mask(w, h, mask.data());
    for (auto& m : mask) m = (uint8_t)(rand() % 256);
    std::vector<float> depth(w * h), filt(w * h), xyz(w * h * 3), rgb(w * h * 3);
    orc_depth_preprocess(raw.data(), mask.data(), w, h, 1000.f, depth.data());
    orc_bilateral_filter(depth.data(), filt.data(), w, h, 1.5f, 0.05f);
    int n = orc_unproject(depth.data(), bgr.data(), w, h, 60.f, 60.f, 32.f, 24.f, 1.5f, xyz.data(), rgb.data());
    if (n <= 0) { n = 300; for (int i = 0; i < n * 3; ++i) xyz[i] = frand(); }
    std::vector<float> vx(n * 3), vc(n * 3); std::vector<int> first(n);
    int m = orc_voxel_downsample(xyz.data(), rgb.data(), n, 0.02f, vx.data(), vc.data(), first.data(), n);
    // poisoned coordinates: NaN, +-inf and cells outside int range (the x86 rule: all of them key INT_MIN)
    const float poison[6] = {NAN, INFINITY, -INFINITY, 3e7f, -3e7f, 1e19f};
    std::vector<float> pz(xyz.begin(), xyz.begin() + n * 3);
    for (int i = 0; i < 6 && i < n; ++i) pz[3 * i + i % 3] = poison[i];
    m += orc_voxel_downsample(pz.data(), rgb.data(), n, 0.01f, vx.data(), vc.data(), first.data(), n);
    const int ns = 400, nt = 300;
    std::vector<float> src(ns * 3), tgt(nt * 3), nrm(nt * 3), fs(ns * 33), ft(nt * 33), desc(nt * 33);
    for (auto& v : src) v = frand(); for (auto& v : tgt) v = frand();
    for (auto& v : fs) v = frand(); for (auto& v : ft) v = frand();
    std::vector<int> knn(nt * 30), nb(nt * 100), cnt(nt), corr(ns), trace(200);
    orc_estimate_normals(tgt.data(), nt, 30, nrm.data(), knn.data());
    orc_compute_fpfh(tgt.data(), nrm.data(), nt, 0.2f, desc.data(), nb.data(), cnt.data());
    // poisoned normals: +-inf, NaN, 1e19 and length-3e4 normals put the bins' casts at NaN and outside int range (the x86 rule)
    {
        std::vector<float> pn(nrm);
        const float npoison[5] = {INFINITY, -INFINITY, NAN, 1e19f, 3e4f};
        for (int i = 0; i < nt; i += 2) pn[3 * i + (i / 2) % 3] = npoison[(i / 2) % 5];
        orc_compute_fpfh(tgt.data(), pn.data(), nt, 0.2f, desc.data(), nb.data(), cnt.data());
    }
    orc_feature_match(fs.data(), ns, ft.data(), nt, corr.data());
    float T[16], fit, rmse; int bi, ir;
    orc_ransac(src.data(), ns, tgt.data(), nt, fs.data(), ft.data(), nullptr, 0.05f, 200, 0.999f, T, &fit, &rmse, trace.data(), corr.data(), &bi, &ir);
    float I[16] = {1,0,0,0, 0,1,0,0, 0,0,1,0, 0,0,0,1}, To[16];
    std::vector<float> tr(20 * 20);
    int it = orc_icp(src.data(), ns, tgt.data(), nrm.data(), nt, I, 0.2f, 20, 1, To, &fit, &rmse, tr.data());
    it += orc_icp(src.data(), ns, tgt.data(), nullptr, nt, I, 0.2f, 20, 1, To, &fit, &rmse, tr.data());
    int amb = 0;
    it += orc_icp_criteria(src.data(), ns, tgt.data(), nrm.data(), nt, I, 0.2f, 20, 1, To, &fit, &rmse, tr.data(), 1, &amb, 1e-2f, 1e-4f);
    std::vector<float> poses(16 * 10), kept(16 * 10);
    for (int p = 0; p < 10; ++p) { for (int i = 0; i < 16; ++i) poses[16 * p + i] = I[i]; poses[16 * p + 12] = 0.05f * (p % 4); }
    int k = orc_filter_duplicates(poses.data(), 10, 0.1f, kept.data());
    std::vector<float> mx(3 * 2000), mn(3 * 2000);
    int nm = orc_demo_model(mx.data(), mn.data(), 2000);
    // the batch solver exports, poisoned entries included
    {
        const int nb = 64;
        std::vector<float> A9(nb * 9), U(nb * 9), S(nb * 3), V(nb * 9), w(nb * 3), A36(nb * 36), b6(nb * 6), x6(nb * 6), abg(nb * 3), A16(nb * 16), B16(nb * 16), C16(nb * 16), lm(nb * 3);
        std::vector<int> sw(nb), rc(nb), qr(nb);
        for (auto& v : A9) v = frand() - 0.5f; for (auto& v : A36) v = frand() - 0.5f; for (auto& v : b6) v = frand();
        for (auto& v : abg) v = 300.f * (frand() - 0.5f); for (auto& v : A16) v = frand(); for (auto& v : B16) v = frand();
        for (int i = 0; i < 6; ++i) { A9[9 * i + i] = poison[i % 3]; A36[36 * (i + 8) + 7 * i] = poison[i % 3]; abg[3 * i] = poison[i % 3]; A16[16 * i + i] = poison[i % 3]; }
        for (int i = 0; i < 9; ++i) A9[9 * 10 + i] = 0.f;
        orc_jacobi_svd3_batch(nb, A9.data(), U.data(), S.data(), V.data(), sw.data());
        orc_kabsch_rotation_batch(nb, A9.data(), U.data());
        orc_self_adjoint_eig3_batch(nb, A9.data(), w.data(), V.data(), rc.data(), qr.data());
        orc_ldlt6_solve_batch(nb, A36.data(), b6.data(), x6.data());
        orc_euler_xyz_matrix_batch(nb, abg.data(), U.data());
        orc_mul44_batch(nb, A16.data(), B16.data(), C16.data());
        orc_hypothesis_from_pairs_batch(nb / 2, A9.data(), A9.data() + 9 * (nb / 2), C16.data());
        for (int op = 0; op < 4; ++op) it += orc_libm_f32_batch(op, nb * 3, abg.data(), A9.data(), lm.data());
        it += sw[0] - sw[0] + qr[1] - qr[1];
    }
    printf("asan_check ok: cloud %d voxels %d ransac best %d icp iters %d kept %d model %d\n", n, m, bi, it, k, nm);
    return 0;
}
