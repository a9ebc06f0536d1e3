/*
 * tdv_hip.h — C ABI of the MI355X (gfx950) point-cloud registration backend.
 *
 * This is the drop-in boundary: the thin extern "C" dispatch layer that replaces the
 * reference's CUDA dispatch TU src/gpu_impl.cpp and its launcher set in cuda/ (the .cuh headers)
 * (launchDepthPreprocess, launchDeproject, launchFindCorrespondences,
 * launchBuildLinearSystem).  The C++ adapter in 3dvision_amd/host/ defines the reference's
 * operator API (include/gpu_depth.hpp:9-22, include/gpu_registration.hpp:8-19,
 * include/registration.hpp:32-60) on top of these entry points; INTEGRATION.md shows the
 * binding a maintainer adds.
 *
 * Conventions
 *  - Every function returns a tdv_status (0 = ok, negative = error); nothing throws.
 *  - A tdv_ctx owns one HIP stream, a grow-only device workspace and pinned staging; it is
 *    NOT thread-safe: use one ctx per host thread (the reference calls its GPU ops from up to
 *    8 pool threads, include/thread_pool.hpp:17-33 / src/pipeline.cpp:321-327).
 *  - Host entry points take caller-owned host buffers; "_dev" entry points take device
 *    pointers valid on the ctx's device and enqueue on the ctx's stream.
 *  - Clouds are AoS float[n*3] (bit-identical to std::vector<Eigen::Vector3f>::data()),
 *    FPFH is float[n*33] (std::vector<std::array<float,33>>::data()),
 *    4x4 transforms are COLUMN-MAJOR float[16] (Eigen::Matrix4f::data()).
 *  - Results follow the reference's CPU path src/registration.cpp (the parity oracle), not its
 *    CUDA kernels, where the two differ.
 */
#ifndef TDV_HIP_H
#define TDV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tdv_ctx tdv_ctx;

typedef enum tdv_status {
    TDV_OK = 0,
    TDV_ERR_NO_DEVICE = -1,   /* no HIP device / HIP runtime failure at init                   */
    TDV_ERR_BAD_ARG = -2,     /* null pointer, negative size, capacity too small               */
    TDV_ERR_OOM = -3,         /* device or pinned allocation failed                            */
    TDV_ERR_LAUNCH = -4,      /* kernel launch / stream / copy failure (hipGetLastError)       */
    TDV_ERR_INTERNAL = -5
} tdv_status;

/* ---- lifecycle ---------------------------------------------------------------------------- */
/* Replaces GPUDepth::isCudaAvailable / GPURegistration::isCudaAvailable (src/gpu_impl.cpp:18-26,
 * 131-139): *count = number of HIP devices (0 when none; still TDV_OK). */
int tdv_device_count(int* count);
int tdv_ctx_create(int device, tdv_ctx** out);
/* Use an existing hipStream_t (e.g. torch's current stream) instead of the ctx's own. */
int tdv_ctx_set_stream(tdv_ctx* ctx, void* hip_stream);
void* tdv_ctx_get_stream(tdv_ctx* ctx);
int tdv_ctx_synchronize(tdv_ctx* ctx);
void tdv_ctx_destroy(tdv_ctx* ctx);
/* ICP correspondence search.  The reference's kernel is a brute-force scan (cuda/icp.cu:14-55); the pruned search
 * (bounding-box walk over the Morton-ordered target) and the grid search (hash grid with cells of 2.2 x the acceptance
 * threshold: a neighbour within the threshold lies in 8 cells around the query) return the SAME correspondences bit
 * for bit (exact lower bounds resp. every candidate verified with the scan's distance expression, lowest index on ties)
 * and only differ in time.  AUTO (default; env TDV_ICP_SEARCH=brute|pruned|grid overrides at ctx creation) picks by
 * size and by how many target points a cell holds; GRID falls back to PRUNED when the grid is not usable (threshold
 * large against the point spacing, or coordinates beyond 2^17 cells). */
#define TDV_ICP_SEARCH_AUTO 0
#define TDV_ICP_SEARCH_BRUTE 1
#define TDV_ICP_SEARCH_PRUNED 2
#define TDV_ICP_SEARCH_GRID 3
int tdv_ctx_set_icp_search(tdv_ctx* ctx, int mode);
/* ICP accumulation of the per-iteration sums (n_corr, total_error, ATA, ATb resp. the means and the cross-covariance of the
 * point-to-point branch; src/registration.cpp:340-358,374-386).  The reference adds one correspondence after the other in
 * float, in ascending source index; a float sum depends on its order.
 *   TREE (default)  double accumulators in a fixed tree over the whole chip: ~25 us per iteration at 200k points, the same
 *                   bits run to run, and within ~1e-7 (relative) of the reference's sums - the refined transform agrees with
 *                   the CPU path to the tolerances of DESIGN.md 2, not to the bit.
 *   REFERENCE       the reference's own order and precision: every accepted correspondence's terms are stored as rows and one
 *                   workgroup adds them in index order, one lane per accumulator.  With it transformation, fitness, rmse and
 *                   the iteration count EQUAL the CPU path's (tests/test_gpu_icp_reference_order.py); the cost is a chain of
 *                   n dependent additions per iteration (~0.5 ms at 200k points).  Env TDV_ICP_ACCUMULATE=reference selects
 *                   it at ctx creation; tdv_register_batch_dev honours it for every instance. */
#define TDV_ICP_ACCUMULATE_TREE 0
#define TDV_ICP_ACCUMULATE_REFERENCE 1
int tdv_ctx_set_icp_accumulation(tdv_ctx* ctx, int mode);
/* Launches per ICP iteration, for tests and measurements.  With the hash-grid search, TREE sums and a point-to-plane or point-to-point
 * objective (L2 or a robust loss) a single call's iteration can run as ONE kernel, which searches one lane per source point and forms the
 * sums from per-point records handed over in LDS, in the same f64 tree: the same bits as the TWO launches (search, then accumulation).
 * AUTO (default) takes ONE inside the range of source counts where it measured faster (ICP); TWO and ONE ask for one form.
 * ONE on a path that has no such kernel (GICP, colored ICP, another search, REFERENCE sums, the small-problem loop, batches) runs that
 * path as it is.  tdv_ctx_last_icp_launches: TDV_ICP_LAUNCHES_ONE if the last tdv_icp* / tdv_gicp* / tdv_colored_icp* call on the ctx ran
 * the one-launch kernel, else TDV_ICP_LAUNCHES_TWO (0 before any); TDV_ERR_BAD_ARG for a null ctx, as the setter for a null ctx or an
 * unknown mode.  No environment variable selects it. */
#define TDV_ICP_LAUNCHES_AUTO 0
#define TDV_ICP_LAUNCHES_TWO 1
#define TDV_ICP_LAUNCHES_ONE 2
int tdv_ctx_set_icp_launches(tdv_ctx* ctx, int mode);
int tdv_ctx_last_icp_launches(tdv_ctx* ctx);
/* The probe cache of the hash-grid search, for tests and measurements.  The search probes an open-addressing table for the eight cells
 * around a transformed source point; what it finds there (each cell's list head) depends only on the point's cell, on which side of the
 * cell it sits per axis, and on the table.  With the cache a single call keeps every point's cell key and eight heads in its workspace
 * and takes them in a later iteration whenever the key computed from that iteration's pose is the stored one - then they are the heads
 * the probes would find, so correspondences and every sum keep their bits.  Keys are invalid at the start of every call.  AUTO
 * (default) takes the cache where the one-launch iteration runs, when the call may run four iterations or more (the first only fills
 * the cache; a shorter call measured no faster with it); ON takes it on the single call's grid path in either launch form from two
 * iterations on; OFF never.  A call of one iteration, batches and tdv_register_batch_dev's instances run without it.  tdv_ctx_last_icp_probe_misses: the
 * number of (point, iteration) pairs of the last ICP call on the ctx that probed the table (the rest took cached heads), -1 if the call
 * ran without the cache; TDV_ERR_BAD_ARG for a null ctx, as the setter for a null ctx or an unknown mode. */
#define TDV_ICP_PROBE_CACHE_AUTO 0
#define TDV_ICP_PROBE_CACHE_OFF 1
#define TDV_ICP_PROBE_CACHE_ON 2
int tdv_ctx_set_icp_probe_cache(tdv_ctx* ctx, int mode);
int tdv_ctx_last_icp_probe_misses(tdv_ctx* ctx);
/* ICP robust loss: iteratively reweighted least squares, one weight w per accepted correspondence (d2 <= thr^2, unchanged), set
 * per ctx and honoured by tdv_icp, tdv_icp_dev, tdv_icp_batch_dev, tdv_refine_batch_dev and tdv_register_batch_dev (batch lanes
 * included).  tdv_icp_correspondences is unaffected.  L2 (default) gives every accepted correspondence weight 1: today's results,
 * bit for bit.
 *   Residual e: point-to-plane the signed r = (p - q) . n the sums use; point-to-point e = sqrtf(d2).
 *   Weight, in f32 without contraction, a = |e|, k = scale:
 *     HUBER   w = a <= k ? 1 : k / a
 *     TUKEY   w = a <= k ? t * t : 0,  t = 1 - u * u,  u = a / k
 *     CAUCHY  w = 1 / (1 + u * u),     u = a / k
 *   Point-to-plane sums: (double)w * (double)(J[a] * J[b]) and (double)w * (double)(J[a] * r) - exact products in f64.
 *   Point-to-point (weighted Kabsch): W = sum (double)w, sums of (double)w * (double)p[a] and (double)w * (double)q[a] (exact),
 *   and of (double)w * ((double)p[a] * (double)q[b]) (the f64 product of p and q is exact; the one rounding is the product with w);
 *   means sm = sum w p / W, tm = sum w q / W and H = f32(sum w p q^T - (W * sm[a]) * tm[b]), all in f64.
 *   Unweighted, as with L2: n_corr, fitness = n_corr / ns, rmse = sqrt(sum d2 / n_corr) and the stopping rule |delta rmse| < 1e-6.
 *   An iteration where fewer than 3 accepted correspondences have w > 0 (Tukey only) breaks as n_corr < 3 does: the pose is kept,
 *   and with fixed_iterations the loop goes on.
 *   A non-finite residual or term has no special case: w follows the formulas above (an infinite e gives w = 0, a NaN e gives NaN
 *   except Tukey's 0) and its products still enter the sums, so 0 * inf is NaN there, and a sum with an infinite product (and no
 *   NaN, no infinity of the other sign) is that infinity.
 * An unknown loss, or a scale that is not finite and > 0 for a non-L2 loss, returns TDV_ERR_BAD_ARG and leaves the setting as it
 * was; L2 ignores scale (and reads back 0).  No environment variable selects a loss.  Reference-order accumulation reproduces the
 * reference's float sums, which have no loss: with TDV_ICP_ACCUMULATE_REFERENCE and a non-L2 loss, the five ICP entry points above
 * return TDV_ERR_BAD_ARG before anything is enqueued or written, with the reason in tdv_last_error. */
#define TDV_ICP_LOSS_L2 0
#define TDV_ICP_LOSS_HUBER 1
#define TDV_ICP_LOSS_TUKEY 2
#define TDV_ICP_LOSS_CAUCHY 3
int tdv_ctx_set_icp_loss(tdv_ctx* ctx, int loss, float scale);
int tdv_ctx_get_icp_loss(tdv_ctx* ctx, int* loss, float* scale);
/* RANSAC hypothesis scoring.  FAST (default; env TDV_RANSAC_SCORE=exact overrides) evaluates every (hypothesis, point) with
 * fused multiply-adds and re-scores, with the reference's unfused arithmetic, every chunk of points in which a distance
 * falls inside the rounding band where the two could disagree: the inlier counts are those of EXACT, which runs the
 * reference's arithmetic only (registration.cpp:270-279). */
#define TDV_RANSAC_SCORE_FAST 0
#define TDV_RANSAC_SCORE_EXACT 1
#define TDV_RANSAC_SCORE_MATRIX 2 /* A/B variant kept in the STUDY library only (lib3dvision_hip_study.so): the transform on the
                                   * matrix cores (f32 MFMA), same band scheme, same counts; measured slower than FAST.  The product
                                   * library returns TDV_ERR_BAD_ARG for it */
int tdv_ctx_set_ransac_score(tdv_ctx* ctx, int mode);
/* The order of the leaves that RANSAC's leaf-box bound walks (a call with bail-out and bound).  MORTON: along the pairs' Morton
 * curve.  CLASSES: class-major - the outliers of the ordering pose first, its inliers behind them, each class along its own Morton
 * curve; tighter leaves, a shorter fine list.  AUTO (default): CLASSES for a call with at least 50,000 pairs, MORTON below.  The
 * order changes which hypotheses the bound proves dead before they are scored, never a result. */
#define TDV_RANSAC_LEAVES_AUTO 0
#define TDV_RANSAC_LEAVES_MORTON 1
#define TDV_RANSAC_LEAVES_CLASSES 2
int tdv_ctx_set_ransac_leaf_order(tdv_ctx* ctx, int mode);
/* How a RANSAC batch's index triples, which the host draws into pinned memory, reach the device.  DIRECT: the batch's hypothesis
 * kernel reads them from the host's memory.  STAGED: the host draws a batch further ahead and the leaf-box bound's coarse level of
 * the batch before carries them to the device while it walks, so the hypothesis kernel finds them there - in a call with bail-out
 * and bound (more than 16,384 iterations, no trace) whose triples pack into one word (at most 2^21 pairs), for every batch behind
 * the second; every other batch and call reads directly whatever the mode.  AUTO (default): STAGED.  Same results either way.
 * tdv_ctx_last_ransac_staged: how many batches of the last tdv_ransac* call on this ctx, of those its loop reached, ran from staged
 * triples (0 before any). */
#define TDV_RANSAC_TRIPLES_AUTO 0
#define TDV_RANSAC_TRIPLES_DIRECT 1
#define TDV_RANSAC_TRIPLES_STAGED 2
int tdv_ctx_set_ransac_triples(tdv_ctx* ctx, int mode);
int tdv_ctx_last_ransac_staged(tdv_ctx* ctx);
/* Statistics of the last tdv_ransac* call on this ctx: the fraction of the (hypothesis, point) tests the FAST pass scored a second time
 * with the reference arithmetic - whole waves of 64 hypotheses on a pair of points that one of them has inside its rounding band
 * (until round 4: on the whole 8-point chunk) - (-1 if the call ran in EXACT mode or none has run). */
double tdv_ctx_last_ransac_rescore(tdv_ctx* ctx);
/* The share of the (hypothesis, point) tests the last tdv_ransac* call on this ctx evaluated.  Below 1 when the call ran without
 * a per-iteration trace: a hypothesis whose count over a prefix of the points plus ALL remaining points cannot exceed the best
 * count of the earlier batches is not scored further — the loop of registration.cpp:284-290 only asks whether a count beats the
 * best so far, so transform, inlier count, fitness, rmse and best iteration are unchanged (env TDV_RANSAC_BAILOUT=0 turns it off). */
double tdv_ctx_last_ransac_scored(tdv_ctx* ctx);
/* The search the last tdv_icp* / tdv_icp_correspondences call on this ctx ran (BRUTE, PRUNED or GRID; 0 before any). */
int tdv_ctx_last_icp_search(tdv_ctx* ctx);
/* The search the last tdv_feature_match* call on this ctx ran (0 before any): the reference's scan (small sets), the leaf-major
 * search over the packed index, or the per-source walk of that index the leaf-major search hands over to when the descriptors
 * have no structure (its pair pool would run over).  Same correspondences every way. */
#define TDV_FM_PATH_SCAN 1
#define TDV_FM_PATH_LEAF_MAJOR 2
#define TDV_FM_PATH_WALK 3
int tdv_ctx_last_feature_match_path(tdv_ctx* ctx);
/* How the last tdv_register_batch_dev / tdv_voxel_downsample_batch_dev call on this ctx grouped its points into voxels (0 before any):
 * TABLE = a hash table over all clouds (any cloud), PIXELS = pixel windows in LDS, without the table - for clouds the call itself unprojected
 * from a depth image (row-major pixel order, known intrinsics); it hands over to TABLE when a tile is not covered (coarse voxels, rows longer
 * than its halo).  Same voxels, means and orders either way; TDV_VOXEL_PIXELS=0 forces TABLE (parity tests). */
#define TDV_VOXEL_GROUPING_TABLE 1
#define TDV_VOXEL_GROUPING_PIXELS 2
int tdv_ctx_last_voxel_grouping(tdv_ctx* ctx);
/* Whether the last batched voxel pass on this ctx (tdv_voxel_downsample_batch*_dev, tdv_register_batch_dev, a voxelised level of
 * tdv_icp_multiscale_batch_dev - there the last such level) kept its result (0) or found a voxel of more points than the table's member
 * rows hold (16) and was redone cloud by cloud (1); -1 before any.  Same voxels either way.  TDV_ERR_BAD_ARG for a NULL ctx. */
int tdv_ctx_last_voxel_batch_redone(tdv_ctx* ctx);
/* Host lanes (the caller's thread + helper threads) the last tdv_register_batch_dev call on this ctx used (0 before any). */
int tdv_ctx_last_batch_lanes(tdv_ctx* ctx);
/* Device memory this ctx holds in its grow-only workspace arenas, its batch lanes' included: the high-water mark of every
 * call made on it so far (the arena never shrinks; steady state allocates nothing). */
unsigned long long tdv_ctx_workspace_bytes(tdv_ctx* ctx);
/* Test aid: sets every byte of every workspace arena block this ctx holds, and of every batch lane's, to `byte` (on each
 * one's stream, then waits for it), and every byte of their pinned host staging as well.  A call's outputs are a function of its
 * arguments and the ctx's settings only, so a call made after this gives the bytes it gives on a fresh ctx
 * (tests/test_gpu_ctx_state.py).  The persistent device words - the last-workgroup tickets and the chained scan's status words
 * with its epoch and ticket base - are NOT touched: they carry an invariant from one call to the next (every kernel that uses a
 * ticket leaves it at zero; a status word is told apart by its epoch), and a kernel that waits on them would wait for ever.
 * The ctx must be idle.  A NULL ctx or a byte outside 0..255 returns TDV_ERR_BAD_ARG.  Not for production use. */
int tdv_ctx_workspace_fill(tdv_ctx* ctx, int byte);
const char* tdv_status_string(int status);
/* Text of the last HIP error seen by this ctx ("" if none). */
const char* tdv_last_error(tdv_ctx* ctx);
const char* tdv_version(void);

/* Kernel timing (HIP events on the ctx's stream around the dominant kernels).  Slots:
 * 0 = ICP nearest-neighbour scan, 1 = RANSAC scoring, 2 = feature match, 3 = kNN scan,
 * 4 = radius scan, 5 = depth+unproject, 6 = voxel, 7 = descriptor index.  Enabling adds one event pair per launch.
 * Slot 1 is read without events where the fast scoring kernel runs (tdv_ransac* in its default mode): every dispatch stamps
 * the device's constant-rate clock itself, and its time is the first workgroup's start to the last workgroup's end - inside the
 * dispatch, so a little below what two events around it read (they read from one queue marker to the next), and without the
 * idle time an event record puts between two kernels.  The exact kernel and the batched small-cloud pass stay on events. */
#define TDV_TIMER_ICP_NN 0
#define TDV_TIMER_RANSAC_SCORE 1
#define TDV_TIMER_FEATURE_MATCH 2
#define TDV_TIMER_KNN 3
#define TDV_TIMER_RADIUS 4
#define TDV_TIMER_DEPTH 5
#define TDV_TIMER_VOXEL 6
#define TDV_TIMER_FM_INDEX 7   /* packing of the target descriptors (once per model in the batched chain) */
#define TDV_TIMER_COUNT 8
int tdv_timing_enable(tdv_ctx* ctx, int on);
/* Synchronizes the stream, then returns accumulated milliseconds and launch count; resets the slot. */
int tdv_timing_read(tdv_ctx* ctx, int slot, double* total_ms, int* launches);

/* ---- R1: depth scale + mask --------------------------------------------------------------- */
/* Replaces GPUDepth::preprocess (src/gpu_impl.cpp:28-66, kernel cuda/depth_processing.cu:10-30);
 * oracle = the CPU branch src/pipeline.cpp:46-54.
 * out[i] = float(raw[i]) * float(1.0 / scale); zeroed where the mask rejects the pixel.
 * mask may be NULL (no masking).  mask_mode: 0 = reference CPU semantics (keep mask > 10),
 * 1 = reference CUDA semantics (keep mask != 0). */
#define TDV_MASK_THRESHOLD10 0
#define TDV_MASK_NONZERO 1
/* label image: keep pixels whose mask value equals `label` (1..255): pass
 * TDV_MASK_LABEL_BASE + label.  One u8 image then serves every instance of a scene instead of one
 * full-frame mask per instance (src/pipeline.cpp:251-257, src/segmentation.cpp:12-42 produce those). */
#define TDV_MASK_LABEL_BASE 256
int tdv_depth_preprocess(tdv_ctx* ctx, const uint16_t* raw, const uint8_t* mask, int width, int height,
                         float scale, int mask_mode, float* out_depth);

/* Bilateral depth filter: the reference's kernel cuda/depth_processing.cu:62-122 /
 * launcher :124-155, which its dispatch never calls (config flag depth.bilateral_filter is parsed at
 * src/main.cpp:24 and never read).  in/out: float depth images; zero depths stay zero. */
int tdv_bilateral_filter(tdv_ctx* ctx, const float* depth, int width, int height, float sigma_spatial, float sigma_range,
                         float* out_depth);

/* ---- R2: unprojection --------------------------------------------------------------------- */
/* Replaces GPUPointCloud::generate (src/gpu_impl.cpp:69-128, kernel cuda/pointcloud.cu:11-51);
 * oracle = src/pipeline.cpp:61-84.  Keeps 0 < z <= zmax, x = (u-cx)*z/fx, y = (v-cy)*z/fy,
 * colour = BGR->RGB / 255.  Output order is the CPU's ROW-MAJOR scan order (deterministic; the
 * reference CUDA kernel's global-atomic order is not reproduced).  bgr / out_rgb may be NULL.
 * capacity = room in out_xyz/out_rgb in points; *n_out = points produced (TDV_ERR_BAD_ARG and
 * *n_out set to the needed count if capacity is too small). */
int tdv_deproject(tdv_ctx* ctx, const float* depth, const uint8_t* bgr, int width, int height,
                  float fx, float fy, float cx, float cy, float zmax,
                  float* out_xyz, float* out_rgb, int capacity, int* n_out);
/* Fused R1+R2 (one pass over the frame, no intermediate depth image on the host). */
int tdv_depth_to_cloud(tdv_ctx* ctx, const uint16_t* raw, const uint8_t* mask, const uint8_t* bgr,
                       int width, int height, float scale, int mask_mode,
                       float fx, float fy, float cx, float cy, float zmax,
                       float* out_xyz, float* out_rgb, int capacity, int* n_out);

/* All instances of a scene in two launches: n_instances masks — stacked u8 images
 * (mask_format 0, mask_mode as above), ONE u8 label image with label b+1 for instance b (mask_format 1, <= 255 instances) or ONE u16 label image, same rule (mask_format 2, <= 65535 instances; label images: one frame
 * only) — give n_instances clouds stored back to back, each in row-major pixel order.
 * Frames: d_raw (and d_bgr) hold n_frames images back to back (n_frames <= 1: one frame shared by every instance, the
 * reference's case, src/pipeline.cpp:321-327); instance b reads frame h_frame_of_instance[b] (host array), or, when that
 * is NULL, frame b * n_frames / n_instances (equal contiguous groups; n_frames == n_instances: one frame each).
 * All pointers are device pointers except h_frame_of_instance and h_offsets (host, n_instances + 1 entries): instance b
 * occupies points [h_offsets[b], h_offsets[b+1]).  capacity = room in d_xyz/d_rgb in points; if the total exceeds it
 * the call returns TDV_ERR_BAD_ARG with h_offsets filled (so the caller can size the buffers and call again). */
int tdv_depth_to_cloud_batch_dev(tdv_ctx* ctx, const uint16_t* d_raw, const uint8_t* d_masks, const uint8_t* d_bgr,
                                 int n_instances, int mask_format, int n_frames, const int* h_frame_of_instance,
                                 int width, int height, float scale, int mask_mode,
                                 float fx, float fy, float cx, float cy, float zmax,
                                 float* d_xyz, float* d_rgb, long long capacity, int* h_offsets);

/* ---- R3: voxel downsample ----------------------------------------------------------------- */
/* Replaces Registration::voxelDownsample (src/registration.cpp:29-60).  Per-voxel mean of points
 * (and colours) summed in ascending input index, divided by the count; normals are dropped.
 * order: TDV_VOXEL_ORDER_FIRST = voxels ordered by their smallest input index (deterministic,
 * computed on the GPU); TDV_VOXEL_ORDER_REFERENCE = libstdc++ std::unordered_map iteration order
 * of the reference (the slot order is replayed on the host with the reference's hash,
 * registration.cpp:20-27; the means are still computed on the GPU).
 * Key of a point: static_cast<int>(std::floor(x * (1 / voxel_size))) per axis, as the reference - undefined in C++ for NaN and
 * for values outside int range.  The rule here is what that cast does on x86 (cvttss2si): every such coordinate gets INT_MIN.
 * So NaN, +-inf and far-out points (|x / voxel_size| >= 2^31) share a cell with each other and with x / voxel_size in
 * [-2^31, -2^31 + 1); their voxel's mean is NaN or infinite as the f32 sum makes it. */
#define TDV_VOXEL_ORDER_FIRST 0
#define TDV_VOXEL_ORDER_REFERENCE 1
int tdv_voxel_downsample(tdv_ctx* ctx, const float* xyz, const float* rgb, int n, float voxel_size, int order,
                         float* out_xyz, float* out_rgb, int capacity, int* n_out);
/* The same grid with the normals kept (the reference drops them): what a coarse point-to-plane or GICP level needs (tdv_icp_multiscale).
 * Points, colours, the voxel set and both orders are tdv_voxel_downsample's, bit for bit; the normals ride the same grouping pass as a
 * second 3-wide companion.  A voxel's normal is the colours' expression applied to the normals - f32 sums in ascending input index, each
 * divided by (float)count - and the mean m is then brought to unit length in f32 without contraction:
 *   l2 = m_x * m_x + (m_y * m_y + m_z * m_z)      (the reference's three-term order),      l = sqrtf(l2)
 *   l2 > 0 and l finite: m_x / l, m_y / l, m_z / l;  otherwise m as it is - zero where the members' normals cancel, NaN or infinite
 *   where a member is (or where a square overflows).
 * Input normals are taken as given (unit length is not checked).  normals == NULL or out_normals == NULL: no normals, the call is
 * tdv_voxel_downsample.  rgb / out_rgb are optional as there. */
int tdv_voxel_downsample_normals(tdv_ctx* ctx, const float* xyz, const float* normals, const float* rgb /* optional */, int n, float voxel_size,
                                 int order, float* out_xyz, float* out_normals, float* out_rgb, int capacity, int* n_out);

/* ---- R4a: normals ------------------------------------------------------------------------- */
/* Replaces Registration::estimateNormals (src/registration.cpp:105-130): exact brute-force kNN
 * ((d2, idx) lexicographic order, self included), PCA normal, flipped towards the origin.
 * out_knn (optional, int[n*k], -1 padded) receives the neighbour lists. */
int tdv_estimate_normals(tdv_ctx* ctx, const float* xyz, int n, int k, float* out_normals, int* out_knn);

/* ---- R4b: FPFH ---------------------------------------------------------------------------- */
/* Replaces Registration::computeFPFH (src/registration.cpp:133-201): radius search d2 <= r^2,
 * (d2, idx) order, capped at 100 neighbours; SPFH + weighted FPFH, 33 bins.  Normals are taken as given (unit length is not
 * checked).  A bin is static_cast<int>((alpha + 1) * 5.5), likewise for phi and (theta / pi + 1) * 5.5, clamped to [0, 10]; the
 * cast is undefined in C++ for NaN and outside int range, and the rule here is what it does on x86 (cvttss2si / cvttsd2si): such a
 * value gets INT_MIN, so bin 0 - e.g. alpha = +inf or >= ~3.9e8 from an infinite or far from unit normal. */
int tdv_compute_fpfh(tdv_ctx* ctx, const float* xyz, const float* normals, int n, float radius,
                     float* out_desc33, int* out_nbr /* optional int[n*100] */, int* out_nbr_cnt /* optional int[n] */);

/* ---- R5: RANSAC --------------------------------------------------------------------------- */
/* Feature correspondences of src/registration.cpp:216-232: argmin_j sum_d (fs[i][d]-ft[j][d])^2,
 * accumulated in d order, strict <, lowest j on ties. */
int tdv_feature_match(tdv_ctx* ctx, const float* fs, int ns, const float* ft, int nt, int* out_corr);

typedef struct tdv_ransac_result {
    float T[16];        /* column-major; identity if no hypothesis ever had an inlier            */
    float fitness;      /* inliers / ns of the winning hypothesis (0 if none)                    */
    float rmse;
    int inliers;        /* inlier count of the winning hypothesis                                 */
    int best_iteration; /* iteration index that produced it (-1 if none)                          */
    int iterations_run; /* iterations consumed, including skipped (degenerate-triple) ones        */
} tdv_ransac_result;

/* Replaces Registration::ransacRegistration (src/registration.cpp:204-295).  corr may be NULL
 * (then fs/ft are matched first) or a precomputed int[ns] (then fs/ft may be NULL).
 * Index triples come from mt19937(seed) + libstdc++-11 uniform_int_distribution<size_t>
 * (Lemire), iteration semantics (skip on repeated index, strict-> best, early exit on
 * fitness > confidence) as the reference.  seed = 42 reproduces registration.cpp:235.
 * trace_inliers (optional int[max_iterations]): per-iteration inlier count, -1 = skipped. */
int tdv_ransac(tdv_ctx* ctx, const float* src, int ns, const float* tgt, int nt,
               const float* fs, const float* ft, const int* corr,
               float voxel_size, int max_iterations, float confidence, uint32_t seed,
               tdv_ransac_result* out, int* trace_inliers);

/* ---- R6: ICP ------------------------------------------------------------------------------ */
typedef struct tdv_icp_result {
    float T[16];     /* column-major */
    float fitness;
    float rmse;
    int iterations;  /* iterations whose update was applied */
    int n_corr;      /* accepted correspondences of the last applied iteration */
} tdv_icp_result;

/* Replaces GPURegistration::icpRefine (src/gpu_impl.cpp:141-260, kernels cuda/icp.cu:14-55,90-142)
 * and Registration::icpRefine (src/registration.cpp:297-414, the oracle).  tgt_normals may be NULL;
 * point-to-plane is used iff point_to_plane != 0 and tgt_normals != NULL, else point-to-point
 * Kabsch (registration.cpp:343,365).  The whole loop runs on the device; the host polls a
 * convergence flag every few iterations. */
int tdv_icp(tdv_ctx* ctx, const float* src, int ns, const float* tgt, const float* tgt_normals, int nt,
            const float* T0, float distance_threshold, int max_iterations, int point_to_plane,
            tdv_icp_result* out);

/* One correspondence pass for a given T (registration.cpp:325-359): nearest target index per
 * source (always written), its squared distance, and the accepted flag; n_corr = accepted count.
 * Exposed for parity tests.  Full scan by default; with TDV_ICP_SEARCH_PRUNED set on the ctx the pruned
 * search is used and rows beyond the threshold report corr 0 / d2 FLT_MAX (accepted rows are identical). */
int tdv_icp_correspondences(tdv_ctx* ctx, const float* src, int ns, const float* tgt, int nt,
                            const float* T, float distance_threshold,
                            int* out_corr, float* out_d2, uint8_t* out_accepted, int* out_n_corr);

/* ---- device-resident entry points (inputs already in HBM; used by bench.py and by batched callers)
 * All pointers are device pointers on the ctx's device; work is enqueued on the ctx's stream and
 * the call returns after the stream has been synchronized (results are host structs). ------------ */
/* fixed_iterations != 0: run exactly max_iterations iterations (convergence and the n_corr<3 break
 * are still evaluated on the device and reported, but do not stop the loop) — benchmarking only. */
int tdv_icp_dev(tdv_ctx* ctx, const float* d_src, int ns, const float* d_tgt, const float* d_tgt_normals, int nt,
                const float* T0, float distance_threshold, int max_iterations, int point_to_plane,
                int fixed_iterations, tdv_icp_result* out);
/* Registration::icpRefine (src/registration.cpp:297-414) for n_instances source clouds against ONE target, in one call: refining
 * many instances from poses the caller already has (a bin imaged again after a pick, a pose from another estimator).
 * Cloud b = points [h_src_offsets[b], h_src_offsets[b+1]) of d_src (host array, n_instances + 1 entries, starting at 0,
 * non-decreasing); start pose h_T0 + 16*b (host, column-major); out: host array of n_instances results.
 * Per instance the result is, bit for bit, what tdv_icp_dev returns for that cloud on the same ctx (search mode and
 * accumulation mode included).  fixed_iterations as in tdv_icp_dev.  A cloud with 0 points, nt == 0 or max_iterations == 0
 * returns its start pose with fitness, rmse, iterations and n_corr 0, as tdv_icp_dev does.
 * With tree sums, the AUTO or GRID search and a target whose hash grid is usable (built once per call), all instances iterate
 * together: two launches per iteration for the whole batch and one read-back of all states every few iterations.  Small
 * problems (target and every cloud within 2,048 points) run in one launch; otherwise (BRUTE / PRUNED forced, an unusable grid,
 * reference-order sums) the call runs the single-instance loop per instance with the target's grid or Morton order built once.
 * tdv_ctx_last_icp_search reports the search that ran.  Every argument is checked before anything is enqueued: TDV_ERR_BAD_ARG
 * writes nothing to out. */
int tdv_icp_batch_dev(tdv_ctx* ctx, const float* d_src, const int* h_src_offsets, int n_instances,
                      const float* d_tgt, const float* d_tgt_normals /* may be NULL */, int nt, const float* h_T0,
                      float distance_threshold, int max_iterations, int point_to_plane, int fixed_iterations,
                      tdv_icp_result* out);
/* Generalized ICP, plane-to-plane (Segal et al. 2009, plane-regularised covariances): both surfaces are modelled as planes with a
 * normal variance epsilon, C_x = I - (1 - epsilon) n n^T per point (eigenvalues 1, 1, epsilon about the normal).  tdv_gicp /
 * tdv_gicp_dev / tdv_gicp_batch_dev are tdv_icp / tdv_icp_dev / tdv_icp_batch_dev (same search on every path, same acceptance
 * d2 <= thr^2, same batch paths and bit-for-bit batch = single guarantee, same tdv_ctx_last_icp_search) with the source normals
 * (laid out like the source points) and these per-correspondence terms in place of point-to-plane's.  f32 without contraction except
 * where stated;
 * p = the transformed source point (as ICP forms it), q / nt the target point and normal, ns the source normal, R the pose's 3x3,
 * c = 1 - epsilon (f32):
 *   a    = R ns, each row R_r0 * ns_x + (R_r1 * ns_y + R_r2 * ns_z)              (the transform's row form, no translation)
 *   C_ii = 2 - c * (a_i * a_i + nt_i * nt_i)                                     (C = 2 I - c (a a^T + nt nt^T) = C_t + R C_s R^T)
 *   C_ij = -(c * (a_i * a_j + nt_i * nt_j))                  i < j, C symmetric
 *   in f64 from the f32 C_ij (C's condition number is ~1 / epsilon; the products of two f32 are exact in f64):
 *   A00 = C11 * C22 - C12 * C12   A11 = C00 * C22 - C02 * C02   A22 = C00 * C11 - C01 * C01     (cofactors, A symmetric)
 *   A01 = C02 * C12 - C01 * C22   A02 = C01 * C12 - C02 * C11   A12 = C01 * C02 - C00 * C12
 *   s    = 1 / (C00 * A00 + (C01 * A01 + C02 * A02)),  M_ij = (float)(A_ij * s)           (M = C^-1, symmetric; f32 from here on)
 *   e    = p - q per component;  g_i = M_i0 * e_0 + (M_i1 * e_1 + M_i2 * e_2)          (g = M e)
 *   p x v = (p_y * v_2 - p_z * v_1,  p_z * v_0 - p_x * v_2,  p_x * v_1 - p_y * v_0)
 *   P_j  = p x (M_j0, M_j1, M_j2) for j = 0, 1, 2;  K_b = (P_0[b], P_1[b], P_2[b])
 * With J = [-[p]x | I] (d p / d(omega, t)), H_ab = J_a . M J_b (a <= b) and v_a = J_a . g are:
 *   H_ab = (p x K_b)[a] for a <= b < 3;  H_a,3+j = P_j[a];  H_3+i,3+j = M_ij;  v_a = (p x g)[a] for a < 3;  v_3+j = g_j
 * each widened to f64 and summed in point-to-plane's slots and tree; the step is point-to-plane's (x = ldlt6_solve(H, -v), rotation
 * euler_xyz(x0, x1, x2), translation x3..5).  n_corr, fitness, rmse = sqrt(sum d2 / n_corr) (Euclidean d2), the |delta rmse| < 1e-6
 * rule, the n_corr < 3 break and fixed_iterations are ICP's: the results compare directly with ICP's.
 * Normals are used as given: unit or zero length (a zero normal makes that cloud's covariance I).  An epsilon below ~3e-8 rounds c to
 * 1 and can leave C singular.  The ctx's loss (tdv_ctx_set_icp_loss) weighs each correspondence by its Mahalanobis residual
 * e_m = sqrtf(fmaxf(0, e_0 * g_0 + (e_1 * g_1 + e_2 * g_2))): (double)w * term for the 27 terms, n_eff last, as for point-to-plane.
 * TDV_ERR_BAD_ARG before anything is enqueued or written to out: either normal array NULL, epsilon not finite or outside (0, 1], a ctx
 * in TDV_ICP_ACCUMULATE_REFERENCE mode (the reference has no GICP; the reason is in tdv_last_error), or what the ICP entry point
 * checks.  0 points, nt == 0 or max_iterations == 0 return what ICP returns. */
int tdv_gicp(tdv_ctx* ctx, const float* src, const float* src_normals, int ns, const float* tgt, const float* tgt_normals, int nt,
             const float* T0, float distance_threshold, int max_iterations, float epsilon, tdv_icp_result* out);
int tdv_gicp_dev(tdv_ctx* ctx, const float* d_src, const float* d_src_normals, int ns, const float* d_tgt, const float* d_tgt_normals,
                 int nt, const float* T0, float distance_threshold, int max_iterations, float epsilon, int fixed_iterations,
                 tdv_icp_result* out);
int tdv_gicp_batch_dev(tdv_ctx* ctx, const float* d_src, const float* d_src_normals, const int* h_src_offsets, int n_instances,
                       const float* d_tgt, const float* d_tgt_normals, int nt, const float* h_T0, float distance_threshold,
                       int max_iterations, float epsilon, int fixed_iterations, tdv_icp_result* out);
/* Colored ICP (Park, Zhou, Koltun, ICCV 2017; Open3D's registration_colored_icp): point-to-plane's geometric row plus a photometric
 * row on the target's tangent plane, which pins the in-plane slide and the spin about the normal on textured surfaces.
 *
 * tdv_color_gradients / tdv_color_gradients_dev: out_color / d_color = float[n * 4], per point (I, d_x, d_y, d_z), the intensity
 * and its gradient on the point's tangent plane.  f32 without contraction except where stated:
 *   I_i  = ((r_i + g_i) + b_i) / 3.0f                                            (correctly rounded division)
 *   neighbours: point i's exact kNN list for k, as tdv_estimate_normals returns it ((d2, idx) order, self included, -1 padded) -
 *   self (index i) and the pads dropped, in list order; m = how many are left.  d_knn == NULL: that search runs inside the call;
 *   otherwise d_knn must be tdv_estimate_normals' int[n * k] list for the same cloud and k, and no search runs.
 *   per neighbour j, with q the point and n its normal:
 *     t_j = (q_j - q)_x * n_x + ((q_j - q)_y * n_y + (q_j - q)_z * n_z);  u_j = (q_j - q) - t_j * n per component;  b_j = I_j - I_i
 *   in f64 from the f32 values, summed from 0.0 in list order:  S_ab = sum u_j[a] * u_j[b],  c_a = sum u_j[a] * b_j
 *   A_ab = S_ab + ((m * m) * n_a) * n_b                                         (Open3D's tangent row m n; m * m in f64)
 *   cofactors  C00 = A11 * A22 - A12 * A12   C11 = A00 * A22 - A02 * A02   C22 = A00 * A11 - A01 * A01
 *              C01 = A02 * A12 - A01 * A22   C02 = A01 * A12 - A02 * A11   C12 = A01 * A02 - A00 * A12   (C symmetric)
 *   det = A00 * C00 + (A01 * C01 + A02 * C02);  d_a = (float)((C_a0 * c_0 + (C_a1 * c_1 + C_a2 * c_2)) / det)
 *   d = 0 when m < 3 or det is not > 0 and finite.
 * Normals are taken as given.  TDV_ERR_BAD_ARG: k <= 0 or k > 255 (as tdv_estimate_normals), a NULL array with n > 0.
 *
 * tdv_colored_icp / tdv_colored_icp_dev / tdv_colored_icp_batch_dev are tdv_icp / tdv_icp_dev / tdv_icp_batch_dev, point-to-plane
 * (same search on every path, same acceptance d2 <= thr^2, same batch paths and bit-for-bit batch = single guarantee, same
 * tdv_ctx_last_icp_search) with the source colours (float[ns * 3], laid out like the source points), the target's colour table
 * tgt_color = tdv_color_gradients of the target (float[nt * 4]; on the device 16-byte aligned) and lambda = lambda_geometric in
 * [0, 1] (Open3D's default 0.968).  Per accepted correspondence, f32 without contraction, lg = sqrtf(lambda), lc = sqrtf(1 - lambda):
 *   p = the transformed source point (as ICP forms it), q / n the target point and normal, (I_q, d) its colour table entry,
 *   I_s = ((r + g) + b) / 3.0f of the source point's colour
 *   e    = p - q per component;  en = e_x * n_x + (e_y * n_y + e_z * n_z)      (point-to-plane's r)
 *   J    = [p x n | n], p x v = (p_y * v_z - p_z * v_y,  p_z * v_x - p_x * v_z,  p_x * v_y - p_y * v_x)   (point-to-plane's row)
 *   e_t  = e - en * n per component                                             (p's offset on the target's tangent plane)
 *   dn   = d_x * n_x + (d_y * n_y + d_z * n_z);  g = dn * n - d per component    (g = -m, m = d - (d . n) n)
 *   de   = d_x * e_t,x + (d_y * e_t,y + d_z * e_t,z)
 *   r_G  = lg * en                          J_G[a] = lg * J[a]
 *   r_C  = lc * (I_s - (I_q + de))          J_C = [lc * (p x g) | lc * g]
 * H_ab (a <= b, point-to-plane's 21 slots in its order) = (double)(J_G[a] * J_G[b]) + (double)(J_C[a] * J_C[b]);
 * v_a (its 6 slots) = (double)(J_G[a] * r_G) + (double)(J_C[a] * r_C): each product formed in f32, widened, the two added in f64.
 * The f64 tree, the step (x = ldlt6_solve(H, -v), rotation euler_xyz(x0, x1, x2), translation x3..5), n_corr, fitness, rmse
 * (Euclidean d2), the |delta rmse| < 1e-6 rule, the n_corr < 3 break and fixed_iterations are ICP's: the results compare directly
 * with ICP's and GICP's.  At lambda = 1 the terms equal point-to-plane's in value.  The ctx's loss (tdv_ctx_set_icp_loss) weighs
 * each row by its own residual: w_G = weight(r_G), w_C = weight(r_C), each slot (double)w_G * (J_G product) + (double)w_C * (J_C
 * product), and n_eff counts the correspondences with w_G > 0 || w_C > 0.
 * TDV_ERR_BAD_ARG before anything is enqueued or written to out: a NULL colour, colour table or normal array, lambda not finite or
 * outside [0, 1], a device colour table not 16-byte aligned, a ctx in TDV_ICP_ACCUMULATE_REFERENCE mode (the reference has no
 * colored ICP; the reason is in tdv_last_error), or what the ICP entry point checks.  0 points, nt == 0 or max_iterations == 0
 * return what ICP returns. */
int tdv_color_gradients(tdv_ctx* ctx, const float* xyz, const float* rgb, const float* normals, int n, int k, float* out_color);
int tdv_color_gradients_dev(tdv_ctx* ctx, const float* d_xyz, const float* d_rgb, const float* d_normals, int n, int k,
                            const int* d_knn /* may be NULL */, float* d_color);
int tdv_colored_icp(tdv_ctx* ctx, const float* src, const float* src_rgb, int ns, const float* tgt, const float* tgt_normals,
                    const float* tgt_color /* float[nt*4] */, int nt, const float* T0, float distance_threshold, int max_iterations,
                    float lambda_geometric, tdv_icp_result* out);
int tdv_colored_icp_dev(tdv_ctx* ctx, const float* d_src, const float* d_src_rgb, int ns, const float* d_tgt, const float* d_tgt_normals,
                        const float* d_tgt_color, int nt, const float* T0, float distance_threshold, int max_iterations,
                        float lambda_geometric, int fixed_iterations, tdv_icp_result* out);
int tdv_colored_icp_batch_dev(tdv_ctx* ctx, const float* d_src, const float* d_src_rgb, const int* h_src_offsets, int n_instances,
                              const float* d_tgt, const float* d_tgt_normals, const float* d_tgt_color, int nt, const float* h_T0,
                              float distance_threshold, int max_iterations, float lambda_geometric, int fixed_iterations,
                              tdv_icp_result* out);
/* Multi-scale ICP: coarse-to-fine refinement over a voxel pyramid (Open3D's t.pipelines.registration.multi_scale_icp).  A single-scale
 * call accepts correspondences within one threshold, so its basin of convergence is a fraction of that threshold; a schedule starts with
 * coarse clouds and a wide threshold and hands each level's pose to the next, finer one.
 * A level: voxel_size > 0 - source and target are voxel-downsampled at that size in TDV_VOXEL_ORDER_FIRST with their normals kept
 * (tdv_voxel_downsample_normals: the target's where it has any, the source's for GICP); voxel_size <= 0, the last level only - the
 * clouds as given.  Then the ICP loop of the estimation from the pose the level before left (level 0: T0), with the level's
 * max_correspondence_distance as distance_threshold, at most max_iterations iterations and the level's convergence criteria, which are
 * Open3D's ICPConvergenceCriteria: the loop is done after an applied iteration iff it is not the first and
 *   fabsf(prev_fitness - fitness) < relative_fitness  &&  fabsf(prev_rmse - rmse) < relative_rmse,
 * prev_* being what the previous applied iteration of the same level left.  relative_fitness = +INFINITY with relative_rmse = 1e-6f is
 * the rule of every other ICP entry point (registration.cpp:406); relative_rmse = 0 never fires.  A level that breaks on n_corr < 3, or
 * that has 0 iterations or no points on either side, passes its pose on unchanged and reports fitness, rmse, iterations and n_corr 0, as
 * tdv_icp_dev does.
 * estimation: TDV_ICP_POINT_TO_PLANE (without target normals: point-to-point, as tdv_icp), TDV_ICP_POINT_TO_POINT, TDV_ICP_GICP (both
 * normal arrays and epsilon as tdv_gicp; epsilon is ignored otherwise).  The ctx's search mode, accumulation mode, launch form, probe
 * cache and robust loss apply at every level as they do to tdv_icp_dev; tdv_ctx_last_icp_* report the last level.
 * THE CONTRACT: out[l] (the batch: out[b * n_levels + l]) is, bit for bit, what the stagewise public calls return on the same ctx -
 * tdv_voxel_downsample_normals_dev(TDV_VOXEL_ORDER_FIRST) of the source and of the target, then tdv_icp_dev / tdv_gicp_dev from the
 * level before's pose (with default criteria; other criteria have no stagewise entry point) - in T, fitness, rmse, iterations, n_corr and
 * the level's point counts ns, nt.  The batch is per instance what the single call returns.
 * What the one call saves: the batch builds the target's level once per level, takes all sources' levels from the batched voxel path
 * (one set of launches per level; a level so coarse that a voxel holds more than 16 points is redone cloud by cloud on the path
 * without that limit, as tdv_voxel_downsample_batch_dev does), iterates all instances together where tdv_icp_batch_dev would, and keeps the
 * level clouds in the ctx's workspace (each level rewinds it: a call needs the room of its largest level; no allocation in steady state).
 * Levels: 1 .. TDV_ICP_MAX_LEVELS; voxel sizes strictly decreasing, only the last may be <= 0; max_correspondence_distance > 0 and
 * finite; max_iterations >= 0; relative_fitness > 0 or +INFINITY; relative_rmse >= 0.  Everything is checked before anything is
 * enqueued: TDV_ERR_BAD_ARG (NaN anywhere, an unknown estimation, GICP without both normal arrays or under reference-order sums, a
 * robust loss under reference-order sums, what tdv_icp_batch_dev checks) writes nothing to out.  ns == 0, nt == 0 and n_instances == 0
 * behave as in tdv_icp_batch_dev. */
typedef struct tdv_icp_level {
    float voxel_size;                   /* > 0: the level's voxel grid; <= 0, last level only: the clouds as given            */
    float max_correspondence_distance;  /* the level's distance_threshold: > 0, finite                                        */
    int   max_iterations;               /* >= 0                                                                               */
    float relative_fitness, relative_rmse;
} tdv_icp_level;
/* voxel_size -1, max_correspondence_distance 0 (the caller must set it), 30 iterations, relative_fitness +INFINITY, relative_rmse 1e-6f */
void tdv_icp_level_default(tdv_icp_level* level);
typedef struct tdv_icp_level_result {
    tdv_icp_result icp;
    int ns, nt;                         /* points of the level's source and target clouds                                     */
} tdv_icp_level_result;
#define TDV_ICP_MAX_LEVELS 8
#define TDV_ICP_POINT_TO_PLANE 0
#define TDV_ICP_POINT_TO_POINT 1
#define TDV_ICP_GICP 3
int tdv_icp_multiscale(tdv_ctx* ctx, const float* src, const float* src_normals /* GICP only */, int ns, const float* tgt,
                       const float* tgt_normals /* may be NULL */, int nt, const float* T0, const tdv_icp_level* levels, int n_levels,
                       int estimation, float epsilon, tdv_icp_level_result* out /* [n_levels] */);
int tdv_icp_multiscale_dev(tdv_ctx* ctx, const float* d_src, const float* d_src_normals, int ns, const float* d_tgt,
                           const float* d_tgt_normals, int nt, const float* T0, const tdv_icp_level* levels, int n_levels,
                           int estimation, float epsilon, tdv_icp_level_result* out);
/* clouds, offsets and start poses laid out as tdv_icp_batch_dev's (d_src_normals like d_src); out: n_instances * n_levels, instance-major */
int tdv_icp_multiscale_batch_dev(tdv_ctx* ctx, const float* d_src, const float* d_src_normals, const int* h_src_offsets, int n_instances,
                                 const float* d_tgt, const float* d_tgt_normals, int nt, const float* h_T0, const tdv_icp_level* levels,
                                 int n_levels, int estimation, float epsilon, tdv_icp_level_result* out);
/* Fast Global Registration (Zhou, Park, Koltun, ECCV 2016; Open3D's registration_fgr_based_on_feature_matching): a global pose from the
 * FPFH matches without hypotheses - mutual nearest descriptors, a tuple test, then iteration_number Geman-McClure weighted Gauss-Newton
 * steps under a graduated non-convexity schedule.  Open3D's options and defaults; its rand() and its pair order are replaced by the
 * deterministic rules below.  Every step, in order:
 *  1. Matching: cst[i] = the target index tdv_feature_match gives source i (exact, strict <, lowest index on ties); cts[j] the same from
 *     target j to the source.
 *  2. Mutual filter: pair (i, cst[i]) is kept iff cts[cst[i]] == i; kept pairs in ascending i; n_mutual = their count.
 *  3. Tuple test (tuple_test != 0): trials t = 0 .. 100 * n_mutual - 1 (64-bit).  Trial t takes words x0, x1, x2 of Philox4x32-10 with
 *     counter (lo32(t), hi32(t), 0, 0) and key (seed, 0); index k = (uint32)(((uint64)x_k * n_mutual) >> 32) into the mutual list (a
 *     multiply-shift: index m comes up floor or ceil of 2^32 / n_mutual times, a bias of at most n_mutual / 2^32).  With a_k / b_k the
 *     source / target points of the three pairs: l_a0 = |a0 - a1|, l_a1 = |a1 - a2|, l_a2 = |a2 - a0|, likewise l_b, each component
 *     difference in f64 from the f32 inputs, |d| = sqrt((dx*dx + dy*dy) + dz*dz) without contraction.  The trial passes iff
 *     l_a*s < l_b && l_b < l_a/s for all three, s = (double)tuple_scale (a repeated index gives 0 < 0 and fails, as in Open3D; a NaN
 *     fails).  The tuple set is the pairs of the FIRST maximum_tuple_count passing trials in trial order, three per trial as (pair 0,
 *     pair 1, pair 2); n_tuple = 3 x (trials kept).  Trials are evaluated in chunks: chunk k holds TDV_FGR_TRIAL_CHUNK << min(k, 5)
 *     trials, and the test stops after the chunk in which the count was reached or at 100 * n_mutual trials; trials_run = the trials
 *     evaluated.  tuple_test == 0: the mutual set is used as it is (n_tuple = 0, trials_run = 0).  The test reads the raw points, so
 *     these sets depend on no sum.
 *  4. Normalisation (Open3D's NormalizePointCloud): mu_s, mu_t = f64 means of ALL points of each cloud (f64 sums); sigma = the largest
 *     |x - mu| = sqrt((dx*dx + dy*dy) + dz*dz) (f64) over both clouds (a NaN never wins; 0 if no value is > 0), or 1 with
 *     use_absolute_scale; p = (x_s - mu_s) / sigma, q = (x_t - mu_t) / sigma per component in f64.
 *  5. Optimisation (Open3D's OptimizePairwise) over the pair list (tuples, or the mutual pairs with tuple_test == 0).  Fewer than 10
 *     pairs: T = identity (f32), degenerate = 1, no optimisation.  Otherwise, f64 throughout: T = I; mu = 1 (with use_absolute_scale the
 *     largest |x - mu|, Open3D's scale_start); iterations itr = 0 .. iteration_number - 1, no early exit:
 *       if decrease_mu && itr % 4 == 0 && mu > maximum_correspondence_distance: mu = mu / division_factor  (a squared distance against a
 *       distance, as Open3D); per pair q'_a = ((T_a0 q_x + T_a1 q_y) + T_a2 q_z) + T_a3, r = p - q', rr = (r_x r_x + r_y r_y) + r_z r_z,
 *       w = (mu / (rr + mu))^2 (the quotient squared); rows (0, -q'z, q'y, -1, 0, 0 | r_x), (q'z, 0, -q'x, 0, -1, 0 | r_y),
 *       (-q'y, q'x, 0, 0, 0, -1 | r_z); per pair JtJ_ab = (w (J0_a J0_b) + w (J1_a J1_b)) + w (J2_a J2_b) (a <= b) and Jtr_a likewise
 *       with r, summed over the pairs in a fixed tree (the order is fixed, not the restatement's);
 *       step: JtJ = L D L^T unpivoted, for j = 0..5, i = j..5: s = A_ij - sum_{k<j} (L_ik d_k) L_jk (k ascending), d_j = s (i == j) or
 *       L_ij = s / d_j; a d_j not > 0 or not finite gives x = 0; else y = L^-1 Jtr, z_i = y_i / d_i, back substitution, x = -(L^-T z)
 *       (the solution of (-JtJ) x = Jtr);  delta = [Rz(x2) Ry(x1) Rx(x0) | x3..5] with c_i = cos x_i, s_i = sin x_i:
 *         [c2 c1, (c2 s1) s0 - s2 c0, (c2 s1) c0 + s2 s0;  s2 c1, (s2 s1) s0 + c2 c0, (s2 s1) c0 - c2 s0;  -s1, c1 s0, c1 c0];
 *       T = delta T (4x4 product, k ascending).
 *     T moves the target onto the source in normalised units; the result is Open3D's GetInvTransformationOriginalScale:
 *     R' = R^T, t' = -R^T u with u = (mu_s + sigma t) - R mu_t (products k ascending), rounded to f32 (column-major).
 *  6. Score, as tdv_ransac scores its winner (src/registration.cpp:276-288): over the one-way matches cst, threshold 1.5 * voxel_size,
 *     inlier iff sqrtf(d2) < thr, error sum of (double)(err * err) in ransac's f64 tree; fitness = inliers / ns, rmse = sqrtf((float)sum /
 *     inliers), 999 with no inlier.  The numbers compare directly with tdv_ransac_result; either pose can seed tdv_icp.
 * Non-finite coordinates have no special case: they propagate through the means (a NaN or infinite coordinate makes mu, sigma, and from
 * there the pose NaN, unless the pair list is degenerate) and fail every tuple trial they enter.
 * The ctx's ICP switches (search, accumulation, loss) do not apply.  Not provided: FGR inside tdv_register_batch_dev /
 * tdv_refine_batch_dev (a tdv_batch_params field: an ABI change), a batched form, the C++ operator mirror, FGR on given correspondences.
 * TDV_ERR_BAD_ARG, before anything is enqueued and with out untouched: a NULL ctx, params or out; a NULL cloud or descriptor array of a
 * non-empty cloud; ns or nt < 0; voxel_size not finite or not > 0; division_factor not > 1; tuple_scale outside (0, 1];
 * maximum_correspondence_distance not > 0; iteration_number < 0; maximum_tuple_count < 1; any non-finite float parameter.
 * ns == 0 or nt == 0: identity, zero counts, fitness and rmse 0, degenerate = 1.
 * tdv_fgr takes host arrays; tdv_fgr_dev device pointers (it synchronises and returns a host struct, as tdv_ransac_dev).
 * tdv_fgr_correspondences (host arrays, for parity tests) writes steps 1-3: the mutual pairs as (i, j) int pairs into out_mutual (room
 * for cap_mutual pairs) and the tuple pairs into out_tuple (cap_tuple pairs), with *n_mutual, *n_tuple and *trials_run; when a buffer is
 * too small (NULL with capacity 0 is a query) it returns TDV_ERR_BAD_ARG with the three counts written. */
#define TDV_FGR_TRIAL_CHUNK 131072
typedef struct tdv_fgr_params {
    float division_factor;                 /* 1.4   */
    float maximum_correspondence_distance; /* 0.025 */
    float tuple_scale;                     /* 0.95  */
    int   iteration_number;                /* 64    */
    int   maximum_tuple_count;             /* 1000  */
    int   use_absolute_scale;              /* 0     */
    int   decrease_mu;                     /* 1     */
    int   tuple_test;                      /* 1     */
    uint32_t seed;                         /* 42    */
} tdv_fgr_params;
typedef struct tdv_fgr_result {
    float T[16];          /* column-major, source onto target */
    float fitness;        /* inliers / ns of T over the one-way matches */
    float rmse;           /* 999 with no inlier */
    int inliers;
    int n_mutual;         /* mutual pairs */
    int n_tuple;          /* pairs kept by the tuple test (3 per trial; 0 with tuple_test == 0) */
    int degenerate;       /* 1: fewer than 10 pairs, T is the identity */
    long long trials_run; /* tuple trials evaluated */
} tdv_fgr_result;
void tdv_fgr_default_params(tdv_fgr_params* p);
int tdv_fgr(tdv_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const float* fs, const float* ft, float voxel_size,
            const tdv_fgr_params* params, tdv_fgr_result* out);
int tdv_fgr_dev(tdv_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const float* d_fs, const float* d_ft, float voxel_size,
                const tdv_fgr_params* params, tdv_fgr_result* out);
int tdv_fgr_correspondences(tdv_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const float* fs, const float* ft,
                            const tdv_fgr_params* params, int* out_mutual, int cap_mutual, int* out_tuple, int cap_tuple,
                            int* n_mutual, int* n_tuple, long long* trials_run);
/* Plane segmentation by RANSAC (Open3D's PointCloud::segment_plane(distance_threshold, ransac_n = 3, num_iterations, probability)),
 * repeated to strip several planes in one call (floor, then walls).  Open3D's rand() and its OpenMP order are replaced by the
 * deterministic rules below.  Plane k = 0, 1, ... is searched among the CANDIDATES of round k: the points no earlier plane labelled, in
 * ascending original index; m_k = their count (m_0 = n).  Every step, in order:
 *  1. Draw: hypothesis t = 0 .. num_iterations - 1 of round k takes words x0, x1, x2 of Philox4x32-10 with counter (t, k, 0, 0) and key
 *     (seed, 1) (FGR's key is (seed, 0): the streams differ); candidate j = (uint32)(((uint64)x_j * m_k) >> 32).  A repeated index makes
 *     the hypothesis invalid.
 *  2. Plane, f64 from the f32 inputs without contraction (Open3D's ComputeTrianglePlane, the order made explicit): u = p1 - p0,
 *     v = p2 - p0 per component; n = (u_y v_z - u_z v_y, u_z v_x - u_x v_z, u_x v_y - u_y v_x); s = (n_x n_x + n_y n_y) + n_z n_z;
 *     invalid iff !(s > 0) or s is not finite; r = sqrt(s), (a, b, c) = n / r per component, d = -((a p0x + b p0y) + c p0z).
 *  3. Score: dist(p) = |((a p_x + b p_y) + c p_z) + d|; a candidate is an inlier iff dist < (double)distance_threshold (strict, as
 *     Open3D; a NaN distance never is); count = the inlier candidates.  An invalid hypothesis scores nothing but counts as run.
 *  4. Winner and early stop: hypotheses run in chunks of TDV_PLANE_CHUNK; the winner is the largest count, ties to the LOWEST t (Open3D
 *     breaks ties by rmse in OpenMP order, which does not reproduce).  After each chunk, with b the best count so far and
 *     f = (double)b / m_k: the round stops iff probability < 1 and b > 0 and (f >= 1 or (L = log(1 - (f * f) * f) < 0 and
 *     run >= log(1 - probability) / L)), run = the hypotheses evaluated so far - Open3D's break rule at chunk granularity.  Two
 *     deliberate differences: probability = 1 never stops early (Open3D stops at f = 1), and L = 0 (f^3 below half an ulp of 1, where
 *     Open3D's bound is -inf) does not stop.  iterations_run = the hypotheses of the chunks evaluated.
 *  5. Acceptance: plane k is kept iff its winner is valid and count >= min_inliers; its inliers (the winner's membership, as Open3D
 *     returns it) get label k and leave the candidate set.  Otherwise the search ends and that round labels nothing.  Rounds run until
 *     max_planes planes are kept, fewer than 3 candidates remain, or a round is rejected.
 *  6. Reported plane: hypothesis = (a, b, c, d) rounded to f32, negated as a whole if d < 0 (the camera origin lies on the positive
 *     side: a floor's normal faces the sensor).  With refit (Open3D's closing GetPlaneFromPoints), plane = the least-squares plane of the
 *     inliers: f64 mean mu and covariance sum_i (p_i - mu)(p_i - mu)^T over the inliers in a fixed order (no division), the unit
 *     eigenvector of its smallest eigenvalue (cyclic Jacobi in f64), negated if its dot product with the hypothesis normal is < 0,
 *     d = -((n_x mu_x + n_y mu_y) + n_z mu_z), rounded to f32; plane = hypothesis if that is not finite.  Without refit,
 *     plane = hypothesis.  fitness = (float)((double)count / m_k); rmse = (float)sqrt(sum dist^2 / count) over the inliers, the sum an
 *     f64 fixed tree.
 *  7. Non-finite coordinates have no special case: a hypothesis that draws one is invalid (s is NaN or infinite), such a point is never
 *     an inlier, and it stays unlabelled.
 * labels (optional, int[n]): k for the points of plane k, -1 for every other.  d_rest_xyz (optional, float[3n]) receives the unlabelled
 * points in ascending original index, *n_rest their count (ready for tdv_voxel_downsample_dev).  n < 3: n_planes = 0, every label -1,
 * rest = the input.  The ctx's ICP switches do not apply.  Not provided: ransac_n > 3, a batched per-instance form, plane removal inside
 * tdv_register_batch_dev / tdv_refine_batch_dev (a tdv_batch_params field: an ABI change), the C++ operator mirror.
 * TDV_ERR_BAD_ARG, before anything is enqueued and with out untouched: a NULL ctx, params, out or n_planes; a NULL cloud with n > 0;
 * n < 0; distance_threshold not finite or not > 0; probability outside (0, 1] or NaN; num_iterations < 1; max_planes outside
 * [1, TDV_PLANE_MAX]; min_inliers < 3.  tdv_segment_planes takes host arrays; tdv_segment_planes_dev device pointers (it reads back
 * once, at the end, and returns host structs). */
#define TDV_PLANE_CHUNK 1024
#define TDV_PLANE_MAX   16
typedef struct tdv_plane_params {
    double   probability;        /* 0.99999999 (Open3D); a double: in f32 it rounds to 1.0 */
    float    distance_threshold; /* 0.01 */
    int      num_iterations;     /* 100 (Open3D) */
    int      max_planes;         /* 1, at most TDV_PLANE_MAX */
    int      min_inliers;        /* 3 */
    int      refit;              /* 1 */
    uint32_t seed;               /* 42 */
} tdv_plane_params;
typedef struct tdv_plane_result {
    float plane[4];        /* (a, b, c, d): a x + b y + c z + d = 0, unit normal */
    float hypothesis[4];   /* the winning hypothesis' plane */
    float fitness, rmse;
    int inliers;           /* points labelled with this plane */
    int candidates;        /* m_k */
    int best_iteration;    /* t of the winner */
    int iterations_run;
} tdv_plane_result;
void tdv_plane_default_params(tdv_plane_params* p);
int tdv_segment_planes(tdv_ctx* ctx, const float* xyz, int n, const tdv_plane_params* params, tdv_plane_result* out /* [max_planes] */,
                       int* n_planes, int* labels /* int[n], optional */);
int tdv_segment_planes_dev(tdv_ctx* ctx, const float* d_xyz, int n, const tdv_plane_params* params, tdv_plane_result* out, int* n_planes,
                           int* d_labels /* optional */, float* d_rest_xyz /* optional, float[3n] */, int* n_rest /* host, optional */);
/* Euclidean clustering (DBSCAN; Open3D's PointCloud::cluster_dbscan(eps, min_points)): which points of a cloud form an instance.  Every
 * output is an integer and every rule below is exact, so the result does not depend on the order in which the device works:
 *  1. Distance: d2(i, j) = (dx * dx + dy * dy) + dz * dz in f32 without contraction, dx, dy, dz the differences of the raw coordinates
 *     (their sign does not matter: negation is exact); eps2 = eps * eps in f32, FLT_MAX where that overflows (so that an infinite d2
 *     never passes).
 *  2. Neighbour: j is a neighbour of i iff d2(i, j) <= eps2 - this library's radius convention (tdv_compute_fpfh), a deliberate
 *     difference from the strict test of nanoflann behind Open3D's search.  A point counts itself (d2 = 0), as in Open3D.
 *  3. Non-finite coordinates have no special case: a row with a NaN or infinite coordinate has d2 NaN or +inf to every row, itself
 *     included, so it is nobody's neighbour, has no neighbour, and ends as noise.
 *  4. Core: a point with at least min_points neighbours (itself included).
 *  5. Clusters: the connected components of the core points under the neighbour relation, numbered 0, 1, ... in ascending order of
 *     their lowest-index core point.  That is the order in which Open3D's ascending scan opens them: on core points the labels equal
 *     Open3D's (wherever the two neighbour tests agree).
 *  6. Border: a non-core point with at least one core neighbour.  Open3D gives it to the cluster that reaches it first, which depends
 *     on the scan order; here it joins the cluster of its NEAREST core neighbour, ties in d2 to the lowest index - the order of the
 *     64-bit key (d2 bits, index) that the neighbour lists of this library follow.  A border point joins, it does not connect.
 *  7. Noise: every other point; label -1.
 *  8. min_cluster_size (1: Open3D's behaviour): a cluster's size is its core plus its border points; clusters below it become noise and
 *     the others are numbered again by rule 5.
 * result: n_clusters (after rule 8), n_core and n_border (rules 4 and 6, before rule 8), n_noise (labels of -1 at the end), n_dropped
 * (clusters rule 8 removed), largest (members of the largest kept cluster, 0 without one).
 * labels (optional, int[n]).  order (optional, int[n]): the original indices of the labelled points sorted by (label, index), then the
 * noise points in ascending index; *n_labelled (optional) = the labelled ones.  grouped_xyz (optional, float[3n]): the rows of the
 * cloud in that order.  offsets (HOST memory in either entry point, room for offsets_capacity + 1 ints): cluster b is
 * [offsets[b], offsets[b + 1]) of order and grouped_xyz, offsets[n_clusters] = n_labelled - the (d_src, h_src_offsets) layout of
 * tdv_icp_batch_dev, tdv_gicp_batch_dev, tdv_voxel_downsample_batch_dev and (with the clusters' normals laid out likewise)
 * tdv_ppf_match_batch_dev, which finds the start poses the first two need: cluster b goes straight into a batch call.  When
 * n_clusters > offsets_capacity (NULL with capacity 0 is a query) the call returns TDV_ERR_BAD_ARG with result, labels, order,
 * grouped_xyz and n_labelled written and offsets untouched.
 * TDV_ERR_BAD_ARG before anything is enqueued or written: a NULL ctx, params or result; a NULL cloud with n > 0; n < 0; eps not finite
 * or not > 0; min_points < 1; min_cluster_size < 1; offsets_capacity < 0, or > 0 with NULL offsets.  n == 0 is accepted (zero counts,
 * offsets[0] = 0).  tdv_cluster_default_params sets min_cluster_size = 1 and leaves eps = 0 and min_points = 0 for the caller (Open3D has
 * no defaults for them).  tdv_cluster_dbscan takes host arrays; tdv_cluster_dbscan_dev device pointers (it reads back the result, then
 * the offsets, at the end).  The ctx's ICP switches do not apply.  Not provided: clustering inside tdv_register_batch_dev (an ABI
 * change), a batched per-frame form, the C++ operator mirror, normal- or colour-aware region growing, HDBSCAN / OPTICS. */
typedef struct tdv_cluster_params {
    float eps;               /* no default: the caller's */
    int   min_points;        /* no default: the caller's */
    int   min_cluster_size;  /* 1 */
} tdv_cluster_params;
typedef struct tdv_cluster_result {
    int n_clusters;
    int n_core;
    int n_border;
    int n_noise;
    int n_dropped;
    int largest;
} tdv_cluster_result;
void tdv_cluster_default_params(tdv_cluster_params* p);
int tdv_cluster_dbscan(tdv_ctx* ctx, const float* xyz, int n, const tdv_cluster_params* params, tdv_cluster_result* result,
                       int* labels /* optional */, int* order /* optional */, float* grouped_xyz /* optional */,
                       int* offsets /* optional */, int offsets_capacity, int* n_labelled /* optional */);
int tdv_cluster_dbscan_dev(tdv_ctx* ctx, const float* d_xyz, int n, const tdv_cluster_params* params, tdv_cluster_result* result,
                           int* d_labels /* optional */, int* d_order /* optional */, float* d_grouped_xyz /* optional */,
                           int* offsets /* host, optional */, int offsets_capacity, int* n_labelled /* host, optional */);
/* Outlier removal (Open3D's PointCloud::remove_statistical_outlier(nb_neighbors, std_ratio) and remove_radius_outlier(nb_points,
 * radius)): the flying pixels and speckle of a depth frame, taken out before anything fits a model to the cloud.  Every rule is exact.
 * Statistical filter:
 *  1. Neighbours: the library's kNN list of point i for k = nb_neighbors - what tdv_estimate_normals(_dev) returns in out_knn:
 *     d2 = dx * dx + (dy * dy + dz * dz) in f32 without contraction over every row j whose d2 is not NaN, ordered by (d2 bits, index),
 *     self included (d2 = 0), the first min(nb_neighbors, n) entries.  count_i = the entries found; a query with a NaN coordinate finds
 *     none, and a d2 of +inf (an infinite row, an overflow) is a distance like any other.
 *  2. mean_i = (sum over the list in list order, sequentially from 0.0, of sqrt((double)d2_r)) / (double)count_i, in f64 with the
 *     correctly rounded sqrt: Open3D's std::accumulate order.  count_i = 0: the quiet NaN 0x7ff8000000000000.
 *  3. valid_i iff count_i > 0 and mean_i is finite and > 0 (Open3D's > 0 guard: a point with nb_neighbors exact duplicates of itself is
 *     not valid).  Non-finite rows and overflowing distances fall out by the arithmetic alone (their mean is NaN or +inf).
 *  4. n_valid = the valid points.  cloud_mean = (sum of mean_i over them) / n_valid, std_dev = sqrt((sum of (mean_i - cloud_mean)^2) /
 *     (n_valid - 1)), threshold = cloud_mean + std_ratio * std_dev, all f64, two passes (no sum of squares).  Either sum runs in ONE fixed
 *     order, so that two calls give the same bits: the term of point i (+0.0 where it is not valid) belongs to workgroup i / 256, thread
 *     t = i % 256; a workgroup sum is the shuffle tree over each wave of 64 (v += v[lane + off] for off = 32, 16, 8, 4, 2, 1; lane 0
 *     holds it), then (w0 + w1) + (w2 + w3) over its four waves; one workgroup then adds the workgroup sums b = t, t + 256, t + 512,
 *     ... in that order into thread t and sums its 256 threads the same way.  No float atomics.  n_valid = 0: cloud_mean, std_dev and
 *     threshold are NaN; n_valid = 1: std_dev and threshold are NaN.  Nothing is kept in either case.
 *  5. Kept iff valid_i and mean_i < threshold (strict; NaN fails it).
 * Radius filter: d2 and eps2 = radius * radius are rule 1 of tdv_cluster_dbscan (the tree (dx * dx + dy * dy) + dz * dz, FLT_MAX where
 * eps2 overflows), neighbour iff d2 <= eps2 (rule 2 there: this library's radius convention), self counts, rows with a NaN or infinite
 * coordinate have no neighbour (rule 3 there).  Kept iff the count > nb_points, as in Open3D: the core flag of tdv_cluster_dbscan at
 * min_points = nb_points + 1.  count[i] is saturated at nb_points + 1 (the walk stops there).
 * result: n_valid (statistical: rule 4; radius: the rows that count themselves, i.e. the finite ones), n_kept, and cloud_mean, std_dev,
 * threshold (0 from the radius filter).  Optional outputs, NULL to skip: mask (uint8[n], 1 = kept), mean (double[n], rule 2) resp.
 * count (int[n]), index (int[n]: the kept original indices in ascending order, n_kept of them), out_xyz and out_rgb (float[3n]: the kept
 * rows in that order, n_kept of them - a cloud ready for tdv_voxel_downsample_dev or tdv_cluster_dbscan_dev; out_rgb needs rgb).  Entries
 * beyond n_kept are not written.  rgb is optional.  The host entry points take host arrays and read back twice (the result with mask and
 * mean / count, then the n_kept rows); the _dev entry points take device pointers and read back once, the result.
 * TDV_ERR_BAD_ARG before anything is enqueued or written: a NULL ctx or result; a NULL cloud with n > 0; n < 0; nb_neighbors outside
 * [1, 255]; std_ratio NaN or infinite (a negative one is allowed); nb_points < 0; radius not finite or not > 0.  n == 0 is accepted (zero
 * counts; the statistical doubles are NaN).  The ctx's ICP switches do not apply.  Not provided: a per-instance (offsets) form, the filter
 * inside tdv_register_batch_dev / tdv_refine_batch_dev (an ABI change), the C++ operator mirror, normals pass-through (gather with
 * index). */
typedef struct tdv_outlier_result {
    int    n_valid;
    int    n_kept;
    double cloud_mean;
    double std_dev;
    double threshold;
} tdv_outlier_result;
int tdv_remove_statistical_outlier(tdv_ctx* ctx, const float* xyz, const float* rgb /* optional */, int n, int nb_neighbors, double std_ratio,
                                   tdv_outlier_result* result, uint8_t* mask /* optional */, double* mean /* optional */,
                                   int* index /* optional */, float* out_xyz /* optional */, float* out_rgb /* optional */);
int tdv_remove_statistical_outlier_dev(tdv_ctx* ctx, const float* d_xyz, const float* d_rgb /* optional */, int n, int nb_neighbors,
                                       double std_ratio, tdv_outlier_result* result, uint8_t* d_mask /* optional */,
                                       double* d_mean /* optional */, int* d_index /* optional */, float* d_out_xyz /* optional */,
                                       float* d_out_rgb /* optional */);
int tdv_remove_radius_outlier(tdv_ctx* ctx, const float* xyz, const float* rgb /* optional */, int n, int nb_points, float radius,
                              tdv_outlier_result* result, uint8_t* mask /* optional */, int* count /* optional */, int* index /* optional */,
                              float* out_xyz /* optional */, float* out_rgb /* optional */);
int tdv_remove_radius_outlier_dev(tdv_ctx* ctx, const float* d_xyz, const float* d_rgb /* optional */, int n, int nb_points, float radius,
                                  tdv_outlier_result* result, uint8_t* d_mask /* optional */, int* d_count /* optional */,
                                  int* d_index /* optional */, float* d_out_xyz /* optional */, float* d_out_rgb /* optional */);
/* ISS keypoints (Intrinsic Shape Signatures, Zhong 2009; Open3D's keypoint::ComputeISSKeypoints(salient_radius, non_max_radius, gamma_21,
 * gamma_32, min_neighbors)): the few percent of a cloud's points whose neighbourhood has three distinct principal extents - fewer source
 * points for the descriptor match, RANSAC or FGR without a coarser voxel.  The sums are defined over integers, so every output is fixed bit
 * for bit whatever order the device works in:
 *  1. Distance and neighbour: rules 1-3 of tdv_cluster_dbscan for each of the two radii: d2 = (dx * dx + dy * dy) + dz * dz in f32 without
 *     contraction, r2 = r * r in f32, FLT_MAX where that overflows, j is a neighbour of i iff d2 <= r2, a point counts itself, a row with a
 *     NaN or infinite coordinate has no neighbour and is nobody's.
 *  2. Support: support_i = the neighbours of i within salient_radius.  support_i < min_neighbors: saliency 0 (Open3D's `continue`), and
 *     the eigenvalues reported for i are +0.0.
 *  3. Scatter, in integers: salient_radius = m * 2^E with m in [0.5, 1) (frexpf; E = 0 for a radius of 0), sh = 20 - E.  For every
 *     neighbour j and axis a: d_a = p_j,a - p_i,a in f32 (one rounding), u_a = (int64)rintf(ldexpf(d_a, sh)), round-half-even; |u_a| <=
 *     2^20 + 1 follows from rule 1 (wherever r * r is a normal f32; u_a is saturated to [-2^31, 2^31 - 128] beyond, and the sums wrap).
 *     S_a = sum of u_a, S_ab = sum of u_a * u_b over the support: three first and six second moments, all int64.  Integer sums are
 *     associative: neither the walk order nor the reduction tree matters.  The quantum is 2^-21 of the radius's binade - coordinates
 *     differences are rounded to it, the price of exactness (it moves the eigenvalues by parts in 10^6: tests/test_iss_abi.py derives the
 *     bound).  n > TDV_ISS_MAX_POINTS (2^22) is refused, which keeps S_ab below 2^63.
 *  4. Covariance, f64 without contraction, c = (double)support_i, a <= b: C_ab = ((double)S_ab - ((double)S_a * (double)S_b) / c) / c:
 *     Open3D's covariance about the neighbourhood's own mean, in units of the quantum squared.
 *  5. Eigenvalues: f64 cyclic Jacobi on the symmetric 3 x 3, TDV_ISS_JACOBI_SWEEPS (6) sweeps, each over the pairs (p, q) = (0, 1), (0, 2),
 *     (1, 2) in that order.  A pair whose a_pq is exactly 0 is skipped; otherwise theta = (a_qq - a_pp) / (2 a_pq), t = sign / (|theta| +
 *     sqrt(theta * theta + 1)) with sign = -1 if theta < 0, else 1, c = 1 / sqrt(t * t + 1), s = t * c, h = t * a_pq, a_pp -= h, a_qq += h,
 *     and with r the third index a_rp' = c * a_rp - s * a_rq, a_rq' = s * a_rp + c * a_rq (from the old a_rp, a_rq), a_pq = 0.  Only +, -, *,
 *     / and the correctly rounded sqrt.  (On the 3 x 3 matrices of noisy clouds the off-diagonal is below 1e-44 of the largest eigenvalue
 *     after 4 sweeps and exactly 0 after 6.)  lambda1 >= lambda2 >= lambda3: the diagonal through the exchanges (0, 1), (1, 2), (0, 1),
 *     each swapping iff first < second.  Reported: ldexp(lambda, -2 sh), exact, in m^2.
 *  6. salient_i iff support_i >= min_neighbors and lambda2 / lambda1 < gamma_21 and lambda3 / lambda2 < gamma_32 and lambda3 > 0 (IEEE
 *     comparisons: the NaN of 0 / 0 fails).  saliency_i = lambda3 (reported scale) if salient, else +0.0.  A perfectly flat or collinear
 *     neighbourhood has lambda3 == 0 exactly and is never a keypoint.
 *  7. Non-maximum suppression: i is a keypoint iff saliency_i > 0, i has at least min_neighbors neighbours within non_max_radius (itself
 *     included), and no neighbour j within that radius has saliency_j > saliency_i.  Ties keep both points, as Open3D's IsLocalMaxima.
 *  8. Default radii (salient_radius == 0 and non_max_radius == 0): from the cloud's resolution, Open3D's ComputeModelResolution.  nn_i =
 *     sqrt((double)d2) of entry 1 of the library's kNN list of i at k = 2 (rule 1 of the statistical filter above); valid_i iff the list
 *     has two entries and nn_i is finite; resolution = (sum of the valid nn_i) / (their number) in the fixed f64 tree of the statistical
 *     filter's rule 4 (NaN without a valid one); salient_radius = (float)(6.0 * resolution), non_max_radius = (float)(4.0 * resolution).
 *     A NaN radius has no neighbours: every count is then 0.
 * result: n_finite (support_i >= 1: the rows that count themselves), n_supported (support_i >= min_neighbors), n_salient (saliency_i > 0),
 * n_keypoints, the two radii used, resolution (NaN when the radii were given).
 * attr (optional): one companion array of attr_width floats per point - FPFH rows (33), normals or colours (3), colored ICP's colour
 * table (4).  Optional outputs, NULL to skip: mask (uint8[n], 1 = keypoint), saliency (double[n]), eigenvalues (double[3n]: lambda1,
 * lambda2, lambda3 per point), support (int[n]), index (int[n]: the keypoints' original indices in ascending order, n_keypoints of them),
 * out_xyz (float[3n]) and out_attr (float[attr_width * n]; needs attr): their rows in that order - (out_xyz, out_attr) of a cloud and its
 * FPFH rows are the (src, fs) of tdv_ransac_dev or tdv_fgr_dev as they stand.  Entries beyond n_keypoints are not written.  The FPFH rows
 * are those of the full cloud: the descriptor stage costs what it did.  tdv_iss_keypoints takes host arrays and reads back twice (the
 * result with the per-point arrays, then the n_keypoints rows); tdv_iss_keypoints_dev takes device pointers and reads back once, the result.
 * TDV_ERR_BAD_ARG before anything is enqueued or written: a NULL ctx, params or result; a NULL cloud with n > 0; n < 0; n >
 * TDV_ISS_MAX_POINTS; a radius that is negative, NaN or infinite; exactly one radius 0; a gamma that is NaN or <= 0; min_neighbors < 1;
 * attr_width < 0; attr_width > 0 with a NULL attr; out_attr without attr.  n == 0 is accepted (zero counts).  The ctx's ICP switches do
 * not apply.  Not provided: keypoints inside tdv_register_batch_dev / tdv_refine_batch_dev (an ABI change), a per-instance (offsets) form,
 * the C++ operator mirror, other detectors, a descriptor computed at the keypoints only. */
#define TDV_ISS_JACOBI_SWEEPS 6
#define TDV_ISS_MAX_POINTS (1 << 22)
typedef struct tdv_iss_params {
    float  salient_radius;  /* 0 (with non_max_radius 0): 6 x the cloud's resolution */
    float  non_max_radius;  /* 0: 4 x the cloud's resolution */
    double gamma_21;        /* 0.975 */
    double gamma_32;        /* 0.975 */
    int    min_neighbors;   /* 5 */
} tdv_iss_params;
typedef struct tdv_iss_result {
    int    n_finite;
    int    n_supported;
    int    n_salient;
    int    n_keypoints;
    float  salient_radius;
    float  non_max_radius;
    double resolution;
} tdv_iss_result;
void tdv_iss_default_params(tdv_iss_params* p);
int tdv_iss_keypoints(tdv_ctx* ctx, const float* xyz, int n, const tdv_iss_params* params, const float* attr /* optional */, int attr_width,
                      tdv_iss_result* result, uint8_t* mask /* optional */, double* saliency /* optional */, double* eigenvalues /* optional */,
                      int* support /* optional */, int* index /* optional */, float* out_xyz /* optional */, float* out_attr /* optional */);
int tdv_iss_keypoints_dev(tdv_ctx* ctx, const float* d_xyz, int n, const tdv_iss_params* params, const float* d_attr /* optional */,
                          int attr_width, tdv_iss_result* result, uint8_t* d_mask /* optional */, double* d_saliency /* optional */,
                          double* d_eigenvalues /* optional */, int* d_support /* optional */, int* d_index /* optional */,
                          float* d_out_xyz /* optional */, float* d_out_attr /* optional */);
/* Farthest point sampling (Open3D's PointCloud::farthest_point_down_sample(num_samples, start_index); the sampling step of PointNet++ and
 * of the PPF pipelines): exactly num_samples points of a cloud, spread as evenly as a greedy rule manages - the one way here to thin a
 * cloud to a COUNT (a model under TDV_PPF_MODEL_MAX, a cloud under the 2,048 points of the small ICP batch, clusters of one size for the
 * batch entry points).  Prefix-stable: the first k entries of a K-sample are the k-sample.  The distance is f32 with one rounding per
 * operation and the choice an integer maximum, so every output is fixed bit for bit whatever order the device works in:
 *  1. Usable row: a row is usable iff its three coordinates are finite.  n_usable = the usable rows.  An unusable row is never selected
 *     and takes no part in any distance.
 *  2. Count: n_selected = min(num_samples, n_usable).
 *  3. Distance: d2(j, s) = (dx * dx + dy * dy) + dz * dz in f32 without contraction, dx = p_j.x - p_s.x and likewise y, z, one rounding
 *     each (rule 1 of tdv_cluster_dbscan).  Between usable rows it is never NaN and never -0; it is +inf on overflow, a distance like any
 *     other.
 *  4. Running minimum: m_j = +inf for every usable row at first; after sample s is taken, m_j = (d2(j, s) < m_j) ? d2(j, s) : m_j for
 *     every usable j.
 *  5. First sample: row start_index if it is usable, else the lowest usable index.
 *  6. Every later sample: among the usable rows not yet selected the one with the largest m_j, ties to the lowest index: one maximum
 *     over the 64-bit keys (bits(m_j) << 32) | (0xFFFFFFFF - j) - the bits of a non-negative f32 order as unsigned integers.  Selected
 *     and unusable rows carry key 0.
 *  7. No repeats: a selected row is never selected again.  This is the one deliberate difference from Open3D's loop, which on a cloud
 *     with fewer than num_samples distinct points repeats one index, and with NaN or infinite rows selects those first.  On distinct
 *     finite points the rule is Open3D's (strict >, the lowest index among equals), in f32 where Open3D works in f64.
 *  8. Outputs, in selection order, each optional (NULL to skip), entries beyond n_selected not written: index (int[n_selected], original
 *     row indices), out_d2 (float[n_selected]: the row's m at the moment it was selected: +inf for entry 0, non-increasing from entry 1
 *     on), out_xyz (the selected rows), out_attr (the rows of one companion array of attr_width floats per point - normals, colours, FPFH
 *     rows - as tdv_iss_keypoints; needs attr).
 *  9. result: n_usable, n_selected, path (TDV_FPS_WORKGROUP or TDV_FPS_GRID: the kernel family the call's size and the ctx's switch
 *     chose, also where nothing had to run), cover_d2 = the largest final m_j over the usable rows not selected, +0.0 without one: every
 *     usable point lies within sqrt(cover_d2) of a sample (it is the maximum that would have chosen the next sample).
 * Two kernel families give the same bytes.  Workgroup path: one workgroup of TDV_FPS_WORKGROUP_LANES lanes holds the whole cloud and the
 * running minima in registers, up to TDV_FPS_WORKGROUP_MAX rows; one workgroup barrier per sample.  Grid path: any size, one launch per
 * sample on the ctx's stream, the maximum through one 64-bit integer atomic per workgroup; no kernel waits for another workgroup.
 * tdv_ctx_set_fps_path: TDV_FPS_AUTO (default: the workgroup path iff n <= TDV_FPS_WORKGROUP_MAX) or one of the two, for tests and
 * measurements; tdv_ctx_last_fps_path: what the last call on the ctx chose (a batch: TDV_FPS_GRID if any of its clouds took the grid
 * path, else TDV_FPS_WORKGROUP); 0 before the first call.
 * tdv_farthest_point_down_sample takes host arrays and reads back twice (the result, then the n_selected rows);
 * tdv_farthest_point_down_sample_dev takes device pointers and reads back once, the result.
 * tdv_farthest_point_down_sample_batch_dev is, per cloud, tdv_farthest_point_down_sample_dev at start_index 0: cloud b is rows
 * [h_offsets[b], h_offsets[b + 1]) of d_xyz and d_attr - the layout tdv_cluster_dbscan_dev writes and tdv_ppf_match_batch_dev and
 * tdv_icp_batch_dev take - its index counts inside the cloud, and its outputs are rows [h_out_offsets[b], h_out_offsets[b + 1]) of
 * d_index, d_out_d2, d_out_xyz and d_out_attr, packed back to back (h_out_offsets[b + 1] - h_out_offsets[b] = results[b].n_selected), so
 * that they go into those batch entry points as they stand.  results[b] and cloud b's rows are byte for byte the single call's.  Clouds of
 * at most TDV_FPS_WORKGROUP_MAX rows run together, one workgroup each; larger ones go through the grid path one after another.  The call
 * reads back once (the per-cloud results), whatever n_clouds is.
 * TDV_ERR_BAD_ARG before anything is enqueued or written: a NULL ctx or result; a NULL cloud with n > 0; n < 0 or n > TDV_FPS_MAX_POINTS;
 * num_samples < 0; start_index outside [0, n) when n > 0; attr_width < 0; attr_width > 0 with a NULL attr; out_attr without attr;
 * TDV_FPS_WORKGROUP forced on a cloud above TDV_FPS_WORKGROUP_MAX; batch: n_clouds < 0, a NULL h_offsets or h_out_offsets, NULL results
 * with n_clouds > 0, offsets that do not start at 0 or that decrease, a cloud above TDV_FPS_MAX_POINTS.  n == 0 and num_samples == 0 are
 * accepted (zero counts; start_index is then not looked at when n == 0).  The ctx's ICP switches do not apply.  Not provided: the C++
 * operator mirror, sampling inside tdv_register_batch_dev / tdv_refine_batch_dev (an ABI change), per-cloud sample counts or start rows
 * in the batch form, other samplers (uniform, random, Poisson disk). */
#define TDV_FPS_MAX_POINTS (1 << 22)
#define TDV_FPS_WORKGROUP_LANES 1024
#define TDV_FPS_WORKGROUP_MAX 16384   /* 16 rows per lane: csrc/fps.hip has the register report */
#define TDV_FPS_AUTO 0
#define TDV_FPS_WORKGROUP 1
#define TDV_FPS_GRID 2
typedef struct tdv_fps_result {
    int   n_usable;
    int   n_selected;
    int   path;
    float cover_d2;
} tdv_fps_result;
int tdv_farthest_point_down_sample(tdv_ctx* ctx, const float* xyz, int n, int num_samples, int start_index, const float* attr /* optional */,
                                   int attr_width, tdv_fps_result* result, int* index /* optional */, float* out_d2 /* optional */,
                                   float* out_xyz /* optional */, float* out_attr /* optional */);
int tdv_farthest_point_down_sample_dev(tdv_ctx* ctx, const float* d_xyz, int n, int num_samples, int start_index,
                                       const float* d_attr /* optional */, int attr_width, tdv_fps_result* result, int* d_index /* optional */,
                                       float* d_out_d2 /* optional */, float* d_out_xyz /* optional */, float* d_out_attr /* optional */);
int tdv_farthest_point_down_sample_batch_dev(tdv_ctx* ctx, const float* d_xyz, const float* d_attr /* optional */, int attr_width,
                                             const int* h_offsets /* host, [n_clouds + 1], starting at 0, non-decreasing */, int n_clouds,
                                             int num_samples, tdv_fps_result* results /* host, [n_clouds] */,
                                             int* h_out_offsets /* host, [n_clouds + 1], written */, int* d_index /* optional */,
                                             float* d_out_d2 /* optional */, float* d_out_xyz /* optional */, float* d_out_attr /* optional */);
int tdv_ctx_set_fps_path(tdv_ctx* ctx, int mode);
int tdv_ctx_last_fps_path(tdv_ctx* ctx);
/* Pose verification (the hypothesis-verification stage of the bin-picking pipelines): the model is rendered as a point splat at each
 * candidate pose into the camera's depth image, and every rendered pixel is classified against the observed depth: it agrees, something
 * stands in front of it, or the camera saw through it.  The fitness of tdv_icp_correspondences asks how many scene points lie near the
 * model; this asks whether the model, at the pose, is consistent with what the camera saw.  One call takes all of a frame's candidates.
 * Every output is an integer and every float that decides one is fixed by the rules below, so the results do not depend on the order the
 * device works in.  All in f32, one rounding per operation, no contraction, the order exactly as written.
 *  1. Camera coordinates of model point m under T (column-major, t = T[12..14]):
 *     TDV_POSE_SOURCE_ONTO_TARGET (T as every registration here returns it, camera/scene onto model): d = m - t per component, then
 *       xc = (T[0]*d0 + T[1]*d1) + T[2]*d2
 *       yc = (T[4]*d0 + T[5]*d1) + T[6]*d2
 *       zc = (T[8]*d0 + T[9]*d1) + T[10]*d2
 *     This is R^T (m - t).  The rotation block is taken as orthonormal and is not checked.
 *     TDV_POSE_MODEL_TO_CAMERA (T as synth.py's poses):
 *       xc = ((T[0]*m0 + T[4]*m1) + T[8]*m2) + T[12]
 *       yc = ((T[1]*m0 + T[5]*m1) + T[9]*m2) + T[13]
 *       zc = ((T[2]*m0 + T[6]*m1) + T[10]*m2) + T[14]
 *  2. Usable: xc, yc, zc are finite and 0 < zc <= zmax.
 *  3. Pixel: uf = (xc*fx)/zc + cx, vf = (yc*fy)/zc + cy.  The point is unusable if either is non-finite or has magnitude >= 2^20.
 *     u = (int)floorf(uf + 0.5f), v likewise.  The point covers the pixels [u-splat, u+splat] x [v-splat, v+splat] clipped to the frame.
 *     A point whose centre is outside the frame still covers what its square reaches inside.  n_projected counts the usable points
 *     (rules 2 and 3), whether or not they cover a pixel of the frame.
 *  4. Rendered depth of a pixel: the minimum zc over the points that cover it.  The u32 bit pattern of a positive f32 orders as the
 *     float, so an integer minimum is exact and its order free.
 *  5. Observed depth: zo = float(raw) * float(1.0 / scale), the rule of tdv_depth_preprocess.  It is valid iff raw != 0 and zo <= zmax.
 *  6. Class of a rendered pixel with valid zo: take diff = zo - zr.  Exactly one class holds: consistent iff fabsf(diff) <= tau; occluded
 *     iff diff < -tau; violating iff diff > tau.  A rendered pixel without a valid zo is unknown.
 *  7. err_q20: the sum over the consistent pixels of (uint32)(fabsf(diff) * 1048576.0f), the product in f32 and truncated; a product of
 *     2^32 or more counts as 0xFFFFFFFF.
 * NaN or infinite rows of the model and non-finite entries of a pose fall out through the usable test: a pose of NaNs gives a result of
 * zeros, not an error.  For every pose n_rendered == n_consistent + n_occluded + n_violating + n_unknown.  The result is defined over the
 * whole frame: the kernels bound their work by each pose's pixel box, cut into tiles of TDV_VERIFY_TILE_W x TDV_VERIFY_TILE_H pixels
 * whose z-buffer lives in LDS (csrc/verify.hip), and none of that shows in a result.
 * h_order (optional): the pose indices by n_consistent - n_violating descending, ties to the lower index, computed on the host from the
 * integers.  tdv_verify_poses_dev takes the model and the raw u16 frame (row-major, the frame tdv_depth_to_cloud_dev reads) as device
 * pointers, the poses (n_poses x 16 floats, column-major each) and the results on the host, and reads back once; tdv_verify_poses takes
 * host arrays for the model and the frame too.  tdv_render_depth_dev writes the rendered depth of one pose as f32 (width x height, 0 where
 * nothing rendered) to device memory and the number of rendered pixels to *n_rendered (optional); it reads no frame, and of params it uses
 * pose_direction, splat and zmax (tau is checked all the same).  tdv_render_depth is its host form.
 * TDV_ERR_BAD_ARG before anything is enqueued or written: a NULL ctx, params, poses (n_poses > 0), results (n_poses > 0), model
 * (n_model > 0), frame or depth output (width * height > 0); n_model < 0 or > TDV_VERIFY_MAX_MODEL; n_poses < 0 or > TDV_VERIFY_MAX_POSES;
 * width or height < 0 or > TDV_VERIFY_MAX_SIDE; splat outside [0, TDV_VERIFY_MAX_SPLAT]; tau <= 0 or non-finite; scale, fx or fy <= 0 or
 * non-finite; an unknown pose_direction.  n_poses == 0 and n_model == 0 are valid and give zeros.  The ctx's switches do not apply.  Not
 * provided: per-instance masks, a splat chosen from the model's resolution, verification inside tdv_register_batch_dev, the C++
 * operator mirror.  A model that has faces is drawn by tdv_verify_poses_mesh, below. */
#define TDV_POSE_SOURCE_ONTO_TARGET 0
#define TDV_POSE_MODEL_TO_CAMERA 1
#define TDV_VERIFY_MAX_SPLAT 3
#define TDV_VERIFY_MAX_MODEL (1 << 22)
#define TDV_VERIFY_MAX_POSES 65536
#define TDV_VERIFY_MAX_SIDE 8192
#define TDV_VERIFY_TILE_W 128   /* 128 x 128 u32 = 64 KiB of LDS per workgroup: two workgroups per CU (csrc/verify.hip) */
#define TDV_VERIFY_TILE_H 128
#define TDV_VERIFY_LANES 1024   /* lanes of the workgroup that renders a tile */
typedef struct tdv_verify_params {
    int   pose_direction;  /* TDV_POSE_SOURCE_ONTO_TARGET (default) or TDV_POSE_MODEL_TO_CAMERA */
    int   splat;           /* half-width in pixels of the square each model point covers, 0..TDV_VERIFY_MAX_SPLAT; default 1 */
    float tau;             /* depth agreement band in metres, > 0; default 0.002 */
    float zmax;            /* as tdv_deproject: observed and rendered depths beyond it do not count; default 10 */
} tdv_verify_params;
void tdv_verify_default_params(tdv_verify_params* params);
typedef struct tdv_verify_result {   /* one per pose; every field an integer */
    int n_projected;     /* model points that pass the usable test (rules 2 and 3) */
    int n_rendered;      /* pixels of the frame that got a rendered depth */
    int n_consistent;    /* rendered pixels with a valid observed depth within tau */
    int n_occluded;      /* ... observed nearer than rendered by more than tau (something in front: explained) */
    int n_violating;     /* ... observed farther than rendered by more than tau (seen through: contradicts the pose) */
    int n_unknown;       /* rendered pixels with no valid observed depth */
    unsigned long long err_q20;   /* rule 7 */
} tdv_verify_result;
int tdv_verify_poses_dev(tdv_ctx* ctx, const float* d_model_xyz, int n_model, const float* h_poses /* host, n_poses x 16 */, int n_poses,
                         const uint16_t* d_raw_depth /* u16, width x height */, int width, int height, float scale, float fx, float fy, float cx,
                         float cy, const tdv_verify_params* params, tdv_verify_result* h_results /* host, [n_poses] */,
                         int* h_order /* optional, host, [n_poses] */);
int tdv_verify_poses(tdv_ctx* ctx, const float* model_xyz, int n_model, const float* poses, int n_poses, const uint16_t* raw_depth, int width,
                     int height, float scale, float fx, float fy, float cx, float cy, const tdv_verify_params* params,
                     tdv_verify_result* results, int* order /* optional */);
int tdv_render_depth_dev(tdv_ctx* ctx, const float* d_model_xyz, int n_model, const float* h_pose /* host, 16 */, int width, int height, float fx,
                         float fy, float cx, float cy, const tdv_verify_params* params, float* d_out_depth /* f32, width x height */,
                         int* n_rendered /* optional, host */);
int tdv_render_depth(tdv_ctx* ctx, const float* model_xyz, int n_model, const float* pose, int width, int height, float fx, float fy, float cx,
                     float cy, const tdv_verify_params* params, float* out_depth, int* n_rendered /* optional */);
/* Pose verification from a triangle mesh: the second renderer beside the splat.  The same poses, frame, classification, result struct and
 * one read-back; the model is an indexed triangle mesh (vertices n_vertices x 3 floats, triangles n_triangles x 3 ints) and its faces are
 * rasterised: an exact silhouette (no rim of splat pixels), a depth interpolated over each face, and with TDV_MESH_CULL_BACK only the faces
 * that look at the camera.  Every output is an integer or is fixed bit for bit: f32 and f64 as named, one rounding per operation, no
 * contraction, the order exactly as written; the integers are exact.
 *  M1. Vertex: camera coordinates, the usable test and uf, vf are rules 1 to 3 above (usable: xc, yc, zc finite, 0 < zc <= zmax, and
 *      |uf|, |vf| < 2^20).  The snapped position is X = (int64)floorf(uf * 16.0f + 0.5f), Y likewise from vf (TDV_MESH_SUBPIXEL = 16:
 *      multiples of 1/16 pixel).  Pixel (x, y) has its centre at (16 x, 16 y): the convention of rule 3's floorf(uf + 0.5f) and of
 *      tdv_deproject.
 *  M2. Triangle (a, b, c).  It is unusable if an index lies outside [0, n_vertices) - tested on the device before anything is read, so a
 *      bad index reads no memory - or if one of its vertices is unusable.  There is NO near-plane clipping: a triangle with a vertex behind
 *      the camera or beyond zmax is dropped whole.  A = (Xb - Xa) * (Yc - Ya) - (Yb - Ya) * (Xc - Xa) in int64 (exact: every factor is
 *      below 2^26).  A == 0: unusable.  A > 0 means the normal (vb - va) x (vc - va) points away from the camera (image y grows
 *      downwards): under TDV_MESH_CULL_BACK such a triangle is unusable.  A triangle with A < 0 - one that looks at the camera - has b and c
 *      swapped and A negated, so every usable triangle goes on with A > 0.  (The rule as first drafted swapped the triangles with A > 0 instead,
 *      which leaves every A negative and rule M4's "E > 0 inside" without a covered pixel; the swap is stated here as M4 needs it, and
 *      nothing else changed.)
 *  M3. n_projected is the number of usable triangles, whether or not they cover a pixel of the frame.
 *  M4. Coverage.  After M2 each directed edge i -> j has E(P) = (Xj - Xi) * (Py - Yi) - (Yj - Yi) * (Px - Xi) at the pixel centre P, in
 *      int64; w0 = E_bc, w1 = E_ca, w2 = E_ab, and w0 + w1 + w2 = A.  The pixel is covered iff for every edge E > 0, or E == 0 and the edge
 *      owns its boundary.  An edge owns its boundary when Yj - Yi < 0, or Yj - Yi == 0 and Xj - Xi > 0 (with A > 0 and y downwards these
 *      are the left edges and the horizontal top edge: the top-left rule).  Two usable triangles of one facing that share an edge walk it in
 *      opposite directions, so a centre on it belongs to exactly one of them.
 *  M5. Depth of a covered pixel, perspective-correct in f64: iz_i = 1.0 / (double)zc_i for the vertices after M2's swap;
 *      s = ((double)w0 * iz_a + (double)w1 * iz_b) + (double)w2 * iz_c; zr = (float)((double)A / s).  zr lies within the vertices' depths:
 *      positive, finite and <= zmax.
 *  M6. Rendered depth of a pixel: the minimum zr over the triangles that cover it, taken over the u32 bits as in rule 4.  Only pixels of
 *      the frame are rendered; a triangle partly or wholly outside the frame covers what it covers inside.
 *  M7. Rules 5 to 7 and the classes are those above, unchanged (one implementation: csrc/verify_common.hpp).
 * tdv_verify_result is reused: n_projected counts the usable triangles (M3), every other field keeps its meaning, and for every pose
 * n_rendered == n_consistent + n_occluded + n_violating + n_unknown.  h_order is the splat's (same code).  A vertex of NaNs or infinities
 * takes its triangles out through the usable test, a pose of NaNs gives a result of zeros.  Vertices no triangle names are never read.
 * The result is defined over the whole frame.  The kernels (csrc/verify_mesh.hip) cut each pose's pixel box into the splat's tiles; in a
 * tile a lane rasterises a triangle itself when the triangle's pixel box inside the tile holds at most TDV_MESH_COOP_PIXELS pixels, larger
 * ones go through a queue of TDV_MESH_QUEUE setup records in LDS that the workgroup drains together, one pixel per lane.  Neither constant
 * shows in a result; they are exported so that tests can stand on their edges.
 * tdv_verify_poses_mesh_dev takes vertices, triangles and the raw frame as device pointers, poses and results on the host, and reads back
 * once; tdv_verify_poses_mesh takes host arrays throughout.  tdv_render_depth_mesh_dev writes the rendered depth of one pose as f32 (0 where
 * nothing rendered) and the number of rendered pixels; of params it uses pose_direction, cull and zmax (tau is checked all the same).
 * TDV_ERR_BAD_ARG before anything is enqueued or written: a NULL ctx, params, poses (n_poses > 0), results (n_poses > 0), vertices
 * (n_vertices > 0), triangles (n_triangles > 0), frame or depth output (width * height > 0); n_vertices < 0 or > TDV_MESH_MAX_VERTICES;
 * n_triangles < 0 or > TDV_MESH_MAX_TRIANGLES; n_poses, width, height outside the splat's limits; an unknown cull or pose_direction; tau,
 * scale, fx or fy <= 0 or non-finite.  n_triangles == 0, n_vertices == 0 and n_poses == 0 are valid and give zeros.  Not provided: mesh
 * file loaders, near-plane clipping, per-instance masks, verification inside tdv_register_batch_dev, the C++ operator mirror. */
#define TDV_MESH_CULL_NONE 0
#define TDV_MESH_CULL_BACK 1
#define TDV_MESH_MAX_VERTICES (1 << 22)
#define TDV_MESH_MAX_TRIANGLES (1 << 22)
#define TDV_MESH_SUBPIXEL 16      /* snapped positions are multiples of 1/16 pixel */
#define TDV_MESH_COOP_PIXELS 64   /* a pixel box inside a tile of more pixels than this is rasterised by the workgroup together */
#define TDV_MESH_QUEUE 128        /* setup records of 64 bytes in LDS: 8 KiB beside the 64 KiB tile (csrc/verify_mesh.hip) */
typedef struct tdv_mesh_verify_params {
    int   pose_direction;  /* TDV_POSE_SOURCE_ONTO_TARGET (default) or TDV_POSE_MODEL_TO_CAMERA */
    int   cull;            /* TDV_MESH_CULL_NONE (default) or TDV_MESH_CULL_BACK (rule M2) */
    float tau;             /* depth agreement band in metres, > 0; default 0.002 */
    float zmax;            /* observed and rendered depths beyond it do not count; default 10 */
} tdv_mesh_verify_params;
void tdv_mesh_verify_default_params(tdv_mesh_verify_params* params);
int tdv_verify_poses_mesh_dev(tdv_ctx* ctx, const float* d_vertices, int n_vertices, const int* d_triangles, int n_triangles,
                              const float* h_poses /* host, n_poses x 16 */, int n_poses, const uint16_t* d_raw_depth /* u16, width x height */,
                              int width, int height, float scale, float fx, float fy, float cx, float cy, const tdv_mesh_verify_params* params,
                              tdv_verify_result* h_results /* host, [n_poses] */, int* h_order /* optional, host, [n_poses] */);
int tdv_verify_poses_mesh(tdv_ctx* ctx, const float* vertices, int n_vertices, const int* triangles, int n_triangles, const float* poses,
                          int n_poses, const uint16_t* raw_depth, int width, int height, float scale, float fx, float fy, float cx, float cy,
                          const tdv_mesh_verify_params* params, tdv_verify_result* results, int* order /* optional */);
int tdv_render_depth_mesh_dev(tdv_ctx* ctx, const float* d_vertices, int n_vertices, const int* d_triangles, int n_triangles,
                              const float* h_pose /* host, 16 */, int width, int height, float fx, float fy, float cx, float cy,
                              const tdv_mesh_verify_params* params, float* d_out_depth /* f32, width x height */,
                              int* n_rendered /* optional, host */);
int tdv_render_depth_mesh(tdv_ctx* ctx, const float* vertices, int n_vertices, const int* triangles, int n_triangles, const float* pose, int width,
                          int height, float fx, float fy, float cx, float cy, const tdv_mesh_verify_params* params, float* out_depth,
                          int* n_rendered /* optional */);
/* Mesh sampling (Open3D's TriangleMesh::sample_points_uniformly): n_samples points drawn uniformly over the surface of an indexed triangle
 * mesh, each with the exact outward normal of its face - the step from a model that is a mesh (tdv_verify_poses_mesh) to the points and
 * normals every other stage takes (tdv_ppf_model_dev, tdv_prepare_model_dev, the ICP entry points, the splat verifier).  Thinned with
 * tdv_farthest_point_down_sample_dev it is the even-spread model of sample_points_poisson_disk (oversample and eliminate; the Python
 * front end composes the two as Context.mesh_model).  The random numbers are counter-based, the choice of a triangle and the barycentric
 * coordinates are integers, and the floats are f32 with one rounding per operation, no contraction, the expression evaluated as written
 * (sqrtf and / correctly rounded), so every output is fixed bit for bit whatever order the device works in:
 *  S1. Triangle (a, b, c) of vertex indices.  It is bad if an index lies outside [0, n_vertices) - tested on the device before any vertex is
 *      read, so a bad index reads no memory - or if one of its nine coordinates is not finite.  Vertices no triangle names are never read.
 *  S2. Normal and area: e1 = vb - va, e2 = vc - va per component; n = (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z, e1x*e2y - e1y*e2x);
 *      L = sqrtf((nx*nx + ny*ny) + nz*nz); area = 0.5f * L.  A non-finite area (an overflow, or the NaN of inf - inf) makes the triangle
 *      bad.  The orientation is rule M2's (vb - va) x (vc - va): outwards for a mesh wound as tdv_verify_poses_mesh's TDV_MESH_CULL_BACK
 *      expects.
 *  S3. Integer weights.  area_max = the largest area over the triangles that are not bad: an order-free maximum over the u32 bits of a
 *      non-negative f32; 0 without such a triangle.  area_max == 0: e = 0 and every weight is 0.  Otherwise e = floor(log2(area_max)), read
 *      from the exponent field of (double)area_max (exact for f32 subnormals too), and w_t = (uint64)((double)area_t * 2^(31 - e)),
 *      truncated; a bad triangle has w_t = 0.  The scaling is by a power of two and exact, w_t < 2^32, and the largest triangle has
 *      w >= 2^31.  W = the sum of the w_t, below 2^54, and C_t = w_0 + ... + w_t, the inclusive prefix sum in triangle order: integers, so
 *      any scan order gives the same C.  A triangle whose area is below 2^-32 of the largest has weight 0 and is never chosen: the price of
 *      integer weights, stated and not hidden.  (Between 2^-32 and 2^-8 of the largest a weight carries fewer than 24 bits: its share of
 *      the samples is its truncated weight's, off by less than 1 / w_t of itself.)
 *  S4. Sample k of the call has the global index g = first_sample + k (uint64).  x = philox4x32_10(counter ((uint32)g, (uint32)(g >> 32),
 *      0, 0), key (seed, 2)): key word 2 is this stage's tag (tdv_fgr draws with 0, tdv_segment_planes with 1).
 *      target = mulhi64(((uint64)x0 << 32) | x1, W), the high 64 bits of the 128-bit product: in [0, W).  The sample's triangle is the
 *      smallest t with C_t > target; a triangle of weight 0 can never be it.
 *  S5. Barycentric coordinates on integers: i1 = x2 >> 8, i2 = x3 >> 8; if i1 + i2 > 2^24 then i1 = 2^24 - i1 and i2 = 2^24 - i2 (the
 *      reflection of the unit square's far half onto the near one).  u = i1 * 2^-24, v = i2 * 2^-24, w = (2^24 - i1 - i2) * 2^-24: all
 *      three exact in f32, none negative, and u + v + w == 1 exactly.
 *  S6. Outputs of sample k, each optional (NULL to skip), rows beyond n_sampled not written:
 *      out_xyz[3k..]      (w*va + u*vb) + v*vc per coordinate
 *      out_normals[3k..]  n / L per component: the face normal of S2 (L > 0 where w_t > 0)
 *      out_triangle[k]    t
 *      out_bary[2k..]     (u, v)
 *      out_attr[width k..] (w*Aa + u*Ab) + v*Ac per column of one per-vertex companion array attr (n_vertices x attr_width floats:
 *                         vertex normals or colours, interpolated as Open3D interpolates them, not renormalised); needs attr.
 *  S7. Sample g depends on the mesh, seed and g only: the rows of a call with (first_sample = f, n_samples = n) are rows f .. f + n - 1
 *      of the call with (0, f + n).  A caller can draw in chunks, or extend a sample it has.
 * result: n_bad (S1, S2), n_usable (w_t > 0), n_degenerate (not bad, w_t == 0: zero area, or below 2^-32 of the largest) - the three sum to
 * n_triangles -, n_sampled = n_samples if n_usable > 0, else 0; weight_exponent = e, area_max, total_weight = W.  The surface area the
 * weights stand for is ldexp((double)total_weight, weight_exponent - 31): one rounding, the conversion of W (below 2^54) to double; the
 * scaling is exact.  n_triangles == 0 gives a result of zeros.  n_samples == 0 fills the mesh's fields and writes nothing.  A mesh without a
 * usable triangle gives n_sampled == 0 and writes nothing.
 * Kernels (csrc/mesh_sample.hip): one pass over the triangles (areas, n_bad, area_max through one u32 atomic maximum per workgroup),
 * the weights and their 64-bit inclusive scan in three plain launches (workgroup sums, one workgroup over the sums, add back - no kernel
 * waits on another workgroup), then one lane per sample: Philox, the 64 x 64 high product, a branch-free upper-bound search over C (22
 * steps at most, the coarse ones over a table of at most 4,096 entries staged in LDS), three vertex fetches, the row stores.
 * tdv_mesh_sample_points takes host arrays and reads back twice (the result, then the n_sampled rows); tdv_mesh_sample_points_dev takes
 * device pointers, the result on the host, and reads back once, the result.
 * TDV_ERR_BAD_ARG before anything is enqueued or written: a NULL ctx, params or result; NULL vertices with n_vertices > 0 or NULL triangles
 * with n_triangles > 0; n_vertices < 0 or > TDV_MESH_MAX_VERTICES; n_triangles < 0 or > TDV_MESH_MAX_TRIANGLES; n_samples < 0 or
 * > TDV_MESH_SAMPLE_MAX; first_sample + n_samples beyond 2^64 - 1; attr_width < 0; attr_width > 0 with a NULL attr; out_attr without attr.
 * The ctx's switches do not apply.  Not provided: mesh file loaders, per-triangle densities, blue-noise elimination other than farthest
 * point sampling, the C++ operator mirror. */
#define TDV_MESH_SAMPLE_MAX (1 << 24)
typedef struct tdv_mesh_sample_params {
    uint32_t seed;           /* default 0 */
    uint64_t first_sample;   /* the global index of the call's sample 0 (S7); default 0 */
} tdv_mesh_sample_params;
void tdv_mesh_sample_default_params(tdv_mesh_sample_params* params);
typedef struct tdv_mesh_sample_result {
    int      n_usable;          /* triangles with weight > 0 */
    int      n_degenerate;      /* indices in range, coordinates and area finite, weight 0 */
    int      n_bad;             /* an index out of range, a non-finite coordinate or a non-finite area */
    int      n_sampled;         /* n_samples if n_usable > 0, else 0 */
    int      weight_exponent;   /* e of rule S3 */
    float    area_max;
    uint64_t total_weight;      /* W of rule S3 */
} tdv_mesh_sample_result;
int tdv_mesh_sample_points(tdv_ctx* ctx, const float* vertices, int n_vertices, const int* triangles, int n_triangles,
                           const float* attr /* optional, per vertex */, int attr_width, int n_samples, const tdv_mesh_sample_params* params,
                           tdv_mesh_sample_result* result, float* out_xyz /* optional */, float* out_normals /* optional */,
                           int* out_triangle /* optional */, float* out_bary /* optional */, float* out_attr /* optional */);
int tdv_mesh_sample_points_dev(tdv_ctx* ctx, const float* d_vertices, int n_vertices, const int* d_triangles, int n_triangles,
                               const float* d_attr /* optional, per vertex */, int attr_width, int n_samples,
                               const tdv_mesh_sample_params* params, tdv_mesh_sample_result* result /* host */, float* d_out_xyz /* optional */,
                               float* d_out_normals /* optional */, int* d_out_triangle /* optional */, float* d_out_bary /* optional */,
                               float* d_out_attr /* optional */);
/* TSDF fusion (Open3D's UniformTSDFVolume::integrate and extract_point_cloud; Curless and Levoy 1996): several raw depth frames taken at
 * known camera poses are fused into one truncated signed distance volume, and the volume's zero crossings come out as one cloud whose
 * normals are the gradient of the fused field - measured, not fitted to a neighbourhood.  Noise is averaged over the frames that saw a
 * voxel and a surface seen twice comes out once.  A voxel's update depends on that voxel and one pixel per frame, and the frames apply
 * in ascending index, so with f32, one rounding per operation, no contraction and the order exactly as written every output is fixed bit
 * for bit whatever order the device works in (sqrtf and / correctly rounded).
 * The volume is a caller-owned device buffer of nx*ny*nz pairs (f32 tsdf, f32 weight), tdv_tsdf_volume_bytes(vol) bytes; voxel (i, j, k)
 * sits at pair index (k*ny + j)*nx + i.  The layout is public.  tdv_tsdf_reset_dev makes every pair (1.0f, 0.0f).
 *  T1. Voxel centre: xw = origin[0] + ((float)i + 0.5f) * voxel_length, and yw (j, origin[1]), zw (k, origin[2]) likewise.
 *  T2. Camera coordinates of the centre under the frame's pose T: rule 1 of tdv_verify_poses for params->pose_direction, the voxel
 *      centre standing in for m.  TDV_POSE_MODEL_TO_CAMERA (the default): T takes the volume's frame to the camera's, Open3D's extrinsic.
 *      TDV_POSE_SOURCE_ONTO_TARGET: T is the camera's pose in the volume's frame.
 *  T3. Usable: xc, yc, zc are finite and 0 < zc <= zmax; uf = (xc*fx)/zc + cx and vf = (yc*fy)/zc + cy are finite and below 2^20 in
 *      magnitude; u = (int)floorf(uf + 0.5f), v likewise, and 0 <= u < width, 0 <= v < height.
 *  T4. Observed depth of frame f at (u, v): rule 5 of tdv_verify_poses, zo = float(raw) * float(1.0 / scale), valid iff raw != 0 and
 *      zo <= zmax.
 *  T5. Update: sdf = zo - zc, projective along z.  A voxel with sdf < -trunc is not touched (sdf == -trunc is updated).  Otherwise
 *      t = fminf(1.0f, sdf / trunc); tsdf' = (tsdf*w + t) / (w + 1.0f); w' = fminf(w + 1.0f, max_weight).  trunc is params->trunc, or
 *      4.0f * voxel_length where that is 0.  The frames of a call apply to a voxel in ascending frame index, and a call with frames A, B
 *      leaves what a call with A and then a call with B leave.  h_n_updated[f] = the number of voxels frame f updated.
 *  T6. Observed voxel: w >= min_weight.
 *  T7. Crossings.  For an observed voxel a and its +x, +y or +z neighbour b, inside the volume and observed: they bracket the surface
 *      iff (f_a < 0) != (f_b < 0) - zero counts as non-negative.  With r_a = fabsf(f_a), r_b = fabsf(f_b) the point is a's centre with its
 *      coordinate on that axis replaced by (c_a*r_b + c_b*r_a) / (r_a + r_b), c_a and c_b the two centres' coordinates on the axis (T1);
 *      the denominator is positive by construction.  Output order: ascending 3*voxel_index + axis (x = 0, y = 1, z = 2).
 *  T8. Normal.  Per axis the gradient at a voxel is f(fwd) - f(bwd), its two neighbours on the axis; a neighbour outside the volume or not
 *      observed is replaced by the voxel itself; if exactly one of the two is replaced the difference is multiplied by 2.0f; if both are,
 *      it is 0.  The crossing's normal is n = g_a*r_b + g_b*r_a per component, L = sqrtf((nx*nx + ny*ny) + nz*nz), and the row is n / L per
 *      component, or (0, 0, 0) where L is zero or not finite.  A positive tsdf is in front of the surface, so the normal points out of the
 *      object, towards where it was seen from.
 * The mesh (Open3D's extract_triangle_mesh; marching cubes, Lorensen and Cline 1987): vertex v of the mesh IS row v of
 * tdv_tsdf_extract_dev's cloud, same bytes and same normals, and the new output is the triangle list over those rows.  A crossing that
 * no triangle uses stays in the vertex array unreferenced (at the rim of the observed region, where a cell has an unobserved corner).
 *  T9. Cell.  Cell (i, j, k) exists for 0 <= i < nx-1, 0 <= j < ny-1, 0 <= k < nz-1; a volume with a side of 1 has no cell.  Its corner q,
 *      q = 0..7, is voxel (i + (q&1), j + ((q>>1)&1), k + ((q>>2)&1)).  The cell is usable iff all eight corners are observed (T6).  Its
 *      case is the sum of 1 << q over the corners with f_q < 0; zero and negative zero count as non-negative, as in T7.
 *  T10. Cell edge.  e = 4*axis + idx, and its owner is the corner at which it starts: x: idx = dy + 2*dz, owner (0, dy, dz); y: idx =
 *      dx + 2*dz, owner (dx, 0, dz); z: idx = dx + 2*dy, owner (dx, dy, 0).  Its vertex is T7's crossing with key 3*voxel_index(owner) +
 *      axis: in a usable cell every edge whose ends differ in sign is one of T7's crossings.  The vertex index is the rank of that key
 *      among T7's keys, which is the row number in tdv_tsdf_extract_dev's output.
 *  T11. The table (256 cases), by rule; tools/gen_tsdf_mc_table.py makes csrc/tsdf_mc_table.hpp from it.
 *      1. Segments.  Each of the cube's six faces has 0, 2 or 4 edges that cross.  With 2, one segment joins them.  With 4 the two
 *         negative corners lie on a diagonal, and each is cut off on its own: a segment joins the two face edges that meet at it.  A
 *         face's segments depend on that face's four signs only, so the two cells that share a face draw the same segments.
 *      2. Loops.  Every crossing edge lies on exactly two segments, so the segments chain into closed loops.
 *      3. Direction.  A loop is listed from its smallest edge number.  With m_e the midpoint of edge e on the unit cube, N = the sum of
 *         m_i x m_(i+1), cyclic over the loop, and D = the sum over the loop's edges of (the non-negative end - the negative end), the
 *         direction is the one with N . D > 0 (it is never 0).
 *      4. A case's loops come in ascending order of their smallest edge.
 *      5. Triangles.  The loop is rotated to start at the first position r = 0, 1, ... for which no fan diagonal (m_0, m_i),
 *         2 <= i <= n-2, joins two edges that lie on a common cube face (such an r exists); the triangles are then (m_0, m_i, m_(i+1))
 *         for i = 1 .. n-2.  Without the rotation a diagonal inside an ambiguous face would be drawn by both cells that share the face.
 *      820 triangles in all, at most TDV_TSDF_MC_MAX_TRIANGLES in a case; the mesh is watertight wherever the cells are usable.
 *  T12. Output.  A triangle is a row of three int32 vertex indices.  Rows come in ascending cell index (k*ny + j)*nx + i, and within a
 *      cell in the table's order.  (vb - va) x (vc - va) points to the non-negative side: T8's normal side, the front face under
 *      TDV_MESH_CULL_BACK, tdv_mesh_sample_points' outward normal.  A triangle of zero area (a corner's value is exactly 0 and the three
 *      crossings at it coincide) is emitted like any other; the sampler and the verifier set such triangles aside.
 * tdv_tsdf_integrate_dev: d_raw holds n_frames u16 images (width x height, row-major) back to back on the device, h_poses n_frames x 16
 * floats (column-major each) on the host; h_n_updated (optional, host, [n_frames]) costs the call its one read-back.  All frames of a call
 * are integrated in one pass over the volume.  n_frames == 0 is valid and leaves the volume as it is.  NaN or infinite pose entries fall
 * out through T3: such a frame updates nothing.
 * tdv_tsdf_extract_dev: d_out_xyz and d_out_normals (optional) receive *n_out rows of 3 floats; capacity = their room in rows, n_out on
 * the host.  If capacity is too small (NULL d_out_xyz with capacity 0 is a query) the call returns TDV_ERR_BAD_ARG with *n_out set to the
 * needed count and no row written, as tdv_deproject does.  One read-back, the count.
 * tdv_tsdf_fuse: host arrays throughout - reset, integrate and extract with the volume in the ctx's workspace; volumes above
 * TDV_TSDF_HOST_MAX_VOXELS are refused.
 * tdv_tsdf_extract_mesh_dev: d_out_vertices and d_out_normals (optional) receive *n_vertices rows of 3 floats, tdv_tsdf_extract_dev's
 * rows; d_out_triangles receives *n_triangles rows of 3 ints (T12).  If either capacity is too small (NULL outputs with capacity 0 are a
 * query) the call returns TDV_ERR_BAD_ARG with both counts set and nothing written.  One read-back: both counts in one copy.
 * tdv_tsdf_fuse_mesh: tdv_tsdf_fuse with the mesh outputs, host arrays throughout.
 * Kernels (csrc/tsdf.hip): integrate is one launch per call, a lane per voxel, the pair loaded and stored once (and not at all where no
 * frame updates it), the poses read through scalar loads.  Extract stages tiles of TDV_TSDF_TILE_X x _Y x _Z voxels with their halo in
 * LDS, counts the crossings per run of TDV_TSDF_TILE_X voxels along x, scans the counts (no atomic decides an output position) and
 * writes the rows.  The mesh counts the triangles of a run's cells in the same pass as its crossings, scans both, and a lane per cell
 * writes the triangles; a vertex index is the run offset of the edge's owner voxel plus the crossings ranked before it, from ballots kept
 * in LDS.  Its workspace is a few ints per run.
 * TDV_ERR_BAD_ARG before anything is enqueued or written: a NULL ctx, vol, params, volume buffer, frames or poses (n_frames > 0), n_out,
 * n_vertices, n_triangles, or d_out_xyz / d_out_vertices / d_out_triangles with its capacity > 0; a side < 1 or > TDV_TSDF_MAX_SIDE; nx*ny*nz above TDV_TSDF_MAX_VOXELS (tdv_tsdf_fuse:
 * TDV_TSDF_HOST_MAX_VOXELS); voxel_length, scale, fx or fy <= 0 or non-finite; trunc < 0 or non-finite; max_weight < 1 or non-finite;
 * min_weight <= 0 or non-finite; n_frames < 0 or > TDV_TSDF_MAX_FRAMES; width or height < 0 or > TDV_VERIFY_MAX_SIDE; an unknown
 * pose_direction; capacity < 0.  The ctx's switches do not apply.
 * Not provided: per-frame masks (a caller zeroes the pixels), per-frame weights, a hashed or sparse volume, the C++ operator mirror, a
 * coloured sequence tracker (today a loop over tdv_tsdf_track_dev and tdv_tsdf_integrate_color_dev), a colour term in tracking and
 * odometry.  Colour: tdv_tsdf_integrate_color_dev, below.  Ray casting and tracking against the volume: tdv_tsdf_raycast_dev, below. */
typedef struct tdv_tsdf_volume { float origin[3]; float voxel_length; int nx, ny, nz; } tdv_tsdf_volume;   /* 28 bytes */
typedef struct tdv_tsdf_params {   /* 20 bytes */
    float trunc;           /* truncation distance in metres; default 0, which means 4.0f * voxel_length */
    float max_weight;      /* default 255 */
    float zmax;            /* as tdv_deproject; default 10 */
    float min_weight;      /* T6; default 1 */
    int   pose_direction;  /* TDV_POSE_MODEL_TO_CAMERA (default) or TDV_POSE_SOURCE_ONTO_TARGET */
} tdv_tsdf_params;
#define TDV_TSDF_MAX_SIDE 1024
#define TDV_TSDF_MAX_VOXELS (1 << 27)      /* 1 GiB of volume */
#define TDV_TSDF_HOST_MAX_VOXELS (1 << 25) /* the host form keeps its volume in the ctx's workspace */
#define TDV_TSDF_MAX_FRAMES 64             /* per integrate call */
#define TDV_TSDF_TILE_X 64   /* the tile k_tsdf_extract stages in LDS; a wave owns a run of TILE_X voxels along x */
#define TDV_TSDF_TILE_Y 8
#define TDV_TSDF_TILE_Z 8
#define TDV_TSDF_MC_MAX_TRIANGLES 5        /* T11: the most triangles of one cell */
void tdv_tsdf_default_params(tdv_tsdf_params* params);
unsigned long long tdv_tsdf_volume_bytes(const tdv_tsdf_volume* vol);
int tdv_tsdf_reset_dev(tdv_ctx* ctx, const tdv_tsdf_volume* vol, float* d_volume);
int tdv_tsdf_integrate_dev(tdv_ctx* ctx, const tdv_tsdf_volume* vol, float* d_volume, const uint16_t* d_raw /* n_frames images */, int n_frames,
                           int width, int height, float scale, float fx, float fy, float cx, float cy,
                           const float* h_poses /* host, n_frames x 16 */, const tdv_tsdf_params* params,
                           long long* h_n_updated /* optional, host, [n_frames] */);
int tdv_tsdf_extract_dev(tdv_ctx* ctx, const tdv_tsdf_volume* vol, const float* d_volume, const tdv_tsdf_params* params, float* d_out_xyz,
                         float* d_out_normals /* optional */, int capacity, int* n_out /* host */);
int tdv_tsdf_fuse(tdv_ctx* ctx, const tdv_tsdf_volume* vol, const uint16_t* raw, int n_frames, int width, int height, float scale, float fx,
                  float fy, float cx, float cy, const float* poses, const tdv_tsdf_params* params, float* out_xyz,
                  float* out_normals /* optional */, int capacity, int* n_out);
int tdv_tsdf_extract_mesh_dev(tdv_ctx* ctx, const tdv_tsdf_volume* vol, const float* d_volume, const tdv_tsdf_params* params,
                              float* d_out_vertices, float* d_out_normals /* optional */, int vertex_capacity, int* n_vertices /* host */,
                              int* d_out_triangles, int triangle_capacity, int* n_triangles /* host */);
int tdv_tsdf_fuse_mesh(tdv_ctx* ctx, const tdv_tsdf_volume* vol, const uint16_t* raw, int n_frames, int width, int height, float scale,
                       float fx, float fy, float cx, float cy, const float* poses, const tdv_tsdf_params* params, float* out_vertices,
                       float* out_normals /* optional */, int vertex_capacity, int* n_vertices, int* out_triangles, int triangle_capacity,
                       int* n_triangles);
/* TSDF ray casting and frame-to-model tracking (KinectFusion, Newcombe et al. 2011; Open3D's VoxelBlockGrid ray_cast): the fused volume
 * seen from a camera pose - a depth image, a vertex map and a normal map without holes or splats - and the next frame registered against
 * that view of the model instead of against the frame before, so that a sequence's drift is held by everything fused so far.  Every
 * pixel's march is independent, every loop is bounded, and all arithmetic is f32, one rounding per operation, no contraction, the order
 * exactly as written (sqrtf and / correctly rounded): every output is fixed bit for bit whatever order the device works in.  The rules
 * continue T1 to T12; the odometry's are O1 to O10 below.
 *  T13. Ray.  The point of pixel (u, v) at camera depth z is O2's vertex, c = ((((float)u - cx) * z) / fx, (((float)v - cy) * z) / fy, z).
 *      Its volume-frame point p under the pose T (column-major): TDV_POSE_SOURCE_ONTO_TARGET - T is the camera's pose in the volume's
 *      frame - p0 = ((T[0]*c0 + T[4]*c1) + T[8]*c2) + T[12], p1 = ((T[1]*c0 + T[5]*c1) + T[9]*c2) + T[13],
 *      p2 = ((T[2]*c0 + T[6]*c1) + T[10]*c2) + T[14]: rule 1's model-to-camera form applied to c.  TDV_POSE_MODEL_TO_CAMERA: d = c -
 *      (T[12], T[13], T[14]) per component and p0 = (T[0]*d0 + T[1]*d1) + T[2]*d2, p1 = (T[4]*d0 + T[5]*d1) + T[6]*d2,
 *      p2 = (T[8]*d0 + T[9]*d1) + T[10]*d2: rule 1's other form.  The march runs in z, not in ray length: the z of a hit is directly the
 *      depth image O1 to O3 and T4 work with.
 *  T14. Field sample F(p).  Per axis a: g_a = (p_a - origin[a]) / voxel_length - 0.5f, i_a = floorf(g_a), t_a = g_a - i_a.  The sample is
 *      known iff every g_a is finite, g_a >= 0 and g_a < (float)(n_a - 1), all eight voxels (i0 + dx, i1 + dy, i2 + dz), dx, dy, dz in
 *      {0, 1}, are observed (T6), and the value below is not NaN; the g_a are judged as floats, before any conversion to int.  With
 *      lerp(a, b, t) = a + t * (b - a): four lerps along x, x_(dy dz) = lerp(f(0, dy, dz), f(1, dy, dz), t_0); two along y,
 *      y_dz = lerp(x_(0 dz), x_(1 dz), t_1); one along z, F = lerp(y_0, y_1, t_2).  A volume with a side of 1 has no known sample.
 *  T15. March.  z_0 = zmin.  At sample k = 0, 1, ...: if !(z_k <= zmax) or k == max_steps the ray ends without a hit.  Otherwise
 *      s_k = F(p(z_k)) by T13 and T14.  Unknown: z_(k+1) = z_k + trunc.  Known and s_k >= 0: z_(k+1) = z_k + fmaxf(s_k * trunc,
 *      voxel_length), Open3D's ray-cast stride.  Known and s_k < 0: the ray ends, and it is a hit iff k > 0 and sample k-1 was known;
 *      sample k-1 is then non-negative.  A back face, or a camera inside the surface, gives no hit.  trunc is T5's, zmax params->zmax.
 *  T16. Hit depth: z = fminf(z_(k-1) + ((z_k - z_(k-1)) * s_(k-1)) / (s_(k-1) - s_k), z_k); the denominator is positive, and z > 0.
 *  T17. Vertex: O2's vertex of (u, v) at that z.
 *  T18. Normal.  With p the hit's volume-frame point (T13 at T16's z) and L = voxel_length: G_a = F(p + L e_a) - F(p - L e_a), only
 *      component a of p changed.  The normal is absent, (0, 0, 0), if any of the six samples is unknown.  Into the camera's frame:
 *      source-onto-target n0 = (T[0]*G0 + T[1]*G1) + T[2]*G2, n1 = (T[4]*G0 + T[5]*G1) + T[6]*G2, n2 = (T[8]*G0 + T[9]*G1) + T[10]*G2;
 *      model-to-camera n0 = (T[0]*G0 + T[4]*G1) + T[8]*G2, n1 = (T[1]*G0 + T[5]*G1) + T[9]*G2, n2 = (T[2]*G0 + T[6]*G1) + T[10]*G2.  Then
 *      T8's normalisation: L = sqrtf((n0*n0 + n1*n1) + n2*n2), the row n / L per component, (0, 0, 0) where L is zero or not finite.  A
 *      surface seen from the front gets a normal towards the camera: O3's sign.
 * tdv_tsdf_raycast_dev: the volume from h_pose (host, 16 floats, column-major, params->pose_direction).  Of params it uses trunc, zmax,
 * min_weight and pose_direction (the others are checked all the same).  d_depth: width*height floats, 0.0f where the ray has no hit;
 * d_vertex_map and d_normal_map: width*height*3 floats in camera coordinates, tdv_depth_maps_dev's layout, zeros where there is no hit
 * resp. no normal.  Every output is optional; h_n_hit (optional, host) is the number of rays that hit - the non-zero depths - and costs
 * the call its only read-back.  width*height == 0 is valid and writes nothing.  NaN or infinite pose entries fall out through T14: no
 * sample is known, so nothing hits.  The step cap makes every ray finite whatever the arguments - a voxel_length below an ulp of z
 * marches to the cap and ends.  tdv_tsdf_raycast is the host form: the volume (nx*ny*nz pairs) goes up through the ctx's workspace;
 * volumes above TDV_TSDF_HOST_MAX_VOXELS are refused.
 * Tracking.  tdv_tsdf_track_dev: one raw frame (device) against the volume from the guess G (host, 16 floats) - the camera's pose in the
 * volume's frame, typically the frame before's; params->pose_direction must be TDV_POSE_SOURCE_ONTO_TARGET, the direction O9 produces.
 *  K1. The volume is ray cast at G (T13 to T16) into a depth image in the ctx's workspace; n_hit is its count of hits.
 *  K2. tdv_depth_odometry_to_depth_dev with the frame as the source and that image as the target, from the identity: odom.
 *  K3. pose = G * odom.T by O9's product: each entry the f64 sum of four f64 products in index order, rounded once to f32.
 * The result is byte for byte what the three public steps give on the same ctx, in one read-back.  width*height == 0: pose = G * I, zeros.
 * tdv_tsdf_track_sequence_dev: d_raw holds n_frames images back to back.  Frame 0 is integrated (T1 to T5) at P_0 = h_pose0 (NULL: the
 * identity); for k >= 1 frame k is tracked from the guess P_(k-1) and then integrated at P_k.  h_poses (host, n_frames x 16) receives the
 * P_k, h_results (optional, host, [n_frames]) the frames' results, entry 0 holding P_0 and zeros.  The volume is taken as it is: a caller
 * resets it first.  The cost is one read-back per frame - the pose has to reach the host for K3 and for integrate's h_poses.  Per frame
 * the pose and the result, and the volume at the end, are byte for byte those of a loop over the public calls.  n_frames of 0 or 1 is
 * valid.
 * Kernel (csrc/tsdf_raycast.hip): one launch, a lane per pixel, a wave per 8 x 8 pixel tile so that neighbouring rays' eight pair loads
 * share lines, a pair loaded as 8 bytes, the pose read through scalar loads; no LDS but the hit count's four ints and no atomic but that
 * count's one per workgroup.
 * TDV_ERR_BAD_ARG before anything is enqueued or written: as tdv_tsdf_extract_dev for ctx, vol, the volume buffer and params, as
 * tdv_render_depth_dev for width, height, fx, fy and a NULL pose; a NULL ray, zmin <= 0 or non-finite, max_steps outside
 * [1, TDV_TSDF_RAYCAST_MAX_STEPS]; the host form above TDV_TSDF_HOST_MAX_VOXELS.  Tracking also: as tdv_depth_odometry_dev for scale and
 * odom, a NULL frame (width*height > 0), guess or result, a pose_direction other than TDV_POSE_SOURCE_ONTO_TARGET; the sequence: n_frames
 * < 0 or > TDV_TSDF_MAX_FRAMES, NULL frames or h_poses with n_frames > 0.
 * Not provided: a sparse volume, adaptive refinement of the hit beyond T16's one interpolation, loop closure, a device-resident pose
 * hand-off from tracking to integrate (the read-back per frame), a coloured sequence tracker (today a loop over tdv_tsdf_track_dev and
 * tdv_tsdf_integrate_color_dev), a colour term in tracking and odometry.  The ray-cast colour: tdv_tsdf_raycast_color_dev, below. */
#define TDV_TSDF_RAYCAST_MAX_STEPS 16384
typedef struct tdv_tsdf_raycast_params {   /* 8 bytes */
    float zmin;            /* T15: where the march starts, metres, > 0; default 0.05 */
    int   max_steps;       /* T15: the most samples of a ray, 1 .. TDV_TSDF_RAYCAST_MAX_STEPS; default 4096 */
} tdv_tsdf_raycast_params;
void tdv_tsdf_raycast_default_params(tdv_tsdf_raycast_params* params);
int tdv_tsdf_raycast_dev(tdv_ctx* ctx, const tdv_tsdf_volume* vol, const float* d_volume, int width, int height, float fx, float fy, float cx,
                         float cy, const float* h_pose /* host, 16 */, const tdv_tsdf_params* params, const tdv_tsdf_raycast_params* ray,
                         float* d_depth /* optional */, float* d_vertex_map /* optional */, float* d_normal_map /* optional */,
                         long long* h_n_hit /* optional, host */);
int tdv_tsdf_raycast(tdv_ctx* ctx, const tdv_tsdf_volume* vol, const float* volume, int width, int height, float fx, float fy, float cx, float cy,
                     const float* pose, const tdv_tsdf_params* params, const tdv_tsdf_raycast_params* ray, float* depth /* optional */,
                     float* vertex_map /* optional */, float* normal_map /* optional */, long long* n_hit /* optional */);
/* Coloured TSDF fusion (Open3D's ColoredTSDFVolume; KinectFusion's colour volume): the frames' colour images are fused beside their depths,
 * and the cloud, the mesh and the ray-cast view of the volume carry colours - float RGB in [0, 1], what tdv_color_gradients and
 * tdv_colored_icp take, so a model scanned here can be the target of this library's Colored ICP.  No existing call changes: the pair
 * volume's layout and every byte the calls above write stay as they are, and each call below is its plain counterpart plus the colour
 * arguments.  The rules continue T1 to T18, under the same arithmetic: f32, one rounding per operation, no contraction, the order as
 * written, / correctly rounded - every output is fixed bit for bit whatever order the device works in.
 *  T19. Colour volume: a second caller-owned device buffer of nx*ny*nz quads (f32 r, f32 g, f32 b, f32 wc), 16 bytes each, the buffer
 *      16-byte aligned, tdv_tsdf_color_bytes(vol) bytes (0 for a volume the checks refuse, as tdv_tsdf_volume_bytes); voxel (i, j, k) sits
 *      at quad index (k*ny + j)*nx + i, the pair volume's index.  The layout is public.  tdv_tsdf_color_reset_dev makes every quad
 *      (0, 0, 0, 0).  wc is the colour's own weight, not the pair's w: a volume may take some frames through tdv_tsdf_integrate_dev (no
 *      colour image) and others through tdv_tsdf_integrate_color_dev.
 *  T20. Pixel colour.  Frame f's colour image is width x height x 3 bytes, row-major, B, G, R at bytes 3*(v*width + u) + 0, 1, 2 - the
 *      layout tdv_depth_to_cloud_dev takes.  A channel is (float)byte / 255.0f, the cloud's rule.
 *  T21. Update.  A frame updates a voxel's quad exactly where T5 updates its pair, with the pixel at T3's (u, v): r' = (r*wc + c_r) /
 *      (wc + 1.0f), g' and b' likewise, wc' = fminf(wc + 1.0f, max_weight).  The frames apply in ascending index, and a call with frames
 *      A, B leaves what a call with A and then a call with B leave.  The pair volume and h_n_updated are byte for byte
 *      tdv_tsdf_integrate_dev's.  Every stored channel stays in [0, 1] (from a reset volume, or any whose channels are in [0, 1] and whose
 *      wc are not negative): rounding is monotone.  A pixel colour is the rounded quotient of 0 .. 255 by 255, so it lies in [0, 1]; with
 *      r and c_r in [0, 1] the product r*wc rounds into [0, wc], wc being a float; the sum is then at most wc + 1 before its rounding
 *      and at most the rounded wc + 1.0f - the divisor - after it (up to max_weight's range, 2^24, wc + 1.0f is exact besides); so the
 *      quotient is at most 1 before its rounding and after, and nothing is negative.
 *  T22. Coloured voxel: wc > 0.
 *  T23. Crossing colour.  With a, b, r_a, r_b of T7: both voxels coloured - per channel (c_a*r_b + c_b*r_a) / (r_a + r_b), the point's own
 *      interpolation with the voxels' channel values for the centres' coordinates; exactly one coloured - that voxel's colour; neither -
 *      (0, 0, 0).  Row i of the colour output belongs to row i of tdv_tsdf_extract_dev's cloud; since vertex v of the mesh is row v, it is
 *      the mesh's vertex colour too.
 *  T24. Ray-cast colour.  At a hit, p is T18's point (T13 at T16's z) and g_a, i_a, t_a are T14's for p.  If T14's conditions on the g_a
 *      hold and all eight voxels (i0 + dx, i1 + dy, i2 + dz) are coloured (T22), each channel is T14's seven lerps over the eight voxels'
 *      channel values.  Otherwise, and where the ray has no hit, the value is (0, 0, 0).  Nothing is clamped (a lerp may leave [0, 1] by
 *      a rounding).
 * tdv_tsdf_integrate_color_dev: tdv_tsdf_integrate_dev with d_color, the colour volume, and d_bgr, the n_frames colour images back to
 * back on the device.  tdv_tsdf_extract_color_dev and tdv_tsdf_extract_mesh_color_dev: their plain counterparts with d_color and
 * d_out_rgb (capacity resp. vertex_capacity rows of 3 floats, r, g, b); the same capacity and query protocol; d_out_xyz, d_out_normals and
 * the triangles get the bytes of the plain calls.  tdv_tsdf_raycast_color_dev: tdv_tsdf_raycast_dev with d_color and d_rgb_map (optional,
 * width*height*3 floats, the vertex map's layout); depth, vertex map, normal map and h_n_hit are byte for byte the plain call's.
 * tdv_tsdf_fuse_color, the host form: host frames and images in, vertices, normals (optional) and colours out, both volumes in the ctx's
 * workspace (24 bytes a voxel); volumes above TDV_TSDF_HOST_MAX_VOXELS are refused.  Triangles are optional: with a NULL n_triangles
 * (then out_triangles must be NULL and triangle_capacity 0) the call is the cloud's, tdv_tsdf_fuse's protocol; with n_triangles it is the
 * mesh's, tdv_tsdf_fuse_mesh's protocol, where a NULL out_triangles with capacity 0 is a query for both counts.
 * Kernels: the plain calls' own (csrc/tsdf.hip, csrc/tsdf_raycast.hip) with a compile-time colour switch.  Integrate keeps a voxel's quad
 * in registers beside its pair across the frames of a call - one 16-byte load when the first frame updates the voxel, one store after
 * the last, neither for a voxel no frame updates - and only updating lanes read their pixel's three bytes.  Extract stages no colour:
 * a lane that owns a crossing loads the two quads in the emit pass; the count pass is the plain one.  The ray cast loads the eight quads
 * once per ray, at a hit.
 * TDV_ERR_BAD_ARG before anything is enqueued or written: everything the plain counterpart refuses; a NULL d_color, or one that is not
 * 16-byte aligned; a NULL d_bgr (bgr) with n_frames > 0 and width*height > 0; a NULL d_out_rgb (out_rgb) with its capacity > 0;
 * tdv_tsdf_fuse_color with a NULL n_triangles and a non-NULL out_triangles or a triangle_capacity other than 0.
 * Not provided: compact (u8 or f16) colour storage - the f32 quad keeps the rules exact -, and what the two lists above name. */
unsigned long long tdv_tsdf_color_bytes(const tdv_tsdf_volume* vol);
int tdv_tsdf_color_reset_dev(tdv_ctx* ctx, const tdv_tsdf_volume* vol, float* d_color);
int tdv_tsdf_integrate_color_dev(tdv_ctx* ctx, const tdv_tsdf_volume* vol, float* d_volume, float* d_color, const uint16_t* d_raw /* n_frames images */,
                                 const uint8_t* d_bgr /* n_frames images */, int n_frames, int width, int height, float scale, float fx, float fy,
                                 float cx, float cy, const float* h_poses /* host, n_frames x 16 */, const tdv_tsdf_params* params,
                                 long long* h_n_updated /* optional, host, [n_frames] */);
int tdv_tsdf_extract_color_dev(tdv_ctx* ctx, const tdv_tsdf_volume* vol, const float* d_volume, const float* d_color, const tdv_tsdf_params* params,
                               float* d_out_xyz, float* d_out_normals /* optional */, float* d_out_rgb, int capacity, int* n_out /* host */);
int tdv_tsdf_extract_mesh_color_dev(tdv_ctx* ctx, const tdv_tsdf_volume* vol, const float* d_volume, const float* d_color,
                                    const tdv_tsdf_params* params, float* d_out_vertices, float* d_out_normals /* optional */, float* d_out_rgb,
                                    int vertex_capacity, int* n_vertices /* host */, int* d_out_triangles, int triangle_capacity,
                                    int* n_triangles /* host */);
int tdv_tsdf_raycast_color_dev(tdv_ctx* ctx, const tdv_tsdf_volume* vol, const float* d_volume, const float* d_color, int width, int height, float fx,
                               float fy, float cx, float cy, const float* h_pose /* host, 16 */, const tdv_tsdf_params* params,
                               const tdv_tsdf_raycast_params* ray, float* d_depth /* optional */, float* d_vertex_map /* optional */,
                               float* d_normal_map /* optional */, float* d_rgb_map /* optional */, long long* h_n_hit /* optional, host */);
int tdv_tsdf_fuse_color(tdv_ctx* ctx, const tdv_tsdf_volume* vol, const uint16_t* raw, const uint8_t* bgr, int n_frames, int width, int height,
                        float scale, float fx, float fy, float cx, float cy, const float* poses, const tdv_tsdf_params* params, float* out_vertices,
                        float* out_normals /* optional */, float* out_rgb, int vertex_capacity, int* n_vertices, int* out_triangles /* optional */,
                        int triangle_capacity, int* n_triangles /* optional: NULL = the cloud only */);
/* Depth odometry (KinectFusion's tracking step, Newcombe et al. 2011; Open3D's compute_odometry_result_point_to_plane): the camera's
 * motion between two raw depth frames of one sensor, on the device - the piece between "scan" and "fuse".  Two frames need no search
 * structure: the pixel grid gives a vertex its neighbours, so a normal is one cross product, and the projection gives a source pixel its
 * partner, so an iteration is one gather per pixel.  The terms, the solver and the update are point-to-plane ICP's own (tdv_icp).
 * All arithmetic is f32, one rounding per operation, no contraction, the order exactly as written (sqrtf and / correctly rounded); the
 * exceptions are the f64 sums of O7 and the pose chain of O9.  Every output is fixed bit for bit whatever order the device works in.
 *  O1. Level 0 depth: z = float(raw) * float(1.0 / scale), rule 5 of tdv_verify_poses.  Valid iff raw != 0 && z <= zmax.  An invalid
 *      pixel holds 0.0f (a valid one is > 0).
 *  O2. Vertex of a valid pixel (u, v) at depth z: tdv_deproject's rule, x = (((float)u - cx) * z) / fx, y = (((float)v - cy) * z) / fy, z.
 *  O3. Normal at (u, v).  Present iff u + 1 < w and v + 1 < h, the depths at (u, v), (u+1, v) and (u, v+1) are valid, and
 *      fabsf(z(u+1, v) - z(u, v)) <= depth_diff and fabsf(z(u, v+1) - z(u, v)) <= depth_diff.  With a = V(u+1, v) - V(u, v) and
 *      b = V(u, v+1) - V(u, v) per component, n = b x a = (b1*a2 - b2*a1, b2*a0 - b0*a2, b0*a1 - b1*a0),
 *      L = sqrtf((n0*n0 + n1*n1) + n2*n2), and the row is n / L per component.  Absent where L is zero or not finite; an absent normal
 *      is (0, 0, 0).  A front-on plane gives (0, 0, -1): towards the camera, the side T8's normals point to.
 *  O4. Pyramid.  Level l+1 has (w/2) x (h/2) pixels (integer division).  Pixel (u, v) of it takes the pixels (2u, 2v), (2u+1, 2v),
 *      (2u, 2v+1), (2u+1, 2v+1) of level l in that order: z0 is the first valid one, the members are the valid ones with
 *      fabsf(z - z0) <= depth_diff, and z' is their f32 sum in that order divided by (float)count, or 0.0f if none is valid.
 *      Intrinsics: fx' = fx*0.5f, fy' = fy*0.5f, cx' = (cx - 0.5f)*0.5f, cy' = (cy - 0.5f)*0.5f (a pixel's centre is its integer
 *      coordinate, as u = floorf(uf + 0.5f) says).  O2 and O3 hold on every level with the level's depth and intrinsics.
 *  O5. Association.  The pose T (column-major) takes source-camera coordinates to target-camera coordinates: Open3D's source-to-target
 *      convention.  A source pixel with a valid vertex p has a partner iff: q = T p by rule 1 of tdv_verify_poses in its
 *      TDV_POSE_MODEL_TO_CAMERA form; q is usable by rules 2 and 3 (zmax is params->zmax, the intrinsics the level's); its pixel
 *      (u, v) lies inside the target frame; the target has a normal nt there (O3), with vertex pt (O2); fabsf(pt_z - q_z) <= depth_diff.
 *  O6. Terms: exactly point-to-plane ICP's record with the transformed point q, the target point pt and the normal nt:
 *      J = (q x nt, nt) = (qy*n2 - qz*n1, qz*n0 - qx*n2, qx*n1 - qy*n0, n0, n1, n2); e = q - pt per component; r = ex*n0 + (ey*n1 + ez*n2);
 *      d2 = ex*ex + (ey*ey + ez*ez), as tdv_icp_correspondences' squared distance.  The 29 terms are
 *      {1, d2, 21 x (double)(J[a]*J[b]) for a <= b in row order, 6 x (double)(J[a]*r)}, each product formed in f32 and widened.
 *  O7. Sums.  Each of the 29 sums goes over the fixed f64 tree (tdv_remove_statistical_outlier, rule 4) in source-pixel index
 *      i = v*w + u of the level, 256 per workgroup; a pixel without a partner contributes +0.0 to each.
 *  O8. Iteration and level.  One iteration is point-to-plane ICP's on those sums: n_corr = the first sum; n_corr < 3 ends the level
 *      and keeps the pose; else the 6 x 6 system (the 21 sums rounded to f32, symmetric) is solved for x against minus the 6 sums
 *      rounded to f32 by the pivoted LDL^T, delta = (Rx(x0) Ry(x1) Rz(x2), x3..5), T' = delta * T (k ascending);
 *      rmse = sqrtf((float)sum_d2 / (float)n_corr); fitness = (float)n_corr / (float)(the level's count of valid source pixels).  The
 *      level ends after an iteration with iter > 0 && fabsf(prev_rmse - rmse) < 1e-6f, or after max_iterations[l].  Levels run from
 *      the coarsest, n_levels - 1, to 0; each restarts the iteration state, T is carried.  max_iterations[l] == 0 skips the level.
 *  O9. Sequence.  Frames 0 .. n-1; pair k has source k, target k-1 and start h_init[k] (or the identity).  P_0 = I and
 *      P_k = P_(k-1) * T_k, formed on the host: each entry the f64 sum of four f64 products in index order, rounded once to f32.  P_k is
 *      camera k's pose in camera 0's frame: TDV_POSE_SOURCE_ONTO_TARGET for tdv_tsdf_integrate_dev with the volume in camera 0's frame.
 *  O10. An f32 target.  Where the target is an f32 depth image d instead of a raw frame, its level 0 depth is z = d if d is not NaN and
 *      0 < d <= zmax, else 0.0f.  O3 to O8 are unchanged; the source stays a raw frame (O1).
 * tdv_depth_maps_dev: O1 to O3 of one frame at level 0.  Every output is optional.  d_vertex_map and d_normal_map are width*height*3
 * floats, zeros at invalid pixels resp. absent normals.  d_out_xyz and d_out_normals receive, in pixel order, the rows of the pixels
 * that have a normal - a cloud with normals and no neighbour search; they need n_out, which bounds them.  Count and capacity as
 * tdv_tsdf_extract_dev: capacity = the room in rows, NULL rows with capacity 0 are a query, and a capacity that is too small returns
 * TDV_ERR_BAD_ARG with *n_out set to the needed count and nothing written, the maps included.  One read-back, and only when n_out is
 * asked for.  tdv_depth_maps is its host form.  Of params it uses depth_diff and zmax (the others are checked all the same).
 * tdv_depth_odometry_terms_dev: the 29 sums of O7 for the pose h_T at one level and that level's count of valid source pixels
 * (optional), exposed for parity tests as tdv_icp_correspondences is.
 * tdv_depth_odometry_dev: O8 from h_T0 (NULL: the identity).  The frames are device pointers, the pose and the result on the host; one
 * read-back.  The result holds T, then fitness, rmse and n_corr of the last level that applied an iteration (zeros if none did), and
 * per level the iterations applied and the correspondences of its last applied iteration.  tdv_depth_odometry is its host form.
 * tdv_depth_odometry_to_depth_dev: tdv_depth_odometry_dev with the target given as an f32 depth image d_depth_tgt (width*height floats,
 * metres along the camera's z, device) by O10 - what tdv_tsdf_raycast_dev writes, which is frame-to-model tracking, and also what
 * tdv_render_depth_dev writes, which tracks a part against its own rendering.  Where the image holds exactly O1's depth of a raw frame
 * the result is byte for byte tdv_depth_odometry_dev's with that frame as the target.  tdv_depth_odometry_to_depth is its host form.
 * tdv_depth_odometry_sequence_dev: d_raw holds n_frames images back to back; h_init (optional, n_frames x 16, entry 0 unused), h_poses
 * (n_frames x 16) and h_pairs (optional, n_frames results, entry 0 zeros) on the host.  Per pair the result is, byte for byte, what
 * tdv_depth_odometry_dev returns for that pair on the same ctx.  Each frame's pyramid is built once, all pairs iterate together - the
 * launches of an iteration cover every pair still running - and the states come down once.
 * Kernels (csrc/odometry.hip): one launch per iteration; per workgroup of 256 pixels one row of partial sums; the workgroup that takes
 * the pair's last ticket folds the rows in O7's order and applies the update, so the next launch reads the new pose with no host round
 * trip.  No float atomics.  The workspace keeps 16 bytes per pixel and level (depth and normal; vertices are recomputed, O2 gives the
 * same bits): about 21 bytes per pixel of a frame at three levels.
 * TDV_ERR_BAD_ARG before anything is enqueued or written: a NULL ctx, params, frames (width*height > 0), pose (terms), sums or result;
 * rows without n_out, or capacity > 0 with both row pointers NULL; width or height < 0 or > TDV_VERIFY_MAX_SIDE; scale, fx or fy <= 0 or
 * non-finite; depth_diff or zmax <= 0 or non-finite; n_levels outside [1, TDV_ODOM_MAX_LEVELS] or so many that a level would have a side
 * of 0; a negative max_iterations; level outside [0, n_levels); n_frames < 0 or > TDV_TSDF_MAX_FRAMES; capacity < 0.  Valid, and
 * returning the start pose with zeros: width*height == 0, n_frames of 0 or 1, a frame with no valid pixel.  NaN or infinite entries of a
 * start pose fall out through O5: no partner, so the n_corr < 3 rule applies.  The ctx's ICP switches (search, loss, accumulation,
 * launches) do not apply.
 * Not provided: colour (hybrid) odometry, the information matrix, masks (a caller zeroes the pixels), the C++ operator mirror.
 * Frame-to-model tracking against the volume: tdv_tsdf_track_dev (K1 to K3, with tdv_tsdf_raycast_dev above). */
#define TDV_ODOM_MAX_LEVELS 4
typedef struct tdv_odometry_params {   /* 28 bytes */
    float depth_diff;                          /* O3, O4, O5: metres, > 0; default 0.03 (Open3D's) */
    float zmax;                                /* as tdv_deproject; default 10 */
    int   n_levels;                            /* 1 .. TDV_ODOM_MAX_LEVELS; default 3 */
    int   max_iterations[TDV_ODOM_MAX_LEVELS]; /* per level, level 0 the finest; default {20, 10, 5, 0} */
} tdv_odometry_params;
typedef struct tdv_odometry_result {   /* 108 bytes */
    float T[16];                               /* column-major, source camera to target camera */
    float fitness, rmse;                       /* of the last level that applied an iteration */
    int   n_corr;
    int   iterations[TDV_ODOM_MAX_LEVELS];     /* iterations applied per level */
    int   n_corr_level[TDV_ODOM_MAX_LEVELS];   /* partners of the level's last applied iteration */
} tdv_odometry_result;
void tdv_odometry_default_params(tdv_odometry_params* params);
int tdv_depth_maps_dev(tdv_ctx* ctx, const uint16_t* d_raw, int width, int height, float scale, float fx, float fy, float cx, float cy,
                       const tdv_odometry_params* params, float* d_vertex_map /* optional */, float* d_normal_map /* optional */,
                       float* d_out_xyz /* optional */, float* d_out_normals /* optional */, int capacity, int* n_out /* optional, host */);
int tdv_depth_maps(tdv_ctx* ctx, const uint16_t* raw, int width, int height, float scale, float fx, float fy, float cx, float cy,
                   const tdv_odometry_params* params, float* vertex_map, float* normal_map, float* out_xyz, float* out_normals, int capacity,
                   int* n_out);
int tdv_depth_odometry_terms_dev(tdv_ctx* ctx, const uint16_t* d_raw_src, const uint16_t* d_raw_tgt, int width, int height, float scale,
                                 float fx, float fy, float cx, float cy, const float* h_T /* host, 16 */, int level,
                                 const tdv_odometry_params* params, double* h_sums /* host, [29] */, int* n_valid_src /* optional, host */);
int tdv_depth_odometry_dev(tdv_ctx* ctx, const uint16_t* d_raw_src, const uint16_t* d_raw_tgt, int width, int height, float scale, float fx,
                           float fy, float cx, float cy, const float* h_T0 /* optional, host, 16 */, const tdv_odometry_params* params,
                           tdv_odometry_result* out /* host */);
int tdv_depth_odometry(tdv_ctx* ctx, const uint16_t* raw_src, const uint16_t* raw_tgt, int width, int height, float scale, float fx, float fy,
                       float cx, float cy, const float* T0 /* optional */, const tdv_odometry_params* params, tdv_odometry_result* out);
int tdv_depth_odometry_sequence_dev(tdv_ctx* ctx, const uint16_t* d_raw /* n_frames images */, int n_frames, int width, int height, float scale,
                                    float fx, float fy, float cx, float cy, const float* h_init /* optional, host, n_frames x 16 */,
                                    const tdv_odometry_params* params, float* h_poses /* host, n_frames x 16 */,
                                    tdv_odometry_result* h_pairs /* optional, host, [n_frames] */);
int tdv_depth_odometry_to_depth_dev(tdv_ctx* ctx, const uint16_t* d_raw_src, const float* d_depth_tgt /* O10 */, int width, int height,
                                    float scale, float fx, float fy, float cx, float cy, const float* h_T0 /* optional, host, 16 */,
                                    const tdv_odometry_params* params, tdv_odometry_result* out /* host */);
int tdv_depth_odometry_to_depth(tdv_ctx* ctx, const uint16_t* raw_src, const float* depth_tgt, int width, int height, float scale, float fx,
                                float fy, float cx, float cy, const float* T0 /* optional */, const tdv_odometry_params* params,
                                tdv_odometry_result* out);
/* Frame-to-model tracking, K1 to K3: stated with tdv_tsdf_raycast_dev above. */
typedef struct tdv_tsdf_track_result {   /* 184 bytes */
    float pose[16];                            /* K3: the camera's pose in the volume's frame, column-major */
    tdv_odometry_result odom;                  /* K2: the frame against the ray cast; T takes the frame's camera to the guess's */
    long long n_hit;                           /* K1: the rays of the guess's view that hit */
} tdv_tsdf_track_result;
int tdv_tsdf_track_dev(tdv_ctx* ctx, const tdv_tsdf_volume* vol, const float* d_volume, const uint16_t* d_raw, int width, int height,
                       float scale, float fx, float fy, float cx, float cy, const float* h_guess /* host, 16 */,
                       const tdv_tsdf_params* params, const tdv_tsdf_raycast_params* ray, const tdv_odometry_params* odom,
                       tdv_tsdf_track_result* out /* host */);
int tdv_tsdf_track_sequence_dev(tdv_ctx* ctx, const tdv_tsdf_volume* vol, float* d_volume, const uint16_t* d_raw /* n_frames images */,
                                int n_frames, int width, int height, float scale, float fx, float fy, float cx, float cy,
                                const float* h_pose0 /* optional, host, 16 */, const tdv_tsdf_params* params,
                                const tdv_tsdf_raycast_params* ray, const tdv_odometry_params* odom, float* h_poses /* host, n_frames x 16 */,
                                tdv_tsdf_track_result* h_results /* optional, host, [n_frames] */);
/* PPF matching (point-pair-feature voting: Drost, Ulrich, Navab, Ilic, CVPR 2010; OpenCV's ppf_match_3d, PCL's PPFRegistration): a third
 * global registration beside tdv_ransac and tdv_fgr, from points and normals only - no descriptors.  Conventions as there: source = scene,
 * target = model, T moves the source onto the target.  It returns up to max_poses ranked candidate poses.  The votes are integers and
 * every float that decides an integer is fixed by the rules below, so peaks, votes and clusters do not depend on the order the device works
 * in.  "f32" means IEEE single precision, one rounding per operation, no contraction, the expression evaluated as written; atan2f is
 * glibc's (csrc/libm_f32.hpp, held to the running libm by tests/test_libm_restatement.py).  PI = 3.14159274f, TWO_PI = 6.28318548f.
 * dot(u, v) = (u.x * v.x + u.y * v.y) + u.z * v.z.  cross(u, v) = (u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x).
 * norm(u) = sqrtf(dot(u, u)).  ang(u, v) = atan2f(norm(cross(u, v)), dot(u, v)), in [0, PI].
 *  0. Usable point: a point (p, n) of either cloud is usable iff its six floats are finite and nn = dot(n, n) is > 0 and finite (a normal
 *     whose squared length underflows to 0 counts as zero, one whose squared length overflows as non-finite).  An unusable point takes no
 *     part in any pair, as first or as second point, and has no other effect.  With flip_model_normals every model normal is replaced by
 *     -n (exact) before anything else: for a model whose normals came from tdv_estimate_normals with the origin inside the part - that call
 *     turns normals towards the origin, so they point inward, while a scene's point at the camera.
 *  1. Diameter: over the model points whose three coordinates are finite (the normal does not matter), e_a = max_a - min_a per axis in f32,
 *     diameter = sqrtf((e_x * e_x + e_y * e_y) + e_z * e_z); 0 without such a point.  distance_step = distance_step_relative * diameter.
 *     n_dist = (int)floorf(1.0f / distance_step_relative) + 1, n_keys = n_dist * A * A * A with A = angle_bins.
 *  2. Pair feature of the ordered pair (a, b), a != b, both usable: d = p_b - p_a per component, len = norm(d), f1 = ang(n_a, d),
 *     f2 = ang(n_b, d), f3 = ang(n_a, n_b) (the normals as they are, not normalised).  q0f = floorf(len / distance_step),
 *     q_k = min((int)floorf(f_k / (PI / (float)A)), A - 1) for k = 1..3, key = ((q0 * A + q1) * A + q2) * A + q3 with q0 = (int)q0f.
 *     The pair has no key unless len > 0, len is finite, q0f < (float)n_dist (false for the NaN and infinity of a zero step), none of f1,
 *     f2, f3 is NaN, and the alpha of rule 3 is not NaN.
 *  3. Alpha of the pair: the frame of a is the rotation that moves n_a onto +x.  norm_a = sqrtf(nn), u = n_a / norm_a per component;
 *     neg = n_a.x < 0; w = neg ? -u : u (so w.x >= 0: the case n_a ~ -x, where the shortest rotation onto +x is ill-conditioned, is turned
 *     into the case w ~ +x followed by the half turn diag(-1, 1, -1) about y); k = 1.0f + w.x, ca = w.y / k, cb = w.z / k.  The shortest
 *     rotation of w onto +x has the rows (w.x, w.y, w.z), (-w.y, 1 - w.y * ca, -w.y * cb), (-w.z, -w.z * ca, 1 - w.z * cb); with neg, rows 0
 *     and 2 change sign.  Applied to d in f32: t = w.y * d.y + w.z * d.z, y = (d.y - ca * t) - w.y * d.x, z = (d.z - cb * t) - w.z * d.x,
 *     z = -z with neg; alpha = atan2f(-z, y).
 *  4. Model table: every ordered pair (i, j) of the model that has a key, sorted by (key, i * nt + j) (the stable radix sort of
 *     tdv_radix_sort_pairs_dev on the keys of the pairs in ascending i * nt + j: a total order), with its alpha as f32 bits.  Layout of
 *     d_model, 32-bit words: offsets[n_keys + 1] (int: the entries of key k are [offsets[k], offsets[k + 1]); offsets[n_keys] = n_pairs),
 *     padding to a multiple of 4 words, then two arrays of cap = nt * (nt - 1) words each: pair (i * nt + j) and alpha (f32 bits); an
 *     entry's key is the k whose range holds it.
 *     Entries beyond n_pairs are not written.  tdv_ppf_model_bytes gives the size; info carries diameter, distance_step, n_pairs, n_keys
 *     and nt.  With a relative step the key space depends on the parameters only.  TDV_PPF_MODEL_MAX is 2048, not 4096: the table of a
 *     4096-point model is 192 MiB and its sort needs 600 MiB of scratch, four times what 2048 takes, and a model for voting is sampled at
 *     about the distance step anyway (OpenCV, PCL and Drost et al. all do): 2048 points at step 0.05 is already denser than that.
 *  5. Voting: scene point r is a reference point iff r % ref_stride == 0; n_ref = ceil(ns / ref_stride), reference point q is scene point
 *     q * ref_stride.  A usable reference point s_r owns nt * rotation_bins 32-bit counters, all 0 at first.  For every usable scene point
 *     s_i, i != r (by index), whose pair (s_r, s_i) has a key (rule 2 with the MODEL's distance_step and n_dist): for every table entry
 *     (i_m * nt + j_m, alpha_m) of that key, counter [i_m][bin(alpha_m - alpha_s)] += 1.  x = alpha_m - alpha_s in f32; x = x + TWO_PI if
 *     x < -PI, else x = x - TWO_PI if x >= PI; bin = min(max((int)floorf((x + PI) / (TWO_PI / (float)rotation_bins)), 0), rotation_bins - 1).
 *     One workgroup per reference point (in turn, where there are more reference points than workgroups); the counters sit in LDS when
 *     nt * rotation_bins <= TDV_PPF_LDS_CELLS (39,000: 152.3 of the 160 KiB; the tile's staging takes the rest), else in a slab of the workspace per workgroup; the same
 *     integers either way.  The slabs of a call take at most 128 MiB of the workspace (fewer workgroups where a slab is large; at least one).
 *     A workgroup takes the scene points in tiles; each lane forms one pair's key and bucket, then the lanes share the
 *     tile's table entries evenly, whatever bucket they come from.
 *  6. Peak of reference point q: the counter with the most votes, ties to the lowest i_m, then the lowest bin (one maximum over
 *     (votes << 32) | (0xFFFFFFFF - (i_m * rotation_bins + bin))).  tdv_ppf_peak = (ref = q * ref_stride, model_index, bin, votes);
 *     votes = 0 (with model_index = bin = 0): none - an unusable reference point, or no vote.
 *  7. Poses, clusters, score: on the host in f64 (IEEE double, the expression as written), from the f32 inputs converted exactly.
 *     Frame of a point (p, n), as rule 3 in f64: norm = sqrt((n.x * n.x + n.y * n.y) + n.z * n.z), u = n / norm, neg = n.x < 0, w, k, ca, cb
 *     and the rows as there: R.  Pose of a peak (scene point s, model point m): alpha_c = (float)(-pi + (bin + 0.5) * ((2 pi) /
 *     rotation_bins)), the bin's centre rounded once to f32 (pi = 3.141592653589793); c = cos(alpha_c), sn = sin(alpha_c); M = Rx(-alpha_c)
 *     R_s: M[0] = R_s[0], M[1] = c * R_s[1] + sn * R_s[2], M[2] = c * R_s[2] - sn * R_s[1]; Rot[i][j] = (R_m[0][i] * M[0][j] + R_m[1][i] *
 *     M[1][j]) + R_m[2][i] * M[2][j]; t[i] = p_m[i] - ((Rot[i][0] * p_s[0] + Rot[i][1] * p_s[1]) + Rot[i][2] * p_s[2]): T = T_m^-1 Rx(-alpha)
 *     T_s.  Clustering: the peaks with votes > 0 by votes descending, then ref ascending; each joins the first cluster (in founding order)
 *     whose founder's pose is within both thresholds, else founds one: sqrt((dx * dx + dy * dy) + dz * dz) <= cluster_translation_relative *
 *     diameter for the difference of the two t, and ((sum over i, then j, of RotA[i][j] * RotB[i][j], added in that order from 0.0) - 1) / 2
 *     >= cos(cluster_rotation) (the angle between the rotations is at most cluster_rotation).  A cluster's votes are the sum of its
 *     members' votes, its pose (T, ref, model_index, bin) is its founder's, rounded once to f32 and stored column-major.  Returned: the
 *     max_poses clusters with the most votes, the earlier-founded first among equals.  Score of a returned pose: tdv_icp_correspondences
 *     at (T, thr): n_corr is its count, fitness = (float)n_corr / (float)ns, rmse = (float)sqrt(S / n_corr) with S the sum of (double)d2[i]
 *     over the accepted i in ascending order (0 when n_corr = 0): the numbers compare with every ICP result.  The ctx's ICP search switch
 *     applies to that pass as it does to tdv_icp_correspondences, and tdv_ctx_last_icp_search afterwards reports that pass.
 * tdv_ppf_model_dev builds the table once into a caller-owned device buffer (the pattern of tdv_prepare_model_dev: no handle, nothing
 * kept in the ctx); tdv_ppf_match_dev votes against it (device pointers; out_poses, n_poses and n_ref are host memory; d_peaks, optional,
 * receives n_ref peaks); tdv_ppf_match takes host arrays, builds the table itself in the workspace and returns the peaks (optional) in
 * host memory.  Both read back twice: the peaks, then each returned pose's score.
 * TDV_ERR_BAD_ARG before anything is enqueued or written: a NULL ctx, params, out_poses or n_poses (match), info (model_dev, match_dev),
 * bytes (model_bytes) or d_model; ns < 0; nt < 0; nt > TDV_PPF_MODEL_MAX; a NULL cloud or normal array with a count > 0; thr NaN, infinite or
 * not > 0; distance_step_relative NaN, not > 0 or > 1; angle_bins outside [1, 64]; rotation_bins outside [1, 256]; n_keys >
 * TDV_PPF_KEYS_MAX (2^24); ref_stride < 1; max_poses outside [1, TDV_PPF_POSES_MAX]; cluster_translation_relative NaN, infinite or < 0;
 * cluster_rotation NaN, < 0 or > PI; flip_model_normals neither 0 nor 1; d_model not 4-byte aligned; model_bytes below
 * tdv_ppf_model_bytes; an info that does not fit the call (info->nt != nt, n_keys other than the parameters give, n_pairs outside
 * [0, nt * (nt - 1)], a diameter or distance_step that is NaN, infinite or < 0).  Accepted and empty (status OK, *n_poses = 0, *n_ref = 0,
 * no peak written): ns == 0, nt < 2, or a table without pairs.  The call obeys the ctx's state rule (README, "What a context keeps
 * between calls").
 * tdv_ppf_match_batch_dev is, per instance, tdv_ppf_match_dev: instance b is rows [h_src_offsets[b], h_src_offsets[b + 1]) of d_src and
 * d_src_normals (the layout of tdv_icp_batch_dev and of tdv_cluster_dbscan_dev's output), and its poses (out_poses + b * max_poses, every
 * field), n_poses[b] and peaks are byte for byte what tdv_ppf_match_dev returns for that cloud alone on the same ctx; a peak's ref counts
 * inside its instance.  Instance b's peaks start at h_peak_offsets[b] = the sum over a < b of ceil(ns_a / ref_stride) (h_peak_offsets, optional,
 * host, [n_instances + 1]; d_peaks, optional, device, [h_peak_offsets[n_instances]]).  An instance without points has n_poses[b] = 0 and no
 * peak.  All instances' reference points vote in one launch (a workgroup takes work items = (instance, reference point) in instance order and
 * finds an item's instance by binary search in the reference offsets, uploaded with the call) and all returned poses are scored in one
 * launch: the model in LDS, one lane per source point, the brute scan of tdv_icp_correspondences.  Every search gives the same accepted
 * rows and the scores use only those, so the ctx's ICP search switch does not enter the result; after a call that scored at least one
 * pose tdv_ctx_last_icp_search reports TDV_ICP_SEARCH_BRUTE.  The call reads back twice in all: the peaks, then d2 and the accepted flag of
 * every (returned pose, source point), summed on the host as rule 7 says: 5 bytes x the sum over b of n_poses[b] * ns_b of workspace and of
 * pinned staging (8 poses of 256 instances of 1,446 points: 14.8 MB), neither capped nor chunked.
 * TDV_ERR_BAD_ARG before anything is enqueued or written: the list of tdv_ppf_match_dev (ns being h_src_offsets[n_instances]), and
 * n_instances < 0; NULL h_src_offsets with n_instances > 0; offsets that do not start at 0 or that decrease; a sum of reference points or
 * n_instances * max_poses beyond INT_MAX.  Accepted and empty (status OK, every n_poses[b] = 0, every h_peak_offsets entry 0, no peak
 * written): n_instances == 0, no instance with a point, nt < 2, or a table without pairs.  The call obeys the ctx's state rule.
 * Not provided: PPF inside tdv_register_batch_dev (an ABI change), a host-array form of the batch, several models in one call, the C++
 * operator mirror, averaging the poses of a cluster, an absolute distance step, voting into neighbouring bins. */
#define TDV_PPF_MODEL_MAX 2048
#define TDV_PPF_POSES_MAX 64
#define TDV_PPF_KEYS_MAX (1 << 24)
#define TDV_PPF_LDS_CELLS 39000
typedef struct tdv_ppf_params {
    float distance_step_relative;        /* 0.05: the distance step as a share of the model's diameter */
    int   angle_bins;                    /* 30: bins of the three feature angles over [0, pi] */
    int   rotation_bins;                 /* 30: bins of alpha over [-pi, pi) */
    int   ref_stride;                    /* 5 */
    int   max_poses;                     /* 8 */
    float cluster_translation_relative;  /* 0.1: of the diameter */
    float cluster_rotation;              /* 2 pi / 30, radians */
    int   flip_model_normals;            /* 0 */
} tdv_ppf_params;
typedef struct tdv_ppf_model_info {
    float diameter;
    float distance_step;
    int   n_pairs;
    int   n_keys;
    int   nt;
} tdv_ppf_model_info;
typedef struct tdv_ppf_pose {
    float T[16];            /* column-major */
    float fitness, rmse;
    int   n_corr;
    int   votes;            /* of the cluster */
    int   members;
    int   ref, model_index, bin;   /* the founder's peak */
} tdv_ppf_pose;
typedef struct tdv_ppf_peak {
    int ref, model_index, bin, votes;
} tdv_ppf_peak;
void tdv_ppf_default_params(tdv_ppf_params* p);
int tdv_ppf_model_bytes(int nt, const tdv_ppf_params* params, size_t* bytes);
int tdv_ppf_model_dev(tdv_ctx* ctx, const float* d_tgt, const float* d_tgt_normals, int nt, const tdv_ppf_params* params, void* d_model,
                      size_t model_bytes, tdv_ppf_model_info* info);
int tdv_ppf_match_dev(tdv_ctx* ctx, const float* d_src, const float* d_src_normals, int ns, const float* d_tgt, const float* d_tgt_normals,
                      int nt, const void* d_model, const tdv_ppf_model_info* info, float thr, const tdv_ppf_params* params,
                      tdv_ppf_pose* out_poses /* host, [max_poses] */, int* n_poses, tdv_ppf_peak* d_peaks /* optional, device */,
                      int* n_ref /* host, optional */);
int tdv_ppf_match_batch_dev(tdv_ctx* ctx, const float* d_src, const float* d_src_normals,
                            const int* h_src_offsets /* host, [n_instances + 1], starting at 0, non-decreasing */, int n_instances,
                            const float* d_tgt, const float* d_tgt_normals, int nt, const void* d_model, const tdv_ppf_model_info* info,
                            float thr, const tdv_ppf_params* params,
                            tdv_ppf_pose* out_poses /* host, [n_instances * max_poses]: instance b's poses at b * max_poses */,
                            int* n_poses /* host, [n_instances] */,
                            tdv_ppf_peak* d_peaks /* optional, device, [sum of the instances' n_ref] */,
                            int* h_peak_offsets /* optional, host, [n_instances + 1] */);
int tdv_ppf_match(tdv_ctx* ctx, const float* src, const float* src_normals, int ns, const float* tgt, const float* tgt_normals, int nt,
                  float thr, const tdv_ppf_params* params, tdv_ppf_pose* out_poses /* [max_poses] */, int* n_poses,
                  tdv_ppf_peak* peaks /* optional, host, [ceil(ns / ref_stride)] */, int* n_ref /* optional */);
int tdv_ransac_dev(tdv_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt,
                   const float* d_fs, const float* d_ft, const int* d_corr,
                   float voxel_size, int max_iterations, float confidence, uint32_t seed,
                   tdv_ransac_result* out, int* trace_inliers /* host, optional */);
int tdv_feature_match_dev(tdv_ctx* ctx, const float* d_fs, int ns, const float* d_ft, int nt, int* d_corr);
int tdv_estimate_normals_dev(tdv_ctx* ctx, const float* d_xyz, int n, int k, float* d_normals, int* d_knn);
int tdv_compute_fpfh_dev(tdv_ctx* ctx, const float* d_xyz, const float* d_normals, int n, float radius,
                         float* d_desc33, int* d_nbr, int* d_nbr_cnt);
/* estimateNormals(k) followed by computeFPFH(radius) on the same cloud (src/pipeline.cpp:93-95) with ONE neighbour walk: the radius
 * lists are sorted by (d2, idx) and capped at the 100 smallest, so wherever a point has >= k neighbours in radius its k nearest
 * neighbours ARE the head of its radius list (registration.cpp:68-74,95-99); only the deficient points (isolated points, silhouette
 * edges) go through a kNN search of their own, as a subset.  Normals and descriptors are those of the two separate calls bit for bit
 * (tests/test_gpu_features.py); what tdv_register_batch_dev and tdv_prepare_model_dev run.  k <= 100 shares the walk; larger k falls
 * back to the two calls. */
int tdv_normals_fpfh_dev(tdv_ctx* ctx, const float* d_xyz, int n, int k, float radius, float* d_normals, float* d_desc33);
/* The stable radix sort the descriptor index build uses (csrc/sort.hip, hand-written: a utility without a counterpart in the reference,
 * exported so that it is tested on its own): n (64-bit key, 32-bit value) pairs in device memory ordered by the low end_bit bits of the
 * key, pairs of equal keys in input order.  The in and out buffers must not overlap. */
int tdv_radix_sort_pairs_dev(tdv_ctx* ctx, const unsigned long long* d_keys_in, unsigned long long* d_keys_out, const unsigned* d_vals_in,
                             unsigned* d_vals_out, size_t n, int end_bit);
int tdv_depth_to_cloud_dev(tdv_ctx* ctx, const uint16_t* d_raw, const uint8_t* d_mask, const uint8_t* d_bgr,
                           int width, int height, float scale, int mask_mode,
                           float fx, float fy, float cx, float cy, float zmax,
                           float* d_xyz, float* d_rgb, int capacity, int* n_out /* host */);
/* order: TDV_VOXEL_ORDER_FIRST or TDV_VOXEL_ORDER_REFERENCE; for the latter the host receives 16 B per voxel (cell and
 * input index of its first point) to replay the reference's container — the cloud itself stays on the device. */
int tdv_voxel_downsample_dev(tdv_ctx* ctx, const float* d_xyz, const float* d_rgb, int n, float voxel_size, int order,
                             float* d_out_xyz, float* d_out_rgb, int capacity, int* n_out /* host */);
/* tdv_voxel_downsample_normals on device arrays: xyz, rgb and the voxel set as tdv_voxel_downsample_dev's, the voxels' unit mean normals
 * beside them (d_normals == NULL or d_out_normals == NULL: no normals). */
int tdv_voxel_downsample_normals_dev(tdv_ctx* ctx, const float* d_xyz, const float* d_normals, const float* d_rgb /* optional */, int n,
                                     float voxel_size, int order, float* d_out_xyz, float* d_out_normals, float* d_out_rgb, int capacity,
                                     int* n_out /* host */);

/* Registration::voxelDownsample (src/registration.cpp:29-60) for n_clouds clouds stored back to back at d_xyz (cloud b =
 * points [h_cloud_offsets[b], h_cloud_offsets[b+1]); host array of n_clouds + 1 entries starting at 0), in ONE set of launches:
 * cloud b's voxels, in first-occurrence order (TDV_VOXEL_ORDER_FIRST), come back at [h_voxel_offsets[b], h_voxel_offsets[b+1])
 * of d_out_xyz, which has room for as many points as d_xyz holds.  Means are the reference's (f32 sums in ascending input
 * index).  What tdv_register_batch_dev runs for its instances. */
int tdv_voxel_downsample_batch_dev(tdv_ctx* ctx, const float* d_xyz, const int* h_cloud_offsets, int n_clouds, float voxel_size,
                                   float* d_out_xyz, int* h_voxel_offsets);
/* The same for clouds that were unprojected from depth images with the given pinhole intrinsics and are still in the row-major pixel
 * order tdv_depth_to_cloud*_dev emits (src/pipeline.cpp:68-83): the members of a voxel then lie within a few pixels of each other, and the
 * points are grouped through pixel windows in LDS instead of a hash table (no device-scope atomics; csrc/voxel.hip: k_vs_group) - what
 * tdv_register_batch_dev does for its own clouds.  Same voxels, means and order, bit for bit; a cloud or voxel size the window argument
 * does not cover (coarse voxels, rows longer than the halo, points not in pixel order, points whose position cx + fx * x / z or
 * cy + fy * y / z lies more than 0.004 px off an integer pixel: a cloud unprojected with other intrinsics than the ones passed, or moved
 * by a fraction of a pixel) is redone through the table inside the call (tdv_ctx_last_voxel_grouping tells). */
int tdv_voxel_downsample_batch_pinhole_dev(tdv_ctx* ctx, const float* d_xyz, const int* h_cloud_offsets, int n_clouds, float voxel_size,
                                           float fx, float fy, float cx, float cy, float* d_out_xyz, int* h_voxel_offsets);

/* ---- batched, device-resident Pipeline::processInstance ------------------------
 * One call runs the whole per-instance chain of src/pipeline.cpp:25-150 for n_instances masks that
 * share one depth/colour frame and one prepared reference model, without returning to the host
 * between stages (the reference's operator API crosses PCIe at every op boundary):
 *   mask -> depth scale+mask -> unproject -> voxelDownsample -> estimateNormals(k) ->
 *   computeFPFH(voxel * fpfh_radius_factor) -> feature match + RANSAC -> ICP(threshold = voxel *
 *   icp_distance_factor) -> refined transform.
 * All pointers are device pointers; d_masks holds n_instances full-frame uint8 masks back to back;
 * the model (points, normals, FPFH) is what Pipeline::run prepares once (src/pipeline.cpp:291-294);
 * results is a HOST array of n_instances entries.  An instance whose masked depth image holds no non-zero value gets
 * status 1 (the reference returns nullopt at src/pipeline.cpp:57-60, "empty depth after masking"); one that has depth but
 * no pixel inside 0 < z <= zmax gets status 2 (:86-89, "empty point cloud").
 * voxel_order: TDV_VOXEL_ORDER_REFERENCE gives, per instance, exactly what the chain of host-buffer operators (and
 * the reference's processInstance) gives — RANSAC's mt19937 index stream picks points by position, so the pose depends
 * on the order of the downsampled cloud; TDV_VOXEL_ORDER_FIRST skips the computation of the reference's container order
 * (done on the device, ~17 small passes per batch) and yields a different, equally valid, coarse pose.
 * The RANSAC index stream is seeded per instance exactly as the reference does (mt19937(42) restarted for every
 * ransacRegistration call).  Frames: as tdv_depth_to_cloud_batch_dev (n_frames, frame_of_instance).
 * The call spreads the instances over several lanes (the caller's thread plus helper threads, each with its own stream
 * and workspace owned by the ctx): 6 for large instances, 12 for small ones (under 8,192 points on average), never more than the
 * host has hardware threads; TDV_BATCH_LANES=n overrides (at most 16).  Stages that do not depend on an instance run once for the
 * whole batch: the clouds (2 launches), the voxels and their reference order (on the device: no leader leaves it) and, for
 * small instances, the descriptor match of all instances' points against the model. */
typedef struct tdv_batch_params {
    int width, height;
    float scale_to_meters;      /* depth.scale_to_meters      (include/pipeline_config.hpp:18) */
    int mask_mode;              /* TDV_MASK_THRESHOLD10 / TDV_MASK_NONZERO                        */
    float fx, fy, cx, cy, zmax; /* intrinsics; zmax = depth.clipping_max                          */
    float voxel_size;           /* registration.voxel_size                                        */
    int normals_k;              /* 30                        (src/pipeline.cpp:93)                */
    float fpfh_radius_factor;   /* 5.0                       (src/pipeline.cpp:95)                */
    int ransac_max_iterations;  /* registration.ransac_max_iterations                             */
    float ransac_confidence;    /* 0.999                                                          */
    float icp_distance_factor;  /* 0.4                       (src/pipeline.cpp:104)               */
    int icp_max_iterations;     /* registration.icp_max_iterations                                */
    int point_to_plane;         /* registration.use_point_to_plane                                */
    uint32_t seed;              /* 42                        (src/registration.cpp:235)           */
    int voxel_order;            /* TDV_VOXEL_ORDER_FIRST / TDV_VOXEL_ORDER_REFERENCE                */
    int n_frames;               /* depth frames stored back to back at d_raw_depth (0 or 1: one)    */
    const int* frame_of_instance; /* HOST array [n_instances] or NULL (b * n_frames / n_instances)   */
    int mask_format;            /* 0: n_instances stacked u8 masks (mask_mode applies); 1: ONE u8 label image, instance b keeps
                                   the pixels equal to b + 1 (<= 255 instances); 2: ONE u16 label image, same rule (<= 65535
                                   instances).  Label images need n_frames <= 1.  SURVEY.md 8f N2                          */
    int mask_width, mask_height; /* size of the masks when it differs from the frame (0: the frame's): they are resized with
                                   nearest neighbour first, as cv::resize(..., INTER_NEAREST) in src/pipeline.cpp:38-41   */
} tdv_batch_params;

typedef struct tdv_instance_result {
    float T[16];            /* refined.transformation, column-major */
    float fitness, rmse;    /* of the ICP result */
    float coarse_fitness;   /* of the RANSAC result */
    int coarse_inliers;
    int icp_iterations;
    int n_points;           /* unprojected points */
    int n_voxels;           /* after voxelDownsample */
    int status;             /* 0 ok, 1 empty depth after masking, 2 empty cloud */
} tdv_instance_result;

/* cv::resize(mask, out, dsize, 0, 0, cv::INTER_NEAREST) (src/pipeline.cpp:38-41) for n_masks u8 images stored back to back:
 * out(y, x) = in(min(floor(y * ify), sh - 1), min(floor(x * ifx), sw - 1)), ifx = 1 / ((double)dw / sw) in double, as OpenCV's
 * resizeNN computes its index tables.  Host buffers; the _dev form takes device pointers. */
int tdv_mask_resize_nearest(tdv_ctx* ctx, const uint8_t* masks, int n_masks, int src_width, int src_height,
                            int dst_width, int dst_height, uint8_t* out);
int tdv_mask_resize_nearest_dev(tdv_ctx* ctx, const uint8_t* d_masks, int n_masks, int src_width, int src_height,
                                int dst_width, int dst_height, uint8_t* d_out);

int tdv_register_batch_dev(tdv_ctx* ctx, const uint16_t* d_raw_depth, const uint8_t* d_bgr /* may be NULL */,
                           const uint8_t* d_masks, int n_instances, const tdv_batch_params* params,
                           const float* d_model_xyz, const float* d_model_normals, const float* d_model_fpfh, int n_model,
                           tdv_instance_result* results);
/* tdv_register_batch_dev with the caller's poses in place of normals + FPFH + match + RANSAC:
 *   mask -> depth scale+mask -> unproject -> voxelDownsample(voxel_order) -> ICP from h_T0 + 16*b (host, column-major),
 * with the front end (clouds in one pass, the voxels and their reference order) of tdv_register_batch_dev and the ICP of
 * tdv_icp_batch_dev: per instance, bit for bit, the stagewise chain depth_to_cloud -> voxel_downsample(voxel_order) -> icp(T0).
 * Honoured fields of params: the frame, intrinsics and zmax; mask_mode, mask_format, mask_width and mask_height; n_frames and
 * frame_of_instance; voxel_size, voxel_order, icp_distance_factor, icp_max_iterations and point_to_plane.  Ignored: normals_k,
 * fpfh_radius_factor, ransac_* and seed.
 * Results: coarse_fitness = -1 and coarse_inliers = -1 (there is no coarse stage); status, n_points and n_voxels as in
 * tdv_register_batch_dev; an instance with status 1 or 2 gets back its T0 with fitness, rmse and icp_iterations 0.
 * n_instances == 0 is accepted.  Every argument is checked before anything is enqueued: TDV_ERR_BAD_ARG writes nothing to results. */
int tdv_refine_batch_dev(tdv_ctx* ctx, const uint16_t* d_raw_depth, const uint8_t* d_bgr /* may be NULL */,
                         const uint8_t* d_masks, int n_instances, const tdv_batch_params* params, const float* h_T0,
                         const float* d_model_xyz, const float* d_model_normals /* may be NULL */, int n_model,
                         tdv_instance_result* results);
/* Model preparation of src/pipeline.cpp:291-294 on device buffers: voxelDownsample(voxel_order) ->
 * estimateNormals(k) -> computeFPFH(voxel * radius_factor).  Outputs have capacity n. */
int tdv_prepare_model_dev(tdv_ctx* ctx, const float* d_xyz, int n, float voxel_size, int voxel_order, int normals_k,
                          float fpfh_radius_factor, float* d_out_xyz, float* d_out_normals, float* d_out_fpfh, int* n_out /* host */);

/* ---- multi-GPU: instances shard across one process per GPU; the reference's only parallel axis is the
 * same one, over host threads (src/pipeline.cpp:321-327).  rccl_comm is the caller's ncclComm_t (RCCL; one rank per
 * process, created by the host with ncclCommInitRank) — this library does not link RCCL, it resolves ncclBroadcast /
 * ncclAllGather among the process's loaded symbols, else from librccl.so.1, at the first call.  Both calls enqueue on the
 * ctx's stream and return after it has been synchronized; every rank must make the same calls in the same order.
 *
 * tdv_broadcast_model: the prepared model (what tdv_prepare_model_dev / Pipeline::run :291-294 produce) from rank `root`
 * to every rank, in place: on root *n_model is the input count, elsewhere it receives it; buffers hold `capacity` points
 * on every rank (TDV_ERR_BAD_ARG if the model does not fit).  d_normals may be NULL (no normals: ICP falls back to
 * point-to-point, registration.cpp:343); normals travel only if EVERY rank passed a buffer.
 * Rank-local arguments (buffers, capacity, counts) are validated through one all-gather of a 16-byte header before any
 * payload moves, so every rank takes the same branch and returns the SAME status — a bad argument on one rank makes all
 * ranks return TDV_ERR_BAD_ARG instead of leaving the others blocked in a collective.  `root` (and slots_per_rank below)
 * must agree across ranks like the arguments of any collective; a disagreement in slots_per_rank is detected and refused.
 * STATUS: verified on hardware at world size 1 only (tests/test_gpu_comm.py); world > 1 needs more GPUs than a test box has —
 * "parity unpinned" for world > 1 until the driver's multi-GPU run.
 * tdv_gather_results: every rank contributes n_local results in slots_per_rank slots (the same number on every rank,
 * >= n_local; unused slots come back with status -1) and receives all ranks' slots, rank-major, in `all`
 * (world_size * slots_per_rank entries).  Both are host arrays. */
int tdv_broadcast_model(tdv_ctx* ctx, void* rccl_comm, int root, float* d_xyz, float* d_normals, float* d_fpfh, int capacity, int* n_model);
int tdv_gather_results(tdv_ctx* ctx, void* rccl_comm, const tdv_instance_result* local, int n_local, int slots_per_rank,
                       tdv_instance_result* all);

/* ---- host-side helpers that are part of the path's semantics -------------------------------- */
/* The RANSAC index stream: count triples from mt19937(seed) + Lemire uniform over [0, n-1]
 * (src/registration.cpp:235-239 on libstdc++ 11).  Own implementation, no <random>. */
int tdv_sample_triples(uint32_t seed, uint64_t n, int count, uint64_t* out_triples);
/* The same stream in the form tdv_ransac uploads a batch of it (host only; n <= 2^31).  n <= 2^21: *packed = 1 and out
 * receives one 64-bit word per triple - i0 in bits 0..20, i1 in 21..41, i2 in 42..62, bit 63 = the three indices differ
 * (src/registration.cpp:240).  Above: *packed = 0 and out receives four ints per triple (i0, i1, i2, valid).
 * out holds 16 * count bytes either way. */
int tdv_sample_triples_batch(uint32_t seed, uint64_t n, int count, void* out, int* packed);
/* Pose composition of src/pipeline.cpp:136-137: out = extrinsics * inverse(T). */
int tdv_pose_compose(const float* extrinsics, const float* T, float* out);
/* Pipeline::filterDuplicates (src/pipeline.cpp:153-180): greedy pass over n column-major 4x4 poses; a pose
 * within min_distance of a kept one is a duplicate and replaces it only if it is closer to the origin.
 * out_poses has room for n poses; *n_out = kept count. */
int tdv_filter_duplicates(const float* poses, int n, float min_distance, float* out_poses, int* n_out);
/* Test aids (host only): how the scoring dispatches over a RANSAC batch's live list hand out their work.  The chunks [r0, r1) of the
 * point pairs go to the eight XCDs in contiguous shares; an XCD's share of one hypothesis block is drawn in units of
 * tdv_ransac_score_unit_chunks() chunks, ticket by ticket.  tdv_ransac_score_unit: 1 and the unit's chunks [*c0, *c1) for `ticket`
 * of XCD `xcd` (0..7), 0 when the share has no such unit.  tdv_ransac_score_unit_block: the block that workgroup `wg` of an XCD
 * takes at its visit-th move (0 <= visit < n_blk) among n_blk blocks.  TDV_ERR_BAD_ARG for arguments outside these ranges. */
int tdv_ransac_score_unit(int ticket, int r0, int r1, int xcd, int* c0, int* c1);
int tdv_ransac_score_unit_block(int wg, int visit, int n_blk);
int tdv_ransac_score_unit_chunks(void);
/* Test aid (host only): the batch schedule of a RANSAC call that runs with the bail-out (more than 16,384 iterations, not traced, the
 * fast scoring kernel).  The size of the batch that starts at iteration it0: 8,192 at 0, 65,536 while it0 < 270,336, the grown size
 * from there on; the call's last batch is what is left of max_iterations.  TDV_ERR_BAD_ARG for it0 < 0. */
int tdv_ransac_batch_size(int it0);
/* Test aid (host only): the voxel stage's rules as every voxel kernel compiles them.  For each of n points xyz[3 i ...]: its cell
 * (int)floor(p * (1 / voxel_size)) per axis, converted as x86 does (tdv_voxel_downsample), to out_cells[3 i ...], and the reference's
 * key hash of that cell (src/registration.cpp:20-27, std::hash<int> the sign-extended value) to out_codes[i].  TDV_ERR_BAD_ARG for
 * n < 0, a voxel_size that is not positive, or a NULL array with n > 0. */
int tdv_voxel_rules(const float* xyz, int n, float voxel_size, int* out_cells, unsigned long long* out_codes);
/* Registration::loadReferenceModel (src/registration.cpp:416-461): ASCII PLY, x y z [r g b] per vertex.
 * Keeps the reference's behaviour: colours are detected by "red" appearing in any header line and are
 * divided by 255 when r > 1; the header loop consumes the line AFTER end_header, so the first vertex is
 * skipped and the last read fails — the reference then pushes x = 0 and unspecified y, z (and colour);
 * here that last point is (0,0,0) with colour (0,0,0).  out_xyz / out_rgb (either may be NULL) have room
 * for `capacity` points; *n_out = points the reference would return (= the header's vertex count);
 * *has_color = 1 if colours are present.  Returns TDV_ERR_BAD_ARG if the file cannot be opened
 * (the reference returns an empty cloud there). */
int tdv_load_ply_ascii(const char* path, float* out_xyz, float* out_rgb, int capacity, int* n_out, int* has_color);

/* Segmentation::loadMasksFromDir (src/segmentation.cpp:12-42): every .png/.jpg/.jpeg of `dir` in sorted order, read
 * as 8-bit grey and thresholded (> 10 -> 255, else 0).  Decodable here: non-interlaced greyscale PNGs (colour type 0 or
 * 4, any bit depth); colour / palette PNGs and JPEGs are skipped and counted in *n_skipped (their grey conversion
 * depends on the image library).  tdv_load_mask_png: out may be NULL to query the size; capacity in pixels.
 * tdv_load_masks_from_dir: masks of exactly width x height are stacked into out[n][height][width] — the layout
 * tdv_register_batch_dev and tdv_depth_to_cloud_batch_dev take; *n_out = masks found (may exceed capacity_masks when
 * out is NULL: count query).  A missing directory yields 0 masks, as in the reference. */
int tdv_load_mask_png(const char* path, uint8_t* out, long long capacity, int* width, int* height);
int tdv_load_masks_from_dir(const char* dir, int width, int height, uint8_t* out, int capacity_masks, int* n_out, int* n_skipped);

/* The leaf-box bound's lists in the last tdv_ransac* call on this ctx, added up over its bounded batches (every batch after the
 * first of a call without a per-iteration trace): out[0] hypotheses bounded, out[1] of them close to the running best pose and
 * therefore live without a walk, out[2] put on the fine level's list, out[3] live - the hypotheses that were scored at all.  All
 * zero for a call without bounded batches or before any.  The counts are the same from call to call; they change no result. */
void tdv_ctx_last_ransac_bound(tdv_ctx* ctx, long long out[4]);

#ifdef __cplusplus
}
#endif
#endif /* TDV_HIP_H */
