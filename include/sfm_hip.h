/*
 * sfm_hip.h — C-ABI of libsfmhip.so, the MI355X (gfx950) back-end for the
 * incremental-SfM hot path of FlagArihant2000/sfm-mvs.
 *
 * The reference has no FFI of its own: its operator boundary is the set of
 * cv2.* calls made by sfm.py.  Each entry point below names the reference call
 * site (file:line under /root/reference) whose arithmetic it replaces; the
 * ctypes stubs a maintainer would add to sfm.py are shown in INTEGRATION.md.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only.  Every `*_dev` pointer is a
 *     DEVICE pointer (HBM) owned by the caller; `stream` is a hipStream_t
 *     passed as void* (NULL = the null stream).
 *   - All functions are stream-ordered and asynchronous; none synchronises.
 *   - The library allocates nothing persistent: scratch is caller-provided
 *     workspace, sized by the `_ws_bytes` twin of each call.
 *   - Return value: 0 = OK, negative = error code below; a human-readable
 *     message for the calling thread's last error is at sfm_last_error().
 *   - There is NO CPU fallback.  If no HIP device is usable the call fails
 *     with SFM_ERR_DEVICE.
 */
#ifndef SFM_HIP_H
#define SFM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SFM_ABI_VERSION 3   /* 3 (round 6): + sfm_host_poll_count, sfm_debug_pnp_sweep_server; sfm_build_id() names every source file;
                               later, backward-compatible additions: sfm_mvs_plane_sweep, sfm_mvs_consistency; sfm_tsdf_integrate,
                               sfm_mesh_count(_ws_bytes), sfm_mesh_extract(_ws_bytes); sfm_mvs_cost_shift, sfm_mvs_cost_aggregate,
                               sfm_mvs_cost_depth; sfm_mvs_patchmatch */

#define SFM_OK             0
#define SFM_ERR_ARG       -1   /* null pointer, negative size, unsupported dim, misaligned pointer/stride */
#define SFM_ERR_WORKSPACE -2   /* ws_bytes smaller than the _ws_bytes twin reports */
#define SFM_ERR_DEVICE    -3   /* HIP runtime error (launch failure, no device) */

int         sfm_abi_version(void);
const char* sfm_last_error(void);
/* What the loaded binary was built from: "knn.hip:<sha256 of csrc/knn.hip's code> assoc.hip:<first 16 digits> ... sfm_hip.h:<16>",
 * one entry per source file (comments and whitespace do not count; scripts/knn_code_hash.py --build-id prints the same for a tree),
 * " dev-build" appended when the library honours the SFM_KNN_* tuning variables (release builds read none).  The parity sweeps and
 * PMC stamps under profiles/ name these hashes, each family its own sources. */
const char* sfm_build_id(void);

/* ------------------------------------------------------------------------
 * A2  cv2.BFMatcher().knnMatch(des0, des1, k=2)           sfm.py:259-260
 *     (also isfm.py:47,71; test.py:41-42,225,352)
 *
 * Brute-force L2 2-nearest-neighbour of every query row among the train rows.
 * Semantics of OpenCV's batchDistance(NORM_L2, K=2): dist = sqrtf(sum (q-t)^2)
 * in float32, best-2 kept sorted ascending, a candidate replaces only on
 * strict `<`, so on ties the LOWER train index stays ahead.
 *
 *   q_dev   [nq x dim] float32, row stride ldq (elements)   — des0
 *   t_dev   [nt x dim] float32, row stride ldt (elements)   — des1
 *   idx_dev [nq x 2]   int32   trainIdx of 1st / 2nd neighbour (-1 if nt < k)
 *   dist_dev[nq x 2]   float32 DMatch.distance            (+inf if nt < k)
 *   stats_dev (optional, may be NULL) int32[4]:
 *       [0] queries for which at least one filter stream had to be rescanned exactly
 *       [1] filter workgroups launched   [2] candidate streams reserved per query
 *       [3] filter arithmetic that ran: 0 fp16 single product, exact inputs; 1 fp16 single product;
 *           2 bf16 hi/mid split; 3 fp32 MFMA; 4 exact-integer i8 MFMA (u8-integer descriptors: real SIFT output);
 *           5 the i8 MFMA body on float descriptors QUANTISED to 8 bits (certified by their measured residual norms)
 *
 * dim must be 128 (SIFT); q_dev/t_dev 16-byte aligned; ldq, ldt multiples of 4; nt <= 4 000 000.
 * The result is bit-identical to the direct-form float32 evaluation for any finite input whose squared row
 * norms are finite in float32 (|x| up to ~1e18; see docs/knn.md, "Domain of the parity claim").  Beyond that the
 * filters' scores ||t||^2 + ||q||^2 - 2 q.t are +inf / NaN while some direct-form distances are still finite: measured
 * wrong at 3e18, right again from 1e19 on, where every distance is +inf and the index order decides (scripts/dev/q8_huge.py of the round-5 tree).
 *
 * `filter` — the candidate filter that runs before the exact refine.  A per-call argument (ABI 1 had
 * a process-global switch); results are bit-identical whichever runs, the _ws_bytes twin takes the same value:
 *   SFM_KNN_FILTER_AUTO       MFMA filter, fragments streamed L2 -> registers (knn_filter_q4_kernel); its
 *                             arithmetic is chosen ON THE DEVICE from the data: the exact-integer body
 *                             (v_mfma_i32_32x32x32_i8, i32 scores, integer certificate) when every value of the batch is an
 *                             integer 0 .. 255 — what cv2 SIFT emits (sfm.py:246-252) —; the same body on the pairs'
 *                             values QUANTISED to 8 bits (x ~ lo + s k, one grid per pair from a sample of its rows, the
 *                             residual norms measured, | ||q - t|| - s sqrt(D) | <= ||q - q^|| + ||t - t^|| as the
 *                             certificate, survivors re-evaluated in float32) when the sampled values have compact
 *                             support (range <= 5 standard deviations: e.g. uniform data) and the grid turns out to
 *                             fit; else one fp16 product when the values fit fp16's range, else the three-product
 *                             bf16 hi/mid split
 *   SFM_KNN_FILTER_NOQUANT    as AUTO, but float data never run quantised (the exact-integer body still serves u8 data)
 *   SFM_KNN_FILTER_HALF       as AUTO without the exact-integer body (16-bit arithmetic whatever the data)
 *   SFM_KNN_FILTER_F32        fp32 MFMA filter (single pair only)
 *   SFM_KNN_FILTER_SPLIT      as AUTO but pinned to the bf16 split
 *   SFM_KNN_FILTER_LDS, SFM_KNN_FILTER_LDS_SPLIT   round 2's LDS-ring kernel (knn_filter_split2_kernel), auto / pinned
 * ---------------------------------------------------------------------- */
#define SFM_KNN_FILTER_AUTO      0
#define SFM_KNN_FILTER_F32       1
#define SFM_KNN_FILTER_SPLIT     2
#define SFM_KNN_FILTER_LDS       3
#define SFM_KNN_FILTER_LDS_SPLIT 4
#define SFM_KNN_FILTER_HALF      5
#define SFM_KNN_FILTER_NOQUANT   6
size_t sfm_knn2_l2_f32_ws_bytes(int64_t nq, int64_t nt, int dim, int filter);
int    sfm_knn2_l2_f32(const float* q_dev, int64_t nq, int64_t ldq,
                       const float* t_dev, int64_t nt, int64_t ldt, int dim, int filter,
                       int32_t* idx_dev, float* dist_dev, int32_t* stats_dev,
                       void* ws_dev, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * A3  Lowe ratio loop + gather                           sfm.py:262-268
 *     `if m.distance < 0.70 * n.distance: good.append(m)`
 *
 * The reference compares float32 distances promoted to Python double against
 * a double constant; the kernel does exactly that in fp64.  Survivors are
 * written in ascending queryIdx order (the order of the Python loop).
 *
 *   out_q_dev, out_t_dev [nq] int32   queryIdx / trainIdx of survivors
 *   out_count_dev        [1]  int32   number of survivors M
 *   mask_dev (optional)  [nq] uint8   1 where the query passed
 *   idx_dev / dist_dev must be 8-byte aligned (they are the outputs of sfm_knn2_l2_f32)
 * ---------------------------------------------------------------------- */
size_t sfm_ratio_compact_ws_bytes(int64_t nq);
int sfm_ratio_compact(const int32_t* idx_dev, const float* dist_dev, int64_t nq,
                      double ratio, int32_t* out_q_dev, int32_t* out_t_dev,
                      int32_t* out_count_dev, uint8_t* mask_dev,
                      void* ws_dev, size_t ws_bytes, void* stream);

/* A2 + A3 in one call: the matcher part of find_features (sfm.py:259-266).  Same outputs as
 * sfm_knn2_l2_f32 followed by sfm_ratio_compact, bit for bit; the Lowe test is folded into the
 * last KNN kernel, which saves one launch per image pair.  Workspace: sfm_match_l2_f32_ws_bytes. */
size_t sfm_match_l2_f32_ws_bytes(int64_t nq, int64_t nt, int dim, int filter);
int sfm_match_l2_f32(const float* q_dev, int64_t nq, int64_t ldq,
                     const float* t_dev, int64_t nt, int64_t ldt, int dim, int filter, double ratio,
                     int32_t* idx_dev, float* dist_dev,
                     int32_t* out_q_dev, int32_t* out_t_dev, int32_t* out_count_dev,
                     uint8_t* mask_dev /*optional*/, int32_t* stats_dev /*optional*/,
                     void* ws_dev, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * The same for `batch` (1..8) image pairs of ONE shape in one set of launches — what a caller
 * with many independent pairs (sfm.py:347 matches every consecutive pair; isfm.py:56-71 all
 * pairs) should use: the filter's unit space becomes batch x query row blocks x train tiles
 * under a single work partition, so a workgroup's prologue, the launch ramp and the kernel
 * boundaries are paid once per batch instead of once per pair (10k x 10k: 31 -> ~23 us of
 * filter time per pair at batch 4).  Results are those of `batch` separate calls, bit for bit.
 * q, t, idx, dist, out_q, out_t, out_count, mask, stats: HOST arrays of `batch` device
 * pointers (mask / stats: NULL array or NULL entries allowed); all pairs share nq, nt, ldq, ldt.
 * Not available with SFM_KNN_FILTER_F32 (the fp32-MFMA variant is single-pair).
 * ---------------------------------------------------------------------- */
size_t sfm_match_batch_l2_f32_ws_bytes(int64_t nq, int64_t nt, int dim, int batch, int filter);
int sfm_match_batch_l2_f32(int batch, const float* const* q_dev, int64_t nq, int64_t ldq,
                           const float* const* t_dev, int64_t nt, int64_t ldt, int dim, int filter, double ratio,
                           int32_t* const* idx_dev, float* const* dist_dev, int32_t* const* out_q_dev,
                           int32_t* const* out_t_dev, int32_t* const* out_count_dev, uint8_t* const* mask_dev,
                           int32_t* const* stats_dev, void* ws_dev, size_t ws_bytes, void* stream);

/* Self-test of the hardware property the KNN certificate's "MFMA chain" term rests on: how far one MFMA is from the exact
 * c + sum a_k b_k, in units of 2^-24 (|c| + sum |a_k b_k|), maximum over 4096 waves x trials_per_wave MFMAs x 1024 outputs, for
 * seven operand regimes (equal exponents ... 2^16 spread with cancellation; the last one is the filter's own).
 * kind: 0 v_mfma_f32_32x32x16_f16, 1 v_mfma_f32_32x32x16_bf16, 2 v_mfma_f32_32x32x8_bf16 (the accumulator-init MFMA).
 * regime_max_host: 7 doubles; ws: 32 KiB + 512 B of device memory.  Synchronises `stream`. */
int sfm_selftest_mfma_accumulation(int kind, int trials_per_wave, double* regime_max_host, void* ws_dev, size_t ws_bytes,
                                   void* stream);

/* What the library measured on the CURRENT device the first time a 16-bit KNN filter ran there (it runs the self-test above
 * once per device and process: a few ms and one synchronisation of a private stream, inside that first call): the largest E
 * over the three MFMA kinds and seven regimes, and the factor applied to the certificate's chain term — 1 while E <= 8 (the
 * certificate assumes 16), E / 8 above: an unknown matrix pipe costs speed (more rescans), never exactness. */
int sfm_knn_mfma_selftest_result(double* worst_units_host, float* chain_scale_host);

/* Gather keypoint coordinates of the survivors: pts0 = kp0[out_q], pts1 = kp1[out_t]
 * (sfm.py:267-268).  kp*_dev are [n x 2] float32 (KeyPoint.pt); count_dev is the
 * device scalar written by sfm_ratio_compact; capacity = rows available in pts*_dev. */
int sfm_gather_matches(const float* kp0_dev, const float* kp1_dev,
                       const int32_t* out_q_dev, const int32_t* out_t_dev,
                       const int32_t* count_dev, int64_t capacity,
                       float* pts0_dev, float* pts1_dev, void* stream);

/* ------------------------------------------------------------------------
 * A2, train set split over `shards` devices (SURVEY 8e's fallback for one pair
 * whose train descriptors do not fit one device): merge of the shards' partial
 * knnMatch(k=2) results into the result of a single scan (sfm.py:259-260).
 *   cand_dev [shards][2][nq][2] int32: per shard the (GLOBAL) trainIdx plane and
 *   the distance-bits plane of its partial result (idx < 0: no neighbour) — the
 *   layout one all-gather of the shards' result blocks produces;
 *   out_idx_dev [nq][2] int32 (-1: none), out_dist_dev [nq][2] float32 (0: none).
 * Order: (distance, trainIdx) — the lower index wins ties, as BFMatcher's scan.
 * ---------------------------------------------------------------------- */
int sfm_knn_merge_top2(const int32_t* cand_dev, int shards, int64_t nq, int32_t* out_idx_dev, float* out_dist_dev, void* stream);

/* ------------------------------------------------------------------------
 * A9  common_points(pts1, pts2, pts3)                       sfm.py:215-239
 *
 * For every row i of pts1 ([n1 x 2] float32) the FIRST row of pts2 ([n2 x 2])
 * whose x OR y is bit-equal (the reference's broadcast `pts2 == pts1[i,:]`,
 * SURVEY 3.6-2).  Matches are written in ascending i:
 *   idx1_dev, idx2_dev [n1] int32   (indx1, indx2), first *count_dev entries valid
 *   keep2_dev [n2] uint8            0 for rows of pts2 (and pts3) named in indx2 —
 *                                   the complement the reference mask-compresses
 *   first_ws_dev [n1] int32         scratch
 * ---------------------------------------------------------------------- */
int sfm_common_points(const float* pts1_dev, int64_t n1, const float* pts2_dev, int64_t n2,
                      int32_t* first_ws_dev, int32_t* idx1_dev, int32_t* idx2_dev,
                      int32_t* count_dev, uint8_t* keep2_dev, void* stream);

/* ------------------------------------------------------------------------
 * Mask -> row indices: `pts0[mask.ravel() == 1]` (sfm.py:309: OpenCV's {0,1} essential-matrix mask),
 * `pts0[mask.ravel() > 0]` (sfm.py:313: the {0,255} cheirality mask), and the complement rows of
 * common_points (sfm.py:233-238).  idx_out_dev [n] int32 receives the rows whose mask byte passes —
 * mode 0: byte == 1, mode 1: byte != 0 — in ascending order, *count_dev their number; the row gather
 * itself is then an indexed copy.  Deterministic (two passes, no atomics).
 * ---------------------------------------------------------------------- */
size_t sfm_mask_indices_ws_bytes(int64_t n);
int sfm_mask_indices(const uint8_t* mask_dev, int64_t n, int mode, int32_t* idx_out_dev, int32_t* count_dev,
                     void* ws_dev, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * A4  cv2.triangulatePoints(P1, P2, points1, points2)    sfm.py:53
 *     + `cloud = cloud / cloud[3]`                        sfm.py:54
 *
 * Per correspondence: homogeneous DLT in fp64, X = right singular vector of the
 * smallest singular value (one-sided Jacobi as in OpenCV's SVD), cast to
 * float32.  rows = 4 → modern 4x4 system (x*P3-P1, y*P3-P2 per view);
 * rows = 6 → legacy cvTriangulatePoints 6x4 system (adds x*P2-y*P1).
 * normalise_w = 1 additionally performs the reference's float32 division by w.
 * normalise_w = 2 (rows = 4 only) is the same normalised result by a ~20x cheaper route:
 *   the smallest eigenvector of A^T A by inverse iteration (LDL^T, fp64), unit-normalised,
 *   cast and divided exactly like the faithful path — bit-identical to it on > 99.9 % of
 *   points, within 1 float32 ulp otherwise; lanes that do not converge (degenerate geometry),
 *   or whose conditioning the normal equations cannot carry (16 sens > 2^-26 |w|, sens as in
 *   normalise_w = 3: a baseline of 1e-4 of the depth), run the Jacobi sweeps.  The un-normalised vector (normalise_w = 0) has OpenCV's sign and
 *   is only offered by the faithful path.
 * normalise_w = 3 (rows = 4 only) is the GUARDED fast path: the result of 2 is kept only where every component of the unit
 *   vector keeps a margin of max(2^-40, 16 eps lambda1/lambda3) from the nearest float32 rounding boundary (the distance
 *   two backward-stable solutions of this point can have; lambda1/lambda3 is read off the iteration), the other points —
 *   a fraction of a percent on well-conditioned geometry, all of them when the baseline vanishes — are redone by the
 *   Jacobi sweeps in a second, compacted pass: bit-identical to normalise_w = 1 on every point.
 *   Scratch: this entry point takes no workspace.  For n >= 2^18 the guarded path asks the device's default memory pool
 *   for n / 8 + 2 ints ON THE CALLER'S STREAM (hipMallocAsync / hipFreeAsync: stream-ordered, no synchronisation) — the
 *   first pass's compact list of rejected points; if the request is refused, or the list overflows, the second pass finds
 *   the marked points by scanning X4 as it does for smaller calls.  Same results either way.
 *
 *   P1, P2        HOST pointers, 12 doubles each, row-major 3x4
 *   x1_dev,x2_dev float32; point i has x at [i*stride_pt] and y at
 *                 [i*stride_pt + stride_xy] — covers (2,N) (stride_pt=1,
 *                 stride_xy=N), (N,2) (2,1) and the reference's transposed views
 *   X4_dev        float32 [4 x n] row-major (the cv2 output layout)
 * ---------------------------------------------------------------------- */
int sfm_triangulate_dlt(const double* P1_host, const double* P2_host,
                        const float* x1_dev, const float* x2_dev, int64_t n,
                        int64_t stride_pt, int64_t stride_xy, int rows,
                        int normalise_w, float* X4_dev, void* stream);

/* ------------------------------------------------------------------------
 * A3 + A4 for `batch` (1..8) image pairs in one set of launches: the Lowe loop and keypoint gather of
 * find_features (sfm.py:262-268) followed by Triangulation (sfm.py:53-54: cv2.triangulatePoints and
 * `cloud / cloud[3]`) — what the pair-sharded path runs on a rank's own pairs before the all-gather of
 * the 3-D points.  Input are the KNN blocks sfm_knn2_l2_f32 / sfm_match_batch_l2_f32 wrote (here or on
 * another rank); nothing goes through the host and no survivor list or gathered coordinate array is
 * materialised:  survivors = queries with a second neighbour and (double)d0 < ratio * (double)d1, in
 * ascending queryIdx order; column e of the output is the triangulation of (kp0[queryIdx_e],
 * kp1[trainIdx_e]) under (P[b][0], P[b][1]), computed as sfm_triangulate_dlt(rows = 4, normalise_w = 3)
 * does (bit-identical to normalise_w = 1); columns >= the survivor count are zeroed.
 *   knn_idx_dev, knn_dist_dev, kp0_dev, kp1_dev, X4_dev, count_dev: HOST arrays of `batch` device pointers
 *     knn_idx_dev[b] [nq_b x 2] int32, knn_dist_dev[b] [nq_b x 2] float32 (8-byte aligned)
 *     kp0_dev[b], kp1_dev[b]   [n x 2] float32 KeyPoint.pt of the query / train image (8-byte aligned)
 *     X4_dev[b]                float32 [4 x cap] row-major;  count_dev[b] int32[1] (array or entries may be NULL)
 *   nq_host  `batch` query counts (<= cap);  P_host [batch][2][12] doubles (row-major 3x4 of both views)
 * ---------------------------------------------------------------------- */
size_t sfm_triangulate_matches_batch_ws_bytes(int batch, int64_t cap);
int sfm_triangulate_matches_batch(int batch, const int32_t* const* knn_idx_dev, const float* const* knn_dist_dev,
                                  const int64_t* nq_host, double ratio,
                                  const float* const* kp0_dev, const float* const* kp1_dev,
                                  const double* P_host, int64_t cap, float* const* X4_dev,
                                  int32_t* const* count_dev, void* ws_dev, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * A5  ReprojectionError: cv2.Rodrigues + cv2.projectPoints + cv2.norm
 *                                                        sfm.py:79-100
 * A6  solvePnPRansac inlier scoring                      sfm.py:67
 * A8  OptimReprojectionError / BundleAdjustment sweep    sfm.py:104-157
 *
 * One sweep over `nobs` observations.  Observation o sees point pt_idx[o]
 * through camera cam_idx[o]; either index array may be NULL (NULL cam_idx =
 * camera 0; NULL pt_idx = point o).  Projection is OpenCV's distortion-free
 * projectPoints in fp64: X' = R(rvec) X + t, u = fx X'/Z' + cx, v = fy Y'/Z' + cy
 * (skew ignored).  Optional outputs (pass NULL to skip):
 *   proj_dev    [nobs x 2] float32  projected pixel (the `p` of sfm.py:88-90)
 *   sumsq_dev   [1] float64  sum over o of ||f32(proj) - obs||^2, i.e. the
 *               square of cv2.norm(p, pts, NORM_L2) (sfm.py:93,95); caller
 *               zeroes it; accumulation is a fixed-order two-level sum
 *   inlier_dev  [nobs] uint8  1 iff float32 squared error <= thr2 (PnP-RANSAC)
 *   JtJ_cam_dev [ncam x 36], Jtr_cam_dev [ncam x 6] float64: Gauss-Newton normal
 *               equations per camera in (rvec, tvec), residual = proj - obs
 *   JtJ_pt_dev  [npt x 9],  Jtr_pt_dev [npt x 3] float64: same per 3D point
 *   res2_dev    [1] float64  sum of ||proj - obs||^2 in fp64 (the squared error norm
 *               OpenCV's Levenberg-Marquardt compares); accumulated (+=), caller zeroes
 *   cams_dev    [ncam x 6] float64 (rvec3, tvec3);  K_host 9 doubles row-major
 *   X_dev       [npt x 3] float32 with row stride ldx
 * ---------------------------------------------------------------------- */
size_t sfm_project_residual_ws_bytes(int64_t nobs, int64_t ncam, int64_t npt);
int sfm_project_residual(const double* cams_dev, int64_t ncam, const double* K_host,
                         const float* X_dev, int64_t npt, int64_t ldx,
                         const float* obs_dev, const int32_t* cam_idx_dev,
                         const int32_t* pt_idx_dev, int64_t nobs,
                         float* proj_dev, double* sumsq_dev,
                         uint8_t* inlier_dev, float thr2,
                         double* JtJ_cam_dev, double* Jtr_cam_dev,
                         double* JtJ_pt_dev, double* Jtr_pt_dev, double* res2_dev,
                         void* ws_dev, size_t ws_bytes, void* stream);

/* Dense visibility variant (BASELINE config 4: every camera sees every point).
 * obs_dev is [ncam x npt x 2] float32.  Same arithmetic as above; per-camera
 * blocks are reduced in a fixed order and per-point blocks are owned by one lane,
 * so the result is deterministic and needs no atomics.  All outputs (sumsq
 * included) are OVERWRITTEN, not accumulated; JtJ_* / Jtr_* may be NULL. */
size_t sfm_ba_dense_sweep_ws_bytes(int64_t ncam, int64_t npt);
int sfm_ba_dense_sweep(const double* cams_dev, int64_t ncam, const double* K_host,
                       const float* X_dev, int64_t npt, int64_t ldx,
                       const float* obs_dev, double* sumsq_dev,
                       double* JtJ_cam_dev, double* Jtr_cam_dev,
                       double* JtJ_pt_dev, double* Jtr_pt_dev,
                       void* ws_dev, size_t ws_bytes, void* stream);

/* Matrix-free products with the camera-point coupling W of the dense normal equations
 *     [ B   W ] [dc]   [g_c]       W_ij = Jc_ij^T Jp_ij  (6x3),  B, C, g_c, g_p from sfm_ba_dense_sweep
 *     [ W^T C ] [dp] = [g_p]
 * for a Schur-complement solver (replaces scipy least_squares + finite differences,
 * sfm.py:138-157): S = B - W C^-1 W^T is applied as  S x = B x - W (C^-1 (W^T x)).
 *   sfm_ba_schur_wt:  u_pt_dev  [npt x 3]  = W^T x,   x_cam_dev [ncam x 6]
 *   sfm_ba_schur_w :  w_cam_dev [ncam x 6] = W v,     v_pt_dev  [npt x 3]
 * The W blocks are never stored: both Jacobians are re-derived from (cams, X) in registers, so a
 * product reads no observation data.  Fixed-order reductions: deterministic.  fp64 throughout. */
size_t sfm_ba_schur_ws_bytes(int64_t ncam, int64_t npt);
int sfm_ba_schur_wt(const double* cams_dev, int64_t ncam, const double* K_host,
                    const float* X_dev, int64_t npt, int64_t ldx,
                    const double* x_cam_dev, double* u_pt_dev,
                    void* ws_dev, size_t ws_bytes, void* stream);
int sfm_ba_schur_w(const double* cams_dev, int64_t ncam, const double* K_host,
                   const float* X_dev, int64_t npt, int64_t ldx,
                   const double* v_pt_dev, double* w_cam_dev,
                   void* ws_dev, size_t ws_bytes, void* stream);
/* Sparse visibility (observation o = camera cam_idx[o] sees point pt_idx[o]): mode 0 → out = W^T in,
 * mode 1 → out = W in.  One lane per observation, fp64 atomics (order-dependent in the last bits). */
size_t sfm_ba_schur_indexed_ws_bytes(int64_t ncam);
int sfm_ba_schur_indexed(const double* cams_dev, int64_t ncam, const double* K_host,
                         const float* X_dev, int64_t npt, int64_t ldx,
                         const int32_t* cam_idx_dev, const int32_t* pt_idx_dev, int64_t nobs, int mode,
                         const double* in_dev, double* out_dev,
                         void* ws_dev, size_t ws_bytes, void* stream);

/* One damped Gauss-Newton (Levenberg-Marquardt) step of the DENSE problem, solved on the device: the reduced camera system
 *     S dc = g_c - W Cd^-1 g_p,   S = Bd - W Cd^-1 W^T,   dp = Cd^-1 (g_p - W^T dc),   Bd / Cd = blocks with diagonals x (1 + lam)
 * by block-Jacobi-preconditioned conjugate gradients; S is applied matrix-free (the two products above), the CG vectors and
 * scalars stay on the device, the host reads the residual norm every fifth iteration.  Inputs: the blocks
 * sfm_ba_dense_sweep returned at (cams, X).  Outputs: dc_dev [ncam x 6], dp_dev [npt x 3] (update = parameters - step);
 * iters_host = CG iterations run; status_host bit 0 = a singular camera block was met (its preconditioner block is the
 * identity), bit 1 = a singular point block.  Synchronises `stream`.  Replaces the reference's
 * scipy.optimize.least_squares call (sfm.py:146), which differentiates the dense problem by finite differences. */
size_t sfm_ba_schur_solve_ws_bytes(int64_t ncam, int64_t npt);
int sfm_ba_schur_solve(const double* cams_dev, int64_t ncam, const double* K_host, const float* X_dev, int64_t npt, int64_t ldx,
                       const double* JtJ_cam_dev, const double* Jtr_cam_dev, const double* JtJ_pt_dev, const double* Jtr_pt_dev,
                       double lam, int fix_first_camera, double cg_tol, int cg_iters, double* dc_dev, double* dp_dev,
                       int32_t* iters_host, int32_t* status_host, void* ws_dev, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Small batched block kernels of the Schur-complement solver (row f-3; the reference hands the
 * problem to SciPy's dense least_squares, sfm.py:146) and cv2.norm of the metric (sfm.py:93,95).
 *   sfm_block_inverse  A_dev [n x k x k] f64 (k = 3 point blocks, 6 camera blocks) -> Ainv_dev
 *   sfm_block_matvec   y_i = A_i x_i;  x_dev, y_dev [n x k]
 *   sfm_norm_l2        cv2.norm(a, b, NORM_L2) over n elements (float32, or float64 with is_f64):
 *                      differences in the inputs' type, squares accumulated in double, fixed
 *                      order; b_dev may be NULL (norm of a).  out_dev: one double (device).
 * ---------------------------------------------------------------------- */
int sfm_block_inverse(const double* A_dev, int64_t n, int k, double* Ainv_dev, void* stream);
/* ... with a device status word: *bad_count_dev = number of blocks whose Gauss-Jordan met a zero or non-finite pivot (their
 * inverse is non-finite); the caller decides (sfm_mvs_amd.ops.block_inverse raises unless told otherwise). */
int sfm_block_inverse_checked(const double* A_dev, int64_t n, int k, double* Ainv_dev, int32_t* bad_count_dev, void* stream);
int sfm_block_matvec(const double* A_dev, const double* x_dev, int64_t n, int k, double* y_dev, void* stream);
size_t sfm_norm_l2_ws_bytes(void);
int sfm_norm_l2(const void* a_dev, const void* b_dev, int64_t n, int is_f64, double* out_dev,
                void* ws_dev, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * A7  cv2.findEssentialMat RANSAC scoring                sfm.py:307
 *
 * For h candidate essential matrices (host-generated by the 5-point solver)
 * score n K-normalised correspondences with the Sampson distance in fp64,
 * cast to float32 and compared `<= thr2` as OpenCV's RANSAC does.
 *   E_dev [h x 9] f64;  x1n_dev, x2n_dev [n x 2] f64
 *   counts_dev [h] int32;  mask_dev (optional) [h x n] uint8
 * ---------------------------------------------------------------------- */
int sfm_score_essential(const double* E_dev, int h, const double* x1n_dev,
                        const double* x2n_dev, int64_t n, float thr2,
                        int32_t* counts_dev, uint8_t* mask_dev, void* stream);

/* cv2.recoverPose cheirality vote (sfm.py:311): for up to 4 candidate poses [R|t]
 * (P_host: h x 12 doubles, row-major 3x4) triangulate every K-normalised pair
 * against [I|0] in fp64 and count points with positive depth < dist_thresh in
 * both views.  mask (optional) [h x n] uint8 is 255/0 like OpenCV's. */
int sfm_recover_pose_score(const double* P_host, int h, const double* x1n_dev,
                           const double* x2n_dev, int64_t n, double dist_thresh, int rows,
                           int32_t* counts_dev, uint8_t* mask_dev, void* stream);

/* PnP-RANSAC scoring for h hypotheses (rvec,tvec) over n 3D-2D pairs:
 * err = ||proj - obs||^2 as float32, inlier iff err <= thr2 (sfm.py:67 defaults:
 * reprojectionError 8.0 → thr2 = 64). */
int sfm_score_pnp(const double* poses_dev, int h, const double* K_host,
                  const float* X_dev, const float* obs_dev, int64_t n, float thr2,
                  int32_t* counts_dev, uint8_t* mask_dev, void* stream);

/* ------------------------------------------------------------------------
 * A7  cv2.findEssentialMat(points1, points2, K, method=RANSAC, prob, threshold)      sfm.py:307
 *     (also isfm.py:80, test.py:240)
 * The whole call: K-normalisation, five-point hypotheses (host) drawn with OpenCV's RNG,
 * Sampson scoring of a chunk of hypotheses per launch (device), OpenCV's sequential
 * best-model / niters bookkeeping.  Returns host scalars, so it synchronises `stream`.
 *   pts0_dev, pts1_dev [n x 2] float32 (pixels);  K_host 9 doubles (row-major 3x3)
 *   E_host      9 doubles (row-major);  90 when n == 5 (OpenCV then returns all the solver's models stacked)
 *   info_host   int32[4]: [0] models written to E_host (0 = no model), [1] inlier count,
 *               [2] RANSAC iterations run, [3] models scored
 *   mask_dev    [n] uint8, 1 = inlier of the returned model (OpenCV's {0,1} mask)
 * ---------------------------------------------------------------------- */
size_t sfm_find_essential_mat_ws_bytes(int64_t n);
int sfm_find_essential_mat(const float* pts0_dev, const float* pts1_dev, int64_t n, const double* K_host,
                           double prob, double threshold, int max_iters, double* E_host, int32_t* info_host,
                           uint8_t* mask_dev, void* ws_dev, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * A7' cv2.recoverPose(E, points1, points2, K)                                        sfm.py:311
 * decomposeEssentialMat (host) + the cheirality vote of the four (R, t) candidates over all
 * correspondences (device, fp64 DLT per point, distanceThresh = 50 by default) + OpenCV's
 * cascade of >= tests.  rows = 4 (current cv::triangulatePoints system) or 6 (legacy).
 *   R_host 9 doubles, t_host 3 doubles (unit norm), good_host int32[1] = return value of recoverPose
 *   mask_dev (optional) [n] uint8, 255 = point passed the vote (OpenCV's {0,255} mask)
 * ---------------------------------------------------------------------- */
size_t sfm_recover_pose_ws_bytes(int64_t n);
int sfm_recover_pose(const double* E_host, const float* pts0_dev, const float* pts1_dev, int64_t n,
                     const double* K_host, double distance_thresh, int rows, double* R_host, double* t_host,
                     int32_t* good_host, uint8_t* mask_dev, void* ws_dev, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * A6  cv2.solvePnPRansac(objectPoints, imagePoints, K, distCoeffs = 0)               sfm.py:67
 * (the reference's 5th positional argument lands in OpenCV's `rvec` slot — SURVEY 3.6-1 — so
 * every tunable is the default: iterations 100, reprojectionError 8.0, confidence 0.99,
 * flags ITERATIVE).  EPnP hypotheses on 5-point samples (host), reprojection scoring of a
 * chunk of hypotheses per launch (device), then solvePnP(ITERATIVE) on the inliers: DLT
 * initialisation (host) and Levenberg-Marquardt whose residual / J^T J sweeps run on the
 * device.  n >= 5 (OpenCV's P3P branch for n == 4 is not on this path: SFM_ERR_ARG).
 *   X_dev [n x 3] float32, uv_dev [n x 2] float32;  rvec_host, tvec_host 3 doubles each
 *   info_host   int32[4]: [0] 1 = pose found, [1] inlier count, [2] initialisation of the
 *               refinement (0 DLT, 1 planar object / 2 fewer than 6 inliers: the RANSAC model
 *               is refined instead — OpenCV uses a homography / raises there), [3] LM iterations
 *   inliers_dev [n] int32: indices of the best RANSAC model's inliers, ascending (first info[1])
 * ---------------------------------------------------------------------- */
size_t sfm_solve_pnp_ransac_ws_bytes(int64_t n);
int sfm_solve_pnp_ransac(const float* X_dev, const float* uv_dev, int64_t n, const double* K_host, int iterations,
                         float reproj_error, double confidence, double* rvec_host, double* tvec_host,
                         int32_t* info_host, int32_t* inliers_dev, void* ws_dev, size_t ws_bytes, void* stream);

/* cv2.projectPoints(X, rvec, tvec, K, None) on float64 object points (sfm.py:119-121: the residual of the
 * reference's BundleAdjustment is fp64 end to end).  rvec, tvec, K on the host; X_dev [n x 3], proj_dev [n x 2] f64. */
int sfm_project_points_f64(const double* rvec_host, const double* tvec_host, const double* K_host,
                           const double* X_dev, int64_t n, double* proj_dev, void* stream);

/* ------------------------------------------------------------------------
 * The host-side hypothesis generators behind the three calls above, reachable on their own
 * (pure host code, HOST pointers, no GPU needed): unit-tested against the oracle.
 *   sfm_host_epnp                 EPnP on 4..64 correspondences (solvePnPRansac's minimal solver):
 *                                 K 9 doubles, Xw [n x 3], uv [n x 2] pixels -> R 9, t 3 doubles
 *   sfm_host_p3p                  solvePnP(P3P) on exactly four correspondences (solvePnPRansac's npoints == 4
 *                                 branch): Xw [4 x 3], uv [4 x 2] pixels -> R 9, t 3 doubles, ok_host 1 / 0
 *   sfm_host_five_point           five K-normalised correspondences [5 x 2] each -> up to 10
 *                                 essential matrices (E_host 90 doubles), count_host int32
 *   sfm_host_decompose_essential  E -> R1, R2 (9 doubles each), t (3)
 *   sfm_host_pnp_dlt_init         ITERATIVE's non-planar initialisation: X [n x 3], uv [n x 2]
 *                                 doubles -> rvec, tvec; status 0 ok / 1 planar / 2 fewer than 6 points
 *   sfm_host_rodrigues            cv2.Rodrigues (sfm.py:69,84,119): src 3 (vector) or 9 (matrix)
 *                                 doubles; jac_host (optional, vector input) dR/dr 3 x 9
 * ---------------------------------------------------------------------- */
int sfm_host_epnp(const double* K_host, const double* Xw_host, const double* uv_host, int n,
                  double* R_host, double* t_host);
int sfm_host_p3p(const double* K_host, const double* Xw_host, const double* uv_host, double* R_host, double* t_host,
                 int32_t* ok_host);
int sfm_host_five_point(const double* x1n_host, const double* x2n_host, double* E_host, int32_t* count_host);
int sfm_host_decompose_essential(const double* E_host, double* R1_host, double* R2_host, double* t_host);
int sfm_host_pnp_dlt_init(const double* K_host, const double* X_host, const double* uv_host, int64_t n,
                          double* rvec_host, double* tvec_host, int32_t* status_host);
int sfm_host_rodrigues(const double* src_host, int src_is_matrix, double* dst_host, double* jac_host);

/* ------------------------------------------------------------------------
 * Next row f-1: image preprocessing + SIFT
 *   cv2.pyrDown(img)                                  sfm.py:40
 *   cv2.cvtColor(img, cv2.COLOR_BGR2GRAY)             sfm.py:243-244
 *   cv2.xfeatures2d.SIFT_create().detectAndCompute(gray, None)   sfm.py:246-252
 *
 * sfm_bgr2gray_u8 / sfm_pyrdown_u8: OpenCV's uint8 fixed-point programs
 * ((1868 B + 9617 G + 4899 R + 8192) >> 14; 5x5 binomial, (sum + 128) >> 8,
 * BORDER_REFLECT_101, output ((w+1)/2, (h+1)/2)).  All pointers are device memory.
 *
 * sfm_sift_detect_and_compute: the whole of detectAndCompute (nfeatures = 0), stream
 * ordered, no host round trip: 2x bilinear base image, Gaussian / DoG pyramid,
 * 26-neighbour extrema with sub-pixel refinement, contrast and edge tests,
 * orientation histograms (one keypoint per peak >= 0.8 max), OpenCV's keypoint
 * ordering + duplicate removal, 4x4x8 descriptors (clip 0.2, x512, u8-valued float32).
 *   gray_dev        [h x stride] uint8
 *   max_keypoints   capacity of the outputs and of the internal lists, 64 <= max_keypoints < 2^24
 *   keypoints_dev   [max_keypoints x 8] float32: x, y, size, angle (degrees), response,
 *                   octave (int32 bits, OpenCV packing), class_id (int32 bits, -1), 0
 *   descriptors_dev [max_keypoints x 128] float32 (NULL: detect only)
 *   count_dev       int32[4]: [0] keypoints written (ordered), [1] keypoints before
 *                   duplicate removal, [2] refined extrema, [3] raw extrema (before the
 *                   contrast / edge tests); [1] or [2] > max_keypoints, or [3] >
 *                   8 * max_keypoints, means a capacity was exceeded and the output is truncated
 * Blur kernels longer than 55 taps (a per-layer sigma above 6.8) are rejected with
 * SFM_ERR_ARG; the defaults (3, 0.04, 10, 1.6) need 27.
 * ---------------------------------------------------------------------- */
int sfm_bgr2gray_u8(const uint8_t* bgr_dev, int64_t w, int64_t h, int64_t stride_bytes, uint8_t* gray_dev, void* stream);
int sfm_pyrdown_u8(const uint8_t* src_dev, int64_t w, int64_t h, int channels, uint8_t* dst_dev, void* stream);
size_t sfm_sift_ws_bytes(int64_t w, int64_t h, int n_octave_layers, int64_t max_keypoints);
int sfm_sift_detect_and_compute(const uint8_t* gray_dev, int64_t w, int64_t h, int64_t stride_bytes,
                                int n_octave_layers, double contrast_threshold, double edge_threshold,
                                double sigma, int64_t max_keypoints, float* keypoints_dev,
                                float* descriptors_dev, int32_t* count_dev, void* ws, size_t ws_bytes,
                                void* stream);

/* ------------------------------------------------------------------------
 * MVS  dense reconstruction                     sfm.py:298 (`densify = False`)
 *      the cloud of to_ply's dense.ply branch   sfm.py:199
 *
 * The reference stops at the sparse cloud; these two entry points are the
 * plane-sweep multi-view stereo that feeds `to_ply(..., densify=True)`
 * (sfm_mvs_amd/mvs.py, docs/mvs.md).  Every step is a correctly rounded
 * float32 operation in the order written here (no FMA, no reassociation), so
 * an independent float32 restatement reproduces the outputs bit for bit.
 * Non-finite inputs (matrix entries, depths, field values) follow IEEE 754
 * through the same operations: a comparison with a NaN is false, so a NaN
 * depth is no depth and a NaN h_2 or p_2 no sample.  Where an output is a NaN,
 * its sign and payload are unspecified (IEEE 754 leaves them to the
 * implementation); the same holds for "MESH" below.
 *
 * sfm_mvs_plane_sweep — the depth map of one reference view.
 *   ref_dev    [h][w] uint8 reference gray frame; I' = (float)I - 128
 *   src_dev    host array of nsrc DEVICE pointers, [h][w] uint8 source gray frames (same size), 1 <= nsrc <= 8
 *   mv_host    host float32 [nsrc][12] = M (3x3 row-major) | v (3) per source, copied into the kernel arguments:
 *              pixel (x, y) of plane j maps to h_i = ((M_i0*x + M_i1*y) + M_i2) + v_i*invd[j]; valid iff h_2 > 0,
 *              0 <= px = h_0/h_2 <= w-1 and 0 <= py = h_1/h_2 <= h-1; x0 = min(floor(px), w-2), fx = px - x0 (same in y);
 *              val = (1-fy)*((1-fx)*I'00 + fx*I'01) + fy*((1-fx)*I'10 + fx*I'11)
 *   invd_dev   [ndepth] float32 inverse depths of the fronto-parallel planes (caller-owned, > 0), 2 <= ndepth <= 1024
 *   radius     1..4: the window is (2r+1)^2 pixels about (x, y), n = (float)(2r+1)^2; 2r+1 <= w, h <= 32767
 *   topk       1..nsrc: C_j = mean of the topk smallest per-source costs (ascending, summed left to right, / (float)topk)
 *   var_min    > 0: a source is invalid where var_r < var_min or var_w < var_min, or any window sample is invalid
 *   cost_max   depth = 0 where C_{j*} >= cost_max
 *   moments    row sums of 2r+1 terms left to right, then the row sums top to bottom: S_r, S_rr, S_w, S_ww, S_rw
 *   cost_s     1 - cov / sqrtf(var_r*var_w) clamped to [0, 2] with var = S_xx - (S_x*S_x)/n, cov = S_rw - (S_r*S_w)/n;
 *              2 for an invalid source, and for every source where the reference window leaves the frame
 *   j*         the first j of smallest C_j; if 0 < j* < ndepth-1, den = (C_{j*-1} + C_{j*+1}) - 2*C_{j*} and
 *              delta = den > 0 ? clamp(0.5*(C_{j*-1} - C_{j*+1})/den, -0.5, 0.5) : 0,
 *              invd* = invd[j*] + delta*(delta >= 0 ? invd[j*+1]-invd[j*] : invd[j*]-invd[j*-1]); else invd* = invd[j*]
 *   depth_dev  [h][w] float32 1/invd*, 0 where the reference window leaves the frame or C_{j*} >= cost_max
 *   cost_dev   [h][w] float32 C_{j*}
 *   plane_dev  optional [h][w] int32 j* (NULL: not written)
 *   volume_dev optional [ndepth][h][w] float32 C_j (NULL: not written; the volume never reaches HBM otherwise)
 * Whether the optional outputs are present changes no other output.  No workspace.
 *
 * sfm_mvs_consistency — geometric-consistency filter of one reference depth map and the world point of each kept pixel.
 *   depth_dev      [h][w] float32 reference depth map (0 = no depth)
 *   nbr_depth_dev  host array of nview DEVICE pointers to the neighbours' [h][w] depth maps, 0 <= nview <= 8
 *   nbr_index_host host int32 [nview] the neighbours' view indices; ref_index the reference's
 *   ab_host        host float32 [nview][12] = A (3x3) | b (3): p_i = d*((A_i0*x + A_i1*y) + A_i2) + b_i; neighbour v is consistent
 *                  iff p_2 > 0, its nearest pixel (floor(p_0/p_2 + 0.5), floor(p_1/p_2 + 0.5)) lies in the frame, the neighbour's
 *                  depth dv there is > 0 and |p_2 - dv| <= tau*dv
 *   bc_host        host float32 [12] = B (3x3) | c (3): xyz_i = d*((B_i0*x + B_i1*y) + B_i2) + c_i
 *   tau >= 0 (finite), 0 <= min_consistent <= nview, 1 <= w, h <= 32767
 *   unique         != 0: a pixel with a consistent neighbour of lower view index is dropped (the lowest-index consistent observer
 *                  emits a surface sample, once)
 *   mask_dev       [h][w] uint8 1 = kept (d > 0, count >= min_consistent, unique rule), else 0
 *   xyz_dev        [h][w][3] float32 world point, 0 where the mask is 0
 * Compaction: sfm_mask_indices over the masks.  No workspace.
 * ---------------------------------------------------------------------- */
int sfm_mvs_plane_sweep(const uint8_t* ref_dev, const uint8_t* const* src_dev, const float* mv_host, int nsrc, int64_t w, int64_t h,
                        const float* invd_dev, int ndepth, int radius, int topk, float var_min, float cost_max,
                        float* depth_dev, float* cost_dev, int32_t* plane_dev, float* volume_dev, void* stream);
int sfm_mvs_consistency(const float* depth_dev, const float* const* nbr_depth_dev, const int32_t* nbr_index_host,
                        const float* ab_host, int nview, int ref_index, const float* bc_host, int64_t w, int64_t h, float tau,
                        int min_consistent, int unique, uint8_t* mask_dev, float* xyz_dev, void* stream);

/* ------------------------------------------------------------------------
 * MVS-AGGREGATE  shiftable windows and semi-global aggregation of the sweep's cost volume (opt-in; no reference counterpart)
 *
 * Three entry points between sfm_mvs_plane_sweep (volume_dev) and sfm_mvs_consistency (sfm_mvs_amd/mvs.py `aggregate_depth`,
 * docs/mvs.md §7).  Only the quantisation and the final parabola touch floating point; everything between is integer
 * arithmetic, hence exact and independent of any summation order, so an integer restatement (tests/np_mvs_aggregate.py)
 * reproduces every output bit for bit.  Volumes are plane-major [ndepth][h][w], element (j, y, x) at (j*h + y)*w + x (64-bit).
 * Limits of all three, as the sweep's: 2 <= ndepth <= 1024, 1 <= w, h <= 32767.  No workspace, no atomics on global memory,
 * no host wait.
 *
 * sfm_mvs_cost_shift — quantise and take the best window that contains the pixel (a spatial min filter per plane).
 *   volume_dev [ndepth][h][w] float32 costs (the sweep's C_j in [0, 2]; any float is accepted)
 *   q(c)       = !(c < 2) ? 2048 : (c > 0 ? (uint16)floorf(c*1024.f + 0.5f) : 0), the product and the sum correctly rounded
 *                float32 operations: both comparisons are false for a NaN, so a NaN gives 2048; +inf gives 2048, every
 *                c <= 0 (-0, negatives, -inf) gives 0.  q is monotone and 0 <= q <= 2048.
 *   shift      0..4;  q_dev [ndepth][h][w] uint16:  Q(j, y, x) = min of q(volume(j, y+dy, x+dx)) over |dx|, |dy| <= shift with
 *              0 <= x+dx <= w-1 and 0 <= y+dy <= h-1 (the taps outside the frame are left out; shift 0 is q alone).
 *              Because q is monotone, filtering before or after quantising is the same function.
 *
 * sfm_mvs_cost_aggregate — Hirschmueller's path costs summed over ndir directions.
 *   q_dev, s_dev  [ndepth][h][w] uint16, distinct buffers;  integers 0 <= p1 <= p2 <= 2048;  ndir 4 or 8: the first ndir of
 *              (dx, dy) = (1,0), (-1,0), (0,1), (0,-1), (1,1), (-1,1), (1,-1), (-1,-1)
 *   L_r        for direction r = (dx, dy) the predecessor of p = (x, y) is p' = (x-dx, y-dy).  p' outside the frame:
 *              L_r(p, j) = Q(p, j).  Otherwise, with m = min_k L_r(p', k):
 *              L_r(p, j) = Q(p, j) + min(L_r(p', j), L_r(p', j-1) + p1, L_r(p', j+1) + p1, m + p2) - m
 *              (the j-1 term is absent for j = 0, the j+1 term for j = ndepth-1).
 *   S(p, j)    = sum over the ndir directions of L_r(p, j).
 *   Ranges: the min is >= m and <= m + p2, so Q <= L_r <= Q + p2 <= 2048 + 2048 = 4096, and S <= 8*4096 = 32768: uint16
 *   holds every value.  (A caller's own Q above 2048 is accepted: L_r is formed in 32 bits and S is the sum modulo 65536.)
 *
 * sfm_mvs_cost_depth — winner-take-all on S with the sweep's sub-plane parabola.
 *   j*         the first j of smallest S(p, j).  If 0 < j* < ndepth-1: a = (float)S(j*-1), b = (float)S(j*), c = (float)S(j*+1)
 *              (exact), den = (a + c) - 2*b, delta = den > 0 ? clamp(0.5*(a - c)/den, -0.5, 0.5) : 0,
 *              invd* = invd[j*] + delta*(delta >= 0 ? invd[j*+1]-invd[j*] : invd[j*]-invd[j*-1]); else invd* = invd[j*]
 *              (float32, each operation correctly rounded in the order written, no FMA — as sfm_mvs_plane_sweep)
 *   gate       integer 0..65535 (the wrapper passes q(cost_max))
 *   depth_dev  [h][w] float32 1/invd*, 0 where Q(p, j*) >= gate
 *   cost_dev   [h][w] float32 (float)Q(p, j*) / 1024
 *   plane_dev  optional [h][w] int32 j* (NULL: not written; changes no other output)
 * ---------------------------------------------------------------------- */
int sfm_mvs_cost_shift(const float* volume_dev, int64_t w, int64_t h, int ndepth, int shift, uint16_t* q_dev, void* stream);
int sfm_mvs_cost_aggregate(const uint16_t* q_dev, int64_t w, int64_t h, int ndepth, int p1, int p2, int ndir, uint16_t* s_dev,
                           void* stream);
int sfm_mvs_cost_depth(const uint16_t* s_dev, const uint16_t* q_dev, const float* invd_dev, int64_t w, int64_t h, int ndepth, int gate,
                       float* depth_dev, float* cost_dev, int32_t* plane_dev, void* stream);

/* ------------------------------------------------------------------------
 * MVS-PATCHMATCH  refinement of a depth map over slanted support planes (opt-in; no reference counterpart; csrc/mvs_patchmatch.hip)
 *
 * One entry point between sfm_mvs_plane_sweep (or sfm_mvs_cost_depth) and sfm_mvs_consistency (sfm_mvs_amd/mvs.py
 * `patchmatch_refine`, docs/mvs.md §9).  In the reference camera the inverse depth of a plane is affine in the pixel, so a slanted
 * matching window needs only a per-sample inverse depth; the warp of "MVS" is unchanged.  As in "MVS", every step is a correctly
 * rounded float32 operation in the order written here (no FMA, IEEE `/` and sqrtf), and tests/np_mvs_patchmatch.py restates every
 * output bit for bit.  Integer-to-float conversions below are exact ((float) of a small integer).
 *
 * sfm_mvs_patchmatch — enqueues 1 + 2*iters + 1 launches on the stream (init; per iteration a red then a black half-sweep; finish).
 *   ref_dev, src_dev, mv_host, nsrc, w, h, radius, topk, var_min, cost_max: as sfm_mvs_plane_sweep (r 1..4, nsrc 1..8, 2r+1 <= w, h <= 32767)
 *   qmin, qmax   0 < qmin <= qmax < inf: the admissible inverse depths of a plane at its pixel
 *   state_dev    [h][w][4] float32 (q0, a, b, cost) per pixel, 16-byte aligned, caller-owned; written by every launch, final on return
 *   plane        the plane (q0, a, b) of the pixel (x, y) has inverse depth q = (q0 + a*(float)(u-x)) + b*(float)(v-y) at sample (u, v)
 *   cost         C(x, y; q0, a, b): sfm_mvs_plane_sweep's C_j at (x, y) with invd[j] replaced, per window sample (u, v), by that q:
 *                h_i = ((M_i0*u + M_i1*v) + M_i2) + v_i*q, validity, bilinear value, the moments' order, var_min, the clamp to [0, 2],
 *                the top-k mean and the cost 2 where the reference window leaves the frame are all as written under "MVS".
 *                With a = b = 0 and q0 = invd[j] it is the sweep's volume word (q0 + 0 + 0 = q0).
 *   hash         U(pix, it, c): x = seed ^ (pix*0x9E3779B9u + it*0x85EBCA6Bu + c*0xC2B2AE35u) in wrapping uint32, pix = y*w + x;
 *                x ^= x>>16; x *= 0x7feb352du; x ^= x>>15; x *= 0x846ca68bu; x ^= x>>16;  U = (float)(int32_t)x * 0x1p-31f
 *                (the conversion rounds to nearest even; -1 <= U <= 1).  No state: a word of (seed, pixel, iteration, draw index).
 *   init         d = depth_init_dev[y][x] (depth_init_dev may be NULL: every pixel is hashed).  If d > 0 and qmin <= 1/d <= qmax:
 *                q0 = 1/d; else q0 = qmin + (qmax-qmin)*(0.5f*U(pix, 0, 0) + 0.5f).  a = b = 0, cost = C(x, y; q0, 0, 0).
 *                (A NaN, zero, negative or infinite d fails one of the comparisons.)
 *   half-sweep   iteration it = 0..iters-1, colour 0 (red: (x+y) even) then colour 1 (black: (x+y) odd).  Every pixel of the colour
 *                tries its candidates in this order; a candidate (q0', a', b') is evaluated only if it is admissible, and replaces
 *                the pixel's state (with cost = its C) only if its C is strictly smaller than the state's cost:
 *                1. for (dx, dy) = (-1,0), (1,0), (0,-1), (0,1), and if far != 0 then (-3,0), (3,0), (0,-3), (0,3): the neighbour
 *                   (xn, yn) = (x+dx, y+dy), skipped outside the frame, with state (qn, an, bn, .):
 *                   q0' = (qn + an*(float)(x-xn)) + bn*(float)(y-yn), a' = an, b' = bn
 *                2. with ds = depth_step*s, ss = slope_step*s, s = 2^-it (both products exact), U_c = U(pix, it, c), and (q0, a, b)
 *                   the state as it stands when the candidate is formed:
 *                   depth:  (q0*(1 + ds*U_1), a, b)
 *                   slopes: (q0, a + (ss*q0)*U_2, b + (ss*q0)*U_3)
 *                   both:   (q0*(1 + ds*U_4), a + (ss*q0)*U_5, b + (ss*q0)*U_6)
 *                admissible: q0', a', b' finite, qmin <= q0' <= qmax, (float)r*(fabsf(a') + fabsf(b')) <= 0.5f*q0'
 *                (so every sample's q is >= q0'/2 > 0).  Every neighbour has the other colour (odd Manhattan distance) and a
 *                half-sweep writes its own colour only: no word depends on the order of execution, and the update is in place.
 *   finish       depth_dev [h][w] float32 1/q0, 0 where the reference window leaves the frame or !(cost < cost_max);
 *                cost_dev [h][w] float32 the state's cost;
 *                normal_dev optional [h][w][3] float32 (NULL: not written, nmat_host not read): with A = a, B = b,
 *                C = (q0 - a*(float)x) - b*(float)y:  n_i = (N_i0*A + N_i1*B) + N_i2*C, divided by sqrtf((n_0*n_0 + n_1*n_1) + n_2*n_2);
 *                (0, 0, 0) where the depth is 0
 *   nmat_host    host float32 [9] N (3x3 row-major) = -R^T K^T of the reference camera, formed in float64 and cast once: the plane is
 *                (A, B, C).K X_c = 1 in camera coordinates, so N (A, B, C) is its world normal turned towards the camera
 *   iters 0..16 (0: init and finish only); depth_step, slope_step finite and >= 0; seed any uint32; far any int.
 * No workspace, no atomics, no host wait.
 * ---------------------------------------------------------------------- */
int sfm_mvs_patchmatch(const uint8_t* ref_dev, const uint8_t* const* src_dev, const float* mv_host, int nsrc, int64_t w, int64_t h,
                       float qmin, float qmax, int radius, int topk, float var_min, float cost_max, const float* depth_init_dev,
                       int iters, int far, float depth_step, float slope_step, uint32_t seed, const float* nmat_host,
                       float* state_dev, float* depth_dev, float* cost_dev, float* normal_dev, void* stream);

/* ------------------------------------------------------------------------
 * MVS-FUSE  merging fusion of the depth maps of all views: averaged oriented points, a normal check (opt-in; no reference
 *           counterpart; csrc/mvs_fuse.hip)
 *
 * One entry point in the place of the per-view sfm_mvs_consistency calls (sfm_mvs_amd/mvs.py `fuse`, `run_mvs(fuse=...)`,
 * docs/mvs.md §10).  Where the filter emits a kept pixel's own sample, this merges it with the samples of its consistent neighbours:
 * position, normal and colour averaged, and a neighbour whose normal disagrees is not consistent.  As in "MVS", every float step is a
 * correctly rounded float32 operation in the order written here (no FMA, IEEE `/` and sqrtf), neighbours strictly in table order, and
 * tests/np_mvs_fuse.py restates every output bit for bit.  All element offsets are 64-bit.
 *
 * sfm_mvs_fuse — one launch over all views: a workgroup per 16 x 16 tile and view, a lane per pixel.
 *   depth_dev   [n][h][w] float32 depth maps of all views, stacked (0 = no depth)
 *   normal_dev  [n][h][w][3] float32 world normals, or NULL (then normal_out_dev must be NULL too)
 *   bgr_dev     [n][h][w][3] uint8 frames, or NULL (then bgr_out_dev must be NULL too)
 *   table_dev   DEVICE array of n records of 512 bytes (128 32-bit words), view i at byte 512*i, holding view indices only, never an
 *               address:
 *                 word 0          int32   nnbr             the kernel uses min(nnbr, 8); <= 0: no neighbour
 *                 word 1          int32   min_consistent
 *                 words 2..9      int32   nbr[8]           the neighbours' view indices in the caller's order; an index outside
 *                                                          0..n-1 or equal to i is skipped (so a corrupt table reads nothing out of range)
 *                 words 10..21    float32 bc[12]           B (3x3 row-major) | c (3) of view i itself, as sfm_mvs_consistency's bc_host
 *                 words 22..117   float32 ab[8][12]        A (3x3 row-major) | b (3) per neighbour slot, as sfm_mvs_consistency's ab_host
 *                 words 118..127  unused (padding; not read)
 *   1 <= n <= 4096, 1 <= w, h <= 32767, tau finite and >= 0, cos_min not NaN (-inf and +inf are accepted)
 *   Per pixel (x, y) of view i, with d = depth[i][y][x], n = normal[i][y][x] (three words) and the record R_i:
 *     projection  for slot s = 0 .. min(nnbr, 8)-1 with v = nbr[s] (not skipped) and a = ab[s]:
 *                 p_k = d*((a_k0*x + a_k1*y) + a_k2) + b_k as sfm_mvs_consistency; the slot is consistent iff d > 0, p_2 > 0,
 *                 (u, t) = (floor(p_0/p_2 + 0.5), floor(p_1/p_2 + 0.5)) lies in the frame (0 <= u <= w-1, 0 <= t <= h-1),
 *                 dv = depth[v][t][u] > 0, |p_2 - dv| <= tau*dv, and, when normal_dev is given, with m = normal[v][t][u]:
 *                 (n_0*m_0 + n_1*m_1) + n_2*m_2 >= cos_min (false for a NaN; cos_min = -inf passes every non-NaN product)
 *     counting    count = the consistent slots (a view listed twice counts twice); lower = one of them has v < i
 *     keep        d > 0 && count >= min_consistent && !(unique && lower): sfm_mvs_consistency's rule; k = 1 + count
 *     position    X_k = d*((B_k0*x + B_k1*y) + B_k2) + c_k from R_i.bc (sfm_mvs_consistency's xyz word); then, for every consistent
 *                 slot in order, X_k = X_k + (dv*((B'_k0*u + B'_k1*t) + B'_k2) + c'_k) with B' | c' = R_v.bc (the neighbour's own sample
 *                 at its own pixel); xyz_k = X_k / (float)k
 *     normal      N = n; N_k = N_k + m_k for every consistent slot in order; len = sqrtf((N_0*N_0 + N_1*N_1) + N_2*N_2);
 *                 normal_out_k = len > 0 ? N_k / len : n_k  (a zero or NaN length gives the pixel's own normal back)
 *     colour      per channel S = the byte of the pixel + the bytes of the consistent slots' pixels (u, t) (integers);
 *                 bgr_out = (2*S + k) / (2*k) in integer division: the mean rounded half up, exact and order-free
 *   mask_dev        [n][h][w] uint8 1 = kept, else 0
 *   xyz_dev         [n][h][w][3] float32
 *   normal_out_dev  [n][h][w][3] float32, written iff normal_dev is given
 *   bgr_out_dev     [n][h][w][3] uint8, written iff bgr_dev is given
 *   support_dev     [n][h][w] uint8 k
 *   Every output is 0 where the mask is 0.  Whether an optional input is present changes no other output (normal_dev = NULL
 *   gives the mask and positions of cos_min = -inf, unless a NaN normal fails the product).  Two identities: with normal_dev = NULL (or
 *   cos_min = -inf and no NaN normal) the mask of view i is sfm_mvs_consistency's for its neighbour list; where support is 1, xyz
 *   is sfm_mvs_consistency's xyz word for word (one term, and x / 1.0f = x).
 * No workspace beyond the table, no atomics, no host wait; a second run gives the same bits.
 * ---------------------------------------------------------------------- */
int sfm_mvs_fuse(const float* depth_dev, const float* normal_dev, const uint8_t* bgr_dev, const void* table_dev, int n, int64_t w,
                 int64_t h, float tau, float cos_min, int unique, uint8_t* mask_dev, float* xyz_dev, float* normal_out_dev,
                 uint8_t* bgr_out_dev, uint8_t* support_dev, void* stream);

/* ------------------------------------------------------------------------
 * MESH a surface from the MVS depth maps     after sfm.py:298 (`densify`)
 *
 * Volumetric fusion of depth maps into a truncated signed distance field (TSDF) and its zero set by marching tetrahedra
 * (sfm_mvs_amd/mesh.py, docs/mesh.md).  As in "MVS", every step is a correctly rounded float32 operation in the order written
 * here (no FMA, no reassociation), so an independent float32 restatement reproduces the outputs bit for bit.
 *
 * Grid: nx, ny, nz >= 2 lattice points per axis, nx*ny*nz <= 2^27; point (i, j, k) has linear index (k*ny + j)*nx + i and sits
 * at x = ox + (float)i*voxel, y = oy + (float)j*voxel, z = oz + (float)k*voxel (origin_host float32 [3] = ox, oy, oz; voxel > 0).
 *
 * sfm_tsdf_integrate — folds nview views into the running sums of every lattice point.  No workspace, no atomics.
 *   depth_dev  [nview][h][w] float32 camera depth, 0 = no depth; 1 <= w, h <= 32767, nview >= 0
 *   mask_dev   optional [nview][h][w] uint8: a pixel is used only where it is nonzero (NULL: every pixel)
 *   bgr_dev    optional [nview][h][w][3] uint8 B, G, R (NULL: no colour; then CWc_dev must be NULL too)
 *   P_dev      [nview][12] float32 = K[R|t] row-major (formed in float64 by the caller, cast once)
 *   trunc      > 0 (finite)
 *   per view v in ascending order:  p_r = ((P_r0*x + P_r1*y) + P_r2*z) + P_r3;  the sample is valid iff p_2 > 0, the nearest
 *              pixel (u, t) = (floor(p_0/p_2 + 0.5), floor(p_1/p_2 + 0.5)) lies in the frame (0 <= u <= w-1, 0 <= t <= h-1 tested
 *              in float), d = depth[v][t][u] > 0 and the mask there (if given) is nonzero;  sdf = d - p_2;  no contribution if
 *              sdf < -trunc;  otherwise f = min(sdf, trunc) / trunc, S = S + f, W = W + 1, and where also sdf <= trunc:
 *              C_b = C_b + (float)B, C_g = C_g + (float)G, C_r = C_r + (float)R, Wc = Wc + 1
 *   S_dev, W_dev  [nz][ny][nx] float32, read and written back once per call (the caller zeroes them before the first call)
 *   CWc_dev    optional [nz][ny][nx][4] float32 (C_b, C_g, C_r, Wc), likewise
 *   Sums run left to right in view order from the values read, so integrating views in two consecutive calls is bit-identical
 *   to one call over all of them.
 *
 * sfm_mesh_count / sfm_mesh_extract — marching tetrahedra over a finished field.
 *   w_min      >= 1 (finite): point p is known iff W >= w_min; its value F = S/W, it is inside iff F < 0
 *   cube (i, j, k), i < nx-1, j < ny-1, k < nz-1, is split into the 6 Kuhn tetrahedra {000, e1, e1+e2, 111}, the permutations
 *              (e1, e2, e3) in the order xyz, xzy, yxz, yzx, zxy, zyx; corners are numbered 0..3 in that order; a tetrahedron with
 *              an unknown corner emits nothing
 *   edges      every tetrahedron edge joins a lattice point a to a + one of the 7 directions, numbered 0..6: +x, +y, +z, +x+y, +x+z,
 *              +y+z, +x+y+z; it belongs to a (its lower end).  Edge (a, dir) with b = a + dir in the grid crosses iff a and b are
 *              both known and exactly one of them is inside.
 *   vertices   one per crossing edge; its id is the exclusive count of crossing edges before it in (linear index of a, dir) order.
 *              t = Fa / (Fa - Fb); position xa + t*(xb - xa) per coordinate (xa, xb by the lattice formula above); colour
 *              ca + t*(cb - ca) per channel (B, G, R), c = C/Wc per channel, or 0 where Wc = 0
 *   triangles  per tetrahedron with every corner known: one inside or one outside corner c -> 1 triangle over the 3 crossing
 *              edges (c, o) in ascending order of the other corner o; two of each -> 2 triangles splitting the quad on the diagonal
 *              from edge (in0, out0) to edge (in1, out1) (in0 < in1, out0 < out1 in corner order): (in0,out0) (in0,out1) (in1,out1)
 *              and (in0,out0) (in1,out1) (in1,out0).  A triangle whose right-hand normal would point from outside to inside has
 *              its last two vertices swapped.  Order: cube linear index, tetrahedron, triangle.
 *   The case table is generated from these rules at compile time (csrc/mesh.hip); consistent splitting across neighbouring
 *   cubes makes the surface watertight wherever the field is known.  Counts are int32: 7*2^27 edges and 12*2^27 triangles fit.
 *
 *   sfm_mesh_count     counts_dev int32[2] = (vertices, triangles), written on the stream (the caller reads them to size the
 *                      outputs).  Workspace: sfm_mesh_count_ws_bytes.
 *   sfm_mesh_extract   vertices_dev [max_vertices][3] float32, optional colors_dev [max_vertices][3] float32 B G R (needs CWc_dev),
 *                      faces_dev [max_faces][3] int32 vertex ids.  Writes exactly the counted elements; nothing past max_vertices /
 *                      max_faces is written (the caller passes the counts).  Workspace: sfm_mesh_extract_ws_bytes (5 bytes per
 *                      lattice point and a little).  Deterministic: two passes with an int32 scan, no atomics.
 * The _ws_bytes twins return 0 for an invalid grid.
 * ---------------------------------------------------------------------- */
int sfm_tsdf_integrate(const float* depth_dev, const uint8_t* mask_dev, const uint8_t* bgr_dev, const float* P_dev, int nview, int64_t w,
                       int64_t h, const float* origin_host, float voxel, int64_t nx, int64_t ny, int64_t nz, float trunc, float* S_dev,
                       float* W_dev, float* CWc_dev, void* stream);
size_t sfm_mesh_count_ws_bytes(int64_t nx, int64_t ny, int64_t nz);
int sfm_mesh_count(const float* S_dev, const float* W_dev, int64_t nx, int64_t ny, int64_t nz, float w_min, int32_t* counts_dev,
                   void* ws_dev, size_t ws_bytes, void* stream);
size_t sfm_mesh_extract_ws_bytes(int64_t nx, int64_t ny, int64_t nz);
int sfm_mesh_extract(const float* S_dev, const float* W_dev, const float* CWc_dev, const float* origin_host, float voxel, int64_t nx,
                     int64_t ny, int64_t nz, float w_min, int64_t max_vertices, int64_t max_faces, float* vertices_dev, float* colors_dev,
                     int32_t* faces_dev, void* ws_dev, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * MESH-CLEAN (no reference counterpart; csrc/mesh_clean.hip, docs/mesh.md §7): connected components of a triangle mesh and the
 * removal of the small ones, after sfm_mesh_extract.  Everything is int32 arithmetic or a bit-for-bit copy; no result depends
 * on a summation or arrival order; tests/np_mesh_clean.py restates every output exactly.
 *
 *   input       vertices_dev [nv][3] float32, optional colors_dev [nv][3] float32, faces_dev [nf][3] int32; 0 <= nv, nf <= 2^31 - 1
 *   valid face  its three indices lie in 0..nv-1.  An invalid face joins nothing and is never output, and no index outside that
 *               range is dereferenced.  Repeated indices within a face ((a,a,b), (a,a,a)) and duplicate faces are valid and count.
 *   components  two vertices are connected when a valid face names both; label[v] = the smallest vertex id of v's component.  A
 *               vertex in no valid face is its own component with 0 faces.  faces_of[c] = the valid faces whose vertices carry
 *               label c.
 *   keep rule   integers min_faces >= 0 and largest_only (0 or 1).  Without largest_only, component c is kept iff
 *               faces_of[c] >= min_faces.  With it, only the component with the most faces is kept (ties: the lowest label), and
 *               only if it passes min_faces too.  min_faces = 0, largest_only = 0 keeps everything, face-less vertices included.
 *   output      kept vertices in their original order, the new id = the rank among the kept vertices; position and colour rows
 *               copied bit for bit (NaN payloads survive); the valid faces of kept components in their original order, remapped
 *               to the new ids; counts_dev int32[4] = (vertices kept, faces kept, components, components kept).  The outputs are
 *               buffers of the input sizes, distinct from the inputs; nothing is written at or past the counted rows.
 *
 * sfm_mesh_components — labels by min-label hooking and pointer jumping, at most `rounds` (1..1024) rounds, all enqueued at once.
 *   labels_dev  [nv] int32.  resume == 0: started from label[v] = v.  resume != 0: continued from the labels given, which must be
 *               a state an earlier call over the same faces left.
 *   a round     per valid face m = min(label[a], label[b], label[c]); the three labels and the labels of the three current labels
 *               are lowered to m (atomic min); per vertex label[v] is lowered to where label[label[..]] leads within 4 hops.
 *               A round that lowers nothing ends the work: the launches of the later rounds return at once.
 *   status_dev  int32[2] = (converged 0/1, rounds that lowered a label).  Converged labels are the component minima whatever
 *               order the atomics landed in.  Unconverged labels are a valid intermediate state: every label is an id of the
 *               vertex's own component and >= its minimum; call again with resume != 0.
 * sfm_mesh_clean — labels_dev must be converged labels of these faces (otherwise the outputs are unspecified, though every write
 *   stays inside the counted rows).  colors_dev and out_colors_dev are both given or both NULL.
 * Errors (SFM_ERR_ARG, before any device call): negative counts or counts above 2^31 - 1, rounds outside 1..1024, negative
 *   min_faces, largest_only not 0 or 1, NULL where the count is non-zero (status_dev, counts_dev and the workspace always),
 *   colours in without colours out or the reverse, a workspace smaller than the _ws_bytes twin says.
 * The _ws_bytes twins return 0 for invalid sizes.
 * ---------------------------------------------------------------------- */
size_t sfm_mesh_components_ws_bytes(int64_t nv, int64_t nf);
int sfm_mesh_components(const int32_t* faces_dev, int64_t nv, int64_t nf, int rounds, int resume, int32_t* labels_dev, int32_t* status_dev,
                        void* ws_dev, size_t ws_bytes, void* stream);
size_t sfm_mesh_clean_ws_bytes(int64_t nv, int64_t nf);
int sfm_mesh_clean(const float* vertices_dev, const float* colors_dev, const int32_t* faces_dev, int64_t nv, int64_t nf,
                   const int32_t* labels_dev, int64_t min_faces, int largest_only, float* out_vertices_dev, float* out_colors_dev,
                   int32_t* out_faces_dev, int32_t* counts_dev, void* ws_dev, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * MESH-FINISH (no reference counterpart; csrc/mesh_finish.hip, docs/mesh.md §8): vertex normals and Taubin smoothing of a triangle
 * mesh, after sfm_mesh_extract or sfm_mesh_clean.  Every sum over faces is an int64 sum of quantised terms, so no result depends
 * on the order in which atomics land or on whether an implementation scatters or gathers; every float32 and float64 operation is
 * correctly rounded in the order written here (no FMA, no reassociation); int64 -> float64 rounds to nearest even.
 * tests/np_mesh_finish.py restates both outputs bit for bit.
 *
 *   input       vertices_dev [nv_cap][3] float32, faces_dev [nf_cap][3] int32; 0 <= nv_cap, nf_cap <= 2^31 - 1
 *   counts_dev  optional int32[2] = (nv, nf), READ ON THE DEVICE (the first two words of sfm_mesh_clean's counts are this pair, so
 *               the call follows it on the stream with no host wait).  NULL: nv = nv_cap, nf = nf_cap.  A count that is negative
 *               or above its capacity is taken as the capacity.
 *   valid face  one of the first nf faces whose three indices lie in 0..nv-1.  Anything else contributes nothing, and no index
 *               outside that range is dereferenced.  Repeated indices and duplicate faces follow the formulas, no special case.
 *   output      [nv_cap][3] float32, distinct from the input; rows at or past nv are never written.
 *
 * sfm_mesh_normals — normals_dev.  Per valid face (i0, i1, i2) with positions a, b, c:
 *     e1 = b - a, e2 = c - a per coordinate;
 *     n_x = e1_y*e2_z - e1_z*e2_y,  n_y = e1_z*e2_x - e1_x*e2_z,  n_z = e1_x*e2_y - e1_y*e2_x  (the right-hand normal: outward by
 *     the winding sfm_mesh_extract guarantees);  len = sqrtf((n_x*n_x + n_y*n_y) + n_z*n_z);
 *     the face contributes iff len is finite and > 0:  u_c = n_c / len,  q_c = (int64) rintf(u_c * 2^30);  q is added to the
 *     accumulator of each of its three corners, once per corner (a repeated index adds twice).
 *   Per vertex: d_c = (double) acc_c;  L = sqrt((d_x*d_x + d_y*d_y) + d_z*d_z);  normal_c = (float)(d_c / L), or (0, 0, 0) when
 *   L == 0.  This is the equal-weight sum of unit face normals (open3d's compute_vertex_normals), normalised.
 *
 * sfm_mesh_smooth — out_vertices_dev after nsteps (0..64) steps; factors_host float32 [nsteps] (finite), origin_host float32 [3]
 *   = o (finite), pscale > 0 (finite; the wrapper passes a power of two).  Step s maps positions p to p':
 *     r_c = rintf((p_c - o_c) * pscale);  a vertex is USABLE iff all three |r_c| <= 2^30 (NaN fails);
 *     for every valid face and each of its corners k, each of the OTHER two corners j that is usable adds (int64) r(j) to acc[i_k]
 *     and 1 to cnt[i_k] (int64);
 *     a vertex moves iff it is usable and cnt > 0:  m_c = ((double)acc_c / (double)cnt) / (double)pscale + (double)o_c,
 *     p'_c = (float)((double)p_c + (double)factor[s] * (m_c - (double)p_c));  every other vertex keeps its row bit for bit
 *     (NaN payloads included).
 *   This is the face-umbrella Laplacian: an edge shared by two faces counts twice, a boundary edge once.  Taubin smoothing is the
 *   factor sequence lambda, mu, lambda, mu, ... with lambda > 0 > mu.  nsteps = 0 copies the counted rows.  The steps ping-pong
 *   through the workspace; the last one lands in the output.
 * Errors (SFM_ERR_ARG, before any device call): a capacity negative or above 2^31 - 1, NULL where a capacity is non-zero (vertices,
 *   the output and the workspace with nv_cap; faces with nf_cap; origin_host always; factors_host with nsteps), the output equal to
 *   the input pointer, a workspace smaller than the _ws_bytes twin says; sfm_mesh_smooth also nsteps outside 0..64, a factor or an
 *   origin coordinate that is not finite, pscale not finite or not positive.
 * The _ws_bytes twins return 0 for invalid sizes (32 bytes per vertex; smoothing 24 more).
 * ---------------------------------------------------------------------- */
size_t sfm_mesh_normals_ws_bytes(int64_t nv_cap, int64_t nf_cap);
int sfm_mesh_normals(const float* vertices_dev, const int32_t* faces_dev, int64_t nv_cap, int64_t nf_cap, const int32_t* counts_dev,
                     float* normals_dev, void* ws_dev, size_t ws_bytes, void* stream);
size_t sfm_mesh_smooth_ws_bytes(int64_t nv_cap, int64_t nf_cap);
int sfm_mesh_smooth(const float* vertices_dev, const int32_t* faces_dev, int64_t nv_cap, int64_t nf_cap, const int32_t* counts_dev, int nsteps,
                    const float* factors_host, const float* origin_host, float pscale, float* out_vertices_dev, void* ws_dev,
                    size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * MESH-DECIMATE (no reference counterpart; csrc/mesh_decimate.hip, docs/mesh.md §9): simplification of a triangle mesh by vertex
 * clustering, after sfm_mesh_extract, sfm_mesh_clean or sfm_mesh_smooth: the vertices of one cell of a regular grid become one
 * vertex at their mean, the faces are renumbered, and the faces that lose a corner go.  This is open3d's
 * simplify_vertex_clustering with average contraction and its rotation-normalised triangle set, made order-exact: every sum is an
 * int64 sum of quantised terms and every choice is a minimum, so no result depends on the order in which atomics land; every float32
 * and float64 operation is correctly rounded in the order written here (no FMA, no reassociation); int64 -> float64 rounds to
 * nearest even.  tests/np_mesh_decimate.py restates every output bit for bit.
 *
 *   input       vertices_dev [nv_cap][3] float32, optional colors_dev [nv_cap][3] float32, faces_dev [nf_cap][3] int32;
 *               0 <= nv_cap, nf_cap <= 2^31 - 1
 *   counts_dev  optional int32[2] = (nv, nf), READ ON THE DEVICE, exactly as in MESH-FINISH (the first two words of sfm_mesh_clean's
 *               counts are this pair).  NULL: the capacities.  A count that is negative or above its capacity is taken as the capacity.
 *   frame       origin_host float32 [3] = o (finite), cell > 0 (finite), dims_host int32 [3] = (dims_x, dims_y, dims_z), each >= 1,
 *               dims_x * dims_y * dims_z <= 2^27; pscale > 0 (finite; the wrapper passes MESH-FINISH's power of two).
 *   cell of a vertex   per coordinate t_c = floor(((double)p_c - (double)o_c) / (double)cell).  The vertex is USABLE iff for all
 *               three c:  t_c >= 0 && t_c < dims_c, tested in float64 before any conversion to an integer (NaN and +-inf fail), and
 *               r_c = rintf((p_c - o_c) * pscale) has |r_c| <= 2^30 (MESH-FINISH's quantisation; NaN fails).
 *               key = (t_z * dims_y + t_y) * dims_x + t_x  (< 2^27).
 *   leader      leader(key) = the smallest usable vertex id of the cell among the first nv.
 *   new vertices   the leaders in ascending id order; the new id of a leader is its rank among the leaders, and the new id of every
 *               usable vertex is that of its cell's leader.  With acc_c = the int64 sum of r_c over the usable members of the cell
 *               and cnt = their number:  p'_c = (float)(((double)acc_c / (double)cnt) / (double)pscale + (double)o_c).
 *               Colours, when given: per component the term of a member is (int64) rintf(c * 65536.0f) if fabsf(c) <= 32768.0f (NaN
 *               fails), else 0; the member counts in cnt either way;  c' = (float)(((double)acc / (double)cnt) / 65536.0).
 *               (|r| <= 2^30, terms <= 2^31, at most 2^31 members: every sum stays below 2^63.)
 *   faces       of the first nf, a face is VALID iff its three indices lie in 0..nv-1 (no other index is dereferenced), and a valid
 *               face is LIVE iff its three corners are usable and their three new ids are pairwise different.  The live faces are
 *               output in their input order as (a', b', c') in the input corner order: winding is kept.
 *   dedupe == 1 two live faces are EQUAL iff their new triples are equal after rotating each so that its smallest id comes first (a
 *               face and its flipped twin are not equal).  Of equal faces only the one with the lowest input index is output.
 *               dedupe == 0 outputs every live face.
 *   output      out_vertices_dev, out_colors_dev (iff colors_dev), out_faces_dev: buffers of the input capacities, distinct from
 *               the inputs; nothing is written at or past the counted rows.  out_counts_dev int32[4] = (vertices out, faces out,
 *               unusable vertices among the first nv, live faces dropped as duplicates); its first two words are what
 *               sfm_mesh_normals reads as counts_dev, so normals follow on the stream with no host wait.
 * Errors (SFM_ERR_ARG, before any device call): a capacity negative or above 2^31 - 1; a dim < 1 or a product above 2^27; cell or
 *   pscale not finite or not positive; an origin coordinate that is not finite; dedupe not 0 or 1; NULL where a capacity is non-zero
 *   (vertices in and out with nv_cap, faces in and out with nf_cap; origin_host, dims_host, out_counts_dev and the workspace
 *   always); colours in without colours out or the reverse; an output pointer equal to an input pointer; a workspace smaller than
 *   the _ws_bytes twin says.
 * The _ws_bytes twin returns 0 for invalid sizes (76 bytes per vertex, 4 per cell, 1 per face and 4 per slot of the face set: the
 *   smallest power of two >= 2 * nf_cap).
 * ---------------------------------------------------------------------- */
size_t sfm_mesh_decimate_ws_bytes(int64_t nv_cap, int64_t nf_cap, const int32_t dims[3]);
int sfm_mesh_decimate(const float* vertices_dev, const float* colors_dev, const int32_t* faces_dev, int64_t nv_cap, int64_t nf_cap,
                      const int32_t* counts_dev, const float* origin_host, float cell, const int32_t* dims_host, float pscale, int dedupe,
                      float* out_vertices_dev, float* out_colors_dev, int32_t* out_faces_dev, int32_t* out_counts_dev, void* ws_dev,
                      size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * MESH-TEXTURE (no reference counterpart; csrc/mesh_texture.hip, docs/mesh.md §10): a texture map for a triangle mesh from the
 * photographs it was built from, after sfm_mesh_extract, sfm_mesh_clean, sfm_mesh_smooth or sfm_mesh_decimate: a depth map of the
 * mesh in every view (the occlusion test), the view each face is textured from, and an atlas in which every face owns half of a
 * square cell.  Every result is a minimum or a pure function of its inputs, so nothing depends on the order in which atomics land;
 * everything is float32 and every operation is correctly rounded in the order written here (no FMA, no reassociation; IEEE `/`,
 * rintf = to nearest even, floorf, ceilf).  tests/np_mesh_texture.py restates the three outputs bit for bit.
 *
 *   input       vertices_dev [nv_cap][3] float32, faces_dev [nf_cap][3] int32; 0 <= nv_cap, nf_cap <= 2^31 - 1
 *   counts_dev  optional int32[2] = (nv, nf), READ ON THE DEVICE, exactly as in MESH-FINISH and MESH-DECIMATE.  NULL: the
 *               capacities.  A count that is negative or above its capacity is taken as the capacity.
 *   valid face  one of the first nf faces whose three indices lie in 0..nv-1; no other index is dereferenced.
 *   views       P_dev [n][12] float32, row-major 3 x 4 (mesh.projection_rows), 1 <= n <= 65536; frames of w x h pixels,
 *               w, h >= 2, w * h <= 2^26.
 *   projection  of a point (x, y, z) in view v, with P = P_dev[v]:  p_r = ((P_r0*x + P_r1*y) + P_r2*z) + P_r3 for r = 0, 1, 2;
 *               sx = p_0 / p_2,  sy = p_1 / p_2,  depth = p_2.  The point is PROJECTABLE iff p_2 > 0 and sx, sy and p_2 are finite.
 *               Pixel (x, y) has its centre at (x, y).
 *   edge function   E_ab(x, y) = (bx - ax)*(y - ay) - (by - ay)*(x - ax) over screen points a, b;  area2 = E_ab(cx, cy).
 *
 * sfm_mesh_render_depth — zbuf_dev [n][h][w] float32, written with +inf by the same call and then, for every view and every valid
 *   face whose three corners a, b, c are projectable and whose area2 is < 0 or > 0 (both orientations: back faces occlude too):
 *     x runs over max(0, ceilf(min(ax, bx, cx))) .. min(w - 1, floorf(max(ax, bx, cx))), y likewise, the bounds compared as floats
 *     before any conversion to an integer;
 *     wa = E_bc(x, y), wb = E_ca(x, y), wc = E_ab(x, y) with (float) x, (float) y;  the pixel is COVERED iff all three are >= 0
 *     (area2 > 0) or all three are <= 0 (area2 < 0): a pixel centre on an edge belongs to both faces of the edge;
 *     iz = ((wa*(1/depth_a) + wb*(1/depth_b)) + wc*(1/depth_c)) / area2,  d = 1/iz;
 *     if d is finite and > 0:  zbuf[v][y][x] = min(zbuf[v][y][x], d), an unsigned 32-bit atomic minimum on the bits (positive floats
 *     order as their bits).
 *   A face with a corner that is not projectable is skipped in that view.  THERE IS NO NEAR-PLANE CLIPPING: the cameras stand
 *   outside the surface, and a face that crosses a camera's plane z = 0 does not occlude in that camera.  Any triangle is handled,
 *   one that covers the whole frame included; no loop exceeds w * h steps.  No workspace: the corners are projected per face.
 *
 * sfm_mesh_face_views — face_view_dev int32 [nf_cap], face_score_dev float32 [nf_cap]; zbuf_dev as sfm_mesh_render_depth left it;
 *   vis_tol >= 0 (finite).  A valid face is a CANDIDATE of view v iff
 *     its three corners are projectable and lie in 0 <= sx <= w - 1, 0 <= sy <= h - 1;
 *     area2 < 0 (sfm_mesh_extract winds faces with the normal toward the cameras; with x right, y down, z forward that is a
 *     negative screen area);
 *     it is VISIBLE: each of four samples, the three corners and the centroid g_c = ((a_c + b_c) + c_c) / 3.0f of the positions
 *     (projected like a vertex), is projectable, its nearest pixel (rintf(sx), rintf(sy)) lies in the frame (compared as floats)
 *     and depth <= zbuf[v][py][px] * (1.0f + vis_tol).  An empty pixel holds +inf and passes.
 *   score = -area2.  face_view = the candidate view of the largest score, the lowest index among equal scores; -1 and score 0 when
 *   there is none or the face is not valid.  Rows at or past nf are never written.  No atomics.
 *
 * sfm_mesh_texture_fill — atlas_dev [side][side][3] uint8 B G R.  The layout is a function of (nf_cap, texels) alone, texels = L the
 *   texels per triangle leg, 1 <= L <= 64:  cell side c = L + 5;  cols = the smallest integer >= 1 with cols^2 >= ceil(nf_cap / 2);
 *   side = cols * c <= 16384.  Face f owns half `f & 1` of cell q = f >> 1 whose origin is ((q % cols)*c, (q / cols)*c); in the
 *   cell's texel coordinates (i, j), half 0 owns i + j <= c - 1 and half 1 the rest.  Corners a, b, c of the face sit at
 *     half 0:  (1, 1), (1 + L, 1), (1, 1 + L)        half 1:  (c - 2, c - 2), (c - 2 - L, c - 2), (c - 2, c - 2 - L)
 *   so that a chart keeps at least one texel to the diagonal and to the cell's border; those texels are filled by the same
 *   formula, extrapolated, which dilates the chart against bleeding under bilinear lookups.  Per texel, row-major:
 *     half 0:  u = (float)(i - 1) / (float)L,  v = (float)(j - 1) / (float)L;   half 1:  u = (float)(c - 2 - i) / (float)L,
 *     v = (float)(c - 2 - j) / (float)L;   w0 = (1.0f - u) - v;   X_c = (w0*A_c + u*B_c) + v*C_c per coordinate;
 *     if k = face_view_dev[f] lies in 0..n-1: X is projected by P_k (projectable or not) and frame k, frames_dev [n][h][w][3] uint8,
 *     is sampled:  sx clamped to [0, w - 1] and sy to [0, h - 1] (NaN -> 0);  x0 = min((int)floorf(sx), w - 2),  fx = sx - (float)x0,
 *     y0, fy likewise;  value = ((p00*(1 - fx) + p10*fx)*(1 - fy)) + ((p01*(1 - fx) + p11*fx)*fy) per channel, p10 = pixel (x0 + 1, y0);
 *     otherwise, with colors_dev [nv_cap][3] float32 given, value = (w0*Ca + u*Cb) + v*Cc per channel, and without it 0;
 *     texel = (uint8) min(max(rintf(value), 0), 255)  (NaN -> 0).
 *   Texels of faces at or past nf, of cells past the last face and of faces that are not valid are 0.
 * Errors (SFM_ERR_ARG, before any device call): a capacity negative or above 2^31 - 1; n outside 1..65536; w or h < 2 or
 *   w * h > 2^26; vis_tol negative or not finite; texels outside 1..64, a layout whose side exceeds 16384, cols or side that
 *   disagree with the layout; NULL where required (vertices with nv_cap, faces, face_view_dev and face_score_dev with nf_cap; P_dev,
 *   zbuf_dev, frames_dev and atlas_dev always).  None of the three takes a workspace.
 * ---------------------------------------------------------------------- */
int sfm_mesh_render_depth(const float* vertices_dev, const int32_t* faces_dev, int64_t nv_cap, int64_t nf_cap, const int32_t* counts_dev,
                          const float* P_dev, int n, int64_t w, int64_t h, float* zbuf_dev, void* stream);
int sfm_mesh_face_views(const float* vertices_dev, const int32_t* faces_dev, int64_t nv_cap, int64_t nf_cap, const int32_t* counts_dev,
                        const float* P_dev, int n, int64_t w, int64_t h, const float* zbuf_dev, float vis_tol, int32_t* face_view_dev,
                        float* face_score_dev, void* stream);
int sfm_mesh_texture_fill(const float* vertices_dev, const float* colors_dev, const int32_t* faces_dev, int64_t nv_cap, int64_t nf_cap,
                          const int32_t* counts_dev, const float* P_dev, const uint8_t* frames_dev, int n, int64_t w, int64_t h,
                          const int32_t* face_view_dev, int texels, int cols, int side, uint8_t* atlas_dev, void* stream);

/* ------------------------------------------------------------------------
 * Measurement hook (no reference counterpart): when enabled, the library brackets
 * its dominant kernels with hipEvents recorded on the launch stream.
 * sfm_profile_read synchronises those events, returns the summed device time
 * and launch count of one slot, and resets the slot (toggling the switch does not).
 *   slot 0 knn filter (MFMA)   1 knn refine (+ rescans)   2 triangulate
 *        3 dense BA sweep       4 indexed residual sweep    5 Schur products (W^T x, W v)
 *        6 SIFT scale space (all blur + decimate launches of one image = 1 "launch")   7 SIFT descriptors
 * sfm_profile_enable(n) with n > 1: as 1, and the knn filter kernel is launched n times back-to-back
 * inside one event pair (idempotent), so the few microseconds an event pair adds to a single short
 * launch are amortised; sfm_profile_read then reports n launches per bracket.
 * ---------------------------------------------------------------------- */
int sfm_profile_enable(int on);

/* ------------------------------------------------------------------------
 * TRACKS (no reference counterpart: isfm.py:56-94 matches and verifies every pair and ends there; csrc/tracks.hip, docs/tracks.md):
 * feature tracks, scene points followed through all the images that see them, from the match store of all pairs, and their
 * N-view triangulation.  Every integer output below is a minimum, a count, a rank or a copy of its inputs: no word depends on
 * the order in which atomics land.  Every float64 operation of the triangulation is correctly rounded in the order written here
 * (no FMA, no reassociation, IEEE / and sqrt).  tests/np_tracks.py restates every output exactly.
 *
 *   node        img_off[image] + keypoint.  img_off_dev int32 [n_img + 1], img_off[0] = 0, non-decreasing (an image may be empty),
 *               N = img_off[n_img] = n_nodes <= 2^31 - 1;  1 <= n_img <= 65 536.  The image of node u is the largest i < n_img with
 *               img_off[i] <= u, found by binary search (at most 17 steps).
 *
 * sfm_match_edges — the match store as edges, with no compaction and no host wait: one item per (pair p, slot q < cap).
 *   store_dev   int32 [n_pairs][2][cap][2] as sharded.match_pairs_sharded leaves it: [p][0][q] = the two trainIdx, [p][1][q] = the
 *               bits of the two float32 distances (d0, d1).  pair_img_dev int32 [n_pairs][2], nq_dev int32 [n_pairs]: on the device.
 *   survivor    q < nq[p], both images of the pair in 0..n_img-1, q below the size of the first and trainIdx0 in 0..size-1 of the
 *               second, a second neighbour (trainIdx1 >= 0), (double)d0 < ratio * (double)d1 (the rule of sfm_ratio_compact), and,
 *               when keep_dev (uint8 [n_pairs][cap], optional) is given, keep[p][q] != 0.
 *   edges_dev   int32 [n_pairs * cap][2]: a survivor writes (img_off[pair[p][0]] + q, img_off[pair[p][1]] + trainIdx0) at p * cap + q,
 *               every other slot (-1, -1).  n_pairs * cap <= 2^31 - 1.
 *
 * sfm_track_components — label[u] = the smallest node id of u's component over the VALID edges; the contract of sfm_mesh_components.
 *   valid edge  both ends lie in 0..N-1 and differ.  An invalid edge joins nothing and is never dereferenced; duplicates are harmless.
 *   a round     per valid edge m = min(label[a], label[b]): the end with the larger label and that label's own entry are lowered
 *               to m (a read first, an atomic min only when it can lower); per node label[u] is lowered to where
 *               label[label[..]] leads within 4 hops.  `rounds` (1..1024) launches are enqueued with no host wait; a round that
 *               lowers nothing ends the work: the later launches return at once.
 *   labels_dev  [N] int32.  resume == 0: started from label[u] = u; otherwise continued from a state an earlier call left.
 *   status_dev  int32[2] = (converged 0/1, rounds that lowered a label).  Unconverged labels are a valid state to resume from:
 *               every label is a node of the node's own component, >= its minimum and <= the node.
 *
 * sfm_track_build — labels_dev must be converged (otherwise the outputs are unspecified, though every write stays in bounds).
 *   candidate   a component with >= 2 nodes.  conflicting: two of its nodes lie in one image (decided per (label, image) by an
 *               open-addressing set that holds the smallest node of each pair).  kept: a candidate that is not conflicting with
 *               min_len <= size <= max_len (2 <= min_len <= max_len <= 2^31 - 1).
 *   tracks      the kept components in ascending label order are tracks 0..T-1.
 *   node_track_dev int32 [N]: the node's track or -1.   track_off_dev int32 [N / 2 + 2], of which T + 1 words are written.
 *   obs_node_dev   int32 [N], of which nobs = track_off[T] are written: a track's nodes in ascending id, hence ascending image.
 *   counts_dev  int32[6] = (T, nobs, candidates, conflicting, longest kept, nodes in components of one node).  The first two
 *               words are what sfm_track_triangulate reads on the device.  Nothing at or past the counted rows is written.
 *
 * sfm_track_triangulate — one lane per track t < counts[0] (a count outside 0..N/2+1, or nobs outside 0..N, is taken as that
 *   capacity; offsets are clamped to 0 <= lo <= hi <= nobs).  kp_dev float32 [N][2], all images concatenated; P_dev float64
 *   [n_img][12], row-major 3 x 4.  In observation order, with (x, y) = the keypoint promoted to float64 and P the image's matrix:
 *     r0[k] = x * P[8 + k] - P[k],  r1[k] = y * P[8 + k] - P[4 + k]   (k = 0..3: the rows of the rows = 4 DLT, not normalised)
 *     M[a][b] = (M[a][b] + r0[a] * r0[b]) + r1[a] * r1[b]             for a <= b, from M = 0; then M[b][a] = M[a][b]
 *   (an observation whose node lies outside 0..N-1 adds nothing).  Eigenvectors by cyclic Jacobi on the 4 x 4, V = I:
 *     sweeps      at most 30; a sweep visits the pivots (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); the sweep in which no pivot rotates
 *                 is the last.
 *     a pivot     (p, q), apq = M[p][q], app = M[p][p], aqq = M[q][q], is SKIPPED when apq == 0 or
 *                 |apq| <= 2^-52 * sqrt(|app| * |aqq|).  Otherwise
 *                   theta = (aqq - app) / (2 * apq);  root = sqrt(theta * theta + 1)
 *                   t = theta >= 0 ? 1 / (theta + root) : -1 / (root - theta);  c = 1 / sqrt(t * t + 1);  s = t * c
 *                   for k not in {p, q}:  M[k][p] = M[p][k] = c * akp - s * akq;  M[k][q] = M[q][k] = s * akp + c * akq
 *                                         (akp, akq = the old M[k][p], M[k][q])
 *                   M[p][p] = app - t * apq;  M[q][q] = aqq + t * apq;  M[p][q] = M[q][p] = 0
 *                   for k = 0..3:         V[k][p] = c * vkp - s * vkq;  V[k][q] = s * vkp + c * vkq
 *     the vector  v = column j of V, j = the index of the smallest M[j][j] (ties: the lowest j).
 *   X_dev       float32 [N / 2 + 1][3]: X[c] = (float)(v[c] / v[3]).
 *   err_dev, depth_dev  float32 [N] per observation, with (Xd, Yd, Zd) = X promoted to float64 and P its image's matrix:
 *                 h_r = ((P[4r] * Xd + P[4r + 1] * Yd) + P[4r + 2] * Zd) + P[4r + 3];   depth = (float)h_2
 *                 du = h_0 / h_2 - x;  dv = h_1 / h_2 - y;  err = (float)sqrt(du * du + dv * dv)
 *               (both NaN for a node outside 0..N-1).
 *   flags_dev   int32 [N / 2 + 1]: bit 0 = every depth of the track is finite and > 0; bit 1 = v[3] != 0 and X is finite.
 *   max_err_dev float32 [N / 2 + 1]: from m = 0, in observation order, m = err when err > m or err is NaN (a NaN stays).
 *   Every float32 NaN that is written is the quiet NaN 0x7FC00000.
 *
 * Errors (SFM_ERR_ARG, before any device call): negative counts or counts above 2^31 - 1, n_pairs * cap above 2^31 - 1, n_img
 *   outside 1..65 536, a NaN ratio, rounds outside 1..1024, min_len / max_len outside 2 <= min_len <= max_len <= 2^31 - 1, NULL where
 *   the count is non-zero (img_off_dev, status_dev, counts_dev, track_off_dev, P_dev, X_dev, flags_dev, max_err_dev and the
 *   workspaces always), a workspace smaller than the _ws_bytes twin says.  The _ws_bytes twins return 0 for invalid sizes.
 * ---------------------------------------------------------------------- */
int sfm_match_edges(const int32_t* store_dev, int64_t n_pairs, int64_t cap, const int32_t* pair_img_dev, const int32_t* nq_dev,
                    const int32_t* img_off_dev, int n_img, double ratio, const uint8_t* keep_dev, int32_t* edges_dev, void* stream);
size_t sfm_track_components_ws_bytes(int64_t n_nodes, int64_t ne);
int sfm_track_components(const int32_t* edges_dev, int64_t n_nodes, int64_t ne, int rounds, int resume, int32_t* labels_dev,
                         int32_t* status_dev, void* ws_dev, size_t ws_bytes, void* stream);
size_t sfm_track_build_ws_bytes(int64_t n_nodes);
int sfm_track_build(const int32_t* labels_dev, const int32_t* img_off_dev, int64_t n_nodes, int n_img, int64_t min_len, int64_t max_len,
                    int32_t* node_track_dev, int32_t* track_off_dev, int32_t* obs_node_dev, int32_t* counts_dev, void* ws_dev,
                    size_t ws_bytes, void* stream);
int sfm_track_triangulate(const int32_t* counts_dev, const int32_t* track_off_dev, const int32_t* obs_node_dev, const int32_t* img_off_dev,
                          int n_img, const float* kp_dev, const double* P_dev, int64_t n_nodes, float* X_dev, float* err_dev,
                          float* depth_dev, int32_t* flags_dev, float* max_err_dev, void* stream);

/* ------------------------------------------------------------------------
 * TRACKS-REFINE (no reference counterpart; csrc/tracks_refine.hip, docs/tracks.md §8): robust refinement of the N-view points and
 * pruning of single observations.  counts_dev, track_off_dev, obs_node_dev, img_off_dev, kp_dev, P_dev and n_nodes are
 * sfm_track_triangulate's and are read and clamped as it clamps them (T to 0..N/2+1, nobs to 0..N, 0 <= lo <= hi <= nobs).  Every
 * float64 operation is correctly rounded in the order written here (no FMA, no reassociation, IEEE / and sqrt); every integer output
 * is a count, a rank or a copy: no word depends on the order in which atomics land (there are none).  tests/np_tracks_refine.py
 * restates every output word from this text.  The ranges [lo, hi) of the tracks must not OVERLAP (sfm_track_build's and
 * sfm_track_prune's never do): where they do, as with a count above the true one over offsets nobody wrote, the outputs of both
 * calls are unspecified, but every read and write stays inside the arrays: the state a lane keeps in a row of depth_dev is checked
 * against n_img and N each time it is read, and sfm_track_prune writes no observation at or past row N.
 *
 * sfm_track_refine — one lane per track t < counts[0].  X_in_dev float32 [N / 2 + 1][3] and flags_in_dev int32 [N / 2 + 1] are
 *   sfm_track_triangulate's outputs (not aliased by the outputs here).  huber > 0 px or +inf (plain least squares); obs_thresh > 0
 *   px; iters, iters2 in 0..50.  ws_dev holds the camera centres, filled by a kernel of the same call: with p = an image's P,
 *     a00 = p5 * p10 - p6 * p9;   a01 = p2 * p9 - p1 * p10;   a02 = p1 * p6 - p2 * p5
 *     a10 = p6 * p8 - p4 * p10;   a11 = p0 * p10 - p2 * p8;   a12 = p2 * p4 - p0 * p6
 *     a20 = p4 * p9 - p5 * p8;    a21 = p1 * p8 - p0 * p9;    a22 = p0 * p5 - p1 * p4
 *     det = (p0 * a00 + p1 * a10) + p2 * a20;    C[r] = -(((a_r0 * p3 + a_r1 * p7) + a_r2 * p11) / det)        (r = 0..2)
 *   At a point q = (q0, q1, q2), for an observation with keypoint (kx, ky) promoted to float64 and P its image's matrix:
 *     h_r = ((P[4r] * q0 + P[4r + 1] * q1) + P[4r + 2] * q2) + P[4r + 3];   u = h_0 / h_2;  v = h_1 / h_2
 *     du = u - kx;  dv = v - ky;  e = sqrt(du * du + dv * dv)
 *   start      x = X_in[t] promoted to float64.  If bit 1 of flags_in[t] is clear or a coordinate of x is not finite the track is
 *              NOT STARTED: X_out[t] = X_in[t], no observation is an inlier, flags = n_inl = steps = 0, max_err = 0, cos_min = 1,
 *              err and depth as below at X_in[t].
 *   usable     an observation whose node lies in 0..N-1 and for which, at the start point, h_2 is finite and > 0 and e is finite.
 *              The set is fixed; an observation outside it takes no part in anything and is no inlier.
 *   an attempt (the loop of both phases; `active` = the usable observations in phase 1, the inliers in phase 2; lam = 1e-3 at the
 *              start of a phase; cost = the sum of rho(e) over the active observations at x, in observation order from 0):
 *                w = 1 when e <= huber, else huber / e                                 (phase 2: w = 1)
 *                ja[k] = (P[k] - u * P[8 + k]) / h_2;  jb[k] = (P[4 + k] - v * P[8 + k]) / h_2              (k = 0..2)
 *                A[a][b] = (A[a][b] + w * (ja[a] * ja[b])) + w * (jb[a] * jb[b])       (a <= b)
 *                g[a]    = (g[a] + w * (ja[a] * du)) + w * (jb[a] * dv)                (over the active observations in order, from 0)
 *                s00 = A00 + lam * A00;  s11 = A11 + lam * A11;  s22 = A22 + lam * A22
 *                c00 = s11 * s22 - A12 * A12;  c01 = A02 * A12 - A01 * s22;  c02 = A01 * A12 - A02 * s11
 *                c11 = s00 * s22 - A02 * A02;  c12 = A01 * A02 - s00 * A12;  c22 = s00 * s11 - A01 * A01
 *                det = (s00 * c00 + A01 * c01) + A02 * c02
 *                d0 = -(((c00 * g0 + c01 * g1) + c02 * g2) / det);  d1 = -(((c01 * g0 + c11 * g1) + c12 * g2) / det)
 *                d2 = -(((c02 * g0 + c12 * g1) + c22 * g2) / det);  trial point x + d
 *              ACCEPTED iff det != 0, d is finite, every active observation has a finite h_2 > 0 at the trial point, and the
 *              trial cost (same sum, at the trial point) is < cost.  Accepted: x = x + d, cost = trial cost, lam = lam / 10,
 *              steps + 1; rejected: lam = lam * 10.  There is no stopping rule: a phase makes all its attempts.
 *   phase 1    iters attempts with rho(e) = e * e / 2 when e <= huber, else huber * (e - huber / 2).
 *   inliers    the usable observations with e <= obs_thresh at the end of phase 1; n_inl of them.  The set is fixed from here on.
 *   phase 2    only when n_inl >= 2: iters2 attempts with rho(e) = e * e / 2.
 *   X_out_dev  float32 [N / 2 + 1][3] = (float)x.  The outputs below are taken at Xf = X_out[t] promoted to float64:
 *   err_dev, depth_dev  float32 [N]: err = (float)e, depth = (float)h_2 at Xf for a node in 0..N-1, both NaN otherwise (the
 *              formulas of sfm_track_triangulate).  Between its passes the call keeps one int32 per observation in the rows of
 *              depth_dev that it overwrites at the end.
 *   inlier_dev uint8 [N]: 1 for an inlier, else 0.     n_inl_dev int32 [N / 2 + 1].     steps_dev int32 [N / 2 + 1]: accepted
 *              attempts of both phases.
 *   max_err_dev float32 [N / 2 + 1]: from m = 0 over the INLIERS in observation order, m = err when err > m or err is NaN.
 *   cos_min_dev float32 [N / 2 + 1]: rays r_i = Xf - C[image] (component by component) of the first 64 inliers in observation
 *              order; n_i = (r_i0 * r_i0 + r_i1 * r_i1) + r_i2 * r_i2; from m = 1, over the pairs i < j (i outer, j inner)
 *              c = ((r_i0 * r_j0 + r_i1 * r_j1) + r_i2 * r_j2) / sqrt(n_i * n_j), m = c when c < m (a NaN never is);
 *              cos_min = (float)m: 1 with fewer than two inliers.  There is no acos on the device: callers compare cosines.
 *   flags_dev  int32 [N / 2 + 1]: bit 0 = n_inl >= 2; bit 1 = X_out[t] is finite (0 for a track that is not started).
 *   Every float32 NaN that is written is the quiet NaN 0x7FC00000.  Rows at or past counts[0] / counts[1] are not written.
 *
 * sfm_track_prune — keeps track t iff flags[t] == 3 and n_inl[t] >= min_len (>= 2) and (double)max_err[t] <= max_reproj (+inf
 *   switches it off; a NaN max_err fails) and (double)cos_min[t] <= max_cos (1 switches it off).  X_dev, inlier_dev, n_inl_dev,
 *   max_err_dev, cos_min_dev, flags_dev: sfm_track_refine's outputs.  Kept tracks in ascending old order are tracks 0..T'-1 and hold
 *   their observations with inlier != 0 in the old order; ranks come from per-block counts and a one-workgroup scan, no host wait.
 *   track_off2_dev int32 [N / 2 + 2] (T' + 1 words written), obs_node2_dev int32 [N] (nobs'), X2_dev float32 [N / 2 + 1][3] (the
 *   words of X), track_src_dev int32 [N / 2 + 1] (the old index): T' rows each.  counts2_dev int32[4] = (T', nobs', tracks dropped,
 *   observations dropped from kept tracks).  Nothing at or past the counted rows is written.  (counts2, track_off2, obs_node2) have
 *   the shape sfm_track_build leaves: sfm_track_triangulate and sfm_track_refine run on them again.
 *
 * Errors (SFM_ERR_ARG, before any device call): n_nodes outside 0..2^31-1, n_img outside 1..65 536, huber or obs_thresh NaN or <= 0,
 *   iters or iters2 outside 0..50, min_len outside 2..2^31-1, a NaN max_reproj or max_cos, NULL where the count is non-zero (the
 *   per-track arrays, counts, P, img_off and the workspaces always), a workspace smaller than the _ws_bytes twin says.  The _ws_bytes
 *   twins return 0 for invalid sizes.
 * ---------------------------------------------------------------------- */
size_t sfm_track_refine_ws_bytes(int n_img);
int sfm_track_refine(const int32_t* counts_dev, const int32_t* track_off_dev, const int32_t* obs_node_dev, const int32_t* img_off_dev,
                     int n_img, const float* kp_dev, const double* P_dev, int64_t n_nodes, const float* X_in_dev, const int32_t* flags_in_dev,
                     double huber, double obs_thresh, int iters, int iters2, float* X_out_dev, uint8_t* inlier_dev, float* err_dev,
                     float* depth_dev, int32_t* n_inl_dev, float* max_err_dev, float* cos_min_dev, int32_t* steps_dev, int32_t* flags_dev,
                     void* ws_dev, size_t ws_bytes, void* stream);
size_t sfm_track_prune_ws_bytes(int64_t n_nodes);
int sfm_track_prune(const int32_t* counts_dev, const int32_t* track_off_dev, const int32_t* obs_node_dev, int64_t n_nodes, const float* X_dev,
                    const uint8_t* inlier_dev, const int32_t* n_inl_dev, const float* max_err_dev, const float* cos_min_dev,
                    const int32_t* flags_dev, int64_t min_len, double max_reproj, double max_cos, int32_t* track_off2_dev,
                    int32_t* obs_node2_dev, float* X2_dev, int32_t* track_src_dev, int32_t* counts2_dev, void* ws_dev, size_t ws_bytes,
                    void* stream);

/* ------------------------------------------------------------------------
 * TRACKS-BA (no reference counterpart; csrc/tracks_ba.hip, docs/tracks.md §9): bundle adjustment of the tracks, a fixed-order sparse
 * Schur Levenberg-Marquardt with a Huber loss.  It stands beside sfm_project_residual / sfm_ba_schur_indexed (fp64 atomics, float32
 * points, no loss) and changes nothing of theirs.
 *
 * Problem layout (every entry point): cams_dev float64 [ncam][6] (rvec, tvec), K_host float64 [9], X_dev FLOAT64 [npt][3], obs_dev
 *   float32 [nobs][2];  1 <= ncam < 2^24, 1 <= npt <= 2^31-1, 0 <= nobs <= 2^31-1.
 *   point side   track_off_dev int32 [npt + 1], cam_idx_dev, pt_idx_dev int32 [nobs]: point-major as tracks.run_tracks returns them,
 *                observation o belongs to track pt_idx[o] and track_off is its CSR.
 *   camera side  cam_off_dev int32 [ncam + 1], cam_obs_dev int32 [nobs]: the stable counting sort of the observations by camera,
 *                observation indices ascending inside a camera.
 *   No index is trusted.  An observation whose cam_idx is outside 0..ncam-1 or whose pt_idx is outside 0..npt-1 is inactive; a CSR
 *   row is clamped to 0 <= lo <= hi <= nobs; an entry of cam_obs outside 0..nobs-1, or naming an observation whose cam_idx is not the
 *   row's camera, adds nothing.  The camera rows are cut into chunks of 256 entries, granted in camera order while fewer than
 *   nobs / 256 + ncam are in use (rows that overlap can ask for more; consistent rows never do): a camera reads the entries of the
 *   chunks it was granted.  Every read and write stays inside the arrays, whatever the CSRs hold.
 *
 * The workspace belongs to ONE linearisation: sfm_track_ba_sweep leaves the rows in it, sfm_track_ba_product and sfm_track_ba_step
 *   read them.  A trial sweep therefore takes a second workspace (track_ba.py keeps two and swaps them on acceptance).  The rows
 *   start at the first 256-byte aligned address of ws_dev: float64 [nobs][20].
 *
 * sfm_track_ba_sweep — linearisation at (cams, X).
 *   projection  as sfm_project_residual: X' = R(rvec) X + t, u = fx X'/Z' + cx, v = fy Y'/Z' + cy, r = (u, v) - obs in float64.
 *   active set  mode 0: observation o is active iff its indices are in range, Z' is finite and > 0 and r is finite; active_dev uint8
 *               [nobs] is WRITTEN.  mode 1 (a trial point): active_dev is READ and stays; an active observation (indices in range)
 *               whose Z' is not finite and > 0 or whose r is not finite counts in `crossed` and contributes nothing.  The caller
 *               refuses a trial with crossed > 0 (the rule of sfm_track_refine: no step may put a point behind a camera that sees it).
 *   loss        e = |r|;  w = 1 when e <= huber, else huber / e;  rho = e * e when e <= huber, else 2 * huber * e - huber * huber
 *               (continuous at e = huber; huber = +inf: plain least squares).
 *   rows        per observation 20 doubles: sqrt(w) Jc (d(u,v)/d(rvec,tvec), 2 x 6: the u row, then the v row), sqrt(w) Jp (d(u,v)/dX,
 *               2 x 3), sqrt(w) r (2).  Rows of observations that do not contribute are all zero.
 *   blocks      JtJ_pt_dev [npt][9] = C_j = sum Jp^T w Jp, Jtr_pt_dev [npt][3] = sum Jp^T w r, JtJ_cam_dev [ncam][36] = B_i = sum
 *               Jc^T w Jc, Jtr_cam_dev [ncam][6] = sum Jc^T w r (symmetric blocks written in full).  A point or camera without
 *               contributing observations gets zeros.
 *   stat_dev    float64 [2] = (sum of rho, sum of e * e) over the contributing observations.
 *   count_dev   int32 [3] = (contributing observations, crossed, contributing observations with e > huber).
 *
 * Summation order — the contract.  Every sum is a fixed function of the CSRs and of the data; none depends on the grid, on the waves
 *   in flight or on the order in which workgroups finish.  THERE ARE NO FLOATING-POINT ATOMICS in csrc/tracks_ba.hip.
 *   point side   G = 8 lanes per track (SFM_TBA_GROUP): lane l adds observations lo + l, lo + l + G, ... in ascending order, the G
 *                partial sums meet in a xor tree (strides G / 2 .. 1).
 *   camera side  a camera's list is cut into chunks of 256 observations; one workgroup sums a chunk (a lane per observation, a xor
 *                tree over each wave of 64, strides 32 .. 1, then the four waves in ascending order); a fold kernel adds the chunk
 *                sums of a camera in ascending order.
 *   cost, counts the same workgroup tree over 256 consecutive observations, then one workgroup of 1024 lanes: lane l adds the block
 *                sums l, l + 1024, ... ascending, then a tree (strides 512 .. 1).
 *   Appending tracks and cameras after a problem (not observing its points) leaves the blocks of its rows bit for bit.  The values
 *   are held to 1e-10 of the largest entry against tests/np_track_ba.py, not to the bit (a * b + c may be fused).
 *
 * sfm_track_ba_product — over the rows a sweep left in ws_dev (the weights are in them):
 *   mode 0: out [npt][3] = W^T in, u_j = sum_o Jp_o^T (Jc_o in[cam_idx[o]]);  mode 1: out [ncam][6] = W in, w_i = sum_o Jc_o^T (Jp_o
 *   in[pt_idx[o]]).  The summation orders of the sweep's point and camera side.
 *
 * sfm_track_ba_step — one damped step, the sparse twin of sfm_ba_schur_solve: Bd = B with its diagonal times (1 + lam), Cd likewise;
 *   S dc = g_c - W Cd^-1 g_p with S = Bd - W Cd^-1 W^T by block-Jacobi (Bd^-1) preconditioned conjugate gradients over the two
 *   products; dp = Cd^-1 (g_p - W^T dc).  The update is parameters - step.  fix_first_camera: camera 0 does not move.  Every vector
 *   operation of the camera side runs in one workgroup with fixed-order sums, the scalars stay on the device.
 *   host waits   one per look at r.r, taken before iterations 0, 5, 10, ... while iterations remain (stop: r.r <= cg_tol^2 rhs.rhs):
 *                it / 5 + 1 when the bound stops it after `it` iterations, (cg_iters + 4) / 5 when cg_iters runs out, 1 for
 *                cg_iters = 0.  The status comes with the first look.  dc_dev [ncam][6] and dp_dev [npt][3] are complete in stream
 *                order, not at return.  track_ba.bundle_adjust_tracks adds ONE wait per attempt, its read of stat and count.
 *   status_host  bit 0: a singular camera block (a zero or non-finite pivot; its preconditioner block is the identity); bit 1: a
 *                singular point block (|det| outside 1e-300..1e300, as for a point whose observations are all inactive): its inverse
 *                is the zero block, so its dp is 0, not NaN, and it adds nothing to S.   iters_host: the iterations run.
 *
 * Errors (SFM_ERR_ARG / SFM_ERR_WORKSPACE, before any device call): sizes outside the limits above, mode outside 0..1, huber NaN or
 *   <= 0, lam, cg_tol or cg_iters negative, NULL where the count is non-zero (the CSR offsets, cams, K, X, the blocks, stat, count,
 *   in, out, dc, dp and the workspace always), a workspace smaller than sfm_track_ba_ws_bytes says (0 for invalid sizes; 160 bytes
 *   per observation for the rows, 216 per chunk, the step's vectors).
 * ---------------------------------------------------------------------- */
size_t sfm_track_ba_ws_bytes(int64_t ncam, int64_t npt, int64_t nobs);
int sfm_track_ba_sweep(const double* cams_dev, int64_t ncam, const double* K_host, const double* X_dev, int64_t npt, const float* obs_dev,
                       const int32_t* track_off_dev, const int32_t* cam_idx_dev, const int32_t* pt_idx_dev, const int32_t* cam_off_dev,
                       const int32_t* cam_obs_dev, int64_t nobs, double huber, int mode, uint8_t* active_dev, double* JtJ_cam_dev,
                       double* Jtr_cam_dev, double* JtJ_pt_dev, double* Jtr_pt_dev, double* stat_dev, int32_t* count_dev, void* ws_dev,
                       size_t ws_bytes, void* stream);
int sfm_track_ba_product(int64_t ncam, int64_t npt, const int32_t* track_off_dev, const int32_t* cam_idx_dev, const int32_t* pt_idx_dev,
                         const int32_t* cam_off_dev, const int32_t* cam_obs_dev, int64_t nobs, int mode, const double* in_dev, double* out_dev,
                         void* ws_dev, size_t ws_bytes, void* stream);
int sfm_track_ba_step(int64_t ncam, int64_t npt, const int32_t* track_off_dev, const int32_t* cam_idx_dev, const int32_t* pt_idx_dev,
                      const int32_t* cam_off_dev, const int32_t* cam_obs_dev, int64_t nobs, const double* JtJ_cam_dev, const double* Jtr_cam_dev,
                      const double* JtJ_pt_dev, const double* Jtr_pt_dev, double lam, int fix_first_camera, double cg_tol, int cg_iters,
                      double* dc_dev, double* dp_dev, int32_t* iters_host, int32_t* status_host, void* ws_dev, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * TRACKS-CAL (no reference counterpart; csrc/tracks_cal.hip, docs/tracks.md §15): TRACKS-BA with one set of intrinsics shared by all
 * images among the unknowns, and the undistortion that goes with the model.  Opt-in: nothing of TRACKS-BA changes.
 *
 * Camera model.  theta = (f, cx, cy, k1, k2), float64, shared by all images; a fixed aspect a = K[1][1] / K[0][0] from the caller's K,
 *   no skew.  With X' = R(rvec) X + t, x = X'/Z', y = Y'/Z', r2 = x*x + y*y, d = 1 + k1*r2 + k2*r2*r2:
 *       u = f*d*x + cx        v = a*f*d*y + cy
 *   (products from the left: (f*d)*x, ((a*f)*d)*y; d = (1 + k1*r2) + (k2*r2)*r2).  With k1 = k2 = 0 this is the projection of
 *   sfm_track_ba_sweep term for term (fy = a*f).  A bit mask `free` (bit i frees theta[i]: 1 f, 2 cx, 4 cy, 8 k1, 16 k2) chooses
 *   what moves; it acts in sfm_track_cal_step only.
 *
 * The problem layout, the CSRs, the "no index is trusted" rules, the chunks, the active-set rules (mode 0 writes active_dev, mode 1
 *   reads it and counts `crossed`), the Huber weight and cost, stat_dev and count_dev are those of TRACKS-BA.  The workspace again
 *   belongs to ONE linearisation; the rows start at its first 256-byte aligned address: float64 [nobs][30], 240 bytes each.
 *
 * sfm_track_cal_sweep — linearisation at (cams, theta_host - dtheta_dev, X).  theta_host float64 [5] is checked on the host;
 *   dtheta_dev float64 [5] (may be NULL: zero) is a step that is still on the device, subtracted by every lane, so that a trial
 *   sweep needs no host wait for the step of theta.  Where the difference has f <= 0 or a non-finite entry no observation passes
 *   the active test (mode 0: none is active; mode 1: every active one counts in `crossed`).
 *   rows     per observation 30 doubles, each times sqrt(w): Jc (d(u,v)/d(rvec,tvec), 2 x 6: the u row, then the v row), Ji
 *            (d(u,v)/d theta, 2 x 5: u row (d*x, 1, 0, f*x*r2, f*x*r2*r2), v row (a*d*y, 0, 1, a*f*y*r2, a*f*y*r2*r2)), Jp (d(u,v)/dX,
 *            2 x 3), r (2).  Rows of observations that do not contribute are all zero.
 *   blocks   JtJ_cam_dev [ncam][36], Jtr_cam_dev [ncam][6], JtJ_pt_dev [npt][9], Jtr_pt_dev [npt][3] as TRACKS-BA.
 *   border   E_dev [ncam][30] = E_i = sum Jc^T Ji (6 x 5, row-major);  G_dev [25] = sum Ji^T Ji, written in full;  Jtr_theta_dev [5]
 *            = g_i = sum Ji^T r;  F_dev [npt][15] = F_j = sum Jp^T Ji (3 x 5, row-major).  The columns of parameters that are not
 *            free are computed all the same.
 *
 * Summation order — the contract.  THERE ARE NO FLOATING-POINT ATOMICS in csrc/tracks_cal.hip.
 *   point side (C_j, g_p, F_j, out of product mode 0) and camera side (B_i, g_c, E_i, out of product mode 1): as TRACKS-BA; a chunk's
 *                27 values grow by the 30 of E_i.
 *   G, g_i, out_theta and the cost: a workgroup tree over 256 consecutive observations, then one workgroup of 1024 lanes folding the
 *                block sums (lane l the blocks l, l + 1024, ... ascending, then a tree).
 *   A second run gives the same bits.  Appending cameras and tracks that do not observe a problem's points leaves the problem's
 *   per-camera and per-point blocks (B_i, g_c, E_i, C_j, g_p, F_j) and its rows bit for bit.  The values are held to 1e-10 of the
 *   largest entry against tests/np_track_cal.py.
 *
 * sfm_track_cal_product — over the rows a sweep left in ws_dev:
 *   mode 0: (in [ncam][6], in_theta [5]) -> out [npt][3] = sum_o Jp^T (Jc in[cam_idx[o]] + Ji in_theta)   (out_theta unused)
 *   mode 1: in [npt][3] -> out [ncam][6] = sum_o Jc^T (Jp in[pt_idx[o]]) and out_theta [5] = sum_o Ji^T (Jp in[pt_idx[o]])
 *   (in_theta unused; out_theta sums the observations whose two indices are in range).
 *
 * sfm_track_cal_step — one damped step on the bordered system.  Unknowns y = (dc, di), 6 ncam + 5 entries;
 *   S = [Bd E; E^T Gd] - [W; F^T] Cd^-1 [W^T F], the diagonals of B, G and C times (1 + lam) (Marquardt: the step does not depend on
 *   the very different scales of f and k1);  S y = (g_c, g_i) - [W; F^T] Cd^-1 g_p by conjugate gradients preconditioned with
 *   blockdiag(Bd^-1, Gd^-1), the recurrence and the single-workgroup vector kernels of sfm_track_ba_step, with two guards: alpha = 0
 *   unless p.Sp > 0 and beta = 0 unless r.z > 0 (with a handful of unknowns, one free parameter and a fixed camera say, the residual
 *   reaches exactly 0 between two looks of the host; the iterations that remain are then no-ops instead of 0 / 0);
 *   dp = Cd^-1 (g_p - W^T dc - F di).  The update is parameters - step.
 *   free         a parameter that is not free has its row and column of the system replaced by the identity and a zero right-hand
 *                side: its entry of dtheta_dev is exactly 0.  Gd^-1 is the inverse of Gd so restricted.
 *   fix_first_camera, iters_host, the host waits (one per look at r.r before iterations 0, 5, 10, ...) as sfm_track_ba_step.
 *   status_host  bits 0 and 1 as sfm_track_ba_step; bit 2: Gd restricted to the free set is singular (a zero or non-finite pivot;
 *                its preconditioner block is the identity).
 *
 * sfm_undistort_points — px_dev float32 [n][2] pixels of the distorted image -> out_dev float32 [n][2] pixels of the ideal pinhole
 *   image with K_out_host (float64 [9]; fx', fy', cx', cy' are read).  In float64, without contraction, in this order:
 *   xd = (u - cx) / f, yd = (v - cy) / (a*f), rd = sqrt(xd*xd + yd*yd); r = rd, then TEN times, without a data-dependent exit,
 *   r2 = r*r, g = r*(1 + r2*(k1 + k2*r2)) - rd, h = 1 + r2*(3*k1 + 5*k2*r2), r = r - g/h;  s = r/rd (1 when rd = 0);
 *   out = float32(fx'*(xd*s) + cx', fy'*(yd*s) + cy').  A non-finite input or result gives NaN in both coordinates.  0 <= n <= 2^31-1.
 *
 * sfm_undistort_image — src_dev uint8 [nimg][H][W][C], C in {1, 3} -> dst_dev of the same shape (another buffer) and, when
 *   mask_dev is not NULL, uint8 [nimg][H][W] of 0 / 1: one BATCHED call, no host wait.  Every output pixel (xo, yo) is mapped forward
 *   in float64: x = (xo - cx')/fx', y = (yo - cy')/fy', r2, d as above, su = float32(f*d*x + cx), sv = float32(a*f*d*y + cy).
 *   It is valid iff 0 <= su <= W-1 and 0 <= sv <= H-1, i.e. iff none of the four taps x0 = floor(su), x0 + 1, y0 = floor(sv), y0 + 1
 *   that carry weight is outside (a tap past the last column or row has weight exactly 0 and is read at W-1, H-1).  In float32,
 *   without contraction, ax = su - x0, ay = sv - y0, top = p00 + ax*(p10 - p00), bot = p01 + ax*(p11 - p01),
 *   val = top + ay*(bot - top), out = floor(val + 0.5) (round half up) clamped to 0..255.  An invalid pixel is 0 in every channel and
 *   0 in the mask.  With k1 = k2 = 0 and K_out = K the image comes back byte for byte.  0 <= nimg <= 65535, 1 <= H, W <= 65536.
 *   Both undistortions match tests/np_track_cal.py to the bit.
 *
 * Errors (SFM_ERR_ARG / SFM_ERR_WORKSPACE, before any device call): those of TRACKS-BA (the border arrays, dtheta_dev of the step and
 *   the theta vectors of the product among the pointers that must not be NULL), and: an entry of theta_host not finite, f <= 0,
 *   a <= 0 or not finite, free outside 0..31, channels outside {1, 3}, K_out not finite or without positive focal lengths, sizes of
 *   the undistortions outside their limits, src_dev == dst_dev.  sfm_track_cal_ws_bytes is 0 for invalid sizes (240 bytes per
 *   observation for the rows, 456 per chunk, 240 per 256 observations, the step's vectors).
 * ---------------------------------------------------------------------- */
size_t sfm_track_cal_ws_bytes(int64_t ncam, int64_t npt, int64_t nobs);
int sfm_track_cal_sweep(const double* cams_dev, int64_t ncam, const double* theta_host, double aspect, const double* dtheta_dev,
                        const double* X_dev, int64_t npt, const float* obs_dev, const int32_t* track_off_dev, const int32_t* cam_idx_dev,
                        const int32_t* pt_idx_dev, const int32_t* cam_off_dev, const int32_t* cam_obs_dev, int64_t nobs, double huber, int mode,
                        uint8_t* active_dev, double* JtJ_cam_dev, double* Jtr_cam_dev, double* JtJ_pt_dev, double* Jtr_pt_dev, double* E_dev,
                        double* G_dev, double* Jtr_theta_dev, double* F_dev, double* stat_dev, int32_t* count_dev, void* ws_dev, size_t ws_bytes,
                        void* stream);
int sfm_track_cal_product(int64_t ncam, int64_t npt, const int32_t* track_off_dev, const int32_t* cam_idx_dev, const int32_t* pt_idx_dev,
                          const int32_t* cam_off_dev, const int32_t* cam_obs_dev, int64_t nobs, int mode, const double* in_dev,
                          const double* in_theta_dev, double* out_dev, double* out_theta_dev, void* ws_dev, size_t ws_bytes, void* stream);
int sfm_track_cal_step(int64_t ncam, int64_t npt, const int32_t* track_off_dev, const int32_t* cam_idx_dev, const int32_t* pt_idx_dev,
                       const int32_t* cam_off_dev, const int32_t* cam_obs_dev, int64_t nobs, const double* JtJ_cam_dev, const double* Jtr_cam_dev,
                       const double* JtJ_pt_dev, const double* Jtr_pt_dev, const double* E_dev, const double* G_dev, const double* Jtr_theta_dev,
                       double lam, int free_mask, int fix_first_camera, double cg_tol, int cg_iters, double* dc_dev, double* dtheta_dev,
                       double* dp_dev, int32_t* iters_host, int32_t* status_host, void* ws_dev, size_t ws_bytes, void* stream);
int sfm_undistort_points(const float* px_dev, int64_t n, const double* theta_host, double aspect, const double* K_out_host, float* out_dev,
                         void* stream);
int sfm_undistort_image(const uint8_t* src_dev, int64_t nimg, int64_t H, int64_t W, int channels, const double* theta_host, double aspect,
                        const double* K_out_host, uint8_t* dst_dev, uint8_t* mask_dev, void* stream);

/* ------------------------------------------------------------------------
 * MVS-PLAN (no reference counterpart; csrc/mvs_plan.hip, docs/mvs.md §8): the sources and the depth range of every view of the plane
 * sweep from the sparse model, i.e. from the point-major observations of TRACKS-BA's problem layout (track_off_dev [npt + 1], cam_idx_dev,
 * pt_idx_dev [nobs], cam_off_dev [ncam + 1], cam_obs_dev [nobs]), X_dev FLOAT64 [npt][3] and P_dev float64 [ncam][12].
 *   1 <= ncam <= 4096, 0 <= npt <= 2^31-1, 0 <= nobs <= 2^31-1, 1 <= nsrc <= SFM_PLAN_MAX_SRC = 8 (mvs.MAX_VIEWS).
 *   No index is trusted: a CSR row is clamped to 0 <= lo <= hi <= nobs; an observation whose cam_idx is outside 0..ncam-1 takes part in
 *   no pair; an entry of cam_obs outside 0..nobs-1, or naming an observation whose cam_idx is not the row's camera or whose pt_idx is
 *   outside 0..npt-1, has no depth.  Every read and write stays inside the arrays.  No entry point waits for the host and none takes a
 *   workspace.  Every output word is a count, a rank, a copy or an order statistic: the integer atomics of csrc/mvs_plan.hip commute,
 *   THERE ARE NO FLOATING-POINT ATOMICS, and a second run gives the same bits.
 *
 * sfm_view_pair_counts — shared_dev, good_dev int32 [ncam][ncam], symmetric, zero diagonal (counts modulo 2^32); C_dev float64 [ncam][3].
 *   centres    C_dev is WRITTEN by a small kernel of the same call (the cosines depend on the centres to the bit, so they come from one
 *              stated formula, and P is what callers hold), by adjugate over determinant as sfm_track_refine's centres:
 *                a00 = p5 * p10 - p6 * p9;  a01 = p2 * p9 - p1 * p10;  a02 = p1 * p6 - p2 * p5
 *                a10 = p6 * p8 - p4 * p10;  a11 = p0 * p10 - p2 * p8;  a12 = p2 * p4 - p0 * p6
 *                a20 = p4 * p9 - p5 * p8;   a21 = p1 * p8 - p0 * p9;   a22 = p0 * p5 - p1 * p4
 *                det = (p0 * a00 + p1 * a10) + p2 * a20;   C_r = -(((ar0 * p3 + ar1 * p7) + ar2 * p11) / det)
 *   shared     every pair p < q of the observations of one track (row t of track_off) whose cameras a = cam_idx[p], b = cam_idx[q] are
 *              both in 0..ncam-1 and differ adds 1 to shared[a][b] and to shared[b][a].
 *   good       the same pair also adds 1 to good[a][b] and good[b][a] iff X[t] is finite in its three components and, with the rays
 *              r = X[t] - C[a], s = X[t] - C[b] (component by component), n_r = (r0 * r0 + r1 * r1) + r2 * r2, n_s likewise,
 *                c = ((r0 * s0 + r1 * s1) + r2 * s2) / sqrt(n_r * n_s)
 *              (the order of cos_min in sfm_track_refine) satisfies cos_lo <= c <= cos_hi; a NaN c fails.  There is no acos on the
 *              device: callers pass cosines (cos_lo = cos(max angle), cos_hi = cos(min angle)).
 *   kernels    SFM_PLAN_GROUP = 16 lanes per track; the rays of a track are computed once per tile of 64 observations and kept in LDS.
 *              While ncam <= SFM_PLAN_LDS_CAMS = 96 a workgroup counts in LDS (two upper triangles of int32: 36 480 bytes at 96, with the
 *              36 KiB of ray tiles two workgroups per CU of 160 KiB) and flushes one global atomic per non-zero cell; above it every
 *              contribution is a global atomic.  A last kernel mirrors the upper triangles.
 *
 * sfm_view_depth_ranges — m_dev int32 [ncam], z_lo_dev, z_hi_dev float32 [ncam].
 *   depth      of entry k of camera i's row (o = cam_obs[k], j = pt_idx[o]):  z = (float)(((P8 * X[j]0 + P9 * X[j]1) + P10 * X[j]2) + P11)
 *              with P = P_dev[i], in float64 and rounded once; VALID iff it is finite and > 0 (denormals are valid).
 *   m          the number of valid depths of the camera.
 *   z_lo, z_hi the valid depths of rank floor(lo_permille * (m - 1) / 1000) and ceil(hi_permille * (m - 1) / 1000) in ascending order
 *              (int64 arithmetic): order statistics, what np.sort gives, ties included; not interpolated.  m == 0 writes 0, 0.
 *   kernel     one workgroup per camera; a radix select over the uint32 views of the depths, four passes of 8 bits with both ranks at once,
 *              histograms in LDS.  The depths are recomputed in every pass: rows that overlap cannot race and there is no workspace.
 *
 * sfm_view_select — nbr_dev int32 [ncam][nsrc], n_nbr_dev int32 [ncam].
 *   For view i the views j != i with good[i][j] >= min_good (>= 0), ordered by good[i][j] descending, then shared[i][j] descending, then j
 *   ascending: the first nsrc of them, then -1; n_nbr[i] = how many were written.  One wave per view, nsrc rounds over the row.
 *
 * Errors (SFM_ERR_ARG, before any device call): sizes outside the limits above, a NaN cosine bound, permille bounds that are not
 *   0 <= lo <= hi <= 1000, nsrc outside 1..8, a negative min_good, NULL where the count is non-zero (the CSR offsets, P, C and the
 *   outputs always).
 * ---------------------------------------------------------------------- */
#define SFM_PLAN_GROUP 16
#define SFM_PLAN_LDS_CAMS 96
#define SFM_PLAN_MAX_SRC 8
int sfm_view_pair_counts(const int32_t* track_off_dev, const int32_t* cam_idx_dev, const double* X_dev, int64_t npt, int64_t nobs,
                         const double* P_dev, int64_t ncam, double cos_lo, double cos_hi, double* C_dev, int32_t* shared_dev, int32_t* good_dev,
                         void* stream);
int sfm_view_depth_ranges(const int32_t* cam_off_dev, const int32_t* cam_obs_dev, const int32_t* cam_idx_dev, const int32_t* pt_idx_dev,
                          int64_t nobs, const double* X_dev, int64_t npt, const double* P_dev, int64_t ncam, int lo_permille, int hi_permille,
                          int32_t* m_dev, float* z_lo_dev, float* z_hi_dev, void* stream);
int sfm_view_select(const int32_t* shared_dev, const int32_t* good_dev, int64_t ncam, int nsrc, int min_good, int32_t* nbr_dev,
                    int32_t* n_nbr_dev, void* stream);

/* ------------------------------------------------------------------------
 * TRACKS-REGISTER (no reference counterpart; csrc/tracks_register.hip, docs/tracks.md §10): the bookkeeping of track-driven incremental
 * registration.  The FULL table is what sfm_track_build leaves: counts_dev int32 [>= 2] = (T, nobs), track_off_dev int32 [N / 2 + 2],
 * obs_node_dev int32 [N], node_track_dev int32 [N], with img_off_dev int32 [n_img + 1] and kp_dev float32 [N][2] of TRACKS;
 * N = n_nodes in 0..2^31-1, n_img in 1..65 536.
 *   counts     every counts array is read on the device and clamped as sfm_track_prune clamps it: T to 0..N / 2 + 1, nobs to 0..N (a value
 *              outside becomes the upper end); a track's range is lo = min(max(track_off[t], 0), nobs), hi = min(max(track_off[t + 1],
 *              lo), nobs).
 *   image of a node u: the largest i < n_img with img_off[i] <= u (a binary search of at most 17 steps; its result lies in 0..n_img-1
 *              whatever img_off holds).
 *   Every output word is a count, a rank, a bit-or or a copy: no word depends on the order in which atomics land (the only atomics are
 *   the integer add and or of sfm_track_view_scores).  Nothing at or past the counted rows is written.  Every read and write stays
 *   inside the arrays for garbage counts, nodes outside 0..N-1 and offsets in no order (the outputs are then unspecified); every loop
 *   is bounded.  No entry point waits for the host.
 *
 * sfm_track_restrict — registered_dev uint8 [n_img], min_len in 1..2^31-1.  Observation o is LIVE iff its node obs_node[o] lies in 0..N-1
 *   and registered[image of the node] != 0.  Track t < T is KEPT iff it has at least min_len live observations.  Kept tracks in ascending
 *   old order are tracks 0..T2-1 and hold their live observations in the old order: track_off2_dev int32 [N / 2 + 2] (T2 + 1 words
 *   written), obs_node2_dev int32 [N] (nobs2 words), track_src_dev int32 [N / 2 + 1] (the old index, T2 words), counts2_dev int32 [4] =
 *   (T2, nobs2, tracks with 1..min_len-1 live observations, non-live observations of kept tracks).  Ranks come from per-block counts and
 *   a one-workgroup scan; no atomics.  (counts2, track_off2, obs_node2) have the shape sfm_track_build leaves: sfm_track_triangulate,
 *   sfm_track_refine and sfm_track_prune run on them unchanged, and since every observation left lies in a registered image they never
 *   read a row of P_dev that belongs to an unregistered one.
 *
 * sfm_track_adopt — composes two compactions of the full table: counts_r_dev / track_src_r_dev are the counts2 / track_src that
 *   sfm_track_restrict wrote, counts_p_dev / track_off_p_dev / obs_node_p_dev / X_p_dev / track_src_p_dev the counts2 / track_off2 /
 *   obs_node2 / X2 / track_src that sfm_track_prune wrote on the (triangulated, refined) restricted table.  Pruned track p <
 *   Tp is ADOPTED by t = track_src_r[r], r = track_src_p[p], when r lies in 0..Tr-1 and t in 0..T-1.
 *   X_full_dev float32 [N / 2 + 1][3], has_point_dev uint8 [N / 2 + 1]: every row t < T is rewritten by every call: 1 and the words of
 *              X_p[p] for an adopted track, 0 and three quiet NaNs 0x7FC00000 for any other.
 *   obs_live_dev uint8 [N]: every row o < nobs is rewritten: for an adopted track, with j starting at the first observation of p, the
 *              observations o of t in ascending order: when j is before the end of p and obs_node[o] == obs_node_p[j], obs_live[o] = 1
 *              and j advances; every other row is 0.  (Both compactions keep the old order, so the list of p is a subsequence of the
 *              list of t and obs_live marks exactly the observations that survived both.)
 *
 * sfm_track_view_scores — has_point_dev as sfm_track_adopt wrote it; one frame size (width, height), finite and > 0; grid in 1..8.
 *   Node u in 0..N-1 COUNTS iff t = node_track[u] lies in 0..T-1 and has_point[t] != 0.  For every image i:
 *   seen_dev   int32 [n_img]: the nodes that count and whose image is i.
 *   cover_dev  uint64 [n_img]: the OR of the bits 1 << (cy * grid + cx) over those nodes, with, in float32,
 *                sx = (float)grid / (float)width;  sy = (float)grid / (float)height   (one division each, on the host)
 *                cx = cell(kp[u][0] * sx);  cy = cell(kp[u][1] * sy)
 *                cell(c) = NONE when c is NaN, 0 when c < 0, grid - 1 when c >= grid, else (int)c (towards zero)
 *              so keypoints outside the frame fall into the border cell.  A node with a NaN coordinate counts in seen and sets NO bit.
 *   cells_dev  int32 [n_img]: the number of set bits of cover.
 *   Registered images are scored like any other.  One lane per node; while n_img <= SFM_REGISTER_LDS_IMAGES = 256 a workgroup keeps its
 *   counters and masks in LDS (3 072 bytes) and flushes one global atomic add and or per non-zero entry; above it every node is one
 *   global atomic add and at most one 64-bit atomic or.
 *
 * sfm_track_correspondences — for image `image` in 0..n_img-1 and its nodes u in [min(max(img_off[image], 0), N), min(max(img_off[image +
 *   1], lo), N)) in ascending order, each node that counts (as above) is a row k: X_out_dev float32 [capacity][3] = the words of
 *   X_full[t], uv_out_dev float32 [capacity][2] = the words of kp[u], track_out_dev int32 [capacity] = t; count_dev int32 [1] = the
 *   number of rows, which equals seen[image].  Rows at or past min(count, capacity) are not written.  Ranks by per-block counts and a
 *   one-workgroup scan; no atomics.  X_out and uv_out are what sfm_solve_pnp_ransac takes.
 *
 * Errors (SFM_ERR_ARG, before any device call): n_nodes or capacity outside 0..2^31-1, n_img outside 1..65 536, min_len outside
 *   1..2^31-1, grid outside 1..8, a frame size that is NaN, infinite or <= 0, image outside 0..n_img-1, NULL where the count is non-zero
 *   (counts, offsets, per-track and per-image arrays and the workspaces always), a workspace smaller than the _ws_bytes twin says.  The
 *   _ws_bytes twins return 0 for invalid sizes.
 * ---------------------------------------------------------------------- */
#define SFM_REGISTER_LDS_IMAGES 256
size_t sfm_track_restrict_ws_bytes(int64_t n_nodes);
int sfm_track_restrict(const int32_t* counts_dev, const int32_t* track_off_dev, const int32_t* obs_node_dev, const int32_t* img_off_dev,
                       int n_img, int64_t n_nodes, const uint8_t* registered_dev, int64_t min_len, int32_t* track_off2_dev,
                       int32_t* obs_node2_dev, int32_t* track_src_dev, int32_t* counts2_dev, void* ws_dev, size_t ws_bytes, void* stream);
int sfm_track_adopt(const int32_t* counts_dev, const int32_t* track_off_dev, const int32_t* obs_node_dev, int64_t n_nodes,
                    const int32_t* counts_r_dev, const int32_t* track_src_r_dev, const int32_t* counts_p_dev, const int32_t* track_off_p_dev,
                    const int32_t* obs_node_p_dev, const float* X_p_dev, const int32_t* track_src_p_dev, float* X_full_dev,
                    uint8_t* has_point_dev, uint8_t* obs_live_dev, void* stream);
int sfm_track_view_scores(const int32_t* counts_dev, const int32_t* node_track_dev, const uint8_t* has_point_dev, const int32_t* img_off_dev,
                          int n_img, const float* kp_dev, int64_t n_nodes, double width, double height, int grid, int32_t* seen_dev,
                          uint64_t* cover_dev, int32_t* cells_dev, void* stream);
size_t sfm_track_correspondences_ws_bytes(int64_t n_nodes);
int sfm_track_correspondences(int image, const int32_t* counts_dev, const int32_t* node_track_dev, const uint8_t* has_point_dev,
                              const float* X_full_dev, const int32_t* img_off_dev, int n_img, const float* kp_dev, int64_t n_nodes,
                              int64_t capacity, float* X_out_dev, float* uv_out_dev, int32_t* track_out_dev, int32_t* count_dev, void* ws_dev,
                              size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * VERIFY (no reference counterpart: isfm.py:73-94 verifies one pair at a time; csrc/verify.hip, docs/tracks.md section 11): geometric
 * verification of ALL pairs of a match store in six launches (the last three once per chunk of pairs in verify.verify_pairs) and no host wait: a fixed budget of H five-point hypotheses per pair
 * from a counter-based sampler, all scored, the best decomposed and voted on.  A new algorithm, not a restatement of the sequential
 * RANSAC of sfm_find_essential_mat: the masks differ from the per-pair path's.  Every integer output is a count, a rank, a maximum of
 * a key or a copy; every float64 operation is correctly rounded in the order written (no FMA, IEEE / and sqrt; only + - * / sqrt
 * fabs fmax and comparisons are used).  tests/np_verify.py restates every output word.  store, pair_img, nq, img_off, nodes: as TRACKS.
 *
 * sfm_verify_normalise — once per node: xn[u] = ((double)kp[u].x * ifx + bx, (double)kp[u].y * ify + by) with ifx = 1 / K[0],
 *   bx = -K[2] * (1 / K[0]), ify = 1 / K[4], by = -K[5] * (1 / K[4]) (K_host: 9 doubles, row-major).  xn_dev float64 [n_nodes][2].
 *
 * sfm_verify_survivors — pair p = (i, j) with i != j and both in 0..n_img-1: the queries q < min(nq[p], cap, size of i), in ascending q,
 *   that pass the survivor rule of sfm_match_edges without keep (trainIdx0 = t in 0..size of j - 1, trainIdx1 >= 0,
 *   (double)d0 < ratio * (double)d1).  surv_dev int32 [n_pairs][cap][2]: the survivors as (q, t), then (-1, -1) up to cap.
 *   m_dev int32 [n_pairs]: their number; 0 for every other pair.
 *
 * sfm_verify_samples — samp_dev int32 [n_pairs][H][5], H = budget in 1..1024.  In uint32 arithmetic
 *     mix(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
 *     draw c of sample s of pair p:  h = mix(mix(mix(seed + 0x9e3779b9 * p) ^ s) + c);  idx = ((uint64)h * m) >> 32     (m = m_dev[p])
 *   the five slots take, for c = 0, 1, 2, .. 63, the first draws that differ from every slot filled before.  A sample that 64 draws do
 *   not fill, and every sample of a pair with m < 5, is five times -1.
 *
 * sfm_verify_models — one lane per sample.  With m' = min(m, cap): a sample is VALID when both images are in range, m' >= 5, every
 *   slot is in 0..m'-1 and both nodes (img_off[i] + q, img_off[j] + t) of its survivors lie in 0..n_nodes-1.  A valid sample runs the
 *   operations of sfm_host_five_point (csrc/host_solvers.h: cv::SVD of the 5 x 9 system with FULL_UV, the ten cubic constraints,
 *   elimination with partial pivoting, det B(z), cv::solvePoly with 300 sweeps, one 3 x 3 SVD per real root) in the same order on
 *   x1 = xn of the five first nodes, x2 = xn of the five second nodes, and returns the same bits.
 *   nmodels_dev int32 [n_pairs][H]: 0..10 (0 for an invalid sample); E_dev float64 [n_pairs][H][10][9]: the unit-norm matrices,
 *   zero past nmodels.  E_dev is the workspace of the family: n_pairs * H * 720 bytes.
 *
 * sfm_verify_score — a model is (p, s, j) with j < nmodels[p][s] (clamped to 0..10); its slot is 10 s + j.  Over the first
 *   m' = min(m, cap) survivors of the pair whose two nodes lie in 0..n_nodes-1 (m' = 0 when an image is out of range), with
 *   (a1, b1) = xn of the first node, (a2, b2) of the second, residual.hip's score_essential_kernel word for word:
 *     e0 = E0 a1 + E1 b1 + E2 * 1;  e1 = E3 a1 + E4 b1 + E5 * 1;  e2 = E6 a1 + E7 b1 + E8 * 1      (left to right)
 *     f0 = E0 a2 + E3 b2 + E6 * 1;  f1 = E1 a2 + E4 b2 + E7 * 1;  s = a2 e0 + b2 e1 + 1 * e2
 *     inlier  <=>  (float)(s * s / (((e0 e0 + e1 e1) + f0 f0) + f1 f1)) <= thr2
 *   counts_dev int32 [n_pairs][H][10]: the inlier count of every model, 0 in every other slot.
 *   best_dev uint64 [n_pairs]: the maximum over the pair's models of (count << 32) | (0xFFFFFFFF - slot): the largest count, then the
 *   smallest sample, then the smallest model index; 0 for a pair without a model.
 *
 * sfm_verify_select — per pair.  Without a model (best = 0, or a slot >= 10 H): keep row, E and Rt zero, info = (m, scored, 0, 0, -1,
 *   -1, -1, status).  Otherwise E = the model of the best slot; its Sampson inliers as above (a survivor with q >= cap is none);
 *   (R1, R2, t) = the operations of sfm_host_decompose_essential; the candidates c = 0..3 are [R1 | t], [R2 | t], [R1 | -t], [R2 | -t]
 *   (3 x 4 row-major); over the Sampson inliers the vote of sfm_recover_pose_score with rows = 4 and dist_thresh = 50 (the DLT of
 *   [I | 0] and the candidate on (a1, b1), (a2, b2), cv::SVD's one-sided Jacobi, Q2 Q3 > 0, Q2 / Q3 < 50, 0 < z' < 50).  The winner
 *   is the candidate with the most votes, the lowest c on ties.
 *   keep_dev uint8 [n_pairs][cap]: 1 at the queries q of the Sampson inliers that pass the winner's vote, 0 in every other column.
 *   E_out_dev float64 [n_pairs][9], Rt_dev float64 [n_pairs][12] (the winning candidate).
 *   info_dev int32 [n_pairs][8]: survivors m (as given), models scored (the sum of nmodels), Sampson inliers, inliers that pass the
 *   winner's vote, best sample, best model index, winning candidate, status bits (1: m < 5, 2: no model, 4: the winner has no vote).
 *
 * thr2 is (float)(thr * thr), thr = threshold / ((K[0] + K[4]) / 2), computed by the caller as sfm_find_essential_mat computes it.
 * Errors (SFM_ERR_ARG, before any device call): negative sizes, n_pairs * cap or n_nodes above 2^31 - 1, n_pairs above (2^31 - 1) / 1024
 *   (samples, models) or above (2^31 - 1) / 10 240 (score, select), whatever the budget, n_img outside 1..65 536, a NaN ratio, budget outside 1..1024, NULL where the count is non-zero (K_host and img_off_dev always).
 * ---------------------------------------------------------------------- */
#define SFM_VERIFY_MAX_BUDGET 1024
int sfm_verify_normalise(const float* kp_dev, int64_t n_nodes, const double* K_host, double* xn_dev, void* stream);
int sfm_verify_survivors(const int32_t* store_dev, int64_t n_pairs, int64_t cap, const int32_t* pair_img_dev, const int32_t* nq_dev,
                         const int32_t* img_off_dev, int n_img, double ratio, int32_t* surv_dev, int32_t* m_dev, void* stream);
int sfm_verify_samples(const int32_t* m_dev, int64_t n_pairs, int budget, uint32_t seed, int32_t* samp_dev, void* stream);
int sfm_verify_models(const int32_t* samp_dev, const int32_t* surv_dev, const int32_t* m_dev, const int32_t* pair_img_dev,
                      const int32_t* img_off_dev, int n_img, const double* xn_dev, int64_t n_nodes, int64_t n_pairs, int64_t cap, int budget,
                      int32_t* nmodels_dev, double* E_dev, void* stream);
int sfm_verify_score(const double* E_dev, const int32_t* nmodels_dev, const int32_t* surv_dev, const int32_t* m_dev,
                     const int32_t* pair_img_dev, const int32_t* img_off_dev, int n_img, const double* xn_dev, int64_t n_nodes,
                     int64_t n_pairs, int64_t cap, int budget, float thr2, int32_t* counts_dev, uint64_t* best_dev, void* stream);
int sfm_verify_select(const double* E_dev, const int32_t* nmodels_dev, const uint64_t* best_dev, const int32_t* surv_dev, const int32_t* m_dev,
                      const int32_t* pair_img_dev, const int32_t* img_off_dev, int n_img, const double* xn_dev, int64_t n_nodes,
                      int64_t n_pairs, int64_t cap, int budget, float thr2, uint8_t* keep_dev, double* E_out_dev, double* Rt_dev,
                      int32_t* info_dev, void* stream);

/* ------------------------------------------------------------------------
 * VERIFY-LO (csrc/verify_lo.hip, docs/tracks.md section 12): local optimisation of VERIFY's best hypotheses.  Between sfm_verify_score
 * and sfm_verify_select: the T best models of a pair are each refitted R times on their inliers under a widened threshold by the
 * eight-point system, recounted at thr2, and the best of all is handed to the UNCHANGED sfm_verify_select as a one-sample models buffer
 * (budget = 1).  Three launches, on the caller's stream, no host wait.  Arithmetic as VERIFY: float64, correctly rounded, in the order
 * written, no FMA, only + - * / sqrt fabs and comparisons; every integer output is a count, a maximum of a key or a copy.
 * tests/np_verify_lo.py restates every output word.  E, nmodels, counts, surv, m, pair_img, img_off, xn, thr2, m', "slot": as VERIFY.
 *
 * sfm_verify_top — the key of model (s, j), j < nmodels[p][s] (clamped to 0..10), is ((uint32)counts[p][s][j] << 32) |
 *   (0xFFFFFFFF - (10 s + j)).  top_dev uint64 [n_pairs][T], T = top in 1..16: the T largest keys of the pair in descending order,
 *   then zeros.  Keys are distinct; top[p][0] is sfm_verify_score's best[p].
 *
 * sfm_verify_lo — candidate (p, t) has a model when top[p][t] != 0 and its slot is < 10 H; without one E_lo = 0, n_lo = 0,
 *   round_lo = -1.  Otherwise, with v(E, e) the float value sfm_verify_score compares with thr2 for survivor e (over the same survivors:
 *   the first m' whose two nodes lie in 0..n_nodes-1) and n(E) the number of survivors with v <= thr2:
 *     E_cur = the model of the slot;  E_best = E_cur;  n_best = n(E_cur);  round_lo = -1
 *     for r = 0 .. R-1  (R = rounds in 0..8, wide2[r] = wide2_host[r], a float that is not NaN):
 *       W = the survivors with v(E_cur, e) <= wide2[r];  fewer than 8: stop
 *       per survivor a = (a2 a1, a2 b1, a2, b2 a1, b2 b1, b2, a1, b1, 1);  M[i][j] = M[j][i] = the sum over W of a[i] * a[j], i <= j,
 *         in this order: s_l (l = 0..255) starts at 0 and takes, for e = l, l + 256, l + 512, .. < m' in ascending order, s_l = s_l +
 *         a[i] * a[j] when e is in W;  then for h = 1, 2, 4, .. 128:  s_l = s_l + s_(l + h) for every l that is a multiple of 2 h;
 *         M[i][j] = s_0
 *       E_new = refit(M) (below);  a non-finite word in E_new: stop
 *       n_new = n(E_new);  when n_new > n_best:  E_best = E_new, n_best = n_new, round_lo = r
 *       E_cur = E_new
 *   (n(E_new) and the sums of the next round are formed in one pass over the survivors: R + 1 passes.)
 *   E_lo_dev float64 [n_pairs][T][9] = E_best;  n_lo_dev int32 [n_pairs][T] = n_best;  round_lo_dev int32 [n_pairs][T].
 *   n_lo of candidate 0 is never below the count of sfm_verify_score's best model: round -1 is that model itself.
 *
 * refit(M) = sfm_host_verify_refit(M81_host, E_host), the function the kernel's lane 0 runs, compiled for the host:
 *   cv::SVD's one-sided Jacobi (csrc/host_solvers.h, Svd: JacobiSVDImpl_, eps = 10 DBL_EPSILON, at most 30 sweeps, the singular values
 *   sorted descending by its selection sort) on the rows a_i[k] = M[k][i] of the 9 x 9 matrix; F (3 x 3 row-major) = the right
 *   singular vector of the smallest singular value (row 8 of vt; u is not formed).  (U, Vt) = cv::SVD of F (Svd::compute, 3 x 3).
 *   e[i][j] = U[i][0] * Vt[0][j] + U[i][1] * Vt[1][j];  nrm = sqrt(the sum of e[i][j] * e[i][j], row-major from 0);  E = e / nrm.
 *
 * sfm_verify_lo_pick — per pair, over the candidates t that have a model, the largest ((uint32)n_lo[p][t] << 32) | (0xFFFFFFFF - t):
 *   the most inliers, the lowest t on ties.  It writes what sfm_verify_select takes at budget = 1:
 *   E_sel_dev float64 [n_pairs][1][10][9]: the winner's E_lo in slot 0, zeros elsewhere;  nmodels_sel_dev int32 [n_pairs][1]: 1, or 0
 *   when no candidate has a model;  best_sel_dev uint64 [n_pairs]: (n_lo << 32) | 0xFFFFFFFF, or 0.
 *   lo_info_dev int32 [n_pairs][8]: top[p][0] >> 32 (the plain best count), the winner's n_lo, the winner t, its round_lo, its origin
 *   sample slot / 10 and origin model slot % 10 (the slot of top[p][t]), the number of candidates that have a model, 0.  Without a
 *   winner: (top[p][0] >> 32, 0, -1, -1, -1, -1, 0, 0).
 *
 * Errors (SFM_ERR_ARG, before any device call): n_pairs negative or above (2^31 - 1) / 10 240, budget outside 1..1024, top outside
 *   1..16, rounds outside 0..8, a NaN in wide2_host, negative sizes, n_pairs * cap or n_nodes above 2^31 - 1, n_img outside 1..65 536,
 *   NULL where the count is non-zero (img_off_dev always; wide2_host when rounds > 0).
 * ---------------------------------------------------------------------- */
#define SFM_VERIFY_LO_MAX_TOP 16
#define SFM_VERIFY_LO_MAX_ROUNDS 8
int sfm_verify_top(const int32_t* counts_dev, const int32_t* nmodels_dev, int64_t n_pairs, int budget, int top, uint64_t* top_dev, void* stream);
int sfm_verify_lo(const double* E_dev, const uint64_t* top_dev, int top, const int32_t* surv_dev, const int32_t* m_dev,
                  const int32_t* pair_img_dev, const int32_t* img_off_dev, int n_img, const double* xn_dev, int64_t n_nodes, int64_t n_pairs,
                  int64_t cap, int budget, float thr2, int rounds, const float* wide2_host, double* E_lo_dev, int32_t* n_lo_dev,
                  int32_t* round_lo_dev, void* stream);
int sfm_verify_lo_pick(const uint64_t* top_dev, const double* E_lo_dev, const int32_t* n_lo_dev, const int32_t* round_lo_dev, int64_t n_pairs,
                       int budget, int top, double* E_sel_dev, int32_t* nmodels_sel_dev, uint64_t* best_sel_dev, int32_t* lo_info_dev,
                       void* stream);
int sfm_host_verify_refit(const double* M81_host, double* E_host);

/* ------------------------------------------------------------------------
 * VERIFY-H (csrc/verify_h.hip, docs/tracks.md section 13): a homography per pair beside VERIFY's essential matrix, from the same survivors
 * and the same samples, so that a caller can tell the pairs whose essential matrix is not determined (one plane, no baseline).  Three
 * launches per chunk of pairs, on the caller's stream, no host wait.  Arithmetic as VERIFY: float64, correctly rounded, in the order
 * written, no FMA, only + - * / sqrt fabs and comparisons; every integer output is a count, a maximum of a key or a copy.
 * tests/np_verify_h.py restates every output word.  surv, m, m', pair_img, img_off, xn, samp and "valid" survivors: as VERIFY.
 *
 * sfm_verify_h_models — one lane per sample.  Sample s of pair p is the FIRST FOUR slots of samp[p][s] (sfm_verify_samples; there is no
 *   second sampler).  It is valid when both images are in range, m' >= 5, each of the four slots is in 0..m'-1 and both nodes of each of
 *   the four survivors lie in 0..n_nodes-1.  A valid sample runs homography4 (below) on x1 = xn of the four first nodes, x2 = xn of the
 *   four second nodes.  ok_dev int32 [n_pairs][H]: 1 with a model, else 0;  Hm_dev float64 [n_pairs][H][9]: the model (Hm[8] = 1), zero
 *   without one.  72 + 4 + 4 (counts) = 80 bytes a sample.
 *
 * homography4(x1, x2) = sfm_host_homography4(x1_host, x2_host, H_host) (x: four points, (a, b) interleaved; H_host all zero: no model):
 *   the 8 x 9 augmented system of h8 = 1; match k = 0..3 gives row 2k = (a1, b1, 1, 0, 0, 0, -(a2 a1), -(a2 b1) | a2) and row 2k + 1 =
 *   (0, 0, 0, a1, b1, 1, -(b2 a1), -(b2 b1) | b2).  For col = 0..7: the pivot row is the row r >= col with the largest |A[r][col]| under
 *   the comparison v > largest-so-far, r ascending from col (the lowest row on ties; a NaN never wins); it is swapped with row col;
 *   d = A[col][col]; d == 0: no model; for r = col+1..7: f = A[r][col] / d, A[r][k] = A[r][k] - f * A[col][k] for k = col+1..8.
 *   Then for col = 7..0: s = A[col][8]; s = s - A[col][k] * h[k] for k = col+1..7 ascending; h[col] = s / A[col][col].  h[8] = 1.
 *   A non-finite word among h[0..7]: no model.
 *
 * sfm_verify_h_score — over the first m' survivors of the pair whose two nodes are valid, for every sample with ok != 0:
 *     w = H6 a1 + H7 b1 + H8;  u = (H0 a1 + H1 b1 + H2) / w;  v = (H3 a1 + H4 b1 + H5) / w         (left to right)
 *     d = (u - a2) * (u - a2) + (v - b2) * (v - b2);   inlier  <=>  w > 0 and (float)d <= thr2h
 *   counts_dev int32 [n_pairs][H]: the inlier count, 0 for a sample without a model.  best_dev uint64 [n_pairs]: the maximum over the
 *   pair's models of ((uint32)count << 32) | (0xFFFFFFFF - s): the largest count, then the lowest sample; 0 without a model.
 *
 * sfm_verify_h_select — per pair.  Without a model (best = 0, or its sample >= H): keep_h row, H_out and sv zero, h_info = (m, 0, 0, 0,
 *   -1, -1, 0, status | 2).  Otherwise, with n(G) the number of valid survivors e < m' with q < cap that are inliers of G at thr2h:
 *     1. Hs = Hm of the best sample;  n_s = n(Hs).
 *     2. when refit == 1 and n_s >= 8: per inlier of Hs, r1 = (-a1, -b1, -1, 0, 0, 0, a2 a1, a2 b1, a2) and r2 = (0, 0, 0, -a1, -b1, -1,
 *        b2 a1, b2 b1, b2);  M[i][j] = M[j][i] = the sum over the inliers of (r1[i] * r1[j] + r2[i] * r2[j]), i <= j, in VERIFY-LO's order:
 *        s_l (l = 0..255) starts at 0 and takes its survivors e = l, l + 256, .. < m' ascending, then for h = 1, 2, 4, .. 128:
 *        s_l = s_l + s_(l + h) for every l that is a multiple of 2 h;  M[i][j] = s_0.
 *        c = sfm_host_verify_h_refit(M): cv::SVD's one-sided Jacobi on the rows a_i[k] = M[k][i], row 8 of vt (the right singular vector
 *        of the smallest singular value), nine words.  A non-finite word in c: the refit is dropped.  The sign of a null vector is
 *        arbitrary, and -c has the u, v and d of c with w of the other sign, so one pass counts both: n_pos = n(c), n_neg = n(-c);
 *        Hr = -c when n_neg > n_pos, else c;  n_r = max(n_pos, n_neg).
 *     3. the winner Hw = Hr when n_r > n_s (strictly), else Hs: the final count is never below the sample's.
 *     4. (W0 >= W1 >= W2) = the singular values of cv::SVD's Jacobi on Hw (rows a_i[k] = Hw[k][i]);  H_out = Hw / W1 word by word;
 *        sv = (W0 / W1, W1 / W1, W2 / W1)  (= sfm_host_verify_h_normalise).
 *     5. every inlier of Hw has w > 0 by the inlier rule, so the sum of w over them is positive and H_out keeps its sign.
 *   keep_h_dev uint8 [n_pairs][cap]: 1 at the queries q of the inliers of Hw (the winner before step 4), 0 in every other column.
 *   H_out_dev float64 [n_pairs][9];  sv_dev float64 [n_pairs][3].
 *   h_info_dev int32 [n_pairs][8]: survivors m (as given), samples with a model (ok != 0), n(Hw), n_s, best sample, 0 when the refit
 *   won else -1, 0, status bits (1: m < 5, 2: no model).
 *
 * thr2h is (float)(thr * thr), thr = threshold_h / ((K[0] + K[4]) / 2): VERIFY's thr2 at the homography's own threshold.
 * Errors (SFM_ERR_ARG, before any device call): negative sizes, n_pairs * cap or n_nodes above 2^31 - 1, n_pairs above (2^31 - 1) / 1024,
 *   n_img outside 1..65 536, budget outside 1..1024, a NaN thr2h, refit outside 0..1, NULL where the count is non-zero (img_off_dev always).
 * ---------------------------------------------------------------------- */
int sfm_verify_h_models(const int32_t* samp_dev, const int32_t* surv_dev, const int32_t* m_dev, const int32_t* pair_img_dev,
                        const int32_t* img_off_dev, int n_img, const double* xn_dev, int64_t n_nodes, int64_t n_pairs, int64_t cap, int budget,
                        int32_t* ok_dev, double* Hm_dev, void* stream);
int sfm_verify_h_score(const double* Hm_dev, const int32_t* ok_dev, const int32_t* surv_dev, const int32_t* m_dev, const int32_t* pair_img_dev,
                       const int32_t* img_off_dev, int n_img, const double* xn_dev, int64_t n_nodes, int64_t n_pairs, int64_t cap, int budget,
                       float thr2h, int32_t* counts_dev, uint64_t* best_dev, void* stream);
int sfm_verify_h_select(const double* Hm_dev, const int32_t* ok_dev, const uint64_t* best_dev, const int32_t* surv_dev, const int32_t* m_dev,
                        const int32_t* pair_img_dev, const int32_t* img_off_dev, int n_img, const double* xn_dev, int64_t n_nodes,
                        int64_t n_pairs, int64_t cap, int budget, float thr2h, int refit, uint8_t* keep_h_dev, double* H_out_dev,
                        double* sv_dev, int32_t* h_info_dev, void* stream);
int sfm_host_homography4(const double* x1_host, const double* x2_host, double* H_host);
int sfm_host_verify_h_refit(const double* M81_host, double* H_host);
int sfm_host_verify_h_normalise(const double* H_host, double* H_out_host, double* sv_host);

/* ------------------------------------------------------------------------
 * GUIDED (no reference counterpart; csrc/guided.hip, docs/tracks.md section 14): guided matching.  The 2-NN of every query among the
 * train keypoints inside the epipolar band of its pair's essential matrix, as a second match store in the format of the global one,
 * and the mutual check on it.  Two launches and one clear, on the caller's stream, no host wait.  The band test is float64, correctly
 * rounded, in the order written, no FMA, IEEE division; the distances are float32 in the oracle's order; every other output word is a
 * minimum of an integer key, a count or a copy, so no word depends on the order in which lanes or workgroups run.
 * tests/np_guided.py restates every output word.  pair_img, nq, img_off, xn, nodes: as VERIFY.
 *
 * Inputs.  E_dev float64 [n_pairs][9] (sfm_verify_select's E_out).  active_dev uint8 [n_pairs].  desc_dev float32 [n_nodes][128], the
 * descriptors of all images concatenated in node order, 16-byte aligned.  rev_stride: the row length of rev (below).
 *
 * The band.  Pair p = (i, j) has queries q < qb = max(min(nq[p], cap, size of i), 0) and train keypoints t < min(size of j, rev_stride)
 * (size of k = img_off[k + 1] - img_off[k]).  With (a1, b1) = xn[img_off[i] + q], (a2, b2) = xn[img_off[j] + t] and E = E_dev[p]:
 *     e0 = E0 a1 + E1 b1 + E2 * 1;  e1 = E3 a1 + E4 b1 + E5 * 1;  e2 = E6 a1 + E7 b1 + E8 * 1      (left to right)
 *     f0 = E0 a2 + E3 b2 + E6 * 1;  f1 = E1 a2 + E4 b2 + E7 * 1;  s = a2 e0 + b2 e1 + 1 * e2
 *     (q, t) is in the band  <=>  (float)(s * s / (((e0 e0 + e1 e1) + f0 f0) + f1 f1)) <= thr2g
 *   the words of sfm_verify_score.  A NaN quotient is out of the band, so an all-zero or non-finite E has an empty band.  The band is
 *   empty (qb = 0) when an image is outside 0..n_img-1, when i == j and when active[p] == 0; a keypoint whose node lies outside
 *   0..n_nodes-1 is in no band.  (The kernel decides most tests by comparing s * s with thr2g * denominator under a guard band of
 *   2^-22 and divides inside it: the decision is the one above for every input.)
 *
 * The distance of (q, t) is d = sqrtf(l2sqr(desc[img_off[i] + q], desc[img_off[j] + t])) with l2sqr the direct form of A2 (the oracle's
 * orc_l2sqr_f32 at n = 128): acc[l] (l = 0..7) starts at 0 and takes acc[l] = acc[l] + (a[8 k + l] - b[8 k + l])^2 for k = 0..15;
 * s_l = acc[l] + acc[l + 4] (l = 0..3); l2sqr = ((s_0 + s_1) + s_2) + s_3.  A CANDIDATE is a band pair whose d is neither NaN nor +inf.
 *
 * sfm_guided_match — store_g_dev int32 [n_pairs][2][cap][2], the format of sfm_knn2_* blocks stacked per pair (what sfm_match_edges,
 *   sfm_verify_survivors read).  For q < qb the two candidates with the smallest key ((uint64)bits(d) << 32) | t: trainIdx at
 *   [p][0][q][0..1], the float32 bits of d at [p][1][q][0..1]; a missing neighbour is -1 with +inf.  Rows qb <= q < cap are (-1, -1,
 *   +inf, +inf).  (A2's sequential strict-'<' rule restricted to the band.)  In the same pass every candidate lowers
 *   rev[p][t] = min(((uint64)bits(d) << 32) | q).  rev is the workspace: uint64 [n_pairs][rev_stride], cleared to all ones by the call.
 *   With thr2g = +inf, a finite E with a non-zero denominator and rev_stride >= the size of j, store_g[p] is the KNN store of the pair.
 *
 * sfm_guided_mutual — keep_g_dev uint8 [n_pairs][cap]: 1 <=> q < qb', trainIdx0 = t0 in 0..rev_stride-1 and (uint32)rev[p][t0] == q;
 *   0 in every other column.  qb' is qb without the active flag (the store of an inactive pair has no neighbour).
 *   info_g_dev int32 [n_pairs][4]: qb', queries q < qb' with trainIdx0 >= 0, with trainIdx1 >= 0, with keep_g set.
 *
 * sfm_guided_ws_bytes = n_pairs * rev_stride * 8 (0 for arguments sfm_guided_match rejects).
 * Errors (SFM_ERR_ARG, before any device call): negative sizes, n_pairs, cap, rev_stride, n_pairs * cap, n_pairs * rev_stride or
 *   n_nodes above 2^31 - 1, n_img outside 1..65 536, a NaN thr2g, a workspace smaller than sfm_guided_ws_bytes, desc_dev not 16-byte
 *   aligned, NULL where the count is non-zero (img_off_dev always).
 * ---------------------------------------------------------------------- */
size_t sfm_guided_ws_bytes(int64_t n_pairs, int64_t rev_stride);
int sfm_guided_match(const float* desc_dev, const double* xn_dev, int64_t n_nodes, const double* E_dev, const uint8_t* active_dev,
                     const int32_t* pair_img_dev, const int32_t* nq_dev, const int32_t* img_off_dev, int n_img, int64_t n_pairs, int64_t cap,
                     float thr2g, int32_t* store_g_dev, void* ws_dev, size_t ws_bytes, int64_t rev_stride, void* stream);
int sfm_guided_mutual(const int32_t* store_g_dev, const void* ws_dev, size_t ws_bytes, int64_t rev_stride, const int32_t* pair_img_dev,
                      const int32_t* nq_dev, const int32_t* img_off_dev, int n_img, int64_t n_pairs, int64_t cap, uint8_t* keep_g_dev,
                      int32_t* info_g_dev, void* stream);

/* ------------------------------------------------------------------------
 * RETRIEVAL (no reference counterpart; csrc/retrieval.hip, docs/retrieval.md): image retrieval.  One VLAD signature per image from the
 * descriptors of its keypoints and a vocabulary of centres, the k most similar images of every image, and the pair list of those
 * neighbourhoods: what every consumer of a pair list takes in place of all_pairs when the images have no order.  Every integer
 * output is a sum, a minimum, a count, a rank or a copy; every float output is an elementwise, correctly rounded function of
 * integers, in the order written (no FMA, IEEE / and sqrt), so no word depends on the order in which lanes or workgroups run.
 * Every loop is bounded in the code.  All launches go to the caller's stream, no host wait.  tests/np_retrieval.py restates every
 * output word.  Nodes, img_off, n_img (1..65 536): as TRACKS; a node at or past img_off[n_img - 1] belongs to the last image.
 * desc_dev float32 [n_nodes][128], 16-byte aligned, as GUIDED.  centres_dev float32 [C][128], 1 <= C <= 256, 16-byte aligned.
 *
 * sfm_vlad_accumulate — assignment and sums in one entry point (one clear and two launches).
 *   distance    for node u and centre c, d2 = l2sqr(desc[u], centre[c]), the direct form of GUIDED: acc[l] (l = 0..7) starts at 0 and
 *               takes acc[l] = acc[l] + (a[8 k + l] - b[8 k + l])^2 for k = 0..15; s_l = acc[l] + acc[l + 4] (l = 0..3);
 *               l2sqr = ((s_0 + s_1) + s_2) + s_3.  No square root.  A CANDIDATE is a c whose d2 is neither NaN nor +inf.
 *   assign_dev  int32 [n_nodes]: the candidate with the smallest key ((uint64)bits(d2) << 32) | c; -1 when there is none.
 *   term        for an assigned node of image i, r = desc[u][k] - centre[c][k] in float32 and
 *               t = (int64) rintf(fminf(fmaxf(r * scale, -2^30), 2^30)); rintf rounds half to even.  scale: positive, finite.
 *   acc_dev     int64 [n_img][C][128]: acc[i][c][k] = the sum of t.   count_dev int32 [n_img][C]: the assigned nodes.  The call
 *               clears both.  A workgroup owns 1 024 consecutive nodes, cuts them at the image boundaries, sorts a segment by
 *               centre in LDS; eight groups of 32 lanes each walk an eighth of the sorted list and sum in int64 registers while
 *               the centre stays: one 64-bit integer atomic add per (segment, centre, dimension, lane group whose eighth holds
 *               that centre) with a non-zero sum, so at most eight per (segment, centre, dimension).  DEVIATION from "the
 *               descriptors are read once": they are read from global memory TWICE, by the assignment and again by the sums,
 *               which must know the centre before they can form a residual; whether the second read is served by a cache has not
 *               been measured, and the byte floor of scripts/bench_retrieval.py counts both reads.  The centres pass through LDS
 *               32 at a time for the distances and are read from global memory, one row per run of equal centres, for the sums.
 *
 * sfm_vlad_centres — one Lloyd update from an accumulate call made with ONE image (img_off = [0, N]): with count[c] != 0
 *   centre'[c][k] = (float)((double)centre[c][k] + (double)acc[c][k] / ((double)count[c] * (double)scale)); a centre with count 0 keeps
 *   its bits.  centres_out_dev may be centres_dev.
 *
 * sfm_vlad_signature — per (image i, centre c), in float64: a_k = (double)acc[i][c][k] (round to nearest even above 2^53); with
 *   ssr != 0, a_k = copysign(sqrt(|a_k|), a_k).  n2 = the sum of a_k * a_k for k = 0, 1, .. 127, left to right from 0.
 *   q[i][c][k] = (int8) fmin(fmax(rint((a_k / sqrt(n2)) * qs), -127), 127); the block is all zero when n2 is 0 or not finite.
 *   sig_dev int8 [n_img][C * 128].  norm2_dev int32 [n_img]: the sum of q * q over the image, at most 256 * 128 * 127^2 < 2^31; the
 *   call clears it.  qs: float64, positive and finite (127 unless the caller knows better).
 *
 * sfm_vlad_shortlist — n_img <= 16 384 HERE (the similarities of all pairs pass through the workspace: n_img^2 words).
 *   S[i][j]     the int32 sum of sig[i][.] * sig[j][.] over C * 128 bytes, exact (v_mfma_i32_16x16x64_i8; |S| <= the bound above).
 *   sim[i][j]   (float)((double)S / sqrt((double)norm2[i] * (double)norm2[j])).
 *   candidate   j != i with norm2[i] != 0, norm2[j] != 0 and sim[i][j] >= min_sim (float32; -inf admits all, +inf none).
 *   nbr_dev     int32 [n_img][k]: the candidates of i in descending sim, ties to the smaller j; -1 where there are fewer than k.
 *   nbr_sim_dev float32 [n_img][k]: their sim, -inf where missing.   1 <= k <= 64.
 *   The workspace holds one word per (i, j); sfm_vlad_shortlist_ws_bytes(n_img) = n_img^2 * 4 (0 for an n_img outside 1..16 384).
 *
 * sfm_vlad_pairs — n_img <= 16 384 (an adjacency bitmap of n_img^2 bits in the workspace).  A VALID entry of nbr_dev [n_img][k] is
 *   a j in 0..n_img-1 other than its row.  The pair (a, b), a < b, is SELECTED iff b is a valid entry of row a OR a is one of row b;
 *   with mutual != 0: AND.  pairs_out_dev int32 [cap_pairs][2]: the selected pairs in ascending (a, b) order, those that fit.
 *   count_dev int32 [2] = (selected, written = min(selected, cap_pairs)).  Nothing at or past the written rows is written;
 *   cap_pairs < selected is no error.  sfm_vlad_pairs_ws_bytes(n_img): the bitmap and n_img counters, each rounded up to 256 bytes.
 *
 * Errors (SFM_ERR_ARG, before any device call): negative sizes, n_nodes or cap_pairs above 2^31 - 1, C outside 1..256, k outside
 *   1..64, n_img outside 1..65 536 (accumulate, signature) or 1..16 384 (shortlist, pairs), a scale or qs that is NaN, not positive or
 *   infinite, a NaN min_sim, a workspace smaller than the _ws_bytes twin says, desc_dev, centres_dev (accumulate) or sig_dev (shortlist)
 *   not 16-byte aligned, NULL where the count is non-zero (everything but desc_dev, assign_dev at n_nodes = 0 and pairs_out_dev at
 *   cap_pairs = 0).
 * ---------------------------------------------------------------------- */
int sfm_vlad_accumulate(const float* desc_dev, int64_t n_nodes, const float* centres_dev, int n_centres, const int32_t* img_off_dev, int n_img,
                        float scale, int32_t* assign_dev, int64_t* acc_dev, int32_t* count_dev, void* stream);
int sfm_vlad_centres(const float* centres_dev, const int64_t* acc_dev, const int32_t* count_dev, int n_centres, float scale,
                     float* centres_out_dev, void* stream);
int sfm_vlad_signature(const int64_t* acc_dev, int n_img, int n_centres, int ssr, double qs, int8_t* sig_dev, int32_t* norm2_dev, void* stream);
size_t sfm_vlad_shortlist_ws_bytes(int n_img);
int sfm_vlad_shortlist(const int8_t* sig_dev, const int32_t* norm2_dev, int n_img, int n_centres, int k, float min_sim, int32_t* nbr_dev,
                       float* nbr_sim_dev, void* ws_dev, size_t ws_bytes, void* stream);
size_t sfm_vlad_pairs_ws_bytes(int n_img);
int sfm_vlad_pairs(const int32_t* nbr_dev, int n_img, int k, int mutual, int32_t* pairs_out_dev, int64_t cap_pairs, int32_t* count_dev,
                   void* ws_dev, size_t ws_bytes, void* stream);

/* Dev diagnostics: when non-NULL, every knn filter workgroup b writes int64[4] =
 * {start tick, end tick (100 MHz), HW_ID, XCC_ID} at dev_buf[4*b..] and every refine workgroup w
 * int64[16] phase ticks at dev_buf[16384 + 16*w..]; NULL disables. */
int sfm_debug_set_trace(void* dev_buf);
/* Test hook: workgroup `workgroup` of every following knn_split_images_kernel launch starts `microseconds` (<= 100 000) late — the
 * situation of a grid that is not co-resident (tests/test_gpu_knn_q8.py: the repair of pairs quantised in vain must not depend on
 * when a workgroup is dispatched).  workgroup = -1 switches it off. */
int sfm_debug_knn_split_delay(int workgroup, int microseconds);
/* Test hook: with on != 0 every following knn_prep_kernel launch sends pairs that are quantised for the integer body through the
 * GENERAL row loop instead of the lean one (tests/test_gpu_knn_prep_lean.py: both must leave the same words).  0 switches it off. */
int sfm_debug_knn_prep_general(int on);
/* Test hook: every following knn_prep_kernel launch runs `n` (1 .. 256) row workgroups per pair instead of the number the library
 * derives from the batch size (256 up to four pairs, then as many as fill one resident round: 128 for eight); 0 restores the rule.
 * Results do not depend on it (tests/test_gpu_knn_prep_blocks.py); it also serves same-box timing comparisons. */
int sfm_debug_knn_prep_blocks(int n);
/* Test hook: with on == 0 every following knn_refine_kernel launch runs the quantised body's integer row passes per query (two
 * 8-row records of each of a wave's four queries per pass, trip count of the longest list) instead of pooling the wave's four record
 * lists over its eight 8-lane groups (the default, on != 0).  Results do not depend on it (tests/test_gpu_knn_refine_pooled.py); it
 * also serves same-box timing comparisons. */
int sfm_debug_knn_refine_pooled(int on);
/* Test hook: every following plan of the integer bodies' filter (exact-integer and quantised: stats[3] = 4 / 5) gets at most `n`
 * (1 .. 256) workgroups instead of min(256, units); 0 restores the rule.  With few workgroups a segment spans several substreams at
 * small sizes (the key flush inside the tile loop, tests/test_gpu_knn_flush.py).  The count sizes the workspace: call it BEFORE the
 * *_ws_bytes query and keep it until the launch.  Results do not depend on it. */
int sfm_debug_knn_filter_workgroups(int n);
int sfm_profile_read(int slot, double* total_ms_host, int64_t* launches_host);
/* How often library calls of this process have WAITED for the device so far (cumulative; the RANSAC entry points read the
 * hypothesis scores back chunk by chunk, the Schur solver its convergence scalars).  Diagnostics: bench.py reports the
 * difference over a 57-camera run per registered camera. */
int64_t sfm_host_sync_count(void);
/* Where sfm_solve_pnp_ransac's host time went since the last reset (microseconds, accumulated over calls): out10[0] calls,
 * [1..7] copy-in, EPnP hypotheses (host), scoring + wait, mask / inlier bookkeeping, DLT initialisation, LM sweeps (device +
 * wait), LM host algebra; [8] hypothesis chunks, [9] LM sweeps.  reset != 0 clears the accumulators. */
int sfm_pnp_profile_read(double* out10_host, int reset);
/* sfm_solve_pnp_ransac's Levenberg-Marquardt sweeps are answered by ONE resident workgroup per call (the "sweep server",
 * csrc/ransac.hip) that the host drives through its pinned mailbox instead of a launch + stream synchronisation per sweep.
 * sfm_host_poll_count: spins of the host's waiting loop since load (a measure of time spent waiting on the mailbox, not of API
 * calls; those waits do NOT count in sfm_host_sync_count).  sfm_debug_pnp_sweep_server(0) selects the launch-per-sweep path
 * (A/B measurements, parity tests of one path against the other), (1) the server (default); returns the previous setting. */
int64_t sfm_host_poll_count(void);
int sfm_debug_pnp_sweep_server(int on);

#ifdef __cplusplus
}
#endif
#endif /* SFM_HIP_H */
