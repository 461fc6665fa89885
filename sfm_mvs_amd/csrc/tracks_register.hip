// Bookkeeping of track-driven incremental registration (include/sfm_hip.h, "TRACKS-REGISTER"; docs/tracks.md §10).
//   sfm_track_restrict         the tracks with at least min_len observations in registered images, with those observations only, in
//                              the shape sfm_track_build leaves: sfm_track_triangulate / _refine / _prune run on the result unchanged
//   sfm_track_adopt            composes the track_src of restrict and of prune: the point, a flag and the surviving observations of
//                              every track of the FULL table
//   sfm_track_view_scores      per image: keypoints whose track has a point, the grid cells they cover (a 64-bit mask) and its popcount
//   sfm_track_correspondences  the (point, keypoint, track) triples of one image in ascending keypoint: what sfm_solve_pnp_ransac takes
// Every output word is a count, a rank, a bit-or or a copy: the integer atomics of the scores add and or, so no word depends on the order
// in which they land; ranks come from per-block counts and a one-workgroup scan (the count / scan / place of tracks_refine.hip's prune).
// The counts are read and clamped on the device as sfm_track_prune clamps them; every index that comes out of device memory is checked
// against its array before it is used, and every loop runs over a range fixed at launch or clamped to the arrays.  The helpers image_of,
// wave_sum, block_sum and the scan are copies of csrc/tracks_refine.hip's, as the other files copy theirs.  tests/np_tracks_register.py
// restates every output word.
#include <algorithm>
#include <climits>
#include <cmath>

#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxGrid = 1 << 16;               // workgroups per launch; the kernels stride over what is left
constexpr int kScanThreads = 1024;
constexpr int64_t kMaxCount = INT32_MAX;
constexpr int kMaxImages = 65536;
constexpr int kSearchSteps = 17;                // binary search over at most 65 537 offsets
constexpr int kLdsImages = SFM_REGISTER_LDS_IMAGES;   // view_scores keeps its counters and masks in LDS up to this many images
constexpr int kMaxCells = 8;                    // grid <= 8: 64 cells, one bit each
constexpr unsigned kQuietNan = 0x7FC00000u;

static_assert(kLdsImages == kBlock, "scores_kernel initialises and flushes one LDS slot per thread");

__device__ inline bool in_range(int a, int n) { return (unsigned)a < (unsigned)n; }

// The image of node u: the largest i < n_img with img_off[i] <= u.
__device__ inline int image_of(const int* __restrict__ img_off, int n_img, int u) {
    int lo = 0, hi = n_img;                                                     // img_off[lo] <= u < img_off[hi]
    for (int step = 0; step < kSearchSteps && hi - lo > 1; ++step) {
        const int mid = lo + ((hi - lo) >> 1);
        if (img_off[mid] <= u) lo = mid; else hi = mid;
    }
    return lo;                                                                  // in 0..n_img-1 whatever img_off holds
}

__device__ inline int wave_sum(int v) {
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// Sum over the workgroup, valid in every thread.
__device__ inline int block_sum(int v, int* lds) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    int t = 0;
    for (int k = 0; k < kWaves; ++k) t += lds[k];
    return t;
}

// Inclusive scan of v over the workgroup of kBlock threads through buf.
__device__ inline int block_scan(int v, int* buf) {
    const int tid = threadIdx.x;
    __syncthreads();
    buf[tid] = v;
    __syncthreads();
    for (int off = 1; off < kBlock; off <<= 1) {
        const int add = tid >= off ? buf[tid - off] : 0;
        __syncthreads();
        buf[tid] += add;
        __syncthreads();
    }
    return buf[tid];
}

// One workgroup of kScanThreads: part[0..nblocks) -> exclusive offsets in place (keep == false: left as they are); returns the total in
// thread kScanThreads - 1.
__device__ inline int scan_parts(int* __restrict__ part, long long nblocks, bool keep, int* buf) {
    const int tid = threadIdx.x;
    const long long seg = (nblocks + kScanThreads - 1) / kScanThreads;
    const long long lo = min(tid * seg, nblocks), hi = min(lo + seg, nblocks);
    int sum = 0;
    for (long long b = lo; b < hi; ++b) sum += part[b];
    buf[tid] = sum;
    __syncthreads();
    for (int off = 1; off < kScanThreads; off <<= 1) {
        const int add = tid >= off ? buf[tid - off] : 0;
        __syncthreads();
        buf[tid] += add;
        __syncthreads();
    }
    if (keep) {
        int run = buf[tid] - sum;
        for (long long b = lo; b < hi; ++b) {
            const int v = part[b];
            part[b] = run;
            run += v;
        }
    }
    return buf[tid];
}

struct Counts {
    int T, nobs;
};

__device__ inline Counts clamped(const int* __restrict__ counts, int n, int track_cap) {
    Counts c;
    c.T = counts[0];
    c.nobs = counts[1];
    if (c.T < 0 || c.T > track_cap) c.T = track_cap;
    if (c.nobs < 0 || c.nobs > n) c.nobs = n;
    return c;
}

// ---- restrict -------------------------------------------------------------------------------------------------------------

struct RestrictWs {
    int *keep, *part_t, *part_o, *part_s, *part_d;   // keep [cap]: the live observations of a kept track, -1 for any other
    size_t bytes;
};

__device__ inline bool is_live(int node, const int* __restrict__ img_off, int n_img, const unsigned char* __restrict__ registered, int n) {
    return in_range(node, n) && registered[image_of(img_off, n_img, node)] != 0;
}

// Per 256-track block: kept tracks, the live observations they hold, tracks with 1..min_len-1 live observations, the observations
// kept tracks lose.
__global__ __launch_bounds__(kBlock) void restrict_count_kernel(const int* __restrict__ counts, const int* __restrict__ track_off,
                                                                const int* __restrict__ obs_node, const int* __restrict__ img_off, int n_img,
                                                                const unsigned char* __restrict__ registered, int n, int track_cap,
                                                                long long min_len, long long nblocks, RestrictWs w) {
    __shared__ int lds[kWaves];
    const Counts c = clamped(counts, n, track_cap);
    for (long long blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const long long t = blk * kBlock + threadIdx.x;
        int kept = 0, held = 0, few = 0, lost = 0;
        if (t < c.T) {
            const int lo = min(max(track_off[t], 0), c.nobs), hi = min(max(track_off[t + 1], lo), c.nobs);
            int live = 0;
            for (int o = lo; o < hi; ++o) live += is_live(obs_node[o], img_off, n_img, registered, n);
            if ((long long)live >= min_len) {
                kept = 1;
                held = live;
                lost = (hi - lo) - live;
            } else if (live >= 1) {
                few = 1;
            }
            w.keep[t] = kept ? live : -1;
        }
        const int st = block_sum(kept, lds), so = block_sum(held, lds), ss = block_sum(few, lds), sd = block_sum(lost, lds);
        if (threadIdx.x == 0) {
            w.part_t[blk] = st;
            w.part_o[blk] = so;
            w.part_s[blk] = ss;
            w.part_d[blk] = sd;
        }
    }
}

// Workgroups 0 and 1: the kept-track and live-observation block counts -> exclusive offsets in place; 2 and 3 sum theirs.
// counts2 = (T2, nobs2, tracks with 1..min_len-1 live observations, non-live observations of kept tracks).
__global__ __launch_bounds__(kScanThreads) void restrict_scan_kernel(RestrictWs w, long long nblocks, int* __restrict__ counts2) {
    __shared__ int buf[kScanThreads];
    int* part = blockIdx.x == 0 ? w.part_t : blockIdx.x == 1 ? w.part_o : blockIdx.x == 2 ? w.part_s : w.part_d;
    const int total = scan_parts(part, nblocks, blockIdx.x < 2, buf);
    if (threadIdx.x == kScanThreads - 1) counts2[blockIdx.x] = total;
}

__global__ __launch_bounds__(kBlock) void restrict_place_kernel(const int* __restrict__ counts, const int* __restrict__ track_off,
                                                                const int* __restrict__ obs_node, const int* __restrict__ img_off, int n_img,
                                                                const unsigned char* __restrict__ registered, int n, int track_cap,
                                                                long long nblocks, RestrictWs w, const int* __restrict__ counts2,
                                                                int* __restrict__ track_off2, int* __restrict__ obs_node2,
                                                                int* __restrict__ track_src) {
    __shared__ int scan_t[kBlock], scan_o[kBlock];
    const Counts c = clamped(counts, n, track_cap);
    if (blockIdx.x == 0 && threadIdx.x == 0) track_off2[counts2[0]] = counts2[1];  // counts2[0] <= T <= N / 2 + 1: inside the N / 2 + 2 words
    for (long long blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const long long t = blk * kBlock + threadIdx.x;
        const int held = t < c.T ? w.keep[t] : -1;
        const int rank_t = block_scan(held >= 0, scan_t), rank_o = block_scan(max(held, 0), scan_o);
        if (held >= 0) {
            const int r = w.part_t[blk] + rank_t - 1;                                   // < T2 <= T
            int at = w.part_o[blk] + rank_o - held;
            track_off2[r] = at;
            track_src[r] = (int)t;
            const int lo = min(max(track_off[t], 0), c.nobs), hi = min(max(track_off[t + 1], lo), c.nobs);
            const long long end = (long long)at + held;                                 // the row after this track's: no write reaches it
            for (int o = lo; o < hi; ++o) {                                             // (at < n: ranges that overlap can hold more than n rows in all)
                const int node = obs_node[o];
                if (is_live(node, img_off, n_img, registered, n) && at < end && in_range(at, n)) obs_node2[at++] = node;
            }
        }
    }
}

// ---- adopt ----------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock) void adopt_clear_kernel(const int* __restrict__ counts, int n, int track_cap, long long nblocks,
                                                             unsigned* __restrict__ X_full, unsigned char* __restrict__ has_point,
                                                             unsigned char* __restrict__ obs_live) {
    const Counts c = clamped(counts, n, track_cap);
    for (long long blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const long long i = blk * kBlock + threadIdx.x;
        if (i < c.T) {
            has_point[i] = 0;
            X_full[3 * i + 0] = kQuietNan;
            X_full[3 * i + 1] = kQuietNan;
            X_full[3 * i + 2] = kQuietNan;
        }
        if (i < c.nobs) obs_live[i] = 0;
    }
}

// One lane per pruned track p: its track of the full table is t = src_r[src_p[p]].
__global__ __launch_bounds__(kBlock) void adopt_place_kernel(const int* __restrict__ counts, const int* __restrict__ track_off,
                                                             const int* __restrict__ obs_node, int n, int track_cap,
                                                             const int* __restrict__ counts_r, const int* __restrict__ src_r,
                                                             const int* __restrict__ counts_p, const int* __restrict__ track_off_p,
                                                             const int* __restrict__ obs_node_p, const unsigned* __restrict__ X_p,
                                                             const int* __restrict__ src_p, long long nblocks, unsigned* __restrict__ X_full,
                                                             unsigned char* __restrict__ has_point, unsigned char* __restrict__ obs_live) {
    const Counts c = clamped(counts, n, track_cap), cr = clamped(counts_r, n, track_cap), cp = clamped(counts_p, n, track_cap);
    for (long long blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const long long p = blk * kBlock + threadIdx.x;
        if (p >= cp.T) continue;
        const int r = src_p[p];
        if (!in_range(r, cr.T)) continue;
        const int t = src_r[r];
        if (!in_range(t, c.T)) continue;
        has_point[t] = 1;
        X_full[3 * (size_t)t + 0] = X_p[3 * p + 0];
        X_full[3 * (size_t)t + 1] = X_p[3 * p + 1];
        X_full[3 * (size_t)t + 2] = X_p[3 * p + 2];
        const int lo = min(max(track_off[t], 0), c.nobs), hi = min(max(track_off[t + 1], lo), c.nobs);
        const int plo = min(max(track_off_p[p], 0), cp.nobs), phi = min(max(track_off_p[p + 1], plo), cp.nobs);
        int j = plo;
        for (int o = lo; o < hi; ++o)                                                   // the pruned list is a subsequence of the full one
            if (j < phi && obs_node[o] == obs_node_p[j]) {
                obs_live[o] = 1;
                ++j;
            }
    }
}

// ---- view scores ----------------------------------------------------------------------------------------------------------

__device__ inline bool has_point_of(int u, const int* __restrict__ node_track, const unsigned char* __restrict__ has_point, int T, int* track) {
    const int t = node_track[u];
    *track = t;
    return in_range(t, T) && has_point[t] != 0;
}

// The cell of coordinate v at scale s = (float)grid / size: -1 for a NaN, else clamped to 0..grid-1.
__device__ inline int cell_of(float v, float s, int grid) {
    const float c = v * s;
    if (c != c) return -1;
    if (c < 0.0f) return 0;
    if (c >= (float)grid) return grid - 1;
    return (int)c;
}

__global__ __launch_bounds__(kBlock) void scores_zero_kernel(int n_img, int* __restrict__ seen, unsigned long long* __restrict__ cover) {
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n_img; i += (long long)gridDim.x * kBlock) {
        seen[i] = 0;
        cover[i] = 0ull;
    }
}

template <bool kLds>
__global__ __launch_bounds__(kBlock) void scores_kernel(const int* __restrict__ counts, const int* __restrict__ node_track,
                                                        const unsigned char* __restrict__ has_point, const int* __restrict__ img_off, int n_img,
                                                        const float* __restrict__ kp, int n, int track_cap, float sx, float sy, int grid,
                                                        long long nblocks, int* __restrict__ seen, unsigned long long* __restrict__ cover) {
    __shared__ int s_seen[kLds ? kLdsImages : 1];
    __shared__ unsigned long long s_cover[kLds ? kLdsImages : 1];
    const int T = clamped(counts, n, track_cap).T;
    const int tid = threadIdx.x;
    if (kLds) {
        s_seen[tid] = 0;
        s_cover[tid] = 0ull;
        __syncthreads();
    }
    for (long long blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const long long u = blk * kBlock + tid;
        int t;
        if (u < n && has_point_of((int)u, node_track, has_point, T, &t)) {
            const int i = image_of(img_off, n_img, (int)u);                            // 0..n_img-1 (kLds: n_img <= kLdsImages)
            const int cx = cell_of(kp[2 * u + 0], sx, grid), cy = cell_of(kp[2 * u + 1], sy, grid);
            const unsigned long long bit = cx >= 0 && cy >= 0 ? 1ull << (cy * grid + cx) : 0ull;   // cy * grid + cx <= 63
            if (kLds) {
                atomicAdd(&s_seen[i], 1);
                if (bit) atomicOr(&s_cover[i], bit);
            } else {
                atomicAdd(&seen[i], 1);
                if (bit) atomicOr(&cover[i], bit);
            }
        }
    }
    if (kLds) {
        __syncthreads();
        if (tid < n_img) {
            if (s_seen[tid]) atomicAdd(&seen[tid], s_seen[tid]);
            if (s_cover[tid]) atomicOr(&cover[tid], s_cover[tid]);
        }
    }
}

__global__ __launch_bounds__(kBlock) void scores_cells_kernel(int n_img, const unsigned long long* __restrict__ cover, int* __restrict__ cells) {
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n_img; i += (long long)gridDim.x * kBlock) cells[i] = __popcll(cover[i]);
}

// ---- correspondences ------------------------------------------------------------------------------------------------------

struct ImageRange {
    int lo, hi;
};

__device__ inline ImageRange range_of(const int* __restrict__ img_off, int image, int n) {
    ImageRange r;
    r.lo = min(max(img_off[image], 0), n);
    r.hi = min(max(img_off[image + 1], r.lo), n);
    return r;
}

__global__ __launch_bounds__(kBlock) void corr_count_kernel(const int* __restrict__ counts, const int* __restrict__ node_track,
                                                            const unsigned char* __restrict__ has_point, const int* __restrict__ img_off, int image,
                                                            int n, int track_cap, long long nblocks, int* __restrict__ part) {
    __shared__ int lds[kWaves];
    const int T = clamped(counts, n, track_cap).T;
    const ImageRange rg = range_of(img_off, image, n);
    for (long long blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const long long u = (long long)rg.lo + blk * kBlock + threadIdx.x;
        int t;
        const int has = u < rg.hi && has_point_of((int)u, node_track, has_point, T, &t);
        const int s = block_sum(has, lds);
        if (threadIdx.x == 0) part[blk] = s;
    }
}

__global__ __launch_bounds__(kScanThreads) void corr_scan_kernel(int* __restrict__ part, long long nblocks, int* __restrict__ count_out) {
    __shared__ int buf[kScanThreads];
    const int total = scan_parts(part, nblocks, true, buf);
    if (threadIdx.x == kScanThreads - 1) count_out[0] = total;
}

__global__ __launch_bounds__(kBlock) void corr_place_kernel(const int* __restrict__ counts, const int* __restrict__ node_track,
                                                            const unsigned char* __restrict__ has_point, const unsigned* __restrict__ X_full,
                                                            const int* __restrict__ img_off, int image, const unsigned* __restrict__ kp, int n,
                                                            int track_cap, long long nblocks, const int* __restrict__ part, long long capacity,
                                                            unsigned* __restrict__ X_out, unsigned* __restrict__ uv_out, int* __restrict__ track_out) {
    __shared__ int scan[kBlock];
    const int T = clamped(counts, n, track_cap).T;
    const ImageRange rg = range_of(img_off, image, n);
    for (long long blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const long long u = (long long)rg.lo + blk * kBlock + threadIdx.x;
        int t = -1;
        const int has = u < rg.hi && has_point_of((int)u, node_track, has_point, T, &t);
        const int rank = block_scan(has, scan);
        const long long r = (long long)part[blk] + rank - 1;
        if (has && r >= 0 && r < capacity) {
            X_out[3 * r + 0] = X_full[3 * (size_t)t + 0];
            X_out[3 * r + 1] = X_full[3 * (size_t)t + 1];
            X_out[3 * r + 2] = X_full[3 * (size_t)t + 2];
            uv_out[2 * r + 0] = kp[2 * u + 0];
            uv_out[2 * r + 1] = kp[2 * u + 1];
            track_out[r] = t;
        }
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------

int64_t blocks_of(int64_t n, int block = kBlock) { return (n + block - 1) / block; }

unsigned grid_of(int64_t blocks) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks, kMaxGrid)); }

bool count_ok(int64_t n) { return n >= 0 && n <= kMaxCount; }

bool images_ok(int n_img) { return n_img >= 1 && n_img <= kMaxImages; }

RestrictWs carve_restrict(void* base, int64_t n) {
    sfm::Carver c(base);
    RestrictWs w{};
    const int64_t cap = n / 2 + 1;
    w.keep = c.take<int>(cap);
    w.part_t = c.take<int>(blocks_of(cap));
    w.part_o = c.take<int>(blocks_of(cap));
    w.part_s = c.take<int>(blocks_of(cap));
    w.part_d = c.take<int>(blocks_of(cap));
    w.bytes = c.used();
    return w;
}

struct CorrWs {
    int* part;
    size_t bytes;
};

CorrWs carve_corr(void* base, int64_t n) {
    sfm::Carver c(base);
    CorrWs w{};
    w.part = c.take<int>(std::max<int64_t>(1, blocks_of(n)));
    w.bytes = c.used();
    return w;
}

}  // namespace

extern "C" size_t sfm_track_restrict_ws_bytes(int64_t n_nodes) { return count_ok(n_nodes) ? carve_restrict(nullptr, n_nodes).bytes : 0; }

extern "C" int sfm_track_restrict(const int32_t* counts_dev, const int32_t* track_off_dev, const int32_t* obs_node_dev, const int32_t* img_off_dev,
                                  int n_img, int64_t n_nodes, const uint8_t* registered_dev, int64_t min_len, int32_t* track_off2_dev,
                                  int32_t* obs_node2_dev, int32_t* track_src_dev, int32_t* counts2_dev, void* ws_dev, size_t ws_bytes, void* stream) {
    SFM_CHECK_ARG(count_ok(n_nodes), "sfm_track_restrict: n_nodes %lld must be in 0..2^31-1", (long long)n_nodes);
    SFM_CHECK_ARG(images_ok(n_img), "sfm_track_restrict: n_img %d must be in 1..%d", n_img, kMaxImages);
    SFM_CHECK_ARG(min_len >= 1 && min_len <= kMaxCount, "sfm_track_restrict: min_len %lld must be in 1..2^31-1", (long long)min_len);
    SFM_CHECK_ARG(counts_dev && track_off_dev && img_off_dev && registered_dev && track_off2_dev && track_src_dev && counts2_dev && ws_dev &&
                      (n_nodes == 0 || (obs_node_dev && obs_node2_dev)),
                  "sfm_track_restrict: null required pointer");
    const RestrictWs ws = carve_restrict(ws_dev, n_nodes);
    SFM_CHECK_ARG(ws_bytes >= ws.bytes, "sfm_track_restrict: workspace %zu bytes < %zu", ws_bytes, ws.bytes);
    const int n = (int)n_nodes, track_cap = (int)(n_nodes / 2 + 1);
    const long long nblocks = blocks_of(track_cap);
    hipStream_t s = sfm::as_stream(stream);
    const dim3 block(kBlock), grid(grid_of(nblocks));
    hipLaunchKernelGGL(restrict_count_kernel, grid, block, 0, s, counts_dev, track_off_dev, obs_node_dev, img_off_dev, n_img, registered_dev, n,
                       track_cap, (long long)min_len, nblocks, ws);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(restrict_scan_kernel, dim3(4), dim3(kScanThreads), 0, s, ws, nblocks, counts2_dev);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(restrict_place_kernel, grid, block, 0, s, counts_dev, track_off_dev, obs_node_dev, img_off_dev, n_img, registered_dev, n,
                       track_cap, nblocks, ws, counts2_dev, track_off2_dev, obs_node2_dev, track_src_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" int sfm_track_adopt(const int32_t* counts_dev, const int32_t* track_off_dev, const int32_t* obs_node_dev, int64_t n_nodes,
                               const int32_t* counts_r_dev, const int32_t* track_src_r_dev, const int32_t* counts_p_dev,
                               const int32_t* track_off_p_dev, const int32_t* obs_node_p_dev, const float* X_p_dev, const int32_t* track_src_p_dev,
                               float* X_full_dev, uint8_t* has_point_dev, uint8_t* obs_live_dev, void* stream) {
    SFM_CHECK_ARG(count_ok(n_nodes), "sfm_track_adopt: n_nodes %lld must be in 0..2^31-1", (long long)n_nodes);
    SFM_CHECK_ARG(counts_dev && track_off_dev && counts_r_dev && track_src_r_dev && counts_p_dev && track_off_p_dev && X_p_dev && track_src_p_dev &&
                      X_full_dev && has_point_dev && (n_nodes == 0 || (obs_node_dev && obs_node_p_dev && obs_live_dev)),
                  "sfm_track_adopt: null required pointer");
    const int n = (int)n_nodes, track_cap = (int)(n_nodes / 2 + 1);
    hipStream_t s = sfm::as_stream(stream);
    const long long clear_blocks = blocks_of(std::max<int64_t>(track_cap, n)), nblocks = blocks_of(track_cap);
    hipLaunchKernelGGL(adopt_clear_kernel, dim3(grid_of(clear_blocks)), dim3(kBlock), 0, s, counts_dev, n, track_cap, clear_blocks,
                       reinterpret_cast<unsigned*>(X_full_dev), has_point_dev, obs_live_dev);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(adopt_place_kernel, dim3(grid_of(nblocks)), dim3(kBlock), 0, s, counts_dev, track_off_dev, obs_node_dev, n, track_cap,
                       counts_r_dev, track_src_r_dev, counts_p_dev, track_off_p_dev, obs_node_p_dev, reinterpret_cast<const unsigned*>(X_p_dev),
                       track_src_p_dev, nblocks, reinterpret_cast<unsigned*>(X_full_dev), has_point_dev, obs_live_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" int sfm_track_view_scores(const int32_t* counts_dev, const int32_t* node_track_dev, const uint8_t* has_point_dev,
                                     const int32_t* img_off_dev, int n_img, const float* kp_dev, int64_t n_nodes, double width, double height,
                                     int grid, int32_t* seen_dev, uint64_t* cover_dev, int32_t* cells_dev, void* stream) {
    SFM_CHECK_ARG(count_ok(n_nodes), "sfm_track_view_scores: n_nodes %lld must be in 0..2^31-1", (long long)n_nodes);
    SFM_CHECK_ARG(images_ok(n_img), "sfm_track_view_scores: n_img %d must be in 1..%d", n_img, kMaxImages);
    SFM_CHECK_ARG(grid >= 1 && grid <= kMaxCells, "sfm_track_view_scores: grid %d must be in 1..%d", grid, kMaxCells);
    SFM_CHECK_ARG(width > 0.0 && height > 0.0 && std::isfinite(width) && std::isfinite(height),
                  "sfm_track_view_scores: frame size %g x %g must be finite and > 0", width, height);
    SFM_CHECK_ARG(counts_dev && has_point_dev && img_off_dev && seen_dev && cover_dev && cells_dev && (n_nodes == 0 || (node_track_dev && kp_dev)),
                  "sfm_track_view_scores: null required pointer");
    const int n = (int)n_nodes, track_cap = (int)(n_nodes / 2 + 1);
    const float sx = (float)grid / (float)width, sy = (float)grid / (float)height;
    const long long nblocks = blocks_of(n), iblocks = blocks_of(n_img);
    hipStream_t s = sfm::as_stream(stream);
    unsigned long long* cover = reinterpret_cast<unsigned long long*>(cover_dev);
    hipLaunchKernelGGL(scores_zero_kernel, dim3(grid_of(iblocks)), dim3(kBlock), 0, s, n_img, seen_dev, cover);
    SFM_CHECK_LAUNCH();
    if (n_img <= kLdsImages)
        hipLaunchKernelGGL(scores_kernel<true>, dim3(grid_of(nblocks)), dim3(kBlock), 0, s, counts_dev, node_track_dev, has_point_dev, img_off_dev,
                           n_img, kp_dev, n, track_cap, sx, sy, grid, nblocks, seen_dev, cover);
    else
        hipLaunchKernelGGL(scores_kernel<false>, dim3(grid_of(nblocks)), dim3(kBlock), 0, s, counts_dev, node_track_dev, has_point_dev, img_off_dev,
                           n_img, kp_dev, n, track_cap, sx, sy, grid, nblocks, seen_dev, cover);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(scores_cells_kernel, dim3(grid_of(iblocks)), dim3(kBlock), 0, s, n_img, cover, cells_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" size_t sfm_track_correspondences_ws_bytes(int64_t n_nodes) { return count_ok(n_nodes) ? carve_corr(nullptr, n_nodes).bytes : 0; }

extern "C" int sfm_track_correspondences(int image, const int32_t* counts_dev, const int32_t* node_track_dev, const uint8_t* has_point_dev,
                                         const float* X_full_dev, const int32_t* img_off_dev, int n_img, const float* kp_dev, int64_t n_nodes,
                                         int64_t capacity, float* X_out_dev, float* uv_out_dev, int32_t* track_out_dev, int32_t* count_dev,
                                         void* ws_dev, size_t ws_bytes, void* stream) {
    SFM_CHECK_ARG(count_ok(n_nodes), "sfm_track_correspondences: n_nodes %lld must be in 0..2^31-1", (long long)n_nodes);
    SFM_CHECK_ARG(images_ok(n_img), "sfm_track_correspondences: n_img %d must be in 1..%d", n_img, kMaxImages);
    SFM_CHECK_ARG(image >= 0 && image < n_img, "sfm_track_correspondences: image %d must be in 0..%d", image, n_img - 1);
    SFM_CHECK_ARG(count_ok(capacity), "sfm_track_correspondences: capacity %lld must be in 0..2^31-1", (long long)capacity);
    SFM_CHECK_ARG(counts_dev && has_point_dev && X_full_dev && img_off_dev && count_dev && ws_dev && (n_nodes == 0 || (node_track_dev && kp_dev)) &&
                      (capacity == 0 || (X_out_dev && uv_out_dev && track_out_dev)),
                  "sfm_track_correspondences: null required pointer");
    const CorrWs ws = carve_corr(ws_dev, n_nodes);
    SFM_CHECK_ARG(ws_bytes >= ws.bytes, "sfm_track_correspondences: workspace %zu bytes < %zu", ws_bytes, ws.bytes);
    const int n = (int)n_nodes, track_cap = (int)(n_nodes / 2 + 1);
    const long long nblocks = std::max<int64_t>(1, blocks_of(n));
    hipStream_t s = sfm::as_stream(stream);
    const dim3 block(kBlock), grid(grid_of(nblocks));
    hipLaunchKernelGGL(corr_count_kernel, grid, block, 0, s, counts_dev, node_track_dev, has_point_dev, img_off_dev, image, n, track_cap, nblocks,
                       ws.part);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(corr_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, ws.part, nblocks, count_dev);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(corr_place_kernel, grid, block, 0, s, counts_dev, node_track_dev, has_point_dev, reinterpret_cast<const unsigned*>(X_full_dev),
                       img_off_dev, image, reinterpret_cast<const unsigned*>(kp_dev), n, track_cap, nblocks, ws.part, (long long)capacity,
                       reinterpret_cast<unsigned*>(X_out_dev), reinterpret_cast<unsigned*>(uv_out_dev), track_out_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}
