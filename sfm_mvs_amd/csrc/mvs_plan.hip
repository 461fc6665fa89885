// Planning the MVS views from the sparse model (include/sfm_hip.h, "MVS-PLAN"; docs/mvs.md §8).
//   sfm_view_pair_counts   per pair of cameras: the tracks both see (shared) and, of those, the ones whose two rays open an angle inside
//                          the caller's window (good)
//   sfm_view_depth_ranges  per camera: the number of valid depths of the points it observes and two order statistics of them
//   sfm_view_select        per camera: the first nsrc partners by (good, shared, index)
// Every output word is a count, a rank, a copy or an order statistic: integer atomics only, no word depends on the order in which they
// land.  Every float64 operation is written in the header's order (the Makefile compiles with -ffp-contract=off); tests/np_mvs_plan.py
// restates every output word.  Every loop runs over a range fixed at launch (a clamped CSR row, ncam, nsrc) or a constant named here.
//
// Pair counts.  kGroup = 16 lanes own a track; a workgroup of 256 lanes takes 16 tracks a round, the rounds strided over the grid.  The
// rays of a track (camera, X - C, squared norm) are computed once per tile of kTile = 64 observations and kept in LDS; lane l of the
// group owns the first observations p = l, l + 16, ... of the pairs and walks the second ones q > p of the tile from a start that
// depends on the group, so that the groups of a wave which see the same cameras do not meet on one counter in the same instruction.
// While ncam <= SFM_PLAN_LDS_CAMS = 96 the counters are private to the workgroup: two upper triangles of ncam (ncam - 1) / 2 int32 in
// LDS (36 480 bytes at 96; with the 36 KiB of ray tiles a workgroup holds 72.6 KiB, so that 2 fit a CU's 160 KiB: 8 waves per
// CU), flushed by one global atomic per non-zero cell.  Above that every contribution is a global atomic on the upper
// triangle.  A last kernel mirrors the upper triangles into the lower ones.
//
// Depth ranges.  One workgroup per camera, a radix select over the uint32 view of the positive float32 depths: four passes of 8 bits,
// both ranks at once, two histograms of 256 int32 in LDS.  The depth of an observation is recomputed in every pass instead of being
// parked in a workspace: rows of cam_off that overlap (the CSR is not trusted) then cannot race, and the call needs no workspace.
//
// Select.  One wave per view: nsrc rounds, each finds the best partner that comes after the previous round's in the order (good
// descending, shared descending, index ascending) with a lane-strided scan of the row and a xor tree.
#include <algorithm>
#include <climits>
#include <cmath>

#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kGroup = SFM_PLAN_GROUP;          // lanes per track
constexpr int kGroups = kBlock / kGroup;        // tracks per workgroup and round
constexpr int kTile = 64;                       // observations of a track whose rays are in LDS at a time
constexpr int kLdsCams = SFM_PLAN_LDS_CAMS;
constexpr int kLdsCells = kLdsCams * (kLdsCams - 1) / 2;
constexpr int kPairGrid = 512;                  // workgroups of the pair kernel at the most: 2 per CU
constexpr int kMaxCams = 4096;
constexpr int64_t kMaxCount = INT32_MAX;
constexpr double kDblMax = 1.7976931348623157e308;
constexpr unsigned kInfBits = 0x7F800000u;

__device__ inline bool in_range(int a, int n) { return (unsigned)a < (unsigned)n; }

__device__ inline bool finite(double v) { return fabs(v) <= kDblMax; }

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- camera centres (the formula of csrc/tracks_refine.hip's centres_kernel) ----------------------------------------------------

__global__ __launch_bounds__(kBlock) void plan_centres_kernel(const double* __restrict__ P, int ncam, double* __restrict__ C) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= ncam) return;
    const double* p = P + 12 * (size_t)i;
    const double p0 = p[0], p1 = p[1], p2 = p[2], p3 = p[3], p4 = p[4], p5 = p[5], p6 = p[6], p7 = p[7], p8 = p[8], p9 = p[9], p10 = p[10], p11 = p[11];
    const double a00 = p5 * p10 - p6 * p9, a01 = p2 * p9 - p1 * p10, a02 = p1 * p6 - p2 * p5;
    const double a10 = p6 * p8 - p4 * p10, a11 = p0 * p10 - p2 * p8, a12 = p2 * p4 - p0 * p6;
    const double a20 = p4 * p9 - p5 * p8, a21 = p1 * p8 - p0 * p9, a22 = p0 * p5 - p1 * p4;
    const double det = (p0 * a00 + p1 * a10) + p2 * a20;
    C[3 * (size_t)i + 0] = -(((a00 * p3 + a01 * p7) + a02 * p11) / det);
    C[3 * (size_t)i + 1] = -(((a10 * p3 + a11 * p7) + a12 * p11) / det);
    C[3 * (size_t)i + 2] = -(((a20 * p3 + a21 * p7) + a22 * p11) / det);
}

// ---- pair counts ----------------------------------------------------------------------------------------------------------------

struct Ray { double x, y, z, n; };

__device__ __forceinline__ Ray ray_of(const double* __restrict__ C, int cam, double x0, double x1, double x2) {
    Ray r;
    r.x = x0 - C[3 * (size_t)cam + 0];
    r.y = x1 - C[3 * (size_t)cam + 1];
    r.z = x2 - C[3 * (size_t)cam + 2];
    r.n = (r.x * r.x + r.y * r.y) + r.z * r.z;
    return r;
}

// The cell of the pair a < b in an upper triangle stored row by row.
__device__ __forceinline__ int cell_of(int a, int b, int ncam) { return a * (2 * ncam - a - 1) / 2 + (b - a - 1); }

template <bool kLds>
__global__ __launch_bounds__(kBlock) void pair_counts_kernel(const int* __restrict__ track_off, const int* __restrict__ cam_idx,
                                                             const double* __restrict__ X, const double* __restrict__ C, int npt, int nobs, int ncam,
                                                             double cos_lo, double cos_hi, unsigned* __restrict__ shared, unsigned* __restrict__ good) {
    __shared__ double s_ray[kGroups][4][kTile];                                  // [group][x, y, z, n][slot]
    __shared__ int s_cam[kGroups][kTile];
    __shared__ int s_len[kGroups];
    __shared__ unsigned s_cnt[kLds ? 2 * kLdsCells : 1];
    const int tid = threadIdx.x, g = tid / kGroup, l = tid % kGroup;
    const int ncell = ncam * (ncam - 1) / 2;
    if (kLds) {
        for (int i = tid; i < 2 * ncell; i += kBlock) s_cnt[i] = 0u;
    }
    const int rounds = npt / kGroups + (npt % kGroups != 0);
    for (int round = blockIdx.x; round < rounds; round += gridDim.x) {          // uniform over the workgroup
        const int64_t t = (int64_t)round * kGroups + g;
        int lo = 0, hi = 0;
        double x0 = 0.0, x1 = 0.0, x2 = 0.0;
        if (t < npt) {
            lo = clampi(track_off[t], 0, nobs);
            hi = clampi(track_off[t + 1], lo, nobs);
            x0 = X[3 * (size_t)t + 0]; x1 = X[3 * (size_t)t + 1]; x2 = X[3 * (size_t)t + 2];
        }
        const bool x_ok = finite(x0) && finite(x1) && finite(x2);
        __syncthreads();                                                        // the counters are zero; the previous round has read s_len
        if (l == 0) s_len[g] = hi - lo;
        __syncthreads();
        int longest = 0;
        for (int k = 0; k < kGroups; ++k) longest = max(longest, s_len[k]);
        const int tiles = longest / kTile + (longest % kTile != 0);                        // uniform over the workgroup
        for (int tile = 0; tile < tiles; ++tile) {
            const int t0 = lo + min(tile * (int64_t)kTile, (int64_t)(hi - lo)), t1 = t0 + min(kTile, hi - t0);      // this group's slice: q in t0..t1-1
            __syncthreads();                                                    // the previous tile has been read
            for (int slot = l; slot < t1 - t0; slot += kGroup) {
                const int q = t0 + slot;
                const int cam = cam_idx[q];
                const bool ok = in_range(cam, ncam);
                const Ray r = ok ? ray_of(C, cam, x0, x1, x2) : Ray{0.0, 0.0, 0.0, 0.0};
                s_cam[g][slot] = ok ? cam : -1;
                s_ray[g][0][slot] = r.x; s_ray[g][1][slot] = r.y; s_ray[g][2][slot] = r.z; s_ray[g][3][slot] = r.n;
            }
            __syncthreads();
            // first observations: every p < t1 - 1 of the row that lane l owns; its ray from the tile when it lies in it
            for (int64_t p64 = (int64_t)lo + l; t1 > t0 && p64 < t1 - 1; p64 += kGroup) {
                const int p = (int)p64;
                int a;
                Ray ra;
                if (p >= t0) {
                    const int slot = p - t0;
                    a = s_cam[g][slot];
                    ra = Ray{s_ray[g][0][slot], s_ray[g][1][slot], s_ray[g][2][slot], s_ray[g][3][slot]};
                } else {
                    a = cam_idx[p];
                    a = in_range(a, ncam) ? a : -1;
                    ra = a >= 0 ? ray_of(C, a, x0, x1, x2) : Ray{0.0, 0.0, 0.0, 0.0};
                }
                if (a < 0) continue;
                const int qs = max(p + 1, t0), cnt = t1 - qs;                   // cnt >= 1
                int q = qs + (g * 5) % cnt;
                for (int k = 0; k < cnt; ++k) {
                    const int slot = q - t0;
                    const int b = s_cam[g][slot];
                    if (b >= 0 && b != a) {
                        const double dot = (ra.x * s_ray[g][0][slot] + ra.y * s_ray[g][1][slot]) + ra.z * s_ray[g][2][slot];
                        const double c = dot / sqrt(ra.n * s_ray[g][3][slot]);
                        const bool is_good = x_ok && c >= cos_lo && c <= cos_hi;  // a NaN fails both
                        const int cell = a < b ? cell_of(a, b, ncam) : cell_of(b, a, ncam);
                        if (kLds) {
                            atomicAdd(&s_cnt[cell], 1u);
                            if (is_good) atomicAdd(&s_cnt[ncell + cell], 1u);
                        } else {
                            const size_t at = a < b ? (size_t)a * ncam + b : (size_t)b * ncam + a;
                            atomicAdd(&shared[at], 1u);
                            if (is_good) atomicAdd(&good[at], 1u);
                        }
                    }
                    if (++q == t1) q = qs;
                }
            }
        }
    }
    if (kLds) {
        __syncthreads();
        for (int i = tid; i < ncam * ncam; i += kBlock) {
            const int a = i / ncam, b = i - a * ncam;
            if (a >= b) continue;
            const int cell = cell_of(a, b, ncam);
            const unsigned s = s_cnt[cell], gd = s_cnt[ncell + cell];
            if (s) atomicAdd(&shared[i], s);
            if (gd) atomicAdd(&good[i], gd);
        }
    }
}

__global__ __launch_bounds__(kBlock) void mirror_kernel(unsigned* __restrict__ shared, unsigned* __restrict__ good, int ncam) {
    const int64_t total = (int64_t)ncam * ncam;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int a = (int)(i / ncam), b = (int)(i - (int64_t)a * ncam);
        if (a > b) {
            shared[i] = shared[(size_t)b * ncam + a];
            good[i] = good[(size_t)b * ncam + a];
        }
    }
}

// ---- depth ranges ---------------------------------------------------------------------------------------------------------------

// The uint32 view of the depth of row entry k of camera `cam`, 0 when the entry or the depth is not valid.
__device__ __forceinline__ unsigned depth_bits(const int* __restrict__ cam_obs, const int* __restrict__ cam_idx, const int* __restrict__ pt_idx,
                                               const double* __restrict__ X, int nobs, int npt, int cam, double p8, double p9, double p10, double p11,
                                               int k, int hi) {
    if (k >= hi) return 0u;
    const int o = cam_obs[k];
    if (!in_range(o, nobs) || cam_idx[o] != cam) return 0u;
    const int j = pt_idx[o];
    if (!in_range(j, npt)) return 0u;
    const double z = ((p8 * X[3 * (size_t)j + 0] + p9 * X[3 * (size_t)j + 1]) + p10 * X[3 * (size_t)j + 2]) + p11;
    const unsigned u = __float_as_uint((float)z);
    return (u > 0u && u < kInfBits) ? u : 0u;                                    // positive, finite, not zero (a NaN or a negative sign is above)
}

__global__ __launch_bounds__(kBlock) void depth_ranges_kernel(const int* __restrict__ cam_off, const int* __restrict__ cam_obs,
                                                              const int* __restrict__ cam_idx, const int* __restrict__ pt_idx, const double* __restrict__ X,
                                                              const double* __restrict__ P, int nobs, int npt, int lo_pm, int hi_pm,
                                                              int* __restrict__ m_out, float* __restrict__ z_lo, float* __restrict__ z_hi) {
    __shared__ int s_hist[2][kBlock];
    __shared__ int s_scan[2][2][kBlock];
    __shared__ int s_bin[2], s_rank[2];
    const int cam = blockIdx.x, tid = threadIdx.x;
    const int lo = clampi(cam_off[cam], 0, nobs), hi = clampi(cam_off[cam + 1], lo, nobs);
    const double p8 = P[12 * (size_t)cam + 8], p9 = P[12 * (size_t)cam + 9], p10 = P[12 * (size_t)cam + 10], p11 = P[12 * (size_t)cam + 11];
    unsigned prefix[2] = {0u, 0u};
    int rank[2] = {0, 0};
    int m = 0;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const unsigned known = pass == 0 ? 0u : 0xFFFFFFFFu << (shift + 8);     // the bits the earlier passes fixed
        s_hist[0][tid] = 0; s_hist[1][tid] = 0;
        __syncthreads();
        for (int64_t base = lo; base < hi; base += 4 * kBlock) {                    // four entries a lane: their loads are in flight together
            unsigned u[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t k = base + e * kBlock + tid;
                u[e] = k < hi ? depth_bits(cam_obs, cam_idx, pt_idx, X, nobs, npt, cam, p8, p9, p10, p11, (int)k, hi) : 0u;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (u[e] == 0u) continue;
                const int digit = (int)((u[e] >> shift) & 255u);
                if ((u[e] & known) == prefix[0]) atomicAdd(&s_hist[0][digit], 1);
                if ((u[e] & known) == prefix[1]) atomicAdd(&s_hist[1][digit], 1);
            }
        }
        __syncthreads();
        // inclusive scan of both histograms (256 bins, a bin per lane)
        int cur = 0;
        s_scan[0][0][tid] = s_hist[0][tid]; s_scan[1][0][tid] = s_hist[1][tid];
        __syncthreads();
        for (int step = 1; step < kBlock; step <<= 1) {
            const int a = s_scan[0][cur][tid] + (tid >= step ? s_scan[0][cur][tid - step] : 0);
            const int b = s_scan[1][cur][tid] + (tid >= step ? s_scan[1][cur][tid - step] : 0);
            s_scan[0][cur ^ 1][tid] = a; s_scan[1][cur ^ 1][tid] = b;
            cur ^= 1;
            __syncthreads();
        }
        if (pass == 0) {
            m = s_scan[0][cur][kBlock - 1];                                     // every valid depth is in the first pass's histogram
            if (m == 0) break;                                                  // uniform over the workgroup
            rank[0] = (int)(((int64_t)lo_pm * (m - 1)) / 1000);
            rank[1] = (int)(((int64_t)hi_pm * (m - 1) + 999) / 1000);
        }
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            const int incl = s_scan[w][cur][tid], excl = incl - s_hist[w][tid];
            if (excl <= rank[w] && rank[w] < incl) { s_bin[w] = tid; s_rank[w] = rank[w] - excl; }     // one lane: 0 <= rank < the total
        }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            prefix[w] |= (unsigned)s_bin[w] << shift;
            rank[w] = s_rank[w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        m_out[cam] = m;
        z_lo[cam] = m ? __uint_as_float(prefix[0]) : 0.0f;
        z_hi[cam] = m ? __uint_as_float(prefix[1]) : 0.0f;
    }
}

// ---- select ---------------------------------------------------------------------------------------------------------------------

struct Cand { int g, s, j; };                                                    // j < 0: none

// a comes before b in the order good descending, shared descending, index ascending; a candidate comes before none
__device__ __forceinline__ bool before(const Cand& a, const Cand& b) {
    if (a.j < 0) return false;
    if (b.j < 0) return true;
    if (a.g != b.g) return a.g > b.g;
    if (a.s != b.s) return a.s > b.s;
    return a.j < b.j;
}

__global__ __launch_bounds__(kBlock) void select_kernel(const int* __restrict__ shared, const int* __restrict__ good, int ncam, int nsrc, int min_good,
                                                        int* __restrict__ nbr, int* __restrict__ n_nbr) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (i >= ncam) return;                                                       // a whole wave
    const int* grow = good + (size_t)i * ncam;
    const int* srow = shared + (size_t)i * ncam;
    Cand last{0, 0, -1};
    int found = 0;
    for (int k = 0; k < nsrc; ++k) {
        Cand best{0, 0, -1};
        for (int j = lane; j < ncam; j += 64) {
            const Cand c{grow[j], srow[j], j};
            if (j == i || c.g < min_good) continue;
            if (last.j >= 0 && !before(last, c)) continue;                       // taken by an earlier round, or the last one itself
            if (before(c, best)) best = c;
        }
        for (int step = 32; step >= 1; step >>= 1) {
            const Cand o{__shfl_xor(best.g, step), __shfl_xor(best.s, step), __shfl_xor(best.j, step)};
            if (before(o, best)) best = o;
        }
        if (lane == 0) nbr[(size_t)i * nsrc + k] = best.j;                       // -1 pads
        if (best.j < 0) {                                                        // uniform over the wave: nothing is left
            for (int r = k + 1 + lane; r < nsrc; r += 64) nbr[(size_t)i * nsrc + r] = -1;
            break;
        }
        last = best;
        ++found;
    }
    if (lane == 0) n_nbr[i] = found;
}

int grid_for(int64_t items, int per_block, int cap) { return (int)std::max<int64_t>(1, std::min<int64_t>((items + per_block - 1) / per_block, cap)); }

}  // namespace

extern "C" int sfm_view_pair_counts(const int32_t* track_off_dev, const int32_t* cam_idx_dev, const double* X_dev, int64_t npt, int64_t nobs,
                                    const double* P_dev, int64_t ncam, double cos_lo, double cos_hi, double* C_dev, int32_t* shared_dev,
                                    int32_t* good_dev, void* stream) {
    SFM_CHECK_ARG(ncam >= 1 && ncam <= kMaxCams && npt >= 0 && npt <= kMaxCount && nobs >= 0 && nobs <= kMaxCount,
                  "sfm_view_pair_counts: sizes out of range (ncam %lld in 1..4096, npt %lld, nobs %lld in 0..2^31-1)", (long long)ncam, (long long)npt,
                  (long long)nobs);
    SFM_CHECK_ARG(cos_lo == cos_lo && cos_hi == cos_hi, "sfm_view_pair_counts: a NaN cosine bound");
    SFM_CHECK_ARG(track_off_dev && P_dev && C_dev && shared_dev && good_dev && (npt == 0 || X_dev) && (nobs == 0 || cam_idx_dev),
                  "sfm_view_pair_counts: null pointer");
    hipStream_t s = sfm::as_stream(stream);
    const size_t bytes = (size_t)ncam * ncam * sizeof(int32_t);
    SFM_CHECK_HIP(hipMemsetAsync(shared_dev, 0, bytes, s));
    SFM_CHECK_HIP(hipMemsetAsync(good_dev, 0, bytes, s));
    hipLaunchKernelGGL(plan_centres_kernel, dim3(grid_for(ncam, kBlock, 1 << 16)), dim3(kBlock), 0, s, P_dev, (int)ncam, C_dev);
    SFM_CHECK_LAUNCH();
    if (npt > 0 && nobs > 0 && ncam > 1) {
        const dim3 grid(grid_for(npt, kGroups, kPairGrid));
        unsigned* sh = reinterpret_cast<unsigned*>(shared_dev);
        unsigned* gd = reinterpret_cast<unsigned*>(good_dev);
        if (ncam <= kLdsCams)
            hipLaunchKernelGGL(pair_counts_kernel<true>, grid, dim3(kBlock), 0, s, track_off_dev, cam_idx_dev, X_dev, C_dev, (int)npt, (int)nobs, (int)ncam,
                               cos_lo, cos_hi, sh, gd);
        else
            hipLaunchKernelGGL(pair_counts_kernel<false>, grid, dim3(kBlock), 0, s, track_off_dev, cam_idx_dev, X_dev, C_dev, (int)npt, (int)nobs, (int)ncam,
                               cos_lo, cos_hi, sh, gd);
        SFM_CHECK_LAUNCH();
        hipLaunchKernelGGL(mirror_kernel, dim3(grid_for(ncam * ncam, kBlock, 1024)), dim3(kBlock), 0, s, sh, gd, (int)ncam);
        SFM_CHECK_LAUNCH();
    }
    return SFM_OK;
}

extern "C" int sfm_view_depth_ranges(const int32_t* cam_off_dev, const int32_t* cam_obs_dev, const int32_t* cam_idx_dev, const int32_t* pt_idx_dev,
                                     int64_t nobs, const double* X_dev, int64_t npt, const double* P_dev, int64_t ncam, int lo_permille, int hi_permille,
                                     int32_t* m_dev, float* z_lo_dev, float* z_hi_dev, void* stream) {
    SFM_CHECK_ARG(ncam >= 1 && ncam <= kMaxCams && npt >= 0 && npt <= kMaxCount && nobs >= 0 && nobs <= kMaxCount,
                  "sfm_view_depth_ranges: sizes out of range (ncam %lld in 1..4096, npt %lld, nobs %lld in 0..2^31-1)", (long long)ncam, (long long)npt,
                  (long long)nobs);
    SFM_CHECK_ARG(0 <= lo_permille && lo_permille <= hi_permille && hi_permille <= 1000,
                  "sfm_view_depth_ranges: permille bounds need 0 <= lo <= hi <= 1000 (got %d, %d)", lo_permille, hi_permille);
    SFM_CHECK_ARG(cam_off_dev && P_dev && m_dev && z_lo_dev && z_hi_dev && (npt == 0 || X_dev) && (nobs == 0 || (cam_obs_dev && cam_idx_dev && pt_idx_dev)),
                  "sfm_view_depth_ranges: null pointer");
    hipLaunchKernelGGL(depth_ranges_kernel, dim3((int)ncam), dim3(kBlock), 0, sfm::as_stream(stream), cam_off_dev, cam_obs_dev, cam_idx_dev, pt_idx_dev,
                       X_dev, P_dev, (int)nobs, (int)npt, lo_permille, hi_permille, m_dev, z_lo_dev, z_hi_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" int sfm_view_select(const int32_t* shared_dev, const int32_t* good_dev, int64_t ncam, int nsrc, int min_good, int32_t* nbr_dev,
                               int32_t* n_nbr_dev, void* stream) {
    SFM_CHECK_ARG(ncam >= 1 && ncam <= kMaxCams, "sfm_view_select: sizes out of range (ncam %lld in 1..4096)", (long long)ncam);
    SFM_CHECK_ARG(nsrc >= 1 && nsrc <= SFM_PLAN_MAX_SRC, "sfm_view_select: nsrc %d outside 1..%d", nsrc, SFM_PLAN_MAX_SRC);
    SFM_CHECK_ARG(min_good >= 0, "sfm_view_select: min_good %d is negative", min_good);
    SFM_CHECK_ARG(shared_dev && good_dev && nbr_dev && n_nbr_dev, "sfm_view_select: null pointer");
    hipLaunchKernelGGL(select_kernel, dim3(grid_for(ncam, kBlock / 64, 1 << 16)), dim3(kBlock), 0, sfm::as_stream(stream), shared_dev, good_dev, (int)ncam,
                       nsrc, min_good, nbr_dev, n_nbr_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}
