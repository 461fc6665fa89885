// Robust refinement and pruning of feature tracks (include/sfm_hip.h, "TRACKS-REFINE"; docs/tracks.md §8).
//   sfm_track_refine   one lane per track: Levenberg-Marquardt on the Huber cost of the reprojection error from the DLT point, inlier
//                      flags per observation, a second least-squares phase on the inliers, the smallest cosine between inlier rays
//   sfm_track_prune    keeps the tracks that pass (flags, inliers, largest error, cosine) and of those the inlier observations, ranked
//                      by per-block counts and a one-workgroup scan: the output has the shape sfm_track_build leaves
// Every float64 operation is written in the header's order (the Makefile compiles with -ffp-contract=off); tests/np_tracks_refine.py
// restates every output word.  The helpers image_of and the scan are copies of csrc/tracks.hip's, as the mesh files copy theirs.
//
// Refinement.  A lane walks its track's observations once per pass: a start pass, per attempt an accumulation pass (only after the
// point moved) and a trial pass, the inlier pass, the final pass.  The state of an observation between passes is ONE int32 word kept
// in the row of depth_dev the final pass overwrites: image >= 0 while the observation takes part, -2 - image once it does not, -1 for a
// node outside 0..N-1; so the binary search over img_off runs once per observation and the passes load one word instead of three.
// Every read of that word is checked against n_img (and its node against N): the ranges of two tracks must not overlap, and where
// they do the words are unspecified, but nothing is read or written outside the arrays (Track::active, the final pass).
// A, g, x and the Jacobian rows are scalars in registers; the image indices of the first 64 inliers go through LDS ([slot][lane], no
// bank conflict) for the pair loop of the angle, because a register array indexed by the loop counter would go to scratch.
// Every loop runs over a range fixed at launch or bounded by a constant named here.
#include <algorithm>
#include <climits>

#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kLanes = 64;                      // threads per workgroup of refine_kernel: one wave, 8 KiB of LDS
constexpr int kMaxGrid = 1 << 16;               // workgroups per launch; the kernels stride over what is left
constexpr int kScanThreads = 1024;
constexpr int64_t kMaxCount = INT32_MAX;
constexpr int kMaxImages = 65536;
constexpr int kSearchSteps = 17;                // binary search over at most 65 537 offsets
constexpr int kMaxIters = 50;
constexpr int kAngleCap = 64;                   // inliers whose rays enter the pair loop
constexpr unsigned kQuietNan = 0x7FC00000u;
constexpr double kLam0 = 1e-3;
constexpr double kDblMax = 1.7976931348623157e308;
constexpr float kFltMax = 3.4028234663852886e38f;

__device__ inline bool in_range(int a, int n) { return (unsigned)a < (unsigned)n; }

__device__ inline bool finite(double v) { return fabs(v) <= kDblMax; }

__device__ inline float canonical(float v) { return v != v ? __uint_as_float(kQuietNan) : v; }

// The image of node u: the largest i < n_img with img_off[i] <= u.
__device__ inline int image_of(const int* __restrict__ img_off, int n_img, int u) {
    int lo = 0, hi = n_img;                                                     // img_off[lo] <= u < img_off[hi]
    for (int step = 0; step < kSearchSteps && hi - lo > 1; ++step) {
        const int mid = lo + ((hi - lo) >> 1);
        if (img_off[mid] <= u) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- camera centres -------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock) void centres_kernel(const double* __restrict__ P, int n_img, double* __restrict__ C) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_img) return;
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

// ---- refinement -----------------------------------------------------------------------------------------------------------

struct Point { double x, y, z; };

struct Proj { double h0, h1, h2; };

__device__ __forceinline__ Proj project(const double* __restrict__ Pi, const Point& q) {
    Proj h;
    h.h0 = ((Pi[0] * q.x + Pi[1] * q.y) + Pi[2] * q.z) + Pi[3];
    h.h1 = ((Pi[4] * q.x + Pi[5] * q.y) + Pi[6] * q.z) + Pi[7];
    h.h2 = ((Pi[8] * q.x + Pi[9] * q.y) + Pi[10] * q.z) + Pi[11];
    return h;
}

template <bool kHuber> __device__ __forceinline__ double rho(double e, double huber) {
    if (!kHuber) return (e * e) / 2.0;
    return e <= huber ? (e * e) / 2.0 : huber * (e - huber / 2.0);
}

struct Track {
    const int* obs_node;
    const float* kp;
    const double* P;
    int* word;                                   // the rows of depth_dev as int32: the state of an observation between passes
    int lo, hi, n, n_img;
    // The image of row o while its observation takes part, else -1; u = its node.  The word is CHECKED every time it is read: where the
    // ranges of two tracks overlap (offsets no sfm_track_build left) another lane may have written anything into the row, a depth's
    // bits included, and what is read here indexes P, kp and the centres.
    __device__ __forceinline__ int active(int o, int& u) const {
        const int w = word[o];
        u = obs_node[o];
        return in_range(w, n_img) && in_range(u, n) ? w : -1;
    }
};

// `iters` attempts of Levenberg-Marquardt from x with cost `cost` over the observations whose word is >= 0.
template <bool kHuber>
__device__ __forceinline__ void lm_phase(const Track& tr, double huber, int iters, Point& x, double& cost, int& steps) {
    double lam = kLam0;
    double a00 = 0, a01 = 0, a02 = 0, a11 = 0, a12 = 0, a22 = 0, g0 = 0, g1 = 0, g2 = 0;
    bool fresh = false;                                                         // A and g belong to the present x
    for (int it = 0; it < iters; ++it) {
        if (!fresh) {
            a00 = a01 = a02 = a11 = a12 = a22 = g0 = g1 = g2 = 0.0;
            for (int o = tr.lo; o < tr.hi; ++o) {
                int u;
                const int img = tr.active(o, u);
                if (img < 0) continue;
                const double* Pi = tr.P + 12 * (size_t)img;
                const double kx = (double)tr.kp[2 * (size_t)u], ky = (double)tr.kp[2 * (size_t)u + 1];
                const Proj h = project(Pi, x);
                const double pu = h.h0 / h.h2, pv = h.h1 / h.h2;
                const double du = pu - kx, dv = pv - ky;
                double w = 1.0;
                if (kHuber) {
                    const double e = sqrt(du * du + dv * dv);
                    w = e <= huber ? 1.0 : huber / e;
                }
                const double ja0 = (Pi[0] - pu * Pi[8]) / h.h2, ja1 = (Pi[1] - pu * Pi[9]) / h.h2, ja2 = (Pi[2] - pu * Pi[10]) / h.h2;
                const double jb0 = (Pi[4] - pv * Pi[8]) / h.h2, jb1 = (Pi[5] - pv * Pi[9]) / h.h2, jb2 = (Pi[6] - pv * Pi[10]) / h.h2;
                a00 = (a00 + w * (ja0 * ja0)) + w * (jb0 * jb0);
                a01 = (a01 + w * (ja0 * ja1)) + w * (jb0 * jb1);
                a02 = (a02 + w * (ja0 * ja2)) + w * (jb0 * jb2);
                a11 = (a11 + w * (ja1 * ja1)) + w * (jb1 * jb1);
                a12 = (a12 + w * (ja1 * ja2)) + w * (jb1 * jb2);
                a22 = (a22 + w * (ja2 * ja2)) + w * (jb2 * jb2);
                g0 = (g0 + w * (ja0 * du)) + w * (jb0 * dv);
                g1 = (g1 + w * (ja1 * du)) + w * (jb1 * dv);
                g2 = (g2 + w * (ja2 * du)) + w * (jb2 * dv);
            }
            fresh = true;
        }
        const double s00 = a00 + lam * a00, s11 = a11 + lam * a11, s22 = a22 + lam * a22;
        const double c00 = s11 * s22 - a12 * a12, c01 = a02 * a12 - a01 * s22, c02 = a01 * a12 - a02 * s11;
        const double c11 = s00 * s22 - a02 * a02, c12 = a01 * a02 - s00 * a12, c22 = s00 * s11 - a01 * a01;
        const double det = (s00 * c00 + a01 * c01) + a02 * c02;
        const double d0 = -(((c00 * g0 + c01 * g1) + c02 * g2) / det);
        const double d1 = -(((c01 * g0 + c11 * g1) + c12 * g2) / det);
        const double d2 = -(((c02 * g0 + c12 * g1) + c22 * g2) / det);
        bool ok = det != 0.0 && finite(d0) && finite(d1) && finite(d2);
        Point xn;
        xn.x = x.x + d0;
        xn.y = x.y + d1;
        xn.z = x.z + d2;
        double trial = 0.0;
        if (ok) {
            for (int o = tr.lo; o < tr.hi; ++o) {
                int u;
                const int img = tr.active(o, u);
                if (img < 0) continue;
                const Proj h = project(tr.P + 12 * (size_t)img, xn);
                if (!(h.h2 > 0.0 && h.h2 <= kDblMax)) {
                    ok = false;
                    break;
                }
                const double du = h.h0 / h.h2 - (double)tr.kp[2 * (size_t)u], dv = h.h1 / h.h2 - (double)tr.kp[2 * (size_t)u + 1];
                trial = trial + rho<kHuber>(sqrt(du * du + dv * dv), huber);
            }
        }
        if (ok && trial < cost) {
            x = xn;
            cost = trial;
            lam = lam / 10.0;
            ++steps;
            fresh = false;
        } else {
            lam = lam * 10.0;
        }
    }
}

__global__ __launch_bounds__(kLanes) void refine_kernel(const int* __restrict__ counts, const int* __restrict__ track_off,
                                                        const int* __restrict__ obs_node, const int* __restrict__ img_off, int n_img,
                                                        const float* __restrict__ kp, const double* __restrict__ P,
                                                        const double* __restrict__ C, int n, int track_cap,
                                                        const float* __restrict__ X_in, const int* __restrict__ flags_in, double huber,
                                                        double obs_thresh, int iters, int iters2, float* __restrict__ X_out,
                                                        unsigned char* __restrict__ inlier, float* __restrict__ err, int* __restrict__ word,
                                                        int* __restrict__ n_inl_out, float* __restrict__ max_err, float* __restrict__ cos_min,
                                                        int* __restrict__ steps_out, int* __restrict__ flags) {
    __shared__ unsigned short simg[kAngleCap][kLanes];
    int T = counts[0], nobs = counts[1];
    if (T < 0 || T > track_cap) T = track_cap;
    if (nobs < 0 || nobs > n) nobs = n;
    const int lane = threadIdx.x;
    const long long stride = (long long)gridDim.x * kLanes;
    for (long long t = (long long)blockIdx.x * kLanes + lane; t < T; t += stride) {
        Track tr;
        tr.obs_node = obs_node;
        tr.kp = kp;
        tr.P = P;
        tr.word = word;
        tr.n = n;
        tr.n_img = n_img;
        tr.lo = min(max(track_off[t], 0), nobs);
        tr.hi = min(max(track_off[t + 1], tr.lo), nobs);                        // the loops' bounds: 0 <= lo <= hi <= nobs <= n
        const float xi0 = X_in[3 * t + 0], xi1 = X_in[3 * t + 1], xi2 = X_in[3 * t + 2];
        Point x;
        x.x = (double)xi0;
        x.y = (double)xi1;
        x.z = (double)xi2;
        const bool start = (flags_in[t] & 2) != 0 && finite(x.x) && finite(x.y) && finite(x.z);
        // the start pass: which observations are usable, and the Huber cost over them
        double cost = 0.0;
        for (int o = tr.lo; o < tr.hi; ++o) {
            const int u = obs_node[o];
            int w = -1;
            if (in_range(u, n)) {
                const int img = image_of(img_off, n_img, u);
                w = -2 - img;
                if (start) {
                    const Proj h = project(P + 12 * (size_t)img, x);
                    const double du = h.h0 / h.h2 - (double)kp[2 * (size_t)u], dv = h.h1 / h.h2 - (double)kp[2 * (size_t)u + 1];
                    const double e = sqrt(du * du + dv * dv);
                    if (h.h2 > 0.0 && h.h2 <= kDblMax && finite(e)) {
                        w = img;
                        cost = cost + rho<true>(e, huber);
                    }
                }
            }
            word[o] = w;
        }
        int steps = 0, n_inl = 0;
        if (start) {
            lm_phase<true>(tr, huber, iters, x, cost, steps);
            // the inliers, fixed from here on, and the least-squares cost over them
            cost = 0.0;
            for (int o = tr.lo; o < tr.hi; ++o) {
                int u;
                const int img = tr.active(o, u);
                if (img < 0) continue;
                const Proj h = project(P + 12 * (size_t)img, x);
                const double du = h.h0 / h.h2 - (double)kp[2 * (size_t)u], dv = h.h1 / h.h2 - (double)kp[2 * (size_t)u + 1];
                const double e = sqrt(du * du + dv * dv);
                if (e <= obs_thresh) {
                    ++n_inl;
                    cost = cost + (e * e) / 2.0;
                } else {
                    word[o] = -2 - img;
                }
            }
            if (n_inl >= 2) lm_phase<false>(tr, huber, iters2, x, cost, steps);
        }
        const float X0 = canonical(start ? (float)x.x : xi0), X1 = canonical(start ? (float)x.y : xi1), X2 = canonical(start ? (float)x.z : xi2);
        X_out[3 * t + 0] = X0;
        X_out[3 * t + 1] = X1;
        X_out[3 * t + 2] = X2;
        const bool point_ok = start && fabsf(X0) <= kFltMax && fabsf(X1) <= kFltMax && fabsf(X2) <= kFltMax;
        Point xf;
        xf.x = (double)X0;
        xf.y = (double)X1;
        xf.z = (double)X2;
        // the final pass: errors and depths at the float32 point, the inlier bytes, the first 64 inliers' images
        float worst = 0.0f;
        int listed = 0;
        for (int o = tr.lo; o < tr.hi; ++o) {
            const int w = word[o], u = obs_node[o];
            const int img = w >= 0 ? w : ~w - 1;                                // -2 - w, without overflow; -1 stays -1
            const bool known = in_range(img, n_img) && in_range(u, n);          // checked as Track::active checks it
            const bool in = known && w >= 0;
            float e = __uint_as_float(kQuietNan), d = __uint_as_float(kQuietNan);
            if (known) {
                const Proj h = project(P + 12 * (size_t)img, xf);
                const double du = h.h0 / h.h2 - (double)kp[2 * (size_t)u], dv = h.h1 / h.h2 - (double)kp[2 * (size_t)u + 1];
                e = canonical((float)sqrt(du * du + dv * dv));
                d = canonical((float)h.h2);
            }
            err[o] = e;
            word[o] = __float_as_int(d);                                        // the row is depth_dev's from here on
            inlier[o] = in ? 1 : 0;
            if (in) {
                if (e > worst || e != e) worst = e;
                if (listed < kAngleCap) simg[listed][lane] = (unsigned short)img;
                ++listed;
            }
        }
        // the smallest cosine between the rays of the first 64 inliers
        double low = 1.0;
        const int m = min(listed, kAngleCap);
        for (int i = 0; i + 1 < m; ++i) {
            const double* Ci = C + 3 * (size_t)simg[i][lane];
            const double r0 = xf.x - Ci[0], r1 = xf.y - Ci[1], r2 = xf.z - Ci[2];
            const double ni = (r0 * r0 + r1 * r1) + r2 * r2;
            for (int j = i + 1; j < m; ++j) {
                const double* Cj = C + 3 * (size_t)simg[j][lane];
                const double q0 = xf.x - Cj[0], q1 = xf.y - Cj[1], q2 = xf.z - Cj[2];
                const double nj = (q0 * q0 + q1 * q1) + q2 * q2;
                const double c = ((r0 * q0 + r1 * q1) + r2 * q2) / sqrt(ni * nj);
                if (c < low) low = c;
            }
        }
        n_inl_out[t] = n_inl;
        max_err[t] = worst;
        cos_min[t] = (float)low;
        steps_out[t] = steps;
        flags[t] = start ? (n_inl >= 2 ? 1 : 0) | (point_ok ? 2 : 0) : 0;
    }
}

// ---- pruning --------------------------------------------------------------------------------------------------------------

struct PruneWs {
    int *keep, *part_t, *part_o, *part_d;        // keep [cap]: the inlier observations of a kept track, -1 for a dropped one
    size_t bytes;
};

__device__ inline int wave_sum(int v) {
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// Sum over the workgroup, valid in thread 0.
__device__ inline int block_sum(int v, int* lds) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    int t = 0;
    for (int k = 0; k < kWaves; ++k) t += lds[k];
    return t;
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

// Per 256-track block: kept tracks, the inlier observations they hold, the observations they lose.
__global__ __launch_bounds__(kBlock) void prune_count_kernel(const int* __restrict__ counts, const int* __restrict__ track_off,
                                                             const unsigned char* __restrict__ inlier, const int* __restrict__ n_inl,
                                                             const float* __restrict__ max_err, const float* __restrict__ cos_min,
                                                             const int* __restrict__ flags, int n, int track_cap, long long min_len,
                                                             double max_reproj, double max_cos, long long nblocks, PruneWs w) {
    __shared__ int lds[kWaves];
    const Counts c = clamped(counts, n, track_cap);
    for (long long blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const long long t = blk * kBlock + threadIdx.x;
        int kept = 0, held = 0, lost = 0;
        if (t < c.T) {
            const bool keep = flags[t] == 3 && (long long)n_inl[t] >= min_len && (double)max_err[t] <= max_reproj && (double)cos_min[t] <= max_cos;
            const int lo = min(max(track_off[t], 0), c.nobs), hi = min(max(track_off[t + 1], lo), c.nobs);
            if (keep) {
                for (int o = lo; o < hi; ++o) held += inlier[o] != 0;
                kept = 1;
                lost = (hi - lo) - held;
            }
            w.keep[t] = keep ? held : -1;
        }
        const int st = block_sum(kept, lds), so = block_sum(held, lds), sd = block_sum(lost, lds);
        if (threadIdx.x == 0) {
            w.part_t[blk] = st;
            w.part_o[blk] = so;
            w.part_d[blk] = sd;
        }
    }
}

// Workgroup 0: the kept-track block counts -> exclusive offsets in place; workgroup 1: the same for the observations they hold;
// workgroup 2 sums the observations lost.  counts2 = (T', nobs', tracks dropped, observations dropped from kept tracks).
__global__ __launch_bounds__(kScanThreads) void prune_scan_kernel(const int* __restrict__ counts, int n, int track_cap, PruneWs w, long long nblocks,
                                                                  int* __restrict__ counts2) {
    __shared__ int buf[kScanThreads];
    int* part = blockIdx.x == 0 ? w.part_t : blockIdx.x == 1 ? w.part_o : w.part_d;
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
    int run = buf[tid] - sum;
    for (long long b = lo; b < hi; ++b) {
        const int v = part[b];
        part[b] = run;
        run += v;
    }
    if (tid == kScanThreads - 1) {
        const int total = buf[tid];
        if (blockIdx.x == 0) {
            counts2[0] = total;
            counts2[2] = clamped(counts, n, track_cap).T - total;
        } else {
            counts2[blockIdx.x == 1 ? 1 : 3] = total;
        }
    }
}

__global__ __launch_bounds__(kBlock) void prune_place_kernel(const int* __restrict__ counts, const int* __restrict__ track_off,
                                                             const int* __restrict__ obs_node, const float* __restrict__ X,
                                                             const unsigned char* __restrict__ inlier, int n, int track_cap, long long nblocks,
                                                             PruneWs w, const int* __restrict__ counts2, int* __restrict__ track_off2,
                                                             int* __restrict__ obs_node2, float* __restrict__ X2, int* __restrict__ track_src) {
    __shared__ int scan_t[kBlock], scan_o[kBlock];
    const Counts c = clamped(counts, n, track_cap);
    if (blockIdx.x == 0 && threadIdx.x == 0) track_off2[counts2[0]] = counts2[1];  // counts2[0] <= T <= N / 2 + 1: inside the N / 2 + 2 words
    for (long long blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const long long t = blk * kBlock + threadIdx.x;
        const int tid = threadIdx.x;
        const int held = t < c.T ? w.keep[t] : -1;
        __syncthreads();
        scan_t[tid] = held >= 0;
        scan_o[tid] = max(held, 0);
        __syncthreads();
        for (int off = 1; off < kBlock; off <<= 1) {
            const int at = tid >= off ? scan_t[tid - off] : 0, ao = tid >= off ? scan_o[tid - off] : 0;
            __syncthreads();
            scan_t[tid] += at;
            scan_o[tid] += ao;
            __syncthreads();
        }
        if (held < 0) continue;
        const int r = w.part_t[blk] + scan_t[tid] - 1;                          // < T' <= T
        int at = w.part_o[blk] + scan_o[tid] - held;
        track_off2[r] = at;
        track_src[r] = (int)t;
        X2[3 * (size_t)r + 0] = X[3 * t + 0];
        X2[3 * (size_t)r + 1] = X[3 * t + 1];
        X2[3 * (size_t)r + 2] = X[3 * t + 2];
        const int lo = min(max(track_off[t], 0), c.nobs), hi = min(max(track_off[t + 1], lo), c.nobs);
        const long long end = (long long)at + held;                                             // the row after this track's: no write reaches it
        for (int o = lo; o < hi; ++o)                                           // (at < n: ranges that overlap can hold more than n rows in all)
            if (inlier[o] != 0 && at < end && in_range(at, n)) obs_node2[at++] = obs_node[o];
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------

int64_t blocks_of(int64_t n, int block = kBlock) { return (n + block - 1) / block; }

unsigned grid_of(int64_t blocks) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks, kMaxGrid)); }

bool count_ok(int64_t n) { return n >= 0 && n <= kMaxCount; }

struct RefineWs {
    double* centres;                             // [n_img][3]
    size_t bytes;
};

RefineWs carve_refine(void* base, int n_img) {
    sfm::Carver c(base);
    RefineWs w{};
    w.centres = c.take<double>(3 * (size_t)n_img);
    w.bytes = c.used();
    return w;
}

PruneWs carve_prune(void* base, int64_t n) {
    sfm::Carver c(base);
    PruneWs w{};
    const int64_t cap = n / 2 + 1;
    w.keep = c.take<int>(cap);
    w.part_t = c.take<int>(blocks_of(cap));
    w.part_o = c.take<int>(blocks_of(cap));
    w.part_d = c.take<int>(blocks_of(cap));
    w.bytes = c.used();
    return w;
}

}  // namespace

extern "C" size_t sfm_track_refine_ws_bytes(int n_img) { return n_img >= 1 && n_img <= kMaxImages ? carve_refine(nullptr, n_img).bytes : 0; }

extern "C" int sfm_track_refine(const int32_t* counts_dev, const int32_t* track_off_dev, const int32_t* obs_node_dev, const int32_t* img_off_dev,
                                int n_img, const float* kp_dev, const double* P_dev, int64_t n_nodes, const float* X_in_dev,
                                const int32_t* flags_in_dev, double huber, double obs_thresh, int iters, int iters2, float* X_out_dev,
                                uint8_t* inlier_dev, float* err_dev, float* depth_dev, int32_t* n_inl_dev, float* max_err_dev, float* cos_min_dev,
                                int32_t* steps_dev, int32_t* flags_dev, void* ws_dev, size_t ws_bytes, void* stream) {
    SFM_CHECK_ARG(count_ok(n_nodes), "sfm_track_refine: n_nodes %lld must be in 0..2^31-1", (long long)n_nodes);
    SFM_CHECK_ARG(n_img >= 1 && n_img <= kMaxImages, "sfm_track_refine: n_img %d must be in 1..%d", n_img, kMaxImages);
    SFM_CHECK_ARG(huber > 0.0, "sfm_track_refine: huber %g must be > 0 px (+inf: plain least squares)", huber);
    SFM_CHECK_ARG(obs_thresh > 0.0, "sfm_track_refine: obs_thresh %g must be > 0 px", obs_thresh);
    SFM_CHECK_ARG(iters >= 0 && iters <= kMaxIters && iters2 >= 0 && iters2 <= kMaxIters, "sfm_track_refine: iters %d, iters2 %d: each must be in 0..%d",
                  iters, iters2, kMaxIters);
    SFM_CHECK_ARG(counts_dev && track_off_dev && img_off_dev && P_dev && X_in_dev && flags_in_dev && X_out_dev && n_inl_dev && max_err_dev &&
                      cos_min_dev && steps_dev && flags_dev && ws_dev && (n_nodes == 0 || (obs_node_dev && kp_dev && inlier_dev && err_dev && depth_dev)),
                  "sfm_track_refine: null required pointer");
    const RefineWs ws = carve_refine(ws_dev, n_img);
    SFM_CHECK_ARG(ws_bytes >= ws.bytes, "sfm_track_refine: workspace %zu bytes < %zu", ws_bytes, ws.bytes);
    const int track_cap = (int)(n_nodes / 2 + 1);
    hipStream_t s = sfm::as_stream(stream);
    hipLaunchKernelGGL(centres_kernel, dim3(grid_of(blocks_of(n_img))), dim3(kBlock), 0, s, P_dev, n_img, ws.centres);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(refine_kernel, dim3(grid_of(blocks_of(track_cap, kLanes))), dim3(kLanes), 0, s, counts_dev, track_off_dev, obs_node_dev,
                       img_off_dev, n_img, kp_dev, P_dev, ws.centres, (int)n_nodes, track_cap, X_in_dev, flags_in_dev, huber, obs_thresh, iters, iters2,
                       X_out_dev, inlier_dev, err_dev, reinterpret_cast<int*>(depth_dev), n_inl_dev, max_err_dev, cos_min_dev, steps_dev, flags_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" size_t sfm_track_prune_ws_bytes(int64_t n_nodes) { return count_ok(n_nodes) ? carve_prune(nullptr, n_nodes).bytes : 0; }

extern "C" int sfm_track_prune(const int32_t* counts_dev, const int32_t* track_off_dev, const int32_t* obs_node_dev, int64_t n_nodes,
                               const float* X_dev, const uint8_t* inlier_dev, const int32_t* n_inl_dev, const float* max_err_dev,
                               const float* cos_min_dev, const int32_t* flags_dev, int64_t min_len, double max_reproj, double max_cos,
                               int32_t* track_off2_dev, int32_t* obs_node2_dev, float* X2_dev, int32_t* track_src_dev, int32_t* counts2_dev,
                               void* ws_dev, size_t ws_bytes, void* stream) {
    SFM_CHECK_ARG(count_ok(n_nodes), "sfm_track_prune: n_nodes %lld must be in 0..2^31-1", (long long)n_nodes);
    SFM_CHECK_ARG(min_len >= 2 && min_len <= kMaxCount, "sfm_track_prune: min_len %lld must be in 2..2^31-1", (long long)min_len);
    SFM_CHECK_ARG(max_reproj == max_reproj, "sfm_track_prune: max_reproj is NaN (+inf switches the filter off)");
    SFM_CHECK_ARG(max_cos == max_cos, "sfm_track_prune: max_cos is NaN (1 switches the filter off)");
    SFM_CHECK_ARG(counts_dev && track_off_dev && X_dev && n_inl_dev && max_err_dev && cos_min_dev && flags_dev && track_off2_dev && X2_dev &&
                      track_src_dev && counts2_dev && ws_dev && (n_nodes == 0 || (obs_node_dev && inlier_dev && obs_node2_dev)),
                  "sfm_track_prune: null required pointer");
    const PruneWs ws = carve_prune(ws_dev, n_nodes);
    SFM_CHECK_ARG(ws_bytes >= ws.bytes, "sfm_track_prune: workspace %zu bytes < %zu", ws_bytes, ws.bytes);
    const int n = (int)n_nodes, track_cap = (int)(n_nodes / 2 + 1);
    const long long nblocks = blocks_of(track_cap);
    hipStream_t s = sfm::as_stream(stream);
    const dim3 block(kBlock), grid(grid_of(nblocks));
    hipLaunchKernelGGL(prune_count_kernel, grid, block, 0, s, counts_dev, track_off_dev, inlier_dev, n_inl_dev, max_err_dev, cos_min_dev, flags_dev, n,
                       track_cap, (long long)min_len, max_reproj, max_cos, nblocks, ws);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(prune_scan_kernel, dim3(3), dim3(kScanThreads), 0, s, counts_dev, n, track_cap, ws, nblocks, counts2_dev);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(prune_place_kernel, grid, block, 0, s, counts_dev, track_off_dev, obs_node_dev, X_dev, inlier_dev, n, track_cap, nblocks, ws,
                       counts2_dev, track_off2_dev, obs_node2_dev, X2_dev, track_src_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}
