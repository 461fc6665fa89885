// Self-calibrating bundle adjustment of feature tracks and the undistortion that goes with it (include/sfm_hip.h, "TRACKS-CAL";
// docs/tracks.md §15).  The sibling of csrc/tracks_ba.hip with one set of intrinsics shared by all images,
// theta = (f, cx, cy, k1, k2), a fixed aspect a and the radial model u = f d x + cx, v = a f d y + cy, d = 1 + k1 r2 + k2 r2 r2.
//   sfm_track_cal_sweep     linearisation at (cams, theta - dtheta, X): a row of 30 doubles per observation (sqrt(w) Jc, sqrt(w) Ji,
//                           sqrt(w) Jp, sqrt(w) r), the active set, the blocks of TRACKS-BA and the border E_i, G, g_i, F_j
//   sfm_track_cal_product   (xc, xi) -> sum Jp^T (Jc xc + Ji xi) and v -> (sum Jc^T Jp v, sum Ji^T Jp v) over the stored rows
//   sfm_track_cal_step      one damped step on the bordered system of 6 ncam + 5 unknowns: block inverses, PCG preconditioned with
//                           blockdiag(Bd^-1, Gd^-1), back-substitution; the host reads r.r before iterations 0, 5, 10, ...
//   sfm_undistort_points    distorted pixels -> pixels of the ideal pinhole image (a fixed number of Newton steps on the radius)
//   sfm_undistort_image     the ideal pinhole image sampled bilinearly from the distorted one, a batch of frames per call
// THERE ARE NO FLOATING-POINT ATOMICS IN THIS FILE.  Every sum is a fixed function of the CSR and of the data:
//   point side   a group of kGroup lanes per track, lane l adds observations l, l + kGroup, ... of the track ascending, the kGroup
//                partial sums meet in a xor tree (strides kGroup / 2 .. 1)
//   camera side  a camera's list (cam_off / cam_obs) is cut into chunks of kChunk observations; one workgroup sums a chunk (a lane
//                per observation, xor tree over the wave, the four waves in ascending order); a fold kernel adds a camera's chunk
//                sums in ascending order
//   cost, G, g_i, out_i   per workgroup of kBlock consecutive observations the same tree, then one workgroup adds the block sums
//                (lane l blocks l, l + 1024, ... ascending, then a tree)
// None depends on the grid, on the waves in flight or on the order in which workgroups finish.
// The file is compiled with floating-point contraction OFF (the library's default): the two undistortion kernels are held to the
// bit against tests/np_track_cal.py, the sums to a tolerance.
// Rodrigues with its derivative, the trees, the chunk scan, the small block kernels and the single-workgroup CG kernels are copies of
// csrc/tracks_ba.hip's, as the families copy theirs.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>

#include "common.h"

#ifndef SFM_TCAL_GROUP
#define SFM_TCAL_GROUP 8                        // lanes per track on the point side, as SFM_TBA_GROUP
#endif

namespace {

constexpr int kRow = 30;                        // doubles per observation: Jc (2 x 6), Ji (2 x 5), Jp (2 x 3), r (2), each times sqrt(w)
constexpr int kJi = 12, kJp = 22, kRes = 28;    // offsets inside a row
constexpr int kTheta = 5;                       // f, cx, cy, k1, k2
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kGroup = SFM_TCAL_GROUP;
constexpr int kChunk = kBlock;                  // observations of a camera one workgroup sums
constexpr int kCamStride = 40;
constexpr int kBlockVals = 57;                  // the upper triangle of B_i (21), g_c (6), E_i (6 x 5)
constexpr int kCostVals = 5;                    // robust cost, plain sum of e^2, active, crossed, outliers
constexpr int kObsVals = kCostVals + 15 + 5;    // ... the upper triangle of G (15) and g_i (5)
constexpr int kPointVals = 24;                  // the upper triangle of C_j (6), g_p (3), F_j (3 x 5)
constexpr int kScanThreads = 1024;
constexpr int kSearchSteps = 26;                // binary search over at most 2^24 + 1 chunk offsets
constexpr int kCgThreads = 1024;
constexpr int kNewton = 10;                     // Newton steps of sfm_undistort_points
constexpr double kDblMax = 1.7976931348623157e308;
static_assert(kGroup == 1 || kGroup == 2 || kGroup == 4 || kGroup == 8 || kGroup == 16 || kGroup == 32 || kGroup == 64, "kGroup divides a wave");

struct Theta {
    double f, cx, cy, k1, k2, a;
};

__device__ inline bool in_range(int a, int64_t n) { return a >= 0 && (int64_t)a < n; }

__device__ inline bool finite(double v) { return fabs(v) <= kDblMax; }

// [lo, hi) of row i of a CSR nobody vouches for: 0 <= lo <= hi <= n
__device__ inline void csr_range(const int* __restrict__ off, int64_t i, int n, int& lo, int& hi) {
    lo = min(max(off[i], 0), n);
    hi = min(max(off[i + 1], lo), n);
}

__device__ void rodrigues_tcal(const double* __restrict__ rv, double* __restrict__ R, double* __restrict__ J) {
    const double theta = sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2]);
    if (theta < DBL_EPSILON) {
        for (int k = 0; k < 9; ++k) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
        for (int k = 0; k < 27; ++k) J[k] = 0;
        J[5] = J[15] = J[19] = -1;
        J[7] = J[11] = J[21] = 1;
        return;
    }
    // 1 - cos(theta) as 2 sin^2(theta / 2): see csrc/ba_schur.hip
    const double c = cos(theta), s = sin(theta), sh = sin(0.5 * theta), c1 = 2. * sh * sh, itheta = 1. / theta;
    const double r[3] = {rv[0] * itheta, rv[1] * itheta, rv[2] * itheta};
    const double rrt[9] = {r[0] * r[0], r[0] * r[1], r[0] * r[2], r[0] * r[1], r[1] * r[1],
                           r[1] * r[2], r[0] * r[2], r[1] * r[2], r[2] * r[2]};
    const double rx[9] = {0, -r[2], r[1], r[2], 0, -r[0], -r[1], r[0], 0};
    for (int k = 0; k < 9; ++k) R[k] = c * ((k % 4 == 0) ? 1.0 : 0.0) + c1 * rrt[k] + s * rx[k];
    const double drrt[27] = {r[0] + r[0], r[1], r[2], r[1], 0, 0, r[2], 0, 0,
                             0, r[0], 0, r[0], r[1] + r[1], r[2], 0, r[2], 0,
                             0, 0, r[0], 0, 0, r[1], r[0], r[1], r[2] + r[2]};
    const double drx[27] = {0, 0, 0, 0, 0, -1, 0, 1, 0, 0, 0, 1, 0, 0, 0, -1, 0, 0, 0, -1, 0, 1, 0, 0, 0, 0, 0};
    for (int i = 0; i < 3; ++i) {
        const double ri = r[i];
        const double a0 = -s * ri, a1 = (s - 2 * c1 * itheta) * ri, a2 = c1 * itheta;
        const double a3 = (c - s * itheta) * ri, a4 = s * itheta;
        for (int k = 0; k < 9; ++k)
            J[i * 9 + k] = a0 * ((k % 4 == 0) ? 1.0 : 0.0) + a1 * rrt[k] + a2 * drrt[i * 9 + k] + a3 * rx[k] +
                           a4 * drx[i * 9 + k];
    }
}

// camera table: R (9), t (3), dR/dr (27), pad
__global__ void tcal_cam_prepare_kernel(const double* __restrict__ cams, int64_t ncam, double* __restrict__ table) {
    const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (c >= ncam) return;
    double R[9], J[27];
    rodrigues_tcal(cams + 6 * c, R, J);
    double* e = table + c * kCamStride;
    for (int k = 0; k < 9; ++k) e[k] = R[k];
    for (int k = 0; k < 3; ++k) e[9 + k] = cams[6 * c + 3 + k];
    for (int k = 0; k < 27; ++k) e[12 + k] = J[k];
    e[39] = 0;
}

// ---- sums in a fixed shape ------------------------------------------------------------------------------------------------

__device__ __forceinline__ double wave_tree(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

template <int G> __device__ __forceinline__ double group_tree(double v) {
#pragma unroll
    for (int m = G / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// The workgroup's sum of NV values per thread: xor tree over each wave, then the waves in ascending order; thread k < NV returns
// value k, every other thread 0.
template <int NV> __device__ __forceinline__ double block_values(const double (&val)[NV], double (*lds)[NV]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const double s = wave_tree(val[k]);
        if (lane == 0) lds[wave][k] = s;
    }
    __syncthreads();
    double s = 0.0;
    if ((int)threadIdx.x < NV) {
        s = lds[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) s += lds[w][threadIdx.x];
    }
    return s;
}

__device__ __forceinline__ double cg_block_sum(double v, double* lds) {
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int m = kCgThreads / 2; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m) lds[threadIdx.x] += lds[threadIdx.x + m];
        __syncthreads();
    }
    const double s = lds[0];
    __syncthreads();
    return s;
}

// ---- the rows -------------------------------------------------------------------------------------------------------------

// One lane per observation: the row, the active byte (MODE 0) and the terms of the cost, of G and of g_i; a workgroup's sums go to
// obs_part.  The intrinsics are T minus dtheta (a trial step that is still on the device; null: zero).
template <int MODE>
__global__ __launch_bounds__(kBlock) void tcal_obs_kernel(const double* __restrict__ table, Theta T, const double* __restrict__ dtheta, int64_t ncam,
                                                          const double* __restrict__ X, int64_t npt, const float* __restrict__ obs,
                                                          const int* __restrict__ cam_idx, const int* __restrict__ pt_idx, int nobs, double huber,
                                                          unsigned char* __restrict__ active, double* __restrict__ rows,
                                                          double* __restrict__ obs_part) {
    __shared__ double lds[kWaves][kObsVals];
    const int64_t o = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    double val[kObsVals];
#pragma unroll
    for (int k = 0; k < kObsVals; ++k) val[k] = 0.0;
    if (o < nobs) {
        if (dtheta) {
            T.f -= dtheta[0]; T.cx -= dtheta[1]; T.cy -= dtheta[2]; T.k1 -= dtheta[3]; T.k2 -= dtheta[4];
        }
        const bool th_ok = T.f > 0.0 && finite(T.f) && finite(T.cx) && finite(T.cy) && finite(T.k1) && finite(T.k2);
        const int ci = cam_idx[o], pi = pt_idx[o];
        const bool inr = in_range(ci, ncam) && in_range(pi, npt);
        double row[kRow];
#pragma unroll
        for (int k = 0; k < kRow; ++k) row[k] = 0.0;
        bool ok = false;
        double ru = 0, rv = 0;
        double Ju[6], Jv[6], Iu[kTheta], Iv[kTheta], Pu[3], Pv[3];
        if (inr) {
            const double* __restrict__ e = table + (int64_t)ci * kCamStride;
            const double Xw = X[3 * (int64_t)pi], Yw = X[3 * (int64_t)pi + 1], Zw = X[3 * (int64_t)pi + 2];
            double x = e[0] * Xw + e[1] * Yw + e[2] * Zw + e[9];
            double y = e[3] * Xw + e[4] * Yw + e[5] * Zw + e[10];
            const double zc = e[6] * Xw + e[7] * Yw + e[8] * Zw + e[11];
            const double z = 1. / zc;
            x *= z;
            y *= z;
            const double fy = T.a * T.f;
            const double r2 = x * x + y * y;
            const double d = 1.0 + T.k1 * r2 + T.k2 * r2 * r2;
            const double q2 = 2.0 * (T.k1 + 2.0 * T.k2 * r2);                   // 2 dd/dr2
            ru = (T.f * d * x + T.cx) - (double)obs[2 * o];
            rv = (fy * d * y + T.cy) - (double)obs[2 * o + 1];
            ok = th_ok && zc > 0.0 && zc <= kDblMax && finite(ru) && finite(rv);
            // d(d x, d y)/d(x, y)
            const double a11 = d + q2 * x * x, a12 = q2 * x * y, a22 = d + q2 * y * y;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double* dd = e + 12 + 9 * j;
                const double dx0 = Xw * dd[0] + Yw * dd[1] + Zw * dd[2];
                const double dy0 = Xw * dd[3] + Yw * dd[4] + Zw * dd[5];
                const double dz0 = Xw * dd[6] + Yw * dd[7] + Zw * dd[8];
                const double dx = z * (dx0 - x * dz0), dy = z * (dy0 - y * dz0);
                Ju[j] = T.f * (a11 * dx + a12 * dy);
                Jv[j] = fy * (a12 * dx + a22 * dy);
            }
            Ju[3] = T.f * (a11 * z); Ju[4] = T.f * (a12 * z); Ju[5] = T.f * (a11 * (-x * z) + a12 * (-y * z));
            Jv[3] = fy * (a12 * z);  Jv[4] = fy * (a22 * z);  Jv[5] = fy * (a12 * (-x * z) + a22 * (-y * z));
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double dx = z * (e[k] - x * e[6 + k]), dy = z * (e[3 + k] - y * e[6 + k]);
                Pu[k] = T.f * (a11 * dx + a12 * dy);
                Pv[k] = fy * (a12 * dx + a22 * dy);
            }
            Iu[0] = d * x;       Iu[1] = 1.0; Iu[2] = 0.0; Iu[3] = T.f * x * r2; Iu[4] = T.f * x * r2 * r2;
            Iv[0] = T.a * d * y; Iv[1] = 0.0; Iv[2] = 1.0; Iv[3] = fy * y * r2;  Iv[4] = fy * y * r2 * r2;
        }
        bool act;
        if (MODE == 0) {
            act = ok;
            active[o] = act ? 1 : 0;
        } else {
            const bool was = inr && active[o] != 0;
            act = was && ok;
            if (was && !ok) val[3] = 1.0;
        }
        if (act) {
            const double e2 = ru * ru + rv * rv, e = sqrt(e2);
            const bool in = e <= huber;
            const double w = in ? 1.0 : huber / e, sw = sqrt(w);
            val[0] = in ? e2 : 2.0 * huber * e - huber * huber;
            val[1] = e2;
            val[2] = 1.0;
            val[4] = in ? 0.0 : 1.0;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                row[a] = sw * Ju[a];
                row[6 + a] = sw * Jv[a];
            }
#pragma unroll
            for (int i = 0; i < kTheta; ++i) {
                row[kJi + i] = sw * Iu[i];
                row[kJi + kTheta + i] = sw * Iv[i];
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                row[kJp + k] = sw * Pu[k];
                row[kJp + 3 + k] = sw * Pv[k];
            }
            row[kRes] = sw * ru;
            row[kRes + 1] = sw * rv;
            int n = kCostVals;
#pragma unroll
            for (int i = 0; i < kTheta; ++i)
#pragma unroll
                for (int j = i; j < kTheta; ++j) val[n++] = row[kJi + i] * row[kJi + j] + row[kJi + kTheta + i] * row[kJi + kTheta + j];
#pragma unroll
            for (int i = 0; i < kTheta; ++i) val[kCostVals + 15 + i] = row[kJi + i] * row[kRes] + row[kJi + kTheta + i] * row[kRes + 1];
        }
        double2* dst = reinterpret_cast<double2*>(rows + o * kRow);             // 240-byte rows at a 256-byte aligned base
#pragma unroll
        for (int k = 0; k < kRow / 2; ++k) dst[k] = make_double2(row[2 * k], row[2 * k + 1]);
    }
    const double s = block_values<kObsVals>(val, lds);
    if (threadIdx.x < kObsVals) obs_part[(int64_t)blockIdx.x * kObsVals + threadIdx.x] = s;
}

// out_i of the product's mode 1, in the cost's shape: per observation Ji^T (Jp v[point]), a workgroup's sums to part [nblk][5].
__global__ __launch_bounds__(kBlock) void tcal_obs_i_kernel(const int* __restrict__ cam_idx, const int* __restrict__ pt_idx, int64_t ncam, int64_t npt,
                                                            int nobs, const double* __restrict__ rows, const double* __restrict__ v,
                                                            double* __restrict__ part) {
    __shared__ double lds[kWaves][kTheta];
    const int64_t o = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    double val[kTheta] = {0, 0, 0, 0, 0};
    if (o < nobs) {
        const int ci = cam_idx[o], pi = pt_idx[o];
        if (in_range(ci, ncam) && in_range(pi, npt)) {
            const double* __restrict__ r = rows + o * kRow;
            const double* __restrict__ x = v + (int64_t)pi * 3;
            const double su = r[kJp] * x[0] + r[kJp + 1] * x[1] + r[kJp + 2] * x[2];
            const double sv = r[kJp + 3] * x[0] + r[kJp + 4] * x[1] + r[kJp + 5] * x[2];
#pragma unroll
            for (int i = 0; i < kTheta; ++i) val[i] = r[kJi + i] * su + r[kJi + kTheta + i] * sv;
        }
    }
    const double s = block_values<kTheta>(val, lds);
    if (threadIdx.x < kTheta) part[(int64_t)blockIdx.x * kTheta + threadIdx.x] = s;
}

// One workgroup: for each of the nv values, lane l adds the block sums l, l + 1024, ... ascending, then a tree.  FIRST values of
// the sweep: stat (2 doubles), count (3 ints), the upper triangle of G (written in full), g_i; of the product (nv = 5): out_i.
template <bool SWEEP>
__global__ __launch_bounds__(kScanThreads) void tcal_fold_kernel(const double* __restrict__ part, int64_t nblk, double* __restrict__ stat,
                                                                 int* __restrict__ count, double* __restrict__ G, double* __restrict__ gi) {
    __shared__ double lds[kScanThreads];
    constexpr int nv = SWEEP ? kObsVals : kTheta;
    for (int k = 0; k < nv; ++k) {
        double s = 0.0;
        for (int64_t b = threadIdx.x; b < nblk; b += kScanThreads) s += part[b * nv + k];
        s = cg_block_sum(s, lds);
        if (threadIdx.x != 0) continue;
        if (!SWEEP) {
            gi[k] = s;
        } else if (k < 2) {
            stat[k] = s;
        } else if (k < kCostVals) {
            count[k - 2] = (int)s;
        } else if (k < kCostVals + 15) {
            int i = 0, j = k - kCostVals;
            while (j >= kTheta - i) {
                j -= kTheta - i;
                ++i;
            }
            j += i;
            G[i * kTheta + j] = s;
            G[j * kTheta + i] = s;
        } else {
            gi[k - kCostVals - 15] = s;
        }
    }
}

// ---- point side -----------------------------------------------------------------------------------------------------------

// MODE 0: C_t (9), g_p (3) and F_t (3 x 5) from the rows.  MODE 1: u_t = sum Jp^T (Jc xc[cam] + Ji xi).
template <int MODE>
__global__ __launch_bounds__(kBlock) void tcal_point_kernel(const int* __restrict__ track_off, const int* __restrict__ cam_idx, int64_t ncam, int64_t npt,
                                                            int nobs, const double* __restrict__ rows, const double* __restrict__ xc,
                                                            const double* __restrict__ xi, double* __restrict__ out9, double* __restrict__ out3,
                                                            double* __restrict__ out15) {
    constexpr int NV = MODE == 0 ? kPointVals : 3;
    const int64_t id = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    const int64_t t = id / kGroup;
    const int l = (int)(id % kGroup);
    double acc[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = 0.0;
    double ti[kTheta] = {0, 0, 0, 0, 0};
    if (MODE == 1)
#pragma unroll
        for (int i = 0; i < kTheta; ++i) ti[i] = xi[i];
    if (t < npt) {
        int lo, hi;
        csr_range(track_off, t, nobs, lo, hi);
        for (int o = lo + l; o < hi; o += kGroup) {
            const double* __restrict__ r = rows + (int64_t)o * kRow;
            const double pu0 = r[kJp], pu1 = r[kJp + 1], pu2 = r[kJp + 2], pv0 = r[kJp + 3], pv1 = r[kJp + 4], pv2 = r[kJp + 5];
            if (MODE == 0) {
                const double ru = r[kRes], rv = r[kRes + 1];
                acc[0] += pu0 * pu0 + pv0 * pv0;
                acc[1] += pu0 * pu1 + pv0 * pv1;
                acc[2] += pu0 * pu2 + pv0 * pv2;
                acc[3] += pu1 * pu1 + pv1 * pv1;
                acc[4] += pu1 * pu2 + pv1 * pv2;
                acc[5] += pu2 * pu2 + pv2 * pv2;
                acc[6] += pu0 * ru + pv0 * rv;
                acc[7] += pu1 * ru + pv1 * rv;
                acc[8] += pu2 * ru + pv2 * rv;
#pragma unroll
                for (int i = 0; i < kTheta; ++i) {
                    const double iu = r[kJi + i], iv = r[kJi + kTheta + i];
                    acc[9 + i] += pu0 * iu + pv0 * iv;
                    acc[9 + kTheta + i] += pu1 * iu + pv1 * iv;
                    acc[9 + 2 * kTheta + i] += pu2 * iu + pv2 * iv;
                }
            } else {
                const int ci = cam_idx[o];
                if (!in_range(ci, ncam)) continue;
                const double* __restrict__ x = xc + (int64_t)ci * 6;
                double tu = 0, tv = 0;
#pragma unroll
                for (int a = 0; a < 6; ++a) {
                    tu += r[a] * x[a];
                    tv += r[6 + a] * x[a];
                }
#pragma unroll
                for (int i = 0; i < kTheta; ++i) {
                    tu += r[kJi + i] * ti[i];
                    tv += r[kJi + kTheta + i] * ti[i];
                }
                acc[0] += pu0 * tu + pv0 * tv;
                acc[1] += pu1 * tu + pv1 * tv;
                acc[2] += pu2 * tu + pv2 * tv;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = group_tree<kGroup>(acc[k]);           // every lane of the wave takes part
    if (t < npt && l == 0) {
        if (MODE == 0) {
            double* C = out9 + t * 9;
            C[0] = acc[0]; C[1] = acc[1]; C[2] = acc[2];
            C[3] = acc[1]; C[4] = acc[3]; C[5] = acc[4];
            C[6] = acc[2]; C[7] = acc[4]; C[8] = acc[5];
            out3[t * 3] = acc[6]; out3[t * 3 + 1] = acc[7]; out3[t * 3 + 2] = acc[8];
#pragma unroll
            for (int k = 0; k < 15; ++k) out15[t * 15 + k] = acc[9 + k];
        } else {
            out3[t * 3] = acc[0]; out3[t * 3 + 1] = acc[1]; out3[t * 3 + 2] = acc[2];
        }
    }
}

// ---- camera side ----------------------------------------------------------------------------------------------------------

// chunk_off[c] = the chunks of the cameras before c, chunk_off[ncam] = all of them, none above `cap` (a CSR whose ranges overlap
// can ask for more chunks than the workspace holds: the cameras at the end then go short, nothing is written outside it).
__global__ __launch_bounds__(kScanThreads) void tcal_chunk_scan_kernel(const int* __restrict__ cam_off, int64_t ncam, int nobs, int64_t cap,
                                                                       int* __restrict__ chunk_off) {
    __shared__ long long buf[kScanThreads];
    const int tid = threadIdx.x;
    const int64_t seg = (ncam + kScanThreads - 1) / kScanThreads;
    const int64_t lo = min(tid * seg, ncam), hi = min(lo + seg, ncam);
    long long sum = 0;
    for (int64_t c = lo; c < hi; ++c) {
        int a, b;
        csr_range(cam_off, c, nobs, a, b);
        sum += (b - a + kChunk - 1) / kChunk;
    }
    buf[tid] = sum;
    __syncthreads();
    for (int off = 1; off < kScanThreads; off <<= 1) {
        const long long add = tid >= off ? buf[tid - off] : 0;
        __syncthreads();
        buf[tid] += add;
        __syncthreads();
    }
    long long run = buf[tid] - sum;
    for (int64_t c = lo; c < hi; ++c) {
        int a, b;
        csr_range(cam_off, c, nobs, a, b);
        chunk_off[c] = (int)min(run, (long long)cap);
        run += (b - a + kChunk - 1) / kChunk;
    }
    if (tid == kScanThreads - 1) chunk_off[ncam] = (int)min(buf[tid], (long long)cap);
}

// Workgroup b sums chunk b: its camera c has chunk_off[c] <= b < chunk_off[c + 1].  MODE 0: the upper triangle of B_c, g_c and E_c
// (57 values); MODE 1: w_c = sum Jc^T (Jp v[point]) (6 values).  An entry of cam_obs outside 0..nobs-1, or naming an observation
// of another camera, adds nothing.
template <int MODE>
__global__ __launch_bounds__(kBlock) void tcal_cam_chunk_kernel(const int* __restrict__ cam_off, const int* __restrict__ cam_obs,
                                                                const int* __restrict__ cam_idx, const int* __restrict__ pt_idx,
                                                                const int* __restrict__ chunk_off, int64_t ncam, int64_t npt, int nobs,
                                                                const double* __restrict__ rows, const double* __restrict__ v,
                                                                double* __restrict__ part) {
    constexpr int NV = MODE == 0 ? kBlockVals : 6;
    __shared__ double lds[kWaves][NV];
    const int b = blockIdx.x;
    if (b >= chunk_off[ncam]) return;
    int64_t lo = 0, hi = ncam;                                                  // chunk_off[lo] <= b < chunk_off[hi]
    for (int step = 0; step < kSearchSteps && hi - lo > 1; ++step) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (chunk_off[mid] <= b) lo = mid; else hi = mid;
    }
    const int c = (int)lo;
    int first, last;
    csr_range(cam_off, c, nobs, first, last);
    const int64_t p = (int64_t)first + (int64_t)(b - chunk_off[c]) * kChunk + threadIdx.x;
    double val[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) val[k] = 0.0;
    if (p < last) {
        const int o = cam_obs[p];
        if (in_range(o, nobs) && cam_idx[o] == c) {
            const double* __restrict__ r = rows + (int64_t)o * kRow;
            double ju[6], jv[6];
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                ju[a] = r[a];
                jv[a] = r[6 + a];
            }
            if (MODE == 0) {
                const double ru = r[kRes], rv = r[kRes + 1];
                int n = 0;
#pragma unroll
                for (int i = 0; i < 6; ++i)
#pragma unroll
                    for (int j = i; j < 6; ++j) val[n++] = ju[i] * ju[j] + jv[i] * jv[j];
#pragma unroll
                for (int a = 0; a < 6; ++a) val[21 + a] = ju[a] * ru + jv[a] * rv;
#pragma unroll
                for (int i = 0; i < kTheta; ++i) {
                    const double iu = r[kJi + i], iv = r[kJi + kTheta + i];
#pragma unroll
                    for (int a = 0; a < 6; ++a) val[27 + a * kTheta + i] = ju[a] * iu + jv[a] * iv;
                }
            } else {
                const int pi = pt_idx[o];
                if (in_range(pi, npt)) {
                    const double* __restrict__ x = v + (int64_t)pi * 3;
                    const double su = r[kJp] * x[0] + r[kJp + 1] * x[1] + r[kJp + 2] * x[2];
                    const double sv = r[kJp + 3] * x[0] + r[kJp + 4] * x[1] + r[kJp + 5] * x[2];
#pragma unroll
                    for (int a = 0; a < 6; ++a) val[a] = ju[a] * su + jv[a] * sv;
                }
            }
        }
    }
    const double s = block_values<NV>(val, lds);
    if ((int)threadIdx.x < NV) part[(int64_t)b * NV + threadIdx.x] = s;
}

// 64 lanes per camera: lane k < NV adds value k of the camera's chunk sums in ascending order.  A camera without observations
// writes zeros.
template <int MODE>
__global__ __launch_bounds__(kBlock) void tcal_cam_fold_kernel(const int* __restrict__ chunk_off, int64_t ncam, const double* __restrict__ part,
                                                               double* __restrict__ out36, double* __restrict__ out6, double* __restrict__ out30) {
    constexpr int NV = MODE == 0 ? kBlockVals : 6;
    const int64_t c = blockIdx.x * (int64_t)(kBlock / 64) + (threadIdx.x >> 6);
    const int k = threadIdx.x & 63;
    if (c >= ncam || k >= NV) return;
    const int first = chunk_off[c], last = chunk_off[c + 1];
    double s = 0.0;
    for (int b = first; b < last; ++b) s += part[(int64_t)b * NV + k];
    if (MODE == 0) {
        if (k < 21) {
            int i = 0, j = k;
            while (j >= 6 - i) {
                j -= 6 - i;
                ++i;
            }
            j += i;
            out36[c * 36 + i * 6 + j] = s;
            out36[c * 36 + j * 6 + i] = s;
        } else if (k < 27) {
            out6[c * 6 + (k - 21)] = s;
        } else {
            out30[c * 30 + (k - 27)] = s;
        }
    } else {
        out6[c * 6 + k] = s;
    }
}

// ---- the damped step ------------------------------------------------------------------------------------------------------

// Bd = B with the diagonal scaled by (1 + lam); Minv = Bd^-1 (Gauss-Jordan with partial pivoting, one lane per camera).  A singular
// or non-finite pivot sets bit 0 of *status and leaves the identity as that camera's preconditioner block.
__global__ __launch_bounds__(64) void tcal_damp_cam_kernel(const double* __restrict__ B, int ncam, double lam, double* __restrict__ Bd,
                                                           double* __restrict__ Minv, int* __restrict__ status) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ncam) return;
    double a[6][6], b[6][6];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            double v = B[(int64_t)i * 36 + r * 6 + c];
            if (r == c) v *= 1.0 + lam;
            Bd[(int64_t)i * 36 + r * 6 + c] = v;
            a[r][c] = v;
            b[r][c] = r == c ? 1.0 : 0.0;
        }
    bool bad = false;
#pragma unroll
    for (int col = 0; col < 6; ++col) {
#pragma unroll
        for (int r = col + 1; r < 6; ++r) {
            const bool sw = fabs(a[r][col]) > fabs(a[col][col]);
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                const double ta = a[col][c], tb = b[col][c];
                a[col][c] = sw ? a[r][c] : ta;
                a[r][c] = sw ? ta : a[r][c];
                b[col][c] = sw ? b[r][c] : tb;
                b[r][c] = sw ? tb : b[r][c];
            }
        }
        const double piv = a[col][col];
        if (!(fabs(piv) > 0.0) || !(fabs(piv) < 1e300)) bad = true;
        const double d = 1.0 / piv;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            a[col][c] *= d;
            b[col][c] *= d;
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            if (r == col) continue;
            const double f = a[r][col];
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                a[r][c] -= f * a[col][c];
                b[r][c] -= f * b[col][c];
            }
        }
    }
    if (bad) atomicOr(status, 1);
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) Minv[(int64_t)i * 36 + r * 6 + c] = bad ? (r == c ? 1.0 : 0.0) : b[r][c];
}

// One lane: Gd = G with the diagonal scaled by (1 + lam); Ginv = the inverse of Gd with the rows and columns of the parameters
// that are not free replaced by the identity (the same Gauss-Jordan).  A singular or non-finite pivot sets bit 2 of *status and
// leaves the identity.
__global__ void tcal_damp_theta_kernel(const double* __restrict__ G, double lam, int free_mask, double* __restrict__ Gd, double* __restrict__ Ginv,
                                       int* __restrict__ status) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double a[kTheta][kTheta], b[kTheta][kTheta];
    for (int r = 0; r < kTheta; ++r)
        for (int c = 0; c < kTheta; ++c) {
            double v = G[r * kTheta + c];
            if (r == c) v *= 1.0 + lam;
            Gd[r * kTheta + c] = v;
            const bool fr = ((free_mask >> r) & 1) && ((free_mask >> c) & 1);
            a[r][c] = fr ? v : (r == c ? 1.0 : 0.0);
            b[r][c] = r == c ? 1.0 : 0.0;
        }
    bool bad = false;
    for (int col = 0; col < kTheta; ++col) {
        for (int r = col + 1; r < kTheta; ++r) {
            if (fabs(a[r][col]) > fabs(a[col][col]))
                for (int c = 0; c < kTheta; ++c) {
                    const double ta = a[col][c], tb = b[col][c];
                    a[col][c] = a[r][c]; a[r][c] = ta;
                    b[col][c] = b[r][c]; b[r][c] = tb;
                }
        }
        const double piv = a[col][col];
        if (!(fabs(piv) > 0.0) || !(fabs(piv) < 1e300)) bad = true;
        const double d = 1.0 / piv;
        for (int c = 0; c < kTheta; ++c) {
            a[col][c] *= d;
            b[col][c] *= d;
        }
        for (int r = 0; r < kTheta; ++r) {
            if (r == col) continue;
            const double f = a[r][col];
            for (int c = 0; c < kTheta; ++c) {
                a[r][c] -= f * a[col][c];
                b[r][c] -= f * b[col][c];
            }
        }
    }
    if (bad) atomicOr(status, 4);
    for (int r = 0; r < kTheta; ++r)
        for (int c = 0; c < kTheta; ++c) Ginv[r * kTheta + c] = bad ? (r == c ? 1.0 : 0.0) : b[r][c];
}

// Cd^-1 of the damped symmetric 3 x 3 point blocks (adjugate / determinant).  A vanishing or non-finite determinant sets bit 1 of
// *status and leaves the ZERO block: such a point (all its observations inactive, say) takes no step and adds nothing to S.
__global__ __launch_bounds__(256) void tcal_damp_pt_kernel(const double* __restrict__ C, int64_t npt, double lam, double* __restrict__ Cinv,
                                                           int* __restrict__ status) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= npt) return;
    const double* s = C + i * 9;
    const double a = s[0] * (1.0 + lam), b = s[1], c = s[2], d = s[4] * (1.0 + lam), e = s[5], f = s[8] * (1.0 + lam);
    const double c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d;
    const double c11 = a * f - c * c, c12 = b * c - a * e, c22 = a * d - b * b;
    const double det = a * c00 + b * c01 + c * c02;
    const bool ok = fabs(det) > 1e-300 && fabs(det) < 1e300;
    if (!ok) atomicOr(status, 2);
    const double inv = ok ? 1.0 / det : 0.0;
    double* o = Cinv + i * 9;
    o[0] = ok ? c00 * inv : 0.0; o[1] = ok ? c01 * inv : 0.0; o[2] = ok ? c02 * inv : 0.0;
    o[3] = ok ? c01 * inv : 0.0; o[4] = ok ? c11 * inv : 0.0; o[5] = ok ? c12 * inv : 0.0;
    o[6] = ok ? c02 * inv : 0.0; o[7] = ok ? c12 * inv : 0.0; o[8] = ok ? c22 * inv : 0.0;
}

// y_j = Cinv_j (sign * x_j + g_j)   (g may be null)
__global__ __launch_bounds__(256) void tcal_pt_apply_kernel(const double* __restrict__ Cinv, const double* __restrict__ x, const double* __restrict__ g,
                                                            double sign, int64_t npt, double* __restrict__ y) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= npt) return;
    double v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = sign * x[i * 3 + k] + (g ? g[i * 3 + k] : 0.0);
    const double* m = Cinv + i * 9;
#pragma unroll
    for (int r = 0; r < 3; ++r) y[i * 3 + r] = m[3 * r] * v[0] + m[3 * r + 1] * v[1] + m[3 * r + 2] * v[2];
}

enum { kScalRz = 0, kScalRr = 1, kScalStop2 = 2, kScalStatus = 4, kScalWords = 8 };   // word 4 holds the int32 status

// The vectors of the bordered system hold 6 ncam camera entries, then the 5 of theta.
struct Border {
    const double *Bd, *Minv, *E, *Gd, *Ginv;
    int nc;                                     // 6 ncam
    int fix_first, free_mask;
};

__device__ __forceinline__ bool held(const Border& s, int e) {
    return e < s.nc ? (s.fix_first && e < 6) : !((s.free_mask >> (e - s.nc)) & 1);
}

__device__ __forceinline__ double block6_row(const double* __restrict__ M, const double* __restrict__ v, int e) {
    const int c = e / 6, r = e - 6 * c;
    const double* m = M + (int64_t)c * 36 + 6 * r;
    const double* x = v + (int64_t)c * 6;
    return m[0] * x[0] + m[1] * x[1] + m[2] * x[2] + m[3] * x[3] + m[4] * x[4] + m[5] * x[5];
}

__device__ __forceinline__ double row5(const double* __restrict__ m, const double* __restrict__ x) {
    return m[0] * x[0] + m[1] * x[1] + m[2] * x[2] + m[3] * x[3] + m[4] * x[4];
}

// entry e of blockdiag(Bd^-1, Ginv) r
__device__ __forceinline__ double precond(const Border& s, const double* __restrict__ r, int e) {
    return e < s.nc ? block6_row(s.Minv, r, e) : row5(s.Ginv + (e - s.nc) * kTheta, r + s.nc);
}

// rhs = ((g_c, g_i) - w0) where not held;  x = 0;  r = rhs;  z = M^-1 r where not held;  p = z;  scalars r.z, r.r, stop^2 = tol^2 rhs.rhs
__global__ __launch_bounds__(kCgThreads) void tcal_cg_init_kernel(Border s, const double* __restrict__ gc, const double* __restrict__ gi,
                                                                  const double* __restrict__ w0, double tol2, double* __restrict__ x,
                                                                  double* __restrict__ r, double* __restrict__ p, double* __restrict__ scal) {
    __shared__ double lds[kCgThreads];
    const int n = s.nc + kTheta;
    double rr = 0;
    for (int e = threadIdx.x; e < n; e += kCgThreads) {
        const double v = held(s, e) ? 0.0 : (e < s.nc ? gc[e] : gi[e - s.nc]) - w0[e];
        r[e] = v;
        x[e] = 0.0;
        rr += v * v;
    }
    __threadfence_block();
    __syncthreads();
    rr = cg_block_sum(rr, lds);
    double rz = 0;
    for (int e = threadIdx.x; e < n; e += kCgThreads) {
        const double z = held(s, e) ? 0.0 : precond(s, r, e);
        p[e] = z;
        rz += r[e] * z;
    }
    rz = cg_block_sum(rz, lds);
    if (threadIdx.x == 0) {
        scal[kScalRz] = rz;
        scal[kScalRr] = rr;
        scal[kScalStop2] = tol2 * rr;
    }
}

// One CG iteration, given w = [W; F^T] Cd^-1 [W^T F] p:  Sp = ([Bd E; E^T Gd] p - w) where not held;  alpha = r.z / p.Sp;
// x += alpha p;  r -= alpha Sp;  z = M^-1 r where not held;  beta = r.z' / r.z;  p = z + beta p.  alpha is 0 unless p.Sp > 0 and beta is 0
// unless r.z > 0: with a handful of unknowns the residual can reach exactly 0 between two looks of the host, and 0 / 0 must not follow.
__global__ __launch_bounds__(kCgThreads) void tcal_cg_step_kernel(Border s, const double* __restrict__ w, double* __restrict__ x, double* __restrict__ r,
                                                                  double* __restrict__ p, double* __restrict__ tmp, double* __restrict__ scal) {
    __shared__ double lds[kCgThreads];
    const int n = s.nc + kTheta;
    double etp[kTheta];                                                         // E^T p_c
#pragma unroll
    for (int i = 0; i < kTheta; ++i) {
        double t = 0;
        for (int e = threadIdx.x; e < s.nc; e += kCgThreads) t += s.E[(int64_t)e * kTheta + i] * p[e];
        etp[i] = cg_block_sum(t, lds);
    }
    double pSp = 0;
    for (int e = threadIdx.x; e < n; e += kCgThreads) {
        double sp = 0.0;
        if (!held(s, e)) {
            if (e < s.nc) sp = block6_row(s.Bd, p, e) + row5(s.E + (int64_t)e * kTheta, p + s.nc) - w[e];
            else sp = etp[e - s.nc] + row5(s.Gd + (e - s.nc) * kTheta, p + s.nc) - w[e];
        }
        tmp[e] = sp;
        pSp += p[e] * sp;
    }
    pSp = cg_block_sum(pSp, lds);
    const double rz = scal[kScalRz];
    const double alpha = pSp > 0.0 ? rz / pSp : 0.0;                           // p = 0 after an exact solve (one unknown, say): the iteration is then a no-op
    double rr = 0;
    for (int e = threadIdx.x; e < n; e += kCgThreads) {
        x[e] += alpha * p[e];
        const double v = r[e] - alpha * tmp[e];
        r[e] = v;
        rr += v * v;
    }
    __threadfence_block();
    __syncthreads();
    rr = cg_block_sum(rr, lds);
    double rz_new = 0;
    for (int e = threadIdx.x; e < n; e += kCgThreads) {
        const double z = held(s, e) ? 0.0 : precond(s, r, e);
        tmp[e] = z;
        rz_new += r[e] * z;
    }
    rz_new = cg_block_sum(rz_new, lds);
    const double beta = rz > 0.0 ? rz_new / rz : 0.0;
    for (int e = threadIdx.x; e < n; e += kCgThreads) p[e] = tmp[e] + beta * p[e];
    if (threadIdx.x == 0) {
        scal[kScalRz] = rz_new;
        scal[kScalRr] = rr;
    }
}

// ---- undistortion ---------------------------------------------------------------------------------------------------------

struct Pinhole {
    double fx, fy, cx, cy;
};

// One lane per point.  xd = (u - cx) / f, yd = (v - cy) / (a f), rd = sqrt(xd xd + yd yd); r = rd, then kNewton times
// r2 = r r, g = r (1 + r2 (k1 + k2 r2)) - rd, h = 1 + r2 (3 k1 + 5 k2 r2), r = r - g / h;  s = r / rd (1 when rd = 0);
// out = (float)(fx (xd s) + cx', fy (yd s) + cy').  A non-finite input or result gives NaN in both coordinates.
__global__ __launch_bounds__(kBlock) void tcal_undistort_points_kernel(const float* __restrict__ in, int64_t n, Theta T, Pinhole O,
                                                                       float* __restrict__ out) {
    const int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    if (i >= n) return;
    const double u = (double)in[2 * i], v = (double)in[2 * i + 1];
    const double xd = (u - T.cx) / T.f, yd = (v - T.cy) / (T.a * T.f);
    const double rd = sqrt(xd * xd + yd * yd);
    double r = rd;
#pragma unroll 1
    for (int k = 0; k < kNewton; ++k) {
        const double r2 = r * r;
        const double g = r * (1.0 + r2 * (T.k1 + T.k2 * r2)) - rd;
        const double h = 1.0 + r2 * (3.0 * T.k1 + 5.0 * T.k2 * r2);
        r = r - g / h;
    }
    const double s = rd > 0.0 ? r / rd : 1.0;
    const double ou = O.fx * (xd * s) + O.cx, ov = O.fy * (yd * s) + O.cy;
    const bool ok = finite(u) && finite(v) && finite(ou) && finite(ov);
    const float nanv = __int_as_float(0x7fc00000);
    out[2 * i] = ok ? (float)ou : nanv;
    out[2 * i + 1] = ok ? (float)ov : nanv;
}

// One lane per output pixel (xo, yo) of frame blockIdx.z.  x = (xo - cx') / fx', y = (yo - cy') / fy', r2 = x x + y y,
// d = 1 + k1 r2 + k2 r2 r2, su = (float)(f d x + cx), sv = (float)(a f d y + cy).  Valid iff 0 <= su <= W - 1 and 0 <= sv <= H - 1.
// x0 = floor(su), ax = su - x0, x1 = min(x0 + 1, W - 1) (a tap past the last column has weight 0), likewise in y; in float32
// top = p00 + ax (p10 - p00), bot = p01 + ax (p11 - p01), val = top + ay (bot - top), out = floor(val + 0.5) clamped to 0..255.
// An invalid pixel is 0 in every channel and 0 in the mask.
template <int C>
__global__ __launch_bounds__(kBlock) void tcal_undistort_image_kernel(const uint8_t* __restrict__ src, int64_t H, int64_t W, Theta T, Pinhole O,
                                                                      uint8_t* __restrict__ dst, uint8_t* __restrict__ mask) {
    const int64_t xo = blockIdx.x * (int64_t)64 + (threadIdx.x & 63), yo = blockIdx.y * (int64_t)4 + (threadIdx.x >> 6);
    if (xo >= W || yo >= H) return;
    const int64_t frame = (int64_t)blockIdx.z * H * W;
    const double x = ((double)xo - O.cx) / O.fx, y = ((double)yo - O.cy) / O.fy;
    const double r2 = x * x + y * y;
    const double d = 1.0 + T.k1 * r2 + T.k2 * r2 * r2;
    const float su = (float)(T.f * d * x + T.cx), sv = (float)(T.a * T.f * d * y + T.cy);
    const bool ok = su >= 0.0f && su <= (float)(W - 1) && sv >= 0.0f && sv <= (float)(H - 1);
    uint8_t* o = dst + (frame + yo * W + xo) * C;
    if (mask) mask[frame + yo * W + xo] = ok ? 1 : 0;
    if (!ok) {
#pragma unroll
        for (int c = 0; c < C; ++c) o[c] = 0;
        return;
    }
    const float fx0 = floorf(su), fy0 = floorf(sv);
    const float ax = su - fx0, ay = sv - fy0;
    const int64_t x0 = (int64_t)fx0, y0 = (int64_t)fy0;
    const int64_t x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    const uint8_t* s = src + frame * C;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float p00 = (float)s[(y0 * W + x0) * C + c], p10 = (float)s[(y0 * W + x1) * C + c];
        const float p01 = (float)s[(y1 * W + x0) * C + c], p11 = (float)s[(y1 * W + x1) * C + c];
        const float top = p00 + ax * (p10 - p00), bot = p01 + ax * (p11 - p01);
        const float val = floorf(top + ay * (bot - top) + 0.5f);
        o[c] = (uint8_t)fminf(fmaxf(val, 0.0f), 255.0f);
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------

int64_t blocks_of(int64_t n, int block = kBlock) { return (n + block - 1) / block; }

bool sizes_ok(int64_t ncam, int64_t npt, int64_t nobs) { return ncam >= 1 && ncam < (1 << 24) && npt >= 1 && npt <= INT32_MAX && nobs >= 0 && nobs <= INT32_MAX; }

struct Ws {
    double *rows, *table, *cam_part, *obs_part, *i_part;
    int* chunk_off;
    double *Bd, *Minv, *Cinv, *u, *v, *Gd, *Ginv, *x, *wv, *r, *p, *tmp, *scal;
    int64_t chunk_cap;
    size_t bytes;
};

Ws carve(void* base, int64_t ncam, int64_t npt, int64_t nobs) {
    sfm::Carver c(base);
    Ws w{};
    const size_t n = (size_t)ncam * 6 + kTheta;
    const size_t nblk = (size_t)std::max<int64_t>(blocks_of(nobs), 1);
    w.chunk_cap = nobs / kChunk + ncam;                                         // a camera of d observations has at most d / kChunk + 1 chunks
    w.rows = c.take<double>((size_t)nobs * kRow);
    w.table = c.take<double>((size_t)ncam * kCamStride);
    w.cam_part = c.take<double>((size_t)w.chunk_cap * kBlockVals);
    w.obs_part = c.take<double>(nblk * kObsVals);
    w.i_part = c.take<double>(nblk * kTheta);
    w.chunk_off = c.take<int>((size_t)ncam + 1);
    w.Bd = c.take<double>((size_t)ncam * 36);
    w.Minv = c.take<double>((size_t)ncam * 36);
    w.Cinv = c.take<double>((size_t)npt * 9);
    w.u = c.take<double>((size_t)npt * 3);
    w.v = c.take<double>((size_t)npt * 3);
    w.Gd = c.take<double>(kTheta * kTheta);
    w.Ginv = c.take<double>(kTheta * kTheta);
    w.x = c.take<double>(n);
    w.wv = c.take<double>(n);
    w.r = c.take<double>(n);
    w.p = c.take<double>(n);
    w.tmp = c.take<double>(n);
    w.scal = c.take<double>(kScalWords);
    w.bytes = c.used();
    return w;
}

struct Csr {
    const int *track_off, *cam_idx, *pt_idx, *cam_off, *cam_obs;
};

void launch_scan(hipStream_t s, const Ws& w, const Csr& g, int64_t ncam, int64_t nobs) {
    hipLaunchKernelGGL(tcal_chunk_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, g.cam_off, ncam, (int)nobs, w.chunk_cap, w.chunk_off);
}

unsigned point_grid(int64_t npt) { return (unsigned)blocks_of(npt * kGroup); }

// u = W^T xc + F xi
void launch_wt(hipStream_t s, const Ws& w, const Csr& g, int64_t ncam, int64_t npt, int64_t nobs, const double* xc, const double* xi, double* u) {
    hipLaunchKernelGGL(tcal_point_kernel<1>, dim3(point_grid(npt)), dim3(kBlock), 0, s, g.track_off, g.cam_idx, ncam, npt, (int)nobs, w.rows, xc, xi,
                       (double*)nullptr, u, (double*)nullptr);
}

// (out_c, out_i) = (W v, F^T v)   (chunk_off is in place)
void launch_w(hipStream_t s, const Ws& w, const Csr& g, int64_t ncam, int64_t npt, int64_t nobs, const double* v, double* out_c, double* out_i) {
    if (w.chunk_cap > 0 && nobs > 0)
        hipLaunchKernelGGL(tcal_cam_chunk_kernel<1>, dim3((unsigned)w.chunk_cap), dim3(kBlock), 0, s, g.cam_off, g.cam_obs, g.cam_idx, g.pt_idx,
                           w.chunk_off, ncam, npt, (int)nobs, w.rows, v, w.cam_part);
    hipLaunchKernelGGL(tcal_cam_fold_kernel<1>, dim3((unsigned)blocks_of(ncam, kBlock / 64)), dim3(kBlock), 0, s, w.chunk_off, ncam, w.cam_part,
                       (double*)nullptr, out_c, (double*)nullptr);
    const int64_t nblk = blocks_of(nobs);
    if (nobs > 0)
        hipLaunchKernelGGL(tcal_obs_i_kernel, dim3((unsigned)nblk), dim3(kBlock), 0, s, g.cam_idx, g.pt_idx, ncam, npt, (int)nobs, w.rows, v, w.i_part);
    hipLaunchKernelGGL(tcal_fold_kernel<false>, dim3(1), dim3(kScanThreads), 0, s, w.i_part, nblk, (double*)nullptr, (int*)nullptr, (double*)nullptr,
                       out_i);
}

int check_common(const char* who, int64_t ncam, int64_t npt, int64_t nobs, const Csr& g, const void* ws, size_t ws_bytes) {
    SFM_CHECK_ARG(sizes_ok(ncam, npt, nobs), "%s: bad sizes (1 <= ncam < 2^24, 1 <= npt <= 2^31-1, 0 <= nobs <= 2^31-1)", who);
    SFM_CHECK_ARG(g.track_off && g.cam_off && (nobs == 0 || (g.cam_idx && g.pt_idx && g.cam_obs)), "%s: null pointer", who);
    const size_t need = sfm_track_cal_ws_bytes(ncam, npt, nobs);
    if (!ws || ws_bytes < need) {
        sfm::set_error("%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
        return SFM_ERR_WORKSPACE;
    }
    return SFM_OK;
}

Ws carve_at(void* ws, int64_t ncam, int64_t npt, int64_t nobs) {
    return carve(reinterpret_cast<void*>(sfm::align_up((size_t)(uintptr_t)ws, 256)), ncam, npt, nobs);
}

bool host_finite(double v) { return std::fabs(v) <= kDblMax; }

// theta finite, f > 0, aspect finite and > 0
int check_theta(const char* who, const double* theta, double aspect) {
    SFM_CHECK_ARG(theta, "%s: null pointer (theta)", who);
    for (int k = 0; k < kTheta; ++k) SFM_CHECK_ARG(host_finite(theta[k]), "%s: theta[%d] = %g is not finite", who, k, theta[k]);
    SFM_CHECK_ARG(theta[0] > 0.0, "%s: the focal length f = %g must be > 0", who, theta[0]);
    SFM_CHECK_ARG(aspect > 0.0 && host_finite(aspect), "%s: the aspect a = %g must be finite and > 0", who, aspect);
    return SFM_OK;
}

int check_pinhole(const char* who, const double* K) {
    SFM_CHECK_ARG(K, "%s: null pointer (K_out)", who);
    SFM_CHECK_ARG(host_finite(K[0]) && host_finite(K[4]) && host_finite(K[2]) && host_finite(K[5]) && K[0] > 0.0 && K[4] > 0.0,
                  "%s: K_out must be finite with positive focal lengths", who);
    return SFM_OK;
}

}  // namespace

extern "C" size_t sfm_track_cal_ws_bytes(int64_t ncam, int64_t npt, int64_t nobs) {
    return sizes_ok(ncam, npt, nobs) ? carve(nullptr, ncam, npt, nobs).bytes + 256 : 0;
}

extern "C" int sfm_track_cal_sweep(const double* cams_dev, int64_t ncam, const double* theta_host, double aspect, const double* dtheta_dev,
                                   const double* X_dev, int64_t npt, const float* obs_dev, const int32_t* track_off_dev, const int32_t* cam_idx_dev,
                                   const int32_t* pt_idx_dev, const int32_t* cam_off_dev, const int32_t* cam_obs_dev, int64_t nobs, double huber,
                                   int mode, uint8_t* active_dev, double* JtJ_cam_dev, double* Jtr_cam_dev, double* JtJ_pt_dev, double* Jtr_pt_dev,
                                   double* E_dev, double* G_dev, double* Jtr_theta_dev, double* F_dev, double* stat_dev, int32_t* count_dev,
                                   void* ws_dev, size_t ws_bytes, void* stream) {
    const Csr g{track_off_dev, cam_idx_dev, pt_idx_dev, cam_off_dev, cam_obs_dev};
    int rc = check_common("sfm_track_cal_sweep", ncam, npt, nobs, g, ws_dev, ws_bytes);
    if (rc != SFM_OK) return rc;
    SFM_CHECK_ARG(mode == 0 || mode == 1, "sfm_track_cal_sweep: mode %d must be 0 or 1", mode);
    SFM_CHECK_ARG(huber > 0.0, "sfm_track_cal_sweep: huber %g must be > 0 px (+inf: plain least squares)", huber);
    SFM_CHECK_ARG(cams_dev && X_dev && JtJ_cam_dev && Jtr_cam_dev && JtJ_pt_dev && Jtr_pt_dev && E_dev && G_dev && Jtr_theta_dev && F_dev && stat_dev &&
                      count_dev && (nobs == 0 || (obs_dev && active_dev)),
                  "sfm_track_cal_sweep: null pointer");
    rc = check_theta("sfm_track_cal_sweep", theta_host, aspect);
    if (rc != SFM_OK) return rc;
    const Ws w = carve_at(ws_dev, ncam, npt, nobs);
    const Theta T{theta_host[0], theta_host[1], theta_host[2], theta_host[3], theta_host[4], aspect};
    hipStream_t s = sfm::as_stream(stream);
    const int64_t nblk = blocks_of(nobs);
    hipLaunchKernelGGL(tcal_cam_prepare_kernel, dim3((unsigned)blocks_of(ncam, 64)), dim3(64), 0, s, cams_dev, ncam, w.table);
    launch_scan(s, w, g, ncam, nobs);
    SFM_CHECK_LAUNCH();
    if (nobs > 0) {
        if (mode == 0)
            hipLaunchKernelGGL(tcal_obs_kernel<0>, dim3((unsigned)nblk), dim3(kBlock), 0, s, w.table, T, dtheta_dev, ncam, X_dev, npt, obs_dev,
                               cam_idx_dev, pt_idx_dev, (int)nobs, huber, active_dev, w.rows, w.obs_part);
        else
            hipLaunchKernelGGL(tcal_obs_kernel<1>, dim3((unsigned)nblk), dim3(kBlock), 0, s, w.table, T, dtheta_dev, ncam, X_dev, npt, obs_dev,
                               cam_idx_dev, pt_idx_dev, (int)nobs, huber, active_dev, w.rows, w.obs_part);
        SFM_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(tcal_fold_kernel<true>, dim3(1), dim3(kScanThreads), 0, s, w.obs_part, nblk, stat_dev, count_dev, G_dev, Jtr_theta_dev);
    hipLaunchKernelGGL(tcal_point_kernel<0>, dim3(point_grid(npt)), dim3(kBlock), 0, s, track_off_dev, cam_idx_dev, ncam, npt, (int)nobs, w.rows,
                       (const double*)nullptr, (const double*)nullptr, JtJ_pt_dev, Jtr_pt_dev, F_dev);
    SFM_CHECK_LAUNCH();
    if (nobs > 0 && w.chunk_cap > 0) {
        hipLaunchKernelGGL(tcal_cam_chunk_kernel<0>, dim3((unsigned)w.chunk_cap), dim3(kBlock), 0, s, cam_off_dev, cam_obs_dev, cam_idx_dev, pt_idx_dev,
                           w.chunk_off, ncam, npt, (int)nobs, w.rows, (const double*)nullptr, w.cam_part);
        SFM_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(tcal_cam_fold_kernel<0>, dim3((unsigned)blocks_of(ncam, kBlock / 64)), dim3(kBlock), 0, s, w.chunk_off, ncam, w.cam_part,
                       JtJ_cam_dev, Jtr_cam_dev, E_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" int sfm_track_cal_product(int64_t ncam, int64_t npt, const int32_t* track_off_dev, const int32_t* cam_idx_dev, const int32_t* pt_idx_dev,
                                     const int32_t* cam_off_dev, const int32_t* cam_obs_dev, int64_t nobs, int mode, const double* in_dev,
                                     const double* in_theta_dev, double* out_dev, double* out_theta_dev, void* ws_dev, size_t ws_bytes,
                                     void* stream) {
    const Csr g{track_off_dev, cam_idx_dev, pt_idx_dev, cam_off_dev, cam_obs_dev};
    const int rc = check_common("sfm_track_cal_product", ncam, npt, nobs, g, ws_dev, ws_bytes);
    if (rc != SFM_OK) return rc;
    SFM_CHECK_ARG(mode == 0 || mode == 1, "sfm_track_cal_product: mode %d must be 0 or 1", mode);
    SFM_CHECK_ARG(in_dev && out_dev && (mode == 0 ? in_theta_dev != nullptr : out_theta_dev != nullptr), "sfm_track_cal_product: null pointer");
    const Ws w = carve_at(ws_dev, ncam, npt, nobs);
    hipStream_t s = sfm::as_stream(stream);
    if (mode == 0) {
        launch_wt(s, w, g, ncam, npt, nobs, in_dev, in_theta_dev, out_dev);
    } else {
        launch_scan(s, w, g, ncam, nobs);
        launch_w(s, w, g, ncam, npt, nobs, in_dev, out_dev, out_theta_dev);
    }
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

// Waits for `stream` once per look at r.r (before iterations 0, 5, 10, ... while iterations remain); the status word comes with the
// first look.  dc_dev, dtheta_dev and dp_dev are complete in stream order, not at return.
extern "C" int sfm_track_cal_step(int64_t ncam, int64_t npt, const int32_t* track_off_dev, const int32_t* cam_idx_dev, const int32_t* pt_idx_dev,
                                  const int32_t* cam_off_dev, const int32_t* cam_obs_dev, int64_t nobs, const double* JtJ_cam_dev,
                                  const double* Jtr_cam_dev, const double* JtJ_pt_dev, const double* Jtr_pt_dev, const double* E_dev,
                                  const double* G_dev, const double* Jtr_theta_dev, double lam, int free_mask, int fix_first_camera, double cg_tol,
                                  int cg_iters, double* dc_dev, double* dtheta_dev, double* dp_dev, int32_t* iters_host, int32_t* status_host,
                                  void* ws_dev, size_t ws_bytes, void* stream) {
    const Csr g{track_off_dev, cam_idx_dev, pt_idx_dev, cam_off_dev, cam_obs_dev};
    const int rc = check_common("sfm_track_cal_step", ncam, npt, nobs, g, ws_dev, ws_bytes);
    if (rc != SFM_OK) return rc;
    SFM_CHECK_ARG(cg_iters >= 0 && lam >= 0.0 && cg_tol >= 0.0, "sfm_track_cal_step: cg_iters %d, lam %g, cg_tol %g: each must be >= 0", cg_iters, lam,
                  cg_tol);
    SFM_CHECK_ARG(free_mask >= 0 && free_mask <= 31, "sfm_track_cal_step: free %d must be a mask of the 5 parameters (0..31)", free_mask);
    SFM_CHECK_ARG(JtJ_cam_dev && Jtr_cam_dev && JtJ_pt_dev && Jtr_pt_dev && E_dev && G_dev && Jtr_theta_dev && dc_dev && dtheta_dev && dp_dev,
                  "sfm_track_cal_step: null pointer");
    const Ws w = carve_at(ws_dev, ncam, npt, nobs);
    hipStream_t s = sfm::as_stream(stream);
    const int nc = (int)ncam * 6;
    const Border sys{w.Bd, w.Minv, E_dev, w.Gd, w.Ginv, nc, fix_first_camera ? 1 : 0, free_mask};
    int* status = reinterpret_cast<int*>(w.scal + kScalStatus);
    SFM_CHECK_HIP(hipMemsetAsync(w.scal, 0, sizeof(double) * kScalWords, s));
    launch_scan(s, w, g, ncam, nobs);
    hipLaunchKernelGGL(tcal_damp_cam_kernel, dim3((unsigned)blocks_of(ncam, 64)), dim3(64), 0, s, JtJ_cam_dev, (int)ncam, lam, w.Bd, w.Minv, status);
    hipLaunchKernelGGL(tcal_damp_theta_kernel, dim3(1), dim3(64), 0, s, G_dev, lam, free_mask, w.Gd, w.Ginv, status);
    const unsigned pblocks = (unsigned)blocks_of(npt);
    hipLaunchKernelGGL(tcal_damp_pt_kernel, dim3(pblocks), dim3(256), 0, s, JtJ_pt_dev, npt, lam, w.Cinv, status);
    SFM_CHECK_LAUNCH();
    // rhs = (g_c, g_i) - [W; F^T] Cd^-1 g_p
    hipLaunchKernelGGL(tcal_pt_apply_kernel, dim3(pblocks), dim3(256), 0, s, w.Cinv, Jtr_pt_dev, (const double*)nullptr, 1.0, npt, w.v);
    launch_w(s, w, g, ncam, npt, nobs, w.v, w.wv, w.wv + nc);
    hipLaunchKernelGGL(tcal_cg_init_kernel, dim3(1), dim3(kCgThreads), 0, s, sys, Jtr_cam_dev, Jtr_theta_dev, w.wv, cg_tol * cg_tol, w.x, w.r, w.p,
                       w.scal);
    SFM_CHECK_LAUNCH();
    double h[kScalWords] = {0};
    bool looked = false;
    int it = 0;
    while (it < cg_iters) {
        if (it % 5 == 0) {
            SFM_CHECK_HIP(hipMemcpyAsync(h, w.scal, sizeof(h), hipMemcpyDeviceToHost, s));
            SFM_CHECK_HIP(sfm::stream_sync(s));
            looked = true;
            if (h[kScalRr] <= h[kScalStop2]) break;
        }
        launch_wt(s, w, g, ncam, npt, nobs, w.p, w.p + nc, w.u);                                                // u = W^T p_c + F p_i
        hipLaunchKernelGGL(tcal_pt_apply_kernel, dim3(pblocks), dim3(256), 0, s, w.Cinv, w.u, (const double*)nullptr, 1.0, npt, w.v);
        launch_w(s, w, g, ncam, npt, nobs, w.v, w.wv, w.wv + nc);                                               // w = [W; F^T] Cd^-1 u
        hipLaunchKernelGGL(tcal_cg_step_kernel, dim3(1), dim3(kCgThreads), 0, s, sys, w.wv, w.x, w.r, w.p, w.tmp, w.scal);
        SFM_CHECK_LAUNCH();
        ++it;
    }
    // dp = Cd^-1 (g_p - W^T dc - F di)
    launch_wt(s, w, g, ncam, npt, nobs, w.x, w.x + nc, w.u);
    hipLaunchKernelGGL(tcal_pt_apply_kernel, dim3(pblocks), dim3(256), 0, s, w.Cinv, w.u, Jtr_pt_dev, -1.0, npt, dp_dev);
    SFM_CHECK_LAUNCH();
    SFM_CHECK_HIP(hipMemcpyAsync(dc_dev, w.x, sizeof(double) * nc, hipMemcpyDeviceToDevice, s));
    SFM_CHECK_HIP(hipMemcpyAsync(dtheta_dev, w.x + nc, sizeof(double) * kTheta, hipMemcpyDeviceToDevice, s));
    if (!looked) {                                                              // cg_iters == 0: the status still has to come back
        SFM_CHECK_HIP(hipMemcpyAsync(h, w.scal, sizeof(h), hipMemcpyDeviceToHost, s));
        SFM_CHECK_HIP(sfm::stream_sync(s));
    }
    int st = 0;
    memcpy(&st, &h[kScalStatus], sizeof(st));
    if (iters_host) *iters_host = it;
    if (status_host) *status_host = st;
    return SFM_OK;
}

extern "C" int sfm_undistort_points(const float* px_dev, int64_t n, const double* theta_host, double aspect, const double* K_out_host,
                                    float* out_dev, void* stream) {
    SFM_CHECK_ARG(n >= 0 && n <= INT32_MAX, "sfm_undistort_points: n %lld outside 0..2^31-1", (long long)n);
    int rc = check_theta("sfm_undistort_points", theta_host, aspect);
    if (rc != SFM_OK) return rc;
    rc = check_pinhole("sfm_undistort_points", K_out_host);
    if (rc != SFM_OK) return rc;
    SFM_CHECK_ARG(n == 0 || (px_dev && out_dev), "sfm_undistort_points: null pointer");
    if (n == 0) return SFM_OK;
    const Theta T{theta_host[0], theta_host[1], theta_host[2], theta_host[3], theta_host[4], aspect};
    const Pinhole O{K_out_host[0], K_out_host[4], K_out_host[2], K_out_host[5]};
    hipLaunchKernelGGL(tcal_undistort_points_kernel, dim3((unsigned)blocks_of(n)), dim3(kBlock), 0, sfm::as_stream(stream), px_dev, n, T, O, out_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" int sfm_undistort_image(const uint8_t* src_dev, int64_t nimg, int64_t H, int64_t W, int channels, const double* theta_host, double aspect,
                                   const double* K_out_host, uint8_t* dst_dev, uint8_t* mask_dev, void* stream) {
    SFM_CHECK_ARG(nimg >= 0 && nimg <= 65535 && H >= 1 && H <= 65536 && W >= 1 && W <= 65536,
                  "sfm_undistort_image: bad sizes (0 <= nimg <= 65535, 1 <= H, W <= 65536)");
    SFM_CHECK_ARG(channels == 1 || channels == 3, "sfm_undistort_image: channels %d must be 1 or 3", channels);
    int rc = check_theta("sfm_undistort_image", theta_host, aspect);
    if (rc != SFM_OK) return rc;
    rc = check_pinhole("sfm_undistort_image", K_out_host);
    if (rc != SFM_OK) return rc;
    SFM_CHECK_ARG(nimg == 0 || (src_dev && dst_dev && src_dev != dst_dev), "sfm_undistort_image: null pointer, or src and dst are the same buffer");
    if (nimg == 0) return SFM_OK;
    const Theta T{theta_host[0], theta_host[1], theta_host[2], theta_host[3], theta_host[4], aspect};
    const Pinhole O{K_out_host[0], K_out_host[4], K_out_host[2], K_out_host[5]};
    const dim3 grid((unsigned)blocks_of(W, 64), (unsigned)blocks_of(H, 4), (unsigned)nimg);
    if (channels == 1)
        hipLaunchKernelGGL(tcal_undistort_image_kernel<1>, grid, dim3(kBlock), 0, sfm::as_stream(stream), src_dev, H, W, T, O, dst_dev, mask_dev);
    else
        hipLaunchKernelGGL(tcal_undistort_image_kernel<3>, grid, dim3(kBlock), 0, sfm::as_stream(stream), src_dev, H, W, T, O, dst_dev, mask_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}
