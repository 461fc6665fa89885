// Bundle adjustment of feature tracks: fixed-order sparse Schur Levenberg-Marquardt with a Huber loss (include/sfm_hip.h, "TRACKS-BA";
// docs/tracks.md §9).
//   sfm_track_ba_sweep    linearisation at (cams, X): a row of 20 doubles per observation (sqrt(w) Jc, sqrt(w) Jp, sqrt(w) r), the
//                         active set, the normal-equation blocks of both sides, the robust cost and the counts
//   sfm_track_ba_product  u = W^T x and w = W v over the stored rows: streaming reads, no camera table, no Rodrigues
//   sfm_track_ba_step     one damped step: block inverses, block-Jacobi PCG on the reduced camera system with the two products,
//                         back-substitution; the scalars stay on the device, the host reads r.r before iterations 0, 5, 10, ...
// THERE ARE NO FLOATING-POINT ATOMICS IN THIS FILE.  Every sum is a fixed function of the CSR and of the data:
//   point side   a group of kGroup lanes per track, lane l adds observations l, l + kGroup, ... of the track ascending, the kGroup
//                partial sums meet in a xor tree (strides kGroup / 2 .. 1)
//   camera side  a camera's list (cam_off / cam_obs) is cut into chunks of kChunk observations; one workgroup sums a chunk (a lane
//                per observation, xor tree over the wave, the four waves in ascending order); a fold kernel adds a camera's chunk
//                sums in ascending order
//   cost         per workgroup of kBlock observations the same tree, then one workgroup adds the block sums (lane l blocks l,
//                l + 1024, ... ascending, then a tree)
// None depends on the grid, on the waves in flight or on the order in which workgroups finish.  The sums are held to a tolerance
// against tests/np_track_ba.py, not to the bit (the compiler may fuse a * b + c here).
// Rodrigues with its derivative, the small block kernels and the single-workgroup CG kernels are copies of csrc/ba_schur.hip's, the
// segmented scan is a copy of csrc/tracks_refine.hip's, as the mesh files copy theirs.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cstring>

#include "common.h"

#pragma clang fp contract(fast)

#ifndef SFM_TBA_GROUP
#define SFM_TBA_GROUP 8                         // lanes per track on the point side: 1, 8 and 64 measured (docs/tracks.md §9.4)
#endif

namespace {

constexpr int kRow = 20;                        // doubles per observation: Jc (2 x 6), Jp (2 x 3), r (2), each times sqrt(w)
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kGroup = SFM_TBA_GROUP;
constexpr int kChunk = kBlock;                  // observations of a camera one workgroup sums
constexpr int kCamStride = 40;
constexpr int kBlockVals = 27;                  // the upper triangle of a 6 x 6 block (21) and the gradient (6)
constexpr int kCostVals = 5;                    // robust cost, plain sum of e^2, active, crossed, outliers
constexpr int kScanThreads = 1024;
constexpr int kSearchSteps = 26;                // binary search over at most 2^24 + 1 chunk offsets
constexpr int kCgThreads = 1024;
constexpr double kDblMax = 1.7976931348623157e308;
static_assert(kGroup == 1 || kGroup == 2 || kGroup == 4 || kGroup == 8 || kGroup == 16 || kGroup == 32 || kGroup == 64, "kGroup divides a wave");

struct Intrin {
    double fx, fy, cx, cy;
};

__device__ inline bool in_range(int a, int64_t n) { return a >= 0 && (int64_t)a < n; }

__device__ inline bool finite(double v) { return fabs(v) <= kDblMax; }

// [lo, hi) of row i of a CSR nobody vouches for: 0 <= lo <= hi <= n
__device__ inline void csr_range(const int* __restrict__ off, int64_t i, int n, int& lo, int& hi) {
    lo = min(max(off[i], 0), n);
    hi = min(max(off[i + 1], lo), n);
}

__device__ void rodrigues_tba(const double* __restrict__ rv, double* __restrict__ R, double* __restrict__ J) {
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
__global__ void tba_cam_prepare_kernel(const double* __restrict__ cams, int64_t ncam, double* __restrict__ table) {
    const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (c >= ncam) return;
    double R[9], J[27];
    rodrigues_tba(cams + 6 * c, R, J);
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

// ---- the rows -------------------------------------------------------------------------------------------------------------

// One lane per observation: the row, the active byte (MODE 0) and the cost terms; a workgroup's cost terms go to cost_part.
template <int MODE>
__global__ __launch_bounds__(kBlock) void tba_obs_kernel(const double* __restrict__ table, Intrin K, int64_t ncam, const double* __restrict__ X,
                                                         int64_t npt, const float* __restrict__ obs, const int* __restrict__ cam_idx,
                                                         const int* __restrict__ pt_idx, int nobs, double huber,
                                                         unsigned char* __restrict__ active, double* __restrict__ rows,
                                                         double* __restrict__ cost_part) {
    __shared__ double lds[kWaves][kCostVals];
    const int64_t o = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    double val[kCostVals] = {0, 0, 0, 0, 0};
    if (o < nobs) {
        const int ci = cam_idx[o], pi = pt_idx[o];
        const bool inr = in_range(ci, ncam) && in_range(pi, npt);
        double row[kRow];
#pragma unroll
        for (int k = 0; k < kRow; ++k) row[k] = 0.0;
        bool ok = false;
        double ru = 0, rv = 0;
        double Ju[6], Jv[6], Pu[3], Pv[3];
        if (inr) {
            const double* __restrict__ e = table + (int64_t)ci * kCamStride;
            const double Xw = X[3 * (int64_t)pi], Yw = X[3 * (int64_t)pi + 1], Zw = X[3 * (int64_t)pi + 2];
            double x = e[0] * Xw + e[1] * Yw + e[2] * Zw + e[9];
            double y = e[3] * Xw + e[4] * Yw + e[5] * Zw + e[10];
            const double zc = e[6] * Xw + e[7] * Yw + e[8] * Zw + e[11];
            const double z = 1. / zc;
            x *= z;
            y *= z;
            ru = (K.fx * x + K.cx) - (double)obs[2 * o];
            rv = (K.fy * y + K.cy) - (double)obs[2 * o + 1];
            ok = zc > 0.0 && zc <= kDblMax && finite(ru) && finite(rv);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double* d = e + 12 + 9 * j;
                const double dx0 = Xw * d[0] + Yw * d[1] + Zw * d[2];
                const double dy0 = Xw * d[3] + Yw * d[4] + Zw * d[5];
                const double dz0 = Xw * d[6] + Yw * d[7] + Zw * d[8];
                Ju[j] = K.fx * (z * (dx0 - x * dz0));
                Jv[j] = K.fy * (z * (dy0 - y * dz0));
            }
            Ju[3] = K.fx * z; Ju[4] = 0;        Ju[5] = K.fx * (-x * z);
            Jv[3] = 0;        Jv[4] = K.fy * z; Jv[5] = K.fy * (-y * z);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                Pu[k] = K.fx * (z * (e[k] - x * e[6 + k]));
                Pv[k] = K.fy * (z * (e[3 + k] - y * e[6 + k]));
            }
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
            for (int k = 0; k < 3; ++k) {
                row[12 + k] = sw * Pu[k];
                row[15 + k] = sw * Pv[k];
            }
            row[18] = sw * ru;
            row[19] = sw * rv;
        }
        double2* dst = reinterpret_cast<double2*>(rows + o * kRow);             // 160-byte rows at a 256-byte aligned base
#pragma unroll
        for (int k = 0; k < kRow / 2; ++k) dst[k] = make_double2(row[2 * k], row[2 * k + 1]);
    }
    const double s = block_values<kCostVals>(val, lds);
    if (threadIdx.x < kCostVals) cost_part[(int64_t)blockIdx.x * kCostVals + threadIdx.x] = s;
}

// One workgroup: lane l adds the block sums l, l + 1024, ... ascending, then a tree -> stat (2 doubles), count (3 ints).
__global__ __launch_bounds__(kScanThreads) void tba_cost_fold_kernel(const double* __restrict__ cost_part, int64_t nblk, double* __restrict__ stat,
                                                                     int* __restrict__ count) {
    __shared__ double lds[kCostVals][kScanThreads];
    double s[kCostVals] = {0, 0, 0, 0, 0};
    for (int64_t b = threadIdx.x; b < nblk; b += kScanThreads)
#pragma unroll
        for (int k = 0; k < kCostVals; ++k) s[k] += cost_part[b * kCostVals + k];
#pragma unroll
    for (int k = 0; k < kCostVals; ++k) lds[k][threadIdx.x] = s[k];
    __syncthreads();
    for (int m = kScanThreads / 2; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m)
#pragma unroll
            for (int k = 0; k < kCostVals; ++k) lds[k][threadIdx.x] += lds[k][threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x < 2) stat[threadIdx.x] = lds[threadIdx.x][0];
    else if (threadIdx.x < kCostVals) count[threadIdx.x - 2] = (int)lds[threadIdx.x][0];
}

// ---- point side -----------------------------------------------------------------------------------------------------------

// MODE 0: C_t (9) and g_p (3) from the rows.  MODE 1: u_t = sum Jp^T (Jc x[cam]).
template <int MODE>
__global__ __launch_bounds__(kBlock) void tba_point_kernel(const int* __restrict__ track_off, const int* __restrict__ cam_idx, int64_t ncam, int64_t npt,
                                                           int nobs, const double* __restrict__ rows, const double* __restrict__ xc,
                                                           double* __restrict__ out9, double* __restrict__ out3) {
    constexpr int NV = MODE == 0 ? 9 : 3;
    const int64_t id = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    const int64_t t = id / kGroup;
    const int l = (int)(id % kGroup);
    double acc[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = 0.0;
    if (t < npt) {
        int lo, hi;
        csr_range(track_off, t, nobs, lo, hi);
        for (int o = lo + l; o < hi; o += kGroup) {
            const double* __restrict__ r = rows + (int64_t)o * kRow;
            const double pu0 = r[12], pu1 = r[13], pu2 = r[14], pv0 = r[15], pv1 = r[16], pv2 = r[17];
            if (MODE == 0) {
                const double ru = r[18], rv = r[19];
                acc[0] += pu0 * pu0 + pv0 * pv0;
                acc[1] += pu0 * pu1 + pv0 * pv1;
                acc[2] += pu0 * pu2 + pv0 * pv2;
                acc[3] += pu1 * pu1 + pv1 * pv1;
                acc[4] += pu1 * pu2 + pv1 * pv2;
                acc[5] += pu2 * pu2 + pv2 * pv2;
                acc[6] += pu0 * ru + pv0 * rv;
                acc[7] += pu1 * ru + pv1 * rv;
                acc[8] += pu2 * ru + pv2 * rv;
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
        } else {
            out3[t * 3] = acc[0]; out3[t * 3 + 1] = acc[1]; out3[t * 3 + 2] = acc[2];
        }
    }
}

// ---- camera side ----------------------------------------------------------------------------------------------------------

// chunk_off[c] = the chunks of the cameras before c, chunk_off[ncam] = all of them, none above `cap` (a CSR whose ranges overlap
// can ask for more chunks than the workspace holds: the cameras at the end then go short, nothing is written outside it).
__global__ __launch_bounds__(kScanThreads) void tba_chunk_scan_kernel(const int* __restrict__ cam_off, int64_t ncam, int nobs, int64_t cap,
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

// Workgroup b sums chunk b: its camera c has chunk_off[c] <= b < chunk_off[c + 1].  MODE 0: the upper triangle of B_c and g_c (27
// values); MODE 1: w_c = sum Jc^T (Jp v[point]) (6 values).  An entry of cam_obs outside 0..nobs-1, or naming an observation of
// another camera, adds nothing.
template <int MODE>
__global__ __launch_bounds__(kBlock) void tba_cam_chunk_kernel(const int* __restrict__ cam_off, const int* __restrict__ cam_obs,
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
                const double ru = r[18], rv = r[19];
                int n = 0;
#pragma unroll
                for (int i = 0; i < 6; ++i)
#pragma unroll
                    for (int j = i; j < 6; ++j) val[n++] = ju[i] * ju[j] + jv[i] * jv[j];
#pragma unroll
                for (int a = 0; a < 6; ++a) val[21 + a] = ju[a] * ru + jv[a] * rv;
            } else {
                const int pi = pt_idx[o];
                if (in_range(pi, npt)) {
                    const double* __restrict__ x = v + (int64_t)pi * 3;
                    const double su = r[12] * x[0] + r[13] * x[1] + r[14] * x[2];
                    const double sv = r[15] * x[0] + r[16] * x[1] + r[17] * x[2];
#pragma unroll
                    for (int a = 0; a < 6; ++a) val[a] = ju[a] * su + jv[a] * sv;
                }
            }
        }
    }
    const double s = block_values<NV>(val, lds);
    if ((int)threadIdx.x < NV) part[(int64_t)b * NV + threadIdx.x] = s;
}

// 32 lanes per camera: lane k < NV adds value k of the camera's chunk sums in ascending order.  A camera without observations
// writes zeros.
template <int MODE>
__global__ __launch_bounds__(kBlock) void tba_cam_fold_kernel(const int* __restrict__ chunk_off, int64_t ncam, const double* __restrict__ part,
                                                              double* __restrict__ out36, double* __restrict__ out6) {
    constexpr int NV = MODE == 0 ? kBlockVals : 6;
    const int64_t c = blockIdx.x * (int64_t)(kBlock / 32) + (threadIdx.x >> 5);
    const int k = threadIdx.x & 31;
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
        } else {
            out6[c * 6 + (k - 21)] = s;
        }
    } else {
        out6[c * 6 + k] = s;
    }
}

// ---- the damped step (copies of csrc/ba_schur.hip's kernels) ---------------------------------------------------------------

// Bd = B with the diagonal scaled by (1 + lam); Minv = Bd^-1 (Gauss-Jordan with partial pivoting, one lane per camera).  A singular
// or non-finite pivot sets bit 0 of *status and leaves the identity as that camera's preconditioner block.
__global__ __launch_bounds__(64) void tba_damp_cam_kernel(const double* __restrict__ B, int ncam, double lam, double* __restrict__ Bd,
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

// Cd^-1 of the damped symmetric 3 x 3 point blocks (adjugate / determinant).  A vanishing or non-finite determinant sets bit 1 of
// *status and leaves the ZERO block: such a point (all its observations inactive, say) takes no step and adds nothing to S.
__global__ __launch_bounds__(256) void tba_damp_pt_kernel(const double* __restrict__ C, int64_t npt, double lam, double* __restrict__ Cinv,
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
__global__ __launch_bounds__(256) void tba_pt_apply_kernel(const double* __restrict__ Cinv, const double* __restrict__ x, const double* __restrict__ g,
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

__device__ __forceinline__ double block6_row(const double* __restrict__ M, const double* __restrict__ v, int e) {
    const int c = e / 6, r = e - 6 * c;
    const double* m = M + (int64_t)c * 36 + 6 * r;
    const double* x = v + (int64_t)c * 6;
    return m[0] * x[0] + m[1] * x[1] + m[2] * x[2] + m[3] * x[3] + m[4] * x[4] + m[5] * x[5];
}

// rhs = (g_c - w0) * free;  x = 0;  r = rhs;  z = Minv r * free;  p = z;  scalars r.z, r.r, stop^2 = tol^2 rhs.rhs
__global__ __launch_bounds__(kCgThreads) void tba_cg_init_kernel(const double* __restrict__ gc, const double* __restrict__ w0,
                                                                 const double* __restrict__ Minv, int n, int fix_first, double tol2,
                                                                 double* __restrict__ x, double* __restrict__ r, double* __restrict__ p,
                                                                 double* __restrict__ scal) {
    __shared__ double lds[kCgThreads];
    double rr = 0;
    for (int e = threadIdx.x; e < n; e += kCgThreads) {
        const double v = (fix_first && e < 6) ? 0.0 : gc[e] - w0[e];
        r[e] = v;
        x[e] = 0.0;
        rr += v * v;
    }
    __threadfence_block();
    __syncthreads();
    rr = cg_block_sum(rr, lds);
    double rz = 0;
    for (int e = threadIdx.x; e < n; e += kCgThreads) {
        const double z = (fix_first && e < 6) ? 0.0 : block6_row(Minv, r, e);
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

// One CG iteration on the camera side, given w = W Cd^-1 W^T p:  Sp = (Bd p - w) * free;  alpha = r.z / p.Sp;  x += alpha p;
// r -= alpha Sp;  z = Minv r * free;  beta = r.z' / r.z;  p = z + beta p
__global__ __launch_bounds__(kCgThreads) void tba_cg_step_kernel(const double* __restrict__ Bd, const double* __restrict__ Minv,
                                                                 const double* __restrict__ w, int n, int fix_first, double* __restrict__ x,
                                                                 double* __restrict__ r, double* __restrict__ p, double* __restrict__ tmp,
                                                                 double* __restrict__ scal) {
    __shared__ double lds[kCgThreads];
    double pSp = 0;
    for (int e = threadIdx.x; e < n; e += kCgThreads) {
        const double sp = (fix_first && e < 6) ? 0.0 : block6_row(Bd, p, e) - w[e];
        tmp[e] = sp;
        pSp += p[e] * sp;
    }
    pSp = cg_block_sum(pSp, lds);
    const double rz = scal[kScalRz];
    const double alpha = rz / pSp;
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
        const double z = (fix_first && e < 6) ? 0.0 : block6_row(Minv, r, e);
        tmp[e] = z;
        rz_new += r[e] * z;
    }
    rz_new = cg_block_sum(rz_new, lds);
    const double beta = rz_new / rz;
    for (int e = threadIdx.x; e < n; e += kCgThreads) p[e] = tmp[e] + beta * p[e];
    if (threadIdx.x == 0) {
        scal[kScalRz] = rz_new;
        scal[kScalRr] = rr;
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------

int64_t blocks_of(int64_t n, int block = kBlock) { return (n + block - 1) / block; }

bool sizes_ok(int64_t ncam, int64_t npt, int64_t nobs) { return ncam >= 1 && ncam < (1 << 24) && npt >= 1 && npt <= INT32_MAX && nobs >= 0 && nobs <= INT32_MAX; }

struct Ws {
    double *rows, *table, *cam_part, *cost_part;
    int* chunk_off;
    double *Bd, *Minv, *Cinv, *u, *v, *wv, *r, *p, *tmp, *scal;
    int64_t chunk_cap;
    size_t bytes;
};

Ws carve(void* base, int64_t ncam, int64_t npt, int64_t nobs) {
    sfm::Carver c(base);
    Ws w{};
    w.chunk_cap = nobs / kChunk + ncam;                                         // a camera of d observations has at most d / kChunk + 1 chunks
    w.rows = c.take<double>((size_t)nobs * kRow);
    w.table = c.take<double>((size_t)ncam * kCamStride);
    w.cam_part = c.take<double>((size_t)w.chunk_cap * kBlockVals);
    w.cost_part = c.take<double>((size_t)std::max<int64_t>(blocks_of(nobs), 1) * kCostVals);
    w.chunk_off = c.take<int>((size_t)ncam + 1);
    w.Bd = c.take<double>((size_t)ncam * 36);
    w.Minv = c.take<double>((size_t)ncam * 36);
    w.Cinv = c.take<double>((size_t)npt * 9);
    w.u = c.take<double>((size_t)npt * 3);
    w.v = c.take<double>((size_t)npt * 3);
    w.wv = c.take<double>((size_t)ncam * 6);
    w.r = c.take<double>((size_t)ncam * 6);
    w.p = c.take<double>((size_t)ncam * 6);
    w.tmp = c.take<double>((size_t)ncam * 6);
    w.scal = c.take<double>(kScalWords);
    w.bytes = c.used();
    return w;
}

struct Csr {
    const int *track_off, *cam_idx, *pt_idx, *cam_off, *cam_obs;
};

void launch_scan(hipStream_t s, const Ws& w, const Csr& g, int64_t ncam, int64_t nobs) {
    hipLaunchKernelGGL(tba_chunk_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, g.cam_off, ncam, (int)nobs, w.chunk_cap, w.chunk_off);
}

unsigned point_grid(int64_t npt) { return (unsigned)blocks_of(npt * kGroup); }

// u = W^T x
void launch_wt(hipStream_t s, const Ws& w, const Csr& g, int64_t ncam, int64_t npt, int64_t nobs, const double* x, double* u) {
    hipLaunchKernelGGL(tba_point_kernel<1>, dim3(point_grid(npt)), dim3(kBlock), 0, s, g.track_off, g.cam_idx, ncam, npt, (int)nobs, w.rows, x,
                       (double*)nullptr, u);
}

// w = W v   (chunk_off is in place)
void launch_w(hipStream_t s, const Ws& w, const Csr& g, int64_t ncam, int64_t npt, int64_t nobs, const double* v, double* out) {
    if (w.chunk_cap > 0 && nobs > 0)
        hipLaunchKernelGGL(tba_cam_chunk_kernel<1>, dim3((unsigned)w.chunk_cap), dim3(kBlock), 0, s, g.cam_off, g.cam_obs, g.cam_idx, g.pt_idx,
                           w.chunk_off, ncam, npt, (int)nobs, w.rows, v, w.cam_part);
    hipLaunchKernelGGL(tba_cam_fold_kernel<1>, dim3((unsigned)blocks_of(ncam, kBlock / 32)), dim3(kBlock), 0, s, w.chunk_off, ncam, w.cam_part,
                       (double*)nullptr, out);
}

int check_common(const char* who, int64_t ncam, int64_t npt, int64_t nobs, const Csr& g, const void* ws, size_t ws_bytes) {
    SFM_CHECK_ARG(sizes_ok(ncam, npt, nobs), "%s: bad sizes (1 <= ncam < 2^24, 1 <= npt <= 2^31-1, 0 <= nobs <= 2^31-1)", who);
    SFM_CHECK_ARG(g.track_off && g.cam_off && (nobs == 0 || (g.cam_idx && g.pt_idx && g.cam_obs)), "%s: null pointer", who);
    const size_t need = sfm_track_ba_ws_bytes(ncam, npt, nobs);
    if (!ws || ws_bytes < need) {
        sfm::set_error("%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
        return SFM_ERR_WORKSPACE;
    }
    return SFM_OK;
}

Ws carve_at(void* ws, int64_t ncam, int64_t npt, int64_t nobs) {
    return carve(reinterpret_cast<void*>(sfm::align_up((size_t)(uintptr_t)ws, 256)), ncam, npt, nobs);
}

}  // namespace

extern "C" size_t sfm_track_ba_ws_bytes(int64_t ncam, int64_t npt, int64_t nobs) {
    return sizes_ok(ncam, npt, nobs) ? carve(nullptr, ncam, npt, nobs).bytes + 256 : 0;
}

extern "C" int sfm_track_ba_sweep(const double* cams_dev, int64_t ncam, const double* K_host, const double* X_dev, int64_t npt, const float* obs_dev,
                                  const int32_t* track_off_dev, const int32_t* cam_idx_dev, const int32_t* pt_idx_dev, const int32_t* cam_off_dev,
                                  const int32_t* cam_obs_dev, int64_t nobs, double huber, int mode, uint8_t* active_dev, double* JtJ_cam_dev,
                                  double* Jtr_cam_dev, double* JtJ_pt_dev, double* Jtr_pt_dev, double* stat_dev, int32_t* count_dev, void* ws_dev,
                                  size_t ws_bytes, void* stream) {
    const Csr g{track_off_dev, cam_idx_dev, pt_idx_dev, cam_off_dev, cam_obs_dev};
    const int rc = check_common("sfm_track_ba_sweep", ncam, npt, nobs, g, ws_dev, ws_bytes);
    if (rc != SFM_OK) return rc;
    SFM_CHECK_ARG(mode == 0 || mode == 1, "sfm_track_ba_sweep: mode %d must be 0 or 1", mode);
    SFM_CHECK_ARG(huber > 0.0, "sfm_track_ba_sweep: huber %g must be > 0 px (+inf: plain least squares)", huber);
    SFM_CHECK_ARG(cams_dev && K_host && X_dev && JtJ_cam_dev && Jtr_cam_dev && JtJ_pt_dev && Jtr_pt_dev && stat_dev && count_dev &&
                      (nobs == 0 || (obs_dev && active_dev)),
                  "sfm_track_ba_sweep: null pointer");
    const Ws w = carve_at(ws_dev, ncam, npt, nobs);
    const Intrin K{K_host[0], K_host[4], K_host[2], K_host[5]};
    hipStream_t s = sfm::as_stream(stream);
    const int64_t nblk = blocks_of(nobs);
    hipLaunchKernelGGL(tba_cam_prepare_kernel, dim3((unsigned)blocks_of(ncam, 64)), dim3(64), 0, s, cams_dev, ncam, w.table);
    launch_scan(s, w, g, ncam, nobs);
    SFM_CHECK_LAUNCH();
    if (nobs > 0) {
        if (mode == 0)
            hipLaunchKernelGGL(tba_obs_kernel<0>, dim3((unsigned)nblk), dim3(kBlock), 0, s, w.table, K, ncam, X_dev, npt, obs_dev, cam_idx_dev,
                               pt_idx_dev, (int)nobs, huber, active_dev, w.rows, w.cost_part);
        else
            hipLaunchKernelGGL(tba_obs_kernel<1>, dim3((unsigned)nblk), dim3(kBlock), 0, s, w.table, K, ncam, X_dev, npt, obs_dev, cam_idx_dev,
                               pt_idx_dev, (int)nobs, huber, active_dev, w.rows, w.cost_part);
        SFM_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(tba_cost_fold_kernel, dim3(1), dim3(kScanThreads), 0, s, w.cost_part, nblk, stat_dev, count_dev);
    hipLaunchKernelGGL(tba_point_kernel<0>, dim3(point_grid(npt)), dim3(kBlock), 0, s, track_off_dev, cam_idx_dev, ncam, npt, (int)nobs, w.rows,
                       (const double*)nullptr, JtJ_pt_dev, Jtr_pt_dev);
    SFM_CHECK_LAUNCH();
    if (nobs > 0 && w.chunk_cap > 0) {
        hipLaunchKernelGGL(tba_cam_chunk_kernel<0>, dim3((unsigned)w.chunk_cap), dim3(kBlock), 0, s, cam_off_dev, cam_obs_dev, cam_idx_dev, pt_idx_dev,
                           w.chunk_off, ncam, npt, (int)nobs, w.rows, (const double*)nullptr, w.cam_part);
        SFM_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(tba_cam_fold_kernel<0>, dim3((unsigned)blocks_of(ncam, kBlock / 32)), dim3(kBlock), 0, s, w.chunk_off, ncam, w.cam_part,
                       JtJ_cam_dev, Jtr_cam_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" int sfm_track_ba_product(int64_t ncam, int64_t npt, const int32_t* track_off_dev, const int32_t* cam_idx_dev, const int32_t* pt_idx_dev,
                                    const int32_t* cam_off_dev, const int32_t* cam_obs_dev, int64_t nobs, int mode, const double* in_dev,
                                    double* out_dev, void* ws_dev, size_t ws_bytes, void* stream) {
    const Csr g{track_off_dev, cam_idx_dev, pt_idx_dev, cam_off_dev, cam_obs_dev};
    const int rc = check_common("sfm_track_ba_product", ncam, npt, nobs, g, ws_dev, ws_bytes);
    if (rc != SFM_OK) return rc;
    SFM_CHECK_ARG(mode == 0 || mode == 1, "sfm_track_ba_product: mode %d must be 0 or 1", mode);
    SFM_CHECK_ARG(in_dev && out_dev, "sfm_track_ba_product: null pointer");
    const Ws w = carve_at(ws_dev, ncam, npt, nobs);
    hipStream_t s = sfm::as_stream(stream);
    if (mode == 0) {
        launch_wt(s, w, g, ncam, npt, nobs, in_dev, out_dev);
    } else {
        launch_scan(s, w, g, ncam, nobs);
        launch_w(s, w, g, ncam, npt, nobs, in_dev, out_dev);
    }
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

// Waits for `stream` once per look at r.r (before iterations 0, 5, 10, ... while iterations remain); the status word comes with the
// first look.  dc_dev and dp_dev are complete in stream order, not at return.
extern "C" int sfm_track_ba_step(int64_t ncam, int64_t npt, const int32_t* track_off_dev, const int32_t* cam_idx_dev, const int32_t* pt_idx_dev,
                                 const int32_t* cam_off_dev, const int32_t* cam_obs_dev, int64_t nobs, const double* JtJ_cam_dev,
                                 const double* Jtr_cam_dev, const double* JtJ_pt_dev, const double* Jtr_pt_dev, double lam, int fix_first_camera,
                                 double cg_tol, int cg_iters, double* dc_dev, double* dp_dev, int32_t* iters_host, int32_t* status_host,
                                 void* ws_dev, size_t ws_bytes, void* stream) {
    const Csr g{track_off_dev, cam_idx_dev, pt_idx_dev, cam_off_dev, cam_obs_dev};
    const int rc = check_common("sfm_track_ba_step", ncam, npt, nobs, g, ws_dev, ws_bytes);
    if (rc != SFM_OK) return rc;
    SFM_CHECK_ARG(cg_iters >= 0 && lam >= 0.0 && cg_tol >= 0.0, "sfm_track_ba_step: cg_iters %d, lam %g, cg_tol %g: each must be >= 0", cg_iters, lam,
                  cg_tol);
    SFM_CHECK_ARG(JtJ_cam_dev && Jtr_cam_dev && JtJ_pt_dev && Jtr_pt_dev && dc_dev && dp_dev, "sfm_track_ba_step: null pointer");
    const Ws w = carve_at(ws_dev, ncam, npt, nobs);
    hipStream_t s = sfm::as_stream(stream);
    const int n = (int)ncam * 6, fix = fix_first_camera ? 1 : 0;
    int* status = reinterpret_cast<int*>(w.scal + kScalStatus);
    SFM_CHECK_HIP(hipMemsetAsync(w.scal, 0, sizeof(double) * kScalWords, s));
    launch_scan(s, w, g, ncam, nobs);
    hipLaunchKernelGGL(tba_damp_cam_kernel, dim3((unsigned)blocks_of(ncam, 64)), dim3(64), 0, s, JtJ_cam_dev, (int)ncam, lam, w.Bd, w.Minv, status);
    const unsigned pblocks = (unsigned)blocks_of(npt);
    hipLaunchKernelGGL(tba_damp_pt_kernel, dim3(pblocks), dim3(256), 0, s, JtJ_pt_dev, npt, lam, w.Cinv, status);
    SFM_CHECK_LAUNCH();
    // rhs = g_c - W Cd^-1 g_p
    hipLaunchKernelGGL(tba_pt_apply_kernel, dim3(pblocks), dim3(256), 0, s, w.Cinv, Jtr_pt_dev, (const double*)nullptr, 1.0, npt, w.v);
    launch_w(s, w, g, ncam, npt, nobs, w.v, w.wv);
    hipLaunchKernelGGL(tba_cg_init_kernel, dim3(1), dim3(kCgThreads), 0, s, Jtr_cam_dev, w.wv, w.Minv, n, fix, cg_tol * cg_tol, dc_dev, w.r, w.p, w.scal);
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
        launch_wt(s, w, g, ncam, npt, nobs, w.p, w.u);                                                          // u = W^T p
        hipLaunchKernelGGL(tba_pt_apply_kernel, dim3(pblocks), dim3(256), 0, s, w.Cinv, w.u, (const double*)nullptr, 1.0, npt, w.v);
        launch_w(s, w, g, ncam, npt, nobs, w.v, w.wv);                                                          // w = W Cd^-1 u
        hipLaunchKernelGGL(tba_cg_step_kernel, dim3(1), dim3(kCgThreads), 0, s, w.Bd, w.Minv, w.wv, n, fix, dc_dev, w.r, w.p, w.tmp, w.scal);
        SFM_CHECK_LAUNCH();
        ++it;
    }
    // dp = Cd^-1 (g_p - W^T dc)
    launch_wt(s, w, g, ncam, npt, nobs, dc_dev, w.u);
    hipLaunchKernelGGL(tba_pt_apply_kernel, dim3(pblocks), dim3(256), 0, s, w.Cinv, w.u, Jtr_pt_dev, -1.0, npt, dp_dev);
    SFM_CHECK_LAUNCH();
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
