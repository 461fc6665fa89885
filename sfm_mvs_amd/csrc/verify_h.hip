// The homography beside the essential matrix of the batched two-view verification (include/sfm_hip.h, "VERIFY-H"; docs/tracks.md §13):
//   sfm_verify_h_models   one lane per sample: the four-point homography of the first four slots of VERIFY's sample (8 x 8 elimination)
//   sfm_verify_h_score    one lane per model: transfer-error inlier counts over the pair's survivors, the best sample by an integer key
//   sfm_verify_h_select   per pair: the best sample's inliers, one refit on them (9 x 9 cv::SVD Jacobi on lane 0) kept only when it counts
//                         strictly more, the winner scaled to a middle singular value of 1, keep_h / H / sv / h_info
//   sfm_host_homography4, sfm_host_verify_h_refit, sfm_host_verify_h_normalise   the __host__ __device__ functions the lanes call
// Nothing depends on the order in which lanes or workgroups run: counts are integers, the best sample is the maximum of a 64-bit key,
// and the 45 float64 sums of the refit are formed in the fixed order the header writes out (VERIFY-LO's).
//
// The helpers (cv::SVD's one-sided Jacobi, the node lookup of a survivor) are copies of verify_lo.hip's, as that file copies verify.hip's.
// They use + - * / sqrt fabs and comparisons only, every loop is bounded, and the library is built with -ffp-contract=off, so that a
// lane returns the bits the host returns.
#include <cfloat>
#include <climits>
#include <cmath>

#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxImages = 65536;
constexpr int kMaxBudget = 1024;
constexpr int kScoreGridY = 4;                  // workgroups of a pair that share its batches of 256 samples
constexpr int kTri = 45;                        // the upper triangle of a 9 x 9 matrix
constexpr int kRefitWork = 81 + 81 + 9;         // a, v, W of the 9 x 9 Jacobi

__device__ inline bool in_range(int a, int n) { return (unsigned)a < (unsigned)n; }

__host__ __device__ inline bool finite_hd(double x) { return fabs(x) <= DBL_MAX; }

// ---- cv::SVD (sfm::host::Svd), for the host and the device ------------------------------------------------------------------------
__host__ __device__ inline double hypot_cv(double a, double b) {
    a = fabs(a);
    b = fabs(b);
    if (a > b) {
        b /= a;
        return a * sqrt(1 + b * b);
    }
    if (b > 0) {
        a /= b;
        return b * sqrt(1 + a * a);
    }
    return 0;
}

__host__ __device__ inline double dot2(const double* x, const double* y, int mm) {
    double p = 0;
    int k = 0;
    if (mm >= 4) {
        double s0 = 0, s1 = 0;
        for (; k <= mm - 2; k += 2) {
            s0 = s0 + x[k] * y[k];
            s1 = s1 + x[k + 1] * y[k + 1];
        }
        p = s0 + s1;
    }
    for (; k < mm; ++k) p += x[k] * y[k];
    return p;
}

// JacobiSVDImpl_ on the nn rows of a (each of mm words): W descending, v the right singular vectors as rows.
__host__ __device__ inline void jacobi_hd(double* a, int mm, int nn, double* W, double* v) {
    const double eps = DBL_EPSILON * 10;
    const int max_iter = mm > 30 ? mm : 30;
    for (int i = 0; i < nn; ++i) {
        double sd = 0;
        for (int k = 0; k < mm; ++k) sd += a[i * mm + k] * a[i * mm + k];
        W[i] = sd;
        for (int k = 0; k < nn; ++k) v[i * nn + k] = k == i ? 1.0 : 0.0;
    }
    for (int iter = 0; iter < max_iter; ++iter) {
        bool changed = false;
        for (int i = 0; i < nn - 1; ++i)
            for (int j = i + 1; j < nn; ++j) {
                double *Ai = a + i * mm, *Aj = a + j * mm;
                double aa = W[i], bb = W[j], p = dot2(Ai, Aj, mm);
                if (fabs(p) <= eps * sqrt(aa * bb)) continue;
                p *= 2;
                const double beta = aa - bb, gamma = hypot_cv(p, beta);
                double c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = sqrt(delta / gamma);
                    c = p / (gamma * s * 2);
                } else {
                    c = sqrt((gamma + beta) / (gamma * 2));
                    s = p / (gamma * c * 2);
                }
                int k = 0;
                aa = bb = 0;
                if (mm >= 4) {
                    double a0 = 0, a1 = 0, b0 = 0, b1 = 0;
                    for (; k <= mm - 2; k += 2) {
                        const double t0 = c * Ai[k] + s * Aj[k], t1 = c * Aj[k] - s * Ai[k];
                        const double u0 = c * Ai[k + 1] + s * Aj[k + 1], u1 = c * Aj[k + 1] - s * Ai[k + 1];
                        Ai[k] = t0; Aj[k] = t1; Ai[k + 1] = u0; Aj[k + 1] = u1;
                        a0 = a0 + t0 * t0; b0 = b0 + t1 * t1;
                        a1 = a1 + u0 * u0; b1 = b1 + u1 * u1;
                    }
                    aa = a0 + a1;
                    bb = b0 + b1;
                }
                for (; k < mm; ++k) {
                    const double t0 = c * Ai[k] + s * Aj[k], t1 = -s * Ai[k] + c * Aj[k];
                    Ai[k] = t0; Aj[k] = t1;
                    aa += t0 * t0;
                    bb += t1 * t1;
                }
                W[i] = aa;
                W[j] = bb;
                changed = true;
                double *Vi = v + i * nn, *Vj = v + j * nn;
                for (k = 0; k < nn; ++k) {
                    const double t0 = c * Vi[k] + s * Vj[k], t1 = -s * Vi[k] + c * Vj[k];
                    Vi[k] = t0; Vj[k] = t1;
                }
            }
        if (!changed) break;
    }
    for (int i = 0; i < nn; ++i) {
        double sd = 0;
        for (int k = 0; k < mm; ++k) sd += a[i * mm + k] * a[i * mm + k];
        W[i] = sqrt(sd);
    }
    for (int i = 0; i < nn - 1; ++i) {
        int j = i;
        for (int k = i + 1; k < nn; ++k)
            if (W[j] < W[k]) j = k;
        if (i != j) {
            double t = W[i]; W[i] = W[j]; W[j] = t;
            for (int k = 0; k < mm; ++k) { t = a[i * mm + k]; a[i * mm + k] = a[j * mm + k]; a[j * mm + k] = t; }
            for (int k = 0; k < nn; ++k) { t = v[i * nn + k]; v[i * nn + k] = v[j * nn + k]; v[j * nn + k] = t; }
        }
    }
}

// ---- the four-point homography ----------------------------------------------------------------------------------------------------
// x1, x2: four points each, (a, b) interleaved.  h: nine words, h[8] = 1.  false: a zero pivot or a non-finite word.
// Every index is a constant after unrolling, so the 8 x 9 system stays in registers on the device.
__host__ __device__ inline bool homography4_hd(const double* x1, const double* x2, double* h) {
    double A[8][9];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double a1 = x1[2 * k], b1 = x1[2 * k + 1], a2 = x2[2 * k], b2 = x2[2 * k + 1];
        double* r = A[2 * k];
        r[0] = a1; r[1] = b1; r[2] = 1.0; r[3] = 0.0; r[4] = 0.0; r[5] = 0.0; r[6] = -(a2 * a1); r[7] = -(a2 * b1); r[8] = a2;
        r = A[2 * k + 1];
        r[0] = 0.0; r[1] = 0.0; r[2] = 0.0; r[3] = a1; r[4] = b1; r[5] = 1.0; r[6] = -(b2 * a1); r[7] = -(b2 * b1); r[8] = b2;
    }
#pragma unroll
    for (int col = 0; col < 8; ++col) {
        int piv = col;
        double big = fabs(A[col][col]);
#pragma unroll
        for (int r = col + 1; r < 8; ++r) {
            const double v = fabs(A[r][col]);
            if (v > big) {
                big = v;
                piv = r;
            }
        }
#pragma unroll
        for (int r = col + 1; r < 8; ++r)
            if (r == piv) {
#pragma unroll
                for (int k = col; k < 9; ++k) {
                    const double t = A[col][k];
                    A[col][k] = A[r][k];
                    A[r][k] = t;
                }
            }
        const double d = A[col][col];
        if (d == 0) return false;
#pragma unroll
        for (int r = col + 1; r < 8; ++r) {
            const double f = A[r][col] / d;
#pragma unroll
            for (int k = col + 1; k < 9; ++k) A[r][k] = A[r][k] - f * A[col][k];
        }
    }
    double x[8];
#pragma unroll
    for (int col = 7; col >= 0; --col) {
        double s = A[col][8];
#pragma unroll
        for (int k = col + 1; k < 8; ++k) s = s - A[col][k] * x[k];
        x[col] = s / A[col][col];
    }
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        ok = ok && finite_hd(x[k]);
        h[k] = x[k];
    }
    h[8] = 1.0;
    return ok;
}

// The refit: M (9 x 9 row-major, symmetric) -> the right singular vector of its smallest singular value.  work: kRefitWork doubles.
__host__ __device__ inline void h_refit_hd(const double* M, double* Hc, double* work) {
    double *a = work, *v = work + 81, *W = work + 162;
    for (int i = 0; i < 9; ++i)
        for (int k = 0; k < 9; ++k) a[i * 9 + k] = M[k * 9 + i];
    jacobi_hd(a, 9, 9, W, v);
    for (int k = 0; k < 9; ++k) Hc[k] = v[72 + k];
}

// H / (its middle singular value) and the three singular values over the middle one.
__host__ __device__ inline void h_normalise_hd(const double* Hw, double* H_out, double* sv) {
    double a[9], v[9], W[3];
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) a[i * 3 + k] = Hw[k * 3 + i];
    jacobi_hd(a, 3, 3, W, v);
    const double mid = W[1];
    for (int k = 0; k < 3; ++k) sv[k] = W[k] / mid;
    for (int k = 0; k < 9; ++k) H_out[k] = Hw[k] / mid;
}

// ---- the survivors of a pair (verify.hip) -----------------------------------------------------------------------------------------
__device__ inline bool survivor_point(const int2* __restrict__ surv_p, int e, int oa, int ob, long long n_nodes,
                                      const double2* __restrict__ xn, double* pt) {
    const int2 qt = surv_p[e];
    const long long u = (long long)oa + qt.x, v = (long long)ob + qt.y;
    if (qt.x < 0 || qt.y < 0 || u < 0 || v < 0 || u >= n_nodes || v >= n_nodes) return false;
    const double2 a = xn[u], b = xn[v];
    pt[0] = a.x; pt[1] = a.y; pt[2] = b.x; pt[3] = b.y;
    return true;
}

// m' of a pair and the offsets of its two images (0, 0, 0 when an image is out of range).
__device__ inline long long pair_extent(const int* __restrict__ m_arr, const int* __restrict__ pair_img, const int* __restrict__ img_off,
                                        int n_img, long long cap, long long p, int* oa, int* ob) {
    const int a = pair_img[2 * p], b = pair_img[2 * p + 1];
    long long m = m_arr[p];
    if (m > cap) m = cap;
    if (m < 0 || !in_range(a, n_img) || !in_range(b, n_img)) m = 0;
    *oa = m ? img_off[a] : 0;
    *ob = m ? img_off[b] : 0;
    return m;
}

// The transfer test of one survivor: +1 an inlier of H, -1 an inlier of -H (the same u, v and d; w of the other sign), 0 neither.
__device__ __forceinline__ int transfer_class(const double* __restrict__ H, double a1, double b1, double a2, double b2, float thr2h) {
    const double w = H[6] * a1 + H[7] * b1 + H[8];
    const double u = (H[0] * a1 + H[1] * b1 + H[2]) / w;
    const double v = (H[3] * a1 + H[4] * b1 + H[5]) / w;
    const double d = (u - a2) * (u - a2) + (v - b2) * (v - b2);
    if (!((float)d <= thr2h)) return 0;
    return w > 0 ? 1 : w < 0 ? -1 : 0;
}

// ---- models -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void h_models_kernel(const int* __restrict__ samp, const int2* __restrict__ surv, const int* __restrict__ m_arr,
                                                          const int* __restrict__ pair_img, const int* __restrict__ img_off, int n_img,
                                                          const double2* __restrict__ xn, long long n_nodes, long long n_pairs, long long cap,
                                                          int H, int* __restrict__ ok_out, double* __restrict__ Hm) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_pairs * H) return;
    const long long p = i / H;
    double x1[8], x2[8], h[9];
    const int a = pair_img[2 * p], b = pair_img[2 * p + 1];
    long long m = m_arr[p];
    if (m > cap) m = cap;
    bool ok = in_range(a, n_img) && in_range(b, n_img) && m >= 5;
    if (ok) {
        const int oa = img_off[a], ob = img_off[b];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int idx = samp[5 * i + k];
            double pt[4] = {0, 0, 0, 0};
            ok = ok && idx >= 0 && idx < m && survivor_point(surv + p * cap, idx < 0 || idx >= m ? 0 : idx, oa, ob, n_nodes, xn, pt);
            x1[2 * k] = pt[0]; x1[2 * k + 1] = pt[1];
            x2[2 * k] = pt[2]; x2[2 * k + 1] = pt[3];
        }
    }
    ok = ok && homography4_hd(x1, x2, h);
    ok_out[i] = ok ? 1 : 0;
    double* __restrict__ out = Hm + (size_t)i * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k) out[k] = ok ? h[k] : 0.0;
}

// ---- score ------------------------------------------------------------------------------------------------------------------------
// Workgroup (p, y): the samples of pair p in batches of 256, one lane per sample; the pair's survivors pass through LDS 256 at a time
// and every lane reads each of them (a broadcast).  Counts stay in a register; nothing is reduced but the key.
__global__ __launch_bounds__(kBlock) void h_score_kernel(const double* __restrict__ Hm, const int* __restrict__ ok_arr, const int2* __restrict__ surv,
                                                         const int* __restrict__ m_arr, const int* __restrict__ pair_img,
                                                         const int* __restrict__ img_off, int n_img, const double2* __restrict__ xn,
                                                         long long n_nodes, long long cap, int H, float thr2h, int* __restrict__ counts,
                                                         unsigned long long* __restrict__ best) {
    __shared__ double pts[kBlock][4];
    __shared__ int valid[kBlock];
    const long long p = blockIdx.x;
    const int tid = threadIdx.x;
    int oa, ob;
    const long long m = pair_extent(m_arr, pair_img, img_off, n_img, cap, p, &oa, &ob);
    for (int s0 = blockIdx.y * kBlock; s0 < H; s0 += gridDim.y * kBlock) {
        const int s = s0 + tid;
        const bool live = s < H && ok_arr[p * H + s] != 0;
        double Hl[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (live) {
            const double* __restrict__ src = Hm + (size_t)(p * H + s) * 9;
#pragma unroll
            for (int k = 0; k < 9; ++k) Hl[k] = src[k];
        }
        int count = 0;
        for (long long e0 = 0; e0 < m; e0 += kBlock) {
            const long long e = e0 + tid;
            double pt[4] = {0, 0, 0, 0};
            const bool have = e < m && survivor_point(surv + p * cap, (int)e, oa, ob, n_nodes, xn, pt);
            pts[tid][0] = pt[0]; pts[tid][1] = pt[1]; pts[tid][2] = pt[2]; pts[tid][3] = pt[3];
            valid[tid] = have;
            __syncthreads();
            const int nt = (int)(m - e0 < kBlock ? m - e0 : kBlock);
            if (live)
                for (int k = 0; k < nt; ++k) count += valid[k] && transfer_class(Hl, pts[k][0], pts[k][1], pts[k][2], pts[k][3], thr2h) > 0;
            __syncthreads();
        }
        unsigned long long key = 0;
        if (s < H) counts[p * H + s] = live ? count : 0;
        if (live) key = ((unsigned long long)(unsigned)count << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)s);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const unsigned long long o = __shfl_xor(key, d, 64);
            key = o > key ? o : key;
        }
        if ((tid & 63) == 0 && key) atomicMax(&best[p], key);
    }
}

// ---- select -----------------------------------------------------------------------------------------------------------------------
enum Status { kFewSurvivors = 1, kNoModel = 2 };

// One workgroup per pair.  Pass A: the inliers of the sample's H and the 45 sums over them; the refit on lane 0; pass B: the candidate's
// counts under both signs; pass C: the winner's inliers into keep_h.
__global__ __launch_bounds__(kBlock) void h_select_kernel(const double* __restrict__ Hm, const int* __restrict__ ok_arr,
                                                          const unsigned long long* __restrict__ best, const int2* __restrict__ surv,
                                                          const int* __restrict__ m_arr, const int* __restrict__ pair_img,
                                                          const int* __restrict__ img_off, int n_img, const double2* __restrict__ xn,
                                                          long long n_nodes, long long cap, int H, float thr2h, int refit,
                                                          unsigned char* __restrict__ keep, double* __restrict__ H_out, double* __restrict__ sv_out,
                                                          int* __restrict__ info) {
    __shared__ double wsum[kBlock / 64][kTri];
    __shared__ double Msh[81];
    __shared__ double work[kRefitWork];
    __shared__ double Hsh[9];
    __shared__ int wcnt[kBlock / 64][3];
    __shared__ int flag;
    const long long p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int oa, ob;
    const long long m = pair_extent(m_arr, pair_img, img_off, n_img, cap, p, &oa, &ob);
    const int2* __restrict__ surv_p = surv + p * cap;
    const unsigned long long key = best[p];
    const unsigned bs = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
    const bool has = key != 0 && bs < (unsigned)H;
    for (long long c = tid; c < cap; c += kBlock) keep[p * cap + c] = 0;
    if (!has) {
        if (tid < 9) H_out[9 * p + tid] = 0.0;
        if (tid < 3) sv_out[3 * p + tid] = 0.0;
        if (tid == 0) {
            int* w = info + 8 * p;
            w[0] = m_arr[p]; w[1] = 0; w[2] = 0; w[3] = 0; w[4] = -1; w[5] = -1; w[6] = 0;
            w[7] = (m_arr[p] < 5 ? kFewSurvivors : 0) | kNoModel;
        }
        return;
    }
    double Hcur[9];
    {
        const double* __restrict__ src = Hm + (size_t)(p * H + bs) * 9;
#pragma unroll
        for (int k = 0; k < 9; ++k) Hcur[k] = src[k];
    }
    // samples with a model, and pass A
    int n_ok = 0;
    for (int s = tid; s < H; s += kBlock) n_ok += ok_arr[p * H + s] != 0;
    int c_in = 0;
    double acc[kTri];
#pragma unroll
    for (int k = 0; k < kTri; ++k) acc[k] = 0.0;
    for (long long e = tid; e < m; e += kBlock) {
        double pt[4];
        if (!survivor_point(surv_p, (int)e, oa, ob, n_nodes, xn, pt)) continue;
        if (surv_p[e].x >= cap || transfer_class(Hcur, pt[0], pt[1], pt[2], pt[3], thr2h) <= 0) continue;
        ++c_in;
        if (refit) {
            const double a1 = pt[0], b1 = pt[1], a2 = pt[2], b2 = pt[3];
            const double r1[9] = {-a1, -b1, -1.0, 0.0, 0.0, 0.0, a2 * a1, a2 * b1, a2};
            const double r2[9] = {0.0, 0.0, 0.0, -a1, -b1, -1.0, b2 * a1, b2 * b1, b2};
            int k = 0;
#pragma unroll
            for (int i = 0; i < 9; ++i)
#pragma unroll
                for (int j = i; j < 9; ++j, ++k) acc[k] = acc[k] + (r1[i] * r1[j] + r2[i] * r2[j]);
        }
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        c_in += __shfl_xor(c_in, d, 64);
        n_ok += __shfl_xor(n_ok, d, 64);
    }
    if (refit) {
        // the fixed tree, levels h = 1, 2, .. 32 inside a wave: lane l (a multiple of 2h) takes s[l] + s[l + h]
#pragma unroll
        for (int k = 0; k < kTri; ++k) {
            double s = acc[k];
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) s = s + __shfl_xor(s, d, 64);
            acc[k] = s;
        }
    }
    if (lane == 0) {
        wcnt[wave][0] = c_in;
        wcnt[wave][1] = n_ok;
        if (refit)
#pragma unroll
            for (int k = 0; k < kTri; ++k) wsum[wave][k] = acc[k];
    }
    __syncthreads();
    const int n_s = wcnt[0][0] + wcnt[1][0] + wcnt[2][0] + wcnt[3][0];
    n_ok = wcnt[0][1] + wcnt[1][1] + wcnt[2][1] + wcnt[3][1];
    int n_final = n_s, won = -1;
    if (refit && n_s >= 8) {
        if (tid < kTri) {
            // levels h = 64, 128: (wave 0 + wave 1) + (wave 2 + wave 3)
            const double s = (wsum[0][tid] + wsum[1][tid]) + (wsum[2][tid] + wsum[3][tid]);
            int i = 0, k = tid;
            while (k >= 9 - i) {
                k -= 9 - i;
                ++i;
            }
            const int j = i + k;
            Msh[9 * i + j] = s;
            Msh[9 * j + i] = s;
        }
        __syncthreads();
        if (tid == 0) {
            double Hn[9];
            h_refit_hd(Msh, Hn, work);
            bool ok = true;
            for (int k = 0; k < 9; ++k) {
                ok = ok && finite_hd(Hn[k]);
                Hsh[k] = Hn[k];
            }
            flag = ok;
        }
        __syncthreads();
        if (flag) {
            double Hn[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) Hn[k] = Hsh[k];
            int c_pos = 0, c_neg = 0;
            for (long long e = tid; e < m; e += kBlock) {
                double pt[4];
                if (!survivor_point(surv_p, (int)e, oa, ob, n_nodes, xn, pt) || surv_p[e].x >= cap) continue;
                const int cls = transfer_class(Hn, pt[0], pt[1], pt[2], pt[3], thr2h);
                c_pos += cls > 0;
                c_neg += cls < 0;
            }
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                c_pos += __shfl_xor(c_pos, d, 64);
                c_neg += __shfl_xor(c_neg, d, 64);
            }
            if (lane == 0) {
                wcnt[wave][1] = c_pos;
                wcnt[wave][2] = c_neg;
            }
            __syncthreads();
            const int n_pos = wcnt[0][1] + wcnt[1][1] + wcnt[2][1] + wcnt[3][1];
            const int n_neg = wcnt[0][2] + wcnt[1][2] + wcnt[2][2] + wcnt[3][2];
            const bool flip = n_neg > n_pos;
            const int n_r = flip ? n_neg : n_pos;
            if (n_r > n_s) {
                n_final = n_r;
                won = 0;
#pragma unroll
                for (int k = 0; k < 9; ++k) Hcur[k] = flip ? -Hn[k] : Hn[k];
            }
        }
    }
    // pass C: the winner's inliers
    for (long long e = tid; e < m; e += kBlock) {
        double pt[4];
        if (!survivor_point(surv_p, (int)e, oa, ob, n_nodes, xn, pt)) continue;
        const int q = surv_p[e].x;
        if (q >= cap || transfer_class(Hcur, pt[0], pt[1], pt[2], pt[3], thr2h) <= 0) continue;
        keep[p * cap + q] = 1;
    }
    if (tid == 0) {
        double Hn[9], sv[3];
        h_normalise_hd(Hcur, Hn, sv);
        for (int k = 0; k < 9; ++k) H_out[9 * p + k] = Hn[k];
        for (int k = 0; k < 3; ++k) sv_out[3 * p + k] = sv[k];
        int* w = info + 8 * p;
        w[0] = m_arr[p]; w[1] = n_ok; w[2] = n_final; w[3] = n_s; w[4] = (int)bs; w[5] = won; w[6] = 0;
        w[7] = m_arr[p] < 5 ? kFewSurvivors : 0;
    }
}

bool h_sizes_ok(int64_t n_pairs, int64_t cap, int n_img, int64_t n_nodes) {
    return n_pairs >= 0 && cap >= 0 && n_pairs <= INT32_MAX / kMaxBudget && cap <= INT32_MAX && n_pairs * cap <= INT32_MAX && n_img >= 1 &&
           n_img <= kMaxImages && n_nodes >= 0 && n_nodes <= INT32_MAX;
}

}  // namespace

extern "C" int sfm_verify_h_models(const int32_t* samp_dev, const int32_t* surv_dev, const int32_t* m_dev, const int32_t* pair_img_dev,
                                   const int32_t* img_off_dev, int n_img, const double* xn_dev, int64_t n_nodes, int64_t n_pairs, int64_t cap,
                                   int budget, int32_t* ok_dev, double* Hm_dev, void* stream_) {
    SFM_CHECK_ARG(h_sizes_ok(n_pairs, cap, n_img, n_nodes), "sfm_verify_h_models: bad sizes");
    SFM_CHECK_ARG(budget >= 1 && budget <= kMaxBudget, "sfm_verify_h_models: the budget must be 1..%d (got %d)", kMaxBudget, budget);
    SFM_CHECK_ARG(img_off_dev, "sfm_verify_h_models: null img_off");
    if (n_pairs == 0) return SFM_OK;
    SFM_CHECK_ARG(samp_dev && m_dev && pair_img_dev && ok_dev && Hm_dev && (cap == 0 || surv_dev) && (n_nodes == 0 || xn_dev),
                  "sfm_verify_h_models: null pointer");
    const long long n = (long long)n_pairs * budget;
    hipLaunchKernelGGL(h_models_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, sfm::as_stream(stream_), samp_dev,
                       reinterpret_cast<const int2*>(surv_dev), m_dev, pair_img_dev, img_off_dev, n_img, reinterpret_cast<const double2*>(xn_dev),
                       (long long)n_nodes, (long long)n_pairs, (long long)cap, budget, ok_dev, Hm_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" int sfm_verify_h_score(const double* Hm_dev, const int32_t* ok_dev, const int32_t* surv_dev, const int32_t* m_dev,
                                  const int32_t* pair_img_dev, const int32_t* img_off_dev, int n_img, const double* xn_dev, int64_t n_nodes,
                                  int64_t n_pairs, int64_t cap, int budget, float thr2h, int32_t* counts_dev, uint64_t* best_dev, void* stream_) {
    SFM_CHECK_ARG(h_sizes_ok(n_pairs, cap, n_img, n_nodes), "sfm_verify_h_score: bad sizes");
    SFM_CHECK_ARG(budget >= 1 && budget <= kMaxBudget, "sfm_verify_h_score: the budget must be 1..%d (got %d)", kMaxBudget, budget);
    SFM_CHECK_ARG(thr2h == thr2h, "sfm_verify_h_score: thr2h is NaN");
    SFM_CHECK_ARG(img_off_dev, "sfm_verify_h_score: null img_off");
    if (n_pairs == 0) return SFM_OK;
    SFM_CHECK_ARG(Hm_dev && ok_dev && m_dev && pair_img_dev && counts_dev && best_dev && (cap == 0 || surv_dev) && (n_nodes == 0 || xn_dev),
                  "sfm_verify_h_score: null pointer");
    hipStream_t stream = sfm::as_stream(stream_);
    SFM_CHECK_HIP(hipMemsetAsync(best_dev, 0, sizeof(uint64_t) * (size_t)n_pairs, stream));
    const int batches = (budget + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(h_score_kernel, dim3((unsigned)n_pairs, (unsigned)(batches < kScoreGridY ? batches : kScoreGridY)), dim3(kBlock), 0, stream,
                       Hm_dev, ok_dev, reinterpret_cast<const int2*>(surv_dev), m_dev, pair_img_dev, img_off_dev, n_img,
                       reinterpret_cast<const double2*>(xn_dev), (long long)n_nodes, (long long)cap, budget, thr2h, counts_dev,
                       reinterpret_cast<unsigned long long*>(best_dev));
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" int sfm_verify_h_select(const double* Hm_dev, const int32_t* ok_dev, const uint64_t* best_dev, const int32_t* surv_dev,
                                   const int32_t* m_dev, const int32_t* pair_img_dev, const int32_t* img_off_dev, int n_img, const double* xn_dev,
                                   int64_t n_nodes, int64_t n_pairs, int64_t cap, int budget, float thr2h, int refit, uint8_t* keep_h_dev,
                                   double* H_out_dev, double* sv_dev, int32_t* h_info_dev, void* stream_) {
    SFM_CHECK_ARG(h_sizes_ok(n_pairs, cap, n_img, n_nodes), "sfm_verify_h_select: bad sizes");
    SFM_CHECK_ARG(budget >= 1 && budget <= kMaxBudget, "sfm_verify_h_select: the budget must be 1..%d (got %d)", kMaxBudget, budget);
    SFM_CHECK_ARG(thr2h == thr2h, "sfm_verify_h_select: thr2h is NaN");
    SFM_CHECK_ARG(refit == 0 || refit == 1, "sfm_verify_h_select: refit must be 0 or 1 (got %d)", refit);
    SFM_CHECK_ARG(img_off_dev, "sfm_verify_h_select: null img_off");
    if (n_pairs == 0) return SFM_OK;
    SFM_CHECK_ARG(Hm_dev && ok_dev && best_dev && m_dev && pair_img_dev && H_out_dev && sv_dev && h_info_dev &&
                      (cap == 0 || (surv_dev && keep_h_dev)) && (n_nodes == 0 || xn_dev),
                  "sfm_verify_h_select: null pointer");
    hipLaunchKernelGGL(h_select_kernel, dim3((unsigned)n_pairs), dim3(kBlock), 0, sfm::as_stream(stream_), Hm_dev, ok_dev,
                       reinterpret_cast<const unsigned long long*>(best_dev), reinterpret_cast<const int2*>(surv_dev), m_dev, pair_img_dev,
                       img_off_dev, n_img, reinterpret_cast<const double2*>(xn_dev), (long long)n_nodes, (long long)cap, budget, thr2h, refit,
                       keep_h_dev, H_out_dev, sv_dev, h_info_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" int sfm_host_homography4(const double* x1_host, const double* x2_host, double* H_host) {
    SFM_CHECK_ARG(x1_host && x2_host && H_host, "sfm_host_homography4: null pointer");
    double h[9];
    const bool ok = homography4_hd(x1_host, x2_host, h);
    for (int k = 0; k < 9; ++k) H_host[k] = ok ? h[k] : 0.0;
    return SFM_OK;
}

extern "C" int sfm_host_verify_h_refit(const double* M81_host, double* H_host) {
    SFM_CHECK_ARG(M81_host && H_host, "sfm_host_verify_h_refit: null pointer");
    double work[kRefitWork];
    h_refit_hd(M81_host, H_host, work);
    return SFM_OK;
}

extern "C" int sfm_host_verify_h_normalise(const double* H_host, double* H_out_host, double* sv_host) {
    SFM_CHECK_ARG(H_host && H_out_host && sv_host, "sfm_host_verify_h_normalise: null pointer");
    h_normalise_hd(H_host, H_out_host, sv_host);
    return SFM_OK;
}
