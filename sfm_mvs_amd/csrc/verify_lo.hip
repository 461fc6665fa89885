// Local optimisation of the batched two-view verification (include/sfm_hip.h, "VERIFY-LO"; docs/tracks.md §12):
//   sfm_verify_top       per pair: the T best models of sfm_verify_score's counts by the integer key, in descending order
//   sfm_verify_lo        per (pair, candidate): R rounds of refit-on-the-wide-inliers (eight-point system, 9 x 9 and 3 x 3 cv::SVD
//                        Jacobi on lane 0) and recount, R + 1 passes over the survivors; the best of the candidate and its refits
//   sfm_verify_lo_pick   per pair: the candidate with the most inliers, written as a one-sample models buffer for sfm_verify_select
//   sfm_host_verify_refit  the refit (M -> E) on the host: the same __host__ __device__ function the kernel calls
// Nothing depends on the order in which lanes or workgroups run: counts are integers, the choices are maxima of 64-bit keys, and
// the 45 float64 sums of a refit are formed in the fixed order the header writes out (a lane's survivors ascending, then a fixed
// tree over the 256 lanes).
//
// The helpers (cv::SVD's one-sided Jacobi and its 3 x 3 completion, the Sampson expression, the node lookup of a survivor) are
// copies of verify.hip's, as tracks_refine.hip and the mesh files copy theirs.  They use + - * / sqrt fabs and comparisons only,
// every loop is bounded, and the library is built with -ffp-contract=off, so that lane 0 returns the bits the host returns.
#include <cfloat>
#include <climits>
#include <cmath>

#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxImages = 65536;
constexpr int kMaxBudget = 1024;
constexpr int kSlots = 10;
constexpr int kMaxTop = SFM_VERIFY_LO_MAX_TOP;
constexpr int kMaxRounds = SFM_VERIFY_LO_MAX_ROUNDS;
constexpr int kTri = 45;                        // the upper triangle of a 9 x 9 matrix
constexpr int kRefitWork = 81 + 81 + 9;         // a, v, W of the 9 x 9 Jacobi

__device__ inline bool in_range(int a, int n) { return (unsigned)a < (unsigned)n; }

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

// Svd::compute of a 3 x 3 matrix: u (3 x 3 row-major) and vt.
__host__ __device__ inline void svd3_hd(const double* A, double* u_out, double* vt_out) {
    const int mm = 3, nn = 3;
    double a[9], v[9], W[3];
    for (int i = 0; i < nn; ++i)
        for (int k = 0; k < mm; ++k) a[i * mm + k] = A[k * 3 + i];
    jacobi_hd(a, mm, nn, W, v);
    const double minval = DBL_MIN, eps = DBL_EPSILON * 10;
    unsigned long long state = 0x12345678u;                 // cv::RNG(0x12345678)
    for (int i = 0; i < nn; ++i) {
        double sd = W[i];
        for (int ii = 0; ii < 100 && sd <= minval; ++ii) {
            const double val0 = 1. / mm;
            for (int k = 0; k < mm; ++k) {
                state = (unsigned long long)(unsigned)state * 4164903690u + (unsigned)(state >> 32);
                a[i * mm + k] = ((unsigned)state & 256) != 0 ? val0 : -val0;
            }
            for (int iter = 0; iter < 2; ++iter)
                for (int j = 0; j < i; ++j) {
                    sd = 0;
                    for (int k = 0; k < mm; ++k) sd += a[i * mm + k] * a[j * mm + k];
                    double asum = 0;
                    for (int k = 0; k < mm; ++k) {
                        const double t = a[i * mm + k] - sd * a[j * mm + k];
                        a[i * mm + k] = t;
                        asum += fabs(t);
                    }
                    asum = asum > eps * 100 ? 1 / asum : 0;
                    for (int k = 0; k < mm; ++k) a[i * mm + k] *= asum;
                }
            sd = 0;
            for (int k = 0; k < mm; ++k) sd += a[i * mm + k] * a[i * mm + k];
            sd = sqrt(sd);
        }
        const double s = sd > minval ? 1 / sd : 0.;
        for (int k = 0; k < mm; ++k) a[i * mm + k] *= s;
    }
    for (int k = 0; k < mm; ++k)
        for (int i = 0; i < nn; ++i) u_out[k * nn + i] = a[i * mm + k];
    for (int k = 0; k < 9; ++k) vt_out[k] = v[k];
}

// The refit: M (9 x 9 row-major, symmetric) -> E_new (unit Frobenius norm).  work: kRefitWork doubles.
__host__ __device__ inline void refit_hd(const double* M, double* E, double* work) {
    double *a = work, *v = work + 81, *W = work + 162;
    for (int i = 0; i < 9; ++i)
        for (int k = 0; k < 9; ++k) a[i * 9 + k] = M[k * 9 + i];
    jacobi_hd(a, 9, 9, W, v);
    double F[9], U[9], Vt[9];
    for (int k = 0; k < 9; ++k) F[k] = v[72 + k];
    svd3_hd(F, U, Vt);
    double nrm = 0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double e = U[3 * i] * Vt[j] + U[3 * i + 1] * Vt[3 + j];
            E[3 * i + j] = e;
            nrm += e * e;
        }
    nrm = sqrt(nrm);
    for (int k = 0; k < 9; ++k) E[k] = E[k] / nrm;
}

__host__ __device__ inline bool finite_hd(double x) { return fabs(x) <= DBL_MAX; }

// ---- the survivors of a pair (verify.hip) -----------------------------------------------------------------------------------------
__device__ inline bool survivor_point(const int2* __restrict__ surv_p, int e, int oa, int ob, long long n_nodes,
                                      const double2* __restrict__ xn, double* pt) {
    const int2 qt = surv_p[e];
    const long long u = (long long)oa + qt.x, v = (long long)ob + qt.y;
    if (qt.x < 0 || qt.y < 0 || u >= n_nodes || v >= n_nodes) return false;
    const double2 a = xn[u], b = xn[v];
    pt[0] = a.x; pt[1] = a.y; pt[2] = b.x; pt[3] = b.y;
    return true;
}

// The value sfm_verify_score compares with thr2.
__device__ __forceinline__ float sampson_value(const double* __restrict__ E, double a1, double b1, double a2, double b2) {
    const double e0 = E[0] * a1 + E[1] * b1 + E[2] * 1., e1 = E[3] * a1 + E[4] * b1 + E[5] * 1., e2 = E[6] * a1 + E[7] * b1 + E[8] * 1.;
    const double f0 = E[0] * a2 + E[3] * b2 + E[6] * 1., f1 = E[1] * a2 + E[4] * b2 + E[7] * 1.;
    const double x2tEx1 = a2 * e0 + b2 * e1 + 1. * e2;
    const double a = e0 * e0, b = e1 * e1, c = f0 * f0, d = f1 * f1;
    return (float)(x2tEx1 * x2tEx1 / (a + b + c + d));
}

__device__ inline bool slot_of(unsigned long long key, int H, unsigned* slot) {
    *slot = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
    return key != 0 && *slot < (unsigned)H * kSlots;
}

// ---- top --------------------------------------------------------------------------------------------------------------------------
// One workgroup per pair, T rounds: the largest key below the previous round's (keys are distinct).
__global__ __launch_bounds__(kBlock) void top_kernel(const int* __restrict__ counts, const int* __restrict__ nmodels, int H, int T,
                                                     unsigned long long* __restrict__ top) {
    __shared__ unsigned long long wmax[kBlock / 64];
    const long long p = blockIdx.x;
    const int tid = threadIdx.x;
    const int n = H * kSlots;
    unsigned long long prev = 0;                          // (unused in round 0: a key may be all ones)
    for (int k = 0; k < T; ++k) {
        unsigned long long best = 0;
        for (int slot = tid; slot < n; slot += kBlock) {
            const int s = slot / kSlots, j = slot - kSlots * s;
            int nm = nmodels[p * H + s];
            nm = nm < 0 ? 0 : nm > kSlots ? kSlots : nm;
            if (j >= nm) continue;
            const unsigned long long key =
                ((unsigned long long)(unsigned)counts[(p * H + s) * kSlots + j] << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)slot);
            if ((k == 0 || key < prev) && key > best) best = key;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const unsigned long long o = __shfl_xor(best, d, 64);
            best = o > best ? o : best;
        }
        if ((tid & 63) == 0) wmax[tid >> 6] = best;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) best = wmax[w] > best ? wmax[w] : best;
        __syncthreads();
        if (tid == 0) top[p * T + k] = best;
        prev = best;
    }
}

// ---- lo ---------------------------------------------------------------------------------------------------------------------------
struct Wide {
    float w[kMaxRounds];
};

// Workgroup (p, t).  Pass r = 0..R over the survivors: the count of E_cur at thr2 and, for r < R, the 45 sums over its wide set.
__global__ __launch_bounds__(kBlock) void lo_kernel(const double* __restrict__ E, const unsigned long long* __restrict__ top, int T,
                                                    const int2* __restrict__ surv, const int* __restrict__ m_arr, const int* __restrict__ pair_img,
                                                    const int* __restrict__ img_off, int n_img, const double2* __restrict__ xn, long long n_nodes,
                                                    long long cap, int H, float thr2, int R, Wide wide, double* __restrict__ E_lo,
                                                    int* __restrict__ n_lo, int* __restrict__ round_lo) {
    __shared__ double wsum[kBlock / 64][kTri];
    __shared__ double Msh[81];
    __shared__ double work[kRefitWork];
    __shared__ double Enew[9];
    __shared__ int wcnt[kBlock / 64][2];
    __shared__ int finite;
    const long long g = blockIdx.x;                       // p * T + t
    const long long p = g / T;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned slot;
    const bool has = slot_of(top[g], H, &slot);
    if (!has) {
        if (tid < 9) E_lo[9 * g + tid] = 0.0;
        if (tid == 0) {
            n_lo[g] = 0;
            round_lo[g] = -1;
        }
        return;
    }
    const int a = pair_img[2 * p], b = pair_img[2 * p + 1];
    long long m = m_arr[p];
    if (m > cap) m = cap;
    if (m < 0 || !in_range(a, n_img) || !in_range(b, n_img)) m = 0;
    const int oa = m ? img_off[a] : 0, ob = m ? img_off[b] : 0;
    double Ecur[9], Ebest[9];
    {
        const double* __restrict__ src = E + ((size_t)p * H * kSlots + slot) * 9;
#pragma unroll
        for (int k = 0; k < 9; ++k) Ebest[k] = Ecur[k] = src[k];
    }
    int n_best = 0, r_best = -1;
    for (int r = 0; r <= R; ++r) {
        const bool gather = r < R;
        const float wide2 = gather ? wide.w[r] : 0.f;
        double acc[kTri];
#pragma unroll
        for (int k = 0; k < kTri; ++k) acc[k] = 0.0;
        int c_in = 0, c_wide = 0;
        for (long long e = tid; e < m; e += kBlock) {
            double pt[4];
            if (!survivor_point(surv + p * cap, (int)e, oa, ob, n_nodes, xn, pt)) continue;
            const float err = sampson_value(Ecur, pt[0], pt[1], pt[2], pt[3]);
            c_in += err <= thr2;
            if (gather && err <= wide2) {
                ++c_wide;
                const double av[9] = {pt[2] * pt[0], pt[2] * pt[1], pt[2], pt[3] * pt[0], pt[3] * pt[1], pt[3], pt[0], pt[1], 1.0};
                int k = 0;
#pragma unroll
                for (int i = 0; i < 9; ++i)
#pragma unroll
                    for (int j = i; j < 9; ++j, ++k) acc[k] = acc[k] + av[i] * av[j];
            }
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            c_in += __shfl_xor(c_in, d, 64);
            c_wide += __shfl_xor(c_wide, d, 64);
        }
        if (gather) {
            // the fixed tree, levels h = 1, 2, .. 32 inside a wave: lane l (a multiple of 2h) takes s[l] + s[l + h]
#pragma unroll
            for (int k = 0; k < kTri; ++k) {
                double s = acc[k];
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) s = s + __shfl_xor(s, d, 64);
                acc[k] = s;
            }
        }
        __syncthreads();                                   // the previous round's readers of wcnt, wsum, Enew are done
        if (lane == 0) {
            wcnt[wave][0] = c_in;
            wcnt[wave][1] = c_wide;
            if (gather)
#pragma unroll
                for (int k = 0; k < kTri; ++k) wsum[wave][k] = acc[k];
        }
        __syncthreads();
        const int n_cur = wcnt[0][0] + wcnt[1][0] + wcnt[2][0] + wcnt[3][0];
        const int n_wide = wcnt[0][1] + wcnt[1][1] + wcnt[2][1] + wcnt[3][1];
        if (r == 0) {
            n_best = n_cur;
        } else if (n_cur > n_best) {
            n_best = n_cur;
            r_best = r - 1;
#pragma unroll
            for (int k = 0; k < 9; ++k) Ebest[k] = Ecur[k];
        }
        if (!gather || n_wide < 8) break;
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
            double En[9];
            refit_hd(Msh, En, work);
            bool ok = true;
            for (int k = 0; k < 9; ++k) {
                ok = ok && finite_hd(En[k]);
                Enew[k] = En[k];
            }
            finite = ok;
        }
        __syncthreads();
        if (!finite) break;
#pragma unroll
        for (int k = 0; k < 9; ++k) Ecur[k] = Enew[k];
    }
    if (tid < 9) {
        double v = 0;
#pragma unroll
        for (int k = 0; k < 9; ++k)
            if (k == tid) v = Ebest[k];
        E_lo[9 * g + tid] = v;
    }
    if (tid == 0) {
        n_lo[g] = n_best;
        round_lo[g] = r_best;
    }
}

// ---- pick -------------------------------------------------------------------------------------------------------------------------
// One wave per pair; lane t holds candidate t.
__global__ __launch_bounds__(64) void pick_kernel(const unsigned long long* __restrict__ top, const double* __restrict__ E_lo,
                                                  const int* __restrict__ n_lo, const int* __restrict__ round_lo, int T, int H,
                                                  double* __restrict__ E_sel, int* __restrict__ nmodels_sel, unsigned long long* __restrict__ best_sel,
                                                  int* __restrict__ lo_info) {
    const long long p = blockIdx.x;
    const int l = threadIdx.x;
    unsigned long long key = 0;
    bool has = false;
    if (l < T) {
        unsigned slot;
        has = slot_of(top[p * T + l], H, &slot);
        if (has) key = ((unsigned long long)(unsigned)n_lo[p * T + l] << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)l);
    }
    const int n_has = __popcll(__ballot(has));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(key, d, 64);
        key = o > key ? o : key;
    }
    const int win = key ? (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull)) : -1;
    for (int k = l; k < 9 * kSlots; k += 64) E_sel[p * (9 * kSlots) + k] = (win >= 0 && k < 9) ? E_lo[(p * T + win) * 9 + k] : 0.0;
    if (l == 0) {
        nmodels_sel[p] = win >= 0 ? 1 : 0;
        best_sel[p] = win >= 0 ? (key | 0xFFFFFFFFull) : 0ull;
        int* w = lo_info + 8 * p;
        unsigned slot = 0;
        if (win >= 0) slot_of(top[p * T + win], H, &slot);
        w[0] = (int)(top[p * T] >> 32);
        w[1] = win >= 0 ? (int)(key >> 32) : 0;
        w[2] = win;
        w[3] = win >= 0 ? round_lo[p * T + win] : -1;
        w[4] = win >= 0 ? (int)(slot / kSlots) : -1;
        w[5] = win >= 0 ? (int)(slot % kSlots) : -1;
        w[6] = n_has;
        w[7] = 0;
    }
}

bool lo_sizes_ok(int64_t n_pairs, int budget, int top) {
    return n_pairs >= 0 && n_pairs <= INT32_MAX / (kMaxBudget * kSlots) && budget >= 1 && budget <= kMaxBudget && top >= 1 && top <= kMaxTop;
}

}  // namespace

extern "C" int sfm_verify_top(const int32_t* counts_dev, const int32_t* nmodels_dev, int64_t n_pairs, int budget, int top, uint64_t* top_dev,
                              void* stream_) {
    SFM_CHECK_ARG(lo_sizes_ok(n_pairs, budget, top), "sfm_verify_top: bad sizes (n_pairs %lld, budget %d of 1..%d, top %d of 1..%d)",
                  (long long)n_pairs, budget, kMaxBudget, top, kMaxTop);
    if (n_pairs == 0) return SFM_OK;
    SFM_CHECK_ARG(counts_dev && nmodels_dev && top_dev, "sfm_verify_top: null pointer");
    hipLaunchKernelGGL(top_kernel, dim3((unsigned)n_pairs), dim3(kBlock), 0, sfm::as_stream(stream_), counts_dev, nmodels_dev, budget, top,
                       reinterpret_cast<unsigned long long*>(top_dev));
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" int sfm_verify_lo(const double* E_dev, const uint64_t* top_dev, int top, const int32_t* surv_dev, const int32_t* m_dev,
                             const int32_t* pair_img_dev, const int32_t* img_off_dev, int n_img, const double* xn_dev, int64_t n_nodes,
                             int64_t n_pairs, int64_t cap, int budget, float thr2, int rounds, const float* wide2_host, double* E_lo_dev,
                             int32_t* n_lo_dev, int32_t* round_lo_dev, void* stream_) {
    SFM_CHECK_ARG(lo_sizes_ok(n_pairs, budget, top) && cap >= 0 && cap <= INT32_MAX && n_pairs * cap <= INT32_MAX && n_img >= 1 &&
                      n_img <= kMaxImages && n_nodes >= 0 && n_nodes <= INT32_MAX,
                  "sfm_verify_lo: bad sizes");
    SFM_CHECK_ARG(rounds >= 0 && rounds <= kMaxRounds, "sfm_verify_lo: rounds must be 0..%d (got %d)", kMaxRounds, rounds);
    SFM_CHECK_ARG(rounds == 0 || wide2_host, "sfm_verify_lo: null wide2");
    SFM_CHECK_ARG(img_off_dev, "sfm_verify_lo: null img_off");
    Wide wide{};
    for (int r = 0; r < rounds; ++r) {
        SFM_CHECK_ARG(wide2_host[r] == wide2_host[r], "sfm_verify_lo: wide2[%d] is NaN", r);
        wide.w[r] = wide2_host[r];
    }
    if (n_pairs == 0) return SFM_OK;
    SFM_CHECK_ARG(E_dev && top_dev && m_dev && pair_img_dev && E_lo_dev && n_lo_dev && round_lo_dev && (cap == 0 || surv_dev) &&
                      (n_nodes == 0 || xn_dev),
                  "sfm_verify_lo: null pointer");
    hipLaunchKernelGGL(lo_kernel, dim3((unsigned)(n_pairs * top)), dim3(kBlock), 0, sfm::as_stream(stream_), E_dev,
                       reinterpret_cast<const unsigned long long*>(top_dev), top, reinterpret_cast<const int2*>(surv_dev), m_dev, pair_img_dev,
                       img_off_dev, n_img, reinterpret_cast<const double2*>(xn_dev), (long long)n_nodes, (long long)cap, budget, thr2, rounds, wide,
                       E_lo_dev, n_lo_dev, round_lo_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" int sfm_verify_lo_pick(const uint64_t* top_dev, const double* E_lo_dev, const int32_t* n_lo_dev, const int32_t* round_lo_dev,
                                  int64_t n_pairs, int budget, int top, double* E_sel_dev, int32_t* nmodels_sel_dev, uint64_t* best_sel_dev,
                                  int32_t* lo_info_dev, void* stream_) {
    SFM_CHECK_ARG(lo_sizes_ok(n_pairs, budget, top), "sfm_verify_lo_pick: bad sizes (n_pairs %lld, budget %d of 1..%d, top %d of 1..%d)",
                  (long long)n_pairs, budget, kMaxBudget, top, kMaxTop);
    if (n_pairs == 0) return SFM_OK;
    SFM_CHECK_ARG(top_dev && E_lo_dev && n_lo_dev && round_lo_dev && E_sel_dev && nmodels_sel_dev && best_sel_dev && lo_info_dev,
                  "sfm_verify_lo_pick: null pointer");
    hipLaunchKernelGGL(pick_kernel, dim3((unsigned)n_pairs), dim3(64), 0, sfm::as_stream(stream_),
                       reinterpret_cast<const unsigned long long*>(top_dev), E_lo_dev, n_lo_dev, round_lo_dev, top, budget, E_sel_dev,
                       nmodels_sel_dev, reinterpret_cast<unsigned long long*>(best_sel_dev), lo_info_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" int sfm_host_verify_refit(const double* M81_host, double* E_host) {
    SFM_CHECK_ARG(M81_host && E_host, "sfm_host_verify_refit: null pointer");
    double work[kRefitWork];
    refit_hd(M81_host, E_host, work);
    return SFM_OK;
}
