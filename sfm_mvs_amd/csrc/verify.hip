// Geometric verification of ALL matched pairs in a fixed number of launches and without a host wait (include/sfm_hip.h, "VERIFY";
// docs/tracks.md §11):
//   sfm_verify_normalise   K-normalised float64 coordinates of every node, once
//   sfm_verify_survivors   the Lowe survivors of every pair, compacted in ascending query order (a scan, no cursor)
//   sfm_verify_samples     H five-point samples per pair from a counter-based generator: a function of (seed, pair, sample) alone
//   sfm_verify_models      one lane per sample: the five-point solver of host_solvers.h, operation for operation, on the device
//   sfm_verify_score       one lane per model: Sampson inlier counts over the pair's survivors, the best model by an integer key
//   sfm_verify_select      per pair: the best model's inlier mask, its four pose candidates, the cheirality vote, keep / E / Rt / info
// A fixed budget of hypotheses replaces the adaptive sequential loop of sfm_find_essential_mat; nothing depends on the order in
// which lanes or workgroups run: counts are integers, the best model is the maximum of a 64-bit key, the vote is four counts.
//
// The device helpers (one-sided Jacobi SVD, Durand-Kerner roots, the five-point solver, the essential decomposition) are copies
// of sfm::host's in host_solvers.h and the DLT null vector is a copy of triangulate.hip's, as tracks_refine.hip and the mesh files
// copy theirs.  They use + - * / sqrt fabs fmax and comparisons only, every loop is bounded, and the library is built with
// -ffp-contract=off, so that a lane returns the bits the host function returns (tests/test_gpu_verify.py compares them).
// The polynomial cubes of the host (4 x 4 x 4, 20 slots used) are kept compact here: 20 coefficients and a table of the 84 products
// in the order the host's six nested loops visit them, so that every sum keeps its terms and their order.
#include <cfloat>
#include <climits>

#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxImages = 65536;
constexpr int kMaxBudget = 1024;                // samples per pair
constexpr int kMaxDraws = 64;                   // draws a sample may use to fill its five slots
constexpr int kSlots = 10;                      // models per sample
constexpr int kScoreGridY = 4;                  // workgroups of a pair that share its batches of 256 models
constexpr int kSolveIters = 300;                // Durand-Kerner sweeps (cv::solvePoly's default)
constexpr double kDistThresh = 50.0;            // cv2.recoverPose's distanceThresh as HipVerifyEngine passes it

__device__ inline bool in_range(int a, int n) { return (unsigned)a < (unsigned)n; }

// the scaled conversion of ransac.hip's KNorm: x * (1 / fx) + (-cx * (1 / fx)), multiply and add rounded separately
struct KNorm {
    double ifx, ify, bx, by;
    explicit KNorm(const double* K) : ifx(1. / K[0]), ify(1. / K[4]), bx(-K[2] * (1. / K[0])), by(-K[5] * (1. / K[4])) {}
};

__global__ __launch_bounds__(kBlock) void normalise_kernel(const float2* __restrict__ kp, long long n, KNorm k, double2* __restrict__ xn) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float2 p = kp[i];
    xn[i] = make_double2((double)p.x * k.ifx + k.bx, (double)p.y * k.ify + k.by);
}

// ---- survivors --------------------------------------------------------------------------------------------------------------
// One workgroup per pair walks the cap slots 256 at a time; a survivor's position is the number of survivors before it (ballot
// ranks inside a wave, the waves' totals through LDS, a running base across the chunks).
__global__ __launch_bounds__(kBlock) void survivors_kernel(const int* __restrict__ store, long long cap, const int* __restrict__ pair_img,
                                                           const int* __restrict__ nq, const int* __restrict__ img_off, int n_img,
                                                           double ratio, int2* __restrict__ surv, int* __restrict__ m_out) {
    __shared__ int wsum[kBlock / 64];
    const long long p = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int a = pair_img[2 * p], b = pair_img[2 * p + 1];
    long long limit = 0, nb = 0;
    if (in_range(a, n_img) && in_range(b, n_img) && a != b) {
        const long long na = (long long)img_off[a + 1] - img_off[a];
        nb = (long long)img_off[b + 1] - img_off[b];
        limit = nq[p];
        if (limit > cap) limit = cap;
        if (limit > na) limit = na;
    }
    int2* __restrict__ out = surv + p * cap;
    int base = 0;
    for (long long q0 = 0; q0 < limit; q0 += kBlock) {
        const long long q = q0 + threadIdx.x;
        bool pass = false;
        int t = -1;
        if (q < limit) {
            const int2 ii = *reinterpret_cast<const int2*>(store + ((2 * p) * cap + q) * 2);
            const int2 dd = *reinterpret_cast<const int2*>(store + ((2 * p + 1) * cap + q) * 2);
            const float d0 = __int_as_float(dd.x), d1 = __int_as_float(dd.y);
            pass = ii.y >= 0 && ii.x >= 0 && ii.x < nb && (double)d0 < ratio * (double)d1;
            t = ii.x;
        }
        const unsigned long long bal = __ballot(pass);
        const int rank = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) {
            if (w < wave) before += wsum[w];
            total += wsum[w];
        }
        if (pass) out[base + before + rank] = make_int2((int)q, t);
        base += total;
        __syncthreads();
    }
    for (long long c = base + threadIdx.x; c < cap; c += kBlock) out[c] = make_int2(-1, -1);
    if (threadIdx.x == 0) m_out[p] = base;
}

// ---- samples ----------------------------------------------------------------------------------------------------------------
__device__ inline unsigned mix(unsigned x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

__global__ __launch_bounds__(kBlock) void samples_kernel(const int* __restrict__ m_arr, long long n_pairs, int H, unsigned seed,
                                                         int* __restrict__ samp) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_pairs * H) return;
    const long long p = i / H;
    const unsigned s = (unsigned)(i - p * H);
    const int m = m_arr[p];
    int slot[5] = {-1, -1, -1, -1, -1};
    if (m >= 5) {
        const unsigned base = mix(mix(seed + 0x9e3779b9u * (unsigned)p) ^ s);
        int filled = 0;
        for (int c = 0; c < kMaxDraws && filled < 5; ++c) {
            const int idx = (int)(((unsigned long long)mix(base + (unsigned)c) * (unsigned long long)(unsigned)m) >> 32);
            bool dup = false;
#pragma unroll
            for (int k = 0; k < 5; ++k) dup = dup || (k < filled && slot[k] == idx);
            if (!dup) {
#pragma unroll
                for (int k = 0; k < 5; ++k)
                    if (k == filled) slot[k] = idx;
                ++filled;
            }
        }
        if (filled < 5) {
#pragma unroll
            for (int k = 0; k < 5; ++k) slot[k] = -1;
        }
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) samp[5 * i + k] = slot[k];
}

// ---- cv::SVD (sfm::host::Svd) -----------------------------------------------------------------------------------------------
// Sizes used here: 5 x 9 with FULL_UV (mm = 9, nn = 5, nine rows) and 3 x 3 (mm = nn = 3).
constexpr int kSvdMm = 9, kSvdNn = 5;

__device__ inline double hypot_cv(double a, double b) {
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

__device__ inline double dot2(const double* x, const double* y, int mm) {
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

__device__ inline void jacobi_dev(double* a, int mm, int nn, double* W, double* v) {
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

// Svd::compute(A, rows, cols, full_uv).  u_out (optional): the whole of u; vt_out (optional): rows vt_row0.. of vt, packed.
__device__ __noinline__ void svd_dev(const double* A, int rows, int cols, bool full_uv, double* u_out, double* vt_out, int vt_row0) {
    const int m = rows, n = cols;
    const bool at = m < n;
    const int mm = at ? n : m, nn = at ? m : n;
    const int urows = full_uv ? mm : nn;
    double a[kSvdMm * kSvdMm], v[kSvdNn * kSvdNn], W[kSvdNn];
    for (int i = 0; i < kSvdMm * kSvdMm; ++i) a[i] = 0;
    for (int i = 0; i < nn; ++i)
        for (int k = 0; k < mm; ++k) a[i * mm + k] = at ? A[i * n + k] : A[k * n + i];
    jacobi_dev(a, mm, nn, W, v);
    const double minval = DBL_MIN, eps = DBL_EPSILON * 10;
    unsigned long long state = 0x12345678u;                 // cv::RNG(0x12345678)
    for (int i = 0; i < urows; ++i) {
        double sd = i < nn ? W[i] : 0;
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
    if (!at) {
        if (u_out)
            for (int k = 0; k < mm; ++k)
                for (int i = 0; i < urows; ++i) u_out[k * urows + i] = a[i * mm + k];
        if (vt_out)
            for (int r = vt_row0; r < nn; ++r)
                for (int k = 0; k < nn; ++k) vt_out[(r - vt_row0) * nn + k] = v[r * nn + k];
    } else {
        if (u_out)
            for (int k = 0; k < nn; ++k)
                for (int i = 0; i < nn; ++i) u_out[k * nn + i] = v[i * nn + k];
        if (vt_out)
            for (int r = vt_row0; r < urows; ++r)
                for (int k = 0; k < mm; ++k) vt_out[(r - vt_row0) * mm + k] = a[r * mm + k];
    }
}

// ---- cv::solvePoly (sfm::host::solve_poly) ----------------------------------------------------------------------------------
struct Cx {
    double re, im;
};
__device__ inline Cx operator*(Cx a, Cx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ inline Cx operator-(Cx a, Cx b) { return {a.re - b.re, a.im - b.im}; }
__device__ inline Cx operator+(Cx a, Cx b) { return {a.re + b.re, a.im + b.im}; }
__device__ inline Cx operator/(Cx a, Cx b) {
    const double t = 1. / (b.re * b.re + b.im * b.im);
    return {(a.re * b.re + a.im * b.im) * t, (-a.re * b.im + a.im * b.re) * t};
}

__device__ __noinline__ int solve_poly_dev(const double* c, int deg, Cx* roots) {
    Cx coeffs[16];
    int n = deg;
    for (int i = 0; i <= n; ++i) coeffs[i] = {c[i], 0};
    for (; n > 1; --n)
        if (fabs(coeffs[n].re) + fabs(coeffs[n].im) > DBL_EPSILON) break;
    Cx p{1, 0};
    const Cx r{1, 1};
    for (int i = 0; i < n; ++i) {
        roots[i] = p;
        p = p * r;
    }
    for (int iter = 0; iter < kSolveIters; ++iter) {
        double max_diff = 0;
        for (int i = 0; i < n; ++i) {
            p = roots[i];
            Cx num = coeffs[n], denom = coeffs[n];
            for (int j = 0; j < n; ++j) {
                num = num * p + coeffs[n - j - 1];
                if (j != i) denom = denom * (p - roots[j]);
            }
            num = num / denom;
            roots[i] = p - num;
            max_diff = fmax(max_diff, sqrt(num.re * num.re + num.im * num.im));
        }
        if (max_diff <= 0) break;
    }
    for (int i = 0; i < n; ++i)
        if (fabs(roots[i].im) < 1e-100) roots[i].im = 0;
    return n;
}

// ---- five-point (sfm::host::five_point) -------------------------------------------------------------------------------------
// A polynomial in (x, y, z) of total degree <= 3: 20 coefficients; idx[i][j][k] is the slot of x^i y^j z^k.  mul lists the
// products (slot of a, slot of b, slot of the result) in the order of the host's loops over (i, j, k) then (l, m, o).
struct PolyTab {
    signed char idx[4][4][4];
    unsigned char mul[84][3];
    unsigned char mono[20];
};

constexpr PolyTab make_poly_tab() {
    PolyTab t{};
    int n = 0;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            for (int k = 0; k < 4; ++k) t.idx[i][j][k] = (i + j + k < 4) ? (signed char)n++ : (signed char)-1;
    int q = 0;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; i + j < 4; ++j)
            for (int k = 0; i + j + k < 4; ++k)
                for (int l = 0; i + l < 4; ++l)
                    for (int mm = 0; j + mm < 4; ++mm)
                        for (int o = 0; k + o < 4; ++o)
                            if (i + j + k + l + mm + o < 4) {
                                t.mul[q][0] = (unsigned char)t.idx[i][j][k];
                                t.mul[q][1] = (unsigned char)t.idx[l][mm][o];
                                t.mul[q][2] = (unsigned char)t.idx[i + l][j + mm][k + o];
                                ++q;
                            }
    const int mono[20][3] = {{3, 0, 0}, {0, 3, 0}, {2, 1, 0}, {1, 2, 0}, {2, 0, 1}, {2, 0, 0}, {0, 2, 1}, {0, 2, 0}, {1, 1, 1}, {1, 1, 0},
                             {1, 0, 2}, {1, 0, 1}, {1, 0, 0}, {0, 1, 2}, {0, 1, 1}, {0, 1, 0}, {0, 0, 3}, {0, 0, 2}, {0, 0, 1}, {0, 0, 0}};
    for (int m = 0; m < 20; ++m) t.mono[m] = (unsigned char)t.idx[mono[m][0]][mono[m][1]][mono[m][2]];
    return t;
}
static_assert(make_poly_tab().mul[83][2] == make_poly_tab().idx[3][0][0], "the last product is x^3 * 1");

__constant__ PolyTab kPoly = make_poly_tab();

struct Poly3 {
    double c[20];
};

__device__ inline void poly_zero(Poly3& p) {
    for (int i = 0; i < 20; ++i) p.c[i] = 0;
}
__device__ inline void poly_linear(Poly3& p, double cx, double cy, double cz, double c1) {
    poly_zero(p);
    p.c[kPoly.idx[1][0][0]] = cx;
    p.c[kPoly.idx[0][1][0]] = cy;
    p.c[kPoly.idx[0][0][1]] = cz;
    p.c[kPoly.idx[0][0][0]] = c1;
}
__device__ __noinline__ void poly_mul(const Poly3& a, const Poly3& b, Poly3& r) {
    poly_zero(r);
    for (int t = 0; t < 84; ++t) {
        const double av = a.c[kPoly.mul[t][0]];
        if (av == 0) continue;
        r.c[kPoly.mul[t][2]] += av * b.c[kPoly.mul[t][1]];
    }
}
__device__ inline void poly_axpy(Poly3& y, double a, const Poly3& x) {
    for (int i = 0; i < 20; ++i) y.c[i] += a * x.c[i];
}

// The ten cubic constraints on E = x E0 + y E1 + z E2 + E3 as the rows of A over Nister's monomial order.
__device__ __noinline__ void five_point_constraints(const double* EE /*4 x 9*/, double (*A)[20]) {
    Poly3 e[3][3], eet[3][3], tr, t0, t1;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) poly_linear(e[r][c], EE[3 * r + c], EE[9 + 3 * r + c], EE[18 + 3 * r + c], EE[27 + 3 * r + c]);
    Poly3 row;
    poly_zero(row);
    {
        const int cof[3][2] = {{1, 2}, {0, 2}, {0, 1}};
        for (int c = 0; c < 3; ++c) {
            poly_mul(e[1][cof[c][0]], e[2][cof[c][1]], t0);
            poly_mul(e[1][cof[c][1]], e[2][cof[c][0]], t1);
            poly_axpy(t0, -1.0, t1);
            poly_mul(e[0][c], t0, t1);
            poly_axpy(row, c == 1 ? -1.0 : 1.0, t1);
        }
    }
    for (int mm = 0; mm < 20; ++mm) A[0][mm] = row.c[kPoly.mono[mm]];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            poly_zero(eet[r][c]);
            for (int k = 0; k < 3; ++k) {
                poly_mul(e[r][k], e[c][k], t0);
                poly_axpy(eet[r][c], 1.0, t0);
            }
        }
    tr = eet[0][0];
    poly_axpy(tr, 1.0, eet[1][1]);
    poly_axpy(tr, 1.0, eet[2][2]);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            poly_zero(row);
            for (int k = 0; k < 3; ++k) {
                poly_mul(eet[r][k], e[k][c], t0);
                poly_axpy(row, 2.0, t0);
            }
            poly_mul(tr, e[r][c], t0);
            poly_axpy(row, -1.0, t0);
            for (int mm = 0; mm < 20; ++mm) A[1 + 3 * r + c][mm] = row.c[kPoly.mono[mm]];
        }
}

__device__ inline bool finite_dev(double x) { return fabs(x) <= DBL_MAX; }

__device__ int five_point_dev(const double* x1, const double* x2, double* E_out) {
    double EE[36];
    {
        double Q[45];
        for (int i = 0; i < 5; ++i) {
            const double a1 = x1[2 * i], b1 = x1[2 * i + 1], a2 = x2[2 * i], b2 = x2[2 * i + 1];
            double* q = Q + 9 * i;
            q[0] = a1 * a2; q[1] = b1 * a2; q[2] = a2;
            q[3] = a1 * b2; q[4] = b1 * b2; q[5] = b2;
            q[6] = a1;      q[7] = b1;      q[8] = 1.0;
        }
        svd_dev(Q, 5, 9, true, nullptr, EE, 5);
    }
    double A[10][20];
    five_point_constraints(EE, A);
    for (int col = 0; col < 10; ++col) {
        int piv = col;
        for (int r = col + 1; r < 10; ++r)
            if (fabs(A[r][col]) > fabs(A[piv][col])) piv = r;
        if (fabs(A[piv][col]) < DBL_EPSILON) return 0;
        if (piv != col)
            for (int mm = 0; mm < 20; ++mm) {
                const double t = A[col][mm];
                A[col][mm] = A[piv][mm];
                A[piv][mm] = t;
            }
        const double d = 1 / A[col][col];
        for (int r = col + 1; r < 10; ++r) {
            const double f = A[r][col] * d;
            for (int mm = col; mm < 20; ++mm) A[r][mm] -= f * A[col][mm];
        }
    }
    for (int col = 9; col >= 0; --col) {
        const double d = 1 / A[col][col];
        for (int mm = 10; mm < 20; ++mm) {
            double s = A[col][mm];
            for (int k = col + 1; k < 10; ++k) s -= A[col][k] * A[k][mm];
            A[col][mm] = s * d;
        }
    }
    double b[3][13];
    for (int i = 0; i < 3; ++i) {
        const double* ra = &A[2 * i + 4][10];
        const double* rb = &A[2 * i + 5][10];
        double r1[13], r2[13];
        for (int k = 0; k < 13; ++k) r1[k] = r2[k] = 0;
        for (int k = 0; k < 3; ++k) { r1[1 + k] = ra[k]; r1[5 + k] = ra[3 + k]; }
        for (int k = 0; k < 4; ++k) r1[9 + k] = ra[6 + k];
        for (int k = 0; k < 3; ++k) { r2[k] = rb[k]; r2[4 + k] = rb[3 + k]; }
        for (int k = 0; k < 4; ++k) r2[8 + k] = rb[6 + k];
        for (int k = 0; k < 13; ++k) b[i][k] = r1[k] - r2[k];
    }
    double pz[3][3][5];
    const int dg[3] = {3, 3, 4};
    for (int i = 0; i < 3; ++i) {
        for (int k = 0; k < 4; ++k) { pz[i][0][k] = b[i][3 - k]; pz[i][1][k] = b[i][7 - k]; }
        for (int k = 0; k < 5; ++k) pz[i][2][k] = b[i][12 - k];
    }
    double c[11];
    for (int k = 0; k < 11; ++k) c[k] = 0;
    const int perm[6][4] = {{0, 1, 2, 1}, {1, 2, 0, 1}, {2, 0, 1, 1}, {2, 1, 0, -1}, {1, 0, 2, -1}, {0, 2, 1, -1}};
    for (int p = 0; p < 6; ++p) {
        double t[11], uu[11];
        const int c0 = perm[p][0], c1 = perm[p][1], c2 = perm[p][2];
        {
            const double *pa = pz[0][c0], *pb = pz[1][c1];
            const int da = dg[c0], db = dg[c1];
            for (int i = 0; i <= da + db; ++i) t[i] = 0;
            for (int i = 0; i <= da; ++i)
                for (int j = 0; j <= db; ++j) t[i + j] += pa[i] * pb[j];
        }
        {
            const double* pb = pz[2][c2];
            const int da = dg[c0] + dg[c1], db = dg[c2];
            for (int i = 0; i <= da + db; ++i) uu[i] = 0;
            for (int i = 0; i <= da; ++i)
                for (int j = 0; j <= db; ++j) uu[i + j] += t[i] * pb[j];
        }
        for (int k = 0; k <= 10; ++k) c[k] += perm[p][3] * uu[k];
    }
    for (int k = 0; k < 11; ++k)
        if (!finite_dev(c[k])) return 0;
    Cx roots[10];
    const int nroots = solve_poly_dev(c, 10, roots);
    int count = 0;
    for (int i = 0; i < nroots; ++i) {
        if (fabs(roots[i].im) > 1e-10) continue;
        const double z1 = roots[i].re, z2 = z1 * z1, z3 = z2 * z1, z4 = z3 * z1;
        double bz[9];
        for (int j = 0; j < 3; ++j) {
            const double* br = b[j];
            bz[3 * j + 0] = br[0] * z3 + br[1] * z2 + br[2] * z1 + br[3];
            bz[3 * j + 1] = br[4] * z3 + br[5] * z2 + br[6] * z1 + br[7];
            bz[3 * j + 2] = br[8] * z4 + br[9] * z3 + br[10] * z2 + br[11] * z1 + br[12];
        }
        double xy1[3];
        svd_dev(bz, 3, 3, false, nullptr, xy1, 2);
        if (fabs(xy1[2]) < 1e-10) continue;
        const double x = xy1[0] / xy1[2], y = xy1[1] / xy1[2];
        double Ev[9], nrm = 0;
        for (int k = 0; k < 9; ++k) {
            Ev[k] = EE[k] * x + EE[9 + k] * y + EE[18 + k] * z1 + EE[27 + k];
            nrm += Ev[k] * Ev[k];
        }
        nrm = sqrt(nrm);
        for (int k = 0; k < 9; ++k) E_out[9 * count + k] = Ev[k] / nrm;
        ++count;
    }
    return count;
}

// The float64 coordinates of survivor e of a pair, (a1, b1, a2, b2); false when it names no node.
__device__ inline bool survivor_point(const int2* __restrict__ surv_p, int e, int oa, int ob, long long n_nodes,
                                      const double2* __restrict__ xn, double* pt) {
    const int2 qt = surv_p[e];
    const long long u = (long long)oa + qt.x, v = (long long)ob + qt.y;
    if (qt.x < 0 || qt.y < 0 || u >= n_nodes || v >= n_nodes) return false;
    const double2 a = xn[u], b = xn[v];
    pt[0] = a.x; pt[1] = a.y; pt[2] = b.x; pt[3] = b.y;
    return true;
}

// One lane per (pair, sample).
__global__ __launch_bounds__(64) void models_kernel(const int* __restrict__ samp, const int2* __restrict__ surv, const int* __restrict__ m_arr,
                                                    const int* __restrict__ pair_img, const int* __restrict__ img_off, int n_img,
                                                    const double2* __restrict__ xn, long long n_nodes, long long n_pairs, long long cap, int H,
                                                    int* __restrict__ nmodels, double* __restrict__ E) {
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    if (i >= n_pairs * H) return;
    const long long p = i / H;
    double x1[10], x2[10], Em[9 * kSlots];
    const int a = pair_img[2 * p], b = pair_img[2 * p + 1];
    long long m = m_arr[p];
    if (m > cap) m = cap;
    bool ok = in_range(a, n_img) && in_range(b, n_img) && m >= 5;
    if (ok) {
        const int oa = img_off[a], ob = img_off[b];
        for (int k = 0; k < 5; ++k) {
            const int idx = samp[5 * i + k];
            double pt[4] = {0, 0, 0, 0};
            ok = ok && idx >= 0 && idx < m && survivor_point(surv + p * cap, idx < 0 || idx >= m ? 0 : idx, oa, ob, n_nodes, xn, pt);
            x1[2 * k] = pt[0]; x1[2 * k + 1] = pt[1];
            x2[2 * k] = pt[2]; x2[2 * k + 1] = pt[3];
        }
    }
    const int count = ok ? five_point_dev(x1, x2, Em) : 0;
    nmodels[i] = count;
    double* __restrict__ out = E + (size_t)i * (9 * kSlots);
    for (int k = 0; k < 9 * kSlots; ++k) out[k] = k < 9 * count ? Em[k] : 0.0;
}

// ---- score ------------------------------------------------------------------------------------------------------------------
// The expression of residual.hip's score_essential_kernel.
__device__ __forceinline__ bool sampson_in(const double* __restrict__ E, double a1, double b1, double a2, double b2, float thr2) {
    const double e0 = E[0] * a1 + E[1] * b1 + E[2] * 1., e1 = E[3] * a1 + E[4] * b1 + E[5] * 1., e2 = E[6] * a1 + E[7] * b1 + E[8] * 1.;
    const double f0 = E[0] * a2 + E[3] * b2 + E[6] * 1., f1 = E[1] * a2 + E[4] * b2 + E[7] * 1.;
    const double x2tEx1 = a2 * e0 + b2 * e1 + 1. * e2;
    const double a = e0 * e0, b = e1 * e1, c = f0 * f0, d = f1 * f1;
    const float err = (float)(x2tEx1 * x2tEx1 / (a + b + c + d));
    return err <= thr2;
}

// Workgroup (p, y): the models of pair p, compacted over its samples, in batches of 256, one lane per model; the pair's survivors
// pass through LDS 256 at a time and every lane reads each of them (a broadcast).  Counts stay in a register; nothing is reduced.
__global__ __launch_bounds__(kBlock) void score_kernel(const double* __restrict__ E, const int* __restrict__ nmodels, const int2* __restrict__ surv,
                                                       const int* __restrict__ m_arr, const int* __restrict__ pair_img,
                                                       const int* __restrict__ img_off, int n_img, const double2* __restrict__ xn,
                                                       long long n_nodes, long long cap, int H, float thr2, int* __restrict__ counts,
                                                       unsigned long long* __restrict__ best) {
    __shared__ int pref[kMaxBudget + 1];
    __shared__ int part[kBlock];
    __shared__ double pts[kBlock][4];
    __shared__ int valid[kBlock];
    const long long p = blockIdx.x;
    const int tid = threadIdx.x;
    // exclusive prefix of the model counts over the samples: four samples a lane, the lanes' totals by a Hillis-Steele scan
    int mine[4], tot = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int s = 4 * tid + k;
        int c = s < H ? nmodels[p * H + s] : 0;
        c = c < 0 ? 0 : c > kSlots ? kSlots : c;
        mine[k] = c;
        tot += c;
    }
    part[tid] = tot;
    __syncthreads();
    for (int d = 1; d < kBlock; d <<= 1) {
        const int add = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    int run = part[tid] - tot;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        pref[4 * tid + k] = run;
        run += mine[k];
    }
    if (tid == kBlock - 1) pref[kMaxBudget] = run;
    __syncthreads();
    const int T = pref[kMaxBudget];
    const int a = pair_img[2 * p], b = pair_img[2 * p + 1];
    long long m = m_arr[p];
    if (m > cap) m = cap;
    if (m < 0 || !in_range(a, n_img) || !in_range(b, n_img)) m = 0;
    const int oa = m ? img_off[a] : 0, ob = m ? img_off[b] : 0;
    for (int g0 = blockIdx.y * kBlock; g0 < T; g0 += gridDim.y * kBlock) {
        const int g = g0 + tid;
        const bool live = g < T;
        int s = 0, j = 0;
        double Em[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (live) {
            int lo = 0, hi = kMaxBudget;                                        // pref[lo] <= g < pref[hi]
            for (int step = 0; step < 10; ++step) {
                const int mid = (lo + hi) >> 1;
                if (pref[mid] <= g) lo = mid; else hi = mid;
            }
            s = lo;
            j = g - pref[lo];
            const double* __restrict__ src = E + ((size_t)(p * H + s) * kSlots + j) * 9;
#pragma unroll
            for (int k = 0; k < 9; ++k) Em[k] = src[k];
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
                for (int k = 0; k < nt; ++k)
                    count += valid[k] && sampson_in(Em, pts[k][0], pts[k][1], pts[k][2], pts[k][3], thr2);
            __syncthreads();
        }
        unsigned long long key = 0;
        if (live) {
            const unsigned slot = (unsigned)(kSlots * s + j);
            counts[(p * H + s) * kSlots + j] = count;
            key = ((unsigned long long)(unsigned)count << 32) | (unsigned long long)(0xFFFFFFFFu - slot);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const unsigned long long o = __shfl_xor(key, d, 64);
            key = o > key ? o : key;
        }
        if ((tid & 63) == 0 && key) atomicMax(&best[p], key);
    }
}

// ---- select -----------------------------------------------------------------------------------------------------------------
__device__ inline double det3(const double* M) {
    return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}
__device__ inline void mul3(const double* A, const double* B, double* C) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0;
            for (int k = 0; k < 3; ++k) s += A[3 * i + k] * B[3 * k + j];
            C[3 * i + j] = s;
        }
}

// sfm::host::decompose_essential
__device__ void decompose_essential_dev(const double* E, double* R1, double* R2, double* t) {
    double U[9], Vt[9], T[9];
    svd_dev(E, 3, 3, false, U, Vt, 0);
    if (det3(U) < 0)
        for (int k = 0; k < 9; ++k) U[k] *= -1.;
    if (det3(Vt) < 0)
        for (int k = 0; k < 9; ++k) Vt[k] *= -1.;
    const double W[9] = {0, 1, 0, -1, 0, 0, 0, 0, 1}, Wt[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1};
    mul3(U, W, T);
    mul3(T, Vt, R1);
    mul3(U, Wt, T);
    mul3(T, Vt, R2);
    t[0] = U[2] * 1.0; t[1] = U[5] * 1.0; t[2] = U[8] * 1.0;
}

// triangulate.hip's rows = 4 DLT and its one-sided Jacobi null vector (cv2.triangulatePoints inside cv2.recoverPose)
template <int I, int J>
__device__ __forceinline__ void jacobi_pair(double (&At)[4][4], double (&V)[4][4], double (&W)[4], bool& changed) {
    const double eps = DBL_EPSILON * 10;
    double a = W[I], b = W[J];
    double s0 = 0, s1 = 0;
#pragma unroll
    for (int k = 0; k < 4; k += 2) {
        s0 = s0 + At[I][k] * At[J][k];
        s1 = s1 + At[I][k + 1] * At[J][k + 1];
    }
    double p = s0 + s1;
    if (fabs(p) <= eps * sqrt(a * b)) return;
    p *= 2;
    const double beta = a - b, gamma = hypot_cv(p, beta);
    double c, s;
    if (beta < 0) {
        const double delta = (gamma - beta) * 0.5;
        s = sqrt(delta / gamma);
        c = p / (gamma * s * 2);
    } else {
        c = sqrt((gamma + beta) / (gamma * 2));
        s = p / (gamma * c * 2);
    }
    double a0 = 0, a1 = 0, b0 = 0, b1 = 0;
#pragma unroll
    for (int k = 0; k < 4; k += 2) {
        const double t0 = c * At[I][k] + s * At[J][k], t1 = c * At[J][k] - s * At[I][k];
        const double u0 = c * At[I][k + 1] + s * At[J][k + 1], u1 = c * At[J][k + 1] - s * At[I][k + 1];
        At[I][k] = t0; At[J][k] = t1; At[I][k + 1] = u0; At[J][k + 1] = u1;
        a0 = a0 + t0 * t0; b0 = b0 + t1 * t1;
        a1 = a1 + u0 * u0; b1 = b1 + u1 * u1;
    }
    W[I] = a0 + a1;
    W[J] = b0 + b1;
    changed = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double t0 = c * V[I][k] + s * V[J][k], t1 = -s * V[I][k] + c * V[J][k];
        V[I][k] = t0; V[J][k] = t1;
    }
}

__device__ __forceinline__ void dlt_nullvec(double (&At)[4][4], double (&X)[4]) {
    double V[4][4], W[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) sd += At[a][k] * At[a][k];
        W[a] = sd;
#pragma unroll
        for (int k = 0; k < 4; ++k) V[a][k] = (a == k) ? 1.0 : 0.0;
    }
    for (int iter = 0; iter < 30; ++iter) {
        bool changed = false;
        jacobi_pair<0, 1>(At, V, W, changed);
        jacobi_pair<0, 2>(At, V, W, changed);
        jacobi_pair<0, 3>(At, V, W, changed);
        jacobi_pair<1, 2>(At, V, W, changed);
        jacobi_pair<1, 3>(At, V, W, changed);
        jacobi_pair<2, 3>(At, V, W, changed);
        if (!changed) break;
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) sd += At[a][k] * At[a][k];
        W[a] = sqrt(sd);
    }
    int id[4] = {0, 1, 2, 3};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double wj = W[a];
        int j = a;
#pragma unroll
        for (int k = a + 1; k < 4; ++k)
            if (wj < W[k]) { wj = W[k]; j = k; }
#pragma unroll
        for (int k = a + 1; k < 4; ++k)
            if (j == k) {
                const double tw = W[a]; W[a] = W[k]; W[k] = tw;
                const int ti = id[a]; id[a] = id[k]; id[k] = ti;
            }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) X[k] = id[3] == 0 ? V[0][k] : id[3] == 1 ? V[1][k] : id[3] == 2 ? V[2][k] : V[3][k];
}

// recover_pose_kernel<4>'s test of one correspondence against [I | 0] and P1 = [R | t]
__device__ __forceinline__ bool cheirality(const double* __restrict__ P1, double a1, double b1, double a2, double b2) {
    double At[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double p0 = k == 0 ? 1. : 0., p4 = k == 1 ? 1. : 0., p8 = k == 2 ? 1. : 0.;
        At[k][0] = a1 * p8 - p0;
        At[k][1] = b1 * p8 - p4;
        At[k][2] = a2 * P1[8 + k] - P1[k];
        At[k][3] = b2 * P1[8 + k] - P1[4 + k];
    }
    double Q[4];
    dlt_nullvec(At, Q);
    bool good = Q[2] * Q[3] > 0;
    const double q0 = Q[0] / Q[3], q1 = Q[1] / Q[3], q2 = Q[2] / Q[3], q3 = Q[3] / Q[3];
    good = (q2 < kDistThresh) && good;
    const double z = ((P1[8] * q0 + P1[9] * q1) + P1[10] * q2) + P1[11] * q3;
    good = (z > 0) && good;
    good = (z < kDistThresh) && good;
    return good;
}

enum Status { kFewSurvivors = 1, kNoModel = 2, kNoVote = 4 };

// One workgroup per pair.  keep[p][q] first holds a survivor's five bits (Sampson inlier, four votes) and then, written by the
// same lane, its final value; the counts are integer sums in LDS.
__global__ __launch_bounds__(kBlock) void select_kernel(const double* __restrict__ E, const int* __restrict__ nmodels,
                                                        const unsigned long long* __restrict__ best, const int2* __restrict__ surv,
                                                        const int* __restrict__ m_arr, const int* __restrict__ pair_img,
                                                        const int* __restrict__ img_off, int n_img, const double2* __restrict__ xn,
                                                        long long n_nodes, long long cap, int H, float thr2, unsigned char* __restrict__ keep,
                                                        double* __restrict__ E_out, double* __restrict__ Rt_out, int* __restrict__ info) {
    __shared__ double Eb[9];
    __shared__ double cand[4][12];
    __shared__ int cnt[5], scored, has, bs, bj;
    const long long p = blockIdx.x;
    const int tid = threadIdx.x;
    const int a = pair_img[2 * p], b = pair_img[2 * p + 1];
    long long m = m_arr[p];
    if (m > cap) m = cap;
    if (m < 0 || !in_range(a, n_img) || !in_range(b, n_img)) m = 0;
    const int oa = m ? img_off[a] : 0, ob = m ? img_off[b] : 0;
    if (tid == 0) {
        scored = 0;
        for (int k = 0; k < 5; ++k) cnt[k] = 0;
        const unsigned long long key = best[p];
        const unsigned slot = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
        const int s = (int)(slot / kSlots), j = (int)(slot % kSlots);
        const bool ok = key != 0 && slot < (unsigned)H * kSlots;
        has = ok;
        bs = ok ? s : -1;
        bj = ok ? j : -1;
        if (ok) {
            const double* __restrict__ src = E + ((size_t)(p * H + s) * kSlots + j) * 9;
            double Em[9], R1[9], R2[9], t[3];
            for (int k = 0; k < 9; ++k) Eb[k] = Em[k] = src[k];
            decompose_essential_dev(Em, R1, R2, t);
            for (int c = 0; c < 4; ++c)
                for (int i = 0; i < 3; ++i) {
                    for (int k = 0; k < 3; ++k) cand[c][4 * i + k] = (c & 1) ? R2[3 * i + k] : R1[3 * i + k];
                    cand[c][4 * i + 3] = (c < 2 ? 1. : -1.) * t[i];
                }
        }
    }
    for (long long c = tid; c < cap; c += kBlock) keep[p * cap + c] = 0;
    __syncthreads();
    int sum = 0;
    for (int s = tid; s < H; s += kBlock) {
        const int c = nmodels[p * H + s];
        sum += c < 0 ? 0 : c > kSlots ? kSlots : c;
    }
    if (sum) atomicAdd(&scored, sum);
    const bool have_model = has != 0;
    if (have_model) {
        double Em[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) Em[k] = Eb[k];
        for (long long e = tid; e < m; e += kBlock) {
            double pt[4];
            if (!survivor_point(surv + p * cap, (int)e, oa, ob, n_nodes, xn, pt)) continue;
            const int q = surv[p * cap + e].x;
            if (q >= cap || !sampson_in(Em, pt[0], pt[1], pt[2], pt[3], thr2)) continue;
            int bits = 16;
            for (int c = 0; c < 4; ++c)
                if (cheirality(cand[c], pt[0], pt[1], pt[2], pt[3])) bits |= 1 << c;
            keep[p * cap + q] = (unsigned char)bits;
            atomicAdd(&cnt[4], 1);
            for (int c = 0; c < 4; ++c)
                if (bits & (1 << c)) atomicAdd(&cnt[c], 1);
        }
    }
    __syncthreads();
    int win = 0;
    for (int c = 1; c < 4; ++c)
        if (cnt[c] > cnt[win]) win = c;
    if (have_model)
        for (long long e = tid; e < m; e += kBlock) {
            const int q = surv[p * cap + e].x;
            if (q < 0 || q >= cap) continue;
            const int bits = keep[p * cap + q];
            if (bits & 16) keep[p * cap + q] = (bits >> win) & 1;
        }
    if (tid == 0) {
        for (int k = 0; k < 9; ++k) E_out[9 * p + k] = have_model ? Eb[k] : 0.0;
        for (int k = 0; k < 12; ++k) Rt_out[12 * p + k] = have_model ? cand[win][k] : 0.0;
        int* w = info + 8 * p;
        w[0] = (int)m_arr[p];
        w[1] = scored;
        w[2] = cnt[4];
        w[3] = have_model ? cnt[win] : 0;
        w[4] = bs;
        w[5] = bj;
        w[6] = have_model ? win : -1;
        w[7] = (m_arr[p] < 5 ? kFewSurvivors : 0) | (have_model ? 0 : kNoModel) | (have_model && cnt[win] == 0 ? kNoVote : 0);
    }
}

bool pair_sizes_ok(int64_t n_pairs, int64_t cap, int n_img) {
    return n_pairs >= 0 && cap >= 0 && n_pairs <= INT32_MAX && cap <= INT32_MAX && n_pairs * cap <= INT32_MAX && n_img >= 1 && n_img <= kMaxImages;
}

}  // namespace

extern "C" int sfm_verify_normalise(const float* kp_dev, int64_t n_nodes, const double* K_host, double* xn_dev, void* stream_) {
    SFM_CHECK_ARG(n_nodes >= 0 && n_nodes <= INT32_MAX, "sfm_verify_normalise: bad n_nodes");
    SFM_CHECK_ARG(K_host, "sfm_verify_normalise: null K");
    if (n_nodes == 0) return SFM_OK;
    SFM_CHECK_ARG(kp_dev && xn_dev, "sfm_verify_normalise: null pointer");
    hipLaunchKernelGGL(normalise_kernel, dim3((unsigned)((n_nodes + kBlock - 1) / kBlock)), dim3(kBlock), 0, sfm::as_stream(stream_),
                       reinterpret_cast<const float2*>(kp_dev), (long long)n_nodes, KNorm(K_host), reinterpret_cast<double2*>(xn_dev));
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" int sfm_verify_survivors(const int32_t* store_dev, int64_t n_pairs, int64_t cap, const int32_t* pair_img_dev, const int32_t* nq_dev,
                                    const int32_t* img_off_dev, int n_img, double ratio, int32_t* surv_dev, int32_t* m_dev, void* stream_) {
    SFM_CHECK_ARG(pair_sizes_ok(n_pairs, cap, n_img), "sfm_verify_survivors: bad sizes");
    SFM_CHECK_ARG(ratio == ratio, "sfm_verify_survivors: the ratio is NaN");
    SFM_CHECK_ARG(img_off_dev, "sfm_verify_survivors: null img_off");
    if (n_pairs == 0) return SFM_OK;
    SFM_CHECK_ARG(pair_img_dev && nq_dev && m_dev && (cap == 0 || (store_dev && surv_dev)), "sfm_verify_survivors: null pointer");
    hipLaunchKernelGGL(survivors_kernel, dim3((unsigned)n_pairs), dim3(kBlock), 0, sfm::as_stream(stream_), store_dev, (long long)cap, pair_img_dev,
                       nq_dev, img_off_dev, n_img, ratio, reinterpret_cast<int2*>(surv_dev), m_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" int sfm_verify_samples(const int32_t* m_dev, int64_t n_pairs, int budget, uint32_t seed, int32_t* samp_dev, void* stream_) {
    SFM_CHECK_ARG(n_pairs >= 0 && n_pairs <= INT32_MAX / kMaxBudget, "sfm_verify_samples: bad n_pairs");
    SFM_CHECK_ARG(budget >= 1 && budget <= kMaxBudget, "sfm_verify_samples: the budget must be 1..%d (got %d)", kMaxBudget, budget);
    if (n_pairs == 0) return SFM_OK;
    SFM_CHECK_ARG(m_dev && samp_dev, "sfm_verify_samples: null pointer");
    const long long n = (long long)n_pairs * budget;
    hipLaunchKernelGGL(samples_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, sfm::as_stream(stream_), m_dev, (long long)n_pairs,
                       budget, seed, samp_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" int sfm_verify_models(const int32_t* samp_dev, const int32_t* surv_dev, const int32_t* m_dev, const int32_t* pair_img_dev,
                                 const int32_t* img_off_dev, int n_img, const double* xn_dev, int64_t n_nodes, int64_t n_pairs, int64_t cap,
                                 int budget, int32_t* nmodels_dev, double* E_dev, void* stream_) {
    SFM_CHECK_ARG(pair_sizes_ok(n_pairs, cap, n_img) && n_pairs <= INT32_MAX / kMaxBudget && n_nodes >= 0 && n_nodes <= INT32_MAX,
                  "sfm_verify_models: bad sizes");
    SFM_CHECK_ARG(budget >= 1 && budget <= kMaxBudget, "sfm_verify_models: the budget must be 1..%d (got %d)", kMaxBudget, budget);
    SFM_CHECK_ARG(img_off_dev, "sfm_verify_models: null img_off");
    if (n_pairs == 0) return SFM_OK;
    SFM_CHECK_ARG(samp_dev && m_dev && pair_img_dev && nmodels_dev && E_dev && (cap == 0 || surv_dev) && (n_nodes == 0 || xn_dev),
                  "sfm_verify_models: null pointer");
    const long long n = (long long)n_pairs * budget;
    hipLaunchKernelGGL(models_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, sfm::as_stream(stream_), samp_dev,
                       reinterpret_cast<const int2*>(surv_dev), m_dev, pair_img_dev, img_off_dev, n_img, reinterpret_cast<const double2*>(xn_dev),
                       (long long)n_nodes, (long long)n_pairs, (long long)cap, budget, nmodels_dev, E_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" int sfm_verify_score(const double* E_dev, const int32_t* nmodels_dev, const int32_t* surv_dev, const int32_t* m_dev,
                                const int32_t* pair_img_dev, const int32_t* img_off_dev, int n_img, const double* xn_dev, int64_t n_nodes,
                                int64_t n_pairs, int64_t cap, int budget, float thr2, int32_t* counts_dev, uint64_t* best_dev, void* stream_) {
    SFM_CHECK_ARG(pair_sizes_ok(n_pairs, cap, n_img) && n_pairs <= INT32_MAX / (kMaxBudget * kSlots) && n_nodes >= 0 && n_nodes <= INT32_MAX,
                  "sfm_verify_score: bad sizes");
    SFM_CHECK_ARG(budget >= 1 && budget <= kMaxBudget, "sfm_verify_score: the budget must be 1..%d (got %d)", kMaxBudget, budget);
    SFM_CHECK_ARG(img_off_dev, "sfm_verify_score: null img_off");
    if (n_pairs == 0) return SFM_OK;
    SFM_CHECK_ARG(E_dev && nmodels_dev && m_dev && pair_img_dev && counts_dev && best_dev && (cap == 0 || surv_dev) && (n_nodes == 0 || xn_dev),
                  "sfm_verify_score: null pointer");
    hipStream_t stream = sfm::as_stream(stream_);
    SFM_CHECK_HIP(hipMemsetAsync(counts_dev, 0, sizeof(int32_t) * (size_t)n_pairs * (size_t)budget * kSlots, stream));
    SFM_CHECK_HIP(hipMemsetAsync(best_dev, 0, sizeof(uint64_t) * (size_t)n_pairs, stream));
    const int batches = (budget * kSlots + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(score_kernel, dim3((unsigned)n_pairs, (unsigned)(batches < kScoreGridY ? batches : kScoreGridY)), dim3(kBlock), 0, stream, E_dev,
                       nmodels_dev, reinterpret_cast<const int2*>(surv_dev), m_dev, pair_img_dev, img_off_dev, n_img,
                       reinterpret_cast<const double2*>(xn_dev), (long long)n_nodes, (long long)cap, budget, thr2, counts_dev,
                       reinterpret_cast<unsigned long long*>(best_dev));
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" int sfm_verify_select(const double* E_dev, const int32_t* nmodels_dev, const uint64_t* best_dev, const int32_t* surv_dev,
                                 const int32_t* m_dev, const int32_t* pair_img_dev, const int32_t* img_off_dev, int n_img, const double* xn_dev,
                                 int64_t n_nodes, int64_t n_pairs, int64_t cap, int budget, float thr2, uint8_t* keep_dev, double* E_out_dev,
                                 double* Rt_dev, int32_t* info_dev, void* stream_) {
    SFM_CHECK_ARG(pair_sizes_ok(n_pairs, cap, n_img) && n_pairs <= INT32_MAX / (kMaxBudget * kSlots) && n_nodes >= 0 && n_nodes <= INT32_MAX,
                  "sfm_verify_select: bad sizes");
    SFM_CHECK_ARG(budget >= 1 && budget <= kMaxBudget, "sfm_verify_select: the budget must be 1..%d (got %d)", kMaxBudget, budget);
    SFM_CHECK_ARG(img_off_dev, "sfm_verify_select: null img_off");
    if (n_pairs == 0) return SFM_OK;
    SFM_CHECK_ARG(E_dev && nmodels_dev && best_dev && m_dev && pair_img_dev && E_out_dev && Rt_dev && info_dev &&
                      (cap == 0 || (surv_dev && keep_dev)) && (n_nodes == 0 || xn_dev),
                  "sfm_verify_select: null pointer");
    hipLaunchKernelGGL(select_kernel, dim3((unsigned)n_pairs), dim3(kBlock), 0, sfm::as_stream(stream_), E_dev, nmodels_dev,
                       reinterpret_cast<const unsigned long long*>(best_dev), reinterpret_cast<const int2*>(surv_dev), m_dev, pair_img_dev,
                       img_off_dev, n_img, reinterpret_cast<const double2*>(xn_dev), (long long)n_nodes, (long long)cap, budget, thr2, keep_dev,
                       E_out_dev, Rt_dev, info_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}
