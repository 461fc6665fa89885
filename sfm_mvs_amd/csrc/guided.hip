// Guided matching (include/sfm_hip.h, "GUIDED"; docs/tracks.md §14): the 2-NN of every query among the train keypoints inside the
// epipolar band of its pair's essential matrix, and the mutual check on it.
//   sfm_guided_match    workgroup (pair, block of 256 queries): a lane owns a query with e0, e1, e2 in registers; the train keypoints
//                       pass through LDS 256 at a time with their f0^2 and f1^2 and are read as broadcasts; band hits are compacted by
//                       ballot into a queue of (lane, t) per wave, which the wave drains two lanes a candidate; best two keys in the
//                       owner's registers; one 64-bit atomicMin per candidate on rev
//   sfm_guided_mutual   workgroup per pair: keep_g and the four counts
// Nothing depends on the order in which lanes or workgroups run: the store holds the two smallest of a set of distinct integer keys,
// rev a minimum of integer keys, info counts.
//
// The band test is verify.hip's sampson_in (a copy of its words, as verify_h.hip copies that file's helpers), split into the part that
// belongs to the query, the part that belongs to the train keypoint and the part that belongs to both.  The library is built with
// -ffp-contract=off: no FMA is formed.
#include <cfloat>
#include <climits>
#include <cmath>

#include "common.h"

namespace {

constexpr int kBlock = 256;                     // queries of a workgroup = train keypoints of a tile
constexpr int kWaves = kBlock / 64;
constexpr int kQueue = 128;                     // entries of a wave's queue: drained from 64, one step appends at most 64
constexpr int kDim = 128;
constexpr int kMaxImages = 65536;
constexpr unsigned long long kNoKey = ~0ull;

__device__ inline bool in_range(int a, int n) { return (unsigned)a < (unsigned)n; }

// The guard band of the multiplied test.  With T = thr2g a positive normal float, den > 0 and T * den neither subnormal nor
// infinite: fl(T den) = T den (1 + d), |d| <= 2^-53, and q = fl(num / den).
//   num <= fl(T den) (1 - 2^-50)  =>  num / den < T  =>  q <= T (T is a double)  =>  (float)q <= T: in the band.
//   num >= fl(T den) (1 + 2^-22)  =>  num / den > T (1 + 2^-23) >= the float above T  =>  (float)q > T: out of the band.
// Everything between, and every input outside these conditions (NaN, inf, zero, T <= 0, T subnormal or infinite), is divided.
constexpr double kGuardLo = 1.0 - 0x1p-50;
constexpr double kGuardHi = 1.0 + 0x1p-22;
constexpr double kMinBound = 0x1p-900;

// A wave's lanes read what other lanes of the SAME wave wrote to LDS: the writes are complete and the compiler moves nothing across.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ void insert_key(unsigned long long key, unsigned long long& k0, unsigned long long& k1) {
    const unsigned long long lo = key < k0 ? key : k0, mid = key < k0 ? k0 : key;      // the two smallest of three, without a branch
    k1 = mid < k1 ? mid : k1;
    k0 = lo;
}

// The query bound of a pair and the offsets and sizes it needs; 0 when the pair has no band.
struct PairBand {
    int qb, nt, oa, ob;
};

__device__ __forceinline__ PairBand pair_band(const int* __restrict__ pair_img, const int* __restrict__ nq, const int* __restrict__ img_off, int n_img,
                                     long long cap, long long rev_stride, long long p, bool active) {
    PairBand b = {0, 0, 0, 0};
    const int i = pair_img[2 * p], j = pair_img[2 * p + 1];
    if (!active || !in_range(i, n_img) || !in_range(j, n_img) || i == j) return b;
    b.oa = img_off[i];
    b.ob = img_off[j];
    long long qb = nq[p];
    const long long na = (long long)img_off[i + 1] - b.oa;
    long long nt = (long long)img_off[j + 1] - b.ob;
    if (qb > cap) qb = cap;
    if (qb > na) qb = na;
    if (nt > rev_stride) nt = rev_stride;
    b.qb = qb < 0 ? 0 : (int)qb;
    b.nt = nt < 0 ? 0 : (int)nt;
    return b;
}

// Two lanes a candidate: lane h = lane & 1 is accumulators 4 h .. 4 h + 3 of the oracle's eight and reads 16 bytes of every 32.
// n entries of the wave's queue (n <= kQueue); the keys of the candidates go to q_key, kNoKey for a band pair that is none.
__device__ __forceinline__ void drain_queue(int n, const int* __restrict__ q_lane, const int* __restrict__ q_t, unsigned long long* __restrict__ q_key,
                                            int lane, long long qnode, int q_first, long long ob, const float4* __restrict__ desc,
                                            unsigned long long* __restrict__ rev_p, unsigned long long& k0, unsigned long long& k1) {
    const int h = lane & 1;
    for (int base = 0; base < n; base += 32) {
        const int idx = base + (lane >> 1);
        const bool have = idx < n;
        const int ql = have ? q_lane[idx] : 0, t = have ? q_t[idx] : 0;
        const long long qn = __shfl(qnode, ql, 64);
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        if (have) {
            const float4* __restrict__ x = desc + qn * (kDim / 4) + h;
            const float4* __restrict__ y = desc + (ob + t) * (kDim / 4) + h;
#pragma unroll 4
            for (int k = 0; k < kDim / 8; ++k) {
                const float4 u = x[2 * k], v = y[2 * k];
                const float t0 = u.x - v.x, t1 = u.y - v.y, t2 = u.z - v.z, t3 = u.w - v.w;
                a0 = a0 + t0 * t0;
                a1 = a1 + t1 * t1;
                a2 = a2 + t2 * t2;
                a3 = a3 + t3 * t3;
            }
        }
        // s_l = acc[l] + acc[l + 4]: the partner holds the other half, and a + b is b + a
        const float s0 = a0 + __shfl_xor(a0, 1, 64), s1 = a1 + __shfl_xor(a1, 1, 64);
        const float s2 = a2 + __shfl_xor(a2, 1, 64), s3 = a3 + __shfl_xor(a3, 1, 64);
        const float d = sqrtf(((s0 + s1) + s2) + s3);
        if (have && h == 0) {
            const unsigned bits = __float_as_uint(d);
            const bool cand = d < INFINITY;                      // neither NaN nor +inf; d is never negative
            q_key[idx] = cand ? ((unsigned long long)bits << 32) | (unsigned)t : kNoKey;
            if (cand) atomicMin(rev_p + t, ((unsigned long long)bits << 32) | (unsigned)(q_first + ql));
        }
    }
    wave_lds_sync();
    for (int i = 0; i < n; ++i)
        if (q_lane[i] == lane) insert_key(q_key[i], k0, k1);
    wave_lds_sync();
}

__global__ __launch_bounds__(kBlock) void guided_match_kernel(const float4* __restrict__ desc, const double2* __restrict__ xn, long long n_nodes,
                                                              const double* __restrict__ E, const unsigned char* __restrict__ active,
                                                              const int* __restrict__ pair_img, const int* __restrict__ nq,
                                                              const int* __restrict__ img_off, int n_img, long long cap, float thr2g,
                                                              int* __restrict__ store, unsigned long long* __restrict__ rev, long long rev_stride,
                                                              unsigned blocks_per_pair) {
    __shared__ double4 tile[kBlock];                             // a2, b2, f0 f0, f1 f1
    __shared__ int q_lane[kWaves][kQueue];
    __shared__ int q_t[kWaves][kQueue];
    __shared__ unsigned long long q_key[kWaves][kQueue];
    const long long p = blockIdx.x / blocks_per_pair, q_block = (long long)(blockIdx.x % blocks_per_pair) * kBlock;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long q = q_block + tid;
    PairBand b = pair_band(pair_img, nq, img_off, n_img, cap, rev_stride, p, active[p] != 0);
    if (q_block >= b.qb) b.nt = 0;       // no query of this workgroup is in range: it only fills its rows
    double Em[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Em[k] = E[9 * p + k];
    const long long qnode = (long long)b.oa + q;
    const bool live = q < b.qb && qnode >= 0 && qnode < n_nodes;
    // a lane without a query computes on (e0, e1, e2) = (0, 0, 1): finite words that take the fast path; `live` masks its hits
    double e0 = 0.0, e1 = 0.0, e2 = 1.0;
    if (live) {
        const double2 x1 = xn[qnode];
        e0 = Em[0] * x1.x + Em[1] * x1.y + Em[2] * 1.;
        e1 = Em[3] * x1.x + Em[4] * x1.y + Em[5] * 1.;
        e2 = Em[6] * x1.x + Em[7] * x1.y + Em[8] * 1.;
    }
    const double ee = e0 * e0 + e1 * e1;
    const double T = (double)thr2g;
    const bool fast = thr2g >= FLT_MIN && thr2g <= FLT_MAX;
    const double Tlo = T * kGuardLo, Thi = T * kGuardHi;
    unsigned long long k0 = kNoKey, k1 = kNoKey;
    unsigned long long* __restrict__ rev_p = rev + p * rev_stride;
    const int q_first = (int)q_block + 64 * wave;
    int fill = 0;                                                // entries in this wave's queue (wave-uniform)
    for (int t0 = 0; t0 < b.nt; t0 += kBlock) {
        {
            const long long node = (long long)b.ob + t0 + tid;
            double4 w = {0.0, 0.0, NAN, NAN};                    // a keypoint without a node: a NaN denominator, out of every band
            if (t0 + tid < b.nt && node >= 0 && node < n_nodes) {
                const double2 x2 = xn[node];
                const double f0 = Em[0] * x2.x + Em[3] * x2.y + Em[6] * 1.;
                const double f1 = Em[1] * x2.x + Em[4] * x2.y + Em[7] * 1.;
                w.x = x2.x; w.y = x2.y; w.z = f0 * f0; w.w = f1 * f1;
            }
            tile[tid] = w;
        }
        __syncthreads();
        const int cnt = b.nt - t0 < kBlock ? b.nt - t0 : kBlock;
        for (int k = 0; k < cnt; ++k) {
            const double4 w = tile[k];
            const double s = w.x * e0 + w.y * e1 + 1. * e2;
            const double num = s * s, den = (ee + w.z) + w.w;
            const double lo = Tlo * den, hi = Thi * den;
            const bool sure = fast && lo >= kMinBound && hi <= DBL_MAX && (num <= lo || num >= hi);
            bool in;
            if (sure)
                in = num <= lo;
            else
                in = (float)(num / den) <= thr2g;
            in = in && live;
            const unsigned long long hits = __ballot(in);
            if (hits) {
                if (in) {
                    const int at = fill + __popcll(hits & ((1ull << lane) - 1ull));
                    q_lane[wave][at] = lane;
                    q_t[wave][at] = t0 + k;
                }
                fill += __popcll(hits);
                if (fill >= 64) {
                    wave_lds_sync();
                    drain_queue(fill, q_lane[wave], q_t[wave], q_key[wave], lane, qnode, q_first, b.ob, desc, rev_p, k0, k1);
                    fill = 0;
                }
            }
        }
        __syncthreads();
    }
    if (fill) {
        wave_lds_sync();
        drain_queue(fill, q_lane[wave], q_t[wave], q_key[wave], lane, qnode, q_first, b.ob, desc, rev_p, k0, k1);
    }
    if (q < cap) {
        const unsigned inf_bits = 0x7F800000u;
        int2 idx, dist;
        idx.x = k0 == kNoKey ? -1 : (int)(unsigned)(k0 & 0xFFFFFFFFull);
        idx.y = k1 == kNoKey ? -1 : (int)(unsigned)(k1 & 0xFFFFFFFFull);
        dist.x = (int)(k0 == kNoKey ? inf_bits : (unsigned)(k0 >> 32));
        dist.y = (int)(k1 == kNoKey ? inf_bits : (unsigned)(k1 >> 32));
        int2* __restrict__ out = reinterpret_cast<int2*>(store);
        out[(2 * p + 0) * cap + q] = idx;
        out[(2 * p + 1) * cap + q] = dist;
    }
}

__global__ __launch_bounds__(kBlock) void guided_mutual_kernel(const int2* __restrict__ store, const unsigned long long* __restrict__ rev,
                                                               long long rev_stride, const int* __restrict__ pair_img, const int* __restrict__ nq,
                                                               const int* __restrict__ img_off, int n_img, long long cap,
                                                               unsigned char* __restrict__ keep, int* __restrict__ info) {
    __shared__ int wcnt[kWaves][3];
    const long long p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PairBand b = pair_band(pair_img, nq, img_off, n_img, cap, rev_stride, p, true);
    const int2* __restrict__ idx = store + (2 * p) * cap;
    int c1 = 0, c2 = 0, ck = 0;
    for (long long q = tid; q < cap; q += kBlock) {
        unsigned char k = 0;
        if (q < b.qb) {
            const int2 t = idx[q];
            c1 += t.x >= 0;
            c2 += t.y >= 0;
            if (t.x >= 0 && t.x < rev_stride) k = (unsigned)(rev[p * rev_stride + t.x] & 0xFFFFFFFFull) == (unsigned)q;
            ck += k;
        }
        keep[p * cap + q] = k;
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        c1 += __shfl_xor(c1, d, 64);
        c2 += __shfl_xor(c2, d, 64);
        ck += __shfl_xor(ck, d, 64);
    }
    if (lane == 0) {
        wcnt[wave][0] = c1;
        wcnt[wave][1] = c2;
        wcnt[wave][2] = ck;
    }
    __syncthreads();
    if (tid == 0) {
        int* w = info + 4 * p;
        w[0] = b.qb;
        for (int k = 0; k < 3; ++k) w[1 + k] = wcnt[0][k] + wcnt[1][k] + wcnt[2][k] + wcnt[3][k];
    }
}

bool guided_sizes_ok(int64_t n_pairs, int64_t cap, int64_t rev_stride, int n_img, int64_t n_nodes) {
    return n_pairs >= 0 && cap >= 0 && rev_stride >= 0 && n_pairs <= INT32_MAX && cap <= INT32_MAX && rev_stride <= INT32_MAX &&
           n_pairs * cap <= INT32_MAX && n_pairs * rev_stride <= INT32_MAX && n_img >= 1 && n_img <= kMaxImages && n_nodes >= 0 &&
           n_nodes <= INT32_MAX;
}

}  // namespace

extern "C" size_t sfm_guided_ws_bytes(int64_t n_pairs, int64_t rev_stride) {
    if (n_pairs < 0 || rev_stride < 0 || n_pairs > INT32_MAX || rev_stride > INT32_MAX || n_pairs * rev_stride > INT32_MAX) return 0;
    return (size_t)n_pairs * (size_t)rev_stride * sizeof(uint64_t);
}

extern "C" int sfm_guided_match(const float* desc_dev, const double* xn_dev, int64_t n_nodes, const double* E_dev, const uint8_t* active_dev,
                                const int32_t* pair_img_dev, const int32_t* nq_dev, const int32_t* img_off_dev, int n_img, int64_t n_pairs,
                                int64_t cap, float thr2g, int32_t* store_g_dev, void* ws_dev, size_t ws_bytes, int64_t rev_stride, void* stream_) {
    SFM_CHECK_ARG(guided_sizes_ok(n_pairs, cap, rev_stride, n_img, n_nodes), "sfm_guided_match: bad sizes");
    SFM_CHECK_ARG(thr2g == thr2g, "sfm_guided_match: thr2g is NaN");
    SFM_CHECK_ARG(img_off_dev, "sfm_guided_match: null img_off");
    SFM_CHECK_ARG((reinterpret_cast<uintptr_t>(desc_dev) & 15) == 0, "sfm_guided_match: desc is not 16-byte aligned");
    const size_t need = sfm_guided_ws_bytes(n_pairs, rev_stride);
    SFM_CHECK_ARG(ws_bytes >= need, "sfm_guided_match: the workspace holds %zu bytes, %zu are needed", ws_bytes, need);
    if (n_pairs == 0) return SFM_OK;
    SFM_CHECK_ARG(E_dev && active_dev && pair_img_dev && nq_dev && (cap == 0 || store_g_dev) && (n_nodes == 0 || (xn_dev && desc_dev)) &&
                      (need == 0 || ws_dev),
                  "sfm_guided_match: null pointer");
    hipStream_t stream = sfm::as_stream(stream_);
    if (need) SFM_CHECK_HIP(hipMemsetAsync(ws_dev, 0xFF, need, stream));
    if (cap == 0) return SFM_OK;
    const unsigned blocks_per_pair = (unsigned)((cap + kBlock - 1) / kBlock);       // n_pairs * cap <= 2^31 - 1: the product fits a grid
    hipLaunchKernelGGL(guided_match_kernel, dim3((unsigned)n_pairs * blocks_per_pair), dim3(kBlock), 0, stream,
                       reinterpret_cast<const float4*>(desc_dev), reinterpret_cast<const double2*>(xn_dev), (long long)n_nodes, E_dev, active_dev,
                       pair_img_dev, nq_dev, img_off_dev, n_img, (long long)cap, thr2g, store_g_dev, static_cast<unsigned long long*>(ws_dev),
                       (long long)rev_stride, blocks_per_pair);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" int sfm_guided_mutual(const int32_t* store_g_dev, const void* ws_dev, size_t ws_bytes, int64_t rev_stride, const int32_t* pair_img_dev,
                                 const int32_t* nq_dev, const int32_t* img_off_dev, int n_img, int64_t n_pairs, int64_t cap, uint8_t* keep_g_dev,
                                 int32_t* info_g_dev, void* stream_) {
    SFM_CHECK_ARG(guided_sizes_ok(n_pairs, cap, rev_stride, n_img, 0), "sfm_guided_mutual: bad sizes");
    SFM_CHECK_ARG(img_off_dev, "sfm_guided_mutual: null img_off");
    const size_t need = sfm_guided_ws_bytes(n_pairs, rev_stride);
    SFM_CHECK_ARG(ws_bytes >= need, "sfm_guided_mutual: the workspace holds %zu bytes, %zu are needed", ws_bytes, need);
    if (n_pairs == 0) return SFM_OK;
    SFM_CHECK_ARG(pair_img_dev && nq_dev && info_g_dev && (cap == 0 || (store_g_dev && keep_g_dev)) && (need == 0 || ws_dev),
                  "sfm_guided_mutual: null pointer");
    hipLaunchKernelGGL(guided_mutual_kernel, dim3((unsigned)n_pairs), dim3(kBlock), 0, sfm::as_stream(stream_),
                       reinterpret_cast<const int2*>(store_g_dev), static_cast<const unsigned long long*>(ws_dev), (long long)rev_stride,
                       pair_img_dev, nq_dev, img_off_dev, n_img, (long long)cap, keep_g_dev, info_g_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}
