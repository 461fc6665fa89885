// Image retrieval (include/sfm_hip.h, "RETRIEVAL"; docs/retrieval.md): VLAD signatures of the images on the device and the shortlist of
// pairs that replaces all_pairs for unordered collections.
//   sfm_vlad_accumulate   vlad_assign_kernel: a lane owns a node with its descriptor in registers, the centres pass through LDS 32 at a
//                         time and are read as broadcasts; the smallest key (bits(d2) << 32) | c is the assignment.
//                         vlad_accumulate_kernel: a workgroup owns 1 024 consecutive nodes and cuts them at the image boundaries; the
//                         nodes of a segment are counting-sorted by centre in LDS, eight groups of 32 lanes walk the sorted list, a lane
//                         sums four dimensions in int64 registers while the centre stays and adds them to acc with one 64-bit integer
//                         atomic per (segment, centre, dimension) and lane group whose share of the list holds that centre: at most eight.
//   sfm_vlad_centres      a lane per (centre, dimension)
//   sfm_vlad_signature    a workgroup of 128 lanes per (image, centre); every lane sums the 128 squares left to right
//   sfm_vlad_shortlist    vlad_sim_kernel: S = sig sig^T on v_mfma_i32_16x16x64_i8, a wave per 32 x 32 tile, fragments straight from
//                         global memory (the signatures are a few megabytes and stay in L2); the tile is written as ordering keys.
//                         vlad_topk_kernel: a wave per image, k rounds of "smallest key above the last one".
//   sfm_vlad_pairs        an adjacency bitmap (atomicOr is idempotent), a count per row, one scan, an ordered emit
// Nothing depends on the order in which lanes or workgroups run: acc, count and norm2 are integer sums, the neighbours are minima of
// distinct integer keys, the pair list is a rank.  The library is built with -ffp-contract=off: no FMA is formed.
// image_of and the wave scan are copies of what tracks.hip and the mesh files keep for themselves.
#include <cfloat>
#include <climits>
#include <cmath>

#include "common.h"

namespace {

constexpr int kDim = 128;
constexpr int kRow4 = kDim / 4;                 // float4 words of a descriptor
constexpr int kMaxCentres = 256;
constexpr int kMaxImages = 65536;
constexpr int kMaxShortlist = 16384;
constexpr int kMaxK = 64;
constexpr int kBlock = 256;
constexpr int kCentreTile = 32;                 // centres in LDS at a time: 16 kB, so C = 256 costs eight tiles and no occupancy
constexpr int kChunk = 1024;                    // nodes of an accumulate workgroup (10 bits of an `order` word)
constexpr int kGroups = kBlock / kRow4;         // 8 groups of 32 lanes, a lane per float4 of the row
constexpr unsigned long long kNoKey = ~0ull;
constexpr unsigned kNoSim = 0xFFFFFFFFu;

typedef int i32x4 __attribute__((ext_vector_type(4)));

// The image of node u: the largest i < n_img with img_off[i] <= u (0 when there is none); at most 17 steps.
__device__ inline int image_of(const int* __restrict__ img_off, int n_img, long long u) {
    int lo = 0, hi = n_img - 1;
    for (int it = 0; it < 17 && lo < hi; ++it) {
        const int mid = (lo + hi + 1) >> 1;
        if ((long long)img_off[mid] <= u) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ int wave_inclusive_scan(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

__device__ __forceinline__ long long vlad_term(float r, float scale) {
    return (long long)rintf(fminf(fmaxf(r * scale, -0x1p30f), 0x1p30f));
}

// ---- accumulate ----------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock) void vlad_assign_kernel(const float4* __restrict__ desc, const float4* __restrict__ centres, long long n_nodes,
                                                             int C, int* __restrict__ assign) {
    __shared__ float4 tile[kCentreTile * kRow4];
    const int tid = threadIdx.x;
    const long long u = (long long)blockIdx.x * kBlock + tid;
    const bool live = u < n_nodes;
    float4 x[kRow4];
#pragma unroll
    for (int m = 0; m < kRow4; ++m) x[m] = live ? desc[u * kRow4 + m] : make_float4(0.f, 0.f, 0.f, 0.f);
    unsigned long long best = kNoKey;
    for (int c0 = 0; c0 < C; c0 += kCentreTile) {
        const int cnt = C - c0 < kCentreTile ? C - c0 : kCentreTile;
        __syncthreads();                                         // the previous tile has been read
        for (int e = tid; e < cnt * kRow4; e += kBlock) tile[e] = centres[(long long)c0 * kRow4 + e];
        __syncthreads();
        for (int c = 0; c < cnt; ++c) {
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f, a5 = 0.f, a6 = 0.f, a7 = 0.f;
#pragma unroll
            for (int k = 0; k < kDim / 8; ++k) {
                const float4 v = tile[c * kRow4 + 2 * k], w = tile[c * kRow4 + 2 * k + 1];
                const float t0 = x[2 * k].x - v.x, t1 = x[2 * k].y - v.y, t2 = x[2 * k].z - v.z, t3 = x[2 * k].w - v.w;
                const float t4 = x[2 * k + 1].x - w.x, t5 = x[2 * k + 1].y - w.y, t6 = x[2 * k + 1].z - w.z, t7 = x[2 * k + 1].w - w.w;
                a0 = a0 + t0 * t0; a1 = a1 + t1 * t1; a2 = a2 + t2 * t2; a3 = a3 + t3 * t3;
                a4 = a4 + t4 * t4; a5 = a5 + t5 * t5; a6 = a6 + t6 * t6; a7 = a7 + t7 * t7;
            }
            const float s0 = a0 + a4, s1 = a1 + a5, s2 = a2 + a6, s3 = a3 + a7;
            const float d2 = ((s0 + s1) + s2) + s3;
            if (d2 < INFINITY) {                                 // neither NaN nor +inf; d2 is never negative
                const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)(c0 + c);
                best = key < best ? key : best;
            }
        }
    }
    if (live) assign[u] = best == kNoKey ? -1 : (int)(unsigned)(best & 0xFFFFFFFFull);
}

__global__ __launch_bounds__(kBlock) void vlad_accumulate_kernel(const float4* __restrict__ desc, const float4* __restrict__ centres,
                                                                 const int* __restrict__ assign, const int* __restrict__ img_off, int n_img,
                                                                 long long n_nodes, int C, float scale, unsigned long long* __restrict__ acc,
                                                                 int* __restrict__ count) {
    __shared__ int cnt[kMaxCentres];
    __shared__ int cursor[kMaxCentres];
    __shared__ int order[kChunk];                                // (centre << 10) | offset in the chunk, sorted by centre
    __shared__ int total;
    const int tid = threadIdx.x, lane = tid & 63;
    const long long n0 = (long long)blockIdx.x * kChunk;
    const long long n1 = n0 + kChunk < n_nodes ? n0 + kChunk : n_nodes;
    long long lo = n0;
    for (int seg = 0; seg < kChunk && lo < n1; ++seg) {          // a segment holds at least one node
        const int i = image_of(img_off, n_img, lo);
        long long hi = i + 1 < n_img ? (long long)img_off[i + 1] : n1;
        if (hi > n1 || hi <= lo) hi = n1;                        // (hi <= lo: offsets that do not ascend; the rest goes to image i)
        const int m = (int)(hi - lo), base = (int)(lo - n0);
        cnt[tid] = 0;
        __syncthreads();
        for (int e = tid; e < m; e += kBlock) {
            const int a = assign[lo + e];
            if ((unsigned)a < (unsigned)C) atomicAdd(&cnt[a], 1);
        }
        __syncthreads();
        if (tid < 64) {                                          // exclusive scan of the 256 counts: four a lane
            const int c0 = cnt[4 * lane], c1 = cnt[4 * lane + 1], c2 = cnt[4 * lane + 2], c3 = cnt[4 * lane + 3];
            const int incl = wave_inclusive_scan(c0 + c1 + c2 + c3, lane);
            const int ex = incl - (c0 + c1 + c2 + c3);
            cursor[4 * lane] = ex;
            cursor[4 * lane + 1] = ex + c0;
            cursor[4 * lane + 2] = ex + c0 + c1;
            cursor[4 * lane + 3] = ex + c0 + c1 + c2;
            if (lane == 63) total = incl;
        }
        if (tid < C && cnt[tid]) atomicAdd(&count[(long long)i * C + tid], cnt[tid]);
        __syncthreads();
        for (int e = tid; e < m; e += kBlock) {
            const int a = assign[lo + e];
            if ((unsigned)a < (unsigned)C) order[atomicAdd(&cursor[a], 1)] = (a << 10) | (base + e);
        }
        __syncthreads();
        {
            const int M = total, g = tid / kRow4, kq = tid % kRow4;
            const int p0 = (int)((long long)M * g / kGroups), p1 = (int)((long long)M * (g + 1) / kGroups);
            long long s0 = 0, s1 = 0, s2 = 0, s3 = 0;
            int cur = -1;
            float4 cen = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int p = p0; p <= p1; ++p) {
                const int w = p < p1 ? order[p] : -1;            // the last turn only flushes
                const int c = w < 0 ? -1 : w >> 10;
                if (c != cur && cur >= 0) {
                    unsigned long long* __restrict__ out = acc + (((long long)i * C + cur) * kDim + 4 * kq);
                    if (s0) atomicAdd(out + 0, (unsigned long long)s0);
                    if (s1) atomicAdd(out + 1, (unsigned long long)s1);
                    if (s2) atomicAdd(out + 2, (unsigned long long)s2);
                    if (s3) atomicAdd(out + 3, (unsigned long long)s3);
                }
                if (w < 0) break;
                if (c != cur) {
                    cur = c;
                    cen = centres[(long long)c * kRow4 + kq];
                    s0 = s1 = s2 = s3 = 0;
                }
                const float4 x = desc[(n0 + (w & (kChunk - 1))) * kRow4 + kq];
                s0 += vlad_term(x.x - cen.x, scale);
                s1 += vlad_term(x.y - cen.y, scale);
                s2 += vlad_term(x.z - cen.z, scale);
                s3 += vlad_term(x.w - cen.w, scale);
            }
        }
        __syncthreads();                                         // order, cnt and total are rewritten by the next segment
        lo = hi;
    }
}

// ---- centres -------------------------------------------------------------------------------------------------------------------------

// centres and out may be the same buffer (the header allows an update in place): neither is __restrict__
__global__ __launch_bounds__(kBlock) void vlad_centres_kernel(const float* centres, const long long* __restrict__ acc,
                                                              const int* __restrict__ count, int C, float scale, float* out) {
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    if (idx >= C * kDim) return;
    const int n = count[idx / kDim];
    const float old = centres[idx];
    out[idx] = n != 0 ? (float)((double)old + (double)acc[idx] / ((double)n * (double)scale)) : old;
}

// ---- signature -----------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kDim) void vlad_signature_kernel(const long long* __restrict__ acc, int C, int ssr, double qs,
                                                              signed char* __restrict__ sig, int* __restrict__ norm2) {
    __shared__ double sq[kDim];
    __shared__ int wsum[2];
    const long long b = blockIdx.x;
    const int k = threadIdx.x;
    double a = (double)acc[b * kDim + k];
    if (ssr) a = copysign(sqrt(fabs(a)), a);
    sq[k] = a * a;
    __syncthreads();
    double n2 = 0.0;
    for (int j = 0; j < kDim; ++j) n2 = n2 + sq[j];
    int q = 0;
    if (n2 != 0.0 && n2 < (double)INFINITY) q = (int)fmin(fmax(rint(a / sqrt(n2) * qs), -127.0), 127.0);
    sig[b * kDim + k] = (signed char)q;
    int s = q * q;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) s += __shfl_xor(s, d, 64);
    if ((k & 63) == 0) wsum[k >> 6] = s;
    __syncthreads();
    if (k == 0 && wsum[0] + wsum[1]) atomicAdd(&norm2[b / C], wsum[0] + wsum[1]);
}

// ---- shortlist -----------------------------------------------------------------------------------------------------------------------

// float32 bits -> a uint32 that ascends with the value, and back
__device__ __forceinline__ unsigned ordered_of(unsigned u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ unsigned bits_of_ordered(unsigned o) { return (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o; }

// A workgroup is four waves, a wave a 32 x 32 tile of S as 2 x 2 MFMA tiles of 16 x 16.  Lane l holds bytes 16 (l >> 4) .. + 15 of
// row l & 15 of a 64-byte step for both operands, so the k order inside the instruction cancels; D[row 4 (l >> 4) + r][col l & 15].
// The workspace word of (i, j) is ~ordered(sim) for a candidate (ascending keys = descending sim) and kNoSim for everything else.
__global__ __launch_bounds__(kBlock) void vlad_sim_kernel(const signed char* __restrict__ sig, const int* __restrict__ norm2, int n, int D,
                                                          float min_sim, unsigned* __restrict__ ws) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = blockIdx.y * 64 + (wave >> 1) * 32, j0 = blockIdx.x * 64 + (wave & 1) * 32;
    if (i0 >= n || j0 >= n) return;                              // wave-uniform; the kernel has no barrier
    const signed char* pa[2];
    const signed char* pb[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int ra = i0 + 16 * t + (lane & 15), rb = j0 + 16 * t + (lane & 15);
        pa[t] = sig + (long long)(ra < n ? ra : n - 1) * D + 16 * (lane >> 4);
        pb[t] = sig + (long long)(rb < n ? rb : n - 1) * D + 16 * (lane >> 4);
    }
    i32x4 acc[2][2];
#pragma unroll
    for (int ta = 0; ta < 2; ++ta)
#pragma unroll
        for (int tb = 0; tb < 2; ++tb) acc[ta][tb] = (i32x4){0, 0, 0, 0};
    for (int k0 = 0; k0 < D; k0 += 64) {
        i32x4 a[2], b[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            a[t] = *reinterpret_cast<const i32x4*>(pa[t] + k0);
            b[t] = *reinterpret_cast<const i32x4*>(pb[t] + k0);
        }
#pragma unroll
        for (int ta = 0; ta < 2; ++ta)
#pragma unroll
            for (int tb = 0; tb < 2; ++tb) acc[ta][tb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[ta], b[tb], acc[ta][tb], 0, 0, 0);
    }
#pragma unroll
    for (int ta = 0; ta < 2; ++ta)
#pragma unroll
        for (int tb = 0; tb < 2; ++tb) {
            const int col = j0 + 16 * tb + (lane & 15);
            const int nc = col < n ? norm2[col] : 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = i0 + 16 * ta + 4 * (lane >> 4) + r;
                if (row >= n || col >= n) continue;
                const int nr = norm2[row];
                unsigned word = kNoSim;
                if (row != col && nr != 0 && nc != 0) {
                    const float sim = (float)((double)acc[ta][tb][r] / sqrt((double)nr * (double)nc));
                    if (sim >= min_sim) word = ~ordered_of(__float_as_uint(sim));
                }
                ws[(long long)row * n + col] = word;
            }
        }
}

__global__ __launch_bounds__(64) void vlad_topk_kernel(const unsigned* __restrict__ ws, int n, int k, int* __restrict__ nbr,
                                                       float* __restrict__ nbr_sim) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const unsigned* __restrict__ row = ws + (long long)i * n;
    unsigned long long floor_key = 0;                            // the smallest key still admitted
    int s = 0;
    for (; s < k; ++s) {
        unsigned long long best = kNoKey;
        for (int j = lane; j < n; j += 64) {
            const unsigned w = row[j];
            const unsigned long long key = ((unsigned long long)w << 32) | (unsigned)j;
            if (w != kNoSim && key >= floor_key && key < best) best = key;
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long o = __shfl_xor(best, d, 64);
            best = o < best ? o : best;
        }
        if (best == kNoKey) break;
        if (lane == 0) {
            nbr[(long long)i * k + s] = (int)(unsigned)(best & 0xFFFFFFFFull);
            nbr_sim[(long long)i * k + s] = __uint_as_float(bits_of_ordered(~(unsigned)(best >> 32)));
        }
        floor_key = best + 1;
    }
    for (int t = s + lane; t < k; t += 64) {
        nbr[(long long)i * k + t] = -1;
        nbr_sim[(long long)i * k + t] = -INFINITY;
    }
}

// ---- pairs ---------------------------------------------------------------------------------------------------------------------------

__device__ inline bool names(const int* __restrict__ nbr, int k, int row, int who) {
    bool hit = false;
    for (int s = 0; s < k; ++s) hit = hit || nbr[(long long)row * k + s] == who;
    return hit;
}

__global__ __launch_bounds__(kBlock) void vlad_pairs_mark_kernel(const int* __restrict__ nbr, int n, int k, int mutual, int W,
                                                                 unsigned* __restrict__ bits) {
    const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (e >= (long long)n * k) return;
    const int i = (int)(e / k), j = nbr[e];
    if ((unsigned)j >= (unsigned)n || j == i) return;
    if (mutual && !names(nbr, k, j, i)) return;
    const int a = i < j ? i : j, b = i < j ? j : i;
    atomicOr(&bits[(long long)a * W + (b >> 5)], 1u << (b & 31));
}

__global__ __launch_bounds__(64) void vlad_pairs_count_kernel(const unsigned* __restrict__ bits, int W, int* __restrict__ rows) {
    const int a = blockIdx.x, lane = threadIdx.x;
    int s = 0;
    for (int w = lane; w < W; w += 64) s += __popc(bits[(long long)a * W + w]);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) s += __shfl_xor(s, d, 64);
    if (lane == 0) rows[a] = s;
}

// One workgroup: rows[a] becomes the number of pairs in front of row a; count = (selected, written).
__global__ __launch_bounds__(kBlock) void vlad_pairs_scan_kernel(int* __restrict__ rows, int n, long long cap, int* __restrict__ count) {
    __shared__ int part[kBlock];
    const int tid = threadIdx.x, per = (n + kBlock - 1) / kBlock;        // <= 64
    const int a0 = tid * per, a1 = a0 + per < n ? a0 + per : n;
    int s = 0;
    for (int a = a0; a < a1; ++a) s += rows[a];
    part[tid] = s;
    __syncthreads();
    int before = 0;
    for (int t = 0; t < tid; ++t) before += part[t];
    for (int a = a0; a < a1; ++a) {
        const int c = rows[a];
        rows[a] = before;
        before += c;
    }
    if (tid == kBlock - 1) {
        count[0] = before;
        count[1] = (long long)before < cap ? before : (int)cap;
    }
}

__global__ __launch_bounds__(64) void vlad_pairs_emit_kernel(const unsigned* __restrict__ bits, const int* __restrict__ rows, int W, long long cap,
                                                             int2* __restrict__ pairs) {
    const int a = blockIdx.x, lane = threadIdx.x;
    long long pos = rows[a];
    for (int w0 = 0; w0 < W; w0 += 64) {
        unsigned word = w0 + lane < W ? bits[(long long)a * W + w0 + lane] : 0u;
        const int pc = __popc(word), incl = wave_inclusive_scan(pc, lane);
        long long at = pos + incl - pc;
        for (int t = 0; t < 32 && word; ++t) {
            const int bit = __ffs(word) - 1;
            word &= word - 1;
            if (at < cap) pairs[at] = make_int2(a, 32 * (w0 + lane) + bit);
            ++at;
        }
        pos += __shfl(incl, 63, 64);
    }
}

bool finite_positive(double v) { return v > 0.0 && v < (double)INFINITY; }

}  // namespace

extern "C" int sfm_vlad_accumulate(const float* desc_dev, int64_t n_nodes, const float* centres_dev, int n_centres, const int32_t* img_off_dev,
                                   int n_img, float scale, int32_t* assign_dev, int64_t* acc_dev, int32_t* count_dev, void* stream_) {
    SFM_CHECK_ARG(n_nodes >= 0 && n_nodes <= INT32_MAX, "sfm_vlad_accumulate: n_nodes must be 0..2^31-1");
    SFM_CHECK_ARG(n_centres >= 1 && n_centres <= kMaxCentres, "sfm_vlad_accumulate: n_centres must be 1..256 (got %d)", n_centres);
    SFM_CHECK_ARG(n_img >= 1 && n_img <= kMaxImages, "sfm_vlad_accumulate: n_img must be 1..65536 (got %d)", n_img);
    SFM_CHECK_ARG(finite_positive(scale), "sfm_vlad_accumulate: scale must be positive and finite");
    SFM_CHECK_ARG((reinterpret_cast<uintptr_t>(desc_dev) & 15) == 0 && (reinterpret_cast<uintptr_t>(centres_dev) & 15) == 0,
                  "sfm_vlad_accumulate: desc and centres must be 16-byte aligned");
    SFM_CHECK_ARG(centres_dev && img_off_dev && acc_dev && count_dev && (n_nodes == 0 || (desc_dev && assign_dev)),
                  "sfm_vlad_accumulate: null pointer");
    hipStream_t stream = sfm::as_stream(stream_);
    const size_t cells = (size_t)n_img * (size_t)n_centres;
    SFM_CHECK_HIP(hipMemsetAsync(acc_dev, 0, cells * kDim * sizeof(int64_t), stream));
    SFM_CHECK_HIP(hipMemsetAsync(count_dev, 0, cells * sizeof(int32_t), stream));
    if (n_nodes == 0) return SFM_OK;
    hipLaunchKernelGGL(vlad_assign_kernel, dim3((unsigned)((n_nodes + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream,
                       reinterpret_cast<const float4*>(desc_dev), reinterpret_cast<const float4*>(centres_dev), (long long)n_nodes, n_centres,
                       assign_dev);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(vlad_accumulate_kernel, dim3((unsigned)((n_nodes + kChunk - 1) / kChunk)), dim3(kBlock), 0, stream,
                       reinterpret_cast<const float4*>(desc_dev), reinterpret_cast<const float4*>(centres_dev), assign_dev, img_off_dev, n_img,
                       (long long)n_nodes, n_centres, scale, reinterpret_cast<unsigned long long*>(acc_dev), count_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" int sfm_vlad_centres(const float* centres_dev, const int64_t* acc_dev, const int32_t* count_dev, int n_centres, float scale,
                                float* centres_out_dev, void* stream_) {
    SFM_CHECK_ARG(n_centres >= 1 && n_centres <= kMaxCentres, "sfm_vlad_centres: n_centres must be 1..256 (got %d)", n_centres);
    SFM_CHECK_ARG(finite_positive(scale), "sfm_vlad_centres: scale must be positive and finite");
    SFM_CHECK_ARG(centres_dev && acc_dev && count_dev && centres_out_dev, "sfm_vlad_centres: null pointer");
    hipLaunchKernelGGL(vlad_centres_kernel, dim3((unsigned)((n_centres * kDim + kBlock - 1) / kBlock)), dim3(kBlock), 0, sfm::as_stream(stream_),
                       centres_dev, reinterpret_cast<const long long*>(acc_dev), count_dev, n_centres, scale, centres_out_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" int sfm_vlad_signature(const int64_t* acc_dev, int n_img, int n_centres, int ssr, double qs, int8_t* sig_dev, int32_t* norm2_dev,
                                  void* stream_) {
    SFM_CHECK_ARG(n_img >= 1 && n_img <= kMaxImages, "sfm_vlad_signature: n_img must be 1..65536 (got %d)", n_img);
    SFM_CHECK_ARG(n_centres >= 1 && n_centres <= kMaxCentres, "sfm_vlad_signature: n_centres must be 1..256 (got %d)", n_centres);
    SFM_CHECK_ARG(finite_positive(qs), "sfm_vlad_signature: qs must be positive and finite");
    SFM_CHECK_ARG(acc_dev && sig_dev && norm2_dev, "sfm_vlad_signature: null pointer");
    hipStream_t stream = sfm::as_stream(stream_);
    SFM_CHECK_HIP(hipMemsetAsync(norm2_dev, 0, (size_t)n_img * sizeof(int32_t), stream));
    hipLaunchKernelGGL(vlad_signature_kernel, dim3((unsigned)n_img * (unsigned)n_centres), dim3(kDim), 0, stream,
                       reinterpret_cast<const long long*>(acc_dev), n_centres, ssr, qs, reinterpret_cast<signed char*>(sig_dev), norm2_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" size_t sfm_vlad_shortlist_ws_bytes(int n_img) {
    if (n_img < 1 || n_img > kMaxShortlist) return 0;
    return (size_t)n_img * (size_t)n_img * sizeof(uint32_t);
}

extern "C" int sfm_vlad_shortlist(const int8_t* sig_dev, const int32_t* norm2_dev, int n_img, int n_centres, int k, float min_sim,
                                  int32_t* nbr_dev, float* nbr_sim_dev, void* ws_dev, size_t ws_bytes, void* stream_) {
    SFM_CHECK_ARG(n_img >= 1 && n_img <= kMaxShortlist, "sfm_vlad_shortlist: n_img must be 1..16384 (got %d)", n_img);
    SFM_CHECK_ARG(n_centres >= 1 && n_centres <= kMaxCentres, "sfm_vlad_shortlist: n_centres must be 1..256 (got %d)", n_centres);
    SFM_CHECK_ARG(k >= 1 && k <= kMaxK, "sfm_vlad_shortlist: k must be 1..64 (got %d)", k);
    SFM_CHECK_ARG(min_sim == min_sim, "sfm_vlad_shortlist: min_sim is NaN");
    const size_t need = sfm_vlad_shortlist_ws_bytes(n_img);
    SFM_CHECK_ARG(ws_bytes >= need, "sfm_vlad_shortlist: the workspace holds %zu bytes, %zu are needed", ws_bytes, need);
    SFM_CHECK_ARG((reinterpret_cast<uintptr_t>(sig_dev) & 15) == 0, "sfm_vlad_shortlist: sig is not 16-byte aligned");
    SFM_CHECK_ARG(sig_dev && norm2_dev && nbr_dev && nbr_sim_dev && ws_dev, "sfm_vlad_shortlist: null pointer");
    hipStream_t stream = sfm::as_stream(stream_);
    const unsigned tiles = (unsigned)((n_img + 63) / 64);
    hipLaunchKernelGGL(vlad_sim_kernel, dim3(tiles, tiles), dim3(kBlock), 0, stream, reinterpret_cast<const signed char*>(sig_dev), norm2_dev,
                       n_img, n_centres * kDim, min_sim, static_cast<unsigned*>(ws_dev));
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(vlad_topk_kernel, dim3((unsigned)n_img), dim3(64), 0, stream, static_cast<const unsigned*>(ws_dev), n_img, k, nbr_dev,
                       nbr_sim_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" size_t sfm_vlad_pairs_ws_bytes(int n_img) {
    if (n_img < 1 || n_img > kMaxShortlist) return 0;
    const size_t W = ((size_t)n_img + 31) / 32;
    return sfm::align_up((size_t)n_img * W * sizeof(uint32_t), 256) + sfm::align_up((size_t)n_img * sizeof(int32_t), 256);
}

extern "C" int sfm_vlad_pairs(const int32_t* nbr_dev, int n_img, int k, int mutual, int32_t* pairs_out_dev, int64_t cap_pairs, int32_t* count_dev,
                              void* ws_dev, size_t ws_bytes, void* stream_) {
    SFM_CHECK_ARG(n_img >= 1 && n_img <= kMaxShortlist, "sfm_vlad_pairs: n_img must be 1..16384 (got %d)", n_img);
    SFM_CHECK_ARG(k >= 1 && k <= kMaxK, "sfm_vlad_pairs: k must be 1..64 (got %d)", k);
    SFM_CHECK_ARG(cap_pairs >= 0 && cap_pairs <= INT32_MAX, "sfm_vlad_pairs: cap_pairs must be 0..2^31-1");
    const size_t need = sfm_vlad_pairs_ws_bytes(n_img);
    SFM_CHECK_ARG(ws_bytes >= need, "sfm_vlad_pairs: the workspace holds %zu bytes, %zu are needed", ws_bytes, need);
    SFM_CHECK_ARG(nbr_dev && count_dev && ws_dev && (cap_pairs == 0 || pairs_out_dev), "sfm_vlad_pairs: null pointer");
    hipStream_t stream = sfm::as_stream(stream_);
    const int W = (n_img + 31) / 32;
    const size_t bitmap = sfm::align_up((size_t)n_img * W * sizeof(uint32_t), 256);
    unsigned* bits = static_cast<unsigned*>(ws_dev);
    int* rows = reinterpret_cast<int*>(static_cast<char*>(ws_dev) + bitmap);
    SFM_CHECK_HIP(hipMemsetAsync(bits, 0, bitmap, stream));
    hipLaunchKernelGGL(vlad_pairs_mark_kernel, dim3((unsigned)(((long long)n_img * k + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, nbr_dev,
                       n_img, k, mutual, W, bits);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(vlad_pairs_count_kernel, dim3((unsigned)n_img), dim3(64), 0, stream, bits, W, rows);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(vlad_pairs_scan_kernel, dim3(1), dim3(kBlock), 0, stream, rows, n_img, (long long)cap_pairs, count_dev);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(vlad_pairs_emit_kernel, dim3((unsigned)n_img), dim3(64), 0, stream, bits, rows, W, (long long)cap_pairs,
                       reinterpret_cast<int2*>(pairs_out_dev));
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}
