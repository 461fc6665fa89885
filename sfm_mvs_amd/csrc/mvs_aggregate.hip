// Shiftable windows and semi-global aggregation of the plane sweep's cost volume (include/sfm_hip.h, "MVS-AGGREGATE";
// docs/mvs.md §7): the opt-in stage between sfm_mvs_plane_sweep and sfm_mvs_consistency.
//   sfm_mvs_cost_shift      float32 volume -> uint16 Q: quantise at 1/1024, spatial min filter per plane
//   sfm_mvs_cost_aggregate  Q -> uint16 S: Hirschmueller's path costs L_r summed over 4 or 8 directions
//   sfm_mvs_cost_depth      S, Q -> depth / cost / plane: winner-take-all on S, the sweep's sub-plane parabola
// Everything after the quantisation is integer arithmetic: exact, and free of any summation order, so the directions may run
// in any order and tests/np_mvs_aggregate.py restates every output bit for bit.
//
// path_kernel, the one with a dependent chain.  A workgroup owns PX adjacent lines (rows for the horizontal directions,
// columns — slid by dx per row, wrapping round the frame — for the other six) and walks them step by step; a thread owns one
// (line, plane) pair, PX * ndepth_pad2 = blockDim, so that the planes of a pixel are spread over lanes.  The previous step's
// L_r lives in LDS (double-buffered, a pad row above and below stands for the absent j-1 / j+1 terms); min_k L_r is a
// reduction over the wave's lanes of equal line (xor-shuffles across the rows of 16, DPP within them) followed by one LDS
// atomic min per wave and line (triple-buffered, so that a step costs ONE barrier, and that one waits for LDS only).
// Global traffic is kept off that chain: Q (and S, read-modify-write by the one thread that owns the element) moves in
// chunks of 8 steps held in registers, the next chunk loaded while the current one is walked.  For the horizontal directions
// a chunk is 8 consecutive pixels of a row, so that their accesses stay within a cache line.  Each direction is one launch;
// the first one writes S, the others add to it.  Every loop is bounded by w, h, ndepth.
#include "common.h"

namespace {

constexpr int kMaxShift = 4;
constexpr int kTileW = 64, kTileH = 32;                                  // cost_shift: pixels per workgroup (256 lanes, 8 pixels each)
constexpr int kHaloW = kTileW + 2 * kMaxShift, kHaloH = kTileH + 2 * kMaxShift;
constexpr int kQMax = 2048;
constexpr int kAbsent = 0xFFFF;                                          // a tap outside the frame: above every q

__device__ inline int quantise(float c) {
    if (!(c < 2.0f)) return kQMax;                                       // NaN, +inf, >= 2
    if (c > 0.0f) return (int)floorf(c * 1024.0f + 0.5f);
    return 0;
}

__global__ __launch_bounds__(256) void cost_shift_kernel(const float* __restrict__ vol, int w, int h, int shift, uint16_t* __restrict__ q_out) {
    __shared__ int sA[kHaloH * kHaloW];                                  // q of tile + halo
    __shared__ int sB[kHaloH * kTileW];                                  // row minima: halo rows x tile columns
    const int bx = blockIdx.x * kTileW, by = blockIdx.y * kTileH;
    const size_t plane = (size_t)blockIdx.z * ((size_t)w * h);
    const int side_w = kTileW + 2 * shift, side_h = kTileH + 2 * shift;
    for (int i = threadIdx.x; i < side_w * side_h; i += 256) {
        const int hy = i / side_w, hx = i - hy * side_w;
        const int gx = bx - shift + hx, gy = by - shift + hy;
        sA[hy * kHaloW + hx] = (gx >= 0 && gx < w && gy >= 0 && gy < h) ? quantise(vol[plane + (size_t)gy * w + gx]) : kAbsent;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < side_h * kTileW; i += 256) {
        const int hy = i / kTileW, c = i - hy * kTileW;
        const int* row = sA + hy * kHaloW + c;
        int m = row[0];
        for (int dx = 1; dx <= 2 * shift; ++dx) m = min(m, row[dx]);
        sB[i] = m;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kTileH * kTileW; i += 256) {
        const int ty = i / kTileW, tx = i - ty * kTileW;
        const int x = bx + tx, y = by + ty;
        if (x >= w || y >= h) continue;
        int m = sB[ty * kTileW + tx];
        for (int dy = 1; dy <= 2 * shift; ++dy) m = min(m, sB[(ty + dy) * kTileW + tx]);
        q_out[plane + (size_t)y * w + x] = (uint16_t)m;
    }
}

#ifndef SFM_AGG_CHUNK
#define SFM_AGG_CHUNK 8
#endif
constexpr int kChunk = SFM_AGG_CHUNK;           // steps per register chunk of Q / S
constexpr int kBig = 1 << 20;                   // above every L_r (<= 65535 + 2048), small enough to add p2 to
constexpr int kMaxThreads = 1024;               // = the largest ndepth, padded to a power of two
#ifndef SFM_AGG_THREADS
#define SFM_AGG_THREADS 512                     // (a compile-time knob for A/B builds: 256, 512 or 1024; docs/mvs.md §7)
#endif
constexpr int kTargetThreads = SFM_AGG_THREADS; // workgroup size while ndepth_pad2 <= this
constexpr int kLdsL = 2 * kMaxThreads;          // (ndepth_pad2 + 2) * PX <= 1024 + 2*512
constexpr int kLdsM = kMaxThreads / 2;          // PX <= 512 (ndepth >= 2)

// The barrier of a step orders LDS traffic only: no thread reads a global element that another thread of the launch writes
// (Q is read-only, every element of S belongs to one thread), so the chunk loads in flight need not be waited for here, as
// __syncthreads() would (its fence covers global memory: s_waitcnt vmcnt(0) in front of every s_barrier).
__device__ inline void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// min over the lanes of a row of 16 that differ from this one by a multiple of `px` (1, 2, 4 or 8), by DPP: rotations by 8 and 4
// within the row, then the quad permutations [2,3,0,1] and [1,0,3,2]
__device__ inline int row_min(int v, int px) {
    if (px <= 8) v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x128, 0xF, 0xF, false));
    if (px <= 4) v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x124, 0xF, 0xF, false));
    if (px <= 2) v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false));
    if (px <= 1) v = min(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false));
    return v;
}

// One direction.  horiz: lines are rows, steps run along x (dy = 0).  Otherwise lines are the columns at the first row, steps
// run along y and line k sits at x = (k + dx*t) mod w in step t: where it wraps, the predecessor lies outside the frame and the
// path restarts, so that one wrapped line carries several true paths one after the other.
template <bool kFirst>
__global__ __launch_bounds__(kMaxThreads) void path_kernel(const uint16_t* __restrict__ Q, uint16_t* __restrict__ S, int w, int h, int nd,
                                                            int px_log2, int horiz, int dx, int dy, int p1, int p2) {
    __shared__ int sL[2][kLdsL];
    __shared__ int sM[3][kLdsM];
    const int tid = threadIdx.x, PX = 1 << px_log2;
    const int p = tid & (PX - 1), j = tid >> px_log2;
    const int nsteps = horiz ? w : h, nlines = horiz ? h : w;
    const int k = (int)blockIdx.x * PX + p;
    const bool live = k < nlines && j < nd;
    for (int i = tid; i < 2 * kLdsL; i += blockDim.x) (&sL[0][0])[i] = kBig;
    for (int i = tid; i < 3 * kLdsM; i += blockDim.x) (&sM[0][0])[i] = kBig;
    __syncthreads();

    const size_t base = (size_t)(live ? j : 0) * ((size_t)w * h);
    // the cursor of the loads runs a chunk ahead of the cursor of the stores
    int lx = horiz ? (dx > 0 ? 0 : w - 1) : k, ly = horiz ? k : (dy > 0 ? 0 : h - 1);
    int sx = lx, sy = ly;
    const int x_restart = dx > 0 ? 0 : (dx < 0 ? w - 1 : -1);       // the x whose predecessor x - dx lies outside the frame
    const int row = (j + 1) * PX + p;                               // this thread's cell of sL: rows 0 and nd + 1 stay kBig

    int qn[kChunk], sn[kChunk];
    unsigned rn = 0;
    auto load_chunk = [&](int t0) {
        rn = 0;
#pragma unroll
        for (int i = 0; i < kChunk; ++i) {
            qn[i] = 0;
            sn[i] = 0;
            if (live && t0 + i < nsteps) {
                const size_t o = base + (size_t)ly * w + lx;
                qn[i] = Q[o];
                if (!kFirst) sn[i] = S[o];
                if (t0 + i == 0 || lx == x_restart) rn |= 1u << i;
                lx += dx;
                if (!horiz) lx = lx < 0 ? lx + w : (lx >= w ? lx - w : lx);
                ly += dy;
            }
        }
    };
    load_chunk(0);
    int m_prev = 2, m_cur = 0, m_next = 1;                          // slots of sM: read, reduced into, reset
    for (int t0 = 0; t0 < nsteps; t0 += kChunk) {
        int qc[kChunk], sc[kChunk];
#pragma unroll
        for (int i = 0; i < kChunk; ++i) {
            qc[i] = qn[i];
            sc[i] = sn[i];
        }
        const unsigned rc = rn;
        if (t0 + kChunk < nsteps) load_chunk(t0 + kChunk);
#pragma unroll
        for (int i = 0; i < kChunk; ++i) {
            const int t = t0 + i;
            if (t < nsteps) {                                       // uniform over the workgroup
                const int cur = t & 1;
                const int* lp = sL[cur ^ 1] + row;
                int L = qc[i];
                if (!((rc >> i) & 1u)) {
                    const int m = sM[m_prev][p];
                    const int best = min(min(lp[0], min(lp[-PX], lp[PX]) + p1), m + p2);
                    L += best - m;
                }
                if (!live) L = kBig;
                if (j < nd) sL[cur][row] = L;
                sc[i] += L;
                int v = L;
                for (int off = 32; off >= PX && off >= 16; off >>= 1) v = min(v, __shfl_xor(v, off));
                v = row_min(v, PX);
                if ((tid & 63) < PX) atomicMin(&sM[m_cur][p], v);
                if (j == 0) sM[m_next][p] = kBig;
                lds_barrier();
                const int r = m_prev;
                m_prev = m_cur;
                m_cur = m_next;
                m_next = r;
            }
        }
#pragma unroll
        for (int i = 0; i < kChunk; ++i) {
            if (live && t0 + i < nsteps) {
                S[base + (size_t)sy * w + sx] = (uint16_t)sc[i];
                sx += dx;
                if (!horiz) sx = sx < 0 ? sx + w : (sx >= w ? sx - w : sx);
                sy += dy;
            }
        }
    }
}

__global__ __launch_bounds__(256) void cost_depth_kernel(const uint16_t* __restrict__ S, const uint16_t* __restrict__ Q,
                                                         const float* __restrict__ invd, int w, int h, int nd, int gate,
                                                         float* __restrict__ depth_out, float* __restrict__ cost_out, int* __restrict__ plane_out) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const size_t o = (size_t)y * w + x, stride = (size_t)w * h;
    int best = 0, best_j = 0, prev = 0, sm1 = 0, sp1 = 0;
    bool pending = false;
    for (int j = 0; j < nd; ++j) {
        const int s = S[(size_t)j * stride + o];
        if (pending) {
            sp1 = s;
            pending = false;
        }
        if (j == 0 || s < best) {
            best = s;
            best_j = j;
            sm1 = prev;
            pending = true;
        }
        prev = s;
    }
    float inv = invd[best_j];
    if (best_j > 0 && best_j < nd - 1) {
        const float a = (float)sm1, b = (float)best, c = (float)sp1;
        const float den = (a + c) - 2.0f * b;
        float delta = 0.0f;
        if (den > 0.0f) delta = fminf(fmaxf(0.5f * (a - c) / den, -0.5f), 0.5f);
        inv = invd[best_j] + delta * (delta >= 0.0f ? invd[best_j + 1] - invd[best_j] : invd[best_j] - invd[best_j - 1]);
    }
    const int q = Q[(size_t)best_j * stride + o];
    depth_out[o] = q >= gate ? 0.0f : 1.0f / inv;
    cost_out[o] = (float)q / 1024.0f;
    if (plane_out) plane_out[o] = best_j;
}

bool frame_ok(int64_t w, int64_t h) { return w >= 1 && h >= 1 && w < (1 << 15) && h < (1 << 15); }

template <bool kFirst>
void launch_path(const uint16_t* q, uint16_t* s, int w, int h, int nd, int horiz, int dx, int dy, int p1, int p2, hipStream_t stream) {
    int pad = 2;
    while (pad < nd) pad <<= 1;                                      // ndepth padded to a power of two, 2..1024
    const int threads = pad > kTargetThreads ? pad : kTargetThreads;
    int px_log2 = 0;
    while ((pad << (px_log2 + 1)) <= threads) ++px_log2;             // PX = threads / pad
    const int lines = horiz ? h : w, px = 1 << px_log2;
    hipLaunchKernelGGL(path_kernel<kFirst>, dim3((unsigned)((lines + px - 1) / px)), dim3(threads), 0, stream, q, s, w, h, nd, px_log2, horiz,
                       dx, dy, p1, p2);
}

}  // namespace

extern "C" int sfm_mvs_cost_shift(const float* volume_dev, int64_t w, int64_t h, int ndepth, int shift, uint16_t* q_dev, void* stream) {
    SFM_CHECK_ARG(shift >= 0 && shift <= kMaxShift, "sfm_mvs_cost_shift: shift %d outside 0..%d", shift, kMaxShift);
    SFM_CHECK_ARG(ndepth >= 2 && ndepth <= 1024, "sfm_mvs_cost_shift: ndepth %d outside 2..1024", ndepth);
    SFM_CHECK_ARG(frame_ok(w, h), "sfm_mvs_cost_shift: %lld x %lld frame: each side must be in 1..32767", (long long)w, (long long)h);
    SFM_CHECK_ARG(volume_dev && q_dev, "sfm_mvs_cost_shift: null required pointer");
    const dim3 grid((unsigned)((w + kTileW - 1) / kTileW), (unsigned)((h + kTileH - 1) / kTileH), (unsigned)ndepth);
    hipLaunchKernelGGL(cost_shift_kernel, grid, dim3(256), 0, sfm::as_stream(stream), volume_dev, (int)w, (int)h, shift, q_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" int sfm_mvs_cost_aggregate(const uint16_t* q_dev, int64_t w, int64_t h, int ndepth, int p1, int p2, int ndir, uint16_t* s_dev,
                                      void* stream) {
    SFM_CHECK_ARG(ndir == 4 || ndir == 8, "sfm_mvs_cost_aggregate: ndir %d is neither 4 nor 8", ndir);
    SFM_CHECK_ARG(p1 >= 0 && p1 <= p2 && p2 <= kQMax, "sfm_mvs_cost_aggregate: penalties p1 %d, p2 %d: need 0 <= p1 <= p2 <= %d", p1, p2, kQMax);
    SFM_CHECK_ARG(ndepth >= 2 && ndepth <= 1024, "sfm_mvs_cost_aggregate: ndepth %d outside 2..1024", ndepth);
    SFM_CHECK_ARG(frame_ok(w, h), "sfm_mvs_cost_aggregate: %lld x %lld frame: each side must be in 1..32767", (long long)w, (long long)h);
    SFM_CHECK_ARG(q_dev && s_dev, "sfm_mvs_cost_aggregate: null required pointer");
    SFM_CHECK_ARG((const void*)q_dev != (const void*)s_dev, "sfm_mvs_cost_aggregate: q_dev and s_dev must be distinct buffers");
    static const int dirs[8][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}, {1, 1}, {-1, 1}, {1, -1}, {-1, -1}};
    hipStream_t st = sfm::as_stream(stream);
    for (int r = 0; r < ndir; ++r) {
        const int dx = dirs[r][0], dy = dirs[r][1], horiz = dy == 0;
        if (r == 0)
            launch_path<true>(q_dev, s_dev, (int)w, (int)h, ndepth, horiz, dx, dy, p1, p2, st);
        else
            launch_path<false>(q_dev, s_dev, (int)w, (int)h, ndepth, horiz, dx, dy, p1, p2, st);
        SFM_CHECK_LAUNCH();
    }
    return SFM_OK;
}

extern "C" int sfm_mvs_cost_depth(const uint16_t* s_dev, const uint16_t* q_dev, const float* invd_dev, int64_t w, int64_t h, int ndepth,
                                  int gate, float* depth_dev, float* cost_dev, int32_t* plane_dev, void* stream) {
    SFM_CHECK_ARG(gate >= 0 && gate <= 65535, "sfm_mvs_cost_depth: gate %d outside 0..65535", gate);
    SFM_CHECK_ARG(ndepth >= 2 && ndepth <= 1024, "sfm_mvs_cost_depth: ndepth %d outside 2..1024", ndepth);
    SFM_CHECK_ARG(frame_ok(w, h), "sfm_mvs_cost_depth: %lld x %lld frame: each side must be in 1..32767", (long long)w, (long long)h);
    SFM_CHECK_ARG(s_dev && q_dev && invd_dev && depth_dev && cost_dev, "sfm_mvs_cost_depth: null required pointer");
    const dim3 grid((unsigned)((w + 63) / 64), (unsigned)((h + 3) / 4));
    hipLaunchKernelGGL(cost_depth_kernel, grid, dim3(256), 0, sfm::as_stream(stream), s_dev, q_dev, invd_dev, (int)w, (int)h, ndepth, gate,
                       depth_dev, cost_dev, plane_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}
