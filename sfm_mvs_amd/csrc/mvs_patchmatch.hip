// PatchMatch refinement of an MVS depth map over slanted support planes (include/sfm_hip.h, "MVS-PATCHMATCH"; docs/mvs.md §9): the
// opt-in stage between sfm_mvs_plane_sweep (or the aggregation) and sfm_mvs_consistency.
//   sfm_mvs_patchmatch   per pixel a plane (q0, a, b) of inverse depth and its cost; red-black propagation from the neighbours and
//                        three random perturbations per half-sweep; a depth map, a cost map and (optionally) world normals
// The cost of a plane is the sweep's windowed ZNCC cost with the plane's inverse depth taken per window sample, every arithmetic
// step a correctly rounded float32 operation in the header's order (no FMA: the Makefile passes -ffp-contract=off), so that
// tests/np_mvs_patchmatch.py restates the kernels bit for bit and a zero-slope plane at invd[j] gives the sweep's volume word.
//
// pm_init_kernel:   a workgroup owns a 16 x 16 tile, one lane per pixel.
// pm_sweep_kernel:  a workgroup owns a 32 x 16 tile, one lane per pixel of the active colour (256 of the 512).  It reads the other
//                   colour's planes only (every candidate neighbour sits at an odd Manhattan distance) and writes its own colour's:
//                   in place, and no word depends on the order in which lanes or workgroups run.
// Both load the reference tile plus its halo into LDS once; the two plane-independent reference moments are formed from it once per
// lane and kept in registers (a lane owns one pixel for the whole launch, so LDS would only hold a copy).  The source samples are
// gathered from global memory: a tile's samples of one source lie in a patch of that source, which L2 holds.
// pm_finish_kernel: one lane per pixel, no LDS.
// No atomics, no scratch; every loop is bounded by radius <= 4, nsrc <= 8, 8 neighbours, iters <= 16.  A pixel whose reference
// window leaves the frame or has too little texture costs 2 under every plane, and no candidate can be strictly cheaper: its lane
// leaves before the candidates (no output word changes).
#include "common.h"

namespace {

constexpr int kTileH = 16;
constexpr int kInitTileW = 16;                  // 256 lanes, one pixel each
constexpr int kSweepTileW = 32;                 // 256 lanes, one pixel of the active colour each
constexpr int kMaxRadius = 4;
constexpr int kMaxViews = 8;
constexpr int kMaxIters = 16;
constexpr int kStride = kSweepTileW + 2 * kMaxRadius;   // LDS row stride of the reference tile + halo (40)
constexpr int kRows = kTileH + 2 * kMaxRadius;           // 24

struct PmViews {
    const uint8_t* src[kMaxViews];
    float mv[kMaxViews][12];                    // M (3x3 row-major) | v (3) per source
};

struct PmFrame {
    int nsrc, w, h, r, topk;
    float var_min, qmin, qmax;
};

struct PmNormal {
    float n[9];                                 // N = -R^T K^T (3x3 row-major)
};

__device__ inline float pix(const uint8_t* img, int w, int x, int y) { return (float)img[(size_t)y * w + x] - 128.0f; }

// counter-based uniform in [-1, 1]: no state, a function of (seed, pixel, iteration, draw index)
__device__ inline float draw(uint32_t seed, uint32_t pixel, uint32_t it, uint32_t c) {
    uint32_t x = seed ^ (pixel * 0x9E3779B9u + it * 0x85EBCA6Bu + c * 0xC2B2AE35u);
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return (float)(int32_t)x * 0x1p-31f;
}

// reference I' of a tw x kTileH tile at (bx, by) plus its halo of r, 0 outside the frame; ends with a barrier
__device__ inline void load_ref(float* sR, const uint8_t* __restrict__ ref, int w, int h, int bx, int by, int tw, int r) {
    const int sw = tw + 2 * r, sh = kTileH + 2 * r;
    for (int i = threadIdx.x; i < sw * sh; i += 256) {
        const int hy = i / sw, hx = i - hy * sw;
        const int gx = bx - r + hx, gy = by - r + hy;
        sR[hy * kStride + hx] = (gx >= 0 && gx < w && gy >= 0 && gy < h) ? pix(ref, w, gx, gy) : 0.0f;
    }
    __syncthreads();
}

// S_r and var_r of the window whose top-left sample is win[0]: row sums left to right, rows top to bottom
__device__ inline void ref_moments(const float* win, int diam, float n, float& s_r, float& var_r) {
    float s_rr = 0.0f;
    s_r = 0.0f;
    for (int i = 0; i < diam; ++i) {
        const float* row = win + i * kStride;
        float a = row[0], b = row[0] * row[0];
        for (int j = 1; j < diam; ++j) {
            a = a + row[j];
            b = b + row[j] * row[j];
        }
        if (i == 0) {
            s_r = a;
            s_rr = b;
        } else {
            s_r = s_r + a;
            s_rr = s_rr + b;
        }
    }
    var_r = s_rr - (s_r * s_r) / n;
}

// C of the plane (q0, a, b) at pixel (x, y) whose reference window lies in the frame and has var_r >= var_min
__device__ inline float plane_cost(const float* win, const PmViews& views, const PmFrame& f, float n, float s_r, float var_r, int x, int y,
                                   float q0, float a, float b) {
    const int r = f.r, diam = 2 * r + 1, w = f.w, h = f.h;
    float k8[kMaxViews];
#pragma unroll
    for (int q = 0; q < kMaxViews; ++q) k8[q] = 3.0f;          // above every cost (<= 2): the list of the smallest, ascending
    for (int s = 0; s < f.nsrc; ++s) {
        const uint8_t* src = views.src[s];
        const float* m = views.mv[s];
        float s_w = 0.0f, s_ww = 0.0f, s_rw = 0.0f;
        bool bad = false;
        for (int i = 0; i < diam; ++i) {
            const float fyp = (float)(y - r + i);
            const float tb = b * (float)(i - r);
            const float* rrow = win + i * kStride;
            float ra = 0.0f, rb = 0.0f, re = 0.0f;
            for (int j = 0; j < diam; ++j) {
                const float fxp = (float)(x - r + j);
                const float id = (q0 + a * (float)(j - r)) + tb;
                const float h0 = ((m[0] * fxp + m[1] * fyp) + m[2]) + m[9] * id;
                const float h1 = ((m[3] * fxp + m[4] * fyp) + m[5]) + m[10] * id;
                const float h2 = ((m[6] * fxp + m[7] * fyp) + m[8]) + m[11] * id;
                float val = 0.0f;
                bool ok = false;
                if (h2 > 0.0f) {
                    const float px = h0 / h2, py = h1 / h2;
                    if (px >= 0.0f && px <= (float)(w - 1) && py >= 0.0f && py <= (float)(h - 1)) {
                        const int x0 = min((int)floorf(px), w - 2), y0 = min((int)floorf(py), h - 2);
                        const float fx = px - (float)x0, fy = py - (float)y0;
                        const float i00 = pix(src, w, x0, y0), i01 = pix(src, w, x0 + 1, y0);
                        const float i10 = pix(src, w, x0, y0 + 1), i11 = pix(src, w, x0 + 1, y0 + 1);
                        val = (1.0f - fy) * ((1.0f - fx) * i00 + fx * i01) + fy * ((1.0f - fx) * i10 + fx * i11);
                        ok = true;
                    }
                }
                bad = bad || !ok;
                if (j == 0) {
                    ra = val;
                    rb = val * val;
                    re = rrow[0] * val;
                } else {
                    ra = ra + val;
                    rb = rb + val * val;
                    re = re + rrow[j] * val;
                }
            }
            if (i == 0) {
                s_w = ra;
                s_ww = rb;
                s_rw = re;
            } else {
                s_w = s_w + ra;
                s_ww = s_ww + rb;
                s_rw = s_rw + re;
            }
        }
        float c = 2.0f;
        const float var_w = s_ww - (s_w * s_w) / n;
        if (!bad && !(var_w < f.var_min)) {
            const float cov = s_rw - (s_r * s_w) / n;
            c = 1.0f - cov / sqrtf(var_r * var_w);
            c = fminf(fmaxf(c, 0.0f), 2.0f);
        }
#pragma unroll
        for (int q = 0; q < kMaxViews; ++q) {                   // insertion into the ascending list, no dynamic register index
            const float lo = fminf(c, k8[q]), hi = fmaxf(c, k8[q]);
            k8[q] = lo;
            c = hi;
        }
    }
    float sum = k8[0];
#pragma unroll
    for (int q = 1; q < kMaxViews; ++q)
        if (q < f.topk) sum = sum + k8[q];
    return sum / (float)f.topk;
}

__device__ inline bool window_in_frame(int x, int y, int r, int w, int h) { return x - r >= 0 && x + r <= w - 1 && y - r >= 0 && y + r <= h - 1; }

__global__ __launch_bounds__(256) void pm_init_kernel(const uint8_t* __restrict__ ref, PmViews views, PmFrame f, const float* __restrict__ depth_init,
                                                      uint32_t seed, float4* __restrict__ state) {
    __shared__ float sR[kRows * kStride];
    const int tx = threadIdx.x & (kInitTileW - 1), ty = threadIdx.x / kInitTileW;
    const int bx = blockIdx.x * kInitTileW, by = blockIdx.y * kTileH;
    load_ref(sR, ref, f.w, f.h, bx, by, kInitTileW, f.r);
    const int x = bx + tx, y = by + ty;
    if (x >= f.w || y >= f.h) return;
    const size_t o = (size_t)y * f.w + x;
    float q0 = 0.0f;
    bool have = false;
    if (depth_init) {
        const float d = depth_init[o];
        if (d > 0.0f) {
            q0 = 1.0f / d;
            have = q0 >= f.qmin && q0 <= f.qmax;
        }
    }
    if (!have) q0 = f.qmin + (f.qmax - f.qmin) * (0.5f * draw(seed, (uint32_t)o, 0u, 0u) + 0.5f);
    float cost = 2.0f;
    if (window_in_frame(x, y, f.r, f.w, f.h)) {
        const int diam = 2 * f.r + 1;
        const float n = (float)(diam * diam);
        const float* win = sR + ty * kStride + tx;
        float s_r, var_r;
        ref_moments(win, diam, n, s_r, var_r);
        if (!(var_r < f.var_min)) cost = plane_cost(win, views, f, n, s_r, var_r, x, y, q0, 0.0f, 0.0f);
    }
    state[o] = make_float4(q0, 0.0f, 0.0f, cost);
}

__global__ __launch_bounds__(256) void pm_sweep_kernel(const uint8_t* __restrict__ ref, PmViews views, PmFrame f, int colour, uint32_t it, int far,
                                                       float depth_s, float slope_s, uint32_t seed, float4* state) {
    __shared__ float sR[kRows * kStride];
    const int ty = threadIdx.x / (kSweepTileW / 2);
    const int bx = blockIdx.x * kSweepTileW, by = blockIdx.y * kTileH;
    load_ref(sR, ref, f.w, f.h, bx, by, kSweepTileW, f.r);
    const int y = by + ty;
    const int lx = 2 * (threadIdx.x & (kSweepTileW / 2 - 1)) + ((y ^ colour) & 1);   // bx is even: (x + y) & 1 == colour
    const int x = bx + lx;
    if (x >= f.w || y >= f.h || !window_in_frame(x, y, f.r, f.w, f.h)) return;
    const int diam = 2 * f.r + 1;
    const float n = (float)(diam * diam);
    const float* win = sR + ty * kStride + lx;
    float s_r, var_r;
    ref_moments(win, diam, n, s_r, var_r);
    if (var_r < f.var_min) return;
    const size_t o = (size_t)y * f.w + x;
    const float4 st = state[o];
    float q0 = st.x, a = st.y, b = st.z, cost = st.w;
    const float fr = (float)f.r;
    auto consider = [&](float cq, float ca, float cb) {
        const bool finite = fabsf(cq) < INFINITY && fabsf(ca) < INFINITY && fabsf(cb) < INFINITY;
        if (!(finite && cq >= f.qmin && cq <= f.qmax && fr * (fabsf(ca) + fabsf(cb)) <= 0.5f * cq)) return;
        const float c = plane_cost(win, views, f, n, s_r, var_r, x, y, cq, ca, cb);
        if (c < cost) {
            q0 = cq;
            a = ca;
            b = cb;
            cost = c;
        }
    };
    const int nn = far ? 8 : 4;
    for (int i = 0; i < nn; ++i) {                              // (-1,0) (1,0) (0,-1) (0,1), then the same at distance 3
        const int step = i < 4 ? 1 : 3, k = i & 3;
        const int xn = x + (k == 0 ? -step : k == 1 ? step : 0), yn = y + (k == 2 ? -step : k == 3 ? step : 0);
        if (xn < 0 || xn >= f.w || yn < 0 || yn >= f.h) continue;
        const float4 nb = state[(size_t)yn * f.w + xn];
        consider((nb.x + nb.y * (float)(x - xn)) + nb.z * (float)(y - yn), nb.y, nb.z);
    }
    const uint32_t p = (uint32_t)o;
    consider(q0 * (1.0f + depth_s * draw(seed, p, it, 1u)), a, b);
    {
        const float t = slope_s * q0;
        consider(q0, a + t * draw(seed, p, it, 2u), b + t * draw(seed, p, it, 3u));
    }
    {
        const float t = slope_s * q0;
        consider(q0 * (1.0f + depth_s * draw(seed, p, it, 4u)), a + t * draw(seed, p, it, 5u), b + t * draw(seed, p, it, 6u));
    }
    state[o] = make_float4(q0, a, b, cost);
}

__global__ __launch_bounds__(256) void pm_finish_kernel(const float4* __restrict__ state, PmNormal nm, int w, int h, int r, float cost_max,
                                                        float* __restrict__ depth, float* __restrict__ cost, float* __restrict__ normal) {
    const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= w || y >= h) return;
    const size_t o = (size_t)y * w + x;
    const float4 st = state[o];
    float d = 1.0f / st.x;
    if (!window_in_frame(x, y, r, w, h) || !(st.w < cost_max)) d = 0.0f;
    depth[o] = d;
    cost[o] = st.w;
    if (!normal) return;
    float n0 = 0.0f, n1 = 0.0f, n2 = 0.0f;
    if (d != 0.0f) {
        const float A = st.y, B = st.z, C = (st.x - st.y * (float)x) - st.z * (float)y;
        n0 = (nm.n[0] * A + nm.n[1] * B) + nm.n[2] * C;
        n1 = (nm.n[3] * A + nm.n[4] * B) + nm.n[5] * C;
        n2 = (nm.n[6] * A + nm.n[7] * B) + nm.n[8] * C;
        const float len = sqrtf((n0 * n0 + n1 * n1) + n2 * n2);
        n0 = n0 / len;
        n1 = n1 / len;
        n2 = n2 / len;
    }
    normal[3 * o + 0] = n0;
    normal[3 * o + 1] = n1;
    normal[3 * o + 2] = n2;
}

}  // namespace

extern "C" int sfm_mvs_patchmatch(const uint8_t* ref_dev, const uint8_t* const* src_dev, const float* mv_host, int nsrc, int64_t w, int64_t h,
                                  float qmin, float qmax, int radius, int topk, float var_min, float cost_max, const float* depth_init_dev,
                                  int iters, int far, float depth_step, float slope_step, uint32_t seed, const float* nmat_host,
                                  float* state_dev, float* depth_dev, float* cost_dev, float* normal_dev, void* stream) {
    SFM_CHECK_ARG(radius >= 1 && radius <= kMaxRadius, "sfm_mvs_patchmatch: radius %d outside 1..%d", radius, kMaxRadius);
    SFM_CHECK_ARG(nsrc >= 1 && nsrc <= kMaxViews, "sfm_mvs_patchmatch: nsrc %d outside 1..%d", nsrc, kMaxViews);
    SFM_CHECK_ARG(topk >= 1 && topk <= nsrc, "sfm_mvs_patchmatch: topk %d outside 1..nsrc (%d)", topk, nsrc);
    SFM_CHECK_ARG(iters >= 0 && iters <= kMaxIters, "sfm_mvs_patchmatch: iters %d outside 0..%d", iters, kMaxIters);
    SFM_CHECK_ARG(w >= 2 * radius + 1 && h >= 2 * radius + 1 && w < (1 << 15) && h < (1 << 15),
                  "sfm_mvs_patchmatch: %lld x %lld frame: each side must be in 2*radius+1 .. 32767", (long long)w, (long long)h);
    SFM_CHECK_ARG(qmin > 0.0f && qmin <= qmax && qmax < INFINITY, "sfm_mvs_patchmatch: need 0 < qmin <= qmax, finite");
    SFM_CHECK_ARG(var_min > 0.0f && var_min < INFINITY, "sfm_mvs_patchmatch: var_min must be positive and finite");
    SFM_CHECK_ARG(!(cost_max != cost_max), "sfm_mvs_patchmatch: cost_max is NaN");
    SFM_CHECK_ARG(depth_step >= 0.0f && depth_step < INFINITY && slope_step >= 0.0f && slope_step < INFINITY,
                  "sfm_mvs_patchmatch: depth_step and slope_step must be finite and >= 0");
    SFM_CHECK_ARG(ref_dev && src_dev && mv_host && state_dev && depth_dev && cost_dev, "sfm_mvs_patchmatch: null required pointer");
    SFM_CHECK_ARG((reinterpret_cast<uintptr_t>(state_dev) & 15) == 0, "sfm_mvs_patchmatch: state_dev must be 16-byte aligned");
    SFM_CHECK_ARG(!normal_dev || nmat_host, "sfm_mvs_patchmatch: normals need nmat_host");
    PmViews views{};
    for (int s = 0; s < nsrc; ++s) {
        SFM_CHECK_ARG(src_dev[s], "sfm_mvs_patchmatch: source frame %d is null", s);
        views.src[s] = src_dev[s];
        for (int k = 0; k < 12; ++k) views.mv[s][k] = mv_host[12 * s + k];
    }
    PmNormal nm{};
    if (normal_dev)
        for (int k = 0; k < 9; ++k) nm.n[k] = nmat_host[k];
    const PmFrame f{nsrc, (int)w, (int)h, radius, topk, var_min, qmin, qmax};
    hipStream_t st = sfm::as_stream(stream);
    float4* state = reinterpret_cast<float4*>(state_dev);
    const dim3 grid16((unsigned)((w + 15) / 16), (unsigned)((h + kTileH - 1) / kTileH));
    const dim3 grid32((unsigned)((w + kSweepTileW - 1) / kSweepTileW), (unsigned)((h + kTileH - 1) / kTileH));
    hipLaunchKernelGGL(pm_init_kernel, grid16, dim3(256), 0, st, ref_dev, views, f, depth_init_dev, seed, state);
    SFM_CHECK_LAUNCH();
    for (int it = 0; it < iters; ++it) {
        const float s = ldexpf(1.0f, -it);                      // 2^-it: exact, and so are the two products' scalings
        for (int colour = 0; colour < 2; ++colour) {            // red ((x + y) even) first, then black
            hipLaunchKernelGGL(pm_sweep_kernel, grid32, dim3(256), 0, st, ref_dev, views, f, colour, (uint32_t)it, far ? 1 : 0, depth_step * s,
                               slope_step * s, seed, state);
            SFM_CHECK_LAUNCH();
        }
    }
    hipLaunchKernelGGL(pm_finish_kernel, grid16, dim3(256), 0, st, state, nm, (int)w, (int)h, radius, cost_max, depth_dev, cost_dev, normal_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}
