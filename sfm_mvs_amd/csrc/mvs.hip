// Plane-sweep multi-view stereo: the "mvs" half the reference leaves for later (sfm.py:298 `densify = False`, the dense.ply
// branch of to_ply at sfm.py:194-201 that nothing feeds).
//   sfm_mvs_plane_sweep   one depth map per reference view: fronto-parallel planes uniform in inverse depth, windowed ZNCC
//                         against each source view, top-k aggregation, winner-take-all, sub-plane parabola
//   sfm_mvs_consistency   geometric consistency of a depth map with its neighbours' maps; the world point of every kept pixel
// Every arithmetic step is a correctly rounded float32 operation in the order include/sfm_hip.h writes it (no FMA: the Makefile
// passes -ffp-contract=off), so that tests/np_mvs.py restates the kernels bit for bit.
//
// plane_sweep_kernel: a workgroup owns a 16 x 16 tile of output pixels, one lane per pixel, and walks every plane with the
// winner-take-all state in registers (the cost volume reaches HBM only when the caller asks for it).  Per (plane, source) the
// tile plus its halo is warped into LDS (bilinear; the source frames are <= 0.6 MB and stay in L2), the three plane-dependent
// window moments are formed as row sums (one LDS pass over the halo rows) then column sums of those (registers), and the
// per-source costs are kept in a sorted 8-slot register list.  The two reference moments do not depend on the plane: computed
// once per pixel.  No atomics; every loop is bounded by radius <= 4, nsrc <= 8, ndepth <= 1024.
#include "common.h"

namespace {

constexpr int kTile = 16;                       // output tile side (256 lanes, one pixel each)
constexpr int kMaxRadius = 4;
constexpr int kHaloMax = kTile + 2 * kMaxRadius;   // 24
constexpr int kMaxViews = 8;

struct SweepViews {
    const uint8_t* src[kMaxViews];
    float mv[kMaxViews][12];                    // M (3x3 row-major) | v (3) per source
};

struct ConsistencyViews {
    const float* depth[kMaxViews];
    float ab[kMaxViews][12];                    // A (3x3 row-major) | b (3) per neighbour
    int index[kMaxViews];
};

struct WorldMap {
    float bc[12];                               // B (3x3 row-major) | c (3)
};

__device__ inline float pix(const uint8_t* img, int w, int x, int y) { return (float)img[(size_t)y * w + x] - 128.0f; }

__global__ __launch_bounds__(256) void plane_sweep_kernel(const uint8_t* __restrict__ ref, SweepViews views, int nsrc, int w, int h,
                                                          const float* __restrict__ invd, int ndepth, int r, int topk, float var_min,
                                                          float cost_max, float* __restrict__ depth_out, float* __restrict__ cost_out,
                                                          int* __restrict__ plane_out, float* __restrict__ volume_out) {
    __shared__ float sR[kHaloMax * kHaloMax];      // reference I' of tile + halo (row stride kHaloMax)
    __shared__ float sW[kHaloMax * kHaloMax];      // warped source I'
    __shared__ int sV[kHaloMax * kHaloMax];        // 1 where the warped sample is valid
    __shared__ float hW[kHaloMax * kTile], hWW[kHaloMax * kTile], hRW[kHaloMax * kTile];   // row sums: halo rows x tile columns
    __shared__ int hBad[kHaloMax * kTile];

    const int tx = threadIdx.x & (kTile - 1), ty = threadIdx.x / kTile;
    const int bx = blockIdx.x * kTile, by = blockIdx.y * kTile;
    const int x = bx + tx, y = by + ty;
    const int side = kTile + 2 * r, diam = 2 * r + 1;
    const float n = (float)(diam * diam);

    for (int i = threadIdx.x; i < side * side; i += 256) {
        const int hy = i / side, hx = i - hy * side;
        const int gx = bx - r + hx, gy = by - r + hy;
        sR[hy * kHaloMax + hx] = (gx >= 0 && gx < w && gy >= 0 && gy < h) ? pix(ref, w, gx, gy) : 0.0f;
    }
    __syncthreads();

    // reference moments: row sums left to right, rows top to bottom
    float s_r = 0.0f, s_rr = 0.0f;
    for (int dy = 0; dy < diam; ++dy) {
        const float* row = sR + (ty + dy) * kHaloMax + tx;
        float a = row[0], b = row[0] * row[0];
        for (int dx = 1; dx < diam; ++dx) {
            a = a + row[dx];
            b = b + row[dx] * row[dx];
        }
        if (dy == 0) {
            s_r = a;
            s_rr = b;
        } else {
            s_r = s_r + a;
            s_rr = s_rr + b;
        }
    }
    const float var_r = s_rr - (s_r * s_r) / n;
    const bool inside = x < w && y < h;
    const bool ref_in = x - r >= 0 && x + r <= w - 1 && y - r >= 0 && y + r <= h - 1;   // the reference window lies in the frame
    const bool ref_ok = ref_in && !(var_r < var_min);

    float best_c = 0.0f, prev_c = 0.0f, cm1 = 0.0f, cp1 = 0.0f;
    int best_j = 0;
    bool pending = false;
    const size_t plane_stride = (size_t)w * h;

    for (int j = 0; j < ndepth; ++j) {
        const float id = invd[j];
        float k8[kMaxViews];
#pragma unroll
        for (int q = 0; q < kMaxViews; ++q) k8[q] = 3.0f;      // above every cost (<= 2): the list of the smallest, ascending
        for (int s = 0; s < nsrc; ++s) {
            const uint8_t* src = views.src[s];
            const float* m = views.mv[s];
            for (int i = threadIdx.x; i < side * side; i += 256) {
                const int hy = i / side, hx = i - hy * side;
                const float fxp = (float)(bx - r + hx), fyp = (float)(by - r + hy);
                const float h0 = ((m[0] * fxp + m[1] * fyp) + m[2]) + m[9] * id;
                const float h1 = ((m[3] * fxp + m[4] * fyp) + m[5]) + m[10] * id;
                const float h2 = ((m[6] * fxp + m[7] * fyp) + m[8]) + m[11] * id;
                float val = 0.0f;
                int ok = 0;
                if (h2 > 0.0f) {
                    const float px = h0 / h2, py = h1 / h2;
                    if (px >= 0.0f && px <= (float)(w - 1) && py >= 0.0f && py <= (float)(h - 1)) {
                        const int x0 = min((int)floorf(px), w - 2), y0 = min((int)floorf(py), h - 2);
                        const float fx = px - (float)x0, fy = py - (float)y0;
                        const float i00 = pix(src, w, x0, y0), i01 = pix(src, w, x0 + 1, y0);
                        const float i10 = pix(src, w, x0, y0 + 1), i11 = pix(src, w, x0 + 1, y0 + 1);
                        val = (1.0f - fy) * ((1.0f - fx) * i00 + fx * i01) + fy * ((1.0f - fx) * i10 + fx * i11);
                        ok = 1;
                    }
                }
                sW[hy * kHaloMax + hx] = val;
                sV[hy * kHaloMax + hx] = ok;
            }
            __syncthreads();
            for (int i = threadIdx.x; i < side * kTile; i += 256) {
                const int hy = i / kTile, c = i - hy * kTile;
                const float* wr = sW + hy * kHaloMax + c;
                const float* rr = sR + hy * kHaloMax + c;
                const int* vr = sV + hy * kHaloMax + c;
                float a = wr[0], b = wr[0] * wr[0], e = rr[0] * wr[0];
                int bad = vr[0] ^ 1;
                for (int dx = 1; dx < diam; ++dx) {
                    a = a + wr[dx];
                    b = b + wr[dx] * wr[dx];
                    e = e + rr[dx] * wr[dx];
                    bad |= vr[dx] ^ 1;
                }
                hW[i] = a;
                hWW[i] = b;
                hRW[i] = e;
                hBad[i] = bad;
            }
            __syncthreads();
            float s_w = hW[ty * kTile + tx], s_ww = hWW[ty * kTile + tx], s_rw = hRW[ty * kTile + tx];
            int bad = hBad[ty * kTile + tx];
            for (int dy = 1; dy < diam; ++dy) {
                const int k = (ty + dy) * kTile + tx;
                s_w = s_w + hW[k];
                s_ww = s_ww + hWW[k];
                s_rw = s_rw + hRW[k];
                bad |= hBad[k];
            }
            // (the next source's warp writes sW / sV only: the row sums read here are rewritten after the next barrier)
            float c = 2.0f;
            const float var_w = s_ww - (s_w * s_w) / n;
            if (ref_ok && !bad && !(var_w < var_min)) {
                const float cov = s_rw - (s_r * s_w) / n;
                c = 1.0f - cov / sqrtf(var_r * var_w);
                c = fminf(fmaxf(c, 0.0f), 2.0f);
            }
#pragma unroll
            for (int q = 0; q < kMaxViews; ++q) {       // insertion into the ascending list, no dynamic register index
                const float lo = fminf(c, k8[q]), hi = fmaxf(c, k8[q]);
                k8[q] = lo;
                c = hi;
            }
        }
        float sum = k8[0];
#pragma unroll
        for (int q = 1; q < kMaxViews; ++q)
            if (q < topk) sum = sum + k8[q];
        const float cj = sum / (float)topk;
        if (inside && volume_out) volume_out[(size_t)j * plane_stride + (size_t)y * w + x] = cj;
        if (pending) {
            cp1 = cj;
            pending = false;
        }
        if (j == 0 || cj < best_c) {
            best_c = cj;
            best_j = j;
            cm1 = prev_c;
            pending = true;
        }
        prev_c = cj;
    }
    if (!inside) return;
    float inv = invd[best_j];
    if (best_j > 0 && best_j < ndepth - 1) {
        const float den = (cm1 + cp1) - 2.0f * best_c;
        float delta = 0.0f;
        if (den > 0.0f) delta = fminf(fmaxf(0.5f * (cm1 - cp1) / den, -0.5f), 0.5f);
        inv = invd[best_j] + delta * (delta >= 0.0f ? invd[best_j + 1] - invd[best_j] : invd[best_j] - invd[best_j - 1]);
    }
    float d = 1.0f / inv;
    if (!ref_in || !(best_c < cost_max)) d = 0.0f;
    const size_t o = (size_t)y * w + x;
    depth_out[o] = d;
    cost_out[o] = best_c;
    if (plane_out) plane_out[o] = best_j;
}

__global__ __launch_bounds__(256) void consistency_kernel(const float* __restrict__ depth, ConsistencyViews views, int nview, int ref_index,
                                                          WorldMap world, int w, int h, float tau, int min_consistent, int unique,
                                                          uint8_t* __restrict__ mask, float* __restrict__ xyz) {
    const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= w || y >= h) return;
    const size_t o = (size_t)y * w + x;
    const float d = depth[o];
    const float fx = (float)x, fy = (float)y;
    int count = 0;
    bool lower = false;
    if (d > 0.0f) {
        for (int v = 0; v < nview; ++v) {
            const float* a = views.ab[v];
            const float p0 = d * ((a[0] * fx + a[1] * fy) + a[2]) + a[9];
            const float p1 = d * ((a[3] * fx + a[4] * fy) + a[5]) + a[10];
            const float p2 = d * ((a[6] * fx + a[7] * fy) + a[8]) + a[11];
            if (!(p2 > 0.0f)) continue;
            const float u = floorf(p0 / p2 + 0.5f), t = floorf(p1 / p2 + 0.5f);
            if (!(u >= 0.0f && u <= (float)(w - 1) && t >= 0.0f && t <= (float)(h - 1))) continue;
            const float dv = views.depth[v][(size_t)(int)t * w + (int)u];
            if (dv > 0.0f && fabsf(p2 - dv) <= tau * dv) {
                ++count;
                lower = lower || views.index[v] < ref_index;
            }
        }
    }
    const bool keep = d > 0.0f && count >= min_consistent && !(unique && lower);
    mask[o] = keep ? 1 : 0;
    const float* b = world.bc;
    xyz[3 * o + 0] = keep ? d * ((b[0] * fx + b[1] * fy) + b[2]) + b[9] : 0.0f;
    xyz[3 * o + 1] = keep ? d * ((b[3] * fx + b[4] * fy) + b[5]) + b[10] : 0.0f;
    xyz[3 * o + 2] = keep ? d * ((b[6] * fx + b[7] * fy) + b[8]) + b[11] : 0.0f;
}

}  // namespace

extern "C" int sfm_mvs_plane_sweep(const uint8_t* ref_dev, const uint8_t* const* src_dev, const float* mv_host, int nsrc, int64_t w, int64_t h,
                                   const float* invd_dev, int ndepth, int radius, int topk, float var_min, float cost_max,
                                   float* depth_dev, float* cost_dev, int32_t* plane_dev, float* volume_dev, void* stream) {
    SFM_CHECK_ARG(radius >= 1 && radius <= kMaxRadius, "sfm_mvs_plane_sweep: radius %d outside 1..%d", radius, kMaxRadius);
    SFM_CHECK_ARG(nsrc >= 1 && nsrc <= kMaxViews, "sfm_mvs_plane_sweep: nsrc %d outside 1..%d", nsrc, kMaxViews);
    SFM_CHECK_ARG(topk >= 1 && topk <= nsrc, "sfm_mvs_plane_sweep: topk %d outside 1..nsrc (%d)", topk, nsrc);
    SFM_CHECK_ARG(ndepth >= 2 && ndepth <= 1024, "sfm_mvs_plane_sweep: ndepth %d outside 2..1024", ndepth);
    SFM_CHECK_ARG(w >= 2 * radius + 1 && h >= 2 * radius + 1 && w < (1 << 15) && h < (1 << 15),
                  "sfm_mvs_plane_sweep: %lld x %lld frame: each side must be in 2*radius+1 .. 32767", (long long)w, (long long)h);
    SFM_CHECK_ARG(var_min > 0.0f && var_min < INFINITY, "sfm_mvs_plane_sweep: var_min must be positive and finite");
    SFM_CHECK_ARG(!(cost_max != cost_max), "sfm_mvs_plane_sweep: cost_max is NaN");
    SFM_CHECK_ARG(ref_dev && src_dev && mv_host && invd_dev && depth_dev && cost_dev, "sfm_mvs_plane_sweep: null required pointer");
    SweepViews views{};
    for (int s = 0; s < nsrc; ++s) {
        SFM_CHECK_ARG(src_dev[s], "sfm_mvs_plane_sweep: source frame %d is null", s);
        views.src[s] = src_dev[s];
        for (int k = 0; k < 12; ++k) views.mv[s][k] = mv_host[12 * s + k];
    }
    const dim3 grid((unsigned)((w + kTile - 1) / kTile), (unsigned)((h + kTile - 1) / kTile));
    hipLaunchKernelGGL(plane_sweep_kernel, grid, dim3(256), 0, sfm::as_stream(stream), ref_dev, views, nsrc, (int)w, (int)h, invd_dev, ndepth,
                       radius, topk, var_min, cost_max, depth_dev, cost_dev, plane_dev, volume_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" int sfm_mvs_consistency(const float* depth_dev, const float* const* nbr_depth_dev, const int32_t* nbr_index_host,
                                   const float* ab_host, int nview, int ref_index, const float* bc_host, int64_t w, int64_t h, float tau,
                                   int min_consistent, int unique, uint8_t* mask_dev, float* xyz_dev, void* stream) {
    SFM_CHECK_ARG(nview >= 0 && nview <= kMaxViews, "sfm_mvs_consistency: nview %d outside 0..%d", nview, kMaxViews);
    SFM_CHECK_ARG(min_consistent >= 0 && min_consistent <= nview, "sfm_mvs_consistency: min_consistent %d outside 0..nview (%d)", min_consistent, nview);
    SFM_CHECK_ARG(w >= 1 && h >= 1 && w < (1 << 15) && h < (1 << 15), "sfm_mvs_consistency: %lld x %lld frame: each side must be in 1..32767",
                  (long long)w, (long long)h);
    SFM_CHECK_ARG(tau >= 0.0f && tau < INFINITY, "sfm_mvs_consistency: tau must be finite and >= 0");
    SFM_CHECK_ARG(depth_dev && bc_host && mask_dev && xyz_dev && (nview == 0 || (nbr_depth_dev && nbr_index_host && ab_host)),
                  "sfm_mvs_consistency: null required pointer");
    ConsistencyViews views{};
    for (int v = 0; v < nview; ++v) {
        SFM_CHECK_ARG(nbr_depth_dev[v], "sfm_mvs_consistency: neighbour depth map %d is null", v);
        views.depth[v] = nbr_depth_dev[v];
        views.index[v] = nbr_index_host[v];
        for (int k = 0; k < 12; ++k) views.ab[v][k] = ab_host[12 * v + k];
    }
    WorldMap world{};
    for (int k = 0; k < 12; ++k) world.bc[k] = bc_host[k];
    const dim3 grid((unsigned)((w + 15) / 16), (unsigned)((h + 15) / 16));
    hipLaunchKernelGGL(consistency_kernel, grid, dim3(256), 0, sfm::as_stream(stream), depth_dev, views, nview, ref_index, world, (int)w, (int)h,
                       tau, min_consistent, unique ? 1 : 0, mask_dev, xyz_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}
