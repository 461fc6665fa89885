// Mesh texturing (include/sfm_hip.h, "MESH-TEXTURE"; docs/mesh.md §10): a depth map of the mesh in every view, the view each face is
// textured from, and a texture atlas with one half-cell chart per face.
//   sfm_mesh_render_depth   z-buffer rasteriser: min over the covering faces of the interpolated depth, by atomicMin on the bits
//   sfm_mesh_face_views     per face the visible, front-facing, in-frame view of the largest screen area (lowest index on ties)
//   sfm_mesh_texture_fill   one lane per atlas texel: its point on the face, projected into the face's view, sampled bilinearly
// Every result is a minimum or a pure function of its inputs; the float32 operations are the ones the header writes, in its order,
// compiled without contraction.  tests/np_mesh_texture.py restates the three outputs bit for bit.
//
// The rasteriser.  One lane per (view, face).  The three corners are projected per face, not once per (view, vertex) into a
// workspace: a vertex is shared by about six faces, so this repeats 36 multiply-adds and 6 divisions six times, but it spares a
// workspace of 12 B * views * vertices written and then gathered just the same (the gather of the three rows is what a lane waits
// for either way), and the call needs no workspace at all.  A lane walks its bounding box while that holds at most kSmallBox
// pixels (marching-tetrahedra faces span 2 to 7 pixels); a wave then takes its larger faces one after another, all 64 lanes
// striding over the box of one face, so any triangle is handled, a frame-filling one included, with every loop bounded by w * h and
// neither a list nor a second launch.  Atomics are no-return; a lane has at most kSmallBox of them in flight, about half of which
// pass the coverage test.
#include <algorithm>
#include <climits>
#include <cmath>

#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxGrid = 1 << 16;               // workgroups per launch; the kernels stride over what is left
constexpr int kSmallBox = 64;                   // pixels of a bounding box one lane walks alone
constexpr int64_t kMaxCount = INT32_MAX;
constexpr int64_t kMaxPixels = 1ll << 26;
constexpr int kMaxViews = 1 << 16;
constexpr int kMaxTexels = 64;                  // L: texels per triangle leg
constexpr int kCellExtra = 5;                   // cell side = L + 5
constexpr int kMaxSide = 16384;

typedef unsigned long long u64;

struct Counts {
    int nv, nf;
};

// (nv, nf): the capacities, or the pair counts_dev holds where it lies in 0..capacity.
__device__ inline Counts load_counts(const int* __restrict__ counts, int nv_cap, int nf_cap) {
    Counts c{nv_cap, nf_cap};
    if (counts) {
        const int v = counts[0], f = counts[1];
        if (v >= 0 && v <= nv_cap) c.nv = v;
        if (f >= 0 && f <= nf_cap) c.nf = f;
    }
    return c;
}

__device__ inline bool in_range(int a, int nv) { return (unsigned)a < (unsigned)nv; }

__device__ inline bool finite(float x) { return fabsf(x) < INFINITY; }          // false for NaN

struct Proj {
    float sx, sy, z;
    bool ok;                                     // projectable
};

__device__ inline Proj project(const float* __restrict__ P, float x, float y, float z) {
    const float p0 = ((P[0] * x + P[1] * y) + P[2] * z) + P[3];
    const float p1 = ((P[4] * x + P[5] * y) + P[6] * z) + P[7];
    const float p2 = ((P[8] * x + P[9] * y) + P[10] * z) + P[11];
    Proj r;
    r.sx = p0 / p2;
    r.sy = p1 / p2;
    r.z = p2;
    r.ok = p2 > 0.0f && finite(r.sx) && finite(r.sy) && finite(p2);
    return r;
}

// The three vertex rows of face f; false unless the face is valid.
__device__ inline bool corners(const float* __restrict__ verts, const int* __restrict__ faces, long long f, int nv, const float*& a,
                               const float*& b, const float*& c) {
    const int* t = faces + 3 * (size_t)f;
    const int i = t[0], j = t[1], k = t[2];
    if (!in_range(i, nv) || !in_range(j, nv) || !in_range(k, nv)) return false;
    a = verts + 3 * (size_t)i;
    b = verts + 3 * (size_t)j;
    c = verts + 3 * (size_t)k;
    return true;
}

struct Tri {
    float ax, ay, bx, by, cx, cy, ia, ib, ic, area2;
    int x0, y0, bw, bh;                          // the clipped bounding box: its corner and its size in pixels
};

// The screen triangle of face f in the view P and its box; false when the face is skipped in this view.
__device__ inline bool setup(const float* __restrict__ verts, const int* __restrict__ faces, long long f, int nv,
                             const float* __restrict__ P, int w, int h, Tri& t) {
    const float *a, *b, *c;
    if (!corners(verts, faces, f, nv, a, b, c)) return false;
    const Proj pa = project(P, a[0], a[1], a[2]), pb = project(P, b[0], b[1], b[2]), pc = project(P, c[0], c[1], c[2]);
    if (!pa.ok || !pb.ok || !pc.ok) return false;
    t.ax = pa.sx, t.ay = pa.sy, t.bx = pb.sx, t.by = pb.sy, t.cx = pc.sx, t.cy = pc.sy;
    t.area2 = (t.bx - t.ax) * (t.cy - t.ay) - (t.by - t.ay) * (t.cx - t.ax);
    if (!(t.area2 < 0.0f) && !(t.area2 > 0.0f)) return false;                   // zero, or NaN after an overflow
    const float lox = fmaxf(0.0f, ceilf(fminf(fminf(t.ax, t.bx), t.cx))), hix = fminf((float)(w - 1), floorf(fmaxf(fmaxf(t.ax, t.bx), t.cx)));
    const float loy = fmaxf(0.0f, ceilf(fminf(fminf(t.ay, t.by), t.cy))), hiy = fminf((float)(h - 1), floorf(fmaxf(fmaxf(t.ay, t.by), t.cy)));
    if (!(lox <= hix) || !(loy <= hiy)) return false;
    t.x0 = (int)lox;                                                            // all four lie in 0..w-1 / 0..h-1
    t.y0 = (int)loy;
    t.bw = (int)hix - t.x0 + 1;
    t.bh = (int)hiy - t.y0 + 1;
    t.ia = 1.0f / pa.z;
    t.ib = 1.0f / pb.z;
    t.ic = 1.0f / pc.z;
    return true;
}

// Pixel (x, y) of the triangle, 0 <= x < w, 0 <= y < h: coverage, depth, minimum.  z: the view's plane.
__device__ inline void shade(const Tri& t, int x, int y, unsigned* z, int w) {
    const float fx = (float)x, fy = (float)y;
    const float wa = (t.cx - t.bx) * (fy - t.by) - (t.cy - t.by) * (fx - t.bx);
    const float wb = (t.ax - t.cx) * (fy - t.cy) - (t.ay - t.cy) * (fx - t.cx);
    const float wc = (t.bx - t.ax) * (fy - t.ay) - (t.by - t.ay) * (fx - t.ax);
    const bool in = t.area2 > 0.0f ? (wa >= 0.0f && wb >= 0.0f && wc >= 0.0f) : (wa <= 0.0f && wb <= 0.0f && wc <= 0.0f);
    if (!in) return;
    const float iz = ((wa * t.ia + wb * t.ib) + wc * t.ic) / t.area2;
    const float d = 1.0f / iz;
    if (d > 0.0f && d < INFINITY) atomicMin(&z[(size_t)y * w + x], __float_as_uint(d));
}

__global__ __launch_bounds__(kBlock) void tex_clear_kernel(unsigned* __restrict__ z, long long words) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < words; i += stride) z[i] = 0x7f800000u;      // +inf
}

__global__ __launch_bounds__(kBlock) void tex_raster_kernel(const float* __restrict__ verts, const int* __restrict__ faces, int nv_cap, int nf_cap,
                                                            const int* __restrict__ counts, const float* __restrict__ P, int nviews, int w, int h,
                                                            long long nblk, unsigned* zbuf) {
    const Counts n = load_counts(counts, nv_cap, nf_cap);
    const int lane = threadIdx.x & 63;
    const long long items = nblk * nviews;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int view = (int)(item / nblk);
        const long long f = (item % nblk) * kBlock + threadIdx.x;
        const float* Pv = P + 12 * (size_t)view;
        unsigned* z = zbuf + (size_t)view * h * w;
        Tri t;
        const bool ok = f < n.nf && setup(verts, faces, f, n.nv, Pv, w, h, t);
        const bool big = ok && t.bw * t.bh > kSmallBox;                          // bw * bh <= w * h <= 2^26
        if (ok && !big)
            for (int y = t.y0; y < t.y0 + t.bh; ++y)
                for (int x = t.x0; x < t.x0 + t.bw; ++x) shade(t, x, y, z, w);
        // the wave's larger faces, one after another, 64 pixels at a time (the ballot is the same word in every lane)
        for (u64 m = __ballot(big); m; m &= m - 1) {
            const int src = __ffsll((long long)m) - 1;
            const int bf = __shfl((int)f, src);                                  // f < nf <= 2^31 - 1
            Tri b;
            if (!setup(verts, faces, bf, n.nv, Pv, w, h, b)) continue;         // it passed in lane src: never taken
            const int px = b.bw * b.bh;
            for (int p = lane; p < px; p += 64) shade(b, b.x0 + p % b.bw, b.y0 + p / b.bw, z, w);
        }
    }
}

// A sample is visible iff it is projectable, its nearest pixel lies in the frame and it is no deeper than the map there.
__device__ inline bool visible(const Proj& s, const float* __restrict__ z, int w, int h, float tol1) {
    if (!s.ok) return false;
    const float px = rintf(s.sx), py = rintf(s.sy);
    if (!(px >= 0.0f && px <= (float)(w - 1) && py >= 0.0f && py <= (float)(h - 1))) return false;
    return s.z <= z[(size_t)(int)py * w + (int)px] * tol1;
}

__device__ inline bool in_frame(const Proj& s, int w, int h) {
    return s.sx >= 0.0f && s.sx <= (float)(w - 1) && s.sy >= 0.0f && s.sy <= (float)(h - 1);
}

__global__ __launch_bounds__(kBlock) void tex_view_kernel(const float* __restrict__ verts, const int* __restrict__ faces, int nv_cap, int nf_cap,
                                                          const int* __restrict__ counts, const float* __restrict__ P, int nviews, int w, int h,
                                                          const float* __restrict__ zbuf, float vis_tol, int* __restrict__ face_view,
                                                          float* __restrict__ face_score) {
    const Counts n = load_counts(counts, nv_cap, nf_cap);
    const float tol1 = 1.0f + vis_tol;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long f = (long long)blockIdx.x * kBlock + threadIdx.x; f < n.nf; f += stride) {
        int best = -1;
        float score = 0.0f;
        const float *a, *b, *c;
        if (corners(verts, faces, f, n.nv, a, b, c)) {
            const float ax = a[0], ay = a[1], az = a[2], bx = b[0], by = b[1], bz = b[2], cx = c[0], cy = c[1], cz = c[2];
            const float gx = ((ax + bx) + cx) / 3.0f, gy = ((ay + by) + cy) / 3.0f, gz = ((az + bz) + cz) / 3.0f;
            for (int k = 0; k < nviews; ++k) {
                const float* Pk = P + 12 * (size_t)k;
                const Proj pa = project(Pk, ax, ay, az), pb = project(Pk, bx, by, bz), pc = project(Pk, cx, cy, cz);
                if (!pa.ok || !pb.ok || !pc.ok) continue;
                if (!in_frame(pa, w, h) || !in_frame(pb, w, h) || !in_frame(pc, w, h)) continue;
                const float area2 = (pb.sx - pa.sx) * (pc.sy - pa.sy) - (pb.sy - pa.sy) * (pc.sx - pa.sx);
                if (!(area2 < 0.0f)) continue;
                const float s = -area2;
                if (!(s > score)) continue;                                     // the views come in ascending order: a tie keeps the lower
                const float* z = zbuf + (size_t)k * h * w;
                if (!visible(pa, z, w, h, tol1) || !visible(pb, z, w, h, tol1) || !visible(pc, z, w, h, tol1)) continue;
                if (!visible(project(Pk, gx, gy, gz), z, w, h, tol1)) continue;
                best = k;
                score = s;
            }
        }
        face_view[f] = best;
        face_score[f] = score;
    }
}

__device__ inline float clamp_to(float v, float hi) {                           // NaN -> 0
    v = v >= 0.0f ? v : 0.0f;
    return v <= hi ? v : hi;
}

__global__ __launch_bounds__(kBlock) void tex_fill_kernel(const float* __restrict__ verts, const float* __restrict__ colors,
                                                          const int* __restrict__ faces, int nv_cap, int nf_cap, const int* __restrict__ counts,
                                                          const float* __restrict__ P, const unsigned char* __restrict__ frames, int nviews, int w,
                                                          int h, const int* __restrict__ face_view, int L, int cols, int side,
                                                          unsigned char* __restrict__ atlas) {
    const Counts n = load_counts(counts, nv_cap, nf_cap);
    const int cell = L + kCellExtra;
    const float fl = (float)L;
    const long long texels = (long long)side * side, stride = (long long)gridDim.x * kBlock;
    for (long long t = (long long)blockIdx.x * kBlock + threadIdx.x; t < texels; t += stride) {
        const int tx = (int)(t % side), ty = (int)(t / side);
        const int i = tx % cell, j = ty % cell;
        const long long q = (long long)(ty / cell) * cols + tx / cell;          // < cols^2 <= 2^24
        const int half = i + j <= cell - 1 ? 0 : 1;
        const long long f = 2 * q + half;
        float val[3] = {0.0f, 0.0f, 0.0f};
        const int* tri = faces + 3 * (size_t)f;
        int ia, ib, ic;
        if (f < n.nf && in_range(ia = tri[0], n.nv) && in_range(ib = tri[1], n.nv) && in_range(ic = tri[2], n.nv)) {
            const float u = (float)(half ? cell - 2 - i : i - 1) / fl, v = (float)(half ? cell - 2 - j : j - 1) / fl;
            const float w0 = (1.0f - u) - v;
            const int k = face_view[f];
            if (k >= 0 && k < nviews) {
                const float *a = verts + 3 * (size_t)ia, *b = verts + 3 * (size_t)ib, *c = verts + 3 * (size_t)ic;
                const float x = (w0 * a[0] + u * b[0]) + v * c[0], y = (w0 * a[1] + u * b[1]) + v * c[1], z = (w0 * a[2] + u * b[2]) + v * c[2];
                const Proj s = project(P + 12 * (size_t)k, x, y, z);
                const float sx = clamp_to(s.sx, (float)(w - 1)), sy = clamp_to(s.sy, (float)(h - 1));
                const int x0 = min((int)floorf(sx), w - 2), y0 = min((int)floorf(sy), h - 2);
                const float fx = sx - (float)x0, fy = sy - (float)y0;
                const unsigned char* p0 = frames + 3 * (((size_t)k * h + y0) * w + x0);      // rows y0 and y0 + 1 <= h - 1, x0 + 1 <= w - 1
                const unsigned char* p1 = p0 + 3 * (size_t)w;
                for (int ch = 0; ch < 3; ++ch)
                    val[ch] = (((float)p0[ch] * (1.0f - fx) + (float)p0[3 + ch] * fx) * (1.0f - fy)) +
                              (((float)p1[ch] * (1.0f - fx) + (float)p1[3 + ch] * fx) * fy);
            } else if (colors) {
                const float *ca = colors + 3 * (size_t)ia, *cb = colors + 3 * (size_t)ib, *cc = colors + 3 * (size_t)ic;
                for (int ch = 0; ch < 3; ++ch) val[ch] = (w0 * ca[ch] + u * cb[ch]) + v * cc[ch];
            }
        }
        unsigned char* o = atlas + 3 * (size_t)t;
        o[0] = (unsigned char)clamp_to(rintf(val[0]), 255.0f);
        o[1] = (unsigned char)clamp_to(rintf(val[1]), 255.0f);
        o[2] = (unsigned char)clamp_to(rintf(val[2]), 255.0f);
    }
}

int64_t blocks_of(int64_t n) { return (n + kBlock - 1) / kBlock; }

unsigned grid_of(int64_t blocks) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks, kMaxGrid)); }

// cols of the layout: the smallest integer >= 1 whose square holds ceil(nf / 2) cells.
int64_t cols_of(int64_t nf) {
    const int64_t slots = (nf + 1) / 2;
    int64_t c = (int64_t)std::sqrt((double)slots);
    while (c * c < slots) ++c;
    while (c > 1 && (c - 1) * (c - 1) >= slots) --c;
    return std::max<int64_t>(c, 1);
}

}  // namespace

#define TEX_CHECK_MESH(name)                                                                                                        \
    SFM_CHECK_ARG(nv_cap >= 0 && nf_cap >= 0 && nv_cap <= kMaxCount && nf_cap <= kMaxCount,                                         \
                  name ": nv_cap %lld, nf_cap %lld: each must be in 0..2^31-1", (long long)nv_cap, (long long)nf_cap);             \
    SFM_CHECK_ARG(n >= 1 && n <= kMaxViews, name ": n %d views: must be in 1..65536", n);                                           \
    SFM_CHECK_ARG(w >= 2 && h >= 2 && w <= kMaxPixels && h <= kMaxPixels && w * h <= kMaxPixels,                                    \
                  name ": frame %lld x %lld: w and h must be >= 2 and w * h <= 2^26", (long long)w, (long long)h);                 \
    SFM_CHECK_ARG((nv_cap == 0 || vertices_dev) && (nf_cap == 0 || faces_dev) && P_dev, name ": null required pointer")

extern "C" int sfm_mesh_render_depth(const float* vertices_dev, const int32_t* faces_dev, int64_t nv_cap, int64_t nf_cap,
                                     const int32_t* counts_dev, const float* P_dev, int n, int64_t w, int64_t h, float* zbuf_dev, void* stream) {
    TEX_CHECK_MESH("sfm_mesh_render_depth");
    SFM_CHECK_ARG(zbuf_dev, "sfm_mesh_render_depth: null required pointer");
    hipStream_t s = sfm::as_stream(stream);
    const long long words = (long long)n * w * h, nblk = blocks_of(nf_cap);
    hipLaunchKernelGGL(tex_clear_kernel, dim3(grid_of(blocks_of(words))), dim3(kBlock), 0, s, reinterpret_cast<unsigned*>(zbuf_dev), words);
    SFM_CHECK_LAUNCH();
    if (nf_cap) {
        hipLaunchKernelGGL(tex_raster_kernel, dim3(grid_of(nblk * n)), dim3(kBlock), 0, s, vertices_dev, faces_dev, (int)nv_cap, (int)nf_cap,
                           counts_dev, P_dev, n, (int)w, (int)h, nblk, reinterpret_cast<unsigned*>(zbuf_dev));
        SFM_CHECK_LAUNCH();
    }
    return SFM_OK;
}

extern "C" int sfm_mesh_face_views(const float* vertices_dev, const int32_t* faces_dev, int64_t nv_cap, int64_t nf_cap, const int32_t* counts_dev,
                                   const float* P_dev, int n, int64_t w, int64_t h, const float* zbuf_dev, float vis_tol, int32_t* face_view_dev,
                                   float* face_score_dev, void* stream) {
    TEX_CHECK_MESH("sfm_mesh_face_views");
    SFM_CHECK_ARG(std::isfinite(vis_tol) && vis_tol >= 0.0f, "sfm_mesh_face_views: vis_tol %g must be finite and >= 0", (double)vis_tol);
    SFM_CHECK_ARG(zbuf_dev && (nf_cap == 0 || (face_view_dev && face_score_dev)), "sfm_mesh_face_views: null required pointer");
    if (nf_cap == 0) return SFM_OK;
    hipLaunchKernelGGL(tex_view_kernel, dim3(grid_of(blocks_of(nf_cap))), dim3(kBlock), 0, sfm::as_stream(stream), vertices_dev, faces_dev,
                       (int)nv_cap, (int)nf_cap, counts_dev, P_dev, n, (int)w, (int)h, zbuf_dev, vis_tol, face_view_dev, face_score_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" int sfm_mesh_texture_fill(const float* vertices_dev, const float* colors_dev, const int32_t* faces_dev, int64_t nv_cap, int64_t nf_cap,
                                     const int32_t* counts_dev, const float* P_dev, const uint8_t* frames_dev, int n, int64_t w, int64_t h,
                                     const int32_t* face_view_dev, int texels, int cols, int side, uint8_t* atlas_dev, void* stream) {
    TEX_CHECK_MESH("sfm_mesh_texture_fill");
    SFM_CHECK_ARG(texels >= 1 && texels <= kMaxTexels, "sfm_mesh_texture_fill: texels %d per leg: must be in 1..64", texels);
    const int64_t want_cols = cols_of(nf_cap), want_side = want_cols * (texels + kCellExtra);
    SFM_CHECK_ARG(want_side <= kMaxSide, "sfm_mesh_texture_fill: layout of %lld faces at %d texels: side %lld exceeds 16384", (long long)nf_cap,
                  texels, (long long)want_side);
    SFM_CHECK_ARG(cols == want_cols && side == want_side, "sfm_mesh_texture_fill: layout cols %d, side %d: %lld faces at %d texels give %lld, %lld",
                  cols, side, (long long)nf_cap, texels, (long long)want_cols, (long long)want_side);
    SFM_CHECK_ARG(frames_dev && atlas_dev && (nf_cap == 0 || face_view_dev), "sfm_mesh_texture_fill: null required pointer");
    hipLaunchKernelGGL(tex_fill_kernel, dim3(grid_of(blocks_of((int64_t)side * side))), dim3(kBlock), 0, sfm::as_stream(stream), vertices_dev,
                       colors_dev, faces_dev, (int)nv_cap, (int)nf_cap, counts_dev, P_dev, frames_dev, n, (int)w, (int)h, face_view_dev, texels,
                       cols, side, atlas_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}
