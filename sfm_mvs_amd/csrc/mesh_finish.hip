// Mesh finishing after extraction and clean-up: vertex normals and Taubin smoothing of a triangle mesh
// (include/sfm_hip.h, "MESH-FINISH"; docs/mesh.md §8).
//   sfm_mesh_normals   normal[v] = the normalised equal-weight sum of the unit normals of the faces that name v
//   sfm_mesh_smooth    nsteps face-umbrella Laplacian steps p' = p + factor * (mean of the neighbours - p)
// Every sum over faces is an int64 sum of quantised terms, so the order in which the atomics land changes no word; the float32
// and float64 operations are the ones the header writes, in its order, compiled without contraction.  tests/np_mesh_finish.py
// restates both exactly.
//
// Plain form: one accumulator row of four int64 per vertex (x, y, z and, for smoothing, the neighbour count; 32 bytes, one
// aligned segment), a face kernel with one lane per face and no-return 8-byte atomic adds (9 for normals, 12 for a smoothing
// step), and a vertex kernel that reads the row, writes the result and zeroes the row for the next step: 1 + 2 launches for
// normals, 1 + 2 * nsteps for smoothing.  The counts are read from the device by every kernel, so the launches follow
// sfm_mesh_clean on the stream with no host wait; the grids are sized by the capacities.  Every loop runs over a range fixed
// at launch and the kernel boundary is the only synchronisation between workgroups.
#include <algorithm>
#include <climits>
#include <cmath>

#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxGrid = 1 << 16;               // workgroups per launch; the kernels stride over what is left
constexpr int kMaxSteps = 64;
constexpr int64_t kMaxCount = INT32_MAX;
constexpr float kUnit = 1073741824.0f;          // 2^30: the quantum of a unit normal's coordinate, and the bound of a usable |r|

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

// The three indices of face i; false when one of them names no vertex.
__device__ inline bool load_face(const int* __restrict__ faces, long long i, int nv, int& a, int& b, int& c) {
    const int* f = faces + 3 * (size_t)i;
    a = f[0];
    b = f[1];
    c = f[2];
    return in_range(a, nv) && in_range(b, nv) && in_range(c, nv);
}

__device__ inline void add64(long long* p, long long v) { atomicAdd(reinterpret_cast<u64*>(p), (u64)v); }

// acc[0 .. 4*nv_cap) = 0 (all rows: the counts may not be on the device yet when the caller sizes the launch).
__global__ __launch_bounds__(kBlock) void finish_zero_kernel(long long* __restrict__ acc, long long words) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < words; i += stride) acc[i] = 0;
}

// ---- normals --------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock) void normals_face_kernel(const float* __restrict__ verts, const int* __restrict__ faces, int nv_cap,
                                                              int nf_cap, const int* __restrict__ counts, long long* acc) {
    const Counts n = load_counts(counts, nv_cap, nf_cap);
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n.nf; i += stride) {
        int ia, ib, ic;
        if (!load_face(faces, i, n.nv, ia, ib, ic)) continue;
        const float* a = verts + 3 * (size_t)ia;
        const float* b = verts + 3 * (size_t)ib;
        const float* c = verts + 3 * (size_t)ic;
        const float ax = a[0], ay = a[1], az = a[2];
        const float e1x = b[0] - ax, e1y = b[1] - ay, e1z = b[2] - az;
        const float e2x = c[0] - ax, e2y = c[1] - ay, e2z = c[2] - az;
        const float nx = e1y * e2z - e1z * e2y;
        const float ny = e1z * e2x - e1x * e2z;
        const float nz = e1x * e2y - e1y * e2x;
        const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
        if (!(len > 0.0f) || !(len <= 3.402823466e38f)) continue;              // zero, NaN or infinite: no contribution
        const long long qx = (long long)rintf((nx / len) * kUnit);
        const long long qy = (long long)rintf((ny / len) * kUnit);
        const long long qz = (long long)rintf((nz / len) * kUnit);
        long long* ra = acc + 4 * (size_t)ia;
        long long* rb = acc + 4 * (size_t)ib;
        long long* rc = acc + 4 * (size_t)ic;
        add64(ra + 0, qx), add64(ra + 1, qy), add64(ra + 2, qz);
        add64(rb + 0, qx), add64(rb + 1, qy), add64(rb + 2, qz);
        add64(rc + 0, qx), add64(rc + 1, qy), add64(rc + 2, qz);
    }
}

__global__ __launch_bounds__(kBlock) void normals_vertex_kernel(const long long* __restrict__ acc, int nv_cap, int nf_cap,
                                                                const int* __restrict__ counts, float* __restrict__ normals) {
    const Counts n = load_counts(counts, nv_cap, nf_cap);
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < n.nv; v += stride) {
        const long long* r = acc + 4 * (size_t)v;
        const double dx = (double)r[0], dy = (double)r[1], dz = (double)r[2];
        const double L = sqrt((dx * dx + dy * dy) + dz * dz);
        float* o = normals + 3 * (size_t)v;
        const bool zero = L == 0.0;
        o[0] = zero ? 0.0f : (float)(dx / L);
        o[1] = zero ? 0.0f : (float)(dy / L);
        o[2] = zero ? 0.0f : (float)(dz / L);
    }
}

// ---- smoothing ------------------------------------------------------------------------------------------------------------

struct Frame {
    float ox, oy, oz, pscale;
};

// r = rintf((p - o) * pscale) per coordinate; false when the vertex is not usable (one |r| above 2^30, or NaN).
__device__ inline bool quantise(const float* __restrict__ p, const Frame& fr, long long& rx, long long& ry, long long& rz) {
    const float fx = rintf((p[0] - fr.ox) * fr.pscale), fy = rintf((p[1] - fr.oy) * fr.pscale), fz = rintf((p[2] - fr.oz) * fr.pscale);
    if (!(fabsf(fx) <= kUnit) || !(fabsf(fy) <= kUnit) || !(fabsf(fz) <= kUnit)) return false;
    rx = (long long)fx;
    ry = (long long)fy;
    rz = (long long)fz;
    return true;
}

__global__ __launch_bounds__(kBlock) void smooth_face_kernel(const float* __restrict__ verts, const int* __restrict__ faces, int nv_cap,
                                                             int nf_cap, const int* __restrict__ counts, Frame fr, long long* acc) {
    const Counts n = load_counts(counts, nv_cap, nf_cap);
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n.nf; i += stride) {
        int id[3];
        if (!load_face(faces, i, n.nv, id[0], id[1], id[2])) continue;
        long long r[3][3] = {};
        long long use[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const bool ok = quantise(verts + 3 * (size_t)id[k], fr, r[k][0], r[k][1], r[k][2]);
            use[k] = ok;
            if (!ok) r[k][0] = r[k][1] = r[k][2] = 0;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {                                          // corner k receives its two other corners
            const int j1 = (k + 1) % 3, j2 = (k + 2) % 3;
            const long long cnt = use[j1] + use[j2];
            if (!cnt) continue;
            long long* row = acc + 4 * (size_t)id[k];
            add64(row + 0, r[j1][0] + r[j2][0]);
            add64(row + 1, r[j1][1] + r[j2][1]);
            add64(row + 2, r[j1][2] + r[j2][2]);
            add64(row + 3, cnt);
        }
    }
}

// One step's update; the accumulator row is left zero for the next step.
__global__ __launch_bounds__(kBlock) void smooth_vertex_kernel(const int* __restrict__ src, long long* __restrict__ acc, int nv_cap, int nf_cap,
                                                               const int* __restrict__ counts, Frame fr, float factor, int* __restrict__ dst) {
    const Counts n = load_counts(counts, nv_cap, nf_cap);
    const long long stride = (long long)gridDim.x * kBlock;
    const double ps = (double)fr.pscale, f = (double)factor;
    const double o[3] = {(double)fr.ox, (double)fr.oy, (double)fr.oz};
    for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < n.nv; v += stride) {
        long long* row = acc + 4 * (size_t)v;
        const long long a[3] = {row[0], row[1], row[2]}, cnt = row[3];
        row[0] = row[1] = row[2] = row[3] = 0;
        const int w[3] = {src[3 * (size_t)v], src[3 * (size_t)v + 1], src[3 * (size_t)v + 2]};
        const float p[3] = {__int_as_float(w[0]), __int_as_float(w[1]), __int_as_float(w[2])};
        long long rx, ry, rz;
        const bool moves = cnt > 0 && quantise(p, fr, rx, ry, rz);
        for (int c = 0; c < 3; ++c) {
            int out = w[c];                                                     // kept bit for bit
            if (moves) {
                const double m = ((double)a[c] / (double)cnt) / ps + o[c];
                out = __float_as_int((float)((double)p[c] + f * (m - (double)p[c])));
            }
            dst[3 * (size_t)v + c] = out;
        }
    }
}

__global__ __launch_bounds__(kBlock) void copy_rows_kernel(const int* __restrict__ src, int nv_cap, int nf_cap, const int* __restrict__ counts,
                                                           int* __restrict__ dst) {
    const Counts n = load_counts(counts, nv_cap, nf_cap);
    const long long words = 3ll * n.nv, stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < words; i += stride) dst[i] = src[i];
}

bool sizes_ok(int64_t nv, int64_t nf) { return nv >= 0 && nf >= 0 && nv <= kMaxCount && nf <= kMaxCount; }

unsigned grid_of(int64_t items) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + kBlock - 1) / kBlock, kMaxGrid)); }

struct FinishWs {
    long long* acc;                              // [nv][4] int64
    float *ping, *pong;                          // [nv][3] each (smoothing only)
    size_t bytes;
};

FinishWs carve(void* base, int64_t nv, bool smooth) {
    sfm::Carver c(base);
    FinishWs w{};
    w.acc = c.take<long long>(4 * (size_t)nv);
    if (smooth) {
        w.ping = c.take<float>(3 * (size_t)nv);
        w.pong = c.take<float>(3 * (size_t)nv);
    }
    w.bytes = c.used();
    return w;
}

}  // namespace

extern "C" size_t sfm_mesh_normals_ws_bytes(int64_t nv_cap, int64_t nf_cap) {
    return sizes_ok(nv_cap, nf_cap) ? carve(nullptr, nv_cap, false).bytes : 0;
}

extern "C" size_t sfm_mesh_smooth_ws_bytes(int64_t nv_cap, int64_t nf_cap) {
    return sizes_ok(nv_cap, nf_cap) ? carve(nullptr, nv_cap, true).bytes : 0;
}

extern "C" int sfm_mesh_normals(const float* vertices_dev, const int32_t* faces_dev, int64_t nv_cap, int64_t nf_cap, const int32_t* counts_dev,
                                float* normals_dev, void* ws_dev, size_t ws_bytes, void* stream) {
    SFM_CHECK_ARG(sizes_ok(nv_cap, nf_cap), "sfm_mesh_normals: nv_cap %lld, nf_cap %lld: each must be in 0..2^31-1", (long long)nv_cap,
                  (long long)nf_cap);
    SFM_CHECK_ARG((nv_cap == 0 || (vertices_dev && normals_dev && ws_dev)) && (nf_cap == 0 || faces_dev), "sfm_mesh_normals: null required pointer");
    SFM_CHECK_ARG(nv_cap == 0 || vertices_dev != normals_dev, "sfm_mesh_normals: the output must be distinct from the input");
    const FinishWs ws = carve(ws_dev, nv_cap, false);
    SFM_CHECK_ARG(ws_bytes >= ws.bytes, "sfm_mesh_normals: workspace %zu bytes < %zu", ws_bytes, ws.bytes);
    if (nv_cap == 0) return SFM_OK;                                             // no vertex: every face is invalid, no row to write
    hipStream_t s = sfm::as_stream(stream);
    const int v = (int)nv_cap, f = (int)nf_cap;
    const dim3 block(kBlock);
    hipLaunchKernelGGL(finish_zero_kernel, dim3(grid_of(4 * nv_cap)), block, 0, s, ws.acc, 4ll * v);
    SFM_CHECK_LAUNCH();
    if (f) {
        hipLaunchKernelGGL(normals_face_kernel, dim3(grid_of(nf_cap)), block, 0, s, vertices_dev, faces_dev, v, f, counts_dev, ws.acc);
        SFM_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(normals_vertex_kernel, dim3(grid_of(nv_cap)), block, 0, s, ws.acc, v, f, counts_dev, normals_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" int sfm_mesh_smooth(const float* vertices_dev, const int32_t* faces_dev, int64_t nv_cap, int64_t nf_cap, const int32_t* counts_dev,
                               int nsteps, const float* factors_host, const float* origin_host, float pscale, float* out_vertices_dev,
                               void* ws_dev, size_t ws_bytes, void* stream) {
    SFM_CHECK_ARG(sizes_ok(nv_cap, nf_cap), "sfm_mesh_smooth: nv_cap %lld, nf_cap %lld: each must be in 0..2^31-1", (long long)nv_cap,
                  (long long)nf_cap);
    SFM_CHECK_ARG(nsteps >= 0 && nsteps <= kMaxSteps, "sfm_mesh_smooth: nsteps %d must be in 0..%d", nsteps, kMaxSteps);
    SFM_CHECK_ARG(origin_host && (nsteps == 0 || factors_host) && (nv_cap == 0 || (vertices_dev && out_vertices_dev && ws_dev)) &&
                      (nf_cap == 0 || faces_dev),
                  "sfm_mesh_smooth: null required pointer");
    for (int k = 0; k < nsteps; ++k)
        SFM_CHECK_ARG(std::isfinite(factors_host[k]), "sfm_mesh_smooth: factor %d is not finite", k);
    SFM_CHECK_ARG(std::isfinite(origin_host[0]) && std::isfinite(origin_host[1]) && std::isfinite(origin_host[2]),
                  "sfm_mesh_smooth: the origin is not finite");
    SFM_CHECK_ARG(std::isfinite(pscale) && pscale > 0.0f, "sfm_mesh_smooth: pscale %g must be finite and positive", (double)pscale);
    SFM_CHECK_ARG(nv_cap == 0 || vertices_dev != out_vertices_dev, "sfm_mesh_smooth: the output must be distinct from the input");
    const FinishWs ws = carve(ws_dev, nv_cap, true);
    SFM_CHECK_ARG(ws_bytes >= ws.bytes, "sfm_mesh_smooth: workspace %zu bytes < %zu", ws_bytes, ws.bytes);
    if (nv_cap == 0) return SFM_OK;
    hipStream_t s = sfm::as_stream(stream);
    const int v = (int)nv_cap, f = (int)nf_cap;
    const dim3 block(kBlock), grid_v(grid_of(nv_cap)), grid_f(grid_of(nf_cap));
    if (nsteps == 0) {
        hipLaunchKernelGGL(copy_rows_kernel, dim3(grid_of(3 * nv_cap)), block, 0, s, reinterpret_cast<const int*>(vertices_dev), v, f, counts_dev,
                           reinterpret_cast<int*>(out_vertices_dev));
        SFM_CHECK_LAUNCH();
        return SFM_OK;
    }
    const Frame fr{origin_host[0], origin_host[1], origin_host[2], pscale};
    hipLaunchKernelGGL(finish_zero_kernel, dim3(grid_of(4 * nv_cap)), block, 0, s, ws.acc, 4ll * v);
    SFM_CHECK_LAUNCH();
    const float* src = vertices_dev;
    for (int k = 0; k < nsteps; ++k) {
        float* dst = k == nsteps - 1 ? out_vertices_dev : (k & 1) ? ws.pong : ws.ping;
        if (f) {
            hipLaunchKernelGGL(smooth_face_kernel, grid_f, block, 0, s, src, faces_dev, v, f, counts_dev, fr, ws.acc);
            SFM_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL(smooth_vertex_kernel, grid_v, block, 0, s, reinterpret_cast<const int*>(src), ws.acc, v, f, counts_dev, fr,
                           factors_host[k], reinterpret_cast<int*>(dst));
        SFM_CHECK_LAUNCH();
        src = dst;
    }
    return SFM_OK;
}
