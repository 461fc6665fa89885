// A surface from the MVS depth maps: volumetric fusion into a truncated signed distance field and its zero set by marching
// tetrahedra (include/sfm_hip.h, "MESH"; docs/mesh.md).
//   sfm_tsdf_integrate   voxel-parallel: one lane per lattice point, the loop over views inside the kernel, no atomics
//   sfm_mesh_count       crossing edges and triangles of the field -> two int32 totals on the device
//   sfm_mesh_extract     the welded, oriented triangle mesh, in the order the header specifies
// Every arithmetic step is a correctly rounded float32 operation in the order the header writes it (no FMA: the Makefile passes
// -ffp-contract=off), so that tests/np_mesh.py restates the kernels bit for bit.
//
// tsdf_kernel: a workgroup owns a 64 x 4 tile of one z slice (a wave is one row of 64 points along x: the sum read-modify-writes
// are 256-byte coalesced rows, and neighbouring points gather neighbouring pixels).  The per-view matrix is read at a
// wave-uniform address (scalar loads).  The running sums stay in registers over all views and are written back once.
//
// Extraction is two passes over 256-point blocks in linear order: a count (crossing edges, triangles of the cube at each
// point), an int32 scan of the block totals by one workgroup, then the emitting kernels recompute the same per-point counts,
// scan them inside the block and write at block offset + local offset.  The vertex pass also leaves each point's first vertex
// id and its 7 crossing flags in the workspace, from which the triangle pass names the vertices of the neighbouring points.
#include <algorithm>
#include <cmath>

#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kTsdfX = 64, kTsdfY = 4;          // tsdf tile: 64 points along x (one wave) x 4 rows
constexpr int64_t kMaxPoints = int64_t(1) << 27;
constexpr int kScanThreads = 1024;

// ---- the marching-tetrahedra case table, generated from the header's rules at compile time ------------------------------
// Corner / direction bitmask: bit 0 = +x, bit 1 = +y, bit 2 = +z.  A cube corner with offset bitmask c is cube corner c.
struct TetTable {
    uint8_t corner[6][4];                       // offset bitmask of tetrahedron corner 0..3
    uint8_t ntri[6][16];                        // triangles per inside-mask case (bit q = corner q inside)
    uint8_t tri[6][16][2][3][2];                // per triangle vertex: the edge's corners (a < b, tetrahedron numbering)
};

constexpr int kDirIndex[8] = {-1, 0, 1, 3, 2, 4, 5, 6};   // direction bitmask -> 0..6 (+x, +y, +z, +x+y, +x+z, +y+z, +x+y+z)
constexpr int kDirMask[7] = {1, 2, 4, 3, 5, 6, 7};

constexpr TetTable make_tet_table() {
    TetTable T{};
    const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};   // xyz xzy yxz yzx zxy zyx
    for (int t = 0; t < 6; ++t) {
        const int c1 = 1 << perm[t][0], c2 = c1 | (1 << perm[t][1]);
        T.corner[t][0] = 0;
        T.corner[t][1] = (uint8_t)c1;
        T.corner[t][2] = (uint8_t)c2;
        T.corner[t][3] = 7;
        for (int cs = 0; cs < 16; ++cs) {
            int in[4] = {}, out[4] = {}, nin = 0, nout = 0;
            for (int q = 0; q < 4; ++q) {
                if (cs >> q & 1) in[nin++] = q;
                else out[nout++] = q;
            }
            int e[2][3][2] = {};
            int n = 0;
            if (nin == 1 || nout == 1) {
                const int c = nin == 1 ? in[0] : out[0];
                int m = 0;
                for (int o = 0; o < 4; ++o)
                    if (o != c) {
                        e[0][m][0] = c < o ? c : o;
                        e[0][m][1] = c < o ? o : c;
                        ++m;
                    }
                n = 1;
            } else if (nin == 2) {
                const int pr[2][3][2] = {{{in[0], out[0]}, {in[0], out[1]}, {in[1], out[1]}}, {{in[0], out[0]}, {in[1], out[1]}, {in[1], out[0]}}};
                for (int r = 0; r < 2; ++r)
                    for (int q = 0; q < 3; ++q) {
                        const int a = pr[r][q][0], b = pr[r][q][1];
                        e[r][q][0] = a < b ? a : b;
                        e[r][q][1] = a < b ? b : a;
                    }
                n = 2;
            }
            // winding: the right-hand normal of the edge midpoints (doubled integer coordinates) against inside -> outside
            int g[3] = {};
            for (int ax = 0; ax < 3; ++ax) {
                int si = 0, so = 0;
                for (int q = 0; q < nin; ++q) si += T.corner[t][in[q]] >> ax & 1;
                for (int q = 0; q < nout; ++q) so += T.corner[t][out[q]] >> ax & 1;
                g[ax] = nin * so - nout * si;
            }
            for (int r = 0; r < n; ++r) {
                int m[3][3] = {};
                for (int q = 0; q < 3; ++q)
                    for (int ax = 0; ax < 3; ++ax)
                        m[q][ax] = (T.corner[t][e[r][q][0]] >> ax & 1) + (T.corner[t][e[r][q][1]] >> ax & 1);
                const int u[3] = {m[1][0] - m[0][0], m[1][1] - m[0][1], m[1][2] - m[0][2]};
                const int v[3] = {m[2][0] - m[0][0], m[2][1] - m[0][1], m[2][2] - m[0][2]};
                const int nrm[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
                const bool flip = nrm[0] * g[0] + nrm[1] * g[1] + nrm[2] * g[2] < 0;
                for (int q = 0; q < 3; ++q) {
                    const int src = flip && q > 0 ? 3 - q : q;
                    T.tri[t][cs][r][q][0] = (uint8_t)e[r][src][0];
                    T.tri[t][cs][r][q][1] = (uint8_t)e[r][src][1];
                }
            }
            T.ntri[t][cs] = (uint8_t)n;
        }
    }
    return T;
}

__constant__ const TetTable kTets = make_tet_table();

// ---- TSDF integration ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tsdf_kernel(const float* __restrict__ depth, const uint8_t* __restrict__ mask,
                                                   const uint8_t* __restrict__ bgr, const float* __restrict__ P, int nview, int w, int h,
                                                   float ox, float oy, float oz, float voxel, int nx, int ny, int nz, float trunc,
                                                   float* __restrict__ S, float* __restrict__ W, float* __restrict__ CWc, int tiles_x,
                                                   int tiles_y, long long ntiles) {
    const size_t frame = (size_t)w * h;
    const float wmax = (float)(w - 1), hmax = (float)(h - 1);
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int tx = (int)(tile % tiles_x);
        const long long rest = tile / tiles_x;
        const int ty = (int)(rest % tiles_y), k = (int)(rest / tiles_y);
        const int i = tx * kTsdfX + (int)(threadIdx.x % kTsdfX), j = ty * kTsdfY + (int)(threadIdx.x / kTsdfX);
        if (i >= nx || j >= ny) continue;
        const float x = ox + (float)i * voxel, y = oy + (float)j * voxel, z = oz + (float)k * voxel;
        const size_t o = ((size_t)k * ny + j) * nx + i;
        float s = S[o], wt = W[o];
        float cb = 0.0f, cg = 0.0f, cr = 0.0f, cw = 0.0f;
        if (CWc) {
            cb = CWc[4 * o + 0];
            cg = CWc[4 * o + 1];
            cr = CWc[4 * o + 2];
            cw = CWc[4 * o + 3];
        }
        for (int v = 0; v < nview; ++v) {
            const float* m = P + 12 * v;
            const float p2 = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
            if (!(p2 > 0.0f)) continue;
            const float p0 = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
            const float p1 = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
            const float u = floorf(p0 / p2 + 0.5f), t = floorf(p1 / p2 + 0.5f);
            if (!(u >= 0.0f && u <= wmax && t >= 0.0f && t <= hmax)) continue;
            const size_t px = (size_t)v * frame + (size_t)(int)t * w + (int)u;
            const float d = depth[px];
            if (!(d > 0.0f)) continue;
            if (mask && mask[px] == 0) continue;
            const float sdf = d - p2;
            if (sdf < -trunc) continue;
            const float f = fminf(sdf, trunc) / trunc;
            s = s + f;
            wt = wt + 1.0f;
            if (CWc && sdf <= trunc) {
                cb = cb + (float)bgr[3 * px + 0];
                cg = cg + (float)bgr[3 * px + 1];
                cr = cr + (float)bgr[3 * px + 2];
                cw = cw + 1.0f;
            }
        }
        S[o] = s;
        W[o] = wt;
        if (CWc) {
            CWc[4 * o + 0] = cb;
            CWc[4 * o + 1] = cg;
            CWc[4 * o + 2] = cr;
            CWc[4 * o + 3] = cw;
        }
    }
}

// ---- marching tetrahedra ---------------------------------------------------------------------------------------------
struct Grid {
    int nx, ny, nz;
    long long n;                                // nx*ny*nz
};

struct Cell {                                   // the 8 corners of the cube at a point (those in the grid)
    float F[8];
    int known, inside;                          // bit c: corner c is known / inside
};

__device__ inline Cell load_cell(const float* __restrict__ S, const float* __restrict__ W, const Grid g, int i, int j, int k, float w_min) {
    Cell c;
    c.known = 0;
    c.inside = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int dx = q & 1, dy = q >> 1 & 1, dz = q >> 2;
        c.F[q] = 0.0f;
        if (i + dx < g.nx && j + dy < g.ny && k + dz < g.nz) {
            const size_t o = ((size_t)(k + dz) * g.ny + (j + dy)) * g.nx + (i + dx);
            const float wt = W[o];
            if (wt >= w_min) {
                const float F = S[o] / wt;
                c.F[q] = F;
                c.known |= 1 << q;
                if (F < 0.0f) c.inside |= 1 << q;
            }
        }
    }
    return c;
}

__device__ inline int edge_flags(const Cell& c) {   // bit d (direction index): edge (point, d) crosses
    int f = 0;
    if (!(c.known & 1)) return 0;
#pragma unroll
    for (int d = 0; d < 7; ++d) {
        const int m = kDirMask[d];
        if ((c.known >> m & 1) && ((c.inside ^ (c.inside >> m)) & 1)) f |= 1 << d;
    }
    return f;
}

__device__ inline int cube_triangles(const Cell& c, bool is_cube) {
    if (!is_cube) return 0;
    int n = 0;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        int all = 1, cs = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int cq = kTets.corner[t][q];
            all &= c.known >> cq & 1;
            cs |= (c.inside >> cq & 1) << q;
        }
        if (all) n += kTets.ntri[t][cs];
    }
    return n;
}

__device__ inline void point_of(long long p, const Grid g, int& i, int& j, int& k) {
    i = (int)(p % g.nx);
    const long long r = p / g.nx;
    j = (int)(r % g.ny);
    k = (int)(r / g.ny);
}

// Exclusive scan of one int per lane over the workgroup (kBlock lanes, LDS Hillis-Steele, deterministic); returns the total.
__device__ inline int block_exclusive_scan(int v, int* buf, int& total) {
    const int tid = threadIdx.x;
    buf[tid] = v;
    __syncthreads();
    for (int off = 1; off < kBlock; off <<= 1) {
        const int add = tid >= off ? buf[tid - off] : 0;
        __syncthreads();
        buf[tid] += add;
        __syncthreads();
    }
    const int incl = buf[tid];
    total = buf[kBlock - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(kBlock) void mesh_count_kernel(const float* __restrict__ S, const float* __restrict__ W, Grid g, float w_min,
                                                            int* __restrict__ part_v, int* __restrict__ part_t) {
    __shared__ int buf[kBlock];
    const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
    int nv = 0, nt = 0;
    if (p < g.n) {
        int i, j, k;
        point_of(p, g, i, j, k);
        const Cell c = load_cell(S, W, g, i, j, k, w_min);
        nv = __popc(edge_flags(c));
        nt = cube_triangles(c, i < g.nx - 1 && j < g.ny - 1 && k < g.nz - 1);
    }
    int tv, tt;
    block_exclusive_scan(nv, buf, tv);
    block_exclusive_scan(nt, buf, tt);
    if (threadIdx.x == 0) {
        part_v[blockIdx.x] = tv;
        part_t[blockIdx.x] = tt;
    }
}

// One workgroup: the block totals -> exclusive block offsets (in place), the two grand totals -> totals[0..1].
__global__ __launch_bounds__(kScanThreads) void mesh_scan_kernel(int* __restrict__ part_v, int* __restrict__ part_t, int nb,
                                                                 int* __restrict__ totals) {
    __shared__ int bv[kScanThreads], bt[kScanThreads];
    const int tid = threadIdx.x;
    const int seg = (nb + kScanThreads - 1) / kScanThreads;
    const int lo = min(tid * seg, nb), hi = min(lo + seg, nb);
    int sv = 0, st = 0;
    for (int b = lo; b < hi; ++b) {
        sv += part_v[b];
        st += part_t[b];
    }
    bv[tid] = sv;
    bt[tid] = st;
    __syncthreads();
    for (int off = 1; off < kScanThreads; off <<= 1) {
        const int av = tid >= off ? bv[tid - off] : 0, at = tid >= off ? bt[tid - off] : 0;
        __syncthreads();
        bv[tid] += av;
        bt[tid] += at;
        __syncthreads();
    }
    int ov = bv[tid] - sv, ot = bt[tid] - st;
    for (int b = lo; b < hi; ++b) {
        const int v = part_v[b], t = part_t[b];
        part_v[b] = ov;
        part_t[b] = ot;
        ov += v;
        ot += t;
    }
    if (tid == kScanThreads - 1) {
        totals[0] = bv[tid];
        totals[1] = bt[tid];
    }
}

__global__ __launch_bounds__(kBlock) void mesh_vertex_kernel(const float* __restrict__ S, const float* __restrict__ W,
                                                             const float* __restrict__ CWc, Grid g, float w_min, float ox, float oy,
                                                             float oz, float voxel, const int* __restrict__ part_v, long long max_vertices,
                                                             float* __restrict__ verts, float* __restrict__ colors,
                                                             int* __restrict__ vbase, uint8_t* __restrict__ flags_out) {
    __shared__ int buf[kBlock];
    const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
    int i = 0, j = 0, k = 0, fl = 0;
    Cell c{};
    if (p < g.n) {
        point_of(p, g, i, j, k);
        c = load_cell(S, W, g, i, j, k, w_min);
        fl = edge_flags(c);
    }
    int total;
    const int local = block_exclusive_scan(__popc(fl), buf, total);
    if (p >= g.n) return;
    const int base = part_v[blockIdx.x] + local;
    vbase[p] = base;
    flags_out[p] = (uint8_t)fl;
    if (!fl) return;
    const float xa = ox + (float)i * voxel, ya = oy + (float)j * voxel, za = oz + (float)k * voxel;
    float ca[3] = {0.0f, 0.0f, 0.0f};
    if (colors) {
        const float* q = CWc + 4 * (size_t)p;
        if (q[3] != 0.0f) {
            ca[0] = q[0] / q[3];
            ca[1] = q[1] / q[3];
            ca[2] = q[2] / q[3];
        }
    }
    int id = base;
    for (int d = 0; d < 7; ++d) {
        if (!(fl >> d & 1)) continue;
        const int m = kDirMask[d], dx = m & 1, dy = m >> 1 & 1, dz = m >> 2;
        const float Fa = c.F[0], Fb = c.F[m];
        const float t = Fa / (Fa - Fb);
        const float xb = ox + (float)(i + dx) * voxel, yb = oy + (float)(j + dy) * voxel, zb = oz + (float)(k + dz) * voxel;
        if (id < max_vertices) {
            verts[3 * (size_t)id + 0] = xa + t * (xb - xa);
            verts[3 * (size_t)id + 1] = ya + t * (yb - ya);
            verts[3 * (size_t)id + 2] = za + t * (zb - za);
            if (colors) {
                const size_t ob = ((size_t)(k + dz) * g.ny + (j + dy)) * g.nx + (i + dx);
                const float* q = CWc + 4 * ob;
                float cb[3] = {0.0f, 0.0f, 0.0f};
                if (q[3] != 0.0f) {
                    cb[0] = q[0] / q[3];
                    cb[1] = q[1] / q[3];
                    cb[2] = q[2] / q[3];
                }
                for (int ch = 0; ch < 3; ++ch) colors[3 * (size_t)id + ch] = ca[ch] + t * (cb[ch] - ca[ch]);
            }
        }
        ++id;
    }
}

__global__ __launch_bounds__(kBlock) void mesh_triangle_kernel(const float* __restrict__ S, const float* __restrict__ W, Grid g, float w_min,
                                                               const int* __restrict__ part_t, const int* __restrict__ vbase,
                                                               const uint8_t* __restrict__ flags, long long max_faces,
                                                               int* __restrict__ faces) {
    __shared__ int buf[kBlock];
    const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
    int i = 0, j = 0, k = 0, nt = 0;
    Cell c{};
    bool is_cube = false;
    if (p < g.n) {
        point_of(p, g, i, j, k);
        is_cube = i < g.nx - 1 && j < g.ny - 1 && k < g.nz - 1;
        if (is_cube) {
            c = load_cell(S, W, g, i, j, k, w_min);
            nt = cube_triangles(c, true);
        }
    }
    int total;
    const int local = block_exclusive_scan(nt, buf, total);
    if (!nt) return;
    long long tri = (long long)part_t[blockIdx.x] + local;
    const long long plane = (long long)g.nx * g.ny;
    for (int t = 0; t < 6; ++t) {
        int all = 1, cs = 0;
        for (int q = 0; q < 4; ++q) {
            const int cq = kTets.corner[t][q];
            all &= c.known >> cq & 1;
            cs |= (c.inside >> cq & 1) << q;
        }
        if (!all) continue;
        for (int r = 0; r < kTets.ntri[t][cs]; ++r) {
            int ids[3];
            for (int q = 0; q < 3; ++q) {
                const int a = kTets.corner[t][kTets.tri[t][cs][r][q][0]], b = kTets.corner[t][kTets.tri[t][cs][r][q][1]];
                const long long pa = p + (a & 1) + (long long)(a >> 1 & 1) * g.nx + (long long)(a >> 2) * plane;
                const int d = kDirIndex[b & ~a];
                ids[q] = vbase[pa] + __popc(flags[pa] & ((1 << d) - 1));
            }
            if (tri < max_faces) {
                faces[3 * (size_t)tri + 0] = ids[0];
                faces[3 * (size_t)tri + 1] = ids[1];
                faces[3 * (size_t)tri + 2] = ids[2];
            }
            ++tri;
        }
    }
}

bool grid_ok(int64_t nx, int64_t ny, int64_t nz) {
    return nx >= 2 && ny >= 2 && nz >= 2 && nx <= kMaxPoints && ny <= kMaxPoints && nz <= kMaxPoints && nx * ny <= kMaxPoints &&
           nx * ny * nz <= kMaxPoints;
}

// Workspace: the block totals (scanned in place into block offsets) and the two grand totals; for extraction also each
// point's first vertex id and crossing flags.  base = nullptr only sizes it.
struct MeshWs {
    int *part_v, *part_t, *tot, *vbase;
    uint8_t* flags;
    size_t bytes;
};

MeshWs carve(void* base, int64_t n, bool extract) {
    sfm::Carver c(base);
    const int64_t nb = (n + kBlock - 1) / kBlock;
    MeshWs m{};
    m.part_v = c.take<int>(nb);
    m.part_t = c.take<int>(nb);
    m.tot = c.take<int>(2);
    if (extract) {
        m.vbase = c.take<int>(n);
        m.flags = c.take<uint8_t>(n);
    }
    m.bytes = c.used();
    return m;
}

// The count pass and the scan, shared by both entry points.
int count_and_scan(const float* S_dev, const float* W_dev, const Grid g, float w_min, const MeshWs& ws, int32_t* totals_dev,
                   hipStream_t s) {
    const int nb = (int)((g.n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(mesh_count_kernel, dim3(nb), dim3(kBlock), 0, s, S_dev, W_dev, g, w_min, ws.part_v, ws.part_t);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(mesh_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, ws.part_v, ws.part_t, nb, totals_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

}  // namespace

#define SFM_CHECK_GRID(fn, nx, ny, nz)                                                                                           \
    SFM_CHECK_ARG(grid_ok(nx, ny, nz), fn ": %lld x %lld x %lld grid: each side must be >= 2 and nx*ny*nz <= 2^27", (long long)(nx), \
                  (long long)(ny), (long long)(nz))

extern "C" int sfm_tsdf_integrate(const float* depth_dev, const uint8_t* mask_dev, const uint8_t* bgr_dev, const float* P_dev, int nview,
                                  int64_t w, int64_t h, const float* origin_host, float voxel, int64_t nx, int64_t ny, int64_t nz,
                                  float trunc, float* S_dev, float* W_dev, float* CWc_dev, void* stream) {
    SFM_CHECK_ARG(nview >= 0, "sfm_tsdf_integrate: nview %d is negative", nview);
    SFM_CHECK_ARG(w >= 1 && h >= 1 && w < (1 << 15) && h < (1 << 15), "sfm_tsdf_integrate: %lld x %lld frame: each side must be in 1..32767",
                  (long long)w, (long long)h);
    SFM_CHECK_GRID("sfm_tsdf_integrate", nx, ny, nz);
    SFM_CHECK_ARG(voxel > 0.0f && voxel < INFINITY, "sfm_tsdf_integrate: voxel must be positive and finite");
    SFM_CHECK_ARG(trunc > 0.0f && trunc < INFINITY, "sfm_tsdf_integrate: trunc must be positive and finite");
    SFM_CHECK_ARG(origin_host && S_dev && W_dev && (nview == 0 || (depth_dev && P_dev)), "sfm_tsdf_integrate: null required pointer");
    SFM_CHECK_ARG(!CWc_dev || bgr_dev || nview == 0, "sfm_tsdf_integrate: colour sums need bgr_dev");
    for (int a = 0; a < 3; ++a) SFM_CHECK_ARG(std::isfinite(origin_host[a]), "sfm_tsdf_integrate: origin must be finite");
    if (nview == 0) return SFM_OK;
    const int tiles_x = (int)((nx + kTsdfX - 1) / kTsdfX), tiles_y = (int)((ny + kTsdfY - 1) / kTsdfY);
    const long long ntiles = (long long)tiles_x * tiles_y * nz;
    const unsigned grid = (unsigned)std::min<long long>(ntiles, 1 << 20);
    hipLaunchKernelGGL(tsdf_kernel, dim3(grid), dim3(kTsdfX * kTsdfY), 0, sfm::as_stream(stream), depth_dev, mask_dev,
                       CWc_dev ? bgr_dev : nullptr, P_dev, nview, (int)w, (int)h, origin_host[0], origin_host[1], origin_host[2], voxel,
                       (int)nx, (int)ny, (int)nz, trunc, S_dev, W_dev, CWc_dev, tiles_x, tiles_y, ntiles);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" size_t sfm_mesh_count_ws_bytes(int64_t nx, int64_t ny, int64_t nz) {
    return grid_ok(nx, ny, nz) ? carve(nullptr, nx * ny * nz, false).bytes : 0;
}

extern "C" size_t sfm_mesh_extract_ws_bytes(int64_t nx, int64_t ny, int64_t nz) {
    return grid_ok(nx, ny, nz) ? carve(nullptr, nx * ny * nz, true).bytes : 0;
}

extern "C" int sfm_mesh_count(const float* S_dev, const float* W_dev, int64_t nx, int64_t ny, int64_t nz, float w_min, int32_t* counts_dev,
                              void* ws_dev, size_t ws_bytes, void* stream) {
    SFM_CHECK_GRID("sfm_mesh_count", nx, ny, nz);
    SFM_CHECK_ARG(w_min >= 1.0f && w_min < INFINITY, "sfm_mesh_count: w_min must be finite and >= 1");
    SFM_CHECK_ARG(S_dev && W_dev && counts_dev && ws_dev, "sfm_mesh_count: null required pointer");
    const MeshWs ws = carve(ws_dev, nx * ny * nz, false);
    if (ws_bytes < ws.bytes) {
        sfm::set_error("sfm_mesh_count: workspace %zu bytes < %zu", ws_bytes, ws.bytes);
        return SFM_ERR_WORKSPACE;
    }
    const Grid g{(int)nx, (int)ny, (int)nz, (long long)(nx * ny * nz)};
    return count_and_scan(S_dev, W_dev, g, w_min, ws, counts_dev, sfm::as_stream(stream));
}

extern "C" int sfm_mesh_extract(const float* S_dev, const float* W_dev, const float* CWc_dev, const float* origin_host, float voxel, int64_t nx,
                                int64_t ny, int64_t nz, float w_min, int64_t max_vertices, int64_t max_faces, float* vertices_dev,
                                float* colors_dev, int32_t* faces_dev, void* ws_dev, size_t ws_bytes, void* stream) {
    SFM_CHECK_GRID("sfm_mesh_extract", nx, ny, nz);
    SFM_CHECK_ARG(w_min >= 1.0f && w_min < INFINITY, "sfm_mesh_extract: w_min must be finite and >= 1");
    SFM_CHECK_ARG(voxel > 0.0f && voxel < INFINITY, "sfm_mesh_extract: voxel must be positive and finite");
    SFM_CHECK_ARG(max_vertices >= 0 && max_faces >= 0, "sfm_mesh_extract: negative capacity");
    SFM_CHECK_ARG(S_dev && W_dev && origin_host && ws_dev && (max_vertices == 0 || vertices_dev) && (max_faces == 0 || faces_dev),
                  "sfm_mesh_extract: null required pointer");
    SFM_CHECK_ARG(!colors_dev || CWc_dev, "sfm_mesh_extract: colours need CWc_dev");
    for (int a = 0; a < 3; ++a) SFM_CHECK_ARG(std::isfinite(origin_host[a]), "sfm_mesh_extract: origin must be finite");
    const MeshWs ws = carve(ws_dev, nx * ny * nz, true);
    if (ws_bytes < ws.bytes) {
        sfm::set_error("sfm_mesh_extract: workspace %zu bytes < %zu", ws_bytes, ws.bytes);
        return SFM_ERR_WORKSPACE;
    }
    hipStream_t s = sfm::as_stream(stream);
    const Grid g{(int)nx, (int)ny, (int)nz, (long long)(nx * ny * nz)};
    const int nb = (int)((g.n + kBlock - 1) / kBlock);
    const int rc = count_and_scan(S_dev, W_dev, g, w_min, ws, ws.tot, s);
    if (rc != SFM_OK) return rc;
    hipLaunchKernelGGL(mesh_vertex_kernel, dim3(nb), dim3(kBlock), 0, s, S_dev, W_dev, colors_dev ? CWc_dev : nullptr, g, w_min,
                       origin_host[0], origin_host[1], origin_host[2], voxel, ws.part_v, (long long)max_vertices, vertices_dev, colors_dev,
                       ws.vbase, ws.flags);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(mesh_triangle_kernel, dim3(nb), dim3(kBlock), 0, s, S_dev, W_dev, g, w_min, ws.part_t, ws.vbase, ws.flags,
                       (long long)max_faces, faces_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}
