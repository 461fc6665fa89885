// Mesh decimation by vertex clustering, after clean-up and smoothing (include/sfm_hip.h, "MESH-DECIMATE"; docs/mesh.md §9).
//   sfm_mesh_decimate   the vertices of one cell of a regular grid collapse into their mean; faces are renumbered, the ones that
//                       lose a corner are dropped and, on request, so are all but the first of the faces that became equal
// Every sum is an int64 sum of quantised terms and every choice among candidates is an atomic minimum, so the order in which the
// atomics land changes no word; the float32 and float64 operations are the ones the header writes, in its order, compiled without
// contraction.  tests/np_mesh_decimate.py restates the outputs exactly.
//
// Plain form, twelve launches (ten without dedupe), each one lane per vertex, per face or per word:
//   init      table[cell] = INT_MAX, the accumulator rows = 0, the face set = empty
//   key       key[v] = the vertex's cell or -1, atomicMin(table[key], v): the leader of a cell is its smallest usable vertex id
//   sum       each usable vertex adds its quantised row to acc[leader] (8 x int64 = 64 B per row, no-return 8-byte adds)
//   count     leaders per 256-vertex block, the unusable vertices; then a one-workgroup scan
//   vertex    a leader's rank among the leaders is its new id; it writes the mean row
//   map       newid[v] = the new id of v's leader, -1 for an unusable vertex
//   insert    (dedupe) every live face enters an open-addressing set keyed by its rotation-normalised new triple
//   resolve   flag[i] = face i is live and (dedupe) the slot of its class holds i; flags per 256-face block; then a scan
//   face      flagged faces to their rank, renumbered, corner order kept
// The face set.  One int32 word per slot, "empty" or a face index.  A lane claims an empty slot with one atomicCAS; the slot's
// class (the normalised triple of its occupant) is read from the faces array through newid, both read-only in that launch, never
// from a word the claimant has yet to publish.  An arriving face of the same class lowers the slot to its index by atomicMin, one
// of another class probes on: a slot never changes its class, the probe is bounded by the slot count, and no lane waits for another.
// After the launch the slot of a class holds the lowest index of the class whatever the landing order was, although WHICH slot it
// is may differ from run to run.  The kernel boundary is the only synchronisation between workgroups.
#include <algorithm>
#include <climits>
#include <cmath>

#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxGrid = 1 << 16;               // workgroups per launch; the kernels stride over what is left
constexpr int kScanThreads = 1024;
constexpr int64_t kMaxCount = INT32_MAX;
constexpr int64_t kMaxCells = 1ll << 27;
constexpr float kUnit = 1073741824.0f;          // 2^30: the bound of a usable |r|
constexpr float kColourUnit = 65536.0f, kColourMax = 32768.0f;
constexpr int kRow = 8;                         // int64 words per accumulator row: x y z cnt b g r (one spare)
constexpr int kEmpty = -1;

enum Scalar { kUnusable = 0, kDropped = 1, kScalars = 2 };

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

__device__ inline void add64(long long* p, long long v) { atomicAdd(reinterpret_cast<u64*>(p), (u64)v); }

struct Frame {
    float ox, oy, oz, cell, pscale;
    int dx, dy, dz;
};

// The cell of a position and its quantised row; false when the vertex is not usable.
__device__ inline bool locate(const float* __restrict__ p, const Frame& fr, int& key, long long& rx, long long& ry, long long& rz) {
    const double c = (double)fr.cell;
    const double tx = floor(((double)p[0] - (double)fr.ox) / c);
    const double ty = floor(((double)p[1] - (double)fr.oy) / c);
    const double tz = floor(((double)p[2] - (double)fr.oz) / c);
    if (!(tx >= 0.0 && tx < (double)fr.dx) || !(ty >= 0.0 && ty < (double)fr.dy) || !(tz >= 0.0 && tz < (double)fr.dz)) return false;
    const float fx = rintf((p[0] - fr.ox) * fr.pscale), fy = rintf((p[1] - fr.oy) * fr.pscale), fz = rintf((p[2] - fr.oz) * fr.pscale);
    if (!(fabsf(fx) <= kUnit) || !(fabsf(fy) <= kUnit) || !(fabsf(fz) <= kUnit)) return false;
    key = ((int)tz * fr.dy + (int)ty) * fr.dx + (int)tx;                       // < dx * dy * dz <= 2^27
    rx = (long long)fx;
    ry = (long long)fy;
    rz = (long long)fz;
    return true;
}

__device__ inline long long colour_term(float c) { return fabsf(c) <= kColourMax ? (long long)rintf(c * kColourUnit) : 0; }

__global__ __launch_bounds__(kBlock) void dec_init_kernel(int* __restrict__ table, long long cells, long long* __restrict__ acc, long long words,
                                                          int* __restrict__ set, long long slots, int* __restrict__ scal) {
    const long long stride = (long long)gridDim.x * kBlock, first = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (first < kScalars) scal[first] = 0;
    for (long long i = first; i < cells; i += stride) table[i] = INT_MAX;
    for (long long i = first; i < words; i += stride) acc[i] = 0;
    for (long long i = first; i < slots; i += stride) set[i] = kEmpty;
}

__global__ __launch_bounds__(kBlock) void dec_key_kernel(const float* __restrict__ verts, int nv_cap, int nf_cap, const int* __restrict__ counts,
                                                         Frame fr, int* __restrict__ key, int* table) {
    const Counts n = load_counts(counts, nv_cap, nf_cap);
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < n.nv; v += stride) {
        int k = -1;
        long long rx, ry, rz;
        if (locate(verts + 3 * (size_t)v, fr, k, rx, ry, rz)) atomicMin(&table[k], (int)v);
        key[v] = k;
    }
}

__global__ __launch_bounds__(kBlock) void dec_sum_kernel(const float* __restrict__ verts, const float* __restrict__ colors, int nv_cap,
                                                         int nf_cap, const int* __restrict__ counts, Frame fr, const int* __restrict__ key,
                                                         const int* __restrict__ table, long long* acc) {
    const Counts n = load_counts(counts, nv_cap, nf_cap);
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < n.nv; v += stride) {
        const int k = key[v];
        if (k < 0) continue;
        const float* p = verts + 3 * (size_t)v;
        long long* row = acc + kRow * (size_t)table[k];                         // the leader: a usable vertex id <= v
        add64(row + 0, (long long)rintf((p[0] - fr.ox) * fr.pscale));
        add64(row + 1, (long long)rintf((p[1] - fr.oy) * fr.pscale));
        add64(row + 2, (long long)rintf((p[2] - fr.oz) * fr.pscale));
        add64(row + 3, 1);
        if (colors) {
            const float* c = colors + 3 * (size_t)v;
            add64(row + 4, colour_term(c[0]));
            add64(row + 5, colour_term(c[1]));
            add64(row + 6, colour_term(c[2]));
        }
    }
}

__device__ inline bool is_leader(const int* __restrict__ key, const int* __restrict__ table, long long v) {
    const int k = key[v];
    return k >= 0 && table[k] == (int)v;
}

// Leaders per 256-vertex block, and the unusable vertices.
__global__ __launch_bounds__(kBlock) void dec_vertex_count_kernel(int nv_cap, int nf_cap, const int* __restrict__ counts,
                                                                  const int* __restrict__ key, const int* __restrict__ table, long long ncv,
                                                                  int* __restrict__ part_v, int* __restrict__ scal) {
    const Counts n = load_counts(counts, nv_cap, nf_cap);
    int unusable = 0;
    for (long long blk = blockIdx.x; blk < ncv; blk += gridDim.x) {
        const long long v = blk * kBlock + threadIdx.x;
        const bool in = v < n.nv;
        const int lead = __syncthreads_count(in && is_leader(key, table, v));
        unusable += __syncthreads_count(in && key[v] < 0);
        if (threadIdx.x == 0) part_v[blk] = lead;
    }
    if (threadIdx.x == 0 && unusable) atomicAdd(&scal[kUnusable], unusable);
}

// The block counts -> exclusive offsets in place; counts[slot] = their sum; with scal, counts[2..3] = the two scalars.
__global__ __launch_bounds__(kScanThreads) void dec_scan_kernel(int* __restrict__ part, long long n, int slot, const int* __restrict__ scal,
                                                                int* __restrict__ counts) {
    __shared__ int buf[kScanThreads];
    const int tid = threadIdx.x;
    const long long seg = (n + kScanThreads - 1) / kScanThreads;
    const long long lo = min(tid * seg, n), hi = min(lo + seg, n);
    int sum = 0;
    for (long long b = lo; b < hi; ++b) sum += part[b];
    buf[tid] = sum;
    __syncthreads();
    for (int off = 1; off < kScanThreads; off <<= 1) {
        const int add = tid >= off ? buf[tid - off] : 0;
        __syncthreads();
        buf[tid] += add;
        __syncthreads();
    }
    int run = buf[tid] - sum;
    for (long long b = lo; b < hi; ++b) {
        const int v = part[b];
        part[b] = run;
        run += v;
    }
    if (tid == kScanThreads - 1) counts[slot] = buf[tid];
    if (scal && tid < kScalars) counts[2 + tid] = scal[tid];
}

// Rank of this lane among the set flags of the workgroup.
__device__ inline int block_rank(bool flag, int* wsum) {
    const u64 b = __ballot(flag);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) wsum[w] = __popcll(b);
    __syncthreads();
    int off = 0;
    for (int k = 0; k < kWaves; ++k) off += k < w ? wsum[k] : 0;
    __syncthreads();
    return off + __popcll(b & ((1ull << lane) - 1));
}

// Leaders to their rank: the mean row of the cell, the new id left in rank_of[v].
__global__ __launch_bounds__(kBlock) void dec_vertex_kernel(int nv_cap, int nf_cap, const int* __restrict__ counts, Frame fr,
                                                            const int* __restrict__ key, const int* __restrict__ table,
                                                            const long long* __restrict__ acc, long long ncv, const int* __restrict__ part_v,
                                                            int* __restrict__ rank_of, float* __restrict__ out_verts,
                                                            float* __restrict__ out_colors) {
    __shared__ int wsum[kWaves];
    const Counts n = load_counts(counts, nv_cap, nf_cap);
    const double ps = (double)fr.pscale;
    const double o[3] = {(double)fr.ox, (double)fr.oy, (double)fr.oz};
    for (long long blk = blockIdx.x; blk < ncv; blk += gridDim.x) {
        const long long v = blk * kBlock + threadIdx.x;
        const bool lead = v < n.nv && is_leader(key, table, v);
        const int rank = block_rank(lead, wsum);
        if (!lead) continue;
        const size_t id = (size_t)part_v[blk] + rank;                           // < leaders <= nv
        rank_of[v] = (int)id;
        const long long* row = acc + kRow * (size_t)v;
        const double cnt = (double)row[3];                                      // >= 1: the leader itself
        for (int c = 0; c < 3; ++c) out_verts[3 * id + c] = (float)(((double)row[c] / cnt) / ps + o[c]);
        if (out_colors)
            for (int c = 0; c < 3; ++c) out_colors[3 * id + c] = (float)(((double)row[4 + c] / cnt) / 65536.0);
    }
}

__global__ __launch_bounds__(kBlock) void dec_map_kernel(int nv_cap, int nf_cap, const int* __restrict__ counts, const int* __restrict__ key,
                                                         const int* __restrict__ table, const int* __restrict__ rank_of,
                                                         int* __restrict__ newid) {
    const Counts n = load_counts(counts, nv_cap, nf_cap);
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < n.nv; v += stride) {
        const int k = key[v];
        newid[v] = k < 0 ? -1 : rank_of[table[k]];
    }
}

struct Triple {
    int a, b, c;
    __device__ bool operator==(const Triple& o) const { return a == o.a && b == o.b && c == o.c; }
};

// The new ids of face i in corner order; false unless the face is live (valid, three usable corners, three different new ids).
__device__ inline bool live_face(const int* __restrict__ faces, long long i, int nv, const int* __restrict__ newid, Triple& t) {
    const int* f = faces + 3 * (size_t)i;
    const int a = f[0], b = f[1], c = f[2];
    if (!in_range(a, nv) || !in_range(b, nv) || !in_range(c, nv)) return false;
    t.a = newid[a];
    t.b = newid[b];
    t.c = newid[c];
    return t.a >= 0 && t.b >= 0 && t.c >= 0 && t.a != t.b && t.b != t.c && t.a != t.c;
}

// Rotated so that the smallest id comes first (the ids of a live face differ, so there is one such rotation).
__device__ inline Triple normalised(const Triple& t) {
    if (t.a < t.b && t.a < t.c) return t;
    if (t.b < t.c) return Triple{t.b, t.c, t.a};
    return Triple{t.c, t.a, t.b};
}

__device__ inline u64 slot_of(const Triple& t, u64 mask) {
    u64 h = (u64)(unsigned)t.a * 0x9E3779B97F4A7C15ull;
    h ^= (u64)(unsigned)t.b * 0xC2B2AE3D27D4EB4Full;
    h ^= (u64)(unsigned)t.c * 0x165667B19E3779F9ull;
    h ^= h >> 29;
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 32;
    return h & mask;
}

__global__ __launch_bounds__(kBlock) void dec_insert_kernel(const int* __restrict__ faces, int nv_cap, int nf_cap, const int* __restrict__ counts,
                                                            const int* __restrict__ newid, int* set, u64 slots) {
    const Counts n = load_counts(counts, nv_cap, nf_cap);
    const long long stride = (long long)gridDim.x * kBlock;
    const u64 mask = slots - 1;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n.nf; i += stride) {
        Triple t;
        if (!live_face(faces, i, n.nv, newid, t)) continue;
        const Triple mine = normalised(t);
        u64 s = slot_of(mine, mask);
        for (u64 probe = 0; probe < slots; ++probe, s = (s + 1) & mask) {
            const int cur = atomicCAS(&set[s], kEmpty, (int)i);
            if (cur == kEmpty) break;                                           // claimed: the slot's class is mine from now on
            Triple other;                                                       // cur: a live face among the first nf
            live_face(faces, cur, n.nv, newid, other);
            if (normalised(other) == mine) {
                if (cur > (int)i) atomicMin(&set[s], (int)i);
                break;
            }
        }
    }
}

// flag[i] = face i is output; flags per 256-face block; the live faces dropped as duplicates.
__global__ __launch_bounds__(kBlock) void dec_resolve_kernel(const int* __restrict__ faces, int nv_cap, int nf_cap, const int* __restrict__ counts,
                                                             const int* __restrict__ newid, const int* __restrict__ set, u64 slots, int dedupe,
                                                             long long ncf, unsigned char* __restrict__ flag, int* __restrict__ part_f,
                                                             int* __restrict__ scal) {
    const Counts n = load_counts(counts, nv_cap, nf_cap);
    const u64 mask = slots - 1;
    int dropped = 0;
    for (long long blk = blockIdx.x; blk < ncf; blk += gridDim.x) {
        const long long i = blk * kBlock + threadIdx.x;
        Triple t;
        const bool live = i < n.nf && live_face(faces, i, n.nv, newid, t);
        bool out = live;
        if (live && dedupe) {
            const Triple mine = normalised(t);
            u64 s = slot_of(mine, mask);
            out = false;
            for (u64 probe = 0; probe < slots; ++probe, s = (s + 1) & mask) {
                const int cur = set[s];
                if (cur == kEmpty) break;                                       // not a state the insert launch leaves
                Triple other;
                live_face(faces, cur, n.nv, newid, other);
                if (normalised(other) == mine) {
                    out = cur == (int)i;
                    break;
                }
            }
        }
        if (i < nf_cap) flag[i] = out;
        const int kept = __syncthreads_count(out);
        dropped += __syncthreads_count(live && !out);
        if (threadIdx.x == 0) part_f[blk] = kept;
    }
    if (threadIdx.x == 0 && dropped) atomicAdd(&scal[kDropped], dropped);
}

__global__ __launch_bounds__(kBlock) void dec_face_kernel(const int* __restrict__ faces, int nf_cap, const int* __restrict__ newid,
                                                          const unsigned char* __restrict__ flag, long long ncf, const int* __restrict__ part_f,
                                                          int* __restrict__ out_faces) {
    __shared__ int wsum[kWaves];
    for (long long blk = blockIdx.x; blk < ncf; blk += gridDim.x) {
        const long long i = blk * kBlock + threadIdx.x;
        const bool out = i < nf_cap && flag[i];
        const int rank = block_rank(out, wsum);
        if (!out) continue;
        const size_t id = (size_t)part_f[blk] + rank;                           // < faces out <= nf
        const int* f = faces + 3 * (size_t)i;                                   // an output face is live: its indices name vertices
        out_faces[3 * id + 0] = newid[f[0]];
        out_faces[3 * id + 1] = newid[f[1]];
        out_faces[3 * id + 2] = newid[f[2]];
    }
}

bool sizes_ok(int64_t nv, int64_t nf, const int32_t* dims) {
    if (!(nv >= 0 && nf >= 0 && nv <= kMaxCount && nf <= kMaxCount) || !dims) return false;
    int64_t cells = 1;
    for (int c = 0; c < 3; ++c) {
        if (dims[c] < 1) return false;
        cells *= dims[c];                                                       // each factor < 2^31, the running product <= 2^27
        if (cells > kMaxCells) return false;
    }
    return true;
}

int64_t blocks_of(int64_t n) { return (n + kBlock - 1) / kBlock; }

unsigned grid_of(int64_t blocks) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks, kMaxGrid)); }

// The smallest power of two >= 2 * nf (at least 2).
uint64_t slots_of(int64_t nf) {
    uint64_t s = 2;
    while (s < 2 * (uint64_t)nf) s <<= 1;
    return s;
}

struct DecimateWs {
    long long* acc;                              // [nv][8] int64, rows indexed by the leader's vertex id
    int *table, *key, *rank_of, *newid, *part_v, *part_f, *set, *scal;
    unsigned char* flag;                         // [nf]
    size_t bytes;
};

DecimateWs carve(void* base, int64_t nv, int64_t nf, const int32_t* dims) {
    sfm::Carver c(base);
    DecimateWs w{};
    w.acc = c.take<long long>(kRow * (size_t)nv);
    w.table = c.take<int>((size_t)dims[0] * dims[1] * dims[2]);
    w.key = c.take<int>(nv);
    w.rank_of = c.take<int>(nv);
    w.newid = c.take<int>(nv);
    w.part_v = c.take<int>(blocks_of(nv));
    w.part_f = c.take<int>(blocks_of(nf));
    w.set = c.take<int>(slots_of(nf));
    w.scal = c.take<int>(kScalars);
    w.flag = c.take<unsigned char>(nf);
    w.bytes = c.used();
    return w;
}

}  // namespace

extern "C" size_t sfm_mesh_decimate_ws_bytes(int64_t nv_cap, int64_t nf_cap, const int32_t dims[3]) {
    return sizes_ok(nv_cap, nf_cap, dims) ? carve(nullptr, nv_cap, nf_cap, dims).bytes : 0;
}

extern "C" int sfm_mesh_decimate(const float* vertices_dev, const float* colors_dev, const int32_t* faces_dev, int64_t nv_cap, int64_t nf_cap,
                                 const int32_t* counts_dev, const float* origin_host, float cell, const int32_t* dims_host, float pscale,
                                 int dedupe, float* out_vertices_dev, float* out_colors_dev, int32_t* out_faces_dev, int32_t* out_counts_dev,
                                 void* ws_dev, size_t ws_bytes, void* stream) {
    SFM_CHECK_ARG(nv_cap >= 0 && nf_cap >= 0 && nv_cap <= kMaxCount && nf_cap <= kMaxCount,
                  "sfm_mesh_decimate: nv_cap %lld, nf_cap %lld: each must be in 0..2^31-1", (long long)nv_cap, (long long)nf_cap);
    SFM_CHECK_ARG(origin_host && dims_host && out_counts_dev && ws_dev, "sfm_mesh_decimate: null required pointer");
    SFM_CHECK_ARG(sizes_ok(nv_cap, nf_cap, dims_host), "sfm_mesh_decimate: dims %d x %d x %d: each must be >= 1 and the product <= 2^27",
                  dims_host[0], dims_host[1], dims_host[2]);
    SFM_CHECK_ARG(std::isfinite(cell) && cell > 0.0f, "sfm_mesh_decimate: cell %g must be finite and positive", (double)cell);
    SFM_CHECK_ARG(std::isfinite(pscale) && pscale > 0.0f, "sfm_mesh_decimate: pscale %g must be finite and positive", (double)pscale);
    SFM_CHECK_ARG(std::isfinite(origin_host[0]) && std::isfinite(origin_host[1]) && std::isfinite(origin_host[2]),
                  "sfm_mesh_decimate: the origin is not finite");
    SFM_CHECK_ARG(dedupe == 0 || dedupe == 1, "sfm_mesh_decimate: dedupe %d must be 0 or 1", dedupe);
    SFM_CHECK_ARG((nv_cap == 0 || (vertices_dev && out_vertices_dev)) && (nf_cap == 0 || (faces_dev && out_faces_dev)),
                  "sfm_mesh_decimate: null required pointer");
    SFM_CHECK_ARG(!colors_dev == !out_colors_dev, "sfm_mesh_decimate: colours in and colours out go together");
    SFM_CHECK_ARG((nv_cap == 0 || vertices_dev != out_vertices_dev) && (!colors_dev || colors_dev != out_colors_dev) &&
                      (nf_cap == 0 || faces_dev != out_faces_dev) && counts_dev != out_counts_dev,
                  "sfm_mesh_decimate: every output must be distinct from the inputs");
    const DecimateWs ws = carve(ws_dev, nv_cap, nf_cap, dims_host);
    SFM_CHECK_ARG(ws_bytes >= ws.bytes, "sfm_mesh_decimate: workspace %zu bytes < %zu", ws_bytes, ws.bytes);
    hipStream_t s = sfm::as_stream(stream);
    const int v = (int)nv_cap, f = (int)nf_cap;
    const long long ncv = blocks_of(nv_cap), ncf = blocks_of(nf_cap);
    const long long cells = (long long)dims_host[0] * dims_host[1] * dims_host[2], words = (long long)kRow * v;
    const uint64_t slots = slots_of(nf_cap);
    const long long fill_slots = dedupe ? (long long)slots : 0;
    const Frame fr{origin_host[0], origin_host[1], origin_host[2], cell, pscale, dims_host[0], dims_host[1], dims_host[2]};
    const dim3 block(kBlock), grid_v(grid_of(ncv)), grid_f(grid_of(ncf));
    hipLaunchKernelGGL(dec_init_kernel, dim3(grid_of(blocks_of(std::max(std::max(cells, words), fill_slots)))), block, 0, s, ws.table, cells,
                       ws.acc, words, ws.set, fill_slots, ws.scal);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(dec_key_kernel, grid_v, block, 0, s, vertices_dev, v, f, counts_dev, fr, ws.key, ws.table);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(dec_sum_kernel, grid_v, block, 0, s, vertices_dev, colors_dev, v, f, counts_dev, fr, ws.key, ws.table, ws.acc);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(dec_vertex_count_kernel, grid_v, block, 0, s, v, f, counts_dev, ws.key, ws.table, ncv, ws.part_v, ws.scal);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(dec_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, ws.part_v, ncv, 0, (const int*)nullptr, out_counts_dev);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(dec_vertex_kernel, grid_v, block, 0, s, v, f, counts_dev, fr, ws.key, ws.table, ws.acc, ncv, ws.part_v, ws.rank_of,
                       out_vertices_dev, out_colors_dev);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(dec_map_kernel, grid_v, block, 0, s, v, f, counts_dev, ws.key, ws.table, ws.rank_of, ws.newid);
    SFM_CHECK_LAUNCH();
    if (dedupe && f) {
        hipLaunchKernelGGL(dec_insert_kernel, grid_f, block, 0, s, faces_dev, v, f, counts_dev, ws.newid, ws.set, (u64)slots);
        SFM_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(dec_resolve_kernel, grid_f, block, 0, s, faces_dev, v, f, counts_dev, ws.newid, ws.set, (u64)slots, dedupe, ncf, ws.flag,
                       ws.part_f, ws.scal);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(dec_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, ws.part_f, ncf, 1, ws.scal, out_counts_dev);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(dec_face_kernel, grid_f, block, 0, s, faces_dev, f, ws.newid, ws.flag, ncf, ws.part_f, out_faces_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}
