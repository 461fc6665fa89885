// Mesh clean-up after extraction: connected components of a triangle mesh and the removal of the small ones
// (include/sfm_hip.h, "MESH-CLEAN"; docs/mesh.md §7).
//   sfm_mesh_components   label[v] = the smallest vertex id of v's component, by min-label hooking and pointer jumping
//   sfm_mesh_clean        faces per component, the keep rule, and the order-preserving compaction of vertices and faces
// Everything is int32 arithmetic or a bit-for-bit copy; tests/np_mesh_clean.py restates it exactly.
//
// Labelling.  One kernel per round over nf + nv items: a face lowers the labels of its three vertices and of their three current
// labels to the smallest of the three (atomicMin); a vertex follows label[label[..]] for at most kJumpHops hops and lowers its own
// label to where it got (atomicMin too: a face of the same launch may lower it meanwhile, and a plain store could raise it
// again).  Labels only ever fall and always name a vertex of the same component, so every interleaving is a valid state and the
// only fixed point is the component minimum.  A round that lowers nothing leaves flag[r] = 0, and the kernel of round r + 1
// returns at once on flag[r] == 0: `rounds` launches go onto the stream and nobody waits.  The kernel boundary is the only
// synchronisation between workgroups.
//
// Cleaning.  faces_of[label] by one atomicAdd per distinct label of a wave (usually one: most faces share a component); the
// largest count by atomicMax and, among the roots that reach it, the lowest label by atomicMin, a launch apart; then keep flags,
// per-block counts, a one-workgroup int32 scan of each of the two count arrays, and the two gathers, which recompute the flags and
// rank them inside the block by ballot.  Every loop runs over a range fixed at launch.
#include <algorithm>
#include <climits>

#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxGrid = 1 << 16;               // workgroups per launch; the kernels stride over what is left
constexpr int kCountGrid = 512;                 // workgroups of the kernels that end in atomics on one address: two per CU
constexpr int kMaxRounds = 1024;
constexpr int kJumpHops = 4;                    // hop cap of the pointer chase; the next round picks up the rest
constexpr int kScanThreads = 1024;
constexpr int64_t kMaxCount = INT32_MAX;

enum Scalar { kBestCount = 0, kBestLabel = 1, kComponents = 2, kComponentsKept = 3, kScalars = 4 };

__device__ inline int load_relaxed(const int* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

__device__ inline bool in_range(int a, int nv) { return (unsigned)a < (unsigned)nv; }

// The three indices of face i; false when one of them names no vertex.
__device__ inline bool load_face(const int* __restrict__ faces, long long i, int nv, int& a, int& b, int& c) {
    const int* f = faces + 3 * (size_t)i;
    a = f[0];
    b = f[1];
    c = f[2];
    return in_range(a, nv) && in_range(b, nv) && in_range(c, nv);
}

__global__ __launch_bounds__(kBlock) void cc_init_kernel(int* __restrict__ labels, int nv, int resume, int* __restrict__ flags, int nflags) {
    const long long stride = (long long)gridDim.x * kBlock, first = (long long)blockIdx.x * kBlock + threadIdx.x;
    for (long long i = first; i < nflags; i += stride) flags[i] = i == 0;      // "round 0 changed something": round 1 runs
    if (resume) return;
    for (long long i = first; i < nv; i += stride) labels[i] = (int)i;
}

// Lowers labels[x] to m; true when that changed it.
__device__ inline bool lower(int* labels, int x, int m) { return atomicMin(&labels[x], m) > m; }

__global__ __launch_bounds__(kBlock) void cc_round_kernel(const int* __restrict__ faces, int nv, int nf, int* labels,
                                                          const int* __restrict__ prev_flag, int* __restrict__ flag) {
    if (*prev_flag == 0) return;                                                // the round before changed nothing: converged
    const long long n = (long long)nf + nv, stride = (long long)gridDim.x * kBlock;
    int changed = 0;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        if (i < nf) {                                                           // hook
            int a, b, c;
            if (!load_face(faces, i, nv, a, b, c)) continue;
            const int la = load_relaxed(labels + a), lb = load_relaxed(labels + b), lc = load_relaxed(labels + c);
            if (!in_range(la, nv) || !in_range(lb, nv) || !in_range(lc, nv)) continue;   // not a state this entry point leaves
            const int m = min(la, min(lb, lc));
            if (la > m) changed |= (int)lower(labels, a, m) | (int)lower(labels, la, m);
            if (lb > m) changed |= (int)lower(labels, b, m) | (int)lower(labels, lb, m);
            if (lc > m) changed |= (int)lower(labels, c, m) | (int)lower(labels, lc, m);
        } else {                                                                // jump
            const int v = (int)(i - nf);
            const int p = load_relaxed(labels + v);
            int q = p;
            for (int hop = 0; hop < kJumpHops && in_range(q, nv); ++hop) {
                const int next = load_relaxed(labels + q);                      // q is a label: a vertex id below nv
                if (next == q) break;
                q = next;
            }
            if (q < p && q >= 0) changed |= (int)lower(labels, v, q);
        }
    }
    if (__syncthreads_or(changed) && threadIdx.x == 0) *flag = 1;
}

__global__ __launch_bounds__(kScanThreads) void cc_status_kernel(const int* __restrict__ flags, int rounds, int* __restrict__ status) {
    const int r = threadIdx.x + 1;
    const int total = __syncthreads_count(r <= rounds && flags[r <= rounds ? r : 0] != 0);
    if (threadIdx.x == 0) {
        status[0] = flags[rounds] == 0;
        status[1] = total;
    }
}

// ---- cleaning -------------------------------------------------------------------------------------------------------------

__device__ inline int wave_sum(int v) {
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ inline int wave_max(int v) {
    for (int off = 32; off; off >>= 1) v = max(v, __shfl_xor(v, off));
    return v;
}
__device__ inline int wave_min(int v) {
    for (int off = 32; off; off >>= 1) v = min(v, __shfl_xor(v, off));
    return v;
}

__global__ __launch_bounds__(kBlock) void clean_init_kernel(int* __restrict__ faces_of, int nv, int* __restrict__ scal) {
    const long long stride = (long long)gridDim.x * kBlock, first = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (first < kScalars) scal[first] = first == kBestLabel ? INT_MAX : 0;
    for (long long i = first; i < nv; i += stride) faces_of[i] = 0;
}

// faces_of[label of the face's first vertex] += 1 per valid face.  A wave peels its distinct labels off one by one (usually there is
// one: most faces share a component) and carries one label's count over its iterations (the one with the larger count when two
// meet), so the component most faces belong to costs about one atomic per wave, not one per 64 faces: the launch is kept to
// kCountGrid workgroups for that.
__global__ __launch_bounds__(kBlock) void clean_face_count_kernel(const int* __restrict__ faces, int nv, int nf, const int* __restrict__ labels,
                                                                  int* __restrict__ faces_of) {
    const long long stride = (long long)gridDim.x * kBlock;
    const int lane = threadIdx.x & 63;
    int run_label = -1, run_count = 0;                                                     // uniform over the wave
    for (long long base = (long long)blockIdx.x * kBlock; base < nf; base += stride) {     // uniform over the workgroup
        const long long i = base + threadIdx.x;
        int l = -1, a, b, c;
        if (i < nf && load_face(faces, i, nv, a, b, c)) {
            l = labels[a];
            if (!in_range(l, nv)) l = -1;
        }
        unsigned long long todo = __ballot(l >= 0);
        for (int it = 0; it < 64 && todo; ++it) {
            const int cur = __shfl(l, __ffsll((long long)todo) - 1);
            const unsigned long long same = __ballot(l == cur) & todo;
            const int n = __popcll(same);
            todo &= ~same;
            if (cur == run_label) {
                run_count += n;
            } else if (n > run_count) {                                                    // the larger count stays in the register
                if (run_count && lane == 0) atomicAdd(&faces_of[run_label], run_count);
                run_label = cur;
                run_count = n;
            } else if (lane == 0) {
                atomicAdd(&faces_of[cur], n);
            }
        }
    }
    if (run_count && lane == 0) atomicAdd(&faces_of[run_label], run_count);
}

// Components (roots: label[v] == v) and the largest face count among them.
__global__ __launch_bounds__(kBlock) void clean_stats_kernel(const int* __restrict__ labels, int nv, const int* __restrict__ faces_of,
                                                             int* __restrict__ scal) {
    __shared__ int sroots[kWaves], sbest[kWaves];
    const long long stride = (long long)gridDim.x * kBlock;
    int roots = 0, best = 0;
    for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < nv; v += stride)
        if (labels[v] == (int)v) {
            ++roots;
            best = max(best, faces_of[v]);
        }
    roots = wave_sum(roots);
    best = wave_max(best);
    if ((threadIdx.x & 63) == 0) {
        sroots[threadIdx.x >> 6] = roots;
        sbest[threadIdx.x >> 6] = best;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kWaves; ++w) {
            roots += sroots[w];
            best = max(best, sbest[w]);
        }
        if (roots) atomicAdd(&scal[kComponents], roots);
        if (best) atomicMax(&scal[kBestCount], best);
    }
}

// The lowest root among those with the largest face count.
__global__ __launch_bounds__(kBlock) void clean_best_label_kernel(const int* __restrict__ labels, int nv, const int* __restrict__ faces_of,
                                                                  int* __restrict__ scal) {
    __shared__ int slow[kWaves];
    const long long stride = (long long)gridDim.x * kBlock;
    const int best = scal[kBestCount];
    int low = INT_MAX;
    for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < nv; v += stride)
        if (labels[v] == (int)v && faces_of[v] == best) low = min(low, (int)v);
    low = wave_min(low);
    if ((threadIdx.x & 63) == 0) slow[threadIdx.x >> 6] = low;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kWaves; ++w) low = min(low, slow[w]);
        if (low != INT_MAX) atomicMin(&scal[kBestLabel], low);
    }
}

struct Keep {
    const int* labels;
    const int* faces_of;
    long long min_faces;
    int nv, largest_only, best_label;
    // Is the component with label l kept?  (A label that names no vertex keeps nothing: labels are the caller's.)
    __device__ bool label(int l) const {
        if (!in_range(l, nv)) return false;
        return (long long)faces_of[l] >= min_faces && (!largest_only || l == best_label);
    }
};

// Rank of this lane among the set flags of the workgroup, and their number.
__device__ inline int block_rank(bool flag, int* wsum, int& total) {
    const unsigned long long b = __ballot(flag);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) wsum[w] = __popcll(b);
    __syncthreads();
    int off = 0;
    total = 0;
    for (int k = 0; k < kWaves; ++k) {
        off += k < w ? wsum[k] : 0;
        total += wsum[k];
    }
    __syncthreads();
    return off + __popcll(b & ((1ull << lane) - 1));
}

// Kept vertices per 256-vertex block (blocks 0..ncv-1), kept faces per 256-face block (blocks ncv..ncv+ncf-1), kept components.
__global__ __launch_bounds__(kBlock) void clean_flag_count_kernel(const int* __restrict__ faces, int nv, int nf, const int* __restrict__ labels,
                                                                  const int* __restrict__ faces_of, long long min_faces, int largest_only,
                                                                  long long ncv, long long ncf, int* __restrict__ part_v,
                                                                  int* __restrict__ part_f, int* __restrict__ scal) {
    const Keep keep{labels, faces_of, min_faces, nv, largest_only, scal[kBestLabel]};
    int kept_roots = 0;
    for (long long blk = blockIdx.x; blk < ncv + ncf; blk += gridDim.x) {
        if (blk < ncv) {
            const long long v = blk * kBlock + threadIdx.x;
            bool k = false, root = false;
            if (v < nv) {
                const int l = labels[v];
                k = keep.label(l);
                root = k && l == (int)v;
            }
            const int n = __syncthreads_count(k);
            kept_roots += __syncthreads_count(root);
            if (threadIdx.x == 0) part_v[blk] = n;
        } else {
            const long long i = (blk - ncv) * kBlock + threadIdx.x;
            int a, b, c;
            const bool k = i < nf && load_face(faces, i, nv, a, b, c) && keep.label(labels[a]);
            const int n = __syncthreads_count(k);
            if (threadIdx.x == 0) part_f[blk - ncv] = n;
        }
    }
    if (threadIdx.x == 0 && kept_roots) atomicAdd(&scal[kComponentsKept], kept_roots);
}

// Workgroup 0: the vertex block counts -> exclusive offsets in place, counts[0] = kept vertices, counts[2] = components;
// workgroup 1: the same for faces, counts[1] and counts[3] = components kept.
__global__ __launch_bounds__(kScanThreads) void clean_scan_kernel(int* __restrict__ part_v, long long ncv, int* __restrict__ part_f,
                                                                  long long ncf, const int* __restrict__ scal, int* __restrict__ counts) {
    __shared__ int buf[kScanThreads];
    int* part = blockIdx.x ? part_f : part_v;
    const long long n = blockIdx.x ? ncf : ncv;
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
    if (tid == kScanThreads - 1) counts[blockIdx.x] = buf[tid];
    if (tid == 0) counts[2 + blockIdx.x] = scal[blockIdx.x ? kComponentsKept : kComponents];
}

// Kept vertices to their rank: rows copied as int32 words (NaN payloads survive), the new id left in remap[v].
__global__ __launch_bounds__(kBlock) void clean_vertex_kernel(const int* __restrict__ verts, const int* __restrict__ colors, int nv,
                                                              const int* __restrict__ labels, const int* __restrict__ faces_of,
                                                              long long min_faces, int largest_only, const int* __restrict__ scal,
                                                              long long ncv, const int* __restrict__ part_v, int* __restrict__ remap,
                                                              int* __restrict__ out_verts, int* __restrict__ out_colors) {
    __shared__ int wsum[kWaves];
    const Keep keep{labels, faces_of, min_faces, nv, largest_only, scal[kBestLabel]};
    for (long long blk = blockIdx.x; blk < ncv; blk += gridDim.x) {
        const long long v = blk * kBlock + threadIdx.x;
        const bool k = v < nv && keep.label(labels[v]);
        int total;
        const int rank = block_rank(k, wsum, total);
        if (!k) continue;
        const size_t id = (size_t)part_v[blk] + rank;                           // < kept vertices <= nv
        remap[v] = (int)id;
        for (int ch = 0; ch < 3; ++ch) out_verts[3 * id + ch] = verts[3 * (size_t)v + ch];
        if (colors)
            for (int ch = 0; ch < 3; ++ch) out_colors[3 * id + ch] = colors[3 * (size_t)v + ch];
    }
}

__global__ __launch_bounds__(kBlock) void clean_face_kernel(const int* __restrict__ faces, int nv, int nf, const int* __restrict__ labels,
                                                            const int* __restrict__ faces_of, long long min_faces, int largest_only,
                                                            const int* __restrict__ scal, long long ncf, const int* __restrict__ part_f,
                                                            const int* __restrict__ remap, int* __restrict__ out_faces) {
    __shared__ int wsum[kWaves];
    const Keep keep{labels, faces_of, min_faces, nv, largest_only, scal[kBestLabel]};
    for (long long blk = blockIdx.x; blk < ncf; blk += gridDim.x) {
        const long long i = blk * kBlock + threadIdx.x;
        int a = 0, b = 0, c = 0;
        const bool k = i < nf && load_face(faces, i, nv, a, b, c) && keep.label(labels[a]);
        int total;
        const int rank = block_rank(k, wsum, total);
        if (!k) continue;
        const size_t id = (size_t)part_f[blk] + rank;                           // < kept faces <= nf
        out_faces[3 * id + 0] = remap[a];
        out_faces[3 * id + 1] = remap[b];
        out_faces[3 * id + 2] = remap[c];
    }
}

bool sizes_ok(int64_t nv, int64_t nf) { return nv >= 0 && nf >= 0 && nv <= kMaxCount && nf <= kMaxCount; }

int64_t blocks_of(int64_t n) { return (n + kBlock - 1) / kBlock; }

unsigned grid_of(int64_t blocks) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks, kMaxGrid)); }

struct ComponentsWs {
    int* flags;                                  // [kMaxRounds + 1]: flags[r] = round r lowered a label; flags[0] = 1
    size_t bytes;
};

ComponentsWs carve_components(void* base) {
    sfm::Carver c(base);
    ComponentsWs w{};
    w.flags = c.take<int>(kMaxRounds + 1);
    w.bytes = c.used();
    return w;
}

struct CleanWs {
    int *faces_of, *remap, *part_v, *part_f, *scal;
    size_t bytes;
};

CleanWs carve_clean(void* base, int64_t nv, int64_t nf) {
    sfm::Carver c(base);
    CleanWs w{};
    w.faces_of = c.take<int>(nv);
    w.remap = c.take<int>(nv);
    w.part_v = c.take<int>(blocks_of(nv));
    w.part_f = c.take<int>(blocks_of(nf));
    w.scal = c.take<int>(kScalars);
    w.bytes = c.used();
    return w;
}

}  // namespace

extern "C" size_t sfm_mesh_components_ws_bytes(int64_t nv, int64_t nf) { return sizes_ok(nv, nf) ? carve_components(nullptr).bytes : 0; }

extern "C" size_t sfm_mesh_clean_ws_bytes(int64_t nv, int64_t nf) { return sizes_ok(nv, nf) ? carve_clean(nullptr, nv, nf).bytes : 0; }

extern "C" int sfm_mesh_components(const int32_t* faces_dev, int64_t nv, int64_t nf, int rounds, int resume, int32_t* labels_dev,
                                   int32_t* status_dev, void* ws_dev, size_t ws_bytes, void* stream) {
    SFM_CHECK_ARG(sizes_ok(nv, nf), "sfm_mesh_components: nv %lld, nf %lld: each must be in 0..2^31-1", (long long)nv, (long long)nf);
    SFM_CHECK_ARG(rounds >= 1 && rounds <= kMaxRounds, "sfm_mesh_components: rounds %d must be in 1..%d", rounds, kMaxRounds);
    SFM_CHECK_ARG(status_dev && ws_dev && (nv == 0 || labels_dev) && (nf == 0 || faces_dev), "sfm_mesh_components: null required pointer");
    const ComponentsWs ws = carve_components(ws_dev);
    SFM_CHECK_ARG(ws_bytes >= ws.bytes, "sfm_mesh_components: workspace %zu bytes < %zu", ws_bytes, ws.bytes);
    hipStream_t s = sfm::as_stream(stream);
    hipLaunchKernelGGL(cc_init_kernel, dim3(grid_of(blocks_of(std::max<int64_t>(nv, kMaxRounds + 1)))), dim3(kBlock), 0, s, labels_dev, (int)nv,
                       resume, ws.flags, kMaxRounds + 1);
    SFM_CHECK_LAUNCH();
    const unsigned grid = grid_of(blocks_of(nv + nf));
    for (int r = 1; r <= rounds; ++r) {
        hipLaunchKernelGGL(cc_round_kernel, dim3(grid), dim3(kBlock), 0, s, faces_dev, (int)nv, (int)nf, labels_dev, ws.flags + r - 1,
                           ws.flags + r);
        SFM_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(cc_status_kernel, dim3(1), dim3(kScanThreads), 0, s, ws.flags, rounds, status_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" int sfm_mesh_clean(const float* vertices_dev, const float* colors_dev, const int32_t* faces_dev, int64_t nv, int64_t nf,
                              const int32_t* labels_dev, int64_t min_faces, int largest_only, float* out_vertices_dev, float* out_colors_dev,
                              int32_t* out_faces_dev, int32_t* counts_dev, void* ws_dev, size_t ws_bytes, void* stream) {
    SFM_CHECK_ARG(sizes_ok(nv, nf), "sfm_mesh_clean: nv %lld, nf %lld: each must be in 0..2^31-1", (long long)nv, (long long)nf);
    SFM_CHECK_ARG(min_faces >= 0, "sfm_mesh_clean: min_faces %lld is negative", (long long)min_faces);
    SFM_CHECK_ARG(largest_only == 0 || largest_only == 1, "sfm_mesh_clean: largest_only %d must be 0 or 1", largest_only);
    SFM_CHECK_ARG(counts_dev && ws_dev && (nv == 0 || (vertices_dev && out_vertices_dev && labels_dev)) &&
                      (nf == 0 || (faces_dev && out_faces_dev)),
                  "sfm_mesh_clean: null required pointer");
    SFM_CHECK_ARG(!colors_dev == !out_colors_dev, "sfm_mesh_clean: colours in and colours out go together");
    const CleanWs ws = carve_clean(ws_dev, nv, nf);
    SFM_CHECK_ARG(ws_bytes >= ws.bytes, "sfm_mesh_clean: workspace %zu bytes < %zu", ws_bytes, ws.bytes);
    hipStream_t s = sfm::as_stream(stream);
    const int v = (int)nv, f = (int)nf;
    const long long ncv = blocks_of(nv), ncf = blocks_of(nf), mf = (long long)min_faces;
    const dim3 block(kBlock), grid_v(grid_of(ncv)), grid_f(grid_of(ncf));
    hipLaunchKernelGGL(clean_init_kernel, grid_v, block, 0, s, ws.faces_of, v, ws.scal);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(clean_face_count_kernel, dim3(std::min(grid_f.x, (unsigned)kCountGrid)), block, 0, s, faces_dev, v, f, labels_dev, ws.faces_of);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(clean_stats_kernel, dim3(std::min(grid_v.x, (unsigned)kCountGrid)), block, 0, s, labels_dev, v, ws.faces_of, ws.scal);
    SFM_CHECK_LAUNCH();
    if (largest_only) {
        hipLaunchKernelGGL(clean_best_label_kernel, dim3(std::min(grid_v.x, (unsigned)kCountGrid)), block, 0, s, labels_dev, v, ws.faces_of, ws.scal);
        SFM_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(clean_flag_count_kernel, dim3(grid_of(ncv + ncf)), block, 0, s, faces_dev, v, f, labels_dev, ws.faces_of, mf, largest_only,
                       ncv, ncf, ws.part_v, ws.part_f, ws.scal);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(clean_scan_kernel, dim3(2), dim3(kScanThreads), 0, s, ws.part_v, ncv, ws.part_f, ncf, ws.scal, counts_dev);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(clean_vertex_kernel, grid_v, block, 0, s, reinterpret_cast<const int*>(vertices_dev),
                       reinterpret_cast<const int*>(colors_dev), v, labels_dev, ws.faces_of, mf, largest_only, ws.scal, ncv, ws.part_v, ws.remap,
                       reinterpret_cast<int*>(out_vertices_dev), reinterpret_cast<int*>(out_colors_dev));
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(clean_face_kernel, grid_f, block, 0, s, faces_dev, v, f, labels_dev, ws.faces_of, mf, largest_only, ws.scal, ncf,
                       ws.part_f, ws.remap, out_faces_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}
