// Feature tracks from all-pairs matches and their N-view triangulation (include/sfm_hip.h, "TRACKS"; docs/tracks.md).
//   sfm_match_edges        the Lowe survivors of a match store as graph edges between nodes (image offset + keypoint), in place
//   sfm_track_components   label[u] = the smallest node id of u's component, by min-label hooking and pointer jumping
//   sfm_track_build        sizes, the same-image conflict rule, the length rule, tracks in label order, observations in node order
//   sfm_track_triangulate  one lane per track: M = A^T A over the track's rows, cyclic Jacobi on the 4 x 4, errors and depths
// Every integer output is a minimum, a count, a rank or a copy; tests/np_tracks.py restates all of it exactly.
//
// Labelling.  As csrc/mesh_clean.hip's, over edges instead of faces: one kernel per round over ne + N items; an edge lowers the
// labels of its two ends and of their two current labels to the smaller one; a node follows label[label[..]] for at most kJumpHops
// hops.  A label is READ before it is lowered and the atomic is skipped when it cannot lower: a 64-image track funnels 2 016 edges
// onto one root, and an atomic min that changes nothing still serialises on its cache line.  Labels only fall and always name a
// node of the same component, so every interleaving is a valid state; flag[r] = 0 stops the rounds after r.
//
// Building.  size[label] by atomicAdd (a count); an open-addressing set keyed by (label, image) that holds the smallest node of
// the key (atomicCAS on the key, atomicMin on the value); a node that is not the smallest of its key marks its label conflicting
// (a plain store of 1).  Roots are ranked by per-block counts and a one-workgroup scan; a track's nodes claim slots of a scratch
// list by atomicAdd and then each node writes itself at the rank it has among them, so the order of the claims is never seen.
// Every loop runs over a range fixed at launch or bounded by a constant named here.
#include <algorithm>
#include <climits>

#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxGrid = 1 << 16;               // workgroups per launch; the kernels stride over what is left
constexpr int kMaxRounds = 1024;
constexpr int kJumpHops = 4;                    // hop cap of the pointer chase; the next round picks up the rest
constexpr int kScanThreads = 1024;
constexpr int64_t kMaxCount = INT32_MAX;
constexpr int kMaxImages = 65536;               // an image index takes the low 16 bits of a set key
constexpr int kSearchSteps = 17;                // binary search over at most 65 537 offsets
constexpr int kSweeps = 30;                     // Jacobi sweep bound
constexpr unsigned kQuietNan = 0x7FC00000u;
constexpr unsigned long long kEmptyKey = ~0ull;

enum Scalar { kCandidates = 0, kConflicting = 1, kLongest = 2, kSingles = 3, kScalars = 4 };

__device__ inline int load_relaxed(const int* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

__device__ inline bool in_range(int a, int n) { return (unsigned)a < (unsigned)n; }

// The image of node u: the largest i < n_img with img_off[i] <= u (empty images share an offset: the last one that starts at or
// before u and is not empty is found because the search keeps the upper half on equality).
__device__ inline int image_of(const int* __restrict__ img_off, int n_img, int u) {
    int lo = 0, hi = n_img;                                                     // img_off[lo] <= u < img_off[hi]
    for (int step = 0; step < kSearchSteps && hi - lo > 1; ++step) {
        const int mid = lo + ((hi - lo) >> 1);
        if (img_off[mid] <= u) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- edges ----------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock) void edges_kernel(const int* __restrict__ store, long long n_pairs, long long cap,
                                                       const int* __restrict__ pair_img, const int* __restrict__ nq,
                                                       const int* __restrict__ img_off, int n_img, double ratio,
                                                       const unsigned char* __restrict__ keep, int2* __restrict__ edges) {
    const long long n = n_pairs * cap, stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const long long p = i / cap, q = i - p * cap;
        int2 e = make_int2(-1, -1);
        const int a = pair_img[2 * p], b = pair_img[2 * p + 1];
        if (in_range(a, n_img) && in_range(b, n_img) && q < nq[p] && (!keep || keep[i])) {
            const int oa = img_off[a], ob = img_off[b];
            const long long na = (long long)img_off[a + 1] - oa, nb = (long long)img_off[b + 1] - ob;
            const int2 ii = *reinterpret_cast<const int2*>(store + ((2 * p) * cap + q) * 2);
            const int2 dd = *reinterpret_cast<const int2*>(store + ((2 * p + 1) * cap + q) * 2);
            const float d0 = __int_as_float(dd.x), d1 = __int_as_float(dd.y);
            if (q < na && ii.y >= 0 && ii.x >= 0 && ii.x < nb && (double)d0 < ratio * (double)d1) e = make_int2(oa + (int)q, ob + ii.x);
        }
        edges[i] = e;
    }
}

// ---- components -----------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock) void cc_init_kernel(int* __restrict__ labels, int n, int resume, int* __restrict__ flags, int nflags) {
    const long long stride = (long long)gridDim.x * kBlock, first = (long long)blockIdx.x * kBlock + threadIdx.x;
    for (long long i = first; i < nflags; i += stride) flags[i] = i == 0;      // "round 0 changed something": round 1 runs
    if (resume) return;
    for (long long i = first; i < n; i += stride) labels[i] = (int)i;
}

// Lowers labels[x] to m if it is above m; true when that changed it.  The read first: most calls find nothing to lower.
__device__ inline bool lower(int* labels, int x, int m) { return load_relaxed(labels + x) > m && atomicMin(&labels[x], m) > m; }

__global__ __launch_bounds__(kBlock) void cc_round_kernel(const int2* __restrict__ edges, int n, long long ne, int* labels,
                                                          const int* __restrict__ prev_flag, int* __restrict__ flag) {
    if (*prev_flag == 0) return;                                                // the round before changed nothing: converged
    const long long total = ne + n, stride = (long long)gridDim.x * kBlock;
    int changed = 0;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += stride) {
        if (i < ne) {                                                           // hook
            const int2 e = edges[i];
            if (!in_range(e.x, n) || !in_range(e.y, n) || e.x == e.y) continue;
            const int lu = load_relaxed(labels + e.x), lv = load_relaxed(labels + e.y);
            if (lu == lv || !in_range(lu, n) || !in_range(lv, n)) continue;     // (out of range: not a state this entry point leaves)
            const int m = min(lu, lv), big = max(lu, lv);
            changed |= (int)lower(labels, lu > lv ? e.x : e.y, m) | (int)lower(labels, big, m);
        } else {                                                                // jump
            const int v = (int)(i - ne);
            const int p = load_relaxed(labels + v);
            int q = p;
            for (int hop = 0; hop < kJumpHops && in_range(q, n); ++hop) {
                const int next = load_relaxed(labels + q);                      // q is a label: a node id below n
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

// ---- build ----------------------------------------------------------------------------------------------------------------

struct BuildWs {
    int *size, *conflict, *track_of, *fill, *scratch, *part_t, *part_o, *vals, *scal;
    unsigned long long* keys;
    unsigned long long slots;                    // a power of two >= 2 N
    size_t bytes;
};

__global__ __launch_bounds__(kBlock) void build_init_kernel(BuildWs w, int n) {
    const long long stride = (long long)gridDim.x * kBlock, first = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (first < kScalars) w.scal[first] = 0;
    for (long long i = first; i < n; i += stride) {
        w.size[i] = 0;
        w.conflict[i] = 0;
        w.fill[i] = 0;
    }
    for (unsigned long long i = (unsigned long long)first; i < w.slots; i += (unsigned long long)stride) {
        w.keys[i] = kEmptyKey;
        w.vals[i] = INT_MAX;
    }
}

__global__ __launch_bounds__(kBlock) void build_size_kernel(const int* __restrict__ labels, int n, int* __restrict__ size) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long u = (long long)blockIdx.x * kBlock + threadIdx.x; u < n; u += stride) {
        const int l = labels[u];
        if (in_range(l, n)) atomicAdd(&size[l], 1);
    }
}

__device__ inline unsigned long long set_key(int label, int image) { return ((unsigned long long)(unsigned)label << 16) | (unsigned)image; }

__device__ inline unsigned long long set_home(unsigned long long key, unsigned long long slots) {
    return ((key * 0x9E3779B97F4A7C15ull) >> 20) & (slots - 1);
}

// The set of (label, image) pairs over the nodes of components with two nodes or more; vals[slot] = the smallest node of the key.
__global__ __launch_bounds__(kBlock) void build_insert_kernel(const int* __restrict__ labels, const int* __restrict__ img_off, int n, int n_img,
                                                              BuildWs w) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long u = (long long)blockIdx.x * kBlock + threadIdx.x; u < n; u += stride) {
        const int l = labels[u];
        if (!in_range(l, n) || w.size[l] < 2) continue;
        const unsigned long long key = set_key(l, image_of(img_off, n_img, (int)u));
        unsigned long long s = set_home(key, w.slots);
        for (unsigned long long probe = 0; probe < w.slots; ++probe, s = (s + 1) & (w.slots - 1)) {   // keys <= N < slots: a slot is found
            const unsigned long long seen = atomicCAS(&w.keys[s], kEmptyKey, key);
            if (seen == kEmptyKey || seen == key) {
                atomicMin(&w.vals[s], (int)u);
                break;
            }
        }
    }
}

__global__ __launch_bounds__(kBlock) void build_conflict_kernel(const int* __restrict__ labels, const int* __restrict__ img_off, int n, int n_img,
                                                                BuildWs w) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long u = (long long)blockIdx.x * kBlock + threadIdx.x; u < n; u += stride) {
        const int l = labels[u];
        if (!in_range(l, n) || w.size[l] < 2) continue;
        const unsigned long long key = set_key(l, image_of(img_off, n_img, (int)u));
        unsigned long long s = set_home(key, w.slots);
        for (unsigned long long probe = 0; probe < w.slots; ++probe, s = (s + 1) & (w.slots - 1)) {
            const unsigned long long seen = w.keys[s];
            if (seen == kEmptyKey) break;                                       // (not reached: the key was inserted a launch ago)
            if (seen == key) {
                if (w.vals[s] != (int)u) w.conflict[l] = 1;
                break;
            }
        }
    }
}

struct Rule {
    const int* labels;
    const int* size;
    const int* conflict;
    long long min_len, max_len;
    int n;
    // Is r the root of a kept component?  Its size then, else 0.
    __device__ int kept(long long r) const {
        if (r >= n || labels[r] != (int)r) return 0;
        const int s = size[r];
        return s >= 2 && !conflict[r] && s >= min_len && s <= max_len ? s : 0;
    }
};

__device__ inline int wave_sum(int v) {
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ inline int wave_max(int v) {
    for (int off = 32; off; off >>= 1) v = max(v, __shfl_xor(v, off));
    return v;
}

// Sum over the workgroup, valid in thread 0.
__device__ inline int block_sum(int v, int* lds) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    int t = 0;
    for (int k = 0; k < kWaves; ++k) t += lds[k];
    return t;
}

// Per 256-node block: kept roots and the nodes they hold; over all: candidates, conflicting, the longest kept, single nodes.
__global__ __launch_bounds__(kBlock) void build_root_count_kernel(Rule rule, long long nblocks, BuildWs w) {
    __shared__ int lds[kWaves];
    int cand = 0, conf = 0, longest = 0, singles = 0;
    for (long long blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const long long r = blk * kBlock + threadIdx.x;
        const int s = rule.kept(r);
        if (r < rule.n && rule.labels[r] == (int)r) {
            const int sz = rule.size[r];
            cand += sz >= 2;
            conf += sz >= 2 && rule.conflict[r] != 0;
            singles += sz < 2;
            longest = max(longest, s);
        }
        const int kept = block_sum(s > 0, lds), nodes = block_sum(s, lds);
        if (threadIdx.x == 0) {
            w.part_t[blk] = kept;
            w.part_o[blk] = nodes;
        }
    }
    cand = block_sum(cand, lds);
    conf = block_sum(conf, lds);
    singles = block_sum(singles, lds);
    longest = wave_max(longest);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = longest;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 0; k < kWaves; ++k) longest = max(longest, lds[k]);
        if (cand) atomicAdd(&w.scal[kCandidates], cand);
        if (conf) atomicAdd(&w.scal[kConflicting], conf);
        if (singles) atomicAdd(&w.scal[kSingles], singles);
        if (longest) atomicMax(&w.scal[kLongest], longest);
    }
}

// Workgroup 0: the kept-root block counts -> exclusive offsets in place, counts[0] = tracks; workgroup 1: the same for the nodes
// they hold, counts[1] = observations.  Workgroup 0 also copies the four other counts.
__global__ __launch_bounds__(kScanThreads) void build_scan_kernel(BuildWs w, long long nblocks, int* __restrict__ counts) {
    __shared__ int buf[kScanThreads];
    int* part = blockIdx.x ? w.part_o : w.part_t;
    const int tid = threadIdx.x;
    const long long seg = (nblocks + kScanThreads - 1) / kScanThreads;
    const long long lo = min(tid * seg, nblocks), hi = min(lo + seg, nblocks);
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
    if (blockIdx.x == 0 && tid < kScalars) counts[2 + tid] = w.scal[tid];
}

// Kept roots to their track: track_of[root] = rank among the kept roots, track_off[track] = nodes of the tracks before it.
__global__ __launch_bounds__(kBlock) void build_root_rank_kernel(Rule rule, long long nblocks, BuildWs w, const int* __restrict__ counts,
                                                                 int* __restrict__ track_off) {
    __shared__ int scan_t[kBlock], scan_o[kBlock];
    if (blockIdx.x == 0 && threadIdx.x == 0) track_off[counts[0]] = counts[1];  // counts[0] <= N / 2: inside the N / 2 + 2 words
    for (long long blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const long long r = blk * kBlock + threadIdx.x;
        const int s = rule.kept(r), tid = threadIdx.x;
        __syncthreads();
        scan_t[tid] = s > 0;
        scan_o[tid] = s;
        __syncthreads();
        for (int off = 1; off < kBlock; off <<= 1) {
            const int at = tid >= off ? scan_t[tid - off] : 0, ao = tid >= off ? scan_o[tid - off] : 0;
            __syncthreads();
            scan_t[tid] += at;
            scan_o[tid] += ao;
            __syncthreads();
        }
        if (r >= rule.n) continue;
        if (s > 0) {
            const int t = w.part_t[blk] + scan_t[tid] - 1;                      // < tracks <= N / 2
            w.track_of[r] = t;
            track_off[t] = w.part_o[blk] + scan_o[tid] - s;
        } else {
            w.track_of[r] = -1;
        }
    }
}

__global__ __launch_bounds__(kBlock) void build_claim_kernel(const int* __restrict__ labels, int n, BuildWs w, const int* __restrict__ track_off,
                                                             int* __restrict__ node_track) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long u = (long long)blockIdx.x * kBlock + threadIdx.x; u < n; u += stride) {
        const int l = labels[u];
        int t = -1;
        if (in_range(l, n) && labels[l] == l) t = w.track_of[l];
        node_track[u] = t;
        if (t < 0) continue;
        const int pos = atomicAdd(&w.fill[l], 1);                               // < size[l]: one claim per node with this label
        if (pos < w.size[l]) w.scratch[(long long)track_off[t] + pos] = (int)u;
    }
}

__global__ __launch_bounds__(kBlock) void build_place_kernel(const int* __restrict__ labels, int n, BuildWs w, const int* __restrict__ track_off,
                                                             const int* __restrict__ node_track, int* __restrict__ obs_node) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long u = (long long)blockIdx.x * kBlock + threadIdx.x; u < n; u += stride) {
        const int t = node_track[u];
        if (t < 0) continue;
        const long long lo = track_off[t];
        const int len = w.size[labels[u]];                                      // the loop's bound: the track's length
        int rank = 0;
        for (int k = 0; k < len; ++k) rank += w.scratch[lo + k] < (int)u;
        obs_node[lo + rank] = (int)u;
    }
}

// ---- triangulation --------------------------------------------------------------------------------------------------------

__device__ inline float canonical(float v) { return v != v ? __uint_as_float(kQuietNan) : v; }

// One Jacobi rotation of the symmetric M (full storage) at pivot (p, q); V's columns follow.
__device__ __forceinline__ void rotate(double (&M)[4][4], double (&V)[4][4], int p, int q, bool& rotated) {
    const double apq = M[p][q], app = M[p][p], aqq = M[q][q];
    if (apq == 0.0 || fabs(apq) <= 0x1p-52 * sqrt(fabs(app) * fabs(aqq))) return;
    rotated = true;
    const double theta = (aqq - app) / (2.0 * apq);
    const double root = sqrt(theta * theta + 1.0);
    const double t = theta >= 0.0 ? 1.0 / (theta + root) : -1.0 / (root - theta);
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    for (int k = 0; k < 4; ++k) {
        if (k == p || k == q) continue;
        const double akp = M[k][p], akq = M[k][q];
        const double np_ = c * akp - s * akq, nq_ = s * akp + c * akq;
        M[k][p] = np_; M[p][k] = np_;
        M[k][q] = nq_; M[q][k] = nq_;
    }
    M[p][p] = app - t * apq;
    M[q][q] = aqq + t * apq;
    M[p][q] = 0.0;
    M[q][p] = 0.0;
    for (int k = 0; k < 4; ++k) {
        const double vkp = V[k][p], vkq = V[k][q];
        V[k][p] = c * vkp - s * vkq;
        V[k][q] = s * vkp + c * vkq;
    }
}

__global__ __launch_bounds__(kBlock) void triangulate_kernel(const int* __restrict__ counts, const int* __restrict__ track_off,
                                                             const int* __restrict__ obs_node, const int* __restrict__ img_off, int n_img,
                                                             const float* __restrict__ kp, const double* __restrict__ P, int n, int track_cap,
                                                             float* __restrict__ X, float* __restrict__ err, float* __restrict__ depth,
                                                             int* __restrict__ flags, float* __restrict__ max_err) {
    int T = counts[0], nobs = counts[1];
    if (T < 0 || T > track_cap) T = track_cap;
    if (nobs < 0 || nobs > n) nobs = n;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long t = (long long)blockIdx.x * kBlock + threadIdx.x; t < T; t += stride) {
        int lo = track_off[t], hi = track_off[t + 1];
        lo = min(max(lo, 0), nobs);
        hi = min(max(hi, lo), nobs);                                            // the loops' bounds: 0 <= lo <= hi <= nobs <= n
        double M[4][4];
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) M[a][b] = 0.0;
        for (int o = lo; o < hi; ++o) {
            const int u = obs_node[o];
            if (!in_range(u, n)) continue;
            const double* Pi = P + 12 * (size_t)image_of(img_off, n_img, u);
            const double x = (double)kp[2 * (size_t)u], y = (double)kp[2 * (size_t)u + 1];
            double r0[4], r1[4];
            for (int k = 0; k < 4; ++k) {
                r0[k] = x * Pi[8 + k] - Pi[k];
                r1[k] = y * Pi[8 + k] - Pi[4 + k];
            }
            for (int a = 0; a < 4; ++a)
                for (int b = a; b < 4; ++b) M[a][b] = (M[a][b] + r0[a] * r0[b]) + r1[a] * r1[b];
        }
        for (int a = 1; a < 4; ++a)
            for (int b = 0; b < a; ++b) M[a][b] = M[b][a];
        double V[4][4];
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) V[a][b] = a == b ? 1.0 : 0.0;
        for (int sweep = 0; sweep < kSweeps; ++sweep) {
            bool rotated = false;
            rotate(M, V, 0, 1, rotated);
            rotate(M, V, 0, 2, rotated);
            rotate(M, V, 0, 3, rotated);
            rotate(M, V, 1, 2, rotated);
            rotate(M, V, 1, 3, rotated);
            rotate(M, V, 2, 3, rotated);
            if (!rotated) break;
        }
        int best = 0;
        double low = M[0][0];
        for (int k = 1; k < 4; ++k)
            if (M[k][k] < low) {
                low = M[k][k];
                best = k;
            }
        double v[4];                                                            // column `best`, by selects: a register array stays in registers
        for (int k = 0; k < 4; ++k) v[k] = best == 0 ? V[k][0] : best == 1 ? V[k][1] : best == 2 ? V[k][2] : V[k][3];
        const double v0 = v[0], v1 = v[1], v2 = v[2], v3 = v[3];
        const float X0 = canonical((float)(v0 / v3)), X1 = canonical((float)(v1 / v3)), X2 = canonical((float)(v2 / v3));
        X[3 * t + 0] = X0;
        X[3 * t + 1] = X1;
        X[3 * t + 2] = X2;
        const bool finite = fabsf(X0) <= 3.4028234663852886e38f && fabsf(X1) <= 3.4028234663852886e38f && fabsf(X2) <= 3.4028234663852886e38f;
        const double xd = (double)X0, yd = (double)X1, zd = (double)X2;
        bool front = true;
        float worst = 0.0f;
        for (int o = lo; o < hi; ++o) {
            const int u = obs_node[o];
            float e = __uint_as_float(kQuietNan), d = __uint_as_float(kQuietNan);
            if (in_range(u, n)) {
                const double* Pi = P + 12 * (size_t)image_of(img_off, n_img, u);
                const double x = (double)kp[2 * (size_t)u], y = (double)kp[2 * (size_t)u + 1];
                const double h0 = ((Pi[0] * xd + Pi[1] * yd) + Pi[2] * zd) + Pi[3];
                const double h1 = ((Pi[4] * xd + Pi[5] * yd) + Pi[6] * zd) + Pi[7];
                const double h2 = ((Pi[8] * xd + Pi[9] * yd) + Pi[10] * zd) + Pi[11];
                const double du = h0 / h2 - x, dv = h1 / h2 - y;
                e = canonical((float)sqrt(du * du + dv * dv));
                d = canonical((float)h2);
            }
            err[o] = e;
            depth[o] = d;
            front = front && d > 0.0f && d <= 3.4028234663852886e38f;
            if (e > worst || e != e) worst = e;
        }
        flags[t] = (front ? 1 : 0) | (v3 != 0.0 && finite ? 2 : 0);
        max_err[t] = worst;
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------

int64_t blocks_of(int64_t n) { return (n + kBlock - 1) / kBlock; }

unsigned grid_of(int64_t blocks) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks, kMaxGrid)); }

bool count_ok(int64_t n) { return n >= 0 && n <= kMaxCount; }

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

BuildWs carve_build(void* base, int64_t n) {
    sfm::Carver c(base);
    BuildWs w{};
    w.slots = 2;
    while (w.slots < 2 * (unsigned long long)n) w.slots <<= 1;
    w.size = c.take<int>(n);
    w.conflict = c.take<int>(n);
    w.track_of = c.take<int>(n);
    w.fill = c.take<int>(n);
    w.scratch = c.take<int>(n);
    w.part_t = c.take<int>(blocks_of(n));
    w.part_o = c.take<int>(blocks_of(n));
    w.vals = c.take<int>(w.slots);
    w.scal = c.take<int>(kScalars);
    w.keys = c.take<unsigned long long>(w.slots);
    w.bytes = c.used();
    return w;
}

}  // namespace

extern "C" int sfm_match_edges(const int32_t* store_dev, int64_t n_pairs, int64_t cap, const int32_t* pair_img_dev, const int32_t* nq_dev,
                               const int32_t* img_off_dev, int n_img, double ratio, const uint8_t* keep_dev, int32_t* edges_dev, void* stream) {
    SFM_CHECK_ARG(count_ok(n_pairs) && count_ok(cap), "sfm_match_edges: n_pairs %lld, cap %lld: each must be in 0..2^31-1", (long long)n_pairs,
                  (long long)cap);
    SFM_CHECK_ARG(n_pairs == 0 || cap <= kMaxCount / n_pairs, "sfm_match_edges: n_pairs %lld x cap %lld edge slots exceed 2^31-1",
                  (long long)n_pairs, (long long)cap);
    SFM_CHECK_ARG(n_img >= 1 && n_img <= kMaxImages, "sfm_match_edges: n_img %d must be in 1..%d", n_img, kMaxImages);
    SFM_CHECK_ARG(ratio == ratio, "sfm_match_edges: ratio is NaN");
    const int64_t ne = n_pairs * cap;
    SFM_CHECK_ARG(img_off_dev && (ne == 0 || (store_dev && pair_img_dev && nq_dev && edges_dev)), "sfm_match_edges: null required pointer");
    if (ne == 0) return SFM_OK;
    hipLaunchKernelGGL(edges_kernel, dim3(grid_of(blocks_of(ne))), dim3(kBlock), 0, sfm::as_stream(stream), store_dev, (long long)n_pairs,
                       (long long)cap, pair_img_dev, nq_dev, img_off_dev, n_img, ratio, keep_dev, reinterpret_cast<int2*>(edges_dev));
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" size_t sfm_track_components_ws_bytes(int64_t n_nodes, int64_t ne) {
    return count_ok(n_nodes) && count_ok(ne) ? carve_components(nullptr).bytes : 0;
}

extern "C" int sfm_track_components(const int32_t* edges_dev, int64_t n_nodes, int64_t ne, int rounds, int resume, int32_t* labels_dev,
                                    int32_t* status_dev, void* ws_dev, size_t ws_bytes, void* stream) {
    SFM_CHECK_ARG(count_ok(n_nodes) && count_ok(ne), "sfm_track_components: n_nodes %lld, ne %lld: each must be in 0..2^31-1", (long long)n_nodes,
                  (long long)ne);
    SFM_CHECK_ARG(rounds >= 1 && rounds <= kMaxRounds, "sfm_track_components: rounds %d must be in 1..%d", rounds, kMaxRounds);
    SFM_CHECK_ARG(status_dev && ws_dev && (n_nodes == 0 || labels_dev) && (ne == 0 || edges_dev), "sfm_track_components: null required pointer");
    const ComponentsWs ws = carve_components(ws_dev);
    SFM_CHECK_ARG(ws_bytes >= ws.bytes, "sfm_track_components: workspace %zu bytes < %zu", ws_bytes, ws.bytes);
    hipStream_t s = sfm::as_stream(stream);
    hipLaunchKernelGGL(cc_init_kernel, dim3(grid_of(blocks_of(std::max<int64_t>(n_nodes, kMaxRounds + 1)))), dim3(kBlock), 0, s, labels_dev,
                       (int)n_nodes, resume, ws.flags, kMaxRounds + 1);
    SFM_CHECK_LAUNCH();
    const unsigned grid = grid_of(blocks_of(n_nodes + ne));       // (capped at 4 096 workgroups a real round takes 2.7 x as long: docs/tracks.md §5)
    for (int r = 1; r <= rounds; ++r) {
        hipLaunchKernelGGL(cc_round_kernel, dim3(grid), dim3(kBlock), 0, s, reinterpret_cast<const int2*>(edges_dev), (int)n_nodes, (long long)ne,
                           labels_dev, ws.flags + r - 1, ws.flags + r);
        SFM_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(cc_status_kernel, dim3(1), dim3(kScanThreads), 0, s, ws.flags, rounds, status_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" size_t sfm_track_build_ws_bytes(int64_t n_nodes) { return count_ok(n_nodes) ? carve_build(nullptr, n_nodes).bytes : 0; }

extern "C" int sfm_track_build(const int32_t* labels_dev, const int32_t* img_off_dev, int64_t n_nodes, int n_img, int64_t min_len,
                               int64_t max_len, int32_t* node_track_dev, int32_t* track_off_dev, int32_t* obs_node_dev, int32_t* counts_dev,
                               void* ws_dev, size_t ws_bytes, void* stream) {
    SFM_CHECK_ARG(count_ok(n_nodes), "sfm_track_build: n_nodes %lld must be in 0..2^31-1", (long long)n_nodes);
    SFM_CHECK_ARG(n_img >= 1 && n_img <= kMaxImages, "sfm_track_build: n_img %d must be in 1..%d", n_img, kMaxImages);
    SFM_CHECK_ARG(min_len >= 2 && min_len <= max_len && max_len <= kMaxCount, "sfm_track_build: min_len %lld, max_len %lld: need 2 <= min_len <= max_len <= 2^31-1",
                  (long long)min_len, (long long)max_len);
    SFM_CHECK_ARG(img_off_dev && track_off_dev && counts_dev && ws_dev && (n_nodes == 0 || (labels_dev && node_track_dev && obs_node_dev)),
                  "sfm_track_build: null required pointer");
    const BuildWs ws = carve_build(ws_dev, n_nodes);
    SFM_CHECK_ARG(ws_bytes >= ws.bytes, "sfm_track_build: workspace %zu bytes < %zu", ws_bytes, ws.bytes);
    hipStream_t s = sfm::as_stream(stream);
    const int n = (int)n_nodes;
    const long long nblocks = blocks_of(n_nodes);
    const dim3 block(kBlock), grid(grid_of(nblocks));
    const Rule rule{labels_dev, ws.size, ws.conflict, (long long)min_len, (long long)max_len, n};
    hipLaunchKernelGGL(build_init_kernel, dim3(grid_of(blocks_of((int64_t)ws.slots))), block, 0, s, ws, n);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(build_size_kernel, grid, block, 0, s, labels_dev, n, ws.size);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(build_insert_kernel, grid, block, 0, s, labels_dev, img_off_dev, n, n_img, ws);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(build_conflict_kernel, grid, block, 0, s, labels_dev, img_off_dev, n, n_img, ws);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(build_root_count_kernel, grid, block, 0, s, rule, nblocks, ws);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(build_scan_kernel, dim3(2), dim3(kScanThreads), 0, s, ws, nblocks, counts_dev);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(build_root_rank_kernel, grid, block, 0, s, rule, nblocks, ws, counts_dev, track_off_dev);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(build_claim_kernel, grid, block, 0, s, labels_dev, n, ws, track_off_dev, node_track_dev);
    SFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(build_place_kernel, grid, block, 0, s, labels_dev, n, ws, track_off_dev, node_track_dev, obs_node_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}

extern "C" int sfm_track_triangulate(const int32_t* counts_dev, const int32_t* track_off_dev, const int32_t* obs_node_dev,
                                     const int32_t* img_off_dev, int n_img, const float* kp_dev, const double* P_dev, int64_t n_nodes,
                                     float* X_dev, float* err_dev, float* depth_dev, int32_t* flags_dev, float* max_err_dev, void* stream) {
    SFM_CHECK_ARG(count_ok(n_nodes), "sfm_track_triangulate: n_nodes %lld must be in 0..2^31-1", (long long)n_nodes);
    SFM_CHECK_ARG(n_img >= 1 && n_img <= kMaxImages, "sfm_track_triangulate: n_img %d must be in 1..%d", n_img, kMaxImages);
    SFM_CHECK_ARG(counts_dev && track_off_dev && img_off_dev && P_dev && X_dev && flags_dev && max_err_dev &&
                      (n_nodes == 0 || (obs_node_dev && kp_dev && err_dev && depth_dev)),
                  "sfm_track_triangulate: null required pointer");
    const int track_cap = (int)(n_nodes / 2 + 1);
    if (n_nodes < 2) return SFM_OK;                                             // no track has fewer than two nodes
    hipLaunchKernelGGL(triangulate_kernel, dim3(grid_of(blocks_of(track_cap))), dim3(kBlock), 0, sfm::as_stream(stream), counts_dev, track_off_dev,
                       obs_node_dev, img_off_dev, n_img, kp_dev, P_dev, (int)n_nodes, track_cap, X_dev, err_dev, depth_dev, flags_dev, max_err_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}
