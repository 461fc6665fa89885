// Merging fusion of the MVS depth maps (include/sfm_hip.h, "MVS-FUSE"; docs/mvs.md §10).
//   sfm_mvs_fuse   one launch over all views: geometric consistency of every pixel with its view's neighbours (mvs.hip's
//                  consistency_kernel, word for word), a normal-agreement test, and the mean of the consistent samples: position,
//                  unit normal and colour, with the number of samples merged.
// Every float step is a correctly rounded float32 operation in the order the header writes it (no FMA: the Makefile passes
// -ffp-contract=off), neighbours strictly in table order, so that tests/np_mvs_fuse.py restates the kernel bit for bit.
//
// fuse_kernel: a workgroup owns a 16 x 16 tile of one view (blockIdx.z), a lane per pixel.  The view's 512-byte record and the
// neighbours' records are addressed by wave-uniform values only, so they arrive through scalar loads; neighbouring lanes project to
// neighbouring pixels of the neighbour view, so the depth, normal and colour gathers touch a handful of cache lines per wave.  The
// table holds view indices, never addresses: an index outside 0..n-1 (or the view itself) is skipped, nnbr is clamped to 8, and (u, t)
// passes the frame test before it is an index, so no table content makes the kernel read out of range.  No atomics, no LDS.
#include "common.h"

namespace {

constexpr int kTile = 16;
constexpr int kMaxSlots = 8;

struct FuseRecord {                             // the header's layout: 128 words
    int32_t nnbr;
    int32_t min_consistent;
    int32_t nbr[kMaxSlots];
    float bc[12];                               // B (3x3 row-major) | c (3) of the view itself
    float ab[kMaxSlots][12];                    // A (3x3 row-major) | b (3) per neighbour slot
    int32_t pad[10];
};
static_assert(sizeof(FuseRecord) == 512, "the fusion table's record is 512 bytes");

__global__ __launch_bounds__(256) void fuse_kernel(const float* __restrict__ depth, const float* __restrict__ normal,
                                                   const uint8_t* __restrict__ bgr, const FuseRecord* __restrict__ table, int n, int w, int h,
                                                   float tau, float cos_min, int unique, uint8_t* __restrict__ mask, float* __restrict__ xyz,
                                                   float* __restrict__ normal_out, uint8_t* __restrict__ bgr_out, uint8_t* __restrict__ support) {
    const int x = blockIdx.x * kTile + (threadIdx.x & (kTile - 1)), y = blockIdx.y * kTile + (threadIdx.x >> 4);
    if (x >= w || y >= h) return;
    const int i = blockIdx.z;                                   // < n: the grid's z extent
    const size_t plane = (size_t)w * (size_t)h;
    const size_t o = (size_t)i * plane + (size_t)y * w + x;
    const FuseRecord& rec = table[i];
    const float d = depth[o];
    const float fx = (float)x, fy = (float)y;
    const float* b = rec.bc;
    float X0 = d * ((b[0] * fx + b[1] * fy) + b[2]) + b[9];
    float X1 = d * ((b[3] * fx + b[4] * fy) + b[5]) + b[10];
    float X2 = d * ((b[6] * fx + b[7] * fy) + b[8]) + b[11];
    float n0 = 0.0f, n1 = 0.0f, n2 = 0.0f;
    if (normal) {
        n0 = normal[3 * o + 0];
        n1 = normal[3 * o + 1];
        n2 = normal[3 * o + 2];
    }
    float N0 = n0, N1 = n1, N2 = n2;
    int s0 = 0, s1 = 0, s2 = 0;
    if (bgr) {
        s0 = bgr[3 * o + 0];
        s1 = bgr[3 * o + 1];
        s2 = bgr[3 * o + 2];
    }
    int count = 0;
    bool lower = false;
    if (d > 0.0f) {
        const int nnbr = min(rec.nnbr, kMaxSlots);
        for (int s = 0; s < nnbr; ++s) {
            const int v = rec.nbr[s];
            if (v < 0 || v >= n || v == i) continue;            // wave-uniform
            const float* a = rec.ab[s];
            const float p0 = d * ((a[0] * fx + a[1] * fy) + a[2]) + a[9];
            const float p1 = d * ((a[3] * fx + a[4] * fy) + a[5]) + a[10];
            const float p2 = d * ((a[6] * fx + a[7] * fy) + a[8]) + a[11];
            if (!(p2 > 0.0f)) continue;
            const float u = floorf(p0 / p2 + 0.5f), t = floorf(p1 / p2 + 0.5f);
            if (!(u >= 0.0f && u <= (float)(w - 1) && t >= 0.0f && t <= (float)(h - 1))) continue;
            const size_t q = (size_t)v * plane + (size_t)(int)t * w + (size_t)(int)u;
            const float dv = depth[q];
            if (!(dv > 0.0f && fabsf(p2 - dv) <= tau * dv)) continue;
            float m0 = 0.0f, m1 = 0.0f, m2 = 0.0f;
            if (normal) {
                m0 = normal[3 * q + 0];
                m1 = normal[3 * q + 1];
                m2 = normal[3 * q + 2];
                if (!((n0 * m0 + n1 * m1) + n2 * m2 >= cos_min)) continue;
            }
            ++count;
            lower = lower || v < i;
            const float* c = table[v].bc;
            X0 = X0 + (dv * ((c[0] * u + c[1] * t) + c[2]) + c[9]);
            X1 = X1 + (dv * ((c[3] * u + c[4] * t) + c[5]) + c[10]);
            X2 = X2 + (dv * ((c[6] * u + c[7] * t) + c[8]) + c[11]);
            N0 = N0 + m0;
            N1 = N1 + m1;
            N2 = N2 + m2;
            if (bgr) {
                s0 += bgr[3 * q + 0];
                s1 += bgr[3 * q + 1];
                s2 += bgr[3 * q + 2];
            }
        }
    }
    const bool keep = d > 0.0f && count >= rec.min_consistent && !(unique && lower);
    const int k = 1 + count;                                    // 1..9
    const float kf = (float)k;
    mask[o] = keep ? 1 : 0;
    support[o] = keep ? (uint8_t)k : 0;
    xyz[3 * o + 0] = keep ? X0 / kf : 0.0f;
    xyz[3 * o + 1] = keep ? X1 / kf : 0.0f;
    xyz[3 * o + 2] = keep ? X2 / kf : 0.0f;
    if (normal) {
        const float len = sqrtf((N0 * N0 + N1 * N1) + N2 * N2);
        const bool good = len > 0.0f;
        normal_out[3 * o + 0] = keep ? (good ? N0 / len : n0) : 0.0f;
        normal_out[3 * o + 1] = keep ? (good ? N1 / len : n1) : 0.0f;
        normal_out[3 * o + 2] = keep ? (good ? N2 / len : n2) : 0.0f;
    }
    if (bgr) {
        bgr_out[3 * o + 0] = keep ? (uint8_t)((2 * s0 + k) / (2 * k)) : 0;
        bgr_out[3 * o + 1] = keep ? (uint8_t)((2 * s1 + k) / (2 * k)) : 0;
        bgr_out[3 * o + 2] = keep ? (uint8_t)((2 * s2 + k) / (2 * k)) : 0;
    }
}

}  // namespace

extern "C" int sfm_mvs_fuse(const float* depth_dev, const float* normal_dev, const uint8_t* bgr_dev, const void* table_dev, int n, int64_t w,
                            int64_t h, float tau, float cos_min, int unique, uint8_t* mask_dev, float* xyz_dev, float* normal_out_dev,
                            uint8_t* bgr_out_dev, uint8_t* support_dev, void* stream) {
    SFM_CHECK_ARG(n >= 1 && n <= 4096, "sfm_mvs_fuse: n %d outside 1..4096", n);
    SFM_CHECK_ARG(w >= 1 && h >= 1 && w < (1 << 15) && h < (1 << 15), "sfm_mvs_fuse: %lld x %lld frame: each side must be in 1..32767",
                  (long long)w, (long long)h);
    SFM_CHECK_ARG(tau >= 0.0f && tau < INFINITY, "sfm_mvs_fuse: tau must be finite and >= 0");
    SFM_CHECK_ARG(!(cos_min != cos_min), "sfm_mvs_fuse: cos_min is NaN");
    SFM_CHECK_ARG(depth_dev && table_dev && mask_dev && xyz_dev && support_dev, "sfm_mvs_fuse: null required pointer");
    SFM_CHECK_ARG((normal_dev != nullptr) == (normal_out_dev != nullptr), "sfm_mvs_fuse: normal_out_dev goes with normal_dev (both or neither)");
    SFM_CHECK_ARG((bgr_dev != nullptr) == (bgr_out_dev != nullptr), "sfm_mvs_fuse: bgr_out_dev goes with bgr_dev (both or neither)");
    const dim3 grid((unsigned)((w + kTile - 1) / kTile), (unsigned)((h + kTile - 1) / kTile), (unsigned)n);
    hipLaunchKernelGGL(fuse_kernel, grid, dim3(256), 0, sfm::as_stream(stream), depth_dev, normal_dev, bgr_dev,
                       static_cast<const FuseRecord*>(table_dev), n, (int)w, (int)h, tau, cos_min, unique ? 1 : 0, mask_dev, xyz_dev,
                       normal_out_dev, bgr_out_dev, support_dev);
    SFM_CHECK_LAUNCH();
    return SFM_OK;
}
