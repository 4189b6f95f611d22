// gradreduce.hip -- the rank-ordered mean of W gradient rows: the arithmetic of a data-parallel training step (vt_grad_rank_mean, include/vistracker.h).
//
// out[i] = (float)((((double)parts[0][i] + parts[1][i]) + ... + parts[W-1][i]) / (double)W): the rows are added left to right in fp64, divided once, rounded to
// fp32 once.  No atomics, no workspace, no cross-thread traffic: every element is owned by ONE thread, which loads it from all W rows before it stores it, so
// `out` may be a row of `parts` and the bits are the same on every call.  A pure stream of (W + 1) . 4 . n bytes.
//
// Shape: a scalar head up to the first 16-byte aligned address of row 0, a body of 4-float groups (one 16-byte load per row, all W issued before the dependent
// chain of fp64 adds, one 16-byte store), a scalar tail.  The body needs every row and `out` aligned alike: stride % 4 == 0 and out = parts (mod 16 bytes), which
// holds for torch allocations, for the encoders' 64-float padded offsets and for `out` a row of `parts`; anything else takes the scalar path for all n.
// Grid-stride launch of 256-thread workgroups, 8 per CU at the most.
#include "common.h"
#include <cstdint>

namespace grm {

constexpr int THREADS = 256;
constexpr int BLOCKS_PER_CU = 8;
constexpr int CHUNK = 4;            // rows loaded together by the generic kernel

template <int W>
__device__ __forceinline__ float grm_mean(const float (&v)[W])
{
    double s = (double)v[0];
#pragma unroll
    for (int r = 1; r < W; r++) s += (double)v[r];
    return (float)(s / (double)W);
}

// one element, any W: rows CHUNK at a time, the loads of a chunk ahead of its adds
__device__ __forceinline__ float grm_scalar(const float *parts, int W, size_t stride, size_t i)
{
    double s = 0.0;
    int r = 0;
    for (; r + CHUNK <= W; r += CHUNK) {
        float v[CHUNK];
#pragma unroll
        for (int k = 0; k < CHUNK; k++) v[k] = parts[(size_t)(r + k) * stride + i];
#pragma unroll
        for (int k = 0; k < CHUNK; k++) s = (r + k == 0) ? (double)v[k] : s + (double)v[k];
    }
    for (; r < W; r++) {
        const float v = parts[(size_t)r * stride + i];
        s = (r == 0) ? (double)v : s + (double)v;
    }
    return (float)(s / (double)W);
}

// W > 0: the unrolled instantiation for exactly W rows; W == 0: the generic loop over `Wrt` rows.
// Elements [0, head) and [head + 4 nvec, n) are scalar, [head, head + 4 nvec) are the nvec groups of the body.
template <int W>
__global__ __launch_bounds__(THREADS) void mean_kernel(const float *parts, int Wrt, size_t n, size_t stride, float *out, size_t head, size_t nvec)
{
    const size_t tid = (size_t)blockIdx.x * THREADS + threadIdx.x;
    const size_t nthreads = (size_t)gridDim.x * THREADS;
    const size_t tail0 = head + 4 * nvec;

    for (size_t g = tid; g < nvec; g += nthreads) {
        const size_t i = head + 4 * g;
        float4 o;
        if constexpr (W > 0) {
            float4 v[W];
#pragma unroll
            for (int r = 0; r < W; r++) v[r] = *reinterpret_cast<const float4 *>(parts + (size_t)r * stride + i);
            float x[W], y[W], z[W], w[W];
#pragma unroll
            for (int r = 0; r < W; r++) { x[r] = v[r].x; y[r] = v[r].y; z[r] = v[r].z; w[r] = v[r].w; }
            o = make_float4(grm_mean<W>(x), grm_mean<W>(y), grm_mean<W>(z), grm_mean<W>(w));
        } else {
            double s[4] = {0.0, 0.0, 0.0, 0.0};
            int r = 0;
            for (; r + CHUNK <= Wrt; r += CHUNK) {
                float4 v[CHUNK];
#pragma unroll
                for (int k = 0; k < CHUNK; k++) v[k] = *reinterpret_cast<const float4 *>(parts + (size_t)(r + k) * stride + i);
#pragma unroll
                for (int k = 0; k < CHUNK; k++) {
                    const bool first = (r + k == 0);
                    s[0] = first ? (double)v[k].x : s[0] + (double)v[k].x;
                    s[1] = first ? (double)v[k].y : s[1] + (double)v[k].y;
                    s[2] = first ? (double)v[k].z : s[2] + (double)v[k].z;
                    s[3] = first ? (double)v[k].w : s[3] + (double)v[k].w;
                }
            }
            for (; r < Wrt; r++) {
                const float4 v = *reinterpret_cast<const float4 *>(parts + (size_t)r * stride + i);
                const bool first = (r == 0);
                s[0] = first ? (double)v.x : s[0] + (double)v.x;
                s[1] = first ? (double)v.y : s[1] + (double)v.y;
                s[2] = first ? (double)v.z : s[2] + (double)v.z;
                s[3] = first ? (double)v.w : s[3] + (double)v.w;
            }
            const double d = (double)Wrt;
            o = make_float4((float)(s[0] / d), (float)(s[1] / d), (float)(s[2] / d), (float)(s[3] / d));
        }
        *reinterpret_cast<float4 *>(out + i) = o;
    }

    // head and tail: fewer than 4 elements each when there is a body, all n when there is none
    const size_t nscalar = head + (n - tail0);
    for (size_t k = tid; k < nscalar; k += nthreads) {
        const size_t i = k < head ? k : tail0 + (k - head);
        float o;
        if constexpr (W > 0) {
            float v[W];
#pragma unroll
            for (int r = 0; r < W; r++) v[r] = parts[(size_t)r * stride + i];
            o = grm_mean<W>(v);
        } else {
            o = grm_scalar(parts, Wrt, stride, i);
        }
        out[i] = o;
    }
}

}  // namespace grm

extern "C" int vt_grad_rank_mean(const float *parts, int W, size_t n, size_t stride, float *out, void *stream)
{
    VT_REQUIRE(W >= 1, "vt_grad_rank_mean: W = %d, at least one row expected", W);
    VT_REQUIRE(stride >= n, "vt_grad_rank_mean: stride %zu < n %zu", stride, n);
    if (n == 0) return VT_OK;
    VT_REQUIRE(parts && out, "vt_grad_rank_mean: NULL pointer with n = %zu", n);
    const uintptr_t pa = reinterpret_cast<uintptr_t>(parts), oa = reinterpret_cast<uintptr_t>(out);
    VT_REQUIRE(pa % 4 == 0 && oa % 4 == 0, "vt_grad_rank_mean: pointers must be 4-byte aligned");
    // out: a row of parts (in place: an element is read from every row by the one thread that writes it) or memory that overlaps none of the rows read
    const uintptr_t span = ((uintptr_t)(W - 1) * stride + n) * 4;
    if (oa + n * 4 > pa && oa < pa + span) {
        const uintptr_t off = oa - pa;
        VT_REQUIRE(oa >= pa && off % ((uintptr_t)stride * 4) == 0 && off / ((uintptr_t)stride * 4) < (uintptr_t)W,
                   "vt_grad_rank_mean: out overlaps parts without being one of its rows");
    }

    size_t head = n, nvec = 0;
    if (stride % 4 == 0 && oa % 16 == pa % 16) {
        head = ((16 - pa % 16) % 16) / 4;
        if (head > n) head = n;
        nvec = (n - head) / 4;
        if (nvec == 0) head = n;
    }
    int cus = 0;
    if (int rc = vt_cu_count(&cus)) return rc;
    const size_t nscalar = n - 4 * nvec;
    const size_t work = nvec > nscalar ? nvec : nscalar;
    size_t blocks = (work + grm::THREADS - 1) / grm::THREADS;
    const size_t cap = (size_t)cus * grm::BLOCKS_PER_CU;
    if (blocks > cap) blocks = cap;
    const dim3 grid((unsigned)blocks), block(grm::THREADS);
    hipStream_t st = vt_stream(stream);
    switch (W) {
    case 1: hipLaunchKernelGGL(grm::mean_kernel<1>, grid, block, 0, st, parts, W, n, stride, out, head, nvec); break;
    case 2: hipLaunchKernelGGL(grm::mean_kernel<2>, grid, block, 0, st, parts, W, n, stride, out, head, nvec); break;
    case 4: hipLaunchKernelGGL(grm::mean_kernel<4>, grid, block, 0, st, parts, W, n, stride, out, head, nvec); break;
    case 8: hipLaunchKernelGGL(grm::mean_kernel<8>, grid, block, 0, st, parts, W, n, stride, out, head, nvec); break;
    default: hipLaunchKernelGGL(grm::mean_kernel<0>, grid, block, 0, st, parts, W, n, stride, out, head, nvec); break;
    }
    VT_LAUNCH_CHECK();
    return VT_OK;
}
