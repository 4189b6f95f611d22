// losshead.hip -- SIF-Net's training objective at labelled points: the six losses of CHORETriplaneVisibility.get_errors (model/chore_tri_vis.py:52-99,
// with CHORE.get_df_loss, model/chore.py:312-325) over S stacks of predictions, and the gradient of gscale * error to every prediction, in one pass.
//
// Per stack (p = prediction, g = label, md = max_dist, mask = [df_o < 0.05] on the UNCLAMPED label, strict):
//   df_h, df_o  sum_N |min(p, md) - min(g, md)|, mean over B            d/dp = sign(min(p, md) - min(g, md)) [p <= md]   (sign(0) = 0; torch.clamp passes p == md)
//   parts       sum_N (logsumexp(x) - x[label]), mean over B            d/dx = softmax(x) - onehot(label)                (14 classes, max-shifted)
//   pca         mean over B 9 N of (p - g)^2 mask                       d/dp = 2 (p - g) mask
//   vis         mean over B N of |p - g| mask (l1) or (p - g)^2 mask    d/dp = sign(p - g) mask or 2 (p - g) mask
//   obj_center  mean over B 3 N of (p - g)^2 mask                       d/dp = 2 (p - g) mask
// terms[0..5] = these six in the slot order of the reference's losses_all (df_h, df_o, parts, pca, vis -- the slot it calls loss_smpl_center --, obj_center),
// averaged over the stacks, UNWEIGHTED: the host applies the weights to values, the kernel applies them to gradients.  error = sum_k w_k term_k with
// weights[6] in the order of loss_weights (dfh, dfo, parts, pca, obj_center, vis: slot 4 takes weights[5], slot 5 takes weights[4], as the reference does).
// The gradient written for an element is gscale * w * (d term / d element) with the term's 1 / (count S) folded in.
//
// Arithmetic: the fp32 inputs are widened and every difference, square, exponential and sum is taken in fp64; a gradient is rounded to fp32 once, when it is
// stored.  The comparisons that DECIDE something (min with md, p <= md, df_o < 0.05) are on the fp32 values as they were read.  No NaN for finite inputs: the
// log-sum-exp is shifted by the largest logit, and an all-false mask gives zero terms and zero gradients.  A part label outside [0, 14) is clamped into it
// (nothing is indexed by it: the label selects among registers), so such a point gets the loss of the clamped label and no other point is affected.
//
// pca_gt, obj_center and visibility come per point ((B,9,N), (B,3,N), (B,N)) or per frame ((B,9), (B,3), (B)): the reference repeats a frame's value over its
// points (data/traindata_online.py:102,177-183).  Both forms give identical bits: the value read is the same fp32 number.
//
// MI355X mapping: a streaming kernel, one thread per point, 256 points of one frame per workgroup.  All tensors are channel-major with N innermost, so for
// every channel the 64 lanes of a wave read (and write) 256 contiguous bytes; rows start at multiples of N floats, which are 16-byte aligned only when N is a
// multiple of 4, so the access is one dword per lane for every N.  Per point and stack: 29 loads, 29 stores, all independent of each other.
// DETERMINISTIC reduction, no atomics: six fp64 partials per lane -> wave butterfly (shuffles) -> the four waves through LDS in wave order -> one record of
// six doubles per workgroup in the caller's workspace -> ll_finish_kernel: one wave per term adds the records lane-strided in index order, then the same
// butterfly, and divides by the term's count.  The same inputs give the same bits on every call, with or without gradient pointers.
#include "common.h"

#define LL_BLK 256
#define LL_NW (LL_BLK / 64)
#define LL_PARTS 14

struct ll_args {
    const float *df, *pca, *parts, *centers, *vis;             // (S,B,2,N) (S,B,9,N) (S,B,14,N) (S,B,3,N) (S,B,1,N)
    const float *df_h, *df_o, *pca_gt, *obj_center, *visibility;
    const int *parts_gt;
    float *d_df, *d_pca, *d_parts, *d_centers, *d_vis;         // each may be NULL
    double g[6];                                               // per SLOT: gscale * weight / (count * S), the factor of a gradient element
    double *records;
    int S, B, N, per_frame, vis_l2;
    float max_dist;
};

__device__ __forceinline__ double ll_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ double ll_sign(double d) { return d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0); }

__global__ __launch_bounds__(LL_BLK, 3) void ll_loss_kernel(const ll_args a)
{
    __shared__ double red[LL_NW][6];
    const int n = blockIdx.x * LL_BLK + threadIdx.x, b = blockIdx.y, N = a.N;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (n < N) {
        const size_t bn = (size_t)b * N + n;
        const float gh = a.df_h[bn], go = a.df_o[bn], md = a.max_dist;
        const int label = min(max(a.parts_gt[bn], 0), LL_PARTS - 1);
        const bool mask = go < 0.05f;
        const float ghc = fminf(gh, md), goc = fminf(go, md);
        float pg[9], og[3];
#pragma unroll
        for (int c = 0; c < 9; c++) pg[c] = a.per_frame ? a.pca_gt[b * 9 + c] : a.pca_gt[((size_t)b * 9 + c) * N + n];
#pragma unroll
        for (int c = 0; c < 3; c++) og[c] = a.per_frame ? a.obj_center[b * 3 + c] : a.obj_center[((size_t)b * 3 + c) * N + n];
        const float vg = a.per_frame ? a.visibility[b] : a.visibility[bn];
        for (int s = 0; s < a.S; s++) {
            const size_t sb = (size_t)s * a.B + b;
            // distance fields
            {
                const size_t o = sb * 2 * N + n;
                const float ph = a.df[o], po = a.df[o + N];
                const double dh = (double)fminf(ph, md) - (double)ghc, dq = (double)fminf(po, md) - (double)goc;
                acc[0] += fabs(dh); acc[1] += fabs(dq);
                if (a.d_df) {
                    a.d_df[o] = ph <= md ? (float)(ll_sign(dh) * a.g[0]) : 0.f;
                    a.d_df[o + N] = po <= md ? (float)(ll_sign(dq) * a.g[1]) : 0.f;
                }
            }
            // parts: cross-entropy over 14 logits
            {
                const size_t o = sb * LL_PARTS * N + n;
                float x[LL_PARTS];
#pragma unroll
                for (int c = 0; c < LL_PARTS; c++) x[c] = a.parts[o + (size_t)c * N];
                float m = x[0];
#pragma unroll
                for (int c = 1; c < LL_PARTS; c++) m = fmaxf(m, x[c]);
                double e[LL_PARTS], sum = 0.0, xl = 0.0;
#pragma unroll
                for (int c = 0; c < LL_PARTS; c++) {
                    const double z = (double)x[c] - (double)m;
                    e[c] = exp(z); sum += e[c];
                    xl = c == label ? z : xl;
                }
                acc[2] += log(sum) - xl;
                if (a.d_parts) {
                    const double inv = 1.0 / sum;
#pragma unroll
                    for (int c = 0; c < LL_PARTS; c++) a.d_parts[o + (size_t)c * N] = (float)((e[c] * inv - (c == label ? 1.0 : 0.0)) * a.g[2]);
                }
            }
            // pca axes
            {
                const size_t o = sb * 9 * N + n;
#pragma unroll
                for (int c = 0; c < 9; c++) {
                    const double d = (double)a.pca[o + (size_t)c * N] - (double)pg[c];
                    acc[3] += mask ? d * d : 0.0;
                    if (a.d_pca) a.d_pca[o + (size_t)c * N] = mask ? (float)(2.0 * d * a.g[3]) : 0.f;
                }
            }
            // visibility
            {
                const size_t o = sb * N + n;
                const double d = (double)a.vis[o] - (double)vg;
                acc[4] += mask ? (a.vis_l2 ? d * d : fabs(d)) : 0.0;
                if (a.d_vis) a.d_vis[o] = mask ? (float)((a.vis_l2 ? 2.0 * d : ll_sign(d)) * a.g[4]) : 0.f;
            }
            // object centre
            {
                const size_t o = sb * 3 * N + n;
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const double d = (double)a.centers[o + (size_t)c * N] - (double)og[c];
                    acc[5] += mask ? d * d : 0.0;
                    if (a.d_centers) a.d_centers[o + (size_t)c * N] = mask ? (float)(2.0 * d * a.g[5]) : 0.f;
                }
            }
        }
    }
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const double v = ll_wave_sum(acc[k]);
        if (lane == 0) red[w][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        double v = red[0][threadIdx.x];
#pragma unroll
        for (int i = 1; i < LL_NW; i++) v += red[i][threadIdx.x];
        a.records[((size_t)b * gridDim.x + blockIdx.x) * 6 + threadIdx.x] = v;
    }
}

struct ll_den { double d[6]; };

// one wave per term: lane l adds records l, l + 64, ... in index order, then the butterfly; terms[k] = sum / den[k]
__global__ __launch_bounds__(6 * 64) void ll_finish_kernel(const double *__restrict__ records, int n_records, const ll_den den, double *__restrict__ terms)
{
    const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double v = 0.0;
    for (int r = lane; r < n_records; r += 64) v += records[(size_t)r * 6 + k];
    v = ll_wave_sum(v);
    if (lane == 0) terms[k] = v / den.d[k];
}

extern "C" long vt_sifnet_loss_head_ws_bytes(int B, int n_points)
{
    if (B <= 0 || n_points <= 0) return -1;
    return (long)B * ((n_points + LL_BLK - 1) / LL_BLK) * 6 * (long)sizeof(double);
}

extern "C" int vt_sifnet_loss_head(const float *df, const float *pca, const float *parts, const float *centers, const float *vis, int S, int B, int n_points,
                                   const float *df_h, const float *df_o, const int *parts_gt, const float *pca_gt, const float *obj_center,
                                   const float *visibility, int per_frame, float max_dist, const double *weights, int vis_loss, float gscale, double *terms,
                                   float *d_df, float *d_pca, float *d_parts, float *d_centers, float *d_vis, void *workspace, void *stream)
{
    VT_REQUIRE(df && pca && parts && centers && vis && df_h && df_o && parts_gt && pca_gt && obj_center && visibility && weights && terms && workspace,
               "vt_sifnet_loss_head: null pointer (only the five gradient pointers may be NULL)");
    VT_REQUIRE(S > 0 && B > 0 && B <= 65535 && n_points > 0, "vt_sifnet_loss_head: S, B, n_points > 0 and B <= 65535");
    VT_REQUIRE((per_frame == 0 || per_frame == 1) && (vis_loss == 0 || vis_loss == 1), "vt_sifnet_loss_head: per_frame and vis_loss are 0 or 1");
    VT_REQUIRE(((size_t)workspace & 7) == 0 && ((size_t)terms & 7) == 0, "vt_sifnet_loss_head: workspace and terms must be 8-byte aligned");
    const int N = n_points, nblk = (N + LL_BLK - 1) / LL_BLK;
    VT_REQUIRE((long long)nblk * B < (1ll << 31), "vt_sifnet_loss_head: B * ceil(n_points / 256) must stay below 2^31");
    // elements a term averages over, per SLOT, and the loss weight the slot takes
    const double cnt[6] = {(double)B, (double)B, (double)B, (double)B * 9 * N, (double)B * N, (double)B * 3 * N};
    const int wk[6] = {0, 1, 2, 3, 5, 4};
    ll_args a;
    a.df = df; a.pca = pca; a.parts = parts; a.centers = centers; a.vis = vis;
    a.df_h = df_h; a.df_o = df_o; a.pca_gt = pca_gt; a.obj_center = obj_center; a.visibility = visibility; a.parts_gt = parts_gt;
    a.d_df = d_df; a.d_pca = d_pca; a.d_parts = d_parts; a.d_centers = d_centers; a.d_vis = d_vis;
    a.records = static_cast<double *>(workspace);
    a.S = S; a.B = B; a.N = N; a.per_frame = per_frame; a.vis_l2 = vis_loss; a.max_dist = max_dist;
    ll_den den;
    for (int k = 0; k < 6; k++) {
        den.d[k] = cnt[k] * S;
        a.g[k] = (double)gscale * weights[wk[k]] / den.d[k];
    }
    hipStream_t st = vt_stream(stream);
    hipLaunchKernelGGL(ll_loss_kernel, dim3(nblk, B), dim3(LL_BLK), 0, st, a);
    VT_LAUNCH_CHECK();
    hipLaunchKernelGGL(ll_finish_kernel, dim3(1), dim3(6 * 64), 0, st, a.records, nblk * B, den, terms);
    VT_LAUNCH_CHECK();
    return VT_OK;
}
