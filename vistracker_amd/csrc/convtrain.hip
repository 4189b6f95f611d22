// convtrain.hip -- the backward of the encoders' ConvBlock (model/net_util.py:346-396: three pre-activated 3x3 convolutions GroupNorm(32) -> ReLU -> conv,
// bias-free, outputs concatenated, + identity or GN -> ReLU -> conv1x1 residual).  The forward is conv.hip; its split-f16 operand format assumes
// |activation| < 4094 and cannot carry a gradient (1e-7 .. 1e+3 depending on loss scale and depth), so nothing of it is reused here:
//
// ARITHMETIC.  Every product of both GEMMs is an exact fp32 product accumulated in fp32 on v_mfma_f32_16x16x4_f32 (builtin, no inline assembly), as in
// dectrain.hip; no range assumption on any gradient -- scaling the upstream gradient by a power of two scales every output by it, bit for bit.  No atomics,
// one writer per output element per launch, a fixed order of every sum: the same inputs give the same bits.  All tensors are NHWC fp32 slices
// (pointer, channel stride, channel offset), weights plain fp32 device memory in the reference's (Cout, Cin, kh, kw) layout.
//
// KERNELS.
//   wtrans_kernel   W (Cout, Cin, taps) -> [tap][Cout / 4][Cin][4 co]: the data-gradient kernel's A fragments (4 consecutive K steps) become one 16-byte load,
//                   256 contiguous bytes per 16 lanes.  Runs per call: training changes the weights every step.
//   dgrad_kernel    d_a[b,y,x,ci] = sum (co,ky,kx) W[co,ci,ky,kx] d_o[b,y-ky+1,x-kx+1,co].  Workgroup = an 8 x 16 pixel tile x 64 input channels, wave = 16 of them
//                   x 128 pixels (8 accumulator tiles).  Per 32-channel chunk of d_o the 10 x 18 halo patch goes to LDS once as fp32 ([pixel][36], double buffered,
//                   one barrier per chunk); the nine taps read it at flipped offsets, one ds_read_b128 per four MFMAs; the MFMA chain covers one tap row of a chunk (96 terms) and is then
//                   added to a running total (a blocked sum).  K3 = false: the 1x1 form (no halo, one tap).
//   wgrad_kernel    dW[co,ci,ky,kx] = sum (b,y,x) d_o[b,y,x,co] a[b,y+ky-1,x+kx-1,ci], a = max(fma(x, rstd gamma, beta - mean rstd gamma), 0) recomputed from the
//                   saved pre-norm input while the patch is staged (the forward's own fp32 expression; the rectified tensor never exists in memory).  Split K:
//                   workgroup = (split of a frame's pixel tiles, frame, chunk of input channels), wave = 64 (32) output channels x 16 input channels x all taps
//                   (36 accumulator tiles); the A fragment of a K step (4 pixels) is loaded once and serves the nine taps.  Partials [frame][split][tap][co][ci].
//   wfinish_kernel  the partials added in fp64 in (frame, split) order, rounded once, stored or added to dW (accumulate).
//   gnb_*           GroupNorm + ReLU backward (below).
#include "common.h"

namespace convt {

typedef float f32x4 __attribute__((ext_vector_type(4)));
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

#define CT_TH 8
#define CT_TW 16
#define CT_PW 18
#define CT_PX 180           /* 10 x 18 halo pixels */
#define CT_DS 36            /* LDS floats per pixel of the d_o patch: 32 channels + 4 (the b128 reads of 8 lanes cover the 32 banks) */
#define CT_GNB_MAXBLK 64

static inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

__global__ __launch_bounds__(256) void wtrans_kernel(const float *__restrict__ w, int Cout, int Cin, int ntap, float *__restrict__ wt)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x, n = (long)Cout * Cin * ntap;
    if (i >= n) return;
    const int t = (int)(i % ntap); const long r = i / ntap; const int ci = (int)(r % Cin), co = (int)(r / Cin);
    wt[(((size_t)t * (Cout >> 2) + (co >> 2)) * Cin + ci) * 4 + (co & 3)] = w[i];
}

template <bool K3>
__global__ __launch_bounds__(256, 2) void dgrad_kernel(const float4 *__restrict__ wt, int Cout, int Cin, const float *__restrict__ dout, int do_cs, int do_co,
                                                       int H, int W, float *__restrict__ din, int di_cs, int di_co)
{
    constexpr int PW = K3 ? CT_PW : CT_TW, PX = K3 ? CT_PX : CT_TH * CT_TW, NTAP = K3 ? 9 : 1, NLD = K3 ? 6 : 4;
    __shared__ __attribute__((aligned(16))) float patch[2][CT_PX * CT_DS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, q = lane >> 4, j = lane & 15;
    const int tiles_x = W / CT_TW, tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x, b = blockIdx.y;
    const int y0 = ty * CT_TH - (K3 ? 1 : 0), x0 = tx * CT_TW - (K3 ? 1 : 0);
    const int ci0 = blockIdx.z * 64 + wave * 16;
    const bool live = ci0 < Cin;                 // Cin % 32 == 0: a wave's 16 channels are all inside or all outside
    const float *__restrict__ dob = dout + (size_t)b * H * W * do_cs + do_co;
    const int nchunk = Cout >> 5, cog = Cout >> 2;

    // two-level sum: the MFMA chain `acc` runs over one tap row of one chunk (96 terms; 32 in the 1x1 form) and is then added to `tot` -- a single fp32 chain
    // over K = 9 Cout = 1152 terms measured 4.16 e32 on the 256 <- 128 layer, the blocked sum stays inside the float32 model's own error
    f32x4 acc[CT_TH], tot[CT_TH];
#pragma unroll
    for (int p = 0; p < CT_TH; p++) { acc[p] = (f32x4){0.f, 0.f, 0.f, 0.f}; tot[p] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
    float4 ld[NLD];
    auto issue = [&](int c) {
#pragma unroll
        for (int r = 0; r < NLD; r++) {
            const int it = tid + 256 * r, px = it >> 3, piece = it & 7;
            const int yy = y0 + px / PW, xx = x0 + px % PW;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);      // zero padding of the output gradient outside the image
            if (it < PX * 8 && yy >= 0 && yy < H && xx >= 0 && xx < W)
                v = *reinterpret_cast<const float4 *>(dob + ((size_t)yy * W + xx) * do_cs + c * 32 + piece * 4);
            ld[r] = v;
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int r = 0; r < NLD; r++) {
            const int it = tid + 256 * r, px = it >> 3, piece = it & 7;
            if (it < PX * 8) *reinterpret_cast<float4 *>(&patch[buf][px * CT_DS + piece * 4]) = ld[r];
        }
    };
    issue(0);
    stage(0);
    for (int c = 0; c < nchunk; c++) {
        if (c + 1 < nchunk) issue(c + 1);
        __syncthreads();            // patch of chunk c visible; every wave is past its reads of the other buffer
        if (live) {
            const float *P = patch[c & 1];
#pragma unroll 1            // one tap = 64 MFMAs per wave; unrolled over the taps the compiler hoists all 18 weight loads and spills
            for (int t = 0; t < NTAP; t++) {
                // d_a[y,x] takes d_o[y - ky + 1, x - kx + 1]: patch pixel (p + 2 - ky, j + 2 - kx) with the patch origin at (-1, -1)
                const int dy = K3 ? 2 - t / 3 : 0, dx = K3 ? 2 - t % 3 : 0;
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    // K step s of this group: lane (q, j) carries co = 32 c + 16 h + 4 q + s on both operands
                    const float4 a = wt[((size_t)t * cog + c * 8 + h * 4 + q) * Cin + ci0 + j];
#pragma unroll
                    for (int p = 0; p < CT_TH; p++) {
                        const float4 bv = *reinterpret_cast<const float4 *>(&P[((p + dy) * PW + j + dx) * CT_DS + h * 16 + 4 * q]);
                        acc[p] = MFMA16(a.x, bv.x, acc[p]); acc[p] = MFMA16(a.y, bv.y, acc[p]);
                        acc[p] = MFMA16(a.z, bv.z, acc[p]); acc[p] = MFMA16(a.w, bv.w, acc[p]);
                    }
                }
                if (!K3 || t % 3 == 2) {
#pragma unroll
                    for (int p = 0; p < CT_TH; p++) { tot[p] += acc[p]; acc[p] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
                }
            }
        }
        if (c + 1 < nchunk) stage((c + 1) & 1);
    }
    if (live) {
        float *__restrict__ dib = din + (size_t)b * H * W * di_cs + di_co + ci0 + 4 * q;       // D row 4 q + r = input channel ci0 + 4 q + r, column j = pixel x
#pragma unroll
        for (int p = 0; p < CT_TH; p++)
            *reinterpret_cast<float4 *>(dib + ((size_t)(ty * CT_TH + p) * W + tx * CT_TW + j) * di_cs) = make_float4(tot[p][0], tot[p][1], tot[p][2], tot[p][3]);
    }
}

// MT: M tiles per wave (row j of tile mt is output channel cobase + MT j + mt: a lane's A values of a K step are MT consecutive floats of one pixel).
// MH waves split the output channels (64 each; 32 when MT = 2), the other 4 / MH split the workgroup's 16 * 4 / MH input channels.
template <int MT, bool K3>
__global__ __launch_bounds__(256) void wgrad_kernel(const float *__restrict__ dout, int do_cs, int do_co, const float *__restrict__ xin, int xi_cs, int xi_co,
                                                    const float2 *__restrict__ stats, const float *__restrict__ gamma, const float *__restrict__ beta, int groups,
                                                    int H, int W, int Cin, int Cout, int MH, int nsplit, int tpw, float *__restrict__ partials)
{
    constexpr int PW = K3 ? CT_PW : CT_TW, PX = K3 ? CT_PX : CT_TH * CT_TW, NTAP = K3 ? 9 : 1;
    extern __shared__ __attribute__((aligned(16))) float wpatch[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, q = lane >> 4, j = lane & 15;
    const int NH = 4 / MH, CIW = 16 * NH, LS = CIW == 64 ? 80 : 48, P4 = CIW >> 2;       // LS % 32 == 16: the four pixels of a K step read disjoint bank halves
    const int mh = wave % MH, nh = wave / MH, cobase = mh * 16 * MT, n0 = nh * 16;
    const int split = blockIdx.x, b = blockIdx.y, ci0 = blockIdx.z * CIW;
    const bool live = ci0 + n0 < Cin;
    const int tiles_x = W / CT_TW, tiles = tiles_x * (H / CT_TH);
    const int t_lo = split * tpw, t_hi = min(tiles, t_lo + tpw);
    const float *__restrict__ dob = dout + (size_t)b * H * W * do_cs + do_co + cobase + MT * j;
    const float *__restrict__ xb = xin + (size_t)b * H * W * xi_cs + xi_co;

    // this thread's four channels of the staged patch (the same in every round: P4 divides 256) and their GroupNorm + ReLU coefficients,
    // the forward's expression (conv.hip stage()): y = max(fma(x, a, s), 0), a = rstd gamma, s = beta - mean a
    const int piece = tid % P4, chb = ci0 + piece * 4;
    const bool chok = chb < Cin;
    float ga[4] = {1.f, 1.f, 1.f, 1.f}, gs[4] = {0.f, 0.f, 0.f, 0.f};
    if (stats && chok) {
        const int cg = Cin / groups;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float2 st = stats[b * groups + (chb + k) / cg];
            const float a_ = st.y * gamma[chb + k];
            ga[k] = a_; gs[k] = beta[chb + k] - st.x * a_;
        }
    }
    f32x4 acc[NTAP][MT];
#pragma unroll
    for (int t = 0; t < NTAP; t++)
#pragma unroll
        for (int mt = 0; mt < MT; mt++) acc[t][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int tile = t_lo; tile < t_hi; tile++) {
        const int tx = tile % tiles_x, ty = tile / tiles_x;
        const int y0 = ty * CT_TH - (K3 ? 1 : 0), x0 = tx * CT_TW - (K3 ? 1 : 0);
        __syncthreads();            // the readers of the previous tile's patch are done
#pragma unroll 4
        for (int it = tid; it < PX * P4; it += 256) {
            const int px = it / P4, yy = y0 + px / PW, xx = x0 + px % PW;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);      // the padding pads the RECTIFIED activation
            if (chok && yy >= 0 && yy < H && xx >= 0 && xx < W) {
                v = *reinterpret_cast<const float4 *>(xb + ((size_t)yy * W + xx) * xi_cs + chb);
                if (stats) {
                    v.x = fmaxf(__builtin_fmaf(v.x, ga[0], gs[0]), 0.f); v.y = fmaxf(__builtin_fmaf(v.y, ga[1], gs[1]), 0.f);
                    v.z = fmaxf(__builtin_fmaf(v.z, ga[2], gs[2]), 0.f); v.w = fmaxf(__builtin_fmaf(v.w, ga[3], gs[3]), 0.f);
                }
            }
            *reinterpret_cast<float4 *>(&wpatch[px * LS + piece * 4]) = v;
        }
        __syncthreads();
        if (live) {
#pragma unroll 2
            for (int s = 0; s < 32; s++) {           // K step = the four pixels (row p, columns 4 t4 + q)
                const int p = s >> 2, xc = 4 * (s & 3) + q;
                const float *ap = dob + ((size_t)(ty * CT_TH + p) * W + tx * CT_TW + xc) * do_cs;
                float a[MT];
                if constexpr (MT == 4) { const float4 v = *reinterpret_cast<const float4 *>(ap); a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w; }
                else { const float2 v = *reinterpret_cast<const float2 *>(ap); a[0] = v.x; a[1] = v.y; }
#pragma unroll
                for (int t = 0; t < NTAP; t++) {
                    const int dy = K3 ? t / 3 : 0, dx = K3 ? t % 3 : 0;
                    const float bv = wpatch[((p + dy) * PW + xc + dx) * LS + n0 + j];
#pragma unroll
                    for (int mt = 0; mt < MT; mt++) acc[t][mt] = MFMA16(a[mt], bv, acc[t][mt]);
                }
            }
        }
    }
    if (live) {
        float *__restrict__ out = partials + ((size_t)b * nsplit + split) * ((size_t)NTAP * Cout * Cin);
#pragma unroll
        for (int t = 0; t < NTAP; t++)
#pragma unroll
            for (int mt = 0; mt < MT; mt++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int co = cobase + MT * (4 * q + r) + mt;
                    out[((size_t)t * Cout + co) * Cin + ci0 + n0 + j] = acc[t][mt][r];
                }
    }
}

__global__ __launch_bounds__(256) void wfinish_kernel(const float *__restrict__ partials, long P, int nparts, int Cout, int Cin, int ntap, float *__restrict__ dW, int accumulate)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    double s = 0.0;
    for (int k = 0; k < nparts; k++) s += (double)partials[(size_t)k * P + i];
    const int ci = (int)(i % Cin); const long r = i / Cin; const int co = (int)(r % Cout), t = (int)(r / Cout);
    float *o = dW + ((size_t)co * Cin + ci) * ntap + t;
    *o = accumulate ? *o + (float)s : (float)s;
}

// ---- GroupNorm(groups) + ReLU backward --------------------------------------------------------------------------------------------------------------------
// y = max(xhat gamma + beta, 0), xhat = (x - mean) rstd.  With g = dL/dy, m = [xhat gamma + beta > 0] and n = elements of a group in one frame:
//   dbeta_c = sum g m, dgamma_c = sum g m xhat (over frames and pixels); per (frame, group) s1 = sum g m gamma, s2 = sum g m gamma xhat;
//   d_x = rstd (g m gamma - (s1 + xhat s2) / n)      (d xhat / d x = rstd (I - 1 1^T / n - xhat xhat^T / n) applied to d xhat = g m gamma).
// m is evaluated with the forward's staging expression fma(x, rstd gamma, beta - mean rstd gamma) > 0 in fp32, so both directions agree on every sign; the sums
// and the element formula run in fp64 and round once.  gnb_reduce: per (pixel block, frame, channel) the two sums -> fp64 partials; gnb_group: s1, s2 per
// (frame, group) from the partials in (block, channel) order; gnb_param: dgamma / dbeta per channel in (frame, block) order; gnb_apply: d_x = base + the formula.
__device__ __forceinline__ bool gnb_mask(float x, float2 st, float gm, float bt)
{
    const float a_ = st.y * gm;
    return __builtin_fmaf(x, a_, bt - st.x * a_) > 0.f;
}
// YM: the mask is read from the forward's saved rectified output, m = [y > 0] (vt_gn_relu_backward_y: a forward whose expression is not the staging one)
template <bool YM>
__global__ __launch_bounds__(256) void gnb_reduce_kernel(const float *__restrict__ g, int g_cs, const float *__restrict__ x, int x_cs, const float2 *__restrict__ stats,
                                                         const float *__restrict__ gamma, const float *__restrict__ beta, int groups, int HW, int C, int rows_per_block,
                                                         double *__restrict__ part, const float *__restrict__ y, int y_cs)
{
    const int C4 = C >> 2, b = blockIdx.y, c4 = threadIdx.x % C4, slot = threadIdx.x / C4, nslot = 256 / C4, cg = C / groups;
    const int p0 = blockIdx.x * rows_per_block, p1 = min(HW, p0 + rows_per_block);
    double sa[4] = {0, 0, 0, 0}, sb[4] = {0, 0, 0, 0};
    if (slot < nslot) {
        float2 st[4]; float gm[4], bt[4];
#pragma unroll
        for (int k = 0; k < 4; k++) { st[k] = stats[b * groups + (4 * c4 + k) / cg]; gm[k] = gamma[4 * c4 + k]; bt[k] = beta[4 * c4 + k]; }
        for (int p = p0 + slot; p < p1; p += nslot) {
            const float4 gv = *reinterpret_cast<const float4 *>(g + ((size_t)b * HW + p) * g_cs + 4 * c4);
            const float4 xv = *reinterpret_cast<const float4 *>(x + ((size_t)b * HW + p) * x_cs + 4 * c4);
            const float gg[4] = {gv.x, gv.y, gv.z, gv.w}, xx[4] = {xv.x, xv.y, xv.z, xv.w};
            float yy[4] = {0.f, 0.f, 0.f, 0.f};
            if constexpr (YM) { const float4 yv = *reinterpret_cast<const float4 *>(y + ((size_t)b * HW + p) * y_cs + 4 * c4); yy[0] = yv.x; yy[1] = yv.y; yy[2] = yv.z; yy[3] = yv.w; }
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (YM ? yy[k] > 0.f : gnb_mask(xx[k], st[k], gm[k], bt[k])) {
                    sa[k] += (double)gg[k];
                    sb[k] += (double)gg[k] * (((double)xx[k] - (double)st[k].x) * (double)st[k].y);
                }
        }
    }
    __shared__ double red[256 * 8];
#pragma unroll
    for (int k = 0; k < 4; k++) { red[threadIdx.x * 8 + k] = sa[k]; red[threadIdx.x * 8 + 4 + k] = sb[k]; }
    __syncthreads();
    if (threadIdx.x < C4) {
        double da[4] = {0, 0, 0, 0}, db[4] = {0, 0, 0, 0};
        for (int sl = 0; sl < nslot; sl++)
#pragma unroll
            for (int k = 0; k < 4; k++) { da[k] += red[(sl * C4 + threadIdx.x) * 8 + k]; db[k] += red[(sl * C4 + threadIdx.x) * 8 + 4 + k]; }
        double *o = part + (((size_t)blockIdx.x * gridDim.y + b) * C + 4 * threadIdx.x) * 2;
#pragma unroll
        for (int k = 0; k < 4; k++) { o[2 * k] = da[k]; o[2 * k + 1] = db[k]; }
    }
}
__global__ __launch_bounds__(64) void gnb_group_kernel(const double *__restrict__ part, int nblk, int B, int C, int groups, const float *__restrict__ gamma, double *__restrict__ gsum)
{
    const int i = blockIdx.x, b = i / groups, gi = i - b * groups, cg = C / groups, lane = threadIdx.x;
    double s1 = 0, s2 = 0;
    for (int e = lane; e < nblk * cg; e += 64) {
        const int blk = e / cg, k = e - blk * cg, c = gi * cg + k;
        const double *p = part + (((size_t)blk * B + b) * C + c) * 2;
        const double gm = (double)gamma[c];
        s1 += gm * p[0]; s2 += gm * p[1];
    }
    for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }
    if (lane == 0) { gsum[2 * i] = s1; gsum[2 * i + 1] = s2; }
}
__global__ __launch_bounds__(64) void gnb_param_kernel(const double *__restrict__ part, int nblk, int B, int C, float *__restrict__ dgamma, float *__restrict__ dbeta, int accumulate)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    double sa = 0, sb = 0;
    for (int b = 0; b < B; b++)
        for (int blk = 0; blk < nblk; blk++) { const double *p = part + (((size_t)blk * B + b) * C + c) * 2; sa += p[0]; sb += p[1]; }
    if (dbeta) dbeta[c] = accumulate ? dbeta[c] + (float)sa : (float)sa;
    if (dgamma) dgamma[c] = accumulate ? dgamma[c] + (float)sb : (float)sb;
}
template <bool YM>
__global__ __launch_bounds__(256) void gnb_apply_kernel(const float *__restrict__ g, int g_cs, const float *__restrict__ x, int x_cs, const float2 *__restrict__ stats,
                                                        const float *__restrict__ gamma, const float *__restrict__ beta, const double *__restrict__ gsum, int groups,
                                                        int B, int HW, int C, const float *base, int base_cs, float *dx, int dx_cs, const float *__restrict__ y, int y_cs)
{
    const int C4 = C >> 2, cg = C / groups;
    const long t = (long)blockIdx.x * 256 + threadIdx.x, total = (long)B * HW * C4;
    if (t >= total) return;
    const int c4 = (int)(t % C4); const long pix = t / C4; const int b = (int)(pix / HW);
    const float4 gv = *reinterpret_cast<const float4 *>(g + pix * g_cs + 4 * c4);
    const float4 xv = *reinterpret_cast<const float4 *>(x + pix * x_cs + 4 * c4);
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (base) bv = *reinterpret_cast<const float4 *>(base + pix * base_cs + 4 * c4);       // may alias dx: each element is read and written by this thread only
    const float gg[4] = {gv.x, gv.y, gv.z, gv.w}, xx[4] = {xv.x, xv.y, xv.z, xv.w}, bb[4] = {bv.x, bv.y, bv.z, bv.w};
    float yy[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (YM) { const float4 yv = *reinterpret_cast<const float4 *>(y + pix * y_cs + 4 * c4); yy[0] = yv.x; yy[1] = yv.y; yy[2] = yv.z; yy[3] = yv.w; }
    const double inv_n = 1.0 / ((double)HW * cg);
    float o[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int c = 4 * c4 + k, gi = b * groups + c / cg;
        const float2 st = stats[gi];
        const float gm = gamma[c];
        const double xhat = ((double)xx[k] - (double)st.x) * (double)st.y;
        const double e = (YM ? yy[k] > 0.f : gnb_mask(xx[k], st, gm, beta[c])) ? (double)gg[k] * (double)gm : 0.0;
        const float d = (float)((double)st.y * (e - (gsum[2 * gi] + xhat * gsum[2 * gi + 1]) * inv_n));
        o[k] = base ? bb[k] + d : d;
    }
    *reinterpret_cast<float4 *>(dx + pix * dx_cs + 4 * c4) = make_float4(o[0], o[1], o[2], o[3]);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------------------
static int gnb_blocks(int HW) { const int n = (HW + 63) / 64; return n < 1 ? 1 : (n > CT_GNB_MAXBLK ? CT_GNB_MAXBLK : n); }
static int wgrad_splits(int B, int tiles) { int s = 128 / B; s = s < 1 ? 1 : (s > 8 ? 8 : s); return s < tiles ? s : tiles; }
static long gnb_ws_bytes(int B, int HW, int C, int groups) { return (long)align256(((size_t)gnb_blocks(HW) * B * C * 2 + (size_t)B * groups * 2) * sizeof(double)); }
static long dgrad_ws_bytes(int cout, int cin, int ntap) { return (long)align256((size_t)cout * cin * ntap * sizeof(float)); }
static long wgrad_ws_bytes(int B, int H, int W, int cout, int cin, int ntap)
{
    return (long)align256((size_t)B * wgrad_splits(B, (H / CT_TH) * (W / CT_TW)) * cout * cin * ntap * sizeof(float));
}
static bool shape_ok(int B, int H, int W) { return B > 0 && B <= 65535 && H > 0 && W > 0 && H % CT_TH == 0 && W % CT_TW == 0; }
static bool slice_ok(const void *p, int cstride, int coff, int c)
{
    return p && coff >= 0 && cstride >= coff + c && cstride % 4 == 0 && coff % 4 == 0 && ((uintptr_t)p & 15) == 0;
}
static bool k3_ok(int cout, int cin) { return (cout == 32 || cout == 64 || cout == 128) && cin >= 32 && cin <= 256 && cin % 32 == 0; }
static bool k1_ok(int cout, int cin) { return (cout == 64 || cout == 128 || cout == 256) && cin >= 32 && cin <= 256 && cin % 32 == 0; }

static int dgrad(bool k3, const float *weight, int cout, int cin, const float *d_out, int do_cs, int do_co, int B, int H, int W, float *d_in, int di_cs, int di_co,
                 void *ws, hipStream_t st)
{
    const int ntap = k3 ? 9 : 1;
    const long n = (long)cout * cin * ntap;
    float *wt = static_cast<float *>(ws);
    hipLaunchKernelGGL(wtrans_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, weight, cout, cin, ntap, wt);
    const dim3 grid((H / CT_TH) * (W / CT_TW), B, (cin + 63) / 64);
    if (k3) hipLaunchKernelGGL(dgrad_kernel<true>, grid, dim3(256), 0, st, reinterpret_cast<const float4 *>(wt), cout, cin, d_out, do_cs, do_co, H, W, d_in, di_cs, di_co);
    else hipLaunchKernelGGL(dgrad_kernel<false>, grid, dim3(256), 0, st, reinterpret_cast<const float4 *>(wt), cout, cin, d_out, do_cs, do_co, H, W, d_in, di_cs, di_co);
    VT_LAUNCH_CHECK();
    return VT_OK;
}
static int wgrad(bool k3, const float *d_out, int do_cs, int do_co, const float *x_in, int xi_cs, int xi_co, const float *gn_stats, const float *gamma, const float *beta,
                 int groups, int B, int H, int W, int cin, int cout, float *dW, int accumulate, void *ws, hipStream_t st)
{
    const int ntap = k3 ? 9 : 1, tiles = (H / CT_TH) * (W / CT_TW), ns = wgrad_splits(B, tiles), tpw = (tiles + ns - 1) / ns;
    const int mt = cout == 32 ? 2 : 4, mh = cout <= 64 ? 1 : cout / 64, ciw = 16 * (4 / mh), ls = ciw == 64 ? 80 : 48;
    const size_t lds = (size_t)(k3 ? CT_PX : CT_TH * CT_TW) * ls * sizeof(float);
    const dim3 grid(ns, B, (cin + ciw - 1) / ciw);
    float *part = static_cast<float *>(ws);
    const float2 *st2 = reinterpret_cast<const float2 *>(gn_stats);
#define CT_WG(MT_, K3_) hipLaunchKernelGGL((wgrad_kernel<MT_, K3_>), grid, dim3(256), lds, st, d_out, do_cs, do_co, x_in, xi_cs, xi_co, st2, gamma, beta, groups, H, W, cin, cout, mh, ns, tpw, part)
    if (k3) { if (mt == 2) CT_WG(2, true); else CT_WG(4, true); }
    else { if (mt == 2) CT_WG(2, false); else CT_WG(4, false); }
#undef CT_WG
    const long P = (long)ntap * cout * cin;
    hipLaunchKernelGGL(wfinish_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, part, P, B * ns, cout, cin, ntap, dW, accumulate);
    VT_LAUNCH_CHECK();
    return VT_OK;
}
static int gnb(const float *g, int g_cs, const float *x, int x_cs, const float *gn_stats, const float *gamma, const float *beta, int groups, int B, int HW, int C,
               const float *base, int base_cs, float *dx, int dx_cs, float *dgamma, float *dbeta, int accumulate, void *ws, hipStream_t st,
               const float *y = nullptr, int y_cs = 0)
{
    const int nblk = gnb_blocks(HW), rows = (HW + nblk - 1) / nblk;
    double *part = static_cast<double *>(ws), *gsum = part + (size_t)nblk * B * C * 2;
    const float2 *st2 = reinterpret_cast<const float2 *>(gn_stats);
    if (y) hipLaunchKernelGGL(gnb_reduce_kernel<true>, dim3(nblk, B), dim3(256), 0, st, g, g_cs, x, x_cs, st2, gamma, beta, groups, HW, C, rows, part, y, y_cs);
    else hipLaunchKernelGGL(gnb_reduce_kernel<false>, dim3(nblk, B), dim3(256), 0, st, g, g_cs, x, x_cs, st2, gamma, beta, groups, HW, C, rows, part, y, y_cs);
    if (dgamma || dbeta) hipLaunchKernelGGL(gnb_param_kernel, dim3((C + 63) / 64), dim3(64), 0, st, part, nblk, B, C, dgamma, dbeta, accumulate);
    if (dx) {
        hipLaunchKernelGGL(gnb_group_kernel, dim3(B * groups), dim3(64), 0, st, part, nblk, B, C, groups, gamma, gsum);
        const long total = (long)B * HW * (C >> 2);
        const dim3 ag((unsigned)((total + 255) / 256));
        if (y) hipLaunchKernelGGL(gnb_apply_kernel<true>, ag, dim3(256), 0, st, g, g_cs, x, x_cs, st2, gamma, beta, gsum, groups, B, HW, C, base, base_cs, dx, dx_cs, y, y_cs);
        else hipLaunchKernelGGL(gnb_apply_kernel<false>, ag, dim3(256), 0, st, g, g_cs, x, x_cs, st2, gamma, beta, gsum, groups, B, HW, C, base, base_cs, dx, dx_cs, y, y_cs);
    }
    VT_LAUNCH_CHECK();
    return VT_OK;
}

}  // namespace convt

extern "C" {

long vt_conv_dgrad_workspace_bytes(int cout, int cin, int taps)
{
    if (!(taps == 9 ? convt::k3_ok(cout, cin) : (taps == 1 && convt::k1_ok(cout, cin)))) return -1;
    return convt::dgrad_ws_bytes(cout, cin, taps);
}
long vt_conv_wgrad_workspace_bytes(int B, int H, int W, int cout, int cin, int taps)
{
    if (!convt::shape_ok(B, H, W) || !(taps == 9 ? convt::k3_ok(cout, cin) : (taps == 1 && convt::k1_ok(cout, cin)))) return -1;
    return convt::wgrad_ws_bytes(B, H, W, cout, cin, taps);
}
long vt_gn_relu_backward_workspace_bytes(int B, int HW, int C, int groups)
{
    if (B <= 0 || B > 65535 || HW <= 0 || C < 4 || C > 1024 || C % 4 != 0 || groups <= 0 || C % groups != 0) return -1;
    return convt::gnb_ws_bytes(B, HW, C, groups);
}

int vt_conv3x3_dgrad(const float *weight, int cout, int cin, const float *d_out, int do_cstride, int do_coff, int B, int H, int W,
                     float *d_in, int di_cstride, int di_coff, void *workspace, void *stream)
{
    VT_REQUIRE(weight && workspace && convt::k3_ok(cout, cin), "vt_conv3x3_dgrad: needs Cout in {32, 64, 128} and Cin a multiple of 32 up to 256");
    VT_REQUIRE(convt::shape_ok(B, H, W), "vt_conv3x3_dgrad: needs H %% 8 == 0, W %% 16 == 0, 0 < B <= 65535");
    VT_REQUIRE(convt::slice_ok(d_out, do_cstride, do_coff, cout) && convt::slice_ok(d_in, di_cstride, di_coff, cin), "vt_conv3x3_dgrad: needs 16-byte aligned channel slices");
    return convt::dgrad(true, weight, cout, cin, d_out, do_cstride, do_coff, B, H, W, d_in, di_cstride, di_coff, workspace, vt_stream(stream));
}
int vt_conv1x1_dgrad(const float *weight, int cout, int cin, const float *d_out, int do_cstride, int do_coff, int B, int H, int W,
                     float *d_in, int di_cstride, int di_coff, void *workspace, void *stream)
{
    VT_REQUIRE(weight && workspace && convt::k1_ok(cout, cin), "vt_conv1x1_dgrad: needs Cout in {64, 128, 256} and Cin a multiple of 32 up to 256");
    VT_REQUIRE(convt::shape_ok(B, H, W), "vt_conv1x1_dgrad: needs H %% 8 == 0, W %% 16 == 0, 0 < B <= 65535");
    VT_REQUIRE(convt::slice_ok(d_out, do_cstride, do_coff, cout) && convt::slice_ok(d_in, di_cstride, di_coff, cin), "vt_conv1x1_dgrad: needs 16-byte aligned channel slices");
    return convt::dgrad(false, weight, cout, cin, d_out, do_cstride, do_coff, B, H, W, d_in, di_cstride, di_coff, workspace, vt_stream(stream));
}
int vt_conv3x3_wgrad(const float *d_out, int do_cstride, int do_coff, const float *x_in, int xi_cstride, int xi_coff, const float *gn_stats, const float *gamma,
                     const float *beta, int groups, int B, int H, int W, int cin, int cout, float *dW, int accumulate, void *workspace, void *stream)
{
    VT_REQUIRE(dW && workspace && convt::k3_ok(cout, cin), "vt_conv3x3_wgrad: needs Cout in {32, 64, 128} and Cin a multiple of 32 up to 256");
    VT_REQUIRE(convt::shape_ok(B, H, W), "vt_conv3x3_wgrad: needs H %% 8 == 0, W %% 16 == 0, 0 < B <= 65535");
    VT_REQUIRE(convt::slice_ok(d_out, do_cstride, do_coff, cout) && convt::slice_ok(x_in, xi_cstride, xi_coff, cin), "vt_conv3x3_wgrad: needs 16-byte aligned channel slices");
    VT_REQUIRE(!gn_stats || (gamma && beta && groups > 0 && cin % groups == 0), "vt_conv3x3_wgrad: the GroupNorm prologue needs gamma, beta and Cin %% groups == 0");
    return convt::wgrad(true, d_out, do_cstride, do_coff, x_in, xi_cstride, xi_coff, gn_stats, gamma, beta, groups, B, H, W, cin, cout, dW, accumulate, workspace, vt_stream(stream));
}
int vt_conv1x1_wgrad(const float *d_out, int do_cstride, int do_coff, const float *x_in, int xi_cstride, int xi_coff, const float *gn_stats, const float *gamma,
                     const float *beta, int groups, int B, int H, int W, int cin, int cout, float *dW, int accumulate, void *workspace, void *stream)
{
    VT_REQUIRE(dW && workspace && convt::k1_ok(cout, cin), "vt_conv1x1_wgrad: needs Cout in {64, 128, 256} and Cin a multiple of 32 up to 256");
    VT_REQUIRE(convt::shape_ok(B, H, W), "vt_conv1x1_wgrad: needs H %% 8 == 0, W %% 16 == 0, 0 < B <= 65535");
    VT_REQUIRE(convt::slice_ok(d_out, do_cstride, do_coff, cout) && convt::slice_ok(x_in, xi_cstride, xi_coff, cin), "vt_conv1x1_wgrad: needs 16-byte aligned channel slices");
    VT_REQUIRE(!gn_stats || (gamma && beta && groups > 0 && cin % groups == 0), "vt_conv1x1_wgrad: the GroupNorm prologue needs gamma, beta and Cin %% groups == 0");
    return convt::wgrad(false, d_out, do_cstride, do_coff, x_in, xi_cstride, xi_coff, gn_stats, gamma, beta, groups, B, H, W, cin, cout, dW, accumulate, workspace, vt_stream(stream));
}
int vt_gn_relu_backward(const float *g, int g_cstride, int g_coff, const float *x_in, int x_cstride, int x_coff, const float *gn_stats, const float *gamma,
                        const float *beta, int groups, int B, int HW, int C, const float *base, int base_cstride, int base_coff,
                        float *d_x, int dx_cstride, int dx_coff, float *dgamma, float *dbeta, int accumulate, void *workspace, void *stream)
{
    VT_REQUIRE(gn_stats && gamma && beta && workspace && B > 0 && B <= 65535 && HW > 0 && C >= 4 && C <= 1024 && C % 4 == 0 && groups > 0 && C % groups == 0,
               "vt_gn_relu_backward: needs statistics, gamma, beta, a workspace, C %% 4 == 0, C <= 1024 and C %% groups == 0");
    VT_REQUIRE(convt::slice_ok(g, g_cstride, g_coff, C) && convt::slice_ok(x_in, x_cstride, x_coff, C), "vt_gn_relu_backward: needs 16-byte aligned channel slices");
    VT_REQUIRE(d_x || dgamma || dbeta, "vt_gn_relu_backward: nothing to compute");
    VT_REQUIRE(!d_x || convt::slice_ok(d_x, dx_cstride, dx_coff, C), "vt_gn_relu_backward: bad d_x slice");
    VT_REQUIRE(!base || (d_x && convt::slice_ok(base, base_cstride, base_coff, C)), "vt_gn_relu_backward: bad base slice");
    return convt::gnb(g + g_coff, g_cstride, x_in + x_coff, x_cstride, gn_stats, gamma, beta, groups, B, HW, C, base ? base + base_coff : nullptr, base_cstride,
                      d_x ? d_x + dx_coff : nullptr, dx_cstride, dgamma, dbeta, accumulate, workspace, vt_stream(stream));
}
// the same passes with m = [y > 0] read from the forward's saved output (the stem's bn1 + ReLU runs on vt_groupnorm_nhwc, whose expression is not the staging one)
int vt_gn_relu_backward_y(const float *g, int g_cstride, int g_coff, const float *x_in, int x_cstride, int x_coff, const float *y, int y_cstride, int y_coff,
                          const float *gn_stats, const float *gamma, int groups, int B, int HW, int C, const float *base, int base_cstride, int base_coff,
                          float *d_x, int dx_cstride, int dx_coff, float *dgamma, float *dbeta, int accumulate, void *workspace, void *stream)
{
    VT_REQUIRE(gn_stats && gamma && workspace && B > 0 && B <= 65535 && HW > 0 && C >= 4 && C <= 1024 && C % 4 == 0 && groups > 0 && C % groups == 0,
               "vt_gn_relu_backward_y: needs statistics, gamma, a workspace, C %% 4 == 0, C <= 1024 and C %% groups == 0");
    VT_REQUIRE(convt::slice_ok(g, g_cstride, g_coff, C) && convt::slice_ok(x_in, x_cstride, x_coff, C) && convt::slice_ok(y, y_cstride, y_coff, C),
               "vt_gn_relu_backward_y: needs 16-byte aligned channel slices");
    VT_REQUIRE(d_x || dgamma || dbeta, "vt_gn_relu_backward_y: nothing to compute");
    VT_REQUIRE(!d_x || convt::slice_ok(d_x, dx_cstride, dx_coff, C), "vt_gn_relu_backward_y: bad d_x slice");
    VT_REQUIRE(!base || (d_x && convt::slice_ok(base, base_cstride, base_coff, C)), "vt_gn_relu_backward_y: bad base slice");
    // beta only enters the mask, which comes from y here: gamma stands in for the pointer the shared passes never read in this form
    return convt::gnb(g + g_coff, g_cstride, x_in + x_coff, x_cstride, gn_stats, gamma, gamma, groups, B, HW, C, base ? base + base_coff : nullptr, base_cstride,
                      d_x ? d_x + dx_coff : nullptr, dx_cstride, dgamma, dbeta, accumulate, workspace, vt_stream(stream), y + y_coff, y_cstride);
}

// workspace of the block: G (the gradient to a rectified activation, the widest of Cin and c1 channels), D (d_o1 | d_o2 = the dy slices + what the later
// convolutions send back), and one area shared by the transposed weights, the split-K partials and the GroupNorm partial sums of whichever kernel runs
static bool block_ok(int B, int H, int W, int cin, int c1, int c2, int c3, bool proj)
{
    const int ct = c1 + c2 + c3;
    return convt::shape_ok(B, H, W) && convt::k3_ok(c1, cin) && convt::k3_ok(c2, c1) && convt::k3_ok(c3, c2) && (proj ? convt::k1_ok(ct, cin) : ct == cin);
}
static size_t block_shared_bytes(int B, int H, int W, int cin, int c1, int c2, int c3)
{
    const int ct = c1 + c2 + c3, cw = cin > c1 ? cin : c1;
    long m = convt::gnb_ws_bytes(B, H * W, cw, 32);
    const int lay[4][3] = {{c1, cin, 9}, {c2, c1, 9}, {c3, c2, 9}, {ct, cin, 1}};
    for (int i = 0; i < 4; i++) {
        const long a = convt::dgrad_ws_bytes(lay[i][0], lay[i][1], lay[i][2]), b = convt::wgrad_ws_bytes(B, H, W, lay[i][0], lay[i][1], lay[i][2]);
        m = a > m ? a : m; m = b > m ? b : m;
    }
    return (size_t)m;
}
long vt_conv_block_backward_workspace(int B, int H, int W, int cin, int c1, int c2, int c3)
{
    if (!(block_ok(B, H, W, cin, c1, c2, c3, true) || block_ok(B, H, W, cin, c1, c2, c3, false))) return -1;
    const size_t px = (size_t)B * H * W;
    return (long)(convt::align256(px * (cin > c1 ? cin : c1) * sizeof(float)) + convt::align256(px * (c1 + c2) * sizeof(float)) + block_shared_bytes(B, H, W, cin, c1, c2, c3));
}
int vt_conv_block_backward(const float *dy, const float *x, const float *raw, const float *stats1, const float *stats2, const float *stats3,
                           const float *w1, const float *w2, const float *w3, const float *gamma1, const float *gamma2, const float *gamma3,
                           const float *beta1, const float *beta2, const float *beta3, const float *wproj, const float *gamma4, const float *beta4,
                           int B, int H, int W, int cin, int c1, int c2, int c3,
                           float *d_x, float *dW1, float *dW2, float *dW3, float *dgamma1, float *dbeta1, float *dgamma2, float *dbeta2, float *dgamma3, float *dbeta3,
                           float *dgamma4, float *dbeta4, float *dWproj, void *workspace, int accumulate, void *stream)
{
    VT_REQUIRE(dy && x && raw && stats1 && stats2 && stats3 && w1 && w2 && w3 && gamma1 && gamma2 && gamma3 && beta1 && beta2 && beta3 && workspace,
               "vt_conv_block_backward: null input");
    VT_REQUIRE(!wproj || (gamma4 && beta4), "vt_conv_block_backward: the projection needs gamma4 and beta4");
    VT_REQUIRE(block_ok(B, H, W, cin, c1, c2, c3, wproj != nullptr),
               "vt_conv_block_backward: needs H %% 8 == 0, W %% 16 == 0, convolution widths in {32, 64, 128}, Cin %% 32 == 0 up to 256, and a projection exactly when Cin != Cout");
    VT_REQUIRE((((uintptr_t)dy | (uintptr_t)x | (uintptr_t)raw | (uintptr_t)workspace | (uintptr_t)d_x) & 15) == 0, "vt_conv_block_backward: tensors must be 16-byte aligned");
    VT_REQUIRE(wproj || !(dgamma4 || dbeta4 || dWproj), "vt_conv_block_backward: projection gradients requested from a block without a projection");
    hipStream_t st = vt_stream(stream);
    const int ct = c1 + c2 + c3, cr = c1 + c2, HW = H * W, cw = cin > c1 ? cin : c1;
    const size_t px = (size_t)B * HW;
    char *wsb = static_cast<char *>(workspace);
    float *G = reinterpret_cast<float *>(wsb);
    float *D = reinterpret_cast<float *>(wsb + convt::align256(px * cw * sizeof(float)));
    void *S = wsb + convt::align256(px * cw * sizeof(float)) + convt::align256(px * cr * sizeof(float));
    int rc;
#define CT_TRY(call_) do { rc = (call_); if (rc) return rc; } while (0)
    // conv3 (net_util.py:385-387): d_o3 is the last slice of dy
    if (dW3) CT_TRY(convt::wgrad(true, dy, ct, cr, raw, cr, c1, stats3, gamma3, beta3, 32, B, H, W, c2, c3, dW3, accumulate, S, st));
    CT_TRY(convt::dgrad(true, w3, c3, c2, dy, ct, cr, B, H, W, G, c2, 0, S, st));
    // d_o2 = dy[c1 : c1 + c2] + the backward of bn3 + ReLU (net_util.py:381-389)
    CT_TRY(convt::gnb(G, c2, raw + c1, cr, stats3, gamma3, beta3, 32, B, HW, c2, dy + c1, ct, D + c1, cr, dgamma3, dbeta3, accumulate, S, st));
    if (dW2) CT_TRY(convt::wgrad(true, D, cr, c1, raw, cr, 0, stats2, gamma2, beta2, 32, B, H, W, c1, c2, dW2, accumulate, S, st));
    CT_TRY(convt::dgrad(true, w2, c2, c1, D, cr, c1, B, H, W, G, c1, 0, S, st));
    // d_o1 = dy[0 : c1] + the backward of bn2 + ReLU (net_util.py:377-389)
    CT_TRY(convt::gnb(G, c1, raw, cr, stats2, gamma2, beta2, 32, B, HW, c1, dy, ct, D, cr, dgamma2, dbeta2, accumulate, S, st));
    if (dW1) CT_TRY(convt::wgrad(true, D, cr, 0, x, cin, 0, stats1, gamma1, beta1, 32, B, H, W, cin, c1, dW1, accumulate, S, st));
    if (d_x || dgamma1 || dbeta1) {
        CT_TRY(convt::dgrad(true, w1, c1, cin, D, cr, 0, B, H, W, G, cin, 0, S, st));
        // identity residual (net_util.py:375, 394): d_x = dy + the backward of bn1 + ReLU; with a projection the residual's share is added below
        CT_TRY(convt::gnb(G, cin, x, cin, stats1, gamma1, beta1, 32, B, HW, cin, wproj ? nullptr : dy, ct, d_x, cin, dgamma1, dbeta1, accumulate, S, st));
    }
    if (wproj) {    // downsample = bn4 -> ReLU -> conv1x1 (net_util.py:364-370, 391-392); bn4 normalises x as bn1 does: the same {mean, rstd}
        if (dWproj) CT_TRY(convt::wgrad(false, dy, ct, 0, x, cin, 0, stats1, gamma4, beta4, 32, B, H, W, cin, ct, dWproj, accumulate, S, st));
        if (d_x || dgamma4 || dbeta4) {
            CT_TRY(convt::dgrad(false, wproj, ct, cin, dy, ct, 0, B, H, W, G, cin, 0, S, st));
            CT_TRY(convt::gnb(G, cin, x, cin, stats1, gamma4, beta4, 32, B, HW, cin, d_x, cin, d_x, cin, dgamma4, dbeta4, accumulate, S, st));
        }
    }
#undef CT_TRY
    return VT_OK;
}

}  // extern "C"
