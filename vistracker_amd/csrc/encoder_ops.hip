// encoder_ops.hip -- the element-wise passes of the image encoders (encoder.py) around the convolutions of conv.hip / stem.hip: layout conversion,
// bicubic up-sampling, GroupNorm statistics / finalize / apply, and the pooling / up-sampling producers that leave GroupNorm partial sums behind.
#include "common.h"
#include "cubic.h"

// NCHW -> NHWC, 32x32 LDS tile transpose per frame: src viewed as [C][HW], dst as [HW][C]
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const float *__restrict__ src, int C, int HW, float *__restrict__ dst)
{
    __shared__ float tile[32][33];
    const size_t base = (size_t)blockIdx.z * C * HW;
    const int p0 = blockIdx.x * 32, c0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8) { const int c = c0 + i, p = p0 + tx; tile[i][tx] = (c < C && p < HW) ? src[base + (size_t)c * HW + p] : 0.f; }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) { const int p = p0 + i, c = c0 + tx; if (p < HW && c < C) dst[base + (size_t)p * C + c] = tile[tx][i]; }
}
extern "C" int vt_nchw_to_nhwc(const float *src, int B, int C, int H, int W, float *dst, void *stream)
{
    VT_REQUIRE(src && dst && B > 0 && C > 0 && H > 0 && W > 0, "vt_nchw_to_nhwc: bad argument");
    const int HW = H * W;
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3((HW + 31) / 32, (C + 31) / 32, B), dim3(256), 0, vt_stream(stream), src, C, HW, dst);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

// ---------------------------------------------------------------------------------------------------
// x2 bicubic upsampling (align_corners = True, A = -0.75, clamped taps: torch.nn.functional.interpolate semantics) of an NHWC tensor,
// fused with the skip connection of the hourglass: out = skip + up(low)   (model/HGFilters.py:45-47).
// thread = one output pixel x 4 channels (16-B accesses; the 16 taps of neighbouring threads hit the same cache lines).
// ---------------------------------------------------------------------------------------------------
// cubic_w: cubic.h (shared with the transpose, resample_bwd.hip)
__global__ __launch_bounds__(256) void upsample2x_bicubic_add_kernel(const float *__restrict__ low, const float *__restrict__ skip, int B, int h, int w, int C,
                                                                     float *__restrict__ out)
{
    const int C4 = C >> 2, H = 2 * h, W = 2 * w;
    const long t = (long)blockIdx.x * 256 + threadIdx.x, total = (long)B * H * W * C4;
    if (t >= total) return;
    const int c4 = (int)(t % C4); long r = t / C4;
    const int ox = (int)(r % W); r /= W;
    const int oy = (int)(r % H); const int b = (int)(r / H);
    const float sy = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f, sx = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
    const float fy = sy * oy, fx = sx * ox;
    const int iy = (int)floorf(fy), ix = (int)floorf(fx);
    float wy[4], wx[4];
    cubic_w(fy - iy, wy); cubic_w(fx - ix, wx);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int yy = min(max(iy - 1 + i, 0), h - 1);
        float4 row = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int xx = min(max(ix - 1 + k, 0), w - 1);
            const float4 v = *reinterpret_cast<const float4 *>(low + (((size_t)b * h + yy) * w + xx) * C + 4 * c4);
            row.x += wx[k] * v.x; row.y += wx[k] * v.y; row.z += wx[k] * v.z; row.w += wx[k] * v.w;
        }
        acc.x += wy[i] * row.x; acc.y += wy[i] * row.y; acc.z += wy[i] * row.z; acc.w += wy[i] * row.w;
    }
    const size_t o = (((size_t)b * H + oy) * W + ox) * C + 4 * c4;
    if (skip) { const float4 s = *reinterpret_cast<const float4 *>(skip + o); acc.x += s.x; acc.y += s.y; acc.z += s.z; acc.w += s.w; }
    *reinterpret_cast<float4 *>(out + o) = acc;
}
// ---------------------------------------------------------------------------------------------------
// GroupNorm (+ ReLU) on an NHWC tensor in two passes over x instead of torch's five (moments; normalise + affine; ReLU as a
// separate element-wise kernel): pass 1 accumulates per-(frame, channel) sum / sum of squares in fp64, pass 2 normalises with the
// group statistics and clamps.  The pre-activated blocks of the encoder are GN -> ReLU -> conv (model/net_util.py:374-388).
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gn_stats_kernel(const float *__restrict__ x, int cstride, int HW, int C, int rows_per_block, double *__restrict__ part)
{
    // thread = (pixel row slot, float4 of channels): C/4 float4 per pixel, 256 / (C/4) pixels per sweep
    const int C4 = C >> 2, b = blockIdx.y, c4 = threadIdx.x % C4, slot = threadIdx.x / C4, nslot = 256 / C4;
    const int p0 = blockIdx.x * rows_per_block, p1 = min(HW, p0 + rows_per_block);
    float s[4] = {0.f, 0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f};
    if (slot < nslot)
        for (int p = p0 + slot; p < p1; p += nslot) {
            const float4 v = *reinterpret_cast<const float4 *>(x + ((size_t)b * HW + p) * cstride + 4 * c4);
            s[0] += v.x; s[1] += v.y; s[2] += v.z; s[3] += v.w;
            q[0] += v.x * v.x; q[1] += v.y * v.y; q[2] += v.z * v.z; q[3] += v.w * v.w;
        }
    // combine the pixel slots of a channel through LDS; one fp64 partial per (block, frame, channel, statistic): no atomics, nothing to zero,
    // and the result does not depend on the order in which the blocks ran
    __shared__ float red[256 * 8];
#pragma unroll
    for (int k = 0; k < 4; k++) { red[threadIdx.x * 8 + k] = s[k]; red[threadIdx.x * 8 + 4 + k] = q[k]; }
    __syncthreads();
    if (threadIdx.x < C4) {
        double ds[4] = {0, 0, 0, 0}, dq[4] = {0, 0, 0, 0};
        for (int sl = 0; sl < nslot; sl++)
#pragma unroll
            for (int k = 0; k < 4; k++) { ds[k] += (double)red[(sl * C4 + threadIdx.x) * 8 + k]; dq[k] += (double)red[(sl * C4 + threadIdx.x) * 8 + 4 + k]; }
        double *o = part + (((size_t)blockIdx.x * gridDim.y + b) * C + 4 * threadIdx.x) * 2;
#pragma unroll
        for (int k = 0; k < 4; k++) { o[2 * k] = ds[k]; o[2 * k + 1] = dq[k]; }
    }
}
// per (frame, group), one wave: mean and 1 / sqrt(var + eps) from the block partials (fp64, fixed order), two floats at stats[b * groups + g]
__global__ __launch_bounds__(64) void gn_finalize_kernel(const double *__restrict__ part, int nblk, int B, int HW, int C, int groups, float eps, float2 *__restrict__ stats)
{
    const int i = blockIdx.x, b = i / groups, g = i - b * groups, cg = C / groups, lane = threadIdx.x;
    double sm = 0, sq = 0;
    for (int e = lane; e < nblk * cg; e += 64) {
        const int blk = e / cg, k = e - blk * cg;
        const double *p = part + (((size_t)blk * B + b) * C + g * cg + k) * 2;
        sm += p[0]; sq += p[1];
    }
    for (int o = 32; o > 0; o >>= 1) { sm += __shfl_xor(sm, o, 64); sq += __shfl_xor(sq, o, 64); }
    if (lane == 0) {
        const double n = (double)HW * cg, mean = sm / n, var = fmax(sq / n - mean * mean, 0.0);
        stats[i] = make_float2((float)mean, (float)(1.0 / sqrt(var + (double)eps)));
    }
}
__global__ __launch_bounds__(256) void gn_apply_kernel(const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                       const float2 *__restrict__ stats, int B, int HW, int C, int groups, int relu,
                                                       float *__restrict__ y)
{
    const int C4 = C >> 2, cg = C / groups;
    const long t = (long)blockIdx.x * 256 + threadIdx.x, total = (long)B * HW * C4;
    if (t >= total) return;
    const int c4 = (int)(t % C4); const long pix = t / C4; const int b = (int)(pix / HW);
    const float4 v = *reinterpret_cast<const float4 *>(x + pix * C + 4 * c4);
    const float4 ga = *reinterpret_cast<const float4 *>(gamma + 4 * c4), be = *reinterpret_cast<const float4 *>(beta + 4 * c4);
    const float in[4] = {v.x, v.y, v.z, v.w}, gm[4] = {ga.x, ga.y, ga.z, ga.w}, bt[4] = {be.x, be.y, be.z, be.w}; float out[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float2 st = stats[b * groups + (4 * c4 + k) / cg];
        const float o = (in[k] - st.x) * st.y * gm[k] + bt[k];
        out[k] = relu ? fmaxf(o, 0.f) : o;
    }
    *reinterpret_cast<float4 *>(y + pix * C + 4 * c4) = make_float4(out[0], out[1], out[2], out[3]);
}
// Producers that leave the GroupNorm partial sums of their OUTPUT behind (layout of gn_stats_kernel: one block of (B, C) x {sum, sum of squares} per
// workgroup), so that the ConvBlock that reads the tensor next calls vt_groupnorm_finalize instead of a statistics pass over it:
//   OP 0: 2 x 2 average pooling (F.avg_pool2d(x, 2, stride=2): model/HGFilters.py:33, 131-136), x (B, 2h, 2w, C) -> (B, h, w, C)
//   OP 1: skip + bicubic x2 up-sampling of low (upsample2x_bicubic_add_kernel's arithmetic), low (B, h / 2, w / 2, C), skip / out (B, h, w, C)
// grid = (blocks of output pixels, B); thread = (pixel slot, float4 of channels) like gn_stats_kernel.
template <int OP>
__global__ __launch_bounds__(256) void sweep_stats_kernel(const float *__restrict__ a, const float *__restrict__ skip, int h, int w, int C, int rows_per_block,
                                                          float *__restrict__ out, double *__restrict__ part)
{
    // (h, w) = the output size.  OP 0: a block item is an output pixel; OP 1: an output QUAD (2 x 2 pixels = one pixel of `low`): its four pixels read
    // their 4 x 4 taps from one 5 x 5 patch of `low` (the tap bases of neighbouring output pixels differ by at most one), 25 loads instead of 64
    const int C4 = C >> 2, b = blockIdx.y, c4 = threadIdx.x % C4, slot = threadIdx.x / C4, nslot = 256 / C4, HW = h * w;
    const int lh = h >> 1, lw = w >> 1, items = OP == 0 ? HW : lh * lw;
    const int p0 = blockIdx.x * rows_per_block, p1 = min(items, p0 + rows_per_block);
    float s[4] = {0.f, 0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f};
    auto emit = [&](int oy, int ox, const float4 v) {
        *reinterpret_cast<float4 *>(out + ((size_t)b * HW + (size_t)oy * w + ox) * C + 4 * c4) = v;
        s[0] += v.x; s[1] += v.y; s[2] += v.z; s[3] += v.w;
        q[0] += v.x * v.x; q[1] += v.y * v.y; q[2] += v.z * v.z; q[3] += v.w * v.w;
    };
    if (slot < nslot)
        for (int p = p0 + slot; p < p1; p += nslot) {
            if (OP == 0) {
                const int oy = p / w, ox = p - oy * w;
                const float *r0 = a + (((size_t)b * 2 * h + 2 * oy) * 2 * w + 2 * ox) * C + 4 * c4, *r1 = r0 + (size_t)2 * w * C;
                const float4 v00 = *reinterpret_cast<const float4 *>(r0), v01 = *reinterpret_cast<const float4 *>(r0 + C);
                const float4 v10 = *reinterpret_cast<const float4 *>(r1), v11 = *reinterpret_cast<const float4 *>(r1 + C);
                // avg_pool2d: the window summed row by row, divided by 4
                emit(oy, ox, make_float4((v00.x + v01.x + v10.x + v11.x) * 0.25f, (v00.y + v01.y + v10.y + v11.y) * 0.25f, (v00.z + v01.z + v10.z + v11.z) * 0.25f,
                                         (v00.w + v01.w + v10.w + v11.w) * 0.25f));
            } else {
                const int qy = p / lw, qx = p - qy * lw;
                const float sy = h > 1 ? (float)(lh - 1) / (float)(h - 1) : 0.f, sx = w > 1 ? (float)(lw - 1) / (float)(w - 1) : 0.f;
                float fy[2], fx[2]; int iy[2], ix[2];
#pragma unroll
                for (int e = 0; e < 2; e++) {
                    fy[e] = sy * (float)(2 * qy + e); iy[e] = (int)floorf(fy[e]);
                    fx[e] = sx * (float)(2 * qx + e); ix[e] = (int)floorf(fx[e]);
                }
                const int ry = iy[0] - 1, rx = ix[0] - 1;       // patch origin; iy[1] - iy[0], ix[1] - ix[0] are 0 or 1
                float4 pt[5][5];
#pragma unroll
                for (int i = 0; i < 5; i++) {
                    const int yy = min(max(ry + i, 0), lh - 1);
#pragma unroll
                    for (int k = 0; k < 5; k++) {
                        const int xx = min(max(rx + k, 0), lw - 1);
                        pt[i][k] = *reinterpret_cast<const float4 *>(a + (((size_t)b * lh + yy) * lw + xx) * C + 4 * c4);
                    }
                }
                // separable form with FIVE-tap weight rows: the four cubic weights of an output pixel sit at patch columns (rows) d .. d + 3 with d = 0 or 1
                // (its tap base against the patch origin), the fifth weight is zero -- every product with it adds an exact zero, so the sums are the ones of
                // the 4 x 4 form (row sums first, then the column sum, in the same order), without a select per tap and channel and with every row sum
                // computed once for both output rows that use it
                float w5x[2][5], w5y[2][5];
#pragma unroll
                for (int e = 0; e < 2; e++) {
                    float wx[4], wy[4]; cubic_w(fx[e] - ix[e], wx); cubic_w(fy[e] - iy[e], wy);
                    const bool dx = ix[e] != ix[0], dy = iy[e] != iy[0];
                    w5x[e][0] = dx ? 0.f : wx[0]; w5x[e][1] = dx ? wx[0] : wx[1]; w5x[e][2] = dx ? wx[1] : wx[2]; w5x[e][3] = dx ? wx[2] : wx[3]; w5x[e][4] = dx ? wx[3] : 0.f;
                    w5y[e][0] = dy ? 0.f : wy[0]; w5y[e][1] = dy ? wy[0] : wy[1]; w5y[e][2] = dy ? wy[1] : wy[2]; w5y[e][3] = dy ? wy[2] : wy[3]; w5y[e][4] = dy ? wy[3] : 0.f;
                }
                float4 rs[5][2];
#pragma unroll
                for (int i = 0; i < 5; i++)
#pragma unroll
                    for (int ex = 0; ex < 2; ex++) {
                        float4 row = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                        for (int k = 0; k < 5; k++) { const float4 t = pt[i][k]; const float wk = w5x[ex][k]; row.x += wk * t.x; row.y += wk * t.y; row.z += wk * t.z; row.w += wk * t.w; }
                        rs[i][ex] = row;
                    }
#pragma unroll
                for (int ey = 0; ey < 2; ey++)
#pragma unroll
                    for (int ex = 0; ex < 2; ex++) {
                        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                        for (int i = 0; i < 5; i++) { const float4 row = rs[i][ex]; const float wi = w5y[ey][i]; v.x += wi * row.x; v.y += wi * row.y; v.z += wi * row.z; v.w += wi * row.w; }
                        const int oy = 2 * qy + ey, ox = 2 * qx + ex;
                        if (skip) { const float4 k4 = *reinterpret_cast<const float4 *>(skip + ((size_t)b * HW + (size_t)oy * w + ox) * C + 4 * c4); v.x += k4.x; v.y += k4.y; v.z += k4.z; v.w += k4.w; }
                        emit(oy, ox, v);
                    }
            }
        }
    if (!part) return;
    __shared__ float red[256 * 8];
#pragma unroll
    for (int k = 0; k < 4; k++) { red[threadIdx.x * 8 + k] = s[k]; red[threadIdx.x * 8 + 4 + k] = q[k]; }
    __syncthreads();
    if (threadIdx.x < C4) {
        double ds[4] = {0, 0, 0, 0}, dq[4] = {0, 0, 0, 0};
        for (int sl = 0; sl < nslot; sl++)
#pragma unroll
            for (int k = 0; k < 4; k++) { ds[k] += (double)red[(sl * C4 + threadIdx.x) * 8 + k]; dq[k] += (double)red[(sl * C4 + threadIdx.x) * 8 + 4 + k]; }
        double *o = part + (((size_t)blockIdx.x * gridDim.y + b) * C + 4 * threadIdx.x) * 2;
#pragma unroll
        for (int k = 0; k < 4; k++) { o[2 * k] = ds[k]; o[2 * k + 1] = dq[k]; }
    }
}
// blocks of output pixels per frame of the sweeping producers: enough workgroups to fill the chip at B = 16 .. 48, few enough partials to finalize
static int sweep_blocks(int HW) { return min(max(HW / 64, 1), 256); }
extern "C" int vt_sweep_blocks(int HW) { return HW > 0 ? sweep_blocks(HW) : 0; }
template <int OP>
static int sweep_launch(const float *a, const float *skip, int B, int h, int w, int C, int groups, float *out, double *stats_ws, hipStream_t st)
{
    const int HW = h * w, nblk = sweep_blocks(HW), items = OP == 0 ? HW : HW / 4, rows = (items + nblk - 1) / nblk;
    double *part = stats_ws ? stats_ws + (size_t)B * groups : nullptr;
    hipLaunchKernelGGL(sweep_stats_kernel<OP>, dim3(nblk, B), dim3(256), 0, st, a, skip, h, w, C, rows, out, part);
    VT_LAUNCH_CHECK();
    return VT_OK;
}
extern "C" int vt_avgpool2x2_stats(const float *x, int B, int H, int W, int C, float *out, double *stats_ws, int stats_groups, void *stream)
{
    VT_REQUIRE(x && out && B > 0 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0 && C > 0 && C % 4 == 0 && C <= 1024 && (!stats_ws || stats_groups > 0),
               "vt_avgpool2x2_stats: bad argument (even H, W; C a multiple of 4, <= 1024)");
    return sweep_launch<0>(x, nullptr, B, H / 2, W / 2, C, stats_groups, out, stats_ws, vt_stream(stream));
}
extern "C" int vt_upsample2x_bicubic_add_stats(const float *low, const float *skip, int B, int h, int w, int C, float *out, double *stats_ws, int stats_groups,
                                               void *stream)
{
    VT_REQUIRE(low && out && B > 0 && h > 0 && w > 0 && C > 0 && C % 4 == 0 && C <= 1024 && (!stats_ws || stats_groups > 0),
               "vt_upsample2x_bicubic_add_stats: bad argument (C a multiple of 4, <= 1024)");
    return sweep_launch<1>(low, skip, B, 2 * h, 2 * w, C, stats_groups, out, stats_ws, vt_stream(stream));
}
static int gn_blocks(int HW) { return min(max(HW / 256, 1), 128); }
// workspace of vt_groupnorm_nhwc / vt_groupnorm_stats in doubles: (B, groups) x {mean, rstd} as float pairs FIRST, then the block partials
extern "C" long vt_groupnorm_workspace_doubles(int B, int HW, int C, int groups)
{
    if (B <= 0 || HW <= 0 || C <= 0 || groups <= 0) return 0;
    return (long)B * groups + (long)gn_blocks(HW) * B * C * 2;
}
static int gn_statistics(const float *x, int cstride, int B, int HW, int C, int groups, float eps, double *ws, hipStream_t st)
{
    const int nblk = gn_blocks(HW), rows = (HW + nblk - 1) / nblk;
    double *part = ws + (size_t)B * groups;
    hipLaunchKernelGGL(gn_stats_kernel, dim3(nblk, B), dim3(256), 0, st, x, cstride, HW, C, rows, part);
    VT_LAUNCH_CHECK();
    hipLaunchKernelGGL(gn_finalize_kernel, dim3(B * groups), dim3(64), 0, st, part, nblk, B, HW, C, groups, eps, reinterpret_cast<float2 *>(ws));
    VT_LAUNCH_CHECK();
    return VT_OK;
}
extern "C" int vt_groupnorm_nhwc(const float *x, const float *gamma, const float *beta, int B, int HW, int C, int groups, float eps, int relu,
                                 double *ws, float *y, void *stream)
{
    VT_REQUIRE(x && gamma && beta && ws && y && B > 0 && HW > 0 && C > 0 && C % 4 == 0 && C <= 1024 && groups > 0 && C % groups == 0,
               "vt_groupnorm_nhwc: bad argument (C must be a multiple of 4 and of groups, C <= 1024)");
    hipStream_t st = vt_stream(stream);
    if (int e = gn_statistics(x, C, B, HW, C, groups, eps, ws, st)) return e;
    const long total = (long)B * HW * (C / 4);
    hipLaunchKernelGGL(gn_apply_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, gamma, beta, reinterpret_cast<const float2 *>(ws), B, HW, C, groups, relu, y);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

// statistics only, on a channel slice [coff, coff + C) of an NHWC tensor with cstride channels: (B, groups) x {mean, 1 / sqrt(var + eps)} as floats
// at the START of ws (vt_groupnorm_workspace_doubles) -- the GroupNorm + ReLU itself is applied by the consumer (vt_conv3x3_forward_gn stages it into
// its operand planes)
extern "C" int vt_groupnorm_stats(const float *x, int cstride, int coff, int B, int HW, int C, int groups, float eps, double *ws, void *stream)
{
    VT_REQUIRE(x && ws && B > 0 && HW > 0 && C > 0 && C % 4 == 0 && groups > 0 && C % groups == 0 && C <= 1024 && cstride >= coff + C && cstride % 4 == 0 && coff % 4 == 0,
               "vt_groupnorm_stats: bad argument");
    return gn_statistics(x + coff, cstride, B, HW, C, groups, eps, ws, vt_stream(stream));
}

// second half of vt_groupnorm_stats for partial sums that somebody else produced: `part` = ws + B * groups doubles holds nblk x (B, C) x {sum, sum of
// squares} (vt_conv3x3_forward_gn_stats writes one block per output tile); the (B, groups) {mean, rstd} float pairs go to the start of ws
extern "C" int vt_groupnorm_finalize(double *ws, int nblk, int B, int HW, int C, int groups, float eps, void *stream)
{
    VT_REQUIRE(ws && nblk > 0 && B > 0 && HW > 0 && C > 0 && groups > 0 && C % groups == 0, "vt_groupnorm_finalize: bad argument");
    hipLaunchKernelGGL(gn_finalize_kernel, dim3(B * groups), dim3(64), 0, vt_stream(stream), ws + (size_t)B * groups, nblk, B, HW, C, groups, eps, reinterpret_cast<float2 *>(ws));
    VT_LAUNCH_CHECK();
    return VT_OK;
}

extern "C" int vt_upsample2x_bicubic_add(const float *low, const float *skip, int B, int h, int w, int C, float *out, void *stream)
{
    VT_REQUIRE(low && out && B > 0 && h > 0 && w > 0 && C > 0 && C % 4 == 0, "vt_upsample2x_bicubic_add: bad argument (C must be a multiple of 4)");
    const long total = (long)B * 4 * h * w * (C / 4);
    hipLaunchKernelGGL(upsample2x_bicubic_add_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, vt_stream(stream), low, skip, B, h, w, C, out);
    VT_LAUNCH_CHECK();
    return VT_OK;
}
