// resample_bwd.hip -- the backward of the two operators that join the ConvBlocks of an hourglass (model/HGFilters.py:26-50): 2 x 2 average pooling and
// skip + bicubic x2 up-sampling.  The forwards are sweep_stats_kernel / upsample2x_bicubic_add_kernel of encoder_ops.hip.  Both kernels are gathers: one
// thread owns one element group of the RESULT (a pixel x 4 channels), reads what contributes to it and writes it once -- no atomics, nothing to zero, a
// fixed order of every sum, the same bits on every call.  Tensors are NHWC fp32.
#include "common.h"
#include "cubic.h"

// d_x[b,y,x,c] = 0.25 d_out[b,y/2,x/2,c]   (F.avg_pool2d(x, 2, stride=2) backward: exact, a power of two times the input)
// thread = one pixel of d_x x 4 channels: the stores are lane-linear, the four readers of a d_out element sit in the same or the next-but-W wave (cache hits)
__global__ __launch_bounds__(256) void avgpool2x2_backward_kernel(const float *__restrict__ d_out, int B, int H, int W, int C, float *__restrict__ d_x)
{
    const int C4 = C >> 2;
    const long t = (long)blockIdx.x * 256 + threadIdx.x, total = (long)B * H * W * C4;
    if (t >= total) return;
    const int c4 = (int)(t % C4); long r = t / C4;
    const int x = (int)(r % W); r /= W;
    const int y = (int)(r % H); const int b = (int)(r / H);
    const float4 v = *reinterpret_cast<const float4 *>(d_out + (((size_t)b * (H >> 1) + (y >> 1)) * (W >> 1) + (x >> 1)) * C + 4 * c4);
    *reinterpret_cast<float4 *>(d_x + (((size_t)b * H + y) * W + x) * C + 4 * c4) = make_float4(0.25f * v.x, 0.25f * v.y, 0.25f * v.z, 0.25f * v.w);
}

// One axis of U (upsample2x_bicubic_add_kernel): does output index o read low index l (of n), and with which weight?  The source coordinate, its floor and
// the four weights are the forward's own fp32 expressions (s = (n - 1) / (2 n - 1) as the forward computed it); every tap i whose CLAMPED index is l adds its
// weight, so a border pixel that the forward read through several taps gets all of them: the transpose by construction, not by inverting the map.
__device__ __forceinline__ bool axis_weight(int o, int l, int n, float s, double *wsum)
{
    const float f = s * o;
    const int i0 = (int)floorf(f);
    float w[4];
    cubic_w(f - i0, w);
    double acc = 0.0; bool hit = false;
#pragma unroll
    for (int i = 0; i < 4; i++)
        if (min(max(i0 - 1 + i, 0), n - 1) == l) { acc += (double)w[i]; hit = true; }
    *wsum = acc;
    return hit;
}

// d_low[b,yy,xx,c] = sum (oy,ox) Uy[oy,yy] Ux[ox,xx] d_out[b,oy,ox,c].  thread = one pixel of d_low x 4 channels.  Candidates are the output rows
// 2 yy - 4 .. 2 yy + 4 inside the image (and the columns likewise): the window holds every contributor (a row has at most 9) for the sizes the forward
// serves; a candidate that does not read (yy, xx) is skipped, not multiplied by zero.  Separable and in fp64: per candidate row the column sum in
// ascending ox, then the rows in ascending oy, rounded once -- memory bound (each d_out element is read by ~16 threads, from cache), the fp64 adds are free.
__global__ __launch_bounds__(256) void upsample2x_bicubic_backward_kernel(const float *__restrict__ d_out, int B, int h, int w, int C, float *__restrict__ d_low)
{
    const int C4 = C >> 2, H = 2 * h, W = 2 * w;
    const long t = (long)blockIdx.x * 256 + threadIdx.x, total = (long)B * h * w * C4;
    if (t >= total) return;
    const int c4 = (int)(t % C4); long r = t / C4;
    const int xx = (int)(r % w); r /= w;
    const int yy = (int)(r % h); const int b = (int)(r / h);
    const float sy = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f, sx = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
    double wx[9]; unsigned okx = 0;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const int ox = 2 * xx - 4 + k;
        wx[k] = 0.0;
        if (ox >= 0 && ox < W && axis_weight(ox, xx, w, sx, &wx[k])) okx |= 1u << k;
    }
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll 1
    for (int j = 0; j < 9; j++) {
        const int oy = 2 * yy - 4 + j;
        double wy;
        if (oy < 0 || oy >= H || !axis_weight(oy, yy, h, sy, &wy)) continue;
        const float *__restrict__ row = d_out + ((size_t)b * H + oy) * W * C + 4 * c4;
        double r0 = 0.0, r1 = 0.0, r2 = 0.0, r3 = 0.0;
#pragma unroll
        for (int k = 0; k < 9; k++)
            if (okx & (1u << k)) {          // implies 0 <= 2 xx - 4 + k < W
                const float4 v = *reinterpret_cast<const float4 *>(row + (size_t)(2 * xx - 4 + k) * C);
                r0 += wx[k] * (double)v.x; r1 += wx[k] * (double)v.y; r2 += wx[k] * (double)v.z; r3 += wx[k] * (double)v.w;
            }
        a0 += wy * r0; a1 += wy * r1; a2 += wy * r2; a3 += wy * r3;
    }
    *reinterpret_cast<float4 *>(d_low + (((size_t)b * h + yy) * w + xx) * C + 4 * c4) = make_float4((float)a0, (float)a1, (float)a2, (float)a3);
}

extern "C" int vt_avgpool2x2_backward(const float *d_out, int B, int H, int W, int C, float *d_x, void *stream)
{
    VT_REQUIRE(d_out && d_x && B > 0 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0 && C > 0 && C % 4 == 0 && (long)B * H * W * (C / 4) <= 0x7fffffffL * 256,
               "vt_avgpool2x2_backward: bad argument (even H, W; C a multiple of 4)");
    const long total = (long)B * H * W * (C / 4);
    hipLaunchKernelGGL(avgpool2x2_backward_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, vt_stream(stream), d_out, B, H, W, C, d_x);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

extern "C" int vt_upsample2x_bicubic_backward(const float *d_out, int B, int h, int w, int C, float *d_low, void *stream)
{
    VT_REQUIRE(d_out && d_low && B > 0 && h > 0 && w > 0 && h <= (1 << 20) && w <= (1 << 20) && C > 0 && C % 4 == 0 && (long)B * h * w * (C / 4) <= 0x7fffffffL * 256,
               "vt_upsample2x_bicubic_backward: bad argument (C a multiple of 4)");
    const long total = (long)B * h * w * (C / 4);
    hipLaunchKernelGGL(upsample2x_bicubic_backward_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, vt_stream(stream), d_out, B, h, w, C, d_low);
    VT_LAUNCH_CHECK();
    return VT_OK;
}
