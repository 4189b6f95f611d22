// enctrain.hip -- the rows of the encoder's backward that join the ConvBlocks (convtrain.hip) and the hourglasses (resample_bwd.hip) into a whole HGFilter
// (model/HGFilters.py:56-203): the 1 x 1 tail of a stack (HGFilters.py:191-201) and the stem (HGFilters.py:120, 125, 167).  Conventions of convtrain.hip: NHWC fp32
// channel slices (pointer, channel stride, channel offset), exact fp32 products, fp64 partial sums added in a fixed order and rounded once, no atomics, one
// writer per element, nothing in a workspace needs initialising, `accumulate` != 0 adds onto PARAMETER gradients, a power-of-two scale of the upstream gradient
// scales every result bit for bit, the same inputs give the same bits on every call.
//
// KERNELS.
//   bias_reduce_kernel   db[c] = sum (b, pixel) d_out[b, pixel, c]: workgroup = (block of pixels, frame), thread = (pixel slot, float4 of channels), fp64 from the
//                        first addition on; one fp64 partial per (block, frame, channel).  bias_finish_kernel adds them in (frame, block) order and rounds once.
//   stem_wgrad_kernel    dW[co,ci,ky,kx] = sum (b,oy,ox) d_y[b,oy,ox,co] x[b,2oy+ky-3,2ox+kx-3,ci] of conv1 = Conv2d(Cin, Cout, 7, stride 2, pad 3).  A GEMM with
//                        M = Cout, N = 49 Cin, K = B H2 W2 on v_mfma_f32_16x16x4_f32 (builtin).  Split K: workgroup = (split of a frame's 16 x 16 output tiles, frame);
//                        per tile the 37 x 37 x Cin input patch goes to LDS once, zero padded, as stem.hip's forward stages it; a K step is four output pixels of
//                        the tile.  Row j of M tile mt is output channel MT j + mt (a lane's A values of a K step are MT consecutive floats of one pixel of d_y);
//                        column n = ci 49 + ky 7 + kx of N reads patch[ci][2 oyl + ky][2 oxl + kx] -- the N axis IS the flattened (Cin, 7, 7) of dW, so a partial has
//                        dW's own layout.  The four waves split the N tiles (NT each); columns past 49 Cin compute on patch element 0 and are not stored.
//                        Pixels of an edge tile past H2 x W2 enter with d_y = 0.  Partials [frame][split][Cout][49 Cin].
//   f32_finish_kernel    the partials added in fp64 in (frame, split) order, rounded once, stored or added to dW (accumulate).
//   add_kernel           out = a + b element-wise (one fp32 addition): the two places of the tail where two data gradients meet (below).
//
// THE TAIL (vt_stack_tail_backward).  Forward of stack i: raw = conv_last(ll) + b, a = ReLU(GN_end(raw)), out = l(a) + b, previous' = previous + bl(a) + b + al(out) + b.
// With d_out (gradient to outputs[i]) and d_prev (gradient to previous'), either may be absent (zero):
//   g_out = d_out + Wal^T d_prev         one fp32 addition per element, in this order (add_kernel; d_out absent: g_out = Wal^T d_prev)
//   d_a   = Wl^T g_out + Wbl^T d_prev    one fp32 addition per element, in this order (add_kernel)
//   d_raw = GN + ReLU backward of d_a at raw (vt_gn_relu_backward: the staging expression IS what l / bl applied), d_ll = Wcl^T d_raw
//   dWal = d_prev (x) out, dWbl = d_prev (x) a, dWl = g_out (x) a, dWcl = d_raw (x) ll, a recomputed in the weight-gradient staging; the four bias gradients.
// The 1 x 1 data and weight gradients and the GroupNorm passes are convtrain.hip's own entry points (vt_conv1x1_dgrad / vt_conv1x1_wgrad / vt_gn_relu_backward);
// the 1 x 1 dgrad has no accumulate form, so the two sums above are a small add kernel.  The gradient to `previous` is d_prev itself (the autograd layer returns it).
#include "common.h"

namespace enct {

typedef float f32x4 __attribute__((ext_vector_type(4)));
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

#define ET_BIAS_ROWS 256        /* pixels per block of the bias reduction (until ET_BIAS_MAXBLK blocks per frame are reached) */
#define ET_BIAS_MAXBLK 64
#define SW_T 16                 /* output tile edge of the stem weight gradient */
#define SW_P 37                 /* input patch edge: 2 * 16 + 5 */
#define SW_PP 40                /* patch row pitch (floats) */

static inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

__global__ __launch_bounds__(256) void bias_reduce_kernel(const float *__restrict__ g, int g_cs, int HW, int C, int rows_per_block, double *__restrict__ part)
{
    const int C4 = C >> 2, b = blockIdx.y, c4 = threadIdx.x % C4, slot = threadIdx.x / C4, nslot = 256 / C4;
    const int p0 = blockIdx.x * rows_per_block, p1 = min(HW, p0 + rows_per_block);
    double s[4] = {0, 0, 0, 0};
    if (slot < nslot)
        for (int p = p0 + slot; p < p1; p += nslot) {
            const float4 v = *reinterpret_cast<const float4 *>(g + ((size_t)b * HW + p) * g_cs + 4 * c4);
            s[0] += (double)v.x; s[1] += (double)v.y; s[2] += (double)v.z; s[3] += (double)v.w;
        }
    __shared__ double red[256 * 4];
#pragma unroll
    for (int k = 0; k < 4; k++) red[threadIdx.x * 4 + k] = s[k];
    __syncthreads();
    if (threadIdx.x < C4) {
        double d[4] = {0, 0, 0, 0};
        for (int sl = 0; sl < nslot; sl++)
#pragma unroll
            for (int k = 0; k < 4; k++) d[k] += red[(sl * C4 + threadIdx.x) * 4 + k];
        double *o = part + ((size_t)blockIdx.x * gridDim.y + b) * C + 4 * threadIdx.x;
#pragma unroll
        for (int k = 0; k < 4; k++) o[k] = d[k];
    }
}
__global__ __launch_bounds__(64) void bias_finish_kernel(const double *__restrict__ part, int nblk, int B, int C, float *__restrict__ db, int accumulate)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    double s = 0;
    for (int b = 0; b < B; b++)
        for (int blk = 0; blk < nblk; blk++) s += part[((size_t)blk * B + b) * C + c];
    db[c] = accumulate ? db[c] + (float)s : (float)s;
}

template <int MT, int NT>
__global__ __launch_bounds__(256) void stem_wgrad_kernel(const float *__restrict__ dy, int dy_cs, int dy_co, const float *__restrict__ x, int x_cs, int x_co, int Cin,
                                                         int H, int W, int H2, int W2, int nsplit, int tpw, float *__restrict__ partials)
{
    extern __shared__ float spatch[];       // [Cin][37][40]
    constexpr int Cout = 16 * MT;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, q = lane >> 4, j = lane & 15;
    const int split = blockIdx.x, b = blockIdx.y, N = 49 * Cin;
    const int tiles_x = (W2 + SW_T - 1) / SW_T, tiles = tiles_x * ((H2 + SW_T - 1) / SW_T);
    const int t_lo = split * tpw, t_hi = min(tiles, t_lo + tpw);
    // column n of this lane in each of the wave's N tiles -> the patch offset of tap (ci, ky, kx) against a pixel's patch origin
    int boff[NT];
#pragma unroll
    for (int nt = 0; nt < NT; nt++) {
        const int n = (wave * NT + nt) * 16 + j, nn = n < N ? n : 0, ci = nn / 49, t = nn - 49 * ci, ky = t / 7, kx = t - 7 * ky;
        boff[nt] = (ci * SW_P + ky) * SW_PP + kx;
    }
    f32x4 acc[NT][MT];
#pragma unroll
    for (int nt = 0; nt < NT; nt++)
#pragma unroll
        for (int mt = 0; mt < MT; mt++) acc[nt][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const float *__restrict__ dyb = dy + (size_t)b * H2 * W2 * dy_cs + dy_co + MT * j;
    const float *__restrict__ xb = x + (size_t)b * H * W * x_cs + x_co;

    for (int tile = t_lo; tile < t_hi; tile++) {
        const int tx = tile % tiles_x, ty = tile / tiles_x;
        const int iy0 = 2 * SW_T * ty - 3, ix0 = 2 * SW_T * tx - 3;
        __syncthreads();            // the readers of the previous tile's patch are done
        for (int p = tid; p < SW_P * SW_P; p += 256) {
            const int py = p / SW_P, px = p - py * SW_P, iy = iy0 + py, ix = ix0 + px;
            const bool inside = iy >= 0 && iy < H && ix >= 0 && ix < W;
            const float *src = xb + ((size_t)(inside ? iy : 0) * W + (inside ? ix : 0)) * x_cs;
            for (int ci = 0; ci < Cin; ci++) spatch[(ci * SW_P + py) * SW_PP + px] = inside ? src[ci] : 0.f;      // zero padding of the image
        }
        __syncthreads();
#pragma unroll 2
        for (int s = 0; s < SW_T * SW_T / 4; s++) {         // K step = the four pixels 4 s + q of the tile
            const int p = 4 * s + q, oyl = p >> 4, oxl = p & 15, oy = SW_T * ty + oyl, ox = SW_T * tx + oxl;
            float a[MT];
#pragma unroll
            for (int mt = 0; mt < MT; mt++) a[mt] = 0.f;
            if (oy < H2 && ox < W2) {
                const float *ap = dyb + ((size_t)oy * W2 + ox) * dy_cs;
                if constexpr (MT == 4) { const float4 v = *reinterpret_cast<const float4 *>(ap); a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w; }
                else { const float2 v = *reinterpret_cast<const float2 *>(ap); a[0] = v.x; a[1] = v.y; }
            }
            const int pbase = 2 * oyl * SW_PP + 2 * oxl;
#pragma unroll
            for (int nt = 0; nt < NT; nt++) {
                const float bv = spatch[boff[nt] + pbase];
#pragma unroll
                for (int mt = 0; mt < MT; mt++) acc[nt][mt] = MFMA16(a[mt], bv, acc[nt][mt]);
            }
        }
    }
    float *__restrict__ out = partials + ((size_t)b * nsplit + split) * ((size_t)Cout * N);
#pragma unroll
    for (int nt = 0; nt < NT; nt++) {
        const int n = (wave * NT + nt) * 16 + j;
        if (n < N)
#pragma unroll
            for (int mt = 0; mt < MT; mt++)
#pragma unroll
                for (int r = 0; r < 4; r++) out[(size_t)(MT * (4 * q + r) + mt) * N + n] = acc[nt][mt][r];       // D row 4 q + r of tile mt = output channel MT (4 q + r) + mt
    }
}

__global__ __launch_bounds__(256) void f32_finish_kernel(const float *__restrict__ partials, long P, int nparts, float *__restrict__ out, int accumulate)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    double s = 0.0;
    for (int k = 0; k < nparts; k++) s += (double)partials[(size_t)k * P + i];
    out[i] = accumulate ? out[i] + (float)s : (float)s;
}

__global__ __launch_bounds__(256) void add_kernel(const float4 *a, const float4 *b, float4 *out, long n4)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const float4 u = a[i], v = b[i];        // a or b may be out: each element is read and written by this thread only
    out[i] = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------------------
static int bias_blocks(int HW) { const int n = (HW + ET_BIAS_ROWS - 1) / ET_BIAS_ROWS; return n < 1 ? 1 : (n > ET_BIAS_MAXBLK ? ET_BIAS_MAXBLK : n); }
static long bias_ws_bytes(int B, int HW, int C) { return (long)align256((size_t)bias_blocks(HW) * B * C * sizeof(double)); }
static bool bias_ok(int B, int HW, int C) { return B > 0 && B <= 65535 && HW > 0 && C >= 4 && C <= 1024 && C % 4 == 0; }
static bool slice_ok(const void *p, int cstride, int coff, int c)
{
    return p && coff >= 0 && cstride >= coff + c && cstride % 4 == 0 && coff % 4 == 0 && ((uintptr_t)p & 15) == 0;
}
static int stem_tiles(int H, int W) { const int H2 = (H - 1) / 2 + 1, W2 = (W - 1) / 2 + 1; return ((H2 + SW_T - 1) / SW_T) * ((W2 + SW_T - 1) / SW_T); }
static int stem_splits(int B, int tiles) { int s = 512 / B; s = s < 1 ? 1 : (s > 32 ? 32 : s); return s < tiles ? s : tiles; }
static bool stem_ok(int B, int H, int W, int cin, int cout)
{
    return B > 0 && B <= 65535 && H > 0 && W > 0 && H <= 32768 && W <= 32768 && (cout == 32 || cout == 64) && cin >= 1 && cin <= 8;
}
static long stem_ws_bytes(int B, int H, int W, int cin, int cout) { return (long)align256((size_t)B * stem_splits(B, stem_tiles(H, W)) * cout * 49 * cin * sizeof(float)); }

static int bias_grad(const float *g, int g_cs, int B, int HW, int C, float *db, int accumulate, void *ws, hipStream_t st)
{
    const int nblk = bias_blocks(HW), rows = (HW + nblk - 1) / nblk;
    double *part = static_cast<double *>(ws);
    hipLaunchKernelGGL(bias_reduce_kernel, dim3(nblk, B), dim3(256), 0, st, g, g_cs, HW, C, rows, part);
    hipLaunchKernelGGL(bias_finish_kernel, dim3((C + 63) / 64), dim3(64), 0, st, part, nblk, B, C, db, accumulate);
    VT_LAUNCH_CHECK();
    return VT_OK;
}
static int add(const float *a, const float *b, float *out, size_t n, hipStream_t st)
{
    const long n4 = (long)(n >> 2);
    hipLaunchKernelGGL(add_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const float4 *>(a), reinterpret_cast<const float4 *>(b),
                       reinterpret_cast<float4 *>(out), n4);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

}  // namespace enct

extern "C" {

long vt_bias_grad_workspace_bytes(int B, int HW, int C)
{
    if (!enct::bias_ok(B, HW, C)) return -1;
    return enct::bias_ws_bytes(B, HW, C);
}
int vt_bias_grad(const float *d_out, int do_cstride, int do_coff, int B, int HW, int C, float *db, int accumulate, void *workspace, void *stream)
{
    VT_REQUIRE(db && workspace && enct::bias_ok(B, HW, C), "vt_bias_grad: needs db, a workspace, 0 < B <= 65535, HW > 0, C %% 4 == 0 and C <= 1024");
    VT_REQUIRE(enct::slice_ok(d_out, do_cstride, do_coff, C), "vt_bias_grad: needs a 16-byte aligned channel slice");
    return enct::bias_grad(d_out + do_coff, do_cstride, B, HW, C, db, accumulate, workspace, vt_stream(stream));
}

long vt_stem7x7_wgrad_workspace_bytes(int B, int H, int W, int cin, int cout)
{
    if (!enct::stem_ok(B, H, W, cin, cout)) return -1;
    return enct::stem_ws_bytes(B, H, W, cin, cout);
}
int vt_stem7x7_wgrad(const float *d_y, int dy_cstride, int dy_coff, const float *x, int x_cstride, int x_coff, int B, int H, int W, int cin, int cout,
                     float *dW, int accumulate, void *workspace, void *stream)
{
    VT_REQUIRE(dW && workspace && enct::stem_ok(B, H, W, cin, cout), "vt_stem7x7_wgrad: needs Cout in {32, 64}, Cin in 1..8, 0 < H, W <= 32768 and 0 < B <= 65535");
    VT_REQUIRE(enct::slice_ok(d_y, dy_cstride, dy_coff, cout), "vt_stem7x7_wgrad: d_y must be a 16-byte aligned channel slice");
    VT_REQUIRE(x && x_coff >= 0 && x_coff + cin <= x_cstride, "vt_stem7x7_wgrad: input channel slice [%d, %d) outside %d channels", x_coff, x_coff + cin, x_cstride);
    hipStream_t st = vt_stream(stream);
    const int H2 = (H - 1) / 2 + 1, W2 = (W - 1) / 2 + 1, tiles = enct::stem_tiles(H, W), ns = enct::stem_splits(B, tiles), tpw = (tiles + ns - 1) / ns;
    const int ntile = (49 * cin + 15) / 16, nt = ntile <= 4 ? 1 : (ntile <= 8 ? 2 : (ntile <= 16 ? 4 : 7));       // N tiles per wave: 4 nt >= ntile (25 at Cin = 8)
    const size_t lds = (size_t)cin * SW_P * SW_PP * sizeof(float);
    const dim3 grid(ns, B);
    float *part = static_cast<float *>(workspace);
#define ET_SW(MT_, NT_) hipLaunchKernelGGL((enct::stem_wgrad_kernel<MT_, NT_>), grid, dim3(256), lds, st, d_y, dy_cstride, dy_coff, x, x_cstride, x_coff, cin, H, W, H2, W2, ns, tpw, part)
    if (cout == 64) { if (nt == 1) ET_SW(4, 1); else if (nt == 2) ET_SW(4, 2); else if (nt == 4) ET_SW(4, 4); else ET_SW(4, 7); }
    else { if (nt == 1) ET_SW(2, 1); else if (nt == 2) ET_SW(2, 2); else if (nt == 4) ET_SW(2, 4); else ET_SW(2, 7); }
#undef ET_SW
    const long P = (long)cout * 49 * cin;
    hipLaunchKernelGGL(enct::f32_finish_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, part, P, B * ns, dW, accumulate);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

// workspace of the tail: GO (g_out, Co channels), DA (d_a, then free), DB (Wbl^T d_prev, then d_raw), and one area shared by whichever of convtrain.hip's
// entry points or the bias reduction runs
static bool tail_ok(int B, int H, int W, int C, int Co)
{
    return vt_conv_wgrad_workspace_bytes(B, H, W, C, C, 1) >= 0 && vt_conv_wgrad_workspace_bytes(B, H, W, Co, C, 1) >= 0 && vt_conv_wgrad_workspace_bytes(B, H, W, C, Co, 1) >= 0;
}
static size_t tail_shared_bytes(int B, int H, int W, int C, int Co)
{
    long m = vt_gn_relu_backward_workspace_bytes(B, H * W, C, 32);
    const long c[] = {vt_conv_wgrad_workspace_bytes(B, H, W, C, C, 1), vt_conv_wgrad_workspace_bytes(B, H, W, Co, C, 1), vt_conv_wgrad_workspace_bytes(B, H, W, C, Co, 1),
                      vt_conv_dgrad_workspace_bytes(C, C, 1), vt_conv_dgrad_workspace_bytes(Co, C, 1), vt_conv_dgrad_workspace_bytes(C, Co, 1),
                      enct::bias_ws_bytes(B, H * W, C > Co ? C : Co)};
    for (long v : c) m = v > m ? v : m;
    return (size_t)m;
}
long vt_stack_tail_backward_workspace(int B, int H, int W, int C, int Co)
{
    if (!tail_ok(B, H, W, C, Co)) return -1;
    const size_t px = (size_t)B * H * W;
    return (long)(enct::align256(px * Co * sizeof(float)) + 2 * enct::align256(px * C * sizeof(float)) + tail_shared_bytes(B, H, W, C, Co));
}
int vt_stack_tail_backward(const float *d_out, const float *d_prev, const float *ll, const float *raw, const float *out, const float *stats,
                           const float *wcl, const float *gamma, const float *beta, const float *wl, const float *wbl, const float *wal,
                           int B, int H, int W, int C, int Co,
                           float *d_ll, float *dWcl, float *dbcl, float *dgamma, float *dbeta, float *dWl, float *dbl, float *dWbl, float *dbbl, float *dWal, float *dbal,
                           void *workspace, int accumulate, void *stream)
{
    VT_REQUIRE(ll && raw && stats && wcl && gamma && beta && wl && workspace, "vt_stack_tail_backward: null input");
    VT_REQUIRE(d_out || d_prev, "vt_stack_tail_backward: both upstream gradients are absent");
    VT_REQUIRE(!d_prev || (wbl && wal && out), "vt_stack_tail_backward: d_prev needs the weights of bl and al and the saved out");
    VT_REQUIRE(d_prev || !(dWbl || dbbl || dWal || dbal), "vt_stack_tail_backward: gradients of bl / al requested without d_prev (the last stack has neither)");
    VT_REQUIRE(tail_ok(B, H, W, C, Co), "vt_stack_tail_backward: needs H %% 8 == 0, W %% 16 == 0, 0 < B <= 65535, C and Co in {64, 128, 256}");
    VT_REQUIRE((((uintptr_t)d_out | (uintptr_t)d_prev | (uintptr_t)ll | (uintptr_t)raw | (uintptr_t)out | (uintptr_t)workspace | (uintptr_t)d_ll) & 15) == 0,
               "vt_stack_tail_backward: tensors must be 16-byte aligned");
    hipStream_t st = vt_stream(stream);
    const int HW = H * W;
    const size_t px = (size_t)B * HW;
    char *wsb = static_cast<char *>(workspace);
    float *GO = reinterpret_cast<float *>(wsb);
    float *DA = reinterpret_cast<float *>(wsb + enct::align256(px * Co * sizeof(float)));
    float *DB = reinterpret_cast<float *>(wsb + enct::align256(px * Co * sizeof(float)) + enct::align256(px * C * sizeof(float)));
    void *S = wsb + enct::align256(px * Co * sizeof(float)) + 2 * enct::align256(px * C * sizeof(float));
    int rc;
#define ET_TRY(call_) do { rc = (call_); if (rc) return rc; } while (0)
    const float *g_out = d_out;
    if (d_prev) {       // previous' = previous + bl(a) + b + al(out) + b (HGFilters.py:199-201)
        if (dbal) ET_TRY(enct::bias_grad(d_prev, C, B, HW, C, dbal, accumulate, S, st));
        if (dbbl) ET_TRY(enct::bias_grad(d_prev, C, B, HW, C, dbbl, accumulate, S, st));
        if (dWal) ET_TRY(vt_conv1x1_wgrad(d_prev, C, 0, out, Co, 0, nullptr, nullptr, nullptr, 32, B, H, W, Co, C, dWal, accumulate, S, stream));
        if (dWbl) ET_TRY(vt_conv1x1_wgrad(d_prev, C, 0, raw, C, 0, stats, gamma, beta, 32, B, H, W, C, C, dWbl, accumulate, S, stream));
        ET_TRY(vt_conv1x1_dgrad(wal, C, Co, d_prev, C, 0, B, H, W, GO, Co, 0, S, stream));
        if (d_out) ET_TRY(enct::add(d_out, GO, GO, px * Co, st));         // g_out = d_out + Wal^T d_prev
        g_out = GO;
    }
    // out = l(a) + b (HGFilters.py:195)
    if (dbl) ET_TRY(enct::bias_grad(g_out, Co, B, HW, Co, dbl, accumulate, S, st));
    if (dWl) ET_TRY(vt_conv1x1_wgrad(g_out, Co, 0, raw, C, 0, stats, gamma, beta, 32, B, H, W, C, Co, dWl, accumulate, S, stream));
    if (d_ll || dWcl || dbcl || dgamma || dbeta) {
        ET_TRY(vt_conv1x1_dgrad(wl, Co, C, g_out, Co, 0, B, H, W, DA, C, 0, S, stream));
        if (d_prev) {
            ET_TRY(vt_conv1x1_dgrad(wbl, C, C, d_prev, C, 0, B, H, W, DB, C, 0, S, stream));
            ET_TRY(enct::add(DA, DB, DA, px * C, st));                  // d_a = Wl^T g_out + Wbl^T d_prev
        }
        // a = ReLU(bn_end(raw)), raw = conv_last(ll) + b (HGFilters.py:191-192)
        const bool need_raw = d_ll || dWcl || dbcl;
        ET_TRY(vt_gn_relu_backward(DA, C, 0, raw, C, 0, stats, gamma, beta, 32, B, HW, C, nullptr, 0, 0, need_raw ? DB : nullptr, C, 0, dgamma, dbeta, accumulate, S, stream));
        if (dbcl) ET_TRY(enct::bias_grad(DB, C, B, HW, C, dbcl, accumulate, S, st));
        if (dWcl) ET_TRY(vt_conv1x1_wgrad(DB, C, 0, ll, C, 0, nullptr, nullptr, nullptr, 32, B, H, W, C, C, dWcl, accumulate, S, stream));
        if (d_ll) ET_TRY(vt_conv1x1_dgrad(wcl, C, C, DB, C, 0, B, H, W, d_ll, C, 0, S, stream));
    }
#undef ET_TRY
    return VT_OK;
}

}  // extern "C"
