// inputs.hip -- the five image channels of the SIF-Net input from decoded uint8 frames in device memory: mask bounding box, zero-padded square crop,
// bilinear resize to the network size, rounding to grey levels, / 255 and composition (data/base_data.py:139-157 masks2bbox, :204-233 crop, :252-265
// compose_images; data/train_data.py:143-162 prepare_image_crop).  The yardstick is the host path of vistracker_amd/sequence_io.py (masks2bbox, crop,
// resize_bilinear and the compose of SequenceLoader.load_crop): both kernels reproduce it bit for bit.
//
// CONTRACT (restated with integers in tests/inputs_model.py):
//   bbox      : a pixel counts when (uint8)(pm + om) > thres -- the sum wraps like the reference's uint8 accumulator (255 + 255 = 254 counts, 200 + 100 = 44
//               does not).  box = xmin, ymin, xmax, ymax, INCLUSIVE; a frame without such a pixel keeps the sentinel (W, H, -1, -1).  Integer min / max
//               only (wave reduction, then integer atomics): the result does not depend on scheduling.
//   corners   : per frame tl.x, tl.y, br.x, br.y = round(centre -+ crop_size / 2), computed on the host exactly as sequence_io.crop does (numpy rounds
//               halves to even, so an odd crop_size gives an extent br - tl of crop_size + 1 or crop_size - 1; an even one gives crop_size).  The crop
//               has n = br - tl pixels per axis, crop pixel c is image pixel tl + c.
//   region    : only what crop() keeps is read: x in [max(0, tl.x), min(W - 1, br.x)), y in [max(0, tl.y), min(H - 1, br.y)) -- the reference's quirk
//               that the last image column / row is dropped once the crop reaches it is kept.  Everything else of the crop is 0.
//   taps      : torch's interpolate(mode="bilinear", align_corners=False), per axis, in fp32: scale = float(n) / out_size,
//               src = max(scale * (d + 0.5) - 0.5, 0), i0 = min(floor(src), n - 1), i1 = min(i0 + 1, n - 1), lambda = clamp(src - i0, 0, 1).
//   blend     : fp32, no contraction, in this order: x = (a w0 + b w1) h0 + (c w0 + d w1) h1 with w1 = lambda_x, w0 = 1 - w1, h1 = lambda_y, h0 = 1 - h1,
//               a b = the taps of row i0, c d = of row i1 (the order of torch's separable CPU kernel).  With weights that are multiples of 1 / 64
//               (crop 1200 -> 512, or any crop -> 32) every product and sum is exact in fp32 and the order does not matter.
//   rounding  : q = clip(floor(x + 0.5), 0, 255).
//   value     : table[q], table = 256 floats from the host with table[q] = float32(q / 255.0) (the host path divides in float64 and narrows).
//   compose   : comb = q_pm >= 128 or q_om >= 128 (the host's `> 0.5` on q / 255); channels 0..2 = table[comb ? q_rgb : 0], 3 = table[q_pm], 4 = table[q_om].
//   output    : frame b at out + b * frame_stride floats, channel c at + c * S * S: channels 0..4 are written, nothing else is touched.
//
// CONTRACT of the step-7 camera panel (vt_resize_panel_u8; render/render_recon.py:157-159: cv2.resize of the camera image to size x H, then the panel's columns;
// restated with integers in tests/panel_model.py).  The yardstick is sequence_io.resize_bilinear_hw(img, H, size)[:, col0:col0 + pw]:
//   taps      : per axis in fp32, as above with n = the image's h (rows, out H) or w (columns, out size): scale = float(in) / out,
//               src = max(scale * (d + 0.5f) - 0.5f, 0), i0 = floor(src), i1 = min(i0 + 1, in - 1), l1 = src - i0, l0 = 1 - l1.  The same device function
//               as the crop's (its extra clamps of i0 and l1 never bind for a src computed this way).
//   blend     : wy0 * (wx0 * p00 + wx1 * p01) + wy1 * (wx0 * p10 + wx1 * p11) per channel in fp32, in that order, no contraction into FMA: the crop's blend.
//   rounding  : q = clip(floor(v + 0.5), 0, 255), stored as the byte it is.
//   source    : frame k is described by six host integers: byte offset into `src`, h, w, x0, sw, row stride in bytes.  Only columns [x0, x0 + sw) of the image
//               are behind `src` (rows of 3 sw packed bytes, row_stride apart); the entry point refuses a range that does not hold every tap of panel
//               columns [col0, col0 + pw), or that leaves [0, src_bytes).  Frames of different sizes share a call.
//   output    : frame k, row y in [0, H), panel column x in [0, pw) = column col0 + x of the H x size resize, at out + out_off[k] + y * out_row_stride + 3 x:
//               straight into the frame strip, as vt_render_panel_u8 writes its panels.  No other byte is touched.
//
// MI355X mapping: three streaming kernels, VALU only, no LDS, no scratch, no float atomics.
//   inp_bbox      a grid-stride pass over the two masks, 16 pixels per lane and step (one 16-byte load per mask; rows of a multiple of 16 pixels from
//                 16-byte aligned bases) or 1 pixel per lane otherwise; per-lane min / max, wave reduction with shuffles, four integer atomics per wave
//                 that saw a pixel.  Reads 2 H W bytes per frame.
//   inp_crop      one thread per output pixel, all five channels: 4 taps x 5 bytes.  Lanes of a wave are 64 neighbours of an output row, so their taps
//                 fall into two source rows of ~150 pixels: every cache line that is fetched is used by the lanes around it.  Stores are five coalesced
//                 256-byte rows per wave.  Reads at most 5 n^2 bytes, writes 20 S^2 bytes per frame.
//   inp_panel     one thread per output pixel, all three channels: 4 taps x 3 byte loads, 3 byte stores (plain C++: vector memory instructions only).  The
//                 frames' descriptors travel in the kernel's arguments (up to 16 frames a launch): no descriptor upload, no synchronisation.  64 neighbours of
//                 an output row per wave, as above.  Reads at most 3 h sw bytes, writes 3 H pw bytes per frame.
#include "common.h"

#define INP_T 256

__device__ __forceinline__ int inp_wave_min(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ int inp_wave_max(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

__global__ void inp_bbox_init_kernel(int *__restrict__ box, int B, int H, int W)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    box[4 * b + 0] = W; box[4 * b + 1] = H; box[4 * b + 2] = -1; box[4 * b + 3] = -1;
}

// bit k = pixel k of the 4 packed in a dword counts
__device__ __forceinline__ unsigned inp_hits4(unsigned p, unsigned o, int thres)
{
    unsigned bits = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int s = (int)((((p >> (8 * k)) & 255u) + ((o >> (8 * k)) & 255u)) & 255u);          // uint8 wrap
        bits |= (s > thres ? 1u : 0u) << k;
    }
    return bits;
}

template <bool VEC>
__global__ __launch_bounds__(INP_T) void inp_bbox_kernel(const unsigned char *__restrict__ pm, const unsigned char *__restrict__ om, int H, int W, int thres,
                                                         int *__restrict__ box)
{
    const int b = blockIdx.y;
    const int npix = H * W;                                          // <= 2^30, checked by the entry point: no index below overflows
    const unsigned char *p = pm + (long long)b * npix, *o = om + (long long)b * npix;
    int x0 = W, y0 = H, x1 = -1, y1 = -1;
    const int stride = gridDim.x * INP_T;
    if (VEC) {
        const int nchunk = npix >> 4;                                // W % 16 == 0: the 16 pixels of a chunk lie in one row
        for (int c = blockIdx.x * INP_T + threadIdx.x; c < nchunk; c += stride) {
            const uint4 a = reinterpret_cast<const uint4 *>(p)[c], d = reinterpret_cast<const uint4 *>(o)[c];
            const unsigned bits = inp_hits4(a.x, d.x, thres) | (inp_hits4(a.y, d.y, thres) << 4) | (inp_hits4(a.z, d.z, thres) << 8)
                                  | (inp_hits4(a.w, d.w, thres) << 12);
            if (bits) {
                const int i = c << 4, y = i / W, x = i - y * W;
                x0 = min(x0, x + __ffs((int)bits) - 1); x1 = max(x1, x + 31 - __clz((int)bits));
                y0 = min(y0, y); y1 = max(y1, y);
            }
        }
    } else {
        for (int i = blockIdx.x * INP_T + threadIdx.x; i < npix; i += stride) {
            const int s = ((int)p[i] + (int)o[i]) & 255;
            if (s > thres) {
                const int y = i / W, x = i - y * W;
                x0 = min(x0, x); x1 = max(x1, x); y0 = min(y0, y); y1 = max(y1, y);
            }
        }
    }
    x0 = inp_wave_min(x0); y0 = inp_wave_min(y0); x1 = inp_wave_max(x1); y1 = inp_wave_max(y1);
    if ((threadIdx.x & 63) == 0 && x1 >= 0) {
        atomicMin(box + 4 * b + 0, x0); atomicMin(box + 4 * b + 1, y0); atomicMax(box + 4 * b + 2, x1); atomicMax(box + 4 * b + 3, y1);
    }
}

extern "C" int vt_mask_bbox(const unsigned char *pm, const unsigned char *om, int B, int H, int W, int thres, int *box, void *stream)
{
    VT_REQUIRE(pm && om && box && B > 0 && B <= 65535 && H > 0 && W > 0 && (long long)H * W <= (1LL << 30), "vt_mask_bbox: bad argument");
    hipStream_t st = vt_stream(stream);
    hipLaunchKernelGGL(inp_bbox_init_kernel, dim3((B + INP_T - 1) / INP_T), dim3(INP_T), 0, st, box, B, H, W);
    VT_LAUNCH_CHECK();
    const bool vec = W % 16 == 0 && ((reinterpret_cast<uintptr_t>(pm) | reinterpret_cast<uintptr_t>(om)) & 15) == 0;
    const long long work = vec ? ((long long)H * W) >> 4 : (long long)H * W;
    long long blocks = (work + INP_T - 1) / INP_T;
    blocks = blocks < 1 ? 1 : (blocks > 256 ? 256 : blocks);        // grid-stride: at most 256 workgroups per frame, a few steps per lane at 1536 x 2048
    if (vec) hipLaunchKernelGGL(inp_bbox_kernel<true>, dim3((unsigned)blocks, B), dim3(INP_T), 0, st, pm, om, H, W, thres, box);
    else hipLaunchKernelGGL(inp_bbox_kernel<false>, dim3((unsigned)blocks, B), dim3(INP_T), 0, st, pm, om, H, W, thres, box);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

// taps of output index d of an axis with n crop pixels (torch: area_pixel_compute_source_index + guard_index_and_lambda); also run on the host, where
// vt_resize_panel_u8 checks the staged columns against it
__host__ __device__ __forceinline__ void inp_taps(int d, int n, int out_size, int &i0, int &i1, float &lam)
{
    const float scale = (float)n / (float)out_size;
    float src = scale * ((float)d + 0.5f) - 0.5f;
    src = src < 0.f ? 0.f : src;
    i0 = (int)src < n - 1 ? (int)src : n - 1;
    i1 = i0 + 1 < n - 1 ? i0 + 1 : n - 1;
    lam = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
}

// blend of the four taps (a b = row i0, c d = row i1) and rounding to a grey level: the contract's `blend` and `rounding`
__device__ __forceinline__ int inp_blend_round(float a, float b, float c, float d, float w0, float w1, float h0, float h1)
{
    const float x = (a * w0 + b * w1) * h0 + (c * w0 + d * w1) * h1;
    return (int)fminf(fmaxf(floorf(x + 0.5f), 0.f), 255.f);
}

__global__ __launch_bounds__(INP_T) void inp_crop_kernel(const unsigned char *__restrict__ rgb, const unsigned char *__restrict__ pm,
                                                         const unsigned char *__restrict__ om, int H, int W, const int *__restrict__ corners, int crop_size,
                                                         int S, const float *__restrict__ table, float *__restrict__ out, long long frame_stride)
{
    const int b = blockIdx.z, dx = blockIdx.x * 64 + threadIdx.x, dy = blockIdx.y * 4 + threadIdx.y;
    if (dx >= S || dy >= S) return;
    const int tlx = corners[4 * b + 0], tly = corners[4 * b + 1], brx = corners[4 * b + 2], bry = corners[4 * b + 3];
    const long long plane = (long long)S * S;
    float *o = out + (long long)b * frame_stride + (long long)dy * S + dx;
    // not a crop of crop_size, or corners beyond +-2^29 (nothing below may overflow an int; ops.crop_resize_compose refuses both): zeros, nothing is read
    const int lim = 1 << 29;
    const bool sane = tlx > -lim && tlx < lim && tly > -lim && tly < lim && brx > -lim && brx < lim && bry > -lim && bry < lim;
    const int nx = sane ? brx - tlx : 0, ny = sane ? bry - tly : 0;
    if (nx <= 0 || ny <= 0 || abs(nx - crop_size) > 1 || abs(ny - crop_size) > 1) {
#pragma unroll
        for (int c = 0; c < 5; c++) o[c * plane] = 0.f;
        return;
    }
    int ix0, ix1, iy0, iy1;
    float w1, h1;
    inp_taps(dx, nx, S, ix0, ix1, w1);
    inp_taps(dy, ny, S, iy0, iy1, h1);
    const float w0 = 1.f - w1, h0 = 1.f - h1;
    const int xlo = max(0, tlx), xhi = min(W - 1, brx), ylo = max(0, tly), yhi = min(H - 1, bry);
    const int xs[2] = {tlx + ix0, tlx + ix1}, ys[2] = {tly + iy0, tly + iy1};
    const long long frame = (long long)b * H * W;
    float v[2][2][5];
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const bool ok = xs[i] >= xlo && xs[i] < xhi && ys[j] >= ylo && ys[j] < yhi;          // inside [0, W - 1) x [0, H - 1): in bounds
            const long long idx = ok ? frame + (long long)ys[j] * W + xs[i] : 0;
            v[j][i][0] = ok ? (float)rgb[3 * idx + 0] : 0.f;
            v[j][i][1] = ok ? (float)rgb[3 * idx + 1] : 0.f;
            v[j][i][2] = ok ? (float)rgb[3 * idx + 2] : 0.f;
            v[j][i][3] = ok ? (float)pm[idx] : 0.f;
            v[j][i][4] = ok ? (float)om[idx] : 0.f;
        }
    int q[5];
#pragma unroll
    for (int c = 0; c < 5; c++) q[c] = inp_blend_round(v[0][0][c], v[0][1][c], v[1][0][c], v[1][1][c], w0, w1, h0, h1);
    const bool comb = q[3] >= 128 || q[4] >= 128;
#pragma unroll
    for (int c = 0; c < 3; c++) o[c * plane] = table[comb ? q[c] : 0];
    o[3 * plane] = table[q[3]];
    o[4 * plane] = table[q[4]];
}

extern "C" int vt_crop_resize_compose(const unsigned char *rgb, const unsigned char *pm, const unsigned char *om, int B, int H, int W, const int *corners,
                                      int crop_size, int out_size, const float *table, float *out, long long frame_stride, void *stream)
{
    VT_REQUIRE(rgb && pm && om && corners && table && out && B > 0 && B <= 65535 && H > 0 && W > 0 && (long long)H * W <= (1LL << 30) && crop_size > 0 && crop_size < (1 << 28)
               && out_size > 0 && out_size <= 16384 && frame_stride >= 5LL * out_size * out_size, "vt_crop_resize_compose: bad argument");
    hipStream_t st = vt_stream(stream);
    hipLaunchKernelGGL(inp_crop_kernel, dim3((out_size + 63) / 64, (out_size + 3) / 4, B), dim3(64, 4), 0, st, rgb, pm, om, H, W, corners, crop_size, out_size,
                       table, out, frame_stride);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

// ---- the camera panel of step 7 ---------------------------------------------------------------------------------------------------------------------------
#define INP_PANEL_FRAMES 16
struct InpPanelFrames {                                              // a launch's frames, by value in the kernel's arguments
    long long off[INP_PANEL_FRAMES], row_stride[INP_PANEL_FRAMES];
    int h[INP_PANEL_FRAMES], w[INP_PANEL_FRAMES], x0[INP_PANEL_FRAMES], sw[INP_PANEL_FRAMES];
};

__global__ __launch_bounds__(INP_T) void inp_panel_kernel(const unsigned char *__restrict__ src, const InpPanelFrames f, int H, int size, int col0, int pw,
                                                          unsigned char *__restrict__ out, const long long *__restrict__ out_off, long long out_row_stride)
{
    const int k = blockIdx.z, px = blockIdx.x * 64 + threadIdx.x, dy = blockIdx.y * 4 + threadIdx.y;
    if (px >= pw || dy >= H) return;
    const int h = f.h[k], w = f.w[k], x0 = f.x0[k], sw = f.sw[k];
    int ix0, ix1, iy0, iy1;
    float w1, h1;
    inp_taps(col0 + px, w, size, ix0, ix1, w1);
    inp_taps(dy, h, H, iy0, iy1, h1);
    const float w0 = 1.f - w1, h0 = 1.f - h1;
    // image column -> staged column.  The entry point has checked that every tap is staged; the clamp keeps the loads inside the row whatever happens
    const int sx0 = min(max(ix0 - x0, 0), sw - 1), sx1 = min(max(ix1 - x0, 0), sw - 1);
    const unsigned char *r0 = src + f.off[k] + (long long)iy0 * f.row_stride[k], *r1 = src + f.off[k] + (long long)iy1 * f.row_stride[k];
    unsigned char *o = out + out_off[k] + (long long)dy * out_row_stride + 3 * px;
#pragma unroll
    for (int c = 0; c < 3; c++)
        o[c] = (unsigned char)inp_blend_round((float)r0[3 * sx0 + c], (float)r0[3 * sx1 + c], (float)r1[3 * sx0 + c], (float)r1[3 * sx1 + c], w0, w1, h0, h1);
}

// frames: HOST, n x 6 = byte offset into src, h, w, x0, sw, row stride (bytes); out_off: DEVICE, n byte offsets into out
extern "C" int vt_resize_panel_u8(const unsigned char *src, long long src_bytes, const long long *frames, int n, int H, int size, int col0, int pw,
                                  unsigned char *out, const long long *out_off, long long out_row_stride, void *stream)
{
    VT_REQUIRE(src && frames && out && out_off && src_bytes > 0 && n > 0 && H > 0 && H <= 16384 && size > 0 && size <= 16384 && col0 >= 0 && pw > 0
               && col0 + pw <= size && out_row_stride >= 3LL * pw, "vt_resize_panel_u8: bad argument");
    for (int k = 0; k < n; k++) {
        const long long off = frames[6 * k], h = frames[6 * k + 1], w = frames[6 * k + 2], x0 = frames[6 * k + 3], sw = frames[6 * k + 4], rs = frames[6 * k + 5];
        VT_REQUIRE(h > 0 && w > 0 && h <= (1 << 20) && w <= (1 << 20) && x0 >= 0 && sw > 0 && x0 + sw <= w && rs >= 3 * sw && rs <= (1LL << 31),
                   "vt_resize_panel_u8: frame %d: bad size (h %lld, w %lld, staged columns [%lld, %lld), row stride %lld)", k, h, w, x0, x0 + sw, rs);
        VT_REQUIRE(off >= 0 && off <= src_bytes && (h - 1) * rs + 3 * sw <= src_bytes - off,          // h <= 2^20, rs <= 2^31: no overflow
                   "vt_resize_panel_u8: frame %d: rows leave the %lld source bytes", k, src_bytes);
        int lo, hi, t;
        float lam;
        inp_taps(col0, (int)w, size, lo, t, lam);                    // the taps grow with the output column: the first column's i0, the last one's i1
        inp_taps(col0 + pw - 1, (int)w, size, t, hi, lam);
        VT_REQUIRE(x0 <= lo && hi < x0 + sw, "vt_resize_panel_u8: frame %d: staged columns [%lld, %lld) do not hold the taps [%d, %d] of panel columns [%d, %d)",
                   k, x0, x0 + sw, lo, hi, col0, col0 + pw);
    }
    hipStream_t st = vt_stream(stream);
    for (int s = 0; s < n; s += INP_PANEL_FRAMES) {
        const int g = n - s < INP_PANEL_FRAMES ? n - s : INP_PANEL_FRAMES;
        InpPanelFrames f = {};
        for (int k = 0; k < g; k++) {
            const long long *d = frames + 6 * (s + k);
            f.off[k] = d[0]; f.h[k] = (int)d[1]; f.w[k] = (int)d[2]; f.x0[k] = (int)d[3]; f.sw[k] = (int)d[4]; f.row_stride[k] = d[5];
        }
        hipLaunchKernelGGL(inp_panel_kernel, dim3((pw + 63) / 64, (H + 3) / 4, g), dim3(64, 4), 0, st, src, f, H, size, col0, pw, out, out_off + s,
                           out_row_stride);
        VT_LAUNCH_CHECK();
    }
    return VT_OK;
}
