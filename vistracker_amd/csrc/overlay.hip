// overlay.hip -- the fit on the camera image (demo.sh step 7): the kid = test_id render composited over the frame's camera panel, and a ground-truth-free
// score of a frame, the overlap of the rasteriser's owner map with the person and object masks the loader decodes.  The reference declares -am / --add_mask
// for the former (render/render_recon.py:346) and never reads it, and has nothing like the latter: both rules are this project's own, written down here and
// restated in float64 / integers by tests/overlay_model.py.
//
// CONTRACT of vt_overlay_panel_u8:
//   inputs    : rgb (B,S,S,3), alpha (B,S,S) of a vt_render_rgb call WITHOUT a static layer and with background (0,0,0): rgb is then premultiplied by coverage,
//               the 2 x 2 anti-aliasing average included (an uncovered sample adds 0 to both).  Crop rows [row0, row0 + nrows) x columns [col0, col0 + ncols),
//               as vt_render_panel_u8 takes it.
//   panels    : one uint8 buffer `out`, rows out_row_stride bytes apart, pixels packed: view b reads its source panel at out + src_off[b] and writes its
//               destination panel at out + dst_off[b] (DEVICE int64 byte offsets).  src_off[b] == dst_off[b] (in place) is allowed -- a thread reads the three
//               bytes of its pixel before it writes them -- any other overlap of a source with a destination is not.
//   rule      : per pixel and channel c, p = the source byte, in fp32, in this order, no contraction into FMA:
//                   a = opacity * alpha,   v = (255 * opacity) * min(max(rgb_c, 0), 1) + (1 - a) * p,   q = clip(floor(v + 0.5), 0, 255).
//               Where alpha == 0 and rgb == 0, and for opacity == 0, v = 0 + 1 * p and q = p, bit for bit.
//   output    : rows [0, nrows) x 3 ncols bytes of every destination panel; no other byte of `out` is written.
//   refusals  : VT_ERR_ARG before any launch for null pointers, non-positive sizes, a crop outside [0, S), rows that overlap (out_row_stride < 3 ncols), an
//               opacity outside [0, 1] (NaN included).
//
// CONTRACT of vt_mask_score:
//   owners    : fidx (B,is,is) int32, the face_index of a vt_render_rgb call WITHOUT a static layer over F faces (image row 0 = top, as it is stored).  A doubled
//               id d maps to the face d < F ? d : d - F; -1 and anything >= 2 F map to none.  A face < nf_body is body (class 0), a face < nf_body + nf_obj is
//               object (class 1), later faces (contact spheres) are neither.
//   masks     : uint8, frame b's person mask behind pm and object mask behind om, described by eight HOST integers frames[8 b ..] = byte offset of the person
//               mask in pm, byte offset of the object mask in om, h, w, pixel stride and row stride of the person mask, pixel stride and row stride of the
//               object mask (bytes; pixel stride 1 for an (h,w) mask, C for an (h,w,C) one, whose channel 0 is read as sequence_io.masks2bbox reads it).  A pixel
//               is on when its value > thres (127).  Every descriptor is checked against pm_bytes / om_bytes before anything is launched.  pm and om may be the
//               same buffer; frames of different sizes share a call, several views may name the same masks.
//   sampling  : raster sample (yi, xi), yi in [0, rows), xi in [0, is), reads mask pixel sy = ((2 yi + 1) h) / (2 rows), sx = ((2 xi + 1) w) / (2 is), integer
//               divisions: nearest neighbour at half-pixel centres, exact.  (rows = H is / S for the H panel rows of a step-7 frame.)
//   output    : count (B,2,4) int32, zeroed by the entry point on the stream; class 0 = body against pm, class 1 = object against om:
//               [0] inter  owner is the class and the mask is on      [1] fit     owner is the class
//               [2] mask   the mask is on                             [3] hidden  the mask is on and the owner is the OTHER class
//   Integer arithmetic only: bit-identical from run to run, independent of B and of a frame's place in the batch.
//
// MI355X mapping: two streaming kernels, VALU only, no scratch, no float atomics.
//   ovl_panel   one thread per output pixel and all three channels: 16 B of render, 3 byte loads, 3 byte stores (plain C++: vector memory instructions only).
//               A wave is 64 neighbours of a panel row.  No LDS, no atomics.
//   ovl_score   at most OVL_SCORE_WGS workgroups of 256 lanes per frame, grid-stride over the rows x is samples with (yi, xi) advanced incrementally (no
//               division for the position; the two of the sampling rule are 32-bit wherever (2 is) max(h, w) fits, which it does up to is = 2048 at 2^20
//               pixels).  Eight integer counters per lane, wave reduction with shuffles, one 128-byte LDS step across the four waves, then lanes 0..7 of the
//               workgroup add their non-zero sums: at most 8 integer atomics per workgroup, 8 OVL_SCORE_WGS per frame (inputs.hip's bounding box pays for 4096
//               on four addresses).  The frames' descriptors travel in the kernel's arguments, 16 frames a launch.
#include "common.h"

#define OVL_T 256
#define OVL_SCORE_WGS 64
#define OVL_SCORE_FRAMES 16

__global__ __launch_bounds__(OVL_T) void ovl_panel_kernel(const float *__restrict__ rgb, const float *__restrict__ alpha, int size, int row0, int nrows, int col0,
                                                          int ncols, unsigned char *out, const long long *__restrict__ src_off,
                                                          const long long *__restrict__ dst_off, long long out_row_stride, float opacity)
{
    const int b = blockIdx.z, x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= ncols || y >= nrows) return;
    const size_t pix = ((size_t)b * size + row0 + y) * size + col0 + x;
    const long long at = (long long)y * out_row_stride + 3 * x;
    const unsigned char *s = out + src_off[b] + at;
    unsigned char *d = out + dst_off[b] + at;
    const float keep = 1.0f - opacity * alpha[pix], gain = 255.0f * opacity;
    float p[3];
#pragma unroll
    for (int c = 0; c < 3; c++) p[c] = (float)s[c];                                        // all reads before the first write: in place is safe
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float v = gain * fminf(fmaxf(rgb[3 * pix + c], 0.f), 1.f) + keep * p[c];
        d[c] = (unsigned char)(int)fminf(fmaxf(floorf(v + 0.5f), 0.f), 255.f);
    }
}

extern "C" int vt_overlay_panel_u8(const float *rgb, const float *alpha, int B, int size, int row0, int nrows, int col0, int ncols, unsigned char *out,
                                   const long long *src_off, const long long *dst_off, long long out_row_stride, float opacity, void *stream)
{
    VT_REQUIRE(rgb && alpha && out && src_off && dst_off && B > 0 && B <= 65535 && size > 0 && size <= 32768 && row0 >= 0 && col0 >= 0 && nrows > 0 && ncols > 0
               && nrows <= size - row0 && ncols <= size - col0 && out_row_stride >= 3LL * ncols, "vt_overlay_panel_u8: bad argument");
    VT_REQUIRE(opacity >= 0.f && opacity <= 1.f, "vt_overlay_panel_u8: opacity %g outside [0, 1]", (double)opacity);
    hipStream_t st = vt_stream(stream);
    hipLaunchKernelGGL(ovl_panel_kernel, dim3((ncols + 63) / 64, (nrows + 3) / 4, B), dim3(64, 4), 0, st, rgb, alpha, size, row0, nrows, col0, ncols, out, src_off,
                       dst_off, out_row_stride, opacity);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

// ---- the mask score -------------------------------------------------------------------------------------------------------------------------------------------
struct OvlScoreFrames {                                              // a launch's frames, by value in the kernel's arguments
    long long pm_off[OVL_SCORE_FRAMES], om_off[OVL_SCORE_FRAMES], pm_rs[OVL_SCORE_FRAMES], om_rs[OVL_SCORE_FRAMES];
    int h[OVL_SCORE_FRAMES], w[OVL_SCORE_FRAMES], pm_ps[OVL_SCORE_FRAMES], om_ps[OVL_SCORE_FRAMES];
};

__device__ __forceinline__ int ovl_wave_sum(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// floor(((2 i + 1) n) / (2 m)): 32-bit when the entry point found that every such product fits, 64-bit otherwise (the same quotient either way)
template <bool SMALL>
__device__ __forceinline__ int ovl_src(int i, int n, int m)
{
    if (SMALL) return (int)(((unsigned)(2 * i + 1) * (unsigned)n) / (unsigned)(2 * m));
    return (int)(((long long)(2 * i + 1) * n) / (2LL * m));
}

template <bool SMALL>
__global__ __launch_bounds__(OVL_T) void ovl_score_kernel(const int *__restrict__ fidx, int is, int rows, int F, int nf_body, int nf_obj,
                                                          const unsigned char *__restrict__ pm, const unsigned char *__restrict__ om, const OvlScoreFrames f,
                                                          int thres, int *__restrict__ count)
{
    __shared__ int red[OVL_T / 64][8];
    const int k = blockIdx.y, t = threadIdx.x;
    const int h = f.h[k], w = f.w[k], pps = f.pm_ps[k], ops_ = f.om_ps[k];
    const long long prs = f.pm_rs[k], ors = f.om_rs[k];
    const unsigned char *p = pm + f.pm_off[k], *o = om + f.om_off[k];
    const int *own = fidx + (size_t)k * is * is;
    const int n = rows * is;                                         // < 2^30: rows <= is < 32768
    const int stride = gridDim.x * OVL_T, dy = stride / is, dx = stride - dy * is;
    int c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int i = blockIdx.x * OVL_T + t;
    int yi = i / is, xi = i - yi * is;
    for (; i < n; i += stride) {
        const int d = own[i];
        const int face = d < 0 ? -1 : (d < F ? d : (d - F < F ? d - F : -1));
        const bool body = face >= 0 && face < nf_body, obj = face >= nf_body && face - nf_body < nf_obj;
        const int sy = min(ovl_src<SMALL>(yi, h, rows), h - 1), sx = min(ovl_src<SMALL>(xi, w, is), w - 1);
        const bool pon = (int)p[sy * prs + (long long)sx * pps] > thres, oon = (int)o[sy * ors + (long long)sx * ops_] > thres;
        c[0] += body && pon; c[1] += body; c[2] += pon; c[3] += pon && obj;
        c[4] += obj && oon; c[5] += obj; c[6] += oon; c[7] += oon && body;
        yi += dy; xi += dx;
        if (xi >= is) { xi -= is; yi++; }
    }
#pragma unroll
    for (int e = 0; e < 8; e++) c[e] = ovl_wave_sum(c[e]);
    if ((t & 63) == 0) {
#pragma unroll
        for (int e = 0; e < 8; e++) red[t >> 6][e] = c[e];
    }
    __syncthreads();
    if (t < 8) {
        int s = 0;
#pragma unroll
        for (int wv = 0; wv < OVL_T / 64; wv++) s += red[wv][t];
        if (s) atomicAdd(count + 8 * (size_t)k + t, s);
    }
}

// frames: HOST, B x 8 = byte offset of the person mask in pm, of the object mask in om, h, w, pixel stride and row stride of the person mask, of the object mask
extern "C" int vt_mask_score(const int *fidx, int B, int is, int rows, int F, int nf_body, int nf_obj, const unsigned char *pm, long long pm_bytes,
                             const unsigned char *om, long long om_bytes, const long long *frames, int thres, int *count, void *stream)
{
    VT_REQUIRE(fidx && pm && om && frames && count && B > 0 && is > 0 && is < 32768 && rows > 0 && rows <= is && F > 0 && F < (1 << 30) && nf_body >= 0 && nf_obj >= 0
               && (long long)nf_body + nf_obj <= F && pm_bytes > 0 && om_bytes > 0 && thres >= 0 && thres <= 255, "vt_mask_score: bad argument");
    bool small = true;
    for (int k = 0; k < B; k++) {
        const long long *d = frames + 8 * k;
        const long long h = d[2], w = d[3];
        VT_REQUIRE(h > 0 && w > 0 && h <= (1 << 20) && w <= (1 << 20), "vt_mask_score: frame %d: bad size (h %lld, w %lld)", k, h, w);
        for (int m = 0; m < 2; m++) {
            const long long off = d[m], ps = d[4 + 2 * m], rs = d[5 + 2 * m], bytes = m ? om_bytes : pm_bytes;
            VT_REQUIRE(ps > 0 && ps <= 64 && rs >= w * ps && rs <= (1LL << 31), "vt_mask_score: frame %d: %s mask: bad strides (pixel %lld, row %lld, w %lld)", k,
                       m ? "object" : "person", ps, rs, w);
            VT_REQUIRE(off >= 0 && off <= bytes && (h - 1) * rs + (w - 1) * ps + 1 <= bytes - off,          // h <= 2^20, rs <= 2^31: no overflow
                       "vt_mask_score: frame %d: %s mask leaves its %lld bytes", k, m ? "object" : "person", bytes);
        }
        small = small && 2LL * rows * h < (1LL << 31) && 2LL * is * w < (1LL << 31);                       // (2 i + 1) n < 2 m n for i < m
    }
    hipStream_t st = vt_stream(stream);
    VT_HIP(hipMemsetAsync(count, 0, sizeof(int) * 8 * (size_t)B, st));
    const long long n = (long long)rows * is;
    long long wgs = (n + OVL_T - 1) / OVL_T;
    wgs = wgs > OVL_SCORE_WGS ? OVL_SCORE_WGS : wgs;
    for (int s = 0; s < B; s += OVL_SCORE_FRAMES) {
        const int g = B - s < OVL_SCORE_FRAMES ? B - s : OVL_SCORE_FRAMES;
        OvlScoreFrames f = {};
        for (int k = 0; k < g; k++) {
            const long long *d = frames + 8 * (s + k);
            f.pm_off[k] = d[0]; f.om_off[k] = d[1]; f.h[k] = (int)d[2]; f.w[k] = (int)d[3];
            f.pm_ps[k] = (int)d[4]; f.pm_rs[k] = d[5]; f.om_ps[k] = (int)d[6]; f.om_rs[k] = d[7];
        }
        const int *fi = fidx + (size_t)s * is * is;
        int *cn = count + 8 * (size_t)s;
        if (small) hipLaunchKernelGGL(ovl_score_kernel<true>, dim3((unsigned)wgs, g), dim3(OVL_T), 0, st, fi, is, rows, F, nf_body, nf_obj, pm, om, f, thres, cn);
        else hipLaunchKernelGGL(ovl_score_kernel<false>, dim3((unsigned)wgs, g), dim3(OVL_T), 0, st, fi, is, rows, F, nf_body, nf_obj, pm, om, f, thres, cn);
        VT_LAUNCH_CHECK();
    }
    return VT_OK;
}
