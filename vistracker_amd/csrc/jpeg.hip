// jpeg.hip -- baseline sequential JPEG (JFIF) encoder for batches of 8-bit RGB frames in device memory: the video of demo step 7
// (render/render_recon.py:113-115, 169, 188: frames appended to an imageio FFMPEG writer; here Motion-JPEG, vistracker_amd/video.py writes the AVI).
//
// CONTRACT (restated independently in tests/jpeg_model.py, float64):
//   input     : n frames of H x W x 3 uint8, frame f at rgb + f * frame_stride, rows row_stride bytes apart, pixels packed (3 bytes).  Any
//               1 <= H, W <= 65535.  The image is padded to whole MCUs by replicating its last row and column (libjpeg's edge rule).
//   colour    : JFIF full-range BT.601 in fp32, no intermediate rounding to 8 bits:
//               Y = .299 R + .587 G + .114 B,  Cb = -.168736 R - .331264 G + .5 B + 128,  Cr = .5 R - .418688 G - .081312 B + 128.
//   chroma    : 4:2:0 (MCU 16 x 16: Y0 Y1 Y2 Y3 Cb Cr) = the mean of the 2 x 2 fp32 values of the padded image, or 4:4:4 (MCU 8 x 8: Y Cb Cr).
//   transform : level shift -128, orthonormal 8 x 8 DCT-II in fp32, separable (rows, then columns).
//   quantise  : coefficient / table entry, rounded half away from zero.  Tables: Annex K luminance / chrominance scaled by IJG's quality rule
//               (libjpeg jpeg_set_quality, force_baseline): s = q < 50 ? 5000 / q : 200 - 2 q, entry = clamp((base s + 50) / 100, 1, 255), integer
//               division, 1 <= q <= 100.
//   entropy   : the Annex K Huffman tables (DC / AC, luminance / chrominance), no optimised-table pass.  Restart interval = one MCU row: every MCU
//               row is a segment with its own DC predictor reset, its own 1-bit padding to a byte boundary and its own 0xFF 0x00 stuffing;
//               RSTm (m = row & 7) between segments, EOI after the last.  The output of a frame is the entropy-coded data after SOS; the header
//               (SOI ... SOS, the same for every frame of a size / quality / subsampling) is built on the host (video.jfif_header).
//   bound     : the Annex K tables give at most 22 + 63 x 26 = 1660 bits per block before stuffing (DC: chroma category 11 has an 11-bit code
//               + 11 bits; AC: a code is at most 16 bits + 10 magnitude bits, |AC| <= 928 < 1024 for 8-bit input), stuffing at most doubles
//               a segment's bytes, + 2 marker bytes: the workspace and the caller's output buffer are sized to that, so nothing can overflow.
//   output    : bytes are a function of the frame alone -- the same whatever the batch size, the position in the batch or the strides.
//
// MI355X mapping: VALU + a little LDS, integer atomics only (no float atomics).  Seven launches per batch, every hand-off a kernel boundary:
//   jpg_convert   one thread per chroma sample (2 x 2 or 1 pixel): colour conversion + chroma mean into fp32 planes padded to whole MCUs;
//   jpg_block     one thread per 8 x 8 block in plane order (waves stay on one component): DCT, quantisation, the 64 coefficients in zig-zag order
//                 (int16, segment order) and the block's AC bit count;
//   jpg_seg_scan  one workgroup per segment: DC difference bits (the predecessor's DC is read, no serial chain), exclusive scan of the block bit
//                 counts, zeroes the segment's used bit-buffer words;
//   jpg_pack      one thread per block: its Huffman bits at its offset -- whole 32-bit words it owns with plain stores, the shared first / last
//                 word with atomicOr (order-independent, so the result is bit-identical run to run); the last block of a segment adds the padding;
//   jpg_seg_count one workgroup per segment: its 0xFF bytes -> stuffed length + 2 marker bytes;
//   jpg_offsets   one workgroup: exclusive scan of all segment lengths -> segment offsets and the n + 1 frame offsets;
//   jpg_stuff     one workgroup per segment: per-thread chunks, 0xFF counts scanned, bytes written with 0x00 after every 0xFF, then RSTm / EOI.
// One host synchronisation reads the n + 1 offsets; one device-to-host copy moves exactly the used bytes.
#include "common.h"

#define JPG_MAX_BLOCK_BITS 1660
#define JPG_T 256

struct JpgQuant { float q[2][64]; };          // natural (row-major) order, [0] luminance, [1] chrominance

struct JpgHuff { unsigned short code[256]; unsigned char len[256]; };

constexpr unsigned char kDcLumBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr unsigned char kDcChrBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr unsigned char kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr unsigned char kAcLumBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
constexpr unsigned char kAcLumVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
constexpr unsigned char kAcChrBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
constexpr unsigned char kAcChrVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// canonical Huffman codes of a (BITS, HUFFVAL) specification (ITU T.81 Annex C), indexed by symbol
constexpr JpgHuff jpg_make_huff(const unsigned char (&bits)[16], const unsigned char *vals)
{
    JpgHuff h{};
    unsigned code = 0;
    int k = 0;
    for (int l = 1; l <= 16; l++) {
        for (int i = 0; i < bits[l - 1]; i++, k++) {
            h.code[vals[k]] = (unsigned short)code;
            h.len[vals[k]] = (unsigned char)l;
            code++;
        }
        code <<= 1;
    }
    return h;
}

// [0] DC luminance, [1] DC chrominance, [2] AC luminance, [3] AC chrominance
__constant__ JpgHuff c_jpg_huff[4] = {jpg_make_huff(kDcLumBits, kDcVals), jpg_make_huff(kDcChrBits, kDcVals), jpg_make_huff(kAcLumBits, kAcLumVals),
                                      jpg_make_huff(kAcChrBits, kAcChrVals)};

constexpr unsigned char kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                               41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                               30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr unsigned char kLumBase[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24,  40,  57,
                                        69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35,  55,  64,
                                        81, 104, 113, 92, 49, 64, 78,  87,  103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr unsigned char kChrBase[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                        99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                        99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// geometry of one call: every size below is per frame unless named otherwise
struct JpgGeom {
    int H, W, hs, vs;           // hs = vs = 2 for 4:2:0, 1 for 4:4:4
    int mcus_x, mcus_y;         // segments per frame = mcus_y
    int PW, PH, CW, CH;         // padded luminance / chroma plane sizes
    int bpm, bps;               // blocks per MCU, per segment
    int ybx, yblocks, cbx, cblocks;   // luminance blocks per row / in all, chroma blocks per row / per plane
    long long segwords;         // 32-bit words of one segment's bit buffer (worst case)
    long long segcap;           // bytes of one segment's stuffed output (worst case)
};

static inline JpgGeom jpg_geom(int H, int W, int sub)
{
    JpgGeom g{};
    g.H = H; g.W = W;
    g.hs = g.vs = (sub == 420) ? 2 : 1;
    const int mw = 8 * g.hs, mh = 8 * g.vs;
    g.mcus_x = (W + mw - 1) / mw; g.mcus_y = (H + mh - 1) / mh;
    g.PW = g.mcus_x * mw; g.PH = g.mcus_y * mh;
    g.CW = g.PW / g.hs; g.CH = g.PH / g.vs;
    g.bpm = g.hs * g.vs + 2; g.bps = g.bpm * g.mcus_x;
    g.ybx = g.PW / 8; g.yblocks = g.ybx * (g.PH / 8);
    g.cbx = g.CW / 8; g.cblocks = g.cbx * (g.CH / 8);
    g.segwords = ((long long)g.bps * JPG_MAX_BLOCK_BITS + 31) / 32 + 1;
    g.segcap = 2 * 4 * g.segwords + 2;
    return g;
}

struct JpgWs {
    float *planes;              // per frame: Y (PH x PW), Cb, Cr (CH x CW)
    short *coef;                // (n, segments, bps, 64) zig-zag order
    unsigned *acbits;           // (n, segments, bps)
    unsigned *boff;             // (n, segments, bps) bit offset of a block inside its segment
    unsigned *bitbuf;           // (n, segments, segwords)
    unsigned *segbits;          // (n, segments) bits incl. padding
    long long *seglen;          // (n, segments) stuffed bytes + 2 marker bytes
    long long *segoff;          // (n, segments) byte offset in the output
    long long *offs;            // (n + 1) frame offsets
    unsigned char *out;         // n x segments x segcap bytes (worst case)
};

static inline size_t jpg_align(size_t b) { return (b + 255) & ~(size_t)255; }

static inline size_t jpg_layout(const JpgGeom &g, int n, char *base, JpgWs *w)
{
    const size_t nseg = (size_t)n * g.mcus_y, nblk = nseg * g.bps;
    const size_t plane = (size_t)g.PW * g.PH + 2 * (size_t)g.CW * g.CH;
    size_t o = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + o : nullptr; o += jpg_align(bytes); return p; };
    char *planes = take(sizeof(float) * plane * n);
    char *coef = take(sizeof(short) * 64 * nblk);
    char *acbits = take(4 * nblk), *boff = take(4 * nblk);
    char *bitbuf = take(4 * (size_t)g.segwords * nseg);
    char *segbits = take(4 * nseg), *seglen = take(8 * nseg), *segoff = take(8 * nseg), *offs = take(8 * ((size_t)n + 1));
    char *out = take((size_t)g.segcap * nseg);
    if (w) {
        w->planes = reinterpret_cast<float *>(planes); w->coef = reinterpret_cast<short *>(coef);
        w->acbits = reinterpret_cast<unsigned *>(acbits); w->boff = reinterpret_cast<unsigned *>(boff);
        w->bitbuf = reinterpret_cast<unsigned *>(bitbuf); w->segbits = reinterpret_cast<unsigned *>(segbits);
        w->seglen = reinterpret_cast<long long *>(seglen); w->segoff = reinterpret_cast<long long *>(segoff);
        w->offs = reinterpret_cast<long long *>(offs); w->out = reinterpret_cast<unsigned char *>(out);
    }
    return o;
}

// ---- block-wide exclusive scan of 256 threads (4 waves): returns the exclusive prefix, *total the sum -------------------------------------------
template <typename T>
__device__ __forceinline__ T jpg_block_scan(T v, T *lds4, T *total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    T x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) lds4[wv] = x;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < JPG_T / 64; k++) { const T s = lds4[k]; if (k < wv) before += s; all += s; }
    __syncthreads();
    *total = all;
    return before + x - v;
}

__device__ __forceinline__ int jpg_category(int v)
{
    const unsigned a = (unsigned)(v < 0 ? -v : v);
    return a ? 32 - __clz(a) : 0;
}

// ---- 1: colour conversion + chroma mean --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(JPG_T) void jpg_convert_kernel(const unsigned char *__restrict__ rgb, long long frame_stride, long long row_stride, JpgGeom g,
                                                           float *__restrict__ planes)
{
    const int s = blockIdx.x * JPG_T + threadIdx.x, f = blockIdx.y;
    if (s >= g.CW * g.CH) return;
    const int cy = s / g.CW, cx = s - cy * g.CW;
    const unsigned char *src = rgb + (long long)f * frame_stride;
    float *Y = planes + (size_t)f * ((size_t)g.PW * g.PH + 2 * (size_t)g.CW * g.CH);
    float *Cb = Y + (size_t)g.PW * g.PH, *Cr = Cb + (size_t)g.CW * g.CH;
    float sb = 0.f, sr = 0.f;
    for (int dy = 0; dy < g.vs; dy++) {
        const int py = cy * g.vs + dy, y = min(py, g.H - 1);
        for (int dx = 0; dx < g.hs; dx++) {
            const int px = cx * g.hs + dx, x = min(px, g.W - 1);
            const unsigned char *p = src + (long long)y * row_stride + 3LL * x;
            const float r = p[0], gg = p[1], b = p[2];
            Y[(size_t)py * g.PW + px] = 0.299f * r + 0.587f * gg + 0.114f * b;
            sb += -0.168736f * r - 0.331264f * gg + 0.5f * b + 128.f;
            sr += 0.5f * r - 0.418688f * gg - 0.081312f * b + 128.f;
        }
    }
    const float inv = g.hs == 2 ? 0.25f : 1.f;
    Cb[s] = sb * inv; Cr[s] = sr * inv;
}

// ---- 2: DCT + quantisation of one 8 x 8 block per thread ---------------------------------------------------------------------------------------
// orthonormal DCT-II basis: kDct[u][x] = c(u) cos((2x + 1) u pi / 16), c(0) = sqrt(1/8), c(u > 0) = 1/2
constexpr float kDct[8][8] = {
    {0.35355339059f, 0.35355339059f, 0.35355339059f, 0.35355339059f, 0.35355339059f, 0.35355339059f, 0.35355339059f, 0.35355339059f},
    {0.49039264020f, 0.41573480615f, 0.27778511651f, 0.09754516101f, -0.09754516101f, -0.27778511651f, -0.41573480615f, -0.49039264020f},
    {0.46193976626f, 0.19134171618f, -0.19134171618f, -0.46193976626f, -0.46193976626f, -0.19134171618f, 0.19134171618f, 0.46193976626f},
    {0.41573480615f, -0.09754516101f, -0.49039264020f, -0.27778511651f, 0.27778511651f, 0.49039264020f, 0.09754516101f, -0.41573480615f},
    {0.35355339059f, -0.35355339059f, -0.35355339059f, 0.35355339059f, 0.35355339059f, -0.35355339059f, -0.35355339059f, 0.35355339059f},
    {0.27778511651f, -0.49039264020f, 0.09754516101f, 0.41573480615f, -0.41573480615f, -0.09754516101f, 0.49039264020f, -0.27778511651f},
    {0.19134171618f, -0.46193976626f, 0.46193976626f, -0.19134171618f, -0.19134171618f, 0.46193976626f, -0.46193976626f, 0.19134171618f},
    {0.09754516101f, -0.27778511651f, 0.41573480615f, -0.49039264020f, 0.49039264020f, -0.41573480615f, 0.27778511651f, -0.09754516101f}};

__global__ __launch_bounds__(JPG_T) void jpg_block_kernel(const float *__restrict__ planes, JpgGeom g, JpgQuant Q, short *__restrict__ coef,
                                                         unsigned *__restrict__ acbits)
{
    const int t = blockIdx.x * JPG_T + threadIdx.x, f = blockIdx.y;
    if (t >= g.yblocks + 2 * g.cblocks) return;
    const float *Y = planes + (size_t)f * ((size_t)g.PW * g.PH + 2 * (size_t)g.CW * g.CH);
    int comp, bx, by, pw;
    const float *pl;
    if (t < g.yblocks) { comp = 0; by = t / g.ybx; bx = t - by * g.ybx; pl = Y; pw = g.PW; }
    else {
        const int c = (t - g.yblocks) / g.cblocks, k = t - g.yblocks - c * g.cblocks;
        comp = 1 + c; by = k / g.cbx; bx = k - by * g.cbx; pw = g.CW;
        pl = Y + (size_t)g.PW * g.PH + (size_t)c * g.CW * g.CH;
    }
    // segment-order index: MCU row, MCU column, block inside the MCU
    int my, mx, b;
    if (comp == 0) { my = by / g.vs; mx = bx / g.hs; b = (by - my * g.vs) * g.hs + (bx - mx * g.hs); }
    else { my = by; mx = bx; b = g.hs * g.vs + comp - 1; }
    const size_t blk = ((size_t)f * g.mcus_y + my) * g.bps + (size_t)mx * g.bpm + b;

    float v[64];
    const float *src = pl + (size_t)(8 * by) * pw + 8 * bx;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const float4 a = *reinterpret_cast<const float4 *>(src + (size_t)r * pw);
        const float4 c = *reinterpret_cast<const float4 *>(src + (size_t)r * pw + 4);
        v[8 * r + 0] = a.x - 128.f; v[8 * r + 1] = a.y - 128.f; v[8 * r + 2] = a.z - 128.f; v[8 * r + 3] = a.w - 128.f;
        v[8 * r + 4] = c.x - 128.f; v[8 * r + 5] = c.y - 128.f; v[8 * r + 6] = c.z - 128.f; v[8 * r + 7] = c.w - 128.f;
    }
#pragma unroll
    for (int r = 0; r < 8; r++) {                      // rows
        float o[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            float s = 0.f;
#pragma unroll
            for (int x = 0; x < 8; x++) s = fmaf(kDct[u][x], v[8 * r + x], s);
            o[u] = s;
        }
#pragma unroll
        for (int u = 0; u < 8; u++) v[8 * r + u] = o[u];
    }
#pragma unroll
    for (int c = 0; c < 8; c++) {                      // columns
        float o[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            float s = 0.f;
#pragma unroll
            for (int y = 0; y < 8; y++) s = fmaf(kDct[u][y], v[8 * y + c], s);
            o[u] = s;
        }
#pragma unroll
        for (int u = 0; u < 8; u++) v[8 * u + c] = o[u];
    }

    const float *q = Q.q[comp ? 1 : 0];
    short zz[64];
#pragma unroll
    for (int k = 0; k < 64; k++) {
        const int nat = kZigzag[k];                  // constexpr: folds in the unrolled loop, v[] stays in registers
        zz[k] = (short)roundf(v[nat] / q[nat]);
    }
    // AC bits of the block (the DC difference is added by jpg_seg_scan, which sees the predecessor)
    const JpgHuff &hac = c_jpg_huff[comp ? 3 : 2];
    unsigned bits = 0;
    int run = 0;
    for (int k = 1; k < 64; k++) {
        const int a = zz[k];
        if (a == 0) { run++; continue; }
        while (run > 15) { bits += hac.len[0xf0]; run -= 16; }
        const int s = jpg_category(a);
        bits += hac.len[(run << 4) | s] + s;
        run = 0;
    }
    if (run > 0) bits += hac.len[0x00];
    int4 *dst = reinterpret_cast<int4 *>(coef + blk * 64);
#pragma unroll
    for (int k = 0; k < 8; k++) {
        int4 p;
        p.x = (zz[8 * k + 0] & 0xffff) | (zz[8 * k + 1] << 16); p.y = (zz[8 * k + 2] & 0xffff) | (zz[8 * k + 3] << 16);
        p.z = (zz[8 * k + 4] & 0xffff) | (zz[8 * k + 5] << 16); p.w = (zz[8 * k + 6] & 0xffff) | (zz[8 * k + 7] << 16);
        dst[k] = p;
    }
    acbits[blk] = bits;
}

// predecessor (same component, coding order, same segment) of block j of a segment, or -1 at the segment's start (DC predictor reset)
__device__ __forceinline__ int jpg_pred(int j, const JpgGeom &g)
{
    const int mx = j / g.bpm, b = j - mx * g.bpm, ny = g.hs * g.vs;
    if (b > 0 && b < ny) return j - 1;
    if (mx == 0) return -1;
    return b == 0 ? j - g.bpm + ny - 1 : j - g.bpm;
}
__device__ __forceinline__ int jpg_comp(int j, const JpgGeom &g)
{
    const int b = j % g.bpm, ny = g.hs * g.vs;
    return b < ny ? 0 : 1 + (b - ny);
}

// ---- 3: per segment, DC bits + exclusive scan of the block bit counts --------------------------------------------------------------------------
__global__ __launch_bounds__(JPG_T) void jpg_seg_scan_kernel(JpgGeom g, const short *__restrict__ coef, const unsigned *__restrict__ acbits,
                                                            unsigned *__restrict__ boff, unsigned *__restrict__ segbits, unsigned *__restrict__ bitbuf)
{
    __shared__ unsigned lds4[JPG_T / 64];
    const size_t seg = (size_t)blockIdx.y * g.mcus_y + blockIdx.x, base = seg * g.bps;
    unsigned carry = 0;
    for (int j0 = 0; j0 < g.bps; j0 += JPG_T) {
        const int j = j0 + threadIdx.x;
        unsigned bits = 0;
        if (j < g.bps) {
            const int p = jpg_pred(j, g);
            const int dc = coef[(base + j) * 64], pdc = p >= 0 ? coef[(base + p) * 64] : 0;
            const int s = jpg_category(dc - pdc);
            bits = acbits[base + j] + c_jpg_huff[jpg_comp(j, g) ? 1 : 0].len[s] + s;
        }
        unsigned tot;
        const unsigned ex = jpg_block_scan(bits, lds4, &tot);
        if (j < g.bps) boff[base + j] = carry + ex;
        carry += tot;
    }
    const unsigned words = ((carry + 7) / 8 + 3) / 4;
    unsigned *buf = bitbuf + seg * g.segwords;
    for (unsigned w = threadIdx.x; w < words; w += JPG_T) buf[w] = 0u;
    if (threadIdx.x == 0) segbits[seg] = (carry + 7) & ~7u;
}

// ---- 4: Huffman bits of one block per thread ---------------------------------------------------------------------------------------------------
struct JpgBits {
    unsigned *buf;
    unsigned w;                  // word the accumulator's first bit belongs to
    unsigned long long acc;      // nb pending bits, MSB first, of word w onwards
    int nb;
    bool shared;                 // word w holds bits of the previous block
    __device__ __forceinline__ void put(unsigned code, int len)
    {
        acc = (acc << len) | code; nb += len;
        while (nb >= 32) {
            nb -= 32;
            const unsigned word = (unsigned)(acc >> nb);
            acc &= (1ull << nb) - 1;
            if (shared) atomicOr(buf + w, word); else buf[w] = word;
            shared = false; w++;
        }
    }
    __device__ __forceinline__ void flush()
    {
        if (nb > 0) atomicOr(buf + w, (unsigned)(acc << (32 - nb)));
    }
};

__global__ __launch_bounds__(JPG_T) void jpg_pack_kernel(JpgGeom g, const short *__restrict__ coef, const unsigned *__restrict__ boff,
                                                        unsigned *__restrict__ bitbuf, int nseg_total)
{
    const long long i = (long long)blockIdx.x * JPG_T + threadIdx.x;
    if (i >= (long long)nseg_total * g.bps) return;
    const long long seg = i / g.bps;
    const int j = (int)(i - seg * g.bps);
    const int comp = jpg_comp(j, g), p = jpg_pred(j, g);
    // nonzero mask of the 64 zig-zag coefficients (constant indices: stays in registers), then a walk over its set bits
    const short *c = coef + i * 64;
    const int4 *src = reinterpret_cast<const int4 *>(c);
    unsigned long long nz = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int4 q = src[k];
        const unsigned w4[4] = {(unsigned)q.x, (unsigned)q.y, (unsigned)q.z, (unsigned)q.w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
            nz |= (unsigned long long)((w4[e] & 0xffffu) != 0) << (8 * k + 2 * e);
            nz |= (unsigned long long)((w4[e] >> 16) != 0) << (8 * k + 2 * e + 1);
        }
    }
    const unsigned off = boff[i];
    JpgBits bw{bitbuf + seg * g.segwords, off >> 5, 0ull, (int)(off & 31), (off & 31) != 0};
    const JpgHuff &hdc = c_jpg_huff[comp ? 1 : 0], &hac = c_jpg_huff[comp ? 3 : 2];
    const int diff = c[0] - (p >= 0 ? (int)coef[(i - j + p) * 64] : 0);
    {
        const int s = jpg_category(diff);
        const unsigned mag = (unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1);
        bw.put(((unsigned)hdc.code[s] << s) | mag, hdc.len[s] + s);
    }
    int prev = 0;
    for (unsigned long long m = nz & ~1ull; m; m &= m - 1) {
        const int k = __ffsll((long long)m) - 1, a = c[k];
        int run = k - prev - 1;
        while (run > 15) { bw.put(hac.code[0xf0], hac.len[0xf0]); run -= 16; }
        const int s = jpg_category(a), sym = (run << 4) | s;
        const unsigned mag = (unsigned)(a < 0 ? a - 1 : a) & ((1u << s) - 1);
        bw.put(((unsigned)hac.code[sym] << s) | mag, hac.len[sym] + s);
        prev = k;
    }
    if (prev != 63) bw.put(hac.code[0x00], hac.len[0x00]);
    if (j == g.bps - 1) {            // the segment's padding to a byte boundary with 1-bits (nb counts from the start of word w: nb & 7 = end & 7)
        const int fill = (8 - (bw.nb & 7)) & 7;
        if (fill) bw.put((1u << fill) - 1, fill);
    }
    bw.flush();
}

// bytes of a segment's bit buffer (big-endian inside each 32-bit word)
__device__ __forceinline__ unsigned jpg_byte(const unsigned *buf, unsigned k) { return (buf[k >> 2] >> (24 - 8 * (k & 3))) & 0xffu; }

// ---- 5: stuffed length per segment -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(JPG_T) void jpg_seg_count_kernel(JpgGeom g, const unsigned *__restrict__ segbits, const unsigned *__restrict__ bitbuf,
                                                             long long *__restrict__ seglen)
{
    __shared__ unsigned lds4[JPG_T / 64];
    const size_t seg = (size_t)blockIdx.y * g.mcus_y + blockIdx.x;
    const unsigned nbytes = segbits[seg] / 8;
    const unsigned *buf = bitbuf + seg * g.segwords;
    unsigned ff = 0;
    for (unsigned k = threadIdx.x; k < nbytes; k += JPG_T) ff += jpg_byte(buf, k) == 0xffu;
    unsigned tot;
    (void)jpg_block_scan(ff, lds4, &tot);
    if (threadIdx.x == 0) seglen[seg] = (long long)nbytes + tot + 2;
}

// ---- 6: segment and frame offsets (one workgroup) ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(JPG_T) void jpg_offsets_kernel(int n, int nseg, const long long *__restrict__ seglen, long long *__restrict__ segoff,
                                                           long long *__restrict__ offs)
{
    __shared__ long long lds4[JPG_T / 64];
    const int total_segs = n * nseg;
    long long carry = 0;
    for (int s0 = 0; s0 < total_segs; s0 += JPG_T) {
        const int s = s0 + threadIdx.x;
        const long long v = s < total_segs ? seglen[s] : 0;
        long long tot;
        const long long ex = jpg_block_scan(v, lds4, &tot);
        if (s < total_segs) {
            segoff[s] = carry + ex;
            if (s % nseg == 0) offs[s / nseg] = carry + ex;
        }
        carry += tot;
    }
    if (threadIdx.x == 0) offs[n] = carry;
}

// ---- 7: stuffing + markers into the output -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(JPG_T) void jpg_stuff_kernel(JpgGeom g, const unsigned *__restrict__ segbits, const unsigned *__restrict__ bitbuf,
                                                         const long long *__restrict__ segoff, unsigned char *__restrict__ out)
{
    __shared__ unsigned lds4[JPG_T / 64];
    const int row = blockIdx.x;
    const size_t seg = (size_t)blockIdx.y * g.mcus_y + row;
    const unsigned nbytes = segbits[seg] / 8;
    const unsigned *buf = bitbuf + seg * g.segwords;
    const unsigned chunk = (nbytes + JPG_T - 1) / JPG_T;
    const unsigned k0 = min(nbytes, threadIdx.x * chunk), k1 = min(nbytes, k0 + chunk);
    unsigned ff = 0;
    for (unsigned k = k0; k < k1; k++) ff += jpg_byte(buf, k) == 0xffu;
    unsigned tot;
    const unsigned before = jpg_block_scan(ff, lds4, &tot);
    unsigned char *o = out + segoff[seg];
    unsigned d = k0 + before;
    for (unsigned k = k0; k < k1; k++) {
        const unsigned c = jpg_byte(buf, k);
        o[d++] = (unsigned char)c;
        if (c == 0xffu) o[d++] = 0;
    }
    if (threadIdx.x == 0) {
        const unsigned e = nbytes + tot;
        o[e] = 0xff;
        o[e + 1] = (unsigned char)(row == g.mcus_y - 1 ? 0xd9 : 0xd0 + (row & 7));
    }
}


static int jpg_check_dims(int n, int H, int W, int sub)
{
    VT_REQUIRE(n > 0 && H >= 1 && W >= 1 && H <= 65535 && W <= 65535, "vt_jpeg: need n >= 1 and 1 <= H, W <= 65535 (got n %d, %d x %d)", n, H, W);
    VT_REQUIRE(sub == 420 || sub == 444, "vt_jpeg: subsampling must be 420 or 444 (got %d)", sub);
    return VT_OK;
}

extern "C" long vt_jpeg_workspace_bytes(int n, int H, int W, int subsampling, long long *max_out_bytes)
{
    if (jpg_check_dims(n, H, W, subsampling) != VT_OK) return -1;
    const JpgGeom g = jpg_geom(H, W, subsampling);
    if (max_out_bytes) *max_out_bytes = (long long)n * g.mcus_y * g.segcap;
    return (long)jpg_layout(g, n, nullptr, nullptr);
}

extern "C" int vt_jpeg_encode(const unsigned char *rgb, int n, int H, int W, long long frame_stride, long long row_stride, int quality, int subsampling,
                              void *ws, long ws_bytes, unsigned char *out, long long out_cap, long long *offsets, void *stream)
{
    {
        const int rc = jpg_check_dims(n, H, W, subsampling);
        if (rc != VT_OK) return rc;
    }
    VT_REQUIRE(rgb && ws && out && offsets, "vt_jpeg_encode: bad argument (NULL pointer)");
    VT_REQUIRE(quality >= 1 && quality <= 100, "vt_jpeg_encode: quality must be 1..100 (got %d)", quality);
    VT_REQUIRE(row_stride >= 3LL * W, "vt_jpeg_encode: row_stride %lld below 3 W = %lld", row_stride, 3LL * W);
    const JpgGeom g = jpg_geom(H, W, subsampling);
    JpgWs w{};
    const size_t need = jpg_layout(g, n, nullptr, nullptr);
    VT_REQUIRE((size_t)ws_bytes >= need && ws_bytes > 0, "vt_jpeg_encode: workspace holds %ld bytes, this call needs %zu (vt_jpeg_workspace_bytes)", ws_bytes, need);
    const long long max_out = (long long)n * g.mcus_y * g.segcap;
    VT_REQUIRE(out_cap >= max_out, "vt_jpeg_encode: output buffer holds %lld bytes, the worst case of this call is %lld (vt_jpeg_workspace_bytes)", out_cap, max_out);
    jpg_layout(g, n, static_cast<char *>(ws), &w);

    JpgQuant Q;
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int k = 0; k < 64; k++) {
        Q.q[0][k] = (float)std::min(255, std::max(1, (kLumBase[k] * s + 50) / 100));
        Q.q[1][k] = (float)std::min(255, std::max(1, (kChrBase[k] * s + 50) / 100));
    }
    hipStream_t st = vt_stream(stream);
    const int nseg = g.mcus_y;
    hipLaunchKernelGGL(jpg_convert_kernel, dim3((g.CW * g.CH + JPG_T - 1) / JPG_T, n), dim3(JPG_T), 0, st, rgb, frame_stride, row_stride, g, w.planes);
    VT_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpg_block_kernel, dim3((g.yblocks + 2 * g.cblocks + JPG_T - 1) / JPG_T, n), dim3(JPG_T), 0, st, w.planes, g, Q, w.coef, w.acbits);
    VT_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpg_seg_scan_kernel, dim3(nseg, n), dim3(JPG_T), 0, st, g, w.coef, w.acbits, w.boff, w.segbits, w.bitbuf);
    VT_LAUNCH_CHECK();
    const long long nblk = (long long)n * nseg * g.bps;
    hipLaunchKernelGGL(jpg_pack_kernel, dim3((unsigned)((nblk + JPG_T - 1) / JPG_T)), dim3(JPG_T), 0, st, g, w.coef, w.boff, w.bitbuf, n * nseg);
    VT_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpg_seg_count_kernel, dim3(nseg, n), dim3(JPG_T), 0, st, g, w.segbits, w.bitbuf, w.seglen);
    VT_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpg_offsets_kernel, dim3(1), dim3(JPG_T), 0, st, n, nseg, w.seglen, w.segoff, w.offs);
    VT_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpg_stuff_kernel, dim3(nseg, n), dim3(JPG_T), 0, st, g, w.segbits, w.bitbuf, w.segoff, w.out);
    VT_LAUNCH_CHECK();
    VT_HIP(hipMemcpyAsync(offsets, w.offs, sizeof(long long) * ((size_t)n + 1), hipMemcpyDeviceToHost, st));
    VT_HIP(hipStreamSynchronize(st));
    const long long used = offsets[n];
    VT_REQUIRE(used >= 0 && used <= max_out, "vt_jpeg_encode: internal error, %lld bytes exceed the bound %lld", used, max_out);
    VT_HIP(hipMemcpyAsync(out, w.out, (size_t)used, hipMemcpyDeviceToHost, st));
    VT_HIP(hipStreamSynchronize(st));
    return VT_OK;
}
