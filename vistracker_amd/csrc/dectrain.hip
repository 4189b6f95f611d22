// dectrain.hip -- training the five SIF-Net point decoders (model/chore.py:113-126 make_decoder): a forward from PLAIN device weights (the flat parameter
// buffer an optimiser updates every step), the gradient of the objective to every weight and bias (what loss.backward() leaves in the decoders' .grad:
// trainer/trainer.py:97-106) and, on request, its gradient to the eight feature maps (what the same backward hands on to the encoders; section 5 below).  The query kernels (query.hip, query_f32.hip) cannot serve this: they
// hold the weights as fragment layouts packed on the host at vt_sifnet_create and never expose a hidden activation.
//
// PARAMETERS.  One flat fp32 buffer: for head h (df 2, pca 9, parts 14, centers 3, vis 1) and layer l = 0..3, W_hl (out,in) row-major (torch's
// Conv1d.weight[:, :, 0]) then b_hl (out).  Layer 0's `in` axis is the reference's 611-channel order (chore_triplane.py:139-151): im_feat 256, z_feat 3,
// tmpx 64, tri_tmpx 3 x 32, tri_feat 3 x 64.  vt_decoder_param_offset is the only statement of the table.
//
// ARITHMETIC.  Every product of every GEMM is an exact fp32 product accumulated in fp32 on v_mfma_f32_16x16x4_f32 (builtins only, no inline assembly).
// The GEMMs run TRANSPOSED: out^T[unit][point] = W[unit][k] x act^T[k][point], so the (out,in) row-major weights are the A operand as they lie in memory
// (a 32-column slice of W goes through LDS by a straight, coalesced copy) and the accumulators hold four consecutive units of one point per lane (one
// 16-byte store into the point-major activation rows).  The delta propagation delta_l = (W_l^T delta_{l+1}) . [z_l > 0] uses the same code with the
// slice transposed on its way into LDS.  ReLU passes the gradient where the pre-activation is > 0 (zero at exactly 0, as torch).  vis carries the
// decoder's sigmoid (chore_tri_vis.py:22-27); df of a point that projects outside the image is OUT_DIST and receives no gradient (chore_triplane.py:155-159).
//
// WEIGHT GRADIENTS: TAPED, NOT RECOMPUTED.  dW_l = sum over points of delta_{l+1} (x) a_l is a GEMM whose K axis is the points, so both operands of all
// 20 layers must exist point-major in memory at once; recomputing them inside the split-K kernel would repeat the gathers and the forward once per
// 64 x 64 output tile (30 times per head).  vt_decoder_weight_grads therefore runs, per SLAB of at most 8192 points (at most 32 chunks):
//   1. feat_kernel   a_0 (the 611 features + one zero pad column, reference channel order) of every point of the slab -> tape
//   2. mlp_kernel<1> per (64-point tile, head): forward from the tape's a_0, a_1..a_3 -> tape, delta_4 from the upstream gradient, delta_3..delta_1 -> tape
//   3. wgrad_kernel  per (chunk, head, 64 x 64 output tile), one wave each: fp32 MFMA partial over the (at most chunk_points) points of the chunk; the bias
//                    gradient (a plain sum, no product) is the chunk's deltas added in fp64 per lane, four lanes in a fixed order, rounded once:
//                    a sequential fp32 chain over the chunk measured 4.4 .. 4.8 e32 on three of the 40 tensors, the fp64 sum costs four adds a step
//   4. finish_kernel per parameter: the slab's chunk partials added in fp64 in the order (frame, chunk) onto the fp64 running sum of the earlier slabs;
//                    the last slab rounds to fp32 once and stores (accumulate = 0) or adds to dparams (accumulate != 0)
// No atomics; every output element has one writer; the order of every sum is fixed, so the same inputs give the same bits.  The tape is 4532 floats per
// point (612 + 5 heads x (3 x 128 activations + 3 x 128 + 16 deltas)): a full tape of B = 8, N = 20 000 would be 2.9 GB, a slab is at most 297 MB (148 MB at
// the default chunk).  Rows of a ragged last tile beyond N carry a_0 = 0 and delta = 0 (exact zeros in every product); tiles wholly beyond N are neither
// written nor read.  Every workspace byte read was written by the same call.
// vt_decoder_grads adds, per slab and after step 3, the map gradient: da0_kernel (d_a0 = sum_h W_h0^T delta_h1, over a_0 in the tape), tapkey_kernel, sort_kernel,
// scatter_kernel -- described at section 5.  With dparams NULL steps 3 and 4 are not launched.
//
// DEFAULT chunk_points = 2048: 80 chunks at B = 8, N = 20 000 -> 12 000 one-wave GEMM tiles for 1024 SIMDs, 2.2 MB of partials per chunk.
#include "common.h"

namespace dect {

typedef float f32x4 __attribute__((ext_vector_type(4)));
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

#define KIN 611             /* VT_FEAT */
#define KP 612              /* tape row of a_0: 611 features + one zero column (16-byte rows) */
#define HID 128
#define FS 36               /* LDS stride of a 32-column slice row: conflict-free ds_read_b64 of the pair-step operands (query_f32.hip) */
#define HS 132              /* LDS stride of a hidden activation row */
#define GS 20               /* LDS stride of a delta_4 row */
#define NSLICE0 20          /* ceil(612 / 32) */
#define OUT_DIST 5.0f       /* chore.py:93 */
#define TAPE_HEAD (6 * HID + 16)            /* floats per point and head: a_1..a_3, delta_1..delta_3, delta_4 (16) */
#define TAPE_POINT (KP + 5 * TAPE_HEAD)
#define DEFAULT_CHUNK 2048
#define MAX_CHUNK 16384
#define SLAB_POINTS 8192
#define SLAB_MAX_CHUNKS 32
#define WG_TILES 30         /* one-wave output tiles per head: layer 0 2 x 10, layers 1, 2 2 x 2 each, layer 3 1 x 2 */

static const int kDims[5] = {2, 9, 14, 3, 1};

struct POff { int w[5][4], b[5][4], head_end[5]; };

static long head_floats(int h) { return (long)HID * KIN + HID + 2L * (HID * HID + HID) + (long)kDims[h] * (HID + 1); }
static long param_floats() { long n = 0; for (int h = 0; h < 5; h++) n += head_floats(h); return n; }
static long param_offset(int head, int layer, int is_bias)
{
    if (head < 0 || head > 4 || layer < 0 || layer > 3) return -1;
    long o = 0;
    for (int h = 0; h < head; h++) o += head_floats(h);
    for (int l = 0; l < layer; l++) o += (long)HID * (l == 0 ? KIN : HID) + HID;
    if (is_bias) o += (long)(layer == 3 ? kDims[head] : HID) * (layer == 0 ? KIN : HID);
    return o;
}
static POff make_off()
{
    POff p;
    for (int h = 0; h < 5; h++) {
        for (int l = 0; l < 4; l++) { p.w[h][l] = (int)param_offset(h, l, 0); p.b[h][l] = (int)param_offset(h, l, 1); }
        p.head_end[h] = p.b[h][3] + kDims[h];
    }
    return p;
}

struct TArgs {
    const float *params; POff off;
    const float *maps[8]; int res[8];
    const float *pts, *crop_center, *body_center;
    int B, N;
    float fx, fy, cx, cy, crop;
    float *out[5];              // forward
    const float *gout[5];       // gradient: upstream, NULL = zero
    float *tape; long rows;     // tape of the slab: `rows` point rows
    int chunk, nc, g0;          // points per chunk, chunks per frame, first global chunk (frame * nc + chunk index) of the slab
    int heads[5], nheads;       // head ids served by blockIdx.y
};

__device__ __forceinline__ int map_channels(int mi) { return mi == 0 ? 256 : (mi == 1 ? 64 : (mi < 5 ? 32 : 64)); }
__device__ __forceinline__ int map_proj(int mi) { return mi < 2 ? 0 : (mi < 5 ? mi - 1 : mi - 4); }
__device__ __forceinline__ int kout_of(int h) { return h == 0 ? 2 : (h == 1 ? 9 : (h == 2 ? 14 : (h == 3 ? 3 : 1))); }
__device__ __forceinline__ const float *tape_a0(const TArgs &a) { return a.tape; }
// part p of head slot hs: 0..2 = a_1..a_3, 3..5 = delta_1..delta_3 (128 floats a row), 6 = delta_4 (16 floats a row)
__device__ __forceinline__ float *tape_part(const TArgs &a, int h, int p) { return a.tape + a.rows * KP + (size_t)a.rows * ((size_t)h * TAPE_HEAD + (size_t)p * HID); }

// block -> (frame, first point of the tile, first tape row of the tile); false when the tile lies wholly beyond N
__device__ __forceinline__ bool tile_of_block(const TArgs &a, int &b, int &n0, long &row0)
{
    const int tpc = a.chunk >> 6, lc = blockIdx.x / tpc, t = blockIdx.x % tpc, g = a.g0 + lc;
    b = g / a.nc;
    n0 = (g % a.nc) * a.chunk + t * 64;
    row0 = (long)lc * a.chunk + t * 64;
    return n0 < a.N;
}

// per-point projections (camera.py:52-90, chore_triplane.py:207-251) of the 64 points of a tile; threads 0..63
__device__ __forceinline__ void project_tile(const TArgs &a, int b, int n0, int tid, float *sPt, int *sIn, float *sUV)
{
    if (tid < 64) {
        const int n = min(n0 + tid, a.N - 1);
        const float *p = a.pts + ((size_t)b * a.N + n) * 3;
        const float x = p[0], y = p[1], z = p[2];
        float px = a.fx * x / z + a.cx, py = a.fy * y / z + a.cy;
        px = a.crop / 2 + px - a.crop_center[2 * b]; py = a.crop / 2 + py - a.crop_center[2 * b + 1];
        const float nx = 2 * px / a.crop - 1, ny = 2 * py / a.crop - 1;
        sIn[tid] = (int)((nx >= -1.0f) && (nx <= 1.0f) && (ny >= -1.0f) && (ny <= 1.0f));
        const float c0 = x - a.body_center[3 * b], c1 = y - a.body_center[3 * b + 1], c2 = z - a.body_center[3 * b + 2];
        sPt[tid * 3] = x; sPt[tid * 3 + 1] = y; sPt[tid * 3 + 2] = z;
        if (sUV) {
            sUV[(0 * 64 + tid) * 2] = nx;  sUV[(0 * 64 + tid) * 2 + 1] = ny;   // perspective
            sUV[(1 * 64 + tid) * 2] = c2;  sUV[(1 * 64 + tid) * 2 + 1] = c1;   // right
            sUV[(2 * 64 + tid) * 2] = -c0; sUV[(2 * 64 + tid) * 2 + 1] = c1;   // back
            sUV[(3 * 64 + tid) * 2] = c0;  sUV[(3 * 64 + tid) * 2 + 1] = -c2;  // top
        }
    }
}

// the bilinear taps of (map, point), grid_sample align_corners=True, zeros padding (geometry.py:12), as query_f32.hip's taps_issue: the four texels are
// read at clamped (valid) positions and the in-bounds flags fold into the weights.  Entry = {offset of tap (y0,x0) inside the frame, flags, wx1, wy1},
// flags = (x1 != x0) | (y1 != y0) << 1 | in-bounds bits << 2.
__device__ __forceinline__ void taps_setup(const TArgs &a, const float *sUV, int4 *sTap, int tid)
{
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int e = tid + 256 * i, mi = e >> 6, pt = e & 63;
        const int R = a.res[mi], C = map_channels(mi), pr = map_proj(mi);
        const float u = sUV[(pr * 64 + pt) * 2], v = sUV[(pr * 64 + pt) * 2 + 1];
        float ix = (u + 1.0f) * 0.5f * (float)(R - 1), iy = (v + 1.0f) * 0.5f * (float)(R - 1);
        ix = fminf(fmaxf(ix, -2.0f), (float)(R + 1)); iy = fminf(fmaxf(iy, -2.0f), (float)(R + 1));
        const float fxl = floorf(ix), fyl = floorf(iy);
        const int x0 = (int)fxl, y0 = (int)fyl, x1 = x0 + 1, y1 = y0 + 1;
        const bool bx0 = x0 >= 0 && x0 < R, bx1 = x1 >= 0 && x1 < R, by0 = y0 >= 0 && y0 < R, by1 = y1 >= 0 && y1 < R;
        const int xc0 = min(max(x0, 0), R - 1), xc1 = min(max(x1, 0), R - 1), yc0 = min(max(y0, 0), R - 1), yc1 = min(max(y1, 0), R - 1);
        const int inb = (bx0 && by0 ? 1 : 0) | (bx1 && by0 ? 2 : 0) | (bx0 && by1 ? 4 : 0) | (bx1 && by1 ? 8 : 0);
        sTap[e] = make_int4((yc0 * R + xc0) * C, (xc1 - xc0) | ((yc1 - yc0) << 1) | (inb << 2), __float_as_int(ix - fxl), __float_as_int(iy - fyl));
    }
}

// feature `ch` (reference channel order, 611 = the zero pad) of point pt of the tile
__device__ __forceinline__ float feat_value(const TArgs &a, int b, int ch, int pt, const int4 *sTap, const float *sPt)
{
    if (ch >= KIN) return 0.f;
    if (ch >= 256 && ch < 259) return sPt[pt * 3 + ch - 256] - (ch == 258 ? 2.2f : 0.f);       // z_feat = (x, y, z - 2.2) (chore_triplane.py:207-218)
    int mi, c;
    if (ch < 256) { mi = 0; c = ch; }
    else if (ch < 323) { mi = 1; c = ch - 259; }
    else if (ch < 419) { mi = 2 + ((ch - 323) >> 5); c = (ch - 323) & 31; }
    else { mi = 5 + ((ch - 419) >> 6); c = (ch - 419) & 63; }
    const int4 t = sTap[mi * 64 + pt];
    const int R = a.res[mi], C = map_channels(mi);
    const float *__restrict__ p = a.maps[mi] + (size_t)b * R * R * C + t.x + c;
    const int dx = (t.y & 1) ? C : 0, dy = (t.y & 2) ? R * C : 0, ib = t.y >> 2;
    const float nw = p[0], ne = p[dx], sw = p[dy], se = p[dx + dy];
    const float wx1 = __int_as_float(t.z), wy1 = __int_as_float(t.w), wx0 = 1.0f - wx1, wy0 = 1.0f - wy1;
    const float w00 = (ib & 1) ? wx0 * wy0 : 0.f, w10 = (ib & 2) ? wx1 * wy0 : 0.f, w01 = (ib & 4) ? wx0 * wy1 : 0.f, w11 = (ib & 8) ? wx1 * wy1 : 0.f;
    return nw * w00 + ne * w10 + sw * w01 + se * w11;
}

// ---- 1. a_0 of a slab -> tape ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void feat_kernel(const TArgs a)
{
    __shared__ float sPt[64 * 3];
    __shared__ int sIn[64];
    __shared__ float sUV[4 * 64 * 2];
    __shared__ int4 sTap[8 * 64];
    int b, n0; long row0;
    if (!tile_of_block(a, b, n0, row0)) return;
    const int tid = threadIdx.x;
    project_tile(a, b, n0, tid, sPt, sIn, sUV);
    __syncthreads();
    taps_setup(a, sUV, sTap, tid);
    __syncthreads();
    float *dst = a.tape + (size_t)row0 * KP;
    const int col = tid & 31, pt0 = tid >> 5;
    for (int s = 0; s < NSLICE0; s++) {
        const int ch = 32 * s + col;
        if (ch >= KP) break;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int pt = pt0 + 8 * i;
            const float v = feat_value(a, b, ch, pt, sTap, sPt);
            dst[(size_t)pt * KP + ch] = (n0 + pt < a.N) ? v : 0.f;        // rows of a ragged tile beyond N: exact zeros
        }
    }
}

// ---- 2. the decoders of one head on a 64-point tile ----------------------------------------------------------------------------------------------------
// accumulators of one wave, D layout of the transposed GEMM: v[mt][nt][r] = unit (2 wave + mt) 16 + (lane >> 4) 4 + r of point nt 16 + (lane & 15)
struct Acc { f32x4 v[2][4]; };
__device__ __forceinline__ void acc_zero(Acc &c)
{
#pragma unroll
    for (int mt = 0; mt < 2; mt++)
#pragma unroll
        for (int nt = 0; nt < 4; nt++) c.v[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
}
// NS pair steps (k = 8 s + 2 q + e) over a 32-column slice: A = weights Wl [128 units][FS], B = activations Bs [64 points][bstride]
template <int NS>
__device__ __forceinline__ void mma_slice(Acc &c, const float *Wl, const float *Bs, int bstride, int wave, int q, int j)
{
#pragma unroll
    for (int s = 0; s < NS; s++) {
        float2 av[2], bv[4];
#pragma unroll
        for (int mt = 0; mt < 2; mt++) av[mt] = *reinterpret_cast<const float2 *>(Wl + ((2 * wave + mt) * 16 + j) * FS + 8 * s + 2 * q);
#pragma unroll
        for (int nt = 0; nt < 4; nt++) bv[nt] = *reinterpret_cast<const float2 *>(Bs + (nt * 16 + j) * bstride + 8 * s + 2 * q);
#pragma unroll
        for (int mt = 0; mt < 2; mt++)
#pragma unroll
            for (int nt = 0; nt < 4; nt++) c.v[mt][nt] = MFMA16(av[mt].x, bv[nt].x, c.v[mt][nt]);
#pragma unroll
        for (int mt = 0; mt < 2; mt++)
#pragma unroll
            for (int nt = 0; nt < 4; nt++) c.v[mt][nt] = MFMA16(av[mt].y, bv[nt].y, c.v[mt][nt]);
    }
}
// a 128 x 32 slice of the weights on its way to LDS.  T = false: Wl[n][kk] = W[n ld + k0 + kk] (columns >= lim read as 0), coalesced along the row.
// T = true: Wl[m][kk] = W[(k0 + kk) 128 + m] (rows >= lim read as 0): the slice of W^T, coalesced along the row of W as well.
struct WReg { float v[16]; };
template <bool T>
__device__ __forceinline__ void load_w(WReg &r, const float *__restrict__ W, int ld, int k0, int lim, int tid)
{
    if (!T) {
        const int k = k0 + (tid & 31), row = tid >> 5;
#pragma unroll
        for (int i = 0; i < 16; i++) r.v[i] = k < lim ? W[(size_t)(row + 8 * i) * ld + k] : 0.f;
    } else {
        const int m = tid & 127, kk0 = tid >> 7;
#pragma unroll
        for (int i = 0; i < 16; i++) { const int rr = k0 + kk0 + 2 * i; r.v[i] = rr < lim ? W[rr * HID + m] : 0.f; }
    }
}
template <bool T>
__device__ __forceinline__ void store_w(const WReg &r, float *Wl, int tid)
{
    if (!T) {
        const int col = tid & 31, row = tid >> 5;
#pragma unroll
        for (int i = 0; i < 16; i++) Wl[(row + 8 * i) * FS + col] = r.v[i];
    } else {
        const int m = tid & 127, kk0 = tid >> 7;
#pragma unroll
        for (int i = 0; i < 16; i++) Wl[m * FS + kk0 + 2 * i] = r.v[i];
    }
}
// c = W (T = false) or W^T (T = true) [128 x 128] x H^T: four slices through the two LDS buffers, one barrier a slice.  The caller stored H (unpublished) and
// guarantees that no wave still reads buffer 0; the first barrier inside publishes H.
template <bool T>
__device__ __forceinline__ void gemm_h(Acc &c, const float *__restrict__ W, float *Wl, const float *H, int tid, int wave, int q, int j)
{
    acc_zero(c);
    WReg r;
    load_w<T>(r, W, HID, 0, HID, tid);
#pragma unroll 1
    for (int s = 0; s < 4; s++) {
        float *buf = Wl + (s & 1) * HID * FS;
        store_w<T>(r, buf, tid);
        __syncthreads();
        if (s + 1 < 4) load_w<T>(r, W, HID, 32 * (s + 1), HID, tid);
        mma_slice<4>(c, buf, H + 32 * s, HS, wave, q, j);
    }
}
// bias + ReLU; returns the mask (bit mt 16 + nt 4 + r) of the pre-activations > 0
__device__ __forceinline__ unsigned bias_relu(Acc &c, const float *__restrict__ bias, int wave, int q)
{
    unsigned m = 0;
#pragma unroll
    for (int mt = 0; mt < 2; mt++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const float bb = bias[(2 * wave + mt) * 16 + q * 4 + r];
#pragma unroll
            for (int nt = 0; nt < 4; nt++) {
                const float x = c.v[mt][nt][r] + bb;
                if (x > 0.f) { m |= 1u << (mt * 16 + nt * 4 + r); c.v[mt][nt][r] = x; } else c.v[mt][nt][r] = 0.f;
            }
        }
    return m;
}
__device__ __forceinline__ void apply_mask(Acc &c, unsigned m)
{
#pragma unroll
    for (int mt = 0; mt < 2; mt++)
#pragma unroll
        for (int nt = 0; nt < 4; nt++)
#pragma unroll
            for (int r = 0; r < 4; r++) if (!((m >> (mt * 16 + nt * 4 + r)) & 1u)) c.v[mt][nt][r] = 0.f;
}
// accumulators -> point-major rows of `stride` floats (LDS H or a tape part): four consecutive units per lane, one 16-byte store
__device__ __forceinline__ void store_rows(const Acc &c, float *dst, int stride, int wave, int q, int j)
{
#pragma unroll
    for (int mt = 0; mt < 2; mt++)
#pragma unroll
        for (int nt = 0; nt < 4; nt++)
            *reinterpret_cast<float4 *>(dst + (size_t)(nt * 16 + j) * stride + (2 * wave + mt) * 16 + q * 4) =
                make_float4(c.v[mt][nt][0], c.v[mt][nt][1], c.v[mt][nt][2], c.v[mt][nt][3]);
}

#define MLP_LDS_FLOATS (2 * HID * FS + 64 * HS + 64 * GS + 64 * 3 + 64)

// MODE 0: forward, features gathered in the kernel, predictions written.  MODE 1: gradient pass, a_0 read from the tape, a_1..a_3 and delta_1..delta_4 written to it.
template <int MODE>
__global__ __launch_bounds__(256, 2) void mlp_kernel(const TArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *Wl = lds;                                // 2 x [128][FS] weight slices
    float *H = Wl + 2 * HID * FS;                   // [64][HS] hidden activations / deltas; during layer 0: 2 x [64][FS] feature slices + (MODE 0) the tap table
    float *Xl = H;
    int4 *sTap = reinterpret_cast<int4 *>(H + 2 * 64 * FS);
    float *G = H + 64 * HS;                         // [64][GS] delta_4; (MODE 0, prologue) the projected coordinates
    float *sPt = G + 64 * GS;                       // [64][3]
    int *sIn = reinterpret_cast<int *>(sPt + 64 * 3);

    int b, n0; long row0;
    if (!tile_of_block(a, b, n0, row0)) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, q = lane >> 4, j = lane & 15;
    const int hid = a.heads[blockIdx.y], kout = kout_of(hid);
    const float *__restrict__ P = a.params;

    project_tile(a, b, n0, tid, sPt, sIn, MODE == 0 ? G : nullptr);
    __syncthreads();
    if (MODE == 0) { taps_setup(a, G, sTap, tid); __syncthreads(); }

    // ---- layer 0: K = 612 in 20 slices of 32 (the last holds 4 columns); weights and features double-buffered, one barrier a slice
    Acc c;
    acc_zero(c);
    {
        const float *__restrict__ W0 = P + a.off.w[hid][0];
        const float *__restrict__ A0 = a.tape + (size_t)row0 * KP;
        WReg wr;
        float4 xr[2];
        float xg[8];
        auto load_x = [&](int s) {
            if (MODE == 1) {
                const int col = 32 * s + 4 * (tid & 7);
#pragma unroll
                for (int p = 0; p < 2; p++)
                    xr[p] = col < KP ? *reinterpret_cast<const float4 *>(A0 + (size_t)((tid >> 3) + 32 * p) * KP + col) : make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
#pragma unroll
                for (int i = 0; i < 8; i++) xg[i] = feat_value(a, b, 32 * s + (tid & 31), (tid >> 5) + 8 * i, sTap, sPt);
            }
        };
        auto store_x = [&](float *buf) {
            if (MODE == 1) {
#pragma unroll
                for (int p = 0; p < 2; p++) *reinterpret_cast<float4 *>(buf + ((tid >> 3) + 32 * p) * FS + 4 * (tid & 7)) = xr[p];
            } else {
#pragma unroll
                for (int i = 0; i < 8; i++) buf[((tid >> 5) + 8 * i) * FS + (tid & 31)] = xg[i];
            }
        };
        load_w<false>(wr, W0, KIN, 0, KIN, tid);
        load_x(0);
#pragma unroll 1
        for (int s = 0; s < NSLICE0; s++) {
            float *wb = Wl + (s & 1) * HID * FS, *xb = Xl + (s & 1) * 64 * FS;
            store_w<false>(wr, wb, tid);
            store_x(xb);
            __syncthreads();
            if (s + 1 < NSLICE0) { load_w<false>(wr, W0, KIN, 32 * (s + 1), KIN, tid); load_x(s + 1); }
            mma_slice<4>(c, wb, xb, FS, wave, q, j);
        }
    }
    const unsigned m1 = bias_relu(c, P + a.off.b[hid][0], wave, q);
    __syncthreads();                                // the feature slices (and the tap table) are dead: the region becomes H
    store_rows(c, H, HS, wave, q, j);
    if (MODE == 1) store_rows(c, tape_part(a, hid, 0) + (size_t)row0 * HID, HID, wave, q, j);
    gemm_h<false>(c, P + a.off.w[hid][1], Wl, H, tid, wave, q, j);
    const unsigned m2 = bias_relu(c, P + a.off.b[hid][1], wave, q);
    __syncthreads();
    store_rows(c, H, HS, wave, q, j);
    if (MODE == 1) store_rows(c, tape_part(a, hid, 1) + (size_t)row0 * HID, HID, wave, q, j);
    gemm_h<false>(c, P + a.off.w[hid][2], Wl, H, tid, wave, q, j);
    const unsigned m3 = bias_relu(c, P + a.off.b[hid][2], wave, q);
    __syncthreads();
    store_rows(c, H, HS, wave, q, j);
    if (MODE == 1) store_rows(c, tape_part(a, hid, 2) + (size_t)row0 * HID, HID, wave, q, j);
    __syncthreads();

    // ---- layer 3: wave w owns the 16 points of N-tile w; M = the kout <= 16 outputs (zero rows beyond)
    f32x4 o4 = (f32x4){0.f, 0.f, 0.f, 0.f};
    {
        const float *__restrict__ W3 = P + a.off.w[hid][3];
#pragma unroll
        for (int s = 0; s < 16; s++) {
            const int k = 8 * s + 2 * q;
            const float a0 = j < kout ? W3[j * HID + k] : 0.f, a1 = j < kout ? W3[j * HID + k + 1] : 0.f;
            const float2 bv = *reinterpret_cast<const float2 *>(H + (wave * 16 + j) * HS + k);
            o4 = MFMA16(a0, bv.x, o4); o4 = MFMA16(a1, bv.y, o4);
        }
    }
    const int pt = wave * 16 + j, n = n0 + pt;
    const bool valid = n < a.N, inimg = sIn[pt] != 0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int u = q * 4 + r;
        const bool live = u < kout;
        float val = o4[r] + (live ? P[a.off.b[hid][3] + u] : 0.f);
        if (MODE == 0) {
            if (hid == 0 && !inimg) val = OUT_DIST;                                 // df[~in_img] = 5.0 (chore_triplane.py:155-159)
            if (hid == 4) val = 1.0f / (1.0f + expf(-val));                          // sigmoid on visibility (chore_tri_vis.py:22-27)
            if (valid && live) a.out[hid][((size_t)b * kout + u) * a.N + n] = val;
        } else {
            float gg = (valid && live) ? a.gout[hid][((size_t)b * kout + u) * a.N + n] : 0.f;
            if (hid == 0 && !inimg) gg = 0.f;
            if (hid == 4) { const float s = 1.0f / (1.0f + expf(-val)); gg *= s * (1.0f - s); }
            if (!(valid && live)) gg = 0.f;
            G[pt * GS + u] = gg;
            tape_part(a, hid, 6)[(size_t)(row0 + pt) * 16 + u] = gg;
        }
    }
    if (MODE == 0) return;

    // ---- delta_3 = (W3^T delta_4) . [z3 > 0]: K = 16 (rows >= kout of W3 read as zero), the slice in buffer 1 (buffer 0 is the first one gemm_h refills)
    {
        WReg wr;
        load_w<true>(wr, P + a.off.w[hid][3], HID, 0, kout, tid);
        store_w<true>(wr, Wl + HID * FS, tid);
    }
    __syncthreads();                                // publishes G and the slice; every wave is past its layer-3 reads of H
    acc_zero(c);
    mma_slice<2>(c, Wl + HID * FS, G, GS, wave, q, j);
    apply_mask(c, m3);
    store_rows(c, H, HS, wave, q, j);
    store_rows(c, tape_part(a, hid, 5) + (size_t)row0 * HID, HID, wave, q, j);
    gemm_h<true>(c, P + a.off.w[hid][2], Wl, H, tid, wave, q, j);       // delta_2 = (W2^T delta_3) . [z2 > 0]
    apply_mask(c, m2);
    __syncthreads();
    store_rows(c, H, HS, wave, q, j);
    store_rows(c, tape_part(a, hid, 4) + (size_t)row0 * HID, HID, wave, q, j);
    gemm_h<true>(c, P + a.off.w[hid][1], Wl, H, tid, wave, q, j);       // delta_1 = (W1^T delta_2) . [z1 > 0]
    apply_mask(c, m1);
    store_rows(c, tape_part(a, hid, 3) + (size_t)row0 * HID, HID, wave, q, j);
}

// ---- 3. split-K weight-gradient GEMM: one wave per (output tile, head, chunk) ------------------------------------------------------------------------------
// dW[m][k] = sum_p delta[p][m] a[p][k].  MFMA row i of tile mt is unit m0 + 4 i + mt and column j of tile nt is input k0 + 4 j + nt, so a lane's four A (B)
// values of a step are ONE 16-byte load from the point-major tape row; the K index of a step is the point 4 t + (lane >> 4).
__global__ __launch_bounds__(64) void wgrad_kernel(const TArgs a, float *__restrict__ partials, long P)
{
    const int lane = threadIdx.x, q = lane >> 4, j = lane & 15;
    const int hid = a.heads[blockIdx.y], kout = kout_of(hid), lc = blockIdx.z, g = a.g0 + lc;
    const int valid = min(a.chunk, a.N - (g % a.nc) * a.chunk), steps = ((valid + 63) >> 6) * 16;
    float *__restrict__ out = partials + (size_t)lc * P;
    const long rbase = (long)lc * a.chunk + q;
    int t = blockIdx.x, l, mtile, ntile;
    if (t < 20) { l = 0; mtile = t / 10; ntile = t % 10; }
    else if (t < 28) { l = 1 + ((t - 20) >> 2); mtile = ((t - 20) >> 1) & 1; ntile = (t - 20) & 1; }
    else { l = 3; mtile = 0; ntile = t - 28; }
    const int in = l == 0 ? KIN : HID, sa = l == 0 ? KP : HID, m0 = mtile * 64, k0 = ntile * 64;
    const float *A = (l == 0 ? tape_a0(a) : tape_part(a, hid, l - 1)) + rbase * sa + k0 + 4 * j;
    const bool colok = k0 + 4 * j < sa;
    f32x4 acc[4][4];
    double sb[4] = {0.0, 0.0, 0.0, 0.0};        // bias gradient: this lane's deltas of the chunk, summed in fp64 (tiles with ntile == 0 only)
#pragma unroll
    for (int mt = 0; mt < 4; mt++)
#pragma unroll
        for (int nt = 0; nt < 4; nt++) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (l < 3) {
        const float *D = tape_part(a, hid, 3 + l) + rbase * HID + m0 + 4 * j;
#pragma unroll 4
        for (int s = 0; s < steps; s++) {
            const float4 dv = *reinterpret_cast<const float4 *>(D + (size_t)s * 4 * HID);
            const float4 av = colok ? *reinterpret_cast<const float4 *>(A + (size_t)s * 4 * sa) : make_float4(0.f, 0.f, 0.f, 0.f);
            const float d[4] = {dv.x, dv.y, dv.z, dv.w}, x[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
            for (int mt = 0; mt < 4; mt++)
#pragma unroll
                for (int nt = 0; nt < 4; nt++) acc[mt][nt] = MFMA16(d[mt], x[nt], acc[mt][nt]);
            if (ntile == 0) {
#pragma unroll
                for (int mt = 0; mt < 4; mt++) sb[mt] += (double)d[mt];
            }
        }
        float *ow = out + a.off.w[hid][l], *ob = out + a.off.b[hid][l];
#pragma unroll
        for (int mt = 0; mt < 4; mt++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int m = m0 + 4 * (q * 4 + r) + mt;
#pragma unroll
                for (int nt = 0; nt < 4; nt++) {
                    const int k = k0 + 4 * j + nt;
                    if (k < in) ow[(size_t)m * in + k] = acc[mt][nt][r];
                }
            }
        if (ntile == 0) {       // the four lanes (q) that share j hold the rows 4 s + q: add them in lane order, round once
#pragma unroll
            for (int mt = 0; mt < 4; mt++) {
                sb[mt] += __shfl_xor(sb[mt], 16, 64); sb[mt] += __shfl_xor(sb[mt], 32, 64);
                if (q == 0) ob[m0 + 4 * j + mt] = (float)sb[mt];
            }
        }
    } else {
        const float *D = tape_part(a, hid, 6) + rbase * 16 + j;          // delta_4: MFMA row j is output j
#pragma unroll 4
        for (int s = 0; s < steps; s++) {
            const float dv = D[(size_t)s * 4 * 16];
            const float4 av = *reinterpret_cast<const float4 *>(A + (size_t)s * 4 * HID);
            const float x[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
            for (int nt = 0; nt < 4; nt++) acc[0][nt] = MFMA16(dv, x[nt], acc[0][nt]);
            if (ntile == 0) sb[0] += (double)dv;
        }
        float *ow = out + a.off.w[hid][3], *ob = out + a.off.b[hid][3];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int m = q * 4 + r;
            if (m < kout) {
#pragma unroll
                for (int nt = 0; nt < 4; nt++) ow[(size_t)m * HID + k0 + 4 * j + nt] = acc[0][nt][r];
            }
        }
        if (ntile == 0) {
            sb[0] += __shfl_xor(sb[0], 16, 64); sb[0] += __shfl_xor(sb[0], 32, 64);
            if (q == 0 && j < kout) ob[j] = (float)sb[0];
        }
    }
}

// ---- 4. the chunk partials of a slab, added in fp64 in chunk order onto the running sum ----------------------------------------------------------------------
__global__ __launch_bounds__(256) void finish_kernel(const float *__restrict__ partials, long P, int nchunks, double *__restrict__ run, int first, int last,
                                                     float *__restrict__ dparams, int accumulate, POff off, unsigned live)
{
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    int h = 0;
    while (h < 4 && p >= off.head_end[h]) h++;
    double s = 0.0;
    if ((live >> h) & 1u) {
        if (!first) s = run[p];
        for (int c = 0; c < nchunks; c++) s += (double)partials[(size_t)c * P + p];
    }
    if (!last) { run[p] = s; return; }
    dparams[p] = accumulate ? dparams[p] + (float)s : (float)s;
}

// ---- 5. the gradient to the feature maps ---------------------------------------------------------------------------------------------------------------
// (model/geometry.py:4-14 backward: grid_sample's gradient to its input, align_corners=True, zeros padding.)  Per slab, after wgrad_kernel has been enqueued:
//   a. da0_kernel    per 64-point tile: d_a0[612][64] = sum over the live heads, in the order 0..4, of W_h0^T (611 x 128) . delta_h1 (128 x 64), the transposed-slice
//                    path of the delta propagation (exact fp32 products, fp32 accumulation on the MFMA, K = heads x 128).  d_a0 OVERWRITES a_0 in the tape (wgrad_kernel,
//                    its last reader, is ahead in the stream).  The z_feat columns 256..258 and the pad column read zero weights and hold exact zeros; nobody reads them.
//   b. tapkey_kernel per tile: the taps_setup entry of every (map, point) -> workspace, and one 64-bit key (frame << 42 | base cell << 20 | tape row) per (map, point),
//                    all ones for rows beyond N, points without an in-bounds tap and maps that are not requested.  Tape rows ascend with (frame, point index).
//   c. sort_kernel   one workgroup per map: bitonic sort of the slab's keys in LDS (at most 16384 keys, 128 KB).  The keys of live entries are unique, so the sorted
//                    sequence does not depend on how it was reached: per (frame, cell) the points stand in ascending index.
//   d. scatter_kernel per map, one wave per (frame, texel), lanes across the channels (one tap = one contiguous row of 128 .. 1024 B of d_a0): the lists of the four
//                    cells (y-1,x-1), (y-1,x), (y,x-1), (y,x) are found by binary search (lanes 0..3, one list each) and walked in that order, each in ascending
//                    point index.  Tap weights are the fp32 products of feat_value (in-bounds flags folded in), so the gradient is that of the forward's own linear
//                    map; weight x d_a0 is an exact fp64 product, summed in fp64 and rounded to fp32 once per slab: FP64 BY CHOICE -- a texel may collect every point
//                    of a slab, and the sequential fp32 chain of that length is the case that measured 4.4 .. 4.8 e32 for the bias gradients above.
//                    The frame's first slab stores (accumulate_maps == 0: zeros where no tap lands, so every element is written once), later slabs and
//                    accumulate_maps != 0 add, and then only texels that a tap lands on are touched.  Across slabs the order is slab order = (frame, chunk) order.
// No floating-point atomics, no atomics at all; one writer per element per launch.
struct GArgs {
    float *dmaps[8];
    unsigned long long *keys;   // [8][kcap]
    int4 *taps;                 // [8][rows]
    int kcap, ksort;            // key stride (a power of two >= rows); power of two >= the rows of this slab
    int nrows, nchunks;         // rows and chunks of this slab
    int accumulate;
};

#define KEY_NONE (~0ull)
#define DA0_LDS_FLOATS (2 * HID * FS + 64 * HS)

__device__ __forceinline__ int map_first_channel(int mi) { return mi == 0 ? 0 : (mi == 1 ? 259 : (mi < 5 ? 323 + 32 * (mi - 2) : 419 + 64 * (mi - 5))); }

// a 128 x 32 slice of W0^T on its way to LDS: Wl[m][kk] = W0[(k0 + kk) 611 + c0 + m]; the z_feat and pad columns read as 0
__device__ __forceinline__ void load_w0t(WReg &r, const float *__restrict__ W0, int c0, int k0, int tid)
{
    const int m = tid & 127, kk0 = tid >> 7, col = c0 + m;
    const bool ok = col < KIN && !(col >= 256 && col < 259);
#pragma unroll
    for (int i = 0; i < 16; i++) r.v[i] = ok ? W0[(size_t)(k0 + kk0 + 2 * i) * KIN + col] : 0.f;
}

__global__ __launch_bounds__(256, 2) void da0_kernel(const TArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *Wl = lds;                                // 2 x [128][FS] slices of W0^T
    float *H = Wl + 2 * HID * FS;                   // [64][HS] delta_1 of one head
    int b, n0; long row0;
    if (!tile_of_block(a, b, n0, row0)) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, q = lane >> 4, j = lane & 15;
    float *dst = a.tape + (size_t)row0 * KP;
#pragma unroll 1
    for (int mb = 0; mb < 5; mb++) {                // 128 feature columns a pass
        Acc c;
        acc_zero(c);
#pragma unroll 1
        for (int hs = 0; hs < a.nheads; hs++) {
            const int hid = a.heads[hs];
            const float *__restrict__ W0 = a.params + a.off.w[hid][0];
            const float *__restrict__ D = tape_part(a, hid, 3) + (size_t)row0 * HID;
            __syncthreads();                        // every wave is past its reads of H and of both slice buffers
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int e = tid + 256 * i, row = e >> 5, c4 = (e & 31) * 4;
                *reinterpret_cast<float4 *>(H + row * HS + c4) = *reinterpret_cast<const float4 *>(D + (size_t)row * HID + c4);
            }
            WReg r;
            load_w0t(r, W0, 128 * mb, 0, tid);
#pragma unroll 1
            for (int s = 0; s < 4; s++) {
                float *buf = Wl + (s & 1) * HID * FS;
                store_w<true>(r, buf, tid);
                __syncthreads();
                if (s + 1 < 4) load_w0t(r, W0, 128 * mb, 32 * (s + 1), tid);
                mma_slice<4>(c, buf, H + 32 * s, HS, wave, q, j);
            }
        }
#pragma unroll
        for (int mt = 0; mt < 2; mt++) {
            const int col = 128 * mb + (2 * wave + mt) * 16 + q * 4;
            if (col < KP) {
#pragma unroll
                for (int nt = 0; nt < 4; nt++)
                    *reinterpret_cast<float4 *>(dst + (size_t)(nt * 16 + j) * KP + col) = make_float4(c.v[mt][nt][0], c.v[mt][nt][1], c.v[mt][nt][2], c.v[mt][nt][3]);
            }
        }
    }
}

__global__ __launch_bounds__(256) void tapkey_kernel(const TArgs a, const GArgs g)
{
    __shared__ float sPt[64 * 3];
    __shared__ int sIn[64];
    __shared__ float sUV[4 * 64 * 2];
    __shared__ int4 sTap[8 * 64];
    int b, n0; long row0;
    const int tid = threadIdx.x;
    if (!tile_of_block(a, b, n0, row0)) {           // a tile wholly beyond N: its tape rows were never written, its keys say so
        for (int e = tid; e < 512; e += 256) g.keys[(size_t)(e >> 6) * g.kcap + row0 + (e & 63)] = KEY_NONE;
        return;
    }
    project_tile(a, b, n0, tid, sPt, sIn, sUV);
    __syncthreads();
    taps_setup(a, sUV, sTap, tid);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int e = tid + 256 * i, mi = e >> 6, pt = e & 63;
        const int4 t = sTap[e];
        const long row = row0 + pt;
        const bool live = n0 + pt < a.N && (t.y >> 2) != 0 && g.dmaps[mi] != nullptr;
        const unsigned long long cell = (unsigned long long)(t.x / map_channels(mi));
        g.keys[(size_t)mi * g.kcap + row] = live ? ((unsigned long long)b << 42) | (cell << 20) | (unsigned long long)row : KEY_NONE;
        g.taps[(size_t)mi * a.rows + row] = t;
    }
}

__global__ __launch_bounds__(1024) void sort_kernel(const GArgs g)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long skey[];
    const int mi = blockIdx.x, tid = threadIdx.x, n = g.ksort;
    if (!g.dmaps[mi]) return;
    unsigned long long *K = g.keys + (size_t)mi * g.kcap;
    for (int i = tid; i < n; i += 1024) skey[i] = i < g.nrows ? K[i] : KEY_NONE;
    for (int k = 2; k <= n; k <<= 1)
        for (int jj = k >> 1; jj > 0; jj >>= 1) {
            __syncthreads();
            for (int t = tid; t < (n >> 1); t += 1024) {
                const int lo = ((t & ~(jj - 1)) << 1) | (t & (jj - 1)), hi = lo | jj;
                const unsigned long long x = skey[lo], y = skey[hi];
                if ((x > y) == ((lo & k) == 0)) { skey[lo] = y; skey[hi] = x; }
            }
        }
    __syncthreads();
    for (int i = tid; i < n; i += 1024) K[i] = skey[i];
}

__global__ __launch_bounds__(256) void scatter_kernel(const TArgs a, const GArgs g, int mi)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int R = a.res[mi], C = map_channels(mi), n = g.ksort;
    const long texel = (long)blockIdx.x * 4 + wave;
    if (texel >= (long)R * R) return;
    const int y = (int)(texel / R), x = (int)(texel % R);
    const int f0 = a.g0 / a.nc, b = f0 + blockIdx.y;
    const long first = (long)b * a.nc;              // the frame's first chunk lies in exactly one slab: that one stores
    const bool store = !g.accumulate && first >= a.g0 && first < (long)a.g0 + g.nchunks;
    const unsigned long long *__restrict__ K = g.keys + (size_t)mi * g.kcap;
    const int4 *__restrict__ T = g.taps + (size_t)mi * a.rows;
    const float *__restrict__ dA = a.tape + map_first_channel(mi);

    // lanes 0..3: the start of the list of cell (y - 1, x - 1), (y - 1, x), (y, x - 1), (y, x)
    const int l4 = lane & 3, cy = y - (l4 < 2 ? 1 : 0), cx = x - ((l4 & 1) == 0 ? 1 : 0);
    const unsigned long long prefix = ((unsigned long long)b << 22) | (unsigned long long)(unsigned)(max(cy, 0) * R + max(cx, 0));
    int pos = 0;
    for (int step = n >> 1; step > 0; step >>= 1) if ((K[pos + step - 1] >> 20) < prefix) pos += step;
    if ((K[pos] >> 20) < prefix) pos++;
    if (cy < 0 || cx < 0) pos = n;

    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    bool touched = false;
#pragma unroll 1
    for (int l = 0; l < 4; l++) {
        const int ly = y - (l < 2 ? 1 : 0), lx = x - ((l & 1) == 0 ? 1 : 0);
        const unsigned long long pf = ((unsigned long long)b << 22) | (unsigned long long)(unsigned)(max(ly, 0) * R + max(lx, 0));
#pragma unroll 1
        for (int i = __shfl(pos, l, 64); i < n; i++) {
            const unsigned long long key = K[i];
            if ((key >> 20) != pf) break;
            const long row = (long)(key & 0xFFFFFull);
            const int4 t = T[row];
            const int dxf = t.y & 1, dyf = (t.y >> 1) & 1, ib = t.y >> 2;
            const float wx1 = __int_as_float(t.z), wy1 = __int_as_float(t.w), wx0 = 1.0f - wx1, wy0 = 1.0f - wy1;
#pragma unroll
            for (int tap = 0; tap < 4; tap++) {
                const int tx = tap & 1, ty = tap >> 1;
                if (!((ib >> tap) & 1) || ly + ty * dyf != y || lx + tx * dxf != x) continue;
                const double w = (double)((tx ? wx1 : wx0) * (ty ? wy1 : wy0));
                const float *__restrict__ src = dA + (size_t)row * KP;
#pragma unroll
                for (int s = 0; s < 4; s++) { const int c = lane + 64 * s; if (c < C) acc[s] += w * (double)src[c]; }
                touched = true;
            }
        }
    }
    if (!store && !touched) return;
    float *out = g.dmaps[mi] + (((size_t)b * R + y) * R + x) * C;
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const int c = lane + 64 * s;
        if (c < C) out[c] = store ? (float)acc[s] : out[c] + (float)acc[s];
    }
}

static int fill_common(TArgs &a, const float *params, const float *cam, const vt_maps *maps, const float *pts, const float *cc, const float *bc, int B, int N,
                       const char *who)
{
    VT_REQUIRE(params && cam && maps && pts && cc && bc, "%s: null argument", who);
    VT_REQUIRE(B > 0 && B <= 65535 && N > 0, "%s: B = %d (1 .. 65535), N = %d", who, B, N);
    memset(&a, 0, sizeof(a));
    for (int i = 0; i < 8; i++) {
        VT_REQUIRE(maps->maps[i] && maps->res[i] >= 2 && maps->res[i] <= 2048, "%s: map %d missing or its resolution outside 2 .. 2048", who, i);
        a.maps[i] = maps->maps[i]; a.res[i] = maps->res[i];
    }
    a.params = params; a.off = make_off();
    a.pts = pts; a.crop_center = cc; a.body_center = bc; a.B = B; a.N = N;
    a.fx = cam[0]; a.fy = cam[1]; a.cx = cam[2]; a.cy = cam[3]; a.crop = cam[4];
    return VT_OK;
}

static int chunk_of(int chunk_points)
{
    if (chunk_points == 0) return DEFAULT_CHUNK;
    return (chunk_points > 0 && chunk_points <= MAX_CHUNK && chunk_points % 64 == 0) ? chunk_points : -1;
}
struct Plan { int chunk, nc, slab; long total, rows, run_bytes, tape_bytes, part_bytes; };
static bool make_plan(Plan &p, int B, int N, int chunk_points)
{
    p.chunk = chunk_of(chunk_points);
    if (B <= 0 || B > 65535 || N <= 0 || p.chunk < 0) return false;
    p.nc = (int)(((long)N + p.chunk - 1) / p.chunk);
    p.total = (long)B * p.nc;
    if (p.total > 0x7fffffffL) return false;
    int s = SLAB_POINTS / p.chunk; s = s < 1 ? 1 : (s > SLAB_MAX_CHUNKS ? SLAB_MAX_CHUNKS : s);
    p.slab = (int)(p.total < s ? p.total : s);
    p.rows = (long)p.slab * p.chunk;
    const long P = param_floats();
    p.run_bytes = ((P * 8 + 15) / 16) * 16;
    p.tape_bytes = p.rows * TAPE_POINT * 4;
    p.part_bytes = (long)p.slab * P * 4;
    return true;
}

}  // namespace dect

extern "C" {

long vt_decoder_param_floats(void) { return dect::param_floats(); }
long vt_decoder_param_offset(int head, int layer, int is_bias) { return dect::param_offset(head, layer, is_bias); }

int vt_decoder_train_forward(const float *params, const float *cam, const vt_maps *maps, const float *pts, const float *crop_center, const float *body_center,
                             int B, int N, float *df, float *pca, float *parts, float *centers, float *vis, void *stream)
{
    using namespace dect;
    TArgs a; int rc = fill_common(a, params, cam, maps, pts, crop_center, body_center, B, N, "vt_decoder_train_forward"); if (rc) return rc;
    float *outs[5] = {df, pca, parts, centers, vis};
    for (int i = 0; i < 5; i++) if (outs[i]) { a.out[i] = outs[i]; a.heads[a.nheads++] = i; }
    VT_REQUIRE(a.nheads > 0, "vt_decoder_train_forward: no output requested");
    const long tiles = ((long)N + 63) / 64;
    VT_REQUIRE(tiles * B <= 0x7fffffffL && tiles * 64 <= 0x7fffffffL, "vt_decoder_train_forward: B x N too large");
    a.chunk = (int)(tiles * 64); a.nc = 1; a.g0 = 0;        // one "chunk" per frame
    const size_t lds = sizeof(float) * MLP_LDS_FLOATS;
    VT_LDS_LIMIT((mlp_kernel<0>), lds);
    hipLaunchKernelGGL((mlp_kernel<0>), dim3((unsigned)(tiles * B), a.nheads), dim3(256), lds, vt_stream(stream), a);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

static long pow2_ceil(long n) { long p = 2; while (p < n) p <<= 1; return p; }
static long align16(long n) { return (n + 15) & ~15L; }
static long grads_ws_bytes(int B, int N, int chunk_points, int want_maps, dect::Plan &p)
{
    if (!dect::make_plan(p, B, N, chunk_points)) return -1;
    long n = p.run_bytes + p.tape_bytes + p.part_bytes;
    if (want_maps) n = align16(n) + 8 * pow2_ceil(p.rows) * 8 + 8 * p.rows * 16;      // the sort keys and the tap entries of a slab, per map
    return n;
}

long vt_decoder_weight_grads_ws_bytes(int B, int N, int chunk_points) { dect::Plan p; return grads_ws_bytes(B, N, chunk_points, 0, p); }
long vt_decoder_grads_ws_bytes(int B, int N, int chunk_points, int want_maps) { dect::Plan p; return grads_ws_bytes(B, N, chunk_points, want_maps, p); }

static int decoder_grads(const char *who, const float *params, const float *cam, const vt_maps *maps, const float *pts, const float *crop_center,
                         const float *body_center, int B, int N, const float *const gs[5], float *dparams, int accumulate, const vt_maps *d_maps,
                         int accumulate_maps, int chunk_points, void *workspace, void *stream)
{
    using namespace dect;
    Plan p;
    VT_REQUIRE(make_plan(p, B, N, chunk_points), "%s: B = %d (1 .. 65535), N = %d, chunk_points = %d (0, or a multiple of 64 up to %d)", who, B, N,
               chunk_points, MAX_CHUNK);
    TArgs a; int rc = fill_common(a, params, cam, maps, pts, crop_center, body_center, B, N, who); if (rc) return rc;
    GArgs g;
    memset(&g, 0, sizeof(g));
    bool want_maps = false;
    if (d_maps)
        for (int i = 0; i < 8; i++) {
            VT_REQUIRE(d_maps->res[i] == maps->res[i], "%s: d_maps->res[%d] = %d, the map's is %d", who, i, d_maps->res[i], maps->res[i]);
            g.dmaps[i] = const_cast<float *>(d_maps->maps[i]);      /* vt_maps serves inputs elsewhere, hence its const */
            want_maps = want_maps || g.dmaps[i];
        }
    VT_REQUIRE(dparams || want_maps, "%s: neither dparams nor a map gradient requested", who);
    VT_REQUIRE(workspace && (reinterpret_cast<size_t>(workspace) & 15) == 0, "%s: workspace null or not 16-byte aligned", who);
    hipStream_t st = vt_stream(stream);
    unsigned live = 0;
    for (int i = 0; i < 5; i++) if (gs[i]) { a.gout[i] = gs[i]; a.heads[a.nheads++] = i; live |= 1u << i; }
    const long P = param_floats();
    char *ws = static_cast<char *>(workspace);
    double *run = reinterpret_cast<double *>(ws);
    a.tape = reinterpret_cast<float *>(ws + p.run_bytes); a.rows = p.rows;
    float *partials = reinterpret_cast<float *>(ws + p.run_bytes + p.tape_bytes);
    g.kcap = (int)pow2_ceil(p.rows);
    g.keys = reinterpret_cast<unsigned long long *>(ws + align16(p.run_bytes + p.tape_bytes + p.part_bytes));
    g.taps = reinterpret_cast<int4 *>(g.keys + 8L * g.kcap);
    g.accumulate = accumulate_maps;
    a.chunk = p.chunk; a.nc = p.nc;
    const unsigned fin_blocks = (unsigned)((P + 255) / 256);
    if (a.nheads == 0) {        // every upstream gradient NULL: the gradients are exactly zero
        if (dparams) {
            hipLaunchKernelGGL(finish_kernel, dim3(fin_blocks), dim3(256), 0, st, partials, P, 0, run, 1, 1, dparams, accumulate, a.off, 0u);
            VT_LAUNCH_CHECK();
        }
        for (int i = 0; i < 8 && !accumulate_maps; i++)
            if (g.dmaps[i]) {
                const hipError_t e = hipMemsetAsync(g.dmaps[i], 0, sizeof(float) * (size_t)B * a.res[i] * a.res[i] * (i == 0 ? 256 : (i == 1 ? 64 : (i < 5 ? 32 : 64))), st);
                if (e != hipSuccess) VT_FAIL(VT_ERR_HIP, "%s: memset -> %s", who, hipGetErrorString(e));
            }
        return VT_OK;
    }
    const size_t lds = sizeof(float) * MLP_LDS_FLOATS, lds_da0 = sizeof(float) * DA0_LDS_FLOATS;
    VT_LDS_LIMIT((mlp_kernel<1>), lds);
    if (want_maps) {
        VT_LDS_LIMIT(da0_kernel, lds_da0);
        VT_LDS_LIMIT(sort_kernel, sizeof(unsigned long long) * (size_t)MAX_CHUNK);      // the largest slab there is: rows <= max(SLAB_POINTS, MAX_CHUNK)
    }
    for (long g0 = 0; g0 < p.total; g0 += p.slab) {
        const int n = (int)(p.total - g0 < p.slab ? p.total - g0 : p.slab);
        a.g0 = (int)g0;
        const unsigned tiles = (unsigned)n * (unsigned)(p.chunk / 64);
        hipLaunchKernelGGL(feat_kernel, dim3(tiles), dim3(256), 0, st, a);
        VT_LAUNCH_CHECK();
        hipLaunchKernelGGL((mlp_kernel<1>), dim3(tiles, a.nheads), dim3(256), lds, st, a);
        VT_LAUNCH_CHECK();
        if (dparams) {
            hipLaunchKernelGGL(wgrad_kernel, dim3(WG_TILES, a.nheads, n), dim3(64), 0, st, a, partials, P);
            VT_LAUNCH_CHECK();
            hipLaunchKernelGGL(finish_kernel, dim3(fin_blocks), dim3(256), 0, st, partials, P, n, run, g0 == 0 ? 1 : 0, g0 + n >= p.total ? 1 : 0, dparams, accumulate,
                               a.off, live);
            VT_LAUNCH_CHECK();
        }
        if (!want_maps) continue;
        g.nrows = n * p.chunk; g.nchunks = n; g.ksort = (int)pow2_ceil(g.nrows);
        hipLaunchKernelGGL(da0_kernel, dim3(tiles), dim3(256), lds_da0, st, a);       // overwrites a_0: wgrad_kernel is ahead in the stream
        VT_LAUNCH_CHECK();
        hipLaunchKernelGGL(tapkey_kernel, dim3(tiles), dim3(256), 0, st, a, g);
        VT_LAUNCH_CHECK();
        hipLaunchKernelGGL(sort_kernel, dim3(8), dim3(1024), sizeof(unsigned long long) * (size_t)g.ksort, st, g);
        VT_LAUNCH_CHECK();
        const unsigned frames = (unsigned)((g0 + n - 1) / p.nc - g0 / p.nc + 1);
        for (int mi = 0; mi < 8; mi++) {
            if (!g.dmaps[mi]) continue;
            const long texels = (long)a.res[mi] * a.res[mi];
            hipLaunchKernelGGL(scatter_kernel, dim3((unsigned)((texels + 3) / 4), frames), dim3(256), 0, st, a, g, mi);
            VT_LAUNCH_CHECK();
        }
    }
    return VT_OK;
}

int vt_decoder_weight_grads(const float *params, const float *cam, const vt_maps *maps, const float *pts, const float *crop_center, const float *body_center,
                            int B, int N, const float *d_df, const float *d_pca, const float *d_parts, const float *d_centers, const float *d_vis,
                            float *dparams, int accumulate, int chunk_points, void *workspace, void *stream)
{
    VT_REQUIRE(dparams, "vt_decoder_weight_grads: dparams null");
    const float *gs[5] = {d_df, d_pca, d_parts, d_centers, d_vis};
    return decoder_grads("vt_decoder_weight_grads", params, cam, maps, pts, crop_center, body_center, B, N, gs, dparams, accumulate, nullptr, 0, chunk_points, workspace,
                         stream);
}

int vt_decoder_grads(const float *params, const float *cam, const vt_maps *maps, const float *pts, const float *crop_center, const float *body_center,
                     int B, int N, const float *d_df, const float *d_pca, const float *d_parts, const float *d_centers, const float *d_vis,
                     float *dparams, int accumulate, const vt_maps *d_maps, int accumulate_maps, int chunk_points, void *workspace, void *stream)
{
    const float *gs[5] = {d_df, d_pca, d_parts, d_centers, d_vis};
    return decoder_grads("vt_decoder_grads", params, cam, maps, pts, crop_center, body_center, B, N, gs, dparams, accumulate, d_maps, accumulate_maps, chunk_points,
                         workspace, stream);
}

}  // extern "C"
