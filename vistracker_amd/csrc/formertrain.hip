// formertrain.hip -- one pre-norm transformer encoder layer of HVOP-Net, forward with a tape and hand-written backward (former_deci.py:77-93), and the
// optional final LayerNorm of a TransformerV2 (former_deci.py:64-65).
//
//   y1 = x + drop1(out_proj(attn(LN1(x) + pos, LN1(x) + pos, LN1(x))))          y = y1 + drop2(W2 drop(act(W1 LN2(y1) + b1)) + b2)
//
// LAUNCHES.  Rows are the M = B T frames; a row tile is 16 rows (one MFMA tile), so T needs no padding outside the attention kernels.
//   forward   k_ln_qkv    per row tile       LN1 (fp64 statistics), q | k | v = in_proj of (LN1 + pos | LN1 + pos | LN1)
//             k_attn_fwd  per (clip, head, 16 queries)   score strip 16 x T in LDS, mask, softmax, dropout, P V
//             k_out_ff    per row tile       out_proj, dropout1, residual, LN2, linear1, activation, dropout, linear2, dropout2, residual
//   backward  k_ff_bwd    per row tile       back through the feed-forward branch, LN2, dropout1 and out_proj: d_y1 and d_O
//             k_attn_bwd  per (clip, head, 16 queries), then per (clip, head, 16 keys): d_q and the softmax row sums from a query strip, then d_k and d_v from
//                         the transposed (key) strip
//             k_qkv_bwd   per row tile       d_LN1 = d_qkv W_in, LN1 backward, d_x
//             k_wgrad, k_colsum, k_reduce    every weight / bias / norm gradient: per-chunk partials, then one fp64 sum in chunk order
//   10 launches for a layer's forward + backward; k_wgrad / k_colsum / k_reduce take all their problems in one launch each.
//
// TAPE (vt_former_layer_tape_floats): {mean, rstd} of LN1 and of LN2 per row as fp64 | q|k|v (M, 3D) | O = P V (M, D) | log-sum-exp of every score row (B, H, T) |
//   y1, the mid residual (M, D) | h, the feed-forward pre-activation (M, F).  SAVED: what a GEMM would have to be run again for, and the row statistics.
//   RECOMPUTED in the backward: the normalised rows of both norms (from x / y1 and the statistics), the attention probabilities (exp(s - lse): T x T per head is
//   the one tensor too large to keep, 66 MB a layer at B = 128), the activation and every dropout mask (from the hash).
//
// ARITHMETIC.  Every GEMM product is an exact fp32 product on v_mfma_f32_16x16x4_f32 with fp32 accumulation in a fixed order; LayerNorm statistics and the sums of
// its backward are fp64; a gradient summed over the M rows (weights, biases, norm parameters) is split into chunks of 512 rows whose partials are added in fp64 in
// chunk order and rounded once.  No atomics: every element has one writer, the same inputs give the same bits, and since the backward is linear in d_y with no
// constant added anywhere a power-of-two scale of d_y scales every result bit for bit.  No row of y or d_x reads another clip's data when p = 0 (a row tile may
// hold rows of two clips, but MFMA rows are independent).
#include "common.h"
#include "dropout_hash.h"

namespace formt {

typedef float f32x4 __attribute__((ext_vector_type(4)));
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

constexpr int NTHR = 256, NWAVE = 4, RT = 16;   // a workgroup: 4 waves, one 16-row tile; thread t owns row t >> 4, columns (t & 15) + 16 n of it
constexpr int SLD = 196;                         // row stride of a score strip: T <= 192 keys + 4 (the strip is zero from T to the next multiple of 16)
constexpr int CHUNK = 512;                       // rows per partial of a sum over the M rows
constexpr int MAXT = 192, MAXD = 160, MAXF = 256;

struct LayerP { const float *wi, *bi, *wo, *bo, *w1, *b1, *w2, *b2, *g1, *be1, *g2, *be2; };
struct Drop { unsigned thr; float inv; unsigned long long seed; };   // thr == 0: p = 0, no hashing

__device__ __forceinline__ float drop_mul(const Drop &d, unsigned site, unsigned long long idx, float v)
{
    if (d.thr == 0u) return v;
    return vt_dropout_hash(d.seed, site, idx) >= d.thr ? v * d.inv : 0.f;
}

__device__ __forceinline__ float act_f(int act, float h)
{
    if (act == 0) return h > 0.f ? h : 0.f;
    if (act == 1) return 0.5f * h * (1.f + erff(h * 0.70710678118654752f));
    return h > 0.f ? h : 0.01f * h;
}
__device__ __forceinline__ float act_d(int act, float h)
{
    if (act == 0) return h > 0.f ? 1.f : 0.f;
    if (act == 1) return 0.5f * (1.f + erff(h * 0.70710678118654752f)) + h * 0.39894228040143268f * expf(-0.5f * h * h);
    return h > 0.f ? 1.f : 0.01f;
}

__device__ __forceinline__ double sum16(double v)
{
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float sum16f(float v)
{
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float max16f(float v)
{
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// C (16 x N) = A (16 x K in LDS, row stride lda) B (K x N in global memory, B(k, n) = Bp[k sk + n sn]); the waves take the column tiles round robin;
// epi(row, col, value) for each of the lane's four results.  K % 4 == 0, N % 16 == 0.
template <class Epi>
__device__ __forceinline__ void tile_gemm(const float *As, int lda, int K, const float *__restrict__ Bp, long sk, long sn, int N, Epi epi)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, q = lane >> 4;
    for (int ct = wave; ct < N / 16; ct += NWAVE) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const float *bp = Bp + (long)(ct * 16 + j) * sn + (long)q * sk;
        const float *ap = As + j * lda + q;
        for (int k = 0; k < K; k += 4) acc = MFMA16(ap[k], bp[(long)k * sk], acc);
#pragma unroll
        for (int i = 0; i < 4; i++) epi(4 * q + i, ct * 16 + j, acc[i]);
    }
}

// the statistics of the thread's row of a 16-row tile in LDS (biased variance, eps 1e-5), fp64
__device__ __forceinline__ void ln_stats(const float *Xs, int ld, int D, double &mean, double &rstd)
{
    const int row = threadIdx.x >> 4, sub = threadIdx.x & 15;
    double s = 0.0;
    for (int c = sub; c < D; c += 16) s += (double)Xs[row * ld + c];
    mean = sum16(s) / (double)D;
    double v = 0.0;
    for (int c = sub; c < D; c += 16) { const double d = (double)Xs[row * ld + c] - mean; v += d * d; }
    rstd = 1.0 / sqrt(sum16(v) / (double)D + 1e-5);
}

// LayerNorm backward of the thread's row: G (LDS) the gradient to the norm's output, Xs (LDS) the norm's input; emit(c, xhat, g, dx) for the thread's columns with
// dx = rstd (gamma g - mean_c(gamma g) - xhat mean_c(gamma g xhat)), sums and the formula in fp64
template <class Emit>
__device__ __forceinline__ void ln_bwd_row(const float *G, const float *Xs, int ld, int D, double mean, double rstd, const float *__restrict__ gamma, Emit emit)
{
    const int row = threadIdx.x >> 4, sub = threadIdx.x & 15;
    double s1 = 0.0, s2 = 0.0;
    for (int c = sub; c < D; c += 16) {
        const double xh = ((double)Xs[row * ld + c] - mean) * rstd, gz = (double)gamma[c] * (double)G[row * ld + c];
        s1 += gz; s2 += gz * xh;
    }
    s1 = sum16(s1) / (double)D; s2 = sum16(s2) / (double)D;
    for (int c = sub; c < D; c += 16) {
        const float g = G[row * ld + c];
        const double xh = ((double)Xs[row * ld + c] - mean) * rstd, gz = (double)gamma[c] * (double)g;
        emit(c, xh, g, (float)(rstd * (gz - s1 - xh * s2)));
    }
}

// ---- forward ------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NTHR) void k_ln_qkv(const float *__restrict__ x, const float *__restrict__ pos, LayerP p, int M, int T, int D,
                                                 double *__restrict__ stats1, float *__restrict__ qkv)
{
    extern __shared__ float lds[];
    const int ld = D + 4, r0 = blockIdx.x * RT, row = threadIdx.x >> 4, sub = threadIdx.x & 15, gr = r0 + row;
    float *XN = lds, *XP = lds + RT * ld;
    for (int c = sub; c < D; c += 16) XN[row * ld + c] = gr < M ? x[(long)gr * D + c] : 0.f;
    double mean, rstd;
    ln_stats(XN, ld, D, mean, rstd);                 // a thread reads and rewrites only its own columns; the sums go through the shuffles
    const int t = gr < M ? gr % T : 0;
    for (int c = sub; c < D; c += 16) {
        const float xn = (float)(((double)XN[row * ld + c] - mean) * rstd * (double)p.g1[c] + (double)p.be1[c]);
        XN[row * ld + c] = xn; XP[row * ld + c] = xn + pos[t * D + c];
    }
    if (stats1 != nullptr && sub == 0 && gr < M) { stats1[2 * (long)gr] = mean; stats1[2 * (long)gr + 1] = rstd; }
    __syncthreads();
    const int D3 = 3 * D;
    tile_gemm(XP, ld, D, p.wi, 1, D, 2 * D, [&](int r, int c, float v) { if (r0 + r < M) qkv[(long)(r0 + r) * D3 + c] = v + p.bi[c]; });
    tile_gemm(XN, ld, D, p.wi + 2 * D * D, 1, D, D, [&](int r, int c, float v) { if (r0 + r < M) qkv[(long)(r0 + r) * D3 + 2 * D + c] = v + p.bi[2 * D + c]; });
}

// strip (16 x W, W = 16 ceil(T / 16)) of X[r0 + r] . Y[c] over the hd columns of a head; rows / columns outside the clip read as zero
__device__ __forceinline__ void score_strip(float *S, const float *__restrict__ X, int sx, const float *__restrict__ Y, int sy, int r0, int T, int hd)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, q = lane >> 4, nkt = (T + 15) / 16;
    const int xi = r0 + j;
    const bool xv = xi < T;
    const float *xp = X + (long)(xv ? xi : 0) * sx + q;
    for (int kt = wave; kt < nkt; kt += NWAVE) {
        const int yi = kt * 16 + j;
        const bool yv = yi < T;
        const float *yp = Y + (long)(yv ? yi : 0) * sy + q;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < hd; k += 4) acc = MFMA16(xv ? xp[k] : 0.f, yv ? yp[k] : 0.f, acc);
#pragma unroll
        for (int i = 0; i < 4; i++) S[(4 * q + i) * SLD + kt * 16 + j] = acc[i];
    }
}

// out rows r0 .. r0 + 15 (< T), hd columns at dst (row stride sd) = S (16 x W strip, zero outside the clip) Z (T x hd, row stride sz)
__device__ __forceinline__ void strip_times(const float *S, const float *__restrict__ Z, int sz, float *__restrict__ dst, int sd, int r0, int T, int hd)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, q = lane >> 4, W = ((T + 15) / 16) * 16;
    for (int ct = wave; ct < hd / 16; ct += NWAVE) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < W; k += 4) {
            const int key = k + q;
            acc = MFMA16(S[j * SLD + key], key < T ? Z[(long)key * sz + ct * 16 + j] : 0.f, acc);
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (r0 + 4 * q + i < T) dst[(long)(r0 + 4 * q + i) * sd + ct * 16 + j] = acc[i];
    }
}

__global__ __launch_bounds__(NTHR) void k_attn_fwd(const float *__restrict__ qkv, const unsigned char *__restrict__ kpm, int T, int D, int H, float scale, Drop dr,
                                                   float *__restrict__ O, float *__restrict__ lse)
{
    __shared__ float S[RT * SLD];
    const int r0 = blockIdx.x * RT, h = blockIdx.y, b = blockIdx.z, hd = D / H, D3 = 3 * D, W = ((T + 15) / 16) * 16;
    const float *Q = qkv + (long)b * T * D3 + h * hd, *K = Q + D, *V = Q + 2 * D;
    score_strip(S, Q, D3, K, D3, r0, T, hd);
    __syncthreads();
    const int row = threadIdx.x >> 4, sub = threadIdx.x & 15, qi = r0 + row;
    float m = -INFINITY;
    for (int c = sub; c < T; c += 16) {
        const float s = (kpm != nullptr && kpm[(long)b * T + c]) ? -INFINITY : S[row * SLD + c] * scale;
        S[row * SLD + c] = s; m = fmaxf(m, s);
    }
    m = max16f(m);
    float sum = 0.f;
    for (int c = sub; c < T; c += 16) { const float e = expf(S[row * SLD + c] - m); S[row * SLD + c] = e; sum += e; }
    sum = sum16f(sum);
    const unsigned long long base = ((unsigned long long)(b * H + h) * T + (qi < T ? qi : 0)) * T;
    for (int c = sub; c < T; c += 16) S[row * SLD + c] = drop_mul(dr, VT_DROP_SITE_ATTN, base + c, S[row * SLD + c] / sum);
    for (int c = T + sub; c < W; c += 16) S[row * SLD + c] = 0.f;
    if (lse != nullptr && sub == 0 && qi < T) lse[(long)(b * H + h) * T + qi] = m + logf(sum);
    __syncthreads();
    strip_times(S, V, D3, O + (long)b * T * D + h * hd, D, r0, T, hd);
}

__global__ __launch_bounds__(NTHR) void k_out_ff(const float *__restrict__ x, const float *__restrict__ O, LayerP p, int M, int D, int F, int act, Drop dr,
                                                 float *__restrict__ y1t, double *__restrict__ stats2, float *__restrict__ ht, float *__restrict__ y)
{
    extern __shared__ float lds[];
    const int ld = D + 4, ldf = F + 4, r0 = blockIdx.x * RT, row = threadIdx.x >> 4, sub = threadIdx.x & 15, gr = r0 + row;
    float *A = lds, *Y1 = lds + RT * ld, *Hs = lds + 2 * RT * ld;
    for (int c = sub; c < D; c += 16) A[row * ld + c] = gr < M ? O[(long)gr * D + c] : 0.f;
    __syncthreads();
    tile_gemm(A, ld, D, p.wo, 1, D, D, [&](int r, int c, float v) {
        const int g = r0 + r;
        Y1[r * ld + c] = (g < M ? x[(long)g * D + c] : 0.f) + drop_mul(dr, VT_DROP_SITE_1, (unsigned long long)g * D + c, v + p.bo[c]);
    });
    __syncthreads();
    double mean, rstd;
    ln_stats(Y1, ld, D, mean, rstd);
    for (int c = sub; c < D; c += 16) {
        const float v = Y1[row * ld + c];
        A[row * ld + c] = (float)(((double)v - mean) * rstd * (double)p.g2[c] + (double)p.be2[c]);
        if (y1t != nullptr && gr < M) y1t[(long)gr * D + c] = v;
    }
    if (stats2 != nullptr && sub == 0 && gr < M) { stats2[2 * (long)gr] = mean; stats2[2 * (long)gr + 1] = rstd; }
    __syncthreads();
    tile_gemm(A, ld, D, p.w1, 1, D, F, [&](int r, int c, float v) {
        const int g = r0 + r;
        const float hv = v + p.b1[c];
        if (ht != nullptr && g < M) ht[(long)g * F + c] = hv;
        Hs[r * ldf + c] = drop_mul(dr, VT_DROP_SITE_FF, (unsigned long long)g * F + c, act_f(act, hv));
    });
    __syncthreads();
    tile_gemm(Hs, ldf, F, p.w2, 1, F, D, [&](int r, int c, float v) {
        const int g = r0 + r;
        if (g < M) y[(long)g * D + c] = Y1[r * ld + c] + drop_mul(dr, VT_DROP_SITE_2, (unsigned long long)g * D + c, v + p.b2[c]);
    });
}

// ---- backward -----------------------------------------------------------------------------------------------------------------------------------------------
// the row-major (M x .) matrices a backward leaves in its workspace for the sums over rows: the gradient side and the input side of every GEMM and norm
struct BwdWs { float *du, *af, *dh, *z, *dz, *e2, *dop, *dO, *dy1, *dqkv, *xn, *xnp, *dxn, *e1; };

__global__ __launch_bounds__(NTHR) void k_ff_bwd(const float *__restrict__ dy, const float *__restrict__ y1t, const float *__restrict__ ht,
                                                 const double *__restrict__ stats2, LayerP p, int M, int D, int F, int act, Drop dr, BwdWs w)
{
    extern __shared__ float lds[];
    const int ld = D + 4, ldf = F + 4, r0 = blockIdx.x * RT, row = threadIdx.x >> 4, sub = threadIdx.x & 15, gr = r0 + row;
    const bool valid = gr < M;
    float *G = lds, *Y1 = lds + RT * ld, *Hs = lds + 2 * RT * ld;
    for (int c = sub; c < D; c += 16) {
        const float du = valid ? drop_mul(dr, VT_DROP_SITE_2, (unsigned long long)gr * D + c, dy[(long)gr * D + c]) : 0.f;
        G[row * ld + c] = du; Y1[row * ld + c] = valid ? y1t[(long)gr * D + c] : 0.f;
        if (valid) w.du[(long)gr * D + c] = du;
    }
    if (valid)
        for (int c = sub; c < F; c += 16) w.af[(long)gr * F + c] = drop_mul(dr, VT_DROP_SITE_FF, (unsigned long long)gr * F + c, act_f(act, ht[(long)gr * F + c]));
    __syncthreads();
    tile_gemm(G, ld, D, p.w2, F, 1, F, [&](int r, int c, float v) {                 // d_a = d_u W2, then through dropout and the activation
        const int g = r0 + r;
        const float hv = g < M ? ht[(long)g * F + c] : 0.f;
        const float dh = drop_mul(dr, VT_DROP_SITE_FF, (unsigned long long)g * F + c, v) * act_d(act, hv);
        Hs[r * ldf + c] = dh;
        if (g < M) w.dh[(long)g * F + c] = dh;
    });
    __syncthreads();
    tile_gemm(Hs, ldf, F, p.w1, D, 1, D, [&](int r, int c, float v) { G[r * ld + c] = v; });      // d_z = d_h W1
    __syncthreads();
    const double mean = valid ? stats2[2 * (long)gr] : 0.0, rstd = valid ? stats2[2 * (long)gr + 1] : 0.0;
    ln_bwd_row(G, Y1, ld, D, mean, rstd, p.g2, [&](int c, double xh, float g, float dx) {
        float dop = 0.f;
        if (valid) {
            const long o = (long)gr * D + c;
            w.z[o] = (float)(xh * (double)p.g2[c] + (double)p.be2[c]); w.dz[o] = g; w.e2[o] = (float)((double)g * xh);
            const float dy1 = dy[o] + dx;
            w.dy1[o] = dy1;
            dop = drop_mul(dr, VT_DROP_SITE_1, (unsigned long long)o, dy1);
            w.dop[o] = dop;
        }
        G[row * ld + c] = dop;          // the thread's own element: nobody else reads it before the barrier
    });
    __syncthreads();
    tile_gemm(G, ld, D, p.wo, D, 1, D, [&](int r, int c, float v) { if (r0 + r < M) w.dO[(long)(r0 + r) * D + c] = v; });
}

// tr = 0 (launched first): the strip's rows are 16 queries; delta_i = sum_j d_P_ij P_ij is summed in fp64 along the row, kept for the second launch, and
// d_q = d_S K.  tr = 1: the rows are 16 keys (the transposed strip), d_k = d_S^T Q and d_v = Pd^T d_O.  d_S = P (d_P - delta) scale.  (delta as sum_c d_O_ic O_ic
// would need no second launch, but it does not cancel d_P exactly where a row of P is one-hot: measured 4.4 e32 on d_x at T = 1.)
__global__ __launch_bounds__(NTHR) void k_attn_bwd(const float *__restrict__ qkv, const float *__restrict__ lse, const float *__restrict__ dO,
                                                   const unsigned char *__restrict__ kpm, int T, int D, int H, float scale, Drop dr, int tr,
                                                   float *__restrict__ delta_ws, float *__restrict__ dqkv)
{
    __shared__ float S1[RT * SLD], S2[RT * SLD], delta[MAXT], lses[MAXT];
    const int r0 = blockIdx.x * RT, h = blockIdx.y, b = blockIdx.z, hd = D / H, D3 = 3 * D, W = ((T + 15) / 16) * 16;
    const float *Q = qkv + (long)b * T * D3 + h * hd, *K = Q + D, *V = Q + 2 * D;
    const float *dOp = dO + (long)b * T * D + h * hd;
    const long bh = (long)(b * H + h) * T;
    for (int i = threadIdx.x; i < T; i += NTHR) { lses[i] = lse[bh + i]; delta[i] = tr ? delta_ws[bh + i] : 0.f; }
    if (tr) { score_strip(S1, K, D3, Q, D3, r0, T, hd); score_strip(S2, V, D3, dOp, D, r0, T, hd); }
    else    { score_strip(S1, Q, D3, K, D3, r0, T, hd); score_strip(S2, dOp, D, V, D3, r0, T, hd); }
    __syncthreads();
    float *dst = dqkv + (long)b * T * D3 + h * hd;
    if (!tr) {
        const int row = threadIdx.x >> 4, sub = threadIdx.x & 15, qi = r0 + row;
        double s = 0.0;
        for (int c = sub; c < W; c += 16) {
            float P = 0.f, dP = 0.f;
            if (qi < T && c < T && !(kpm != nullptr && kpm[(long)b * T + c])) {
                P = expf(S1[row * SLD + c] * scale - lses[qi]);
                dP = drop_mul(dr, VT_DROP_SITE_ATTN, (unsigned long long)(bh + qi) * T + c, S2[row * SLD + c]);
            }
            S1[row * SLD + c] = P; S2[row * SLD + c] = dP;
            s += (double)dP * (double)P;
        }
        const float dl = (float)sum16(s);
        if (sub == 0 && qi < T) delta_ws[bh + qi] = dl;
        for (int c = sub; c < W; c += 16) S1[row * SLD + c] = S1[row * SLD + c] * (S2[row * SLD + c] - dl) * scale;
        __syncthreads();
        strip_times(S1, K, D3, dst, D3, r0, T, hd);
        return;
    }
    for (int idx = threadIdx.x; idx < RT * W; idx += NTHR) {
        const int r = idx / W, qi = idx - r * W, kj = r0 + r;
        float dS = 0.f, Pd = 0.f;
        if (qi < T && kj < T && !(kpm != nullptr && kpm[(long)b * T + kj])) {
            const float P = expf(S1[r * SLD + qi] * scale - lses[qi]);
            const unsigned long long e = (unsigned long long)(bh + qi) * T + kj;
            const float dP = drop_mul(dr, VT_DROP_SITE_ATTN, e, S2[r * SLD + qi]);
            dS = P * (dP - delta[qi]) * scale;
            Pd = drop_mul(dr, VT_DROP_SITE_ATTN, e, P);
        }
        S1[r * SLD + qi] = dS; S2[r * SLD + qi] = Pd;
    }
    __syncthreads();
    strip_times(S1, Q, D3, dst + D, D3, r0, T, hd);
    strip_times(S2, dOp, D, dst + 2 * D, D3, r0, T, hd);
}

__global__ __launch_bounds__(NTHR) void k_qkv_bwd(const float *__restrict__ x, const float *__restrict__ pos, const double *__restrict__ stats1, LayerP p, int M,
                                                  int T, int D, BwdWs w, float *__restrict__ dx_out, int accumulate)
{
    extern __shared__ float lds[];
    const int D3 = 3 * D, ld = D + 4, ld3 = D3 + 4, r0 = blockIdx.x * RT, row = threadIdx.x >> 4, sub = threadIdx.x & 15, gr = r0 + row;
    const bool valid = gr < M;
    float *G = lds, *X = lds + RT * ld3, *DXN = X + RT * ld;
    for (int c = sub; c < D3; c += 16) G[row * ld3 + c] = valid ? w.dqkv[(long)gr * D3 + c] : 0.f;
    for (int c = sub; c < D; c += 16) X[row * ld + c] = valid ? x[(long)gr * D + c] : 0.f;
    __syncthreads();
    tile_gemm(G, ld3, D3, p.wi, D, 1, D, [&](int r, int c, float v) { DXN[r * ld + c] = v; });    // q, k and v all read LN1(x) with derivative 1
    __syncthreads();
    const double mean = valid ? stats1[2 * (long)gr] : 0.0, rstd = valid ? stats1[2 * (long)gr + 1] : 0.0;
    const int t = valid ? gr % T : 0;
    ln_bwd_row(DXN, X, ld, D, mean, rstd, p.g1, [&](int c, double xh, float g, float dx) {
        if (!valid) return;
        const long o = (long)gr * D + c;
        const float xn = (float)(xh * (double)p.g1[c] + (double)p.be1[c]);
        w.xn[o] = xn; w.xnp[o] = xn + pos[t * D + c]; w.dxn[o] = g; w.e1[o] = (float)((double)g * xh);
        if (dx_out != nullptr) { const float v = w.dy1[o] + dx; dx_out[o] = accumulate ? dx_out[o] + v : v; }
    });
}

// ---- sums over the M rows --------------------------------------------------------------------------------------------------------------------------------------
// dW (N x K) = sum_rows G[row, :N]^T A[row, :K]: one partial per chunk of CHUNK rows (fp32 MFMA accumulation inside a chunk), part[chunk][N][K]
struct WgradP { const float *G, *A; float *part; int ldg, lda, N, K, tile0; };
struct WgradTab { WgradP p[5]; int n, tiles; };
__global__ __launch_bounds__(NTHR) void k_wgrad(WgradTab tab, int M)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, q = lane >> 4;
    const int tile = blockIdx.x * NWAVE + wave, chunk = blockIdx.y;
    if (tile >= tab.tiles) return;
    int pi = 0;
    for (int i = 1; i < tab.n; i++) if (tile >= tab.p[i].tile0) pi = i;
    const float *G = tab.p[pi].G, *A = tab.p[pi].A;
    float *part = tab.p[pi].part;
    const int ldg = tab.p[pi].ldg, lda = tab.p[pi].lda, N = tab.p[pi].N, K = tab.p[pi].K, lt = tile - tab.p[pi].tile0;
    const int nkt = K / 16, nt = lt / nkt, kt = lt - nt * nkt;
    const int m0 = chunk * CHUNK, m1 = min(M, m0 + CHUNK);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int m = m0; m < m1; m += 4) {
        const int r = m + q;
        const bool v = r < m1;
        acc = MFMA16(v ? G[(long)r * ldg + nt * 16 + j] : 0.f, v ? A[(long)r * lda + kt * 16 + j] : 0.f, acc);
    }
    float *o = part + (long)chunk * N * K;
#pragma unroll
    for (int i = 0; i < 4; i++) o[(long)(nt * 16 + 4 * q + i) * K + kt * 16 + j] = acc[i];
}

// column sums of a row-major matrix, fp64, one partial per chunk: part[chunk][N]
struct ColP { const float *S; double *part; int ld, N; };
struct ColTab { ColP p[8]; };
__global__ __launch_bounds__(NTHR) void k_colsum(ColTab tab, int M)
{
    const ColP P = tab.p[blockIdx.x];
    const int chunk = blockIdx.y, m0 = chunk * CHUNK, m1 = min(M, m0 + CHUNK);
    for (int c = threadIdx.x; c < P.N; c += NTHR) {
        double s = 0.0;
        for (int r = m0; r < m1; r++) s += (double)P.S[(long)r * P.ld + c];
        P.part[(long)chunk * P.N + c] = s;
    }
}

// out[e] (+)= the chunk partials of e added in fp64 in chunk order, rounded once
struct RedP { float *out; const float *fpart; const double *dpart; int n; };
struct RedTab { RedP p[14]; };
__global__ __launch_bounds__(NTHR) void k_reduce(RedTab tab, int nchunk, int accumulate)
{
    const RedP P = tab.p[blockIdx.y];
    const int e = blockIdx.x * NTHR + threadIdx.x;
    if (e >= P.n) return;
    double s = 0.0;
    if (P.fpart != nullptr) for (int ch = 0; ch < nchunk; ch++) s += (double)P.fpart[(long)ch * P.n + e];
    else for (int ch = 0; ch < nchunk; ch++) s += P.dpart[(long)ch * P.n + e];
    P.out[e] = accumulate ? P.out[e] + (float)s : (float)s;
}

// ---- the final LayerNorm of a stack ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NTHR) void k_ln_fwd(const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ beta, int M, int D,
                                                 float *__restrict__ y, double *__restrict__ stats)
{
    extern __shared__ float lds[];
    const int ld = D + 4, r0 = blockIdx.x * RT, row = threadIdx.x >> 4, sub = threadIdx.x & 15, gr = r0 + row;
    for (int c = sub; c < D; c += 16) lds[row * ld + c] = gr < M ? x[(long)gr * D + c] : 0.f;
    double mean, rstd;
    ln_stats(lds, ld, D, mean, rstd);
    if (gr >= M) return;
    for (int c = sub; c < D; c += 16) y[(long)gr * D + c] = (float)(((double)lds[row * ld + c] - mean) * rstd * (double)gamma[c] + (double)beta[c]);
    if (stats != nullptr && sub == 0) { stats[2 * (long)gr] = mean; stats[2 * (long)gr + 1] = rstd; }
}

__global__ __launch_bounds__(NTHR) void k_ln_bwd(const float *__restrict__ dy, const float *__restrict__ x, const double *__restrict__ stats,
                                                 const float *__restrict__ gamma, int M, int D, float *__restrict__ e, float *__restrict__ dx_out, int accumulate)
{
    extern __shared__ float lds[];
    const int ld = D + 4, r0 = blockIdx.x * RT, row = threadIdx.x >> 4, sub = threadIdx.x & 15, gr = r0 + row;
    const bool valid = gr < M;
    float *G = lds, *X = lds + RT * ld;
    for (int c = sub; c < D; c += 16) { G[row * ld + c] = valid ? dy[(long)gr * D + c] : 0.f; X[row * ld + c] = valid ? x[(long)gr * D + c] : 0.f; }
    const double mean = valid ? stats[2 * (long)gr] : 0.0, rstd = valid ? stats[2 * (long)gr + 1] : 0.0;
    ln_bwd_row(G, X, ld, D, mean, rstd, gamma, [&](int c, double xh, float g, float dx) {
        if (!valid) return;
        const long o = (long)gr * D + c;
        e[o] = (float)((double)g * xh);
        if (dx_out != nullptr) dx_out[o] = accumulate ? dx_out[o] + dx : dx;
    });
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------------------------
static inline bool shape_ok(long B, long T, long D, long H, long F)
{
    if (B < 1 || B > 65535 || T < 1 || T > MAXT || D < 16 || D > MAXD || D % 16 || F < 16 || F > MAXF || F % 16 || H < 1 || D % H) return false;
    const long hd = D / H;
    return hd == 16 || hd == 32 || hd == 160;
}
static inline long nchunks(long M) { return (M + CHUNK - 1) / CHUNK; }
static inline bool aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

static int make_drop(float p, unsigned long long seed, Drop *d)
{
    VT_REQUIRE(p >= 0.f && p < 1.f, "formertrain: dropout p = %g outside [0, 1)", (double)p);
    const double thr = floor((double)p * 4294967296.0);
    d->thr = (unsigned)thr; d->seed = seed;
    d->inv = d->thr == 0u ? 1.f : 1.f / (1.f - p);
    return VT_OK;
}

// the workspace of a layer backward: fp64 column-sum partials first, then the row matrices of BwdWs, then the weight-gradient partials
struct WsLayout { long col_doubles, rows_floats, wpart_floats, total_floats; };
static inline WsLayout ws_layout(long M, long D, long F, long BHT)
{
    WsLayout l;
    const long nc = nchunks(M);
    l.col_doubles = nc * (9 * D + F);                       // b_in 3D | b_out D | b1 F | b2 D | norm1 w, b | norm2 w, b
    l.rows_floats = M * (14 * D + 2 * F) + BHT;             // du af dh z dz e2 dop dO dy1 dqkv(3D) xn xnp dxn e1 | delta (B, H, T)
    l.wpart_floats = nc * (4 * D * D + 2 * F * D);
    l.total_floats = 2 * l.col_doubles + l.rows_floats + l.wpart_floats;
    return l;
}

}  // namespace formt

using namespace formt;

extern "C" long vt_former_layer_tape_floats(int B, int T, int D, int H, int F)
{
    if (!shape_ok(B, T, D, H, F)) return -1;
    const long M = (long)B * T;
    return 8 * M + M * (5L * D + F) + (long)B * H * T;      // 4 fp64 per row | qkv 3D | O D | y1 D | h F | lse
}

extern "C" long vt_former_layer_workspace_floats(int B, int T, int D, int H, int F)
{
    if (!shape_ok(B, T, D, H, F)) return -1;
    return ws_layout((long)B * T, D, F, (long)B * H * T).total_floats;
}

extern "C" long vt_layernorm_backward_workspace_floats(long M, int D)
{
    if (M < 1 || M > (1L << 24) || D < 16 || D > MAXD || D % 16) return -1;
    return 2 * nchunks(M) * 2 * D + M * D;
}

struct TapeP { double *stats1, *stats2; float *qkv, *O, *y1, *h, *lse; };
static TapeP tape_ptrs(float *tape, long M, long B, long T, long D, long H, long F)
{
    TapeP t;
    t.stats1 = reinterpret_cast<double *>(tape); t.stats2 = t.stats1 + 2 * M;
    t.qkv = tape + 8 * M; t.O = t.qkv + 3 * M * D; t.y1 = t.O + M * D; t.h = t.y1 + M * D; t.lse = t.h + M * F;
    return t;
}

extern "C" int vt_former_layer_forward(const float *x, const float *pos, const unsigned char *key_padding_mask, const float *const *params, int B, int T, int D, int H,
                                       int F, int activation, float p, unsigned long long seed, float *y, float *tape, float *workspace, void *stream)
{
    VT_REQUIRE(shape_ok(B, T, D, H, F), "vt_former_layer_forward: unsupported shape B %d T %d D %d H %d F %d (T <= 192, D %% 16 == 0 <= 160, F %% 16 == 0 <= 256, D / H in "
               "{16, 32, 160})", B, T, D, H, F);
    VT_REQUIRE(activation >= 0 && activation <= 2, "vt_former_layer_forward: activation %d (0 relu, 1 gelu, 2 leaky_relu)", activation);
    VT_REQUIRE(x && pos && params && y, "vt_former_layer_forward: NULL x / pos / params / y");
    VT_REQUIRE(tape || workspace, "vt_former_layer_forward: without a tape the q|k|v and P V rows need a workspace of 4 B T D floats");
    VT_REQUIRE(aligned(tape, 8), "vt_former_layer_forward: tape not 8-byte aligned");
    LayerP lp;
    const float **dst = &lp.wi;
    for (int i = 0; i < 12; i++) { VT_REQUIRE(params[i], "vt_former_layer_forward: NULL parameter %d", i); dst[i] = params[i]; }
    Drop dr;
    if (int rc = make_drop(p, seed, &dr)) return rc;
    const long M = (long)B * T;
    TapeP t = {};
    float *qkv, *O;
    if (tape) { t = tape_ptrs(tape, M, B, T, D, H, F); qkv = t.qkv; O = t.O; }
    else { qkv = workspace; O = workspace + 3 * M * D; }
    hipStream_t st = vt_stream(stream);
    const int tiles = (int)((M + RT - 1) / RT), hd = D / H;
    k_ln_qkv<<<tiles, NTHR, 2 * RT * (D + 4) * sizeof(float), st>>>(x, pos, lp, (int)M, T, D, t.stats1, qkv);
    VT_LAUNCH_CHECK();
    k_attn_fwd<<<dim3((T + 15) / 16, H, B), NTHR, 0, st>>>(qkv, key_padding_mask, T, D, H, 1.f / sqrtf((float)hd), dr, O, t.lse);
    VT_LAUNCH_CHECK();
    k_out_ff<<<tiles, NTHR, (2 * RT * (D + 4) + RT * (F + 4)) * sizeof(float), st>>>(x, O, lp, (int)M, D, F, activation, dr, t.y1, t.stats2, t.h, y);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

static int run_sums(const WgradTab &wt, const ColTab &ct, int ncol, const RedTab &rt, int nred, int maxn, long M, int accumulate, hipStream_t st)
{
    const int nc = (int)nchunks(M);
    if (wt.n > 0) { k_wgrad<<<dim3((wt.tiles + NWAVE - 1) / NWAVE, nc), NTHR, 0, st>>>(wt, (int)M); VT_LAUNCH_CHECK(); }
    if (ncol > 0) { k_colsum<<<dim3(ncol, nc), NTHR, 0, st>>>(ct, (int)M); VT_LAUNCH_CHECK(); }
    if (nred > 0) { k_reduce<<<dim3((maxn + NTHR - 1) / NTHR, nred), NTHR, 0, st>>>(rt, nc, accumulate); VT_LAUNCH_CHECK(); }
    return VT_OK;
}

extern "C" int vt_former_layer_backward(const float *d_y, const float *tape, const float *x, const float *pos, const unsigned char *key_padding_mask,
                                        const float *const *params, int B, int T, int D, int H, int F, int activation, float p, unsigned long long seed,
                                        float *d_x, float *const *d_params, int accumulate, float *workspace, void *stream)
{
    VT_REQUIRE(shape_ok(B, T, D, H, F), "vt_former_layer_backward: unsupported shape B %d T %d D %d H %d F %d (T <= 192, D %% 16 == 0 <= 160, F %% 16 == 0 <= 256, D / H in "
               "{16, 32, 160})", B, T, D, H, F);
    VT_REQUIRE(activation >= 0 && activation <= 2, "vt_former_layer_backward: activation %d (0 relu, 1 gelu, 2 leaky_relu)", activation);
    VT_REQUIRE(d_y && tape && x && pos && params && workspace, "vt_former_layer_backward: NULL d_y / tape / x / pos / params / workspace");
    VT_REQUIRE(aligned(tape, 8) && aligned(workspace, 8), "vt_former_layer_backward: tape / workspace not 8-byte aligned");
    LayerP lp;
    const float **dst = &lp.wi;
    for (int i = 0; i < 12; i++) { VT_REQUIRE(params[i], "vt_former_layer_backward: NULL parameter %d", i); dst[i] = params[i]; }
    Drop dr;
    if (int rc = make_drop(p, seed, &dr)) return rc;
    const long M = (long)B * T, nc = nchunks(M), MD = M * D, MF = M * F;
    const TapeP t = tape_ptrs(const_cast<float *>(tape), M, B, T, D, H, F);
    const WsLayout wl = ws_layout(M, D, F, (long)B * H * T);
    double *colp = reinterpret_cast<double *>(workspace);
    float *f = workspace + 2 * wl.col_doubles;
    BwdWs w;
    w.du = f; f += MD; w.af = f; f += MF; w.dh = f; f += MF; w.z = f; f += MD; w.dz = f; f += MD; w.e2 = f; f += MD; w.dop = f; f += MD; w.dO = f; f += MD;
    w.dy1 = f; f += MD; w.dqkv = f; f += 3 * MD; w.xn = f; f += MD; w.xnp = f; f += MD; w.dxn = f; f += MD; w.e1 = f; f += MD;
    float *delta_ws = f; f += (long)B * H * T;
    float *wpart = f;
    hipStream_t st = vt_stream(stream);
    const int tiles = (int)((M + RT - 1) / RT), hd = D / H;
    k_ff_bwd<<<tiles, NTHR, (2 * RT * (D + 4) + RT * (F + 4)) * sizeof(float), st>>>(d_y, t.y1, t.h, t.stats2, lp, (int)M, D, F, activation, dr, w);
    VT_LAUNCH_CHECK();
    for (int tr = 0; tr < 2; tr++) {
        k_attn_bwd<<<dim3((T + 15) / 16, H, B), NTHR, 0, st>>>(t.qkv, t.lse, w.dO, key_padding_mask, T, D, H, 1.f / sqrtf((float)hd), dr, tr, delta_ws, w.dqkv);
        VT_LAUNCH_CHECK();
    }
    k_qkv_bwd<<<tiles, NTHR, (RT * (3 * D + 4) + 2 * RT * (D + 4)) * sizeof(float), st>>>(x, pos, t.stats1, lp, (int)M, T, D, w, d_x, accumulate);
    VT_LAUNCH_CHECK();
    if (d_params == nullptr) return VT_OK;
    // parameter order: in_proj_weight, in_proj_bias, out_proj.weight, out_proj.bias, linear1.weight, linear1.bias, linear2.weight, linear2.bias, norm1.weight,
    // norm1.bias, norm2.weight, norm2.bias
    WgradTab wt = {}; ColTab ct = {}; RedTab rt = {};
    int ncol = 0, nred = 0, maxn = 0;
    auto add_w = [&](const float *G, int ldg, int N, const float *A, int lda, int K, float *out) {
        WgradP &q = wt.p[wt.n++];
        q.G = G; q.A = A; q.ldg = ldg; q.lda = lda; q.N = N; q.K = K; q.part = wpart; q.tile0 = wt.tiles;
        wt.tiles += (N / 16) * (K / 16);
        RedP &r = rt.p[nred++];
        r.out = out; r.fpart = wpart; r.dpart = nullptr; r.n = N * K;
        wpart += nc * N * K; maxn = r.n > maxn ? r.n : maxn;
    };
    auto add_c = [&](const float *S, int ld, int N, float *out) {
        ColP &q = ct.p[ncol++];
        q.S = S; q.ld = ld; q.N = N; q.part = colp;
        RedP &r = rt.p[nred++];
        r.out = out; r.fpart = nullptr; r.dpart = colp; r.n = N;
        colp += nc * N; maxn = N > maxn ? N : maxn;
    };
    if (d_params[0]) { add_w(w.dqkv, 3 * D, 2 * D, w.xnp, D, D, d_params[0]); add_w(w.dqkv + 2 * D, 3 * D, D, w.xn, D, D, d_params[0] + 2 * D * D); }
    if (d_params[1]) add_c(w.dqkv, 3 * D, 3 * D, d_params[1]);
    if (d_params[2]) add_w(w.dop, D, D, t.O, D, D, d_params[2]);
    if (d_params[3]) add_c(w.dop, D, D, d_params[3]);
    if (d_params[4]) add_w(w.dh, F, F, w.z, D, D, d_params[4]);
    if (d_params[5]) add_c(w.dh, F, F, d_params[5]);
    if (d_params[6]) add_w(w.du, D, D, w.af, F, F, d_params[6]);
    if (d_params[7]) add_c(w.du, D, D, d_params[7]);
    if (d_params[8]) add_c(w.e1, D, D, d_params[8]);
    if (d_params[9]) add_c(w.dxn, D, D, d_params[9]);
    if (d_params[10]) add_c(w.e2, D, D, d_params[10]);
    if (d_params[11]) add_c(w.dz, D, D, d_params[11]);
    return run_sums(wt, ct, ncol, rt, nred, maxn, M, accumulate, st);
}

extern "C" int vt_layernorm_forward(const float *x, const float *weight, const float *bias, long M, int D, float *y, double *stats, void *stream)
{
    VT_REQUIRE(vt_layernorm_backward_workspace_floats(M, D) > 0, "vt_layernorm_forward: unsupported M %ld D %d (D %% 16 == 0, 16 <= D <= 160)", M, D);
    VT_REQUIRE(x && weight && bias && y, "vt_layernorm_forward: NULL x / weight / bias / y");
    VT_REQUIRE(aligned(stats, 8), "vt_layernorm_forward: stats not 8-byte aligned");
    k_ln_fwd<<<(int)((M + RT - 1) / RT), NTHR, RT * (D + 4) * sizeof(float), vt_stream(stream)>>>(x, weight, bias, (int)M, D, y, stats);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

extern "C" int vt_layernorm_backward(const float *d_y, const float *x, const double *stats, const float *weight, long M, int D, float *d_x, float *d_weight,
                                     float *d_bias, int accumulate, float *workspace, void *stream)
{
    VT_REQUIRE(vt_layernorm_backward_workspace_floats(M, D) > 0, "vt_layernorm_backward: unsupported M %ld D %d (D %% 16 == 0, 16 <= D <= 160)", M, D);
    VT_REQUIRE(d_y && x && stats && weight && workspace, "vt_layernorm_backward: NULL d_y / x / stats / weight / workspace");
    VT_REQUIRE(aligned(stats, 8) && aligned(workspace, 8), "vt_layernorm_backward: stats / workspace not 8-byte aligned");
    const long nc = nchunks(M);
    double *colp = reinterpret_cast<double *>(workspace);
    float *e = workspace + 2 * nc * 2 * D;
    hipStream_t st = vt_stream(stream);
    k_ln_bwd<<<(int)((M + RT - 1) / RT), NTHR, 2 * RT * (D + 4) * sizeof(float), st>>>(d_y, x, stats, weight, (int)M, D, e, d_x, accumulate);
    VT_LAUNCH_CHECK();
    WgradTab wt = {}; ColTab ct = {}; RedTab rt = {};
    int ncol = 0, nred = 0;
    if (d_weight) { ct.p[ncol++] = ColP{e, colp, D, D}; rt.p[nred++] = RedP{d_weight, nullptr, colp, D}; }
    if (d_bias) { ct.p[ncol++] = ColP{d_y, colp + nc * D, D, D}; rt.p[nred++] = RedP{d_bias, nullptr, colp + nc * D, D}; }
    return run_sums(wt, ct, ncol, rt, nred, D, M, accumulate, st);
}
