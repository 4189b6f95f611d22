// infillhead.hip -- the ends of HVOP-Net's training step: the input projections (mfiller_cond.py:82-96), the predictor MLP (mfiller_cond.py:97-104) and the
// motion objective with its gradient (trainer_infiller.py:33-47).  Same conventions as formertrain.hip, whose k_wgrad / k_colsum / k_reduce pattern is
// restated here for ragged widths.
//
//   y = x W^T + b                                            h = f W1^T + b1,  a = h > 0 ? h : 0.01 h,  pred = a W2^T + b2
//   loss_pos = lw_pose mean |pred - gt|                      loss_accel = lw_accel mean |acc(pred) - acc(gt)|,  acc(a)[t] = a[t] - 2 a[t+1] + a[t+2] inside a clip
//
// LAUNCHES.  Rows are the M = B T frames in tiles of 16.
//   k_proj_fwd   per (problem, row tile)   every projection of a table in one launch; x staged in LDS zero-padded to a multiple of 4 columns
//   k_head_fwd   per row tile              both GEMMs of the predictor; h saved for the backward (NULL: not saved)
//   k_head_bwd   per row tile              the objective's per-tile fp64 partials and d_pred (a gather: the element's writer reads its clip's rows t-2 .. t+2 of
//                                          pred and gt from global memory), or a given d_pred; then d_h = (d_pred W2) slope(h) and d_f = d_h W1
//   k_wgrad, k_colsum, k_reduce            weight and bias gradients: per-chunk partials, then one fp64 sum in chunk order; k_reduce's last block row also adds
//                                          the objective's tile partials (tiles of a chunk in order, then the chunks in order) into the two fp64 terms
//   a step's ends: 1 + 3 launches for the pair of projections, 1 + 4 for the predictor with the objective.
//
// ARITHMETIC.  Every GEMM product is an exact fp32 product on v_mfma_f32_16x16x4_f32 with fp32 accumulation in a fixed order (four chains over k mod 16, each k ascending, added as (0 + 1) + (2 + 3)); ragged K and N are
// zero-padded in the operands and guarded in the stores.  pred - gt and the six-term stencil are formed in fp64 from the fp32 values: exact, so sign() is the
// sign of the real-number definition.  d_pred = upstream (c_pos s + c_acc (sa[t-2] - 2 sa[t-1] + sa[t])) in fp64, rounded once.  A sum over the M rows is split
// into chunks of 512 rows whose partials are added in fp64 in chunk order and rounded once.  No atomics, one writer per element, the same bits on every call;
// everything after d_pred is linear in it with no constant added, so a power-of-two scale scales every gradient bit for bit; no row of pred, d_pred or d_f reads
// another clip's data (a row tile may hold rows of two clips, but MFMA rows are independent, and the stencil stays inside the clip).
// LDS row strides are 2 mod 32 (or 18 mod 32) floats: the A-operand read As[(lane & 15) ld + (lane >> 4) + k] then touches 32 different banks within each half
// wave (lanes 0-31 and 32-63 apart; across the whole wave the banks repeat).  No bank-conflict counter was read: unmeasured.  Known idle lanes, accepted at
// these sizes: a GEMM with N = out_dim <= 16 is one column tile, so wave 0 runs it while three waves wait; k_colsum over out_dim columns uses out_dim of 256 threads.
#include "common.h"

namespace ifh {

typedef float f32x4 __attribute__((ext_vector_type(4)));
#define IFH_MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

constexpr int NTHR = 256, NWAVE = 4, RT = 16;   // a workgroup: 4 waves, one 16-row tile; thread t owns row t >> 4 and column t & 15 (+ 16 n) of it
constexpr int CHUNK = 512;                       // rows per partial of a sum over the M rows
constexpr int TPC = CHUNK / RT;                  // row tiles per chunk
constexpr int MAXD = 160, MAXH = 64, MAXC = 16, MAXPROB = 4;
constexpr int LDX = MAXD + 2, LDH = MAXH + 2, LDP = MAXC + 2;
constexpr long MAXM = 1L << 24;

struct HeadP { const float *w1, *b1, *w2, *b2; };

__device__ __forceinline__ double sum16(double v)
{
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double sgn(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0); }

// C (16 x N) = A (16 x Kp in LDS, row stride lda, zero from K to Kp = the next multiple of 4) B (K x N in global memory, B(k, n) = Bp[k sk + n sn]); rows of B from
// K on and columns from N on read as zero; the waves take the column tiles round robin; epi(row, col < N, value) for each of the lane's four results.
template <class Epi>
__device__ __forceinline__ void tile_gemm(const float *As, int lda, int K, const float *__restrict__ Bp, long sk, long sn, int N, Epi epi)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, q = lane >> 4, Kp = (K + 3) & ~3;
    for (int ct = wave; ct < (N + 15) / 16; ct += NWAVE) {
        const int n = ct * 16 + j;
        const bool nv = n < N;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acc1 = acc, acc2 = acc, acc3 = acc;
        const float *bp = Bp + (long)(nv ? n : 0) * sn;
        const float *ap = As + j * lda + q;
        auto bv = [&](int kk) { return (nv && kk < K) ? bp[(long)kk * sk] : 0.f; };
        int k = 0;
        for (; k + 16 <= Kp; k += 16) {                          // four independent chains over k mod 16: shorter sums and no MFMA waiting on the one before it
            acc = IFH_MFMA16(ap[k], bv(k + q), acc);
            acc1 = IFH_MFMA16(ap[k + 4], bv(k + 4 + q), acc1);
            acc2 = IFH_MFMA16(ap[k + 8], bv(k + 8 + q), acc2);
            acc3 = IFH_MFMA16(ap[k + 12], bv(k + 12 + q), acc3);
        }
        for (; k < Kp; k += 4) acc = IFH_MFMA16(ap[k], bv(k + q), acc);
        acc = (acc + acc1) + (acc2 + acc3);
        if (nv) {
#pragma unroll
            for (int i = 0; i < 4; i++) epi(4 * q + i, n, acc[i]);
        }
    }
}

// ---- the input projections ---------------------------------------------------------------------------------------------------------------------------------------
struct ProjP { const float *x, *w, *b; float *y; int K, N, tile0; };
struct ProjTab { ProjP p[MAXPROB]; int n; };

__global__ __launch_bounds__(NTHR) void k_proj_fwd(ProjTab tab, int M)
{
    __shared__ float X[RT * LDX];
    int pi = 0;
    for (int i = 1; i < tab.n; i++) if ((int)blockIdx.x >= tab.p[i].tile0) pi = i;
    const float *x = tab.p[pi].x, *w = tab.p[pi].w, *b = tab.p[pi].b;
    float *y = tab.p[pi].y;
    const int K = tab.p[pi].K, N = tab.p[pi].N, Kp = (K + 3) & ~3;
    const int r0 = ((int)blockIdx.x - tab.p[pi].tile0) * RT, row = threadIdx.x >> 4, sub = threadIdx.x & 15, gr = r0 + row;
    for (int c = sub; c < Kp; c += 16) X[row * LDX + c] = (gr < M && c < K) ? x[(long)gr * K + c] : 0.f;
    __syncthreads();
    tile_gemm(X, LDX, K, w, 1, K, N, [&](int r, int c, float v) { if (r0 + r < M) y[(long)(r0 + r) * N + c] = v + b[c]; });
}

// ---- the predictor ---------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NTHR) void k_head_fwd(const float *__restrict__ f, HeadP p, int M, int D, int Hd, int C, float *__restrict__ ht, float *__restrict__ pred)
{
    __shared__ float FS[RT * LDX], HS[RT * LDH];
    const int r0 = blockIdx.x * RT, row = threadIdx.x >> 4, sub = threadIdx.x & 15, gr = r0 + row;
    for (int c = sub; c < D; c += 16) FS[row * LDX + c] = gr < M ? f[(long)gr * D + c] : 0.f;
    __syncthreads();
    tile_gemm(FS, LDX, D, p.w1, 1, D, Hd, [&](int r, int c, float v) {
        const int g = r0 + r;
        const float hv = v + p.b1[c];
        if (ht != nullptr && g < M) ht[(long)g * Hd + c] = hv;
        HS[r * LDH + c] = hv > 0.f ? hv : 0.01f * hv;
    });
    __syncthreads();
    tile_gemm(HS, LDH, Hd, p.w2, 1, Hd, C, [&](int r, int c, float v) { if (r0 + r < M) pred[(long)(r0 + r) * C + c] = v + p.b2[c]; });
}

// the objective of a launch: gt and pred (M, C), the coefficients of d_pred (already times the upstream scale), the per-tile partials {sum |e|, sum |ea|}
struct ObjP { const float *gt, *pred; double c_pos, c_acc; double *tpart; };

// dp_in != NULL: d_pred is given.  dp_in == NULL: d_pred and the tile's partial sums come from the objective.  want_grad == 0 stops after them.
__global__ __launch_bounds__(NTHR) void k_head_bwd(const float *__restrict__ dp_in, ObjP o, const float *__restrict__ ht, HeadP p, int M, int T, int D, int Hd, int C,
                                                   int want_grad, float *__restrict__ dp_ws, float *__restrict__ dp_out, float *__restrict__ dh_ws,
                                                   float *__restrict__ d_f, int accumulate)
{
    __shared__ float DP[RT * LDP], DH[RT * LDH];
    __shared__ double RS[2 * RT];
    const int r0 = blockIdx.x * RT, row = threadIdx.x >> 4, c = threadIdx.x & 15, gr = r0 + row;
    const bool valid = gr < M && c < C;
    float dp = 0.f;
    if (dp_in != nullptr) {
        if (valid) dp = dp_in[(long)gr * C + c];
    } else {
        double ae = 0.0, aa = 0.0;
        if (valid) {
            const int t = gr % T;
            const float *P = o.pred + (long)(gr - t) * C + c, *G = o.gt + (long)(gr - t) * C + c;       // the element's column of its clip, row stride C
            const double e = (double)P[(long)t * C] - (double)G[(long)t * C];
            ae = fabs(e);
            double k = 0.0;
#pragma unroll
            for (int s = 0; s < 3; s++) {                        // the acceleration rows a = t - 2, t - 1, t that contain row t, weights 1, -2, 1
                const int a = t - 2 + s;
                if (a < 0 || a + 2 >= T) continue;
                const double d = ((double)P[(long)a * C] - 2.0 * (double)P[(long)(a + 1) * C] + (double)P[(long)(a + 2) * C])
                               - ((double)G[(long)a * C] - 2.0 * (double)G[(long)(a + 1) * C] + (double)G[(long)(a + 2) * C]);
                k += (s == 1 ? -2.0 : 1.0) * sgn(d);
                if (s == 2) aa = fabs(d);                        // row a = t is summed by this thread alone
            }
            dp = (float)(o.c_pos * sgn(e) + o.c_acc * k);
        }
        ae = sum16(ae); aa = sum16(aa);
        if (c == 0) { RS[row] = ae; RS[RT + row] = aa; }
    }
    DP[row * LDP + c] = dp;
    if (valid) {
        if (dp_ws != nullptr) dp_ws[(long)gr * C + c] = dp;
        if (dp_out != nullptr) dp_out[(long)gr * C + c] = dp;
    }
    __syncthreads();
    if (dp_in == nullptr && o.tpart != nullptr && threadIdx.x < 2) {
        double s = 0.0;
        for (int r = 0; r < RT; r++) s += RS[threadIdx.x * RT + r];
        o.tpart[2 * (long)blockIdx.x + threadIdx.x] = s;
    }
    if (!want_grad) return;
    tile_gemm(DP, LDP, C, p.w2, Hd, 1, Hd, [&](int r, int cc, float v) {                        // d_a = d_pred W2, then through the activation
        const int g = r0 + r;
        const float hv = g < M ? ht[(long)g * Hd + cc] : 0.f;
        const float dh = v * (hv > 0.f ? 1.f : 0.01f);
        DH[r * LDH + cc] = dh;
        if (g < M) dh_ws[(long)g * Hd + cc] = dh;
    });
    if (d_f == nullptr) return;
    __syncthreads();
    tile_gemm(DH, LDH, Hd, p.w1, D, 1, D, [&](int r, int cc, float v) {                         // d_f = d_h W1
        if (r0 + r < M) { const long i = (long)(r0 + r) * D + cc; d_f[i] = accumulate ? d_f[i] + v : v; }
    });
}

// ---- sums over the M rows --------------------------------------------------------------------------------------------------------------------------------------
// dW (N x K) = sum_rows G[row, :N]^T A[row, :K] (leaky: of the leaky_relu of A): one partial per chunk of CHUNK rows (fp32 MFMA accumulation inside a chunk),
// part[chunk][N][K]; N and K are ragged: operands past them read as zero and nothing is stored there
struct WgradP { const float *G, *A; float *part; int ldg, lda, N, K, tile0, leaky; };
struct WgradTab { WgradP p[MAXPROB]; int n, tiles; };
__global__ __launch_bounds__(NTHR) void k_wgrad(WgradTab tab, int M)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, q = lane >> 4;
    const int tile = blockIdx.x * NWAVE + wave, chunk = blockIdx.y;
    if (tile >= tab.tiles) return;
    int pi = 0;
    for (int i = 1; i < tab.n; i++) if (tile >= tab.p[i].tile0) pi = i;
    const float *G = tab.p[pi].G, *A = tab.p[pi].A;
    float *part = tab.p[pi].part;
    const int ldg = tab.p[pi].ldg, lda = tab.p[pi].lda, N = tab.p[pi].N, K = tab.p[pi].K, lt = tile - tab.p[pi].tile0, leaky = tab.p[pi].leaky;
    const int nkt = (K + 15) / 16, nt = lt / nkt, kt = lt - nt * nkt;
    const int m0 = chunk * CHUNK, m1 = min(M, m0 + CHUNK);
    const int gc = nt * 16 + j, ac = kt * 16 + j;
    const bool gv = gc < N, av = ac < K;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acc1 = acc, acc2 = acc, acc3 = acc;
    auto step = [&](int m, f32x4 c) {
        const int r = m + q;
        const bool v = r < m1;
        float a = (v && av) ? A[(long)r * lda + ac] : 0.f;
        if (leaky) a = a > 0.f ? a : 0.01f * a;
        return IFH_MFMA16((v && gv) ? G[(long)r * ldg + gc] : 0.f, a, c);
    };
    for (int m = m0; m < m1; m += 16) {                          // four independent chains over the rows mod 16; rows from m1 on read as zero
        acc = step(m, acc); acc1 = step(m + 4, acc1); acc2 = step(m + 8, acc2); acc3 = step(m + 12, acc3);
    }
    acc = (acc + acc1) + (acc2 + acc3);
    float *o = part + (long)chunk * N * K;
    if (av) {
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (nt * 16 + 4 * q + i < N) o[(long)(nt * 16 + 4 * q + i) * K + ac] = acc[i];
    }
}

// column sums of a row-major matrix, fp64, one partial per chunk: part[chunk][N]
struct ColP { const float *S; double *part; int ld, N; };
struct ColTab { ColP p[MAXPROB]; };
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

// out[e] (+)= the chunk partials of e added in fp64 in chunk order, rounded once.  Block row nred (when term.out != NULL): the objective's two terms,
// lw (sum / count), the tile partials of a chunk added in tile order and the chunk sums in chunk order.
struct RedP { float *out; const float *fpart; const double *dpart; int n; };
struct RedTab { RedP p[2 * MAXPROB]; };
struct TermP { const double *tpart; double *out; int ntiles; double cnt[2], lw[2]; };
__global__ __launch_bounds__(NTHR) void k_reduce(RedTab tab, int nred, TermP term, int nchunk, int accumulate)
{
    if ((int)blockIdx.y == nred) {
        if (blockIdx.x != 0 || threadIdx.x >= 2) return;
        const int w = threadIdx.x;
        double s = 0.0;
        for (int t0 = 0; t0 < term.ntiles; t0 += TPC) {
            double sc = 0.0;
            for (int t = t0; t < min(term.ntiles, t0 + TPC); t++) sc += term.tpart[2 * (long)t + w];
            s += sc;
        }
        term.out[w] = term.lw[w] * (s / term.cnt[w]);
        return;
    }
    const RedP P = tab.p[blockIdx.y];
    const int e = blockIdx.x * NTHR + threadIdx.x;
    if (e >= P.n) return;
    double s = 0.0;
    if (P.fpart != nullptr) for (int ch = 0; ch < nchunk; ch++) s += (double)P.fpart[(long)ch * P.n + e];
    else for (int ch = 0; ch < nchunk; ch++) s += P.dpart[(long)ch * P.n + e];
    P.out[e] = accumulate ? P.out[e] + (float)s : (float)s;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------------------------
static inline long nchunks(long M) { return (M + CHUNK - 1) / CHUNK; }
static inline long ntiles(long M) { return (M + RT - 1) / RT; }
static inline bool aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

static inline bool head_ok(long B, long T, long D, long Hd, long C)
{
    return B >= 1 && T >= 3 && B * T <= MAXM && D >= 16 && D <= MAXD && D % 16 == 0 && Hd >= 16 && Hd <= MAXH && Hd % 16 == 0 && C >= 1 && C <= MAXC;
}
static inline bool proj_ok(const int *kin, const int *n, int nprob, long M)
{
    if (kin == nullptr || n == nullptr || nprob < 1 || nprob > MAXPROB || M < 1 || M > MAXM) return false;
    for (int i = 0; i < nprob; i++)
        if (kin[i] < 1 || kin[i] > MAXD || n[i] < 16 || n[i] > MAXD || n[i] % 16) return false;
    return true;
}

// the sums of a backward: weight-gradient, column-sum and reduction tables filled problem by problem, partials carved from the workspace
struct Sums {
    WgradTab wt = {}; ColTab ct = {}; RedTab rt = {};
    int ncol = 0, nred = 0, maxn = 0;
    long nc = 0;
    double *colp = nullptr; float *wpart = nullptr;
    void add_w(const float *G, int ldg, int N, const float *A, int lda, int K, int leaky, float *out)
    {
        WgradP &q = wt.p[wt.n++];
        q.G = G; q.A = A; q.ldg = ldg; q.lda = lda; q.N = N; q.K = K; q.leaky = leaky; q.part = wpart; q.tile0 = wt.tiles;
        wt.tiles += ((N + 15) / 16) * ((K + 15) / 16);
        RedP &r = rt.p[nred++];
        r.out = out; r.fpart = wpart; r.dpart = nullptr; r.n = N * K;
        wpart += nc * N * K; maxn = r.n > maxn ? r.n : maxn;
    }
    void add_c(const float *S, int ld, int N, float *out)
    {
        ColP &q = ct.p[ncol++];
        q.S = S; q.ld = ld; q.N = N; q.part = colp;
        RedP &r = rt.p[nred++];
        r.out = out; r.fpart = nullptr; r.dpart = colp; r.n = N;
        colp += nc * N; maxn = N > maxn ? N : maxn;
    }
    int run(long M, const TermP &term, int accumulate, hipStream_t st)
    {
        const bool terms = term.out != nullptr;
        if (wt.n > 0) { k_wgrad<<<dim3((wt.tiles + NWAVE - 1) / NWAVE, (unsigned)nc), NTHR, 0, st>>>(wt, (int)M); VT_LAUNCH_CHECK(); }
        if (ncol > 0) { k_colsum<<<dim3(ncol, (unsigned)nc), NTHR, 0, st>>>(ct, (int)M); VT_LAUNCH_CHECK(); }
        if (nred > 0 || terms) {
            k_reduce<<<dim3(maxn > 0 ? (maxn + NTHR - 1) / NTHR : 1, nred + (terms ? 1 : 0)), NTHR, 0, st>>>(rt, nred, term, (int)nc, accumulate);
            VT_LAUNCH_CHECK();
        }
        return VT_OK;
    }
};

// the workspace of the head: fp64 first (tile partials of the objective, column-sum partials), then d_pred and d_h as row matrices, then the weight partials
struct HeadWs { long doubles, total_floats; };
static inline HeadWs head_ws(long M, long D, long Hd, long C)
{
    HeadWs l;
    const long nc = nchunks(M);
    l.doubles = 2 * ntiles(M) + nc * (C + Hd);
    l.total_floats = 2 * l.doubles + M * (C + Hd) + nc * (C * Hd + Hd * D);
    return l;
}

static TermP make_term(const double *tpart, double *out, long B, long T, long C, double lw_pose, double lw_accel)
{
    TermP t;
    t.tpart = tpart; t.out = out; t.ntiles = (int)ntiles(B * T);
    t.cnt[0] = (double)(B * T * C); t.cnt[1] = (double)(B * (T - 2) * C); t.lw[0] = lw_pose; t.lw[1] = lw_accel;
    return t;
}

}  // namespace ifh

using namespace ifh;

#define IFH_HEAD_SHAPES "T >= 3, B T <= 2^24, D %% 16 == 0 in 16 .. 160, hidden %% 16 == 0 in 16 .. 64, out_dim in 1 .. 16"
#define IFH_PROJ_SHAPES "1 .. 4 problems, M in 1 .. 2^24, Kin in 1 .. 160, N %% 16 == 0 in 16 .. 160"

extern "C" long vt_infill_proj_workspace_floats(const int *kin, const int *n, int nprob, long M)
{
    if (!proj_ok(kin, n, nprob, M)) return -1;
    long per = 0;
    for (int i = 0; i < nprob; i++) per += 2L * n[i] + (long)n[i] * kin[i];
    return nchunks(M) * per;
}

extern "C" int vt_infill_proj_forward(const float *const *xs, const float *const *weights, const float *const *biases, const int *kin, const int *n, int nprob,
                                      long M, float *const *ys, void *stream)
{
    VT_REQUIRE(proj_ok(kin, n, nprob, M), "vt_infill_proj_forward: unsupported shape (" IFH_PROJ_SHAPES ")");
    VT_REQUIRE(xs && weights && biases && ys, "vt_infill_proj_forward: NULL xs / weights / biases / ys");
    ProjTab tab = {};
    int tiles = 0;
    for (int i = 0; i < nprob; i++) {
        VT_REQUIRE(xs[i] && weights[i] && biases[i] && ys[i], "vt_infill_proj_forward: NULL pointer in problem %d", i);
        tab.p[i] = ProjP{xs[i], weights[i], biases[i], ys[i], kin[i], n[i], tiles};
        tiles += (int)ntiles(M);
    }
    tab.n = nprob;
    k_proj_fwd<<<tiles, NTHR, 0, vt_stream(stream)>>>(tab, (int)M);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

extern "C" int vt_infill_proj_backward(const float *const *d_ys, const float *const *xs, const int *kin, const int *n, int nprob, long M, float *const *d_weights,
                                       float *const *d_biases, int accumulate, float *workspace, void *stream)
{
    VT_REQUIRE(proj_ok(kin, n, nprob, M), "vt_infill_proj_backward: unsupported shape (" IFH_PROJ_SHAPES ")");
    VT_REQUIRE(d_ys && xs && workspace, "vt_infill_proj_backward: NULL d_ys / xs / workspace");
    VT_REQUIRE(aligned(workspace, 8), "vt_infill_proj_backward: workspace not 8-byte aligned");
    Sums s;
    s.nc = nchunks(M);
    long cols = 0;
    for (int i = 0; i < nprob; i++) cols += n[i];
    s.colp = reinterpret_cast<double *>(workspace);
    s.wpart = workspace + 2 * s.nc * cols;
    for (int i = 0; i < nprob; i++) {
        VT_REQUIRE(d_ys[i] && xs[i], "vt_infill_proj_backward: NULL pointer in problem %d", i);
        if (d_weights && d_weights[i]) s.add_w(d_ys[i], n[i], n[i], xs[i], kin[i], kin[i], 0, d_weights[i]);
        if (d_biases && d_biases[i]) s.add_c(d_ys[i], n[i], n[i], d_biases[i]);
    }
    TermP none = {};
    return s.run(M, none, accumulate, vt_stream(stream));
}

extern "C" long vt_infill_head_workspace_floats(int B, int T, int D, int hidden, int out_dim)
{
    if (!head_ok(B, T, D, hidden, out_dim)) return -1;
    return head_ws((long)B * T, D, hidden, out_dim).total_floats;
}

static int head_params(const float *const *params, HeadP *p, const char *who)
{
    VT_REQUIRE(params && params[0] && params[1] && params[2] && params[3], "%s: NULL parameter (predictor weight 1, bias 1, weight 2, bias 2)", who);
    p->w1 = params[0]; p->b1 = params[1]; p->w2 = params[2]; p->b2 = params[3];
    return VT_OK;
}

extern "C" int vt_infill_head_forward(const float *f, const float *const *params, const float *gt, int B, int T, int D, int hidden, int out_dim, double lw_pose,
                                      double lw_accel, float *pred, float *h, double *terms, float *workspace, void *stream)
{
    VT_REQUIRE(head_ok(B, T, D, hidden, out_dim), "vt_infill_head_forward: unsupported shape B %d T %d D %d hidden %d out_dim %d (" IFH_HEAD_SHAPES ")", B, T, D,
               hidden, out_dim);
    VT_REQUIRE(f && pred, "vt_infill_head_forward: NULL f / pred");
    VT_REQUIRE(terms == nullptr || (gt && workspace), "vt_infill_head_forward: the objective's terms need gt and a workspace");
    VT_REQUIRE(aligned(workspace, 8) && aligned(terms, 8), "vt_infill_head_forward: workspace / terms not 8-byte aligned");
    HeadP p;
    if (int rc = head_params(params, &p, "vt_infill_head_forward")) return rc;
    const long M = (long)B * T;
    hipStream_t st = vt_stream(stream);
    k_head_fwd<<<(int)ntiles(M), NTHR, 0, st>>>(f, p, (int)M, D, hidden, out_dim, h, pred);
    VT_LAUNCH_CHECK();
    if (terms == nullptr) return VT_OK;
    double *tpart = reinterpret_cast<double *>(workspace);
    const ObjP o = {gt, pred, 0.0, 0.0, tpart};
    k_head_bwd<<<(int)ntiles(M), NTHR, 0, st>>>(nullptr, o, nullptr, p, (int)M, T, D, hidden, out_dim, 0, nullptr, nullptr, nullptr, nullptr, 0);
    VT_LAUNCH_CHECK();
    Sums s;
    s.nc = nchunks(M);
    return s.run(M, make_term(tpart, terms, B, T, out_dim, lw_pose, lw_accel), 0, st);
}

extern "C" int vt_infill_head_backward(const float *d_pred_in, const float *gt, const float *pred, const float *h, const float *f, const float *const *params, int B,
                                       int T, int D, int hidden, int out_dim, double lw_pose, double lw_accel, double upstream, double *terms, float *d_pred,
                                       float *d_f, float *const *d_params, int accumulate, float *workspace, void *stream)
{
    VT_REQUIRE(head_ok(B, T, D, hidden, out_dim), "vt_infill_head_backward: unsupported shape B %d T %d D %d hidden %d out_dim %d (" IFH_HEAD_SHAPES ")", B, T, D,
               hidden, out_dim);
    VT_REQUIRE(h && f && workspace, "vt_infill_head_backward: NULL h / f / workspace");
    VT_REQUIRE(d_pred_in || (gt && pred), "vt_infill_head_backward: without a given d_pred the objective needs gt and pred");
    VT_REQUIRE(d_pred_in == nullptr || terms == nullptr, "vt_infill_head_backward: the objective's terms are not formed when d_pred is given");
    VT_REQUIRE(aligned(workspace, 8) && aligned(terms, 8), "vt_infill_head_backward: workspace / terms not 8-byte aligned");
    HeadP p;
    if (int rc = head_params(params, &p, "vt_infill_head_backward")) return rc;
    const long M = (long)B * T, C = out_dim, Hd = hidden;
    const HeadWs wl = head_ws(M, D, Hd, C);
    double *tpart = reinterpret_cast<double *>(workspace);
    float *dp_ws = workspace + 2 * wl.doubles, *dh_ws = dp_ws + M * C;
    Sums s;
    s.nc = nchunks(M);
    s.colp = tpart + 2 * ntiles(M);
    s.wpart = dh_ws + M * Hd;
    const ObjP o = {gt, pred, upstream * (lw_pose / (double)(M * C)), upstream * (lw_accel / (double)((long)B * (T - 2) * C)), terms ? tpart : nullptr};
    hipStream_t st = vt_stream(stream);
    k_head_bwd<<<(int)ntiles(M), NTHR, 0, st>>>(d_pred_in, o, h, p, (int)M, T, D, hidden, out_dim, 1, d_pred_in ? nullptr : dp_ws, d_pred, dh_ws, d_f, accumulate);
    VT_LAUNCH_CHECK();
    const float *dp = d_pred_in ? d_pred_in : dp_ws;
    if (d_params != nullptr) {                                   // parameter order: weight 1 (hidden, D), bias 1, weight 2 (out_dim, hidden), bias 2
        if (d_params[0]) s.add_w(dh_ws, hidden, hidden, f, D, D, 0, d_params[0]);
        if (d_params[1]) s.add_c(dh_ws, hidden, hidden, d_params[1]);
        if (d_params[2]) s.add_w(dp, out_dim, out_dim, h, hidden, hidden, 1, d_params[2]);
        if (d_params[3]) s.add_c(dp, out_dim, out_dim, d_params[3]);
    }
    TermP term = {};
    if (terms) term = make_term(tpart, terms, B, T, out_dim, lw_pose, lw_accel);
    return s.run(M, term, accumulate, st);
}
