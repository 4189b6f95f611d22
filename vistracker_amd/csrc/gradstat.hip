// gradstat.hip -- the device-side gradient record and the non-finite step guard of a training step (vt_grad_stats, vt_grad_guard_close, vt_grad_scale:
// include/vistracker.h).
//
// vt_grad_stats: per segment of a flat fp32 gradient, the number of NaN / +-Inf elements, the fp64 sum of g^2 over the FINITE elements (an fp32 value squared in
// fp64 is exact; a NaN therefore never erases the norm of the tensor it sits in) and the largest finite |g|.  No atomics, the same bits on every call:
//
//   * a segment is cut into chunks of CHUNK = 4096 elements counted from the segment's first element; the chunk size is this constant, never a function of the
//     launch.  ONE WAVE owns a chunk, so a bias of 128 values costs one wave, not a workgroup.
//   * inside a chunk, element e belongs to lane (e / 4) % 64, accumulator e % 4, and a lane adds its elements to an accumulator in ascending e.  The lane's four
//     accumulators are added as (a0 + a1) + (a2 + a3), the 64 lanes by the xor tree 32, 16, .. 1.  The assignment does not depend on where the buffer lies, so
//     moving it to another alignment changes the loads (16 bytes per lane when the chunk starts on a 16-byte boundary, four 4-byte loads of the SAME elements
//     otherwise) and never the order of the additions.  That is why there is no scalar head: a head would shift the assignment with the alignment.  The ragged end
//     of a segment's last chunk is loaded element by element, out-of-range lanes contribute +0.
//   * the chunk partials go to the workspace and a second kernel, one wave per segment, adds them in chunk order (fp64, left to right).
//   * max |g| is taken on the bit patterns (for finite floats the order of |x| is the order of its 31 low bits), so denormals count with their value whatever the
//     denormal mode; the fp64 conversion keeps them too (hipcc's default mode).
//
// Launches: index (one workgroup: chunk counts, their prefix sum, the chunk -> segment table; the offsets are clamped into [0, n] so that a bad table can make the
// results meaningless but never a load out of bounds), chunks, finish.
//
// vt_grad_guard_close: one wave closes the step from up to three buffers' results.  vt_grad_scale: the streaming shape of gradreduce.hip.
#include "common.h"
#include <cstdint>

namespace gst {

constexpr int CHUNK = VT_GRAD_STATS_CHUNK;     // elements per chunk
constexpr int THREADS = 256;                   // 4 waves, each on a chunk (or a segment) of its own: no LDS, no barrier
constexpr int WAVES = THREADS / 64;
constexpr int STEP = 256;                      // elements a wave covers per step: 64 lanes x 4
constexpr int INDEX_THREADS = 1024;
constexpr int SCALE_BLOCKS_PER_CU = 8;
static_assert(CHUNK % STEP == 0 && CHUNK / STEP == 16, "the full-chunk path is unrolled for 16 steps");

struct Workspace {
    double *psum; long *chunk_start; long *seg_lo; long *seg_hi; int *table; unsigned *pmax; int *pcnt; long max_chunks;
};

static inline long max_chunks_of(long n, int n_seg) { return n / CHUNK + n_seg; }      // sum over segments of ceil(len / CHUNK) <= floor(n / CHUNK) + n_seg

static inline size_t workspace_bytes(long n, int n_seg)
{
    const size_t M = (size_t)max_chunks_of(n, n_seg);
    const size_t b = 8 * M + 8 * ((size_t)n_seg + 1) + 16 * (size_t)n_seg + 12 * M;
    return (b + 15) / 16 * 16;
}

static inline Workspace carve(void *ws, long n, int n_seg)
{
    Workspace w;
    w.max_chunks = max_chunks_of(n, n_seg);
    char *p = static_cast<char *>(ws);
    w.psum = reinterpret_cast<double *>(p); p += 8 * w.max_chunks;
    w.chunk_start = reinterpret_cast<long *>(p); p += 8 * ((long)n_seg + 1);
    w.seg_lo = reinterpret_cast<long *>(p); p += 8 * (long)n_seg;
    w.seg_hi = reinterpret_cast<long *>(p); p += 8 * (long)n_seg;
    w.table = reinterpret_cast<int *>(p); p += 4 * w.max_chunks;
    w.pmax = reinterpret_cast<unsigned *>(p); p += 4 * w.max_chunks;
    w.pcnt = reinterpret_cast<int *>(p);
    return w;
}

// ---- index: chunk_start[s] = number of chunks of the segments before s, seg_lo / seg_hi the clamped bounds, table[chunk] = its segment ----------------------
__global__ __launch_bounds__(INDEX_THREADS) void index_kernel(const long *seg_off, long n, int n_seg, Workspace w)
{
    __shared__ long sh[INDEX_THREADS];
    __shared__ long carry;
    const int t = threadIdx.x;
    if (t == 0) carry = 0;
    __syncthreads();
    for (int s0 = 0; s0 < n_seg; s0 += INDEX_THREADS) {
        const int s = s0 + t;
        long nch = 0;
        if (s < n_seg) {
            long lo = seg_off[2 * s], hi = seg_off[2 * s + 1];
            lo = lo < 0 ? 0 : (lo > n ? n : lo);
            hi = hi < lo ? lo : (hi > n ? n : hi);
            w.seg_lo[s] = lo; w.seg_hi[s] = hi;
            nch = (hi - lo + CHUNK - 1) / CHUNK;
        }
        sh[t] = nch;
        __syncthreads();
        for (int o = 1; o < INDEX_THREADS; o <<= 1) {          // inclusive scan
            const long add = t >= o ? sh[t - o] : 0;
            __syncthreads();
            sh[t] += add;
            __syncthreads();
        }
        const long base = carry;
        if (s < n_seg) w.chunk_start[s] = base + sh[t] - nch;
        __syncthreads();
        if (t == INDEX_THREADS - 1) carry = base + sh[t];
        __syncthreads();
    }
    if (t == 0) w.chunk_start[n_seg] = carry;
    __syncthreads();                                           // chunk_start is read back below by other threads of this workgroup
    const int wave = t >> 6, lane = t & 63;
    for (int s = wave; s < n_seg; s += INDEX_THREADS / 64) {
        const long start = w.chunk_start[s], cnt = w.chunk_start[s + 1] - start;
        for (long c = lane; c < cnt; c += 64)
            if (start + c < w.max_chunks) w.table[start + c] = s;      // holds for ascending offsets; a table that is not ascending is cut here
    }
}

// ---- one element into a lane's accumulators -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void take(float x, double &s, unsigned &mx, int &cnt)
{
    const unsigned a = __float_as_uint(x) & 0x7fffffffu;
    const bool finite = a < 0x7f800000u;
    const double d = (double)(finite ? x : 0.f);
    s += d * d;
    mx = finite && a > mx ? a : mx;
    cnt += finite ? 0 : 1;
}

__device__ __forceinline__ double readlane_f64(double v, int lane)
{
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane), lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    return __hiloint2double(hi, lo);
}

// ---- chunks: one wave per chunk -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void chunk_kernel(const float *g, int n_seg, Workspace w)
{
    const long item = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * WAVES + (threadIdx.x >> 6)));
    long total = w.chunk_start[n_seg];
    if (total > w.max_chunks) total = w.max_chunks;
    if (item >= total) return;
    const int lane = threadIdx.x & 63;
    const int s = w.table[item];
    const long lo = w.seg_lo[s], hi = w.seg_hi[s];
    const long base = lo + (item - w.chunk_start[s]) * CHUNK;
    const long left = hi - base;
    if (left <= 0) return;                                     // cannot happen with the index kernel's table; guards the loads below all the same
    const int m = left < CHUNK ? (int)left : CHUNK;
    const float *p = g + base;
    const bool aligned = (reinterpret_cast<uintptr_t>(p) & 15) == 0;

    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    unsigned mx = 0;
    int cnt = 0;
    if (m == CHUNK && aligned) {
        // a whole chunk on a 16-byte boundary: 16 loads of 16 bytes per lane, eight in flight
#pragma unroll
        for (int k0 = 0; k0 < CHUNK / STEP; k0 += 8) {
            float4 v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) v[k] = *reinterpret_cast<const float4 *>(p + (k0 + k) * STEP + 4 * lane);
#pragma unroll
            for (int k = 0; k < 8; k++) { take(v[k].x, a0, mx, cnt); take(v[k].y, a1, mx, cnt); take(v[k].z, a2, mx, cnt); take(v[k].w, a3, mx, cnt); }
        }
    } else {
        // the same elements in the same order: 16 bytes where the lane's four lie inside the chunk on a boundary, element by element otherwise
        const int steps = (m + STEP - 1) / STEP;
#pragma unroll 4
        for (int k = 0; k < steps; k++) {
            const int e = k * STEP + 4 * lane;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (aligned && e + 4 <= m) {
                v = *reinterpret_cast<const float4 *>(p + e);
            } else {
                if (e + 0 < m) v.x = p[e + 0];
                if (e + 1 < m) v.y = p[e + 1];
                if (e + 2 < m) v.z = p[e + 2];
                if (e + 3 < m) v.w = p[e + 3];
            }
            take(v.x, a0, mx, cnt); take(v.y, a1, mx, cnt); take(v.z, a2, mx, cnt); take(v.w, a3, mx, cnt);
        }
    }
    double sum = (a0 + a1) + (a2 + a3);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o, 64);
        const unsigned om = (unsigned)__shfl_xor((int)mx, o, 64);
        mx = om > mx ? om : mx;
        cnt += __shfl_xor(cnt, o, 64);
    }
    if (lane == 0) { w.psum[item] = sum; w.pmax[item] = mx; w.pcnt[item] = cnt; }
}

// ---- finish: one wave per segment adds the chunk partials in chunk order -----------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void finish_kernel(int n_seg, Workspace w, double *sumsq, float *maxabs, int *nonfinite)
{
    const int s = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * WAVES + (threadIdx.x >> 6)));
    if (s >= n_seg) return;
    const int lane = threadIdx.x & 63;
    const long start = w.chunk_start[s];
    long cnt = w.chunk_start[s + 1] - start;
    if (start + cnt > w.max_chunks) cnt = w.max_chunks > start ? w.max_chunks - start : 0;
    double tot = 0.0;
    unsigned mx = 0;
    int nf = 0;
    for (long b = 0; b < cnt; b += 64) {
        const long i = b + lane;
        const bool in = i < cnt;
        const double ps = in ? w.psum[start + i] : 0.0;        // +0 past the end: adding it changes nothing
        const unsigned pm = in ? w.pmax[start + i] : 0u;
        nf += in ? w.pcnt[start + i] : 0;
        mx = pm > mx ? pm : mx;
#pragma unroll
        for (int j = 0; j < 64; j++) tot += readlane_f64(ps, j);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned om = (unsigned)__shfl_xor((int)mx, o, 64);
        mx = om > mx ? om : mx;
        nf += __shfl_xor(nf, o, 64);
    }
    if (lane == 0) { sumsq[s] = tot; maxabs[s] = __uint_as_float(mx); nonfinite[s] = nf; }
}

// ---- close ------------------------------------------------------------------------------------------------------------------------------------------------
struct Stats { const double *sumsq; const float *maxabs; const int *nonfinite; int n_seg; };
struct CloseArgs { Stats b[3]; const double *error; double max_norm; char *record; int ring; int n_total; };

__device__ __forceinline__ bool finite_f64(double x)
{
    return (__double2hiint(x) & 0x7ff00000) != 0x7ff00000;
}

// one wave.  The record's layout is that of include/vistracker.h (VT_GUARD_*).
__global__ __launch_bounds__(64) void close_kernel(CloseArgs a)
{
    const int lane = threadIdx.x;
    double total = 0.0;
    int bad = 0;
    for (int k = 0; k < 3; k++) {
        const Stats st = a.b[k];
        for (int b = 0; b < st.n_seg; b += 64) {
            const int i = b + lane;
            const bool in = i < st.n_seg;
            const double ps = in ? st.sumsq[i] : 0.0;
            bad |= in && st.nonfinite[i] > 0 ? 1 : 0;
#pragma unroll
            for (int j = 0; j < 64; j++) total += readlane_f64(ps, j);         // index order, buffer after buffer
        }
    }
    const double error = a.error ? *a.error : 0.0;
    bad = __any(bad) || !finite_f64(error) ? 1 : 0;
    const double norm = sqrt(total);
    float coef = 1.f;
    if (a.max_norm > 0.0) {
        const double c = a.max_norm / (norm + 1e-6);
        coef = (float)(c < 1.0 ? c : 1.0);
    }
    long *head = reinterpret_cast<long *>(a.record);
    const long step = head[0];
    const long slot_bytes = VT_GUARD_SLOT_HEAD + 16L * a.n_total;
    char *slots[2] = {a.record + VT_GUARD_HEAD, a.ring > 0 ? a.record + VT_GUARD_HEAD + (1 + step % a.ring) * slot_bytes : nullptr};
    for (int d = 0; d < 2; d++) {
        char *sl = slots[d];
        if (!sl) continue;
        if (lane == 0) {
            *reinterpret_cast<double *>(sl + VT_GUARD_NORM) = norm;
            *reinterpret_cast<double *>(sl + VT_GUARD_ERROR) = error;
            *reinterpret_cast<float *>(sl + VT_GUARD_COEF) = coef;
            *reinterpret_cast<int *>(sl + VT_GUARD_SKIP) = bad;
            *reinterpret_cast<long *>(sl + VT_GUARD_STEP) = step;
        }
        double *o_s = reinterpret_cast<double *>(sl + VT_GUARD_SLOT_HEAD);
        float *o_m = reinterpret_cast<float *>(sl + VT_GUARD_SLOT_HEAD + 8L * a.n_total);
        int *o_c = reinterpret_cast<int *>(sl + VT_GUARD_SLOT_HEAD + 12L * a.n_total);
        int at = 0;
        for (int k = 0; k < 3; k++) {
            const Stats st = a.b[k];
            for (int i = lane; i < st.n_seg; i += 64) { o_s[at + i] = st.sumsq[i]; o_m[at + i] = st.maxabs[i]; o_c[at + i] = st.nonfinite[i]; }
            at += st.n_seg;
        }
    }
    if (lane == 0) { head[0] = step + 1; head[1] += bad; }
}

// ---- scale: g *= *coef unless *skip; [0, head) and [head + 4 nvec, n) scalar, the body 16 bytes per access --------------------------------------------------
__global__ __launch_bounds__(THREADS) void scale_kernel(float *g, size_t n, const float *coef, const int *skip, size_t head, size_t nvec)
{
    if (skip && *skip) return;
    const float c = *coef;
    if (c == 1.f) return;                                      // x * 1 is x for every x: nothing to stream
    const size_t tid = (size_t)blockIdx.x * THREADS + threadIdx.x;
    const size_t nthreads = (size_t)gridDim.x * THREADS;
    const size_t tail0 = head + 4 * nvec;
    for (size_t q = tid; q < nvec; q += nthreads) {
        float4 *p = reinterpret_cast<float4 *>(g + head + 4 * q);
        float4 v = *p;
        v.x *= c; v.y *= c; v.z *= c; v.w *= c;
        *p = v;
    }
    const size_t nscalar = head + (n - tail0);
    for (size_t k = tid; k < nscalar; k += nthreads) {
        const size_t i = k < head ? k : tail0 + (k - head);
        g[i] *= c;
    }
}

}  // namespace gst

extern "C" long vt_grad_stats_workspace_bytes(long n, int n_seg)
{
    if (n < 0 || n_seg < 0) return 0;
    return (long)gst::workspace_bytes(n, n_seg);
}

extern "C" int vt_grad_stats(const float *g, long n, const long *seg_off, int n_seg, double *sumsq, float *maxabs, int *nonfinite, void *ws, void *stream)
{
    VT_REQUIRE(n >= 0 && n_seg >= 0, "vt_grad_stats: n = %ld, n_seg = %d", n, n_seg);
    if (n_seg == 0) return VT_OK;
    VT_REQUIRE(seg_off && sumsq && maxabs && nonfinite && ws, "vt_grad_stats: NULL pointer with n_seg = %d", n_seg);
    VT_REQUIRE(g || n == 0, "vt_grad_stats: NULL gradient with n = %ld", n);
    VT_REQUIRE(reinterpret_cast<uintptr_t>(g) % 4 == 0 && reinterpret_cast<uintptr_t>(ws) % 8 == 0, "vt_grad_stats: g must be 4-byte and ws 8-byte aligned");
    const gst::Workspace w = gst::carve(ws, n, n_seg);
    hipStream_t st = vt_stream(stream);
    hipLaunchKernelGGL(gst::index_kernel, dim3(1), dim3(gst::INDEX_THREADS), 0, st, seg_off, n, n_seg, w);
    VT_LAUNCH_CHECK();
    if (w.max_chunks > 0) {
        hipLaunchKernelGGL(gst::chunk_kernel, dim3((unsigned)((w.max_chunks + gst::WAVES - 1) / gst::WAVES)), dim3(gst::THREADS), 0, st, g, n_seg, w);
        VT_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(gst::finish_kernel, dim3((unsigned)((n_seg + gst::WAVES - 1) / gst::WAVES)), dim3(gst::THREADS), 0, st, n_seg, w, sumsq, maxabs, nonfinite);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

extern "C" long vt_grad_guard_record_bytes(int n_seg_total, int ring)
{
    if (n_seg_total < 0 || ring < 0) return 0;
    return VT_GUARD_HEAD + (1L + ring) * (VT_GUARD_SLOT_HEAD + 16L * n_seg_total);
}

extern "C" int vt_grad_guard_close(const double *sumsq0, const float *maxabs0, const int *nonfinite0, int n_seg0,
                                   const double *sumsq1, const float *maxabs1, const int *nonfinite1, int n_seg1,
                                   const double *sumsq2, const float *maxabs2, const int *nonfinite2, int n_seg2,
                                   const double *error, double max_norm, void *record, int ring, void *stream)
{
    gst::CloseArgs a;
    a.b[0] = {sumsq0, maxabs0, nonfinite0, n_seg0};
    a.b[1] = {sumsq1, maxabs1, nonfinite1, n_seg1};
    a.b[2] = {sumsq2, maxabs2, nonfinite2, n_seg2};
    a.n_total = 0;
    for (int k = 0; k < 3; k++) {
        const gst::Stats &s = a.b[k];
        VT_REQUIRE(s.n_seg >= 0 && (s.n_seg == 0 || (s.sumsq && s.maxabs && s.nonfinite)), "vt_grad_guard_close: buffer %d has %d segments and a NULL array", k, s.n_seg);
        a.n_total += s.n_seg;
    }
    VT_REQUIRE(record && reinterpret_cast<uintptr_t>(record) % 8 == 0 && ring >= 0, "vt_grad_guard_close: record must be an 8-byte aligned device pointer, ring >= 0");
    VT_REQUIRE(max_norm == max_norm, "vt_grad_guard_close: max_norm is NaN");
    a.error = error; a.max_norm = max_norm; a.record = static_cast<char *>(record); a.ring = ring;
    hipLaunchKernelGGL(gst::close_kernel, dim3(1), dim3(64), 0, vt_stream(stream), a);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

extern "C" int vt_grad_scale(float *g, long n, const float *coef, const int *skip, void *stream)
{
    VT_REQUIRE(n >= 0, "vt_grad_scale: n = %ld", n);
    if (n == 0) return VT_OK;
    VT_REQUIRE(g && coef, "vt_grad_scale: NULL pointer with n = %ld", n);
    const uintptr_t ga = reinterpret_cast<uintptr_t>(g);
    VT_REQUIRE(ga % 4 == 0, "vt_grad_scale: g must be 4-byte aligned");
    size_t head = ((16 - ga % 16) % 16) / 4;
    if (head > (size_t)n) head = (size_t)n;
    size_t nvec = ((size_t)n - head) / 4;
    if (nvec == 0) head = (size_t)n;
    int cus = 0;
    if (int rc = vt_cu_count(&cus)) return rc;
    const size_t nscalar = (size_t)n - 4 * nvec;
    const size_t work = nvec > nscalar ? nvec : nscalar;
    size_t blocks = (work + gst::THREADS - 1) / gst::THREADS;
    const size_t cap = (size_t)cus * gst::SCALE_BLOCKS_PER_CU;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(gst::scale_kernel, dim3((unsigned)blocks), dim3(gst::THREADS), 0, vt_stream(stream), g, (size_t)n, coef, skip, head, nvec);
    VT_LAUNCH_CHECK();
    return VT_OK;
}
