// misc.hip -- the single-purpose small ops of the fit step, one launch each: landmark regressors, priors, SO(3) projection, rigid transform,
// temporal stencils, keypoint terms, Adam, loss reduction with the device-side early stop.  All HBM-bound and tiny next to the point query; the
// design goal is "one launch each, no host sync, deterministic gradients".  What each kernel computes per element is stated in step_ops.h,
// shared with the fused step kernels of step.hip.
#include "step_ops.h"

thread_local char vt_err_buf[512] = {0};
extern "C" const char *vt_last_error(void) { return vt_err_buf; }
extern "C" int vt_version(void) { return 1; }

// ---------------------------------------------------------------------------------------------------
// utilities
// ---------------------------------------------------------------------------------------------------
__global__ void fill_kernel(float *p, long n, float v) { long i = (long)blockIdx.x * blockDim.x + threadIdx.x; if (i < n) p[i] = v; }
__global__ void fill64_kernel(double *p, long n, double v) { long i = (long)blockIdx.x * blockDim.x + threadIdx.x; if (i < n) p[i] = v; }

extern "C" int vt_fill(float *p, long n, float value, void *stream)
{
    VT_REQUIRE(p && n > 0, "vt_fill: bad argument");
    hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, vt_stream(stream), p, n, value);
    VT_LAUNCH_CHECK();
    return VT_OK;
}
extern "C" int vt_fill_f64(double *p, long n, double value, void *stream)
{
    VT_REQUIRE(p && n > 0, "vt_fill_f64: bad argument");
    hipLaunchKernelGGL(fill64_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, vt_stream(stream), p, n, value);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

__global__ __launch_bounds__(256) void sum_to_term_kernel(const float *v, int n, float scale, double *term)
{
    __shared__ double red[4];
    double s = 0;
    for (int i = threadIdx.x; i < n; i += 256) s += (double)v[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(term, (red[0] + red[1] + red[2] + red[3]) * (double)scale);
}
extern "C" int vt_sum_to_term(const float *value, int n, float scale, double *term, void *stream)
{
    VT_REQUIRE(value && term && n > 0, "vt_sum_to_term: bad argument");
    hipLaunchKernelGGL(sum_to_term_kernel, dim3(1), dim3(256), 0, vt_stream(stream), value, n, scale, term);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

// ---------------------------------------------------------------------------------------------------
// landmark regressors: a wave per (landmark, frame) forward, a thread per (vertex, frame) backward
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void landmarks_fwd_kernel(const int *indptr, const int *indices, const float *data,
                                                           const float *verts, int V, int K, float *out)
{
    const int k = blockIdx.x, b = blockIdx.y;
    float a[3];
    landmark_row(indptr, indices, data, verts, b, V, k, threadIdx.x, a);
    if (threadIdx.x == 0) { float *o = out + ((size_t)b * K + k) * 3; o[0] = a[0]; o[1] = a[1]; o[2] = a[2]; }
}

__global__ void landmarks_bwd_kernel(const int *colptr, const int *rowidx, const float *cdata, const float *dout,
                                     int V, int K, int B, float *dverts, int accumulate)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (v >= V) return;
    landmark_col(colptr, rowidx, cdata, dout, (size_t)b * K, v, accumulate, dverts + ((size_t)b * V + v) * 3);
}

extern "C" int vt_landmarks_create(vt_landmarks **out, const int *indptr, const int *indices, const float *data, int K, int V, void *stream)
{
    VT_REQUIRE(out && indptr && indices && data && K > 0 && V > 0, "vt_landmarks_create: bad argument");
    hipStream_t st = vt_stream(stream);
    const int nnz = indptr[K];
    int *colptr = new int[V + 1](), *rowidx = new int[nnz]; float *cdata = new float[nnz];
    for (int e = 0; e < nnz; e++) { VT_REQUIRE(indices[e] >= 0 && indices[e] < V, "vt_landmarks_create: column index out of range"); colptr[indices[e] + 1]++; }
    for (int v = 0; v < V; v++) colptr[v + 1] += colptr[v];
    int *fillp = new int[V];
    memcpy(fillp, colptr, sizeof(int) * V);
    for (int k = 0; k < K; k++) for (int e = indptr[k]; e < indptr[k + 1]; e++) { const int p = fillp[indices[e]]++; rowidx[p] = k; cdata[p] = data[e]; }
    vt_landmarks *h = new vt_landmarks(); h->K = K; h->V = V;
    int rc;
    if ((rc = vt_upload(&h->indptr, indptr, (size_t)K + 1, st)) || (rc = vt_upload(&h->indices, indices, (size_t)nnz, st)) ||
        (rc = vt_upload(&h->data, data, (size_t)nnz, st)) || (rc = vt_upload(&h->colptr, colptr, (size_t)V + 1, st)) ||
        (rc = vt_upload(&h->rowidx, rowidx, (size_t)nnz, st)) || (rc = vt_upload(&h->cdata, cdata, (size_t)nnz, st))) return rc;
    VT_HIP(hipStreamSynchronize(st));
    delete[] colptr; delete[] rowidx; delete[] cdata; delete[] fillp;
    *out = h;
    return VT_OK;
}
extern "C" void vt_landmarks_destroy(vt_landmarks *h)
{
    if (!h) return;
    hipFree(h->indptr); hipFree(h->indices); hipFree(h->data); hipFree(h->colptr); hipFree(h->rowidx); hipFree(h->cdata);
    delete h;
}
extern "C" int vt_landmarks_forward(const vt_landmarks *h, const float *verts, int B, float *out, void *stream)
{
    VT_REQUIRE(h && verts && out && B > 0, "vt_landmarks_forward: bad argument");
    hipLaunchKernelGGL(landmarks_fwd_kernel, dim3(h->K, B), dim3(64), 0, vt_stream(stream), h->indptr, h->indices, h->data, verts, h->V, h->K, out);
    VT_LAUNCH_CHECK();
    return VT_OK;
}
extern "C" int vt_landmarks_backward(const vt_landmarks *h, const float *dout, int B, float *dverts, int accumulate, void *stream)
{
    VT_REQUIRE(h && dout && dverts && B > 0, "vt_landmarks_backward: bad argument");
    hipLaunchKernelGGL(landmarks_bwd_kernel, dim3((h->V + 255) / 256, B), dim3(256), 0, vt_stream(stream), h->colptr, h->rowidx, h->cdata, dout,
                       h->V, h->K, B, dverts, accumulate);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

// ---------------------------------------------------------------------------------------------------
// Mahalanobis priors: a 64-thread workgroup per frame
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void mahalanobis_kernel(const float *x, int stride, int off, int n, const float *mean,
                                                         const float *prec, float *value, float *dx, float gscale)
{
    __shared__ float d[64], t2[64];
    const int b = blockIdx.x;
    const float val = mahalanobis_value(x + (size_t)b * stride + off, n, mean, prec, d, t2);
    if (threadIdx.x == 0) value[b] = val;
    __syncthreads();
    if (dx) mahalanobis_grad(t2, n, prec, dx + (size_t)b * stride + off, gscale);
}
extern "C" int vt_mahalanobis(const float *x, int B, int stride, int off, int n, const float *mean, const float *prec,
                              float *value, float *dx, float gscale, void *stream)
{
    VT_REQUIRE(x && mean && prec && value && B > 0 && n > 0 && n <= 64 && off >= 0 && off + n <= stride, "vt_mahalanobis: bad argument (n must be <= 64)");
    hipLaunchKernelGGL(mahalanobis_kernel, dim3(B), dim3(64), 0, vt_stream(stream), x, stride, off, n, mean, prec, value, dx, gscale);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

// ---------------------------------------------------------------------------------------------------
// SO(3) projection and its VJP: one thread per matrix
// ---------------------------------------------------------------------------------------------------
__global__ void so3_fwd_kernel(const float *M0, const float *noise, int B, float *R)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float M[9]; Svd3 s;
    so3_input(M0, noise, b, M);
    svd3(M, s);
    so3_rotation(s, R + 9 * b);
}

__global__ void so3_bwd_kernel(const float *M0, const float *noise, int B, const float *dR, float *dM)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float M[9], G[9]; Svd3 s;
    so3_input(M0, noise, b, M);
#pragma unroll
    for (int e = 0; e < 9; e++) G[e] = dR[9 * b + e];
    svd3(M, s);
    so3_vjp(s, G, dM + 9 * b);
}

extern "C" int vt_so3_project_forward(const float *M0, const float *noise, int B, float *R, void *stream)
{
    VT_REQUIRE(M0 && R && B > 0, "vt_so3_project_forward: bad argument");
    hipLaunchKernelGGL(so3_fwd_kernel, dim3((B + 63) / 64), dim3(64), 0, vt_stream(stream), M0, noise, B, R);
    VT_LAUNCH_CHECK();
    return VT_OK;
}
extern "C" int vt_so3_project_backward(const float *M0, const float *noise, int B, const float *dR, float *dM, void *stream)
{
    VT_REQUIRE(M0 && dR && dM && B > 0, "vt_so3_project_backward: bad argument");
    hipLaunchKernelGGL(so3_bwd_kernel, dim3((B + 63) / 64), dim3(64), 0, vt_stream(stream), M0, noise, B, dR, dM);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

// ---------------------------------------------------------------------------------------------------
// rigid transform: a thread per point forward, a workgroup per frame backward
// ---------------------------------------------------------------------------------------------------
__global__ void rigid_fwd_kernel(const float *X0, int shared, const float *R, const float *t, const float *s, int B, int N, float *X)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (n >= N) return;
    rigid_point(X0 + ((shared ? 0 : (size_t)b * N) + n) * 3, R + 9 * b, t + 3 * b, s[b], X + ((size_t)b * N + n) * 3);
}

// twelve block sums one after the other (block_sum: a barrier pair each).  objstep_tail_kernel adds the same numbers in the same order behind ONE
// barrier pair; that form needs 4 x 12 floats of LDS and is not brought here (this kernel's LDS size is part of what profiles refer to).
__global__ __launch_bounds__(256) void rigid_bwd_kernel(const float *X0, int shared, const float *s, int N, const float *dX,
                                                        float *dR, float *dt, int accumulate)
{
    __shared__ float red[4];
    const int b = blockIdx.x;
    float a[12];
#pragma unroll
    for (int e = 0; e < 12; e++) a[e] = 0.f;
    const float sc = s[b];
    for (int n = threadIdx.x; n < N; n += 256) rigid_vjp_point<true>(X0 + ((shared ? 0 : (size_t)b * N) + n) * 3, dX + ((size_t)b * N + n) * 3, sc, a);
#pragma unroll
    for (int e = 0; e < 12; e++) {
        const float v = block_sum<4>(a[e], red);
        if (threadIdx.x == 0) {
            float *dst = (e < 9) ? dR + 9 * b + e : dt + 3 * b + (e - 9);
            *dst = accumulate ? *dst + v : v;
        }
    }
}

extern "C" int vt_rigid_forward(const float *X0, int shared_x0, const float *R, const float *t, const float *s, int B, int N, float *X, void *stream)
{
    VT_REQUIRE(X0 && R && t && s && X && B > 0 && N > 0, "vt_rigid_forward: bad argument");
    hipLaunchKernelGGL(rigid_fwd_kernel, dim3((N + 255) / 256, B), dim3(256), 0, vt_stream(stream), X0, shared_x0, R, t, s, B, N, X);
    VT_LAUNCH_CHECK();
    return VT_OK;
}
extern "C" int vt_rigid_backward(const float *X0, int shared_x0, const float *s, int B, int N, const float *dX, float *dR, float *dt,
                                 int accumulate, void *stream)
{
    VT_REQUIRE(X0 && s && dX && dR && dt && B > 0 && N > 0, "vt_rigid_backward: bad argument");
    hipLaunchKernelGGL(rigid_bwd_kernel, dim3(B), dim3(256), 0, vt_stream(stream), X0, shared_x0, s, N, dX, dR, dt, accumulate);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

// ---------------------------------------------------------------------------------------------------
// temporal stencils: thread == one ELEMENT, so every gradient element is written exactly once (no atomics) and the B frames are not walked
// serially (a thread-per-column walk was latency bound: 59 us).
// ---------------------------------------------------------------------------------------------------
// 1024 threads x at most 256 workgroups (round 6; was 256 x 512): every workgroup ends with ONE fp64 atomic on the term, and same-address atomics are
// performed one after the other at the memory side (~12 ns each: 512 of them were 6 of the kernel's 20 us; with 2048 workgroups the kernel took 33 us,
// with 4096 54 us) -- fewer, larger workgroups: 12.3 us at B = 96, D = 20670, `dv` bit-identical (profiles/r06_accel_loss_ab.txt)
#define ACCEL_T 1024
#define ACCEL_MAX_BLOCKS 256
__global__ __launch_bounds__(ACCEL_T) void accel_loss_kernel(const float *__restrict__ v, int B, int Dcols, int D, const float *__restrict__ elem_w,
                                                         float gs, double *term, float *__restrict__ dv)
{
    // D = row stride (floats per frame), Dcols = columns that take part
    __shared__ double red[ACCEL_T / 64];
    double acc = 0;
    // grid-stride over the elements: few blocks, so the fp64 atomics on the loss term (one per block, all arriving at the end) do not serialise
    // the tail of the kernel
    for (int t = blockIdx.x * ACCEL_T + threadIdx.x; t < B * Dcols; t += gridDim.x * ACCEL_T) {
        const int f = t / Dcols, i = t - f * Dcols;
        const float w = elem_w ? elem_w[i] : 1.f;
        float taps[5], g;
        stencil_taps(v, f, B, D, i, taps);
        acc += (double)accel_stencil(taps, f, B, w, gs, g);
        if (dv) dv[(size_t)f * D + i] += g;
    }
    term_add(acc / ((double)(B - 2) * Dcols), term, red);
}

__global__ __launch_bounds__(256) void velocity_loss_kernel(const float *__restrict__ v, int B, int D, float gs, double *term, float *__restrict__ dv)
{
    __shared__ double red[4];
    double acc = 0;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < B * D; t += gridDim.x * 256) {
        const int f = t / D, i = t - f * D;
        // (the 0.f of a neighbour outside the batch never reaches arithmetic: velocity_stencil drops that difference)
        const float vm1 = f >= 1 ? v[(size_t)(f - 1) * D + i] : 0.f, v0 = v[(size_t)f * D + i], vp1 = f + 1 < B ? v[(size_t)(f + 1) * D + i] : 0.f;
        float g;
        acc += (double)velocity_stencil(vm1, v0, vp1, f, B, gs, g);
        if (dv) dv[(size_t)f * D + i] += g;
    }
    term_add(acc / ((double)(B - 1) * D), term, red);
}

extern "C" int vt_accel_loss_strided(const float *v, int B, int D, int stride, const float *elem_w, float gscale, double *term, float *dv, void *stream)
{
    VT_REQUIRE(v && B >= 3 && D > 0 && stride >= D, "vt_accel_loss_strided: needs B >= 3 and stride >= D");
    // d/dv of mean(w a^2): 2 w a / cnt per stencil element; a's own coefficient 2 is folded in the kernel
    const float gs = 2.f * gscale / ((float)(B - 2) * (float)D);
    hipLaunchKernelGGL(accel_loss_kernel, dim3(min((B * D + ACCEL_T - 1) / ACCEL_T, ACCEL_MAX_BLOCKS)), dim3(ACCEL_T), 0, vt_stream(stream), v, B, D, stride, elem_w, gs, term, dv);
    VT_LAUNCH_CHECK();
    return VT_OK;
}
extern "C" int vt_accel_loss(const float *v, int B, int D, const float *elem_w, float gscale, double *term, float *dv, void *stream)
{
    VT_REQUIRE(v && B >= 3 && D > 0, "vt_accel_loss: needs B >= 3 (the reference returns NaN for empty stencils)");
    return vt_accel_loss_strided(v, B, D, D, elem_w, gscale, term, dv, stream);
}
extern "C" int vt_velocity_loss(const float *v, int B, int D, float gscale, double *term, float *dv, void *stream)
{
    VT_REQUIRE(v && B >= 2 && D > 0, "vt_velocity_loss: needs B >= 2");
    const float gs = 2.f * gscale / ((float)(B - 1) * (float)D);
    hipLaunchKernelGGL(velocity_loss_kernel, dim3(min((B * D + 255) / 256, 512)), dim3(256), 0, vt_stream(stream), v, B, D, gs, term, dv);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

// ---------------------------------------------------------------------------------------------------
// 2D keypoint terms: a thread per joint
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kpts_loss_kernel(const float *J, const float *kpts, const float *cc, int BK, int K, int mode, Cam5 cam,
                                                        float net_size, float gscale, float inv_cnt, double *term, float *dJ)
{
    __shared__ double red[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    double acc = 0;
    if (i < BK) acc = (double)kpts_term(J + 3 * i, kpts + 3 * i, cc, i / K, mode, cam, net_size, gscale, inv_cnt, dJ + 3 * i);
    term_add(acc * (double)inv_cnt, term, red);
}
extern "C" int vt_kpts_loss(const float *J, const float *kpts, const float *crop_center, int B, int K, int mode, const float *cam,
                            float net_size, float gscale, double *term, float *dJ, void *stream)
{
    VT_REQUIRE(J && kpts && cam && dJ && B > 0 && K > 0 && (mode == 0 || (mode == 1 && crop_center)), "vt_kpts_loss: bad argument");
    Cam5 c{cam[0], cam[1], cam[2], cam[3], cam[4]};
    const float inv_cnt = 1.f / (mode == 0 ? (float)(B * K * 2) : (float)(B * K));
    hipLaunchKernelGGL(kpts_loss_kernel, dim3((B * K + 255) / 256), dim3(256), 0, vt_stream(stream), J, kpts, crop_center, B * K, K, mode, c,
                       net_size, gscale, inv_cnt, term, dJ);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

__global__ __launch_bounds__(256) void sqdiff_loss_kernel(const float *a, int as, const float *b, int bs, int rows, int cols, float inv_denom,
                                                          float gscale, double *term, float *da)
{
    __shared__ double red[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    double acc = 0;
    if (i < rows * cols) {
        const int r = i / cols, c = i % cols;
        float g;
        acc = (double)sqdiff_elem(a[(size_t)r * as + c], b[(size_t)r * bs + c], inv_denom, gscale, g);
        if (da) da[(size_t)r * as + c] += g;
    }
    term_add(acc * (double)inv_denom, term, red);
}
extern "C" int vt_sqdiff_loss(const float *a, int a_stride, const float *b, int b_stride, int rows, int cols, float denom, float gscale,
                              double *term, float *da, void *stream)
{
    VT_REQUIRE(a && b && rows > 0 && cols > 0 && denom > 0, "vt_sqdiff_loss: bad argument");
    hipLaunchKernelGGL(sqdiff_loss_kernel, dim3((rows * cols + 255) / 256), dim3(256), 0, vt_stream(stream), a, a_stride, b, b_stride, rows, cols,
                       1.f / denom, gscale, term, da);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

// ---------------------------------------------------------------------------------------------------
// Adam + device-side early stop
// ---------------------------------------------------------------------------------------------------
__global__ void adam_kernel(float *p, const float *g, float *m, float *v, long n, float step_size, float bc2s, float beta1, float beta2,
                            float eps, const int *stop_flag)
{
    if (stop_flag && *stop_flag) return;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    adam_update(p[i], g[i], m[i], v[i], step_size, bc2s, beta1, beta2, eps);
}
extern "C" int vt_adam_step(float *p, const float *g, float *m, float *v, long n, int step, float lr, float beta1, float beta2, float eps,
                            const int *stop_flag, void *stream)
{
    VT_REQUIRE(p && g && m && v && n > 0 && step >= 1, "vt_adam_step: bad argument");
    double bc1; const float bc2s = adam_bias(beta1, beta2, step, &bc1);
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, vt_stream(stream), p, g, m, v, n, (float)(lr / bc1), bc2s, beta1, beta2, eps, stop_flag);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

// (B, cols) slices of wider tensors; the strides are `long` here (AdamSlice of the fused tails holds int strides)
__global__ void adam2d_kernel(float *p, long ps, const float *g, long gs, float *m, float *v, int rows, int cols, float step_size, float bc2s,
                              float beta1, float beta2, float eps, const int *stop_flag)
{
    if (stop_flag && *stop_flag) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * cols) return;
    const int r = i / cols, c = i % cols;
    adam_update(p[(size_t)r * ps + c], g[(size_t)r * gs + c], m[i], v[i], step_size, bc2s, beta1, beta2, eps);
}
extern "C" int vt_adam_step_2d(float *p, long p_stride, const float *g, long g_stride, float *m, float *v, int rows, int cols, int step, float lr,
                               float beta1, float beta2, float eps, const int *stop_flag, void *stream)
{
    VT_REQUIRE(p && g && m && v && rows > 0 && cols > 0 && step >= 1 && p_stride >= cols && g_stride >= cols, "vt_adam_step_2d: bad argument");
    double bc1; const float bc2s = adam_bias(beta1, beta2, step, &bc1);
    hipLaunchKernelGGL(adam2d_kernel, dim3((rows * cols + 255) / 256), dim3(256), 0, vt_stream(stream), p, p_stride, g, g_stride, m, v, rows, cols,
                       (float)(lr / bc1), bc2s, beta1, beta2, eps, stop_flag);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

__global__ void loss_reduce_kernel(const double *terms, TermW tw, int nterms, float tol, int armed, float *state, int *stop_flag,
                                   float *history, int slot)
{
    close_loss<false>(terms, tw, nterms, tol, armed, state, stop_flag, history, slot, stop_flag && *stop_flag);
}
extern "C" int vt_loss_reduce_and_stop(const double *terms, const float *w, int nterms, float tol, int armed, float *state, int *stop_flag,
                                       float *history, int slot, void *stream)
{
    VT_REQUIRE(terms && w && state && nterms > 0 && nterms <= 16, "vt_loss_reduce_and_stop: bad argument (nterms <= 16)");
    TermW tw; for (int k = 0; k < 16; k++) tw.w[k] = k < nterms ? w[k] : 0.f;
    hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(1), 0, vt_stream(stream), terms, tw, nterms, tol, armed, state, stop_flag, history, slot);
    VT_LAUNCH_CHECK();
    return VT_OK;
}
