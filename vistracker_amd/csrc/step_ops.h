// step_ops.h -- every small operation of a fit step, stated ONCE for one element / point / frame.  The single-purpose kernels (misc.hip: the
// drop-in path and the VT_FUSED_STEPS=0 reference step) and the fused heads / tails (step.hip) call the same function, so "a fused step equals
// the single-purpose sequence bit for bit"  holds by construction for the arithmetic; what the kernels still own is the plumbing:
// who computes what, in which order, behind which barrier.  The library is built with -ffp-contract=off -fno-slp-vectorize: an expression
// written here is the same instruction sequence wherever it is inlined.
#pragma once
#include "common.h"

// block-level fp64 accumulate into a term: every thread contributes `s`
__device__ __forceinline__ void term_add(double s, double *term, double *red /* >= blockDim/64 doubles */)
{
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const int nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) { double t = 0; for (int i = 0; i < nw; i++) t += red[i]; if (term) atomicAdd(term, t); }
}

// landmark regressors (body_landmark.py:16-28; torch_functions.py:52-76)
// landmark k of frame b by one wave: lane-strided sum over the CSR row, then the wave tree (result in every lane)
__device__ __forceinline__ void landmark_row(const int *indptr, const int *indices, const float *data, const float *verts, int b, int V, int k, int lane, float *a)
{
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int e = indptr[k] + lane; e < indptr[k + 1]; e += 64) {
        const float w = data[e]; const float *v = verts + ((size_t)b * V + indices[e]) * 3;
        a0 += w * v[0]; a1 += w * v[1]; a2 += w * v[2];
    }
    a[0] = wave_sum(a0); a[1] = wave_sum(a1); a[2] = wave_sum(a2);
}

// VJP for vertex v by one thread: the CSC column against the landmark gradients dJ[row0 + row] (three floats each), set or added to o[0..2];
// an empty column leaves an accumulated-into gradient alone
__device__ __forceinline__ void landmark_col(const int *colptr, const int *rowidx, const float *cdata, const float *dJ, size_t row0, int v, int accumulate, float *o)
{
    const int s = colptr[v], e = colptr[v + 1];
    if (s == e && accumulate) return;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int i = s; i < e; i++) { const float w = cdata[i]; const float *g = dJ + (row0 + rowidx[i]) * 3; a0 += w * g[0]; a1 += w * g[1]; a2 += w * g[2]; }
    if (accumulate) { o[0] += a0; o[1] += a1; o[2] += a2; } else { o[0] = a0; o[1] = a1; o[2] = a2; }
}

// Mahalanobis prior (th_smpl_prior.py:30-38; th_hand_prior.py:57-72) of one frame by one 64-thread workgroup, thread j = column j:
// value = |(x - mean) P|^2 (returned in every thread); after a barrier, dx += 2 gscale P ((x - mean) P)^T from the t2 it left.  d, t2: 64 floats of LDS each.
__device__ __forceinline__ float mahalanobis_value(const float *x, int n, const float *mean, const float *prec, float *d, float *t2)
{
    const int j = threadIdx.x;
    d[j] = (j < n) ? x[j] - mean[j] : 0.f;
    __syncthreads();
    float a = 0.f;
    if (j < n) for (int i = 0; i < n; i++) a += d[i] * prec[i * n + j];
    t2[j] = a;
    return wave_sum(a * a);
}
__device__ __forceinline__ void mahalanobis_grad(const float *t2, int n, const float *prec, float *dx, float gscale)
{
    const int j = threadIdx.x;
    if (j >= n) return;
    float g = 0.f;
    for (int k = 0; k < n; k++) g += t2[k] * prec[j * n + k];
    dx[j] += 2.f * g * gscale;
}

// SO(3) projection (recon_fit_base.py:179-199): one thread per matrix, one-sided Jacobi SVD in registers.
// VJP in polar form: dM = U D Z V^T, Q = D U^T G V, Z_ij = (Q_ij - Q_ji)/(h_i + h_j), h = (s1, s2, d*s3)
// (the same derivative autograd takes through torch.svd/det, without its 1/(s_i^2 - s_j^2) cancellation).
struct Svd3 { float U[9], V[9], s[3], d; };
#define SVD_WS 22    /* floats per frame of the head -> tail hand-over: U, V, s, d */

__device__ __forceinline__ void jacobi_pair(float *A, float *V, const int p, const int q)
{
    float a = 0.f, b = 0.f, g = 0.f;
#pragma unroll
    for (int r = 0; r < 3; r++) { a += A[3 * r + p] * A[3 * r + p]; b += A[3 * r + q] * A[3 * r + q]; g += A[3 * r + p] * A[3 * r + q]; }
    if (fabsf(g) <= 1e-30f) return;
    const float zeta = (b - a) / (2.f * g);
    const float t = (zeta >= 0.f ? 1.f : -1.f) / (fabsf(zeta) + sqrtf(1.f + zeta * zeta));
    const float c = 1.f / sqrtf(1.f + t * t), sn = c * t;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        float x = A[3 * r + p], y = A[3 * r + q]; A[3 * r + p] = c * x - sn * y; A[3 * r + q] = sn * x + c * y;
        x = V[3 * r + p]; y = V[3 * r + q]; V[3 * r + p] = c * x - sn * y; V[3 * r + q] = sn * x + c * y;
    }
}

__device__ __forceinline__ void svd3(const float *M, Svd3 &o)
{
    float A[9], V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
#pragma unroll
    for (int e = 0; e < 9; e++) A[e] = M[e];
    for (int sweep = 0; sweep < 8; sweep++) { jacobi_pair(A, V, 0, 1); jacobi_pair(A, V, 0, 2); jacobi_pair(A, V, 1, 2); }
    float sv[3];
#pragma unroll
    for (int c = 0; c < 3; c++) sv[c] = sqrtf(A[c] * A[c] + A[3 + c] * A[3 + c] + A[6 + c] * A[6 + c]);
    // sort columns by singular value, descending (torch.svd order; the last one carries the det sign)
#define SWAPC(i, j)                                                                                          \
    if (sv[j] > sv[i]) {                                                                                     \
        float t_ = sv[i]; sv[i] = sv[j]; sv[j] = t_;                                                         \
        for (int r = 0; r < 3; r++) { t_ = A[3 * r + i]; A[3 * r + i] = A[3 * r + j]; A[3 * r + j] = t_;     \
                                      t_ = V[3 * r + i]; V[3 * r + i] = V[3 * r + j]; V[3 * r + j] = t_; }   \
    }
    SWAPC(0, 1) SWAPC(0, 2) SWAPC(1, 2)
#undef SWAPC
#pragma unroll
    for (int c = 0; c < 3; c++) {
        o.s[c] = sv[c];
        const float inv = sv[c] > 0.f ? 1.f / sv[c] : 0.f;
#pragma unroll
        for (int r = 0; r < 3; r++) { o.U[3 * r + c] = A[3 * r + c] * inv; o.V[3 * r + c] = V[3 * r + c]; }
    }
    // det(U V^T) = det(U) det(V)
    const float *U = o.U, *W = o.V;
    const float dU = U[0] * (U[4] * U[8] - U[5] * U[7]) - U[1] * (U[3] * U[8] - U[5] * U[6]) + U[2] * (U[3] * U[7] - U[4] * U[6]);
    const float dV = W[0] * (W[4] * W[8] - W[5] * W[7]) - W[1] * (W[3] * W[8] - W[5] * W[6]) + W[2] * (W[3] * W[7] - W[4] * W[6]);
    o.d = dU * dV;
}

// the matrix that is projected: frame b of M0 plus 1e-4 noise (the reference's guard against repeated singular values)
__device__ __forceinline__ void so3_input(const float *M0, const float *noise, int b, float *M)
{
#pragma unroll
    for (int e = 0; e < 9; e++) M[e] = M0[9 * b + e] + (noise ? 1e-4f * noise[9 * b + e] : 0.f);
}

// R = U diag(1, 1, d) V^T
__device__ __forceinline__ void so3_rotation(const Svd3 &s, float *R)
{
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) R[3 * r + c] = s.U[3 * r] * s.V[3 * c] + s.U[3 * r + 1] * s.V[3 * c + 1] + s.d * s.U[3 * r + 2] * s.V[3 * c + 2];
}

// dM from G = dL/dR, polar form (header of this section)
__device__ __forceinline__ void so3_vjp(const Svd3 &s, const float *G, float *dM)
{
    const float D[3] = {1.f, 1.f, s.d}, h[3] = {s.s[0], s.s[1], s.d * s.s[2]};
    float UtG[9], Q[9], Z[9], UDZ[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) UtG[3 * r + c] = s.U[r] * G[c] + s.U[3 + r] * G[3 + c] + s.U[6 + r] * G[6 + c];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) Q[3 * r + c] = D[r] * (UtG[3 * r] * s.V[c] + UtG[3 * r + 1] * s.V[3 + c] + UtG[3 * r + 2] * s.V[6 + c]);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) Z[3 * r + c] = (r == c) ? 0.f : (Q[3 * r + c] - Q[3 * c + r]) / (h[r] + h[c]);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) UDZ[3 * r + c] = s.U[3 * r] * D[0] * Z[c] + s.U[3 * r + 1] * D[1] * Z[3 + c] + s.U[3 * r + 2] * D[2] * Z[6 + c];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) dM[3 * r + c] = UDZ[3 * r] * s.V[3 * c] + UDZ[3 * r + 1] * s.V[3 * c + 1] + UDZ[3 * r + 2] * s.V[3 * c + 2];
}

// the decomposition as SVD_WS floats (the step's head leaves it for the tail, which needs the SVD of the SAME matrix for the VJP) and back
__device__ __forceinline__ void svd_ws_store(const Svd3 &s, float *o)
{
#pragma unroll
    for (int e = 0; e < 9; e++) { o[e] = s.U[e]; o[9 + e] = s.V[e]; }
    o[18] = s.s[0]; o[19] = s.s[1]; o[20] = s.s[2]; o[21] = s.d;
}
__device__ __forceinline__ void svd_ws_load(const float *w, Svd3 &s)
{
#pragma unroll
    for (int e = 0; e < 9; e++) { s.U[e] = w[e]; s.V[e] = w[9 + e]; }
    s.s[0] = w[18]; s.s[1] = w[19]; s.s[2] = w[20]; s.d = w[21];
}

// rigid transform (recon_fit_base.py:455-459) of one point: o = (x R + t) s, r = the frame's 9 floats of R, t its translation
__device__ __forceinline__ void rigid_point(const float *x, const float *r, const float *t, float sc, float *o)
{
    const float x0 = x[0], x1 = x[1], x2 = x[2];
#pragma unroll
    for (int c = 0; c < 3; c++) o[c] = (x0 * r[c] + x1 * r[3 + c] + x2 * r[6 + c] + t[c]) * sc;
}
// its VJP, one point's share of a[0..8] = dR and a[9..11] = dt.  ROT = false: the translation's three sums only (phase 'joint' optimises obj_t alone)
template <bool ROT>
__device__ __forceinline__ void rigid_vjp_point(const float *x, const float *g, float sc, float *a)
{
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float gc = g[c] * sc; a[9 + c] += gc;
        if (ROT) { a[c] += x[0] * gc; a[3 + c] += x[1] * gc; a[6 + c] += x[2] * gc; }
    }
}

// temporal stencils over the frames of a batch, v (B, D):  a_b = 2 v_b - v_{b-1} - v_{b+1}  (b = 1 .. B-2);  d_b = v_b - v_{b-1}  (b = 1 .. B-1).
// One ELEMENT (frame f, column i) sums the (up to three) stencils that touch it, so every gradient element is written exactly once.
// column i of frames f-2 .. f+2, frames clamped to the batch (a clamped value only ever meets a stencil that does not exist); D = row stride
__device__ __forceinline__ void stencil_taps(const float *v, int f, int B, int D, int i, float *o)
{
#pragma unroll
    for (int k = 0; k < 5; k++) o[k] = v[(size_t)min(max(f - 2 + k, 0), B - 1) * D + i];
}
// acceleration: returns the element's share w a_0^2 of the loss; grad = gs w (2 a_0 - a_m - a_p).  The un-weighted callers pass w = 1: 1 * a_0 and gs * 1 are
// exact, the same numbers as the forms without the factor.
__device__ __forceinline__ float accel_stencil(const float *o, int f, int B, float w, float gs, float &grad)
{
    const float vm2 = o[0], vm1 = o[1], v0 = o[2], vp1 = o[3], vp2 = o[4];
    // stencils centred on f-1, f, f+1 (a stencil exists for centres 1 .. B-2)
    const float a_m = (f - 1 >= 1 && f - 1 <= B - 2) ? 2.f * vm1 - vm2 - v0 : 0.f;
    const float a_0 = (f >= 1 && f <= B - 2) ? 2.f * v0 - vm1 - vp1 : 0.f;
    const float a_p = (f + 1 >= 1 && f + 1 <= B - 2) ? 2.f * vp1 - v0 - vp2 : 0.f;
    grad = gs * w * (2.f * a_0 - a_m - a_p);
    return w * a_0 * a_0;
}
// velocity: returns d_f^2; grad = gs (d_f - d_{f+1})
__device__ __forceinline__ float velocity_stencil(float vm1, float v0, float vp1, int f, int B, float gs, float &grad)
{
    const float d0 = f >= 1 ? v0 - vm1 : 0.f;          // d_f
    const float d1 = f + 1 < B ? vp1 - v0 : 0.f;       // d_{f+1}
    grad = gs * (d0 - d1);
    return d0 * d0;
}

// 2D keypoint term of one joint (fit_SMPLH_kpts.py:280-310; recon_fit_base.py:767-802): J = the joint, kp = (x, y, confidence), returns
// confidence-weighted squared pixel error, dJ = its gradient (scaled by gscale inv_cnt).  mode 1: pixels of the network crop around cc[b].
struct Cam5 { float fx, fy, cx, cy, crop; };
__device__ __forceinline__ float kpts_term(const float *J, const float *kp, const float *cc, int b, int mode, const Cam5 &cam, float net_size, float gscale, float inv_cnt, float *dJ)
{
    const float x = J[0], y = J[1], z = J[2];
    float px = cam.fx * x / z + cam.cx, py = cam.fy * y / z + cam.cy, sc = 1.f;
    if (mode == 1) {
        px = cam.crop / 2 + px - cc[2 * b]; py = cam.crop / 2 + py - cc[2 * b + 1];
        sc = net_size / cam.crop; px *= sc; py *= sc;
    }
    const float ex = px - kp[0], ey = py - kp[1], conf = kp[2];
    const float gpx = 2.f * ex * conf * gscale * inv_cnt * sc, gpy = 2.f * ey * conf * gscale * inv_cnt * sc;
    dJ[0] = gpx * cam.fx / z; dJ[1] = gpy * cam.fy / z;
    dJ[2] = -gpx * cam.fx * x / (z * z) - gpy * cam.fy * y / (z * z);
    return (ex * ex + ey * ey) * conf;
}

// squared-difference term of one element: returns (a - b)^2, grad = 2 (a - b) inv_denom gscale
__device__ __forceinline__ float sqdiff_elem(float a, float b, float inv_denom, float gscale, float &grad)
{
    const float d = a - b;
    grad = 2.f * d * inv_denom * gscale;
    return d * d;
}

// Adam (torch.optim.Adam single-tensor path) of one element; step_size = lr / (1 - beta1^step), bc2s = sqrt(1 - beta2^step)
__device__ __forceinline__ void adam_update(float &p, float gi, float &m, float &v, float step_size, float bc2s, float beta1, float beta2, float eps)
{
    const float mi = m * beta1 + (1.f - beta1) * gi;
    const float vi = v * beta2 + (1.f - beta2) * gi * gi;
    m = mi; v = vi;
    const float denom = sqrtf(vi) / bc2s + eps;
    p = p - step_size * (mi / denom);
}
// a (B, ncols) parameter slice with its gradient and moments; Adam on column c of row b
struct AdamSlice { float *p; int pstride; const float *g; int gstride; float *m, *v; int ncols; float step_size; };
__device__ __forceinline__ void adam_one(const AdamSlice &a, int b, int c, float bc2s, float beta1, float beta2, float eps)
{
    const int i = b * a.ncols + c;
    adam_update(a.p[(size_t)b * a.pstride + c], a.g[(size_t)b * a.gstride + c], a.m[i], a.v[i], a.step_size, bc2s, beta1, beta2, eps);
}

// closing a step, one thread: weighted loss, history slot, the reference's stop rule, loss state.  A stopped fit records NaN and keeps its state.
// ATOMIC: the terms are read with agent-scope atomic loads (the fused tails read what other workgroups of the SAME launch accumulated).
struct TermW { float w[16]; };
template <bool ATOMIC>
__device__ __forceinline__ void close_loss(const double *terms, const TermW &tw, int nterms, float tol, int armed, float *state, int *stop_flag, float *history, int slot,
                                           bool stopped)
{
    if (stopped) { if (history) history[slot] = nanf(""); return; }
    double l = 0;
    for (int k = 0; k < nterms; k++) l += (double)tw.w[k] * (ATOMIC ? __hip_atomic_load(terms + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : terms[k]);
    const float loss = (float)l, prev = state[0];
    if (history) history[slot] = loss;
    // reference: (abs(prev_loss - loss) / prev_loss < prev_loss * tol) and <iteration gate>
    if (armed && stop_flag && (fabsf(prev - loss) / prev < prev * tol)) *stop_flag = 1;
    state[0] = loss; state[1] = loss;
}

// ---- host side, shared by the launchers of misc.hip and step.hip ----
// the handle of vt_landmarks_create: the regressor as CSR (K rows) and, for the VJP, CSC (V columns), on the device
struct vt_landmarks { int K, V; int *indptr, *indices; float *data; int *colptr, *rowidx; float *cdata; };
// Adam's bias corrections at `step`, in double: returns bc2s = sqrt(1 - beta2^step); a group's step_size is (float)(lr / *bc1), bc1 = 1 - beta1^step
static inline float adam_bias(float beta1, float beta2, int step, double *bc1)
{
    *bc1 = 1.0 - pow((double)beta1, step);
    return (float)sqrt(1.0 - pow((double)beta2, step));
}
