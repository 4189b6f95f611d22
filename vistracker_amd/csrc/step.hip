// step.hip -- fused heads / tails of an Adam step of the two fit loops (vt_objfit_step / vt_smplfit_step).  A step of the object stage
// used to be ~11 launches of 4-16 us kernels around the one query launch (SO(3) projection, rigid transform, two temporal stencils, rigid VJP,
// SO(3) VJP, one Adam launch per parameter group, loss reduction, term zeroing); the same arithmetic, element for element and in the same
// order, now runs as head -> query -> stencils -> tail.  Per-frame work is done by the workgroup of the frame; what needs every frame (loss
// reduction, stop rule, zeroing the term accumulators for the next step) is done by whichever workgroup finishes LAST (ticket counter), after
// every other workgroup has read the stop flag and stepped its parameters.
// The operations themselves are the functions of step_ops.h that the single-purpose kernels of misc.hip call: this file owns their order, the
// barriers between them and the hand-overs, which is what the bitwise fused-vs-single tests guard.
#include "step_ops.h"
#include <vector>

// One workgroup of 1024 threads per frame (round 6; was ceil(N / 256) workgroups of 256): the projection's SVD is ~10 us of ONE thread, and every workgroup of a
// frame computed it while its other threads waited -- 12-24 x 96 workgroups holding their wave slots for the length of the SVD next to the other batches' query
// launches, for a point transform of microseconds.  Same arithmetic per point.
__global__ __launch_bounds__(1024) void objstep_head_kernel(const float *__restrict__ M0, const float *__restrict__ noise, const float *__restrict__ t,
                                                           const float *__restrict__ s, const float *__restrict__ X0p, int N, float *__restrict__ Xp,
                                                           const float *__restrict__ X0v, int NV, float *__restrict__ Xv, float *__restrict__ Rout,
                                                           double *terms, int nzero, float *__restrict__ svd_ws)
{
    __shared__ float sR[9];
    const int b = blockIdx.y;
    if (threadIdx.x == 0) {
        float M[9]; Svd3 sv;
        so3_input(M0, noise, b, M);
        svd3(M, sv);
        so3_rotation(sv, sR);
        if (blockIdx.x == 0) {
#pragma unroll
            for (int e = 0; e < 9; e++) Rout[9 * b + e] = sR[e];
            // the decomposition itself for the step's tail (round 6: the one-sided Jacobi SVD -- 24 rotations with two divisions and two square roots
            // each, ~10 us of one thread -- was computed twice per step)
            if (svd_ws) svd_ws_store(sv, svd_ws + SVD_WS * b);
        }
    }
    if (blockIdx.x == 0 && b == 0 && terms && (int)threadIdx.x < nzero) terms[threadIdx.x] = 0.0;
    __syncthreads();
    const float sc = s[b], t0 = t[3 * b], t1 = t[3 * b + 1], t2 = t[3 * b + 2];
    const float tt[3] = {t0, t1, t2};
    float r[9];
#pragma unroll
    for (int e = 0; e < 9; e++) r[e] = sR[e];
    for (int n = blockIdx.x * blockDim.x + threadIdx.x; n < N; n += gridDim.x * blockDim.x) rigid_point(X0p + (size_t)n * 3, r, tt, sc, Xp + ((size_t)b * N + n) * 3);
    if (Xv)
        for (int n = blockIdx.x * blockDim.x + threadIdx.x; n < NV; n += gridDim.x * blockDim.x) rigid_point(X0v + (size_t)n * 3, r, tt, sc, Xv + ((size_t)b * NV + n) * 3);
}
extern "C" int vt_objstep_head(const float *M0, const float *noise, const float *t, const float *s, int B, const float *X0_points, int N, float *X_points,
                               const float *X0_verts, int NV, float *X_verts, float *R, double *terms, int nzero, float *svd_ws, void *stream)
{
    VT_REQUIRE(M0 && t && s && X0_points && X_points && R && B > 0 && N > 0 && (!X_verts || (X0_verts && NV > 0)) && nzero >= 0 && nzero <= 16, "vt_objstep_head: bad argument");
    hipLaunchKernelGGL(objstep_head_kernel, dim3(1, B), dim3(1024), 0, vt_stream(stream), M0, noise, t, s, X0_points, N, X_points, X0_verts, NV, X_verts,
                       R, terms, nzero, svd_ws);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

// acceleration + velocity stencils of (B, D) in one pass: dv (+)= gs_a (2 a_0 - a_m - a_p), then += gs_v (d_0 - d_1) -- the two updates of
// vt_accel_loss and vt_velocity_loss in their order; init_zero: dv starts from zero (phase 'sil': no query gradient, no fill launch).
// `g` = the gradient so far; returns it with both updates, the elements' shares of the two terms added to acc_a / acc_v.
__device__ __forceinline__ float temporal2_elem(const float *v, int f, int B, int D, int i, float gs_a, float gs_v, float g, double &acc_a, double &acc_v)
{
    float taps[5], ga, gv;
    stencil_taps(v, f, B, D, i, taps);
    acc_a += (double)accel_stencil(taps, f, B, 1.f, gs_a, ga);
    g += ga;
    acc_v += (double)velocity_stencil(taps[1], taps[2], taps[3], f, B, gs_v, gv);
    return g + gv;
}
__global__ __launch_bounds__(256) void temporal2_kernel(const float *__restrict__ v, int B, int D, float gs_a, double *term_a, float gs_v, double *term_v,
                                                        float *__restrict__ dv, int init_zero)
{
    __shared__ double red[4];
    double acc_a = 0, acc_v = 0;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < B * D; t += gridDim.x * 256) {
        const int f = t / D, i = t - f * D;
        dv[(size_t)f * D + i] = temporal2_elem(v, f, B, D, i, gs_a, gs_v, init_zero ? 0.f : dv[(size_t)f * D + i], acc_a, acc_v);
    }
    term_add(acc_a / ((double)(B - 2) * D), term_a, red);
    term_add(acc_v / ((double)(B - 1) * D), term_v, red);
}
extern "C" int vt_temporal_loss2(const float *v, int B, int D, float gscale_accel, double *term_accel, float gscale_velocity, double *term_velocity, float *dv,
                                 int init_zero, void *stream)
{
    VT_REQUIRE(v && dv && B >= 3 && D > 0, "vt_temporal_loss2: bad argument (B >= 3)");
    // derivative scales as in vt_accel_loss / vt_velocity_loss: d/dv of mean(a^2) resp. mean(d^2)
    const float gs_a = 2.f * gscale_accel / ((float)(B - 2) * (float)D), gs_v = 2.f * gscale_velocity / ((float)(B - 1) * (float)D);
    hipLaunchKernelGGL(temporal2_kernel, dim3(min((B * D + 255) / 256, 512)), dim3(256), 0, vt_stream(stream), v, B, D, gs_a, term_accel, gs_v, term_velocity, dv, init_zero);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

struct StepEnd {
    const double *terms_r; double *terms_w; TermW tw; int nterms; float tol; int armed; float *state; int *stop_flag; float *history; int slot;
    int *ticket; int nzero;
};
// the fence-free step end below leans on how gfx942 / gfx950 perform fp64 atomics and count them in vmcnt: any other target gets the fenced form
#ifndef STEP_END_FENCE
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx942__) && !defined(__gfx950__)
#define STEP_END_FENCE 1
#else
#define STEP_END_FENCE 0
#endif
#endif
// the workgroup that takes the last ticket closes the step: close_loss (what vt_loss_reduce_and_stop does), and the term accumulators [0, nzero)
// zeroed for the next step.  Every other workgroup has finished (its writes fenced) by then.
__device__ __forceinline__ void step_end(const StepEnd &e, int nblocks, bool stopped)
{
    __shared__ int last;
    // What the closing workgroup reads of the others are the TERM accumulators only, and those are device-scope atomics (performed at the memory side, dropped from
    // the XCD's L2) read back with agent-scope atomic loads: each wave waits until its own atomics have been performed (s_waitcnt vmcnt(0)) before the workgroup
    // takes its ticket.  No __threadfence(): on a multi-XCD part it writes the XCD's dirty L2 lines back and invalidates the L1 -- ~3.5 us per fencing workgroup,
    // 2-4 x that with all 256 threads fencing (MI355X_MICROARCH.md; measured round 6 in sil_image_kernel: 110 us with a fence per workgroup, 26 us without) -- for
    // plain stores (parameters, Adam moments, history) that nobody reads before the kernel boundary.  -DSTEP_END_FENCE=1 restores the fences.
#if STEP_END_FENCE
    __threadfence();
#else
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#endif
    __syncthreads();
    if (threadIdx.x == 0) last = (atomicAdd(e.ticket, 1) == nblocks - 1);
    __syncthreads();
    if (!last) return;
#if STEP_END_FENCE
    __threadfence();
#endif
    if (threadIdx.x == 0) {
        *e.ticket = 0;
        close_loss<true>(e.terms_r, e.tw, e.nterms, e.tol, e.armed, e.state, e.stop_flag, e.history, e.slot, stopped);
        for (int k = 0; k < e.nzero; k++) e.terms_w[k] = 0.0;
    }
}

// tail of an object-stage step, one workgroup per frame: rigid VJP over the vertex set (phase 'sil') and the surface points, the translation
// regulariser of phase 'sil', the SO(3) VJP, Adam on the frame's rotation parameters (9) and translation (3), then step_end
// vt_objstep_tail_temporal (round 6): the stencils of vt_temporal_loss2 evaluated INSIDE the tail while it reads the points' gradient (temporal2_elem on
// g = dX, or 0 in phase 'sil'), so the rigid VJP sees the same bits -- one launch (19 us of launch-bound stencil work per object-stage step) less.
// mode 0: off (dXp already holds everything), 1: add to dXp, 2: dXp is not read (phase 'sil').
struct TemporalIn { const float *X; float gs_a, gs_v; double *term_a, *term_v; int mode; };
__global__ __launch_bounds__(256) void objstep_tail_kernel(TemporalIn tin, const float *__restrict__ X0v, int NV, const float *__restrict__ dXv, const float *__restrict__ X0p, int N,
                                                           const float *__restrict__ dXp, const float *__restrict__ s, const float *__restrict__ M0,
                                                           const float *__restrict__ noise, const float *__restrict__ tpar, const float *__restrict__ t_init,
                                                           float w_trans, double *term_trans, float *__restrict__ dR, float *__restrict__ dt, float *__restrict__ dM,
                                                           AdamSlice aR, AdamSlice aT, float bc2s, float beta1, float beta2, float eps, StepEnd end,
                                                           const float *__restrict__ svd_ws)
{
    __shared__ float red12[4][12];
    __shared__ double redt[4];
    const int b = blockIdx.x, B = gridDim.x;
    const bool stopped = end.stop_flag && *end.stop_flag;          // read before any workgroup can close the step
    double acc_a = 0, acc_v = 0;
    // phase 'joint' optimises obj_t only (recon_fit_trivis_full.py:343-347: optim.Adam([obj_t], lr=0.002)): the rotation half of the rigid VJP (nine of
    // the twelve sums over the points) and the SO(3) VJP with its second Jacobi SVD feed nothing -- skipped when no rotation slice is optimised
    // (dR / dM are then left untouched; obj_t takes the same three sums in the same order: bit-identical parameters)
    const bool rot = aR.p != nullptr;
    const float sc = s[b];
    float svw[SVD_WS];              // thread 0: the head's SVD of this frame, requested before the sums over the points so that its latency hides behind them
    if (svd_ws && rot && threadIdx.x == 0) {
#pragma unroll
        for (int e = 0; e < SVD_WS; e++) svw[e] = svd_ws[SVD_WS * b + e];
    }
    // trans = mean_{B,3} (t - t_init)^2  (vt_sqdiff_loss with denom 3 B)
    const float inv_denom = 1.f / (float)(3 * B);
    float tot[12];
#pragma unroll
    for (int e = 0; e < 12; e++) tot[e] = 0.f;
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        const float *X0 = pass == 0 ? X0v : X0p; const float *dX = pass == 0 ? dXv : dXp; const int n_ = pass == 0 ? NV : N;
        if (!dX) continue;
        float a[12];
#pragma unroll
        for (int e = 0; e < 12; e++) a[e] = 0.f;
        for (int n = threadIdx.x; n < n_; n += 256) {
            const float *x = X0 + (size_t)n * 3; const float *g = dX + ((size_t)b * n_ + n) * 3;
            float gt[3];
            if (pass == 1 && tin.mode) {
#pragma unroll
                for (int c = 0; c < 3; c++) gt[c] = temporal2_elem(tin.X, b, B, N * 3, n * 3 + c, tin.gs_a, tin.gs_v, tin.mode == 2 ? 0.f : g[c], acc_a, acc_v);
                g = gt;
            }
            if (rot) rigid_vjp_point<true>(x, g, sc, a); else rigid_vjp_point<false>(x, g, sc, a);
        }
        // the twelve block sums of rigid_bwd_kernel (wave tree, then the four waves in order: the same additions) with ONE barrier pair instead of twelve
#pragma unroll
        for (int e = 0; e < 12; e++) a[e] = wave_sum(a[e]);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int e = 0; e < 12; e++) red12[threadIdx.x >> 6][e] = a[e];
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 12; e++) {
            float v = 0.f;
#pragma unroll
            for (int i = 0; i < 4; i++) v += red12[i][e];
            tot[e] = (pass == 0 || !dXv) ? v : tot[e] + v;         // rigid_bwd_kernel: first set written, second accumulated
        }
        if (pass == 0 && t_init) {
            // the regulariser adds its gradient to dt BETWEEN the two rigid VJPs in the unfused sequence (vertex set, regulariser, surface points):
            // same order of the three float additions here
#pragma unroll
            for (int c = 0; c < 3; c++) { float gr; sqdiff_elem(tpar[3 * b + c], t_init[3 * b + c], inv_denom, w_trans, gr); tot[9 + c] += gr; }
        }
    }
    if (tin.mode) {
        // the frame's share of the two stencil terms (vt_temporal_loss2 adds per workgroup of 256 elements: the same fp64 atomics, another grouping)
        term_add(acc_a / ((double)(B - 2) * (N * 3)), tin.term_a, redt);
        term_add(acc_v / ((double)(B - 1) * (N * 3)), tin.term_v, redt);
    }
    if (threadIdx.x == 0) {
        float g[12];
#pragma unroll
        for (int e = 0; e < 12; e++) g[e] = tot[e];
        if (t_init) {
            double acc = 0;
#pragma unroll
            for (int c = 0; c < 3; c++) { float gr; acc += (double)sqdiff_elem(tpar[3 * b + c], t_init[3 * b + c], inv_denom, w_trans, gr); }
            atomicAdd(term_trans, acc * (double)inv_denom);        // the frame's share of the term
        }
#pragma unroll
        for (int c = 0; c < 3; c++) dt[3 * b + c] = g[9 + c];
        if (rot) {
            float M[9]; Svd3 sv;
            if (svd_ws) svd_ws_load(svw, sv);      // the step's head decomposed this matrix already (vt_objstep_head with the same workspace): the same numbers
            else { so3_input(M0, noise, b, M); svd3(M, sv); }
            so3_vjp(sv, g, dM + 9 * b);
#pragma unroll
            for (int e = 0; e < 9; e++) dR[9 * b + e] = g[e];
        }
    }
    __syncthreads();
    if (!stopped) {
        // Adam reads the gradients the way adam2d_kernel does: from the gradient tensors (dM, dt) just written by thread 0 of this workgroup
        if (aR.p && threadIdx.x < 9) adam_one(aR, b, threadIdx.x, bc2s, beta1, beta2, eps);
        if (aT.p && threadIdx.x >= 64 && threadIdx.x < 67) adam_one(aT, b, threadIdx.x - 64, bc2s, beta1, beta2, eps);
    }
    step_end(end, B, stopped);
}
static StepEnd make_end(double *terms, const float *w, int nterms, float tol, int armed, float *state, int *stop_flag, float *history, int slot, int *ticket, int nzero)
{
    StepEnd e; e.terms_r = terms; e.terms_w = terms; e.nterms = nterms; e.tol = tol; e.armed = armed; e.state = state; e.stop_flag = stop_flag; e.history = history; e.slot = slot;
    e.ticket = ticket; e.nzero = nzero;
    for (int k = 0; k < 16; k++) e.tw.w[k] = k < nterms ? w[k] : 0.f;
    return e;
}
// the launch behind both entry points of the object tail; `who` names the entry point in a refusal
static int objstep_tail_launch(const char *who, const TemporalIn &tin, const float *X0_verts, int NV, const float *dX_verts, const float *X0_points, int N, const float *dX_points,
                               const float *s, int B, const float *M0, const float *noise, const float *t, const float *t_init, float w_trans, double *term_trans,
                               float *dR, float *dt, float *dM,
                               float *pR, float *mR, float *vR, float lrR, float *pT, float *mT, float *vT, float lrT, int adam_step, float beta1, float beta2, float eps,
                               double *terms, const float *w, int nterms, float tol, int armed, float *state, int *stop_flag, float *history, int slot, int *ticket, int nzero,
                               const float *svd_ws, void *stream)
{
    VT_REQUIRE(X0_points && dX_points && s && M0 && t && dR && dt && dM && B > 0 && N > 0 && (!dX_verts || (X0_verts && NV > 0)) && (!t_init || term_trans), "%s: bad argument", who);
    VT_REQUIRE(terms && w && state && ticket && nterms > 0 && nterms <= 16 && nzero >= 0 && nzero <= nterms && adam_step >= 1 && (!pR || (mR && vR)) && (!pT || (mT && vT)),
               "%s: bad optimiser / loss arguments", who);
    double bc1; const float bc2s = adam_bias(beta1, beta2, adam_step, &bc1);
    AdamSlice aR = {pR, 9, dM, 9, mR, vR, 9, (float)(lrR / bc1)}, aT = {pT, 3, dt, 3, mT, vT, 3, (float)(lrT / bc1)};
    hipLaunchKernelGGL(objstep_tail_kernel, dim3(B), dim3(256), 0, vt_stream(stream), tin, X0_verts, NV, dX_verts, X0_points, N, dX_points, s, M0, noise, t, t_init, w_trans, term_trans,
                       dR, dt, dM, aR, aT, bc2s, beta1, beta2, eps, make_end(terms, w, nterms, tol, armed, state, stop_flag, history, slot, ticket, nzero), svd_ws);
    VT_LAUNCH_CHECK();
    return VT_OK;
}
extern "C" int vt_objstep_tail(const float *X0_verts, int NV, const float *dX_verts, const float *X0_points, int N, const float *dX_points, const float *s, int B,
                               const float *M0, const float *noise, const float *t, const float *t_init, float w_trans, double *term_trans,
                               float *dR, float *dt, float *dM,
                               float *pR, float *mR, float *vR, float lrR, float *pT, float *mT, float *vT, float lrT, int adam_step, float beta1, float beta2, float eps,
                               double *terms, const float *w, int nterms, float tol, int armed, float *state, int *stop_flag, float *history, int slot, int *ticket, int nzero,
                               float *svd_ws, void *stream)
{
    return objstep_tail_launch("vt_objstep_tail", TemporalIn{nullptr, 0.f, 0.f, nullptr, nullptr, 0}, X0_verts, NV, dX_verts, X0_points, N, dX_points, s, B, M0, noise, t, t_init, w_trans,
                               term_trans, dR, dt, dM, pR, mR, vR, lrR, pT, mT, vT, lrT, adam_step, beta1, beta2, eps, terms, w, nterms, tol, armed, state, stop_flag, history, slot,
                               ticket, nzero, svd_ws, stream);
}
extern "C" int vt_objstep_tail_temporal(const float *X_points, float gscale_accel, double *term_accel, float gscale_velocity, double *term_velocity, int init_zero,
                                        const float *X0_verts, int NV, const float *dX_verts, const float *X0_points, int N, const float *dX_points, const float *s, int B,
                                        const float *M0, const float *noise, const float *t, const float *t_init, float w_trans, double *term_trans,
                                        float *dR, float *dt, float *dM,
                                        float *pR, float *mR, float *vR, float lrR, float *pT, float *mT, float *vT, float lrT, int adam_step, float beta1, float beta2, float eps,
                                        double *terms, const float *w, int nterms, float tol, int armed, float *state, int *stop_flag, float *history, int slot, int *ticket, int nzero,
                                        float *svd_ws, void *stream)
{
    VT_REQUIRE(X_points && term_accel && term_velocity && B >= 3, "vt_objstep_tail_temporal: bad argument (B >= 3)");
    const int D = N * 3;
    const TemporalIn tin = {X_points, 2.f * gscale_accel / ((float)(B - 2) * (float)D), 2.f * gscale_velocity / ((float)(B - 1) * (float)D), term_accel, term_velocity, init_zero ? 2 : 1};
    return objstep_tail_launch("vt_objstep_tail_temporal", tin, X0_verts, NV, dX_verts, X0_points, N, dX_points, s, B, M0, noise, t, t_init, w_trans, term_trans, dR, dt, dM,
                               pR, mR, vR, lrR, pT, mT, vT, lrT, adam_step, beta1, beta2, eps, terms, w, nterms, tol, armed, state, stop_flag, history, slot, ticket, nzero, svd_ws, stream);
}

// tail of a SMPL-stage step, one 64-thread workgroup per frame: body-pose prior (vt_mahalanobis, n = 63 at pose[:, 3:66]) with its gradient,
// the pose-initialisation term mean_B sum (pose[:, 3:72] - pose_init)^2 (vt_sqdiff_loss), Adam on up to three column slices, step_end
__global__ __launch_bounds__(64) void smplstep_tail_kernel(float *__restrict__ pose, const float *__restrict__ pose_init, float *__restrict__ dpose,
                                                           const float *__restrict__ mean, const float *__restrict__ prec, float gscale, double *term_prior,
                                                           float w_pinit, double *term_pinit, AdamSlice a0, AdamSlice a1, AdamSlice a2, float bc2s, float beta1,
                                                           float beta2, float eps, StepEnd end)
{
    __shared__ float d[64], t2[64];
    const int b = blockIdx.x, B = gridDim.x, j = threadIdx.x, n = 63, off = 3, stride = 156;
    const bool stopped = end.stop_flag && *end.stop_flag;
    const float val = mahalanobis_value(pose + (size_t)b * stride + off, n, mean, prec, d, t2);
    __syncthreads();
    mahalanobis_grad(t2, n, prec, dpose + (size_t)b * stride + off, gscale);
    // pinit over columns 3 .. 71 (69 of them): thread j takes columns j and j + 64
    double acc = 0;
    const float inv_denom = 1.f / (float)B;
    for (int c = j; c < 69; c += 64) {
        float g;
        acc += (double)sqdiff_elem(pose[(size_t)b * stride + 3 + c], pose_init[(size_t)b * stride + 3 + c], inv_denom, w_pinit, g);
        dpose[(size_t)b * stride + 3 + c] += g;
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (j == 0) { atomicAdd(term_pinit, acc * (double)inv_denom); atomicAdd(term_prior, (double)val / (double)B); }
    __syncthreads();          // the frame's gradients are complete (same workgroup wrote them)
    if (!stopped) {
        const AdamSlice *sl[3] = {&a0, &a1, &a2};
#pragma unroll
        for (int k = 0; k < 3; k++)
            if (sl[k]->p) for (int c = j; c < sl[k]->ncols; c += 64) adam_one(*sl[k], b, c, bc2s, beta1, beta2, eps);
    }
    step_end(end, B, stopped);
}
extern "C" int vt_smplstep_tail(float *pose, const float *pose_init, float *dpose, int B, const float *prior_mean, const float *prior_prec, float gscale_prior,
                                double *term_prior, float w_pinit, double *term_pinit,
                                float *p0, int ps0, const float *g0, int gs0, float *m0, float *v0, int n0, float lr0,
                                float *p1, int ps1, const float *g1, int gs1, float *m1, float *v1, int n1, float lr1,
                                float *p2, int ps2, const float *g2, int gs2, float *m2, float *v2, int n2, float lr2,
                                int adam_step, float beta1, float beta2, float eps,
                                double *terms, const float *w, int nterms, float tol, int armed, float *state, int *stop_flag, float *history, int slot, int *ticket, int nzero,
                                void *stream)
{
    VT_REQUIRE(pose && pose_init && dpose && prior_mean && prior_prec && term_prior && term_pinit && B > 0 && adam_step >= 1, "vt_smplstep_tail: bad argument");
    VT_REQUIRE(terms && w && state && ticket && nterms > 0 && nterms <= 16 && nzero >= 0 && nzero <= nterms, "vt_smplstep_tail: bad loss arguments");
    // a group that is optimised needs its gradient and both moments (the kernel would follow a NULL pointer otherwise), and strides that hold its columns
    VT_REQUIRE((!p0 || (g0 && m0 && v0 && n0 > 0 && ps0 >= n0 && gs0 >= n0)) && (!p1 || (g1 && m1 && v1 && n1 > 0 && ps1 >= n1 && gs1 >= n1)) &&
               (!p2 || (g2 && m2 && v2 && n2 > 0 && ps2 >= n2 && gs2 >= n2)), "vt_smplstep_tail: a parameter group without its gradient / moments, or a stride below its column count");
    double bc1; const float bc2s = adam_bias(beta1, beta2, adam_step, &bc1);
    AdamSlice a0 = {p0, ps0, g0, gs0, m0, v0, n0, (float)(lr0 / bc1)}, a1 = {p1, ps1, g1, gs1, m1, v1, n1, (float)(lr1 / bc1)}, a2 = {p2, ps2, g2, gs2, m2, v2, n2, (float)(lr2 / bc1)};
    hipLaunchKernelGGL(smplstep_tail_kernel, dim3(B), dim3(64), 0, vt_stream(stream), pose, pose_init, dpose, prior_mean, prior_prec, gscale_prior, term_prior, w_pinit, term_pinit,
                       a0, a1, a2, bc2s, beta1, beta2, eps, make_end(terms, w, nterms, tol, armed, state, stop_flag, history, slot, ticket, nzero));
    VT_LAUNCH_CHECK();
    return VT_OK;
}

// the keypoint chain of a SMPL-stage step in one launch, one workgroup per frame: body25 joints J = regressor . verts (a wave per joint, as
// vt_landmarks_forward), the 2-D keypoint term and dJ (vt_kpts_loss), d verts = regressor^T dJ written -- not accumulated -- for every
// vertex (vt_landmarks_backward): the query launch that follows adds its gradient to it (vt_query_human_step)
__global__ __launch_bounds__(1024) void kpts_step_kernel(const int *__restrict__ indptr, const int *__restrict__ indices, const float *__restrict__ data,
                                                        const int *__restrict__ colptr, const int *__restrict__ rowidx, const float *__restrict__ cdata,
                                                        const float *__restrict__ verts, int V, int K, const float *__restrict__ kpts, const float *__restrict__ cc,
                                                        int mode, Cam5 cam, float net_size, float gscale, float inv_cnt, double *term, float *__restrict__ Jout,
                                                        float *__restrict__ dverts, int accumulate)
{
    __shared__ float sJ[64 * 3], sdJ[64 * 3];
    __shared__ double red[16];
    // 16 waves per frame (round 6; was 4): the landmark rows and the vertex columns are chains of dependent gathers, 7 rows / 27 columns deep per thread
    // with 256 threads -- 83 us of latency for microseconds of work; same sums in the same order
    const int b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    for (int k = wave; k < K; k += nw) {
        float a[3];
        landmark_row(indptr, indices, data, verts, b, V, k, lane, a);
        if (lane == 0) {
            sJ[3 * k] = a[0]; sJ[3 * k + 1] = a[1]; sJ[3 * k + 2] = a[2];
            if (Jout) { float *o = Jout + ((size_t)b * K + k) * 3; o[0] = a[0]; o[1] = a[1]; o[2] = a[2]; }
        }
    }
    __syncthreads();
    double acc = 0;
    if ((int)threadIdx.x < K) {
        const int k = threadIdx.x;
        acc = (double)kpts_term(sJ + 3 * k, kpts + 3 * (b * K + k), cc, b, mode, cam, net_size, gscale, inv_cnt, sdJ + 3 * k);
    }
    term_add(acc * (double)inv_cnt, term, red);          // (its barriers also publish sdJ)
    for (int v = threadIdx.x; v < V; v += blockDim.x) landmark_col(colptr, rowidx, cdata, sdJ, 0, v, accumulate, dverts + ((size_t)b * V + v) * 3);
}
extern "C" int vt_kpts_step(const vt_landmarks *h, const float *verts, const float *kpts, const float *crop_center, int B, int mode, const float *cam, float net_size,
                            float gscale, double *term, float *J, float *dverts, int accumulate, void *stream)
{
    VT_REQUIRE(h && verts && kpts && cam && dverts && B > 0 && h->K <= 64 && (mode == 0 || (mode == 1 && crop_center)), "vt_kpts_step: bad argument (at most 64 landmarks)");
    Cam5 c{cam[0], cam[1], cam[2], cam[3], cam[4]};
    const float inv_cnt = 1.f / (mode == 0 ? (float)(B * h->K * 2) : (float)(B * h->K));
    hipLaunchKernelGGL(kpts_step_kernel, dim3(B), dim3(1024), 0, vt_stream(stream), h->indptr, h->indices, h->data, h->colptr, h->rowidx, h->cdata, verts, h->V, h->K,
                       kpts, crop_center, mode, c, net_size, gscale, inv_cnt, term, J, dverts, accumulate);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

// ---- device-side early stop: per-stream skip flag -------------------------------------------------------------------------------------------
// The stop rules of the fits are evaluated on the device (vt_loss_reduce_and_stop / the step tails) and the host looks at the flag once per outer
// iteration of 10 steps, so up to 9 steps are already queued behind the step that stopped the fit.  Adam and the loss history ignore them; with the
// flag registered for the stream the query and SMPL-H kernels of those steps return at their first instruction as well (results unchanged: the
// reference breaks out of its loop at that step, recon_fit_behave.py:447).  The registry is PER HOST THREAD (thread_local), keyed by (device, stream):
// a fit registers its flag from the thread that issues its launches and only that thread's launches see it -- two fits driven by two threads
// through the SAME stream (e.g. both on the default stream) can neither pick up nor delete each other's flag.
struct SkipEntry { int dev; hipStream_t st; const int *flag; };
static thread_local std::vector<SkipEntry> t_skip_tab;       // (the default stream is the same handle on every device: the device is part of the key)
static int skip_device() { int d = 0; (void)hipGetDevice(&d); return d; }
const int *vt_skip_flag_of(hipStream_t st)
{
    if (t_skip_tab.empty()) return nullptr;
    const int dev = skip_device();
    for (const auto &e : t_skip_tab) if (e.st == st && e.dev == dev) return e.flag;
    return nullptr;
}
extern "C" int vt_stream_set_skip_flag(void *stream, const int *flag)
{
    const hipStream_t st = vt_stream(stream); const int dev = skip_device();
    for (size_t i = 0; i < t_skip_tab.size(); i++)
        if (t_skip_tab[i].st == st && t_skip_tab[i].dev == dev) {
            // a second fit of THIS thread on the stream while the first one's flag is still registered (nested / leaked registration): refuse instead of
            // redirecting the first fit's launches to another flag
            if (flag && t_skip_tab[i].flag != flag) VT_FAIL(VT_ERR_BUSY, "vt_stream_set_skip_flag: another stop flag is already registered for this stream by this thread");
            if (!flag) { t_skip_tab[i] = t_skip_tab.back(); t_skip_tab.pop_back(); }
            return VT_OK;
        }
    if (flag) t_skip_tab.push_back({dev, st, flag});
    return VT_OK;
}
