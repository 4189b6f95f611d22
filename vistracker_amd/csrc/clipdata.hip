// clipdata.hip -- HVOP-Net's training data set on the device (vt_clip_draw, vt_clip_build; include/vistracker.h): the random decisions of a clip and the assembly
// of a batch of clips from the packed sequences, replacing data/traindata_cmfiller.py:19-66 and data/traindata_mfiller.py:222-296 of the reference.
//
// vt_clip_draw: one thread per clip.  Integers only: every decision is vt_dropout_hash(clip key, site, draw number) mapped to its range by multiply-shift, the
// clip key being two hashes of (seed, epoch, global clip index) -- see dropout_hash.h.  Nothing depends on the batch, the position in it or the launch geometry.
//
// vt_clip_build: a thread owns ONE rotation slot of one (clip, frame): slots 0..23 are the body joints (slot 0, the root, also owns the body translation), slot 24
// is the object (rotation, translation, mask and augmentation of the frame).  A 256-thread workgroup takes 10 consecutive frames of the flattened (B T) rows
// (250 slots), each thread leaves its 6 values in an LDS image of the rows, and after one barrier the workgroup streams the image out with consecutive lanes on
// consecutive floats: the rows of 10 frames are one contiguous span of every output, so every store instruction of a wave covers 256 contiguous bytes.
// data_smpl and gt_smpl are the same values (the body is neither masked nor augmented) and are stored from the same LDS words.
// No atomics, no workspace, no cross-workgroup traffic, fp32 with -ffp-contract=off: the same bits on every call, a clip's rows independent of the other clips.
//
// Arithmetic, in the reference's own order (fp32 here, float64 there):
//   axis -> 6D   numpy_axis_to_quat / numpy_quat_to_rotmat / numpy_rotmat_to_6d (geometry_utils.py:284-354) with their quirks: the norm is of theta + 1e-8 while
//                the division uses theta; the quaternion is renormalised by the norm of quat + 1e-8; 6D = the first two COLUMNS, row-major (m00 m01 m10 m11 m20 m21)
//   camera       kid != 1: R_new = R_w2c R(rotvec) and back to a rotvec the way scipy's Rotation does it (largest-of-four quaternion, w >= 0, angle = 2 atan2(|v|, w));
//                t_new = t R_w2c^T + t_w2c, for the body + (roots - t) R_w2c^T - (roots - t) (traindata_mfiller.py:245-257, 279-288).  kid == 1: copies.
//   6D -> axis   rot6d_to_rotmat (Gram-Schmidt, F.normalize's max(|.|, 1e-12)), kornia's rotation_matrix_to_quaternion (eps 1e-6) and quaternion_to_angle_axis,
//                NaN -> 0 (geometry_utils.py:63-77, 92-246); a zeroed (masked) row comes out as (0, pi, 0), as it does there
//   noise        0.5 z, z = sqrt(-2 ln u1) cos(2 pi u2), u1 = (h1 + 1) 2^-32, u2 = h2 2^-32 from two hashed words per value, or the caller's tensor (tests)
#include "common.h"
#include "dropout_hash.h"
#include <cstdint>

namespace clipd {

constexpr int THREADS = 256;
constexpr int SLOTS = 25;                  // 24 body joints + the object
constexpr int FRAMES = THREADS / SLOTS;    // 10 frames a workgroup, 250 of 256 threads own a slot
constexpr int SMPL_DIM = 147;
constexpr int MAX_AUG = 64;

__host__ __device__ __forceinline__ uint64_t clip_key(uint64_t seed, uint32_t epoch, uint32_t clip)
{
    const uint64_t idx = ((uint64_t)epoch << 32) | clip;
    return (uint64_t)vt_dropout_hash(seed, VT_CLIP_SITE_KEY_LO, idx) | ((uint64_t)vt_dropout_hash(seed, VT_CLIP_SITE_KEY_HI, idx) << 32);
}

__host__ __device__ __forceinline__ int draw_range(uint32_t h, int lo, int hi) { return lo + (int)(((uint64_t)h * (uint64_t)(uint32_t)(hi - lo)) >> 32); }

__global__ __launch_bounds__(THREADS) void draw_kernel(const int *__restrict__ clip_index, int B, uint64_t seed, uint32_t epoch, int T, int multi, int min_drop,
                                                       int max_drop, int sf_min, int sf_max, int aug_num, int *__restrict__ kid, int *__restrict__ drop_len,
                                                       int *__restrict__ start_fr, int *__restrict__ aug_start)
{
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= B) return;
    const uint64_t key = clip_key(seed, epoch, (uint32_t)clip_index[b]);
    kid[b] = multi ? draw_range(vt_dropout_hash(key, VT_CLIP_SITE_KID, 0), 0, 4) : 1;
    const int dl = draw_range(vt_dropout_hash(key, VT_CLIP_SITE_DROP_LEN, 0), min_drop, max_drop + 1);
    drop_len[b] = dl;
    const int hi = (T - dl) < sf_max ? (T - dl) : sf_max;
    start_fr[b] = draw_range(vt_dropout_hash(key, VT_CLIP_SITE_START_FR, 0), sf_min, hi);
    for (int j = 0; j < aug_num; j++) aug_start[(size_t)b * aug_num + j] = draw_range(vt_dropout_hash(key, VT_CLIP_SITE_AUG_START, (uint64_t)j), 0, T - aug_num);
}

// ---- rotations --------------------------------------------------------------------------------------------------------------------------------------------------
struct V3 { float x, y, z; };
struct M3 { float m00, m01, m02, m10, m11, m12, m20, m21, m22; };
struct R6 { float v0, v1, v2, v3, v4, v5; };

// numpy_axis_to_rot6D
__device__ __forceinline__ R6 axis_to_6d(V3 a)
{
    const float e = 1e-8f;
    const float ax = a.x + e, ay = a.y + e, az = a.z + e;
    const float n = sqrtf(ax * ax + ay * ay + az * az);
    const float nx = a.x / n, ny = a.y / n, nz = a.z / n;
    const float h = n * 0.5f;
    const float c = cosf(h), s = sinf(h);
    const float qw = c, qx = s * nx, qy = s * ny, qz = s * nz;
    const float pw = qw + e, px = qx + e, py = qy + e, pz = qz + e;
    const float qn = sqrtf(pw * pw + px * px + py * py + pz * pz);
    const float w = qw / qn, x = qx / qn, y = qy / qn, z = qz / qn;
    const float w2 = w * w, x2 = x * x, y2 = y * y, z2 = z * z;
    const float wx = w * x, wy = w * y, wz = w * z, xy = x * y, xz = x * z, yz = y * z;
    R6 r;
    r.v0 = w2 + x2 - y2 - z2;   r.v1 = 2.f * xy - 2.f * wz;
    r.v2 = 2.f * wz + 2.f * xy; r.v3 = w2 - x2 + y2 - z2;
    r.v4 = 2.f * xz - 2.f * wy; r.v5 = 2.f * wx + 2.f * yz;
    return r;
}

// Rotation.from_rotvec(a).as_matrix(): the unit quaternion of the rotation vector (series below 1e-3, as scipy), then its matrix
__device__ __forceinline__ M3 rotvec_to_matrix(V3 a)
{
    const float ang = sqrtf(a.x * a.x + a.y * a.y + a.z * a.z);
    float sc;
    if (ang <= 1e-3f) {
        const float a2 = ang * ang;
        sc = 0.5f - a2 / 48.f + a2 * a2 / 3840.f;
    } else {
        sc = sinf(ang * 0.5f) / ang;
    }
    const float x = sc * a.x, y = sc * a.y, z = sc * a.z, w = cosf(ang * 0.5f);
    const float x2 = x * x, y2 = y * y, z2 = z * z, w2 = w * w;
    const float xy = x * y, zw = z * w, xz = x * z, yw = y * w, yz = y * z, xw = x * w;
    M3 m;
    m.m00 = x2 - y2 - z2 + w2; m.m10 = 2.f * (xy + zw);   m.m20 = 2.f * (xz - yw);
    m.m01 = 2.f * (xy - zw);   m.m11 = -x2 + y2 - z2 + w2; m.m21 = 2.f * (yz + xw);
    m.m02 = 2.f * (xz + yw);   m.m12 = 2.f * (yz - xw);   m.m22 = -x2 - y2 + z2 + w2;
    return m;
}

__device__ __forceinline__ M3 matmul(const float *__restrict__ A, M3 b)      // A: 9 floats row-major (the w2c table)
{
    M3 c;
    c.m00 = A[0] * b.m00 + A[1] * b.m10 + A[2] * b.m20; c.m01 = A[0] * b.m01 + A[1] * b.m11 + A[2] * b.m21; c.m02 = A[0] * b.m02 + A[1] * b.m12 + A[2] * b.m22;
    c.m10 = A[3] * b.m00 + A[4] * b.m10 + A[5] * b.m20; c.m11 = A[3] * b.m01 + A[4] * b.m11 + A[5] * b.m21; c.m12 = A[3] * b.m02 + A[4] * b.m12 + A[5] * b.m22;
    c.m20 = A[6] * b.m00 + A[7] * b.m10 + A[8] * b.m20; c.m21 = A[6] * b.m01 + A[7] * b.m11 + A[8] * b.m21; c.m22 = A[6] * b.m02 + A[7] * b.m12 + A[8] * b.m22;
    return c;
}

// Rotation.from_matrix(m).as_rotvec()
__device__ __forceinline__ V3 matrix_to_rotvec(M3 m)
{
    const float tr = m.m00 + m.m11 + m.m22;
    float x, y, z, w;
    if (tr >= m.m00 && tr >= m.m11 && tr >= m.m22) {
        x = m.m21 - m.m12; y = m.m02 - m.m20; z = m.m10 - m.m01; w = 1.f + tr;
    } else if (m.m00 >= m.m11 && m.m00 >= m.m22) {
        x = 1.f - tr + 2.f * m.m00; y = m.m10 + m.m01; z = m.m20 + m.m02; w = m.m21 - m.m12;
    } else if (m.m11 >= m.m22) {
        y = 1.f - tr + 2.f * m.m11; z = m.m21 + m.m12; x = m.m01 + m.m10; w = m.m02 - m.m20;
    } else {
        z = 1.f - tr + 2.f * m.m22; x = m.m02 + m.m20; y = m.m12 + m.m21; w = m.m10 - m.m01;
    }
    const float qn = sqrtf(x * x + y * y + z * z + w * w);
    x = x / qn; y = y / qn; z = z / qn; w = w / qn;
    if (w < 0.f) { x = -x; y = -y; z = -z; w = -w; }
    const float vn = sqrtf(x * x + y * y + z * z);
    const float ang = 2.f * atan2f(vn, w);
    float sc;
    if (ang <= 1e-3f) {
        const float a2 = ang * ang;
        sc = 2.f + a2 / 12.f + 7.f * a2 * a2 / 2880.f;
    } else {
        sc = ang / sinf(ang * 0.5f);
    }
    return V3{sc * x, sc * y, sc * z};
}

// v R^T + t, component i = (v0 R[i][0] + v1 R[i][1]) + v2 R[i][2]
__device__ __forceinline__ V3 mul_rt(V3 v, const float *__restrict__ R)
{
    return V3{v.x * R[0] + v.y * R[1] + v.z * R[2], v.x * R[3] + v.y * R[4] + v.z * R[5], v.x * R[6] + v.y * R[7] + v.z * R[8]};
}

// rot6D_to_axis
__device__ __forceinline__ V3 rot6d_to_axis(R6 r)
{
    const float a1x = r.v0, a1y = r.v2, a1z = r.v4, a2x = r.v1, a2y = r.v3, a2z = r.v5;
    const float n1 = fmaxf(sqrtf(a1x * a1x + a1y * a1y + a1z * a1z), 1e-12f);
    const float b1x = a1x / n1, b1y = a1y / n1, b1z = a1z / n1;
    const float d = b1x * a2x + b1y * a2y + b1z * a2z;
    const float ux = a2x - d * b1x, uy = a2y - d * b1y, uz = a2z - d * b1z;
    const float n2 = fmaxf(sqrtf(ux * ux + uy * uy + uz * uz), 1e-12f);
    const float b2x = ux / n2, b2y = uy / n2, b2z = uz / n2;
    const float b3x = b1y * b2z - b1z * b2y, b3y = b1z * b2x - b1x * b2z, b3z = b1x * b2y - b1y * b2x;
    // M = columns (b1, b2, b3)
    const float m00 = b1x, m01 = b2x, m02 = b3x, m10 = b1y, m11 = b2y, m12 = b3y, m20 = b1z, m21 = b2z, m22 = b3z;
    float q0, q1, q2, q3, t;
    if (m22 < 1e-6f) {
        if (m00 > m11) { t = 1.f + m00 - m11 - m22; q0 = m21 - m12; q1 = t; q2 = m10 + m01; q3 = m02 + m20; }
        else           { t = 1.f - m00 + m11 - m22; q0 = m02 - m20; q1 = m10 + m01; q2 = t; q3 = m21 + m12; }
    } else {
        if (m00 < -m11) { t = 1.f - m00 - m11 + m22; q0 = m10 - m01; q1 = m02 + m20; q2 = m21 + m12; q3 = t; }
        else            { t = 1.f + m00 + m11 + m22; q0 = t; q1 = m21 - m12; q2 = m02 - m20; q3 = m10 - m01; }
    }
    const float rt = sqrtf(t);
    q0 = q0 / rt * 0.5f; q1 = q1 / rt * 0.5f; q2 = q2 / rt * 0.5f; q3 = q3 / rt * 0.5f;
    const float ss = q1 * q1 + q2 * q2 + q3 * q3;
    const float sn = sqrtf(ss);
    const float two = 2.f * (q0 < 0.f ? atan2f(-sn, -q0) : atan2f(sn, q0));
    const float k = ss > 0.f ? two / sn : 2.f;
    V3 a{q1 * k, q2 * k, q3 * k};
    if (a.x != a.x) a.x = 0.f;
    if (a.y != a.y) a.y = 0.f;
    if (a.z != a.z) a.z = 0.f;
    return a;
}

__device__ __forceinline__ float hashed_normal(uint64_t key, uint64_t value_index)
{
    const uint32_t h1 = vt_dropout_hash(key, VT_CLIP_SITE_NOISE, 2 * value_index), h2 = vt_dropout_hash(key, VT_CLIP_SITE_NOISE, 2 * value_index + 1);
    const float u1 = (float)((uint64_t)h1 + 1ull) * 0x1p-32f, u2 = (float)h2 * 0x1p-32f;
    return sqrtf(-2.f * logf(u1)) * cosf(6.283185307179586f * u2);
}

template <int OD>
__global__ __launch_bounds__(THREADS) void build_kernel(const float *__restrict__ poses, const float *__restrict__ trans, const float *__restrict__ roots,
                                                        const float *__restrict__ obj_angles, const float *__restrict__ obj_trans, long N,
                                                        const float *__restrict__ w2c_R, const float *__restrict__ w2c_t, int n_dates,
                                                        const int *__restrict__ start, const int *__restrict__ date, const int *__restrict__ kid,
                                                        const int *__restrict__ drop_len, const int *__restrict__ start_fr, const int *__restrict__ aug_start,
                                                        int B, int T, int aug_num, const float *__restrict__ noise, const int *__restrict__ clip_index,
                                                        uint64_t seed, uint32_t epoch, float *__restrict__ data_smpl, float *__restrict__ data_obj,
                                                        float *__restrict__ gt_smpl, float *__restrict__ gt_obj, unsigned char *__restrict__ mask_obj,
                                                        unsigned char *__restrict__ mask_smpl)
{
    __shared__ float s_smpl[FRAMES * SMPL_DIM];
    __shared__ float s_objd[FRAMES * OD];
    __shared__ float s_objg[FRAMES * OD];
    __shared__ unsigned char s_mask[FRAMES];

    const long rows = (long)B * T;
    const long row0 = (long)blockIdx.x * FRAMES;
    const int tid = threadIdx.x;
    const int lr = tid / SLOTS, s = tid - lr * SLOTS;
    const long row = row0 + lr;

    if (lr < FRAMES && row < rows) {
        const int b = (int)(row / T), t = (int)(row - (long)b * T);
        const long st = start[b];
        const int kd = kid[b], dt = date[b];
        // a clip whose start, camera or date is outside the tables reads nothing and comes out as zeros (the wrappers refuse such a clip before the launch)
        const bool ok = st >= 0 && st + T <= N && kd >= 0 && kd < 4 && dt >= 0 && dt < n_dates;
        const long f = ok ? st + t : 0;
        const bool cam = ok && kd != 1;
        const float *R = w2c_R + ((size_t)(ok ? dt : 0) * 4 + (ok ? kd : 0)) * 9;
        const float *tw = w2c_t + ((size_t)(ok ? dt : 0) * 4 + (ok ? kd : 0)) * 3;
        if (s < 24) {
            V3 a{poses[f * 72 + 3 * s], poses[f * 72 + 3 * s + 1], poses[f * 72 + 3 * s + 2]};
            if (s == 0) {
                V3 tr{trans[f * 3], trans[f * 3 + 1], trans[f * 3 + 2]};
                if (cam) {
                    a = matrix_to_rotvec(matmul(R, rotvec_to_matrix(a)));
                    const V3 rc{roots[f * 3] - tr.x, roots[f * 3 + 1] - tr.y, roots[f * 3 + 2] - tr.z};
                    const V3 p = mul_rt(tr, R), q = mul_rt(rc, R);
                    tr = V3{p.x + tw[0] + q.x - rc.x, p.y + tw[1] + q.y - rc.y, p.z + tw[2] + q.z - rc.z};
                }
                float *o = s_smpl + lr * SMPL_DIM + 144;
                o[0] = ok ? tr.x : 0.f; o[1] = ok ? tr.y : 0.f; o[2] = ok ? tr.z : 0.f;
            }
            const R6 r = axis_to_6d(a);
            float *o = s_smpl + lr * SMPL_DIM + 6 * s;
            o[0] = ok ? r.v0 : 0.f; o[1] = ok ? r.v1 : 0.f; o[2] = ok ? r.v2 : 0.f; o[3] = ok ? r.v3 : 0.f; o[4] = ok ? r.v4 : 0.f; o[5] = ok ? r.v5 : 0.f;
        } else {
            V3 a{obj_angles[f * 3], obj_angles[f * 3 + 1], obj_angles[f * 3 + 2]};
            V3 tr{obj_trans[f * 3], obj_trans[f * 3 + 1], obj_trans[f * 3 + 2]};
            if (cam) {
                a = matrix_to_rotvec(matmul(R, rotvec_to_matrix(a)));
                const V3 p = mul_rt(tr, R);
                tr = V3{p.x + tw[0], p.y + tw[1], p.z + tw[2]};
            }
            R6 g = axis_to_6d(a);
            if (!ok) { g = R6{0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; tr = V3{0.f, 0.f, 0.f}; }
            const int sf = start_fr[b], dl = drop_len[b];
            const bool masked = t >= sf && t < sf + dl;
            const float keep = 1.f - (masked ? 1.f : 0.f);
            R6 d{g.v0 * keep, g.v1 * keep, g.v2 * keep, g.v3 * keep, g.v4 * keep, g.v5 * keep};
            // the window with the highest number that holds frame t wins (the reference's fancy-index assignment); it reads the masked, un-noised row
            int win = -1, off = 0;
            for (int j = 0; j < aug_num; j++) {
                const int a0 = aug_start[(size_t)b * aug_num + j];
                if (t >= a0 && t < a0 + aug_num) { win = j; off = t - a0; }
            }
            if (win >= 0) {
                const size_t k = (size_t)win * aug_num + off;
                V3 z;
                if (noise != nullptr) {
                    const float *nz = noise + ((size_t)b * aug_num * aug_num + k) * 3;
                    z = V3{nz[0], nz[1], nz[2]};
                } else {
                    const uint64_t key = clip_key(seed, epoch, (uint32_t)clip_index[b]);
                    z = V3{hashed_normal(key, 3 * k), hashed_normal(key, 3 * k + 1), hashed_normal(key, 3 * k + 2)};
                }
                const V3 ax = rot6d_to_axis(d);
                d = axis_to_6d(V3{ax.x + z.x * 0.5f, ax.y + z.y * 0.5f, ax.z + z.z * 0.5f});
            }
            float *og = s_objg + lr * OD, *od = s_objd + lr * OD;
            og[0] = g.v0; og[1] = g.v1; og[2] = g.v2; og[3] = g.v3; og[4] = g.v4; og[5] = g.v5;
            od[0] = d.v0; od[1] = d.v1; od[2] = d.v2; od[3] = d.v3; od[4] = d.v4; od[5] = d.v5;
            if constexpr (OD == 9) {
                og[6] = tr.x; og[7] = tr.y; og[8] = tr.z;
                od[6] = tr.x * keep; od[7] = tr.y * keep; od[8] = tr.z * keep;
            }
            s_mask[lr] = masked ? 1 : 0;
        }
    }
    __syncthreads();

    const long left = rows - row0;
    const int nrow = left < FRAMES ? (int)left : FRAMES;
    const size_t base_s = (size_t)row0 * SMPL_DIM, base_o = (size_t)row0 * OD;
    for (int i = tid; i < nrow * SMPL_DIM; i += THREADS) {
        const float v = s_smpl[i];
        data_smpl[base_s + i] = v;
        gt_smpl[base_s + i] = v;
    }
    for (int i = tid; i < nrow * OD; i += THREADS) {
        data_obj[base_o + i] = s_objd[i];
        gt_obj[base_o + i] = s_objg[i];
    }
    if (tid < nrow) {
        mask_obj[row0 + tid] = s_mask[tid];
        mask_smpl[row0 + tid] = 0;
    }
}

}  // namespace clipd

extern "C" int vt_clip_draw(const int *clip_index, int B, unsigned long long seed, unsigned int epoch, int T, int multi_kinects, int min_drop_len, int max_drop_len,
                            int start_fr_min, int start_fr_max, int aug_num, int *kid, int *drop_len, int *start_fr, int *aug_start, void *stream)
{
    VT_REQUIRE(B >= 1 && T >= 1, "vt_clip_draw: B = %d, T = %d", B, T);
    VT_REQUIRE(clip_index && kid && drop_len && start_fr, "vt_clip_draw: NULL pointer");
    VT_REQUIRE(aug_num >= 0 && aug_num <= clipd::MAX_AUG && (aug_num == 0 || aug_start), "vt_clip_draw: aug_num = %d (0..%d) needs aug_start", aug_num, clipd::MAX_AUG);
    // degenerate ranges are refused, never clamped: every drop length must leave a start, and a window must fit
    VT_REQUIRE(min_drop_len >= 0 && max_drop_len >= min_drop_len, "vt_clip_draw: drop lengths [%d, %d]", min_drop_len, max_drop_len);
    const int hi = (T - max_drop_len) < start_fr_max ? (T - max_drop_len) : start_fr_max;
    VT_REQUIRE(start_fr_min >= 0 && hi > start_fr_min, "vt_clip_draw: no start frame in [%d, min(%d - %d, %d))", start_fr_min, T, max_drop_len, start_fr_max);
    VT_REQUIRE(aug_num == 0 || T - aug_num > 0, "vt_clip_draw: no window start in [0, %d - %d)", T, aug_num);
    hipLaunchKernelGGL(clipd::draw_kernel, dim3((B + clipd::THREADS - 1) / clipd::THREADS), dim3(clipd::THREADS), 0, vt_stream(stream), clip_index, B,
                       (uint64_t)seed, (uint32_t)epoch, T, multi_kinects, min_drop_len, max_drop_len, start_fr_min, start_fr_max, aug_num, kid, drop_len, start_fr,
                       aug_start);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

extern "C" int vt_clip_build(const float *poses, const float *trans, const float *roots, const float *obj_angles, const float *obj_trans, long N,
                             const float *w2c_R, const float *w2c_t, int n_dates, const int *start, const int *date, const int *kid, const int *drop_len,
                             const int *start_fr, const int *aug_start, int B, int T, int obj_dim, int aug_num, const float *noise, const int *clip_index,
                             unsigned long long seed, unsigned int epoch, float *data_smpl, float *data_obj, float *gt_smpl, float *gt_obj,
                             unsigned char *mask_obj, unsigned char *mask_smpl, void *stream)
{
    VT_REQUIRE(B >= 1 && T >= 1 && N >= T && N < 2147483647L, "vt_clip_build: B = %d, T = %d, N = %ld", B, T, N);
    VT_REQUIRE(obj_dim == 6 || obj_dim == 9, "vt_clip_build: obj_dim = %d, 6 or 9", obj_dim);
    VT_REQUIRE(n_dates >= 1 && w2c_R && w2c_t, "vt_clip_build: the world-to-local table needs at least one date");
    VT_REQUIRE(poses && trans && roots && obj_angles && obj_trans && start && date && kid && drop_len && start_fr, "vt_clip_build: NULL input");
    VT_REQUIRE(data_smpl && data_obj && gt_smpl && gt_obj && mask_obj && mask_smpl, "vt_clip_build: NULL output");
    VT_REQUIRE(aug_num >= 0 && aug_num <= clipd::MAX_AUG && (aug_num == 0 || aug_start), "vt_clip_build: aug_num = %d (0..%d) needs aug_start", aug_num, clipd::MAX_AUG);
    VT_REQUIRE(aug_num == 0 || noise || clip_index, "vt_clip_build: hashed noise needs clip_index");
    const long rows = (long)B * T;
    VT_REQUIRE(rows <= 2147483647L / clipd::SMPL_DIM * clipd::FRAMES, "vt_clip_build: B T = %ld rows", rows);
    const dim3 grid((unsigned)((rows + clipd::FRAMES - 1) / clipd::FRAMES)), block(clipd::THREADS);
    hipStream_t st = vt_stream(stream);
    if (obj_dim == 6)
        hipLaunchKernelGGL(clipd::build_kernel<6>, grid, block, 0, st, poses, trans, roots, obj_angles, obj_trans, N, w2c_R, w2c_t, n_dates, start, date, kid, drop_len,
                           start_fr, aug_start, B, T, aug_num, noise, clip_index, (uint64_t)seed, (uint32_t)epoch, data_smpl, data_obj, gt_smpl, gt_obj, mask_obj,
                           mask_smpl);
    else
        hipLaunchKernelGGL(clipd::build_kernel<9>, grid, block, 0, st, poses, trans, roots, obj_angles, obj_trans, N, w2c_R, w2c_t, n_dates, start, date, kid, drop_len,
                           start_fr, aug_start, B, T, aug_num, noise, clip_index, (uint64_t)seed, (uint32_t)epoch, data_smpl, data_obj, gt_smpl, gt_obj, mask_obj,
                           mask_smpl);
    VT_LAUNCH_CHECK();
    return VT_OK;
}
