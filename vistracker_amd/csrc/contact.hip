// contact.hip -- where the body touches the object (demo.sh step 7 with viz_contact: render/nr_utils.py:380-404 ContactVisualizer.get_contact_spheres,
// :100-122 color_contact_faces_all): nearest SMPL vertex of every object vertex, the touched body parts, one sphere per part, recoloured object faces.
//
// The reference builds a scipy cKDTree of the SMPL vertices per frame on the host.  Here the search is brute force on the device, B frames per call:
//   nn_idx  = argmin_j |o_i - s_j|^2 on the squared fp32 distance ((dx dx + dy dy) + dz dz, no contraction), exact ties to the SMALLER index (the kd-tree's
//             tie order is not pinned), nn_dist = sqrtf of it, part = labels[nn_idx] where nn_dist < thres, else -1;
//   count, centre = per part: the number and the mean of the object vertices with that part -- the mean accumulated in fp64 in a fixed order and rounded
//             once to fp32, 0 where the part does not touch.
// PARITY UNPINNED: psbody's Sphere(centre, radius).to_mesh() is not installed, so the tessellation of a contact sphere is this project's own (an icosphere
// of two subdivisions, 162 vertices / 320 faces, built by visualize.icosphere); vt_contact_spheres only places a unit template handed to it.
//
// MI355X mapping: VALU only.  The searched cloud (6890 points) is the larger one and the queries are few (~1252 per frame), so a wave holds CT_Q queries
// (uniform across its lanes) and its 64 lanes take the candidates of an LDS chunk 64 apart: one ds_read_b128 feeds CT_Q pair tests, the lanes read
// consecutive float4 (conflict-free), and a 16-frame chunk makes ceil(1252 / 32) x 16 = 640 workgroups of 256 threads for 256 CUs.  A lane scans its
// candidates in ascending order with a strict compare, the 64 lanes then merge (distance, index) lexicographically: the winner is the smallest index
// among the minima whatever the lane count.  No float atomics anywhere: the per-part reduction is one wave per (frame, part) that walks the object
// vertices lane-strided and merges the fp64 partial sums through a fixed xor butterfly, so results are bit-identical from run to run and do not depend on
// B or on a frame's place in the batch.
#include "common.h"

#define CT_BLK 256
#define CT_Q 8                        /* queries per wave */
#define CT_WG_Q (CT_Q * CT_BLK / 64)  /* queries per workgroup */
#define CT_CHUNK 2048                 /* searched points per LDS chunk (32 KiB as float4) */
#define CT_MAX_PARTS 32

__global__ __launch_bounds__(CT_BLK) void ct_nn_kernel(const float *__restrict__ smpl, int NVs, const int *__restrict__ labels, const float *__restrict__ obj,
                                                      int NVo, float thres, int *__restrict__ nn_idx, float *__restrict__ nn_dist, int *__restrict__ part)
{
    __shared__ float4 sS[CT_CHUNK];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q0 = blockIdx.x * CT_WG_Q + wave * CT_Q;
    const float *sb = smpl + (size_t)b * NVs * 3, *ob = obj + (size_t)b * NVo * 3;
    float qx[CT_Q], qy[CT_Q], qz[CT_Q], best[CT_Q];
    int bj[CT_Q];
#pragma unroll
    for (int u = 0; u < CT_Q; u++) {
        const int i = min(q0 + u, NVo - 1);                       // queries past the end repeat the last one and are not written
        qx[u] = ob[3 * i]; qy[u] = ob[3 * i + 1]; qz[u] = ob[3 * i + 2];
        best[u] = INFINITY; bj[u] = 0x7fffffff;
    }
    for (int c0 = 0; c0 < NVs; c0 += CT_CHUNK) {
        const int cn = min(CT_CHUNK, NVs - c0);
        __syncthreads();
        for (int t = threadIdx.x; t < cn; t += CT_BLK) sS[t] = make_float4(sb[3 * (c0 + t)], sb[3 * (c0 + t) + 1], sb[3 * (c0 + t) + 2], 0.f);
        __syncthreads();
        for (int j = lane; j < cn; j += 64) {
            const float4 s = sS[j];
#pragma unroll
            for (int u = 0; u < CT_Q; u++) {
                const float d0 = qx[u] - s.x, d1 = qy[u] - s.y, d2 = qz[u] - s.z;
                const float d = d0 * d0 + d1 * d1 + d2 * d2;
                if (d < best[u]) { best[u] = d; bj[u] = c0 + j; }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < CT_Q; u++) {
        float d = best[u]; int j = bj[u];
        for (int o = 32; o > 0; o >>= 1) {
            const float d2 = __shfl_xor(d, o, 64); const int j2 = __shfl_xor(j, o, 64);
            if (d2 < d || (d2 == d && j2 < j)) { d = d2; j = j2; }
        }
        const int i = q0 + u;
        if (lane == 0 && i < NVo) {
            const bool found = j < NVs;                                // false only where every distance is NaN
            const float dist = found ? sqrtf(d) : INFINITY;
            const size_t o = (size_t)b * NVo + i;
            nn_idx[o] = found ? j : -1; nn_dist[o] = dist; part[o] = dist < thres ? labels[j] : -1;
        }
    }
}

// one wave per (frame, part): count and fp64 mean of the object vertices with that part
__global__ __launch_bounds__(64) void ct_reduce_kernel(const float *__restrict__ obj, int NVo, const int *__restrict__ part, int P, int *__restrict__ count,
                                                      float *__restrict__ centre)
{
    const int p = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const float *ob = obj + (size_t)b * NVo * 3;
    const int *pb = part + (size_t)b * NVo;
    double sx = 0, sy = 0, sz = 0; int n = 0;
    for (int i = lane; i < NVo; i += 64)
        if (pb[i] == p) { sx += (double)ob[3 * i]; sy += (double)ob[3 * i + 1]; sz += (double)ob[3 * i + 2]; n++; }
    for (int o = 32; o > 0; o >>= 1) {
        sx += __shfl_xor(sx, o, 64); sy += __shfl_xor(sy, o, 64); sz += __shfl_xor(sz, o, 64); n += __shfl_xor(n, o, 64);
    }
    if (lane == 0) {
        const size_t o = (size_t)b * P + p;
        count[o] = n;
        centre[3 * o] = n ? (float)(sx / n) : 0.f; centre[3 * o + 1] = n ? (float)(sy / n) : 0.f; centre[3 * o + 2] = n ? (float)(sz / n) : 0.f;
    }
}

extern "C" int vt_contact_regions(const float *smpl_verts, const int *labels, const float *obj_verts, int B, int NVs, int NVo, int P, float thres, int *nn_idx,
                                  float *nn_dist, int *part, int *count, float *centre, void *stream)
{
    VT_REQUIRE(smpl_verts && labels && obj_verts && nn_idx && nn_dist && part && count && centre && B > 0 && B <= 65535 && NVs > 0 && NVo > 0 && P > 0
               && P <= CT_MAX_PARTS, "vt_contact_regions: bad argument (1 <= B <= 65535, 1 <= P <= 32)");
    hipStream_t st = vt_stream(stream);
    hipLaunchKernelGGL(ct_nn_kernel, dim3((NVo + CT_WG_Q - 1) / CT_WG_Q, B), dim3(CT_BLK), 0, st, smpl_verts, NVs, labels, obj_verts, NVo, thres, nn_idx, nn_dist, part);
    VT_LAUNCH_CHECK();
    hipLaunchKernelGGL(ct_reduce_kernel, dim3(P, B), dim3(64), 0, st, obj_verts, NVo, part, P, count, centre);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

// out (B, P NSV, 3): sphere p of frame b = centre + radius * unit, every vertex AT the (zero) centre where the part does not touch: the faces of an
// absent sphere have three identical corners, which rnd_setup (render.hip) culls (den == 0) before binning -- no pixel, no tile-list entry
__global__ __launch_bounds__(256) void ct_spheres_kernel(const float *__restrict__ centre, const int *__restrict__ count, const float *__restrict__ unit, int NSV,
                                                        float radius, float *__restrict__ out)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x, bp = blockIdx.y;
    if (v >= NSV) return;
    const bool present = count[bp] > 0;
    float *o = out + ((size_t)bp * NSV + v) * 3;
#pragma unroll
    for (int e = 0; e < 3; e++) o[e] = present ? centre[3 * bp + e] + radius * unit[3 * v + e] : centre[3 * bp + e];
}

extern "C" int vt_contact_spheres(const float *centre, const int *count, int B, int P, const float *unit_verts, int NSV, float radius, float *out, void *stream)
{
    VT_REQUIRE(centre && count && unit_verts && out && B > 0 && P > 0 && NSV > 0 && (long long)B * P <= 65535, "vt_contact_spheres: bad argument (B P <= 65535)");
    hipLaunchKernelGGL(ct_spheres_kernel, dim3((NSV + 255) / 256, B * P), dim3(256), 0, vt_stream(stream), centre, count, unit_verts, NSV, radius, out);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

// out (B,NF,3) = base, except the object's faces [face_off, face_off + NFo) with a vertex in contact: those take the palette colour of the HIGHEST part
// among their corners (nr_utils.py:114-122 applies the parts in ascending order, every one overwriting the faces it touches)
__global__ __launch_bounds__(256) void ct_face_colors_kernel(const int *__restrict__ part, int NVo, const int *__restrict__ obj_faces, int NFo, int face_off,
                                                            const float *__restrict__ base, int NF, const float *__restrict__ palette, int P, float *__restrict__ out)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (f >= NF) return;
    const float *c = base + 3 * (size_t)f;
    const int g = f - face_off;
    if (g >= 0 && g < NFo) {
        const int *pb = part + (size_t)b * NVo;
        const int p = max(pb[obj_faces[3 * g]], max(pb[obj_faces[3 * g + 1]], pb[obj_faces[3 * g + 2]]));
        if (p >= 0 && p < P) c = palette + 3 * p;
    }
    float *o = out + ((size_t)b * NF + f) * 3;
    o[0] = c[0]; o[1] = c[1]; o[2] = c[2];
}

extern "C" int vt_contact_face_colors(const int *part, int B, int NVo, const int *obj_faces, int NFo, int face_off, const float *base_colors, int NF,
                                      const float *palette, int P, float *out, void *stream)
{
    VT_REQUIRE(part && obj_faces && base_colors && palette && out && B > 0 && B <= 65535 && NVo > 0 && NFo > 0 && NF > 0 && P > 0 && face_off >= 0
               && (long long)face_off + NFo <= NF, "vt_contact_face_colors: bad argument");
    hipLaunchKernelGGL(ct_face_colors_kernel, dim3((NF + 255) / 256, B), dim3(256), 0, vt_stream(stream), part, NVo, obj_faces, NFo, face_off, base_colors, NF, palette, P, out);
    VT_LAUNCH_CHECK();
    return VT_OK;
}
