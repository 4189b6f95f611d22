// pmdist.hip -- exact point-to-mesh distance with closest point, and nearest mesh vertex: the ground-truth labels of SIF-Net's training samples
// (preprocess/boundary_sampler.py:75-100 compute_labels: igl.signed_distance(...) -> |distance| and closest surface point per mesh,
// trimesh.proximity.ProximityQuery.vertex -> nearest SMPL vertex -> body part).
//
// PARITY UNPINNED, RESTATED FROM THE GEOMETRIC DEFINITION: igl, trimesh and psbody are not installed, nothing could be recorded from them.  What is
// computed is the definition those calls implement -- min over the triangles of the distance to the closest point of the triangle, and the nearest
// vertex in the Euclidean metric -- pinned by the float64 brute force of tests/pmdist_model.py.  The reference searches an AABB tree per frame and mesh on
// the host; here the search is brute force with culling on the device, B frames a call.
//
// Closest point on a triangle (a, b, c) to p, by Voronoi region (C. Ericson, Real-Time Collision Detection, 5.1.5), in fp32 and without contraction, from
// the differences ap = p - a, bp = p - b, cp = p - c and the edges ab = b - a, ac = c - a:
//   d1 = ab.ap  d2 = ac.ap  d3 = ab.bp  d4 = ac.bp  d5 = ab.cp  d6 = ac.cp,  dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z
//   d1 <= 0 and d2 <= 0                       -> a                      d3 >= 0 and d4 <= d3              -> b
//   vc = d1 d4 - d3 d2 <= 0, d1 >= 0, d3 <= 0 -> a + v ab, v = d1 / (d1 - d3)
//   d6 >= 0 and d5 <= d6                      -> c
//   vb = d5 d2 - d1 d6 <= 0, d2 >= 0, d6 <= 0 -> a + w ac, w = d2 / (d2 - d6)
//   va = d3 d6 - d5 d4 <= 0, d4 >= d3, d5 >= d6 -> b + w (c - b), w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
//   else                                      -> a + v ab + w ac, v = vb / (va + vb + vc), w = vc / (va + vb + vc)
// A quotient whose denominator is not positive is taken as 0 (the edge has no length: every parameter names the same point), and the interior weights
// are brought back into v, w >= 0, v + w <= 1 should rounding have carried them out: the point written out always lies on the triangle.
// No NaN for finite inputs.
//
// Which triangle wins: every triangle the culling leaves is evaluated in fp32 as above.  fp32 cannot order two triangles whose distances differ by less than
// its rounding (a query on the bisector of a concave edge: two closest points a fraction of a millimetre apart, distances 1e-9 m apart), so the choice is
// left to an ARBITER: a triangle whose fp32 distance is <= sqrtf(best) (1 + 5e-6) + tau / 2, with best the smallest fp32 squared distance met so far and
// tau = 2e-6 (|p.x| + |p.y| + |p.z|) (30 roundings of a coordinate; measured fp32 deficit of the true winner on the tests' inputs: 2.4e-7 m at tau / 2 >=
// 1.2e-6 m), is evaluated once more by the same rule in fp64 from the same fp32 corners, and the minimum of THOSE values decides: face_id = the smallest face
// index attaining the fp64 minimum, closest = its fp64 closest point rounded to fp32, dist = sqrtf(|p - closest|^2) in fp32 of THAT fp32 point.  The true
// winner is a candidate whenever it is visited (best only decreases), so the outcome does not depend on the order of the triangles.  RANGE ASSUMPTION: the
// fp32 error of a triangle's distance is a few 6e-8 of the largest of |p|, |corner| and |p - corner|, and tau knows |p| only.  It covers the error while the
// corners of the near-minimal triangles are not much farther from the origin, or from p, than ~10 (|p.x| + |p.y| + |p.z|) -- scenes in camera space with
// triangles of centimetres, the sampler's case.  For a query near the origin against a triangle with corners of much larger coordinates the true winner may
// miss the arbiter: face_id and closest are then those of the fp32 order, one of the triangles tied within fp32 rounding; dist stays within that rounding.  After the first few
// tiles a lane sends a handful of triangles to the arbiter.
//
// Degenerate triangles: the set-up kernel recognises a triangle whose squared area |ab x ac|^2 is <= 1e-12 |ab|^2 |ac|^2 (all of its corners on one line
// within fp32 rounding, or two of them equal) and writes it as (e0, e1, e1) with e0, e1 the ends of its longest edge: a segment, or a point.  For such a
// record d3 == d4 and d5 == d6 == d3, so va, vb, vc are exactly 0 and the rule above ends in the a, b or edge-ab case.
//
// Culling: the record carries a bounding sphere (centre = mean of the corners, radius = the largest corner distance, inflated by 1e-5).  A triangle is
// skipped for a lane when |p - centre|^2 > (sqrtf(best) (1 + 1e-5) + tau + radius)^2 with best = the lane's current fp32 minimum; the sphere lower bound then
// exceeds the arbiter's threshold by 5e-6 sqrtf(best) + tau / 2 + 1e-5 radius at least, well above the fp32 rounding of either side (a few 6e-8 of
// |p - centre| + radius), so a culled triangle can be no candidate of the arbiter and every output is bit-identical with culling on or off (tests/test_gpu_boundary.py checks that through
// vt_point_mesh_distance_ex).  A record is skipped by a whole wave only when no lane needs it (one wave-wide vote per record: no divergence); when one lane
// needs it all 64 evaluate it, which changes nothing since the minimum is order-free.
//
// MI355X mapping: VALU only, one thread per query point, 256 points of one frame per workgroup.  Triangle records (4 float4 = 64 B: sphere, a, b, c) are
// written per frame by pm_setup_kernel and staged through LDS in tiles of 256 (16 KiB); every lane reads the same record = an LDS broadcast, no bank
// conflict.  No atomics besides the optional test counter, results independent of B and of a frame's place in the batch.
#include "common.h"

#define PM_BLK 256
#define PM_TILE 256                   /* triangle records per LDS tile: 4 float4 each, 16 KiB */
#define PM_VTILE 1024                 /* vertices per LDS tile of the nearest-vertex kernel, 16 KiB */
#define PM_SLACK 1.00001f

template <typename T>
__host__ __device__ __forceinline__ T pm_dot(T ax, T ay, T az, T bx, T by, T bz) { return (ax * bx + ay * by) + az * bz; }

// one record per (frame, face): rec[4 i] = (sphere centre, inflated radius), rec[4 i + 1 .. 3] = corners (w unused).  Vertex indices are clamped into
// [0, NV) for memory safety (the host wrapper rejects meshes with indices outside it).
__global__ __launch_bounds__(PM_BLK) void pm_setup_kernel(const float *__restrict__ verts, int NV, const int *__restrict__ faces, int NF, float4 *__restrict__ rec)
{
    const int f = blockIdx.x * PM_BLK + threadIdx.x, b = blockIdx.y;
    if (f >= NF) return;
    const float *vb = verts + (size_t)b * NV * 3;
    float c[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int i = min(max(faces[3 * f + k], 0), NV - 1);
        c[k][0] = vb[3 * i]; c[k][1] = vb[3 * i + 1]; c[k][2] = vb[3 * i + 2];
    }
    float e[3][3], l2[3];                                     // edges 0: a->b, 1: a->c, 2: b->c
#pragma unroll
    for (int k = 0; k < 3; k++) { e[0][k] = c[1][k] - c[0][k]; e[1][k] = c[2][k] - c[0][k]; e[2][k] = c[2][k] - c[1][k]; }
#pragma unroll
    for (int k = 0; k < 3; k++) l2[k] = pm_dot(e[k][0], e[k][1], e[k][2], e[k][0], e[k][1], e[k][2]);
    const float nx = e[0][1] * e[1][2] - e[0][2] * e[1][1], ny = e[0][2] * e[1][0] - e[0][0] * e[1][2], nz = e[0][0] * e[1][1] - e[0][1] * e[1][0];
    if (pm_dot(nx, ny, nz, nx, ny, nz) <= 1e-12f * (l2[0] * l2[1])) {      // no area: keep the longest edge as (e0, e1, e1)
        int s = 0, t = 1;                                     // ends of edge 0
        if (l2[1] > l2[0] && l2[1] >= l2[2]) { s = 0; t = 2; }
        else if (l2[2] > l2[0] && l2[2] > l2[1]) { s = 1; t = 2; }
        float p0[3], p1[3];
#pragma unroll
        for (int k = 0; k < 3; k++) { p0[k] = c[s][k]; p1[k] = c[t][k]; }
#pragma unroll
        for (int k = 0; k < 3; k++) { c[0][k] = p0[k]; c[1][k] = p1[k]; c[2][k] = p1[k]; }
    }
    float m[3], r2 = 0.f;
#pragma unroll
    for (int k = 0; k < 3; k++) m[k] = (c[0][k] + c[1][k] + c[2][k]) * (1.f / 3.f);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float dx = c[k][0] - m[0], dy = c[k][1] - m[1], dz = c[k][2] - m[2];
        r2 = fmaxf(r2, pm_dot(dx, dy, dz, dx, dy, dz));
    }
    float4 *o = rec + ((size_t)b * NF + f) * 4;
    o[0] = make_float4(m[0], m[1], m[2], sqrtf(r2) * PM_SLACK);
#pragma unroll
    for (int k = 0; k < 3; k++) o[1 + k] = make_float4(c[k][0], c[k][1], c[k][2], 0.f);
}

// closest point of triangle (a, b, c) to p by Voronoi region (the file header states the rule), evaluated in T; returns |p - closest|^2
template <typename T>
__host__ __device__ __forceinline__ T pm_closest(T px, T py, T pz, const float4 a4, const float4 b4, const float4 c4, T &qx, T &qy, T &qz)
{
    const T ax = a4.x, ay = a4.y, az = a4.z, bx = b4.x, by = b4.y, bz = b4.z, cx = c4.x, cy = c4.y, cz = c4.z;
    const T abx = bx - ax, aby = by - ay, abz = bz - az, acx = cx - ax, acy = cy - ay, acz = cz - az;
    const T apx = px - ax, apy = py - ay, apz = pz - az, bpx = px - bx, bpy = py - by, bpz = pz - bz, cpx = px - cx, cpy = py - cy, cpz = pz - cz;
    const T d1 = pm_dot<T>(abx, aby, abz, apx, apy, apz), d2 = pm_dot<T>(acx, acy, acz, apx, apy, apz);
    const T d3 = pm_dot<T>(abx, aby, abz, bpx, bpy, bpz), d4 = pm_dot<T>(acx, acy, acz, bpx, bpy, bpz);
    const T d5 = pm_dot<T>(abx, aby, abz, cpx, cpy, cpz), d6 = pm_dot<T>(acx, acy, acz, cpx, cpy, cpz);
    const T vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const T zero = 0, one = 1;
    T v, w;                                                   // closest = a + v ab + w ac
    if (d1 <= zero && d2 <= zero) { v = zero; w = zero; }
    else if (d3 >= zero && d4 <= d3) { v = one; w = zero; }
    else if (vc <= zero && d1 >= zero && d3 <= zero) { const T den = d1 - d3; v = den > zero ? d1 / den : zero; w = zero; }
    else if (d6 >= zero && d5 <= d6) { v = zero; w = one; }
    else if (vb <= zero && d2 >= zero && d6 <= zero) { const T den = d2 - d6; v = zero; w = den > zero ? d2 / den : zero; }
    else if (va <= zero && d4 >= d3 && d5 >= d6) { const T num = d4 - d3, den = num + (d5 - d6); w = den > zero ? num / den : zero; v = one - w; }
    else {
        const T den = (va + vb) + vc;
        v = den > zero && vb > zero ? vb / den : zero; w = den > zero && vc > zero ? vc / den : zero;
        const T s = v + w;
        if (s > one) { v = v / s; w = w / s; }
    }
    qx = ax + (v * abx + w * acx); qy = ay + (v * aby + w * acy); qz = az + (v * abz + w * acz);
    const T dx = px - qx, dy = py - qy, dz = pz - qz;
    return pm_dot<T>(dx, dy, dz, dx, dy, dz);
}

template <bool CULL, bool COUNT>
__global__ __launch_bounds__(PM_BLK) void pm_dist_kernel(const float *__restrict__ points, int N, const float4 *__restrict__ rec, int NF, float *__restrict__ dist,
                                                        float *__restrict__ closest, int *__restrict__ face_id, unsigned long long *__restrict__ n_tests)
{
    __shared__ float4 sR[PM_TILE * 4];
    const int b = blockIdx.y, i = blockIdx.x * PM_BLK + threadIdx.x;
    const bool live = i < N;
    const float *pp = points + ((size_t)b * N + (live ? i : N - 1)) * 3;        // lanes past the end repeat the last point and write nothing
    const float px = pp[0], py = pp[1], pz = pp[2];
    const float4 *rb = rec + (size_t)b * NF * 4;
    // best = the smallest fp32 squared distance met so far; tau = the absolute slack, 30 x the rounding of a coordinate of p; a triangle goes to the arbiter
    // when its fp32 distance is <= sqrtf(best) (1 + 5e-6) + tau / 2 (cand, squared) and is culled beyond sqrtf(best) (1 + 1e-5) + tau (reach) + radius
    const float tau = 2e-6f * (fabsf(px) + fabsf(py) + fabsf(pz));
    float best = INFINITY, cand = INFINITY, reach = INFINITY, qx = 0.f, qy = 0.f, qz = 0.f;
    double best64 = INFINITY;                                                     // the arbiter's minimum, and (bf, q) the face and point attaining it
    int bf = 0;
    unsigned int tests = 0;
    for (int t0 = 0; t0 < NF; t0 += PM_TILE) {
        const int tn = min(PM_TILE, NF - t0);
        __syncthreads();
        for (int t = threadIdx.x; t < tn * 4; t += PM_BLK) sR[t] = rb[(size_t)t0 * 4 + t];
        __syncthreads();
        for (int j = 0; j < tn; j++) {
            if (CULL) {
                const float4 s = sR[4 * j];
                const float dx = px - s.x, dy = py - s.y, dz = pz - s.z, lim = reach + s.w;
                const bool need = !(pm_dot<float>(dx, dy, dz, dx, dy, dz) > lim * lim);
                if (!__any(need)) continue;
            }
            float cx, cy, cz;
            const float d = pm_closest<float>(px, py, pz, sR[4 * j + 1], sR[4 * j + 2], sR[4 * j + 3], cx, cy, cz);
            if (COUNT) tests++;
            if (d <= cand) {                                  // as near as the minimum within rounding: the arbiter decides (rare once the minimum has settled)
                double ex, ey, ez;
                const double d64 = pm_closest<double>((double)px, (double)py, (double)pz, sR[4 * j + 1], sR[4 * j + 2], sR[4 * j + 3], ex, ey, ez);
                if (d64 < best64) { best64 = d64; bf = t0 + j; qx = (float)ex; qy = (float)ey; qz = (float)ez; }
                if (d < best) { const float r = sqrtf(d), c = r * 1.000005f + 0.5f * tau; best = d; cand = c * c; reach = r * PM_SLACK + tau; }
            }
        }
    }
    if (COUNT) {
        unsigned long long n = live ? tests : 0u;
        for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
        if ((threadIdx.x & 63) == 0) atomicAdd(n_tests, n);
    }
    if (!live) return;
    const size_t o = (size_t)b * N + i;
    const float dx = px - qx, dy = py - qy, dz = pz - qz;
    dist[o] = sqrtf(pm_dot<float>(dx, dy, dz, dx, dy, dz));
    if (closest) { closest[3 * o] = qx; closest[3 * o + 1] = qy; closest[3 * o + 2] = qz; }
    if (face_id) face_id[o] = bf;
}

// nearest vertex on the squared fp32 distance, exact ties to the smaller index; vert_dist = its sqrtf
__global__ __launch_bounds__(PM_BLK) void pm_vertex_kernel(const float *__restrict__ points, int N, const float *__restrict__ verts, int NV, int *__restrict__ vert_id,
                                                          float *__restrict__ vert_dist)
{
    __shared__ float4 sV[PM_VTILE];
    const int b = blockIdx.y, i = blockIdx.x * PM_BLK + threadIdx.x;
    const bool live = i < N;
    const float *pp = points + ((size_t)b * N + (live ? i : N - 1)) * 3;
    const float px = pp[0], py = pp[1], pz = pp[2];
    const float *vb = verts + (size_t)b * NV * 3;
    float best = INFINITY;
    int bj = 0;
    for (int t0 = 0; t0 < NV; t0 += PM_VTILE) {
        const int tn = min(PM_VTILE, NV - t0);
        __syncthreads();
        for (int t = threadIdx.x; t < tn; t += PM_BLK) sV[t] = make_float4(vb[3 * (size_t)(t0 + t)], vb[3 * (size_t)(t0 + t) + 1], vb[3 * (size_t)(t0 + t) + 2], 0.f);
        __syncthreads();
        for (int j = 0; j < tn; j++) {
            const float4 s = sV[j];
            const float dx = px - s.x, dy = py - s.y, dz = pz - s.z;
            const float d = pm_dot(dx, dy, dz, dx, dy, dz);
            if (d < best) { best = d; bj = t0 + j; }
        }
    }
    if (!live) return;
    const size_t o = (size_t)b * N + i;
    vert_id[o] = bj;
    if (vert_dist) vert_dist[o] = sqrtf(best);
}

extern "C" long vt_point_mesh_workspace_bytes(int B, int n_faces)
{
    if (B <= 0 || n_faces <= 0) return -1;
    return (long)B * n_faces * 4 * (long)sizeof(float4);
}

extern "C" int vt_point_mesh_distance_ex(const float *points, int n_points, const float *verts, int n_verts, const int *faces, int n_faces, int B, float *dist,
                                         float *closest, int *face_id, void *workspace, int flags, unsigned long long *n_tests, void *stream)
{
    VT_REQUIRE(points && verts && faces && dist && workspace && n_points > 0 && n_verts > 0 && n_faces > 0 && B > 0 && B <= 65535,
               "vt_point_mesh_distance: bad argument (null pointer, a size <= 0 or B > 65535)");
    VT_REQUIRE(((size_t)workspace & 15) == 0, "vt_point_mesh_distance: workspace must be 16-byte aligned");
    VT_REQUIRE((flags & ~1) == 0, "vt_point_mesh_distance_ex: flags is 0 or 1");
    hipStream_t st = vt_stream(stream);
    float4 *rec = static_cast<float4 *>(workspace);
    hipLaunchKernelGGL(pm_setup_kernel, dim3((n_faces + PM_BLK - 1) / PM_BLK, B), dim3(PM_BLK), 0, st, verts, n_verts, faces, n_faces, rec);
    VT_LAUNCH_CHECK();
    const dim3 grid((n_points + PM_BLK - 1) / PM_BLK, B), blk(PM_BLK);
    const bool cull = !(flags & 1);
    if (n_tests) {
        if (cull) hipLaunchKernelGGL((pm_dist_kernel<true, true>), grid, blk, 0, st, points, n_points, rec, n_faces, dist, closest, face_id, n_tests);
        else hipLaunchKernelGGL((pm_dist_kernel<false, true>), grid, blk, 0, st, points, n_points, rec, n_faces, dist, closest, face_id, n_tests);
    } else {
        if (cull) hipLaunchKernelGGL((pm_dist_kernel<true, false>), grid, blk, 0, st, points, n_points, rec, n_faces, dist, closest, face_id, n_tests);
        else hipLaunchKernelGGL((pm_dist_kernel<false, false>), grid, blk, 0, st, points, n_points, rec, n_faces, dist, closest, face_id, n_tests);
    }
    VT_LAUNCH_CHECK();
    return VT_OK;
}

extern "C" int vt_point_mesh_distance(const float *points, int n_points, const float *verts, int n_verts, const int *faces, int n_faces, int B, float *dist,
                                      float *closest, int *face_id, void *workspace, void *stream)
{
    return vt_point_mesh_distance_ex(points, n_points, verts, n_verts, faces, n_faces, B, dist, closest, face_id, workspace, 0, nullptr, stream);
}

extern "C" int vt_nearest_vertex(const float *points, int n_points, const float *verts, int n_verts, int B, int *vert_id, float *vert_dist, void *stream)
{
    VT_REQUIRE(points && verts && vert_id && n_points > 0 && n_verts > 0 && B > 0 && B <= 65535, "vt_nearest_vertex: bad argument (null pointer, a size <= 0 or B > 65535)");
    hipLaunchKernelGGL(pm_vertex_kernel, dim3((n_points + PM_BLK - 1) / PM_BLK, B), dim3(PM_BLK), 0, vt_stream(stream), points, n_points, verts, n_verts, vert_id,
                       vert_dist);
    VT_LAUNCH_CHECK();
    return VT_OK;
}
