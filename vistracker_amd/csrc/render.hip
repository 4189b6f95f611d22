// render.hip -- shaded mesh rasteriser of the visualisation step (demo.sh step 7: render/render_side_comp.py RendererSide2side on top of
// render/nr_utils.py NrWrapper.render_meshes -> neural_renderer.Renderer.render in RGB mode).
//
// PARITY UNPINNED: neural_renderer is third-party (not vendored, not installable here).  Its RGB rule, restated from the library's published
// behaviour (Kato et al. 2018 "Neural 3D Mesh Renderer" and its Renderer.render / lighting / projection / rasterize_rgbad), with the conventions
// vt_sil_forward (sil.hip) already states for silhouettes:
//   fill_back : the faces are doubled with reversed winding ([i2, i1, i0]); each copy keeps its colour.  Doubled id of face f of an F-face scene:
//               f (as given), F + f (reversed).
//   lighting  : per face, on the vertices BEFORE projection (camera coordinates) of the face as listed:
//               n = normalize(cross(v0 - v1, v2 - v1), eps 1e-5),  light = I_amb c_amb + I_dir c_dir relu(n . d)  (d as given, not normalised),
//               colour = face colour * light.
//   projection: x' = x / (z + 1e-9), y' = y / (z + 1e-9), [u v] = K [x' y' 1], v <- os - v, (u, v) <- 2 (. - os/2) / os   (os = orig_size).
//   raster    : front faces only (the test of sil.hip), pixel (xi, yi) of an is x is image covered when its centre ((2 xi + 1 - is)/is,
//               (2 yi + 1 - is)/is) is inside the triangle and near 0.1 < z < far 100 for the perspective-correct depth; the nearest face wins,
//               exact ties go to the smaller doubled id; image row 0 shows yi = is - 1.  Uncovered pixels: background colour, alpha 0, depth far.
//   anti_aliasing: the scene is drawn at 2 size and every channel (rgb, alpha, depth) is averaged over 2 x 2 blocks.
// The inside test and the depth formula are copies of sil.hip's (sil_inside / sil_vote, round 6 fast path included), so coverage and owners are
// bit-identical to vt_sil_forward's under its K convention (orig_size 1, no anti-aliasing) -- tests/test_gpu_render.py holds both to that.
//
// MI355X mapping: VALU + LDS, no MFMA, no atomics on colours.  Four launches per batch of views:
//   rnd_setup   one thread per (view, face): projection, front test (picks the orientation that faces the camera), lighting of that
//               orientation, pixel box (sil.hip's box formula), 64-byte face record + 8-byte box;
//   rnd_count / rnd_scan / rnd_fill   bin the boxes to 16 x 16 pixel tiles: a count per tile (integer atomics), one exclusive scan, a fill.
//               A face costs one list entry per tile its box touches, whatever its pixel area;
//   rnd_resolve one 256-thread workgroup per (view, tile): the tile's list is staged through LDS 256 records at a time, every pixel keeps the
//               smallest (depth bits << 32 | doubled id) key and the colour of its owner, then writes rgb / alpha / depth / owner, with the
//               2 x 2 anti-aliasing average fused (LDS exchange inside the tile).
// The list order within a tile depends on scheduling; the result does not (the minimum of a set of keys), so images are bitwise deterministic.
// Static layer (vt_render_static_create): a scene part shared by every view of a camera (the ground checkerboard) is set up, binned and resolved
// ONCE into a per-pixel key map with layer-local ids; a view's resolve starts from that key, renumbered into the concatenated scene
// [mesh faces, layer faces] (local s -> NF + s, reversed NS + s -> 2 NF + NS + s: monotone, so the minimum is that of the concatenated scene).
#include "common.h"

#define RND_NEAR 0.1f
#define RND_FAR 100.0f
#define RND_TILE 16
#define RND_RIM 0.015625f
#define RND_NONE 0xffffffffffffffffull

struct RndLight { float ia, id, ca[3], cd[3], dir[3]; };

// ---- copies of sil.hip's device helpers (sil_inside, sil_ndc, the depth of sil_vote): that file stays untouched --------------------------------
__device__ __forceinline__ bool rnd_inside(const float (&fc)[9], float xp, float yp)
{
    return !(((yp - fc[1]) * (fc[3] - fc[0]) < (xp - fc[0]) * (fc[4] - fc[1])) ||
             ((yp - fc[4]) * (fc[6] - fc[3]) < (xp - fc[3]) * (fc[7] - fc[4])) ||
             ((yp - fc[7]) * (fc[0] - fc[6]) < (xp - fc[6]) * (fc[1] - fc[7])));
}
__device__ __forceinline__ void rnd_ndc(int xi, int yi, int is, bool pow2, float ris, float &xp, float &yp)
{
    const float xn = 2.0f * xi + 1 - is, yn = 2.0f * yi + 1 - is;
    xp = pow2 ? xn * ris : xn / is; yp = pow2 ? yn * ris : yn / is;
}
// perspective-correct depth of a covered pixel centre, or -1 when it fails near < z < far.  Pixels well inside the triangle (every barycentric
// weight in (1/64, 1 - 1/64)) take reciprocal multiplies, pixels on the rim neural_renderer's formula division for division (sil.hip, round 6).
__device__ __forceinline__ float rnd_depth(const float (&fc)[9], float den, float xp, float yp)
{
    const float n0 = (fc[4] - fc[7]) * xp + (fc[6] - fc[3]) * yp + (fc[3] * fc[7] - fc[6] * fc[4]);
    const float n1 = (fc[7] - fc[1]) * xp + (fc[0] - fc[6]) * yp + (fc[6] * fc[1] - fc[0] * fc[7]);
    const float n2 = (fc[1] - fc[4]) * xp + (fc[3] - fc[0]) * yp + (fc[0] * fc[4] - fc[3] * fc[1]);
    {
        const float rden = __builtin_amdgcn_rcpf(den);
        const float a0 = n0 * rden, a1 = n1 * rden, a2 = n2 * rden;
        if (fminf(a0, fminf(a1, a2)) > RND_RIM && fmaxf(a0, fmaxf(a1, a2)) < 1.0f - RND_RIM) {
            const float ws_ = a0 + a1 + a2;
            const float zp_ = ws_ * __builtin_amdgcn_rcpf(a0 * __builtin_amdgcn_rcpf(fc[2]) + a1 * __builtin_amdgcn_rcpf(fc[5]) + a2 * __builtin_amdgcn_rcpf(fc[8]));
            if (zp_ > RND_NEAR * 1.001f && zp_ < RND_FAR * 0.999f) return zp_;
        }
    }
    // (the coefficients are divided by den first, as neural_renderer and sil.hip's sil_vote do: the two rasterisers stay bit-identical)
    float w0 = (fc[4] - fc[7]) / den * xp + (fc[6] - fc[3]) / den * yp + (fc[3] * fc[7] - fc[6] * fc[4]) / den;
    float w1 = (fc[7] - fc[1]) / den * xp + (fc[0] - fc[6]) / den * yp + (fc[6] * fc[1] - fc[0] * fc[7]) / den;
    float w2 = (fc[1] - fc[4]) / den * xp + (fc[3] - fc[0]) / den * yp + (fc[0] * fc[4] - fc[3] * fc[1]) / den;
    w0 = fminf(fmaxf(w0, 0.f), 1.f); w1 = fminf(fmaxf(w1, 0.f), 1.f); w2 = fminf(fmaxf(w2, 0.f), 1.f);
    const float ws = w0 + w1 + w2;
    const float zp = 1.0f / (w0 / ws / fc[2] + w1 / ws / fc[5] + w2 / ws / fc[8]);
    return (zp > RND_NEAR && zp < RND_FAR) ? zp : -1.0f;
}

// ---- set-up: one thread per (view, face) ---------------------------------------------------------------------------------------------------
// record (16 floats): corners x0 y0 z0 x1 y1 z1 x2 y2 z2 of the orientation that faces the camera (sil.hip's order: the reversed copy is
// [i0, i2, i1], the same triangle as neural_renderer's [i2, i1, i0]), den, lit r g b, doubled id (int bits), 2 spare.
// box: x0 | x1 << 16, y0 | y1 << 16 in pixels of the is x is raster (internal y-up); x0 > x1 = culled.
__device__ __forceinline__ void rnd_project(const float *v, const float *k, float os, float &u, float &w)
{
    const float z = v[2], x_ = v[0] / (z + 1e-9f), y_ = v[1] / (z + 1e-9f);
    const float uu = k[0] * x_ + k[1] * y_ + k[2];
    const float vv = os - (k[3] * x_ + k[4] * y_ + k[5]);
    const float h = os * 0.5f;
    u = 2.0f * (uu - h) / os; w = 2.0f * (vv - h) / os;
}
__device__ __forceinline__ bool rnd_front(const float (&fc)[9]) { return !((fc[7] - fc[1]) * (fc[3] - fc[0]) < (fc[4] - fc[1]) * (fc[6] - fc[0])); }
__device__ __forceinline__ int2 rnd_box(const float (&fc)[9], int is)
{
    const float xmin = fminf(fc[0], fminf(fc[3], fc[6])), xmax = fmaxf(fc[0], fmaxf(fc[3], fc[6]));
    const float ymin = fminf(fc[1], fminf(fc[4], fc[7])), ymax = fmaxf(fc[1], fmaxf(fc[4], fc[7]));
    const float fx0 = fminf(fmaxf(floorf((xmin * is + is - 1) * 0.5f) - 1.f, -1.f), (float)is), fx1 = fminf(fmaxf(ceilf((xmax * is + is - 1) * 0.5f) + 1.f, -1.f), (float)is);
    const float fy0 = fminf(fmaxf(floorf((ymin * is + is - 1) * 0.5f) - 1.f, -1.f), (float)is), fy1 = fminf(fmaxf(ceilf((ymax * is + is - 1) * 0.5f) + 1.f, -1.f), (float)is);
    int x0 = max((int)fx0, 0), x1 = min((int)fx1, is - 1), y0 = max((int)fy0, 0), y1 = min((int)fy1, is - 1);
    if (y0 > y1) { x0 = 1; x1 = 0; }
    return make_int2((x0 & 0xffff) | (x1 << 16), (y0 & 0xffff) | (y1 << 16));
}
__device__ __forceinline__ bool rnd_box_ok(int2 bb) { return (bb.x & 0xffff) <= (bb.x >> 16); }

__global__ __launch_bounds__(256) void rnd_setup_kernel(const float *__restrict__ verts, int NV, const int *__restrict__ faces, int NF,
                                                       const float *__restrict__ colors, long c_stride, const float *__restrict__ K, int k_stride, float os, int is,
                                                       RndLight L, int idA, int idB, float4 *__restrict__ rec, int2 *__restrict__ box)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (f >= NF) return;
    const float *vb = verts + (size_t)b * NV * 3, *k = K + (size_t)k_stride * b;
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    const float *v0 = vb + 3 * i0, *v1 = vb + 3 * i1, *v2 = vb + 3 * i2;
    float p[9];
    rnd_project(v0, k, os, p[0], p[1]); p[2] = v0[2];
    rnd_project(v1, k, os, p[3], p[4]); p[5] = v1[2];
    rnd_project(v2, k, os, p[6], p[7]); p[8] = v2[2];
    const float fa[9] = {p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8]};
    const float fb[9] = {p[0], p[1], p[2], p[6], p[7], p[8], p[3], p[4], p[5]};
    int2 bb = make_int2(1, 0);
    bool useA = false, useB = false;
    // no pixel of a face can pass near < z < far when all its corners are behind the camera, all in (0, near) or all beyond far (the
    // perspective-correct depth is a weighted harmonic mean of the corner depths): such faces are not binned
    const float zmin = fminf(p[2], fminf(p[5], p[8])), zmax = fmaxf(p[2], fmaxf(p[5], p[8]));
    const bool dead = zmax < 0.f || (zmin > 0.f && zmax < RND_NEAR * 0.999f) || zmin > RND_FAR * 1.001f;
    if (!dead) {
        if (rnd_front(fa)) { bb = rnd_box(fa, is); useA = rnd_box_ok(bb); }
        if (!useA && rnd_front(fb)) { bb = rnd_box(fb, is); useB = rnd_box_ok(bb); }
    }
    const float *fc = useB ? fb : fa;
    const float den = fc[0] * (fc[4] - fc[7]) + fc[3] * (fc[7] - fc[1]) + fc[6] * (fc[1] - fc[4]);
    if (!(useA || useB) || den == 0.f) bb = make_int2(1, 0);
    // lighting of the listed orientation: [i0, i1, i2] or neural_renderer's reversed copy [i2, i1, i0]
    const float *a = useB ? v2 : v0, *c = useB ? v0 : v2;
    const float e0[3] = {a[0] - v1[0], a[1] - v1[1], a[2] - v1[2]}, e1[3] = {c[0] - v1[0], c[1] - v1[1], c[2] - v1[2]};
    float n[3] = {e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]};
    const float nn = fmaxf(sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]), 1e-5f);
    n[0] = n[0] / nn; n[1] = n[1] / nn; n[2] = n[2] / nn;
    const float cs = fmaxf(n[0] * L.dir[0] + n[1] * L.dir[1] + n[2] * L.dir[2], 0.f);
    float rgb[3];
#pragma unroll
    for (int e = 0; e < 3; e++) {
        float l = 0.f + L.ia * L.ca[e];
        l = l + L.id * (L.cd[e] * cs);
        rgb[e] = colors[c_stride * b + 3 * f + e] * l;
    }
    const int id = useB ? idB + f : idA + f;
    float4 *r = rec + ((size_t)b * NF + f) * 4;
    r[0] = make_float4(fc[0], fc[1], fc[2], fc[3]);
    r[1] = make_float4(fc[4], fc[5], fc[6], fc[7]);
    r[2] = make_float4(fc[8], den, rgb[0], rgb[1]);
    r[3] = make_float4(rgb[2], __int_as_float(id), 0.f, 0.f);
    box[(size_t)b * NF + f] = bb;
}

// ---- binning: count, scan, fill ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rnd_count_kernel(const int2 *__restrict__ box, int NF, int tiles_x, int *__restrict__ cnt)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (f >= NF) return;
    const int2 bb = box[(size_t)b * NF + f];
    if (!rnd_box_ok(bb)) return;
    const int tx0 = (bb.x & 0xffff) / RND_TILE, tx1 = (bb.x >> 16) / RND_TILE, ty0 = (bb.y & 0xffff) / RND_TILE, ty1 = (bb.y >> 16) / RND_TILE;
    int *c = cnt + (size_t)b * tiles_x * tiles_x;
    for (int ty = ty0; ty <= ty1; ty++)
        for (int tx = tx0; tx <= tx1; tx++) atomicAdd(c + ty * tiles_x + tx, 1);
}
// exclusive scan of the n per-tile counts (all views) in one 1024-thread workgroup: off = cursor = start of each tile's list, total at the end
__global__ __launch_bounds__(1024) void rnd_scan_kernel(const int *__restrict__ cnt, int n, int *__restrict__ off, int *__restrict__ cursor,
                                                       long long *__restrict__ total)
{
    __shared__ long long s[1024];
    const int t = threadIdx.x, chunk = (n + 1023) / 1024, lo = min(t * chunk, n), hi = min(lo + chunk, n);
    long long sum = 0;
    for (int i = lo; i < hi; i++) sum += cnt[i];
    s[t] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const long long add = t >= o ? s[t - o] : 0;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    long long run = s[t] - sum;
    for (int i = lo; i < hi; i++) {
        const int o = (int)min(run, (long long)0x7fffffff);
        off[i] = o; cursor[i] = o; run += cnt[i];
    }
    if (t == 1023) *total = s[1023];
}
__global__ __launch_bounds__(256) void rnd_fill_kernel(const int2 *__restrict__ box, int NF, int tiles_x, int *__restrict__ cursor, long long cap,
                                                      int *__restrict__ list)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (f >= NF) return;
    const int2 bb = box[(size_t)b * NF + f];
    if (!rnd_box_ok(bb)) return;
    const int tx0 = (bb.x & 0xffff) / RND_TILE, tx1 = (bb.x >> 16) / RND_TILE, ty0 = (bb.y & 0xffff) / RND_TILE, ty1 = (bb.y >> 16) / RND_TILE;
    int *c = cursor + (size_t)b * tiles_x * tiles_x;
    for (int ty = ty0; ty <= ty1; ty++)
        for (int tx = tx0; tx <= tx1; tx++) {
            const int slot = atomicAdd(c + ty * tiles_x + tx, 1);
            if (slot < cap) list[slot] = f;
        }
}

// ---- resolve + shade ---------------------------------------------------------------------------------------------------------------------------
struct RndOut {
    float *rgb, *alpha, *depth; int *fidx;          // SHADE: (B,S,S,3), (B,S,S), (B,S,S) | NULL, (B,is,is) | NULL   (S = is / 2 with anti-aliasing)
    unsigned long long *keys;                        // !SHADE: (B,is,is) key map, internal y-up order (static layer)
    float bg[3]; int aa;
};
struct RndSeed {
    const unsigned long long *keys;                  // static layer key map (is,is) with layer-local ids, or NULL
    const float4 *rec; int NS; int NF;               // layer records (for the owner's colour), layer faces, mesh faces of this call
};
template <bool SHADE>
__global__ __launch_bounds__(256) void rnd_resolve_kernel(const float4 *__restrict__ rec, int NF, const int *__restrict__ cnt, const int *__restrict__ off,
                                                         const int *__restrict__ list, int is, int tiles_x, RndSeed seed, RndOut out)
{
    __shared__ float4 sRec[256][4];
    __shared__ float sPix[5][256];
    const int t = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int xi = tx * RND_TILE + (t & 15), yi = ty * RND_TILE + (t >> 4);
    const bool pow2 = (is & (is - 1)) == 0;
    const float ris = 1.0f / (float)is;
    float xp, yp; rnd_ndc(xi, yi, is, pow2, ris, xp, yp);
    unsigned long long best = RND_NONE;
    float col[3] = {out.bg[0], out.bg[1], out.bg[2]};
    if (SHADE && seed.keys) {
        const unsigned long long k = seed.keys[(size_t)yi * is + xi];
        if (k != RND_NONE) {
            const unsigned loc = (unsigned)(k & 0xffffffffull);
            const unsigned s = loc < (unsigned)seed.NS ? loc : loc - seed.NS;
            const unsigned glob = loc < (unsigned)seed.NS ? seed.NF + loc : 2 * seed.NF + loc;
            best = (k & 0xffffffff00000000ull) | glob;
            const float4 r2 = seed.rec[4 * s + 2], r3 = seed.rec[4 * s + 3];
            col[0] = r2.z; col[1] = r2.w; col[2] = r3.x;
        }
    }
    const size_t tb = (size_t)b * tiles_x * tiles_x + tile;
    const int start = off[tb], end = start + cnt[tb];
    const float4 *rb = rec + (size_t)b * NF * 4;
    for (int c0 = start; c0 < end; c0 += 256) {
        __syncthreads();
        if (c0 + t < end) {
            const float4 *r = rb + (size_t)list[c0 + t] * 4;
            sRec[t][0] = r[0]; sRec[t][1] = r[1]; sRec[t][2] = r[2]; sRec[t][3] = r[3];
        }
        __syncthreads();
        const int n = min(256, end - c0);
        for (int j = 0; j < n; j++) {
            const float4 a = sRec[j][0], bq = sRec[j][1], cq = sRec[j][2];
            const float fc[9] = {a.x, a.y, a.z, a.w, bq.x, bq.y, bq.z, bq.w, cq.x};
            if (!rnd_inside(fc, xp, yp)) continue;
            const float zp = rnd_depth(fc, cq.y, xp, yp);
            if (zp < 0.f) continue;
            const float4 dq = sRec[j][3];
            const unsigned long long key = ((unsigned long long)__float_as_uint(zp) << 32) | (unsigned)__float_as_int(dq.y);
            if (key < best) { best = key; col[0] = cq.z; col[1] = cq.w; col[2] = dq.x; }
        }
    }
    const bool cov = best != RND_NONE;
    if (!SHADE) { out.keys[((size_t)b * is + yi) * is + xi] = best; return; }
    const float z = cov ? __uint_as_float((unsigned)(best >> 32)) : RND_FAR;
    if (!cov) { col[0] = out.bg[0]; col[1] = out.bg[1]; col[2] = out.bg[2]; }
    const size_t o = ((size_t)b * is + (is - 1 - yi)) * is + xi;                    // image row 0 = top
    if (out.fidx) out.fidx[o] = cov ? (int)(unsigned)(best & 0xffffffffull) : -1;
    if (!out.aa) {
        out.rgb[3 * o] = col[0]; out.rgb[3 * o + 1] = col[1]; out.rgb[3 * o + 2] = col[2];
        out.alpha[o] = cov ? 1.f : 0.f;
        if (out.depth) out.depth[o] = z;
        return;
    }
    // fused 2 x 2 average: the window of output pixel (R, X) covers image rows 2R, 2R + 1 (internal yi = 2k + 1, 2k) and columns 2X, 2X + 1,
    // summed in that row-major order
    sPix[0][t] = col[0]; sPix[1][t] = col[1]; sPix[2][t] = col[2]; sPix[3][t] = cov ? 1.f : 0.f; sPix[4][t] = z;
    __syncthreads();
    if (t < 64) {
        const int ox = t & 7, oy = t >> 3, S = is / 2;
        const int q0 = (2 * oy + 1) * 16 + 2 * ox, q1 = q0 + 1, q2 = (2 * oy) * 16 + 2 * ox, q3 = q2 + 1;
        float v[5];
#pragma unroll
        for (int ch = 0; ch < 5; ch++) v[ch] = (((sPix[ch][q0] + sPix[ch][q1]) + sPix[ch][q2]) + sPix[ch][q3]) * 0.25f;
        const int X = tx * 8 + ox, R = S - 1 - (ty * 8 + oy);
        const size_t po = ((size_t)b * S + R) * S + X;
        out.rgb[3 * po] = v[0]; out.rgb[3 * po + 1] = v[1]; out.rgb[3 * po + 2] = v[2];
        out.alpha[po] = v[3];
        if (out.depth) out.depth[po] = v[4];
    }
}

// uint8 panels: out = (uint8)(clip(rgb, 0, 1) * 255) (truncation, render_side_comp.py:94) of rows [row0, row0 + nrows) x cols [col0, col0 + ncols)
// of each (B,size,size,3) view, written at out + view_off[b] with a row stride of out_row_stride bytes
__global__ __launch_bounds__(256) void rnd_panel_kernel(const float *__restrict__ rgb, int size, int row0, int nrows, int col0, int ncols,
                                                       unsigned char *__restrict__ out, const long long *__restrict__ view_off, long long out_row_stride)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y, b = blockIdx.z;
    if (c >= ncols * 3) return;
    const float x = rgb[(((size_t)b * size + row0 + r) * size + col0) * 3 + c];
    out[view_off[b] + (long long)r * out_row_stride + c] = (unsigned char)(int)(fminf(fmaxf(x, 0.f), 1.f) * 255.0f);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------
struct RndWs { float4 *rec; int2 *box; int *cnt, *off, *cur; long long *total; int *list; long long cap; };
static inline size_t rnd_align(size_t x) { return (x + 255) & ~(size_t)255; }
static inline size_t rnd_fixed_bytes(long B, long NF, long is)
{
    const long nt = (is / RND_TILE) * (is / RND_TILE);
    return rnd_align(B * NF * 64) + rnd_align(B * NF * 8) + 3 * rnd_align(B * nt * 4) + rnd_align(8);
}
static inline RndWs rnd_ws(void *ws, long ws_bytes, long B, long NF, long is)
{
    const long nt = (is / RND_TILE) * (is / RND_TILE);
    char *p = static_cast<char *>(ws);
    RndWs w;
    w.rec = reinterpret_cast<float4 *>(p); p += rnd_align(B * NF * 64);
    w.box = reinterpret_cast<int2 *>(p); p += rnd_align(B * NF * 8);
    w.cnt = reinterpret_cast<int *>(p); p += rnd_align(B * nt * 4);
    w.off = reinterpret_cast<int *>(p); p += rnd_align(B * nt * 4);
    w.cur = reinterpret_cast<int *>(p); p += rnd_align(B * nt * 4);
    w.total = reinterpret_cast<long long *>(p); p += rnd_align(8);
    w.list = reinterpret_cast<int *>(p);
    const long long rest = ws_bytes - (long long)(p - static_cast<char *>(ws));
    w.cap = rest > 0 ? rest / 4 : 0;
    if (w.cap > 0x7fffffffLL) w.cap = 0x7fffffffLL;
    return w;
}
extern "C" long vt_render_workspace_bytes(int B, int NF, int size, int anti_aliasing, long list_entries)
{
    const long is = (long)size * (anti_aliasing ? 2 : 1);
    return (long)rnd_fixed_bytes(B, NF, is) + 4L * list_entries;
}
static inline RndLight rnd_light(const float *l)
{
    RndLight L;
    L.ia = l[0]; L.id = l[1];
    for (int e = 0; e < 3; e++) { L.ca[e] = l[2 + e]; L.cd[e] = l[5 + e]; L.dir[e] = l[8 + e]; }
    return L;
}
// set-up + binning of B views of an NF-face scene; returns the list length through *total_host (the one host synchronisation of a call: the
// caller's workspace must hold the list)
static int rnd_bin(const float *verts, int B, int NV, const int *faces, int NF, const float *colors, long c_stride, const float *K, int k_stride, float os, int is,
                   const RndLight &L, int idA, int idB, const RndWs &w, long long *total_host, hipStream_t st)
{
    const int tiles_x = is / RND_TILE, n = B * tiles_x * tiles_x;
    hipLaunchKernelGGL(rnd_setup_kernel, dim3((NF + 255) / 256, B), dim3(256), 0, st, verts, NV, faces, NF, colors, c_stride, K, k_stride, os, is, L, idA, idB, w.rec, w.box);
    VT_LAUNCH_CHECK();
    VT_HIP(hipMemsetAsync(w.cnt, 0, sizeof(int) * (size_t)n, st));
    hipLaunchKernelGGL(rnd_count_kernel, dim3((NF + 255) / 256, B), dim3(256), 0, st, w.box, NF, tiles_x, w.cnt);
    VT_LAUNCH_CHECK();
    hipLaunchKernelGGL(rnd_scan_kernel, dim3(1), dim3(1024), 0, st, w.cnt, n, w.off, w.cur, w.total);
    VT_LAUNCH_CHECK();
    VT_HIP(hipMemcpyAsync(total_host, w.total, sizeof(long long), hipMemcpyDeviceToHost, st));
    VT_HIP(hipStreamSynchronize(st));
    if (*total_host > w.cap) return VT_OK;                                          // caller reports it
    hipLaunchKernelGGL(rnd_fill_kernel, dim3((NF + 255) / 256, B), dim3(256), 0, st, w.box, NF, tiles_x, w.cur, w.cap, w.list);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

struct VtRenderStatic {
    int NS, size, aa, is;
    float4 *rec;                  // (NS,4) float4 records (lit colours)
    unsigned long long *keys;     // (is,is) key map, layer-local ids
};

extern "C" int vt_render_static_create(void **out, const float *verts, int NV, const int *faces, int NS, const float *face_colors, const float *K,
                                       float orig_size, const float *light, int size, int anti_aliasing, void *stream)
{
    VT_REQUIRE(out && verts && faces && face_colors && K && light && NV > 0 && NS > 0 && size > 0 && orig_size > 0.f, "vt_render_static_create: bad argument");
    const int is = size * (anti_aliasing ? 2 : 1);
    VT_REQUIRE(is % RND_TILE == 0 && is < 32768, "vt_render_static_create: size (x2 with anti-aliasing) must be a multiple of 16");
    hipStream_t st = vt_stream(stream);
    const RndLight L = rnd_light(light);
    long long entries = 4LL * NS + (long long)(is / RND_TILE) * (is / RND_TILE);
    void *ws = nullptr;
    VtRenderStatic *h = new VtRenderStatic{NS, size, anti_aliasing ? 1 : 0, is, nullptr, nullptr};
    int rc = VT_OK;
    for (int attempt = 0; attempt < 2; attempt++) {
        const long bytes = vt_render_workspace_bytes(1, NS, size, anti_aliasing, (long)entries);
        if (hipMalloc(&ws, bytes) != hipSuccess) { rc = VT_ERR_HIP; snprintf(vt_err_buf, sizeof(vt_err_buf), "vt_render_static_create: hipMalloc(%ld) failed", bytes); break; }
        const RndWs w = rnd_ws(ws, bytes, 1, NS, is);
        long long total = 0;
        rc = rnd_bin(verts, 1, NV, faces, NS, face_colors, 0, K, 0, orig_size, is, L, 0, NS, w, &total, st);
        if (rc != VT_OK) break;
        if (total > w.cap) { (void)hipFree(ws); ws = nullptr; entries = total; continue; }   // exact size known now: one retry
        if (hipMalloc(&h->rec, sizeof(float4) * 4 * (size_t)NS) != hipSuccess || hipMalloc(&h->keys, sizeof(unsigned long long) * (size_t)is * is) != hipSuccess) {
            rc = VT_ERR_HIP; snprintf(vt_err_buf, sizeof(vt_err_buf), "vt_render_static_create: hipMalloc failed"); break;
        }
        RndSeed sd{nullptr, nullptr, 0, 0};
        RndOut o{}; o.keys = h->keys;
        const int tiles_x = is / RND_TILE;
        hipLaunchKernelGGL(rnd_resolve_kernel<false>, dim3(tiles_x * tiles_x, 1), dim3(256), 0, st, w.rec, NS, w.cnt, w.off, w.list, is, tiles_x, sd, o);
        if (hipGetLastError() != hipSuccess) { rc = VT_ERR_HIP; snprintf(vt_err_buf, sizeof(vt_err_buf), "vt_render_static_create: launch failed"); break; }
        if (hipMemcpyAsync(h->rec, w.rec, sizeof(float4) * 4 * (size_t)NS, hipMemcpyDeviceToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
            rc = VT_ERR_HIP; snprintf(vt_err_buf, sizeof(vt_err_buf), "vt_render_static_create: copy failed"); break;
        }
        break;
    }
    if (ws) (void)hipFree(ws);
    if (rc == VT_OK && !h->keys) { rc = VT_ERR_HIP; snprintf(vt_err_buf, sizeof(vt_err_buf), "vt_render_static_create: binning did not converge"); }
    if (rc != VT_OK) {
        if (h->rec) (void)hipFree(h->rec);
        if (h->keys) (void)hipFree(h->keys);
        delete h;
        return rc;
    }
    *out = h;
    return VT_OK;
}
extern "C" void vt_render_static_destroy(void *layer)
{
    VtRenderStatic *h = static_cast<VtRenderStatic *>(layer);
    if (!h) return;
    (void)hipFree(h->rec); (void)hipFree(h->keys);
    delete h;
}

// face_colors (NF,3) shared by the views, or (B,NF,3) with colors_per_view (contact-coloured object faces differ from view to view: nr_utils.py:527-535)
extern "C" int vt_render_rgb_pv(const float *verts, int B, int NV, const int *faces, int NF, const float *face_colors, int colors_per_view, const float *K,
                                int k_per_view, float orig_size, const float *light, const float *background, const void *static_layer, int size,
                                int anti_aliasing, float *rgb, float *alpha, float *depth, int *face_index, void *ws, long ws_bytes, long *list_entries,
                                void *stream)
{
    VT_REQUIRE(verts && faces && face_colors && K && light && background && rgb && alpha && ws && B > 0 && NV > 0 && NF > 0 && size > 0 && orig_size > 0.f,
               "vt_render_rgb: bad argument");
    const int is = size * (anti_aliasing ? 2 : 1);
    VT_REQUIRE(is % RND_TILE == 0 && is < 32768, "vt_render_rgb: size (x2 with anti-aliasing) must be a multiple of 16");
    VT_REQUIRE((long)ws_bytes >= (long)rnd_fixed_bytes(B, NF, is), "vt_render_rgb: workspace below vt_render_workspace_bytes(B, NF, size, aa, 0)");
    const VtRenderStatic *sl = static_cast<const VtRenderStatic *>(static_layer);
    if (sl) VT_REQUIRE(sl->size == size && sl->aa == (anti_aliasing ? 1 : 0), "vt_render_rgb: static layer was built for another size / anti-aliasing");
    if (sl) VT_REQUIRE(2LL * (NF + (long long)sl->NS) < 0x7fffffffLL, "vt_render_rgb: too many faces");
    hipStream_t st = vt_stream(stream);
    const RndWs w = rnd_ws(ws, ws_bytes, B, NF, is);
    const RndLight L = rnd_light(light);
    const int NS = sl ? sl->NS : 0;
    long long total = 0;
    const int rc = rnd_bin(verts, B, NV, faces, NF, face_colors, colors_per_view ? 3L * NF : 0L, K, k_per_view ? 9 : 0, orig_size, is, L, 0, NF + NS, w, &total, st);
    if (rc != VT_OK) return rc;
    if (list_entries) *list_entries = (long)total;
    if (total > w.cap) VT_FAIL(VT_ERR_ARG, "vt_render_rgb: workspace holds %lld tile-list entries, this batch needs %lld (vt_render_workspace_bytes)", w.cap, total);
    RndSeed sd{sl ? sl->keys : nullptr, sl ? sl->rec : nullptr, NS, NF};
    RndOut o{rgb, alpha, depth, face_index, nullptr, {background[0], background[1], background[2]}, anti_aliasing ? 1 : 0};
    const int tiles_x = is / RND_TILE;
    hipLaunchKernelGGL(rnd_resolve_kernel<true>, dim3(tiles_x * tiles_x, B), dim3(256), 0, st, w.rec, NF, w.cnt, w.off, w.list, is, tiles_x, sd, o);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

extern "C" int vt_render_panel_u8(const float *rgb, int B, int size, int row0, int nrows, int col0, int ncols, unsigned char *out,
                                  const long long *view_off, long long out_row_stride, void *stream)
{
    VT_REQUIRE(rgb && out && view_off && B > 0 && size > 0 && row0 >= 0 && col0 >= 0 && nrows > 0 && ncols > 0 && row0 + nrows <= size && col0 + ncols <= size
               && out_row_stride >= 3LL * ncols, "vt_render_panel_u8: bad argument");
    hipStream_t st = vt_stream(stream);
    hipLaunchKernelGGL(rnd_panel_kernel, dim3((3 * ncols + 255) / 256, nrows, B), dim3(256), 0, st, rgb, size, row0, nrows, col0, ncols, out, view_off, out_row_stride);
    VT_LAUNCH_CHECK();
    return VT_OK;
}

extern "C" int vt_render_rgb(const float *verts, int B, int NV, const int *faces, int NF, const float *face_colors, const float *K, int k_per_view,
                             float orig_size, const float *light, const float *background, const void *static_layer, int size, int anti_aliasing,
                             float *rgb, float *alpha, float *depth, int *face_index, void *ws, long ws_bytes, long *list_entries, void *stream)
{
    return vt_render_rgb_pv(verts, B, NV, faces, NF, face_colors, 0, K, k_per_view, orig_size, light, background, static_layer, size, anti_aliasing, rgb, alpha,
                            depth, face_index, ws, ws_bytes, list_entries, stream);
}
