// conv_handles.h -- the packed forward handles of the encoder's convolutions (conv.hip: 3 x 3 and 1 x 1 on the split-f16 kernel; stem.hip: the 7 x 7 stem) and
// the rule for the weight scale, shared by the host `create` functions and the device-side packing of repack.hip.
#pragma once
#include "common.h"

#define CV_ACT_SCALE 16.0f
#define VT_REPACK_NPART 32          /* per-convolution partial maxima of the max pass (one per workgroup) */

// A handle packed on the device (vt_*_create_device) is ONE allocation `dev`: the packed weights, then the scale word and the partial maxima of its own repack.
// `scale` is the device word holding 1 / (CV_ACT_SCALE * s_W) that the forward kernel reads; NULL in a handle of the host `create`, which passes inv_scale by value.
struct vt_conv3x3 {
    uint4 *w;           // [Cin / 32][9][4 waves][NT][hi|lo][64 lanes]
    int cin, cout, nt;
    float inv_scale;    // 1 / (CV_ACT_SCALE * s_W): host-created handles only
    float *scale;       // the same value in device memory (device-created handles), else NULL
    float *part;        // VT_REPACK_NPART partial maxima (device-created handles)
    void *dev;          // the allocation of a device-created handle, else NULL (then `w` is its own)
};
struct vt_conv1x1 {
    uint4 *w[2];        // per part of <= 128 output channels: [Cin / 32][4 waves][NT][hi|lo][64 lanes]
    float *bias;        // (Cout) or NULL
    int cin, cout, parts, pcout, nt;
    float inv_scale;
    float *scale, *part;
    void *dev;          // device-created: w[0], w[1], bias, scale and part all live in it
};
struct vt_stem7x7 {
    float *w;       // [Cin][7][7][Cout]
    float *bias;    // [Cout] (zeros without one)
    int cin, cout;
};

// s_W of a convolution from the maximum of |w| over its finite-or-infinite entries (NaN never enters a maximum taken with fmaxf): the power of two that brings
// the maximum into [2^13, 2^14); 1 for an all-zero or non-finite maximum.
__host__ __device__ static inline float cv_weight_scale(float m)
{
    float sw = 1.0f;
    if (m > 0.f && m <= 3.402823466e+38f) { int e; frexpf(m, &e); sw = ldexpf(1.0f, 14 - e); }
    return sw;
}
__host__ __device__ static inline float cv_inv_scale(float sw) { return 1.0f / (CV_ACT_SCALE * sw); }

static inline bool cv3_shape_ok(int cout, int cin) { return (cout == 32 || cout == 64 || cout == 128) && cin >= 32 && cin % 32 == 0; }
static inline bool cv1_shape_ok(int cout, int cin) { return (cout == 64 || cout == 128 || cout == 256) && (cin == 32 || cin == 64 || cin == 128 || cin == 256); }
static inline bool stem_shape_ok(int cout, int cin) { return (cout == 64 || cout == 32) && cin >= 1 && cin <= 8; }
// uint4 count of a packed 3 x 3 weight / of ONE part of a packed 1 x 1 weight
static inline size_t cv3_n16(int cout, int cin) { return (size_t)(cin / 32) * 9 * 4 * (cout == 128 ? 2 : 1) * 2 * 64; }
static inline size_t cv1_n16(int cout, int cin) { return (size_t)(cin / 32) * 4 * ((cout == 256 ? 128 : cout) == 128 ? 2 : 1) * 2 * 64; }
