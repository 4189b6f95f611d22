// repack.hip -- the packed forward weights of the encoder's convolutions (conv.hip, stem.hip) built ON THE DEVICE from fp32 weights in device memory: what an
// optimiser step needs so that the next forward reads the new weights without the device -> host -> device round trip of vt_conv3x3_create / vt_conv1x1_create /
// vt_stem7x7_create (a synchronise, a copy down, the packing loops on the CPU, hipMalloc, a copy up and another synchronise, per convolution and step).
// The packed bytes are those of the host functions bit for bit:
//   * split-f16 kinds (3 x 3, 1 x 1): x = w s_W, hi = (f16)x, lo = (f16)(x - (f32)hi), round to nearest even, f16 denormals kept (the low halves routinely are),
//     in the fragment order documented at vt_conv3x3_create; rows beyond Cout = 32 are zero; s_W = cv_weight_scale(max |w|) (conv_handles.h);
//   * the stem: the (Cout, Cin, 7, 7) -> [Cin][7][7][Cout] transpose and the bias row (zeros without one), no scale.
// s_W exists only on the device after a device-side optimiser step, so 1 / (16 s_W) goes to a device word that the forward kernel reads (conv3x3_kernel's last
// argument) instead of the by-value scalar of a host-packed handle.
// Two launches whatever the number of convolutions (grid.y = the convolution):
//   1. max pass: VT_REPACK_NPART workgroups per convolution, each the maximum of |w| over a grid-strided share -> part[workgroup].  No atomics: a maximum does not
//      depend on the order it is taken in, and fmaxf drops a NaN operand exactly as the host loop does;
//   2. pack pass: every workgroup reduces the VT_REPACK_NPART partials of its convolution again (32 uniform loads), derives s_W and packs a grid-strided share of
//      the fragments; workgroup 0 writes the scale word (and nobody reads it in this launch).
// Ordering on the stream is the whole synchronisation: a forward queued earlier still reads the old packing, one queued later the new.
#include "conv_handles.h"

typedef _Float16 rp_h8 __attribute__((ext_vector_type(8)));
#define RP_NPB 64               /* workgroups per convolution in the pack pass */
#define RP_SCALE_FLOATS 16      /* the scale word's slot in a handle's allocation (64 bytes: the partials behind it stay 64-byte aligned) */

struct RepackDesc {
    const float *w, *bias;      // fp32 sources: (Cout, Cin, k, k) and (Cout) or NULL
    void *packed;               // split kinds: uint4 fragments, the parts of a 256-output 1 x 1 one after the other; stem: [Cin][7][7][Cout] floats + the bias row
    float *bias_out;            // 1 x 1: the handle's copy of the bias, or NULL
    float *scale;               // split kinds: the device word 1 / (16 s_W)
    float *part;                // split kinds: VT_REPACK_NPART partial maxima
    int kind, cout, cin, nt, parts, pcout;
    unsigned nelem;             // weight elements
    unsigned nitem;             // split kinds: (part, step, wave, nt, lane) fragments = pairs of uint4; stem: nelem
    unsigned n16;               // split kinds: uint4 per part
};

__device__ __forceinline__ void repack_max_dev(const RepackDesc &d)
{
    if (d.kind == VT_REPACK_STEM7X7) return;            // uniform per workgroup
    __shared__ float red[4];
    float m = 0.f;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < d.nelem; i += VT_REPACK_NPART * 256u) m = fmaxf(m, fabsf(d.w[i]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) d.part[blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__device__ __forceinline__ void repack_pack_dev(const RepackDesc &d)
{
    const unsigned gtid = blockIdx.x * 256u + threadIdx.x, gsz = RP_NPB * 256u;
    if (d.kind == VT_REPACK_STEM7X7) {
        float *out = static_cast<float *>(d.packed);
        const unsigned co_n = (unsigned)d.cout, cin = (unsigned)d.cin;
        for (unsigned i = gtid; i < d.nelem; i += gsz) {
            const unsigned co = i % co_n, r = i / co_n, t = r % 49u, ci = r / 49u;
            out[i] = d.w[((size_t)co * cin + ci) * 49u + t];
        }
        for (unsigned i = gtid; i < co_n; i += gsz) out[d.nelem + i] = d.bias ? d.bias[i] : 0.f;
        return;
    }
    float m = 0.f;
    for (int k = 0; k < VT_REPACK_NPART; k++) m = fmaxf(m, d.part[k]);
    const float sw = cv_weight_scale(m);
    if (gtid == 0) *d.scale = cv_inv_scale(sw);
    const bool k3 = d.kind == VT_REPACK_CONV3X3;
    const unsigned nt = (unsigned)d.nt, ntap = k3 ? 9u : 1u, nstep = (unsigned)(d.cin >> 5) * ntap, per_part = nstep * 4u * nt * 64u;
    uint4 *pk = static_cast<uint4 *>(d.packed);
    for (unsigned i = gtid; i < d.nitem; i += gsz) {
        const unsigned pt = i / per_part, r0 = i - pt * per_part;
        const unsigned lane = r0 & 63u, n = (r0 >> 6) % nt, r1 = (r0 >> 6) / nt, wave = r1 & 3u, step = r1 >> 2, t = step % ntap, c = step / ntap;
        const unsigned co = pt * (unsigned)d.pcout + (wave * nt + n) * 16u + (lane & 15u), ci = 32u * c + 8u * (lane >> 4);
        rp_h8 hi, lo;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const float x = co < (unsigned)d.cout ? d.w[((size_t)co * d.cin + ci + k) * ntap + t] * sw : 0.f;
            const _Float16 h = (_Float16)x;
            hi[k] = h; lo[k] = (_Float16)(x - (float)h);
        }
        const size_t base = (size_t)pt * d.n16 + (size_t)((step * 4u + wave) * nt + n) * 128u;
        pk[base + lane] = __builtin_bit_cast(uint4, hi);
        pk[base + 64 + lane] = __builtin_bit_cast(uint4, lo);
    }
    if (d.bias_out && d.bias)
        for (unsigned i = gtid; i < (unsigned)d.cout; i += gsz) d.bias_out[i] = d.bias[i];
}

__global__ __launch_bounds__(256) void repack_max_plan_kernel(const RepackDesc *__restrict__ table) { repack_max_dev(table[blockIdx.y]); }
__global__ __launch_bounds__(256) void repack_pack_plan_kernel(const RepackDesc *__restrict__ table) { repack_pack_dev(table[blockIdx.y]); }
__global__ __launch_bounds__(256) void repack_max_one_kernel(const RepackDesc d) { repack_max_dev(d); }
__global__ __launch_bounds__(256) void repack_pack_one_kernel(const RepackDesc d) { repack_pack_dev(d); }

namespace rpk {
static RepackDesc desc3(const float *w, int cout, int cin, void *packed, float *scale, float *part)
{
    RepackDesc d{};
    d.w = w; d.packed = packed; d.scale = scale; d.part = part;
    d.kind = VT_REPACK_CONV3X3; d.cout = cout; d.cin = cin; d.nt = cout == 128 ? 2 : 1; d.parts = 1; d.pcout = 64 * d.nt;
    d.nelem = (unsigned)cout * cin * 9; d.n16 = (unsigned)cv3_n16(cout, cin); d.nitem = d.n16 / 2;
    return d;
}
static RepackDesc desc1(const float *w, const float *bias, int cout, int cin, void *packed, float *bias_out, float *scale, float *part)
{
    RepackDesc d{};
    d.w = w; d.bias = bias; d.packed = packed; d.bias_out = bias_out; d.scale = scale; d.part = part;
    d.kind = VT_REPACK_CONV1X1; d.cout = cout; d.cin = cin; d.parts = cout == 256 ? 2 : 1; d.pcout = cout / d.parts; d.nt = d.pcout == 128 ? 2 : 1;
    d.nelem = (unsigned)cout * cin; d.n16 = (unsigned)cv1_n16(cout, cin); d.nitem = d.parts * (d.n16 / 2);
    return d;
}
static RepackDesc desc7(const float *w, const float *bias, int cout, int cin, void *packed)
{
    RepackDesc d{};
    d.w = w; d.bias = bias; d.packed = packed;
    d.kind = VT_REPACK_STEM7X7; d.cout = cout; d.cin = cin; d.nt = 1; d.parts = 1; d.pcout = cout;
    d.nelem = (unsigned)cout * cin * 49; d.nitem = d.nelem;
    return d;
}
static int run_one(const RepackDesc &d, void *stream)
{
    hipLaunchKernelGGL(repack_max_one_kernel, dim3(VT_REPACK_NPART), dim3(256), 0, vt_stream(stream), d);
    hipLaunchKernelGGL(repack_pack_one_kernel, dim3(RP_NPB), dim3(256), 0, vt_stream(stream), d);
    VT_LAUNCH_CHECK();
    return VT_OK;
}
static inline bool al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static inline bool al4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
}   // namespace rpk

// ---- sizes ------------------------------------------------------------------------------------------------------------------------------------------------
extern "C" long vt_conv3x3_packed_bytes(int cout, int cin) { return cv3_shape_ok(cout, cin) ? (long)(cv3_n16(cout, cin) * 16) : -1; }
extern "C" long vt_conv1x1_packed_bytes(int cout, int cin) { return cv1_shape_ok(cout, cin) ? (long)(cv1_n16(cout, cin) * 16) : -1; }
extern "C" int vt_conv1x1_parts(int cout) { return cout == 256 ? 2 : (cout == 64 || cout == 128) ? 1 : -1; }
extern "C" long vt_stem7x7_packed_bytes(int cout, int cin) { return stem_shape_ok(cout, cin) ? (long)((size_t)cin * 49 * cout + cout) * 4 : -1; }
extern "C" long vt_repack_workspace_bytes(void) { return (long)VT_REPACK_NPART * sizeof(float); }

// ---- raw packing into caller-supplied device buffers ------------------------------------------------------------------------------------------------------
extern "C" int vt_conv3x3_pack(const float *w_dev, int cout, int cin, void *packed_dev, float *scale_dev, void *ws_dev, void *stream)
{
    VT_REQUIRE(cv3_shape_ok(cout, cin), "vt_conv3x3_pack: needs Cout in {32, 64, 128} and Cin a multiple of 32");
    VT_REQUIRE(w_dev && packed_dev && scale_dev && ws_dev && rpk::al4(w_dev) && rpk::al16(packed_dev) && rpk::al4(scale_dev) && rpk::al4(ws_dev),
               "vt_conv3x3_pack: null or misaligned buffer (packed: 16 bytes)");
    return rpk::run_one(rpk::desc3(w_dev, cout, cin, packed_dev, scale_dev, static_cast<float *>(ws_dev)), stream);
}
extern "C" int vt_conv1x1_pack(const float *w_dev, const float *bias_dev, int cout, int cin, void *packed_dev, float *bias_out_dev, float *scale_dev, void *ws_dev,
                               void *stream)
{
    VT_REQUIRE(cv1_shape_ok(cout, cin), "vt_conv1x1_pack: needs Cout in {64, 128, 256} and Cin in {32, 64, 128, 256}");
    VT_REQUIRE(w_dev && packed_dev && scale_dev && ws_dev && rpk::al4(w_dev) && rpk::al16(packed_dev) && rpk::al4(scale_dev) && rpk::al4(ws_dev),
               "vt_conv1x1_pack: null or misaligned buffer (packed: 16 bytes)");
    VT_REQUIRE((bias_dev != nullptr) == (bias_out_dev != nullptr) && rpk::al4(bias_dev) && rpk::al4(bias_out_dev), "vt_conv1x1_pack: a bias needs both its source and its destination");
    return rpk::run_one(rpk::desc1(w_dev, bias_dev, cout, cin, packed_dev, bias_out_dev, scale_dev, static_cast<float *>(ws_dev)), stream);
}
extern "C" int vt_stem7x7_pack(const float *w_dev, const float *bias_dev, int cout, int cin, void *packed_dev, void *stream)
{
    VT_REQUIRE(stem_shape_ok(cout, cin), "vt_stem7x7_pack: needs Cout in {32, 64} and Cin in 1..8");
    VT_REQUIRE(w_dev && packed_dev && rpk::al4(w_dev) && rpk::al4(bias_dev) && rpk::al16(packed_dev), "vt_stem7x7_pack: null or misaligned buffer (packed: 16 bytes)");
    return rpk::run_one(rpk::desc7(w_dev, bias_dev, cout, cin, packed_dev), stream);
}

// ---- handles packed on the device -------------------------------------------------------------------------------------------------------------------------
// One hipMalloc per handle (what a handle owns has to come from somewhere), no host staging and no synchronisation: the packing is queued on `stream`.
namespace rpk {
static RepackDesc of3(const vt_conv3x3 *h, const float *w) { return desc3(w, h->cout, h->cin, h->w, h->scale, h->part); }
static RepackDesc of1(const vt_conv1x1 *h, const float *w, const float *b) { return desc1(w, b, h->cout, h->cin, h->w[0], b ? h->bias : nullptr, h->scale, h->part); }
static RepackDesc of7(const vt_stem7x7 *h, const float *w, const float *b) { return desc7(w, b, h->cout, h->cin, h->w); }
}   // namespace rpk

extern "C" int vt_conv3x3_repack(vt_conv3x3 *h, const float *w_dev, void *stream)
{
    VT_REQUIRE(h && w_dev && rpk::al4(w_dev), "vt_conv3x3_repack: null handle or weights");
    VT_REQUIRE(h->scale && h->part && h->dev, "vt_conv3x3_repack: the handle was packed on the host (vt_conv3x3_create): it has no device scale word");
    return rpk::run_one(rpk::of3(h, w_dev), stream);
}
extern "C" int vt_conv3x3_create_device(vt_conv3x3 **out, const float *w_dev, int cout, int cin, void *stream)
{
    VT_REQUIRE(out && w_dev && rpk::al4(w_dev) && cv3_shape_ok(cout, cin), "vt_conv3x3_create_device: needs Cout in {32, 64, 128} and Cin a multiple of 32");
    const size_t n16 = cv3_n16(cout, cin);
    void *dev = nullptr;
    VT_HIP(hipMalloc(&dev, n16 * 16 + (RP_SCALE_FLOATS + VT_REPACK_NPART) * sizeof(float)));
    vt_conv3x3 *h = new vt_conv3x3();
    h->dev = dev; h->w = static_cast<uint4 *>(dev); h->scale = reinterpret_cast<float *>(h->w + n16); h->part = h->scale + RP_SCALE_FLOATS;
    h->cin = cin; h->cout = cout; h->nt = cout == 128 ? 2 : 1; h->inv_scale = 0.f;
    const int rc = vt_conv3x3_repack(h, w_dev, stream);
    if (rc != VT_OK) { vt_conv3x3_destroy(h); return rc; }
    *out = h;
    return VT_OK;
}

extern "C" int vt_conv1x1_repack(vt_conv1x1 *h, const float *w_dev, const float *bias_dev, void *stream)
{
    VT_REQUIRE(h && w_dev && rpk::al4(w_dev) && rpk::al4(bias_dev), "vt_conv1x1_repack: null handle or weights");
    VT_REQUIRE(h->scale && h->part && h->dev, "vt_conv1x1_repack: the handle was packed on the host (vt_conv1x1_create): it has no device scale word");
    VT_REQUIRE((bias_dev != nullptr) == (h->bias != nullptr), "vt_conv1x1_repack: the handle was created %s a bias", h->bias ? "with" : "without");
    return rpk::run_one(rpk::of1(h, w_dev, bias_dev), stream);
}
extern "C" int vt_conv1x1_create_device(vt_conv1x1 **out, const float *w_dev, const float *bias_dev, int cout, int cin, void *stream)
{
    VT_REQUIRE(out && w_dev && rpk::al4(w_dev) && rpk::al4(bias_dev) && cv1_shape_ok(cout, cin), "vt_conv1x1_create_device: needs Cout in {64, 128, 256} and Cin in {32, 64, 128, 256}");
    const size_t n16 = cv1_n16(cout, cin);
    const int parts = cout == 256 ? 2 : 1;
    void *dev = nullptr;
    VT_HIP(hipMalloc(&dev, parts * n16 * 16 + ((bias_dev ? (size_t)cout : 0) + RP_SCALE_FLOATS + VT_REPACK_NPART) * sizeof(float)));
    vt_conv1x1 *h = new vt_conv1x1();
    h->dev = dev; h->w[0] = static_cast<uint4 *>(dev); h->w[1] = parts == 2 ? h->w[0] + n16 : nullptr;
    float *tail = reinterpret_cast<float *>(h->w[0] + parts * n16);
    h->bias = bias_dev ? tail : nullptr;
    h->scale = tail + (bias_dev ? cout : 0); h->part = h->scale + RP_SCALE_FLOATS;
    h->cin = cin; h->cout = cout; h->parts = parts; h->pcout = cout / parts; h->nt = h->pcout == 128 ? 2 : 1; h->inv_scale = 0.f;
    const int rc = vt_conv1x1_repack(h, w_dev, bias_dev, stream);
    if (rc != VT_OK) { vt_conv1x1_destroy(h); return rc; }
    *out = h;
    return VT_OK;
}

// the stem's packed form has no scale: any handle (vt_stem7x7_create's too) can be repacked; a NULL bias writes the zero row
extern "C" int vt_stem7x7_repack(vt_stem7x7 *h, const float *w_dev, const float *bias_dev, void *stream)
{
    VT_REQUIRE(h && h->w && w_dev && rpk::al4(w_dev) && rpk::al4(bias_dev), "vt_stem7x7_repack: null handle or weights");
    return rpk::run_one(rpk::of7(h, w_dev, bias_dev), stream);
}
extern "C" int vt_stem7x7_create_device(vt_stem7x7 **out, const float *w_dev, const float *bias_dev, int cout, int cin, void *stream)
{
    VT_REQUIRE(out && w_dev && rpk::al4(w_dev) && rpk::al4(bias_dev) && stem_shape_ok(cout, cin), "vt_stem7x7_create_device: needs Cout in {32, 64} and Cin in 1..8");
    const size_t n = (size_t)cin * 49 * cout;
    float *dev = nullptr;
    VT_HIP(hipMalloc(reinterpret_cast<void **>(&dev), (n + cout) * sizeof(float)));
    vt_stem7x7 *h = new vt_stem7x7();
    h->w = dev; h->bias = dev + n; h->cin = cin; h->cout = cout;
    const int rc = vt_stem7x7_repack(h, w_dev, bias_dev, stream);
    if (rc != VT_OK) { vt_stem7x7_destroy(h); return rc; }
    *out = h;
    return VT_OK;
}

// ---- a plan: n convolutions in two launches ---------------------------------------------------------------------------------------------------------------
struct vt_repack_plan {
    RepackDesc *table;      // device
    int n;
};
extern "C" int vt_repack_plan_create(vt_repack_plan **out, int n, const int *kinds, void *const *handles, const float *const *weights, const float *const *biases)
{
    VT_REQUIRE(out && n > 0 && n <= 65535 && kinds && handles && weights && biases, "vt_repack_plan_create: needs 1..65535 convolutions and the four tables");
    RepackDesc *host = new RepackDesc[n];
#define RP_REFUSE(cond_, ...) do { if (!(cond_)) { delete[] host; VT_FAIL(VT_ERR_ARG, __VA_ARGS__); } } while (0)
    for (int i = 0; i < n; i++) {
        RP_REFUSE(handles[i] && weights[i] && rpk::al4(weights[i]) && rpk::al4(biases[i]), "vt_repack_plan_create: entry %d has a null handle or null / misaligned weights", i);
        if (kinds[i] == VT_REPACK_CONV3X3) {
            const vt_conv3x3 *h = static_cast<const vt_conv3x3 *>(handles[i]);
            RP_REFUSE(h->scale && h->part && h->dev && !biases[i], "vt_repack_plan_create: entry %d needs a 3 x 3 handle of vt_conv3x3_create_device and no bias", i);
            host[i] = rpk::of3(h, weights[i]);
        } else if (kinds[i] == VT_REPACK_CONV1X1) {
            const vt_conv1x1 *h = static_cast<const vt_conv1x1 *>(handles[i]);
            RP_REFUSE(h->scale && h->part && h->dev, "vt_repack_plan_create: entry %d needs a 1 x 1 handle of vt_conv1x1_create_device", i);
            RP_REFUSE((biases[i] != nullptr) == (h->bias != nullptr), "vt_repack_plan_create: entry %d was created %s a bias", i, h->bias ? "with" : "without");
            host[i] = rpk::of1(h, weights[i], biases[i]);
        } else if (kinds[i] == VT_REPACK_STEM7X7) {
            const vt_stem7x7 *h = static_cast<const vt_stem7x7 *>(handles[i]);
            RP_REFUSE(h->w, "vt_repack_plan_create: entry %d is an empty stem handle", i);
            host[i] = rpk::of7(h, weights[i], biases[i]);
        } else RP_REFUSE(false, "vt_repack_plan_create: entry %d has kind %d (VT_REPACK_CONV3X3, VT_REPACK_CONV1X1 or VT_REPACK_STEM7X7)", i, kinds[i]);
    }
#undef RP_REFUSE
    RepackDesc *table = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&table), sizeof(RepackDesc) * n);
    if (e == hipSuccess) e = hipMemcpy(table, host, sizeof(RepackDesc) * n, hipMemcpyHostToDevice);        // built once: the one blocking copy of a plan's life
    delete[] host;
    if (e != hipSuccess) { if (table) (void)hipFree(table); VT_HIP(e); }
    vt_repack_plan *p = new vt_repack_plan();
    p->table = table; p->n = n;
    *out = p;
    return VT_OK;
}
extern "C" int vt_repack_plan_launches(const vt_repack_plan *plan) { return plan ? 2 : -1; }
extern "C" int vt_repack_plan_run(const vt_repack_plan *plan, void *stream)
{
    VT_REQUIRE(plan && plan->table && plan->n > 0, "vt_repack_plan_run: null plan");
    hipLaunchKernelGGL(repack_max_plan_kernel, dim3(VT_REPACK_NPART, plan->n), dim3(256), 0, vt_stream(stream), plan->table);
    hipLaunchKernelGGL(repack_pack_plan_kernel, dim3(RP_NPB, plan->n), dim3(256), 0, vt_stream(stream), plan->table);
    VT_LAUNCH_CHECK();
    return VT_OK;
}
extern "C" void vt_repack_plan_destroy(vt_repack_plan *plan) { if (!plan) return; (void)hipFree(plan->table); delete plan; }

// A handle's packed bytes (the parts of a two-part 1 x 1 one after the other; the stem: weights + bias row) and its scale word copied into caller-supplied DEVICE
// buffers on `stream`: what the tests compare, for handles of either origin.  scale_out_dev may be NULL (and is ignored for the stem).
extern "C" int vt_repack_handle_snapshot(int kind, const void *handle, void *packed_out_dev, float *scale_out_dev, void *stream)
{
    VT_REQUIRE(handle && packed_out_dev && (kind == VT_REPACK_CONV3X3 || kind == VT_REPACK_CONV1X1 || kind == VT_REPACK_STEM7X7), "vt_repack_handle_snapshot: bad argument");
    hipStream_t st = vt_stream(stream);
    const float *scale = nullptr; float inv = 0.f;
    if (kind == VT_REPACK_CONV3X3) {
        const vt_conv3x3 *h = static_cast<const vt_conv3x3 *>(handle);
        VT_HIP(hipMemcpyAsync(packed_out_dev, h->w, cv3_n16(h->cout, h->cin) * 16, hipMemcpyDeviceToDevice, st));
        scale = h->scale; inv = h->inv_scale;
    } else if (kind == VT_REPACK_CONV1X1) {
        const vt_conv1x1 *h = static_cast<const vt_conv1x1 *>(handle);
        const size_t nb = cv1_n16(h->cout, h->cin) * 16;
        for (int pt = 0; pt < h->parts; pt++) VT_HIP(hipMemcpyAsync(static_cast<char *>(packed_out_dev) + pt * nb, h->w[pt], nb, hipMemcpyDeviceToDevice, st));
        scale = h->scale; inv = h->inv_scale;
    } else {
        const vt_stem7x7 *h = static_cast<const vt_stem7x7 *>(handle);
        VT_HIP(hipMemcpyAsync(packed_out_dev, h->w, ((size_t)h->cin * 49 * h->cout + h->cout) * sizeof(float), hipMemcpyDeviceToDevice, st));
        return VT_OK;
    }
    if (scale_out_dev) {
        if (scale) VT_HIP(hipMemcpyAsync(scale_out_dev, scale, sizeof(float), hipMemcpyDeviceToDevice, st));
        else { unsigned bits; memcpy(&bits, &inv, 4); VT_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(scale_out_dev), (int)bits, 1, st)); }
    }
    return VT_OK;
}
