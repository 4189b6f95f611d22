// Host memory-error run of csrc/repack.hip's host side WITHOUT a device: every sizing function, and every argument refusal of the pack / create_device / repack /
// plan / snapshot entries -- each call below is answered or refused before any HIP call is made.  Build with the host sanitizers and run on any machine:
//   hipcc -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I vistracker_amd/csrc tools/diag/repack_host_check.hip -o /tmp/repack_host_check && /tmp/repack_host_check
#include "../../vistracker_amd/csrc/repack.hip"

thread_local char vt_err_buf[512] = {0};
// the destroy functions of conv.hip / stem.hip, which repack.hip's create_device entries call on their failure paths only (never reached here)
extern "C" void vt_conv3x3_destroy(vt_conv3x3 *h) { delete h; }
extern "C" void vt_conv1x1_destroy(vt_conv1x1 *h) { delete h; }
extern "C" void vt_stem7x7_destroy(vt_stem7x7 *h) { delete h; }

#define EXPECT(cond_) do { if (!(cond_)) { printf("FAILED line %d: %s (%s)\n", __LINE__, #cond_, vt_err_buf); fails++; } } while (0)

int main()
{
    int fails = 0;
    // sizes: every served shape against the layout's own count, and the refusals
    for (int cin = 32; cin <= 256; cin += 32) {
        EXPECT(vt_conv3x3_packed_bytes(32, cin) == (long)(cin / 32) * 9 * 4 * 1 * 2 * 64 * 16 && vt_conv3x3_packed_bytes(64, cin) == vt_conv3x3_packed_bytes(32, cin));
        EXPECT(vt_conv3x3_packed_bytes(128, cin) == 2 * vt_conv3x3_packed_bytes(64, cin));
        EXPECT(vt_conv3x3_packed_bytes(64, cin + 1) == -1 && vt_conv3x3_packed_bytes(96, cin) == -1);
    }
    EXPECT(vt_conv3x3_packed_bytes(64, 0) == -1 && vt_conv3x3_packed_bytes(0, 32) == -1 && vt_conv3x3_packed_bytes(256, 32) == -1);
    const int c1[4] = {32, 64, 128, 256};
    for (int a = 0; a < 4; a++) {
        EXPECT(vt_conv1x1_packed_bytes(64, c1[a]) == (long)(c1[a] / 32) * 4 * 2 * 64 * 16 && vt_conv1x1_packed_bytes(128, c1[a]) == 2 * vt_conv1x1_packed_bytes(64, c1[a]));
        EXPECT(vt_conv1x1_packed_bytes(256, c1[a]) == vt_conv1x1_packed_bytes(128, c1[a]));                 // per part
        EXPECT(vt_conv1x1_packed_bytes(32, c1[a]) == -1 && vt_conv1x1_packed_bytes(c1[a] == 32 ? 64 : c1[a], 96) == -1);
    }
    EXPECT(vt_conv1x1_parts(64) == 1 && vt_conv1x1_parts(128) == 1 && vt_conv1x1_parts(256) == 2 && vt_conv1x1_parts(32) == -1 && vt_conv1x1_parts(512) == -1);
    for (int cin = 1; cin <= 8; cin++)
        EXPECT(vt_stem7x7_packed_bytes(64, cin) == (long)(cin * 49 * 64 + 64) * 4 && vt_stem7x7_packed_bytes(32, cin) == (long)(cin * 49 * 32 + 32) * 4);
    EXPECT(vt_stem7x7_packed_bytes(64, 0) == -1 && vt_stem7x7_packed_bytes(64, 9) == -1 && vt_stem7x7_packed_bytes(48, 5) == -1);
    EXPECT(vt_repack_workspace_bytes() == VT_REPACK_NPART * 4);
    // the scale rule on the host: the edges of tests/test_host_repack.py
    EXPECT(cv_weight_scale(0.f) == 1.f && cv_weight_scale(INFINITY) == 1.f && cv_weight_scale(0.25f) == 32768.f && cv_weight_scale(nextafterf(0.25f, 0.f)) == 65536.f);
    EXPECT(cv_inv_scale(65536.f) == 1.f / 1048576.f);

    // argument checks: refused before anything is launched or allocated (the pointers are never dereferenced on the host; they only have to be aligned)
    alignas(16) static float buf[64];
    float *p = buf, *odd4 = buf + 1;
    float *odd1 = reinterpret_cast<float *>(reinterpret_cast<char *>(buf) + 2);
    EXPECT(vt_conv3x3_pack(nullptr, 64, 32, p, p, p, nullptr) == VT_ERR_ARG && vt_conv3x3_pack(p, 64, 32, nullptr, p, p, nullptr) == VT_ERR_ARG);
    EXPECT(vt_conv3x3_pack(p, 64, 32, p, nullptr, p, nullptr) == VT_ERR_ARG && vt_conv3x3_pack(p, 64, 32, p, p, nullptr, nullptr) == VT_ERR_ARG);
    EXPECT(vt_conv3x3_pack(p, 48, 32, p, p, p, nullptr) == VT_ERR_ARG && vt_conv3x3_pack(p, 64, 48, p, p, p, nullptr) == VT_ERR_ARG);
    EXPECT(vt_conv3x3_pack(p, 64, 32, odd4, p, p, nullptr) == VT_ERR_ARG && vt_conv3x3_pack(odd1, 64, 32, p, p, p, nullptr) == VT_ERR_ARG);     // packed: 16 bytes; weights: 4
    EXPECT(vt_conv1x1_pack(nullptr, nullptr, 64, 32, p, nullptr, p, p, nullptr) == VT_ERR_ARG && vt_conv1x1_pack(p, nullptr, 32, 32, p, nullptr, p, p, nullptr) == VT_ERR_ARG);
    EXPECT(vt_conv1x1_pack(p, nullptr, 64, 96, p, nullptr, p, p, nullptr) == VT_ERR_ARG && vt_conv1x1_pack(p, nullptr, 64, 32, odd4, nullptr, p, p, nullptr) == VT_ERR_ARG);
    EXPECT(vt_conv1x1_pack(p, p, 64, 32, p, nullptr, p, p, nullptr) == VT_ERR_ARG && vt_conv1x1_pack(p, nullptr, 64, 32, p, p, p, p, nullptr) == VT_ERR_ARG);        // a bias needs both ends
    EXPECT(vt_conv1x1_pack(p, nullptr, 64, 32, p, nullptr, nullptr, p, nullptr) == VT_ERR_ARG && vt_conv1x1_pack(p, nullptr, 64, 32, p, nullptr, p, nullptr, nullptr) == VT_ERR_ARG);
    EXPECT(vt_stem7x7_pack(nullptr, p, 64, 5, p, nullptr) == VT_ERR_ARG && vt_stem7x7_pack(p, p, 64, 5, nullptr, nullptr) == VT_ERR_ARG);
    EXPECT(vt_stem7x7_pack(p, p, 48, 5, p, nullptr) == VT_ERR_ARG && vt_stem7x7_pack(p, p, 64, 9, p, nullptr) == VT_ERR_ARG && vt_stem7x7_pack(p, odd1, 64, 5, p, nullptr) == VT_ERR_ARG);

    vt_conv3x3 *h3 = nullptr; vt_conv1x1 *h1 = nullptr; vt_stem7x7 *h7 = nullptr;
    EXPECT(vt_conv3x3_create_device(nullptr, p, 64, 32, nullptr) == VT_ERR_ARG && vt_conv3x3_create_device(&h3, nullptr, 64, 32, nullptr) == VT_ERR_ARG);
    EXPECT(vt_conv3x3_create_device(&h3, p, 48, 32, nullptr) == VT_ERR_ARG && vt_conv3x3_create_device(&h3, p, 64, 16, nullptr) == VT_ERR_ARG && h3 == nullptr);
    EXPECT(vt_conv1x1_create_device(nullptr, p, p, 64, 32, nullptr) == VT_ERR_ARG && vt_conv1x1_create_device(&h1, nullptr, p, 64, 32, nullptr) == VT_ERR_ARG);
    EXPECT(vt_conv1x1_create_device(&h1, p, p, 32, 32, nullptr) == VT_ERR_ARG && vt_conv1x1_create_device(&h1, p, odd1, 64, 32, nullptr) == VT_ERR_ARG && h1 == nullptr);
    EXPECT(vt_stem7x7_create_device(nullptr, p, p, 64, 5, nullptr) == VT_ERR_ARG && vt_stem7x7_create_device(&h7, nullptr, p, 64, 5, nullptr) == VT_ERR_ARG);
    EXPECT(vt_stem7x7_create_device(&h7, p, p, 64, 0, nullptr) == VT_ERR_ARG && vt_stem7x7_create_device(&h7, p, p, 16, 5, nullptr) == VT_ERR_ARG && h7 == nullptr);

    // repack: a handle as the host `create` functions leave it (no device scale word) is refused; so is a bias that does not match the handle
    vt_conv3x3 host3{}; host3.w = reinterpret_cast<uint4 *>(p); host3.cin = 32; host3.cout = 64; host3.nt = 1; host3.inv_scale = 1.f;
    vt_conv1x1 host1{}; host1.w[0] = reinterpret_cast<uint4 *>(p); host1.cin = 32; host1.cout = 64; host1.parts = 1; host1.pcout = 64; host1.nt = 1;
    EXPECT(vt_conv3x3_repack(nullptr, p, nullptr) == VT_ERR_ARG && vt_conv3x3_repack(&host3, nullptr, nullptr) == VT_ERR_ARG && vt_conv3x3_repack(&host3, p, nullptr) == VT_ERR_ARG);
    EXPECT(vt_conv1x1_repack(nullptr, p, nullptr, nullptr) == VT_ERR_ARG && vt_conv1x1_repack(&host1, nullptr, nullptr, nullptr) == VT_ERR_ARG);
    EXPECT(vt_conv1x1_repack(&host1, p, nullptr, nullptr) == VT_ERR_ARG);
    vt_conv1x1 dev1 = host1; dev1.scale = p; dev1.part = p + 16; dev1.dev = p;                     // device-made, created without a bias
    EXPECT(vt_conv1x1_repack(&dev1, p, p, nullptr) == VT_ERR_ARG);
    dev1.bias = p;                                                                                  // ... and with one
    EXPECT(vt_conv1x1_repack(&dev1, p, nullptr, nullptr) == VT_ERR_ARG);
    vt_stem7x7 empty7{};
    EXPECT(vt_stem7x7_repack(nullptr, p, p, nullptr) == VT_ERR_ARG && vt_stem7x7_repack(&empty7, p, p, nullptr) == VT_ERR_ARG);
    vt_stem7x7 st7{}; st7.w = p; st7.bias = p; st7.cin = 1; st7.cout = 32;
    EXPECT(vt_stem7x7_repack(&st7, nullptr, p, nullptr) == VT_ERR_ARG && vt_stem7x7_repack(&st7, odd1, p, nullptr) == VT_ERR_ARG);

    // the plan: refused before the table is allocated
    vt_conv3x3 dev3 = host3; dev3.scale = p; dev3.part = p + 16; dev3.dev = p;
    vt_repack_plan *plan = nullptr;
    int kinds[3] = {VT_REPACK_CONV3X3, VT_REPACK_CONV1X1, VT_REPACK_STEM7X7};
    void *hs[3] = {&dev3, &dev1, &st7};
    const float *wts[3] = {p, p, p};
    const float *bss[3] = {nullptr, p, p};
    EXPECT(vt_repack_plan_create(nullptr, 3, kinds, hs, wts, bss) == VT_ERR_ARG && vt_repack_plan_create(&plan, 0, kinds, hs, wts, bss) == VT_ERR_ARG);
    EXPECT(vt_repack_plan_create(&plan, 70000, kinds, hs, wts, bss) == VT_ERR_ARG && vt_repack_plan_create(&plan, 3, nullptr, hs, wts, bss) == VT_ERR_ARG);
    EXPECT(vt_repack_plan_create(&plan, 3, kinds, nullptr, wts, bss) == VT_ERR_ARG && vt_repack_plan_create(&plan, 3, kinds, hs, nullptr, bss) == VT_ERR_ARG);
    EXPECT(vt_repack_plan_create(&plan, 3, kinds, hs, wts, nullptr) == VT_ERR_ARG);
    kinds[2] = 3;
    EXPECT(vt_repack_plan_create(&plan, 3, kinds, hs, wts, bss) == VT_ERR_ARG);               // unknown kind
    kinds[2] = VT_REPACK_STEM7X7; hs[0] = nullptr;
    EXPECT(vt_repack_plan_create(&plan, 3, kinds, hs, wts, bss) == VT_ERR_ARG);               // null handle
    hs[0] = &host3;
    EXPECT(vt_repack_plan_create(&plan, 3, kinds, hs, wts, bss) == VT_ERR_ARG);               // host-packed 3 x 3
    hs[0] = &dev3; bss[0] = p;
    EXPECT(vt_repack_plan_create(&plan, 3, kinds, hs, wts, bss) == VT_ERR_ARG);               // a 3 x 3 has no bias
    bss[0] = nullptr; bss[1] = nullptr;
    EXPECT(vt_repack_plan_create(&plan, 3, kinds, hs, wts, bss) == VT_ERR_ARG);               // the 1 x 1 was created with one
    bss[1] = p; wts[2] = nullptr;
    EXPECT(vt_repack_plan_create(&plan, 3, kinds, hs, wts, bss) == VT_ERR_ARG);               // null weights
    wts[2] = p; hs[2] = &empty7;
    EXPECT(vt_repack_plan_create(&plan, 3, kinds, hs, wts, bss) == VT_ERR_ARG && plan == nullptr);
    EXPECT(vt_repack_plan_run(nullptr, nullptr) == VT_ERR_ARG && vt_repack_plan_launches(nullptr) == -1);
    vt_repack_plan_destroy(nullptr);
    EXPECT(vt_repack_handle_snapshot(VT_REPACK_CONV3X3, nullptr, p, p, nullptr) == VT_ERR_ARG && vt_repack_handle_snapshot(VT_REPACK_CONV3X3, &dev3, nullptr, p, nullptr) == VT_ERR_ARG);
    EXPECT(vt_repack_handle_snapshot(5, &dev3, p, p, nullptr) == VT_ERR_ARG);
    printf(fails ? "repack host check: %d FAILED\n" : "repack host check: all refusals and sizes as expected (%d failures)\n", fails);
    return fails ? 1 : 0;
}
