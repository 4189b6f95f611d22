// Host memory-error run of csrc/convtrain.hip's host side (argument checks, workspace sizing, launch geometry helpers) WITHOUT a device: every call below is
// refused by an argument check or answered by a sizing function before any HIP call is made.  Build with the host sanitizers and run on any machine:
//   hipcc -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I vistracker_amd/csrc tools/diag/convtrain_host_check.hip -o /tmp/convtrain_host_check && /tmp/convtrain_host_check
#include "../../vistracker_amd/csrc/convtrain.hip"

thread_local char vt_err_buf[512] = {0};

#define EXPECT(cond_) do { if (!(cond_)) { printf("FAILED line %d: %s (%s)\n", __LINE__, #cond_, vt_err_buf); fails++; } } while (0)

int main()
{
    int fails = 0;
    // sizing: every served layer and block shape, and the refusals
    const int couts3[3] = {32, 64, 128}, couts1[3] = {64, 128, 256};
    for (int cin = 32; cin <= 256; cin += 32)
        for (int k = 0; k < 3; k++) {
            EXPECT(vt_conv_dgrad_workspace_bytes(couts3[k], cin, 9) == (long)((size_t)couts3[k] * cin * 9 * 4 + 255) / 256 * 256);
            EXPECT(vt_conv_dgrad_workspace_bytes(couts1[k], cin, 1) >= (long)couts1[k] * cin * 4);
            for (int B = 1; B <= 65535; B = B * 7 + 1) {
                const long w = vt_conv_wgrad_workspace_bytes(B, 16, 32, couts3[k], cin, 9);
                EXPECT(w >= (long)B * couts3[k] * cin * 9 * 4 && w % 256 == 0);
                EXPECT(convt::wgrad_splits(B, 4) >= 1 && convt::wgrad_splits(B, 4) <= 4);
            }
        }
    EXPECT(vt_conv_dgrad_workspace_bytes(48, 64, 9) == -1 && vt_conv_dgrad_workspace_bytes(64, 48, 9) == -1 && vt_conv_dgrad_workspace_bytes(64, 64, 4) == -1);
    EXPECT(vt_conv_dgrad_workspace_bytes(64, 288, 9) == -1 && vt_conv_dgrad_workspace_bytes(256, 64, 9) == -1 && vt_conv_dgrad_workspace_bytes(32, 64, 1) == -1);
    EXPECT(vt_conv_wgrad_workspace_bytes(0, 16, 32, 64, 64, 9) == -1 && vt_conv_wgrad_workspace_bytes(1, 12, 32, 64, 64, 9) == -1 && vt_conv_wgrad_workspace_bytes(1, 16, 24, 64, 64, 9) == -1);
    EXPECT(vt_conv_wgrad_workspace_bytes(65536, 16, 32, 64, 64, 9) == -1);
    EXPECT(vt_gn_relu_backward_workspace_bytes(2, 512, 32, 32) > 0 && vt_gn_relu_backward_workspace_bytes(2, 512, 1024, 32) > 0);
    EXPECT(vt_gn_relu_backward_workspace_bytes(2, 512, 30, 32) == -1 && vt_gn_relu_backward_workspace_bytes(2, 0, 32, 32) == -1 && vt_gn_relu_backward_workspace_bytes(2, 512, 2048, 32) == -1);
    for (int hw = 1; hw <= 1 << 20; hw *= 3) EXPECT(convt::gnb_blocks(hw) >= 1 && convt::gnb_blocks(hw) <= CT_GNB_MAXBLK);
    EXPECT(vt_conv_block_backward_workspace(2, 16, 32, 64, 64, 32, 32) > 0 && vt_conv_block_backward_workspace(16, 128, 128, 256, 128, 64, 64) > 0);
    EXPECT(vt_conv_block_backward_workspace(2, 16, 32, 128, 64, 32, 32) > 0);
    EXPECT(vt_conv_block_backward_workspace(2, 17, 32, 64, 64, 32, 32) == -1 && vt_conv_block_backward_workspace(2, 16, 32, 48, 64, 32, 32) == -1);
    EXPECT(vt_conv_block_backward_workspace(2, 16, 32, 64, 64, 48, 32) == -1);

    // argument checks: refused before anything is launched (the pointers are never dereferenced on the host; they only have to be aligned)
    alignas(16) static float buf[64];
    float *p = buf, *odd = buf + 1;
    EXPECT(vt_conv3x3_dgrad(nullptr, 64, 64, p, 64, 0, 1, 8, 16, p, 64, 0, p, nullptr) == VT_ERR_ARG);
    EXPECT(vt_conv3x3_dgrad(p, 48, 64, p, 64, 0, 1, 8, 16, p, 64, 0, p, nullptr) == VT_ERR_ARG);
    EXPECT(vt_conv3x3_dgrad(p, 64, 64, p, 64, 0, 1, 9, 16, p, 64, 0, p, nullptr) == VT_ERR_ARG);
    EXPECT(vt_conv3x3_dgrad(p, 64, 64, p, 32, 0, 1, 8, 16, p, 64, 0, p, nullptr) == VT_ERR_ARG);          // channel stride narrower than the slice
    EXPECT(vt_conv3x3_dgrad(p, 64, 64, odd, 64, 0, 1, 8, 16, p, 64, 0, p, nullptr) == VT_ERR_ARG);        // misaligned pointer
    EXPECT(vt_conv3x3_dgrad(p, 64, 64, p, 66, 2, 1, 8, 16, p, 64, 0, p, nullptr) == VT_ERR_ARG);          // offset not a multiple of 4
    EXPECT(vt_conv1x1_dgrad(p, 32, 64, p, 32, 0, 1, 8, 16, p, 64, 0, p, nullptr) == VT_ERR_ARG);
    EXPECT(vt_conv1x1_dgrad(p, 64, 64, p, 64, 0, 1, 8, 16, p, 64, 0, nullptr, nullptr) == VT_ERR_ARG);
    EXPECT(vt_conv3x3_wgrad(p, 64, 0, p, 64, 0, p, nullptr, p, 32, 1, 8, 16, 64, 64, p, 0, p, nullptr) == VT_ERR_ARG);     // statistics without gamma
    EXPECT(vt_conv3x3_wgrad(p, 64, 0, p, 64, 0, p, p, p, 24, 1, 8, 16, 64, 64, p, 0, p, nullptr) == VT_ERR_ARG);           // Cin % groups != 0
    EXPECT(vt_conv3x3_wgrad(p, 64, 0, p, 64, 0, p, p, p, 32, 1, 8, 16, 64, 64, nullptr, 0, p, nullptr) == VT_ERR_ARG);
    EXPECT(vt_conv3x3_wgrad(p, 64, 0, p, 64, 0, p, p, p, 32, 70000, 8, 16, 64, 64, p, 0, p, nullptr) == VT_ERR_ARG);
    EXPECT(vt_conv1x1_wgrad(p, 64, 0, p, 64, 0, p, p, p, 32, 1, 8, 16, 64, 96, p, 0, p, nullptr) == VT_ERR_ARG);
    EXPECT(vt_gn_relu_backward(p, 32, 0, p, 32, 0, nullptr, p, p, 32, 1, 128, 32, nullptr, 0, 0, p, 32, 0, p, p, 0, p, nullptr) == VT_ERR_ARG);
    EXPECT(vt_gn_relu_backward(p, 32, 0, p, 32, 0, p, p, p, 32, 1, 128, 32, nullptr, 0, 0, nullptr, 0, 0, nullptr, nullptr, 0, p, nullptr) == VT_ERR_ARG);       // nothing to compute
    EXPECT(vt_gn_relu_backward(p, 32, 0, p, 32, 0, p, p, p, 32, 1, 128, 32, p, 32, 0, nullptr, 0, 0, p, p, 0, p, nullptr) == VT_ERR_ARG);                   // base without d_x
    EXPECT(vt_gn_relu_backward(p, 32, 0, p, 32, 0, p, p, p, 5, 1, 128, 32, nullptr, 0, 0, p, 32, 0, p, p, 0, p, nullptr) == VT_ERR_ARG);
    EXPECT(vt_conv_block_backward(nullptr, p, p, p, p, p, p, p, p, p, p, p, p, p, p, nullptr, nullptr, nullptr, 1, 8, 16, 128, 64, 32, 32,
                                  p, p, p, p, p, p, p, p, p, p, nullptr, nullptr, nullptr, p, 0, nullptr) == VT_ERR_ARG);
    EXPECT(vt_conv_block_backward(p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, nullptr, nullptr, nullptr, 1, 8, 16, 64, 64, 32, 32,                    // 64 -> 128 without a projection
                                  p, p, p, p, p, p, p, p, p, p, nullptr, nullptr, nullptr, p, 0, nullptr) == VT_ERR_ARG);
    EXPECT(vt_conv_block_backward(p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, nullptr, p, 1, 8, 16, 64, 64, 32, 32,                                // projection without gamma4
                                  p, p, p, p, p, p, p, p, p, p, nullptr, nullptr, nullptr, p, 0, nullptr) == VT_ERR_ARG);
    EXPECT(vt_conv_block_backward(p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, nullptr, nullptr, nullptr, 1, 8, 16, 128, 64, 32, 32,                   // projection gradients from an identity block
                                  p, p, p, p, p, p, p, p, p, p, p, nullptr, nullptr, p, 0, nullptr) == VT_ERR_ARG);
    EXPECT(vt_conv_block_backward(p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, nullptr, nullptr, nullptr, 1, 8, 16, 128, 64, 32, 32,
                                  odd, p, p, p, p, p, p, p, p, p, nullptr, nullptr, nullptr, p, 0, nullptr) == VT_ERR_ARG);                           // misaligned d_x
    printf(fails ? "convtrain host check: %d FAILED\n" : "convtrain host check: all refusals and sizes as expected (%d failures)\n", fails);
    return fails ? 1 : 0;
}
