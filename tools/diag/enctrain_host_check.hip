// Host memory-error run of csrc/enctrain.hip's host side (argument checks, workspace sizing, launch geometry helpers) and of vt_gn_relu_backward_y WITHOUT a device:
// every call below is refused by an argument check or answered by a sizing function before any HIP call is made.  Build with the host sanitizers and run on any
// machine:
//   hipcc -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I vistracker_amd/csrc tools/diag/enctrain_host_check.hip -o /tmp/enctrain_host_check && /tmp/enctrain_host_check
#include "../../vistracker_amd/csrc/convtrain.hip"
#include "../../vistracker_amd/csrc/enctrain.hip"

thread_local char vt_err_buf[512] = {0};

#define EXPECT(cond_) do { if (!(cond_)) { printf("FAILED line %d: %s (%s)\n", __LINE__, #cond_, vt_err_buf); fails++; } } while (0)

int main()
{
    int fails = 0;
    // sizing: every served shape, and the refusals
    for (int hw = 1; hw <= 1 << 20; hw *= 3) {
        EXPECT(enct::bias_blocks(hw) >= 1 && enct::bias_blocks(hw) <= ET_BIAS_MAXBLK);
        for (int B = 1; B <= 65535; B = B * 7 + 1) EXPECT(vt_bias_grad_workspace_bytes(B, hw, 256) >= (long)enct::bias_blocks(hw) * B * 256 * 8);
    }
    EXPECT(enct::bias_blocks(256) == 1 && enct::bias_blocks(257) == 2);
    EXPECT(vt_bias_grad_workspace_bytes(0, 4, 4) == -1 && vt_bias_grad_workspace_bytes(65536, 4, 4) == -1 && vt_bias_grad_workspace_bytes(1, 0, 4) == -1);
    EXPECT(vt_bias_grad_workspace_bytes(1, 4, 6) == -1 && vt_bias_grad_workspace_bytes(1, 4, 1028) == -1 && vt_bias_grad_workspace_bytes(1, 4, 0) == -1);
    for (int cin = 1; cin <= 8; cin++)
        for (int cout = 32; cout <= 64; cout += 32)
            for (int B = 1; B <= 65535; B = B * 7 + 1) {
                const int tiles = enct::stem_tiles(512, 512), ns = enct::stem_splits(B, tiles);
                EXPECT(tiles == 256 && ns >= 1 && ns <= 32 && ns <= tiles);
                EXPECT(vt_stem7x7_wgrad_workspace_bytes(B, 512, 512, cin, cout) >= (long)B * ns * cout * 49 * cin * 4);
                EXPECT(vt_stem7x7_wgrad_workspace_bytes(B, 1, 1, cin, cout) >= (long)B * cout * 49 * cin * 4);
            }
    EXPECT(enct::stem_tiles(1, 1) == 1 && enct::stem_tiles(32, 32) == 1 && enct::stem_tiles(34, 66) == 6 && enct::stem_splits(1, 1) == 1);
    EXPECT(vt_stem7x7_wgrad_workspace_bytes(1, 8, 8, 0, 64) == -1 && vt_stem7x7_wgrad_workspace_bytes(1, 8, 8, 9, 64) == -1 && vt_stem7x7_wgrad_workspace_bytes(1, 8, 8, 5, 48) == -1);
    EXPECT(vt_stem7x7_wgrad_workspace_bytes(0, 8, 8, 5, 64) == -1 && vt_stem7x7_wgrad_workspace_bytes(1, 0, 8, 5, 64) == -1 && vt_stem7x7_wgrad_workspace_bytes(1, 8, 40000, 5, 64) == -1);
    const int ch[3] = {64, 128, 256};
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
            const long w = vt_stack_tail_backward_workspace(2, 16, 32, ch[a], ch[b]);
            EXPECT(w >= (long)2 * 16 * 32 * (2 * ch[a] + ch[b]) * 4 && w % 256 == 0);
        }
    EXPECT(vt_stack_tail_backward_workspace(16, 128, 128, 256, 256) > 0 && vt_stack_tail_backward_workspace(16, 128, 128, 256, 64) > 0);
    EXPECT(vt_stack_tail_backward_workspace(1, 12, 32, 256, 256) == -1 && vt_stack_tail_backward_workspace(1, 16, 24, 256, 256) == -1 && vt_stack_tail_backward_workspace(0, 16, 32, 256, 256) == -1);
    EXPECT(vt_stack_tail_backward_workspace(1, 16, 32, 96, 256) == -1 && vt_stack_tail_backward_workspace(1, 16, 32, 256, 32) == -1 && vt_stack_tail_backward_workspace(1, 16, 32, 512, 256) == -1);

    // argument checks: refused before anything is launched (the pointers are never dereferenced on the host; they only have to be aligned)
    alignas(16) static float buf[64];
    float *p = buf, *odd = buf + 1;
    EXPECT(vt_bias_grad(nullptr, 32, 0, 1, 16, 32, p, 0, p, nullptr) == VT_ERR_ARG);
    EXPECT(vt_bias_grad(p, 32, 0, 1, 16, 32, nullptr, 0, p, nullptr) == VT_ERR_ARG);
    EXPECT(vt_bias_grad(p, 32, 0, 1, 16, 32, p, 0, nullptr, nullptr) == VT_ERR_ARG);
    EXPECT(vt_bias_grad(p, 32, 8, 1, 16, 32, p, 0, p, nullptr) == VT_ERR_ARG);            // slice past the channel stride
    EXPECT(vt_bias_grad(p, 34, 2, 1, 16, 32, p, 0, p, nullptr) == VT_ERR_ARG);            // offset not a multiple of 4
    EXPECT(vt_bias_grad(odd, 32, 0, 1, 16, 32, p, 0, p, nullptr) == VT_ERR_ARG);          // misaligned pointer
    EXPECT(vt_bias_grad(p, 32, 0, 1, 0, 32, p, 0, p, nullptr) == VT_ERR_ARG);
    EXPECT(vt_bias_grad(p, 32, 0, 70000, 16, 32, p, 0, p, nullptr) == VT_ERR_ARG);
    EXPECT(vt_stem7x7_wgrad(p, 64, 0, p, 5, 0, 1, 8, 8, 5, 64, nullptr, 0, p, nullptr) == VT_ERR_ARG);
    EXPECT(vt_stem7x7_wgrad(p, 64, 0, p, 5, 0, 1, 8, 8, 5, 64, p, 0, nullptr, nullptr) == VT_ERR_ARG);
    EXPECT(vt_stem7x7_wgrad(p, 64, 0, p, 5, 0, 1, 8, 8, 5, 48, p, 0, p, nullptr) == VT_ERR_ARG);
    EXPECT(vt_stem7x7_wgrad(p, 64, 0, p, 9, 0, 1, 8, 8, 9, 64, p, 0, p, nullptr) == VT_ERR_ARG);
    EXPECT(vt_stem7x7_wgrad(p, 32, 0, p, 5, 0, 1, 8, 8, 5, 64, p, 0, p, nullptr) == VT_ERR_ARG);             // d_y slice wider than its stride
    EXPECT(vt_stem7x7_wgrad(odd, 64, 0, p, 5, 0, 1, 8, 8, 5, 64, p, 0, p, nullptr) == VT_ERR_ARG);
    EXPECT(vt_stem7x7_wgrad(p, 64, 0, p, 5, 1, 1, 8, 8, 5, 64, p, 0, p, nullptr) == VT_ERR_ARG);             // input slice [1, 6) outside 5 channels
    EXPECT(vt_stem7x7_wgrad(p, 64, 0, nullptr, 5, 0, 1, 8, 8, 5, 64, p, 0, p, nullptr) == VT_ERR_ARG);
    EXPECT(vt_stem7x7_wgrad(p, 64, 0, p, 5, 0, 1, 0, 8, 5, 64, p, 0, p, nullptr) == VT_ERR_ARG);
    EXPECT(vt_gn_relu_backward_y(p, 32, 0, p, 32, 0, nullptr, 32, 0, p, p, 32, 1, 128, 32, nullptr, 0, 0, p, 32, 0, p, p, 0, p, nullptr) == VT_ERR_ARG);     // no saved output
    EXPECT(vt_gn_relu_backward_y(p, 32, 0, p, 32, 0, p, 32, 0, nullptr, p, 32, 1, 128, 32, nullptr, 0, 0, p, 32, 0, p, p, 0, p, nullptr) == VT_ERR_ARG);     // no statistics
    EXPECT(vt_gn_relu_backward_y(p, 32, 0, p, 32, 0, odd, 32, 0, p, p, 32, 1, 128, 32, nullptr, 0, 0, p, 32, 0, p, p, 0, p, nullptr) == VT_ERR_ARG);
    EXPECT(vt_gn_relu_backward_y(p, 32, 0, p, 32, 0, p, 32, 0, p, p, 32, 1, 128, 32, nullptr, 0, 0, nullptr, 0, 0, nullptr, nullptr, 0, p, nullptr) == VT_ERR_ARG);      // nothing to compute
    EXPECT(vt_gn_relu_backward_y(p, 32, 0, p, 32, 0, p, 32, 0, p, p, 5, 1, 128, 32, nullptr, 0, 0, p, 32, 0, p, p, 0, p, nullptr) == VT_ERR_ARG);
    EXPECT(vt_gn_relu_backward_y(p, 32, 0, p, 32, 0, p, 32, 0, p, p, 32, 1, 128, 32, p, 32, 0, nullptr, 0, 0, p, p, 0, p, nullptr) == VT_ERR_ARG);           // base without d_x
#define TAIL(dout_, dprev_, ll_, wbl_, wal_, out_, H_, C_, dll_, dwbl_, ws_) \
    vt_stack_tail_backward(dout_, dprev_, ll_, p, out_, p, p, p, p, p, wbl_, wal_, 1, H_, 16, C_, 256, dll_, p, p, p, p, p, p, dwbl_, nullptr, nullptr, nullptr, ws_, 0, nullptr)
    EXPECT(TAIL(nullptr, nullptr, p, p, p, p, 8, 256, p, nullptr, p) == VT_ERR_ARG);          // both upstream gradients absent
    EXPECT(TAIL(p, p, nullptr, p, p, p, 8, 256, p, nullptr, p) == VT_ERR_ARG);                // null input
    EXPECT(TAIL(p, p, p, nullptr, p, p, 8, 256, p, nullptr, p) == VT_ERR_ARG);                // d_prev without bl's weight
    EXPECT(TAIL(p, p, p, p, p, nullptr, 8, 256, p, nullptr, p) == VT_ERR_ARG);                // d_prev without the saved out
    EXPECT(TAIL(p, nullptr, p, nullptr, nullptr, nullptr, 8, 256, p, p, p) == VT_ERR_ARG);    // bl's gradient from the last stack
    EXPECT(TAIL(p, p, p, p, p, p, 9, 256, p, nullptr, p) == VT_ERR_ARG);                      // H % 8
    EXPECT(TAIL(p, p, p, p, p, p, 8, 96, p, nullptr, p) == VT_ERR_ARG);                       // channels
    EXPECT(TAIL(p, p, p, p, p, p, 8, 256, odd, nullptr, p) == VT_ERR_ARG);                    // misaligned d_ll
    EXPECT(TAIL(p, p, p, p, p, p, 8, 256, p, nullptr, nullptr) == VT_ERR_ARG);                // no workspace
#undef TAIL
    printf(fails ? "enctrain host check: %d FAILED\n" : "enctrain host check: all refusals and sizes as expected (%d failures)\n", fails);
    return fails ? 1 : 0;
}
