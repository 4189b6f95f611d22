"""The forward launch sequences of the HGFilter encoder, issued here for both of their callers: the inference encoder (``encoder.HGFilterEncoder``) and the
autograd functions of the trainable one (``ops._ConvBlockTrainFn`` and its siblings); one launch list is what makes the two forwards equal bit for bit.
The functions are plain: no autograd, no route counting, no CPU path, no argument validation -- those stay with the callers.  Tensors are fp32 device tensors,
contiguous in channels-last format; the launches go to the current stream of the current device (the inference pass runs under HIP-graph capture).

A producer hands the GroupNorm(32) statistics of its output to the block that reads it next as ``t._vt_stats = [workspace, n, finalized]``: a float64 workspace of
``B * 32`` {mean, rstd} slots + ``n`` blocks of per-channel partial sums, reduced to {mean, rstd} at its first use.  Only this module touches it.
"""
import torch

from . import _lib as L


def partials_workspace(B, C, n, device):
    """float64 workspace for the statistics of a (B, C, ., .) tensor: the {mean, rstd} area + ``n`` blocks of partial sums (sum, sum of squares per channel)"""
    return torch.empty(B * 32 + n * B * C * 2, dtype=torch.float64, device=device)


def attach_stats(t, ws, n, finalized=False):
    """the partial sums of ``t`` that its producer left behind in ``ws`` (``n`` blocks); finalized on first use unless they already are"""
    t._vt_stats = [ws, n, finalized]
    return t


def carry_stats(src, dst):
    """``dst`` holds the values of ``src`` (a copy in another layout): it shares the statistics ``src`` carries, if any"""
    if hasattr(src, "_vt_stats"):
        dst._vt_stats = src._vt_stats
    return dst


def partials_of(t):
    """(workspace, n) as attached to ``t``, untouched: for a caller that hands them on itself (an autograd function returns the workspace as an output)"""
    return tuple(t._vt_stats[:2])


def stats_of(x):
    """workspace with the finalized (B, 32) x {mean, rstd} of ``x`` if its producer left the partial sums behind, else None (the consumer runs a pass)"""
    st = getattr(x, "_vt_stats", None)
    if st is None:
        return None
    if not st[2]:
        B, C, H, W = x.shape
        L.check(L.lib().vt_groupnorm_finalize(st[0].data_ptr(), st[1], B, H * W, C, 32, 1e-5, L.stream_ptr()))
        st[2] = True
    return st[0]


def input_stats(x, use_producer):
    """{mean, rstd} workspace of a block's input: what the producer of ``x`` left behind (``use_producer``), else one vt_groupnorm_stats pass over ``x``"""
    ws = stats_of(x) if use_producer else None
    if ws is None:
        B, C, H, W = x.shape
        ws = torch.empty(L.lib().vt_groupnorm_workspace_doubles(B, H * W, C, 32), dtype=torch.float64, device=x.device)
        L.check(L.lib().vt_groupnorm_stats(x.data_ptr(), C, 0, B, H * W, C, 32, 1e-5, ws.data_ptr(), L.stream_ptr()))
    return ws


def conv1x1(handle, x, cout, gn=None, res=None, want_stats=False):
    """1 x 1 convolution (+ the handle's bias) on the split-f16 kernel.  ``gn`` = (stats workspace, gamma, beta): GroupNorm(32) + ReLU of the INPUT with those
    {mean, rstd} pairs, applied while the operand is staged; ``res``: tensor added to the result; ``want_stats``: the GroupNorm statistics of what was written
    (conv + bias [+ res]) are finalized and attached to it.  -> (out, the workspace of those statistics or None)"""
    lib = L.lib()
    B, Cin, H, W = x.shape
    out = torch.empty(B, cout, H, W, device=x.device, memory_format=torch.channels_last)
    tiles = lib.vt_conv3x3_tiles(H, W) if want_stats else 0
    ws_out = partials_workspace(B, cout, tiles, x.device) if want_stats else None
    ws, gamma, beta = gn if gn else (None, None, None)
    L.check(lib.vt_conv1x1_forward(handle, x.data_ptr(), Cin, 0, ws.data_ptr() if gn else None, gamma.data_ptr() if gn else None, beta.data_ptr() if gn else None, 32,
                                   B, H, W, out.data_ptr(), cout, 0, res.data_ptr() if res is not None else None, cout, 0,
                                   ws_out.data_ptr() if want_stats else None, 32, L.stream_ptr()))
    if want_stats:
        stats_of(attach_stats(out, ws_out, tiles))          # finalized at once: ws_out is handed to the consumers of ``out`` as it is
    return out, ws_out


def conv_block(h3, gammas, betas, x, ws_in, res, couts, want_out_stats):
    """The three 3 x 3 convolutions of a ConvBlock (model/net_util.py:346-396) on the split-f16 kernel: GroupNorm + ReLU in the operand staging (``ws_in``: the
    {mean, rstd} of ``x``; the inner convolutions' from the per-tile partial sums of their producer), and the block's result written by the convolutions
    themselves: ``raw`` holds o1 | o2 for the next convolution to read, ``fin`` = cat(o1, o2, o3) + ``res`` (``x`` or its projection, model/net_util.py:390-394),
    with ``want_out_stats`` carrying the partial sums of itself.
    -> (fin, raw, the {mean, rstd} workspaces of the three convolutions' inputs, the workspace of fin's partial sums or None)"""
    lib = L.lib()
    B, Cin, H, W = x.shape
    Ct, Cr = sum(couts), couts[0] + couts[1]
    tiles = lib.vt_conv3x3_tiles(H, W)
    raw = torch.empty(B, Cr, H, W, device=x.device, memory_format=torch.channels_last)
    fin = torch.empty(B, Ct, H, W, device=x.device, memory_format=torch.channels_last)
    ws_fin = partials_workspace(B, Ct, tiles, x.device) if want_out_stats else None
    src, cstride, coff, off = x, Cin, 0, 0
    stats = [ws_in]
    for i, co in enumerate(couts):
        last = i == 2
        ws_out = None if last else partials_workspace(B, co, tiles, x.device)
        L.check(lib.vt_conv3x3_forward_block_stats(h3[i], src.data_ptr(), cstride, coff, stats[-1].data_ptr(), gammas[i].data_ptr(), betas[i].data_ptr(), 32, B, H, W,
                                                   None if last else raw.data_ptr(), Cr, 0 if last else off, res.data_ptr(), Ct, off, fin.data_ptr(), Ct, off,
                                                   None if last else ws_out.data_ptr(), 32, ws_fin.data_ptr() if want_out_stats else None, 32, L.stream_ptr()))
        if not last:
            L.check(lib.vt_groupnorm_finalize(ws_out.data_ptr(), tiles, B, H * W, co, 32, 1e-5, L.stream_ptr()))
            stats.append(ws_out)
        src, cstride, coff = raw, Cr, off
        off += co
    return (attach_stats(fin, ws_fin, tiles) if want_out_stats else fin), raw, stats, ws_fin


def stack_tail(handles, gamma, beta, ll, previous, Co, last):
    """The tail of a stack (model/HGFilters.py:191-201) as four launches of the 1 x 1 kernel (two on the last stack): conv_last leaves the statistics of its
    output ``raw`` behind, bn_end (``gamma``, ``beta``) + ReLU is applied in the operand staging of its two consumers l and bl, and
    ``previous + bl(ll) + al(out)`` is the residual input of bl and al.  ``handles``: conv_last, l, bl, al.
    -> raw, bn_end's {mean, rstd} workspace, out, and the next stack's input with the workspace of its statistics (None, None when ``last``)"""
    h_cl, h_l, h_bl, h_al = handles
    C = ll.shape[1]
    raw, ws = conv1x1(h_cl, ll, C, want_stats=True)
    out, _ = conv1x1(h_l, raw, Co, gn=(ws, gamma, beta))
    if last:
        return raw, ws, out, None, None
    tmp, _ = conv1x1(h_bl, raw, C, gn=(ws, gamma, beta), res=previous)
    prev2, ws2 = conv1x1(h_al, out, C, res=tmp, want_stats=True)            # the next stack's b1 normalises it
    return raw, ws, out, prev2, ws2


def stem(handle, x, cout):
    """conv1 (model/HGFilters.py:118-130: 7 x 7 / stride 2 / pad 3 with bias) on the fp32 kernel -> (B, cout, ceil(H/2), ceil(W/2))"""
    B, cin, H, W = x.shape
    y1 = torch.empty(B, cout, (H - 1) // 2 + 1, (W - 1) // 2 + 1, device=x.device, memory_format=torch.channels_last)
    L.check(L.lib().vt_stem7x7_forward(handle, x.data_ptr(), cin, 0, B, H, W, y1.data_ptr(), cout, 0, L.stream_ptr()))
    return y1


def groupnorm_relu(y1, gamma, beta, groups=32, relu=True):
    """GroupNorm [+ ReLU] as one fused two-pass kernel pair on the channels-last storage (vt_groupnorm_nhwc) -> (y, the {mean, rstd} workspace)"""
    B, C, H, W = y1.shape
    y = torch.empty_like(y1, memory_format=torch.channels_last)
    ws = torch.empty(L.lib().vt_groupnorm_workspace_doubles(B, H * W, C, groups), dtype=torch.float64, device=y1.device)
    L.check(L.lib().vt_groupnorm_nhwc(y1.data_ptr(), gamma.data_ptr(), beta.data_ptr(), B, H * W, C, groups, 1e-5, int(relu), ws.data_ptr(), y.data_ptr(), L.stream_ptr()))
    return y, ws


def avgpool2x2_stats(x):
    """F.avg_pool2d(x, 2, stride=2) + the GroupNorm partial sums of the pooled tensor, attached to it, in one pass (C % 32 == 0 up to 1024, even H and W)"""
    B, C, H, W = x.shape
    out = torch.empty(B, C, H // 2, W // 2, device=x.device, memory_format=torch.channels_last)
    nblk = L.lib().vt_sweep_blocks((H // 2) * (W // 2))
    ws = partials_workspace(B, C, nblk, x.device)
    L.check(L.lib().vt_avgpool2x2_stats(x.data_ptr(), B, H, W, C, out.data_ptr(), ws.data_ptr(), 32, L.stream_ptr()))
    return attach_stats(out, ws, nblk)


def upsample2x_bicubic_add_stats(low, skip):
    """skip + bicubic x2 (align_corners=True) of ``low`` + the GroupNorm partial sums of the sum, attached to it (C % 32 == 0 up to 1024)"""
    B, C, h, w = low.shape
    out = torch.empty_like(skip, memory_format=torch.channels_last)
    nblk = L.lib().vt_sweep_blocks(4 * h * w)
    ws = partials_workspace(B, C, nblk, low.device)
    L.check(L.lib().vt_upsample2x_bicubic_add_stats(low.data_ptr(), skip.data_ptr(), B, h, w, C, out.data_ptr(), ws.data_ptr(), 32, L.stream_ptr()))
    return attach_stats(out, ws, nblk)
