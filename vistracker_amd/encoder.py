"""Image encoders of the SIF-Net (encoder half): inference-only mirror of ``model.HGFilters.HGFilter``
(HGFilters.py:4-203) and of the encoder part of ``CHORETriplane.filter`` (chore.py:128-144, chore_triplane.py:60-95).

The encoder is dense 2-D convolution work that runs ONCE per frame (613 GFLOP/frame).  Round 1 expressed it on the vendor
convolution library (MIOpen through ``torch.nn.functional``); since round 6 every convolution of the shipped configuration runs on the library's own
kernels (csrc/conv.hip: 3 x 3 and 1 x 1 as split-f16 implicit GEMMs; csrc/stem.hip: the 7 x 7 stem in fp32) and ``torch.nn.functional`` is only the
counted fallback for layer shapes those kernels do not serve (``routes``, ``strict_routes``) and the host path of the CPU tests.  Everything is in
channels-last memory format so that the outputs ARE the NHWC feature maps the fused query kernel gathers from -- no NCHW->NHWC pass.
The kernels read their weights from packed handles; ``_PackedHandles`` is the one store of them, for this encoder and for the ``Trainable*`` modules that issue
the same launches (``encoder_fwd``): packed on the device from the weight tensor at a convolution's first use, repacked in place when the tensor changes.
Weights are addressed by the reference's ``state_dict`` names, so a VisTracker checkpoint loads unchanged:

    enc = SIFNetEncoder.from_state_dict(torch.load(ckpt)["model_state_dict"])
    maps = enc(images)                       # images (B,8,512,512): RGB*mask, mask_h, mask_o, tri-right, tri-back, tri-top
    net.set_feature_maps(maps)               # == CHORETriplane.filter(images)

Architecture restated from the reference (stacked hourglass, group norm):
    conv1 7x7/2 -> GN -> ReLU = tmpx ; ConvBlock(tmpx,128) -> avgpool/2 = normx ; ConvBlock(128,128) ; ConvBlock(128,256) = previous
    per stack i: HourGlass(depth) -> ConvBlock(256,256) -> conv_last 1x1 -> GN -> ReLU = ll ; out_i = l_i 1x1 (ll) ;
                 previous += bl_i(ll) + al_i(out_i)            (all but the last stack)
    ConvBlock(cin,cout): three pre-activated 3x3 convs (cout/2, cout/4, cout/4) concatenated + (1x1-projected) residual
    HourGlass level n:   up = b1_n(x) ; low = b3_n( inner(b2_n(avgpool(x))) ) ; up + bicubic-upsample(low) ; inner = level n-1 or b2_plus_1
"""
from __future__ import annotations

import dataclasses
import numpy as np
import os

import torch
import torch.nn.functional as F

from . import _lib as L
from . import encoder_fwd as fwd
from . import ops
from .encoder_fwd import stats_of as _stats_of          # noqa: F401 -- the name the tests know


def state_dict_under(sd, prefix):
    """the entries of a state dict whose key, a leading 'module.' stripped, starts with ``prefix`` -> {key without the prefix: value}"""
    keys = ((k[7:] if k.startswith("module.") else k, v) for k, v in sd.items())
    return {k[len(prefix):]: v for k, v in keys if k.startswith(prefix)}


def as_f32(v, device):
    """a state dict's value (tensor or array) as an fp32 tensor on ``device``; no copy of one that is that already"""
    return torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v).detach().to(device=device, dtype=torch.float32)


def _leaf(v, device):
    return as_f32(v, device).contiguous().clone().requires_grad_(True)


def avgpool2x2(x):
    """F.avg_pool2d(x, 2, stride=2) of a channels-last GPU tensor on vt_avgpool2x2_stats: the pooled tensor + the GroupNorm partial sums of it for the
    ConvBlock that reads it next (one pass instead of torch's pooling kernel + a statistics pass)"""
    B, C, H, W = x.shape
    if not (x.is_cuda and C % 32 == 0 and C <= 1024 and H % 2 == 0 and W % 2 == 0):
        return F.avg_pool2d(x, 2, stride=2)
    return fwd.avgpool2x2_stats(x.contiguous(memory_format=torch.channels_last))


def upsample2x_bicubic_add(low, skip):
    """skip + bicubic x2 (align_corners=True) of ``low``; both NCHW-shaped channels-last tensors on the GPU -> same format
    (``vt_upsample2x_bicubic_add``; torch's channels-last bicubic kernel took 78 % of the encoder time)."""
    B, C, h, w = low.shape
    low = low.contiguous(memory_format=torch.channels_last); skip = skip.contiguous(memory_format=torch.channels_last)
    if C % 32 == 0 and C <= 1024:       # + the GroupNorm partial sums of the sum for the ConvBlock that reads it next (top_m / b3)
        return fwd.upsample2x_bicubic_add_stats(low, skip)
    out = torch.empty_like(skip, memory_format=torch.channels_last)
    L.check(L.lib().vt_upsample2x_bicubic_add(low.data_ptr(), skip.data_ptr(), B, h, w, C, out.data_ptr(), L.stream_ptr()))
    return out


def _gn(x, sd, p, groups=32, relu=False):
    """GroupNorm(32) [+ ReLU]; on the GPU one fused two-pass HIP kernel pair on the channels-last storage (vt_groupnorm_nhwc)"""
    if x.is_cuda and x.shape[1] % 4 == 0:
        return fwd.groupnorm_relu(x.contiguous(memory_format=torch.channels_last), sd[p + ".weight"], sd[p + ".bias"], groups, relu)[0]
    y = F.group_norm(x, groups, sd[p + ".weight"], sd[p + ".bias"], 1e-5)
    return F.relu(y) if relu else y


REPACK_CONV3X3, REPACK_CONV1X1, REPACK_STEM7X7 = 0, 1, 2          # include/vistracker.h: VT_REPACK_*
_HANDLE_FN = {REPACK_CONV3X3: "vt_conv3x3", REPACK_CONV1X1: "vt_conv1x1", REPACK_STEM7X7: "vt_stem7x7"}


@dataclasses.dataclass(eq=False, slots=True)
class _Packed:
    """one packed forward handle and the tensor pair (training leaves, or an inference encoder's stored weights) it was packed from"""
    handle: object          # ctypes.c_void_p
    version: object         # (weight version, bias version) when it was packed; None = repack at the next use
    kind: int               # REPACK_*
    weight: torch.Tensor
    bias: object            # leaf or None
    on_host: bool           # packed on the host (vt_*_create): replaced, not repacked in place


class _PackedHandles:
    """The packed forward handles of a module's convolutions, one per (weight, bias) tensor pair: the one store of the package, for the inference encoder
    (``HGFilterEncoder``, pairs out of its state dict) and the ``Trainable*`` modules (leaf pairs) alike, and the one owner of the handles' lifetime.  A handle is
    created ONCE, at the convolution's first use, on the device and straight from the tensor (``vt_*_create_device``), and repacked in place (``vt_*_repack``, two
    launches on the current stream) when a version counter of its pair changed since it was packed: no copy to the host, no synchronisation, no destroy -- the
    handle's address is stable for the life of the module, and ordering on the stream protects the launches that still read the old packing.  ``EncoderAdam``
    repacks all handles of a network in one plan and marks them current, so that the check here finds nothing to do.  An update that goes round the version
    counters (a kernel writing through ``data_ptr()``, as ``ops.FusedAdam`` does) has to say so with ``invalidate_handles()``.

    ``VT_ENCODER_HOST_REPACK=1`` (``host_repack``) keeps the path this replaced, as the reference of the bit-equality tests and for A/B: synchronise, destroy the
    handle, pull the tensor to the host, pack it there with ``vt_*_create`` and copy it back up, per convolution and change.  It is the package's only use of the
    host packers."""
    host_repack = os.environ.get("VT_ENCODER_HOST_REPACK", "0") != "0"

    def _init_handles(self):
        self._handles = {}          # key -> _Packed

    def _packed(self, key, kind, w, b, device):
        import ctypes as C
        ent = self._handles.get(key)
        ver = (w._version, b._version if b is not None else -1)
        if ent is not None and ent.version == ver and ent.weight is w and ent.bias is b:
            return ent.handle
        lib, fn = L.lib(), _HANDLE_FN[kind]
        cout, cin = w.shape[:2]
        bias_arg = kind != REPACK_CONV3X3
        wc = w.detach().contiguous()            # the packers read (Cout, Cin, ky * k + kx) in NCHW order: a copy only of a weight stored channels-last
        if ent is not None and (self.host_repack or ent.on_host):
            torch.cuda.synchronize(device)          # launches that read the old packing may still be queued
            getattr(lib, fn + "_destroy")(ent.handle)
            ent = None
        with torch.cuda.device(device):
            if self.host_repack:
                wh = np.ascontiguousarray(wc.cpu().numpy().reshape(cout, cin, -1), np.float32)
                bh = np.ascontiguousarray(b.detach().cpu().numpy(), np.float32) if b is not None else None
                h = C.c_void_p()
                args = (wh.ctypes.data, bh.ctypes.data if bh is not None else None) if bias_arg else (wh.ctypes.data,)
                L.check(getattr(lib, fn + "_create")(C.byref(h), *args, cout, cin, L.stream_ptr()))
                ent = _Packed(h, ver, kind, w, b, True)
            else:
                args = (L.dptr(wc), L.dptr(b.detach()) if b is not None else None) if bias_arg else (L.dptr(wc),)
                if ent is None:
                    h = C.c_void_p()
                    L.check(getattr(lib, fn + "_create_device")(C.byref(h), *args, cout, cin, L.stream_ptr()))
                    ent = _Packed(h, ver, kind, w, b, False)
                else:
                    L.check(getattr(lib, fn + "_repack")(ent.handle, *args, L.stream_ptr()))
                    ent.version, ent.weight, ent.bias = ver, w, b          # a replaced leaf object is the pair the handle follows from now on
        self._handles[key] = ent
        return ent.handle

    def invalidate_handles(self):
        """the leaves were written behind the version counters: repack every handle at its next use"""
        for ent in self._handles.values():
            ent.version = None

    def _mark_handles_current(self):
        for ent in self._handles.values():
            ent.version = (ent.weight._version, ent.bias._version if ent.bias is not None else -1)

    def __del__(self):
        try:
            for ent in getattr(self, "_handles", {}).values():
                getattr(L.lib(), _HANDLE_FN[ent.kind] + "_destroy")(ent.handle)
        except Exception:
            pass


class HGFilterEncoder(_PackedHandles):
    # 3x3 convolutions with 32 / 64 / 128 output channels and Cin % 32 == 0 and the 1x1 convolutions (conv_last / l / bl / al of a stack, the
    # ConvBlocks' projections) run on the split-f16 implicit-GEMM kernel (csrc/conv.hip, vt_conv3x3_* / vt_conv1x1_*); the 7x7 stem (Cout 32 / 64, Cin <= 8) on
    # the fp32 kernel of csrc/stem.hip (round 6: until then the encoder's one MIOpen call).  Other shapes fall back to MIOpen -- counted, and refused
    # in strict mode.
    use_hip_conv = True
    # GroupNorm statistics of a block's input from the partial sums its PRODUCER left behind (previous block's epilogue, pooling, up-sampling, the 1 x 1
    # sum at the end of a stack) instead of a statistics pass over the tensor; False = round 2's passes (A/B, tests)
    producer_stats = True
    # Which route every convolution of a pass took (a checkpoint with other widths must not quietly measure MIOpen): ``routes`` counts
    # "hip7x7" / "hip3x3" / "hip1x1" / "miopen:<layer>" per call; with ``strict_routes`` any convolution that leaves the HIP kernels raises.
    strict_routes = os.environ.get("VT_ENCODER_STRICT_ROUTES", "0") != "0"
    use_hip_stem = os.environ.get("VT_ENCODER_HIP_STEM", "1") != "0"        # 0: the stem on MIOpen as before round 6 (A/B only)

    def _miopen(self, what, x, w, b=None, stride=1, padding=0):
        self.routes["miopen:" + what] += 1
        if self.strict_routes and x.is_cuda and self.use_hip_conv:
            raise L.VtError(f"HGFilterEncoder: convolution '{what}' (weight {tuple(w.shape)}, input {tuple(x.shape)}) is not served by the HIP kernels and "
                            f"VT_ENCODER_STRICT_ROUTES is set")
        return F.conv2d(x, w, b, stride, padding)

    def __init__(self, sd: dict, prefix: str, num_stack=3, num_hourglass=2, norm="group", hg_down="ave_pool", device="cuda:0"):
        """``sd``: state dict (tensors or arrays); ``prefix`` e.g. 'image_filter.' or 'triplane_encoder.' (a leading 'module.' is stripped)"""
        if norm != "group" or hg_down != "ave_pool":
            raise NotImplementedError("only the configuration VisTracker ships (config/*.json: norm=group, hg_down=ave_pool) is mirrored")
        self.device = torch.device(device)
        self.num_stack, self.depth = num_stack, num_hourglass
        self.sd = {}
        for k, v in state_dict_under(sd, prefix).items():
            t = as_f32(v, self.device)
            self.sd[k] = t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t
        if "conv1.weight" not in self.sd:
            raise KeyError(f"no encoder weights under prefix '{prefix}'")
        self.in_channels = self.sd["conv1.weight"].shape[1]
        self._init_handles()
        import collections
        self.routes = collections.Counter()

    def _stem(self, x):
        """conv1 (HGFilters.py:118-130, 7 x 7 / stride 2 / pad 3 with bias) -> channels-last (B, 64, ceil(H/2), ceil(W/2))"""
        w = self.sd["conv1.weight"]; cout, cin = w.shape[:2]
        if not (x.is_cuda and self.use_hip_conv and self.use_hip_stem and cout in (32, 64) and cin <= 8 and tuple(w.shape[2:]) == (7, 7)):
            return self._miopen("stem7x7", x, w, self.sd.get("conv1.bias"), 2, 3)
        self.routes["hip7x7"] += 1
        h = self._packed((REPACK_STEM7X7, "conv1.weight"), REPACK_STEM7X7, w, self.sd.get("conv1.bias"), self.device)
        return fwd.stem(h, x.contiguous(memory_format=torch.channels_last), cout)

    def _hip_conv1x1_ok(self, wname, H, W, cuda):
        cout, cin = self.sd[wname].shape[:2]
        return self.use_hip_conv and cuda and cout in (64, 128, 256) and cin in (32, 64, 128, 256) and H % 8 == 0 and W % 16 == 0 and tuple(self.sd[wname].shape[2:]) == (1, 1)

    def _hip_conv_ok(self, name, H, W, cuda):
        cout, cin = self.sd[name].shape[:2]
        return self.use_hip_conv and cuda and cout in (32, 64, 128) and cin % 32 == 0 and H % 8 == 0 and W % 16 == 0

    # ---- blocks ------------------------------------------------------------------------------------------------
    def _conv_block(self, x, p):
        """ConvBlock (model/net_util.py:346-396): three pre-activated 3x3 convolutions (GN -> ReLU -> conv), outputs concatenated, + (projected)
        residual.  On the GPU every convolution writes its channel slice of ONE NHWC buffer (the concatenation is free) and reads its input from
        the previous slice; supported shapes (32 / 64 / 128 output channels, Cin % 32 == 0, H % 8 == 0, W % 16 == 0) run GroupNorm statistics + the fused
        GN/ReLU/conv kernel (vt_groupnorm_stats, vt_conv3x3_forward_gn), anything else normalises with vt_groupnorm_nhwc and convolves on MIOpen."""
        sd = self.sd
        B, Cin, H, W = x.shape
        couts = [sd[p + f"conv{i}.weight"].shape[0] for i in (1, 2, 3)]
        if x.is_cuda and all(self._hip_conv_ok(p + f"conv{i}.weight", H, W, True) for i in (1, 2, 3)):
            return self._conv_block_fused(x, p, couts)
        if not (x.is_cuda and any(self._hip_conv_ok(p + f"conv{i}.weight", H, W, True) for i in (1, 2, 3))):
            o1 = self._miopen(p + "conv1", _gn(x, sd, p + "bn1", relu=True), sd[p + "conv1.weight"], None, 1, 1)
            o2 = self._miopen(p + "conv2", _gn(o1, sd, p + "bn2", relu=True), sd[p + "conv2.weight"], None, 1, 1)
            o3 = self._miopen(p + "conv3", _gn(o2, sd, p + "bn3", relu=True), sd[p + "conv3.weight"], None, 1, 1)
            out = torch.cat((o1, o2, o3), 1)
        else:
            x = x.contiguous(memory_format=torch.channels_last)
            Ct = sum(couts)
            out = torch.empty(B, Ct, H, W, device=x.device, memory_format=torch.channels_last)          # NHWC in memory
            src, cstride, coff, C = x, Cin, 0, Cin
            off = 0
            lib = L.lib()
            tiles = lib.vt_conv3x3_tiles(H, W)
            ws_prev = None              # statistics of the current input slice left behind by the convolution that produced it
            for i, co in zip((1, 2, 3), couts):
                wn, gn = p + f"conv{i}.weight", p + f"bn{i}"
                if self._hip_conv_ok(wn, H, W, True):
                    if ws_prev is None:         # input from outside the block (or from a library convolution): one statistics pass
                        ws = torch.empty(lib.vt_groupnorm_workspace_doubles(B, H * W, C, 32), dtype=torch.float64, device=x.device)
                        L.check(lib.vt_groupnorm_stats(src.data_ptr(), cstride, coff, B, H * W, C, 32, 1e-5, ws.data_ptr(), L.stream_ptr()))
                    else:                       # the producing convolution wrote per-tile partial sums: reduce them, no pass over the tensor
                        ws = ws_prev
                        L.check(lib.vt_groupnorm_finalize(ws.data_ptr(), tiles, B, H * W, C, 32, 1e-5, L.stream_ptr()))
                    nxt = i < 3 and self._hip_conv_ok(p + f"conv{i + 1}.weight", H, W, True)
                    ws_out = fwd.partials_workspace(B, co, tiles, x.device) if nxt else None
                    self.routes["hip3x3"] += 1
                    L.check(lib.vt_conv3x3_forward_gn_stats(self._packed((REPACK_CONV3X3, wn), REPACK_CONV3X3, sd[wn], None, self.device), src.data_ptr(), cstride, coff, ws.data_ptr(),
                                                            sd[gn + ".weight"].data_ptr(), sd[gn + ".bias"].data_ptr(), 32, B, H, W, out.data_ptr(), Ct, off,
                                                            ws_out.data_ptr() if nxt else None, 32, L.stream_ptr()))
                    ws_prev = ws_out
                else:
                    xin = src if (cstride == C and coff == 0) else src[:, coff:coff + C]
                    out[:, off:off + co] = self._miopen(wn[:-7], _gn(xin, sd, gn, relu=True), sd[wn], None, 1, 1)
                    ws_prev = None
                src, cstride, coff, C = out, Ct, off, co
                off += co
        if p + "downsample.2.weight" in sd:
            # downsample = Sequential(bn4, ReLU, conv1x1): the norm is the module the state dict also lists as "bn4" (same tensors in a
            # real checkpoint); "downsample.0" is the name that is loaded last, i.e. the one the reference ends up using
            x = self._miopen(p + "downsample", _gn(x, sd, p + "downsample.0", relu=True), sd[p + "downsample.2.weight"])
        return out + x

    def _conv_block_fused(self, x, p, couts):
        """all three convolutions on the split-f16 kernel (``encoder_fwd.conv_block``): GroupNorm + ReLU in the operand staging, the block's result
        (concatenation + residual, model/net_util.py:390-394) written by the convolutions themselves; the residual is ``x`` or its 1 x 1 projection"""
        sd = self.sd
        H, W = x.shape[2:]
        x = x.contiguous(memory_format=torch.channels_last)
        Ct = sum(couts)
        ws = fwd.input_stats(x, self.producer_stats)      # left behind by the producer of x (previous block, pooling, up-sampling, 1 x 1 sum), else one pass
        res, wp = x, p + "downsample.2.weight"
        if wp in sd:         # see _conv_block: Sequential(bn4, ReLU, conv1x1)
            if self._hip_conv1x1_ok(wp, H, W, True):
                # the projection's GroupNorm normalises the same tensor as bn1: same {mean, rstd}, its own gamma / beta, fused into the staging
                self.routes["hip1x1"] += 1
                res, _ = fwd.conv1x1(self._packed((REPACK_CONV1X1, wp), REPACK_CONV1X1, sd[wp], None, self.device), x, sd[wp].shape[0],
                                     gn=(ws, sd[p + "downsample.0.weight"], sd[p + "downsample.0.bias"]))
            else:
                res = self._miopen(p + "downsample", _gn(x, sd, p + "downsample.0", relu=True), sd[wp]).contiguous(memory_format=torch.channels_last)
        assert res.shape[1] == Ct
        self.routes["hip3x3"] += 3
        handles = [self._packed((REPACK_CONV3X3, n), REPACK_CONV3X3, sd[n], None, self.device) for n in (p + "conv1.weight", p + "conv2.weight", p + "conv3.weight")]
        return fwd.conv_block(handles, [sd[p + f"bn{i}.weight"] for i in (1, 2, 3)], [sd[p + f"bn{i}.bias"] for i in (1, 2, 3)], x, ws, res, couts,
                              self.producer_stats and Ct % 32 == 0)[0]

    def _hourglass(self, level, x, p):
        up1 = self._conv_block(x, f"{p}b1_{level}.")
        low = self._conv_block(avgpool2x2(x) if self.producer_stats else F.avg_pool2d(x, 2, stride=2), f"{p}b2_{level}.")
        low = self._hourglass(level - 1, low, p) if level > 1 else self._conv_block(low, f"{p}b2_plus_{level}.")
        low = self._conv_block(low, f"{p}b3_{level}.")
        if low.is_cuda and low.shape[1] % 4 == 0:
            return upsample2x_bicubic_add(low, up1)
        return up1 + F.interpolate(low, scale_factor=2, mode="bicubic", align_corners=True)       # host tensors (tools / debugging only)

    @torch.no_grad()
    def __call__(self, x):
        """x (B,C,H,W) -> (outputs [num_stack x (B,hourglass_dim,H/4,W/4)], tmpx (B,tmpx_dim,H/2,W/2), normx (B,128,H/4,W/4)); channels-last"""
        sd = self.sd
        x = x.to(self.device).float().contiguous(memory_format=torch.channels_last)
        x = _gn(self._stem(x), sd, "bn1", relu=True)
        tmpx = x
        x = self._conv_block(x, "conv2.")
        x = avgpool2x2(x) if self.producer_stats else F.avg_pool2d(x, 2, stride=2)
        normx = x
        previous = self._conv_block(self._conv_block(x, "conv3."), "conv4.")
        outputs = []
        for i in range(self.num_stack):
            ll = self._conv_block(self._hourglass(self.depth, previous, f"m{i}."), f"top_m_{i}.")
            H, W = ll.shape[2:]
            last = i == self.num_stack - 1
            names = [f"conv_last{i}.weight", f"l{i}.weight"] + ([] if last else [f"bl{i}.weight", f"al{i}.weight"])
            if ll.is_cuda and all(self._hip_conv1x1_ok(n, H, W, True) for n in names):
                # the tail of a stack as four launches of the 1 x 1 kernel (two on the last stack)
                handles = [self._packed((REPACK_CONV1X1, n), REPACK_CONV1X1, sd[n], sd.get(n[:-6] + "bias"), self.device) for n in names] + [None] * (4 - len(names))
                self.routes["hip1x1"] += len(names)
                ll, previous = (t.contiguous(memory_format=torch.channels_last) for t in (ll, previous))
                _, _, out, nxt, _ = fwd.stack_tail(handles, sd[f"bn_end{i}.weight"], sd[f"bn_end{i}.bias"], ll, previous, sd[f"l{i}.weight"].shape[0], last)
                outputs.append(out)
                previous = previous if last else nxt
                continue
            ll = _gn(self._miopen(f"conv_last{i}", ll, sd[f"conv_last{i}.weight"], sd[f"conv_last{i}.bias"]), sd, f"bn_end{i}", relu=True)
            out = self._miopen(f"l{i}", ll, sd[f"l{i}.weight"], sd[f"l{i}.bias"])
            outputs.append(out)
            if not last:
                previous = previous + self._miopen(f"bl{i}", ll, sd[f"bl{i}.weight"], sd[f"bl{i}.bias"]) + self._miopen(f"al{i}", out, sd[f"al{i}.weight"], sd[f"al{i}.bias"])
        return outputs, tmpx, normx


class TrainableConvBlock(_PackedHandles):
    """One ConvBlock (model/net_util.py:346-396) with its parameters as fp32 device LEAVES under the reference's ``state_dict`` keys, differentiable through
    ``ops.conv_block_train``: the forward is the fused inference forward bit for bit (both call ``encoder_fwd.conv_block``), the backward one
    ``vt_conv_block_backward`` call (csrc/convtrain.hip).

        blk = TrainableConvBlock.from_state_dict(sd, "image_filter.conv3.")
        y = blk(x)                      # channels-last (B,Cout,H,W), carries autograd
        y.backward(dy)                  # blk.leaves["conv1.weight"].grad, ..., x.grad

    The forward's packed split-f16 convolution handles follow the leaves on the device (``_PackedHandles``); ``EncoderAdam`` is the optimiser that keeps a step
    free of host waits."""
    _W = ("conv1.weight", "conv2.weight", "conv3.weight")

    def __init__(self, leaves: dict, device):
        self.device = torch.device(device)
        self.leaves = leaves
        self.has_proj = "downsample.2.weight" in leaves
        self._init_handles()

    @classmethod
    def from_state_dict(cls, sd, prefix="", device="cuda:0"):
        """``sd``: tensors or arrays; ``prefix`` e.g. 'image_filter.conv3.' (a leading 'module.' is stripped).  The projection's norm is read from
        'downsample.0.*' when present (the name the reference loads last), else from 'bn4.*'; both names are written by ``state_dict()``."""
        got = {k: _leaf(v, device) for k, v in state_dict_under(sd, prefix).items()}
        for k in cls._W + tuple(f"bn{i}.{s}" for i in (1, 2, 3) for s in ("weight", "bias")):
            if k not in got:
                raise KeyError(f"no ConvBlock parameter '{prefix}{k}'")
        leaves = {k: got[k] for k in cls._W}
        for i in (1, 2, 3):
            leaves[f"bn{i}.weight"], leaves[f"bn{i}.bias"] = got[f"bn{i}.weight"], got[f"bn{i}.bias"]
        n4 = "downsample.0" if "downsample.0.weight" in got else "bn4"
        if n4 + ".weight" in got:
            leaves["bn4.weight"], leaves["bn4.bias"] = got[n4 + ".weight"], got[n4 + ".bias"]
        if "downsample.2.weight" in got:
            leaves["downsample.2.weight"] = got["downsample.2.weight"]
            if "bn4.weight" not in leaves:
                raise KeyError(f"'{prefix}downsample.2.weight' without the projection's norm")
        return cls(leaves, device)

    def state_dict(self):
        out = {k: v.detach().clone() for k, v in self.leaves.items()}
        if self.has_proj:
            out["downsample.0.weight"], out["downsample.0.bias"] = out["bn4.weight"].clone(), out["bn4.bias"].clone()
        return out

    def parameters(self):
        """the leaves an optimiser updates (an identity block's bn4 is carried but not used by the reference's forward either: it never receives a gradient)"""
        return [v for k, v in self.leaves.items() if self.has_proj or not k.startswith("bn4.")]

    def tensors(self):
        """the leaves in ``ops.CONV_BLOCK_PARAMS`` order; None for the projection's three without one"""
        lv = self.leaves
        proj = [lv["downsample.2.weight"], lv["bn4.weight"], lv["bn4.bias"]] if self.has_proj else [None, None, None]
        return [lv[k] for k in self._W] + [lv[f"bn{i}.weight"] for i in (1, 2, 3)] + [lv[f"bn{i}.bias"] for i in (1, 2, 3)] + proj

    def handles(self, device):
        """([3 x vt_conv3x3], vt_conv1x1 or None): the packed forward handles, repacked in place from a leaf whose version counter changed since it was packed"""
        out = [self._packed(k, REPACK_CONV1X1 if self.leaves[k].shape[2] == 1 else REPACK_CONV3X3, self.leaves[k], None, device)
               for k in self._W + (("downsample.2.weight",) if self.has_proj else ())]
        return out[:3], (out[3] if self.has_proj else None)

    def __call__(self, x):
        return ops.conv_block_train(x, self)


class TrainableHourglass:
    """One ``HourGlass(1, depth, features, norm='group')`` (model/HGFilters.py:4-53) that trains: a ``TrainableConvBlock`` per reference module in ``.blocks``
    (keys 'b1_n', 'b2_n', 'b3_n' for n = depth .. 1 and 'b2_plus_1', the reference's ``state_dict`` names), joined by ``ops.avgpool2x2_train`` and
    ``ops.upsample2x_bicubic_add_train``.  The forward is the recursion of ``HGFilterEncoder._hourglass`` bit for bit; the backward is one
    ``vt_conv_block_backward`` call per block, one ``vt_avgpool2x2_backward`` and one ``vt_upsample2x_bicubic_backward`` per level.

        hg = TrainableHourglass.from_state_dict(sd, "image_filter.m0.", depth=2)
        y = hg(x)                       # channels-last (B,features,H,W), carries autograd
        y.backward(dy)                  # hg.blocks["b2_plus_1"].leaves["conv1.weight"].grad, ..., x.grad

    A shape that a block does not serve raises that block's own error (H % 8 == 0 and W % 16 == 0 must still hold at the innermost level)."""

    def __init__(self, blocks: dict, depth: int, device):
        self.device = torch.device(device)
        self.depth = int(depth)
        self.blocks = blocks

    @staticmethod
    def block_names(depth):
        """the reference's module names in registration order (HGFilters.py:14-24)"""
        names = []
        for n in range(depth, 0, -1):
            names += [f"b1_{n}", f"b2_{n}"]
        names.append("b2_plus_1")
        return names + [f"b3_{n}" for n in range(1, depth + 1)]

    @classmethod
    def from_state_dict(cls, sd, prefix="", depth=2, device="cuda:0"):
        """``sd``: tensors or arrays; ``prefix`` e.g. 'image_filter.m0.' (a leading 'module.' is stripped)"""
        if depth < 1:
            raise ValueError("depth >= 1")
        return cls({n: TrainableConvBlock.from_state_dict(sd, f"{prefix}{n}.", device=device) for n in cls.block_names(depth)}, depth, device)

    def state_dict(self):
        return {f"{n}.{k}": v for n, blk in self.blocks.items() for k, v in blk.state_dict().items()}

    def parameters(self):
        return [p for blk in self.blocks.values() for p in blk.parameters()]

    def _level(self, n, x):
        up1 = self.blocks[f"b1_{n}"](x)
        low = self.blocks[f"b2_{n}"](ops.avgpool2x2_train(x))
        low = self._level(n - 1, low) if n > 1 else self.blocks["b2_plus_1"](low)
        low = self.blocks[f"b3_{n}"](low)
        return ops.upsample2x_bicubic_add_train(low, up1)

    def __call__(self, x):
        return self._level(self.depth, x)


class TrainableStem(_PackedHandles):
    """conv1 + bn1 + ReLU (model/HGFilters.py:120-125, 167) with the four parameters as fp32 device leaves under the keys of ``ops.STEM_PARAMS``; differentiable
    through ``ops.stem_train``."""

    def __init__(self, leaves: dict, device):
        self.device = torch.device(device)
        self.leaves = leaves
        self._init_handles()

    def tensors(self):
        return [self.leaves[k] for k in ops.STEM_PARAMS]

    def parameters(self):
        return self.tensors()

    def handles(self, device):
        """the packed vt_stem7x7 forward handle"""
        return self._packed("conv1", REPACK_STEM7X7, self.leaves["conv1.weight"], self.leaves["conv1.bias"], device)

    def __call__(self, x):
        return ops.stem_train(x, self)


class TrainableStackTail(_PackedHandles):
    """conv_last, bn_end, l and, before the last stack, bl and al of one stack (model/HGFilters.py:146-160, 191-201) as fp32 device leaves under the keys of
    ``ops.STACK_TAIL_PARAMS`` (the reference's names without the stack index); differentiable through ``ops.stack_tail_train``."""

    def __init__(self, leaves: dict, last: bool, device):
        self.device = torch.device(device)
        self.leaves = leaves
        self.last = bool(last)
        self._init_handles()

    def tensors(self):
        return [self.leaves.get(k) for k in ops.STACK_TAIL_PARAMS]

    def parameters(self):
        return [t for t in self.tensors() if t is not None]

    def handles(self, device):
        """[conv_last, l, bl, al]: the packed vt_conv1x1 forward handles (bl and al None on the last stack)"""
        return [self._packed(n, REPACK_CONV1X1, self.leaves[n + ".weight"], self.leaves[n + ".bias"], device) if n + ".weight" in self.leaves else None
                for n in ("conv_last", "l", "bl", "al")]

    def __call__(self, ll, previous=None):
        return ops.stack_tail_train(ll, previous, self, self.last)


class TrainableHGFilter:
    """The reference's ``HGFilter`` (model/HGFilters.py:56-203; norm='group', hg_down='ave_pool') that trains: every parameter an fp32 device leaf, the forward
    the launches of ``HGFilterEncoder.__call__`` bit for bit (both sides issue them through ``encoder_fwd``), the backward entirely on the library's kernels.  Built from a ``TrainableStem`` (``.stem``),
    ``TrainableConvBlock``s (``.blocks``: 'conv2', 'conv3', 'conv4', 'top_m_i'), ``TrainableHourglass``es (``.hourglasses[i]`` = m_i) and ``TrainableStackTail``s
    (``.tails[i]``), joined by ``ops.avgpool2x2_train``.

        enc = TrainableHGFilter.from_state_dict(sd, "image_filter.", num_stack=3, num_hourglass=2)
        outputs, tmpx, normx = enc(images)          # tmpx is detached (HGFilters.py:203); outputs and normx carry autograd
        loss.backward()                             # p.grad for p in enc.parameters()

    Serves the image encoder (Cin 5, tmpx 64) and the triplane encoder (Cin 1, tmpx 32).  The input needs H % 32 == 0 and W % 64 == 0 times 2^num_hourglass for
    the innermost level of an hourglass to be a multiple of 8 x 16.

    ``EncoderAdam(enc)`` is the optimiser: one Adam launch over all parameters and one two-launch repack of all packed forward handles, no host wait."""

    def __init__(self, stem, blocks, hourglasses, tails, num_hourglass, device):
        self.device = torch.device(device)
        self.stem, self.blocks, self.hourglasses, self.tails = stem, blocks, hourglasses, tails
        self.num_stack, self.depth = len(tails), int(num_hourglass)

    @classmethod
    def from_state_dict(cls, sd, prefix="", num_stack=3, num_hourglass=2, device="cuda:0"):
        """``sd``: tensors or arrays under the reference's keys; ``prefix`` e.g. 'image_filter.' or 'triplane_encoder.' (a leading 'module.' is stripped)"""
        own = state_dict_under(sd, prefix)

        def need(k):
            if k not in own:
                raise KeyError(f"no encoder parameter '{prefix}{k}'")
            return _leaf(own[k], device)

        stem = TrainableStem({k: need(k) for k in ops.STEM_PARAMS}, device)
        blocks = {n: TrainableConvBlock.from_state_dict(own, n + ".", device=device) for n in ["conv2", "conv3", "conv4"] + [f"top_m_{i}" for i in range(num_stack)]}
        hgs = [TrainableHourglass.from_state_dict(own, f"m{i}.", depth=num_hourglass, device=device) for i in range(num_stack)]
        tails = []
        for i in range(num_stack):
            last = i == num_stack - 1
            names = ("conv_last", "bn_end", "l") + (() if last else ("bl", "al"))
            tails.append(TrainableStackTail({f"{n}.{s}": need(f"{n}{i}.{s}") for n in names for s in ("weight", "bias")}, last, device))
        return cls(stem, blocks, hgs, tails, num_hourglass, device)

    def state_dict(self):
        """the reference's keys (HGFilter.state_dict())"""
        out = {k: v.detach().clone() for k, v in self.stem.leaves.items()}
        for n, blk in self.blocks.items():
            out.update({f"{n}.{k}": v for k, v in blk.state_dict().items()})
        for i, (hg, tail) in enumerate(zip(self.hourglasses, self.tails)):
            out.update({f"m{i}.{k}": v for k, v in hg.state_dict().items()})
            for k, v in tail.leaves.items():
                n, s = k.split(".")
                out[f"{n}{i}.{s}"] = v.detach().clone()
        return out

    def named_parameters(self):
        """(reference key, leaf) of every parameter an optimiser updates"""
        out = list(self.stem.leaves.items())
        for n, blk in self.blocks.items():
            out += [(f"{n}.{k}", v) for k, v in blk.leaves.items() if blk.has_proj or not k.startswith("bn4.")]
        for i, (hg, tail) in enumerate(zip(self.hourglasses, self.tails)):
            for bn, blk in hg.blocks.items():
                out += [(f"m{i}.{bn}.{k}", v) for k, v in blk.leaves.items() if blk.has_proj or not k.startswith("bn4.")]
            for k, v in tail.leaves.items():
                n, s = k.split(".")
                out.append((f"{n}{i}.{s}", v))
        return out

    def parameters(self):
        return [v for _, v in self.named_parameters()]

    def __call__(self, x):
        """x (B,Cin,H,W) -> (outputs [num_stack x (B,hourglass_dim,H/4,W/4)], tmpx (B,tmpx_dim,H/2,W/2) detached, normx (B,128,H/4,W/4)); channels-last"""
        x = x.to(self.device).float().contiguous(memory_format=torch.channels_last)
        t = self.stem(x)
        tmpx = t.detach()
        normx = ops.avgpool2x2_train(self.blocks["conv2"](t))
        previous = self.blocks["conv4"](self.blocks["conv3"](normx))
        outputs = []
        for i, (hg, tail) in enumerate(zip(self.hourglasses, self.tails)):
            ll = self.blocks[f"top_m_{i}"](hg(previous))
            if tail.last:
                outputs.append(tail(ll))
            else:
                out, previous = tail(ll, previous)
                outputs.append(out)
        return outputs, tmpx, normx


def _handle_owners(enc):
    """the modules of a TrainableHGFilter / TrainableHourglass / TrainableConvBlock / TrainableStem / TrainableStackTail that own packed forward handles"""
    if isinstance(enc, TrainableHGFilter):
        return [enc.stem] + list(enc.blocks.values()) + [b for hg in enc.hourglasses for b in hg.blocks.values()] + list(enc.tails)
    if isinstance(enc, TrainableHourglass):
        return list(enc.blocks.values())
    if isinstance(enc, _PackedHandles):
        return [enc]
    raise TypeError(f"no trainable encoder module: {type(enc).__name__}")


def invalidate_handles(enc):
    """``enc``'s leaves were written behind their version counters (a kernel writing through ``data_ptr()``, as ``ops.FusedAdam`` does): every packed forward
    handle is repacked at its next use"""
    for o in _handle_owners(enc):
        o.invalidate_handles()


class EncoderAdam:
    """Adam (``torch.optim.Adam`` semantics, the arithmetic of ``ops.FusedAdam`` element for element) for a ``TrainableHGFilter``, ``TrainableHourglass`` or
    ``TrainableConvBlock``, with the whole step on the device:

        opt = EncoderAdam(enc, lr=1e-4)
        outputs, _, _ = enc(images); loss(outputs).backward()
        opt.step(); opt.zero_grad()

    * every parameter's ``.data`` is re-homed into ONE flat fp32 buffer (``flat``; each leaf keeps its identity, shape and values, at a 256-byte aligned offset)
      and its ``.grad`` is bound to a view of one flat gradient buffer (``grad``), into which autograd accumulates in place; ``zero_grad()`` is one memset;
    * ``m`` and ``v`` are flat too, so ``step()`` is ONE ``vt_adam_step`` launch over everything,
    * followed by ONE repack plan (``vt_repack_plan_run``: two launches) over all packed forward handles of the module, which are then marked current so that the
      version check of the next forward does nothing: ``launches_per_step`` = 3 launches and no host wait, whatever the size of the network.

    A leaf whose ``.grad`` was replaced since (set to None and refilled by autograd, or rebound) has its gradient copied into the flat buffer by ``step()`` and
    is bound again; a leaf WITHOUT a gradient at ``step()`` is skipped as torch and ``ops.FusedAdam`` skip it: its value and its moments are put back after the
    flat launch (three small copies either side, only when it happens) and its ``.grad`` stays None.  ``state_dict()`` of the module is unchanged.  The plan captures
    the leaves' addresses: assigning a leaf's ``.data`` afterwards, or putting another tensor in a module's ``leaves``, is an error ``step()`` reports.  Needs the
    device-side packing (not ``VT_ENCODER_HOST_REPACK``)."""

    def __init__(self, enc, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        import ctypes as C
        self.enc, self.lr, self.betas, self.eps, self.t = enc, float(lr), (float(betas[0]), float(betas[1])), float(eps), 0
        self.device = enc.device
        self.owners = _handle_owners(enc)
        if any(o.host_repack for o in self.owners):
            raise L.VtError("EncoderAdam repacks on the device: it cannot drive handles kept on the host path (VT_ENCODER_HOST_REPACK / host_repack)")
        self.params = list({id(p): p for p in enc.parameters()}.values())
        if not self.params or any(not (p.is_cuda and p.dtype == torch.float32 and p.is_leaf) for p in self.params):
            raise L.VtError("EncoderAdam: the parameters must be fp32 device leaves")
        offs, total = [], 0
        for p in self.params:
            offs.append(total)
            total += (p.numel() + 63) // 64 * 64
        self.n, self._offs = total, offs
        with torch.cuda.device(self.device):
            self.flat = torch.zeros(total, device=self.device)
            self.grad = torch.zeros(total, device=self.device)
            self.m = torch.zeros(total, device=self.device)
            self.v = torch.zeros(total, device=self.device)
            self._pviews, self._gviews = [], []
            for p, o in zip(self.params, offs):
                pv, gv = self.flat[o:o + p.numel()].view(p.shape), self.grad[o:o + p.numel()].view(p.shape)
                pv.copy_(p.detach())
                if p.grad is not None:
                    gv.copy_(p.grad)
                p.data = pv
                p.grad = gv
                self._pviews.append(pv); self._gviews.append(gv)
            # every handle packed from the re-homed leaves, then one plan over all of them
            ents = []
            for o in self.owners:
                o.invalidate_handles()
                o.handles(self.device)
                ents += list(o._handles.values())
            n = len(ents)
            kinds = (C.c_int * n)(*[e.kind for e in ents])
            handles = (C.c_void_p * n)(*[e.handle.value for e in ents])
            weights = (C.c_void_p * n)(*[L.dptr(e.weight.detach()) for e in ents])
            biases = (C.c_void_p * n)(*[L.dptr(e.bias.detach()) if e.bias is not None else None for e in ents])
            self._plan = C.c_void_p()
            L.check(L.lib().vt_repack_plan_create(C.byref(self._plan), n, kinds, handles, weights, biases))
        self.n_handles, self._planned = n, [(e, e.weight, e.bias) for e in ents]
        self.launches_per_step = 1 + int(L.lib().vt_repack_plan_launches(self._plan))

    def __del__(self):
        try:
            if getattr(self, "_plan", None):
                L.lib().vt_repack_plan_destroy(self._plan)
        except Exception:
            pass

    def _bind_grads(self, copy):
        """bind every leaf's ``.grad`` to its view of the flat buffer; with ``copy`` a replaced gradient is copied in first and a leaf without one is left alone
        -> the indices of those leaves"""
        absent = []
        for i, (p, gv) in enumerate(zip(self.params, self._gviews)):
            g = p.grad
            if g is gv or (g is not None and g.data_ptr() == gv.data_ptr() and g.shape == gv.shape and g.is_contiguous()):
                continue
            if copy:
                if g is None:
                    absent.append(i)
                    continue
                gv.copy_(g)
            p.grad = gv
        return absent

    def zero_grad(self):
        """one memset of the flat gradient buffer (and a leaf whose ``.grad`` was replaced is bound to its view again)"""
        self.grad.zero_()
        self._bind_grads(copy=False)

    def step(self, skip=None):
        """``skip``: a device int32 tensor of one value (``ops.StepGuard.close``), the stop flag of the Adam launch of this step: when it is set, ``flat``, ``m`` and
        ``v`` are left untouched.  ``t`` advances all the same (the host cannot know the outcome without waiting: a skipped step costs one step of bias
        correction) and the repack plan still runs: it packs the unchanged weights to the same bytes."""
        for p, pv in zip(self.params, self._pviews):
            if p.data_ptr() != pv.data_ptr():
                raise L.VtError("EncoderAdam.step: a parameter's .data was replaced since the optimiser was built; the flat buffer and the repack plan still point at the old storage")
        for e, w, b in self._planned:
            if e.weight is not w or e.bias is not b:
                raise L.VtError("EncoderAdam.step: a leaf of the module was replaced by another tensor since the optimiser was built; the repack plan still reads the old one")
        absent = self._bind_grads(copy=True)
        self.t += 1
        with torch.cuda.device(self.device):
            # a leaf without a gradient is skipped: whatever the flat launch does to its slice (the gradient slice may hold anything, a NaN included) is undone
            keep = []
            for i in absent:
                sl = slice(self._offs[i], self._offs[i] + self.params[i].numel())
                keep.append((sl, self.flat[sl].clone(), self.m[sl].clone(), self.v[sl].clone()))
            L.check(L.lib().vt_adam_step(L.dptr(self.flat), L.dptr(self.grad), L.dptr(self.m), L.dptr(self.v), self.n, self.t, self.lr, self.betas[0], self.betas[1],
                                         self.eps, L.dptr(skip), L.stream_ptr()))
            for sl, p0, m0, v0 in keep:
                self.flat[sl].copy_(p0); self.m[sl].copy_(m0); self.v[sl].copy_(v0)
            L.check(L.lib().vt_repack_plan_run(self._plan, L.stream_ptr()))
        for o in self.owners:
            o._mark_handles_current()


class SIFNetEncoder:
    """``CHORETriplane.filter`` (chore_triplane.py:60-95): image encoder on channels 0..4, the (shared or per-view) triplane encoder on
    channels 5, 6, 7; returns the eight feature maps of the query as an ``ops.FeatureMaps`` (NHWC, resident on the device)."""

    def __init__(self, sd: dict, num_stack=3, num_hourglass=2, triplane_stack=3, shared_encoder=True, device="cuda:0"):
        self.device = device
        self.image = HGFilterEncoder(sd, "image_filter.", num_stack, num_hourglass, device=device)
        if shared_encoder:
            t = HGFilterEncoder(sd, "triplane_encoder.", triplane_stack, num_hourglass, device=device)
            self.tri = [t, t, t]
        else:
            self.tri = [HGFilterEncoder(sd, f"triplane_encoder_{x}.", triplane_stack, num_hourglass, device=device) for x in range(3)]

    @classmethod
    def from_state_dict(cls, sd, **kw):
        return cls(sd, shared_encoder=bool(state_dict_under(sd, "triplane_encoder.")), **kw)

    def route_report(self):
        """convolution routes taken since construction, summed over the image and triplane encoders: {'hip7x7': n, 'hip3x3': n, 'hip1x1': n, 'miopen:<layer>': n}
        (under a captured HIP graph only the capture pass counts)"""
        import collections
        c = collections.Counter()
        for e in {id(e): e for e in [self.image] + list(self.tri)}.values():
            c.update(e.routes)
        return dict(c)

    chunk = 16      # frames per encoder pass
    _full_chunk_seen = False

    @torch.no_grad()
    def __call__(self, images, out=None):
        """``out``: optional dict of preallocated NHWC tensors (B,H,W,C) per map name to write into (e.g. slices of whole-sequence buffers).
        The batch is encoded ``chunk`` frames at a time (every op of the encoder is per-frame, so the result does not depend on the split;
        the last chunk is zero-padded): ONE set of convolution shapes for MIOpen to pick kernels for whatever the batch size, and
        activation memory bounded by the chunk, while the outputs land in maps preallocated for the whole batch."""
        assert images.shape[1] == 8, f"given image shape invalid: {images.shape}"
        images = images.to(self.device).float()
        B = images.shape[0]
        for s0 in range(0, B, self.chunk):
            x = images[s0:s0 + self.chunk]; n = x.shape[0]
            if n < self.chunk and (B > self.chunk or self._full_chunk_seen):     # reuse the shapes MIOpen already has kernels for
                x = torch.cat([x, torch.zeros(self.chunk - n, *x.shape[1:], device=x.device)], 0)
            self._full_chunk_seen = self._full_chunk_seen or x.shape[0] == self.chunk
            graph_done = None
            if self.use_graph and x.is_cuda and x.shape[0] == self.chunk:
                maps, graph_done = self._chunk_graph(x)
            else:
                maps = self._chunk_eager(x)
            try:
                if out is None:
                    # channels-last NCHW tensors are NHWC in memory: the permuted views are what the query kernel gathers from; written per chunk.
                    # (Inside the try: _chunk_graph returned with the graph lock HELD, an allocation failure here must release it -- ADVICE r05.)
                    out = {k: torch.empty(B, m.shape[2], m.shape[3], m.shape[1], device=m.device) for k, m in maps.items()}
                for k, m in maps.items():
                    out[k][s0:s0 + n] = m[:n].permute(0, 2, 3, 1)
            finally:
                if graph_done is not None:
                    graph_done()
        return ops.FeatureMaps(out)

    def _chunk_eager(self, x):
        """one chunk of frames through both encoders -> the eight maps as channels-last NCHW tensors"""
        feats, tmpx, _ = self.image(x[:, :5])
        maps = {"im_feat": feats[-1], "tmpx": tmpx}
        if self.tri[0] is self.tri[1] and self.tri[1] is self.tri[2]:
            # shared triplane encoder (chore_triplane.py:60-95 applies the same module to the three renders): ONE pass over the 3 x chunk
            # single-channel images instead of three -- every op of the encoder is per frame, so the maps are the same; the launches are
            # three times larger (the 16-frame ones leave the chip half empty at the 1/4- and 1/8-resolution levels of the hourglass)
            nb = x.shape[0]
            f, t, _ = self.tri[0](x[:, 5:8].transpose(0, 1).reshape(3 * nb, 1, *x.shape[2:]))
            for v in range(3):
                maps[f"tri_tmpx{v}"] = t[v * nb:(v + 1) * nb]; maps[f"tri_feat{v}"] = f[-1][v * nb:(v + 1) * nb]
        else:
            for v in range(3):
                f, t, _ = self.tri[v](x[:, 5 + v:6 + v])
                maps[f"tri_tmpx{v}"] = t; maps[f"tri_feat{v}"] = f[-1]
        return maps

    # A full chunk is ~650 launches (two stacked hourglasses of fused ConvBlocks) issued from Python; in the pipeline's SIF-Net pass they come from a
    # second host thread while the first one drives the surface-point generator's rounds (two host round trips each), and the two contend for the
    # interpreter.  The chunk is therefore captured ONCE as a HIP graph (fixed shape: ``chunk`` frames) and replayed: one launch call per chunk, the
    # same kernels on the same data (bit-identical maps).  The static input / output buffers are shared by all callers: a lock serialises the hosts,
    # an event orders a replay behind the previous caller's copies out of the static outputs.  VT_ENCODER_GRAPH=0: eager.
    use_graph = os.environ.get("VT_ENCODER_GRAPH", "1") != "0"
    _graph = None

    def _graph_key(self):
        return (self.__dict__.get("_graph_epoch", 0),) + tuple(bool(e.use_hip_conv) for e in [self.image] + list(self.tri))

    def invalidate_graph(self):
        """call after changing weights (the state dict the encoders were built from) or any switch the captured pass depends on"""
        self._graph_epoch = self.__dict__.get("_graph_epoch", 0) + 1

    def _chunk_graph(self, x):
        import threading
        lock = self.__dict__.setdefault("_graph_lock", threading.Lock())
        lock.acquire(); held = True
        try:
            ent = self._graph
            # a captured graph keeps its kernels and their arguments: a switch of the convolution route (HGFilterEncoder.use_hip_conv, the tests toggle it)
            # or a call of invalidate_graph() after a weight reload must not be served by a stale replay
            key = self._graph_key()
            if ent not in (None, False) and ent[4] != key:
                ent = None
            if ent is None:
                try:
                    sx = x.clone()
                    side = torch.cuda.Stream(device=x.device); side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):
                        self._chunk_eager(sx)              # outside the capture: the handles' creation (an allocation each), MIOpen's kernel choice for the stem, workspaces
                    torch.cuda.current_stream().wait_stream(side)
                    torch.cuda.synchronize(x.device)
                    g = torch.cuda.CUDAGraph()
                    # (thread_local: another host thread -- the pipeline's generator or a second fit stream -- may allocate or synchronise meanwhile)
                    with torch.cuda.graph(g, capture_error_mode="thread_local"):
                        so = self._chunk_eager(sx)
                    ent = (g, sx, so, torch.cuda.Event(), key)
                    ent[3].record()
                except Exception as e:                      # noqa: BLE001 -- something in the pass cannot be captured on this build: stay eager, say so once
                    import warnings
                    warnings.warn(f"SIFNetEncoder: HIP-graph capture of the encoder pass failed ({type(e).__name__}: {e}); running it eagerly")
                    ent = False
                self._graph = ent
            if ent is False or ent[1].shape != x.shape:
                lock.release(); held = False                # the eager pass runs OUTSIDE the lock (and outside this handler's release)
                return self._chunk_eager(x), None
            g, sx, so, ev = ent[:4]
            cur = torch.cuda.current_stream()
            cur.wait_event(ev)                              # the previous caller has copied the static outputs out
            sx.copy_(x)
            g.replay()

            def done():
                ev.record(); lock.release()
            return so, done
        except BaseException:
            if held:
                lock.release()
            raise
