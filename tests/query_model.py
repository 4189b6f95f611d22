"""Float64 model of the SIF-Net point query (include/vistracker.h "SIF-Net point query"), written in numpy from the definition: CHORETriplane.query
(model/chore_triplane.py:97-164), get_zfeat / triplane_project (:207-251), KinectColorCamera.project_screen / normalize (model/camera.py:52-90), grid_sample
bilinear / align_corners=True / zero padding (model/geometry.py:4-14), the five Conv1d decoders 611-128-128-128-k with ReLU (model/chore.py:113-126) and the
sigmoid on the visibility (model/chore_tri_vis.py:17-28).  The backward is the derivative written out, no autograd.  It imports nothing from vistracker_amd or
oracle/.

Besides every output the model returns, per point and per output,
  S       the output's OWN SCALE: the same forward / backward with |W|, |b|, |feature|, |tap difference| and |upstream gradient| -- every term that produces the
          output, without cancellation.  Errors are expressed in units of u S, u = 2^-24.
  margins the point's KINK MARGINS: the distance of every branch quantity from its branch in units of u times that quantity's own S -- hidden pre-activations
          from 0 (`relu`, already divided by KINK_RELU of the layer), the 16 grid coordinates from an integer texel coordinate and nx / ny from +-1 (`coord`), the
          clamped df from its threshold (`clamp`).  excluded() names the points that may take the other branch in float32: the value is continuous there, the
          gradient is not.
Mutants (one deliberate defect each, `mutant=` of QueryModel) serve tests/test_host_query_model.py."""
import numpy as np

U = 2.0 ** -24
GATE = 8                       # the project's margin between two correct float32 evaluation orders (tests/test_gpu_smplh_perjoint.py)
# A branch quantity within KINK u S of its branch may take the other branch in float32 (units of u times the quantity's own S):
KINK_COORD = 8.0               # nx, ny and the 16 texel coordinates: at most 8 float32 roundings from the point to the texel coordinate (x fx, / z, + cx, + crop / 2, - centre,
                               # x 2 / crop, - 1; + 1, x (W - 1) / 2 -- the products with 2 and 1 / 2 are exact), each at most u of the coordinate's own scale
KINK_RELU = (18.0, 1.6, 0.13)  # hidden pre-activations of layers 1, 2, 3.  The worst case of a 611-term float32 sum is 611 u S, which would put every point within reach of a kink and
                               # make the 2 % cap on exclusions unreachable; what float32 and split-operand arithmetic really move a pre-activation by is measured on the CPU (float32
                               # and split emulation, emu_decoder, against this model: the worst unit of every case is 2.1, 0.19, 0.015 u S at layers 1, 2, 3 -- S grows by |W| per
                               # layer, the realised error does not; tests/test_host_query_model.py asserts it, tests/golden/query_perpoint.md records it).  KINK_RELU = GATE x that.
SPLIT = 3 * 2.0 ** -22         # per product: two operands carried to 22 bits + the dropped lo x lo product (tests/encoder_model.py)
OUT_DIST = 5.0
HEADS = ("df", "pca", "parts", "centers", "vis")
HEAD_DIMS = (2, 9, 14, 3, 1)
MAP_ORDER = ("im_feat", "tmpx", "tri_tmpx0", "tri_tmpx1", "tri_tmpx2", "tri_feat0", "tri_feat1", "tri_feat2")
MAP_PROJ = (0, 0, 1, 2, 3, 1, 2, 3)                       # 0 perspective, 1 right, 2 back, 3 top
CHAN_OFF = (0, 259, 323, 355, 387, 419, 483, 547)         # im_feat | x y z-2.2 | tmpx | tri_tmpx x 3 | tri_feat x 3  (chore_triplane.py:139-151)
DEFAULT_CAM = (979.7844, 979.840, 1018.952, 779.486, 1200.0)
THR_HUMAN = float(np.float32(0.1))                       # torch.clamp(max=0.1) of a float32 tensor compares with float32(0.1)
THR_OBJECT = float(np.float32(0.8))

MUTANTS = ("swap_wx", "chan_shift", "relu_other_head", "tile_63_64", "flush_small_go", "df_mask_leak", "no_sigmoid_deriv", "order_write")


def sigmoid(v):
    with np.errstate(over="ignore"):
        return 1 / (1 + np.exp(-v))


def _dist_to_integer(v):
    d = np.abs(v - np.round(v))
    return np.where(d == 0, np.inf, d)          # exactly ON a texel: a placed coordinate, exact in float32 too (the host test checks the cell on the float32 oracle)


class QueryModel:
    def __init__(self, decoders, maps, cam=DEFAULT_CAM, mutant=None, mutant_map=5):
        self.W = [[np.asarray(w, np.float64) for w, _ in decoders[h]] for h in HEADS]
        self.b = [[np.asarray(b, np.float64) for _, b in decoders[h]] for h in HEADS]
        self.maps = [np.asarray(maps[k], np.float64) for k in MAP_ORDER]
        self.cam = [float(np.float32(c)) for c in cam]
        assert mutant is None or mutant in MUTANTS
        self.mutant, self.mutant_map = mutant, mutant_map
        if mutant == "chan_shift":
            self.maps[mutant_map] = np.roll(self.maps[mutant_map], 1, axis=1)

    # ---- projections -------------------------------------------------------------------------------------------------------------------------------------
    def geometry(self, pts, cc, bc):
        """-> uv (B, N, 4, 2), J = d uv / d xyz (B, N, 4, 2, 3), in_img (B, N), border: distance of nx, ny from +-1 over u times their own scale"""
        p = np.asarray(pts, np.float64); cc = np.asarray(cc, np.float64)[:, None]; bc = np.asarray(bc, np.float64)[:, None]
        fx, fy, cx, cy, crop = self.cam
        x, y, z = p[..., 0], p[..., 1], p[..., 2]
        nx = 2 * (crop / 2 + (fx * x / z + cx) - cc[..., 0]) / crop - 1
        ny = 2 * (crop / 2 + (fy * y / z + cy) - cc[..., 1]) / crop - 1
        s_nx = 2 * (crop / 2 + np.abs(fx * x / z) + abs(cx) + np.abs(cc[..., 0])) / crop + 1
        s_ny = 2 * (crop / 2 + np.abs(fy * y / z) + abs(cy) + np.abs(cc[..., 1])) / crop + 1
        c = p - bc
        uv = np.stack([np.stack([nx, ny], -1), np.stack([c[..., 2], c[..., 1]], -1), np.stack([-c[..., 0], c[..., 1]], -1),
                       np.stack([c[..., 0], -c[..., 2]], -1)], 2)
        s_uv = np.stack([np.stack([s_nx, s_ny], -1)] + [np.abs(p[..., [i, j]]) + np.abs(bc[..., [i, j]]) for i, j in ((2, 1), (0, 1), (0, 2))], 2)
        J = np.zeros(p.shape[:2] + (4, 2, 3))
        kx, ky = 2 / crop * fx, 2 / crop * fy
        J[..., 0, 0, 0] = kx / z; J[..., 0, 0, 2] = -kx * x / z ** 2
        J[..., 0, 1, 1] = ky / z; J[..., 0, 1, 2] = -ky * y / z ** 2
        J[..., 1, 0, 2] = 1; J[..., 1, 1, 1] = 1
        J[..., 2, 0, 0] = -1; J[..., 2, 1, 1] = 1
        J[..., 3, 0, 0] = 1; J[..., 3, 1, 2] = -1
        in_img = (nx >= -1) & (nx <= 1) & (ny >= -1) & (ny <= 1)
        bd = np.minimum(np.abs(np.abs(nx) - 1) / s_nx, np.abs(np.abs(ny) - 1) / s_ny)
        return dict(uv=uv, s_uv=s_uv, J=J, in_img=in_img, border=np.where(bd == 0, np.inf, bd) / U, p=p)

    # ---- the 611 features and their derivatives to the grid coordinates -------------------------------------------------------------------------------
    def features(self, geo):
        p = geo["p"]; B, N = p.shape[:2]
        feat, afeat, gu, gv, agu, agv = (np.zeros((B, N, 611)) for _ in range(6))
        feat[..., 256:259] = p - [0, 0, 2.2]; afeat[..., 256:259] = np.abs(p) + [0, 0, 2.2]
        tex = np.full((B, N), np.inf)
        for mi, m in enumerate(self.maps):
            C, H, W = m.shape[1:]; pr = MAP_PROJ[mi]; lo = CHAN_OFF[mi]
            u, v = geo["uv"][..., pr, 0], geo["uv"][..., pr, 1]
            ix, iy = (u + 1) * 0.5 * (W - 1), (v + 1) * 0.5 * (H - 1)
            six, siy = (geo["s_uv"][..., pr, 0] + 1) * 0.5 * (W - 1), (geo["s_uv"][..., pr, 1] + 1) * 0.5 * (H - 1)
            tex = np.minimum(tex, np.minimum(_dist_to_integer(ix) / six, _dist_to_integer(iy) / siy))
            x0 = np.floor(ix).astype(np.int64); y0 = np.floor(iy).astype(np.int64)
            wx1, wy1 = ix - x0, iy - y0; wx0, wy0 = 1 - wx1, 1 - wy1
            if self.mutant == "swap_wx" and mi == self.mutant_map:
                wx0, wx1 = wx1, wx0
            bi = np.arange(B)[:, None]

            def tap(xx, yy):
                ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
                val = m[bi, :, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]          # (B, N, C)
                return val * ok[..., None]
            nw, ne, sw, se = tap(x0, y0), tap(x0 + 1, y0), tap(x0, y0 + 1), tap(x0 + 1, y0 + 1)
            e = lambda a: a[..., None]
            sl = slice(lo, lo + C)
            feat[..., sl] = nw * e(wx0 * wy0) + ne * e(wx1 * wy0) + sw * e(wx0 * wy1) + se * e(wx1 * wy1)
            afeat[..., sl] = np.abs(nw) * e(wx0 * wy0) + np.abs(ne) * e(wx1 * wy0) + np.abs(sw) * e(wx0 * wy1) + np.abs(se) * e(wx1 * wy1)
            sx, sy = 0.5 * (W - 1), 0.5 * (H - 1)
            gu[..., sl] = ((ne - nw) * e(wy0) + (se - sw) * e(wy1)) * sx; agu[..., sl] = (np.abs(ne - nw) * e(wy0) + np.abs(se - sw) * e(wy1)) * sx
            gv[..., sl] = ((sw - nw) * e(wx0) + (se - ne) * e(wx1)) * sy; agv[..., sl] = (np.abs(sw - nw) * e(wx0) + np.abs(se - ne) * e(wx1)) * sy
        return dict(feat=feat, afeat=afeat, gu=gu, gv=gv, agu=agu, agv=agv, texel=tex / U)

    # ---- decoders -----------------------------------------------------------------------------------------------------------------------------------------
    def mlp(self, h, ft):
        """-> pre (3 hidden pre-activations), S (their own scales, and the output's as S[3]), out (B, N, k), relu: min |pre| / (u S KINK_RELU[layer]) over the 384 units (< 1: within float32 reach of the kink)"""
        a, s = ft["feat"], ft["afeat"]; pre, S = [], []
        relu = np.full(a.shape[:2], np.inf)
        for l in range(3):
            z = a @ self.W[h][l].T + self.b[h][l]; s = s @ np.abs(self.W[h][l]).T + np.abs(self.b[h][l])
            pre.append(z); S.append(s); relu = np.minimum(relu, (np.abs(z) / s).min(-1) / (U * KINK_RELU[l]))
            a = np.maximum(z, 0)
        out = a @ self.W[h][3].T + self.b[h][3]; S.append(s @ np.abs(self.W[h][3]).T + np.abs(self.b[h][3]))
        return dict(pre=pre, S=S, out=out, relu=relu)

    def forward(self, pts, cc, bc, heads=range(5)):
        """-> r[name] (B, k, N) values, r['S_' + name] their own scales, r['margin'] (B, N) over the heads asked for, r['in_img'], and the parts for backward"""
        geo = self.geometry(pts, cc, bc); ft = self.features(geo)
        r = dict(geo=geo, ft=ft, in_img=geo["in_img"], mlp={})
        coord = np.minimum(geo["border"], ft["texel"]); relu = np.full(coord.shape, np.inf)
        for h in heads:
            m = self.mlp(h, ft); r["mlp"][h] = m
            val, S = m["out"].copy(), m["S"][3].copy()
            if h == 0:
                val[~geo["in_img"]] = OUT_DIST; S[~geo["in_img"]] = 0.0                      # a constant: no rounding at all
            if h == 4:
                sg = sigmoid(val); S = S * sg * (1 - sg) + sg; val = sg            # the logit's scale through the sigmoid's slope + one u of the result
            r[HEADS[h]] = val.transpose(0, 2, 1); r["S_" + HEADS[h]] = S.transpose(0, 2, 1)
            relu = np.minimum(relu, m["relu"])
        r["margins"] = dict(coord=coord, relu=relu)
        return r

    def backward(self, fw, gouts, agouts=None):
        """gouts {head index: (B, k, N) upstream gradient}, agouts: the gradients' own scales where they are computed quantities (default |gouts|).
        -> dpts (B, N, 3), S (B, N, 3)"""
        geo, ft = fw["geo"], fw["ft"]; B, N = geo["in_img"].shape
        dfeat, adfeat = np.zeros((B, N, 611)), np.zeros((B, N, 611))
        hs = sorted(gouts)
        for h in hs:
            m = fw["mlp"][h]
            go = np.asarray(gouts[h], np.float64).transpose(0, 2, 1).copy()
            ago = np.abs(go) if agouts is None or h not in agouts else np.asarray(agouts[h], np.float64).transpose(0, 2, 1).copy()
            if self.mutant == "flush_small_go":
                for t in range(0, N, 64):
                    big = np.abs(go[:, t:t + 64]).max((1, 2), keepdims=True)
                    go[:, t:t + 64] *= np.abs(go[:, t:t + 64]) >= big * 2.0 ** -12
            if h == 0 and self.mutant != "df_mask_leak":
                go[~geo["in_img"]] = 0; ago[~geo["in_img"]] = 0                              # the masked write kills the gradient
            if h == 4 and self.mutant != "no_sigmoid_deriv":
                sg = sigmoid(m["out"]); go = go * sg * (1 - sg)
                ago = ago * (sg * (1 - sg) + np.abs(sg * (1 - sg) * (1 - 2 * sg)) * m["S"][3])      # the slope, and what the logit's own error moves the slope by
            g, ag = go @ self.W[h][3], ago @ np.abs(self.W[h][3])
            for l in (2, 1, 0):
                pre = m["pre"][l]
                if self.mutant == "relu_other_head" and l == 1 and len(hs) == 2:
                    pre = fw["mlp"][hs[1 - hs.index(h)]]["pre"][l]
                g = g * (pre > 0); ag = ag * (pre > 0)
                g, ag = g @ self.W[h][l], ag @ np.abs(self.W[h][l])
            dfeat += g; adfeat += ag
        d, ad = self.to_points(fw, dfeat, adfeat)
        if self.mutant == "tile_63_64" and N > 64:
            d[:, [63, 64]] = d[:, [64, 63]]
        return d, ad

    def to_points(self, fw, dfeat, adfeat):
        """d feat (B, N, 611) and its own scale -> dpts, S: the features' derivatives to the grid coordinates and the projections' Jacobians"""
        geo, ft = fw["geo"], fw["ft"]
        d, ad = dfeat[..., 256:259].copy(), adfeat[..., 256:259].copy()
        J = geo["J"]
        for mi, m in enumerate(self.maps):
            sl = slice(CHAN_OFF[mi], CHAN_OFF[mi] + m.shape[1]); pr = MAP_PROJ[mi]
            du, dv = (dfeat[..., sl] * ft["gu"][..., sl]).sum(-1), (dfeat[..., sl] * ft["gv"][..., sl]).sum(-1)
            adu, adv = (adfeat[..., sl] * ft["agu"][..., sl]).sum(-1), (adfeat[..., sl] * ft["agv"][..., sl]).sum(-1)
            d += du[..., None] * J[..., pr, 0, :] + dv[..., None] * J[..., pr, 1, :]
            ad += adu[..., None] * np.abs(J[..., pr, 0, :]) + adv[..., None] * np.abs(J[..., pr, 1, :])
        return d, ad

    def apply_order_mutant(self, d, order):
        """`order` applied to the input read but not to the dpts write: slot n holds the gradient of point order[n]"""
        return d[:, np.asarray(order)] if (self.mutant == "order_write" and order is not None) else d

    # ---- fused objectives ---------------------------------------------------------------------------------------------------------------------------------
    def clamp_head(self, fw, col, thr):
        """-> d (B, N) the distance (5.0 outside the image), live (B, N): in the image and d <= thr, margin (B, N) of d from thr in units of u S"""
        d = fw["df"][:, col]; S = fw["S_df"][:, col]
        mg = np.where(fw["in_img"], np.abs(d - thr) / np.where(S > 0, S, 1.0), np.inf) / U
        return d, fw["in_img"] & (d <= thr), mg

    def human_loss(self, pts, cc, bc, labels, w_dfh, w_part):
        """vt_query_human_loss: terms (df_h = mean_{B,N} clamp(df[:, 0], max = .1), part = mean_B sum_N CE(parts, labels)), dpts of w_dfh df_h + w_part part"""
        fw = self.forward(pts, cc, bc, heads=(0, 2)); B, N = fw["in_img"].shape
        d, live, mg = self.clamp_head(fw, 0, THR_HUMAN)
        g_df = np.zeros((B, 2, N)); g_df[:, 0] = live * (w_dfh / (B * N))
        lg = fw["parts"]; mx = lg.max(1, keepdims=True); lse = np.log(np.exp(lg - mx).sum(1)) + mx[:, 0]
        lab = np.broadcast_to(np.asarray(labels)[None], (B, N)); pick = np.take_along_axis(lg, lab[:, None], 1)[:, 0]
        ce = lse - pick
        sm = np.exp(lg - lse[:, None]); oh = np.zeros_like(sm); np.put_along_axis(oh, lab[:, None], 1.0, 1)
        g_parts, ag_parts = (sm - oh) * (w_part / B), (sm + oh) * (w_part / B)
        dp, S = self.backward(fw, {0: g_df, 2: g_parts}, {2: ag_parts})
        s_ce = np.take_along_axis(fw["S_parts"], lab[:, None], 1)[:, 0] + fw["S_parts"].max(1)          # the picked logit's and the log-sum-exp's (<= the largest logit's)
        return dict(terms=np.array([np.minimum(d, THR_HUMAN).mean(), ce.sum(1).mean()]), dpts=dp, S=S, margins=dict(fw["margins"], clamp=mg), fw=fw,
                    summands=(np.minimum(d, THR_HUMAN) / (B * N), ce / B), s_summands=(fw["S_df"][:, 0] / (B * N), s_ce / B), live=live)

    def object_loss(self, pts, cc, bc, occ, w_obj):
        """vt_query_object_loss: term mean_B(mean_N clamp(df[:, 1], max = .8) occ[b]), dpts of w_obj term"""
        fw = self.forward(pts, cc, bc, heads=(0,)); B, N = fw["in_img"].shape; occ = np.asarray(occ, np.float64)[:, None]
        d, live, mg = self.clamp_head(fw, 1, THR_OBJECT)
        g_df = np.zeros((B, 2, N)); g_df[:, 1] = live * occ * (w_obj / (B * N))
        dp, S = self.backward(fw, {0: g_df})
        sm = np.minimum(d, THR_OBJECT) * occ / (B * N)
        return dict(terms=np.array([sm.sum()]), dpts=dp, S=S, margins=dict(fw["margins"], clamp=mg), fw=fw, summands=(sm,),
                    s_summands=(fw["S_df"][:, 1] * occ / (B * N),), live=live)

    def project_step(self, pts, cc, bc, df_idx, thr):
        """one step of Generator.approx_surface (recon/gen/generator.py:72-103): p - normalize(d sum(target) / dp) target, target = clamp(df[:, idx], max = thr)"""
        fw = self.forward(pts, cc, bc, heads=(0,)); B, N = fw["in_img"].shape
        d, live, mg = self.clamp_head(fw, df_idx, thr)
        tgt = np.minimum(d, thr); s_tgt = np.where(d <= thr, fw["S_df"][:, df_idx], 0.0)
        g_df = np.zeros((B, 2, N)); g_df[:, df_idx] = live
        g, Sg = self.backward(fw, {0: g_df})
        nrm = np.maximum(np.sqrt((g ** 2).sum(-1, keepdims=True)), 1e-12); gh = g / nrm
        out = fw["geo"]["p"] - gh * tgt[..., None]
        # d normalize(g)_i / d g_j = (delta_ij - gh_i gh_j) / |g|
        s_gh = (Sg + np.abs(gh) * (np.abs(gh) * Sg).sum(-1, keepdims=True)) / nrm
        S = np.abs(fw["geo"]["p"]) + np.abs(gh) * s_tgt[..., None] + np.abs(tgt)[..., None] * s_gh + np.abs(gh * tgt[..., None])
        return dict(out=out, S=S, target=tgt, S_target=s_tgt, dpts=g, S_dpts=Sg, margins=dict(fw["margins"], clamp=mg), fw=fw, live=live)


def accel(v, w):
    """vt_accel_loss(v (B, D), gscale = w): term mean((v[1:-1] - v[:-2] - (v[2:] - v[1:-1]))^2) (recon_fit_trivis_full.py:170-177), w d term / dv and its own scale"""
    v = np.asarray(v, np.float64); B, D = v.shape
    a = 2 * v[1:-1] - v[:-2] - v[2:]; aa = 2 * np.abs(v[1:-1]) + np.abs(v[:-2]) + np.abs(v[2:])
    k = 2.0 * w / ((B - 2) * D)
    g, S = np.zeros_like(v), np.zeros_like(v)
    g[1:-1] += 2 * k * a; g[:-2] -= k * a; g[2:] -= k * a
    S[1:-1] += 2 * k * aa; S[:-2] += k * aa; S[2:] += k * aa
    return (a ** 2).mean(), g, S, (aa ** 2).mean()        # the last: the term's own scale (every rounding of a and of a^2 is relative to aa^2)


# ---- the number format of the split-f16 decoders ---------------------------------------------------------------------------------------------------------
def split22(v):
    """a float32 array rounded to what a float16 hi + float16 lo pair carries at the kernel's operand scales (no float16 under- or overflow: the scales are
    powers of two chosen for that): hi = 11 significant bits, lo = the next 11 -> 22 bits"""
    v = np.asarray(v, np.float32); m, e = np.frexp(v.astype(np.float64))
    hi = np.ldexp(np.round(np.ldexp(m, 11)), e - 11); r = v - hi; m2, e2 = np.frexp(r)
    return (hi + np.ldexp(np.round(np.ldexp(m2, 11)), e2 - 11)).astype(np.float32)


def operand_scales(decoders, head, level=0):
    """the power-of-two scales the split-f16 kernels carry the forward operands of one head at (csrc/query.hip, vt_sifnet_create; restated in
    tests/test_gpu_parity.py::test_query_fused_objectives_vs_oracle): s_l = 2^max(e_l, 0) lifts max |W_l| into [1, 2) (never below 1); the feature scale U_1 is common to
    the heads and keeps every head's U_4 = s_1 s_2 s_3 U_1 <= 2^6; a range level divides all of them by 16.  -> [U_1, U_2, U_3, U_4], the scale of layer l's input"""
    sexp = lambda w: max(1 - int(np.frexp(np.abs(np.asarray(w)).max())[1]), 0)
    u = 2.0 ** (min(6 - sum(sexp(decoders[h][l][0]) for l in range(3)) for h in HEADS) - 4 * level); out = [u]
    for l in range(3):
        u *= 2.0 ** sexp(decoders[head][l][0]); out.append(u)
    return out


def emu_decoder(W, b, feat, go=None, split=True, scales=None):
    """An emulation of the decoders' NUMBER FORMAT, not of the kernel's code: every GEMM operand (weights, features, activations, gradients) carried to 22 bits
    (split=True) or as float32 (split=False), products and sums in float32 (numpy's float32 matmul), bias and ReLU in float32.  feat (P, 611) float32.
    scales (operand_scales): the forward operands are REAL float16 pairs at the kernel's scales -- hi = float16(x U), lo = float16(x U - hi) -- so that a lo half
    below 2^-14 is a float16 subnormal with the absolute spacing 2^-24: at range level k the operands are 16^k times smaller and an operand of ordinary size keeps
    fewer than 22 bits.  (The rescaling by a power of two is exact; the split of the rescaled number is not level-invariant.)
    -> out (P, k) float32, pre: the three hidden pre-activations, dfeat (P, 611) float32 for the upstream gradient go (P, k) or None"""
    q = split22 if split else (lambda a: np.asarray(a, np.float32))
    Wq = [q(w) for w in W]; pre = []

    def gemm(x, l):
        if not split or scales is None:
            return q(x) @ Wq[l].T
        xs = np.asarray(x, np.float32) * np.float32(scales[l]); hi = xs.astype(np.float16).astype(np.float32); lo = (xs - hi).astype(np.float16).astype(np.float32)
        return (hi @ Wq[l].T + lo @ Wq[l].T) * np.float32(1.0 / scales[l])
    a = feat
    for l in range(3):
        z = gemm(a, l) + np.asarray(b[l], np.float32); pre.append(z); a = np.maximum(z, np.float32(0))
    out = gemm(a, 3) + np.asarray(b[3], np.float32)
    if go is None:
        return out, pre, None
    g = q(go) @ Wq[3]
    for l in (2, 1, 0):
        g = q(g * (pre[l] > 0)) @ Wq[l]
    return out, pre, g


def split_backstop(S, layers=4):
    """the derived worst case of the split format per element: every product of the `layers` GEMMs on the path is off by at most SPLIT, and an activation's error
    propagates through |W| like the scale itself: (1 + SPLIT)^layers - 1 of the own scale"""
    return ((1 + SPLIT) ** layers - 1) * S


def excluded(margins, clamp_units=0.0):
    """the points left out of the GRADIENT gates: a branch quantity within float32 reach of its branch.  clamp_units: what the route may move the clamped value
    by, in units of u S (its value gate)"""
    ex = (margins["coord"] < KINK_COORD) | (margins["relu"] < 1.0)
    return ex | (margins["clamp"] < clamp_units) if "clamp" in margins else ex


# ---- gates ---------------------------------------------------------------------------------------------------------------------------------------------------
def units(got, ref, S):
    """|got - ref| / (u S) per element; where S == 0 the definition gives an exact value: 0 if it is met bit for bit, inf otherwise"""
    e = np.abs(np.asarray(got, np.float64) - ref)
    return np.where(S > 0, e / (U * np.where(S > 0, S, 1.0)), np.where(e > 0, np.inf, 0.0))


def term_gate(n, summands, s_summands, e_val):
    """a term accumulated with float64 atomics over n float32 summands: (n + 8) u sum |summand| for the summands' own roundings (as the Chamfer pins do) + what a
    summand inherits from the network's value it is made of: e_val u S per summand, e_val = the value gate of the route in units of u S"""
    return (n + 8) * U * np.abs(summands).sum() + e_val * U * np.abs(s_summands).sum()


def rel(a, b):
    """the whole-array metric of tests/test_gpu_parity.py"""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)
