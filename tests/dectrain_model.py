"""float64 model of SIF-Net's decoder training step, written from the definitions (it shares no code with the product): the crop-space pinhole projection
(model/camera.py:45-90), the three orthographic planes (chore_triplane.py:220-251), bilinear sampling with align_corners=True and zeros padding written out by
hand (model/geometry.py:4-14 = F.grid_sample), the 611-channel concatenation (chore_triplane.py:139-151), Linear/ReLU chains for the five decoders
(chore.py:113-126; a sigmoid ends vis), the objective of get_errors (chore_tri_vis.py:52-99) and torch autograd for the weight gradients.  Runs in any dtype:
the float32 run against the float64 run on a test's own inputs is that test's e32, and the kernels get 4 e32 -- per prediction head, and per PARAMETER TENSOR
for the gradients (40 bounds, each on its tensor's own scale).
"""
import numpy as np
import torch

HEADS = ("df", "pca", "parts", "centers", "vis")
DIMS = (2, 9, 14, 3, 1)
CAM = (979.7844, 979.840, 1018.952, 779.486, 1200.0)           # fx, fy, cx, cy in pixels, crop size
OUT_DIST = 5.0
WEIGHTS = (1.0, 1.0, 0.006, 500.0, 1000.0, 1000.0)             # dfh, dfo, parts, pca, obj_center, vis
# the feature maps in concatenation order, with the projection each is sampled at; z_feat sits after im_feat
CONCAT = (("im_feat", "persp"), ("z_feat", None), ("tmpx", "persp"), ("tri_tmpx0", "right"), ("tri_tmpx1", "back"), ("tri_tmpx2", "top"),
          ("tri_feat0", "right"), ("tri_feat1", "back"), ("tri_feat2", "top"))
TENSORS = tuple((h, l, kind) for h in HEADS for l in range(4) for kind in ("weight", "bias"))
GOLDEN_ROWS = (0, 17, 31, 64, 77, 100, 126, 127)               # rows of the 128-row weight matrices recorded in tests/golden/dectrain.npz


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype)


def projections(pts, cc, bc, cam=CAM):
    """pts (B,N,3), cc (B,2), bc (B,3) tensors -> {kind: (u, v)} each (B,N), normalised to [-1, 1] inside the image / the plane"""
    fx, fy, cx, cy, crop = cam
    x, y, z = pts[..., 0], pts[..., 1], pts[..., 2]
    px = crop / 2 + (fx * x / z + cx) - cc[:, 0:1]
    py = crop / 2 + (fy * y / z + cy) - cc[:, 1:2]
    c = pts - bc[:, None, :]
    return {"persp": (2 * px / crop - 1, 2 * py / crop - 1), "right": (c[..., 2], c[..., 1]), "back": (-c[..., 0], c[..., 1]), "top": (c[..., 0], -c[..., 2])}


def texel_coords(m, u, v):
    R = m.shape[-1]
    return (u + 1) / 2 * (R - 1), (v + 1) / 2 * (R - 1)


def bilinear(m, u, v):
    """m (B,C,R,R), u (x, along the last axis) and v (B,N) -> (B,C,N): the four neighbouring texels weighted by the opposite areas, a texel outside the map counts 0"""
    B, C, R, _ = m.shape
    ix, iy = texel_coords(m, u, v)
    x0, y0 = torch.floor(ix), torch.floor(iy)
    flat = m.reshape(B, C, R * R)
    out = 0
    for dy in (0, 1):
        for dx in (0, 1):
            xi, yi = x0 + dx, y0 + dy
            w = (1 - (ix - xi).abs()) * (1 - (iy - yi).abs())
            ok = (xi >= 0) & (xi <= R - 1) & (yi >= 0) & (yi <= R - 1)
            idx = (yi.clamp(0, R - 1) * R + xi.clamp(0, R - 1)).long()
            val = flat.gather(2, idx[:, None, :].expand(B, C, idx.shape[1]))
            out = out + val * (w * ok)[:, None, :]
    return out


def features(maps, pts, cc, bc):
    """-> (B,611,N) features in the reference's channel order, in_img (B,N)"""
    pr = projections(pts, cc, bc)
    cols = []
    for name, kind in CONCAT:
        if name == "z_feat":
            cols.append(torch.stack([pts[..., 0], pts[..., 1], pts[..., 2] - 2.2], 1))
        else:
            cols.append(bilinear(maps[name], *pr[kind]))
    u, v = pr["persp"]
    return torch.cat(cols, 1), (u >= -1) & (u <= 1) & (v >= -1) & (v <= 1)


def decode(params, feat, in_img):
    preds = []
    for name in HEADS:
        h = feat
        for l, (w, b) in enumerate(params[name]):
            h = torch.einsum("oi,bin->bon", w, h) + b[None, :, None]
            if l < 3:
                h = torch.relu(h)
        if name == "vis":
            h = torch.sigmoid(h)
        if name == "df":
            h = torch.where(in_img[:, None, :], h, torch.full_like(h, OUT_DIST))
        preds.append(h)
    return preds


def make_params(decoders, dtype):
    return {n: [(_t(w, dtype).requires_grad_(True), _t(b, dtype).requires_grad_(True)) for w, b in decoders[n]] for n in HEADS}


def grads_of(params):
    return {(n, l, kind): (t.grad if t.grad is not None else torch.zeros_like(t)).detach().numpy().astype(np.float64)
            for n in HEADS for l, wb in enumerate(params[n]) for kind, t in zip(("weight", "bias"), wb)}


def get_errors(preds_list, lab, max_dist, weights=WEIGHTS, vis_loss="l2"):
    """chore_tri_vis.py:52-99 on a list of stacks; lab: df_h, df_o (B,N), labels (B,N), pca_axis (B,3,3), obj_center (B,3), visibility (B,) tensors
    -> error, losses_all (6,) in the slot order df_h, df_o, parts, pca, vis, obj_center"""
    F = torch.nn.functional
    error, allv = 0, 0
    for df, pca, parts, centers, vis in preds_list:
        dfl = lambda g, p: (torch.clamp(p, max=max_dist) - torch.clamp(g, max=max_dist)).abs().sum(-1).mean()      # noqa: E731
        lh, lo = dfl(lab["df_h"], df[:, 0]) * weights[0], dfl(lab["df_o"], df[:, 1]) * weights[1]
        lp = (F.cross_entropy(parts, lab["labels"].long(), reduction="none") * weights[2]).sum(-1).mean()
        mask = (lab["df_o"] < 0.05)[:, None, :].to(df.dtype)
        lpca = (((pca - lab["pca_axis"].reshape(-1, 9, 1)) ** 2 * mask) * weights[3]).mean()
        lc = ((centers - lab["obj_center"][:, :, None]) ** 2 * mask).mean() * weights[4]
        d = vis - lab["visibility"][:, None, None]
        lv = ((d.abs() if vis_loss == "l1" else d ** 2) * mask).mean() * weights[5]
        losses = torch.stack([lh, lo, lp, lpca, lv, lc])
        error, allv = error + losses.sum(), allv + losses
    return error / len(preds_list), allv / len(preds_list)


def run(decoders, maps_list, pts, cc, bc, upstream=None, labels=None, max_dist=5.0, dtype=torch.float64):
    """The training query on a list of S map sets and the weight gradients of either sum_s sum(pred_s * upstream_s) (``upstream``: a list of S dicts head ->
    (B,k,N), a missing head = zero) or of get_errors (``labels``).  -> {"preds": [S][5] arrays, "grads": {(head, layer, kind): array}, "error", "losses_all"}"""
    params = make_params(decoders, dtype)
    p, c, b = _t(pts, dtype), _t(cc, dtype), _t(bc, dtype)
    preds_list = []
    for maps in maps_list:
        feat, in_img = features({k: _t(v, dtype) for k, v in maps.items()}, p, c, b)
        preds_list.append(decode(params, feat, in_img))
    out = {"preds": [[t.detach().numpy().astype(np.float64) for t in preds] for preds in preds_list]}
    if upstream is not None:
        loss = sum((preds[HEADS.index(h)] * _t(g, dtype)).sum() for preds, up in zip(preds_list, upstream) for h, g in up.items())
        if torch.is_tensor(loss):
            loss.backward()
    elif labels is not None:
        lab = {k: _t(v, torch.int64 if k == "labels" else dtype) for k, v in labels.items()}
        loss, losses_all = get_errors(preds_list, lab, max_dist)
        loss.backward()
        out["error"], out["losses_all"] = float(loss.detach()), losses_all.detach().numpy().astype(np.float64)
    out["grads"] = grads_of(params)
    return out


def reference_and_e32(*args, **kw):
    """-> (float64 run, e32): e32["preds"][s][head] and e32["grads"][tensor] = the largest element error of the float32 run"""
    r64, r32 = run(*args, dtype=torch.float64, **kw), run(*args, dtype=torch.float32, **kw)
    e32 = {"preds": [[np.abs(a - b).max() for a, b in zip(p64, p32)] for p64, p32 in zip(r64["preds"], r32["preds"])],
           "grads": {k: np.abs(r64["grads"][k] - r32["grads"][k]).max() for k in r64["grads"]}}
    if "losses_all" in r64:
        e32["losses_all"] = np.abs(r64["losses_all"] - r32["losses_all"])
    return r64, e32


# ---- the inputs of the tests ---------------------------------------------------------------------------------------------------------------------------------
def make_inputs(B=2, N=150, seed=11):
    """float32 points around a body centre whose coordinates are exact in float32, with four kinds mixed in at random places (the ragged last tile included):
    outside the image, outside each orthographic plane, on an exact texel coordinate (a plane coordinate of exactly -1 or +1 is texel 0 or R - 1), the bulk
    inside.  -> pts (B,N,3), cc (B,2), bc (B,3)"""
    rng = np.random.default_rng(seed)
    bc = np.array([[0.25, -0.125, 2.25], [-0.5, 0.25, 2.0], [0.0, 0.5, 2.5], [0.125, 0.0, 2.125]], np.float32)[np.arange(B) % 4]
    pts = (bc[:, None, :] + rng.normal(0, 0.25, (B, N, 3))).astype(np.float32)
    special = np.array([[2.5, 0, 0], [-2.5, 0, 0], [0, 2.0, 0], [0, -2.0, 0.5],                       # outside the image (and the planes)
                        [0, 1.1, 0], [0, 0, 1.2], [1.05, 0, 0], [-1.1, 0.3, 0], [0.2, -1.15, 0.1], [0, 0, -1.01],      # outside planes, inside the image
                        [1, 0.3, 0.1], [-1, -0.2, 0.3], [0.1, 1, -0.2], [0.3, -1, 0.2], [0.2, 0.1, 1], [-0.3, 0.2, -1], [1, -1, 1], [-1, 1, -1]], np.float32)
    for b in range(B):
        where = rng.permutation(N)[:min(len(special), N)]
        pts[b, where] = bc[b] + special[:len(where)]
        if N >= 140:
            pts[b, N - 1] = bc[b] + special[10]; pts[b, N - 2] = bc[b] + special[4]; pts[b, N - 3] = bc[b] + special[0]      # the ragged tile gets one of each
    cc = (np.array([[1018.952, 779.486]] * B) + rng.normal(0, 20, (B, 2))).astype(np.float32)
    return pts, cc, bc


def make_upstream(B, N, seed, heads=HEADS):
    rng = np.random.default_rng(seed)
    return {h: rng.normal(0, 1, (B, DIMS[HEADS.index(h)], N)).astype(np.float32) for h in heads}


def make_labels(B, N, seed, md=5.0):
    """a fixed labelled batch in the keys of training.make_training_batch (without the points)"""
    rng = np.random.default_rng(seed)
    return {"df_h": rng.uniform(0.0, 0.6, (B, N)).astype(np.float32),
            "df_o": np.where(rng.random((B, N)) < 0.5, rng.uniform(0.0, 0.05, (B, N)), rng.uniform(0.05, 0.8, (B, N))).astype(np.float32),
            "labels": rng.integers(0, 14, (B, N)).astype(np.int32), "pca_axis": np.linalg.qr(rng.normal(size=(B, 3, 3)))[0].astype(np.float32),
            "obj_center": rng.normal(0, 0.4, (B, 3)).astype(np.float32), "visibility": rng.uniform(0.1, 1.0, (B,)).astype(np.float32)}


def point_classes(maps, pts, cc, bc):
    """-> {class: boolean (B,N)} as the float64 model sees the float32 inputs"""
    dt = torch.float64
    pr = projections(_t(pts, dt), _t(cc, dt), _t(bc, dt))
    inside = lambda uv: (uv[0].abs() <= 1) & (uv[1].abs() <= 1)      # noqa: E731
    out = {"outside_image": ~inside(pr["persp"])}
    exact = torch.zeros_like(out["outside_image"])
    for kind in ("right", "back", "top"):
        out["outside_" + kind] = ~inside(pr[kind]) & inside(pr["persp"])
    for name, kind in CONCAT:
        if kind is not None:
            ix, iy = texel_coords(_t(maps[name], dt), *pr[kind])
            R = maps[name].shape[-1]
            exact |= ((ix == ix.round()) & (ix >= 0) & (ix <= R - 1)) | ((iy == iy.round()) & (iy >= 0) & (iy <= R - 1))
    out["exact_texel"] = exact
    out["bulk"] = inside(pr["persp"]) & inside(pr["right"]) & inside(pr["back"]) & inside(pr["top"]) & ~exact
    return {k: v.numpy() for k, v in out.items()}


def train_model(decoders, maps, pts, cc, bc, labels, steps, lr=1e-3, max_dist=5.0, dtype=torch.float64):
    """``steps`` steps of torch.optim.Adam on the decoders, one fixed batch -> the total error before every step"""
    params = make_params(decoders, dtype)
    opt = torch.optim.Adam([t for n in HEADS for wb in params[n] for t in wb], lr=lr)
    feat, in_img = features({k: _t(v, dtype) for k, v in maps.items()}, _t(pts, dtype), _t(cc, dtype), _t(bc, dtype))
    lab = {k: _t(v, torch.int64 if k == "labels" else dtype) for k, v in labels.items()}
    errors = []
    for _ in range(steps):
        opt.zero_grad()
        error, _ = get_errors([decode(params, feat, in_img)], lab, max_dist)
        error.backward()
        opt.step()
        errors.append(float(error.detach()))
    return errors
