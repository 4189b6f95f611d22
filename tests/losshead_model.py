"""numpy restatement of SIF-Net's training objective at labelled points (model/chore_tri_vis.py:52-99 get_errors, model/chore.py:312-325 get_df_loss) and of
its gradient to the predictions by torch's autograd rules, written from the formulas; shares no code with the product.  Every operation is carried out in
``dtype``: float64 is the model the kernel is held to, float32 is the same expression in the reference's number format, and the difference of the two on a
test's inputs is e32, the bound's unit.

Per stack, with p a prediction, g its label, md = max_dist and mask = [df_o < 0.05] (strict, on the label as given):
    df_h, df_o   |min(p, md) - min(g, md)| summed over N, mean over B       d/dp = sign(min(p, md) - min(g, md)) [p <= md]
    parts        (logsumexp(x) - x[label]) summed over N, mean over B       d/dx = softmax(x) - onehot(label)
    pca          mean over B 9 N of (p - g)^2 mask                          d/dp = 2 (p - g) mask
    vis          mean over B N of |p - g| mask (l1) or (p - g)^2 mask (l2)  d/dp = sign(p - g) mask or 2 (p - g) mask
    obj_center   mean over B 3 N of (p - g)^2 mask                          d/dp = 2 (p - g) mask
terms = the six in the slot order of the reference's losses_all (df_h, df_o, parts, pca, vis, obj_center), averaged over the stacks, unweighted;
losses_all = terms x the slot's weight, weights in the order of loss_weights (dfh, dfo, parts, pca, obj_center, vis); error = their sum."""
import numpy as np

SLOTS = ("df_h", "df_o", "parts", "pca", "vis", "obj_center")
SLOT_WEIGHT = (0, 1, 2, 3, 5, 4)
WEIGHTS = (1.0, 1.0, 0.006, 500.0, 1000.0, 1000.0)
HEADS = ("df", "pca", "parts", "centers", "vis")
DIMS = (2, 9, 14, 3, 1)


def per_point(labels, N):
    """pca_gt (B,9) -> (B,9,N), obj_center (B,3) -> (B,3,N), visibility (B,) -> (B,N): what the reference's loader repeats (traindata_online.py:102,177-183)"""
    pca, oc, vis = labels
    rep = lambda a: np.ascontiguousarray(np.repeat(np.asarray(a)[..., None], N, -1))       # noqa: E731
    return rep(pca), rep(oc), rep(vis)


def loss_head(preds, df_h, df_o, parts_gt, pca_gt, obj_center, visibility, max_dist, weights=WEIGHTS, vis_loss="l2", gscale=1.0, dtype=np.float64):
    """preds: df (S,B,2,N), pca (S,B,9,N), parts (S,B,14,N), centers (S,B,3,N), vis (S,B,1,N); labels per point: df_h, df_o (B,N), parts_gt (B,N) integers in
    [0,14), pca_gt (B,9,N), obj_center (B,3,N), visibility (B,N).  -> dict: terms (6,), losses_all (6,), error, and d_df .. d_vis = gradients of gscale x error"""
    T = dtype
    df, pca, parts, centers, vis = (np.asarray(a).astype(T) for a in preds)
    S, B, _, N = df.shape
    gh, go, pg, og, vg = (np.asarray(a).astype(T) for a in (df_h, df_o, pca_gt, obj_center, visibility))
    lab = np.asarray(parts_gt).astype(np.int64)
    assert lab.min() >= 0 and lab.max() < 14
    md = T(np.float32(max_dist))                                                    # an fp32 scalar by contract
    mask = (np.asarray(df_o) < np.float32(0.05)).astype(T)[:, None]                 # (B,1,N), decided on the label as given (float32)
    w = [T(weights[i]) for i in SLOT_WEIGHT]
    one_s = T(1) / T(S)
    up = [T(gscale) * one_s * wk for wk in w]                                       # what reaches a stack's weighted loss: error /= S, then the weight
    terms = np.zeros(6, T)
    grads = {h: np.zeros((S, B, k, N), T) for h, k in zip(HEADS, DIMS)}
    onehot = (lab[:, None, :] == np.arange(14)[None, :, None]).astype(T)
    for s in range(S):
        for k, g in ((0, gh), (1, go)):                                              # get_df_loss
            p = df[s, :, k]
            a = np.minimum(p, md) - np.minimum(g, md)
            terms[k] += np.abs(a).sum(-1).mean()
            grads["df"][s, :, k] = np.sign(a) * (p <= md).astype(T) * (up[k] / T(B))
        x = parts[s]                                                                 # CrossEntropyLoss(reduction='none'), .sum(-1).mean()
        z = x - x.max(1, keepdims=True)
        ez = np.exp(z)
        se = ez.sum(1, keepdims=True)
        ce = np.log(se[:, 0]) - (z * onehot).sum(1)
        terms[2] += ce.sum(-1).mean()
        grads["parts"][s] = (ez / se - onehot) * (up[2] / T(B))
        d = pca[s] - pg                                                              # mse * mask, .mean()
        terms[3] += (d * d * mask).mean()
        grads["pca"][s] = T(2) * d * mask * (up[3] / T(B * 9 * N))
        d = vis[s] - vg[:, None]
        if vis_loss == "l1":
            terms[4] += (np.abs(d) * mask).mean()
            grads["vis"][s] = np.sign(d) * mask * (up[4] / T(B * N))
        else:
            assert vis_loss == "l2"
            terms[4] += (d * d * mask).mean()
            grads["vis"][s] = T(2) * d * mask * (up[4] / T(B * N))
        d = centers[s] - og
        terms[5] += (d * d * mask).mean()
        grads["centers"][s] = T(2) * d * mask * (up[5] / T(B * 3 * N))
    terms = terms * one_s if S > 1 else terms
    losses_all = terms * np.array(w, T)
    out = {"terms": terms, "losses_all": losses_all, "error": losses_all.sum()}
    out.update({"d_" + h: grads[h] for h in HEADS})
    return out


OUTPUTS = ("terms", "losses_all", "error") + tuple("d_" + h for h in HEADS)


def reference_and_e32(*args, **kw):
    """(float64 run, {output: max |float32 run - float64 run|}) on the same inputs"""
    r64 = loss_head(*args, dtype=np.float64, **kw)
    r32 = loss_head(*args, dtype=np.float32, **kw)
    e32 = {k: np.abs(np.asarray(r32[k]).astype(np.float64) - r64[k]) for k in OUTPUTS}
    # terms and losses_all: one bound per slot (their scales differ by the weights); a gradient tensor: one bound, its largest element error
    return r64, {k: (v if k in ("terms", "losses_all") else float(v.max())) for k, v in e32.items()}


CASES = [(3, "l2"), (3, "l1"), (1, "l2"), (1, "l1")]


def golden_case(g, S, vis_loss):
    """(model arguments, the golden's outputs) of one recorded case"""
    N = g["df"].shape[-1]
    preds = [g[h][:S].astype(np.float32) for h in HEADS]
    labels = (g["df_h"], g["df_o"], g["parts_gt"]) + per_point((g["pca_gt"], g["obj_center"], g["visibility"]), N)
    want = {"error": g[f"S{S}_{vis_loss}_error"], "losses_all": g[f"S{S}_{vis_loss}_losses_all"], "d_vis": g[f"S{S}_{vis_loss}_d_vis"]}
    want.update({k: g[f"S{S}_{k}"] for k in ("d_df", "d_pca", "d_parts", "d_centers")})
    return (preds, *labels, float(g["max_dist"])), dict(weights=tuple(g["weights"]), vis_loss=vis_loss), want
