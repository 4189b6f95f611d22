"""Test helper (not a test file): SMPL-H restated in torch float64 from its definition, gradients from autograd.

Written from the contract the head of csrc/smplh.hip and include/vistracker.h state, not from the kernels and not from oracle/vt_oracle.c (whose backward is a
hand-derived VJP -- the same derivation the kernels implement, so a slip shared by both has nothing to catch it there).  Every sum is an ``einsum`` or a
matrix product, the chain is the recursion ``G_j = G_parent(j) . [R_j | J_j - J_parent(j)]`` over any ``parents`` with ``parents[j] < j``, and no derivative is
written by hand.  Nothing here touches libvistracker_hip.so or the oracle.

Semantics (the reference layer's, quirks included):
  * rotations: axis-angle -> quaternion -> matrix with ``n = |theta + 1e-8|`` (the shift is added to every component BEFORE the norm), axis = ``theta / n``
    (the unshifted theta), ``q = (cos n/2, sin(n/2) axis)`` normalised; so an exactly zero theta has axis 0, R = I exactly, and the derivative of R = I + [theta]x comes out of sin(n/2) / n alone
  * pose map: ``R[1:] - I`` flattened to 459 values; ``v_posed = v_template + shapedirs . betas + posedirs . pose_map``
  * joints: ``J = J_regressor . (v_template + shapedirs . betas)``
  * skinning: ``A_j = [G_rot | G_t - G_rot J_j]``, ``T_v = sum_j weights[v, j] A_j``, ``verts = T_v [v_posed; 1] + trans``, ``jtr = G_t + trans``

The model arrays pass through float32 first: that is what ``ops.SmplhHandle`` uploads, and a reference must see the operator's inputs, not better ones.

``per_row_err`` is the metric the SMPL-H gradient tests share and ``GATE`` the factor of their common gate (see its comment).
"""
from __future__ import annotations

import numpy as np
import torch

F64 = torch.float64

# A kernel's gradient row (a joint of dpose, a column of dbetas, an axis of dtrans) passes when its per_row_err against this model is at most GATE * e32, with
# e32 the largest per_row_err of the float32 CPU oracle on the same case.  The oracle accumulates its long sums in double and rounds once, the kernels add
# float32 partials in another order (MFMA K order, 27 tile partials, 54 split-K slabs): the factor is the allowance for that, from no measurement of a kernel.
# e32 is ONE number per case, the maximum over all 65 rows: a single badly conditioned row (a dbetas column that nearly cancels in a one-frame batch) sets the
# gate of every row of that case.  Measured margins are thin in two cases -- B = 1: the kernels' worst row at 3.2e-5 of 3.6e-5; dverts = 0: 2.0e-5 of 2.6e-5
# (profiles/r14_smplh_perjoint.txt).  A kernel change that only reorders float32 sums can cross them; the factor is widened only with that cause written here,
# and never near the 1e-3 the host mutation test must reject.
GATE = 8.0


def per_row_err(got, ref, rows, zero_rows=()):
    """(B, rows * c) arrays -> per row r: max_{b,c} |got - ref| / max_{b,c} |ref|.  A row whose reference is all zero (or not finite) has no scale and
    would pass anything: that is an error of the case, not a pass.  The one exception is declared by the caller: ``zero_rows`` are rows that the case makes
    zero by construction (every term of their sums is a product with an exact zero).  Their reference must BE zero, and their error is max |got|, absolute:
    sums of exact zeros are zero in any order, so a gate of any size asks such a row to be zero to the gate's size."""
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    B = ref.shape[0]
    g = got.reshape(B, rows, -1); r = ref.reshape(B, rows, -1)
    scale = np.abs(r).max(axis=(0, 2))
    zero = np.zeros(rows, bool); zero[list(zero_rows)] = True
    assert (scale[zero] == 0).all(), f"rows declared zero that are not: {np.nonzero(zero & (scale != 0))[0].tolist()}"
    assert np.isfinite(scale).all() and (scale[~zero] > 0).all(), f"rows without a scale: {np.nonzero(~zero & ~(scale > 0))[0].tolist()}"
    assert np.isfinite(g).all(), "NaN or Inf in the gradient under test"
    return np.abs(g - r).max(axis=(0, 2)) / np.where(zero, 1.0, scale)


GRAD_ROWS = (("dpose", 52), ("dbetas", 10), ("dtrans", 3))


def grad_errs(got, ref, zero_joints=()):
    """(dpose, dbetas, dtrans) x 2 -> {name: per-row errors}; ``zero_joints``: the joints of dpose that the case makes exactly zero (see per_row_err)"""
    return {name: per_row_err(g, r, rows, zero_joints if name == "dpose" else ()) for (name, rows), g, r in zip(GRAD_ROWS, got, ref)}


def worst(errs):
    return max(float(e.max()) for e in errs.values())


def rodrigues(theta):
    """(..., 3) axis-angle -> (..., 3, 3)"""
    shifted = theta + 1e-8
    n = torch.sqrt((shifted * shifted).sum(-1, keepdim=True))
    axis = theta / n
    half = 0.5 * n
    q = torch.cat([torch.cos(half), torch.sin(half) * axis], -1)
    q = q / torch.sqrt((q * q).sum(-1, keepdim=True))
    w, x, y, z = q.unbind(-1)
    R = torch.stack([w * w + x * x - y * y - z * z, 2 * x * y - 2 * w * z, 2 * w * y + 2 * x * z,
                     2 * w * z + 2 * x * y, w * w - x * x + y * y - z * z, 2 * y * z - 2 * w * x,
                     2 * x * z - 2 * w * y, 2 * w * x + 2 * y * z, w * w - x * x - y * y + z * z], -1)
    return R.reshape(theta.shape[:-1] + (3, 3))


def rodrigues_np(aa):
    """(n, 3) -> (n, 9) float64"""
    return rodrigues(torch.as_tensor(np.asarray(aa, np.float64)).reshape(-1, 3)).reshape(-1, 9).numpy()


def rodrigues_bwd_np(aa, dR):
    """(n, 3), (n, 9) -> d sum(R * dR) / d aa, (n, 3) float64"""
    t = torch.as_tensor(np.asarray(aa, np.float64)).reshape(-1, 3).clone().requires_grad_(True)
    (rodrigues(t).reshape(-1, 9) * torch.as_tensor(np.asarray(dR, np.float64)).reshape(-1, 9)).sum().backward()
    return t.grad.numpy()


class SmplhModel:
    def __init__(self, model: dict):
        def arr(k):
            return torch.as_tensor(np.asarray(model[k]).astype(np.float32).astype(np.float64))
        self.v_template, self.shapedirs, self.posedirs = arr("v_template"), arr("shapedirs"), arr("posedirs")
        self.J_regressor, self.weights = arr("J_regressor"), arr("weights")
        self.V, self.J = self.weights.shape
        self.parents = [int(p) for p in np.asarray(model["parents"])]
        assert all(0 <= self.parents[j] < j for j in range(1, self.J)), "parents[j] < j"

    def _forward(self, pose, betas, trans):
        B = pose.shape[0]
        R = rodrigues(pose.reshape(B, self.J, 3))                                       # (B, J, 3, 3)
        v_shaped = self.v_template + torch.einsum("vcl,bl->bvc", self.shapedirs, betas)
        joints = torch.einsum("jv,bvc->bjc", self.J_regressor, v_shaped)
        pose_map = (R[:, 1:] - torch.eye(3, dtype=F64)).reshape(B, -1)
        v_posed = v_shaped + (pose_map @ self.posedirs.reshape(self.V * 3, -1).T).reshape(B, self.V, 3)
        Grot, Gt = [R[:, 0]], [joints[:, 0]]
        for j in range(1, self.J):
            p = self.parents[j]
            Grot.append(Grot[p] @ R[:, j])
            Gt.append((Grot[p] @ (joints[:, j] - joints[:, p])[..., None])[..., 0] + Gt[p])
        Grot, Gt = torch.stack(Grot, 1), torch.stack(Gt, 1)                             # (B, J, 3, 3), (B, J, 3)
        At = Gt - (Grot @ joints[..., None])[..., 0]
        Trot = torch.einsum("vj,bjrc->bvrc", self.weights, Grot)
        Tt = torch.einsum("vj,bjr->bvr", self.weights, At)
        verts = (Trot @ v_posed[..., None])[..., 0] + Tt + trans[:, None]
        return verts, Gt + trans[:, None], v_posed

    @staticmethod
    def _t(a, grad=False):
        return torch.as_tensor(np.asarray(a, np.float64)).clone().requires_grad_(grad)

    def forward(self, pose, betas, trans):
        """-> verts (B, V, 3), jtr (B, J, 3), v_posed (B, V, 3), float64 numpy"""
        with torch.no_grad():
            return tuple(o.numpy() for o in self._forward(self._t(pose), self._t(betas), self._t(trans)))

    def backward(self, pose, betas, trans, dverts, djtr=None):
        """d (sum(verts * dverts) + sum(jtr * djtr)) / d (pose, betas, trans) -> dpose (B, 3 J), dbetas (B, 10), dtrans (B, 3), float64 numpy"""
        return self.backward_many(pose, betas, trans, [(dverts, djtr)])[0]

    def backward_many(self, pose, betas, trans, cotangents):
        """``backward`` for several (dverts, djtr) pairs over one forward pass"""
        p, b, t = self._t(pose, True), self._t(betas, True), self._t(trans, True)
        verts, jtr, _ = self._forward(p, b, t)
        out = []
        for i, (dverts, djtr) in enumerate(cotangents):
            s = (verts * self._t(dverts)).sum()
            if djtr is not None:
                s = s + (jtr * self._t(djtr)).sum()
            out.append(tuple(g.numpy() for g in torch.autograd.grad(s, (p, b, t), retain_graph=i + 1 < len(cotangents))))
        return out
