"""HVOP-Net training, first block: the encoders of ``infill.ConditionalMInfiller`` with gradients.  Mirror of

    model.transformers.former_deci.TransformerV2 / TransformerEncoderLayer.forward_pre          (former_deci.py:33-175; kernels: csrc/formertrain.hip)
    model.infill.mfiller_cond.ConditionalMInfiller.forward                                       (mfiller_cond.py:84-107)
    trainer.trainer_infiller.TrainerInfiller.motion_losses / trainer_cinfiller.compute_loss      (trainer_infiller.py:33-47, trainer_cinfiller.py:30-44)

The encoder layers run ``ops.former_layer_train`` (a taped HIP forward and a hand-written HIP backward per layer); the two input projections and the predictor MLP
are six small GEMMs left to torch autograd -- unless ``fused_ends`` is on: then the projections run ``ops.infill_proj_train`` and the predictor with the objective
``ops.infill_head_train`` (csrc/infillhead.hip), and every gradient of a step comes from the project's own launches.  Dropout masks come from the counter-based hash of csrc/dropout_hash.h, restated here for the per-layer seeds: a step
is a function of its ``seed``.  ``infill.py`` (inference) is untouched; ``export()`` hands the trained weights to it."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _lib as L
from . import infill, ops
from .training import multistep_lr

_M32 = 0xffffffff


def _mix32(x):
    x ^= x >> 16; x = (x * 0x7feb352d) & _M32; x ^= x >> 15; x = (x * 0x846ca68b) & _M32; x ^= x >> 16
    return x


def dropout_hash(seed: int, site: int, index: int) -> int:
    """csrc/dropout_hash.h on python integers"""
    h = _mix32((seed & _M32) ^ ((0x9e3779b9 * (site + 1)) & _M32))
    h = _mix32(h ^ ((seed >> 32) & _M32))
    h = _mix32(h ^ (index & _M32))
    return _mix32(h ^ ((index >> 32) & _M32))


def layer_seed(seed: int, encoder_id: int, layer: int) -> int:
    """the 64-bit seed of layer ``layer`` of encoder ``encoder_id``: two hashes of (seed, site 100 + encoder_id, 2 layer | 2 layer + 1)"""
    return dropout_hash(seed, 100 + encoder_id, 2 * layer) | (dropout_hash(seed, 100 + encoder_id, 2 * layer + 1) << 32)


def _leaf(t, device):
    t = t if torch.is_tensor(t) else torch.as_tensor(__import__("numpy").asarray(t))
    return t.detach().to(device=device, dtype=torch.float32).contiguous().clone().requires_grad_(True)


class TrainableTransformerV2:
    """``TransformerV2`` with gradients: ``num_layers`` pre-norm layers (former_deci.py:143-147 always builds them pre-norm; ``pre_norm`` only decides whether the
    final ``encoder.norm`` exists), the cached sine position table, parameters as leaves under the reference's state_dict keys."""

    def __init__(self, params, num_layers, d_model, num_heads, activation, pre_norm, dropout=0.0, device="cuda:0", encoder_id=0):
        self.L, self.D, self.H, self.activation, self.has_norm = int(num_layers), int(d_model), int(num_heads), activation, bool(pre_norm)
        self.dropout, self.dev, self.encoder_id, self.training = float(dropout), torch.device(device), int(encoder_id), True
        if activation not in ops.FORMER_ACT:
            raise L.VtError(f"TrainableTransformerV2: activation {activation!r}; one of {sorted(ops.FORMER_ACT)}")
        self.params = params
        self._pos = {}

    @classmethod
    def from_state_dict(cls, sd, prefix, num_layers, d_model, num_heads, dim_feedforward, activation, pre_norm, dropout=0.0, device="cuda:0", encoder_id=0):
        keys = [f"encoder.layers.{i}.{k}" for i in range(num_layers) for k in ops.FORMER_PARAM_KEYS] + (["encoder.norm.weight", "encoder.norm.bias"] if pre_norm else [])
        params = {k: _leaf(sd[prefix + k], device) for k in keys}
        F_ = params["encoder.layers.0.linear1.weight"].shape[0] if num_layers else dim_feedforward
        if F_ != dim_feedforward:
            raise L.VtError(f"TrainableTransformerV2: linear1 has {F_} rows, dim_feedforward is {dim_feedforward}")
        return cls(params, num_layers, d_model, num_heads, activation, pre_norm, dropout, device, encoder_id)

    def train(self):
        self.training = True
        return self

    def eval(self):
        self.training = False
        return self

    def named_parameters(self):
        return list(self.params.items())

    def state_dict(self):
        return {k: v.detach().clone() for k, v in self.params.items()}

    def pos(self, T):
        if T not in self._pos:
            self._pos[T] = infill.position_embedding_sine_1d(T, self.D // 2, self.D).to(self.dev).contiguous()
        return self._pos[T]

    def __call__(self, x, key_padding_mask=None, seed=None):
        p = self.dropout if self.training else 0.0
        if p > 0 and seed is None:
            raise L.VtError("TrainableTransformerV2: a training forward with dropout needs a seed")
        pos = self.pos(x.shape[1])
        for l in range(self.L):
            ps = [self.params[f"encoder.layers.{l}.{k}"] for k in ops.FORMER_PARAM_KEYS]
            x = ops.former_layer_train(x, pos, key_padding_mask, ps, self.H, self.activation, p, layer_seed(seed, self.encoder_id, l) if p > 0 else 0)
        if self.has_norm:
            x = ops.layernorm_train(x, self.params["encoder.norm.weight"], self.params["encoder.norm.bias"])
        return x


class TrainableConditionalMInfiller:
    """``ConditionalMInfiller`` (mfiller_cond.py:84-107) that trains; ``opt``: the namespace of config/cmf-k4-lrot.json.  Encoder ids: 0 SMPL, 1 object, 2 joint."""

    ENCODERS = (("encoder_smpl.", "smpl"), ("encoder_obj.", "obj"), ("encoder_joint.", "joint"))

    def __init__(self, sd, opt, dropout=None, device="cuda:0", fused_ends=False):
        sd = infill._strip(sd); self.opt, self.dev = opt, torch.device(device)
        self.sd_keys = list(sd)
        dj = opt.d_model_smpl + opt.d_model_obj
        self.enc = {}
        for e, (prefix, tag) in enumerate(self.ENCODERS):
            d = dj if tag == "joint" else getattr(opt, f"d_model_{tag}")
            self.enc[tag] = TrainableTransformerV2.from_state_dict(
                sd, prefix, getattr(opt, f"num_layers_{tag}"), d, getattr(opt, f"num_heads_{tag}"), getattr(opt, f"dim_forward_{tag}"),
                getattr(opt, f"activation_{tag}"), getattr(opt, f"pre_norm_{tag}"), getattr(opt, f"dropout_{tag}") if dropout is None else dropout, self.dev, e)
        self.plain = {k: _leaf(sd[k], self.dev) for k in sd if not k.startswith(tuple(p for p, _ in self.ENCODERS))}
        self.n_head = len(opt.hidden_dims) + 1
        self.fused_ends = bool(fused_ends)
        self.ends_route = self._ends_route() if self.fused_ends else "torch: fused_ends is off"

    @classmethod
    def from_state_dict(cls, sd, opt, dropout=None, device="cuda:0", fused_ends=False):
        return cls(sd, opt, dropout, device, fused_ends)

    def _ends_route(self):
        """"hip" when the projections and the predictor are inside the contract of csrc/infillhead.hip, else "torch: <reason>" (the torch composition runs).
        Decided once, on the widths alone: a batch the kernels refuse (T < 3, B T > 2^24) raises ``VtError`` from ``loss()``; it does not change the route."""
        P = self.plain
        if self.n_head != 2:
            return f"torch: {self.n_head - 1} hidden layers in the predictor, the kernels take one"
        for k in ("feat_proj_smpl.weight", "feat_proj_obj.weight"):
            n, kin = P[k].shape
            if not (1 <= kin <= 160 and 16 <= n <= 160 and n % 16 == 0):
                return f"torch: {k} is {n} x {kin}; Kin in 1 .. 160 and N % 16 == 0 in 16 .. 160"
        (hd, d), c = P["predictor.0.weight"].shape, P["predictor.2.weight"].shape[0]
        if not (16 <= d <= 160 and d % 16 == 0 and 16 <= hd <= 64 and hd % 16 == 0 and 1 <= c <= 16):
            return f"torch: predictor {d} -> {hd} -> {c}; D % 16 == 0 in 16 .. 160, hidden % 16 == 0 in 16 .. 64, out_dim in 1 .. 16"
        return "hip"

    def train(self):
        for e in self.enc.values():
            e.train()
        return self

    def eval(self):
        for e in self.enc.values():
            e.eval()
        return self

    def named_parameters(self):
        out = dict(self.plain)
        for (prefix, tag) in self.ENCODERS:
            out.update({prefix + k: v for k, v in self.enc[tag].params.items()})
        return [(k, out[k]) for k in self.sd_keys if k in out]

    def state_dict(self):
        return {k: v.detach().clone() for k, v in self.named_parameters()}

    def export(self):
        return infill.ConditionalMInfiller(self.state_dict(), self.opt, device=self.dev)

    def features(self, data_smpl, mask_smpl, data_obj, mask_obj, seed=None):
        """the joint encoder's output (B, T, d_model_smpl + d_model_obj), what the predictor reads"""
        P = self.plain
        xs, xo = data_smpl.to(self.dev).float(), data_obj.to(self.dev).float()
        if self.ends_route == "hip":
            ps, po = ops.infill_proj_train([xs.contiguous(), xo.contiguous()], [P["feat_proj_smpl.weight"], P["feat_proj_obj.weight"]],
                                           [P["feat_proj_smpl.bias"], P["feat_proj_obj.bias"]])
        else:
            ps, po = F.linear(xs, P["feat_proj_smpl.weight"], P["feat_proj_smpl.bias"]), F.linear(xo, P["feat_proj_obj.weight"], P["feat_proj_obj.bias"])
        fs = self.enc["smpl"](ps, mask_smpl.to(self.dev), seed)
        fo = self.enc["obj"](po, mask_obj.to(self.dev), seed)
        return self.enc["joint"](torch.cat([fs, fo], -1).contiguous(), None, seed)

    def loss(self, batch, seed=None, lw=(1.0, 0.1)):
        """-> (loss, loss_pos, loss_accel, pred): the objective of trainer_infiller.py:33-47 on a batch, fp32 device scalars; loss carries the graph.  With the
        "hip" route the predictor and the objective are one ``ops.infill_head_train``; else the torch composition of ``__call__`` and ``motion_losses``."""
        gt = batch["gt_obj"].to(self.dev).float()
        if self.ends_route == "hip":
            x = self.features(batch["data_smpl"], batch["mask_smpl"], batch["data_obj"], batch["mask_obj"], seed)
            loss, lp, la, pred = ops.infill_head_train(x, gt.contiguous(), [self.plain[k] for k in ops.INFILL_HEAD_KEYS], *lw)
            return loss.float(), lp.float(), la.float(), pred
        pred = self(batch["data_smpl"], batch["mask_smpl"], batch["data_obj"], batch["mask_obj"], seed)
        la, lp = motion_losses(gt, pred, *lw)
        return lp + la, lp, la, pred

    def __call__(self, data_smpl, mask_smpl, data_obj, mask_obj, seed=None):
        P = self.plain
        x = self.features(data_smpl, mask_smpl, data_obj, mask_obj, seed)
        for i in range(self.n_head):
            x = F.linear(x, P[f"predictor.{2 * i}.weight"], P[f"predictor.{2 * i}.bias"])
            if i + 1 < self.n_head:
                x = F.leaky_relu(x)
        return x


def motion_losses(gt, pred, lw_pose=1.0, lw_accel=0.1):
    """(loss_accel, loss_pos) of trainer_infiller.py:33-47: the L1 mean times lw_pose, the L1 mean of the second differences along T times lw_accel"""
    loss_pos = F.l1_loss(pred, gt, reduction="mean") * lw_pose
    acc = lambda a: a[:, :-2] - 2 * a[:, 1:-1] + a[:, 2:]
    loss_accel = F.l1_loss(acc(pred), acc(gt), reduction="mean") * lw_accel
    return loss_accel, loss_pos


class HVOPTrainer:
    """one training step of HVOP-Net (trainer_cinfiller.py:30-44 + the Adam / MultiStepLR of the reference's base trainer): zero grads, forward, ``motion_losses``,
    one ``backward()``, one ``ops.FusedAdam.step()`` over the leaves.  Nothing in ``train_step`` waits on the host.  With ``fused_ends=True`` (off by default)
    forward and objective are ``model.loss``: the projections, the predictor and both losses from csrc/infillhead.hip where ``model.ends_route`` is "hip";
    ``train_step``, ``validate`` and ``train_epoch`` return the same fp32 device tensors either way."""

    def __init__(self, sd, opt, lr=1e-4, milestones=(30, 40), gamma=0.1, dropout=None, lw_pose=1.0, lw_accel=0.1, device="cuda:0", fused_ends=False):
        self.model = TrainableConditionalMInfiller(sd, opt, dropout, device, fused_ends).train()
        self.fused_ends = bool(fused_ends)
        self.names = [k for k, _ in self.model.named_parameters()]
        self.optimizer = ops.FusedAdam([p for _, p in self.model.named_parameters()], lr=lr)
        self.lr0, self.milestones, self.gamma, self.lw = float(lr), tuple(milestones), float(gamma), (float(lw_pose), float(lw_accel))

    def set_step(self, epoch):
        lr = multistep_lr(self.lr0, self.milestones, self.gamma, epoch)
        self.optimizer.lrs = [lr] * len(self.optimizer.lrs)
        return lr

    def train_step(self, batch, seed=0):
        """-> (loss (), sep_loss (2,) = [loss_pos, loss_accel]) device tensors of the objective BEFORE the update"""
        dev = self.model.dev
        self.optimizer.zero_grad()
        if self.fused_ends:
            loss, loss_pos, loss_accel, _ = self.model.loss(batch, seed, self.lw)
            loss.backward()
            self.optimizer.step()
            return loss.detach(), torch.stack([loss_pos.detach(), loss_accel.detach()])
        pred = self.model(batch["data_smpl"], batch["mask_smpl"], batch["data_obj"], batch["mask_obj"], seed)
        loss_accel, loss_pos = motion_losses(batch["gt_obj"].to(dev).float(), pred, *self.lw)
        loss = loss_pos + loss_accel
        loss.backward()
        self.optimizer.step()
        return loss.detach(), torch.stack([loss_pos.detach(), loss_accel.detach()])

    def _loss(self, batch, seed=None):
        if self.fused_ends:
            loss, loss_pos, loss_accel, _ = self.model.loss(batch, seed, self.lw)
            return loss, torch.stack([loss_pos, loss_accel])
        pred = self.model(batch["data_smpl"], batch["mask_smpl"], batch["data_obj"], batch["mask_obj"], seed)
        loss_accel, loss_pos = motion_losses(batch["gt_obj"].to(self.model.dev).float(), pred, *self.lw)
        return loss_pos + loss_accel, torch.stack([loss_pos, loss_accel])

    def train_epoch(self, data, epoch, seed, batch_size, world=1, rank=0):
        """one epoch over ``data`` (``infill_data.HVOPClipData``): ``set_step(epoch)``, this rank's clip order from ``training.distributed_indices``, and per
        batch of ``batch_size`` clips (a shorter tail is dropped, as the reference's loader drops it) one ``data.batch`` and one ``train_step`` whose dropout seed
        is ``batch_seed(seed, epoch, batch number)``.  The order is checked and uploaded once, before the loop; nothing waits on the host.
        -> (sum of the losses (), sum of [loss_pos, loss_accel] (2,), number of batches): device tensors and an int."""
        from .training import distributed_indices
        batch_size = int(batch_size)
        if batch_size < 1:
            raise L.VtError(f"train_epoch: batch_size = {batch_size}")
        self.set_step(epoch)
        self.model.train()
        order = distributed_indices(len(data), world, rank, epoch, seed)
        n = len(order) // batch_size
        dev = self.model.dev
        total, sep = torch.zeros((), device=dev), torch.zeros(2, device=dev)
        if n == 0:
            return total, sep, 0
        order = data._indices(order[:n * batch_size])
        for i in range(n):
            loss, s = self.train_step(data.batch(order[i * batch_size:(i + 1) * batch_size], seed, epoch), batch_seed(seed, epoch, i))
            total += loss; sep += s
        return total, sep, n

    def validate(self, data, batch_size, max_batches=1024, seed=0):
        """``compute_val_loss`` (trainer.py:321-346) with the infiller's cap of 1024 batches (trainer_infiller.py:55-57): eval mode, no gradients, a seeded shuffle
        of the clips (the reference's is unseeded), the last short batch kept as its loader keeps it; the model is back in train mode afterwards.
        -> (mean loss (), mean [loss_pos, loss_accel] (2,)) device tensors, the means over the batches; (inf, inf) without a batch."""
        from .training import distributed_indices
        batch_size = int(batch_size)
        if batch_size < 1:
            raise L.VtError(f"validate: batch_size = {batch_size}")
        order = distributed_indices(len(data), 1, 0, 0, seed, drop_last=False)
        n = min(int(max_batches), -(-len(order) // batch_size))
        dev = self.model.dev
        total, sep = torch.zeros((), device=dev), torch.zeros(2, device=dev)
        if n <= 0:
            return total + float("inf"), sep + float("inf")
        order = data._indices(order[:n * batch_size])
        self.model.eval()
        try:
            with torch.no_grad():
                for i in range(n):
                    loss, s = self._loss(data.batch(order[i * batch_size:(i + 1) * batch_size], seed, 0))
                    total += loss; sep += s
        finally:
            self.model.train()
        return total / n, sep / n

    def state_dict(self):
        return self.model.state_dict()

    def export(self):
        return self.model.export()


def batch_seed(seed: int, epoch: int, batch: int) -> int:
    """the 64-bit dropout seed of batch ``batch`` of epoch ``epoch``: two hashes of (seed, site 200 | 201, epoch << 32 | batch)"""
    e = ((int(epoch) & _M32) << 32) | (int(batch) & _M32)
    return dropout_hash(seed, 200, e) | (dropout_hash(seed, 201, e) << 32)
