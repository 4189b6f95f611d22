"""Golden vectors of HVOP-Net training: the reference's ``TransformerV2`` and ``ConditionalMInfiller`` (config/cmf-k4-lrot.json) in TRAIN mode with every dropout
set to 0, in float64, under autograd -- output and gradients.  Build container only; writes tests/golden/former.npz (data only).

  tv2_*   one 2-layer TransformerV2 with its final norm (D 32, H 2, F 64, gelu, B 2, T 20, a masked block in clip 1): name-seeded weights (tv2_w/<key>), x, mask,
          dy, the output and the autograd gradients of every parameter (tv2_g/<key>) and of the input (tv2_dx)
  cmf_*   the whole ConditionalMInfiller at T = 20, B = 2 with the weights of tools/gen_golden_infill.py (seed 31): the batch, the prediction, the two values of
          TrainerInfiller.motion_losses (lw_pose 1, lw_accel 0.1) and the gradient of their sum to every parameter.  The network has about a million parameters
          and a committed file at most 1 MiB, so of each gradient the file keeps its sum, its largest magnitude and up to 256 elements at recorded flat indices
          (cmf_i/<key>, cmf_g/<key>, cmf_s/<key> = [sum, max |.|])."""
import os, sys, zlib
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__)); ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT); sys.path.insert(0, HERE); sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_harness as rh  # noqa: E402
torch = rh.enter_reference()
from unittest.mock import MagicMock  # noqa: E402
for m_ in ("joblib", "behave", "behave.utils", "sklearn", "sklearn.decomposition", "sklearn.neighbors", "lib_smpl", "yacs", "yacs.config", "tensorboardX"):
    sys.modules.setdefault(m_, MagicMock())
from types import SimpleNamespace  # noqa: E402
from config.config_loader import load_configs  # noqa: E402
from model import ConditionalMInfiller  # noqa: E402
from model.transformers.former_deci import TransformerV2  # noqa: E402
import former_cases as FC  # noqa: E402


def seed_weights(model, seed):
    sd = {}
    for k, v in model.state_dict().items():
        rng = np.random.default_rng([seed, zlib.crc32(k.encode())])
        if v.dim() == 2:
            a = rng.normal(0, 1.0 / np.sqrt(v.shape[-1]), tuple(v.shape))
        elif k.endswith(("norm1.weight", "norm2.weight", "norm.weight")):
            a = 1.0 + 0.05 * rng.normal(size=tuple(v.shape))
        else:
            a = 0.02 * rng.normal(size=tuple(v.shape))
        sd[k] = torch.tensor(a.astype(np.float32)).double()
    model.load_state_dict(sd)
    return sd


def no_dropout(model):
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = 0.0
    return model.double().train()


out = {}
# ---- 1. a 2-layer TransformerV2 -------------------------------------------------------------------------------------------------------------------------------
B, T, D, H, Fd = 2, 20, 32, 2, 64
net = no_dropout(TransformerV2(2, D, H, Fd, 0.05, True, "gelu"))
sd = seed_weights(net, 41)
r = np.random.RandomState(42)
f32 = lambda a: a.astype(np.float32).astype(np.float64)                       # noqa: E731
x, dy = f32(r.randn(B, T, D)), f32(r.randn(B, T, D))
mask = np.zeros((B, T), dtype=bool); mask[1, 6:13] = True
xt = torch.tensor(x, requires_grad=True)
y = net(xt, src_key_padding_mask=torch.tensor(mask))
(y * torch.tensor(dy)).sum().backward()
out.update(tv2_x=x, tv2_dy=dy, tv2_mask=mask, tv2_y=y.detach().numpy(), tv2_dx=xt.grad.numpy())
for k, p in net.named_parameters():
    out["tv2_w/" + k] = sd[k].numpy(); out["tv2_g/" + k] = p.grad.numpy()

# ---- 2. the whole ConditionalMInfiller ---------------------------------------------------------------------------------------------------------------------------
opt = load_configs("cmf-k4-lrot")
net = no_dropout(ConditionalMInfiller(opt))
seed_weights(net, 31)
batch = FC.hvop_batch(2, 20, 3)
tb = {k: torch.tensor(v) for k, v in batch.items()}
pred = net(tb["data_smpl"].double(), tb["mask_smpl"], tb["data_obj"].double(), tb["mask_obj"])
try:
    from trainer.trainer_infiller import TrainerInfiller
    la, lp = TrainerInfiller.motion_losses(SimpleNamespace(loss_weights=dict(opt.loss_weights)), tb["gt_obj"].double(), pred)
    out["cmf_loss_source"] = np.array("TrainerInfiller.motion_losses")
except Exception as e:        # noqa: BLE001 -- the trainer module needs wheels that are absent: the two lines of trainer_infiller.py:43-46 through the same torch calls
    print("trainer import failed:", repr(e)[:200])
    import torch.nn.functional as F
    gt = tb["gt_obj"].double()
    acc = lambda a: a[:, :-2, :] - 2 * a[:, 1:-1, :] + a[:, 2:, :]          # noqa: E731
    lp = F.l1_loss(pred, gt, reduction="mean") * opt.loss_weights["lw_pose"]
    la = F.l1_loss(acc(pred), acc(gt), reduction="mean") * opt.loss_weights["lw_accel"]
    out["cmf_loss_source"] = np.array("F.l1_loss as trainer_infiller.py:43-46")
(lp + la).backward()
out.update({"cmf_" + k: v for k, v in batch.items()})
out.update(cmf_pred=pred.detach().numpy(), cmf_loss_accel=np.array(float(la)), cmf_loss_pos=np.array(float(lp)))
for k, p in net.named_parameters():
    g = p.grad.numpy().ravel()
    idx = np.sort(np.random.default_rng([77, zlib.crc32(k.encode())]).choice(g.size, min(256, g.size), replace=False)).astype(np.int32)
    out["cmf_i/" + k], out["cmf_g/" + k], out["cmf_s/" + k] = idx, g[idx], np.array([g.sum(), np.abs(g).max()])
path = os.path.join(ROOT, "tests", "golden", "former.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes;", out["cmf_loss_source"], float(lp), float(la))
