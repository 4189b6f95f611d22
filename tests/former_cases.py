"""The inputs of the HVOP-Net training tests (tests/former_model.py is the model): layer cases, and the HVOP-Net option namespace with seeded weights."""
import zlib
from types import SimpleNamespace

import numpy as np

import former_model as FM

SHAPES = ((32, 2, 64), (128, 4, 256), (160, 1, 256))        # (D, H, F): object, SMPL and joint encoder of config/cmf-k4-lrot.json
TS = (1, 15, 16, 17, 33, 180)                                # below / at / above one tile, two tiles + 1, the workload (11 x 16 + 4)


def _label(B, T, kind):
    """the mask a case really runs with: at T = 1 no kind can mask anything (a clip with every key masked is outside the contract)"""
    m = FM.make_mask(B, T, kind)
    return kind if m is not None and m.any() else "none"


def layer_cases():
    """every T x shape once with B = 3 (B = 1 at T = 180 of the two wide shapes keeps the float64 model quick), masks and activations cycling through them"""
    out = []
    for i, T in enumerate(TS):
        for j, (D, H, F) in enumerate(SHAPES):
            n = i * len(SHAPES) + j
            B = 1 if (T == 180 and D > 32) or n % 4 == 1 else 3
            out.append(dict(id=f"T{T}-D{D}-B{B}-{FM.ACTS[n % 3]}-{_label(B, T, FM.MASKS[n % 4])}", B=B, T=T, D=D, H=H, F=F, act=FM.ACTS[n % 3], mask=FM.MASKS[n % 4],
                            seed=100 + n))
    return out


def dropout_cases():
    """the hashed masks at the narrow shape (two probabilities x two seeds) and once at each wide shape: four heads, and head width 160 at the workload's T"""
    out = [dict(id=f"drop-D32-p{p}-{seed:x}", B=3, T=17, D=32, H=2, F=64, act="gelu", mask="block", seed=55, p=p, dseed=seed)
           for p in (0.05, 0.5) for seed in (3, 0x9abcdef012345678)]
    out.append(dict(id="drop-D128-H4-T33", B=2, T=33, D=128, H=4, F=256, act="gelu", mask="block", seed=56, p=0.05, dseed=0x1122334455667788))
    out.append(dict(id="drop-D160-H1-T180", B=1, T=180, D=160, H=1, F=256, act="gelu", mask="block", seed=57, p=0.5, dseed=11))
    return out


def small_cases():
    """every mask x activation at the smallest ragged two-tile shape"""
    return [dict(id=f"{a}-{m}", B=3, T=17, D=32, H=2, F=64, act=a, mask=m, seed=300 + 4 * i + j) for i, a in enumerate(FM.ACTS) for j, m in enumerate(FM.MASKS)]


_built = {}


def build(c, p=0.0, seed=0):
    """the case's tensors and its float64 reference with e32, computed once"""
    key = (c["id"], p, seed)
    if key not in _built:
        P = FM.make_params(c["D"], c["F"], c["seed"])
        x, pos, dy, mask = FM.make_inputs(c["B"], c["T"], c["D"], c["seed"] + 1000, c["mask"])
        g64, e32, S = FM.reference_and_e32(P, x, pos, mask, dy, c["H"], c["act"], p, seed)
        _built[key] = dict(c, P=P, x=x, pos=pos, dy=dy, m=mask, g64=g64, e32=e32, S=S, p=p, dseed=seed)
    return _built[key]


def hvop_opt(dropout=0.05):
    """the model keys of config/cmf-k4-lrot.json (data)"""
    return SimpleNamespace(clip_len=180, obj_repre="6d", dim_smpl=147, dim_obj=6, out_dim=6, num_layers_smpl=2, d_model_smpl=128, num_heads_smpl=4,
                           dim_forward_smpl=256, pre_norm_smpl=False, activation_smpl="gelu", dropout_smpl=dropout, num_layers_obj=2, d_model_obj=32, num_heads_obj=2,
                           dim_forward_obj=64, pre_norm_obj=False, activation_obj="gelu", dropout_obj=dropout, num_layers_joint=4, num_heads_joint=1,
                           dim_forward_joint=256, pre_norm_joint=False, activation_joint="gelu", dropout_joint=dropout, hidden_dims=[32])


def seeded_weights(g, seed):
    """name-seeded weights under the recorded state_dict keys and shapes of tests/golden/infill.npz"""
    sd = {}
    for n, s, d in zip(g["names"], g["shapes"], g["ndims"]):
        n = str(n); shape = tuple(int(x) for x in s[:d]); rng = np.random.default_rng([seed, zlib.crc32(n.encode())])
        if d == 2: a = rng.normal(0, 1.0 / np.sqrt(shape[-1]), shape)
        elif n.endswith(("norm1.weight", "norm2.weight", "norm.weight")): a = 1.0 + 0.05 * rng.normal(size=shape)
        else: a = 0.02 * rng.normal(size=shape)
        sd[n] = a.astype(np.float32)
    return sd


def hvop_batch(B, T, seed):
    r = np.random.RandomState(seed)
    t = np.linspace(0, 1, T)[None, :, None]
    smooth = lambda d: (np.sin(2 * np.pi * (t * r.uniform(0.5, 2, (B, 1, d)) + r.uniform(0, 1, (B, 1, d)))) * 0.5 + 0.02 * r.randn(B, T, d)).astype(np.float32)
    mask_obj = np.zeros((B, T), dtype=bool); mask_obj[:, T // 3:T // 3 + T // 4] = True
    data_obj = smooth(6); gt = data_obj.copy(); data_obj[mask_obj] = 0
    return dict(data_smpl=smooth(147), mask_smpl=np.zeros((B, T), dtype=bool), data_obj=data_obj, mask_obj=mask_obj, gt_obj=gt)
