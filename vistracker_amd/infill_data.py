"""HVOP-Net training, the data set: clips drawn and assembled on the device.  Mirror of

    data.traindata_mfiller.TrainDataMotionFiller.load_data / __len__ / gen_masks / get_smpl_input / get_obj_input      (traindata_mfiller.py:77-157, 222-296)
    data.traindata_cmfiller.TrainDataCMotionFiller.get_item                                                           (traindata_cmfiller.py:19-66)

The packed sequences are uploaded once; a batch is two launches on the current stream (``ops.clip_draw``, ``ops.clip_build``; kernels: csrc/clipdata.hip) and
no host wait.  The reference's random decisions come from numpy's global generator in 32 loader workers and are not reproducible; here a decision is a function
of (seed, epoch, global clip index) through the hash of csrc/dropout_hash.h, so an epoch is the same on every run and for every batch size and rank layout.
``kinect``: {date: (world2local_R (4, 3, 3), world2local_t (4, 3))}; reading BEHAVE's calibration folders is not here."""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib as L
from . import ops

OBJ_DIM = {"6d": 6, "9d": 9}
PACKED_KEYS = ("poses", "trans", "root_joints", "obj_angles", "obj_trans")


class HVOPClipData:
    def __init__(self, tables, w2c_R, w2c_t, clip_start, clip_date, n_seq, dates, clip_len, start_fr_min, start_fr_max, min_drop_len, max_drop_len, obj_repre,
                 aug_num, multi_kinects, phase, device):
        self.tables, self.w2c_R, self.w2c_t, self.dates = tables, w2c_R, w2c_t, list(dates)
        self.clip_start_host, self.clip_date_host, self.n_seq = np.asarray(clip_start, np.int32), np.asarray(clip_date, np.int32), int(n_seq)
        self.dev = torch.device(device)
        self.clip_start, self.clip_date = torch.as_tensor(self.clip_start_host).to(self.dev), torch.as_tensor(self.clip_date_host).to(self.dev)
        self.clip_len, self.obj_repre, self.obj_dim, self.aug_num = int(clip_len), obj_repre, OBJ_DIM[obj_repre], int(aug_num)
        self.draw_args = (self.clip_len, bool(multi_kinects), int(min_drop_len), int(max_drop_len), int(start_fr_min), int(start_fr_max), self.aug_num)
        self.multi_kinects, self.phase = bool(multi_kinects), phase

    # ---- construction ---------------------------------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_packed(cls, packed, names, clip_len, window, start_fr_min=10, start_fr_max=50, min_drop_len=10, max_drop_len=40, obj_repre="9d", aug_num=0,
                    multi_kinects=False, kinect=None, phase="train", smpl_repre="params", device="cuda:0"):
        """``packed``: the dicts of the packed sequence files (``packing.load``), ``names``: their file names -- the date of a sequence is the first ``_`` field of
        its base name (traindata_mfiller.py:94).  Sequences shorter than ``clip_len`` are skipped; a clip starts every ``window`` frames of a sequence."""
        if smpl_repre != "params":
            raise L.VtError(f"HVOPClipData: smpl_repre {smpl_repre!r}; only 'params' (the joint representations are not here)")
        if obj_repre not in OBJ_DIM:
            raise L.VtError(f"HVOPClipData: obj_repre {obj_repre!r}; one of {sorted(OBJ_DIM)}")
        clip_len, window = int(clip_len), int(window)
        if clip_len < 1 or window < 1 or len(packed) != len(names):
            raise L.VtError(f"HVOPClipData: clip_len {clip_len}, window {window}, {len(packed)} sequences with {len(names)} names")
        cols = {k: [] for k in PACKED_KEYS}
        clip_start, clip_dates, n_seq, offset = [], [], 0, 0
        for d, name in zip(packed, names):
            n = len(d["frames"]) if "frames" in d else len(d["poses"])
            if n < clip_len:
                continue
            date = os.path.basename(str(name)).split("_")[0]
            for i in range(0, n - clip_len + 1, window):
                clip_start.append(i + offset); clip_dates.append(date)
            n_seq += 1; offset += n
            pose = np.asarray(d["poses"])
            if pose.shape != (n, 156):
                raise L.VtError(f"HVOPClipData: {name}: poses {pose.shape}, ({n}, 156) SMPL-H expected")
            cols["poses"].append(np.concatenate([pose[:, :69], pose[:, 111:114]], 1))
            for k in PACKED_KEYS[1:]:
                a = np.asarray(d[k])
                if a.shape != (n, 3):
                    raise L.VtError(f"HVOPClipData: {name}: {k} {a.shape}, ({n}, 3) expected (obj_angles are rotation vectors)")
                cols[k].append(a)
        if not clip_start:
            raise L.VtError(f"HVOPClipData: no sequence has {clip_len} frames")
        if offset >= 2 ** 31:
            raise L.VtError(f"HVOPClipData: {offset} frames; frame indices are int32")
        # the decisions' ranges are refused here, before any launch (ops.clip_draw refuses them again)
        if min(clip_len - int(max_drop_len), int(start_fr_max)) <= int(start_fr_min) or int(max_drop_len) < int(min_drop_len) or int(min_drop_len) < 0 or int(start_fr_min) < 0:
            raise L.VtError(f"HVOPClipData: no start frame in [{start_fr_min}, min({clip_len} - {max_drop_len}, {start_fr_max})) for drops [{min_drop_len}, {max_drop_len}]")
        if not 0 <= int(aug_num) <= 64 or (int(aug_num) > 0 and clip_len - int(aug_num) <= 0):
            raise L.VtError(f"HVOPClipData: aug_num {aug_num} with clip_len {clip_len}")
        dates = sorted(set(clip_dates))
        if multi_kinects:
            missing = [x for x in dates if x not in (kinect or {})]
            if missing:
                raise L.VtError(f"HVOPClipData: multi_kinects needs the world-to-local transforms of {missing}")
            R = np.stack([np.asarray(kinect[x][0], dtype=np.float32).reshape(4, 3, 3) for x in dates])
            t = np.stack([np.asarray(kinect[x][1], dtype=np.float32).reshape(4, 3) for x in dates])
        else:
            R, t = np.tile(np.eye(3, dtype=np.float32), (len(dates), 4, 1, 1)), np.zeros((len(dates), 4, 3), np.float32)
        dev = torch.device(device)
        up = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev).contiguous()          # noqa: E731
        tables = {"poses": up(np.concatenate(cols["poses"])), "trans": up(np.concatenate(cols["trans"])), "roots": up(np.concatenate(cols["root_joints"])),
                  "obj_angles": up(np.concatenate(cols["obj_angles"])), "obj_trans": up(np.concatenate(cols["obj_trans"]))}
        return cls(tables, up(R), up(t), clip_start, [dates.index(x) for x in clip_dates], n_seq, dates, clip_len, start_fr_min, start_fr_max, min_drop_len,
                   max_drop_len, obj_repre, aug_num, multi_kinects, phase, dev)

    @classmethod
    def from_paths(cls, paths, clip_len, window, **kw):
        from . import packing
        paths = list(paths)
        return cls.from_packed([packing.load(p) for p in paths], paths, clip_len, window, **kw)

    # ---- access ---------------------------------------------------------------------------------------------------------------------------------------------
    @property
    def num_clips(self):
        return len(self.clip_start_host)

    def __len__(self):
        """traindata_mfiller.py:153-157: the clips in the 'train' phase, the sequences otherwise"""
        return self.num_clips if self.phase == "train" else self.n_seq

    def _indices(self, indices):
        """-> (B,) int32 device tensor.  A host sequence is checked against the clip table and raises; a device tensor cannot be checked without a host wait: the
        caller promises its range (``train_epoch`` slices a checked order), and entries outside it are brought into it on the device."""
        if torch.is_tensor(indices) and indices.is_cuda:
            if indices.dim() != 1 or indices.numel() < 1 or indices.dtype not in (torch.int32, torch.int64):
                raise L.VtError("HVOPClipData: indices is a (B,) integer tensor, B >= 1")
            return indices.to(self.dev).clamp(0, self.num_clips - 1).to(torch.int32).contiguous()
        idx = np.asarray(indices.numpy() if torch.is_tensor(indices) else indices)
        if idx.ndim != 1 or idx.size < 1 or idx.dtype.kind not in "iu":
            raise L.VtError("HVOPClipData: indices is a (B,) integer sequence, B >= 1")
        if idx.min() < 0 or idx.max() >= self.num_clips:
            raise L.VtError(f"HVOPClipData: clip index out of range [0, {self.num_clips})")
        return torch.as_tensor(idx.astype(np.int32)).to(self.dev)

    def draw(self, indices, seed, epoch):
        """the decisions of the clips ``indices`` in epoch ``epoch``: kid, drop_len, start_fr (B,), aug_start (B, aug_num) int32 on the device"""
        with torch.cuda.device(self.dev):
            return ops.clip_draw(self._indices(indices), seed, epoch, *self.draw_args)

    def build(self, indices, decisions, seed=0, epoch=0, noise=None):
        """the batch dict of ``get_item`` stacked over the clips, with ``drop_start`` and ``drop_len`` (B,) int32; ``noise``: tests only"""
        with torch.cuda.device(self.dev):
            idx = self._indices(indices)
            start, date = self.clip_start.index_select(0, idx.long()), self.clip_date.index_select(0, idx.long())
            out = ops.clip_build(self.tables, self.w2c_R, self.w2c_t, start, date, decisions, self.clip_len, self.obj_dim, noise, idx, seed, epoch)
        out["drop_start"], out["drop_len"] = decisions["start_fr"], decisions["drop_len"]
        return out

    def batch(self, indices, seed, epoch):
        """``draw`` then ``build``: two launches on the current stream; what ``HVOPTrainer.train_step`` takes"""
        with torch.cuda.device(self.dev):
            idx = self._indices(indices)
            return self.build(idx, ops.clip_draw(idx, seed, epoch, *self.draw_args), seed, epoch)
