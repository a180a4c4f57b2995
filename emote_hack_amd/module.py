"""The torch-module-like surface of every model class of this package, written once.

Weights are CALLER-LOADED: `load_state_dict` takes the checkpoint's key names and keeps f32 masters in the checkpoint's layout (`_master`);
`.to(device, dtype)` packs them into the layouts the kernels read (`_w`).  There is no CPU execution path: `_need()` is the gate in
front of every forward.  A subclass declares `_shapes` and writes `_pack_weights()`; `_remap_keys`, `_tolerated` and
`_strict_unexpected` carry what differs between the classes' checkpoints.
"""
from __future__ import annotations

import torch

from . import ops
from ._lib import EmoHipError


def round_up(x, m):
    return (x + m - 1) // m * m


def ln_fold_weights(wt, b, gamma, beta, dtp):
    """(W, bias) of a Linear behind a LayerNorm with affine (gamma, beta) -> (W * gamma rounded to the compute dtype, its row sums,
    bias + W . beta): LN(x) W^T + b = rstd (x W'^T - mean colsum) + b' (unet.FOLD_LAYERNORM; ops.gemm(ln=...))."""
    g_, be = gamma.float(), beta.float()
    wt = wt.reshape(wt.shape[0], -1).float()
    wp = (wt * g_[None, :]).to(dtp)
    bp = wt.to(dtp).float() @ be
    if b is not None:
        bp = bp + b.float()
    return wp.contiguous(), wp.float().sum(1).contiguous(), bp.contiguous()


class HipModule:
    _tolerated = frozenset()        # keys a checkpoint may carry that the model has no use for (non-persistent buffers and the like)
    _strict_unexpected = True       # strict=True raises on unexpected keys too (torch's rule)

    def __init__(self, shapes):
        self._shapes = shapes
        self._master = None         # f32 tensors in the checkpoint's layout, wherever load_state_dict / _pack_weights leave them
        self._w = None              # packed tensors
        self.dtype, self.device = torch.float32, torch.device("cpu")

    def eval(self):
        return self

    def requires_grad_(self, *_):
        return self

    def cuda(self):
        return self.to("cuda")

    def __call__(self, *args, **kwargs):
        return self.forward(*args, **kwargs)

    def state_dict(self):
        if self._master is None:
            raise EmoHipError("no weights loaded")
        return {k: v.detach().cpu() for k, v in self._master.items()}

    def _remap_keys(self, sd):
        """older spellings of a checkpoint's keys -> the ones `_shapes` lists (sd is the caller's dict copied: edit and return it)"""
        return sd

    def load_state_dict(self, sd, strict=True):
        """torch semantics: returns (missing, unexpected) relative to the INCOMING dict; strict raises on either.  Partial loads
        accumulate, and the model (re-)packs whenever the merged master is complete."""
        sd = self._remap_keys(dict(sd))
        missing = [k for k in self._shapes if k not in sd]
        unexpected = [k for k in sd if k not in self._shapes and k not in self._tolerated]
        if strict and (missing or (unexpected and self._strict_unexpected)):
            raise RuntimeError(f"Error(s) in loading state_dict: {len(missing)} missing key(s) {missing[:5]}, "
                               f"{len(unexpected)} unexpected key(s) {unexpected[:5]}")
        for k, shp in self._shapes.items():
            if k in sd and tuple(sd[k].shape) != tuple(shp):
                raise RuntimeError(f"size mismatch for {k}: {tuple(sd[k].shape)} vs {tuple(shp)}")
        master = dict(self._master or {})
        for k in self._shapes:
            if k in sd:
                master[k] = sd[k].detach().to(torch.float32)
        self._master, self._w = master, None        # packed weights are stale from here on
        self._pack()
        return missing, unexpected

    def to(self, *args, **kwargs):
        device, dtype = kwargs.get("device"), kwargs.get("dtype")
        for a in args:
            if isinstance(a, torch.dtype):
                dtype = a
            elif a is not None:
                device = a
        if dtype is not None:
            ops.dt(dtype)
            self.dtype = dtype
        if device is not None:
            self.device = torch.device(device)
        self._pack()
        return self

    def _absent_keys(self):
        return [k for k in self._shapes if self._master is None or k not in self._master]

    def _pack(self):
        if self.device.type != "cuda" or self._master is None or self._absent_keys():
            return      # packed on the first .to('cuda') after every key has a value
        self._w = self._pack_weights()

    def _pack_weights(self):
        raise NotImplementedError

    def _need(self):
        if self._w is None:
            raise EmoHipError(f"{type(self).__name__}: load_state_dict + .to('cuda') first (weights are caller-loaded; there is no CPU execution path)")
