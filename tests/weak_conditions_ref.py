"""CPU restatements of the two weak conditions of the Backbone (test infrastructure, not a test module): a head-rotation speed
embedding PER FRAME in the time embedding and a face-region map behind conv_in.  Built on oracle.unet_ref without editing it:
`unet_forward` runs with two of its module-level functions replaced (unittest.mock.patch.object) by the versions below.

Design choices of the product (the reference gives no runnable arithmetic for either path), restated here in plain torch:
  speed   emb[b, f] = time_emb[b] (+ class_emb[b]) + speed[b, f]; every ResnetBlock3D projects it per frame,
          time_emb_proj(silu(emb[b, f])), and adds it to / modulates with it the frame's pixels (resnet.py:186-195 with the temb
          broadcast (B, C, F, 1, 1) instead of (B, C, 1, 1, 1)); the GroupNorms stay joint over the F frames.
  face    conv_in(sample)[b, :, f] + face_map for every b and f; face_map = FaceRegionController(mask)
          (train_stage_3_speedlayers.py:57-76: four 3x3 convs, ReLU between them).
"""
from __future__ import annotations

from unittest import mock

import torch
import torch.nn.functional as F

from oracle import unet_ref as U

SS = dict(resnet_time_scale_shift="scale_shift")


def face_map(ctl_sd, mask):
    """FaceRegionController.forward on a (1, 1, h, w) mask -> (1, C0, h, w): encoder.0 / 2 / 4 / 6 are the convs, ReLU behind the first three"""
    x = mask
    for k in (0, 2, 4, 6):
        x = F.conv2d(x, ctl_sd[f"encoder.{k}.weight"], ctl_sd[f"encoder.{k}.bias"], padding=1)
        if k != 6:
            x = F.relu(x)
    return x


def pooled_mask(mask, threshold=None):
    """pixel-size (H, W) map -> (1, 1, H / 8, W / 8): the 8 x 8 area mean, of (mask > threshold) when one is given"""
    m = mask.float()
    if threshold is not None:
        m = (m > threshold).float()
    return F.avg_pool2d(m[None, None], 8)


def _resnet_block(speed, scale_shift):
    """ResnetBlock3D.forward with a per-frame embedding: emb (B, D) from unet_forward, speed (B, F, D) or None"""

    def resnet_block(sd, p, x, emb, groups, eps, scale=1.0):
        e = emb[:, None, :] if speed is None else emb[:, None, :] + speed                      # (B, 1 | F, D)
        t = U._lin(sd, p + ".time_emb_proj", F.silu(e)).permute(0, 2, 1)[:, :, :, None, None]     # (B, C | 2C, 1 | F, 1, 1)
        h = F.silu(U.group_norm_5d(sd, p + ".norm1", x, groups, eps))
        h = U._conv_per_frame(sd, p + ".conv1", h)
        if scale_shift:
            sc_, sh_ = t.chunk(2, dim=1)
            h = U.group_norm_5d(sd, p + ".norm2", h, groups, eps) * (1 + sc_) + sh_
        else:
            h = U.group_norm_5d(sd, p + ".norm2", h + t, groups, eps)
        h = U._conv_per_frame(sd, p + ".conv2", F.silu(h))
        if (p + ".conv_shortcut.weight") in sd:
            x = U._conv_per_frame(sd, p + ".conv_shortcut", x, padding=0)
        return (x + h) / scale
    return resnet_block


def _conv_with_face(face):
    plain = U._conv_per_frame

    def _conv_per_frame(sd, p, x, stride=1, padding=1):
        y = plain(sd, p, x, stride=stride, padding=padding)
        if p == "conv_in" and face is not None:
            y = y + face[:, :, None]                      # (1, C0, 1, h, w): every batch row, every frame
        return y
    return _conv_per_frame


def unet_forward(sd, cfg, sample, timestep, ctx, *, speed=None, face=None, **kw):
    """oracle.unet_ref.unet_forward with speed (B, F, 4*C0) per frame and / or face (1, C0, h, w) behind conv_in"""
    scale_shift = cfg.get("resnet_time_scale_shift", "default") == "scale_shift"
    conv = _conv_with_face(face)
    with mock.patch.object(U, "resnet_block", _resnet_block(speed, scale_shift)), mock.patch.object(U, "_conv_per_frame", conv):
        return U.unet_forward(sd, cfg, sample, timestep, ctx, **kw)
