"""The rotated, centre-cropped view of H2RBox.  Mirrors H2RBox.rotate_crop for the image tensor
(python/jdet/models/networks/h2rbox.py:L35-75).

Two routes, same values:
  device   one launch that computes only the cropped window (csrc/rotate_crop.hip: jdet_rotate_crop);
  general  the reference's tensor program: linspace grid, (n h w, 2) x (2, 2) matmul, F.grid_sample over the whole
           frame, then the slice."""
import math

import torch
import torch.nn.functional as F

from jdet_amd import _lib as L

PADDING = {"zeros": 0, "border": 1, "reflection": 2}


def crop_offsets(h, w, size):
    """(crop_h, crop_w) of L39-40"""
    return (h - size[0]) // 2, (w - size[1]) // 2


def rotate_crop_general(img, theta=0.0, size=(768, 768), padding="reflection"):
    n, c, h, w = img.shape
    crop_h, crop_w = crop_offsets(h, w, size)
    if theta != 0:
        cosa, sina = math.cos(theta), math.sin(theta)
        tf = torch.tensor([[cosa, -sina], [sina, cosa]], dtype=torch.float32, device=img.device).to(img.dtype)
        x_range = torch.linspace(-1, 1, w, dtype=img.dtype, device=img.device)
        y_range = torch.linspace(-1, 1, h, dtype=img.dtype, device=img.device)
        y, x = torch.meshgrid(y_range, x_range, indexing="ij")
        grid = torch.stack([x, y], -1).unsqueeze(0).expand(n, -1, -1, -1)
        grid = grid.reshape(-1, 2).matmul(tf).view(n, h, w, 2)
        img = F.grid_sample(img, grid, "bilinear", padding, align_corners=True)
    return img[..., crop_h:crop_h + size[0], crop_w:crop_w + size[1]]


def rotate_crop_device(img, theta=0.0, size=(768, 768), padding="reflection"):
    """jdet_rotate_crop: img (N, C, H, W) fp32 on the device -> (N, C, size_h, size_w), contiguous"""
    L.need_device(img)
    if padding not in PADDING:
        raise ValueError("padding %r: one of %s" % (padding, sorted(PADDING)))
    x = L.f32c(img)
    n, c, h, w = x.shape
    out = torch.empty((n, c, int(size[0]), int(size[1])), dtype=torch.float32, device=x.device)
    cosa, sina = (1.0, 0.0) if theta == 0 else (math.cos(theta), math.sin(theta))
    L.check(L.lib().jdet_rotate_crop(L.ptr(x), n, c, h, w, int(size[0]), int(size[1]), cosa, sina, PADDING[padding],
                                     L.ptr(out), L.stream_ptr(x)), "jdet_rotate_crop")
    return out


def rotate_crop(img, theta=0.0, size=(768, 768), padding="reflection", device_route=True):
    if device_route and img.is_cuda and img.dtype == torch.float32 and not torch.is_autocast_enabled():
        return rotate_crop_device(img, theta, size, padding)
    return rotate_crop_general(img, theta, size, padding)
