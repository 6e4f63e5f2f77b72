"""LSKNet backbones (Large Selective Kernel Network, ICCV 2023) behind the reference's constructor arguments and
parameter names (python/jdet/models/backbones/lsknet.py: Mlp L71-107, LSKblock L111-133, SpatialAttention L135-151, Block
L154-193, OverlapPatchEmbed L196-237, LSKNet L240-328, LSKNet_t / LSKNet_s L352-374), so a reference checkpoint maps 1:1:
`patch_embed{i}.proj/norm`, `block{i}.{j}.norm1 / attn.proj_1 / attn.spatial_gating_unit.{conv0, conv_spatial, conv1, conv2,
conv_squeeze, conv} / attn.proj_2 / norm2 / mlp.{fc1, dwconv.dwconv, fc2} / layer_scale_1 / layer_scale_2`, `norm{i}`.

Own structure.  The whole forward stays channels-last.  The three depthwise convolutions of a block -- the 5x5, the 7x7
dilation-3 (a 19x19 footprint) and the 3x3 + bias + GELU over the MLP's hidden map, 8x wider than the stage -- run on
csrc/dwconv.hip (ops/dwconv.py), and the selection step (channel mean / max of the two branches, a 2 -> 2 7x7 convolution,
a sigmoid, the two-way weighted sum) on csrc/lsk_select.hip (ops/lsk_select.py) without the concatenations.  The 1x1
convolutions, the training-mode BatchNorms and the stage-end LayerNorm -- taken over the channels-last view, no copy --
stay with the library.  Every op takes its composed torch form on other devices, dtypes and layouts.

As in the reference there is no `norm_eval`: the BatchNorms follow train() / eval().  `layer_scale_*` are trainable
(every array attribute of a module is, in the reference's framework)."""
import math
import os

import torch
from torch import nn

from jdet_amd.ops.dwconv import dwconv
from jdet_amd.ops.lsk_select import lsk_select, lsk_squeeze
from jdet_amd.utils.registry import BACKBONES

__all__ = ["LSKNet", "LSKNet_t", "LSKNet_s", "DropPath"]


def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


def _init_weights(m):
    """the reference's `_init_weights`: fan-out normal for convolutions, zero biases; norm layers at (1, 0)"""
    if isinstance(m, nn.Linear):
        nn.init.trunc_normal_(m.weight, std=.02)
        if m.bias is not None:
            nn.init.constant_(m.bias, 0)
    elif isinstance(m, nn.LayerNorm):
        nn.init.constant_(m.bias, 0)
        nn.init.constant_(m.weight, 1.0)
    elif isinstance(m, nn.Conv2d):
        fan_out = m.kernel_size[0] * m.kernel_size[1] * m.out_channels // m.groups
        nn.init.normal_(m.weight, 0.0, math.sqrt(2.0 / fan_out))
        if m.bias is not None:
            nn.init.constant_(m.bias, 0)


class DropPath(nn.Module):
    """stochastic depth: in training a sample's residual branch is dropped with probability p, the others scaled by
    1 / (1 - p)"""

    def __init__(self, p=0.0):
        super().__init__()
        self.p = float(p)

    def forward(self, x):
        if self.p == 0.0 or not self.training:
            return x
        keep = 1.0 - self.p
        mask = torch.empty((x.shape[0],) + (1,) * (x.dim() - 1), dtype=x.dtype, device=x.device).bernoulli_(keep)
        return x * (mask / keep)

    execute = forward


def _dw(conv, x, act=None):
    """a depthwise nn.Conv2d (stride 1) through ops/dwconv"""
    return dwconv(_cl(x), conv.weight, conv.bias, conv.padding, conv.dilation, act)


class DWConv(nn.Module):
    def __init__(self, dim=768):
        super().__init__()
        self.dwconv = nn.Conv2d(dim, dim, 3, 1, 1, bias=True, groups=dim)

    def forward(self, x, act=None):
        return _dw(self.dwconv, x, act)

    execute = forward


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Conv2d(in_features, hidden_features, 1)
        self.dwconv = DWConv(hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Conv2d(hidden_features, out_features, 1)
        self.drop = nn.Dropout(drop)
        self.apply(_init_weights)

    def forward(self, x):
        x = self.fc1(x)
        if type(self.act) is nn.GELU and self.act.approximate == "none":
            x = self.dwconv(x, act="gelu")                   # the 3x3, its bias and the GELU in one pass
        else:
            x = self.act(self.dwconv(x))
        x = self.drop(x)
        x = self.fc2(x)
        return self.drop(x)

    execute = forward


class LSKblock(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.conv0 = nn.Conv2d(dim, dim, kernel_size=5, padding=2, groups=dim)
        self.conv_spatial = nn.Conv2d(dim, dim, kernel_size=7, stride=1, padding=9, groups=dim, dilation=3)
        self.conv1 = nn.Conv2d(dim, dim // 2, kernel_size=1)
        self.conv2 = nn.Conv2d(dim, dim // 2, kernel_size=1)
        self.conv_squeeze = nn.Conv2d(2, 2, kernel_size=7, padding=3)
        self.conv = nn.Conv2d(dim // 2, dim, kernel_size=1)

    def forward(self, x):
        attn1 = _dw(self.conv0, x)
        attn2 = _dw(self.conv_spatial, attn1)
        attn1 = _cl(self.conv1(attn1))
        attn2 = _cl(self.conv2(attn2))
        agg = lsk_squeeze(attn1, attn2)
        sig = _cl(self.conv_squeeze(agg).sigmoid())
        attn = self.conv(lsk_select(attn1, attn2, sig))
        return x * attn

    execute = forward


class SpatialAttention(nn.Module):
    def __init__(self, d_model):
        super().__init__()
        self.proj_1 = nn.Conv2d(d_model, d_model, 1)
        self.activation = nn.GELU()
        self.spatial_gating_unit = LSKblock(d_model)
        self.proj_2 = nn.Conv2d(d_model, d_model, 1)

    def forward(self, x):
        shortcut = x
        x = self.activation(self.proj_1(x))
        x = self.spatial_gating_unit(x)
        return self.proj_2(x) + shortcut

    execute = forward


class Block(nn.Module):
    def __init__(self, dim, mlp_ratio=4., drop=0., drop_path=0., act_layer=nn.GELU):
        super().__init__()
        self.norm1 = nn.BatchNorm2d(dim)
        self.attn = SpatialAttention(dim)
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.norm2 = nn.BatchNorm2d(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self.layer_scale_1 = nn.Parameter(1e-2 * torch.ones(dim))
        self.layer_scale_2 = nn.Parameter(1e-2 * torch.ones(dim))
        self.apply(_init_weights)

    def forward(self, x):
        x = x + self.drop_path(self.layer_scale_1[:, None, None] * self.attn(self.norm1(x)))
        return x + self.drop_path(self.layer_scale_2[:, None, None] * self.mlp(self.norm2(x)))

    execute = forward


class OverlapPatchEmbed(nn.Module):
    """image to patch embedding: a strided convolution whose windows overlap, then BatchNorm"""

    def __init__(self, img_size=1024, patch_size=7, stride=4, in_chans=3, embed_dim=768):
        super().__init__()
        img_size = (img_size, img_size) if isinstance(img_size, (int, float)) else tuple(img_size)
        patch_size = (patch_size, patch_size) if isinstance(patch_size, (int, float)) else tuple(patch_size)
        self.img_size, self.patch_size = img_size, patch_size
        self.H, self.W = img_size[0] // patch_size[0], img_size[1] // patch_size[1]
        self.num_patches = self.H * self.W
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=stride,
                              padding=(patch_size[0] // 2, patch_size[1] // 2))
        self.norm = nn.BatchNorm2d(embed_dim)
        self.apply(_init_weights)

    def forward(self, x):
        return self.norm(self.proj(x))

    execute = forward


@BACKBONES.register_module()
class LSKNet(nn.Module):
    def __init__(self, img_size=1024, in_chans=3, num_classes=10, embed_dims=[64, 128, 256, 512],
                 mlp_ratios=[4, 4, 4, 4], drop_rate=0., drop_path_rate=0., norm_layer=nn.LayerNorm,
                 depths=[3, 4, 6, 3], num_stages=4, flag=False, out_indices=(0, 1, 2)):
        super().__init__()
        if flag is False:
            self.num_classes = num_classes
        self.depths = depths
        self.num_stages = num_stages
        self.out_indices = tuple(out_indices)
        dpr = torch.linspace(0, drop_path_rate, sum(depths)).tolist()        # stochastic depth decay rule
        cur = 0
        for i in range(num_stages):
            patch_embed = OverlapPatchEmbed(img_size=img_size if i == 0 else img_size // (2 ** (i + 1)),
                                            patch_size=7 if i == 0 else 3, stride=4 if i == 0 else 2,
                                            in_chans=in_chans if i == 0 else embed_dims[i - 1], embed_dim=embed_dims[i])
            block = nn.ModuleList([Block(dim=embed_dims[i], mlp_ratio=mlp_ratios[i], drop=drop_rate,
                                         drop_path=dpr[cur + j]) for j in range(depths[i])])
            cur += depths[i]
            setattr(self, "patch_embed%d" % (i + 1), patch_embed)
            setattr(self, "block%d" % (i + 1), block)
            setattr(self, "norm%d" % (i + 1), norm_layer(embed_dims[i]))
        self.apply(_init_weights)

    def freeze_patch_emb(self):
        for p in self.patch_embed1.parameters():
            p.requires_grad = False

    def forward_features(self, x):
        outs = []
        x = _cl(x)
        for i in range(self.num_stages):
            x = _cl(getattr(self, "patch_embed%d" % (i + 1))(x))
            for blk in getattr(self, "block%d" % (i + 1)):
                x = blk(x)
            # the reference flattens to (B, H W, C) for the norm and back: on a channels-last map that is a view
            x = _cl(getattr(self, "norm%d" % (i + 1))(_cl(x).permute(0, 2, 3, 1)).permute(0, 3, 1, 2))
            if i in self.out_indices:
                outs.append(x)
        return outs

    def forward(self, x):
        return self.forward_features(x)

    execute = forward


def _load_pretrained(model, pretrained):
    """a checkpoint file of the reference's names (a pickled dict, or one under "model" / "state_dict"); a path that is
    not present leaves the init in place, as the ResNets do (no fetch)"""
    if not isinstance(pretrained, str) or not os.path.isfile(pretrained):
        return model
    import pickle
    with open(pretrained, "rb") as f:
        data = pickle.load(f)
    for key in ("model", "state_dict"):
        if isinstance(data, dict) and key in data:
            data = data[key]
    own = model.state_dict()
    state = {k: torch.as_tensor(v).reshape(own[k].shape) for k, v in data.items()
             if k in own and own[k].numel() == torch.as_tensor(v).numel()}
    model.load_state_dict(state, strict=False)
    return model


@BACKBONES.register_module()
def LSKNet_t(pretrained=False, **kwargs):
    model = LSKNet(embed_dims=[32, 64, 160, 256], mlp_ratios=[8, 8, 4, 4], norm_layer=nn.LayerNorm, depths=[3, 3, 5, 2],
                   **kwargs)
    return _load_pretrained(model, pretrained)


@BACKBONES.register_module()
def LSKNet_s(pretrained=False, **kwargs):
    model = LSKNet(embed_dims=[64, 128, 320, 512], mlp_ratios=[8, 8, 4, 4], norm_layer=nn.LayerNorm, depths=[2, 2, 4, 2],
                   **kwargs)
    return _load_pretrained(model, pretrained)
