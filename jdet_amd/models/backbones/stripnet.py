"""StripNet backbones (Strip R-CNN: large strip convolutions for remote-sensing detection) behind the reference's
constructor arguments and parameter names (python/jdet/models/backbones/stripnet.py: Mlp L70-97, StripBlock L99-112,
Attention L114-129, Block L131-151, OverlapPatchEmbed L153-168, StripNet L170-229, initialize_weights L232-243,
StripNet_T / StripNet_S L256-278), so a reference checkpoint maps 1:1: `patch_embed{i}.proj/norm`,
`block{i}.{j}.norm1 / attn.proj_1 / attn.spatial_gating_unit.{conv0, conv_spatial1, conv_spatial2, conv1} / attn.proj_2 /
norm2 / mlp.{fc1, dwconv.dwconv, fc2} / layer_scale_1 / layer_scale_2`, `norm{i}`.

A StripNet block is an LSKNet block whose selection step is replaced by a (k1 x k2) then a (k2 x k1) depthwise
convolution, 1 x 19 and 19 x 1 by default.  `Mlp`, `DWConv`, `OverlapPatchEmbed`, `DropPath`, the weight init and the
checkpoint loader are those of lsknet.py.

Own structure.  The whole forward stays channels-last.  `conv0` (5x5) and the MLP's 3x3 + bias + GELU run through
ops/dwconv.py, the two strips through ops/strip_conv.py (csrc/strip_conv.hip, falling to the generic depthwise kernel
where that is the measured faster one); with k1 != 1 they are no strips and go through ops/dwconv.py.  The 1x1
convolutions, the BatchNorms (which follow train() / eval(), there is no `norm_eval`) and the stage-end LayerNorm --
taken over the channels-last view, no copy -- stay with the library.

`norm_cfg` other than None is refused: the reference passes it to a `build_norm_layer` that its file never defines.
The weights are initialised by the rule of the reference file's `initialize_weights` (fan-out normal convolutions, zero
biases, LayerNorm at (1, 0)), which is `_init_weights` of lsknet.py; a `pretrained` path that is absent leaves the init
in place, nothing is fetched."""
import torch
from torch import nn

from jdet_amd.ops.strip_conv import strip_conv
from jdet_amd.utils.registry import BACKBONES

from .lsknet import DropPath, Mlp, OverlapPatchEmbed, _cl, _dw, _init_weights, _load_pretrained

__all__ = ["StripNet", "StripNet_T", "StripNet_S"]


def _strip(conv, x):
    """a depthwise nn.Conv2d through ops/strip_conv where one of its kernel dimensions is 1, ops/dwconv otherwise"""
    if 1 in conv.kernel_size and conv.dilation == (1, 1):
        return strip_conv(_cl(x), conv.weight, conv.bias, conv.padding)
    return _dw(conv, x)


class StripBlock(nn.Module):
    def __init__(self, dim, k1, k2):
        super().__init__()
        self.conv0 = nn.Conv2d(dim, dim, 5, padding=2, groups=dim)
        self.conv_spatial1 = nn.Conv2d(dim, dim, kernel_size=(k1, k2), stride=1, padding=(k1 // 2, k2 // 2), groups=dim)
        self.conv_spatial2 = nn.Conv2d(dim, dim, kernel_size=(k2, k1), stride=1, padding=(k2 // 2, k1 // 2), groups=dim)
        self.conv1 = nn.Conv2d(dim, dim, 1)

    def forward(self, x):
        attn = _dw(self.conv0, x)
        attn = _strip(self.conv_spatial1, attn)
        attn = _strip(self.conv_spatial2, attn)
        return x * self.conv1(attn)

    execute = forward


class Attention(nn.Module):
    def __init__(self, d_model, k1, k2):
        super().__init__()
        self.proj_1 = nn.Conv2d(d_model, d_model, 1)
        self.activation = nn.GELU()
        self.spatial_gating_unit = StripBlock(d_model, k1, k2)
        self.proj_2 = nn.Conv2d(d_model, d_model, 1)

    def forward(self, x):
        shortcut = x
        x = self.activation(self.proj_1(x))
        x = self.spatial_gating_unit(x)
        return self.proj_2(x) + shortcut

    execute = forward


class Block(nn.Module):
    def __init__(self, dim, mlp_ratio=4., k1=1, k2=19, drop=0., drop_path=0., act_layer=nn.GELU, norm_cfg=None):
        super().__init__()
        assert norm_cfg is None, "StripNet: norm_cfg is not supported (BatchNorm2d only)"
        self.norm1 = nn.BatchNorm2d(dim)
        self.norm2 = nn.BatchNorm2d(dim)
        self.attn = Attention(dim, k1, k2)
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self.layer_scale_1 = nn.Parameter(1e-2 * torch.ones(dim))
        self.layer_scale_2 = nn.Parameter(1e-2 * torch.ones(dim))
        self.apply(_init_weights)

    def forward(self, x):
        x = x + self.drop_path(self.layer_scale_1[:, None, None] * self.attn(self.norm1(x)))
        return x + self.drop_path(self.layer_scale_2[:, None, None] * self.mlp(self.norm2(x)))

    execute = forward


@BACKBONES.register_module()
class StripNet(nn.Module):
    def __init__(self, img_size=224, in_chans=3, embed_dims=[64, 128, 256, 512], mlp_ratios=[8, 8, 4, 4],
                 k1s=[1, 1, 1, 1], k2s=[19, 19, 19, 19], drop_rate=0., drop_path_rate=0., norm_layer=nn.LayerNorm,
                 depths=[3, 4, 6, 3], num_stages=4, out_indices=(0, 1, 2), pretrained=None, init_cfg=None, norm_cfg=None):
        super().__init__()
        if norm_cfg is not None:
            raise ValueError("StripNet: norm_cfg is not supported (the reference's build_norm_layer does not exist); "
                             "the blocks and patch embeddings use BatchNorm2d")
        self.depths = depths
        self.num_stages = num_stages
        self.out_indices = tuple(out_indices)
        dpr = torch.linspace(0, drop_path_rate, sum(depths)).tolist()        # stochastic depth decay rule
        cur = 0
        for i in range(num_stages):
            patch_embed = OverlapPatchEmbed(img_size=img_size if i == 0 else img_size // (2 ** (i + 1)),
                                            patch_size=7 if i == 0 else 3, stride=4 if i == 0 else 2,
                                            in_chans=in_chans if i == 0 else embed_dims[i - 1], embed_dim=embed_dims[i])
            block = nn.Sequential(*[Block(dim=embed_dims[i], mlp_ratio=mlp_ratios[i], k1=k1s[i], k2=k2s[i],
                                          drop=drop_rate, drop_path=dpr[cur + j]) for j in range(depths[i])])
            cur += depths[i]
            setattr(self, "patch_embed%d" % (i + 1), patch_embed)
            setattr(self, "block%d" % (i + 1), block)
            setattr(self, "norm%d" % (i + 1), norm_layer(embed_dims[i]))
        self.apply(_init_weights)

    def forward(self, x):
        outs = []
        x = _cl(x)
        for i in range(self.num_stages):
            x = _cl(getattr(self, "patch_embed%d" % (i + 1))(x))
            x = getattr(self, "block%d" % (i + 1))(x)
            # the reference flattens to (B, H W, C) for the norm and back: on a channels-last map that is a view
            x = _cl(getattr(self, "norm%d" % (i + 1))(_cl(x).permute(0, 2, 3, 1)).permute(0, 3, 1, 2))
            if i in self.out_indices:
                outs.append(x)
        return outs

    execute = forward


@BACKBONES.register_module()
def StripNet_T(pretrained=False, **kwargs):
    model = StripNet(embed_dims=[32, 64, 160, 256], mlp_ratios=[8, 8, 4, 4], norm_layer=nn.LayerNorm, depths=[3, 3, 5, 2],
                     **kwargs)
    return _load_pretrained(model, pretrained)


@BACKBONES.register_module()
def StripNet_S(pretrained=False, **kwargs):
    model = StripNet(embed_dims=[64, 128, 320, 512], mlp_ratios=[8, 8, 4, 4], norm_layer=nn.LayerNorm, depths=[2, 2, 4, 2],
                     **kwargs)
    return _load_pretrained(model, pretrained)
