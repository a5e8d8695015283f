"""2-D decoder of the plain LKA net, the ablation partner of decoder2d.py: ``AttentionModule``, ``SpatialAttention``, ``LKABlock`` and ``MyDecoderLayer``
of 2D/networks/MaxViT_LKA_Decoder.py:53-137,492-567 with the same constructor arguments, attribute names and ``state_dict`` keys.

The large-kernel attention inside runs on this repo's HIP kernels (LKA.py); ``DropPath``, ``Mlp`` and the patch-expansion layers are decoder2d.py's.
Two things the reference does and this file keeps, so that a reference checkpoint computes what it computed there: ``MyDecoderLayer`` owns a
``concat_linear`` it never calls, and its forward runs ``layer_lka_1`` TWICE and ``layer_lka_2`` never (:557-559)."""
import torch
import torch.nn as nn

from .decoder2d import DropPath, FinalPatchExpand_X4, Mlp, PatchExpand
from .LKA import LKA, LKA_Attention


class AttentionModule(LKA):
    """MaxViT_LKA_Decoder.py:53-66 — ``LKA`` under the decoder file's name (same keys)."""


class SpatialAttention(LKA_Attention):
    """MaxViT_LKA_Decoder.py:69-85 — ``LKA_Attention`` under the decoder file's name (same keys; ``d_model`` kept as an attribute)."""

    def __init__(self, d_model):
        super().__init__(d_model)
        self.d_model = d_model
        self.spatial_gating_unit = AttentionModule(d_model)


class LKABlock(nn.Module):
    """MaxViT_LKA_Decoder.py:88-137: tokens (B, N, C) -> LayerNorm -> LKA attention (layer-scaled residual) -> LayerNorm -> Mlp (layer-scaled
    residual) -> tokens."""

    def __init__(self, dim, mlp_ratio=4., drop=0., drop_path=0., act_layer=nn.GELU, linear=False):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim)
        self.attn = SpatialAttention(dim)
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop, linear=linear)
        layer_scale_init_value = 1e-2
        self.layer_scale_1 = nn.Parameter(layer_scale_init_value * torch.ones(dim), requires_grad=True)
        self.layer_scale_2 = nn.Parameter(layer_scale_init_value * torch.ones(dim), requires_grad=True)

    def forward(self, x, H, W):
        B, N, C = x.shape
        x = x.permute(0, 2, 1).reshape(B, C, H, W)
        y = self.norm1(x.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)
        y = self.attn(y.contiguous())
        x = x + self.drop_path(self.layer_scale_1.unsqueeze(-1).unsqueeze(-1) * y)
        y = self.norm2(x.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)
        y = self.mlp(y.contiguous())
        x = x + self.drop_path(self.layer_scale_2.unsqueeze(-1).unsqueeze(-1) * y)
        return x.reshape(B, C, N).permute(0, 2, 1)


class MyDecoderLayer(nn.Module):
    """MaxViT_LKA_Decoder.py:492-567: skip fusion by addition, ``layer_lka_1`` applied twice, patch expansion (and the 1x1 class head on the last
    layer).  Called without a skip the layer only expands, so the LKA blocks' parameters get no gradient — and ``layer_lka_2`` and ``concat_linear``
    never do; a data-parallel wrapper must tolerate that (``training.wrap_data_parallel``)."""

    def __init__(self, input_size, in_out_chan, head_count, token_mlp_mode, n_class=9, norm_layer=nn.LayerNorm, is_last=False):
        super().__init__()
        dims, out_dim, key_dim, value_dim, x1_dim = in_out_chan
        self.x1_linear = nn.Linear(x1_dim, out_dim)
        if not is_last:
            self.concat_linear = nn.Linear(2 * dims, out_dim)
            self.layer_up = PatchExpand(input_resolution=input_size, dim=out_dim, dim_scale=2, norm_layer=norm_layer)
            self.last_layer = None
        else:
            self.concat_linear = nn.Linear(4 * dims, out_dim)
            self.layer_up = FinalPatchExpand_X4(input_resolution=input_size, dim=out_dim, dim_scale=4, norm_layer=norm_layer)
            self.last_layer = nn.Conv2d(out_dim, n_class, 1)
        self.layer_lka_1 = LKABlock(dim=out_dim)
        self.layer_lka_2 = LKABlock(dim=out_dim)
        for m in self.modules():   # init_weights, :531-545
            if isinstance(m, nn.Linear):
                nn.init.xavier_uniform_(m.weight)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, nn.LayerNorm):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Conv2d):
                nn.init.xavier_uniform_(m.weight)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def forward(self, x1, x2=None):
        if x2 is None:
            return self.layer_up(x1)
        b, h, w, c = x2.shape
        x2 = x2.reshape(b, -1, c)
        x = self.x1_linear(x1) + x2
        x = self.layer_lka_1(x, h, w)
        x = self.layer_lka_1(x, h, w)   # (:559 — the reference's own second call of layer_lka_1)
        if self.last_layer:
            return self.last_layer(self.layer_up(x).reshape(b, 4 * h, 4 * w, -1).permute(0, 3, 1, 2))
        return self.layer_up(x)
