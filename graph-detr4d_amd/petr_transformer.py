"""PETR's transformer: global cross-attention from every query to every pixel of every camera.

Reference: projects/mmdet3d_plugin/models/utils/petr_transformer.py (PETRTransformer :33-110, PETRTransformerDecoderLayer :113-225,
PETRMultiheadAttention :227-367, PETRTransformerEncoder :371-398, PETRTransformerDecoder :401-448), built by the head of the twelve
projects/configs/petr/* and petrv2/* configs.  Type names, constructor keywords and state-dict keys are the reference's
(`decoder.layers.{i}.attentions.1.attn.in_proj_weight`, `decoder.post_norm.weight`, ...).

Inference runs on the library's kernels: the query and K|V projections on gd4d_linear_fwd (positional encodings added inside the
GEMM), gd4d_cross_mha_pack_kv + gd4d_cross_mha_fwd for the attention over 6 000 - 48 000 keys with the (bs, keys) padding mask, and
the out-projection with the residual (and the LayerNorm that follows) in its epilogue.  Training runs on the kernels with
hip_train=True (autograd.CrossMhaFunction: gd4d_cross_mha_train_fwd / gd4d_cross_mha_bwd, the projections on the library's GEMMs);
without it, and for anything the kernels do not cover, it is the reference's op sequence on torch - chosen with torch_ops=True,
never silently (Fn.torch_ops_route).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.utils.checkpoint as cp

from . import functional as Fn
from . import ops
from .registry import (ATTENTION, TRANSFORMER, TRANSFORMER_LAYER, TRANSFORMER_LAYER_SEQUENCE,
                       build_transformer_layer_sequence)
from .transformer_layers import BaseTransformerLayer, TransformerLayerSequence, _PackedAttnParams


@ATTENTION.register_module()
class PETRMultiheadAttention(nn.Module):
    """Reference :227-367: nn.MultiheadAttention with the positional encodings added to query and key (not to value), a key-padding
    mask, and the identity connection.  torch_ops=True: F.multi_head_attention_forward on this module's parameters (differentiable).

    hip_train=True (opt-in): a call in train mode or under autograd runs on the kernels too - the q, K|V and out projections through
    Fn.linear_autograd (weight gradients on gd4d_linear_bwd_weight, main_grad accumulation as everywhere), the core through
    autograd.CrossMhaFunction with attn_drop applied inside the kernel in train mode (0 in eval mode); proj_drop and dropout_layer
    stay nn.Dropout, the residual and an offered LayerNorm go through Fn.residual_norm_autograd.  Nothing of size queries x keys is
    stored.  An attn_mask, another width or head dim, a dtype other than float32, or B heads Lq Lk >= 2^32 with dropout are refused,
    naming torch_ops=True.  A row whose keys are all masked is NaN forward, as ATen makes it; its gradients are unspecified."""

    def __init__(self, embed_dims, num_heads, attn_drop=0., proj_drop=0., dropout_layer=dict(type='Dropout', drop_prob=0.),
                 init_cfg=None, batch_first=False, torch_ops=False, hip_train=False, **kwargs):
        super().__init__()
        dropout_layer = dict(dropout_layer) if dropout_layer else None
        if 'dropout' in kwargs:                      # deprecated alias used by the reference configs (:258-265)
            attn_drop = kwargs.pop('dropout')
            if dropout_layer is not None:
                dropout_layer['drop_prob'] = attn_drop
        if kwargs:
            raise TypeError(f'PETRMultiheadAttention: nn.MultiheadAttention keywords {sorted(kwargs)} are not supported')
        if embed_dims % num_heads:
            raise ValueError('embed_dims must be divisible by num_heads')
        self.embed_dims = embed_dims
        self.num_heads = num_heads
        self.batch_first = batch_first
        self.attn_drop = float(attn_drop)
        self.torch_ops = bool(torch_ops)
        self.hip_train = bool(hip_train)
        self.attn = _PackedAttnParams(embed_dims)
        self.proj_drop = nn.Dropout(proj_drop)
        self.dropout_layer = nn.Dropout(dropout_layer.get('drop_prob', 0.)) if dropout_layer else nn.Identity()

    def forward(self, query, key=None, value=None, identity=None, query_pos=None, key_pos=None, attn_mask=None,
                key_padding_mask=None, **kwargs):
        if 'residual' in kwargs:                     # (mmcv's deprecated_api_warning: residual -> identity)
            identity = kwargs.pop('residual')
        if key is None:
            key = query
        if value is None:
            value = key
        if identity is None:
            identity = query
        if key_pos is None and query_pos is not None and query_pos.shape == key.shape:
            key_pos = query_pos
        Fn.require_gpu(query, 'query')
        d = self.embed_dims // self.num_heads
        grad = Fn.wants_grad(self, query, key, value, query_pos, key_pos, identity)
        what = (f'PETRMultiheadAttention with embed_dims {self.embed_dims}, head dim {d}, '
                f'{"an attn_mask" if attn_mask is not None else "no attn_mask"}, '
                f'{"train" if self.training else "eval"} mode, {"autograd" if grad else "no autograd"}, dtype {query.dtype}')
        covered = (self.embed_dims == 256 and d == 32 and attn_mask is None
                   and query.dtype == torch.float32 and key.dtype == torch.float32 and value.dtype == torch.float32)
        train = self.hip_train and (self.training or grad)
        if train:
            drop = self.attn_drop if self.training else 0.
            axis = 1 if self.batch_first else 0
            elements = query.shape[1 - axis] * self.num_heads * query.shape[axis] * key.shape[axis]
            what += f', hip_train, attn_drop {drop}, B heads Lq Lk = {elements}'
            supported = covered and (drop == 0. or elements < 2 ** 32)
        else:
            supported = covered and not self.training and not grad
        if Fn.torch_ops_route(what, supported, module=self):
            return self._forward_torch(query, key, value, identity, query_pos, key_pos, attn_mask, key_padding_mask)
        if train:
            tr = (lambda t: None if t is None else t.transpose(0, 1)) if self.batch_first else (lambda t: t)      # noqa: E731
            out = self._attention_train(tr(query), tr(key), tr(value), tr(query_pos), tr(key_pos), key_padding_mask, drop,
                                        value_is_key=value is key)
            out = self.dropout_layer(self.proj_drop(tr(out)))
            return Fn.residual_norm_autograd(kwargs, identity, out)
        if self.batch_first:
            tr = lambda t: None if t is None else t.transpose(0, 1)      # noqa: E731
            out = self._forward_kernels(tr(query), tr(key), tr(value), tr(identity), tr(query_pos), tr(key_pos), key_padding_mask,
                                        None, value_is_key=value is key)
            return out.transpose(0, 1)
        return self._forward_kernels(query, key, value, identity, query_pos, key_pos, key_padding_mask, Fn.take_fused_norm(kwargs),
                                     value_is_key=value is key)

    def _forward_kernels(self, query, key, value, identity, query_pos, key_pos, key_padding_mask, fused, value_is_key):
        """(L, B, C) tensors: 2 GEMMs (q; K|V with key_pos added for the K columns only), the pack, the core (+ its merge), and the
        out-projection with the residual - and the layer's next LayerNorm, when it was offered - in its epilogue."""
        c = self.embed_dims
        w, bias = self.attn.in_proj_weight, self.attn.in_proj_bias
        pos = {} if query_pos is None else dict(x2=query_pos.expand_as(query))
        q = Fn.linear(query, w[:c], bias[:c], **pos)
        if value_is_key:
            kpos = {} if key_pos is None else dict(x2=key_pos.expand_as(key), n_split=c)
            kvp = Fn.linear(key, w[c:], bias[c:], **kpos)
            k, v = kvp[..., :c], kvp[..., c:]
        else:
            kpos = {} if key_pos is None else dict(x2=key_pos.expand_as(key))
            k = Fn.linear(key, w[c:2 * c], bias[c:2 * c], **kpos)
            v = Fn.linear(value, w[2 * c:], bias[2 * c:])
        kv = ops.cross_mha_pack_kv(k, v, num_heads=self.num_heads)
        o = ops.cross_mha_fwd(q, kv, self.num_heads, key_padding_mask=key_padding_mask)
        wo, bo = self.attn.out_proj.weight, self.attn.out_proj.bias
        if fused is not None and identity.shape == o.shape and Fn.rowblock_ok(o, wo, fused['norm']):
            fused['done'] = True
            return Fn.linear_norm(o, wo, bo, fused['norm'], r1=identity)
        return Fn.linear(o, wo, bo, r1=identity.expand_as(o))

    def _attention_train(self, query, key, value, query_pos, key_pos, key_padding_mask, drop, value_is_key):
        """(L, B, C) tensors -> the out-projection's output, every step an autograd node on the library's kernels.  Without a key
        encoding K|V is one GEMM and its gradient one tensor; with one (PETR's case) K and V read different rows: two GEMMs."""
        from .autograd import CrossMhaFunction
        c = self.embed_dims
        w, bias = self.attn.in_proj_weight, self.attn.in_proj_bias
        rows = lambda lo, hi: (Fn.main_grad(w, (lo, hi)), Fn.main_grad(bias, (lo, hi)))      # noqa: E731
        q_in = query if query_pos is None else query + query_pos
        q = Fn.linear_autograd(q_in.contiguous(), w[:c], bias[:c], main=rows(0, c))
        if key_padding_mask is not None and key_padding_mask.dtype not in (torch.bool, torch.uint8):
            raise TypeError('key_padding_mask must be bool or uint8')
        if value_is_key and key_pos is None:
            kvp = Fn.linear_autograd(key.contiguous(), w[c:], bias[c:], main=rows(c, 3 * c))
            o = CrossMhaFunction.apply(q, kvp, None, key_padding_mask, self.num_heads, drop)
        else:
            k_in = key if key_pos is None else key + key_pos
            k = Fn.linear_autograd(k_in.contiguous(), w[c:2 * c], bias[c:2 * c], main=rows(c, 2 * c))
            v = Fn.linear_autograd(value.contiguous(), w[2 * c:], bias[2 * c:], main=rows(2 * c, 3 * c))
            o = CrossMhaFunction.apply(q, k, v, key_padding_mask, self.num_heads, drop)
        return Fn.linear_autograd(o, self.attn.out_proj.weight, self.attn.out_proj.bias)

    def _forward_torch(self, query, key, value, identity, query_pos, key_pos, attn_mask, key_padding_mask):
        """The reference's op sequence (:341-367) with nn.MultiheadAttention.forward spelled as the functional it calls."""
        if query_pos is not None:
            query = query + query_pos
        if key_pos is not None:
            key = key + key_pos
        if self.batch_first:
            query, key, value = (t.transpose(0, 1) for t in (query, key, value))
        if key_padding_mask is not None and key_padding_mask.dtype == torch.uint8:
            key_padding_mask = key_padding_mask.bool()
        out = F.multi_head_attention_forward(
            query, key, value, self.embed_dims, self.num_heads, self.attn.in_proj_weight, self.attn.in_proj_bias, None, None, False,
            self.attn_drop, self.attn.out_proj.weight, self.attn.out_proj.bias, training=self.training,
            key_padding_mask=key_padding_mask, need_weights=False, attn_mask=attn_mask)[0]
        if self.batch_first:
            out = out.transpose(0, 1)
        return identity + self.dropout_layer(self.proj_drop(out))


@TRANSFORMER_LAYER.register_module()
class PETRTransformerDecoderLayer(BaseTransformerLayer):
    """Reference :113-225: a post-norm DETR decoder layer (self_attn, norm, cross_attn, norm, ffn, norm); with_cp recomputes the
    layer in the backward pass (torch.utils.checkpoint) when it trains."""

    def __init__(self, attn_cfgs, feedforward_channels, ffn_dropout=0.0, operation_order=None,
                 act_cfg=dict(type='ReLU', inplace=True), norm_cfg=dict(type='LN'), ffn_num_fcs=2, with_cp=True, **kwargs):
        super().__init__(attn_cfgs=attn_cfgs, feedforward_channels=feedforward_channels, ffn_dropout=ffn_dropout,
                         operation_order=operation_order, norm_cfg=norm_cfg, ffn_num_fcs=ffn_num_fcs, **kwargs)
        assert len(operation_order) == 6
        assert set(operation_order) == set(['self_attn', 'norm', 'cross_attn', 'ffn'])
        self.use_checkpoint = with_cp

    def _forward(self, query, key=None, value=None, query_pos=None, key_pos=None, attn_masks=None, query_key_padding_mask=None,
                 key_padding_mask=None):
        return super().forward(query, key=key, value=value, query_pos=query_pos, key_pos=key_pos, attn_masks=attn_masks,
                               query_key_padding_mask=query_key_padding_mask, key_padding_mask=key_padding_mask)

    def forward(self, query, key=None, value=None, query_pos=None, key_pos=None, attn_masks=None, query_key_padding_mask=None,
                key_padding_mask=None, **kwargs):
        if self.use_checkpoint and self.training:
            return cp.checkpoint(self._forward, query, key, value, query_pos, key_pos, attn_masks, query_key_padding_mask,
                                 key_padding_mask, use_reentrant=True)
        return self._forward(query, key=key, value=value, query_pos=query_pos, key_pos=key_pos, attn_masks=attn_masks,
                             query_key_padding_mask=query_key_padding_mask, key_padding_mask=key_padding_mask)


class _PETRLayerSequence(TransformerLayerSequence):
    """mmcv 1.x TransformerLayerSequence.forward: every layer gets the same keys, values, encodings and masks."""

    def _run_layers(self, query, key, value, query_pos=None, key_pos=None, attn_masks=None, query_key_padding_mask=None,
                    key_padding_mask=None, **kwargs):
        for layer in self.layers:
            query = layer(query, key, value, query_pos=query_pos, key_pos=key_pos, attn_masks=attn_masks,
                          query_key_padding_mask=query_key_padding_mask, key_padding_mask=key_padding_mask, **kwargs)
        return query

    def _norm(self, x):
        return Fn.layer_norm_autograd(x, self.post_norm) if Fn.wants_grad(self.post_norm, x) else Fn.layer_norm(x, self.post_norm)


@TRANSFORMER_LAYER_SEQUENCE.register_module()
class PETRTransformerEncoder(_PETRLayerSequence):
    """Reference :371-398 (no shipped config builds it): a final LayerNorm only for pre-norm layers."""

    def __init__(self, *args, post_norm_cfg=dict(type='LN'), **kwargs):
        super().__init__(*args, **kwargs)
        if post_norm_cfg is not None:
            self.post_norm = nn.LayerNorm(self.embed_dims) if self.pre_norm else None
        else:
            assert not self.pre_norm, f'Use prenorm in {self.__class__.__name__},Please specify post_norm_cfg'
            self.post_norm = None

    def forward(self, *args, **kwargs):
        x = self._run_layers(*args, **kwargs)
        return self._norm(x) if self.post_norm is not None else x


@TRANSFORMER_LAYER_SEQUENCE.register_module()
class PETRTransformerDecoder(_PETRLayerSequence):
    """Reference :401-448: the stack of decoder layers; post_norm is applied to every intermediate that is returned."""

    def __init__(self, *args, post_norm_cfg=dict(type='LN'), return_intermediate=False, **kwargs):
        super().__init__(*args, **kwargs)
        self.return_intermediate = return_intermediate
        self.post_norm = nn.LayerNorm(self.embed_dims) if post_norm_cfg is not None else None

    def forward(self, query, *args, **kwargs):
        """(layers, queries, bs, c) with return_intermediate, every entry through post_norm; else the last layer's state,
        (1, queries, bs, c) after post_norm (and, as in the reference, without the leading axis when there is no post_norm)."""
        normed = (lambda t: t) if self.post_norm is None else self._norm
        states = []
        for layer in self.layers:
            query = layer(query, *args, **kwargs)
            if self.return_intermediate:
                states.append(normed(query))
        if self.return_intermediate:
            return torch.stack(states)
        return query if self.post_norm is None else normed(query)[None]


@TRANSFORMER.register_module()
class PETRTransformer(nn.Module):
    """Reference :33-110: flattens the (bs, n, c, h, w) camera features and their 3D position embedding to (n h w, bs, c) keys and
    runs the decoder on zero targets with the query embedding as positional encoding."""

    def __init__(self, encoder=None, decoder=None, init_cfg=None, cross=False):
        super().__init__()
        self.encoder = build_transformer_layer_sequence(encoder) if encoder is not None else None
        self.decoder = build_transformer_layer_sequence(decoder)
        self.embed_dims = self.decoder.embed_dims
        self.cross = cross

    def init_weights(self):
        # reference :62-67 (mmcv's xavier_init: uniform, gain 1; a bias, where the module has one, to 0)
        for m in self.modules():
            if hasattr(m, 'weight') and m.weight.dim() > 1:
                nn.init.xavier_uniform_(m.weight, gain=1)
                if getattr(m, 'bias', None) is not None:
                    nn.init.constant_(m.bias, 0)
        self._is_init = True

    @staticmethod
    def _camera_pixels_first(t):
        """(bs, n, c, h, w) -> (n h w, bs, c): one key per pixel of every camera, a torch copy."""
        bs, n, c, h, w = t.shape
        return t.permute(1, 3, 4, 0, 2).reshape(n * h * w, bs, c)

    def forward_keys(self, keys, key_pos, key_padding_mask, query_embed, reg_branch=None):
        """The decoder on key-major rows: keys, key_pos (n h w, bs, c) - what forward makes of its (bs, n, c, h, w) arguments with two
        copies, and what ops.petr_keys_fwd writes directly -, key_padding_mask (bs, n h w), nonzero = padded pixel; query_embed
        (num_query, c).  Returns out_dec (num_layers or 1, bs, num_query, c)."""
        bs = keys.shape[1]
        query_pos = query_embed[:, None, :].expand(-1, bs, -1).contiguous()        # the same embedding for every sample
        states = self.decoder(query=torch.zeros_like(query_pos), key=keys, value=keys, key_pos=key_pos, query_pos=query_pos,
                              key_padding_mask=key_padding_mask, reg_branch=reg_branch)
        return states.transpose(1, 2)

    def forward(self, x, mask, query_embed, pos_embed, reg_branch=None):
        """x, pos_embed (bs, n, c, h, w); mask (bs, n, h, w), nonzero = padded pixel; query_embed (num_query, c).  Returns out_dec
        (num_layers or 1, bs, num_query, c) and memory (bs, n, c, h, w) - the keys laid out as x again."""
        bs, n, c, h, w = x.shape
        keys = self._camera_pixels_first(x)
        key_pos = self._camera_pixels_first(pos_embed)
        out_dec = self.forward_keys(keys, key_pos, mask.reshape(bs, n * h * w), query_embed, reg_branch)
        return out_dec, keys.reshape(n, h, w, bs, c).permute(3, 0, 4, 1, 2)
