"""fp64 restatement of PETR's transformer on plain tensors: the attention core (softmax(q k^T / sqrt(d) + key-padding mask) v and
its log-sum-exp), nn.MultiheadAttention with positional encodings and the identity connection, the post-norm decoder layer and the
two-transpose PETRTransformer.forward.  Nothing here imports the package's kernels; whatever dtype comes in is computed in float64.

State-dict keys are the reference's (projects/mmdet3d_plugin/models/utils/petr_transformer.py on mmcv 1.x):
  <layer>.attentions.{0,1}.attn.{in_proj_weight, in_proj_bias, out_proj.weight, out_proj.bias}
  <layer>.ffns.0.layers.0.0.{weight, bias}, <layer>.ffns.0.layers.1.{weight, bias}, <layer>.norms.{0,1,2}.{weight, bias}
  decoder.post_norm.{weight, bias}
"""
import math

import torch

F64 = torch.float64


def petr_config(num_layers, feedforward_channels):
    """The transformer block of projects/configs/petrv2/petrv2_vovnet_gridmask_p4_800x320.py:54-79."""
    return dict(type='PETRTransformer', decoder=dict(
        type='PETRTransformerDecoder', return_intermediate=True, num_layers=num_layers,
        transformerlayers=dict(
            type='PETRTransformerDecoderLayer',
            attn_cfgs=[dict(type='MultiheadAttention', embed_dims=256, num_heads=8, dropout=0.1),
                       dict(type='PETRMultiheadAttention', embed_dims=256, num_heads=8, dropout=0.1)],
            feedforward_channels=feedforward_channels, ffn_dropout=0.1, with_cp=True,
            operation_order=('self_attn', 'norm', 'cross_attn', 'norm', 'ffn', 'norm'))))


def core(q, k, v, num_heads, key_padding_mask=None):
    """q (Lq, B, C), k / v (Lk, B, C), key_padding_mask (B, Lk) nonzero = ignore -> out (Lq, B, C), lse (Lq, B, heads): the natural-log
    sum of exp(scaled, masked scores).  A row whose keys are all masked is NaN (lse -inf), as torch's softmax makes it."""
    q, k, v = q.to(F64), k.to(F64), v.to(F64)
    lq, b, c = q.shape
    lk = k.shape[0]
    d = c // num_heads
    qh = q.reshape(lq, b, num_heads, d).permute(1, 2, 0, 3)
    kh = k.reshape(lk, b, num_heads, d).permute(1, 2, 0, 3)
    vh = v.reshape(lk, b, num_heads, d).permute(1, 2, 0, 3)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(d)                          # (B, H, Lq, Lk)
    if key_padding_mask is not None:
        s = s.masked_fill(key_padding_mask.bool()[:, None, None, :], float('-inf'))
    lse = torch.logsumexp(s, dim=-1)                                      # (B, H, Lq)
    o = torch.softmax(s, dim=-1) @ vh                                     # all -inf -> NaN
    return o.permute(2, 0, 1, 3).reshape(lq, b, c), lse.permute(2, 0, 1)


def linear(x, w, b=None):
    y = x.to(F64) @ w.to(F64).t()
    return y if b is None else y + b.to(F64)


def layer_norm(x, w, b, eps=1e-5):
    x = x.to(F64)
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w.to(F64) + b.to(F64)


def attention(sd, prefix, num_heads, query, key=None, value=None, identity=None, query_pos=None, key_pos=None,
              key_padding_mask=None):
    """mmcv's MultiheadAttention / the reference's PETRMultiheadAttention (:327-367) in eval mode, (L, B, C) tensors."""
    if key is None:
        key = query
    if value is None:
        value = key
    if identity is None:
        identity = query
    if key_pos is None and query_pos is not None and query_pos.shape == key.shape:
        key_pos = query_pos
    w, bias = sd[prefix + 'attn.in_proj_weight'], sd[prefix + 'attn.in_proj_bias']
    c = query.shape[-1]
    q_in = query.to(F64) if query_pos is None else query.to(F64) + query_pos.to(F64)
    k_in = key.to(F64) if key_pos is None else key.to(F64) + key_pos.to(F64)
    q = linear(q_in, w[:c], bias[:c])
    k = linear(k_in, w[c:2 * c], bias[c:2 * c])
    v = linear(value, w[2 * c:], bias[2 * c:])
    o, _ = core(q, k, v, num_heads, key_padding_mask)
    return identity.to(F64) + linear(o, sd[prefix + 'attn.out_proj.weight'], sd[prefix + 'attn.out_proj.bias'])


def ffn(sd, prefix, x):
    h = torch.relu(linear(x, sd[prefix + 'layers.0.0.weight'], sd[prefix + 'layers.0.0.bias']))
    return x.to(F64) + linear(h, sd[prefix + 'layers.1.weight'], sd[prefix + 'layers.1.bias'])


def decoder_layer(sd, prefix, num_heads, query, key, value, query_pos, key_pos, key_padding_mask, want_cross=False):
    """('self_attn', 'norm', 'cross_attn', 'norm', 'ffn', 'norm'); want_cross: also the cross-attention module's output alone."""
    norm = lambda i, x: layer_norm(x, sd[f'{prefix}norms.{i}.weight'], sd[f'{prefix}norms.{i}.bias'])      # noqa: E731
    x = attention(sd, prefix + 'attentions.0.', num_heads, query, query_pos=query_pos, key_pos=query_pos)
    x = norm(0, x)
    cross = attention(sd, prefix + 'attentions.1.', num_heads, x, key, value, query_pos=query_pos, key_pos=key_pos,
                      key_padding_mask=key_padding_mask)
    x = norm(1, cross)
    x = norm(2, ffn(sd, prefix + 'ffns.0.', x))
    return (x, cross) if want_cross else x


def transformer(sd, num_heads, num_layers, x, mask, query_embed, pos_embed):
    """PETRTransformer.forward (:90-110) with a return_intermediate decoder and its post_norm -> out_dec (layers, bs, queries, c),
    memory (bs, n, c, h, w), and layer 0's cross-attention output (queries, bs, c)."""
    bs, n, c, h, w = x.shape
    memory = x.permute(1, 3, 4, 0, 2).reshape(-1, bs, c)
    pos = pos_embed.permute(1, 3, 4, 0, 2).reshape(-1, bs, c)
    qpos = query_embed.unsqueeze(1).repeat(1, bs, 1)
    kpm = mask.reshape(bs, -1)
    query = torch.zeros_like(qpos, dtype=F64)
    outs, cross0 = [], None
    for i in range(num_layers):
        query, cross = decoder_layer(sd, f'decoder.layers.{i}.', num_heads, query, memory, memory, qpos, pos, kpm, want_cross=True)
        if i == 0:
            cross0 = cross
        outs.append(layer_norm(query, sd['decoder.post_norm.weight'], sd['decoder.post_norm.bias']))
    out_dec = torch.stack(outs).transpose(1, 2)
    return out_dec, memory.reshape(n, h, w, bs, c).permute(3, 0, 4, 1, 2), cross0
