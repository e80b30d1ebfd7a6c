"""PETRHead / PETRv2Head: the stage between the neck and the boxes of the twelve projects/configs/petr/* and petrv2/* configs.

Reference: projects/mmdet3d_plugin/models/dense_heads/petr_head.py (PETRHead :43-734) and petrv2_head.py (SELayer :44-56, RegLayer
:58-89, PETRv2Head :91-...).  Type names, constructor keywords and the module tree are the reference's, so a head checkpoint loads
with strict=True: `input_proj`, `cls_branches.N.*`, `reg_branches.N.*`, `adapt_pos3d`, `position_encoder`, `reference_points`,
`query_embedding`, `fpe.conv_reduce / conv_expand`, `code_weights`, `transformer.*`.

Kernel route (eval mode, no autograd): input_proj on the library's 1x1 convolution, then ONE launch for the whole key side
(ops.petr_keys_fwd: position_encoder over the frustum coordinates generated in registers, the SE gate of `fpe`, the adapt_pos3d
branch added, both results written as the (n h w, bs, 256) key rows), PETRTransformer.forward_keys on those rows - the two permute
copies of PETRTransformer.forward are never made -, and the branches + box epilogue through functional.head_outputs.  The sine
branch and query_embedding(pos2posemb3d(reference_points)) depend on parameters (and the padding masks) only: they are kept under
ops._Stamp, the one validity rule.

hip_train=True (opt-in): a call in train mode or under autograd runs on the kernels too.  The key side is ONE autograd node
(autograd.PetrKeysFunction: gd4d_petr_keys_train_fwd forward; gd4d_petr_keys_bwd_rows, gd4d_mlp2_wgrad and the gate's / input_proj's
existing kernels backward - no (rows, 1024) hidden activation and no (rows, 192) frustum tensor in either direction), the query
embedding, the branches and the RegLayers go through Fn.linear_autograd, the box epilogue through autograd.BoxHeadFunction, and every
PETRMultiheadAttention below the head gets hip_train = True.  Eval mode without autograd takes the inference route unchanged.

torch_ops=True: the reference's op sequence on torch, differentiable - what training takes without hip_train; it wins over
hip_train.  What the kernels do not cover is refused in the name of that switch, at construction where the cause is known there;
never a silent fallback.

PETRHeadseg (dense_heads/petr_head_seg.py, the head of petrv2_BEVseg.py) is the same base class plus a lane half: a second
PETRTransformer over the SAME key rows, one shared lane_branches MLP, Sigmoid_ce_loss on gd4d_lane_mask_loss and the map decode on
gd4d_lane_map_fwd (csrc/gd4d_lane_head.hip).  The base class's routes are split into "keys" and "the rest" for it.
"""
import copy
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import functional as Fn
from . import ops
from ._lib import Gd4dError
from .head_pe import FeaturePositionEmbedding, SELayer
from .registry import HEADS, LOSSES, build_bbox_coder, build_loss, build_transformer


def pos2posemb3d(pos, num_pos_feats=128, temperature=10000):
    """petr_head.py:29-41."""
    pos = pos * (2 * math.pi)
    dim_t = torch.arange(num_pos_feats, dtype=torch.float32, device=pos.device)
    dim_t = temperature ** (2 * (dim_t // 2) / num_pos_feats)
    parts = []
    for axis in (1, 0, 2):                                   # (pos_y, pos_x, pos_z)
        p = pos[..., axis, None] / dim_t
        parts.append(torch.stack((p[..., 0::2].sin(), p[..., 1::2].cos()), dim=-1).flatten(-2))
    return torch.cat(parts, dim=-1)


def _sine_encoding(mask, cfg):
    """SinePositionalEncoding3D.forward (models/utils/positional_encoding.py:58-100) for a (B, N, H, W) mask, or mmdet's
    SinePositionalEncoding for a (B, H, W) one, on torch: channels (n,) y, x."""
    nf, temp = cfg['num_feats'], cfg.get('temperature', 10000)
    not_mask = 1 - mask.to(torch.int)
    dims = range(1, mask.dim())
    embeds = [not_mask.cumsum(d, dtype=torch.float32) for d in dims]
    if cfg.get('normalize', False):
        scale, eps, offset = cfg.get('scale', 2 * math.pi), cfg.get('eps', 1e-6), cfg.get('offset', 0.)
        embeds = [(e + offset) / (e.narrow(d, e.shape[d] - 1, 1) + eps) * scale for e, d in zip(embeds, dims)]
    dim_t = torch.arange(nf, dtype=torch.float32, device=mask.device)
    dim_t = temp ** (2 * (dim_t // 2) / nf)
    pos = []
    for e in embeds:
        p = e[..., None] / dim_t
        if mask.dim() == 4:          # :88-96 stacks at dim 4 of a FIVE-dimensional tensor: all sines, then all cosines
            pos.append(torch.cat((p[..., 0::2].sin(), p[..., 1::2].cos()), dim=-1))
        else:                        # mmdet's two-dimensional encoding: interleaved
            pos.append(torch.stack((p[..., 0::2].sin(), p[..., 1::2].cos()), dim=-1).flatten(-2))
    pos = torch.cat(pos, dim=-1)
    return pos.permute(0, 1, 4, 2, 3) if mask.dim() == 4 else pos.permute(0, 3, 1, 2)


class RegLayer(nn.Module):
    """petrv2_head.py:58-89: a shared trunk and five task heads (xy, z, size, rot, velo) whose outputs are concatenated.  On the GPU
    without autograd the five heads run as ONE stacked (5 C, C) Linear + ReLU and ONE block-diagonal (sum of reg dims, 5 C) Linear on
    gd4d_linear_fwd; the stacked fp32 weights - what that kernel reads; it has no packed image form - are kept while the twenty
    parameters they are made of hold (ops._Stamp).  Train mode, autograd and other activations raise and name `torch_ops = True`,
    which is the reference's op sequence on torch; PETRv2Head's torch-op route sets it.  hip_train (set by a head built with
    hip_train=True, not a keyword of its own): train mode / autograd run the trunk and the five heads through Fn.sequential_autograd."""

    def __init__(self, embed_dims=256, shared_reg_fcs=2, group_reg_dims=(2, 1, 3, 2, 2), act_layer=nn.ReLU, drop=0.0):
        super().__init__()
        reg_branch = []
        for _ in range(shared_reg_fcs):
            reg_branch += [nn.Linear(embed_dims, embed_dims), act_layer(), nn.Dropout(drop)]
        self.reg_branch = nn.Sequential(*reg_branch)
        self.task_heads = nn.ModuleList(nn.Sequential(nn.Linear(embed_dims, embed_dims), act_layer(), nn.Linear(embed_dims, d))
                                        for d in group_reg_dims)
        self._stacked = None
        self.torch_ops = False
        self.hip_train = False

    def _stacked_heads(self):
        src = [p for h in self.task_heads for p in (h[0].weight, h[0].bias, h[2].weight, h[2].bias)]
        if self._stacked is None or not self._stacked[0].valid(src):
            with torch.no_grad():
                w1 = torch.cat([h[0].weight for h in self.task_heads]).contiguous()
                b1 = torch.cat([h[0].bias for h in self.task_heads]).contiguous()
                w2 = torch.block_diag(*[h[2].weight for h in self.task_heads]).contiguous()
                b2 = torch.cat([h[2].bias for h in self.task_heads]).contiguous()
            self._stacked = (ops._Stamp(src), (w1, b1, w2, b2))
        return self._stacked[1]

    def forward(self, x):
        grad = Fn.wants_grad(self, x)
        plain = all(isinstance(h[1], nn.ReLU) for h in self.task_heads) and \
            all(isinstance(m, (nn.Linear, nn.ReLU, nn.Dropout)) for m in self.reg_branch)
        what = (f'RegLayer in {"train" if self.training else "eval"} mode, {"autograd" if grad else "no autograd"}, dtype {x.dtype}, '
                f'{"ReLU" if plain else "another activation"}')
        train = self.hip_train and (self.training or grad)
        covered = plain and x.dtype == torch.float32 and (train or (not self.training and not grad))
        if Fn.torch_ops_route(what, covered, module=self):               # (the head's torch-op route sets torch_ops on its RegLayers)
            reg_feat = self.reg_branch(x)                                # petrv2_head.py:82-89
            return torch.cat([head(reg_feat.clone()) for head in self.task_heads], -1)
        Fn.require_gpu(x, 'x')
        if train:                                            # (the stacked form is for inference only)
            reg_feat = Fn.sequential_autograd(self.reg_branch, x)
            return torch.cat([Fn.sequential_autograd(head, reg_feat) for head in self.task_heads], -1)
        for m in self.reg_branch:                            # (eval mode: the Dropouts are the identity)
            if isinstance(m, nn.Linear):
                x = Fn.linear(x, m.weight, m.bias, relu=True)
        w1, b1, w2, b2 = self._stacked_heads()
        return Fn.linear(Fn.linear(x, w1, b1, relu=True), w2, b2)


class _PETRHeadBase(nn.Module):
    """What PETRHead and PETRv2Head share (the reference has it twice); the subclasses choose position_level / fpe / time /
    RegLayer and whether the six levels share one branch object."""
    _version = 2
    _share_branches = True
    _gate_name = 'fpe'                                        # the attribute (and state-dict prefix) of the with_fpe SE gate

    def __init__(self, num_classes, in_channels, num_query=100, num_reg_fcs=2, transformer=None, sync_cls_avg_factor=False,
                 positional_encoding=dict(type='SinePositionalEncoding', num_feats=128, normalize=True), code_weights=None,
                 bbox_coder=None,
                 loss_cls=dict(type='CrossEntropyLoss', bg_cls_weight=0.1, use_sigmoid=False, loss_weight=1.0, class_weight=1.0),
                 loss_bbox=dict(type='L1Loss', loss_weight=5.0), loss_iou=dict(type='GIoULoss', loss_weight=2.0),
                 train_cfg=dict(assigner=dict(type='HungarianAssigner', cls_cost=dict(type='ClassificationCost', weight=1.),
                                              reg_cost=dict(type='BBoxL1Cost', weight=5.0),
                                              iou_cost=dict(type='IoUCost', iou_mode='giou', weight=2.0))),
                 test_cfg=dict(max_per_img=100), with_position=True, with_multiview=False, depth_step=0.8, depth_num=64, LID=False,
                 depth_start=1, position_level=0, position_range=[-65, -65, -8.0, 65, 65, 8.0], group_reg_dims=(2, 1, 3, 2, 2),
                 init_cfg=None, normedlinear=False, with_fpe=False, with_time=False, with_multi=False, torch_ops=False, hip_train=False,
                 **kwargs):
        super().__init__()
        self.torch_ops = bool(torch_ops)
        self.hip_train = bool(hip_train)
        self.code_size = kwargs.get('code_size', 10)
        cw = code_weights if code_weights is not None else [1.0] * 8 + [0.2, 0.2]
        self.num_query, self.num_classes, self.in_channels, self.num_reg_fcs = num_query, num_classes, in_channels, num_reg_fcs
        self.sync_cls_avg_factor = sync_cls_avg_factor
        self.loss_cfg = dict(loss_cls=copy.deepcopy(loss_cls), loss_bbox=copy.deepcopy(loss_bbox), loss_iou=copy.deepcopy(loss_iou))
        self.train_cfg, self.test_cfg = copy.deepcopy(train_cfg), copy.deepcopy(test_cfg)
        self.embed_dims = 256
        self.depth_step, self.depth_num, self.position_dim = depth_step, depth_num, 3 * depth_num
        self.position_range, self.LID, self.depth_start = list(position_range), LID, depth_start
        self.position_level, self.with_position, self.with_multiview = position_level, with_position, with_multiview
        self.normedlinear, self.with_fpe, self.with_time, self.with_multi = normedlinear, with_fpe, with_time, with_multi
        self.group_reg_dims = tuple(group_reg_dims)
        self.num_pred = 6
        assert 'num_feats' in positional_encoding
        assert positional_encoding['num_feats'] * 2 == self.embed_dims, \
            f'embed_dims should be exactly 2 times of num_feats. Found {self.embed_dims} and {positional_encoding["num_feats"]}.'
        self.positional_encoding = dict(positional_encoding)
        self.cls_out_channels = num_classes if loss_cls.get('use_sigmoid', False) else num_classes + 1
        self._refuse_at_construction()
        self.transformer = build_transformer(transformer)
        self.code_weights = nn.Parameter(torch.tensor(cw[:self.code_size], dtype=torch.float32), requires_grad=False)
        self.bbox_coder = build_bbox_coder(bbox_coder)
        self.pc_range = self.bbox_coder.pc_range
        self._init_layers()

    # ---- construction -------------------------------------------------------------------------------------------------
    def _uncovered(self):
        """What of this head's configuration the kernel route does not take: [(what, why)]."""
        no = []
        if not self.LID:
            no.append(('LID=False', 'the frustum kernel generates linear-increasing depth bins'))
        if not self.with_multiview:
            no.append(('with_multiview=False', 'the sine kernel is SinePositionalEncoding3D\'s'))
        if not self.with_position:
            no.append(('with_position=False', 'the key-side launch is built around position_encoder'))
        if self.normedlinear:
            no.append(('normedlinear=True', 'the branch kernels take Linear / LayerNorm / ReLU'))
        if self.depth_num != 64:
            no.append((f'depth_num={self.depth_num}', 'the frustum kernel takes 64 depth bins (192 inputs)'))
        if self.with_multiview and self.positional_encoding.get('type') != 'SinePositionalEncoding3D':
            no.append((f'positional_encoding type {self.positional_encoding.get("type")!r}', 'the sine kernel is SinePositionalEncoding3D\'s'))
        return no

    def _refuse_at_construction(self):
        no = self._uncovered()
        if no and not self.torch_ops:
            raise Gd4dError(f'{type(self).__name__}: ' + '; '.join(f'{w} ({y})' for w, y in no) + ' - outside the limits of graph-detr4d_amd\'s '
                            'kernels.  Construct the head with torch_ops=True to run the reference\'s op sequence on torch instead '
                            '(slower; an explicit choice, not a fallback).')

    def _init_layers(self):
        c = self.embed_dims
        self.input_proj = nn.Conv2d(self.in_channels, c, kernel_size=1)
        cls_branch = []
        for _ in range(self.num_reg_fcs):
            cls_branch += [nn.Linear(c, c), nn.LayerNorm(c), nn.ReLU(inplace=True)]
        if self.normedlinear:
            raise Gd4dError(f'{type(self).__name__}: normedlinear=True (mmdet\'s NormedLinear) is not part of graph-detr4d_amd, on '
                            'either route: torch_ops=True does not cover it')
        cls_branch.append(nn.Linear(c, self.cls_out_channels))
        fc_cls = nn.Sequential(*cls_branch)
        if self.with_multi:
            reg_branch = RegLayer(c, self.num_reg_fcs, self.group_reg_dims)
        else:
            reg_branch = []
            for _ in range(self.num_reg_fcs):
                reg_branch += [nn.Linear(c, c), nn.ReLU()]
            reg_branch.append(nn.Linear(c, self.code_size))
            reg_branch = nn.Sequential(*reg_branch)
        one = (lambda m: m) if self._share_branches else copy.deepcopy
        self.cls_branches = nn.ModuleList([one(fc_cls) for _ in range(self.num_pred)])
        self.reg_branches = nn.ModuleList([one(reg_branch) for _ in range(self.num_pred)])
        sine_in = c * 3 // 2 if self.with_multiview else c
        sine_hidden = c * 4 if self.with_multiview else c
        self.adapt_pos3d = nn.Sequential(nn.Conv2d(sine_in, sine_hidden, 1), nn.ReLU(), nn.Conv2d(sine_hidden, c, 1))
        if self.with_position:
            self.position_encoder = nn.Sequential(nn.Conv2d(self.position_dim, c * 4, 1), nn.ReLU(), nn.Conv2d(c * 4, c, 1))
        self.reference_points = nn.Embedding(self.num_query, 3)
        self.query_embedding = nn.Sequential(nn.Linear(c * 3 // 2, c), nn.ReLU(), nn.Linear(c, c))
        if self.with_fpe:
            setattr(self, self._gate_name, SELayer(c))
        self._kept = {}                                       # name -> (stamp, value): images, input_proj's, the query embedding
        self.__dict__['_pe'] = None                           # FeaturePositionEmbedding's masks / sine pieces over THIS head's modules
        self.__dict__['_xs'] = None                           # (masks, the (R, S, 384) sine expansion): a function of the masks alone
        if self.hip_train:                                    # one keyword trains the stage, as ResNet(hip_train=True) tells its blocks
            from .petr_transformer import PETRMultiheadAttention
            for m in self.modules():
                if isinstance(m, (PETRMultiheadAttention, RegLayer)):
                    m.hip_train = True

    def init_weights(self):
        self.transformer.init_weights()
        nn.init.uniform_(self.reference_points.weight.data, 0, 1)
        if self.loss_cfg['loss_cls'].get('use_sigmoid', False):
            bias_init = float(-np.log((1 - 0.01) / 0.01))
            for m in self.cls_branches:
                nn.init.constant_(m[-1].bias, bias_init)

    def _convert_old_keys(self, state_dict):
        """The `_version < 2` key conversion (petr_head.py:338-352)."""
        convert = {'.self_attn.': '.attentions.0.', '.multihead_attn.': '.attentions.1.', '.decoder.norm.': '.decoder.post_norm.'}
        for k in list(state_dict.keys()):
            for old, new in convert.items():
                if old in k:
                    state_dict[k.replace(old, new)] = state_dict.pop(k)
                    break

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        version = local_metadata.get('version', None)
        if version is None or version < 2:
            self._convert_old_keys(state_dict)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)
        self._kept.clear()
        ops.invalidate_chain_images()

    def train(self, mode=True):
        if mode != self.training:
            self._kept.clear()
            self.__dict__['_pe'] = self.__dict__['_xs'] = None
        return super().train(mode)

    # ---- kept values ---------------------------------------------------------------------------------------------------
    def _keep(self, name, sources, build):
        hit = self._kept.get(name)
        if hit is not None and hit[0].valid(sources):
            return hit[1]
        with torch.no_grad():
            value = build()
        self._kept[name] = (ops._Stamp(sources), value)
        return value

    def _helper(self):
        """FeaturePositionEmbedding.sine_only over this head's own adapt_pos3d: its padding masks (kept per shape key), its
        sine branch (kept while the masks and adapt_pos3d hold) and its persistent img2lidar buffer.  Not a submodule: the head's
        state-dict keys are the reference's."""
        pe = self.__dict__['_pe']
        if pe is None:
            cfg = self.positional_encoding
            pe = FeaturePositionEmbedding.sine_only(
                self.adapt_pos3d, embed_dims=self.embed_dims, depth_num=self.depth_num, depth_start=self.depth_start,
                pc_range=self.position_range, num_feats=cfg['num_feats'], temperature=cfg.get('temperature', 10000),
                normalize=cfg.get('normalize', False), scale=cfg.get('scale', 2 * math.pi), eps=cfg.get('eps', 1e-6),
                offset=cfg.get('offset', 0.))
            self.__dict__['_pe'] = pe
        return pe

    def _gate(self):
        return getattr(self, self._gate_name)

    def _input_proj_image(self):
        conv = self.input_proj
        return self._keep('input_proj', [conv.weight], lambda: (ops.conv1x1_image(conv.weight.detach()),
                                                                torch.ones(conv.out_channels, device=conv.weight.device)))

    def _input_proj(self, feat):
        """input_proj on gd4d_conv1x1_bn_act_fwd (scale 1, shift = the bias, no activation): (bs, n, cin, h, w) -> (bs, n, 256, h, w)."""
        conv = self.input_proj
        image, scale = self._input_proj_image()
        bs, n = feat.shape[:2]
        x = ops.conv1x1_bn_act(feat.flatten(0, 1).contiguous(), image, conv.out_channels, scale, conv.bias.detach().contiguous(), relu=False)
        return x.unflatten(0, (bs, n))

    def _images(self):
        pe0, pe2 = self.position_encoder[0], self.position_encoder[2]
        flat = lambda c: c.weight.detach().view(c.out_channels, c.in_channels).contiguous()      # noqa: E731
        img = {'pe': self._keep('pe_image', [pe0.weight, pe0.bias, pe2.weight],
                                lambda: ops.mlp2_frustum_image(flat(pe0), pe0.bias.detach(), flat(pe2))), 'se': None}
        if self.with_fpe:
            cr, ce = self._gate().conv_reduce, self._gate().conv_expand
            img['se'] = self._keep('se_image', [cr.weight, cr.bias, ce.weight], lambda: ops.mlp2_image(flat(cr), cr.bias.detach(), flat(ce)))
        return img

    def _query_embeds(self):
        """query_embedding(pos2posemb3d(reference_points)): parameters only - kept under the one validity rule."""
        q0, q2 = self.query_embedding[0], self.query_embedding[2]
        src = [self.reference_points.weight, q0.weight, q0.bias, q2.weight, q2.bias]
        return self._keep('query_embeds', src, lambda: Fn.linear(Fn.linear(pos2posemb3d(self.reference_points.weight), q0.weight, q0.bias,
                                                                           relu=True), q2.weight, q2.bias))

    # ---- forward ---------------------------------------------------------------------------------------------------------
    def _mean_time_stamp(self, img_metas, like, batch_size):
        """petrv2_head.py:488-494."""
        ts = like.new_tensor(np.asarray([np.asarray(m['timestamp']) for m in img_metas])).view(batch_size, -1, 6)
        return (ts[:, 1, :] - ts[:, 0, :]).mean(-1)

    def forward(self, mlvl_feats, img_metas):
        """mlvl_feats: (B, N, C, H, W) maps, of which level `position_level` is read.  Returns the reference's dict: all_cls_scores
        (layers, B, Q, classes), all_bbox_preds (layers, B, Q, code), enc_cls_scores = enc_bbox_preds = None."""
        feat = mlvl_feats[self.position_level]
        Fn.require_gpu(feat, 'mlvl_feats')
        grad = Fn.wants_grad(self, feat)
        no = self._uncovered()
        if feat.dim() != 5 or feat.shape[2] != self.in_channels:
            raise Gd4dError(f'{type(self).__name__}: position_level = {self.position_level} names a map of shape {tuple(feat.shape)}, not the '
                            f'(B, N, {self.in_channels}, H, W) map input_proj reads; the kernels take one level, the one input_proj reads, '
                            'and torch_ops=True - the reference\'s op sequence - does not take another one either')
        what = (f'{type(self).__name__} in {"train" if self.training else "eval"} mode, {"autograd" if grad else "no autograd"}, '
                f'in_channels {self.in_channels} (a multiple of 32 up to 2048), dtype {feat.dtype}'
                + ''.join(f', {w}' for w, _ in no))
        train = self.hip_train and (self.training or grad)
        covered = not no and (train or (not self.training and not grad)) and feat.dtype == torch.float32 and \
            self.in_channels % 32 == 0 and 32 <= self.in_channels <= 2048
        if Fn.torch_ops_route(what + (', hip_train' if train else ''), covered, module=self):
            return self._forward_torch(mlvl_feats, img_metas)
        if train:
            return self._forward_train(self._past_frames_detached(feat), img_metas)
        with torch.no_grad():
            return self._forward_kernels(feat, img_metas)

    def _past_frames_detached(self, feat):
        """PETRHeadseg's with_detach; the identity here."""
        return feat

    def _forward_kernels(self, feat, img_metas):
        return self._decode_kernels(*self._keys_kernels(feat, img_metas), img_metas)

    def _keys_kernels(self, feat, img_metas):
        """The key side in ONE launch -> memory, key_pos (n h w, bs, 256) and the key padding mask (bs, n h w)."""
        bs, n, _, h, w = feat.shape
        dev = feat.device
        pe = self._helper()
        masks, pad_hw = pe.padding_masks(img_metas, [feat])
        x = self._input_proj(feat)
        sine = pe._sine_branch(masks, chlast=True)                                # (bs n, h w, 256), kept
        img = self._images()
        i2l = pe._matrices_device(pe._img2lidar(img_metas), dev)
        se_b2 = self._gate().conv_expand.bias if self.with_fpe else None
        memory, key_pos = ops.petr_keys_fwd(x, i2l, pad_hw, self.depth_num, self.depth_start, self.position_range, img['pe'],
                                            self.position_encoder[2].bias, sine, img['se'], se_b2)
        return memory, key_pos, masks[0].reshape(bs, n * h * w)

    def _decode_kernels(self, memory, key_pos, mask, img_metas):
        """The decoder on the key rows, the branches and the box epilogue."""
        bs = memory.shape[1]
        out_dec = self.transformer.forward_keys(memory, key_pos, mask, self._query_embeds(), self.reg_branches)
        out_dec = torch.nan_to_num(out_dec)
        ref = self.reference_points.weight.detach().unsqueeze(0).expand(bs, -1, -1).contiguous()
        # init_reference = every inter_reference = reference_points: the reference adds inverse_sigmoid(reference_points) at every level
        outs = Fn.head_outputs(out_dec.transpose(1, 2), ref, [ref] * out_dec.shape[0], self.cls_branches, self.reg_branches, self.pc_range)
        if self.with_time:
            # (after the pc_range scaling, which touches columns 0, 1 and 4 only; the reference's broadcast, petrv2_head.py:510)
            boxes = outs['all_bbox_preds']
            boxes[..., 8:] = boxes[..., 8:] / self._mean_time_stamp(img_metas, boxes, bs)
        return outs

    def _sine_expansion(self, masks):
        """SinePositionalEncoding3D of the padding masks in channels-last rows, (R, S, 384): a function of the masks alone, kept while
        padding_masks hands out the same mask objects - the one rows x K tensor that lives across training steps."""
        hit = self.__dict__['_xs']
        if hit is not None and hit[0] is masks[0]:
            return hit[1]
        pe, m = self._helper(), masks[0]
        xs = torch.empty(m.shape[0] * m.shape[1], m.shape[2] * m.shape[3], 3 * pe.num_feats, device=m.device, dtype=torch.float32)
        embeds, dim_t = pe._sine_embeds(m)
        ops.sine_pe3d_fwd(*embeds, dim_t, out=xs, row_start=0)
        self.__dict__['_xs'] = (m, xs)
        return xs

    def _forward_train(self, feat, img_metas):
        """hip_train: the kernel route with autograd - the key side as one node, everything behind it on the library's autograd
        Functions."""
        return self._decode_train(*self._keys_train(feat, img_metas), img_metas)

    def _keys_train(self, feat, img_metas):
        from .autograd import PetrKeysFunction
        bs, n, _, h, w = feat.shape
        pe = self._helper()
        masks, pad_hw = pe.padding_masks(img_metas, [feat])
        ip_image, ip_scale = self._input_proj_image()
        img = self._images()
        conv = self.input_proj
        # The node reads the matrices again in its backward (the frustum is generated again there), and _matrices_device hands out ONE
        # persistent buffer that the next call with other img_metas refreshes in place: a second forward before the first backward
        # (losses summed over samples) would give the first one the second one's cameras.  A private copy, as
        # Fn.lidar2img_device makes under autograd (R x 64 bytes, device to device).
        i2l = pe._matrices_device(pe._img2lidar(img_metas), feat.device).clone()
        geom = dict(i2l=i2l, pad_hw=pad_hw, depth_num=self.depth_num,
                    depth_start=self.depth_start, position_range=self.position_range, xs=self._sine_expansion(masks), ip_image=ip_image,
                    ip_scale=ip_scale, pe_image=img['pe'], se_image=img['se'],
                    ip_image_t=lambda: self._keep('input_proj_t', [conv.weight], lambda: ops.fpn_lateral_image_t(conv.weight.detach())))
        seqs = [self.position_encoder, self.adapt_pos3d] + \
            ([(self._gate().conv_reduce, None, self._gate().conv_expand)] if self.with_fpe else [])
        params = [conv.weight, conv.bias] + [p for q in seqs for c in (q[0], q[2]) for p in (c.weight, c.bias)]
        params += [None] * (14 - len(params))
        memory, key_pos = PetrKeysFunction.apply(feat, geom, *params)
        return memory, key_pos, masks[0].reshape(bs, n * h * w)

    def _decode_train(self, memory, key_pos, mask, img_metas):
        bs = memory.shape[1]
        q0, q2 = self.query_embedding[0], self.query_embedding[2]
        query_embeds = Fn.linear_autograd(Fn.linear_autograd(pos2posemb3d(self.reference_points.weight), q0.weight, q0.bias, relu=True),
                                          q2.weight, q2.bias)                     # (not kept while parameters require grad)
        out_dec = self.transformer.forward_keys(memory, key_pos, mask, query_embeds, self.reg_branches)
        out_dec = torch.nan_to_num(out_dec)
        # (not detached: the reference adds inverse_sigmoid(reference_points) at every level, and BoxHeadFunction hands its gradient back)
        ref = self.reference_points.weight.unsqueeze(0).expand(bs, -1, -1)
        outs = Fn.head_outputs(out_dec.transpose(1, 2), ref, ref.unsqueeze(0).expand(out_dec.shape[0], -1, -1, -1), self.cls_branches,
                               self.reg_branches, self.pc_range)
        if self.with_time:                                   # (not in place: the boxes are an autograd node's output)
            boxes = outs['all_bbox_preds']
            outs['all_bbox_preds'] = torch.cat((boxes[..., :8], boxes[..., 8:] / self._mean_time_stamp(img_metas, boxes, bs)), -1)
        return outs

    def position_embeding(self, img_feats, img_metas, masks=None):
        """petr_head.py:282-327 on torch (the torch-op route)."""
        eps = 1e-5
        pad_h, pad_w, _ = img_metas[0]['pad_shape'][0]
        B, N, C, H, W = img_feats[self.position_level].shape
        dev = img_feats[0].device
        coords_h = torch.arange(H, device=dev).float() * pad_h / H
        coords_w = torch.arange(W, device=dev).float() * pad_w / W
        index = torch.arange(start=0, end=self.depth_num, step=1, device=dev).float()
        if self.LID:
            bin_size = (self.position_range[3] - self.depth_start) / (self.depth_num * (1 + self.depth_num))
            coords_d = self.depth_start + bin_size * index * (index + 1)
        else:
            bin_size = (self.position_range[3] - self.depth_start) / self.depth_num
            coords_d = self.depth_start + bin_size * index
        D = coords_d.shape[0]
        coords = torch.stack(torch.meshgrid([coords_w, coords_h, coords_d], indexing='ij')).permute(1, 2, 3, 0)     # W, H, D, 3
        coords = torch.cat((coords, torch.ones_like(coords[..., :1])), -1)
        coords[..., :2] = coords[..., :2] * torch.maximum(coords[..., 2:3], torch.ones_like(coords[..., 2:3]) * eps)
        img2lidars = np.asarray([[np.linalg.inv(m) for m in meta['lidar2img']] for meta in img_metas])
        img2lidars = coords.new_tensor(img2lidars)                                                   # (B, N, 4, 4)
        coords = coords.view(1, 1, W, H, D, 4, 1).repeat(B, N, 1, 1, 1, 1, 1)
        img2lidars = img2lidars.view(B, N, 1, 1, 1, 4, 4).repeat(1, 1, W, H, D, 1, 1)
        coords3d = torch.matmul(img2lidars, coords).squeeze(-1)[..., :3]
        r = self.position_range
        coords3d[..., 0:1] = (coords3d[..., 0:1] - r[0]) / (r[3] - r[0])
        coords3d[..., 1:2] = (coords3d[..., 1:2] - r[1]) / (r[4] - r[1])
        coords3d[..., 2:3] = (coords3d[..., 2:3] - r[2]) / (r[5] - r[2])
        coords_mask = (coords3d > 1.0) | (coords3d < 0.0)
        coords_mask = coords_mask.flatten(-2).sum(-1) > (D * 0.5)
        coords_mask = masks | coords_mask.permute(0, 1, 3, 2)
        coords3d = coords3d.permute(0, 1, 4, 5, 3, 2).contiguous().view(B * N, -1, H, W)
        coords3d = Fn.inverse_sigmoid(coords3d)
        return self.position_encoder(coords3d).view(B, N, self.embed_dims, H, W), coords_mask

    def _forward_torch(self, mlvl_feats, img_metas):
        """The reference's forward (petr_head.py:359-451, petrv2_head.py:418-529), op for op, on torch."""
        x = self._past_frames_detached(mlvl_feats[self.position_level])
        batch_size, num_cams = x.size(0), x.size(1)
        input_img_h, input_img_w, _ = img_metas[0]['pad_shape'][0]
        masks = x.new_ones((batch_size, num_cams, input_img_h, input_img_w))
        for img_id in range(batch_size):
            for cam_id in range(num_cams):
                img_h, img_w, _ = img_metas[img_id]['img_shape'][cam_id]
                masks[img_id, cam_id, :img_h, :img_w] = 0
        x = self.input_proj(x.flatten(0, 1))
        x = x.view(batch_size, num_cams, *x.shape[-3:])
        masks = F.interpolate(masks, size=x.shape[-2:]).to(torch.bool)
        if self.with_multiview:
            sin_embed = _sine_encoding(masks, self.positional_encoding)
        else:
            sin_embed = torch.cat([_sine_encoding(masks[:, i], self.positional_encoding).unsqueeze(1) for i in range(num_cams)], 1)
        if self.with_position:
            pos_embed, _ = self.position_embeding(mlvl_feats, img_metas, masks)
            if self.with_fpe:
                gate = self._gate().gate_logits(x.flatten(0, 1))
                pos_embed = (pos_embed.flatten(0, 1) * gate.sigmoid()).view(x.size())
            pos_embed = pos_embed + self.adapt_pos3d(sin_embed.flatten(0, 1)).view(x.size())
        elif self.with_multiview:
            pos_embed = self.adapt_pos3d(sin_embed.flatten(0, 1)).view(x.size())
        else:
            pos_embed = sin_embed
        reference_points = self.reference_points.weight
        query_embeds = self.query_embedding(pos2posemb3d(reference_points))
        reference_points = reference_points.unsqueeze(0).repeat(batch_size, 1, 1)
        # every module below the head that has a route of its own takes its torch-op route too (the transformer's, the RegLayers)
        with Fn.torch_ops_for(*[m for m in self.modules() if m is not self and hasattr(m, 'torch_ops')]):
            return self._forward_torch_ops(x, masks, query_embeds, pos_embed, reference_points, img_metas, batch_size)

    def _forward_torch_ops(self, x, masks, query_embeds, pos_embed, reference_points, img_metas, batch_size):
        """The second half of _forward_torch (:419-451 / :485-529): the transformer, the branches and the box epilogue."""
        outs_dec, _ = self.transformer(x, masks, query_embeds, pos_embed, self.reg_branches)
        outs_dec = torch.nan_to_num(outs_dec)
        if self.with_time:
            mean_time_stamp = self._mean_time_stamp(img_metas, x, batch_size)
        outputs_classes, outputs_coords = [], []
        for lvl in range(outs_dec.shape[0]):
            reference = Fn.inverse_sigmoid(reference_points.clone())
            outputs_class = self.cls_branches[lvl](outs_dec[lvl])
            tmp = self.reg_branches[lvl](outs_dec[lvl])
            xy = (tmp[..., 0:2] + reference[..., 0:2]).sigmoid()
            z = (tmp[..., 4:5] + reference[..., 2:3]).sigmoid()
            rest = tmp[..., 5:]
            if self.with_time:
                rest = torch.cat((rest[..., :3], rest[..., 3:] / mean_time_stamp), -1)
            outputs_classes.append(outputs_class)
            outputs_coords.append(torch.cat((xy, tmp[..., 2:4], z, rest), -1))
        all_cls_scores = torch.stack(outputs_classes)
        boxes = torch.stack(outputs_coords)
        pc = self.pc_range
        boxes = torch.cat((boxes[..., 0:1] * (pc[3] - pc[0]) + pc[0], boxes[..., 1:2] * (pc[4] - pc[1]) + pc[1], boxes[..., 2:4],
                           boxes[..., 4:5] * (pc[5] - pc[2]) + pc[2], boxes[..., 5:]), -1)
        return {'all_cls_scores': all_cls_scores, 'all_bbox_preds': boxes, 'enc_cls_scores': None, 'enc_bbox_preds': None}

    # ---- loss / boxes ---------------------------------------------------------------------------------------------------
    def criterion(self):
        """The existing Detr3DCriterion built from this head's loss_* / train_cfg dicts, where it covers them: sigmoid FocalLoss
        (gamma 2) + L1Loss, HungarianAssigner3D with FocalLossCost + BBox3DL1Cost and no IoU term - what every PETR config sets.
        Anything else raises Gd4dError naming it."""
        def build():
            from .criterion import Detr3DCriterion
            lc, lb, li = self.loss_cfg['loss_cls'], self.loss_cfg['loss_bbox'], self.loss_cfg['loss_iou']
            assigner = dict((self.train_cfg or {}).get('assigner') or (self.train_cfg or {}).get('pts', {}).get('assigner') or {})
            no = []
            if lc.get('type') != 'FocalLoss' or not lc.get('use_sigmoid', False) or float(lc.get('gamma', 2.0)) != 2.0:
                no.append(f'loss_cls {lc} (sigmoid FocalLoss with gamma 2 is covered)')
            if lb.get('type') != 'L1Loss':
                no.append(f'loss_bbox {lb} (L1Loss is covered)')
            if float((li or {}).get('loss_weight', 0.0)) != 0.0:
                no.append(f'loss_iou {li} (only loss_weight 0.0: the reference never calls it)')
            if assigner.get('type') != 'HungarianAssigner3D' or assigner.get('cls_cost', {}).get('type') != 'FocalLossCost' or \
                    assigner.get('reg_cost', {}).get('type') != 'BBox3DL1Cost' or float(assigner.get('iou_cost', {}).get('weight', 0.0)) != 0.0:
                no.append(f'train_cfg assigner {assigner} (HungarianAssigner3D with FocalLossCost + BBox3DL1Cost and iou weight 0.0 is covered)')
            if no:
                raise Gd4dError(f'{type(self).__name__}.loss: Detr3DCriterion does not cover ' + '; '.join(no))
            assigner.setdefault('pc_range', self.pc_range)
            crit = Detr3DCriterion(num_classes=self.num_classes, code_weights=self.code_weights.tolist(),
                                   sync_cls_avg_factor=self.sync_cls_avg_factor, bg_cls_weight=0.0, loss_cls=lc, loss_bbox=lb,
                                   assigner=assigner, pc_range=self.pc_range)
            return crit.to(self.code_weights.device)
        # Kept in the plain `_kept` table, NOT as an attribute: an nn.Module assigned to one would become a submodule and its
        # `code_weights` a state-dict key the reference does not have.  It is a value built from `code_weights` like the others: rebuilt
        # when that parameter is reloaded, updated in place or moved to another device (ops._Stamp).
        return self._keep('criterion', [self.code_weights], build)

    def loss(self, gt_bboxes_list, gt_labels_list, preds_dicts, gt_bboxes_ignore=None):
        return self.criterion().loss(gt_bboxes_list, gt_labels_list, preds_dicts, gt_bboxes_ignore)

    def get_bboxes(self, preds_dicts, img_metas, rescale=False):
        """petr_head.py:713-734 through the existing coder."""
        ret_list = []
        for i, preds in enumerate(self.bbox_coder.decode(preds_dicts)):
            bboxes = preds['bboxes']
            bboxes[:, 2] = bboxes[:, 2] - bboxes[:, 5] * 0.5
            box_type = img_metas[i].get('box_type_3d')
            if box_type is not None:
                bboxes = box_type(bboxes, bboxes.size(-1))
            ret_list.append([bboxes, preds['scores'], preds['labels']])
        return ret_list


@HEADS.register_module()
class PETRHead(_PETRHeadBase):
    """petr_head.py:43-734: level 0, no fpe / time / RegLayer; ONE fc_cls and ONE reg_branch object shared by the six levels."""
    _share_branches = True

    def __init__(self, num_classes, in_channels, **kwargs):
        for k in ('position_level', 'group_reg_dims', 'with_fpe', 'with_time', 'with_multi'):
            if k in kwargs:
                raise TypeError(f'PETRHead has no keyword {k!r} (PETRv2Head does)')
        super().__init__(num_classes, in_channels, **kwargs)


@HEADS.register_module()
class PETRv2Head(_PETRHeadBase):
    """petrv2_head.py:91-...: position_level, with_fpe (SELayer gate on input_proj's output), with_time (velocity over the mean
    timestamp difference), with_multi (RegLayer); the six levels hold deep copies of the branches."""
    _share_branches = False


def pos2posemb2d(pos, num_pos_feats=128, temperature=10000):
    """petr_head_seg.py:43-55."""
    pos = pos * (2 * math.pi)
    dim_t = torch.arange(num_pos_feats, dtype=torch.float32, device=pos.device)
    dim_t = temperature ** (2 * (dim_t // 2) / num_pos_feats)
    parts = []
    for axis in (1, 0):                                      # (pos_y, pos_x)
        p = pos[..., axis, None] / dim_t
        parts.append(torch.stack((p[..., 0::2].sin(), p[..., 1::2].cos()), dim=-1).flatten(-2))
    return torch.cat(parts, dim=-1)


@LOSSES.register_module()
class Sigmoid_ce_loss(nn.Module):
    """losses/Sigmoid_ce_loss.py:19-43: binary cross entropy with logits, mean over all elements, each row's positives weighted by
    #(t == 0) / max(#(t == 1), 1).  forward(inputs (R, C), targets (R, C)) -> a scalar, as the reference's.  fp32 tensors on the GPU go
    through gd4d_lane_mask_loss (autograd.LaneMaskLossFunction with one layer); anything else (CPU, other dtypes, torch_ops = True)
    through the reference's four lines.

    layers(logits (L, R, C), targets (R, C)) -> (L,): every decoder layer in ONE call, each value through the nan_to_num of
    petr_head_seg.py:785 - what PETRHeadseg.loss uses.  On the kernel a layer whose loss is not finite gets an all-zero gradient
    (torch leaves a NaN at the offending logit).  The kernel applies the nan_to_num in forward() too - the head applies it to the module's
    result next, and a finite loss is unchanged by it -, the torch lines of forward() are the reference's and do not."""

    def __init__(self, loss_weight=1.0, torch_ops=False):
        super().__init__()
        self.loss_weight = loss_weight
        self.torch_ops = bool(torch_ops)

    def _on_kernel(self, inputs, targets):
        return inputs.is_cuda and inputs.dtype == torch.float32 and targets.dtype == torch.float32 and \
            not Fn.torch_ops_route('Sigmoid_ce_loss', True, module=self)

    def _reference(self, inputs, targets):
        pos_weight = (targets == 0).float().sum(dim=1) / (targets == 1).float().sum(dim=1).clamp(min=1.0)
        weight_loss = targets * pos_weight.unsqueeze(1) + (1 - targets)
        loss = F.binary_cross_entropy_with_logits(inputs, targets, reduction='mean', weight=weight_loss)
        return self.loss_weight * loss

    def layers(self, logits, targets):
        if logits.dim() != 3 or tuple(targets.shape) != tuple(logits.shape[1:]):
            raise ValueError(f'Sigmoid_ce_loss.layers: logits (L, R, C) and targets (R, C) expected, got {tuple(logits.shape)} and '
                             f'{tuple(targets.shape)}')
        if self._on_kernel(logits, targets):
            from .autograd import LaneMaskLossFunction
            return LaneMaskLossFunction.apply(logits, targets, float(self.loss_weight))
        return torch.stack([torch.nan_to_num(self._reference(x, targets)) for x in logits])

    def forward(self, inputs, targets):
        if inputs.dim() == 2 and inputs.shape == targets.shape and inputs.numel() and self._on_kernel(inputs, targets):
            from .autograd import LaneMaskLossFunction
            return LaneMaskLossFunction.apply(inputs.unsqueeze(0), targets, float(self.loss_weight))[0]
        return self._reference(inputs, targets)


@HEADS.register_module()
class PETRHeadseg(_PETRHeadBase):
    """petr_head_seg.py:107-905: PETRv2's detection head plus a BEV map branch.  A second PETRTransformer (`transformer_lane`) runs
    num_lane grid queries - query_embedding_lane(pos2posemb2d(reference_points_lane)) - over the SAME keys as the detection decoder, and
    ONE lane_branches MLP under six names maps every lane query to 768 logits, a 3-class 16 x 16 patch of the map.  The SE gate lives
    under `se.*` (keyword with_se); cls / reg / lane branches are shared by the six levels; reference_points_lane is a plain tensor,
    neither a parameter nor a buffer, and follows the module's moves.

    Kernel route: ONE ops.petr_keys_fwd launch feeds both decoders' forward_keys; the lane query embedding is a kept value; the lane
    branch runs over all layers x bs x num_lane rows at once, three Linear launches.  hip_train: one PetrKeysFunction node feeds both
    decoders (autograd sums their gradients into memory / key_pos), the lane embedding and lane_branches go through Fn.linear_autograd.
    torch_ops=True: the reference's op sequence (:466-602).  with_detach: cameras 6: of the feature map are detached under autograd.

    loss(): the detection terms from criterion(), the lane terms of all layers from ONE gd4d_lane_mask_loss call; the reference reads
    gt_lanes[0] and lane_preds.squeeze(0), so it is meaningful at batch 1 only - a larger batch raises.  get_lane_map(): the decode of
    Petr3D_seg.simple_test_pts (petr3d_seg.py:228-246) on gd4d_lane_map_fwd.

    Limits beyond the base class's: num_lane must be a perfect square (the reference's round(sqrt(num_lane)) silently builds another
    number of queries otherwise).  Left off: the two decoders on two streams."""
    _share_branches = True
    _gate_name = 'se'

    def __init__(self, num_classes, in_channels, num_lane=100, transformer_lane=None, loss_lane_mask=None, with_se=False,
                 with_detach=False, **kwargs):
        if 'with_fpe' in kwargs:
            raise TypeError('PETRHeadseg has no keyword \'with_fpe\' (its gate is with_se, under se.*)')
        grid = round(math.sqrt(num_lane)) if num_lane >= 1 else 0
        if grid < 1 or grid * grid != num_lane:
            raise Gd4dError(f'PETRHeadseg: num_lane = {num_lane} is not a positive perfect square; the reference lays its lane queries out on a '
                            f'round(sqrt(num_lane)) = {grid} x {grid} grid and would silently build {grid * grid} of them - refused on '
                            'every route, torch_ops=True included')
        self.num_lane, self.lane_grid, self.with_se, self.with_detach = num_lane, grid, bool(with_se), bool(with_detach)
        self._lane_cfg = (copy.deepcopy(transformer_lane), copy.deepcopy(loss_lane_mask))
        super().__init__(num_classes, in_channels, with_fpe=with_se, **kwargs)

    def _init_layers(self):
        self.transformer_lane = build_transformer(self._lane_cfg[0])
        self.loss_lane_mask = build_loss(self._lane_cfg[1]) if self._lane_cfg[1] is not None else None
        super()._init_layers()
        c = self.embed_dims
        lane_branch = []
        for _ in range(self.num_reg_fcs):
            lane_branch += [nn.Linear(c, c), nn.ReLU()]
        lane_branch.append(nn.Linear(c, 768))
        lane_branch = nn.Sequential(*lane_branch)
        self.lane_branches = nn.ModuleList([lane_branch for _ in range(self.num_pred)])
        x = (torch.arange(self.lane_grid) + 0.5) / self.lane_grid                      # :365-369, without the .cuda()
        xy = torch.meshgrid(x, x, indexing='ij')
        self.reference_points_lane = torch.cat([xy[0].reshape(-1)[..., None], xy[1].reshape(-1)[..., None]], -1)
        self.query_embedding_lane = nn.Sequential(nn.Linear(c, c), nn.ReLU(), nn.Linear(c, c))

    def init_weights(self):
        super().init_weights()
        self.transformer_lane.init_weights()

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self.reference_points_lane = fn(self.reference_points_lane)            # a plain tensor: moved with the parameters
        return out

    def _past_frames_detached(self, feat):
        if not self.with_detach or not torch.is_grad_enabled():
            return feat
        return torch.cat([feat[:, :6], feat[:, 6:].detach()], 1)                # :484-487

    # ---- the lane half of the three routes ------------------------------------------------------------------------------
    def _lane_points(self):
        return self.reference_points_lane.to(self.query_embedding_lane[0].weight.device)

    def _lane_query_embeds(self):
        """query_embedding_lane(pos2posemb2d(reference_points_lane)): parameters only - kept under the one validity rule."""
        q0, q2 = self.query_embedding_lane[0], self.query_embedding_lane[2]
        return self._keep('query_embeds_lane', [q0.weight, q0.bias, q2.weight, q2.bias],
                          lambda: Fn.linear(Fn.linear(pos2posemb2d(self._lane_points()), q0.weight, q0.bias, relu=True), q2.weight, q2.bias))

    @staticmethod
    def _with_lanes(outs, lanes):
        return {'all_cls_scores': outs['all_cls_scores'], 'all_bbox_preds': outs['all_bbox_preds'], 'all_lane_preds': lanes,
                'enc_cls_scores': None, 'enc_bbox_preds': None}

    def _decode_kernels(self, memory, key_pos, mask, img_metas):
        outs = super()._decode_kernels(memory, key_pos, mask, img_metas)
        lane = torch.nan_to_num(self.transformer_lane.forward_keys(memory, key_pos, mask, self._lane_query_embeds(), self.reg_branches))
        branch = self.lane_branches[0]                       # ONE object under six names: all layers x bs x num_lane rows at once
        x = lane.contiguous().view(-1, lane.shape[-1])
        for m in branch:
            if isinstance(m, nn.Linear):
                x = Fn.linear(x, m.weight, m.bias, relu=m is not branch[-1])
        return self._with_lanes(outs, x.view(*lane.shape[:-1], -1))

    def _decode_train(self, memory, key_pos, mask, img_metas):
        outs = super()._decode_train(memory, key_pos, mask, img_metas)
        q0, q2 = self.query_embedding_lane[0], self.query_embedding_lane[2]
        query_lane = Fn.linear_autograd(Fn.linear_autograd(pos2posemb2d(self._lane_points()), q0.weight, q0.bias, relu=True),
                                        q2.weight, q2.bias)
        lane = torch.nan_to_num(self.transformer_lane.forward_keys(memory, key_pos, mask, query_lane, self.reg_branches))
        x = Fn.sequential_autograd(self.lane_branches[0], lane.contiguous().view(-1, lane.shape[-1]))
        return self._with_lanes(outs, x.view(*lane.shape[:-1], -1))

    def _forward_torch_ops(self, x, masks, query_embeds, pos_embed, reference_points, img_metas, batch_size):
        outs = super()._forward_torch_ops(x, masks, query_embeds, pos_embed, reference_points, img_metas, batch_size)
        query_lane = self.query_embedding_lane(pos2posemb2d(self._lane_points()))
        lane, _ = self.transformer_lane(x, masks, query_lane, pos_embed, self.reg_branches)
        lane = torch.nan_to_num(lane)
        return self._with_lanes(outs, torch.stack([self.lane_branches[lvl](lane[lvl]) for lvl in range(lane.shape[0])]))

    # ---- loss / map --------------------------------------------------------------------------------------------------------
    def loss(self, gt_bboxes_list, gt_labels_list, preds_dicts, gt_lanes, gt_bboxes_ignore=None):
        """petr_head_seg.py:790-881: the reference's keys - loss_cls, loss_bbox, loss_mask and d{i}.* of the earlier layers.  gt_lanes[0]
        is the (num_lane, 768) target every layer is compared with."""
        lanes = preds_dicts['all_lane_preds']
        if lanes.shape[1] != 1:
            raise Gd4dError(f'PETRHeadseg.loss: batch size {lanes.shape[1]}; the reference compares lane_preds.squeeze(0) with gt_lanes[0] '
                            '(petr_head_seg.py:782-784), which is meaningful at batch size 1 only - on every route, torch_ops=True included')
        if self.loss_lane_mask is None:
            raise Gd4dError('PETRHeadseg.loss: the head was built without loss_lane_mask (dict(type=\'Sigmoid_ce_loss\', ...))')
        det = self.criterion().loss(gt_bboxes_list, gt_labels_list, preds_dicts, gt_bboxes_ignore)
        with Fn.torch_ops_for(*([self.loss_lane_mask] if self.torch_ops else [])):
            masks = self.loss_lane_mask.layers(lanes.squeeze(1), gt_lanes[0])             # (layers,): ONE call
        out = {'loss_cls': det['loss_cls'], 'loss_bbox': det['loss_bbox'], 'loss_mask': masks[-1]}
        for i in range(lanes.shape[0] - 1):
            out[f'd{i}.loss_cls'], out[f'd{i}.loss_bbox'], out[f'd{i}.loss_mask'] = det[f'd{i}.loss_cls'], det[f'd{i}.loss_bbox'], masks[i]
        return out

    def get_lane_map(self, preds_dicts, gt_map=None):
        """The LAST layer's logits (B, g g, 768) -> (binary map (B, 3, 16 g, 16 g) of 0 / 1, iou (B, 3) against gt_map or None)."""
        logits = preds_dicts['all_lane_preds'][-1]
        covered = logits.is_cuda and logits.dtype == torch.float32 and (gt_map is None or (gt_map.is_cuda and gt_map.dtype == torch.float32))
        if not Fn.torch_ops_route(f'PETRHeadseg.get_lane_map on {logits.device}, dtype {logits.dtype}', covered, module=self):
            with torch.no_grad():
                res = ops.lane_map_fwd(logits.detach().contiguous(), None if gt_map is None else gt_map.contiguous())
            return res[1], (res[3] if gt_map is not None else None)
        with torch.no_grad():                                # petr3d_seg.py:228-246, for any batch and grid
            b, g = logits.shape[0], self.lane_grid
            f_lane = logits.view(b, g, g, 3, 16, 16).permute(0, 3, 1, 4, 2, 5).reshape(b, 3, 16 * g, 16 * g).sigmoid()
            f_lane[f_lane >= 0.5] = 1
            f_lane[f_lane < 0.5] = 0
            iou = None
            if gt_map is not None:
                p, t = f_lane.flatten(2), gt_map.flatten(2)
                iou = (2 * (p * t).sum(dim=2) + 0.01) / (p.sum(dim=2) + t.sum(dim=2) + 0.01)
        return f_lane, iou
