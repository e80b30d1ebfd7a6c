"""fp64 restatement of the lane half of PETRHeadseg (reference: dense_heads/petr_head_seg.py:43-55 pos2posemb2d, :313-318 / :572 the
lane branch, losses/Sigmoid_ce_loss.py:39-43, detectors/petr3d_seg.py:25-29 and :228-246), the fixture's config, and the inputs / cases
of the lane tests as data.  The detection half, the parameter rule and the inputs are tests/petr_head_ref.py's, used as they are: the
head's gate lives under `se.*` here and under `fpe.*` there, so the state dict is handed over with those keys renamed.  Nothing here
imports the package's kernels.

The parameter rule is petr_head_ref.draw's; the six `cls_branches.N.` / `reg_branches.N.` / `lane_branches.N.` names are one shared
module each and are drawn under N = 0.
"""
import math
import re

import numpy as np
import torch

import petr_head_ref as P

F64 = torch.float64
R = P.R
NUM_LANE = 4
LOSS_WEIGHT = 1.0


def draw(name, shape):
    name = re.sub(r'^lane_branches\.\d+\.', 'lane_branches.0.', name)
    return P.draw(name, shape, shared=True)


def state_dict(keys, shapes):
    return {k: draw(k, s) for k, s in zip(keys, shapes)}


def head_config(**over):
    """The v2 fixture's head block plus the lane half of projects/configs/petrv2/petrv2_BEVseg.py:40-125 at 4 lane queries."""
    cfg = P.head_config('v2')
    del cfg['with_fpe']
    cfg.update(type='PETRHeadseg', num_lane=NUM_LANE, with_se=True, transformer_lane=R.petr_config(P.LAYERS, P.FFN),
               loss_lane_mask=dict(type='Sigmoid_ce_loss', loss_weight=LOSS_WEIGHT), train_cfg=None)
    cfg.update(over)
    return cfg


# ---- the restatement -------------------------------------------------------------------------------------------------------
def pos2posemb2d(pos, num_pos_feats=128, temperature=10000):
    pos = pos.to(F64) * (2 * math.pi)
    dim_t = torch.arange(num_pos_feats, dtype=F64)
    dim_t = temperature ** (2 * (dim_t // 2) / num_pos_feats)
    parts = []
    for axis in (1, 0):
        p = pos[..., axis, None] / dim_t
        parts.append(torch.stack((p[..., 0::2].sin(), p[..., 1::2].cos()), dim=-1).flatten(-2))
    return torch.cat(parts, dim=-1)


def lane_points(num_lane):
    """petr_head_seg.py:365-369: the centres of a g x g grid, the first coordinate the slow one."""
    g = round(math.sqrt(num_lane))
    x = (torch.arange(g, dtype=F64) + 0.5) / g
    xy = torch.meshgrid(x, x, indexing='ij')
    return torch.stack((xy[0].reshape(-1), xy[1].reshape(-1)), -1)


def head_forward(sd, cfg, feat, metas):
    """-> petr_head_ref.head_forward's dict for the detection half, plus query_embeds_lane (num_lane, 256) and all_lane_preds
    (layers, bs, num_lane, 768), float64."""
    det_sd = {('fpe.' + k[3:] if k.startswith('se.') else k): v for k, v in sd.items()}
    det_cfg = dict(cfg, with_fpe=cfg.get('with_se', False))
    out = P.head_forward(det_sd, det_cfg, feat, metas)
    masks = P.padding_masks(metas, tuple(feat.shape[-2:]))
    emb = pos2posemb2d(lane_points(cfg['num_lane']))
    query_lane = R.linear(torch.relu(R.linear(emb, sd['query_embedding_lane.0.weight'], sd['query_embedding_lane.0.bias'])),
                          sd['query_embedding_lane.2.weight'], sd['query_embedding_lane.2.bias'])
    tsd = {k[len('transformer_lane.'):]: v for k, v in sd.items() if k.startswith('transformer_lane.')}
    lane, _, _ = R.transformer(tsd, 8, cfg['transformer_lane']['decoder']['num_layers'], out['x'], masks, query_lane, out['pos_embed'])
    lane = torch.nan_to_num(lane)
    out['query_embeds_lane'] = query_lane
    out['all_lane_preds'] = torch.stack([P.sequential(sd, f'lane_branches.{lvl}.', lane[lvl]) for lvl in range(lane.shape[0])])
    return out


def sigmoid_ce(x, t, loss_weight=1.0):
    """Sigmoid_ce_loss.py:39-43 for ONE layer, x / t (R, C) -> (loss before nan_to_num, d loss / d x, the weights w), float64."""
    x, t = x.to(F64), t.to(F64)
    pw = (t == 0).to(F64).sum(1) / (t == 1).to(F64).sum(1).clamp(min=1.0)
    w = t * pw[:, None] + (1 - t)
    term = x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
    loss = loss_weight * (w * term).sum() / x.numel()
    grad = loss_weight * w * (torch.sigmoid(x) - t) / x.numel()
    return loss, grad, w


def fp32_sigmoid(x):
    """1 / (1 + exp(-x)) with every operation rounded to fp32 (exp correctly rounded): the value `binary` is defined on."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over='ignore'):
        e = np.exp(-x.astype(np.float64)).astype(np.float32)
    return np.float32(1) / (np.float32(1) + e)


def lane_map(logits, gt_map=None):
    """petr3d_seg.py:228-246 for any batch and grid: logits (B, g g, 768) fp32 -> prob (fp64 sigmoid), binary (0 / 1 int64, taken on the
    fp32 sigmoid), and with gt_map the int sums (B, 3, 3) = inter, sum(binary), sum(gt) and the fp64 iou (B, 3)."""
    b, n, _ = logits.shape
    g = round(math.sqrt(n))
    place = lambda v: v.view(b, g, g, 3, 16, 16).permute(0, 3, 1, 4, 2, 5).reshape(b, 3, 16 * g, 16 * g)      # noqa: E731
    prob = torch.sigmoid(place(logits.to(F64)))
    binary = place(torch.from_numpy(fp32_sigmoid(logits.numpy()) >= np.float32(0.5))).to(torch.int64)
    if gt_map is None:
        return prob, binary, None, None
    gt = gt_map.to(torch.int64)
    assert torch.equal(gt.to(gt_map.dtype), gt_map), 'the restatement takes 0 / 1 maps'
    sums = torch.stack(((binary * gt).flatten(2).sum(2), binary.flatten(2).sum(2), gt.flatten(2).sum(2)), -1)
    iou = (2 * sums[..., 0].to(F64) + 0.01) / ((sums[..., 1] + sums[..., 2]).to(F64) + 0.01)
    return prob, binary, sums, iou


# ---- the cases, as data ------------------------------------------------------------------------------------------------------
def _hash(n, salt):
    i = np.arange(n, dtype=np.uint64)
    h = (i * np.uint64(2654435761) + np.uint64(salt)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    return h


def loss_case(nl, r, c):
    """logits (L, R, C) on the k / 8 grid in [-3, 3] with one + 90 and one - 90 per layer (the naive log(1 + exp(x)) overflows there), and
    targets (R, C) of 0 / 1: row r % 3 == 0 has every tenth element positive, r % 3 == 1 none (the clamp), r % 3 == 2 all (pw = 0)."""
    n = nl * r * c
    x = ((_hash(n, 17 * r + c) % np.uint64(49)).astype(np.float32) - 24.0) / 8.0
    x = x.reshape(nl, r * c)
    x[:, 0] = 90.0
    x[:, (r * c) // 2] = -90.0 if r * c > 1 else 90.0
    t = np.zeros((r, c), dtype=np.float32)
    for row in range(r):
        if row % 3 == 0:
            t[row, ::10] = 1.0
        elif row % 3 == 2:
            t[row] = 1.0
    return torch.from_numpy(x.reshape(nl, r, c).copy()), torch.from_numpy(t)


LOSS_SHAPES = [(nl, r, c) for nl in (1, 6) for r in (1, 4, 9) for c in (1, 63, 64, 65, 768)]
FIXTURE_LOSS_SHAPES = [(4, 65), (9, 64)]            # the (R, C) whose reference loss and gradient the fixture records (layer 0 of L = 1)
MAP_GRIDS = (1, 2, 3, 16)


def map_case(b, g):
    """logits (B, g g, 768) on the k / 8 grid in [-2, 2] - exact zeros included -, element 0 of every query = -2^-30 (fp32 sigmoid
    exactly 0.5: binary 1) and element 1 = -2^-10 (binary 0); gt (B, 3, 16 g, 16 g) of 0 / 1."""
    n = b * g * g * 768
    x = ((_hash(n, 3 * g + b) % np.uint64(33)).astype(np.float32) - 16.0) / 8.0
    x = x.reshape(b, g * g, 768)
    x[:, :, 0] = -2.0 ** -30
    x[:, :, 1] = -2.0 ** -10
    x[:, :, 2] = 0.0
    gt = (_hash(b * 3 * 256 * g * g, 7 * g + 1) % np.uint64(3) == 0).astype(np.float32).reshape(b, 3, 16 * g, 16 * g)
    return torch.from_numpy(x.copy()), torch.from_numpy(gt)
