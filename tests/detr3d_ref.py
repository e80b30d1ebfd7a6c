"""The two DETR3D-baseline sampling cores (Detr3DCrossAtten, Detr3DCrossAttenV2) in plain torch, restated from the formulas; what the
kernel tests of gd4d_detr3d.hip compare against.  It shares no code with the package.  Every function computes in the dtype of
`ref` (the tests call it in fp64 for the reference and in fp32 for the error of honest fp32 arithmetic) and is differentiable
in feats, ref, logits and offsets; gradients come from torch autograd.
    point        p = ref * (hi - lo) + lo                                       (metres)
    camera n     (cx, cy, cz) = rows 0-2 of lidar2img[n] applied to (p, 1)
    image        u = cx / max(cz, 1e-5) / img_w, v = cy / max(cz, 1e-5) / img_h ; grid g = ((u, v) - 0.5) * 2
    visible      cz > 1e-5 and -1 < g.x < 1 and -1 < g.y < 1                    (strict; no gradient)
    sample       bilinear, zero padding, align_corners=False: x = ((g.x + 1) W - 1) / 2, corners floor(x), floor(x) + 1, a corner
                 outside the map contributes 0 - written out by corners, so a coordinate far beyond the int range is defined (0)
    detr3d       out[b, q, c] = sum_{n, l} sigmoid(logit[b, q, n, l]) vis[b, n, q] sample_l(feats[l][b, n, c], g[b, n, q])
    detr3d_v2    W[b, q, n, h, :] = softmax over L * P of logits[b, q, n, h, :], times vis
                 out[b, q, c] = sum_{n, l, pt} W[b, q, n, h, pt, l] sample_l(feats[l][b, n, c], g[b, n, q] + off[b, q, n, h, l, pt] / (W_l, H_l))
                 with h = c // (C / heads): the sample at (level l, point pt) meets the weight at [pt, l] (the reference's pairing,
                 well-formed for P == L only)."""
import torch

DEPTH_EPS = 1e-5


def rel_err(got, want):
    """max |got - want| over the largest |entry| of want (0 for two all-zero tensors)."""
    scale = float(want.abs().max()) if want.numel() else 0.0
    diff = float((got.to(want.dtype) - want).abs().max()) if want.numel() else 0.0
    return diff / scale if scale > 0 else (0.0 if diff == 0 else float('inf'))


def row_rel_err(got, want, row_dims):
    """The largest error over rows: the last `row_dims` dimensions form a row, and a row's max |got - want| is divided by its own
    largest |entry| - but by no less than the median of that over the tensor's non-zero rows: a row far below the median is one
    whose sum over channels cancelled, and the rounding error of a sum goes with its terms, not with its result.  So one wrong row
    is measured against rows like itself, never against the largest row of the tensor.  A row whose reference is all zero
    counts inf unless `got` is zero there too."""
    w = want.reshape(-1, *want.shape[want.dim() - row_dims:]).flatten(1)
    g = got.to(want.dtype).reshape(w.shape)
    diff, scale = (g - w).abs().amax(1), w.abs().amax(1)
    zero = scale == 0
    if bool((diff[zero] != 0).any()):
        return float('inf')
    live = ~zero
    if not bool(live.any()):
        return 0.0
    scale = scale[live].clamp(min=float(scale[live].median()))
    return float((diff[live] / scale).max())


def project(ref, lidar2img, pc_range, img_h, img_w):
    """ref (B, Q, 3) in [0, 1], lidar2img (B, N, 4, 4) -> grid (B, N, Q, 2) in [-1, 1] where visible, depth (B, N, Q) (unclamped),
    visible (B, N, Q) bool."""
    dt = ref.dtype
    rng = torch.as_tensor(pc_range, dtype=torch.float64)
    lo, scale = rng[:3].to(dt), (rng[3:] - rng[:3]).to(dt)
    p = ref * scale + lo                                                            # (B, Q, 3)
    m = lidar2img.to(dt)
    cam = torch.einsum('bnij,bqj->bnqi', m[:, :, :3, :3], p) + m[:, :, None, :3, 3]    # (B, N, Q, 3)
    depth = cam[..., 2]
    zc = depth.clamp(min=DEPTH_EPS)
    u = cam[..., 0] / zc / img_w
    v = cam[..., 1] / zc / img_h
    grid = (torch.stack([u, v], -1) - 0.5) * 2
    vis = (depth > DEPTH_EPS) & (grid[..., 0] > -1) & (grid[..., 0] < 1) & (grid[..., 1] > -1) & (grid[..., 1] < 1)
    return grid, depth, vis


def pixel_coords(g, size):
    """grid coordinate -> pixel coordinate of a map with `size` pixels along that axis (align_corners=False)."""
    return ((g + 1) * size - 1) / 2


def sample(feats, gx, gy):
    """feats (M, C, H, W), grid coordinates gx, gy (M, K) -> (M, C, K): bilinear, zero padding, align_corners=False, by corners."""
    m, c, h, w = feats.shape
    x, y = pixel_coords(gx, w), pixel_coords(gy, h)
    x0, y0 = torch.floor(x).detach(), torch.floor(y).detach()
    dx, dy = x - x0, y - y0
    flat = feats.reshape(m, c, h * w)
    out = 0
    for ox, oy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        xi, yi = x0 + ox, y0 + oy
        inside = (xi >= 0) & (xi <= w - 1) & (yi >= 0) & (yi <= h - 1)
        idx = (yi.clamp(0, h - 1) * w + xi.clamp(0, w - 1)).long()                  # clamped in floating point first: always defined
        val = torch.gather(flat, 2, idx[:, None, :].expand(m, c, -1))
        wgt = (dx if ox else 1 - dx) * (dy if oy else 1 - dy)
        out = out + val * torch.where(inside, wgt, torch.zeros_like(wgt))[:, None, :]
    return out


def detr3d(feats, ref, logits, lidar2img, pc_range, img_h, img_w):
    """feats: L maps (B, N, C, H_l, W_l); logits: B * Q * N * L elements in (B, Q, N, 1, L) order.
    -> out (B, Q, C), mask (B, N, Q) bool, sampled (B, C, Q, N, 1, L) (every camera, visible or not)."""
    b, n, c = feats[0].shape[:3]
    q, nl = ref.shape[1], len(feats)
    grid, _, vis = project(ref, lidar2img, pc_range, img_h, img_w)
    gx, gy = grid[..., 0].reshape(b * n, q), grid[..., 1].reshape(b * n, q)
    per_level = [sample(f.to(ref.dtype).reshape(b * n, c, *f.shape[-2:]), gx, gy).reshape(b, n, c, q) for f in feats]
    sampled = torch.stack(per_level, -1)                                            # (B, N, C, Q, L)
    w = torch.sigmoid(logits.reshape(b, q, n, nl)) * vis.permute(0, 2, 1)[..., None].to(ref.dtype)
    out = torch.einsum('bqnl,bncql->bqc', w, sampled)
    return out, vis, sampled.permute(0, 2, 3, 1, 4).unsqueeze(4)


def v2_grid(grid, offsets, level, w, h):
    """grid (B, N, Q, 2), offsets (B, Q, N, Hh, L, P, 2) -> the sampling grid coordinates of `level`: gx, gy (B, N, Hh, Q, P)."""
    off = offsets[:, :, :, :, level].permute(0, 2, 3, 1, 4, 5)                      # (B, N, Hh, Q, P, 2)
    return grid[:, :, None, :, None, 0] + off[..., 0] / w, grid[:, :, None, :, None, 1] + off[..., 1] / h


def detr3d_v2(feats, ref, logits, offsets, lidar2img, pc_range, img_h, img_w, num_heads):
    """logits (B, Q, N, Hh, L * P), offsets (B, Q, N, Hh, L, P, 2) in pixels of the level, P == L -> out (B, Q, C), mask (B, N, Q)."""
    b, n, c = feats[0].shape[:3]
    q, nl, hh = ref.shape[1], len(feats), num_heads
    dh = c // hh
    grid, _, vis = project(ref, lidar2img, pc_range, img_h, img_w)
    w = torch.softmax(logits.reshape(b, q, n, hh, nl * nl), -1).reshape(b, q, n, hh, nl, nl)
    w = w * vis.permute(0, 2, 1)[..., None, None, None].to(ref.dtype)
    out = 0
    for l, f in enumerate(feats):
        fh, fw = f.shape[-2:]
        gx, gy = v2_grid(grid, offsets.reshape(b, q, n, hh, nl, nl, 2), l, fw, fh)
        s = sample(f.to(ref.dtype).reshape(b * n * hh, dh, fh, fw), gx.reshape(b * n * hh, q * nl), gy.reshape(b * n * hh, q * nl))
        s = s.reshape(b, n, hh, dh, q, nl)                                          # [..., pt]
        out = out + torch.einsum('bqnhp,bnhdqp->bqhd', w[..., l], s)                # weight [pt, l] for every pt
    return out.reshape(b, q, c), vis
