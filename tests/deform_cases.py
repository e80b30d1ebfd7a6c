"""Inputs for the kernel tests of Deform3DCrossAttn's hot path (gd4d_cross_attn*.hip), chosen from the oracle alone: nothing here looks at
a kernel's output, and every case asserts its own conditions (check_case) before anything touches the GPU.  The arbiter is
oracle/torch_oracle.py::sample_aggregate on value = value_proj(flatten_pyramid(feats)), evaluated in float64 with fp64 autograd.

Rig, image and range are detr3d_cases.py's (rig, focal, 64 x 112, PC_RANGE).  The geometry is not DETR3D's and is restated here
(geometry): offsets are 3-D, in metres, per (query, head, point); one projected (u, v) serves every level; a sample is visible iff
z > 1e-5 and 0 < u < 1 and 0 < v < 1; its pixel coordinate on a W x H level is (u W - 0.5, v H - 0.5) with zero padding, so a visible
sample lies up to half a pixel beyond each border of every level, and a sample in the finest level's band is in every level's band.

Queries of every batch entry, in this order (ref is uniform in [0, 1]^3 everywhere; a placed sample gets the offset that carries it
from ref to the inverse projection of a chosen (camera, finest-level pixel, depth); every other offset is N(0, 2 m)):
  random     37 queries
  sides      4: sample (head 0, point 0) in the half-pixel band beyond the left / right / top / bottom border of camera 0, and sample
             (last head, last point) in the same band of camera N - 1
  corners    4: the same two samples beyond two borders at once (one bilinear corner on the map).  Camera 0 of batch entry 0 and
             camera N - 1 of batch entry B - 1 are the maps at the two ends of every pyramid allocation.
  shared     4: sample (0, 0) in the overlap of two neighbouring cameras
  nobody     1: every sample 300 m above the rig, outside every image
  behind     1: sample (0, 0) behind camera 0: its depth is clamped to 1e-5, the projection lands about 1e8 pixels away
  level      2: sample (0, 0) of camera 0 at u = 1 + d and at u = -d with 1.5 / W_0 < d < 0.5 / W_coarsest: not visible, more than one
             cell beyond the finest map, inside a cell that touches the coarsest one - the same (u, v) hits different cases per level,
             and only the visibility mask keeps it out.  The converse (on the finest map, beyond a coarser one) cannot happen:
             x_l + 0.5 = (x_0 + 0.5) W_l / W_0 with W_l < W_0 (check_case asserts it on every sample).
  block      32: all 32 samples of the query inside one bilinear cell of the coarsest level of camera 1 (offsets within centimetres of
             the placed point): many records of one pixel group in the bucket sort.

Margins (fp64, on the fp32 inputs, for every sample, camera and level; they make fp32 and fp64 agree on every visibility bit and cell):
  visibility   u and v differ from 0 and 1, and z from 1e-5, by more than 1e-3
  cell         both pixel coordinates are more than 1e-3 away from an integer - unless the sample lies more than 1e-3 beyond the last
               cell that touches the map (detr3d_cases.cell_margin_ok)."""
import math

import torch
import torch.nn.functional as F

import detr3d_cases as D
import detr3d_ref as R
from oracle import torch_oracle as O

F64 = torch.float64
IMG_H, IMG_W, PC_RANGE, MARGIN, FACTOR = D.IMG_H, D.IMG_W, D.PC_RANGE, D.MARGIN, D.FACTOR
EPS = 1e-5
C, P = 256, 4
Q_RANDOM, Q_BLOCK = 37, 32

# name -> B, N, heads, levels (H, W)
SHAPES = {
    'base': (1, 6, 8, [(16, 28), (8, 14), (4, 7), (2, 4)]),
    'batch2': (2, 6, 8, [(16, 28), (8, 14), (4, 7), (2, 4)]),
    'narrow': (2, 3, 4, [(5, 9), (3, 5), (1, 2)]),     # 4 heads: test_raw_backward_matches_projected_backward parametrizes that count
}
SEEDS = {'base': 4201, 'batch2': 4202, 'narrow': 4203}


def geometry(ref, offsets, lidar2img):
    """The projection restated in fp64 on the given (fp32) inputs -> u, v, z (B, N, Q, Hh, P) and the visibility mask."""
    rng = torch.tensor(PC_RANGE, dtype=F64)
    pts = ref.to(F64)[:, :, None, None, :] * (rng[3:] - rng[:3]) + rng[:3] + offsets.to(F64)
    hom = torch.cat((pts, torch.ones_like(pts[..., :1])), -1)
    cam = torch.einsum('bnij,bqhpj->bnqhpi', lidar2img.to(F64), hom)
    z = cam[..., 2]
    u, v = cam[..., 0] / z.clamp(min=EPS) / IMG_W, cam[..., 1] / z.clamp(min=EPS) / IMG_H
    return u, v, z, (z > EPS) & (u > 0) & (u < 1) & (v > 0) & (v < 1)


def pixel(u, size):
    return u * size - 0.5


def margins(ref, offsets, lidar2img, levels):
    """-> (B, Q) bool: both margins of the module docstring hold for every sample of the query, on every camera and level."""
    u, v, z, _ = geometry(ref, offsets, lidar2img)
    ok = (u.abs() > MARGIN) & ((u - 1).abs() > MARGIN) & (v.abs() > MARGIN) & ((v - 1).abs() > MARGIN) & ((z - EPS).abs() > MARGIN)
    for h, w in levels:
        ok &= D.cell_margin_ok(pixel(u, w), pixel(v, h), w, h)
    return ok.permute(0, 2, 1, 3, 4).flatten(2).all(2)


class Case:
    pass


def build(name):
    b, n, hh, levels = SHAPES[name]
    nl = len(levels)
    gen = torch.Generator().manual_seed(SEEDS[name])
    m64, rot, centre, k = D.rig(b, n, gen)
    l2i = m64.float()
    (fh, fw), (ch, cw) = levels[0], levels[-1]
    rng = torch.tensor(PC_RANGE, dtype=F64)
    block_cam = 1
    bx, by = (cw - 1) // 2, (ch - 1) // 2
    in_x, in_y = ((0.3, 0.7) if cw > 1 else (0.1, 0.4)), ((0.3, 0.7) if ch > 1 else (0.1, 0.4))
    u_shared = math.tan(math.pi / n) / math.tan(math.pi / n + math.radians(5.0))
    last = (hh - 1, P - 1)

    def px(g, size):
        return R.pixel_coords(torch.tensor(g, dtype=F64), size).item()
    any_x, any_y = (-0.4, fw - 0.6), (-0.4, fh - 0.6)
    lo, hi_x, hi_y = (-0.45, -0.05), (fw - 0.95, fw - 0.55), (fh - 0.95, fh - 0.55)
    mid_y = (0.2 * fh - 0.5, 0.8 * fh - 0.5)
    d_lo, d_hi = 1.6 / fw, 0.45 / cw
    assert d_lo < d_hi
    ends = lambda xr, yr: [((0, 0), 0, xr, yr, (6, 30)), (last, n - 1, xr, yr, (6, 30))]          # noqa: E731
    # (kind, [(head, point), camera, x range, y range, depth range]): pixel coordinates of the finest level
    specs = [('side-left', ends(lo, any_y)), ('side-right', ends(hi_x, any_y)), ('side-top', ends(any_x, lo)), ('side-bottom', ends(any_x, hi_y)),
             ('corner', ends(lo, lo)), ('corner', ends(hi_x, lo)), ('corner', ends(lo, hi_y)), ('corner', ends(hi_x, hi_y))]
    specs += [('shared', [((0, 0), i % n, (px(u_shared - 0.08, fw), px(u_shared + 0.08, fw)), (px(-0.6, fh), px(0.6, fh)), (8, 30))])
              for i in range(4)]
    specs += [('nobody', [])]
    specs += [('behind', [((0, 0), 0, (px(-0.8, fw), px(0.8, fw)), (px(-0.8, fh), px(0.8, fh)), (-30, -8))])]
    specs += [('level', [((0, 0), 0, ((1 + d_lo) * fw - 0.5, (1 + d_hi) * fw - 0.5), mid_y, (6, 30))]),
              ('level', [((0, 0), 0, (-d_hi * fw - 0.5, -d_lo * fw - 0.5), mid_y, (6, 30))])]
    kinds = ['random'] * Q_RANDOM + [s[0] for s in specs] + ['block'] * Q_BLOCK
    q = len(kinds)
    ref = torch.zeros(b, q, 3)
    offsets = torch.zeros(b, q, hh, P, 3)

    def uniform(lo_, hi_):
        return lo_ + (hi_ - lo_) * torch.rand((), generator=gen, dtype=F64).item()

    def target(bi, cam, x, y, depth):
        """The point (metres) that camera `cam` sees at finest-level pixel (x, y) and `depth`."""
        pix = torch.tensor([(x + 0.5) / fw * IMG_W, (y + 0.5) / fh * IMG_H, 1.0], dtype=F64)
        return rot[cam].T @ (depth * torch.linalg.solve(k, pix)) + centre[bi, cam]

    def candidate(bi, placed, spread=2.0, lift=0.0, block=None):
        r = torch.rand(3, generator=gen, dtype=F64).float()
        base = r.to(F64) * (rng[3:] - rng[:3]) + rng[:3]
        off = torch.randn(hh, P, 3, generator=gen, dtype=F64) * spread
        off[..., 2] += lift
        if block is not None:
            off += block - base
        for (h_, p_), cam, xr, yr, dr in placed:
            off[h_, p_] = target(bi, cam, uniform(*xr), uniform(*yr), uniform(*dr)) - base
        return r, off.float()

    def accept(bi, qi, r, off):
        if bool(margins(r.view(1, 1, 3), off.view(1, 1, hh, P, 3), l2i[bi:bi + 1], levels)):
            ref[bi, qi], offsets[bi, qi] = r, off
            return True
        return False

    for bi in range(b):
        qi, tried = 0, 0
        while qi < Q_RANDOM:
            tried += 1
            assert tried < 20 * Q_RANDOM, 'the margins reject almost every candidate: the rig or the margins are wrong'
            if accept(bi, qi, *candidate(bi, [])):
                qi += 1
        for kind, placed in specs:
            for _ in range(200):
                if accept(bi, qi, *candidate(bi, placed, lift=300.0 if kind == 'nobody' else 0.0)):
                    break
            else:
                raise AssertionError(f'no {kind} query passes the margins')
            qi += 1
        for _ in range(Q_BLOCK):
            for _ in range(200):
                x = ((bx + uniform(*in_x)) + 0.5) / cw * fw - 0.5                   # the coarsest level's cell, in finest-level pixels
                y = ((by + uniform(*in_y)) + 0.5) / ch * fh - 0.5
                if accept(bi, qi, *candidate(bi, [], spread=0.04, block=target(bi, block_cam, x, y, uniform(8, 30)))):
                    break
            else:
                raise AssertionError('no block query passes the margins')
            qi += 1
        assert qi == q
    cs = Case()
    cs.name, cs.B, cs.N, cs.C, cs.Hh, cs.P, cs.levels, cs.L, cs.Q = name, b, n, C, hh, P, levels, nl, q
    cs.kinds, cs.block, cs.block_cam, cs.block_cell, cs.last = kinds, slice(q - Q_BLOCK, q), block_cam, (bx, by), last
    cs.ref, cs.offsets, cs.lidar2img = ref, offsets, l2i
    cs.feats = [torch.randn(b, n, C, h, w, generator=gen) for h, w in levels]
    cs.attn = torch.randn(b, q, hh, nl, P, generator=gen)
    cs.cam = torch.randn(b, q, n, generator=gen)
    cs.w_v, cs.b_v = torch.randn(C, C, generator=gen) / 16, torch.randn(C, generator=gen)
    cs.grad_out, cs.grad_out2 = torch.randn(b, q, C, generator=gen), torch.randn(b, q, C, generator=gen)
    return cs


_CASES = {}


def case(name):
    """The case, built once per process and shared (nobody writes into it)."""
    if name not in _CASES:
        _CASES[name] = build(name)
    return _CASES[name]


def of_kind(cs, kind):
    return [i for i, kd in enumerate(cs.kinds) if kd.startswith(kind)]


def block_pixels(cs):
    """(y, x) of the block cell's corners that are on the coarsest map."""
    ch, cw = cs.levels[-1]
    bx, by = cs.block_cell
    return [(y, x) for y in (by, by + 1) for x in (bx, bx + 1) if 0 <= x < cw and 0 <= y < ch]


def corners_on_map(x, y, w, h):
    """How many of the four bilinear corners of (x, y) lie on a W x H map."""
    x0, y0 = torch.floor(x), torch.floor(y)
    return sum(((xx >= 0) & (xx <= w - 1) & (yy >= 0) & (yy <= h - 1)).long() for yy in (y0, y0 + 1) for xx in (x0, x0 + 1))


def check_case(cs):
    """The conditions the tests rely on, from the oracle and the restated geometry alone.  Returns the counts it asserted on."""
    assert bool(margins(cs.ref, cs.offsets, cs.lidar2img, cs.levels).all()), 'margins'
    u, v, z, vis = geometry(cs.ref, cs.offsets, cs.lidar2img)                       # (B, N, Q, Hh, P)
    b, n, q, hh = cs.B, cs.N, cs.Q, cs.Hh
    # the oracle's projection is the restated one, and decides every visibility bit alike in fp64 and in fp32 on the host
    pts = lambda t: (O.denormalise(cs.ref.to(t), PC_RANGE).view(b, q, 1, 1, 3) + cs.offsets.to(t)).reshape(b, q * hh * P, 3)   # noqa: E731
    uv64, m64 = O.project(pts(F64), cs.lidar2img.to(F64), IMG_H, IMG_W)
    _, m32 = O.project(pts(torch.float32), cs.lidar2img, IMG_H, IMG_W)
    assert torch.equal(m64.view(vis.shape), vis) and torch.equal(m32.view(vis.shape), vis), 'visibility: oracle fp64 / fp32 / restatement'
    assert float((uv64.view(b, n, q, hh, P, 2)[vis] - torch.stack((u, v), -1)[vis]).abs().max()) < 1e-12
    (fh, fw), (ch, cw) = cs.levels[0], cs.levels[-1]
    x, y = pixel(u, fw), pixel(v, fh)
    seen = vis.sum(1)                                                               # (B, Q, Hh, P): cameras that see the sample
    counts = dict(visible=int(vis.sum()), seen_by_two=int((seen >= 2).sum()))
    assert set(cs.kinds) == {'random', 'side-left', 'side-right', 'side-top', 'side-bottom', 'corner', 'shared', 'nobody', 'behind', 'level',
                             'block'}
    sides, cor = of_kind(cs, 'side'), of_kind(cs, 'corner')
    assert len(sides) == 4 and len(cor) == 4 and len(of_kind(cs, 'random')) == Q_RANDOM and len(of_kind(cs, 'block')) == Q_BLOCK
    hl, pl = cs.last
    for cam, h_, p_ in ((0, 0, 0), (n - 1, hl, pl)):                                # the placed samples of the two end cameras
        xs, ys, vs = x[:, cam, :, h_, p_], y[:, cam, :, h_, p_], vis[:, cam, :, h_, p_]
        for qi, hit in zip(sides, (xs < 0, xs > fw - 1, ys < 0, ys > fh - 1)):
            assert bool((hit & vs)[:, qi].all()), f'side query {qi} of camera {cam}'
            assert bool((corners_on_map(xs, ys, fw, fh)[:, qi] <= 2).all())
        for qi, hit in zip(cor, ((xs < 0) & (ys < 0), (xs > fw - 1) & (ys < 0), (xs < 0) & (ys > fh - 1), (xs > fw - 1) & (ys > fh - 1))):
            assert bool((hit & vs)[:, qi].all()), f'corner query {qi} of camera {cam}'
            for lh, lw in cs.levels:                                               # one corner on the map, on every level
                assert bool((corners_on_map(pixel(u[:, cam, qi, h_, p_], lw), pixel(v[:, cam, qi, h_, p_], lh), lw, lh) == 1).all())
    # the two allocation ends: top-left of (batch 0, camera 0, level 0), bottom-right of the last camera's coarsest level
    tl = (x[0, 0, cor[0], 0, 0], y[0, 0, cor[0], 0, 0])
    br = (pixel(u[b - 1, n - 1, cor[3], hl, pl], cw), pixel(v[b - 1, n - 1, cor[3], hl, pl], ch))
    assert -0.5 < tl[0] < 0 and -0.5 < tl[1] < 0 and int(corners_on_map(*tl, fw, fh)) == 1
    assert cw - 1 < br[0] < cw - 0.5 and ch - 1 < br[1] < ch - 0.5 and int(corners_on_map(*br, cw, ch)) == 1
    counts['band'] = int((vis & ((x < 0) | (x > fw - 1) | (y < 0) | (y > fh - 1))).sum())
    sh = of_kind(cs, 'shared')
    assert len(sh) == 4 and bool((seen[:, sh, 0, 0] >= 2).all()), 'shared'
    nb = of_kind(cs, 'nobody')
    assert len(nb) == 1 and not bool(vis[:, :, nb].any()), 'nobody'
    assert bool((pixel(v[:, :, nb], fh)[z[:, :, nb] > EPS] < -1).all()), 'nobody: above every image'
    counts['nobody'] = int((~vis.permute(0, 2, 1, 3, 4).flatten(2).any(2)).sum())
    bh = of_kind(cs, 'behind')
    assert len(bh) == 1 and bool((z[:, 0, bh, 0, 0] < -1).all()) and bool((u[:, 0, bh, 0, 0].abs() > 1e5).all() | (v[:, 0, bh, 0, 0].abs() > 1e5).all())
    lv = of_kind(cs, 'level')
    assert len(lv) == 2
    for qi, beyond in zip(lv, (lambda t: t > fw + 1, lambda t: t < -2)):
        us = u[:, 0, qi, 0, 0]
        assert bool((z[:, 0, qi, 0, 0] > 1).all()) and not bool(vis[:, 0, qi, 0, 0].any())
        assert bool(beyond(pixel(us, fw)).all()) and bool(((pixel(us, cw) > -1) & (pixel(us, cw) < cw)).all()), 'level-dependent'
        assert bool((corners_on_map(pixel(us, cw), pixel(v[:, 0, qi, 0, 0], ch), cw, ch) >= 1).all())
        assert bool((corners_on_map(pixel(us, fw), pixel(v[:, 0, qi, 0, 0], fh), fw, fh) == 0).all())
    # the converse cannot happen: a cell that touches the finest map touches every coarser one
    on0 = (x > -1) & (x < fw) & (y > -1) & (y < fh)
    for lh, lw in cs.levels[1:]:
        assert bool(((pixel(u, lw) > -1) & (pixel(u, lw) < lw) & (pixel(v, lh) > -1) & (pixel(v, lh) < lh))[on0].all())
    bx, by = cs.block_cell
    xc, yc = pixel(u[:, cs.block_cam, cs.block], cw), pixel(v[:, cs.block_cam, cs.block], ch)
    in_cell = (torch.floor(xc) == bx) & (torch.floor(yc) == by) & vis[:, cs.block_cam, cs.block]
    counts['block'] = int(in_cell.sum())
    assert bool(in_cell.all()) and counts['block'] == b * Q_BLOCK * hh * P, 'block'
    return counts


# ---- what the tests compare --------------------------------------------------------------------------------------------------------
def subset(cs, queries):
    """The case restricted to a slice of its queries (the maps stay)."""
    sub = Case()
    sub.__dict__.update(cs.__dict__)
    for key in ('ref', 'offsets', 'attn', 'cam', 'grad_out', 'grad_out2'):
        setattr(sub, key, getattr(cs, key)[:, queries].contiguous())
    sub.Q = sub.ref.shape[1]
    sub.kinds = cs.kinds[queries]
    return sub


def leaves(cs, dtype):
    t = lambda x: x.to(dtype).requires_grad_(True)                                  # noqa: E731
    return dict(feats=[t(f) for f in cs.feats], ref=t(cs.ref), offsets=t(cs.offsets), attn=t(cs.attn), cam=t(cs.cam))


def projected(cs, lv, dtype, value=None, **decisions):
    """The arbiter: value = value_proj(flatten_pyramid(feats)) (or the one given), then sample_aggregate -> out, mask, value."""
    flat, shapes = O.flatten_pyramid(lv['feats'])
    if value is None:
        value = F.linear(flat, cs.w_v.to(dtype), cs.b_v.to(dtype)).view(cs.B * cs.N, -1, cs.Hh, C // cs.Hh)
    out, _, mask = O.sample_aggregate(value, shapes, lv['ref'], lv['offsets'], lv['attn'].flatten(-2), lv['cam'], cs.lidar2img.to(dtype),
                                      PC_RANGE, IMG_H, IMG_W, **decisions)
    return out, mask, value


def cell_corners(cs):
    """(B, N, Q, Hh, L, P, 2) int64: floor of every sample's pixel coordinates (fp64), for the oracle's explicit-gather form."""
    u, v, _, _ = geometry(cs.ref, cs.offsets, cs.lidar2img)
    return torch.stack([torch.stack((torch.floor(pixel(u, w)), torch.floor(pixel(v, h))), -1) for h, w in cs.levels], 4).long()


def raw_association(cs, lv, dtype):
    """The raw route restated in torch, in the order the kernels document: the weights (softmax x visibility x camera sigmoid x bilinear,
    zero padding by bilinear_zero_pad's rule) gather the RAW 256-channel pixels into agg (B, Q, Hh, 256), their sum is wsum (B, Q, Hh),
    and value_proj is applied per head afterwards: out[.., h, :] = W_h agg[.., h, :] + b_h wsum[.., h].  -> out, agg, wsum, and the
    part of wsum that belongs to levels 0 and 1 (what the coarse-projected gather leaves in plan.wsum)."""
    b, n, q, hh, nl = cs.B, cs.N, cs.Q, cs.Hh, cs.L
    flat, shapes = O.flatten_pyramid(lv['feats'])                                   # (B N, S, 256)
    s = flat.shape[1]
    pts = O.denormalise(lv['ref'], PC_RANGE).view(b, q, 1, 1, 3) + lv['offsets']
    uv, mask = O.project(pts.reshape(b, q * hh * P, 3), cs.lidar2img.to(dtype), IMG_H, IMG_W)
    uv, mask = uv.view(b, n, q, hh, P, 2), mask.view(b, n, q, hh, P)
    rows = torch.arange(b * n) % b                                                  # the reference's pairing of value rows and logits
    w = lv['attn'].flatten(-2).softmax(-1)[rows].view(b, n, q, hh, nl, P)
    w = w * mask.view(b, n, q, hh, 1, P) * O.scrambled_cam_weights(lv['cam'], n).sigmoid().view(b, n, q, 1, 1, 1)
    bi = torch.arange(b).view(b, 1, 1, 1, 1).expand(b, n, q, hh, P)
    ri = (torch.arange(q).view(q, 1) * hh + torch.arange(hh)).view(1, 1, q, hh, 1).expand(b, n, q, hh, P)
    ni = torch.arange(n).view(1, n, 1, 1, 1)
    assoc = torch.zeros(b, q * hh, n * s, dtype=dtype)
    start = 0
    for lvl, (h, wd) in enumerate(shapes):
        x, y = uv[..., 0] * wd - 0.5, uv[..., 1] * h - 0.5
        x0, y0 = torch.floor(x), torch.floor(y)
        dx, dy = x - x0, y - y0
        for yy, xx, wt in ((y0, x0, (1 - dy) * (1 - dx)), (y0, x0 + 1, (1 - dy) * dx), (y0 + 1, x0, dy * (1 - dx)), (y0 + 1, x0 + 1, dy * dx)):
            ok = (xx >= 0) & (xx <= wd - 1) & (yy >= 0) & (yy <= h - 1)
            col = ni * s + start + yy.detach().clamp(0, h - 1).long() * wd + xx.detach().clamp(0, wd - 1).long()
            assoc = assoc.index_put((bi, ri, col), torch.where(ok, w[:, :, :, :, lvl] * wt, torch.zeros((), dtype=dtype)), accumulate=True)
        start += h * wd
        if lvl == min(1, nl - 1):
            wsum_fine = assoc.detach().sum(-1).view(b, q, hh)
    agg = (assoc @ flat.reshape(b, n * s, C)).view(b, q, hh, C)
    wsum = assoc.sum(-1).view(b, q, hh)
    dh = C // hh
    out = torch.einsum('bqhc,hdc->bqhd', agg, cs.w_v.to(dtype).view(hh, dh, C)) + cs.b_v.to(dtype).view(hh, dh) * wsum.unsqueeze(-1)
    return out.reshape(b, q, C), agg, wsum, wsum_fine


def evaluate(cs, dtype, raw=False):
    """One evaluation in `dtype` from the case's fp32 inputs: out, mask, wsum, the five query-side / value gradients of grad_out, the
    pyramid's gradient of grad_out (grad_feats) and of grad_out and grad_out2 together (grad_feats2: two decoder layers on one
    pyramid).  raw: through raw_association (no projected value: grad_value is absent)."""
    lv = leaves(cs, dtype)
    res = {}
    if raw:
        out, _, wsum, fine = raw_association(cs, lv, dtype)
        wrt = [lv['ref'], lv['offsets'], lv['attn'], lv['cam'], *lv['feats']]
    else:
        out, mask, value = projected(cs, lv, dtype)
        res['mask'] = mask
        with torch.no_grad():
            wsum, fine = raw_association(cs, lv, dtype)[2:]
        wrt = [lv['ref'], lv['offsets'], lv['attn'], lv['cam'], *lv['feats'], value]
    g = torch.autograd.grad(out, wrt, cs.grad_out.to(dtype), retain_graph=True)
    g2 = torch.autograd.grad(out, lv['feats'], cs.grad_out2.to(dtype))
    res.update(out=out.detach(), wsum=wsum.detach(), wsum_fine=fine, grad_ref=g[0], grad_offsets=g[1], grad_attn_logits=g[2], grad_cam_logits=g[3],
               grad_feats=list(g[4:4 + cs.L]), grad_feats2=[a + c for a, c in zip(g[4:4 + cs.L], g2)])
    if not raw:
        res['grad_value'] = g[-1]
    return res


def block_grad(cs, grad_feats):
    """(B, C, pixels): the coarsest level's gradient at the block's camera and the block cell's pixels."""
    g = grad_feats[-1].reshape(cs.B, cs.N, C, *cs.levels[-1])[:, cs.block_cam]
    return torch.stack([g[:, :, y, x] for y, x in block_pixels(cs)], -1)


ROWS = {'grad_attn_logits': 2, 'grad_offsets': 2, 'grad_cam_logits': 1}           # per-row measures: the row's trailing dimensions


def figures(cs, got, want):
    """The error of `got` against `want` (results of evaluate, or a kernel's outputs under the same names) per output, with
    detr3d_cases.figures' measures: max |diff| over the tensor's largest |entry| for out, wsum, grad_ref, grad_value and every
    grad_feats[l] / grad_feats2[l]; per (b, q, head) row for grad_attn_logits and grad_offsets, per (b, q) row for grad_cam_logits
    (detr3d_ref.row_rel_err).  Only what `got` holds is measured."""
    fig = {}
    for key in ('out', 'wsum', 'wsum_fine', 'grad_ref', 'grad_value'):
        if got.get(key) is not None and key in want:
            fig[key] = R.rel_err(got[key].reshape(want[key].shape), want[key])
    for key, dims in ROWS.items():
        if got.get(key) is not None:
            fig[key] = R.row_rel_err(got[key].reshape(want[key].shape), want[key], dims)
    for key in ('grad_feats', 'grad_feats2'):
        if got.get(key) is not None:
            for l in range(cs.L):
                fig[f'{key}[{l}]'] = R.rel_err(got[key][l].reshape(want[key][l].shape), want[key][l])
    return fig


_EVAL = {}


def reference(name, raw=False, block_only=False):
    """(fp64 result, fp32-host figures) of a case, computed once per process.  The fp64 result is the arbiter's (evaluate(raw=False))
    either way.  The figures are the error of an honest fp32 evaluation by torch on the CPU - of the same restatement, or with raw=True
    of the raw association the raw-pyramid kernels compute; a kernel is allowed FACTOR times that.  block_only: the block's queries
    alone, and one figure, the gradient at the block cell's pixels."""
    key = (name, raw, block_only)
    if key not in _EVAL:
        cs = case(name)
        if block_only:
            cs = subset(cs, cs.block)
        wkey = (name, 'want', block_only)
        if wkey not in _EVAL:
            _EVAL[wkey] = evaluate(cs, F64)
        want, host = _EVAL[wkey], evaluate(cs, torch.float32, raw=raw)
        assert raw or torch.equal(want['mask'], host['mask'])
        if block_only:
            fig = {'block grad_feats': R.rel_err(block_grad(cs, host['grad_feats']), block_grad(cs, want['grad_feats']))}
        else:
            fig = figures(cs, host, want)
        _EVAL[key] = (want, fig)
    return _EVAL[key]


def value32(cs, feats=None, levels=slice(None)):
    """value_proj in fp32 on the host, (B N, S, Hh, Dh) over the chosen levels: the projected value the projected-value kernels are fed
    (an input of theirs: the same rounding is in the fp32 host figures)."""
    flat, _ = O.flatten_pyramid((cs.feats if feats is None else feats)[levels])
    return F.linear(flat, cs.w_v, cs.b_v).view(cs.B * cs.N, -1, cs.Hh, C // cs.Hh)


def bf16_value(cs):
    """The projected value as the reduced-precision mode stores it: value32 rounded to bf16."""
    return value32(cs).bfloat16()


def reference_bf16(name, what):
    """(fp64 out, fp32-host figure of out) of the forward fed bf16-rounded inputs: what = 'value' - the projected value rounded
    (bf16_value), through sample_aggregate; what = 'feats' - the pyramid rounded, the fp32 figure through the raw association."""
    key = (name, 'bf16', what)
    if key not in _EVAL:
        cs = case(name)
        res = {}
        with torch.no_grad():
            for dtype in (F64, torch.float32):
                lv = {k: ([f.detach() for f in v] if isinstance(v, list) else v.detach()) for k, v in leaves(cs, dtype).items()}
                if what == 'value':
                    res[dtype] = projected(cs, lv, dtype, value=bf16_value(cs).to(dtype))[0]
                else:
                    lv['feats'] = [f.bfloat16().to(dtype) for f in cs.feats]
                    res[dtype] = projected(cs, lv, dtype)[0] if dtype == F64 else raw_association(cs, lv, dtype)[0]
        _EVAL[key] = (res[F64], {'out': R.rel_err(res[torch.float32], res[F64])})
    return _EVAL[key]
