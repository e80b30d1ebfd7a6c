"""Inputs for the kernel tests of gd4d_detr3d.hip, chosen from the fp64 restatement (detr3d_ref) alone: nothing here looks at a kernel's
output, and every case asserts its own conditions (check_case) before anything touches the GPU.

Rig: N pinhole cameras near the origin, yawed 360 / N degrees apart (lidar axes: x forward, y left, z up; camera axes: x right, y
down, z forward), a few centimetres of translation per camera and batch entry, horizontal field of view 360 / N + 10 degrees so that
neighbours overlap by 10 degrees; a 64 x 112 image.

Queries of every batch entry, in this order:
  random     37 points: candidates uniform in [0, 1]^3, the first that pass the two margins below
  sides      4 points whose finest-level sample lies in the half-pixel band beyond the left / right / top / bottom border
  corners    4 points in the half-pixel band beyond two borders at once (exactly one bilinear corner on the map)
  shared     4 points in the overlap of two neighbouring cameras
  nobody     1 point above every camera's image
  behind     1 point behind camera 0: its depth is clamped to 1e-5, the projection lands about 1e8 pixels away
  block      32 points inside one bilinear cell of the coarsest level of camera 1 (all atomic adds on the same pixels)
Placed points are inverse projections of a chosen (camera, pixel, depth), the pixel drawn inside the band or cell until the margins
hold.  v2 offsets are normal with a standard deviation of 1.5 pixels of the level (the sample moves by half of it), drawn per query
until the cell margin holds; the offsets of the block's camera at the coarsest level are a fiftieth of that, so the block stays in
its cell.  On the `sides` queries three offsets of the visible camera are overwritten: one carries the sample fully out of the map,
one is +3e9 and one -3e9 pixels.

Margins (fp64, on the fp32 inputs; they make fp32 and fp64 agree on every visibility bit and every bilinear cell):
  visibility   |g.x|, |g.y| differ from 1 and the depth from 1e-5 by more than 1e-3, for every camera
  cell         for every sample of a visible camera, at every level, with its offset in v2: the pixel coordinates x and y are more
               than 1e-3 away from an integer - unless the sample lies more than 1e-3 beyond the last cell that touches the map
               (x < -1 or x > W, likewise y): then every corner is outside in either precision and the sample and all its
               derivatives are 0, wherever the integers are (the +-3e9 offsets are such samples: fp32 cannot even represent their
               fraction)."""
import math

import torch

import detr3d_ref as R

F64 = torch.float64
IMG_H, IMG_W = 64, 112
PC_RANGE = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
MARGIN = 1e-3
Q_RANDOM, Q_BLOCK = 37, 32

# name -> B, N, C, heads, levels (H, W)
SHAPES = {
    'base': (1, 6, 256, 8, [(16, 28), (8, 14), (4, 7), (2, 4)]),
    'narrow': (2, 6, 64, 4, [(5, 9), (3, 5), (1, 2)]),
    'ragged': (2, 3, 100, 4, [(1, 1)]),
    'wide': (1, 12, 320, 8, [(8, 14), (4, 7)]),
}
SEEDS = {'base': 3501, 'narrow': 3502, 'ragged': 3503, 'wide': 3504}


def focal(n):
    return (IMG_W / 2) / math.tan(math.radians(180.0 / n + 5.0))


def rig(b, n, gen):
    """lidar2img (B, N, 4, 4) fp64 and its parts (rotation (N, 3, 3), camera centres (B, N, 3))."""
    f = focal(n)
    k = torch.tensor([[f, 0, IMG_W / 2], [0, f, IMG_H / 2], [0, 0, 1]], dtype=F64)
    rot = torch.zeros(n, 3, 3, dtype=F64)
    for i in range(n):
        th = 2 * math.pi * i / n
        rot[i] = torch.tensor([[math.sin(th), -math.cos(th), 0], [0, 0, -1], [math.cos(th), math.sin(th), 0]], dtype=F64)
    centre = (torch.rand(b, n, 3, generator=gen, dtype=F64) - 0.5) * 0.1
    m = torch.zeros(b, n, 4, 4, dtype=F64)
    m[:, :, :3, :3] = k @ rot
    m[:, :, :3, 3] = -torch.einsum('nij,bnj->bni', k @ rot, centre)
    m[:, :, 3, 3] = 1
    return m, rot, centre, k


def grid_of_pixel(x, size):
    """inverse of detr3d_ref.pixel_coords"""
    return (2 * x + 1) / size - 1


def unproject(rot, centre, k, gx, gy, depth):
    """grid coordinate (gx, gy) of one camera at `depth` -> reference point in [0, 1]^3 (fp64)."""
    px, py = (gx / 2 + 0.5) * IMG_W, (gy / 2 + 0.5) * IMG_H
    cam = depth * torch.linalg.solve(k, torch.tensor([px, py, 1.0], dtype=F64))
    p = rot.T @ cam + centre
    rng = torch.tensor(PC_RANGE, dtype=F64)
    return (p - rng[:3]) / (rng[3:] - rng[:3])


def _far_from_integers(x):
    return (x - torch.round(x)).abs() > MARGIN


def cell_margin_ok(x, y, w, h):
    """The cell margin of the module docstring for pixel coordinates x, y on a W x H map (elementwise)."""
    out = (x < -1 - MARGIN) | (x > w + MARGIN) | (y < -1 - MARGIN) | (y > h + MARGIN)
    return out | (_far_from_integers(x) & _far_from_integers(y))


def margins(ref, lidar2img, levels, offsets=None):
    """ref (B, Q, 3), lidar2img fp32 values -> (visibility margin ok, v1 cell margin ok, v2 cell margin ok or None), each (B, Q)."""
    grid, depth, vis = R.project(ref.to(F64), lidar2img.to(F64), PC_RANGE, IMG_H, IMG_W)
    vm = ((grid.abs() - 1).abs() > MARGIN).all(-1) & ((depth - R.DEPTH_EPS).abs() > MARGIN)
    c1 = torch.ones_like(vis)
    for h, w in levels:
        c1 &= cell_margin_ok(R.pixel_coords(grid[..., 0], w), R.pixel_coords(grid[..., 1], h), w, h)
    c1 = (c1 | ~vis).all(1)
    c2 = None
    if offsets is not None:
        c2 = torch.ones_like(vis)
        for l, (h, w) in enumerate(levels):
            gx, gy = R.v2_grid(grid, offsets.to(F64), l, w, h)                       # (B, N, Hh, Q, P)
            c2 &= cell_margin_ok(R.pixel_coords(gx, w), R.pixel_coords(gy, h), w, h).all(-1).all(2)
        c2 = (c2 | ~vis).all(1)
    return vm.all(1), c1, c2


class Case:
    pass


def _draw_offsets(n, hh, nl, gen, small=None):
    off = torch.randn(n, hh, nl, nl, 2, generator=gen, dtype=F64) * 1.5
    if small is not None:
        off[small, :, nl - 1] *= 0.02
    return off.float()


def build(name):
    b, n, c, hh, levels = SHAPES[name]
    nl = len(levels)
    gen = torch.Generator().manual_seed(SEEDS[name])
    m64, rot, centre, k = rig(b, n, gen)
    l2i = m64.float()
    fh, fw = levels[0]
    ch, cw = levels[-1]
    block_cam = 1
    # the block's cell on the coarsest level: corners (bx, by) .. (bx + 1, by + 1), on the map where the map has room
    # (a one-pixel axis has the cell 0 .. 1, of which the visible half 0 .. 0.5 lies inside the image)
    bx, by = (cw - 1) // 2, (ch - 1) // 2
    in_x, in_y = ((0.3, 0.7) if cw > 1 else (0.1, 0.4)), ((0.3, 0.7) if ch > 1 else (0.1, 0.4))
    u_shared = math.tan(math.pi / n) / math.tan(math.pi / n + math.radians(5.0))        # the middle of the overlap, seen from the left camera

    # (kind, camera, x range, y range, depth range): pixel coordinates of the finest level.  The bands stop 0.05 pixels short of
    # the image's edge (the visibility margin is 1e-3 grid units, 0.014 pixels of the widest map)
    def px(g, size):
        return R.pixel_coords(torch.tensor(g, dtype=F64), size).item()
    any_x, any_y = (-0.4, fw - 0.6), (-0.4, fh - 0.6)
    lo_band, hi_x, hi_y = (-0.45, -0.05), (fw - 0.95, fw - 0.55), (fh - 0.95, fh - 0.55)
    specs = [('side-left', 0, lo_band, any_y, (6, 30)), ('side-right', 0, hi_x, any_y, (6, 30)),
             ('side-top', 0, any_x, lo_band, (6, 30)), ('side-bottom', 0, any_x, hi_y, (6, 30)),
             ('corner', 0, lo_band, lo_band, (6, 30)), ('corner', 0, hi_x, lo_band, (6, 30)),
             ('corner', 0, lo_band, hi_y, (6, 30)), ('corner', 0, hi_x, hi_y, (6, 30))]
    specs += [('shared', i % n, (px(u_shared - 0.08, fw), px(u_shared + 0.08, fw)), (px(-0.6, fh), px(0.6, fh)), (8, 30)) for i in range(4)]
    specs += [('nobody', 0, (px(-0.2, fw), px(0.2, fw)), (px(-1.8, fh), px(-1.5, fh)), (0.8, 1.4))]
    specs += [('behind', 0, (px(-0.8, fw), px(0.8, fw)), (px(-0.8, fh), px(0.8, fh)), (-30, -8))]
    kinds = ['random'] * Q_RANDOM + [s[0] for s in specs] + ['block'] * Q_BLOCK
    q = len(kinds)

    ref = torch.zeros(b, q, 3)
    offsets = torch.zeros(b, q, n, hh, nl, nl, 2)

    def accept(bi, qi, point, small=None, edit=None):
        """Try `point` for query qi: draw offsets until the v2 cell margin holds (at most 400 draws); False if the point itself
        fails the visibility or the v1 cell margin."""
        r32 = point.float().view(1, 1, 3)
        vm, c1, _ = margins(r32, l2i[bi:bi + 1], levels)
        if not (bool(vm) and bool(c1)):
            return False
        for _ in range(400):
            off = _draw_offsets(n, hh, nl, gen, small)
            if edit is not None:
                edit(off)
            if bool(margins(r32, l2i[bi:bi + 1], levels, off.view(1, 1, n, hh, nl, nl, 2))[2]):
                ref[bi, qi], offsets[bi, qi] = r32.view(3), off
                return True
        return False

    def uniform(lo, hi):
        return lo + (hi - lo) * torch.rand((), generator=gen, dtype=F64).item()

    def far_offsets(cam):
        def edit(off):
            off[cam, 0, 0, 0, 0] = 2.0 * (fw + 3)                                       # x moves by fw + 3 pixels: fully out of the map
            off[cam, 1 % hh, nl - 1, 0, 0] = 3e9
            off[cam, 2 % hh, 0, nl - 1, 1] = -3e9
        return edit

    for bi in range(b):
        qi, tried = 0, 0
        while qi < Q_RANDOM:
            tried += 1
            assert tried < 20 * Q_RANDOM, 'the margins reject almost every candidate: the rig or the margins are wrong'
            if accept(bi, qi, torch.rand(3, generator=gen, dtype=F64)):
                qi += 1
        for kind, cam, xr, yr, dr in specs:
            for _ in range(200):
                gx, gy = grid_of_pixel(uniform(*xr), fw), grid_of_pixel(uniform(*yr), fh)
                point = unproject(rot[cam], centre[bi, cam], k, gx, gy, uniform(*dr))
                if accept(bi, qi, point, edit=far_offsets(cam) if kind.startswith('side') else None):
                    break
            else:
                raise AssertionError(f'no {kind} point of camera {cam} passes the margins')
            qi += 1
        for _ in range(Q_BLOCK):
            for _ in range(200):
                gx, gy = grid_of_pixel(bx + uniform(*in_x), cw), grid_of_pixel(by + uniform(*in_y), ch)
                point = unproject(rot[block_cam], centre[bi, block_cam], k, gx, gy, uniform(8, 30))
                if accept(bi, qi, point, small=block_cam):
                    break
            else:
                raise AssertionError('no block point passes the margins')
            qi += 1
        assert qi == q

    cs = Case()
    cs.name, cs.B, cs.N, cs.C, cs.Hh, cs.levels, cs.L, cs.Q = name, b, n, c, hh, levels, nl, q
    cs.kinds, cs.block, cs.block_cam, cs.block_cell = kinds, slice(q - Q_BLOCK, q), block_cam, (bx, by)
    cs.ref, cs.offsets, cs.lidar2img = ref, offsets, l2i
    cs.feats = [torch.randn(b, n, c, h, w, generator=gen) for h, w in levels]
    cs.logits = torch.randn(b, q, n, 1, nl, generator=gen)
    cs.logits_v2 = torch.randn(b, q, n, hh, nl * nl, generator=gen)
    cs.grad_out = torch.randn(b, q, c, generator=gen)
    return cs


_CASES = {}


def case(name):
    """The case, built once per process and shared (nobody writes into it)."""
    if name not in _CASES:
        _CASES[name] = build(name)
    return _CASES[name]


def block_pixels(cs):
    """(y, x) of the block cell's corners that are on the coarsest map."""
    ch, cw = cs.levels[-1]
    bx, by = cs.block_cell
    return [(y, x) for y in (by, by + 1) for x in (bx, bx + 1) if 0 <= x < cw and 0 <= y < ch]


def check_case(cs):
    """The conditions the tests rely on, from the fp64 restatement alone.  Returns the counts it asserted on."""
    vm, c1, c2 = margins(cs.ref, cs.lidar2img, cs.levels, cs.offsets)
    assert bool(vm.all()), 'visibility margin'
    assert bool(c1.all()) and bool(c2.all()), 'cell margin'
    grid, depth, vis = R.project(cs.ref.to(F64), cs.lidar2img.to(F64), PC_RANGE, IMG_H, IMG_W)
    seen = vis.sum(1)                                                               # (B, Q)
    counts = dict(nobody=int((seen == 0).sum()), shared=int((seen >= 2).sum()))
    assert (seen == 0).any(1).all() and ((seen >= 2).sum(1) >= 4).all(), counts
    fh, fw = cs.levels[0]
    x, y = R.pixel_coords(grid[..., 0], fw), R.pixel_coords(grid[..., 1], fh)
    for side, hit in (('left', x < 0), ('right', x > fw - 1), ('top', y < 0), ('bottom', y > fh - 1)):
        counts[side] = int((hit & vis).sum())
        assert (hit & vis).flatten(1).any(1).all(), f'no visible sample with a corner beyond the {side} border'
    for corner, hit in (('top-left', (x < 0) & (y < 0)), ('top-right', (x > fw - 1) & (y < 0)), ('bottom-left', (x < 0) & (y > fh - 1)),
                        ('bottom-right', (x > fw - 1) & (y > fh - 1))):
        assert (hit & vis).flatten(1).any(1).all(), f'no visible sample with one corner on the map at the {corner} corner'
    ch, cw = cs.levels[-1]
    bx, by = cs.block_cell
    xc, yc = R.pixel_coords(grid[:, cs.block_cam, :, 0], cw), R.pixel_coords(grid[:, cs.block_cam, :, 1], ch)
    in_cell = (torch.floor(xc) == bx) & (torch.floor(yc) == by) & vis[:, cs.block_cam]
    counts['block'] = int(in_cell.sum(1).min())
    assert counts['block'] >= 32 and bool(in_cell[:, cs.block].all())
    gx, gy = R.v2_grid(grid, cs.offsets.to(F64), cs.L - 1, cw, ch)
    in2 = (torch.floor(R.pixel_coords(gx, cw)) == bx) & (torch.floor(R.pixel_coords(gy, ch)) == by)
    counts['block_v2'] = int(in2[:, cs.block_cam][:, :, cs.block].flatten(1).sum(1).min())
    assert bool(in2[:, cs.block_cam][:, :, cs.block].all())
    bq = [i for i, kd in enumerate(cs.kinds) if kd == 'behind']
    assert bool((depth[:, 0, bq] < -1).all()) and bool((grid[:, 0, bq].abs().amax(-1) > 1e5).all())
    # a v2 sample of a visible camera that its offset carries fully out of the map, and the +-3e9 pair
    sides = [i for i, kd in enumerate(cs.kinds) if kd.startswith('side')]
    assert bool(vis[:, 0, sides].all())
    gx0, _ = R.v2_grid(grid, cs.offsets.to(F64), 0, fw, fh)
    assert bool((R.pixel_coords(gx0[:, 0, 0, sides, 0], fw) > fw).all())
    assert bool((cs.offsets[:, sides, 0].abs().flatten(2).amax(2) == 3e9).all())
    return counts


# ---- what the tests compare: one evaluation of the restatement, forward and autograd, per (case, variant, dtype) ------------------
def subset(cs, queries):
    """The case restricted to a slice of its queries (the maps stay)."""
    sub = Case()
    sub.__dict__.update(cs.__dict__)
    sub.ref, sub.offsets, sub.logits = cs.ref[:, queries].contiguous(), cs.offsets[:, queries].contiguous(), cs.logits[:, queries].contiguous()
    sub.logits_v2, sub.grad_out = cs.logits_v2[:, queries].contiguous(), cs.grad_out[:, queries].contiguous()
    sub.Q = sub.ref.shape[1]
    return sub


def evaluate(cs, variant, dtype):
    """variant 'v1' / 'v2' -> dict of out, mask, (sampled), grad_logits, (grad_offsets), grad_ref, grad_feats (list), computed in
    `dtype` from the case's fp32 inputs."""
    feats = [f.to(dtype).requires_grad_(True) for f in cs.feats]
    ref = cs.ref.to(dtype).requires_grad_(True)
    res = {}
    if variant == 'v1':
        logits = cs.logits.to(dtype).requires_grad_(True)
        out, mask, sampled = R.detr3d(feats, ref, logits, cs.lidar2img, PC_RANGE, IMG_H, IMG_W)
        res['sampled'] = sampled.detach()
        leaves = [logits, ref, *feats]
    else:
        logits = cs.logits_v2.to(dtype).requires_grad_(True)
        offsets = cs.offsets.to(dtype).requires_grad_(True)
        out, mask = R.detr3d_v2(feats, ref, logits, offsets, cs.lidar2img, PC_RANGE, IMG_H, IMG_W, cs.Hh)
        leaves = [logits, ref, *feats, offsets]
    grads = torch.autograd.grad(out, leaves, cs.grad_out.to(dtype))
    res.update(out=out.detach(), mask=mask, grad_logits=grads[0], grad_ref=grads[1], grad_feats=list(grads[2:2 + cs.L]))
    if variant == 'v2':
        res['grad_offsets'] = grads[-1]
    return res


def block_grad(cs, res):
    """(B, C, pixels): grad_feats of the coarsest level at the block's camera and the block cell's pixels."""
    g = res['grad_feats'][-1][:, cs.block_cam]
    return torch.stack([g[:, :, y, x] for y, x in block_pixels(cs)], -1)


def figures(cs, variant, got, want):
    """The error of `got` against `want` (two results of evaluate, or a kernel's outputs in the same form), per output tensor:
    max |diff| over the tensor's largest |entry|; grad_logits and grad_offsets per (query, camera, head) row (detr3d_ref.row_rel_err).
    `forward` / `backward` keys may be missing from `got`: only what it holds is measured."""
    fig = {}
    for key in ('out', 'sampled', 'grad_ref'):
        if got.get(key) is not None and key in want:
            fig[key] = R.rel_err(got[key], want[key])
    if got.get('grad_logits') is not None:
        gl = want['grad_logits']
        fig['grad_logits'] = R.row_rel_err(got['grad_logits'].reshape(gl.shape), gl, 1)
    if got.get('grad_offsets') is not None:
        fig['grad_offsets'] = R.row_rel_err(got['grad_offsets'], want['grad_offsets'], 3)
    if got.get('grad_feats') is not None:
        for l in range(cs.L):
            fig[f'grad_feats[{l}]'] = R.rel_err(got['grad_feats'][l], want['grad_feats'][l])
    return fig


_EVAL = {}


def reference(name, variant, block_only=False):
    """(fp64 result, fp32-host figures) of a case, computed once per process.  The figures are the error of the same restatement
    evaluated in fp32 by torch on the CPU: the error of honest fp32 arithmetic for this operation and these inputs.  A kernel
    is allowed FACTOR times that."""
    key = (name, variant, block_only)
    if key not in _EVAL:
        cs = case(name)
        if block_only:
            cs = subset(cs, cs.block)
        want, host = evaluate(cs, variant, F64), evaluate(cs, variant, torch.float32)
        assert torch.equal(want['mask'], host['mask'])
        fig = figures(cs, variant, host, want)
        if block_only:
            fig = {'block grad_feats': R.rel_err(block_grad(cs, host), block_grad(cs, want))}
        _EVAL[key] = (want, fig)
    return _EVAL[key]


FACTOR = 4.0
VARIANTS = [(n, 'v1') for n in SHAPES] + [(n, 'v2') for n in SHAPES]
