"""Stepping the oracle BACKWARD through every layer of one decoder training call (a helper of the test modules, not a test file).

The forward counterpart is tests/decoder_step.py.  Here layer l of the oracle runs in fp64 on the implementation's OWN input -
x_l = states[l - 1] (query for l = 0), ref_l = refs[l - 1] (init_ref for l = 0) - and with the implementation's own
discontinuous decisions: the visibility mask and the bilinear corners of its gather, the ReLU units of position_encoder and of
the FFN, the dropout keep masks (O.decoder_layer's decision arguments).  What is left between the two is rounding, so the
bounds can be tight.  From the top layer down, G_5 = probe_5 and G_{l-1} = probe_{l-1} + dL/dx_l (the oracle's own gradient
of layer l with respect to its input); the pyramid, query_pos and init_ref gradients are accumulated over the layers, then the
chain is closed through reference_points (Linear + sigmoid) and the query_embed split.  Each layer owns its parameters, so
every parameter gradient of layer l is compared with the implementation's directly.

The refined reference points are detached (detr3d_transformer.py:212-214); the oracle's refinement (O.refine_points) still takes
part in the stepped chain rule - layer l's backward also receives <refine(y_l, ref_l), dL/dref_{l+1}> - so the reg branches' zero
gradient is what the oracle's autograd says, not an assumption.

The decisions are forced, so a spy that recorded the wrong layer's decisions would bend the oracle towards the implementation;
the decision-mismatch report counts, per layer and kind, how often the fp64 oracle's own choice disagrees with the forced one
(mask: query rows with a flipped bit, at most decoder_step.MAX_FLIPPED; corners and ReLU units: at most 1e-4 of their total)."""
import copy
import inspect

import torch
import torch.nn.functional as F

from oracle import torch_oracle as O

from decoder_step import MAX_FLIPPED

TOL_FRO, TOL_ROW = 1e-3, 1e-2          # relative Frobenius error of a tensor / relative error of one of its rows
ROW_FLOOR = 0.1                        # a row's error is relative to max(its norm, ROW_FLOOR x the median row norm)
MAX_FRACTION = 1e-4                    # corners and ReLU units: forced decisions the fp64 oracle disagrees with
RELU_KINDS = ('pe1', 'pe4', 'ffn')


# ----------------------------------------------------------------------------------------------------------------- decisions
def corners_from_uv(uv, level_hw):
    """The top-left bilinear corner of every sample and level as the plan kernel computes it from its fp32 uv:
    x = fmaf(u, W, -0.5f), x0 = floor(x) (one rounding: u * W - 0.5 is exact in fp64).  uv (B, N, Q, Hh, P, 2) fp32 ->
    (B, N, Q, Hh, L, P, 2) int64."""
    u, v = uv[..., 0].double(), uv[..., 1].double()
    out = []
    for h, w in level_hw:
        x0 = torch.floor((u * w - 0.5).float()).long()
        y0 = torch.floor((v * h - 0.5).float()).long()
        out.append(torch.stack((x0, y0), -1))
    return torch.stack(out, dim=4)


def own_corners(uv, level_hw):
    """The corners the oracle itself would take at its own (fp64) coordinates: floor(u * W - 0.5)."""
    return torch.stack([torch.stack((torch.floor(uv[..., 0] * w - 0.5), torch.floor(uv[..., 1] * h - 0.5)), -1).long()
                        for h, w in level_hw], dim=4)


def decisions_from_parts(parts, level_hw, dropout=None):
    """A layer's decisions as the oracle itself took them (O.decoder_layer's parts): what a stand-in implementation records."""
    relu = {k: (parts['pre_' + k] > 0).reshape(-1, parts['pre_' + k].shape[-1]) for k in RELU_KINDS}
    return dict(mask=parts['mask'].detach().clone(), corners=corners_from_uv(parts['uv'].detach().float(), level_hw),
                relu=relu, dropout=dropout, level_hw=list(level_hw))


def plan_corner_mismatch(plan, mask, corners):
    """Reads the bilinear corners the plan's PAIRS form holds (gd4d_cross_attn_sliced.h: header of 16 ints per position
    padded to 256 B, then per (position, head, pass of 4 items) 64 {byte offset, weight}; slot ((item & 1) << 5) | (corner << 3)
    | ((item >> 1 & 1) << 2) | level; the items of a head are its visible (camera, point) pairs camera-major) and compares the
    clamped corners with those `corners` implies.  Decoded on the host.  Returns (item-count mismatches, corner mismatches,
    corners compared).  B = 1."""
    b, n, q, hh, p = mask.shape
    assert b == 1, 'plan_corner_mismatch: B = 1'
    pyr = plan.pyramid
    level_hw = pyr.level_hw
    hdr_bytes = (q * 16 * 4 + 255) & ~255
    cap_t = (n * p + 3) // 4
    need = hdr_bytes + q * hh * cap_t * 64 * 8
    assert plan.buf.numel() >= need, (plan.buf.numel(), need)
    buf = plan.buf[:need].detach().cpu()
    hdr = buf[:q * 16 * 4].view(torch.int32).view(q, 16)[:, :hh].long()
    pairs = buf[hdr_bytes:hdr_bytes + q * hh * cap_t * 64 * 8].view(torch.int32).view(q, hh, cap_t * 64, 2)
    order = torch.arange(q) if plan.order is None else plan.order.detach().cpu().reshape(-1).long()
    pos_of = torch.empty_like(order)
    pos_of[order] = torch.arange(q)
    vis = mask[0].detach().cpu().bool().permute(1, 2, 0, 3).reshape(q, hh, n * p)          # (query, head, camera * P + point)
    m_bad = int((hdr[pos_of] != vis.sum(-1)).sum())
    item = vis.long().cumsum(-1) - 1
    qi, hi, ci = vis.nonzero(as_tuple=True)
    it, cam, pt = item[qi, hi, ci], ci // p, ci % p
    cr = corners[0].detach().cpu()                                                            # (N, Q, Hh, L, P, 2)
    bad = total = 0
    for lvl, (h, w) in enumerate(level_hw):
        x0, y0 = cr[cam, qi, hi, lvl, pt, 0], cr[cam, qi, hi, lvl, pt, 1]
        for c in range(4):
            slot = (it >> 2) * 64 + ((it & 1) << 5) + (c << 3) + (((it >> 1) & 1) << 2) + lvl
            off = pairs[pos_of[qi], hi, slot, 0].long() & 0xFFFFFFFF
            pix = (off - cam * pyr.cam_stride[lvl]) // pyr.pix_stride
            want_x = (x0 + (c & 1)).clamp(0, w - 1)
            want_y = (y0 + (c >> 1)).clamp(0, h - 1)
            bad += int(((pix % w != want_x) | (pix // w != want_y)).sum())
            total += int(qi.numel())
    return m_bad, bad, total


class DecisionSpy:
    """Records, for every layer of ONE fused training call (fused_train.DecoderTrainFunction), the decisions its forward took.
    A context manager that monkeypatches ops functions and changes nothing in the library:
      ops.cross_attn_plan_fwd - the plan itself (kept: its pairs form holds the corners the gather used) and, recomputed from
        the launch's own arguments with want_mask / want_uv (as decoder_step.MaskSpy), the visibility mask and the coordinates;
      ops.chain_layernorm with relu=True and out= - position_encoder's two post-ReLU buffers (s.a1, s.pos_feat);
      ops.chain_gemm with relu=True and out= - the FFN's post-ReLU (and post-dropout) hidden buffer s.h.
    take() clones the buffers: call it after the forward, before the backward."""
    NAMES = ('cross_attn_plan_fwd', 'chain_layernorm', 'chain_gemm')

    def __init__(self):
        self.plans, self.masks, self.uvs, self.kinds, self.ln_relu, self.gemm_relu = [], [], [], [], [], []

    def __enter__(self):
        from graph_detr4d_amd import ops
        self.ops = ops
        self.orig = {name: getattr(ops, name) for name in self.NAMES}
        for name in self.NAMES:
            setattr(ops, name, self._spy(name, self.orig[name]))
        return self

    def __exit__(self, *exc):
        for name, fn in self.orig.items():
            setattr(self.ops, name, fn)

    def _spy(self, name, fn):
        sig = inspect.signature(fn)
        core = list(sig.parameters)[:10]

        def spy(*a, **k):
            res = fn(*a, **k)
            args = sig.bind(*a, **k).arguments
            if name == 'cross_attn_plan_fwd':
                _, mask, uv = fn(*[args[p] for p in core], want_mask=True, want_uv=True)
                self.plans.append(res[0] if isinstance(res, tuple) else res)
                self.masks.append(mask)
                self.uvs.append(uv)
                self.kinds.append(name)
            elif args.get('relu') and args.get('out') is not None:
                (self.ln_relu if name == 'chain_layernorm' else self.gemm_relu).append(args['out'])
            return res
        return spy

    def take(self, dropout=None):
        """Per layer dict(mask, corners, relu {pe1, pe4, ffn}, dropout) (dropout: per layer the five sites or None), plus
        per layer the corner check against the plan: (item-count mismatches, corner mismatches, corners compared)."""
        nl = len(self.plans)
        assert len(self.ln_relu) == 2 * nl and len(self.gemm_relu) == nl, (nl, len(self.ln_relu), len(self.gemm_relu))
        out, checks = [], []
        for lid in range(nl):
            level_hw = self.plans[lid].pyramid.level_hw
            corners = corners_from_uv(self.uvs[lid], level_hw)
            checks.append(plan_corner_mismatch(self.plans[lid], self.masks[lid], corners))
            relu = dict(pe1=self.ln_relu[2 * lid].clone() > 0, pe4=self.ln_relu[2 * lid + 1].clone() > 0,
                        ffn=self.gemm_relu[lid].clone() > 0)
            out.append(dict(mask=self.masks[lid].bool(), corners=corners, relu=relu,
                            dropout=None if dropout is None else dropout[lid], level_hw=list(level_hw)))
        return out, checks


# ------------------------------------------------------------------------------------------------------------ the stepping
def _to(dec, device):
    if dec is None:
        return {}
    mv = lambda t: None if t is None else t.to(device)          # noqa: E731
    kw = dict(vis_mask=mv(dec['mask']), corners=mv(dec['corners']),
              relu_masks={k: mv(v) for k, v in dec['relu'].items()})
    if dec.get('dropout') is not None:
        kw['dropout'] = [None if s is None else (mv(s[0]), s[1]) for s in dec['dropout']]
    return kw


def _mismatch(parts, dec):
    """The decision-mismatch report of one layer: the fp64 oracle's own choices against the forced ones."""
    own_mask, forced = parts['mask'].bool(), dec['mask'].to(parts['mask'].device).bool()
    rows = int((own_mask != forced).any(dim=4).any(dim=3).any(dim=1).any(dim=0).sum())
    level_hw = [(int(h), int(w)) for h, w in dec['level_hw']]
    cr_own = own_corners(parts['uv'].detach(), level_hw)
    cr_forced = dec['corners'].to(cr_own.device)
    vis = forced.unsqueeze(4).expand(*forced.shape[:4], len(level_hw), forced.shape[4])            # (B, N, Q, Hh, L, P)
    diff = (cr_own != cr_forced).any(-1) & vis
    res = dict(mask_rows=rows, corners=(int(diff.sum()), int(vis.sum())))
    drop = dec.get('dropout')
    for k in RELU_KINDS:
        f = dec['relu'][k].to(own_mask.device).bool()
        own = (parts['pre_' + k].detach() > 0).reshape(f.shape)
        live = torch.ones_like(f)
        if k == 'ffn' and drop is not None and drop[3] is not None:
            live = drop[3][0].to(f.device).reshape(f.shape).bool()          # a dropped unit's ReLU decides nothing
        res[k] = (int(((own != f) & live).sum()), int(live.sum()))
    why = []
    if rows > MAX_FLIPPED:
        why.append(f'mask: {rows} rows with flipped bits > {MAX_FLIPPED}')
    for k in ('corners',) + RELU_KINDS:
        bad, tot = res[k]
        if bad > MAX_FRACTION * tot:
            why.append(f'{k}: {bad} of {tot} forced decisions disagree with the oracle (> {MAX_FRACTION:g})')
    res['why'] = why
    return res


def stepped_backward(layer_params, ref_params, query_embed, feats, metas, pc, states, init_ref, refs, decisions, probes,
                     regs=None, ref_probes=None, dtype=torch.float64, device='cpu', **oracle_kw):
    """The oracle's gradients of loss = sum(states * probes) + sum(init_ref ** 2) [+ sum(refs * ref_probes)], stepped layer by
    layer on the implementation's states / refs with its decisions.  layer_params: the oracle's per-layer parameter dicts;
    ref_params: {'weight', 'bias'} of reference_points; query_embed (Q, 2C); feats: the pyramid (B, N, C, H, W) per level;
    states (NL, Q, B, C), init_ref (B, Q, 3), refs (NL, B, Q, 3): what the implementation returned; decisions: per layer
    dict(mask, corners, relu, dropout, level_hw) or None (the oracle's own); regs: the reg branches
    (refinement: the points are detached) or None (no refinement: every layer reads init_ref); ref_probes: the loss's probe of
    the returned refs (no refinement only).  Returns dict(layers=[{name: grad}], reference_points={name: grad},
    query_embed (Q, 2C), feats=[grad per level], regs=[{name: grad or None}] or None, mismatch=[per layer report])."""
    nl = len(layer_params)
    dd = dict(dtype=dtype, device=device)
    cv = lambda t: t.detach().to(**dd)                                  # noqa: E731
    lp = [{k: cv(v).requires_grad_() for k, v in p.items()} for p in layer_params]
    rp = {k: cv(v).requires_grad_() for k, v in ref_params.items()}
    fl = [cv(f).requires_grad_() for f in feats]
    qe = cv(query_embed)
    c = qe.shape[1] // 2
    qp = qe[:, :c].unsqueeze(1).clone().requires_grad_()               # query_pos (Q, B, C): one leaf for every layer
    x0 = qe[:, c:].unsqueeze(1).clone().requires_grad_()               # query
    ref0 = cv(init_ref).requires_grad_()
    regs_o = None if regs is None else [copy.deepcopy(r).to(**dd) for r in regs]
    if regs_o is not None:
        for r in regs_o:
            for prm in r.parameters():
                prm.grad = None
                prm.requires_grad_(True)
    G = cv(probes[nl - 1])
    g_ref_above = None
    mism = [None] * nl
    for lid in range(nl - 1, -1, -1):
        x = x0 if lid == 0 else cv(states[lid - 1]).requires_grad_()
        ref = ref0 if (lid == 0 or regs is None) else cv(refs[lid - 1]).requires_grad_()
        dec = decisions[lid]
        y, parts = O.decoder_layer(lp[lid], x, fl, qp, ref, metas, pc, return_parts=True, **oracle_kw, **_to(dec, device))
        outs, grads = [y], [G]
        if regs_o is not None and lid + 1 < nl:
            r = O.refine_points(regs_o[lid], y, ref)                    # the points layer l + 1 read: detached by the oracle
            if r.requires_grad:
                outs.append(r)
                grads.append(g_ref_above)
        torch.autograd.backward(outs, grads)
        if dec is not None:
            mism[lid] = _mismatch(parts, dec)
        del y, parts, outs
        g_ref_above = ref.grad if ref is not ref0 else None
        if lid > 0:
            G = cv(probes[lid - 1]) + x.grad
    # close the chain: init_ref = sigmoid(reference_points(query_pos)) (detr3d_transformer.py:133-134)
    g_init = ref0.grad + 2 * ref0.detach()
    if ref_probes is not None:
        g_init = g_init + cv(ref_probes).sum(0)
    init = torch.sigmoid(F.linear(qp.permute(1, 0, 2), rp['weight'], rp['bias']))
    torch.autograd.backward([init], [g_init])
    return dict(layers=[{k: v.grad for k, v in p.items()} for p in lp], reference_points={k: v.grad for k, v in rp.items()},
                query_embed=torch.cat([qp.grad[:, 0], x0.grad[:, 0]], 1), feats=[f.grad for f in fl],
                regs=None if regs_o is None else [{k: v.grad for k, v in r.named_parameters()} for r in regs_o],
                mismatch=mism, init_ref=init.detach())


# ------------------------------------------------------------------------------------------------------------ the comparison
def errors(a, b, rows=True):
    """(relative Frobenius error, max relative row error) of a against b (rows: the first dimension).  A row's error is
    relative to max(its norm, ROW_FLOOR x the median row norm); in a 1-D tensor (a bias, a LayerNorm parameter: one scalar per
    output unit, often a sum that cancels) an entry's error is relative to the RMS entry."""
    a, b = a.detach().double().to(b.device), b.detach().double()
    nb = b.norm()
    fro = float((a - b).norm() / nb) if nb > 0 else float((a - b).norm())
    if not rows:
        return fro, fro
    a2, b2 = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    den = b2.norm(dim=1)
    if b.dim() == 1:
        den = torch.full_like(den, float(nb) / b.numel() ** 0.5)      # an entry of a bias / LayerNorm gradient: against the RMS
    else:
        den = torch.maximum(den, ROW_FLOOR * den.median())
    num = (a2 - b2).norm(dim=1)
    row = num / den.clamp_min(1e-300)
    row = torch.where(num == 0, torch.zeros_like(row), row)
    return fro, float(row.max())


def compare(impl, ref):
    """Per checked item (where, name, relative Frobenius error, max row / block error) and the failures.  impl / ref: dicts as
    stepped_backward returns (impl's regs: None or per layer {name: grad or None})."""
    rows, fails = [], []

    def add(where, name, a, b, tol_fro=TOL_FRO, tol_row=TOL_ROW, blocks=None):
        if blocks is None:
            fro, row = errors(a, b)
        else:
            fro, row = blocks
        ok = fro <= tol_fro and row <= tol_row
        rows.append((where, name, fro, row, ok))
        if not ok:
            fails.append((where, name, fro, row))
    for lid, (gi, go) in enumerate(zip(impl['layers'], ref['layers'])):
        assert gi.keys() == go.keys(), (lid, sorted(set(gi) ^ set(go)))
        for k in go:
            if gi[k] is None:
                rows.append((f'layer {lid}', k, float('inf'), float('inf'), False))
                fails.append((f'layer {lid}', k, 'no gradient'))
                continue
            add(f'layer {lid}', k, gi[k], go[k])
    for k in ref['reference_points']:
        add('reference_points', k, impl['reference_points'][k], ref['reference_points'][k])
    c = ref['query_embed'].shape[1] // 2
    add('query_embed', 'query_pos half', impl['query_embed'][:, :c], ref['query_embed'][:, :c])
    add('query_embed', 'query half', impl['query_embed'][:, c:], ref['query_embed'][:, c:])
    for lvl, (a, b) in enumerate(zip(impl['feats'], ref['feats'])):
        a, b = a.detach().double().to(b.device), b.detach().double()
        fro = float((a - b).norm() / b.norm())
        per_cam = ((a - b).flatten(2).norm(dim=2) / b.flatten(2).norm(dim=2)).flatten()          # (B * N,) blocks
        add(f'pyramid level {lvl}', 'grad', a, b, blocks=(fro, float(per_cam.max())))
        for cam in (per_cam > TOL_ROW).nonzero().flatten().tolist():
            fails.append((f'pyramid level {lvl}', f'camera {cam}', float(per_cam[cam])))
    # reg branches: the refined points are detached - what the oracle's autograd gives (None / zero) must be what the
    # implementation gives
    for lid, go in enumerate(ref.get('regs') or []):
        gi = (impl.get('regs') or [None] * len(ref['regs']))[lid] or {}
        for k, g in go.items():
            a = gi.get(k)
            zero_o = g is None or not bool(g.any())
            zero_i = a is None or not bool(a.any())
            if zero_o:
                ok = zero_i
                rows.append((f'reg branch {lid}', k, 0.0 if ok else float('inf'), 0.0, ok))
                if not ok:
                    fails.append((f'reg branch {lid}', k, 'gradient where the oracle has none'))
            else:
                add(f'reg branch {lid}', k, a if a is not None else torch.zeros_like(g), g)
    return rows, fails


def mismatch_failures(mism):
    return {lid: m['why'] for lid, m in enumerate(mism) if m is not None and m['why']}


def layer_table(rows):
    """Per layer the worst tensor: {where: (max Frobenius error, its name, max row error, its name)}."""
    out = {}
    for where, name, fro, row, _ in rows:
        cur = out.get(where)
        if cur is None:
            out[where] = [fro, name, row, name]
        else:
            if fro > cur[0]:
                cur[0], cur[1] = fro, name
            if row > cur[2]:
                cur[2], cur[3] = row, name
    return out
