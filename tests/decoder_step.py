"""Stepping check of a whole multi-layer decoder call against the oracle (a helper of the test modules, not a test file).

A chained comparison of six layers on i.i.d. synthetic features is ill-conditioned (tests/test_full_size_gpu.py: a 1e-6
difference in a refined reference point grows ~3x per layer), and teacher forcing a one-layer call cannot see what crosses
a layer boundary inside the real call (the next layer's in-projection in chain B, the previous layer's reg branch and
refinement in chain A's second program, the position_encoder hand-off, per-layer weight images, ping-pong buffers, the
query order computed once).  Here the oracle is stepped from the implementation's OWN returned state instead: layer l of the
oracle (plus the reference-point refinement) runs on (states[l - 1], refs[l - 1]) - on (query, init_ref) for l = 0 - and
must reproduce (states[l], refs[l]).  The error is one layer's rounding, so the per-layer tolerances of the teacher-forced
tests apply unchanged; a returned state or reference point that is not what the next layer consumed fails at that layer.

Tolerances and the exclusion rule are those of tests/test_full_size_gpu.py: the visibility mask is the path's only
discontinuity, so rows whose implementation and oracle masks differ in a bit are excluded (at most MAX_FLIPPED per layer);
every other row has max error < TOL_MAX, the median row error is < TOL_MEDIAN, the refined points are within TOL_REF.
When the implementation's masks are not available (masks=None), rows that the oracle's own projection puts within NEAR_PX
pixels of a visibility threshold are excluded instead, under the same bound."""
import inspect

import torch

from oracle import torch_oracle as O

MAX_FLIPPED = 2
TOL_MAX, TOL_MEDIAN, TOL_REF = 1e-3, 2e-4, 1e-3
NEAR_PX = 1e-2


def refine(reg, y, ref):
    """Reference-point refinement (detr3d_transformer.py:199-214), as tests/test_full_size_gpu.py restates it."""
    tmp = reg(y.permute(1, 0, 2))
    new = torch.zeros_like(ref)
    new[..., :2] = tmp[..., :2] + O.inverse_sigmoid(ref[..., :2])
    new[..., 2:3] = tmp[..., 4:5] + O.inverse_sigmoid(ref[..., 2:3])
    return new.sigmoid()


def near_threshold_rows(uv, img_h, img_w, px=NEAR_PX):
    """(Q,) bool: queries with a sampling point (any batch, camera, head, point) within `px` pixels of the image border, i.e.
    of a threshold of the visibility mask 0 < u < 1, 0 < v < 1.  uv (B, N, Q, Hh, P, 2) normalised, as O.project returns."""
    u, v = uv[..., 0], uv[..., 1]
    du, dv = px / img_w, px / img_h
    u_in, v_in = (u > -du) & (u < 1 + du), (v > -dv) & (v < 1 + dv)
    u_edge = (u.abs() < du) | ((u - 1).abs() < du)
    v_edge = (v.abs() < dv) | ((v - 1).abs() < dv)
    near = (u_edge & v_in) | (v_edge & u_in)                            # (B, N, Q, Hh, P)
    return near.any(dim=4).any(dim=3).any(dim=1).any(dim=0)


class LayerStat(tuple):
    """(rows excluded, max error of the other rows, median row error, max ref error of the other rows) + the failures."""

    def __new__(cls, excluded, err_max, err_median, ref_max, why):
        self = super().__new__(cls, (excluded, err_max, err_median, ref_max))
        self.why = why
        return self

    @property
    def ok(self):
        return not self.why


def step_stats(layer_params, regs_cpu, query, query_pos, feats, metas, pc, states, init_ref, refs, masks=None,
               near_px=NEAR_PX, **oracle_kw):
    """Per-layer LayerStat of the stepped comparison (nothing asserted).  layer_params: the oracle's per-layer parameter dicts;
    regs_cpu: per-layer reg branches (callables) or None (no refinement: refs[l] must be the points layer l used); query /
    query_pos (Q, B, C); states (NL, Q, B, C), init_ref (B, Q, 3), refs (NL, B, Q, 3): what the implementation returned;
    masks: per layer the implementation's visibility mask (B, N, Q, Hh, P), or None; oracle_kw: O.decoder_layer's options."""
    nl = len(layer_params)
    states, init_ref, refs = states.detach().cpu(), init_ref.detach().cpu(), refs.detach().cpu()
    assert states.shape[0] == nl and refs.shape[0] == nl, (tuple(states.shape), tuple(refs.shape), nl)
    assert masks is None or len(masks) == nl, f'{len(masks)} gather masks recorded for {nl} layers'
    img_h, img_w = metas[0]['img_shape'][0][0], metas[0]['img_shape'][0][1]
    out = []
    with torch.no_grad():
        for lid in range(nl):
            x, ref = (query, init_ref) if lid == 0 else (states[lid - 1], refs[lid - 1])
            y_ref, parts = O.decoder_layer(layer_params[lid], x, feats, query_pos, ref, metas, pc, return_parts=True,
                                           **oracle_kw)
            ref_next = ref if regs_cpu is None else refine(regs_cpu[lid], y_ref, ref)
            if masks is not None:
                mism = masks[lid].detach().cpu().bool() != parts['mask']                  # (B, N, Q, Hh, P)
                skip = mism.any(dim=4).any(dim=3).any(dim=1).any(dim=0)                   # (Q,)
            else:
                skip = near_threshold_rows(parts['uv'], img_h, img_w, near_px)
            err = (states[lid].to(y_ref.dtype) - y_ref).abs().amax(dim=(1, 2))            # per query row
            rerr = (refs[lid].to(ref_next.dtype) - ref_next).abs().amax(dim=(0, 2))
            keep = ~skip
            e_max = float(err[keep].max()) if keep.any() else 0.0
            r_max = float(rerr[keep].max()) if keep.any() else 0.0
            e_med = float(err.median())
            why = []
            if int(skip.sum()) > MAX_FLIPPED:
                why.append(f'{int(skip.sum())} rows excluded > {MAX_FLIPPED}')
            if not e_max < TOL_MAX:
                why.append(f'max row error {e_max:.3g} >= {TOL_MAX}')
            if not e_med < TOL_MEDIAN:
                why.append(f'median row error {e_med:.3g} >= {TOL_MEDIAN}')
            if not r_max < TOL_REF:
                why.append(f'reference-point error {r_max:.3g} >= {TOL_REF}')
            out.append(LayerStat(int(skip.sum()), e_max, e_med, r_max, why))
    return out


def step_check(layer_params, regs_cpu, query, query_pos, feats, metas, pc, states, init_ref, refs, masks=None, label='',
               near_px=NEAR_PX, **oracle_kw):
    """step_stats, printed, and asserted layer by layer: the AssertionError names every failing layer."""
    stats = step_stats(layer_params, regs_cpu, query, query_pos, feats, metas, pc, states, init_ref, refs, masks=masks,
                       near_px=near_px, **oracle_kw)
    kind = 'flipped' if masks is not None else f'within {near_px} px of a threshold'
    print(f'{label}: per layer (rows {kind}, max error of the other rows, median row error, max ref error):',
          [tuple(f'{v:.2e}' if isinstance(v, float) else v for v in s) for s in stats])
    bad = {lid: s.why for lid, s in enumerate(stats) if not s.ok}
    assert not bad, f'{label}: stepped layers fail: {bad}; all layers: {[tuple(s) for s in stats]}'
    return stats


class MaskSpy:
    """Records the visibility mask of every gather of a call, in launch order: the plan kernel's for the sliced gathers
    (ops.cross_attn_plan_fwd: bit-exact to the C oracle, tests/test_timed_size_parity_gpu.py), the row gather's
    (ops.cross_attn_agg_fwd) and the projected-value gather's (ops.cross_attn_fwd) - each recomputed from the arguments of
    the launch being recorded, with want_mask=True, next to it.  A context manager; `masks` is the list."""
    NAMES = ('cross_attn_plan_fwd', 'cross_attn_agg_fwd', 'cross_attn_fwd')

    def __init__(self):
        self.masks, self.kinds = [], []

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
        core = list(sig.parameters)[:10 if name == 'cross_attn_plan_fwd' else (11 if name == 'cross_attn_agg_fwd' else 10)]

        def spy(*a, **k):
            res = fn(*a, **k)
            args = sig.bind(*a, **k).arguments
            extra = {'head_major': args.get('head_major', False)} if name == 'cross_attn_fwd' else {}
            again = fn(*[args[p] for p in core], want_mask=True, **extra)
            self.masks.append(again[-1] if name == 'cross_attn_agg_fwd' else again[1])
            self.kinds.append(name)
            return res
        return spy
