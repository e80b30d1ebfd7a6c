"""Stepped-backward parity of the decoder's training step at the timed size (900 queries x 24 cameras, R50 pyramid, 6 layers).

ONE call through fused_train.DecoderTrainFunction (bench.py --mode train's decoder: build_decoder(G, 24, 6, 'fp32', 1002) and its
reg branches), loss = sum(states * probe) + sum(init_ref ** 2) (+ sum(refs * ref_probe) without refinement), its decisions
recorded by tests/train_step.DecisionSpy; then the oracle is stepped backward layer by layer on the call's own states, refs and
decisions (tests/train_step.stepped_backward) and every gradient is compared:

  (A) the implementation against the fp64 stepped oracle
  (C) the fp32 oracle, stepped with the same decisions, against the same fp64 oracle - what fp32 arithmetic itself loses

Cases: refine (eval mode, reg branches: the bench's default), no-refine (no reg branches: the reference points' gradient flows
through every layer), dropout (train mode, p = 0.1 at the five sites, seeds fixed through fused_train.draw_seeds).
The oracle runs through ATen, on the GPU when there is one.

    python tools/stepped_backward_parity.py [--case refine] [--json OUT]        (GPU)
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

CASES = ('refine', 'no-refine', 'dropout')
NL, Q, N = 6, 900, 24


def _dropout_sites(fused_train, ops, layers, seeds, q):
    """Per layer the five (keep mask, p) sites of fused_train's s.drop, from the seeds the call drew (None: no dropout)."""
    out = []
    for lid, layer in enumerate(layers):
        drops = fused_train._dropouts(layer)
        fc = layer.ffns[0].feedforward_channels
        sites = []
        for i, pr in enumerate(drops):
            if pr <= 0.:
                sites.append(None)
                continue
            seed = seeds[5 * lid + i:5 * lid + i + 1]
            keep = ops.mha_dropout_keep_mask(seed, 1, layer.attentions[0].num_heads, q, q, pr) if i == 0 else \
                ops.chain_dropout_keep_mask(seed, q, fc if i == 3 else 256, pr)
            sites.append((keep, pr))
        out.append(sites)
    return out


def run_case(case, oracle_device=None, yardstick=True):
    """One case: the implementation's gradients, the fp64 (and fp32) stepped oracle's, the comparisons and the checks."""
    import bench
    import graph_detr4d_amd as G
    from graph_detr4d_amd import fused_train, ops, synthetic
    import train_step as TS
    dev = 'cuda'
    odev = oracle_device or dev
    pc = synthetic.PC_RANGE
    tr, regs = bench.build_decoder(G, N, NL, 'fp32', 1002)
    sd, layer_params = bench.state_as_oracle_params(tr)
    ref_params = {'weight': sd['reference_points.weight'], 'bias': sd['reference_points.bias']}
    refine = case != 'no-refine'
    regs_cpu = list(regs) if refine else None
    feats = synthetic.feature_pyramid(N, synthetic.R50_LEVELS, seed=79)
    gen = torch.Generator().manual_seed(8)
    qe = torch.randn(Q, 512, generator=gen)
    probes = torch.randn(NL, Q, 1, 256, generator=gen)
    ref_probes = torch.randn(NL, 1, Q, 3, generator=gen)
    seeds = torch.randint(-2 ** 62, 2 ** 62, (5 * NL,), generator=gen, dtype=torch.int64).to(dev)
    metas = synthetic.make_img_metas(synthetic.camera_rig(4), batch=1)
    tr = tr.to(dev)
    tr.train() if case == 'dropout' else tr.eval()
    regs_d = regs.to(dev).eval() if refine else None
    feats_d = [f.to(dev).requires_grad_() for f in feats]
    qe_d = qe.to(dev).requires_grad_()
    orig_draw = fused_train.draw_seeds
    fused_train.draw_seeds = lambda k, d: seeds[:k].clone()
    before = fused_train.CALLS[0]
    t0 = time.perf_counter()
    try:
        with TS.DecisionSpy() as spy:
            states, init_ref, refs = tr(feats_d, qe_d, reg_branches=regs_d, img_metas=metas)
        torch.cuda.synchronize()
    finally:
        fused_train.draw_seeds = orig_draw
    calls = fused_train.CALLS[0] - before
    layers = list(tr.decoder.layers)
    sites = _dropout_sites(fused_train, ops, layers, seeds, Q) if case == 'dropout' else None
    decisions, plan_checks = spy.take(sites)
    loss = (states * probes.to(dev)).sum() + (init_ref ** 2).sum()
    if not refine:
        loss = loss + (refs * ref_probes.to(dev)).sum()
    loss.backward()
    torch.cuda.synchronize()
    t_impl = time.perf_counter() - t0
    named = dict(tr.named_parameters())
    impl = dict(layers=[{k: named[f'decoder.layers.{lid}.{k}'].grad for k in layer_params[lid]} for lid in range(NL)],
                reference_points={k: named['reference_points.' + k].grad for k in ref_params},
                query_embed=qe_d.grad, feats=[f.grad for f in feats_d],
                regs=None if not refine else [{k: v.grad for k, v in r.named_parameters()} for r in regs_d])
    common = dict(regs=regs_cpu, ref_probes=None if refine else ref_probes, device=odev)
    st, ir, rf = states.detach(), init_ref.detach(), refs.detach()
    t0 = time.perf_counter()
    ora = TS.stepped_backward(layer_params, ref_params, qe, feats, metas, pc, st, ir, rf, decisions, probes,
                              dtype=torch.float64, **common)
    t64 = time.perf_counter() - t0
    res = dict(case=case, calls=calls, kinds=list(spy.kinds), plan_checks=plan_checks, oracle_device=str(odev),
               mismatch=ora['mismatch'], init_ref_err=float((ir.double().to(odev) - ora['init_ref']).abs().max()),
               seconds=dict(implementation=t_impl, oracle_fp64=t64))
    if yardstick:
        t0 = time.perf_counter()
        o32 = TS.stepped_backward(layer_params, ref_params, qe, feats, metas, pc, st, ir, rf, decisions, probes,
                                  dtype=torch.float32, **common)
        res['seconds']['oracle_fp32'] = time.perf_counter() - t0
        res['rows_C'], res['fails_C'] = TS.compare(o32, ora)
        del o32
    res['rows_A'], res['fails_A'] = TS.compare(impl, ora)
    del ora
    torch.cuda.empty_cache()
    return res


def table(res):
    """Per layer (and the closing items) the worst relative Frobenius error and the worst row / block error, A next to C; then
    the decision-mismatch counts."""
    import train_step as TS
    a = TS.layer_table(res['rows_A'])
    c = TS.layer_table(res['rows_C']) if 'rows_C' in res else {}
    lines = [f"case {res['case']} (oracle on {res['oracle_device']}; seconds: "
             + ', '.join(f'{k} {v:.1f}' for k, v in res['seconds'].items()) + ')',
             '| where | A: worst Frobenius (tensor) | A: worst row | C: worst Frobenius | C: worst row |',
             '|---|---|---|---|---|']
    for where, (fro, fn, row, rn) in a.items():
        cc = c.get(where)
        cs = f'{cc[0]:.2e} ({cc[1]}) | {cc[2]:.2e} ({cc[3]})' if cc else '- | -'
        lines.append(f'| {where} | {fro:.2e} ({fn}) | {row:.2e} ({rn}) | {cs} |')
    lines += ['', '| layer | mask rows flipped | corners off | ReLU pe1 off | ReLU pe4 off | ReLU ffn off | plan: counts / corners off |',
              '|---|---|---|---|---|---|---|']
    for lid, m in enumerate(res['mismatch']):
        pc = res['plan_checks'][lid]
        lines.append(f"| {lid} | {m['mask_rows']} | {m['corners'][0]} / {m['corners'][1]} | {m['pe1'][0]} / {m['pe1'][1]} | "
                     f"{m['pe4'][0]} / {m['pe4'][1]} | {m['ffn'][0]} / {m['ffn'][1]} | {pc[0]} / {pc[1]} of {pc[2]} |")
    return '\n'.join(lines)


def _jsonable(res):
    out = dict(res)
    out['mismatch'] = [{k: v for k, v in m.items()} for m in res['mismatch']]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--case', choices=CASES, action='append', help='default: all three')
    ap.add_argument('--oracle-device', default=None, help='where the oracle runs (default: cuda)')
    ap.add_argument('--json', default=None, help='also write the measurements as JSON here')
    a = ap.parse_args()
    torch.set_num_threads(16)
    out = []
    for case in a.case or CASES:
        res = run_case(case, a.oracle_device)
        print(table(res))
        print(f"A fails: {res['fails_A']}\nC fails: {res.get('fails_C')}", flush=True)
        out.append(_jsonable(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
