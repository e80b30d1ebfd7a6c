#!/usr/bin/env python
"""GPU time of PETR's global cross-attention (900 queries x 6 000 - 24 000 keys, batch 1, 8 heads of 32) on gd4d_cross_mha_fwd beside
the two other ways to compute it on the same GPU and the same random data.  Prints ONE JSON line per key count.

    python tools/bench_cross_mha.py [--lk 6000,12000,24000] [--lq 900] [--rounds 7] [--window-ms 100] [--timeout 240]
    python tools/bench_cross_mha.py --one 12000 ...      one key count in this process (what the driver starts)

Without --one the script is a driver that has not touched the GPU: it starts one fresh child process per key count, each under its
own time limit (--timeout seconds), and stops at the first child that fails or runs out of time.

Variants, their windows interleaved in one process (a WINDOW is k consecutive calls between two device events, k sized so that a window
lasts --window-ms; median and min over --rounds windows of the window's time per call, in microseconds):
  core               gd4d_cross_mha_fwd on pre-split planes, the library's own plan (+ its merge kernel)
  core_q<T>_s<S>     the same with a query tile of T and S key splits forced: the alternatives to the plan
  pack               gd4d_cross_mha_pack_kv: the fp32 K|V projection (Lk, 1, 512) -> the planes
  pack+core          the two in sequence: what a layer pays
  mha_core           gd4d_mha_core_fwd on the fp32 K / V rows with the mask expanded to (Lq, Lk) bool - the only way the library could
                     compute this before
  sdpa_fp32          torch's F.scaled_dot_product_attention on fp32 (1, 8, L, 32) tensors with the equivalent boolean mask
  module / module_torch_ops   a whole PETRMultiheadAttention call (two projections, pack, core, out-projection + residual) on the kernel
                     route and with torch_ops=True (F.multi_head_attention_forward)
Data is randn, the mask pads a random 10 % of the keys.  `max_abs_diff_*` compares the variants' outputs at the timed size.

    python tools/bench_cross_mha.py --train [--lk 6000,12000] ...      forward + backward (drop_p = 0.1); same driver, same windows
  core_train         both training packs, gd4d_cross_mha_train_fwd and gd4d_cross_mha_bwd (its query-side pack, two compute kernels
                     and merge): what autograd.CrossMhaFunction runs for one layer
  core_train_fwd / core_train_bwd    the two halves of it, each with its pack
  mha_core_train     gd4d_mha_core_fwd with lse + gd4d_mha_core_bwd on the fp32 rows with the mask expanded to (Lq, Lk): the only
                     kernel way before (valid at batch 1 only)
  module_train / module_torch_ops_train    forward + backward of one PETRMultiheadAttention call in train mode (dropout 0.1),
                     hip_train=True and torch_ops=True; `peak_bytes`: torch.cuda.max_memory_allocated over one such call, minus what
                     was allocated before it
"""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALTERNATIVES = [(64, 1), (64, 2), (64, 3), (64, 4), (64, 6), (64, 9), (32, 1), (32, 2), (32, 3), (32, 5)]


def event_us(fn, calls):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def windows(fns, rounds, window_ms):
    """name -> dict(median_us, min_us, max_us, calls); the callables' windows alternate within every round."""
    import numpy as np
    calls = {}
    for k, f in fns.items():
        f()
        once = event_us(f, 3)
        calls[k] = max(1, min(2000, math.ceil(window_ms * 1e3 / max(once, 1.0))))
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            ts[k].append(event_us(f, calls[k]))
    return {k: dict(median_us=float(np.median(v)), min_us=float(min(v)), max_us=float(max(v)), calls=calls[k]) for k, v in ts.items()}


def bench(lq, lk, rounds, window_ms):
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ROOT)
    import graph_detr4d_amd as G
    from graph_detr4d_amd import ops
    dev, h, c = 'cuda', 8, 256
    g = torch.Generator(dev).manual_seed(lk)
    q = torch.randn(lq, 1, c, device=dev, generator=g)
    kvp = torch.randn(lk, 1, 2 * c, device=dev, generator=g)
    k, v = kvp[..., :c], kvp[..., c:]
    mask = torch.rand(1, lk, device=dev, generator=g) < 0.1
    full = mask.expand(lq, lk).contiguous()
    q4, k4, v4 = (t.reshape(t.shape[0], h, 32).transpose(0, 1)[None].contiguous() for t in (q, k, v))
    keep = (~mask)[:, None, None, :]
    kv = ops.cross_mha_pack_kv(k, v)
    plan = ops.cross_mha_plan(lq, lk, 1, h)
    fns = {'core': lambda: ops.cross_mha_fwd(q, kv, h, key_padding_mask=mask)}
    for qt, s in ALTERNATIVES:
        if (qt, s) != (plan.q_tile, plan.splits):
            fns[f'core_q{qt}_s{s}'] = lambda qt=qt, s=s: ops.cross_mha_fwd(q, kv, h, key_padding_mask=mask, q_tile=qt, splits=s)
    fns['pack'] = lambda: ops.cross_mha_pack_kv(k, v, kv)
    fns['pack+core'] = lambda: ops.cross_mha_fwd(q, ops.cross_mha_pack_kv(k, v, kv), h, key_padding_mask=mask)
    fns['mha_core'] = lambda: ops.mha_core_fwd(q, k, v, h, full)
    fns['sdpa_fp32'] = lambda: F.scaled_dot_product_attention(q4, k4, v4, attn_mask=keep)
    mod = G.build_attention(dict(type='PETRMultiheadAttention', embed_dims=c, num_heads=h)).to(dev).eval()
    tmod = G.build_attention(dict(type='PETRMultiheadAttention', embed_dims=c, num_heads=h, torch_ops=True)).to(dev).eval()
    tmod.load_state_dict(mod.state_dict())
    query, memory = torch.randn(lq, 1, c, device=dev, generator=g), torch.randn(lk, 1, c, device=dev, generator=g)
    qpos, kpos = torch.randn(lq, 1, c, device=dev, generator=g), torch.randn(lk, 1, c, device=dev, generator=g)
    call = lambda m: m(query, memory, memory, None, query_pos=qpos, key_pos=kpos, key_padding_mask=mask)      # noqa: E731
    fns['module'] = lambda: call(mod)
    fns['module_torch_ops'] = lambda: call(tmod)
    with torch.no_grad():
        res = windows(fns, rounds, window_ms)
        a, b_, s_ = fns['core'](), fns['mha_core'](), fns['sdpa_fp32']()
        s_ = s_[0].transpose(0, 1).reshape(lq, 1, c)
        out = dict(device=torch.cuda.get_device_name(0), lq=lq, lk=lk, rounds=rounds, window_ms=window_ms,
                   plan=dict(q_tile=plan.q_tile, splits=plan.splits, grid=list(plan.grid), workgroups=plan.workgroups), variants=res,
                   max_abs_diff_core_vs_mha_core=float((a - b_).abs().max()), max_abs_diff_core_vs_sdpa=float((a - s_).abs().max()),
                   max_abs_diff_module_vs_torch_ops=float((call(mod) - call(tmod)).abs().max()))
    out['pack_plus_core_over_mha_core'] = res['pack+core']['median_us'] / res['mha_core']['median_us']
    return out


def bench_train(lq, lk, rounds, window_ms):
    import torch
    sys.path.insert(0, ROOT)
    import graph_detr4d_amd as G
    from graph_detr4d_amd import ops
    dev, h, c, p = 'cuda', 8, 256, 0.1
    g = torch.Generator(dev).manual_seed(lk)
    q = torch.randn(lq, 1, c, device=dev, generator=g)
    kvp = torch.randn(lk, 1, 2 * c, device=dev, generator=g)
    k, v = kvp[..., :c], kvp[..., c:]
    dout = torch.randn(lq, 1, c, device=dev, generator=g)
    mask = torch.rand(1, lk, device=dev, generator=g) < 0.1
    full = mask.expand(lq, lk).contiguous()
    seed = ops.mha_dropout_seed(dev)
    plan = ops.cross_mha_bwd_plan(lq, lk, 1, h)
    kf, kb = ops.CrossKV(lk, 1, dev, h, train='forward'), ops.CrossKV(lk, 1, dev, h, train='backward')

    def fwd():
        return ops.cross_mha_fwd(q, ops.cross_mha_pack_kv(k, v, kf, train='forward'), h, key_padding_mask=mask, want_lse=True,
                                 dropout_p=p, seed=seed)
    out, lse = fwd()

    def bwd():
        return ops.cross_mha_bwd(dout, q, out, lse, ops.cross_mha_pack_kv(k, v, kb, train='backward'), h, key_padding_mask=mask,
                                 dropout_p=p, seed=seed, packed_kv=True)

    def old():
        o, l = ops.mha_core_fwd(q, k, v, h, full, want_lse=True, dropout_p=p, seed=seed)
        return ops.mha_core_bwd(q, k, v, o, dout, l, h, full, dropout_p=p, seed=seed)
    fns = {'core_train': lambda: (fwd(), bwd()), 'core_train_fwd': fwd, 'core_train_bwd': bwd, 'mha_core_train': old}
    mods = {}
    for name, kw in (('module_train', dict(hip_train=True)), ('module_torch_ops_train', dict(torch_ops=True))):
        m = G.build_attention(dict(type='PETRMultiheadAttention', embed_dims=c, num_heads=h, dropout=p, **kw)).to(dev).train()
        if mods:
            m.load_state_dict(next(iter(mods.values())).state_dict())
        mods[name] = m
    query, memory = (torch.randn(n, 1, c, device=dev, generator=g).requires_grad_(True) for n in (lq, lk))
    qpos, kpos = torch.randn(lq, 1, c, device=dev, generator=g), torch.randn(lk, 1, c, device=dev, generator=g)
    gy = torch.randn(lq, 1, c, device=dev, generator=g)

    def step(m):
        y = m(query, memory, memory, None, query_pos=qpos, key_pos=kpos, key_padding_mask=mask)
        torch.autograd.backward(y, gy)
        for t in (query, memory, *m.parameters()):
            t.grad = None
    for name, m in mods.items():
        fns[name] = lambda m=m: step(m)
    res = windows(fns, rounds, window_ms)
    for name, m in mods.items():
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        step(m)
        torch.cuda.synchronize()
        res[name]['peak_bytes'] = int(torch.cuda.max_memory_allocated() - before)
    new, ref = bwd(), old()
    dkv = torch.cat([ref[1], ref[2]], dim=-1)
    out = dict(device=torch.cuda.get_device_name(0), mode='train', lq=lq, lk=lk, drop_p=p, rounds=rounds, window_ms=window_ms,
               plan=dict(q_tile=plan.q_tile, splits=plan.splits, query_grid=list(plan.query_grid), key_grid=list(plan.key_grid),
                         key_block=plan.key_block, pack_bytes=plan.pack_bytes, partial_bytes=plan.partial_bytes),
               saved_bytes=dict(repack=int(kvp.numel() * 4), keep_planes=int(4 * kf.k.numel() * 2)), variants=res,
               max_abs_diff_dq_vs_mha_core=float((new[0] - ref[0]).abs().max()),
               max_abs_diff_dkv_vs_mha_core=float((new[1] - dkv).abs().max()))
    out['core_train_over_mha_core_train'] = res['core_train']['median_us'] / res['mha_core_train']['median_us']
    out['module_train_over_torch_ops'] = res['module_train']['median_us'] / res['module_torch_ops_train']['median_us']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lk', default='6000,12000,24000')
    ap.add_argument('--lq', type=int, default=900)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--window-ms', type=float, default=100.0)
    ap.add_argument('--timeout', type=float, default=240.0, help='driver: seconds each key count\'s process may take')
    ap.add_argument('--one', type=int, default=0, help='measure this key count in this process')
    ap.add_argument('--train', action='store_true', help='forward + backward variants instead of the inference ones')
    args = ap.parse_args()
    if args.one:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('bench_cross_mha.py needs a GPU: a CPU timing says nothing about the kernels')
        print(json.dumps((bench_train if args.train else bench)(args.lq, args.one, args.rounds, args.window_ms)), flush=True)
        return
    for lk in args.lk.split(','):
        cmd = [sys.executable, os.path.abspath(__file__), '--one', lk, '--lq', str(args.lq), '--rounds', str(args.rounds),
               '--window-ms', str(args.window_ms)] + (['--train'] if args.train else [])
        try:
            rc = subprocess.run(cmd, cwd=ROOT, timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit(f'lk = {lk}: no result within {args.timeout} s - stopping here')
        if rc != 0:
            raise SystemExit(f'lk = {lk}: exit status {rc} - stopping here')


if __name__ == '__main__':
    main()
