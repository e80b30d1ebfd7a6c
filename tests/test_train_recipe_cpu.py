"""TrainRecipe's host side (graph_detr4d_amd/recipe.py) and gd4d_adamw_recipe_flat's argument validation: no GPU.

The schedule is mmcv 1.x's LrUpdaterHook restated (include/gd4d.h carries the formulas); the hand-checked values below are those of
the reference's lr_config (projects/configs/detr4d/detr4d_res50_deform_pe_testaug_320_fullset_ceph.py:215-220)."""
import ctypes
import math
import os
import re

import pytest
import torch

OPTIMIZER = dict(type='AdamW', lr=2e-4, paramwise_cfg=dict(custom_keys={'img_backbone': dict(lr_mult=0.1)}), weight_decay=0.01)
OPTIMIZER_CONFIG = dict(grad_clip=dict(max_norm=35, norm_type=2))
LR_CONFIG = dict(policy='CosineAnnealing', warmup='linear', warmup_iters=500, warmup_ratio=1.0 / 3, min_lr_ratio=1e-3)
FP16 = dict(loss_scale=512.)


class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.img_backbone = torch.nn.ModuleDict(dict(layer1=torch.nn.Linear(5, 3), layer4=torch.nn.Linear(7, 3)))
        self.pts_bbox_head = torch.nn.Linear(3, 9)


def _recipe(model=None, buckets=None, **kw):
    from graph_detr4d_amd import TrainRecipe, dist as D
    model = model or _Model()
    red = D.FlatGradAllReducer(list(model.parameters()), align=4, buckets=buckets)
    args = dict(optimizer=OPTIMIZER, optimizer_config=OPTIMIZER_CONFIG, lr_config=LR_CONFIG, fp16=FP16, max_epochs=24, iters_per_epoch=1000)
    args.update(kw)
    return TrainRecipe(red, model.named_parameters(), **args), red, model


def test_package_exports_the_recipe_and_the_library_its_entry_points(repo_root):
    import graph_detr4d_amd as G
    from graph_detr4d_amd import _lib
    assert 'TrainRecipe' in G.__all__ and G.TrainRecipe is G.recipe.TrainRecipe
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(repo_root, 'include', 'gd4d.h')).read(), flags=re.S)
    lib = _lib.load()
    for name in ('gd4d_adamw_recipe_flat', 'gd4d_adamw_recipe_flat_workspace_bytes', 'gd4d_adamw_recipe_flat_state_bytes'):
        assert re.search(r'\b%s\s*\(' % name, hdr), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.gd4d_abi_version() == 56                                         # additive: the ABI version does not move
    assert lib.gd4d_adamw_recipe_flat_state_bytes() == 64
    assert lib.gd4d_adamw_recipe_flat_workspace_bytes() == 512 * 8              # a partial sum and a flag per block of pass 1
    assert ctypes.sizeof(G.recipe.RecipeRange) == 24


def test_cosine_schedule_equals_torchs_closed_form_where_they_coincide():
    """by_epoch=False and no warmup: mmcv's CosineAnnealing is torch.optim.lr_scheduler.CosineAnnealingLR's closed form.  Both are a
    handful of double operations in another order: 1e-12 relative is ~4000 double ulps of margin over that."""
    max_iters, base, eta_min = 240, 2e-4, 2e-7
    rec, _, _ = _recipe(lr_config=dict(policy='CosineAnnealing', by_epoch=False, min_lr=eta_min), max_epochs=24, iters_per_epoch=10)
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=base)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=max_iters, eta_min=eta_min)
    for it in range(max_iters + 1):
        sched.last_epoch = it
        assert rec.lr_at(it) == pytest.approx(sched._get_closed_form_lr()[0], rel=1e-12, abs=0), it
    ratio, _, _ = _recipe(lr_config=dict(policy='CosineAnnealing', by_epoch=False, min_lr_ratio=1e-3), max_epochs=24, iters_per_epoch=10)
    assert [ratio.lr_at(i) for i in (0, 7, 240)] == pytest.approx([rec.lr_at(i) for i in (0, 7, 240)], rel=1e-15)


def test_reference_config_schedule_hand_checked():
    rec, _, _ = _recipe()
    base, n = 2e-4, 1000
    approx = lambda v: pytest.approx(v, rel=1e-12, abs=0)                      # noqa: E731
    assert rec.lr_at(0) == approx(base / 3)                                    # warmup_ratio
    assert rec.lr_at(1) == approx(base * (1 - (499 / 500) * (2 / 3)))          # 0.33466.. base
    assert rec.lr_at(499) == approx(base * (1 - (1 / 500) * (2 / 3)))          # 0.99866.. base
    assert rec.lr_at(500) == base and rec.lr_at(501) == base                   # epoch 0 after the warmup: cos(0) = 1
    assert rec.lr_at(n - 1) == base
    # by_epoch: the rate moves at epoch boundaries only.  Epoch 1: 2e-7 + 0.5 * 1.998e-4 * (cos(pi / 24) + 1)
    assert rec.lr_at(n) == pytest.approx(1.9914534165e-4, rel=1e-9)
    assert rec.lr_at(n) == rec.lr_at(2 * n - 1) > rec.lr_at(2 * n)
    assert rec.lr_at(12 * n) == approx(0.5 * (base + base * 1e-3))             # half way: cos(pi / 2) = 0
    last, before = rec.lr_at(23 * n), rec.lr_at(22 * n)
    assert base * 1e-3 < last < before
    assert last == pytest.approx(2e-7 + 0.5 * 1.998e-4 * (1 - math.cos(math.pi / 24)), rel=1e-9)
    # the other warmups and the step policy
    const, _, _ = _recipe(lr_config=dict(policy='fixed', warmup='constant', warmup_iters=10, warmup_ratio=0.25))
    assert [const.lr_at(i) for i in (0, 9, 10)] == [base * 0.25, base * 0.25, base]
    exp, _, _ = _recipe(lr_config=dict(policy='fixed', warmup='exp', warmup_iters=10, warmup_ratio=0.25))
    assert exp.lr_at(0) == approx(base * 0.25) and exp.lr_at(5) == approx(base * 0.5) and exp.lr_at(10) == base
    step, _, _ = _recipe(lr_config=dict(policy='step', step=[8, 11]), max_epochs=12)
    assert [step.lr_at(e * n) for e in (0, 7, 8, 10, 11)] == pytest.approx([base, base, base * 0.1, base * 0.1, base * 0.01], rel=1e-12)
    every, _, _ = _recipe(lr_config=dict(policy='step', step=3, gamma=0.5, by_epoch=False))
    assert [every.lr_at(i) for i in (0, 2, 3, 6)] == [base, base, base * 0.5, base * 0.25]


def test_custom_keys_match_as_mmcv_and_ranges_tile_an_interleaved_buffer():
    model = _Model()
    bb, head = model.img_backbone, model.pts_bbox_head
    # buckets interleave the groups: layer1.weight | head | layer1.bias, layer4
    buckets = [[bb['layer1'].weight], list(head.parameters()), [bb['layer1'].bias] + list(bb['layer4'].parameters())]
    opt = dict(OPTIMIZER, paramwise_cfg=dict(custom_keys={'img_backbone': 0.1, 'img_backbone.layer4': dict(lr_mult=0.5, decay_mult=0.0)}))
    rec, red, _ = _recipe(model, buckets=buckets, optimizer=opt)
    mults = dict(rec.param_mults)
    assert mults['img_backbone.layer4.weight'] == (0.5, 0.0) and mults['img_backbone.layer4.bias'] == (0.5, 0.0)   # the longer key wins
    assert mults['img_backbone.layer1.weight'] == (0.1, 1.0) and mults['pts_bbox_head.bias'] == (1.0, 1.0)
    r = rec.ranges
    assert [x[2] for x in r] == [0.1, 1.0, 0.1, 0.5]                           # not contiguous per group
    assert r[0][0] == 0 and r[-1][1] == red.numel
    assert all(a[1] == b[0] for a, b in zip(r, r[1:])) and all(b < e for b, e, _, _ in r)     # sorted, exactly once
    assert all(b % 4 == 0 for b, _, _, _ in r)
    names = {id(p): n for n, p in model.named_parameters()}
    for p, off in zip(red.params, red._offsets):
        hit = [x for x in r if x[0] <= off and off + p.numel() <= x[1]]
        assert len(hit) == 1 and hit[0][2:] == mults[names[id(p)]]
    assert red.numel > sum(p.numel() for p in red.params)                      # (the layout has padding: 15- and 3-element tensors)


def test_what_is_not_implemented_raises_naming_it():
    from graph_detr4d_amd import dist as D
    from graph_detr4d_amd._lib import Gd4dError
    bad = [
        (dict(lr_config=dict(policy='OneCycle')), 'OneCycle'),
        (dict(lr_config=dict(LR_CONFIG, warmup_by_epoch=True)), 'warmup_by_epoch'),
        (dict(lr_config=dict(LR_CONFIG, momentum=0.9)), 'momentum'),
        (dict(lr_config=dict(LR_CONFIG, warmup='cosine')), 'cosine'),
        (dict(optimizer=dict(OPTIMIZER, paramwise_cfg=dict(bias_lr_mult=2.0))), 'bias_lr_mult'),
        (dict(optimizer=dict(OPTIMIZER, paramwise_cfg=dict(custom_keys={}, norm_decay_mult=0.0))), 'norm_decay_mult'),
        (dict(optimizer=dict(OPTIMIZER, type='SGD')), 'SGD'),
        (dict(optimizer=dict(OPTIMIZER, amsgrad=True)), 'amsgrad'),
        (dict(optimizer_config=dict(grad_clip=dict(max_norm=35, norm_type=1))), 'norm_type'),
        (dict(optimizer_config=dict(grad_clip=None, cumulative_iters=4)), 'cumulative_iters'),
        (dict(fp16=dict(loss_scale=512., distributed=True)), 'distributed'),
        (dict(fp16=dict(loss_scale=dict(init_scale=8., growth_factor=1.0))), 'growth_factor'),
    ]
    for kw, word in bad:
        with pytest.raises(Gd4dError, match=word):
            _recipe(**kw)
    model = _Model()
    with pytest.raises(Gd4dError, match='align=4'):
        from graph_detr4d_amd import TrainRecipe
        TrainRecipe(D.FlatGradAllReducer(list(model.parameters())), model.named_parameters(), optimizer=OPTIMIZER)
    # host-only construction; the device step refuses CPU tensors like the rest of the package
    rec, _, _ = _recipe()
    with pytest.raises(Gd4dError, match='CPU'):
        rec.state()


def test_fp16_forms():
    none, _, _ = _recipe(fp16=None)
    assert (none.cfg.init_scale, none.cfg.dynamic_scale) == (1.0, 0)
    static, _, _ = _recipe()
    assert (static.cfg.init_scale, static.cfg.dynamic_scale) == (512.0, 0)
    dyn, _, _ = _recipe(fp16=dict(loss_scale='dynamic'))
    assert (dyn.cfg.init_scale, dyn.cfg.growth_factor, dyn.cfg.backoff_factor, dyn.cfg.growth_interval, dyn.cfg.dynamic_scale) == \
        (65536.0, 2.0, 0.5, 2000, 1)                                           # torch.amp.GradScaler's defaults
    args, _, _ = _recipe(fp16=dict(loss_scale=dict(init_scale=1024., growth_interval=3)))
    assert (args.cfg.init_scale, args.cfg.growth_interval, args.cfg.dynamic_scale) == (1024.0, 3, 1)


def test_entry_point_validates_before_any_gpu_work():
    """gd4d_adamw_recipe_flat: every bad call comes back with its error code on a box without a GPU (tests/test_abi.py's style)."""
    from graph_detr4d_amd import _lib
    from graph_detr4d_amd.recipe import RecipeRange
    lib = _lib.load()
    EINVAL, EALIGN, EWORKSPACE = -1, -3, -5
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 96)()
    ptr = ctypes.c_void_p((ctypes.addressof(buf) + 63) & ~63)
    odd, odd4 = ctypes.c_void_p(ptr.value + 4), ctypes.c_void_p(ptr.value + 2)
    rec, _, _ = _recipe()
    n = 64
    table = lambda *rows: (RecipeRange * len(rows))(*[RecipeRange(*r) for r in rows])     # noqa: E731
    good = table((0, 32, 1.0, 1.0), (32, 64, 0.1, 1.0))
    ws_bytes, st_bytes = lib.gd4d_adamw_recipe_flat_workspace_bytes(), lib.gd4d_adamw_recipe_flat_state_bytes()

    def call(p=ptr, g=ptr, m=ptr, v=ptr, st=ptr, stb=st_bytes, ws=ptr, wsb=ws_bytes, n=n, cfg=rec.cfg, ranges=good, dev=ptr, nr=None):
        return lib.gd4d_adamw_recipe_flat(p, g, m, v, st, stb, ws, wsb, n, ctypes.byref(cfg) if cfg is not None else null,
                                          ranges, dev, len(ranges) if nr is None and ranges is not None else (nr or 0), null)
    for name in ('p', 'g', 'm', 'v', 'st', 'ws', 'cfg', 'ranges', 'dev'):
        assert call(**{name: null if name not in ('cfg', 'ranges') else None}) == EINVAL, name
    assert call(n=0) == EINVAL
    for name in ('p', 'g', 'm', 'v'):
        assert call(**{name: odd}) == EALIGN, name                             # 16 bytes
    assert call(st=odd) == EALIGN and call(dev=odd) == EALIGN and call(ws=odd4) == EALIGN
    assert call(wsb=ws_bytes - 1) == EWORKSPACE and call(stb=st_bytes - 4) == EWORKSPACE
    many = table(*[(4 * i, 4 * i + 4, 1.0, 1.0) for i in range(1025)])
    assert call(ranges=many, n=4 * 1025) == EINVAL                             # more than 1024 ranges
    assert call(ranges=table(*[(4 * i, 4 * i + 4, 1.0, 1.0) for i in range(1024)]), n=4 * 1024, wsb=0) == EWORKSPACE   # 1024 are fine
    assert call(nr=0) == EINVAL
    assert call(ranges=table((32, 64, 1.0, 1.0), (0, 32, 1.0, 1.0))) == EINVAL             # unsorted
    assert call(ranges=table((0, 36, 1.0, 1.0), (32, 64, 1.0, 1.0))) == EINVAL             # overlapping
    assert call(ranges=table((0, 28, 1.0, 1.0), (32, 64, 1.0, 1.0))) == EINVAL             # a gap
    assert call(ranges=table((0, 30, 1.0, 1.0), (30, 64, 1.0, 1.0))) == EINVAL             # a quad in two groups
    assert call(ranges=table((0, 32, 1.0, 1.0), (32, 60, 1.0, 1.0))) == EINVAL             # short of n
    assert call(ranges=table((0, 32, -1.0, 1.0), (32, 64, 1.0, 1.0))) == EINVAL
    assert call(ranges=table((0, 32, 1.0, 1.0), (32, 62, 1.0, 1.0)), n=62, wsb=0) == EWORKSPACE    # n need not be a multiple of 4

    def cfg(**kw):
        c = type(rec.cfg).from_buffer_copy(rec.cfg)
        for k, val in kw.items():
            setattr(c, k, val)
        return c
    for kw in (dict(growth_factor=1.0), dict(growth_factor=0.5), dict(backoff_factor=0.0), dict(backoff_factor=1.0), dict(backoff_factor=1.5),
               dict(growth_interval=0), dict(init_scale=0.0), dict(init_scale=float('inf')), dict(policy=3), dict(policy=-1), dict(warmup=4),
               dict(iters_per_epoch=0), dict(max_epochs=0), dict(warmup_iters=-1), dict(warmup_ratio=0.0), dict(beta1=1.0), dict(beta2=-0.1),
               dict(eps=0.0), dict(weight_decay=-1.0), dict(base_lr=float('nan')), dict(policy=2, n_milestones=17),
               dict(policy=2, n_milestones=0, step_every=0)):
        assert call(cfg=cfg(**kw)) == EINVAL, kw
    assert call(cfg=cfg(), wsb=0) == EWORKSPACE                                # the copy itself is a valid configuration
