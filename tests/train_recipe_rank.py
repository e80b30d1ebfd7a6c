"""One rank of tests/test_train_recipe_gpu.py::test_two_ranks_take_the_same_decision (not a test module): two iterations of
scale -> backward -> all-reduce -> TrainRecipe.step over gloo, both ranks on the one GPU; rank 1's first input holds an inf.

    RANK=r WORLD_SIZE=2 MASTER_PORT=p python tests/train_recipe_rank.py OUT.json
"""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graph_detr4d_amd import TrainRecipe, dist as D  # noqa: E402


def digest(t):
    return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()


def main(out):
    torch.cuda.set_device(0)
    rank, world = D.init(backend='gloo', device='cuda:0')
    torch.manual_seed(0)                                                       # the same parameters on both ranks
    net = torch.nn.Sequential(torch.nn.Linear(64, 96), torch.nn.ReLU(), torch.nn.Linear(96, 32)).cuda()
    red = D.FlatGradAllReducer(list(net.parameters()), align=4)
    red.bind()
    rec = TrainRecipe(red, net.named_parameters(), optimizer=dict(type='AdamW', lr=1e-2, weight_decay=0.01),
                      optimizer_config=dict(grad_clip=dict(max_norm=35, norm_type=2)), lr_config=dict(policy='fixed'),
                      fp16=dict(loss_scale=512.))
    rec.state()
    res = dict(rank=rank, world=world, initial=digest(red.flat_params), steps=[])
    gen = torch.Generator().manual_seed(100 + rank)                            # every rank its own sample
    for it in range(2):
        x = torch.randn(16, 64, generator=gen)
        if it == 0 and rank == 1:
            x[3, 5] = float('inf')
        rec.scale(net(x.cuda()).square().sum()).backward()
        local_finite = bool(torch.isfinite(red.flat[:red.numel]).all())
        red.reduce()
        rec.step(zero_grads=True)
        torch.cuda.synchronize()
        res['steps'].append(dict(local_finite=local_finite, found_inf=int(rec.found_inf), skipped_steps=int(rec.skipped_steps),
                                 optimizer_steps=int(rec.optimizer_steps), iteration=int(rec.iteration), params=digest(red.flat_params),
                                 grads_zero=bool((red.flat[:red.numel] == 0).all())))
    with open(out, 'w') as f:
        json.dump(res, f)
    D.shutdown()


if __name__ == '__main__':
    main(sys.argv[1])
