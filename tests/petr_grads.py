"""What the training tests of PETR's transformer share: the gradients of a run in the form tests/golden/petr_transformer_grads.npz
holds them, and their distance from it.

The fixture's loss is (out_dec * G).sum().  It records grad.x, grad.pos_embed, grad.query_embed, grad.<key> for every bias and
LayerNorm parameter, and rowsum.<key> / colsum.<key> (the gradient summed over dim 1 / dim 0) for every weight matrix."""
import torch


def as_fixture(x, pos_embed, query_embed, named_grads):
    """named_grads: (state-dict key, gradient) pairs.  -> {fixture key: tensor}"""
    out = {'grad.x': x.grad, 'grad.pos_embed': pos_embed.grad, 'grad.query_embed': query_embed.grad}
    for name, g in named_grads:
        if g.dim() == 1:
            out['grad.' + name] = g
        else:
            out['rowsum.' + name] = g.sum(1)
            out['colsum.' + name] = g.sum(0)
    return out


def errors(got, fixture):
    """{key: (max |got - fixture|, max |fixture|)} over every array of the fixture but G; every key must be there."""
    keys = [k for k in fixture.arrays if k != 'G']
    assert sorted(keys) == sorted(got), sorted(set(keys) ^ set(got))
    res = {}
    for k in keys:
        ref = fixture.t(k).double()
        g = got[k].detach().double().cpu()
        assert g.shape == ref.shape and torch.isfinite(g).all(), k
        res[k] = (float((g - ref).abs().max()), float(ref.abs().max()))
    return res


def worst_relative(errs):
    """max over tensors of max-error / max(1, scale), and the key it belongs to"""
    key = max(errs, key=lambda k: errs[k][0] / max(1.0, errs[k][1]))
    return errs[key][0] / max(1.0, errs[key][1]), key


def table(errs, head='max error (scale)'):
    rows = [f'  {k:58s} {e:.2e} ({s:.2e})' for k, (e, s) in sorted(errs.items())]
    return head + '\n' + '\n'.join(rows)
