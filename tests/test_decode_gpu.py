"""gd4d_nms_free_decode_fwd / gd4d_box_head_fwd (through NMSFreeCoder and functional.head_outputs) against the
reference-generated fixtures and the oracle.  GPU only."""
import pytest
import torch
import torch.nn as nn

from golden_io import Golden
from oracle import torch_oracle as O

pytestmark = pytest.mark.gpu

POST_RANGE = [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0]
PC_RANGE = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]


def _coder(**kw):
    from graph_detr4d_amd import build_bbox_coder
    cfg = dict(type='NMSFreeCoder', pc_range=PC_RANGE, post_center_range=POST_RANGE, max_num=300, num_classes=10)
    cfg.update(kw)
    return build_bbox_coder(cfg)


def _check(got, exp):
    assert got['bboxes'].shape == exp['bboxes'].shape
    assert got['labels'].dtype == torch.int64
    assert torch.equal(got['labels'].cpu(), exp['labels'])
    # expf / atan2f on the device differ from glibc's by an ulp or two
    torch.testing.assert_close(got['scores'].cpu(), exp['scores'], rtol=0, atol=2e-7)
    torch.testing.assert_close(got['bboxes'].cpu(), exp['bboxes'], rtol=2e-6, atol=2e-6)


@pytest.mark.parametrize('name', ['decode', 'decode_thr', 'decode_code8'])
def test_decode_matches_reference_fixture(name):
    g = Golden(name)
    m = g.meta
    coder = _coder(max_num=m['max_num'], score_threshold=m['score_threshold'], post_center_range=m['post_center_range'],
                   pc_range=m['pc_range'])
    preds = {'all_cls_scores': g.t('all_cls_scores').cuda(), 'all_bbox_preds': g.t('all_bbox_preds').cuda()}
    out = coder.decode(preds)
    assert len(out) == m['batch']
    for b, d in enumerate(out):
        _check(d, {k: g.t(f'{k}{b}') for k in ('bboxes', 'scores', 'labels')})
    single = coder.decode_single(preds['all_cls_scores'][-1, 0], preds['all_bbox_preds'][-1, 0])
    _check(single, {k: g.t(f'{k}0') for k in ('bboxes', 'scores', 'labels')})


@pytest.mark.parametrize('q,batch,k', [(900, 2, 300), (2700, 1, 300), (900, 1, 1024), (31, 3, 7)])
def test_decode_full_size_matches_oracle(q, batch, k):
    g = torch.Generator().manual_seed(q + k)
    cls = torch.randn(1, batch, q, 10, generator=g) * 2 - 2
    box = torch.randn(1, batch, q, 10, generator=g)
    box[..., 0:2] *= 40.
    box[..., 4] *= 6.
    out = _coder(max_num=k).decode({'all_cls_scores': cls.cuda(), 'all_bbox_preds': box.cuda()})
    exp = O.nms_free_decode({'all_cls_scores': cls, 'all_bbox_preds': box}, POST_RANGE, k, 10)
    for d, e in zip(out, exp):
        _check(d, e)
        s = d['scores']
        assert bool((s[:-1] >= s[1:]).all()), 'scores must come out sorted'


def test_decode_ties_take_lowest_indices():
    """All-equal and partially-equal scores: the K survivors are the lowest flat indices, in index order."""
    from graph_detr4d_amd import ops
    q, c, k = 64, 10, 100
    cls = torch.zeros(1, q, c)
    box = torch.zeros(1, q, 10)
    box[0, :, 8] = torch.arange(q).float()                       # vx carries the query index
    boxes, scores, labels, keep = ops.nms_free_decode_fwd(cls.cuda(), box.cuda(), POST_RANGE, k)
    idx = torch.arange(k)
    assert torch.equal(labels[0].cpu().long(), idx % c)
    assert torch.equal(boxes[0, :, 7].cpu().long(), idx // c)
    assert torch.equal(scores.cpu(), torch.full((1, k), 0.5))
    assert bool(keep.all())
    cls[0, 40:50, 3] = 1.0                                       # ten clear winners, then the tie
    boxes, scores, labels, keep = ops.nms_free_decode_fwd(cls.cuda(), box.cuda(), POST_RANGE, k)
    assert torch.equal(boxes[0, :10, 7].cpu().long(), torch.arange(40, 50))
    assert bool((labels[0, :10] == 3).all())
    rest = torch.tensor([i for i in range(q * c) if not (400 <= i < 500 and i % c == 3)][:k - 10])
    assert torch.equal(labels[0, 10:].cpu().long(), rest % c)
    assert torch.equal(boxes[0, 10:, 7].cpu().long(), rest // c)


def test_decode_errors():
    from graph_detr4d_amd import ops
    from graph_detr4d_amd._lib import Gd4dError
    cls, box = torch.zeros(1, 5, 10).cuda(), torch.zeros(1, 5, 10).cuda()
    with pytest.raises(RuntimeError, match='out of range'):       # torch.topk's message in the reference
        ops.nms_free_decode_fwd(cls, box, POST_RANGE, 300)
    big = torch.zeros(1, 900, 10).cuda()
    with pytest.raises(Gd4dError):
        ops.nms_free_decode_fwd(big, big, POST_RANGE, 2000)       # K > 1024 is not supported
    with pytest.raises(Gd4dError):
        ops.nms_free_decode_fwd(big, torch.zeros(1, 900, 9).cuda(), POST_RANGE, 300)
    with pytest.raises(Gd4dError):
        ops.nms_free_decode_fwd(cls.cpu(), box.cpu(), POST_RANGE, 3)
    with pytest.raises(NotImplementedError):
        _coder(post_center_range=None).decode_single(cls[0], box[0])


def _branches(num_layers, seed):
    torch.manual_seed(seed)

    def cls_branch():
        return nn.Sequential(nn.Linear(256, 256), nn.LayerNorm(256), nn.ReLU(inplace=True),
                             nn.Linear(256, 256), nn.LayerNorm(256), nn.ReLU(inplace=True), nn.Linear(256, 10))

    def reg_branch():
        return nn.Sequential(nn.Linear(256, 256), nn.ReLU(), nn.Linear(256, 256), nn.ReLU(), nn.Linear(256, 10))
    return (nn.ModuleList(cls_branch() for _ in range(num_layers)),
            nn.ModuleList(reg_branch() for _ in range(num_layers)))


@pytest.mark.parametrize('q,batch,depth_factor', [(900, 1, None), (64, 2, 1.25)])
def test_head_outputs_match_oracle(q, batch, depth_factor):
    """cls / reg branches (detr3d_head_pe.py:368-388 shapes) + box epilogue for every decoder layer, then decode."""
    from graph_detr4d_amd import functional as Fn
    nl = 3
    cls_b, reg_b = _branches(nl, 7)
    g = torch.Generator().manual_seed(11)
    hs = torch.randn(nl, q, batch, 256, generator=g)
    init_ref = torch.rand(batch, q, 3, generator=g)
    init_ref[0, 0] = torch.tensor([0., 1., 0.5])                    # the inverse_sigmoid clamps
    inter = torch.rand(nl, batch, q, 3, generator=g)
    with torch.no_grad():
        exp_cls, exp_box = [], []
        for lvl in range(nl):
            x = hs[lvl].permute(1, 0, 2)
            ref = init_ref if lvl == 0 else inter[lvl - 1]
            exp_cls.append(cls_b[lvl](x))
            exp_box.append(O.box_head(reg_b[lvl](x), ref, PC_RANGE, depth_factor))
        exp = {'all_cls_scores': torch.stack(exp_cls), 'all_bbox_preds': torch.stack(exp_box)}
        cls_b.cuda(), reg_b.cuda()
        got = Fn.head_outputs(hs.cuda(), init_ref.cuda(), inter.cuda(), cls_b, reg_b, PC_RANGE, depth_factor)
    assert got['enc_cls_scores'] is None and got['enc_bbox_preds'] is None
    torch.testing.assert_close(got['all_cls_scores'].cpu(), exp['all_cls_scores'], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(got['all_bbox_preds'].cpu(), exp['all_bbox_preds'], rtol=1e-4, atol=1e-4)
    # decoding the device-side head outputs reproduces the oracle's decode of the same tensors
    preds = {k: got[k] for k in ('all_cls_scores', 'all_bbox_preds')}
    dec = _coder(max_num=100).decode(preds)
    ref_dec = O.nms_free_decode({k: v.cpu() for k, v in preds.items()}, POST_RANGE, 100, 10)
    for d, e in zip(dec, ref_dec):
        _check(d, e)


# ---------------------------------------------------------------------------------------------------------------------
# Exact top-k at the kernel's edges.  The logits come from a ladder of multiples of 0.5 in [-6, 6] with many repeats:
# two different steps differ in score by >= 1.2e-3 (sigmoid'(6) * 0.5), far above an ulp of expf, and equal logits are
# true ties - so the expected SELECTION is topk_stable(logits) whatever the device's expf rounds to.  Box column 8 (vx)
# carries the query index, exact in fp32.
# ---------------------------------------------------------------------------------------------------------------------
def _ladder(gen, *shape):
    return torch.randint(0, 25, shape, generator=gen).float() * 0.5 - 6.0


def _index_boxes(b, q):
    box = torch.zeros(b, q, 10)
    box[:, :, 8] = torch.arange(q).float()
    return box


def _check_selection(cls, k, order_key=None, score_threshold=None):
    """Run the kernel on cls (B, Q, C); per sample compare labels / query indices (exactly) and scores (fp32 sigmoid, atol 2e-7)
    with topk_stable over order_key (default: the logits).  Returns the device outputs."""
    from graph_detr4d_amd import ops
    from selection_ref import topk_stable
    b, q, c = cls.shape
    boxes, scores, labels, keep = ops.nms_free_decode_fwd(cls.cuda(), _index_boxes(b, q).cuda(), POST_RANGE, k, score_threshold)
    boxes, scores, labels, keep = boxes.cpu(), scores.cpu(), labels.cpu(), keep.cpu()
    assert boxes.shape == (b, k, 9) and scores.shape == labels.shape == keep.shape == (b, k)
    key = cls if order_key is None else order_key
    for s in range(b):
        idx = torch.from_numpy(topk_stable(key[s].reshape(-1).numpy(), k))
        assert torch.equal(labels[s].long(), idx % c), f'sample {s}: labels'
        assert torch.equal(boxes[s, :, 7].long(), idx // c), f'sample {s}: query indices'
        torch.testing.assert_close(scores[s], cls[s].reshape(-1)[idx].sigmoid(), rtol=0, atol=2e-7)
        assert bool((scores[s, :-1] >= scores[s, 1:]).all()), 'scores must come out sorted'
    return boxes, scores, labels, keep


@pytest.mark.parametrize('b,q,c,k', [
    (1, 901, 10, 300),         # Q*C % 4 != 0: the scalar load path, nine trips of its loop
    (1, 1023, 3, 1024),        # odd n, K = DEC_KMAX
    (2, 100, 10, 1000),        # K = n
    (1, 33, 7, 231),           # K = n, n odd
    (1, 900, 10, 1),           # K = 1
    (3, 2048, 16, 1024),       # n = 32768: the LDS limit, a 32-element chunk per thread in the tie path
])
def test_decode_exact_topk_on_a_ladder(b, q, c, k):
    g = torch.Generator().manual_seed(1000 * q + k)
    cls = _ladder(g, b, q, c)
    if b == 3:                                     # each sample drawn differently: a narrow ladder, a shifted one
        cls[1] = torch.randint(0, 3, (q, c), generator=g).float() * 0.5
        cls[2] = (cls[2] - 3.0).clamp(min=-6.0)
    _check_selection(cls, k)


def test_decode_above_the_lds_limit_raises():
    from graph_detr4d_amd import ops
    from graph_detr4d_amd._lib import Gd4dError
    cls = torch.zeros(1, 2049, 16).cuda()
    with pytest.raises(Gd4dError):
        ops.nms_free_decode_fwd(cls, _index_boxes(1, 2049).cuda(), POST_RANGE, 300)


@pytest.mark.parametrize('size,take', [(5000, 1), (5000, 33), (5000, 1024), (1001, 1000)])
def test_decode_tie_class_straddles_chunks_and_waves(size, take):
    """n = 32768: every thread of the tie path owns 32 consecutive elements.  One tie class of `size` elements (logit 2.0) is
    scattered over the whole range, K - take elements lie above it, everything else below: the kernel must take exactly the
    `take` lowest-index members of the class.  take = size - 1 needs size <= K + 1 = 1025 (K <= DEC_KMAX), hence the second,
    smaller class; with the class of 5000 the third case takes all K survivors from the class instead."""
    q, c, k = 2048, 16, 1024
    n = q * c
    g = torch.Generator().manual_seed(size + take)
    perm = torch.randperm(n, generator=g)
    cls = torch.randint(0, 16, (n,), generator=g).float() * 0.5 - 6.0             # -6 .. 1.5: below the class
    cls[perm[:size]] = 2.0
    above = perm[size:size + k - take]
    cls[above] = torch.randint(5, 13, (above.numel(),), generator=g).float() * 0.5  # 2.5 .. 6: above it
    assert int((cls == 2.0).sum()) == size and int((cls > 2.0).sum()) == k - take
    _, _, labels, _ = _check_selection(cls.view(1, q, c), k)
    members = torch.sort(perm[:size]).values
    # the last wave, the last thread and the first thread all hold members: the class spans every chunk boundary
    assert int(members[0]) < 1024 and int(members[-1]) >= n - 1024


def test_decode_saturated_high_scores_tie_at_one():
    """Logits >= 20 give a score of exactly 1.0 (1 + exp(-20) rounds to 1): 500 of them, drawn from {20, 25, 30, 50}, are ONE tie
    class although their logits differ.  K = 300 < 500: the winners are the 300 lowest indices among them."""
    q, c, k = 900, 10, 300
    g = torch.Generator().manual_seed(21)
    cls = _ladder(g, 1, q, c)
    pos = torch.randperm(q * c, generator=g)[:500]
    cls.view(-1)[pos] = torch.tensor([20., 25., 30., 50.])[torch.randint(0, 4, (500,), generator=g)]
    _, scores, labels, _ = _check_selection(cls, k, order_key=cls.clamp(max=20.0))
    assert torch.equal(scores, torch.ones(1, k))
    assert torch.equal(labels[0].long(), torch.sort(pos).values[:k] % c)


def test_decode_saturated_low_scores_threshold_key_zero():
    """All but K / 2 logits <= -110: exp(110) overflows fp32, the score is exactly 0.0 and the K-th largest key is 0.  The 150
    finite-score elements come first, the rest are the lowest indices of the zero class at score exactly 0.0."""
    q, c, k = 900, 10, 300
    g = torch.Generator().manual_seed(22)
    cls = torch.tensor([-110., -120., -200., -1e4])[torch.randint(0, 4, (1, q, c), generator=g)]
    pos = torch.randperm(q * c, generator=g)[:k // 2]
    cls.view(-1)[pos] = _ladder(g, k // 2)
    _, scores, labels, _ = _check_selection(cls, k, order_key=cls.clamp(min=-110.0))
    assert bool((scores[0, :k // 2] > 0).all()) and torch.equal(scores[0, k // 2:], torch.zeros(k // 2))
    zeros = torch.tensor([i for i in range(q * c) if i not in set(pos.tolist())][:k // 2])
    assert torch.equal(labels[0, k // 2:].long(), zeros % c)


def test_decode_keep_borders_are_inclusive_and_threshold_is_strict():
    """keep at the kernel boundary: a centre exactly on post_center_range's lo or hi is kept (the reference tests >= / <=), one
    fp32 step outside is dropped, on every axis; score_threshold is a strict >: a score of exactly 0.5 (logit 0) is not kept at
    0.5, is kept at None."""
    import numpy as np
    from graph_detr4d_amd import ops
    rng = np.float32(POST_RANGE)
    rows = []                                                        # (cx, cy, cz, expected keep)
    for axis in range(3):
        for side, away in ((0, -np.inf), (3, np.inf)):
            on = rng[axis + side]
            for v, ok in ((on, True), (np.nextafter(on, np.float32(away)), False)):
                ctr = [0.0, 0.0, 0.0]
                ctr[axis] = v
                rows.append((*ctr, ok))
    rows.append((0.0, 0.0, 0.0, True))
    rows.append((rng[0], rng[4], rng[2], True))                      # three borders at once
    q = len(rows)
    box = _index_boxes(1, q)
    t = torch.tensor([r[:3] for r in rows], dtype=torch.float32)
    box[0, :, 0], box[0, :, 1], box[0, :, 4] = t[:, 0], t[:, 1], t[:, 2]
    want = torch.tensor([r[3] for r in rows])
    cls = torch.full((1, q, 1), 1.0)                                 # score 0.73 everywhere
    boxes, scores, labels, keep = ops.nms_free_decode_fwd(cls.cuda(), box.cuda(), POST_RANGE, q)
    qi = boxes[0, :, 7].cpu().long()
    assert torch.equal(qi, torch.arange(q))                          # all tied: index order
    assert torch.equal(boxes[0, :, :3].cpu(), t)                     # centres pass through bit for bit
    assert torch.equal(keep[0].cpu(), want), [r for r, k_ in zip(rows, keep[0].tolist()) if k_ != r[3]]
    assert int(want.sum()) == 8 and int((~want).sum()) == 6
    # the threshold: logits 0.5, 0 (score exactly 0.5), -0.5 per query, every centre inside
    cls = torch.tensor([0.5, 0.0, -0.5]).repeat(4, 1).view(1, 4, 3)
    inside = _index_boxes(1, 4).cuda()
    _, scores, labels, keep = ops.nms_free_decode_fwd(cls.cuda(), inside, POST_RANGE, 12, 0.5)
    assert torch.equal(scores[0, 4:8].cpu(), torch.full((4,), 0.5)) and bool((labels[0, 4:8] == 1).all())
    assert torch.equal(keep[0].cpu(), torch.tensor([True] * 4 + [False] * 8))
    _, _, _, keep = ops.nms_free_decode_fwd(cls.cuda(), inside, POST_RANGE, 12, None)
    assert bool(keep.all())
    # just under the score: kept
    _, _, _, keep = ops.nms_free_decode_fwd(cls.cuda(), inside, POST_RANGE, 12, float(np.nextafter(np.float32(0.5), np.float32(0))))
    assert torch.equal(keep[0].cpu(), torch.tensor([True] * 8 + [False] * 4))


# ---------------------------------------------------------------------------------------------------------------------
# gd4d_box_head_fwd directly against the reference formula in fp64
# ---------------------------------------------------------------------------------------------------------------------
_BOX_HEAD_M = 900


def _box_head_inputs(code):
    g = torch.Generator().manual_seed(300 + code)
    tmp = torch.randn(_BOX_HEAD_M, code, generator=g) * 2.0
    ref = torch.rand(_BOX_HEAD_M, 3, generator=g)
    ref[0] = torch.tensor([0., 1., 0.5])                             # the inverse-sigmoid clamps (row 0: also the M = 1 case)
    ref[7] = torch.tensor([1., 0., 0.])
    ref[254] = torch.tensor([0.5, 0.5, 1.])
    ref[256] = torch.tensor([1e-6, 1. - 1e-6, 0.5])                  # inside the eps clamp
    ref[899] = torch.tensor([1., 1., 1.])
    return tmp, ref


@pytest.fixture(scope='module')
def box_head_reference():
    """Per (code, scale): the inputs, the fp64 evaluation of the reference formula and the largest error of the SAME formula in
    fp32 on the CPU (oracle.torch_oracle.box_head) on these inputs - computed once, shared by every M."""
    out = {}
    for code in (8, 10):
        tmp, ref = _box_head_inputs(code)
        for scale in (1.0, 1.25):
            df = None if scale == 1.0 else scale
            want = O.box_head(tmp.double(), ref.double(), PC_RANGE, df)
            err32 = float((O.box_head(tmp, ref, PC_RANGE, df).double() - want).abs().max())
            out[code, scale] = (tmp, ref, want, err32)
    return out


@pytest.mark.parametrize('m', [1, 255, 257, 900])
@pytest.mark.parametrize('scale', [1.0, 1.25])
@pytest.mark.parametrize('code', [8, 10])
def test_box_head_fwd_matches_fp64_formula(box_head_reference, code, scale, m):
    from graph_detr4d_amd import ops
    tmp, ref, want, err32 = box_head_reference[code, scale]
    got = ops.box_head_fwd(tmp[:m].contiguous().cuda(), ref[:m].contiguous().cuda(), PC_RANGE, scale).cpu()
    assert got.shape == (m, code)
    passthrough = [c for c in range(code) if c not in (0, 1, 4)]
    assert torch.equal(got[:, passthrough], tmp[:m][:, passthrough])
    err = float((got.double() - want[:m]).abs().max())
    # 4 x the fp32 oracle's own largest error on these 900 rows (the factor: device expf / logf against glibc's, an ulp or two).
    # Measured |fp32 oracle - fp64| (code, scale): (8, 1) 1.16e-5, (8, 1.25) 1.35e-5, (10, 1) 1.24e-5, (10, 1.25) 1.45e-5 - about
    # two ulps of a centre near 50 m; so the device is allowed 4.6e-5 .. 5.8e-5.
    # Measured |device - fp64| on the MI355X, largest over M: 1.26e-5, 1.67e-5, 1.50e-5, 1.88e-5 (docs/measurements_r14.md).
    assert err <= 4.0 * err32
