"""The pyramid feature-distillation loss (MixDistill.get_feat_distill_loss, distillation/distillers/mix_distill.py:118-138) restated
in fp64, formula by formula, with its gradients written out (no autograd): the reference for gd4d_feat_distill.hip.

Per level, with R = B * N cameras, C = 256 channels, P = H * W pixels, x / t the student's / teacher's (R, C, P) maps:
    s = W x + b                                                      lateral_convs[l], a 1x1 convolution with bias
    vanilla:    loss_l = mean((s - t)^2)
    attention:  g_c[r, p] = mean_c |t|,  a_c = C softmax_p(g_c / T);  g_s[r, c] = mean_p |t|,  a_s = P softmax_c(g_s / T);  T = 0.5
                loss_l = mean(a_c a_s (t - s)^2)                     both maps from the TEACHER
    loss = loss_weight * sum_l loss_l / levels
    G = d loss / d s = 2 coef a (s - t),  coef = loss_weight / (levels R C P),  a = a_c a_s (1 for vanilla)
    d x = W^T G,  d W = sum_{r, p} G x^T,  d b = sum_{r, p} G
tests/test_feat_distill_cpu.py pins these functions to vectors captured from the reference itself."""
import numpy as np

TEMPERATURE = 0.5


def _softmax(x, axis):
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def attention_maps(t):
    """t (R, C, P) -> a_c (R, 1, P), a_s (R, C, 1), fp64."""
    t = np.asarray(t, dtype=np.float64)
    _, c, p = t.shape
    a_c = c * _softmax(np.abs(t).mean(axis=1, keepdims=True) / TEMPERATURE, axis=2)
    a_s = p * _softmax(np.abs(t).mean(axis=2, keepdims=True) / TEMPERATURE, axis=1)
    return a_c, a_s


def feat_distill_ref(teacher, student, weights, biases, kind, loss_weight):
    """teacher / student: lists of (..., C, H, W) arrays (leading dimensions are flattened to cameras); weights[l] (C, C) or (C, C, 1, 1),
    biases[l] (C).  Returns (loss, [d student_l, shaped like student_l], [d W_l (C, C)], [d b_l (C)]), all fp64."""
    if kind not in ('vanilla', 'attention'):
        raise ValueError(kind)
    nl = len(teacher)
    loss, gx, gw, gb = 0.0, [], [], []
    for l in range(nl):
        shape = np.asarray(student[l]).shape
        c = shape[-3]
        x = np.asarray(student[l], dtype=np.float64).reshape(-1, c, shape[-2] * shape[-1])
        t = np.asarray(teacher[l], dtype=np.float64).reshape(x.shape)
        w = np.asarray(weights[l], dtype=np.float64).reshape(c, c)
        b = np.asarray(biases[l], dtype=np.float64).reshape(c)
        s = np.einsum('oc,rcp->rop', w, x) + b[None, :, None]
        a = 1.0
        if kind == 'attention':
            a_c, a_s = attention_maps(t)
            a = a_c * a_s
        d = s - t
        loss += float((a * d * d).mean())
        g = 2.0 * (loss_weight / (nl * d.size)) * a * d
        gx.append(np.einsum('oc,rop->rcp', w, g).reshape(shape))
        gw.append(np.einsum('rop,rcp->oc', g, x))
        gb.append(g.sum(axis=(0, 2)))
    return loss_weight * loss / nl, gx, gw, gb
