"""Host-side helpers shared by the attention modules (GPU only; no CPU fallback)."""
import numpy as np

import torch

from . import _lib, ops, switches


def wants_grad(module, *tensors):
    """True when autograd must see this call: grad mode on and a parameter or input requires grad."""
    if not torch.is_grad_enabled():
        return False
    if any(t is not None and torch.is_tensor(t) and t.requires_grad for t in tensors):
        return True
    return module is not None and any(p.requires_grad for p in module.parameters())


def require_inference(*tensors):
    """Forward-only entry points: refuse silently-wrong autograd use."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise NotImplementedError(
            'graph-detr4d_amd: this entry point has no backward - call it under torch.no_grad()')


def main_grad(t, rows=None):
    """Where the gradient of parameter `t` is accumulated when a dist.FlatGradAllReducer was bound with
    fuse_weight_grads=True (its view of the flat buffer), else None.  rows=(lo, hi): the same for the row slice t[lo:hi]
    (the thirds of a packed in-projection)."""
    m = getattr(t, '_gd4d_main_grad', None) if t is not None else None
    if m is None or rows is None:
        return m
    return m[rows[0]:rows[1]]


def linear_autograd(x, weight, bias=None, main=None, relu=False):
    """F.linear [+ ReLU] with autograd (training path); on the GPU in fp32 the weight gradient runs on gd4d_linear_bwd_weight.
    main = (weight gradient buffer, bias gradient buffer): see main_grad(); default: the parameters' own."""
    if x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32:
        from .autograd import LinearFunction
        if main is None:
            main = (main_grad(weight), main_grad(bias))
        if main[0] is None or (bias is not None and main[1] is None) or not torch.is_grad_enabled():
            main = (None, None)
        # 2-D inside the Function: its output must not be a view (in-place ReLUs follow in the nn.Sequential stacks)
        y = LinearFunction.apply(x.reshape(-1, x.shape[-1]), weight, bias, main[0], main[1], relu)
        return y.view(*x.shape[:-1], weight.shape[0])
    y = torch.nn.functional.linear(x, weight, bias)
    return torch.relu(y) if relu else y


def linear_group_autograd(x, x2, linears):
    """[lin(x + x2) for lin in linears] (nn.Linear modules, at most 4) with autograd as ONE node and one forward launch
    (autograd.LinearGroupFunction); x, x2 (..., K).  Returns a list of (..., N_g)."""
    from .autograd import LinearGroupFunction
    ws = [m.weight for m in linears]
    bs = [m.bias for m in linears]
    mains = [(main_grad(m.weight), main_grad(m.bias)) for m in linears]
    mains = [(mw, mb) if mw is not None and (m.bias is None or mb is not None) and torch.is_grad_enabled() else (None, None)
             for (mw, mb), m in zip(mains, linears)]
    outs = LinearGroupFunction.apply(x, x2, len(linears), *ws, *bs, *[m[0] for m in mains], *[m[1] for m in mains])
    return [o.view(*x.shape[:-1], w.shape[0]) for o, w in zip(outs, ws)]


def can_group_linears(x, x2, linears):
    return (x2 is not None and x.is_cuda and x.dtype == torch.float32 and x2.dtype == torch.float32 and x2.shape == x.shape
            and x.shape[-1] % 4 == 0 and 0 < len(linears) <= 4
            and all(isinstance(m, torch.nn.Linear) and m.weight.dtype == torch.float32 for m in linears))


def layer_norm_autograd(x, norm, relu=False, res=None):
    """nn.LayerNorm `norm` of x [+ res] [+ ReLU] with autograd on the HIP kernels (gd4d_layernorm_fwd / _bwd); anything
    they do not cover (CPU, other dtypes, no affine parameters, > 1024 channels) goes to the module."""
    c = x.shape[-1]
    if x.is_cuda and x.dtype == torch.float32 and norm.weight is not None and norm.bias is not None \
            and tuple(norm.normalized_shape) == (c,) and c % 4 == 0 and c <= 1024 \
            and (res is None or (res.shape == x.shape and res.dtype == x.dtype)):
        from .autograd import LayerNormFunction
        mg, mb = main_grad(norm.weight), main_grad(norm.bias)
        if mg is None or mb is None:
            mg = mb = None
        return LayerNormFunction.apply(x, norm.weight, norm.bias, norm.eps, relu, mg, mb, res)
    y = norm(x if res is None else x + res)
    return torch.relu(y) if relu else y


def residual_norm_autograd(kwargs, identity, out):
    """identity + out, or - when the layer offered the LayerNorm that follows (take_fused_norm) - that LayerNorm of the sum
    with the sum formed inside the kernel (training path: one launch instead of two, no stored sum)."""
    fused = take_fused_norm(kwargs, autograd=True)
    if fused is not None and out.is_cuda and out.shape == identity.shape:
        fused['done'] = True
        return layer_norm_autograd(identity, fused['norm'], res=out)
    return identity + out


def sequential_autograd(module, x):
    """Run an nn.Sequential / nn.Linear / nn.LayerNorm / any module with autograd: nn.Linear layers (with the ReLU that
    follows, if any) through linear_autograd, nn.LayerNorm (with its ReLU, if any) through layer_norm_autograd."""
    if isinstance(module, torch.nn.Linear):
        return linear_autograd(x, module.weight, module.bias)
    if isinstance(module, torch.nn.LayerNorm):
        return layer_norm_autograd(x, module)
    if isinstance(module, torch.nn.Sequential):
        mods = list(module)
        i = 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, torch.nn.LayerNorm) and i + 1 < len(mods) and isinstance(mods[i + 1], torch.nn.ReLU):
                x = layer_norm_autograd(x, m, relu=True)
                i += 2
                continue
            if isinstance(m, torch.nn.Linear) and i + 1 < len(mods) and isinstance(mods[i + 1], torch.nn.ReLU):
                x = linear_autograd(x, m.weight, m.bias, relu=True)       # (the pre-activation has no other reader)
                i += 2
                continue
            x = sequential_autograd(m, x)
            i += 1
        return x
    return module(x)


def torch_ops_route(what, supported, module=None):
    """Whether `what` runs through differentiable torch ops instead of the library's kernels.  There is no silent detour: shapes
    the kernels cover run on them unless the torch-op route was CHOSEN - per module (`module.torch_ops = True`, the constructor
    keyword `torch_ops=True` where a module has one, or `with Fn.torch_ops_for(module):`) or for the whole process
    (GD4D_TORCH_OPS=1, which the tests compare against); shapes they do not cover raise, naming the switches."""
    if switches.flag('GD4D_TORCH_OPS') or (module is not None and getattr(module, 'torch_ops', False)):
        return True
    if supported:
        return False
    raise _lib.Gd4dError(f'{what}: outside the limits of graph-detr4d_amd\'s kernels.  `module.torch_ops = True` (or GD4D_TORCH_OPS=1 for '
                         'every module of the process) runs it through differentiable torch ops instead (slower; an explicit choice, '
                         'not a fallback).')


class torch_ops_for:
    """`with Fn.torch_ops_for(m1, m2):` - these modules take their torch-op routes inside the block (torch_ops_route)."""

    def __init__(self, *modules):
        self.modules, self.prev = modules, None

    def __enter__(self):
        self.prev = [getattr(m, 'torch_ops', False) for m in self.modules]
        for m in self.modules:
            m.torch_ops = True

    def __exit__(self, *exc):
        for m, v in zip(self.modules, self.prev):
            m.torch_ops = v


def pad_points(offsets, attn_logits, supported, what):
    """offsets (B, Q, Hh, P, 3), attn_logits (B, Q, Hh, L, P) with any P <= max(supported) -> the same tensors padded along the
    point axis to the next count in `supported` (the kernels are compiled for 1 / 2 / 4 / 8 points per head; the reference's
    constructor default is 5, deform3d_cross_attn.py:56).  A padded point gets a NaN offset - its projection then fails every
    comparison of the visibility test (deform3d_cross_attn.py:239, :249-252), so it is never visible, never gathered, and its
    mask entries are 0 - and a -inf logit: its softmax weight is exactly 0 and the real points' weights are those of the
    softmax over L x P.  Differentiable (the gradients of the padding are dropped by the slice autograd makes of F.pad)."""
    p = offsets.shape[3]
    tgt = next((s_ for s_ in sorted(supported) if s_ >= p), None)
    if tgt is None:
        raise _lib.Gd4dError(f'{what}: num_points = {p}, the kernels take up to {max(supported)} points per head')
    if tgt == p:
        return offsets, attn_logits
    pad = tgt - p
    return (torch.nn.functional.pad(offsets, (0, 0, 0, pad), value=float('nan')).contiguous(),
            torch.nn.functional.pad(attn_logits, (0, pad), value=float('-inf')).contiguous())


def require_gpu(t, name):
    if not t.is_cuda:
        raise _lib.Gd4dError(f'{name} is on {t.device}: graph-detr4d_amd runs on the GPU only '
                             '(no CPU fallback)')


def folded_batchnorm(bn, bias=None):
    """(2, C): scale = gamma / sqrt(var + eps) and shift = beta + (bias - mean) scale of an eval()-mode BatchNorm2d behind a
    convolution's bias (None: no bias), in fp32."""
    var, mean = bn.running_var.detach().float(), bn.running_mean.detach().float()
    scale = torch.rsqrt(var + bn.eps)
    if bn.weight is not None:
        scale = scale * bn.weight.detach().float()
    shift = -mean if bias is None else bias.detach().float() - mean
    shift = shift * scale
    if bn.bias is not None:
        shift = shift + bn.bias.detach().float()
    return torch.stack((scale, shift)).contiguous()


def inverse_sigmoid(x, eps=1e-5):
    """Reference: deform3d_cross_attn.py:16-31 / detr3d_transformer.py:28-43."""
    x = x.clamp(min=0, max=1)
    return torch.log(x.clamp(min=eps, max=1) / (1 - x).clamp(min=eps, max=1))


_L2I_BUFFERS = {}          # (device index, request slot | stream, shape) -> [host copy, persistent device tensor]
_REQUEST_SLOT = [None]     # None: no request_slot() active - the buffers are kept per HIP stream


class request_slot:
    """Context manager for callers that keep several samples in flight on different streams (bench.py --inflight): the
    per-sample persistent device buffers (the lidar2img matrices) are kept per slot, so that refreshing one request's
    matrices cannot change what another request's queued kernels read."""

    def __init__(self, slot):
        self.slot, self.prev = int(slot), None

    def __enter__(self):
        self.prev, _REQUEST_SLOT[0] = _REQUEST_SLOT[0], self.slot

    def __exit__(self, *exc):
        _REQUEST_SLOT[0] = self.prev



def slot_key(device):
    """What per-request persistent device buffers are keyed by: the active request_slot(), else the current stream."""
    return _REQUEST_SLOT[0] if _REQUEST_SLOT[0] is not None else ('stream', torch.cuda.current_stream(device).cuda_stream)


def lidar2img_device(img_metas, like):
    """(B, N, 4, 4) fp32 device tensor from img_metas[*]['lidar2img'].

    The reference re-uploads it in every layer (deform3d_cross_attn.py:215-219, a host->device
    copy x6 per sample).  Here ONE persistent device buffer per (device, request slot, shape) is kept and refreshed IN PLACE
    when the host values change (compared every call, so in-place edits by augmentations are seen): a hipGraph
    captured over the decoder keeps a valid address, and replaying it for a new sample only needs this function
    (or the decoder) to be called once outside the graph to refresh the buffer.  A refresh cannot be recorded into
    a capture (it is a host->device copy of host data that changes per sample), so a cache miss while the stream
    is capturing raises instead of baking stale matrices into the graph.
    """
    host = np.ascontiguousarray(np.asarray([m['lidar2img'] for m in img_metas]), dtype=np.float32)
    capturing = torch.cuda.is_current_stream_capturing()
    # without an explicit request_slot() the buffers are per stream: concurrent streams cannot alias each other's matrices
    slot = _REQUEST_SLOT[0] if _REQUEST_SLOT[0] is not None else ('stream', torch.cuda.current_stream(like.device).cuda_stream)
    key = (like.device.index, slot, host.shape)
    entry = _L2I_BUFFERS.get(key)
    if entry is None or not np.array_equal(entry[0], host):
        if capturing:
            # a capture runs on its own stream: bake in the buffer an eager call (on whichever stream) filled with these very
            # matrices - the one a later eager call with new metas on that stream refreshes before the next replay
            entry = None
            for (dev_i, _, shape), other in _L2I_BUFFERS.items():
                if dev_i == like.device.index and shape == host.shape and np.array_equal(other[0], host):
                    entry = other
                    break
            if entry is None:
                raise RuntimeError('graph-detr4d_amd: img_metas[*][\'lidar2img\'] changed (or was never uploaded) while a '
                                   'hipGraph is being captured; call the module once eagerly with these metas first')
        else:
            src = torch.from_numpy(host)
            if entry is None:
                entry = _L2I_BUFFERS[key] = [host.copy(), src.to(like.device)]
            else:
                entry[1].copy_(src)
                entry[0] = host.copy()
    if torch.is_grad_enabled() and not capturing:
        # autograd saves this tensor (CrossAttnFunction, matmul): an in-place refresh of the persistent buffer by a second
        # forward before the first backward (losses summed over samples, a student pass with other metas) would trip the
        # saved-tensor version check - hand out a private copy (1.5 KB device-to-device).  Under capture the persistent
        # buffer itself is what a replay needs.
        return entry[1].clone()
    return entry[1]


def img_hw(img_metas):
    """Un-padded (H, W) of camera 0 of sample 0 - the reference's normaliser (:242-243)."""
    shp = img_metas[0]['img_shape'][0]
    return float(shp[0]), float(shp[1])


def linear(x, weight, bias=None, **kw):
    """Dense layer on the last dim via gd4d_linear_fwd (fp32 MFMA).  Keywords: x2 / n_split (input
    addend for the first output columns), relu, r1 / r2 (residuals), inv_sigmoid_in."""
    return ops.linear_fwd(x.contiguous(), weight.contiguous(), None if bias is None else bias.contiguous(),
                          **{k: (v.contiguous() if torch.is_tensor(v) else v) for k, v in kw.items()})


def layer_norm(x, norm, res=None, relu=False):
    """nn.LayerNorm module `norm` applied through gd4d_layernorm_fwd (optionally LN(x + res), ReLU)."""
    return ops.layernorm_fwd(x.contiguous(), norm.weight.contiguous(), norm.bias.contiguous(), norm.eps,
                             res=None if res is None else res.contiguous(), relu=relu)


NORM_KEY = '_gd4d_fused_norm'


def rowblock_ok(x, weight, norm=None):
    """gd4d_linear_ln_fwd limits: K % 64 == 0; with a LayerNorm at most 256 output columns."""
    return x.is_cuda and x.shape[-1] % 64 == 0 and \
        (norm is None or (weight.shape[0] <= 256 and tuple(norm.normalized_shape) == (weight.shape[0],)))


def linear_norm(x, weight, bias, norm, r1=None, r2=None, relu_after=False):
    """LN(x W^T + b + r1 + r2) [ReLU]: one launch (ops.linear_ln_fwd) when the shapes allow, else Linear + LayerNorm."""
    c = lambda t: None if t is None else t.contiguous()
    if rowblock_ok(x, weight, norm):
        return ops.linear_ln_fwd(x.contiguous(), weight.contiguous(), c(bias), norm.weight.contiguous(),
                                 norm.bias.contiguous(), norm.eps, r1=c(r1), r2=c(r2), relu_after_ln=relu_after)
    kw = {k: v for k, v in (('r1', r1), ('r2', r2)) if v is not None}
    return layer_norm(linear(x, weight, bias, **kw), norm, relu=relu_after)


def take_fused_norm(kwargs, autograd=False):
    """The LayerNorm that follows this module in the layer's operation_order, if the layer offers to have it fused
    (BaseTransformerLayer passes {'norm': module, 'done': False} under NORM_KEY); the taker sets done.  An offer is for
    the forward-only kernels or (key 'autograd') for the training path - never both."""
    holder = kwargs.get(NORM_KEY)
    if holder is None or holder['done'] or bool(holder.get('autograd')) != autograd:
        return None
    return holder


def position_encoder(seq, ref):
    """Reference position_encoder = Linear, LN, ReLU, Linear, LN, ReLU on inverse_sigmoid(ref)
    (deform3d_cross_attn.py:104-111,334): 3 launches - the 3/4-input Linear with inverse_sigmoid, LayerNorm and
    ReLU as one (ops.small_linear_layernorm_fwd), then Linear and LayerNorm+ReLU."""
    if ref.shape[-1] <= 4 and seq[0].out_features % 4 == 0 and seq[0].out_features <= 1024:
        h = ops.small_linear_layernorm_fwd(ref.contiguous(), seq[0].weight.contiguous(), seq[0].bias,
                                           seq[1].weight.contiguous(), seq[1].bias.contiguous(), seq[1].eps,
                                           relu=True, inv_sigmoid_in=True)
    else:
        h = linear(ref, seq[0].weight, seq[0].bias, inv_sigmoid_in=True)
        h = layer_norm(h, seq[1], relu=True)
    return linear_norm(h, seq[3].weight, seq[3].bias, seq[4], relu_after=True)


def use_head_major(value_dtype):
    """Value layout policy: head-major planes (B*N, Hh, S, Dh) pay off for bf16 storage (two
    x-adjacent corners = one 128-byte line: gather 42.9 -> 38.7 us); for fp32 the layouts tie, so the
    mmcv-compatible pixel-major layout is kept.  GD4D_VALUE_LAYOUT=pixel|head overrides (dev A/B)."""
    o = switches.choice('GD4D_VALUE_LAYOUT')
    if o is not None:
        return o == 'head'
    return value_dtype == torch.bfloat16


def value_projection(value, weight, bias, num_heads, out_dtype=torch.float32, max_cus=0):
    """value_proj over the flattened multi-camera pyramid (deform3d_cross_attn.py:264-280), one HIP
    pass (ops.value_proj_fwd): NCHW in, channels-last head-major out, no transposed/concatenated copies.

    value: list of L tensors (B, N, C, H_l, W_l).  Returns ((B*N, S, Hh, Dh) tensor, [(H_l, W_l)]).
    """
    shapes = [tuple(v.shape[-2:]) for v in value]
    b, n, c = value[0].shape[:3]
    hm = use_head_major(out_dtype)
    out = ops.value_proj_fwd([v.contiguous() for v in value], weight.contiguous(),
                             None if bias is None else bias.contiguous(), out_dtype,
                             num_heads=num_heads, head_major=hm, bf16_math=out_dtype == torch.bfloat16, max_cus=max_cus)
    return (out if hm else out.view(b * n, -1, num_heads, c // num_heads)), shapes


def run_branch(branch, x):
    """A head branch (reg_branches[lid] / cls_branches[lid]) applied to x.  nn.Sequential chains of Linear / LayerNorm
    / ReLU - what the heads build (dense_heads/detr3d_head.py:58-75, detr3d_head_pe.py:368-388) - run on
    gd4d_linear_fwd / gd4d_layernorm_fwd with the ReLUs fused; anything else is simply called."""
    nn = torch.nn
    mods = list(branch) if isinstance(branch, nn.Sequential) else None
    if not mods or not x.is_cuda or not all(isinstance(m, (nn.Linear, nn.ReLU, nn.LayerNorm)) for m in mods) \
            or not isinstance(mods[0], nn.Linear):
        return branch(x)
    i = 0
    while i < len(mods):
        m = mods[i]
        relu = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
        if isinstance(m, nn.Linear):
            x = linear(x, m.weight, m.bias, relu=relu)
        elif isinstance(m, nn.LayerNorm):
            x = layer_norm(x, m, relu=relu)
        else:                                   # a ReLU that follows another ReLU
            x, relu = torch.relu(x), False
        i += 2 if relu else 1
    return x


def _branch_program(branch, x_rows, out_rows, exact=False, width=512):
    """An nn.Sequential of Linear / LayerNorm / ReLU (what the heads build) as a row-chain program over x_rows (M, C) -> out_rows
    (M, N_last), or None if the branch has another shape.  LDS buffers 0 .. 2; exact: six bf16 products per GEMM."""
    nn = torch.nn
    mods = list(branch) if isinstance(branch, nn.Sequential) else None
    if not mods or not isinstance(mods[0], nn.Linear) or not isinstance(mods[-1], nn.Linear):
        return None
    prog, src, i = [ops.chain_load(0, x_rows)], 0, 0
    while i < len(mods):
        m = mods[i]
        relu = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
        last = i + (2 if relu else 1) >= len(mods)
        dst = (src + 1) % 3
        if isinstance(m, nn.Linear):
            if m.in_features % 64 or m.in_features > width or (not last and (m.out_features % 64 or m.out_features > width)):
                return None
            prog.append(ops.chain_gemm(src, m.weight, m.bias, dst=-1 if last else dst, relu=relu, exact=exact,
                                       out=out_rows if last else None))
        elif isinstance(m, nn.LayerNorm) and not last:
            if len(m.normalized_shape) != 1 or m.normalized_shape[0] % 64 or m.weight is None:
                return None
            prog.append(ops.chain_layernorm(src, m, dst=dst, relu=relu))
        else:
            return None
        src = dst
        i += 2 if relu else 1
    return prog


def head_outputs(hs, init_reference, inter_references, cls_branches, reg_branches, pc_range, depth_factor=None):
    """The per-layer epilogue of Detr3DHeadPE.forward (dense_heads/detr3d_head_pe.py:568-612).

    hs (num_layers, Q, B, C) as the transformer returns it (the head permutes it to (num_layers, B, Q, C), :568);
    init_reference (B, Q, 3), inter_references (num_layers, B, Q, 3) in [0,1]; cls_branches / reg_branches: one
    branch per layer; depth_factor: img_metas[0]['depth_factors'][0] when the head runs with scale_pred.
    Returns the head's dict: all_cls_scores (num_layers, B, Q, num_classes), all_bbox_preds (num_layers, B, Q, code).
    """
    hs = hs.permute(0, 2, 1, 3)
    classes, coords = [], []
    if wants_grad(cls_branches, hs) or wants_grad(reg_branches):
        # training: the branches through the package's autograd Functions (weight gradients through gd4d_linear_bwd_weight), the
        # box epilogue of all layers as ONE autograd node (autograd.BoxHeadFunction)
        from .autograd import BoxHeadFunction
        tmps = []
        for lvl in range(hs.shape[0]):
            x = hs[lvl].contiguous()
            classes.append(sequential_autograd(cls_branches[lvl], x))
            tmps.append(sequential_autograd(reg_branches[lvl], x))
        refs = torch.cat([init_reference.unsqueeze(0), inter_references[:-1]], 0) if hs.shape[0] > 1 else init_reference.unsqueeze(0)
        boxes = BoxHeadFunction.apply(torch.stack(tmps), refs, pc_range, 1.0 if depth_factor is None else float(depth_factor))
        return {'all_cls_scores': torch.stack(classes), 'all_bbox_preds': boxes,
                'enc_cls_scores': None, 'enc_bbox_preds': None}
    chains = hs.is_cuda and hs.dtype == torch.float32 and switches.flag('GD4D_HEAD_CHAINS')
    for lvl in range(hs.shape[0]):
        reference = init_reference if lvl == 0 else inter_references[lvl - 1]
        x = hs[lvl].contiguous()
        if chains:
            # both branches of a layer as the two programs of ONE row-chain launch (the reg branch on six products, as the decoder
            # computes it for the refinement): 6 launches instead of 6 x (6 Linear + 2 LayerNorm)
            rows = x.view(-1, x.shape[-1])
            seq = isinstance(cls_branches[lvl], torch.nn.Sequential) and isinstance(reg_branches[lvl], torch.nn.Sequential)
            last_c, last_r = (cls_branches[lvl][-1], reg_branches[lvl][-1]) if seq else (None, None)     # (PETRv2's RegLayer: run_branch)
            if isinstance(last_c, torch.nn.Linear) and isinstance(last_r, torch.nn.Linear):
                cls = torch.empty(*x.shape[:-1], last_c.out_features, device=x.device, dtype=torch.float32)
                tmp = torch.empty(*x.shape[:-1], last_r.out_features, device=x.device, dtype=torch.float32)
                pc = _branch_program(cls_branches[lvl], rows, cls.view(rows.shape[0], -1))
                pr = _branch_program(reg_branches[lvl], rows, tmp.view(rows.shape[0], -1), exact=True)
                if pc is not None and pr is not None:
                    ops.row_chain2_fwd(pc, pr, rows.shape[0])
                    classes.append(cls)
                    coords.append(ops.box_head_fwd(tmp, reference.contiguous(), pc_range,
                                                   1.0 if depth_factor is None else float(depth_factor), out=tmp))
                    continue
        classes.append(run_branch(cls_branches[lvl], x))
        tmp = run_branch(reg_branches[lvl], x).contiguous()
        coords.append(ops.box_head_fwd(tmp, reference.contiguous(), pc_range,
                                       1.0 if depth_factor is None else float(depth_factor), out=tmp))
    return {'all_cls_scores': torch.stack(classes), 'all_bbox_preds': torch.stack(coords),
            'enc_cls_scores': None, 'enc_bbox_preds': None}


def refine_reference(tmp, reference_points):
    """detr3d_transformer.py:201-214 as one launch (ops.refine_reference_fwd)."""
    return ops.refine_reference_fwd(tmp.contiguous(), reference_points.contiguous())


VALUE_CACHE_KEY = '_gd4d_value_cache'


def project_values_for_layers(modules, value):
    """Project the SAME pyramid with every layer's value_proj in one launch
    (ops.value_proj_multi_fwd).  Every decoder layer receives the same `value` list
    (detr3d_transformer.py:192-198), so the pyramid is read once instead of once per layer.

    modules: the Deform3DCrossAttn instances (one per decoder layer).  Returns the dict handed to
    them through kwargs[VALUE_CACHE_KEY]: {id(module): (value tensor, shapes, source list)}.
    """
    shapes = [tuple(v.shape[-2:]) for v in value]
    b, n, c = value[0].shape[:3]
    hh = modules[0].num_heads
    hm = use_head_major(modules[0].value_dtype)
    outs = ops.value_proj_multi_fwd([v.contiguous() for v in value],
                                    [m.value_proj.weight.contiguous() for m in modules],
                                    [m.value_proj.bias.contiguous() for m in modules],
                                    modules[0].value_dtype, num_heads=hh, head_major=hm,
                                    bf16_math=modules[0].value_dtype == torch.bfloat16)
    return {id(m): ((o if hm else o.view(b * n, -1, hh, c // hh)), shapes, value) for m, o in zip(modules, outs)}


def raw_pyramid_for_training(modules, value):
    """Training on the inference design (the default; GD4D_TRAIN_VALUES=projected keeps the projected-value pipeline): ONE
    slice-planar copy of the NCHW pyramid behind autograd.PyramidSourceFunction; every layer then runs plan + channel-sliced
    gather + value_proj of its aggregates (autograd.CrossAttnRawFunction) and the pyramid's gradient is assembled once,
    after the last layer's backward.  Returns the dict handed to the layers through kwargs[VALUE_CACHE_KEY]:
    {id(module): (None, shapes, value, (RawPyramid, token))}, or None when the path does not apply (bf16 values, channels-last
    levels, shapes outside the kernels' limits)."""
    if switches.choice('GD4D_TRAIN_VALUES') != 'raw' or not LateValues.applicable(modules, value, ignore_mode=True):
        return None
    if any(v.dtype != torch.float32 for v in value):
        return None
    from .autograd import PyramidSourceFunction, RawPyramid
    raw = RawPyramid()
    # modules built with value_dtype='bf16': the copy the gathers read is stored bf16 (half the bytes forward and backward; the
    # features are ROUNDED, products and sums stay fp32, the gradient is that of the rounded features handed to the fp32 ones)
    raw.copy_dtype = modules[0].value_dtype
    token = PyramidSourceFunction.apply(raw, *value)
    shapes = [tuple(v.shape[-2:]) for v in value]
    return {id(m): (None, shapes, value, (raw, token)) for m in modules}


def project_values_for_layers_autograd(modules, value):
    """Training counterpart of project_values_for_layers: the same launch behind autograd.ValueProjMultiFunction, whose
    backward sums the pyramid's gradient over the layers in place.  fp32 pixel-major value tensors (what
    gd4d_cross_attn_bwd takes)."""
    from .autograd import ValueProjMultiFunction
    shapes = [tuple(v.shape[-2:]) for v in value]
    b, n, c = value[0].shape[:3]
    hh = modules[0].num_heads
    # value_proj's weight gradient from per-head aggregates of the raw pyramid instead of a contraction over every pixel
    # row (autograd.CrossAttnFunction): needs ONE channels-last copy of the pyramid per step (no gradient)
    cl = None
    if LateValues.applicable(modules, value, ignore_mode=True):
        with torch.no_grad():
            # (a PyramidView: the channel-sliced gather reads it; GD4D_AGG=rows keeps the pixel-major copy + gd4d_cross_attn_agg_fwd)
            src = [v.detach().contiguous() for v in value]
            if switches.choice('GD4D_AGG') == 'sliced':
                sp, hw = ops.pyramid_slice_planar_fwd(src)
                cl = ops.PyramidView.slice_planar(sp, hw)
            else:
                cl = ops.pyramid_channels_last_fwd(src)[0]
    outs = ValueProjMultiFunction.apply(-len(modules) if cl is not None else len(modules),
                                        *[m.value_proj.weight for m in modules],
                                        *[m.value_proj.bias for m in modules], *value)
    return {id(m): (o.view(b * n, -1, hh, c // hh), shapes, value, cl) for m, o in zip(modules, outs)}


_SIDE_STREAMS = {}
_AUX_STREAMS = {}


def _companion_stream(table, device):
    """The side / auxiliary stream that belongs to the CURRENT stream of `device`: requests that run concurrently on
    different streams (bench.py --inflight) must not meet on one shared companion stream."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    s = table.get(key)
    if s is None:
        s = table[key] = torch.cuda.Stream(device)
    return s


REF_EVENT_KEY = '_gd4d_ref_event'


def aux_stream(device):
    """Second-branch HIP stream for query-side work that is off the layer's critical path (position_encoder of the
    reference points, the reg branch + refinement between layers).  Those kernels are tiny and latency-bound; run
    next to the main chain they cost nothing.  None when disabled (GD4D_AUX_STREAM=0)."""
    if not switches.flag('GD4D_AUX_STREAM'):
        return None
    return _companion_stream(_AUX_STREAMS, device)


VALUE_PIPELINE_KEY = '_gd4d_value_pipeline'


class ValuePipeline:
    """value_proj of the decoder layers on a second HIP stream, in GROUPS of consecutive layers (one multi-layer launch
    per group), software-pipelined against the query side.

    A layer's value_proj depends on the pyramid only, not on the queries; the query-side kernels (self-attention, small
    linears, LayerNorms, FFN, reg branch) are latency-bound and leave most of the GPU idle.  Group g+1 is launched on the
    side stream as soon as the FIRST gather of group g has been enqueued (it waits for that gather's event) and runs
    underneath the query side of group g's layers; the first gather of group g+1 waits for its event.  Larger groups
    amortise the pyramid's read + split over more layers (a six-layer launch costs 1.98 ms, six single ones 2.9 ms) but
    expose more of the query-side chain: groups=(1,)*6 is the round-1 per-layer pipeline, groups=(6,) one launch."""

    def __init__(self, modules, value, groups=None, first_cus=0):
        self.modules, self.value = list(modules), value
        n = len(self.modules)
        groups = tuple(groups) if groups else (1,) * n
        if sum(groups) != n or any(g < 1 for g in groups):
            raise ValueError(f'layer groups {groups} do not partition {n} layers')
        self.bounds, lo = [], 0
        for g in groups:
            self.bounds.append((lo, lo + g))
            lo += g
        self.group_of = {id(m): gi for gi, (a, b) in enumerate(self.bounds) for m in self.modules[a:b]}
        dev = value[0].device
        self.main = torch.cuda.current_stream(dev)
        self.side = _companion_stream(_SIDE_STREAMS, dev)
        self.side.wait_stream(self.main)             # the pyramid was produced on the main stream
        self.ready = {}
        self.issued = 0
        self._issue(first_cus)                       # nothing runs next to the first group: the whole device

    # CUs the persistent value_proj kernel may take while the query side runs next to it (its workgroups own the whole
    # register file of their CUs, so the query-side kernels only ever run on the CUs left free; the row-chain kernels
    # are 57 workgroups at 900 queries and want one round): 3/4 of the device.  MI355X, groups of two layers, fused
    # decoder: 144: 345, 160: 352, 176: 365, 192: 373, 224: 356 samples/s.  GD4D_PIPELINE_CUS overrides.
    def _cu_share(self, group_size):
        env = switches.integer('GD4D_PIPELINE_CUS')
        if env is not None:
            return env
        cus = torch.cuda.get_device_properties(self.value[0].device).multi_processor_count
        return max(8, (cus * 3 // 4) // 8 * 8)

    def _issue(self, max_cus):
        a, b = self.bounds[self.issued]
        mods = self.modules[a:b]
        with torch.cuda.stream(self.side):
            hh, dt = mods[0].num_heads, mods[0].value_dtype
            hm = use_head_major(dt)
            shapes = [tuple(v.shape[-2:]) for v in self.value]
            bn, c = self.value[0].shape[0] * self.value[0].shape[1], self.value[0].shape[2]
            outs = ops.value_proj_multi_fwd([v.contiguous() for v in self.value],
                                            [m.value_proj.weight.contiguous() for m in mods],
                                            [None if m.value_proj.bias is None else m.value_proj.bias.contiguous() for m in mods],
                                            dt, num_heads=hh, head_major=hm, bf16_math=dt == torch.bfloat16, max_cus=max_cus)
            ev = torch.cuda.Event()
            ev.record(self.side)
        for m, o in zip(mods, outs):
            self.ready[id(m)] = ((o if hm else o.view(bn, -1, hh, c // hh)), shapes, ev)
        self.issued += 1

    def take(self, module, value):
        """(value tensor, shapes) of `module` once the main stream has been made to wait for it; None if not ours."""
        entry = self.ready.get(id(module))
        if entry is None or value is not self.value:
            return None
        self.main.wait_event(entry[2])
        return entry[0], entry[1]

    def gather_enqueued(self, module):
        """Called right after `module`'s fused gather was enqueued on the main stream: release its value tensor; behind
        the first gather of the newest group, start the next group's projection."""
        if self.ready.pop(id(module), None) is None:
            return
        if self.group_of[id(module)] == self.issued - 1 and self.issued < len(self.bounds):
            ev = torch.cuda.Event()
            ev.record(self.main)
            self.side.wait_event(ev)
            a, b = self.bounds[self.issued]
            self._issue(self._cu_share(b - a))

    def finish(self):
        self.main.wait_stream(self.side)             # join (also keeps a graph capture well-formed)
        self.ready.clear()


def _wait_stream(waiter, other):
    """waiter.wait_stream(other) - or, while a request program is being recorded (ops.StepRecorder), its two steps."""
    rec = _lib.recorder()
    if rec is None:
        waiter.wait_stream(other)
    else:
        rec.wait_event(waiter, rec.record_event(other))


def _record_event(stream):
    """A new event recorded on `stream` (recording: the event's id in the request program)."""
    rec = _lib.recorder()
    if rec is not None:
        return rec.record_event(stream)
    ev = torch.cuda.Event()
    ev.record(stream)
    return ev


def _wait_event(stream, event):
    rec = _lib.recorder()
    if rec is None:
        stream.wait_event(event)
    else:
        rec.wait_event(stream, event)


LATE_VALUES_KEY = '_gd4d_late_values'


class LateValues:
    """The aggregate-then-project form of the value path (csrc/gd4d_cross_attn_late.hip): ONE channels-last copy of the
    pyramid for all decoder layers (the reference's flatten / transpose / cat, deform3d_cross_attn.py:264-276), made on the
    side stream next to layer 0's self-attention; every layer then gathers raw features per head (ops.cross_attn_agg_fwd)
    and applies its value_proj to the 900 x Hh aggregates (ops.value_proj_heads_fwd) instead of to 739 800 pixel rows.
    GD4D_PROJECT=early keeps the projected-value path (value_proj kernel + gd4d_cross_attn_fwd)."""

    def __init__(self, value, dtype=torch.float32, coarse_for=None):
        """dtype: storage type of the channels-last copy - torch.bfloat16 for modules built with value_dtype='bf16' (half the
        bytes to copy and to gather, bf16-rounded features, fp32 accumulation).

        Three sources for the gather (GD4D_AGG=rows|sliced, default sliced):
          rows    gd4d_pyramid_channels_last_fwd -> (R, S, 256), gd4d_cross_attn_agg_fwd (one workgroup per query, value_proj
                  in its epilogue); batch 1 only
          sliced  gd4d_pyramid_slice_planar_fwd -> (8, R, S, 32), gd4d_cross_attn_plan_fwd + gd4d_cross_attn_agg_sliced_fwd
          in place (no copy at all): when the caller's levels are already stored channels-last (..., H, W, 256), fp32 or
                  bf16 - the reference's own flatten / transpose (deform3d_cross_attn.py:264-276) has nothing left to do;
                  always the sliced kernels, which read per-level pointers with strides.

        coarse_for: the cross-attention modules of a decoder whose fused loop (fused_decoder.run_single) will consume this object
        with the coarse levels projected first (coarse_setup).  Then the FIRST module's projection of the two coarse levels is
        enqueued here, on the side stream in front of the copy - no chain launch precedes the first gather for it to ride in -
        and the copy leaves the coarse levels out (nobody reads them raw; a consumer that does after all: _ensure_full)."""
        dev = value[0].device
        self.value = value
        self.main = torch.cuda.current_stream(dev)
        self.shapes = [(int(v.shape[-2]), int(v.shape[-1])) for v in value]
        self.cl = self.pyramid = self.event = self.src = None
        self.copy_dtype = torch.float32
        self.coarse = self.coarse_src = self.coarse_first = None
        self.partial = False
        self.project_late = False
        self.waited = set()
        if all(ops.PyramidView.is_channels_last_level(v) for v in value) and len({v.dtype for v in value}) == 1 \
                and value[0].dtype in (torch.float32, torch.bfloat16):
            self.mode, self.side = 'sliced', None
            self.pyramid = ops.PyramidView.channels_last_levels(list(value))
            if coarse_for and self.coarse_setup(coarse_for):
                self.side = _companion_stream(_SIDE_STREAMS, dev)
                _wait_stream(self.side, self.main)
                with torch.cuda.stream(self.side):
                    self._project_first(coarse_for[0])
                    self.event = _record_event(self.side)
                self.coarse.rows.record_stream(self.main)
            return
        self.mode = switches.choice('GD4D_AGG')
        if self.mode == 'rows' and value[0].shape[0] != 1:
            self.mode = 'sliced'                     # B > 1: the row % B pairing lives in the plan kernel
        self.side = _companion_stream(_SIDE_STREAMS, dev)
        _wait_stream(self.side, self.main)             # the pyramid was produced on the main stream
        with torch.cuda.stream(self.side):
            # GD4D_COPY_CUS: compute units of the persistent copy (default 3/4 of the device: the query side of the first layer and the
            # first projection of the coarse levels run on the rest, underneath it - round 6, samples/s one request / two in flight:
            # 160: 646 / 798, 192: 656-658 / 807-810, 224: 657-659 / 785-789, 256: 659 / 778); 0 = the plain one-workgroup-per-tile copy
            env = switches.integer('GD4D_COPY_CUS')
            cus = torch.cuda.get_device_properties(dev).multi_processor_count
            copy_cus = env if env is not None else max(8, (cus * 3 // 4) // 8 * 8)
            src = [v.contiguous() for v in value]
            self.src, self.copy_cus, self.copy_dtype = src, copy_cus, dtype
            if self.mode == 'sliced':
                if coarse_for and self.coarse_setup(coarse_for):
                    # The first layer's projection of the coarse levels: on the MAIN stream behind plan 0 (aggregate), where that
                    # stream would otherwise only wait for the copy - in front of the copy it was 19-26 us of the request's critical
                    # path (one request at a time: 667 against 658 samples/s; two in flight: 786 against 808 - GD4D_FIRST_PROJ=side).
                    if switches.choice('GD4D_FIRST_PROJ') == 'main':
                        self.coarse_first, self.project_late = coarse_for[0], True
                    else:
                        self._project_first(coarse_for[0])
                    self.coarse.rows.record_stream(self.main)
                    self.partial = True
                if self.partial:
                    # the fine levels only: (8, R, S01, 32); the view's coarse entries are never dereferenced by the coarse gather
                    self.cl, _ = ops.pyramid_slice_planar_fwd(src[:2], max_cus=copy_cus, out_dtype=dtype)
                    fine = ops.PyramidView.slice_planar(self.cl, self.shapes[:2])
                    self.pyramid = ops.PyramidView([self.cl], fine.ptrs + fine.ptrs[:1] * 2, self.shapes, fine.cam_stride + fine.cam_stride[:1] * 2,
                                                   fine.pix_stride, fine.slice_stride, fine.dtype, fine.rows)
                else:
                    self.cl, _ = ops.pyramid_slice_planar_fwd(src, max_cus=copy_cus, out_dtype=dtype)
                    self.pyramid = ops.PyramidView.slice_planar(self.cl, self.shapes)
            else:
                self.cl, _ = ops.pyramid_channels_last_fwd(src, max_cus=copy_cus, out_dtype=dtype)
            self.event = _record_event(self.side)
        # allocated under the side stream, read by kernels of the main stream: tell the allocator, so that the block is
        # not handed out again (to a side-stream allocation) while those kernels are still queued
        self.cl.record_stream(self.main)

    def _project_first(self, module):
        """(current stream = the side stream) the first layer's projection of the coarse levels, a launch of its own."""
        ops.value_proj_guest_fwd(self.coarse_guest(module))
        self.coarse_first = module

    def take_first(self, module):
        """Whether the coarse rows of `module` were enqueued at construction and nobody has overwritten them yet (once)."""
        hit, self.coarse_first = self.coarse_first is module, None
        return hit

    def _ensure_full(self):
        """A consumer that gathers ALL levels raw came after the copy was made for the coarse-projected gather: copy again, all levels."""
        if not self.partial:
            return
        self._wait_copy()
        self.cl, _ = ops.pyramid_slice_planar_fwd(self.src, max_cus=0, out_dtype=self.copy_dtype)
        self.pyramid = ops.PyramidView.slice_planar(self.cl, self.shapes)
        self.partial = False

    @staticmethod
    def applicable(modules, value, ignore_mode=False):
        if (not ignore_mode and switches.choice('GD4D_PROJECT') != 'late') or not modules \
                or not isinstance(value, (list, tuple)):
            return False
        in_place = all(torch.is_tensor(v) and ops.PyramidView.is_channels_last_level(v) for v in value)
        ok_dtype = (torch.float32, torch.bfloat16) if in_place else (torch.float32,)
        if any(v.dim() != 5 or v.shape[0] > 16 or v.dtype not in ok_dtype or not v.is_cuda or v.shape[2] != 256 for v in value):
            return False
        rows = value[0].shape[1]
        if rows > 64 or len(value) > 4 or value[0].shape[0] * rows * sum(v.shape[-1] * v.shape[-2] for v in value) >= 2 ** 31:
            return False
        return len({m.value_dtype for m in modules}) == 1 and \
            all((m.num_points <= 4 or (m.num_points <= 8 and m.num_heads == 8)) and m.num_heads in (4, 8, 16) and m.embed_dims == 256
                and m.num_levels == len(value) and m.num_cams == rows for m in modules)

    def coarse_setup(self, modules):
        """Arrange for the two COARSE levels to be gathered from projected rows (ops.cross_attn_agg_coarse_fwd): one (R, S23, 256)
        buffer that a layer's value_proj fills before that layer's gather - coarse_guest(module) is the job, run by guest
        workgroups of a row-chain launch (ops.row_chain_fwd(..., guest=)) - and that the next layer's overwrites after it.  A raw
        corner costs 1 KB through the L1s whatever its level, a projected one 128 B per head; levels 2-3 are 6 % of the pixels and
        were a third of the gather.  Returns whether it applies: 4 levels, 8 heads, fp32 source levels (GD4D_COARSE=0: off)."""
        if self.coarse is not None:
            return True
        if not switches.flag('GD4D_COARSE') or self.mode != 'sliced' or len(self.shapes) != 4 or not modules:
            return False
        if any(m.num_heads != 8 or m.embed_dims != 256 for m in modules) or self.value[0].dtype != torch.float32:
            return False
        if getattr(self, 'copy_dtype', torch.float32) != torch.float32:      # bf16 storage: every level is gathered bf16-rounded
            return False
        src = list(self.value[2:]) if self.src is None else list(self.src[2:])
        rows = src[0].numel() // (256 * self.shapes[2][0] * self.shapes[2][1])
        s23 = sum(h * w for h, w in self.shapes[2:])
        # The projection must fit the window it hides in: ~30 us for the 43 800 rows of the R50 pyramid at 24 cameras beside a 55-us
        # chain; the VoVNet-99 pyramid's coarse levels are 4 x that while its gather gains the same ~30 us (GD4D_COARSE_MAX_ROWS).
        if rows * s23 > switches.integer('GD4D_COARSE_MAX_ROWS'):
            return False
        buf = torch.empty(rows, s23, 256, device=src[0].device, dtype=torch.float32)
        self.coarse_src, self.coarse = src, ops.CoarseValues(buf, self.shapes[2:])
        return True

    def coarse_guest(self, module, workgroups=0):
        """The ChainGuest that projects the coarse levels with `module`'s value_proj into the buffer coarse_setup made."""
        bias = module.value_proj.bias
        img = ops.value_proj_image(module.value_proj.weight, bias)
        return ops.chain_guest(self.coarse_src, img, self.coarse.rows, workgroups=workgroups)

    def _wait_copy(self):
        if self.event is None:
            return
        made = [t for t in (self.cl, None if self.coarse is None else self.coarse.rows) if t is not None]   # what the side stream wrote
        cur = torch.cuda.current_stream(made[0].device)
        if cur.cuda_stream not in self.waited:
            _wait_event(cur, self.event)
            self.waited.add(cur.cuda_stream)
            if cur.cuda_stream != self.main.cuda_stream:
                for t in made:
                    t.record_stream(cur)

    def aggregate(self, module, ref, offsets, attn_logits, cam_logits, lidar2img, img_h, img_w, order=None, vp_weight=None,
                  vp_bias=None, raw_cam_weights=False, coarse=False, reverse=False):
        """Per-head aggregates of the raw features: agg (B, Q, Hh, C), wsum (B, Q, Hh); rows mode with vp_weight:
        (out (B, Q, C),) - value_proj applied in the kernel's epilogue.  raw_cam_weights: the camera logits are used as they
        are, without the sigmoid (the neighbour pass of Deform3DCrossAttnMP).  coarse (after coarse_setup, the buffer holding THIS
        module's projection): (agg, wsum, pagg) - the fine levels' aggregates and weight sums and the coarse levels' already
        projected part (B, Q, C); value_proj of (agg, wsum) plus pagg is the layer's sampled value.  reverse (with coarse): the
        gather walks its slice groups from last to first (ops.cross_attn_agg_coarse_fwd)."""
        # (kernels: 1 / 2 / 4 / 8 points per head with 8 heads on the sliced form, 4 otherwise; other counts - the reference's
        #  constructor default is 5 - are padded with points that are never visible and weigh nothing)
        offsets, attn_logits = pad_points(offsets, attn_logits, (1, 2, 4, 8) if self.mode == 'sliced' and module.num_heads == 8 else (4,),
                                          'Deform3DCrossAttn')
        if not coarse:
            self._ensure_full()
        if self.mode == 'sliced':
            # (the plan needs nothing from the pyramid but its strides: layer 0's runs underneath the copy)
            # GD4D_PLAN=pairs: the 128-bytes-per-item form the training kernels read
            items = coarse or switches.choice('GD4D_PLAN') != 'pairs'     # (the coarse-projected gather walks items)
            plan = ops.cross_attn_plan_fwd(self.pyramid, ref.contiguous(), offsets.contiguous(), attn_logits.contiguous(),
                                           cam_logits.contiguous(), lidar2img, module.pc_range, img_h, img_w, module.num_heads,
                                           query_order=order, items=items, raw_cam_weights=raw_cam_weights)
            if coarse and self.project_late:
                self.project_late = False
                ops.value_proj_guest_fwd(self.coarse_guest(module))
            self._wait_copy()
            if coarse:
                agg, pagg = ops.cross_attn_agg_coarse_fwd(plan, self.coarse, reverse=reverse)
                return agg, plan.wsum, pagg
            agg = ops.cross_attn_agg_sliced_fwd(plan)
            if vp_weight is not None:
                return (ops.value_proj_heads_fwd(agg, plan.wsum, vp_weight, vp_bias),)
            return agg, plan.wsum
        self._wait_copy()
        return ops.cross_attn_agg_fwd(self.cl, self.shapes, ref.contiguous(), offsets.contiguous(), attn_logits.contiguous(),
                                      cam_logits.contiguous(), lidar2img, module.pc_range, img_h, img_w,
                                      module.num_heads, query_order=order, vp_weight=vp_weight, vp_bias=vp_bias,
                                      raw_cam_weights=raw_cam_weights)

    def sample_aggregate(self, module, ref, offsets, attn_logits, cam_logits, lidar2img, img_h, img_w, order=None):
        """What functional.sample_aggregate returns on the projected values of `module`: (B, Q, C), the input of
        output_proj.  value_proj of the per-head aggregates runs in the gather kernel's epilogue (rows form) or as its own launch
        (sliced form: gd4d_value_proj_heads_fwd)."""
        bias = module.value_proj.bias
        weight, bias = module.value_proj.weight.contiguous(), None if bias is None else bias.contiguous()
        return self.aggregate(module, ref, offsets, attn_logits, cam_logits, lidar2img, img_h, img_w, order=order,
                              vp_weight=weight, vp_bias=bias)[0]

    def finish(self):
        if self.side is not None:
            _wait_stream(self.main, self.side)         # join (keeps a graph capture well-formed)


def pipeline_groups(spec, n):
    """GD4D_PREPROJECT: 'auto' -> groups of two layers; 'stream' -> n single layers; 'g3,3' / 'g2,2,2' / ... -> those group sizes (they must add up to
    the number of layers, else the spec is ignored: None)."""
    if spec == 'stream':
        return (1,) * n
    if spec == 'auto':
        return (2,) * (n // 2) + ((1,) if n % 2 else ())
    if spec.startswith('g'):
        try:
            g = tuple(int(x) for x in spec[1:].split(','))
        except ValueError:
            return None
        return g if sum(g) == n and all(x >= 1 for x in g) else None
    return None


QUERY_ORDER_KEY = '_gd4d_query_order'


def query_order(reference_points, pc_range):
    """Locality order of the queries for the fused kernel (ops.query_order_fwd): one tiny launch; the decoder computes
    it once per call and hands it to every layer through kwargs[QUERY_ORDER_KEY].  GD4D_QUERY_ORDER=0 disables."""
    if not query_order_enabled(reference_points):
        return None
    return ops.query_order_fwd(reference_points.detach().contiguous(), pc_range)


def query_order_enabled(reference_points):
    """gd4d_query_order_fwd sorts in one workgroup: up to 4096 queries per call; beyond that run unordered."""
    return switches.flag('GD4D_QUERY_ORDER') and reference_points.is_cuda and \
        reference_points.shape[0] * reference_points.shape[1] <= 4096 and reference_points.shape[0] <= 512


def refine_reference_order(tmp, reference_points, pc_range):
    """refine_reference + the locality order of the refined points in one launch (ops.refine_reference_order_fwd)."""
    return ops.refine_reference_order_fwd(tmp.contiguous(), reference_points.contiguous(), pc_range)


def sample_aggregate(value, shapes, ref, offsets, attn_logits, cam_logits, lidar2img, pc_range,
                     img_h, img_w, order=None):
    """The fused HIP kernel (ops.cross_attn_fwd): projection + mask + softmax + gather + camera sum."""
    offsets, attn_logits = pad_points(offsets, attn_logits, (1, 4), 'Deform3DCrossAttn on projected values')
    nl_pix = sum(h * w for h, w in shapes)
    head_major = value.shape[2] == nl_pix and value.shape[1] != nl_pix      # (B*N, Hh, S, Dh) planes
    return ops.cross_attn_fwd(value, shapes, ref.contiguous(), offsets.contiguous(),
                              attn_logits.contiguous(), cam_logits.contiguous(), lidar2img,
                              pc_range, img_h, img_w, head_major=head_major, query_order=order)
