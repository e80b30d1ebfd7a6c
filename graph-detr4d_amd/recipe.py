"""The reference's training recipe as ONE capturable optimizer step: learning-rate schedule, fp16 loss scale with skip-on-overflow,
gradient clipping and per-group AdamW, all from device-resident state (gd4d_adamw_recipe_flat, include/gd4d.h).

What an mmcv runner spreads over three hooks - `LrUpdaterHook` (lr_config), `Fp16OptimizerHook` (fp16, optimizer_config.grad_clip)
and the optimizer built by `DefaultOptimizerConstructor` (optimizer, paramwise_cfg) - is host work between steps: a replayed hipGraph
gets none of it.  `TrainRecipe` takes the same four dicts, verbatim
(projects/configs/detr4d/detr4d_res50_deform_pe_testaug_320_fullset_ceph.py:4, :205-220), and keeps the iteration counter, the
rate, the scale and Adam's step count on the device; `step()` is two launches and replays correctly for the whole run.

    recipe = TrainRecipe(reducer, model.named_parameters(), optimizer=cfg.optimizer, optimizer_config=cfg.optimizer_config,
                         lr_config=cfg.lr_config, fp16=cfg.get('fp16'), max_epochs=24, iters_per_epoch=len(loader))
    recipe.state()                      # before a capture
    recipe.scale(loss).backward(); reducer.reduce(); recipe.step(zero_grads=True)

Construction is host work only (it runs on CPU parameters); the device is first touched in state().  Anything in the dicts that
is not implemented raises Gd4dError naming the key.
"""
import ctypes
import math

import torch

from . import _lib
from ._lib import Gd4dError

MAX_RANGES, MAX_MILESTONES = 1024, 16
LR_FIXED, LR_COSINE, LR_STEP = 0, 1, 2
WARMUP_NONE, WARMUP_CONSTANT, WARMUP_LINEAR, WARMUP_EXP = 0, 1, 2, 3
_POLICIES = {'fixed': LR_FIXED, 'CosineAnnealing': LR_COSINE, 'step': LR_STEP}
_WARMUPS = {None: WARMUP_NONE, 'constant': WARMUP_CONSTANT, 'linear': WARMUP_LINEAR, 'exp': WARMUP_EXP}


class RecipeRange(ctypes.Structure):            # gd4d_recipe_range
    _fields_ = [('begin', ctypes.c_int64), ('end', ctypes.c_int64), ('lr_mult', ctypes.c_float), ('decay_mult', ctypes.c_float)]


class RecipeConfig(ctypes.Structure):           # gd4d_recipe_config
    _fields_ = [('base_lr', ctypes.c_double), ('end_lr', ctypes.c_double), ('gamma', ctypes.c_double), ('warmup_ratio', ctypes.c_double),
                ('init_scale', ctypes.c_double), ('growth_factor', ctypes.c_double), ('backoff_factor', ctypes.c_double),
                ('iters_per_epoch', ctypes.c_int64), ('max_epochs', ctypes.c_int64), ('max_iters', ctypes.c_int64),
                ('warmup_iters', ctypes.c_int64), ('step_every', ctypes.c_int64), ('milestones', ctypes.c_int64 * MAX_MILESTONES),
                ('policy', ctypes.c_int32), ('by_epoch', ctypes.c_int32), ('warmup', ctypes.c_int32), ('n_milestones', ctypes.c_int32),
                ('dynamic_scale', ctypes.c_int32), ('growth_interval', ctypes.c_int32), ('zero_grads', ctypes.c_int32),
                ('reserved', ctypes.c_int32),
                ('beta1', ctypes.c_float), ('beta2', ctypes.c_float), ('eps', ctypes.c_float), ('weight_decay', ctypes.c_float),
                ('max_norm', ctypes.c_float), ('reserved_f', ctypes.c_float)]


# gd4d_recipe_state as indices into its int64 / float32 / int32 views
_I64_ITERATION, _I64_STEPS, _I64_SKIPPED = 0, 1, 2
_F32_SCALE, _F32_SCALE_IN_USE, _F32_LR, _F32_NORM = 8, 9, 10, 11
_I32_FOUND_INF, _I32_TRACKER = 12, 13


def _only(d, allowed, what):
    for k in d:
        if k not in allowed:
            raise Gd4dError(f'TrainRecipe: {what} key {k!r} is not supported (supported: {sorted(allowed)})')


def _mults(v):
    """custom_keys value: dict(lr_mult=, decay_mult=), or a bare number = lr_mult."""
    if isinstance(v, dict):
        _only(v, {'lr_mult', 'decay_mult'}, 'paramwise_cfg.custom_keys entry')
        return float(v.get('lr_mult', 1.0)), float(v.get('decay_mult', 1.0))
    return float(v), 1.0


class TrainRecipe:
    def __init__(self, reducer, named_parameters, optimizer, optimizer_config=None, lr_config=None, fp16=None, max_epochs=1,
                 iters_per_epoch=1, max_iters=None):
        self.reducer = reducer
        if reducer.align % 4:
            raise Gd4dError('TrainRecipe needs a FlatGradAllReducer(align=4): a 16-byte quad of the flat buffer must not straddle two '
                            'parameter groups')
        self.cfg = c = RecipeConfig()
        # ---- optimizer ----
        opt = dict(optimizer)
        if opt.get('type') != 'AdamW':
            raise Gd4dError(f"TrainRecipe: optimizer type {opt.get('type')!r} is not supported (supported: 'AdamW')")
        _only(opt, {'type', 'lr', 'betas', 'eps', 'weight_decay', 'paramwise_cfg'}, 'optimizer')
        c.base_lr = float(opt['lr'])
        c.beta1, c.beta2 = (float(b) for b in opt.get('betas', (0.9, 0.999)))
        c.eps, c.weight_decay = float(opt.get('eps', 1e-8)), float(opt.get('weight_decay', 1e-2))
        pw = dict(opt.get('paramwise_cfg') or {})
        _only(pw, {'custom_keys'}, 'paramwise_cfg')
        self.custom_keys = {k: _mults(v) for k, v in (pw.get('custom_keys') or {}).items()}
        # ---- optimizer_config ----
        oc = dict(optimizer_config or {})
        _only(oc, {'grad_clip'}, 'optimizer_config')
        clip = oc.get('grad_clip')
        c.max_norm = 0.0
        if clip is not None:
            _only(clip, {'max_norm', 'norm_type'}, 'optimizer_config.grad_clip')
            if float(clip.get('norm_type', 2)) != 2.0:
                raise Gd4dError(f"TrainRecipe: grad_clip norm_type {clip['norm_type']!r} is not supported (supported: 2)")
            c.max_norm = float(clip['max_norm'])
        # ---- lr_config ----
        lc = dict(lr_config or {'policy': 'fixed'})
        policy = lc.get('policy')
        if policy not in _POLICIES:
            raise Gd4dError(f'TrainRecipe: lr_config policy {policy!r} is not supported (supported: {sorted(_POLICIES)})')
        _only(lc, {'policy', 'by_epoch', 'warmup', 'warmup_iters', 'warmup_ratio', 'warmup_by_epoch'} |
              {'CosineAnnealing': {'min_lr', 'min_lr_ratio'}, 'step': {'step', 'gamma'}, 'fixed': set()}[policy], 'lr_config')
        if lc.get('warmup_by_epoch', False):
            raise Gd4dError("TrainRecipe: lr_config key 'warmup_by_epoch' = True is not supported")
        if lc.get('warmup') not in _WARMUPS:
            raise Gd4dError(f"TrainRecipe: lr_config warmup {lc.get('warmup')!r} is not supported (supported: constant, linear, exp)")
        c.policy, c.by_epoch, c.warmup = _POLICIES[policy], int(bool(lc.get('by_epoch', True))), _WARMUPS[lc.get('warmup')]
        c.warmup_iters, c.warmup_ratio = int(lc.get('warmup_iters', 0)), float(lc.get('warmup_ratio', 0.1))
        if c.warmup != WARMUP_NONE and not (c.warmup_iters > 0 and 0 < c.warmup_ratio <= 1.0):
            raise Gd4dError('TrainRecipe: lr_config warmup needs warmup_iters > 0 and 0 < warmup_ratio <= 1')
        c.iters_per_epoch, c.max_epochs = int(iters_per_epoch), int(max_epochs)
        c.max_iters = int(max_iters) if max_iters is not None else c.max_epochs * c.iters_per_epoch
        c.gamma, c.end_lr = 0.1, 0.0
        if c.policy == LR_COSINE:
            has_ratio, has_min = lc.get('min_lr_ratio') is not None, lc.get('min_lr') is not None
            if has_ratio == has_min:
                raise Gd4dError("TrainRecipe: lr_config CosineAnnealing takes exactly one of 'min_lr' and 'min_lr_ratio'")
            c.end_lr = c.base_lr * float(lc['min_lr_ratio']) if has_ratio else float(lc['min_lr'])
        if c.policy == LR_STEP:
            c.gamma = float(lc.get('gamma', 0.1))
            step = lc.get('step')
            if isinstance(step, int) and step > 0:
                c.step_every = step
            elif isinstance(step, (list, tuple)) and 0 < len(step) <= MAX_MILESTONES and list(step) == sorted(set(int(s) for s in step)):
                c.n_milestones = len(step)
                for i, s in enumerate(step):
                    c.milestones[i] = int(s)
            else:
                raise Gd4dError(f"TrainRecipe: lr_config 'step' = {step!r}: a positive int or up to {MAX_MILESTONES} ascending milestones")
        # ---- fp16 ----
        c.init_scale, c.growth_factor, c.backoff_factor, c.growth_interval, c.dynamic_scale = 1.0, 2.0, 0.5, 2000, 0
        if fp16 is not None:
            _only(fp16, {'loss_scale'}, 'fp16')
            ls = fp16.get('loss_scale', 512.)
            if isinstance(ls, dict):
                _only(ls, {'init_scale', 'growth_factor', 'backoff_factor', 'growth_interval'}, 'fp16.loss_scale')
                c.dynamic_scale = 1
                c.init_scale, c.growth_factor = float(ls.get('init_scale', 65536.)), float(ls.get('growth_factor', 2.0))
                c.backoff_factor, c.growth_interval = float(ls.get('backoff_factor', 0.5)), int(ls.get('growth_interval', 2000))
            elif ls == 'dynamic':
                c.dynamic_scale, c.init_scale = 1, 65536.
            elif isinstance(ls, (int, float)) and not isinstance(ls, bool) and ls > 0:
                c.init_scale = float(ls)
            else:
                raise Gd4dError(f"TrainRecipe: fp16 loss_scale {ls!r} is not supported (a positive number, 'dynamic' or GradScaler's arguments)")
        if not c.growth_factor > 1.0 or not 0.0 < c.backoff_factor < 1.0 or c.growth_interval < 1:
            raise Gd4dError('TrainRecipe: fp16.loss_scale needs growth_factor > 1, 0 < backoff_factor < 1, growth_interval >= 1')
        # ---- parameter groups as ranges of the flat buffer ----
        names = {id(p): n for n, p in named_parameters}
        # mmcv's DefaultOptimizerConstructor: keys sorted alphabetically, then by length descending; the first key that is a
        # substring of the parameter's name wins
        keys = sorted(sorted(self.custom_keys), key=len, reverse=True)
        self.param_mults, ranges = [], []
        ends = list(reducer._offsets[1:]) + [reducer.numel]
        for p, off, end in zip(reducer.params, reducer._offsets, ends):
            if id(p) not in names:
                raise Gd4dError('TrainRecipe: a parameter of the reducer is missing from named_parameters (paramwise_cfg matches by name)')
            mult = next((self.custom_keys[k] for k in keys if k in names[id(p)]), (1.0, 1.0))
            self.param_mults.append((names[id(p)], mult))
            if ranges and ranges[-1][2] == mult:
                ranges[-1][1] = end
            else:
                ranges.append([off, end, mult])
        if len(ranges) > MAX_RANGES:
            raise Gd4dError(f'TrainRecipe: {len(ranges)} ranges of the flat buffer (groups interleave); the table holds {MAX_RANGES}')
        self.ranges = [(b, e, m[0], m[1]) for b, e, m in ranges]
        self._ranges_host = (RecipeRange * len(ranges))(*[RecipeRange(b, e, m[0], m[1]) for b, e, m in ranges])
        self._dev = None

    # ---- the schedule on the host (doubles): include/gd4d.h states the formulas ----
    def lr_at(self, it):
        c = self.cfg
        it = int(it)
        ep = it // c.iters_per_epoch
        r = c.base_lr
        if c.policy == LR_COSINE:
            f = ep / c.max_epochs if c.by_epoch else it / c.max_iters
            r = c.end_lr + 0.5 * (c.base_lr - c.end_lr) * (math.cos(math.pi * f) + 1.0)
        elif c.policy == LR_STEP:
            prog = ep if c.by_epoch else it
            e = prog // c.step_every if c.step_every > 0 else sum(1 for i in range(c.n_milestones) if c.milestones[i] <= prog)
            r = c.base_lr * c.gamma ** e
        if c.warmup != WARMUP_NONE and it < c.warmup_iters:
            x = it / c.warmup_iters
            if c.warmup == WARMUP_LINEAR:
                r *= 1.0 - (1.0 - x) * (1.0 - c.warmup_ratio)
            elif c.warmup == WARMUP_CONSTANT:
                r *= c.warmup_ratio
            else:
                r *= c.warmup_ratio ** (1.0 - x)
        return r

    # ---- device state ----
    @staticmethod
    def _capturing():
        return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()

    @torch.no_grad()
    def state(self):
        """Allocate exp_avg, exp_avg_sq, the device state words (loss scale = its initial value, counters zero), the range table and
        the workspace - idempotent.  Must precede a capture: zero-fills recorded into one would reset the run on every replay."""
        if self._dev is not None:
            return self._dev
        red = self.reducer
        if not red.params[0].is_cuda:
            raise Gd4dError('TrainRecipe.state: the parameters are CPU tensors; the optimizer step runs on the GPU only (no CPU fallback)')
        if self._capturing():
            raise RuntimeError('TrainRecipe: first use inside a hipGraph capture (its zero-filled state would be reset by every '
                               'replay) - call state() before capturing')
        lib = _lib.load()
        fp = red.flatten_params()
        dev = fp.device
        words = torch.zeros(int(lib.gd4d_adamw_recipe_flat_state_bytes()) // 4, dtype=torch.int32)
        words.view(torch.float32)[_F32_SCALE] = float(self.cfg.init_scale)
        table = torch.frombuffer(bytearray(bytes(self._ranges_host)), dtype=torch.uint8)
        self._i32 = words.to(dev)
        self._f32, self._i64 = self._i32.view(torch.float32), self._i32.view(torch.int64)
        self._dev = (torch.zeros_like(fp), torch.zeros_like(fp), self._i32,
                     torch.empty(int(lib.gd4d_adamw_recipe_flat_workspace_bytes()), device=dev, dtype=torch.uint8), table.to(dev))
        return self._dev

    def _bound(self):
        red = self.reducer
        flat = red._buffer(red.params[0])
        if red.views is None or any(p.grad is not v for p, v in zip(red.params, red.views)):
            red._bind(flat)
        return flat

    def scale(self, loss):
        """loss * the device's loss-scale word: capturable, and follows a dynamic scale from replay to replay."""
        self.state()
        return loss * self._f32[_F32_SCALE]

    @torch.no_grad()
    def step(self, zero_grads=False):
        """The two launches: unscale + norm + non-finite check + schedule, then clip + per-group AdamW (or the skip) + loss-scale update.
        zero_grads: the gradient buffer is zero afterwards (no separate fill in the captured step)."""
        m, v, words, ws, table = self.state()
        red = self.reducer
        fp, flat = red.flatten_params(), self._bound()
        self.cfg.zero_grads = int(bool(zero_grads))
        code = _lib.load().gd4d_adamw_recipe_flat(fp.data_ptr(), flat.data_ptr(), m.data_ptr(), v.data_ptr(), words.data_ptr(),
                                                  words.numel() * 4, ws.data_ptr(), ws.numel(), red.numel, ctypes.byref(self.cfg),
                                                  self._ranges_host, table.data_ptr(), len(self._ranges_host),
                                                  torch.cuda.current_stream(fp.device).cuda_stream)
        _lib.check(code, 'gd4d_adamw_recipe_flat')
        if not self._capturing():
            bump = getattr(torch.autograd.graph, 'increment_version', None)
            for p in red.params:
                if bump is not None:
                    bump(p)
                else:
                    p.add_(0)

    # device views (0-dim tensors over the state words: reading one on the host synchronises, holding one does not)
    def _word(self, view, index):
        self.state()
        return getattr(self, view)[index]

    lr = property(lambda self: self._word('_f32', _F32_LR))
    loss_scale = property(lambda self: self._word('_f32', _F32_SCALE))
    scale_in_use = property(lambda self: self._word('_f32', _F32_SCALE_IN_USE))
    last_grad_norm = property(lambda self: self._word('_f32', _F32_NORM))
    iteration = property(lambda self: self._word('_i64', _I64_ITERATION))
    optimizer_steps = property(lambda self: self._word('_i64', _I64_STEPS))
    skipped_steps = property(lambda self: self._word('_i64', _I64_SKIPPED))
    found_inf = property(lambda self: self._word('_i32', _I32_FOUND_INF))
    growth_tracker = property(lambda self: self._word('_i32', _I32_TRACKER))

    def _outside_capture(self, what):
        if self._capturing():
            raise RuntimeError(f'TrainRecipe.{what} inside a hipGraph capture: it is host work between replays')

    @torch.no_grad()
    def state_dict(self):
        self._outside_capture('state_dict')
        m, v, words = self.state()[:3]
        return {'exp_avg': m.clone(), 'exp_avg_sq': v.clone(), 'state_words': words.clone(), 'numel': self.reducer.numel,
                'iteration': int(self.iteration), 'optimizer_steps': int(self.optimizer_steps), 'skipped_steps': int(self.skipped_steps),
                'loss_scale': float(self.loss_scale), 'growth_tracker': int(self.growth_tracker)}

    @torch.no_grad()
    def load_state_dict(self, sd):
        self._outside_capture('load_state_dict')
        m, v, words = self.state()[:3]
        if int(sd['numel']) != self.reducer.numel or sd['state_words'].numel() != words.numel():
            raise Gd4dError(f"TrainRecipe.load_state_dict: saved over {sd['numel']} elements, this buffer has {self.reducer.numel}")
        m.copy_(sd['exp_avg'])
        v.copy_(sd['exp_avg_sq'])
        words.copy_(sd['state_words'])

    @torch.no_grad()
    def set_progress(self, iteration):
        """Set the schedule's clock (iterations finished so far), e.g. when resuming from a checkpoint that kept only the epoch."""
        self._outside_capture('set_progress')
        self.state()
        self._i64[_I64_ITERATION].fill_(int(iteration))
