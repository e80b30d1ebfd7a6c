"""The host-side skeleton of the modules that run on the bf16-MFMA convolution kernels: DepthNet, FPN / CPFPN, the two DCNv2 classes,
VoVNet's stem and OSA module, ResNet's blocks with `plain_kernels=True`.  Each mixes in `KernelRoute` and supplies its name for
messages, its limits and what train mode means for it; the route rule, the refusals, the values kept from parameters, `refresh_images()` and the input cast are stated here, once.

THE ROUTE RULE.  `_route(*inputs)` answers, per call, in this order:
    1. chosen     `module.torch_ops` (the constructor keyword `torch_ops=True`, `with Fn.torch_ops_for(module):`) or GD4D_TORCH_OPS=1
                  for the whole process: 'torch', the module's own torch layers - differentiable, any device and dtype.
    2. limits     a configuration or input outside the kernels' limits raises Gd4dError naming `torch_ops=True` (FPN and VoVNet
                  refuse at construction already, through `refuse_outside_limits`).
    3. train mode with `hip_train`: 'train', the module's autograd node on the library's forward and backward kernels.  Without it
                  (or for a module that has no such switch) train mode raises, naming the switches.
    4. autograd   grad mode on and a parameter or an input that requires grad: 'train' with `hip_train`, else it raises.
    5. device     CPU tensors raise: there is no CPU fallback.  Then 'infer', the inference launches (or 'train' from 3 / 4).
There is no quiet detour: the torch-op route runs only where it was chosen.

KEPT VALUES.  `_keep(key, sources, build)` is ops.kept_in_place on the module's own table: a weight image or folded constant is served
while ops._Stamp's rule holds for its sources, and is otherwise rebuilt INTO the buffer it had, so its device address is fixed.  A
forward can therefore be captured in a hipGraph after one eager call; capturing with a missing or stale value raises instead of
allocating, and a replay after an in-place parameter edit shows the new values once `refresh_images()` (or any eager forward) has
run outside the graph.
"""
import torch

from . import _lib
from . import functional as Fn
from . import ops


def f32(x):
    """x as fp32 contiguous NCHW: x itself where it already is, else a torch copy (not fused into the kernels' loads)."""
    return x if x.dtype == torch.float32 and x.is_contiguous() else x.float().contiguous()


def refuse_outside_limits(module, name, limits):
    """Raises, naming `torch_ops=True` and the first few of `limits`, unless there are none or the torch-op route was chosen."""
    if limits:
        more = f' and {len(limits) - 4} more' if len(limits) > 4 else ''
        Fn.torch_ops_route(f'{name}: {"; ".join(limits[:4])}{more} - torch_ops=True serves it', False, module=module)


class KernelRoute:
    """Mixin in front of nn.Module.  A module calls `_init_route` in its constructor and may override `_route_name`, `_limits`,
    `_in_train_mode`, `_kernels` (the phrase of the two refusals), `_kept_values` and the two hooks of a training route; a module with a
    training route has the attribute `hip_train`."""
    torch_ops = False
    _kernels = 'kernels have no backward'          # "graph-detr4d_amd's <_kernels>", in the train-mode and autograd refusals

    def _init_route(self, torch_ops, limits=()):
        self.torch_ops = bool(torch_ops)
        self._kernel_limits = list(limits)
        self._kept = {}             # key -> (ops._Stamp, value at a fixed address)

    # ---- what a module supplies ------------------------------------------------------------------------------------------------
    def _route_name(self):
        return type(self).__name__

    def _limits(self, *inputs):
        """What of this call lies outside the kernels' limits: the list made at construction, or one a module makes per call."""
        return self._kernel_limits

    def _in_train_mode(self):
        return self.training

    def _kept_values(self):
        """Fetches every kept value a captured forward reads (each through `_keep`)."""
        raise NotImplementedError

    def _has_train_route(self):
        """Whether the refusals may name `hip_train=True`: a module with a training route sets the attribute in __init__."""
        return 'hip_train' in self.__dict__

    def _refuse_train_route(self):
        """Called where the rule is about to answer 'train': raises Gd4dError for what the module's training route does not take."""

    # ---- the rule ------------------------------------------------------------------------------------------------------------
    def _route(self, *inputs):
        """'torch', 'train' or 'infer' for a call on these tensor inputs, or Gd4dError: the module docstring's rule."""
        if Fn.torch_ops_route(None, True, module=self):         # (asked whether chosen only: nothing to name)
            return 'torch'
        limits = self._limits(*inputs)
        if limits:                                              # (the name is made only where something is refused)
            refuse_outside_limits(self, self._route_name(), limits)
        switch = self._has_train_route()
        route = 'infer'
        if switch and self.hip_train:
            if self._in_train_mode() or Fn.wants_grad(self, *inputs):
                self._refuse_train_route()
                route = 'train'
        elif self._in_train_mode():
            raise _lib.Gd4dError(f'{self._route_name()} in train() mode: graph-detr4d_amd\'s {self._kernels}.  `torch_ops=True` (or '
                                 'GD4D_TORCH_OPS=1) runs the module\'s own torch layers, the reference arithmetic, trainable by autograd'
                                 + ('; `hip_train=True` trains it on the library\'s own forward and backward kernels.' if switch else '.'))
        elif Fn.wants_grad(self, *inputs):
            raise _lib.Gd4dError(f'{self._route_name()}: autograd is on, and graph-detr4d_amd\'s {self._kernels}.  Run inference under '
                                 'torch.no_grad() (or freeze the parameters and the inputs), or choose the torch-op route '
                                 '(`torch_ops=True` / GD4D_TORCH_OPS=1)'
                                 + ('; `hip_train=True` makes the kernel route differentiable.' if switch else '.'))
        for x in inputs:
            Fn.require_gpu(x, 'inputs')
        return route

    # ---- kept values ---------------------------------------------------------------------------------------------------------
    def _keep(self, key, sources, build):
        return ops.kept_in_place(self._kept, key, sources, build, self)

    def refresh_images(self):
        """For the owner of a hipGraph captured over this module: after an in-place parameter edit, rebuild the changed weight images
        and folded constants into the buffers the graph reads (outside the graph, before the replay).  Writes through `.data` need
        ops.invalidate_chain_images() first, as everywhere."""
        if not next(self.parameters()).is_cuda:
            raise _lib.Gd4dError('refresh_images: the module is not on the GPU (no CPU fallback in graph-detr4d_amd)')
        self._kept_values()
