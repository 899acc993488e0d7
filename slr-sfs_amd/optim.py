"""The optimiser step of the reference's trainer (models/base_model.py:15-46, 80-93) on the package's kernel.

``Adam`` is ``torch.optim.Adam(params, lr, betas, eps)`` -- no weight decay, no amsgrad, what the reference runs -- as a
``torch.optim.Optimizer`` whose ``step()`` is ``slr_adam_step`` (csrc/adam.hip): every parameter of a group in two launches, whatever
their number, from a plan in device memory that is rebuilt only when a parameter's or a gradient's address changes.  The state keeps
torch's names and shapes (``step`` a float32 device scalar, ``exp_avg``, ``exp_avg_sq``): state dicts go both ways between the two
classes.  Nothing in ``step()`` synchronises the host.  ``TrainingOptimizers`` is the reference's pair of optimisers with its betas
rule, its learning-rate decay and its checkpoint keys.  There is no fallback: CPU parameters raise, a missing library raises.
"""
import ctypes

import numpy as np
import torch

from ._lib import call, check, lib, require_device
from .training import _has

ZERO_GRADS = 1                                           # include/slr_splat.h: SLR_ADAM_ZERO_GRADS
_NOT_OFFERED = ("weight_decay", "amsgrad", "maximize")   # torch.optim.Adam's options the reference leaves at their defaults


def _require_parameter(t, what="parameter"):
    """float32, ROCm, contiguous -- the error types of ``_lib.require_device``, the dtype first (a float64 tensor is refused as such
    wherever it lives)."""
    if not torch.is_tensor(t):
        raise TypeError(f"slr_sfs_amd.Adam: {what}s are tensors, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise TypeError(f"slr_sfs_amd: float32 tensors required, got {t.dtype}")
    if t.is_sparse:
        raise TypeError(f"slr_sfs_amd.Adam: dense {what}s required")
    require_device(t)


class Adam(torch.optim.Optimizer):
    """``torch.optim.Adam`` for float32, contiguous parameters on a ROCm device.  ``lr`` is a number or a one-element float32 device
    tensor, which is then used as it is.  ``step(zero_grads=True)`` also writes zeros to every gradient it has read (``zero_grad`` fused
    into the step: the gradient tensors stay, and with them the plan).  Parameters whose ``.grad`` is None are skipped and their ``step``
    does not advance.  After the launch the version counter of every stepped parameter is advanced: whatever is cached per
    ``(data_ptr, _version)`` of a weight (``nets._cached``) is made again."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        if not torch.is_tensor(lr) and not lr >= 0.0:
            raise ValueError(f"Adam: lr {lr}")
        if len(betas) != 2 or not all(0.0 <= float(b) < 1.0 for b in betas):
            raise ValueError(f"Adam: betas {betas}, each in [0, 1)")
        if not eps > 0.0:
            raise ValueError(f"Adam: eps {eps} (> 0)")
        self._plans, self._lrs = {}, {}
        # (the three options that are not offered stay in the groups at torch's defaults: torch.optim.Adam reads them from a loaded state dict)
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0, amsgrad=False, maximize=False))

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        try:
            self._check_group(group)
            for p in group["params"]:
                _require_parameter(p)
        except Exception:
            self.param_groups.pop()
            raise

    @staticmethod
    def _check_group(group):
        for name in _NOT_OFFERED:
            if group.get(name):
                raise TypeError(f"slr_sfs_amd.Adam has no {name} (the reference's trainer uses none): got {group[name]!r}")

    # ---- the plan of a group: rebuilt when an address changes
    def _plan(self, index, params, key):
        plan = self._plans.get(index)
        if plan is not None and plan["key"] == key:
            return plan
        device = params[0].device
        rows = []
        for p in params:
            g = p.grad
            _require_parameter(p)
            _require_parameter(g, "gradient")
            if p.device != device or g.device != device or g.shape != p.shape:
                raise ValueError("slr_sfs_amd.Adam: the parameters of a group and their gradients share one device, a gradient has its parameter's shape")
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.zeros((), dtype=torch.float32, device=device)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            rows.append((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), st["step"].data_ptr()))
        n = len(params)
        addr = np.ascontiguousarray(np.array(rows, dtype=np.uint64).T)          # [5][n]
        numel = np.array([p.numel() for p in params], dtype=np.int64)
        nbytes = int(lib().slr_adam_plan_bytes(n, numel.ctypes.data))
        host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)          # a fresh pinned block per plan: an earlier upload may be in flight
        check(lib().slr_adam_plan_fill(host.data_ptr(), nbytes, n, *(addr[k].ctypes.data for k in range(5)), numel.ctypes.data),
              "slr_adam_plan_fill")
        n_work = int(host.numpy()[12:16].view(np.uint32)[0])
        dev = torch.empty(nbytes, dtype=torch.uint8, device=device)
        dev.copy_(host, non_blocking=True)
        plan = self._plans[index] = dict(key=key, dev=dev, host=host, n=n, n_work=n_work)
        return plan

    def _lr(self, index, group, device):
        lr = group["lr"]
        if torch.is_tensor(lr):
            _require_parameter(lr, "learning rate")
            if lr.numel() != 1 or lr.device != device:
                raise ValueError("slr_sfs_amd.Adam: a tensor lr has one element and lives on the parameters' device")
            return lr
        kept = self._lrs.get(index)
        if kept is None or kept[1].device != device:
            kept = self._lrs[index] = [lr, torch.full((1,), float(lr), dtype=torch.float32, device=device)]
        elif kept[0] != lr:
            kept[0] = lr
            kept[1].fill_(float(lr))
        return kept[1]

    @torch.no_grad()
    def step(self, closure=None, zero_grads=False):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for index, group in enumerate(self.param_groups):
            params, key = [], []
            for p in group["params"]:
                g = p.grad
                if g is not None:
                    params.append(p)
                    key.append(p.data_ptr())
                    key.append(g.data_ptr())
            if not params:
                continue
            self._check_group(group)
            plan = self._plan(index, params, tuple(key))
            device = params[0].device
            betas = (ctypes.c_double * 2)(*group["betas"])
            call("slr_adam_step", device, plan["dev"], plan["n"], plan["n_work"], self._lr(index, group, device), betas,
                 float(group["eps"]), ZERO_GRADS if zero_grads else 0)
            torch.autograd.graph.increment_version(params)
        return loss

    def load_state_dict(self, state_dict):
        """Torch's, then the state as the kernel wants it: ``step`` (a number or a CPU tensor in old checkpoints) becomes a float32 device
        scalar, the moments contiguous float32 tensors of this optimiser's own."""
        super().load_state_dict(state_dict)
        self._plans.clear()
        self._lrs.clear()
        for group in self.param_groups:
            self._check_group(group)
        for p, st in self.state.items():
            if len(st) == 0:
                continue
            st["step"] = torch.as_tensor(st["step"], dtype=torch.float32).reshape(()).to(p.device).clone()
            for name in ("exp_avg", "exp_avg_sq"):
                st[name] = st[name].to(device=p.device, dtype=torch.float32).clone(memory_format=torch.contiguous_format)


def _value(opts, name, default):
    """``opts.name`` of an argparse.Namespace or a dict; ``default`` (the reference's, options/train_options.py:348-387) where it has none."""
    if not _has(opts, name):
        return default
    return opts[name] if isinstance(opts, dict) else getattr(opts, name)


class TrainingOptimizers:
    """The optimisers of ``BaseModel.__init__`` (models/base_model.py:15-46) and its ``update_learning_rate`` (:80-93).
    With ``discriminator_params`` (the reference's ``discriminator_losses != '0'``): ``optimizer_D`` at ``lr_d`` and ``optimizer_G`` at
    ``lr_g``, both with betas ``(beta1, beta2)``; without: ``optimizer_G`` alone with ``(0.99, beta2)``.  ``opts``: the training
    Namespace (or a dict); what it lacks takes the reference's default (beta1 0, beta2 0.9, lr_g 5e-4, lr_d 2e-3, niter_decay 10)."""

    def __init__(self, generator_params, discriminator_params=None, opts=None):
        beta1, beta2 = _value(opts, "beta1", 0.0), _value(opts, "beta2", 0.9)
        self.lr_g, self.lr_d = _value(opts, "lr_g", 1e-3 / 2), _value(opts, "lr_d", 1e-3 * 2)
        self.niter_decay = _value(opts, "niter_decay", 10)
        self.use_discriminator = discriminator_params is not None
        self.optimizer_D = None
        if self.use_discriminator:
            self.optimizer_D = Adam(list(discriminator_params), lr=self.lr_d, betas=(beta1, beta2))
            self.optimizer_G = Adam(list(generator_params), lr=self.lr_g, betas=(beta1, beta2))
        else:
            self.optimizer_G = Adam(list(generator_params), lr=self.lr_g, betas=(0.99, beta2))

    def update_learning_rate(self):
        """Once per epoch of the decay phase: lr <- lr - lr / niter_decay, the reference's arithmetic."""
        lr_g = self.lr_g - self.lr_g / self.niter_decay
        for group in self.optimizer_G.param_groups:
            group["lr"] = lr_g
        self.lr_g = lr_g
        if self.use_discriminator:
            lr_d = self.lr_d - self.lr_d / self.niter_decay
            for group in self.optimizer_D.param_groups:
                group["lr"] = lr_d
            self.lr_d = lr_d

    def state_dict(self):
        """The optimiser entries of the reference's checkpoint: ``optimizerG`` and, with a discriminator, ``optimizerD``."""
        sd = {"optimizerG": self.optimizer_G.state_dict()}
        if self.use_discriminator:
            sd["optimizerD"] = self.optimizer_D.state_dict()
        return sd

    def load_state_dict(self, checkpoint):
        """From a checkpoint of the reference (``torch.optim.Adam`` state dicts) or of ``state_dict()``; other keys are ignored."""
        self.optimizer_G.load_state_dict(checkpoint["optimizerG"])
        if self.use_discriminator:
            self.optimizer_D.load_state_dict(checkpoint["optimizerD"])
