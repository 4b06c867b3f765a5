"""The clipping / non-finite-guard rule of capsyolo_amd.optim.Adam (include/capsyolo_hip.h) in float64 torch on the
CPU: torch.nn.utils.clip_grad_norm_ + torch.optim.Adam on double copies of the parameters and gradients.

    total_norm = sqrt(sum over every gradient of this step of g^2);  coef = min(1, max_norm / (total_norm + 1e-6))
    the Adam update sees coef * g;  skip_nonfinite and a non-finite total_norm: no update, but state['step'] += 1 for every
    parameter that has a gradient (the device cannot tell the host of the skip without a synchronisation), and skipped += 1.

Also the shared recipe of the clipping tests: the 8 tensors of tests/test_gpu_adam.py (sizes 1 .. 70001, parameter 2 without a gradient in
steps 1, 4, 7, ...) with that file's gradients x BASE, and x 50 more on even steps.  BASE = 2^-9 (exact in fp32) is there because the
gradients of test_gpu_adam._grad have a total norm of about 270 as they are (the 16383- and 70001-element tensors are standard
normal): against max_norm = 1.0 every step would clip.  With it the odd steps have a norm near 0.53 (no clipping, coef exactly 1)
and the even ones near 26 (clipping): test_clip_host.py asserts that both cases occur."""
import math

import torch

import test_gpu_adam as A

BASE = 2.0 ** -9
MAX_NORM = 1.0


def recipe_grad(k, t):
    """fp32 gradient of parameter k in step t (1-based) of the clipping recipe."""
    return A._grad(k, t) * (BASE * (50.0 if t % 2 == 0 else 1.0))


def has_grad(k, t):
    return not (k == 2 and t % 3 == 1)


class ClipRef(object):
    """ref = ClipRef(param_groups of float64 Parameters, max_norm or None, skip_nonfinite); set .grad (float64) and call ref.step()."""

    def __init__(self, param_groups, max_norm=None, skip_nonfinite=False):
        self.opt = torch.optim.Adam(param_groups)
        self.max_norm, self.skip_nonfinite = max_norm, skip_nonfinite
        self.skipped, self.norm, self.coef = 0, None, None

    @property
    def state(self):
        return self.opt.state

    @property
    def param_groups(self):
        return self.opt.param_groups

    def step(self):
        ps = [p for g in self.opt.param_groups for p in g['params'] if p.grad is not None]
        if not ps:
            return
        assert all(p.grad.dtype == torch.float64 for p in ps)
        self.norm = math.sqrt(sum(float((p.grad * p.grad).sum()) for p in ps))
        self.coef = 1.0 if self.max_norm is None else min(1.0, self.max_norm / (self.norm + 1e-6))
        if self.skip_nonfinite and not math.isfinite(self.norm):
            self.skipped += 1
            for p in ps:
                st = self.opt.state[p]
                if len(st) == 0:                       # as torch.optim.Adam makes it in a parameter's first step
                    st['step'] = torch.tensor(0.0, dtype=torch.get_default_dtype())
                    st['exp_avg'], st['exp_avg_sq'] = torch.zeros_like(p), torch.zeros_like(p)
                st['step'] += 1
            return
        if self.max_norm is not None:
            torch.nn.utils.clip_grad_norm_(ps, self.max_norm)       # rewrites the double copies; the device leaves p.grad alone
        self.opt.step()
