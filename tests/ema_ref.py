"""The moving-average rule of capsyolo_amd.optim.Adam(ema_decay=..., ema_warmup=...) (include/capsyolo_hip.h) in
float64 torch on the CPU, around clip_ref.ClipRef (clip_grad_norm_ + torch.optim.Adam on double copies):

    a parameter's average starts as a copy of the parameter before its first step;
    after each step, for exactly the parameters that step UPDATED:  ema = d_t * ema + (1 - d_t) * p,
    d_t = ema_decay, or with ema_warmup min(ema_decay, (1 + t) / (10 + t)), t = the parameter's own step count after the step;
    a parameter without a gradient in a step is not updated, and a step that skip_nonfinite skips updates none (its step counts
    advance all the same, as on the device, which cannot tell the host of the skip).

Also the shared recipe of the EMA tests: the 8 tensors, two groups and gradients of tests/test_gpu_adam.py (parameter 2 without a gradient in
steps 1, 4, 7, ...; the learning rate cut tenfold after step 10) over 30 steps, and for the guard test one element made inf in step 5
and one made NaN in step 11."""
import torch

import clip_ref
import test_gpu_adam as A

STEPS = A.STEPS
LR_CUT_AFTER = 10
POISON = {5: (7, 70000, float('inf')),       # the last element of the 70001 tensor (its tail chunk)
          11: (4, 0, float('nan'))}          # the first element of the 16384 tensor
has_grad = clip_ref.has_grad


def recipe_grad(k, t, poison=False):
    """fp32 gradient of parameter k in step t (1-based): test_gpu_adam's, with POISON's element replaced when asked."""
    g = A._grad(k, t).clone()
    if poison and t in POISON and POISON[t][0] == k:
        g.view(-1)[POISON[t][1]] = POISON[t][2]
    return g


def decay_at(ema_decay, ema_warmup, t):
    return min(ema_decay, (1.0 + t) / (10.0 + t)) if ema_warmup else ema_decay


def warmup_end(ema_decay):
    """The first step count at which the warm-up schedule has reached ema_decay: (1 + t) / (10 + t) >= D  <=>  t >= (10 D - 1) / (1 - D)."""
    t = 1
    while (1.0 + t) / (10.0 + t) < ema_decay:
        t += 1
    return t


class EmaTracker(object):
    """The rule alone, in the dtype of the tensors it is given: ema[p] for every parameter it has seen."""

    def __init__(self, ema_decay, ema_warmup=False):
        self.ema_decay, self.ema_warmup, self.ema = ema_decay, ema_warmup, {}

    def before_step(self, params):
        for p in params:
            if p not in self.ema:
                self.ema[p] = p.detach().clone()

    def after_update(self, p, t):
        d = decay_at(self.ema_decay, self.ema_warmup, t)
        self.ema[p] = d * self.ema[p] + (1.0 - d) * p.detach()


class EmaRef(object):
    """ref = EmaRef(param_groups of float64 Parameters, ema_decay, ema_warmup, max_norm or None, skip_nonfinite); set .grad (float64)
    and call ref.step(); ref.ema[p] is the average.  more: further (ema_decay, ema_warmup) pairs followed along the SAME Adam
    trajectory (the average does not act back on it): ref.trackers[1:]."""

    def __init__(self, param_groups, ema_decay, ema_warmup=False, max_norm=None, skip_nonfinite=False, more=()):
        self.inner = clip_ref.ClipRef(param_groups, max_norm, skip_nonfinite)
        self.trackers = [EmaTracker(ema_decay, ema_warmup)] + [EmaTracker(d, w) for d, w in more]

    @property
    def ema(self):
        return self.trackers[0].ema

    @property
    def state(self):
        return self.inner.state

    @property
    def param_groups(self):
        return self.inner.param_groups

    @property
    def skipped(self):
        return self.inner.skipped

    def step(self):
        ps = [p for g in self.inner.param_groups for p in g['params'] if p.grad is not None]
        for tr in self.trackers:
            tr.before_step(ps)
        skipped = self.inner.skipped
        self.inner.step()
        if self.inner.skipped != skipped:
            return                                   # nothing was updated
        for p in ps:
            t = int(self.inner.state[p]['step'])
            for tr in self.trackers:
                tr.after_update(p, t)
