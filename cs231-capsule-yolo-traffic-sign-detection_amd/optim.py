"""torch.optim.Adam replacement: every parameter updated by ONE multi-tensor HIP launch per step
(csrc/adam.hip).  Same hyper-parameters, state layout ('step', 'exp_avg', 'exp_avg_sq') and update
formula as torch.optim.Adam (main.py:280), so optimizer checkpoints interchange.

Optional, both decided on the device without a host synchronisation (csrc/gradnorm.hip):
  max_grad_norm=X      global-norm clipping: the update uses coef * g with coef = min(1, X / (total_norm + 1e-6)), total_norm over
                       every gradient this step() applies.  Unlike torch.nn.utils.clip_grad_norm_, p.grad itself is NOT rewritten.
  skip_nonfinite=True  a step whose total_norm is not finite (an inf or NaN anywhere in the gradients) changes no bit of any
                       parameter, exp_avg or exp_avg_sq, and a device counter goes up by one.  The host does not learn of the skip
                       (that would be a synchronisation): state['step'], hence the bias corrections of later steps, advance as in
                       any other step.
With both off, step() issues exactly the launches it issues without them and none of their device state exists.

Optional, kept inside the same Adam launch (cy_adam_step's ema_table):
  ema_decay=D          an exponential moving average of every parameter the optimizer updates: ema = d_t * ema + (1 - d_t) * p after
                       each update of p, d_t = D, or with ema_warmup=True d_t = min(D, (1 + t) / (10 + t)) with t the parameter's own
                       step count.  opt.ema[p] starts as a copy of p before p's first step and moves exactly in the steps that update
                       p: not in a step in which p has no gradient, not in a step skip_nonfinite skips.  `with opt.ema_weights():`
                       exchanges every parameter with its average (pointers, no copy) for an evaluation; opt.ema_state_dict(model) /
                       opt.load_ema_state_dict(model, sd) are keyed by the model's parameter names.  opt.ema is an attribute:
                       state_dict() stays torch.optim.Adam's.  Deliberately left out: buffers (BatchNorm running statistics are
                       running averages already: both sets of weights use the live ones) and parameters the optimizer never updates
                       (frozen ones contribute their own values wherever the averaged weights are used).
With ema_decay=None step() issues exactly the launches it issues today and no EMA tensor or table exists."""
import contextlib
import ctypes as C
import math
import numbers

import numpy as np
import torch

from . import ops as _ops
from ._lib import AdamStep, call

_CHUNK = 16384


def _n_chunks(p):
    """Block-map entries (workgroups) of one tensor."""
    return (p.numel() + _CHUNK - 1) // _CHUNK


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, skip_nonfinite=False, ema_decay=None,
                 ema_warmup=False):
        if max_grad_norm is not None:
            if isinstance(max_grad_norm, bool) or not isinstance(max_grad_norm, numbers.Real) or \
                    not math.isfinite(max_grad_norm) or not max_grad_norm > 0:
                raise ValueError('capsyolo_amd.optim.Adam: max_grad_norm must be a positive finite number or None, got %r' % (max_grad_norm,))
        if ema_decay is not None:
            if isinstance(ema_decay, bool) or not isinstance(ema_decay, numbers.Real) or not math.isfinite(ema_decay) or \
                    not 0 < ema_decay < 1:
                raise ValueError('capsyolo_amd.optim.Adam: ema_decay must be a number in (0, 1) or None, got %r' % (ema_decay,))
        elif ema_warmup:
            raise ValueError('capsyolo_amd.optim.Adam: ema_warmup shapes the schedule of ema_decay: give ema_decay')
        # weight_decay and amsgrad are in the group only so that a checkpoint of this optimizer loads into torch.optim.Adam, which
        # reads them from the loaded group; step() refuses any value but torch's default (a checkpoint of torch's may carry one)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=0, amsgrad=False))
        self._plan_key, self._plan = None, None
        self.graph_tables = None     # ... and per group (pinned host, device) pointer tables [n parameters with a gradient][5]
        self.graph_hyper = None      # graph_step.GraphedStep: per group a device tensor of step_scalars()'s six floats, eight with an EMA (cy_adam_step's hyper)
        # attributes, not param_groups entries: state_dict() is that of torch.optim.Adam with or without them
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._clip_buf = None        # device int64[3], made by the first step that needs it: {record as 4 floats, skipped}
        self._partial = None         # device float64[chunks of all parameters]: the sums of squares of cy_grad_sumsq_multi
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        self.ema = {}                # parameter -> its moving average (made by the parameter's first step; empty without ema_decay)
        self.graph_ema_tables = None  # graph_step.GraphedStep: per group (pinned host, device) int64[n]: the EMA pointers of graph_tables' rows
        self._ema_swapped = False    # inside ema_weights(): p.data and ema[p] have changed places

    @property
    def clip_record(self):
        """Device float32[4] = {total_norm, coef, go (1 | 0), 0} of the last step; None before the first step with an option on."""
        return None if self._clip_buf is None else self._clip_buf[:2].view(torch.float32)

    @property
    def skipped_dev(self):
        """Device int64[1]: steps skipped by skip_nonfinite so far; None before the first step with an option on."""
        return None if self._clip_buf is None else self._clip_buf[2:3]

    def _clip_reset(self):
        """record = {0, 1, 1, 0}, skipped = 0: the state before any step (graph_step.GraphedStep after its warm-up steps)."""
        self.clip_record.copy_(torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float32))
        self.skipped_dev.zero_()

    def grad_stats(self):
        """{'norm': total gradient norm of the last step, 'coef': its clipping coefficient, 'skipped': steps skipped so far}.
        ONE device-to-host copy and ONE synchronisation: call it once per epoch (main.py does), not per step."""
        if self.max_grad_norm is None and not self.skip_nonfinite:
            raise RuntimeError('capsyolo_amd.optim.Adam.grad_stats: neither max_grad_norm nor skip_nonfinite is on')
        if self._clip_buf is None:
            return {'norm': 0.0, 'coef': 1.0, 'skipped': 0}
        host = self._clip_buf.cpu()
        rec = host[:2].view(torch.float32)
        return {'norm': float(rec[0]), 'coef': float(rec[1]), 'skipped': int(host[2])}

    def step_scalars(self, group, t):
        """{lr, beta1, beta2, eps, 1 - beta1^t, 1 - beta2^t}: the scalars of step t of a group; with ema_decay two more,
        {1 - d_t, 0}: the difference is formed here in double and rounded to fp32 once, on its way to the kernel."""
        b1, b2 = group['betas']
        out = [float(group['lr']), float(b1), float(b2), float(group['eps']), float(1.0 - b1 ** t), float(1.0 - b2 ** t)]
        if self.ema_decay is not None:
            out += [1.0 - self.ema_decay_at(t), 0.0]
        return out

    def ema_decay_at(self, t):
        """d_t of a parameter's step t (1-based): ema_decay, or with ema_warmup min(ema_decay, (1 + t) / (10 + t))."""
        if self.ema_decay is None:
            raise RuntimeError('capsyolo_amd.optim.Adam.ema_decay_at: ema_decay is off')
        return min(self.ema_decay, (1.0 + t) / (10.0 + t)) if self.ema_warmup else self.ema_decay

    def _model_params(self, model):
        mine = set(p for g in self.param_groups for p in g['params'])
        return [(name, p, p in mine) for name, p in model.named_parameters()]

    def ema_state_dict(self, model):
        """{parameter name of `model`: averaged values}: the average of every parameter that has one, the parameter's own values for the
        others (frozen ones, ones that have not had a step).  Copies; no buffers (they are not averaged)."""
        if self.ema_decay is None:
            raise RuntimeError('capsyolo_amd.optim.Adam.ema_state_dict: ema_decay is off')
        out = {}
        for name, p, _ in self._model_params(model):
            # (inside ema_weights() the two have changed places)
            avg = p if (p not in self.ema or self._ema_swapped) else self.ema[p]
            out[name] = avg.detach().clone()
        return out

    def load_ema_state_dict(self, model, sd):
        """The inverse: the entries of the parameters this optimizer updates become their averages (copied into the tensor an average
        already has: a captured step holds its address); entries of other parameters are ignored."""
        if self.ema_decay is None:
            raise RuntimeError('capsyolo_amd.optim.Adam.load_ema_state_dict: ema_decay is off')
        if self._ema_swapped:
            raise RuntimeError('capsyolo_amd.optim.Adam.load_ema_state_dict: not inside ema_weights()')
        todo = [(name, p) for name, p, mine in self._model_params(model) if mine and p.requires_grad]
        for name, p in todo:
            if name not in sd or tuple(sd[name].shape) != tuple(p.shape):
                raise KeyError('capsyolo_amd.optim.Adam.load_ema_state_dict: no entry %r of shape %s' % (name, tuple(p.shape)))
        with torch.no_grad():
            for name, p in todo:
                if p in self.ema:
                    self.ema[p].copy_(sd[name])
                else:
                    self.ema[p] = sd[name].detach().to(device=p.device, dtype=p.dtype, copy=True).contiguous()
        self._plan_key = None

    @contextlib.contextmanager
    def ema_weights(self):
        """`with opt.ema_weights():` every parameter that has an average holds it (p.data and opt.ema[p] change places: two pointers,
        no copy); on exit the parameters are the tensors, with the bits, they were.  For an evaluation or a state_dict() of the averaged
        model; step() is refused inside.  The eval-mode fold caches (ops.fold_eval_bn) are keyed on ops' parameter epoch, which is moved
        on entry and on exit."""
        if self.ema_decay is None:
            raise RuntimeError('capsyolo_amd.optim.Adam.ema_weights: ema_decay is off')
        if self._ema_swapped:
            raise RuntimeError('capsyolo_amd.optim.Adam.ema_weights: already inside')
        if self.graph_hyper is not None or (torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()):
            raise RuntimeError('capsyolo_amd.optim.Adam.ema_weights: a captured step is being recorded (it holds the parameters\' addresses)')
        self._swap_ema()
        try:
            yield self
        finally:
            self._swap_ema()

    def _swap_ema(self):
        for p, avg in list(self.ema.items()):
            live = p.data
            p.data = avg
            self.ema[p] = live
        self._ema_swapped = not self._ema_swapped
        self._plan_key = None
        _ops._bump_param_epoch()

    def _upload(self, entries, table, ema_table):
        """The rows of `entries` into a (pinned host, device) pair of pointer tables [n][5], and the pointers of their averages into a
        pair [n] where there is one: filled on the host, copied asynchronously on the step's stream."""
        host, dev = table
        host.numpy()[...] = np.asarray([(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel())
                                        for p, g, m, v in entries], dtype=np.int64)
        dev.copy_(host, non_blocking=True)
        if ema_table is not None:
            host, dev = ema_table
            host.numpy()[...] = np.asarray([self.ema[p].data_ptr() for p, _, _, _ in entries], dtype=np.int64)
            dev.copy_(host, non_blocking=True)

    def _build_plan(self, entries, device):
        """Pointer table + block map on the device.  The block map depends on the sizes only and is uploaded once; the
        table (the gradient tensors are new allocations every step) goes through a small ring of pinned staging buffers
        with an asynchronous copy on the step's stream: no host synchronisation in the step."""
        blocks = []
        for k, (p, g, m, v) in enumerate(entries):
            blocks.extend((k, c) for c in range(_n_chunks(p)))
        sizes = tuple(e[0].numel() for e in entries)
        if getattr(self, '_bm_key', None) != (sizes, device):
            bm = np.asarray(blocks, dtype=np.int32).reshape(-1, 2)
            self._bm, self._bm_key = torch.from_numpy(bm).to(device), (sizes, device)
            self._table_dev = torch.empty((len(entries), 5), dtype=torch.int64, device=device)
            self._ring = [torch.empty((len(entries), 5), dtype=torch.int64).pin_memory() for _ in range(4)]
            self._ring_events = [None] * 4
            self._ring_pos = 0
            self._ema_table_dev, self._ema_ring = None, None
        if self.ema_decay is not None and self._ema_table_dev is None:
            # the averages' pointers: a second table (the layout of the first stays [n][5]) with a ring of its own
            self._ema_table_dev = torch.empty(len(entries), dtype=torch.int64, device=device)
            self._ema_ring = [torch.empty(len(entries), dtype=torch.int64).pin_memory() for _ in range(4)]
        k = self._ring_pos
        self._ring_pos = (k + 1) % 4
        if self._ring_events[k] is not None:
            self._ring_events[k].synchronize()           # four steps old: long done
        self._upload(entries, (self._ring[k], self._table_dev),
                     (self._ema_ring[k], self._ema_table_dev) if self.ema_decay is not None else None)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        self._ring_events[k] = ev
        return (self._table_dev, self._bm, len(blocks))

    def _tables(self, group, entries):
        """(pointer table, block map, number of blocks) of one launch, uploaded on the step's stream."""
        if self.graph_hyper is not None:
            # inside a captured step (graph_step.GraphedStep): the pointer table is a tensor of the graph's own (uploaded by a
            # captured copy from a pinned buffer that nothing else writes), the block map is the eager plan's (same sizes:
            # the warm-up steps built it), the scalars come from device memory
            sizes = tuple(e[0].numel() for e in entries)
            if getattr(self, '_bm_key', None) != (sizes, entries[0][0].device):
                raise RuntimeError('capsyolo_amd.optim.Adam: capture a step only after an eager step with the same parameters')
            # (pinned and device buffers made by GraphedStep BEFORE the capture: pinning memory is not a capturable operation)
            host, table = self.graph_tables[id(group)]
            if tuple(host.shape) != (len(entries), 5):
                raise RuntimeError('capsyolo_amd.optim.Adam: the captured step updates %d parameters, its table was made for %d'
                                   % (len(entries), host.shape[0]))
            ema_pair = None
            if self.ema_decay is not None:
                if self.graph_ema_tables is None or tuple(self.graph_ema_tables[id(group)][0].shape) != (len(entries),):
                    raise RuntimeError('capsyolo_amd.optim.Adam: the captured step has no table for the %d EMA pointers' % len(entries))
                ema_pair = self.graph_ema_tables[id(group)]
            self._upload(entries, (host, table), ema_pair)
            nblocks = sum(_n_chunks(p) for p, _, _, _ in entries)
            return (table, self._bm, nblocks)
        key = tuple(x.data_ptr() for e in entries for x in e)
        if self.ema_decay is not None:
            key += tuple(self.ema[e[0]].data_ptr() for e in entries)
        if key != self._plan_key:
            self._plan, self._plan_key = self._build_plan(entries, entries[0][0].device), key
        return self._plan

    def _ema_table(self, group):
        """The device table of EMA pointers that belongs to the table _tables(group, ...) has just uploaded."""
        return self.graph_ema_tables[id(group)][1] if self.graph_hyper is not None else self._ema_table_dev

    def _grad_verdict(self, launches, stream):
        """The sums of squares of every launch's gradients into consecutive slices of one partial buffer, then ONE
        cy_grad_clip_finish: the record that every Adam launch of this step reads.  Returns the launches' tables where they are
        still valid for the Adam launches (one launch, or the captured step's per-group tables), else None."""
        dev = launches[0][2][0][0].device
        need = sum(_n_chunks(p) for _, _, entries in launches for p, _, _, _ in entries)
        if self._clip_buf is None:
            self._clip_buf = torch.zeros(3, dtype=torch.int64, device=dev)
            self._clip_reset()
        if self._partial is None or self._partial.numel() < need:
            # once: room for every parameter of every group (each is in at most one launch of a step)
            every = sum(_n_chunks(p) for g in self.param_groups for p in g['params'])
            self._partial = torch.empty(max(need, every), dtype=torch.float64, device=dev)
        tables, off = [], 0
        for group, _, entries in launches:
            table, bm, nblocks = self._tables(group, entries)
            call('cy_grad_sumsq_multi', C.c_void_p(table.data_ptr()), C.c_void_p(bm.data_ptr()), nblocks, _CHUNK,
                 C.c_void_p(self._partial.data_ptr() + 8 * off), stream)
            tables.append((table, bm, nblocks))
            off += nblocks
        call('cy_grad_clip_finish', C.c_void_p(self._partial.data_ptr()), off,
             0.0 if self.max_grad_norm is None else self.max_grad_norm, int(self.skip_nonfinite),
             C.c_void_p(self.clip_record.data_ptr()), C.c_void_p(self.skipped_dev.data_ptr()), stream)
        # the eager plan is ONE device table that the next launch's upload overwrites
        return tables if self.graph_hyper is not None or len(launches) == 1 else None

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        if self._ema_swapped:
            raise RuntimeError('capsyolo_amd.optim.Adam.step: inside ema_weights() the parameters hold their averages; leave it first')
        ema = self.ema_decay is not None
        launches = []
        for group in self.param_groups:
            if group.get('weight_decay', 0) != 0 or group.get('amsgrad', False) or group.get('maximize', False):
                raise RuntimeError('capsyolo_amd.optim.Adam implements plain Adam only: weight_decay, amsgrad and maximize must be off')
            by_step = {}
            for p in group['params']:
                if p.grad is None:
                    continue
                if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                    raise RuntimeError('capsyolo_amd.optim.Adam needs contiguous float32 GPU parameters')
                st = self.state[p]
                if len(st) == 0:
                    st['step'] = 0
                    st['exp_avg'] = torch.zeros_like(p)
                    st['exp_avg_sq'] = torch.zeros_like(p)
                st['step'] = int(st['step']) + 1
                if ema and p not in self.ema:
                    self.ema[p] = p.detach().clone()      # the parameter before its first step
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                by_step.setdefault(st['step'], []).append((p, g, st['exp_avg'], st['exp_avg_sq']))
            if self.graph_hyper is not None and len(by_step) > 1:
                raise RuntimeError('capsyolo_amd.optim.Adam: the parameters of a captured step must share their step count')
            # one launch per step count: a parameter that had no gradient in some step lags behind the others of its group, and
            # the bias corrections are those of its own count (as in torch.optim.Adam)
            launches.extend((group, t, entries) for t, entries in by_step.items())
        if not launches:
            return loss
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        clip = self.max_grad_norm is not None or self.skip_nonfinite
        tables = self._grad_verdict(launches, stream) if clip else None
        for k, (group, t, entries) in enumerate(launches):
            table, bm, nblocks = tables[k] if tables is not None else self._tables(group, entries)
            a = AdamStep(table=table.data_ptr(), blockmap=bm.data_ptr(), n_blocks=nblocks, chunk=_CHUNK)
            if ema:
                a.ema_table = self._ema_table(group).data_ptr()
            if clip:
                a.record = self.clip_record.data_ptr()
            if self.graph_hyper is not None:
                hyper = self.graph_hyper[id(group)]
                if hyper.numel() != (8 if ema else 6):
                    raise RuntimeError('capsyolo_amd.optim.Adam: the captured step\'s scalars are %d floats, this step reads %d'
                                       % (hyper.numel(), 8 if ema else 6))
                a.hyper = hyper.data_ptr()
            else:
                scalars = self.step_scalars(group, t)
                a.lr, a.beta1, a.beta2, a.eps, a.bias_corr1, a.bias_corr2 = scalars[:6]
                if ema:
                    a.one_minus_decay = scalars[6]
            # the label says what was launched: it is read off the descriptor, not off the options
            label = 'cy_adam_step' + ('+dev' if a.hyper else '') + ('+clip' if a.record else '') + ('+ema' if a.ema_table else '')
            call('cy_adam_step', C.byref(a), stream, trace=label)
            _ops._bump_param_epoch()          # parameters changed through raw pointers: eval-mode fold caches are stale
        return loss
