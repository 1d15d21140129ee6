"""Adam over one flat arena (ref: SISR/models/__init__.py:299-308 `optim.Adam(params, lr, betas)`, stepped by
standard_update :481-489).

torch's Adam walks ~2 400 parameter tensors of a QRCAN with seven multi-tensor kernels chunked into ~190 launches and
~14 ms of host work per step.  Here parameters, gradients and both moment estimates live in four flat fp32 arenas laid
out alike; every nn.Parameter / .grad / state tensor is a view into them, so the update is ONE launch of
`sisr_adam_flat` (csrc/misc.hip, torch's operation order) and nothing is gathered:
  * conv weight gradients are written into the gradient arena by the weight-gradient kernels themselves
    (ops.GRAD_SINK), the small remaining gradients are copied in by one multi-tensor copy;
  * a data-parallel GradReducer all-reduces slices of the same arena (parallel.py), no bucket copies.
It IS a torch.optim.Adam: param_groups, state and state_dict() keep torch's schema ({'step', 'exp_avg',
'exp_avg_sq'} per parameter that has received a gradient), so checkpoints interchange with the reference, and LR
schedulers drive it through param_groups[0]['lr'].  Parameters that get no gradient in a step are skipped exactly as
torch skips them (their range is left out of the launch).  CUDA (HIP) parameters only; on CPU the handlers fall back to
constructing a plain torch Adam, which is never stepped (the networks refuse CPU tensors).

Three optional parts of the step, all off by default (csrc/update.hip), none of them in the reference:
  * max_norm: torch.nn.utils.clip_grad_norm_ on the device.  The global norm is an ordered float64 reduction over the ranges
    of the gradient arena the step is about to update (one launch per range + one), and the update kernel reads the clip
    coefficient from device memory: no host synchronisation, no walk over the parameter tensors.
  * weight_decay: the decoupled (AdamW) form, p *= 1 - lr * weight_decay ahead of the Adam update, in the same pass.
  * ema_decay: a fifth arena flat_e with an exponential moving average of the weights, e += (p - e)(1 - ema_decay) after
    every step for every parameter, in the same pass (ranges Adam skips get an average-only launch).
With none of them set step() issues exactly the launches it always has (sisr_adam_flat).
"""
import math

import torch
from torch import optim

from . import hip

ALIGN = 4  # floats: every parameter starts on a 16-byte boundary


class FlatAdam(optim.Adam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, late=(), weight_decay=0.0, max_norm=None,
                 ema_decay=None):
        """late: parameters whose gradients only arrive at the very end of a backward pass (the meta-attention layers, whose
        gates are all computed -- and differentiated -- by one launch before the first block).  They are laid out BEHIND
        the others in the arenas, so that a data-parallel reducer's buckets (contiguous runs of the gradient arena) of conv
        weights complete, and can be all-reduced, while backward is still running.  The arena order is internal:
        param_groups, state and state_dict() keep the registration order.
        weight_decay: decoupled (AdamW); it lives in param_groups[0] (with decoupled_weight_decay=True) and so travels in
        state_dict() as torch's does.  max_norm: clip the global gradient norm of each step to it (grad_norm, clip_coef:
        device tensors of the last step, never read by the step itself).  ema_decay: keep an average of the weights
        (ema_state / load_ema)."""
        params = list(params)
        if not math.isfinite(weight_decay):
            raise ValueError("Invalid weight_decay value: %r" % (weight_decay,))
        if max_norm is not None and not (max_norm > 0 and math.isfinite(max_norm)):
            raise ValueError("max_norm must be a positive finite number; got %r" % (max_norm,))
        if ema_decay is not None and not 0.0 <= ema_decay < 1.0:
            raise ValueError("ema_decay must be in [0, 1); got %r" % (ema_decay,))
        if weight_decay:
            super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled_weight_decay=True)
        else:
            super().__init__(params, lr=lr, betas=betas, eps=eps)
        if len(self.param_groups) != 1:
            raise NotImplementedError("FlatAdam keeps one parameter group (the reference never uses more)")
        ps = self.param_groups[0]['params']
        if not ps or not all(p.is_cuda and p.dtype == torch.float32 for p in ps):
            raise RuntimeError("FlatAdam needs fp32 parameters on a HIP device")
        dev = ps[0].device
        self.offsets, off = {}, 0
        late_ids = {id(p) for p in late}
        self.arena_order = [p for p in ps if id(p) not in late_ids] + [p for p in ps if id(p) in late_ids]
        for p in self.arena_order:
            self.offsets[p] = off
            off += (p.numel() + ALIGN - 1) // ALIGN * ALIGN
        self.total = off
        # The alignment padding between parameters is zero in every arena and never written by anything but the update
        # kernels, which map zeros to zeros (g = m = v = p = e = 0 stays 0): a range that includes padding therefore sums
        # to the same gradient norm as its parameters alone.
        self.flat_p = torch.zeros(off, device=dev)
        self.flat_g = torch.zeros(off, device=dev)
        self.flat_m = torch.zeros(off, device=dev)
        self.flat_v = torch.zeros(off, device=dev)
        with torch.no_grad():
            for p in ps:
                view = self._view(self.flat_p, p)
                view.copy_(p.data)
                p.data = view
        self.grad_views = {p: self._view(self.flat_g, p) for p in ps}
        from . import ops
        for p, view in self.grad_views.items():  # gradients the kernels can produce straight into the arena
            ops.GRAD_SINK[p.data_ptr()] = view
        self._t = 0          # steps taken
        self._missed = {}    # parameter -> number of those steps it had no gradient in (torch counts per parameter)
        self._plan = None    # (frozenset of skipped parameters, [(offset, length, step count)])
        self.max_norm, self.ema_decay = max_norm, ema_decay
        self.flat_e = self.grad_norm = self.grad_norm32 = self.clip_coef = None
        if max_norm is not None:
            L = hip.lib()
            # partial sums of the norm: a merged range never needs more than its parameters' ranges one by one
            parts = sum(L.sisr_sumsq_workspace_bytes((p.numel() + ALIGN - 1) // ALIGN * ALIGN) // 8 for p in ps)
            self._norm_ws = torch.zeros(parts, device=dev, dtype=torch.float64)
            self._norm64 = torch.zeros(1, device=dev, dtype=torch.float64)
            self._norm32 = torch.tensor([0.0, 1.0], device=dev)
            self.grad_norm, self.grad_norm32, self.clip_coef = self._norm64[0], self._norm32[0], self._norm32[1]
        if ema_decay is not None:
            self.flat_e = self.flat_p.clone()
            self._skip_plan = None  # (frozenset of skipped parameters, [(offset, length)])

    def _view(self, flat, p):
        o = self.offsets[p]
        return flat[o:o + p.numel()].view_as(p)

    # -- state in torch's schema, created when a parameter first receives a gradient (as torch's _init_group does)
    def _ensure_state(self, p):
        st = self.state[p]
        if len(st) == 0:
            st['step'] = torch.tensor(0.0, dtype=torch.float32)
            st['exp_avg'] = self._view(self.flat_m, p)
            st['exp_avg_sq'] = self._view(self.flat_v, p)
            self._missed[p] = self._t  # it has missed every step so far

    def _segments(self, skipped):
        skip = frozenset(id(p) for p in skipped)  # identity: `in` on tensors would compare element-wise
        key = (skip, tuple(self._missed.values()) if any(self._missed.values()) else ())
        if self._plan is not None and self._plan[0] == key:
            return self._plan[1]
        segs = []
        for p in self.arena_order:
            if id(p) in skip:
                continue
            o, n = self.offsets[p], (p.numel() + ALIGN - 1) // ALIGN * ALIGN
            missed = self._missed.get(p, 0)
            if segs and segs[-1][0] + segs[-1][1] == o and segs[-1][2] == missed:
                segs[-1][1] += n
            else:
                segs.append([o, n, missed])
        self._plan = (key, segs)
        return segs

    def _skipped_ranges(self, skipped):
        """the arena ranges of the parameters a step leaves out, contiguous ones merged"""
        key = frozenset(id(p) for p in skipped)
        if self._skip_plan is not None and self._skip_plan[0] == key:
            return self._skip_plan[1]
        segs = []
        for p in self.arena_order:
            if id(p) not in key:
                continue
            o, n = self.offsets[p], (p.numel() + ALIGN - 1) // ALIGN * ALIGN
            if segs and segs[-1][0] + segs[-1][1] == o:
                segs[-1][1] += n
            else:
                segs.append([o, n])
        self._skip_plan = (key, segs)
        return segs

    # -- the average of the weights
    def ema_state(self):
        """{index of the parameter in param_groups[0]['params']: view of its average in flat_e} (state_dict()'s indices)"""
        if self.flat_e is None:
            raise RuntimeError("this FlatAdam keeps no average of the weights (ema_decay is None)")
        return {k: self._view(self.flat_e, p) for k, p in enumerate(self.param_groups[0]['params'])}

    @torch.no_grad()
    def load_ema(self, averages=None):
        """averages: {index: tensor} as ema_state() returns it (or a sequence in that order); None: restart the average
        from the parameters as they are"""
        if self.flat_e is None:
            raise RuntimeError("this FlatAdam keeps no average of the weights (ema_decay is None)")
        if averages is None:
            self.flat_e.copy_(self.flat_p)
            return
        items = averages.items() if isinstance(averages, dict) else enumerate(averages)
        views = self.ema_state()
        items = list(items)
        if sorted(k for k, _ in items) != sorted(views):
            raise ValueError("load_ema: expected one average per parameter (%d), got %d" % (len(views), len(items)))
        for k, t in items:
            views[k].copy_(t.reshape(views[k].shape))

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise NotImplementedError("FlatAdam.step takes no closure")
        group = self.param_groups[0]
        lr, (b1, b2), eps = group['lr'], group['betas'], group['eps']
        wd = group.get('weight_decay', 0)
        if (wd and not group.get('decoupled_weight_decay')) or group.get('amsgrad') or group.get('maximize'):
            raise NotImplementedError("FlatAdam implements Adam with decoupled (AdamW) weight decay only (no L2-form weight "
                                      "decay / amsgrad / maximize)")
        skipped, src, dst = [], [], []
        for p in group['params']:
            g = p.grad
            if g is None:
                skipped.append(p)
                continue
            if len(self.state[p]) == 0:
                self._ensure_state(p)
            view = self.grad_views[p]
            if g.data_ptr() != view.data_ptr():
                src.append(g)
                dst.append(view)
        if dst:
            torch._foreach_copy_(dst, src)
        self._t += 1
        for p in skipped:
            if p in self._missed:
                self._missed[p] += 1
        L, st = hip.lib(), hip.stream()
        segs = self._segments(skipped)
        if wd or self.max_norm is not None or self.flat_e is not None:
            return self._step_with_options(L, st, segs, skipped, lr, b1, b2, eps, wd)
        for o, n, missed in segs:
            t = self._t - missed
            bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
            hip.check(L.sisr_adam_flat(self.flat_p.data_ptr() + 4 * o, self.flat_g.data_ptr() + 4 * o,
                                       self.flat_m.data_ptr() + 4 * o, self.flat_v.data_ptr() + 4 * o, n, b2, 1 - b1,
                                       1 - b2, eps, lr / bc1, math.sqrt(bc2), 1.0, st), "sisr_adam_flat")

    def _step_with_options(self, L, st, segs, skipped, lr, b1, b2, eps, wd):
        """the norm over exactly the ranges about to be updated (what clip_grad_norm_ covers: the parameters with a gradient;
        a skipped parameter's range holds a stale one), then sisr_update_flat per range, then the average-only launch over
        the skipped ranges"""
        coef = None
        if self.max_norm is not None:
            if segs:
                parts = 0
                for o, n, _ in segs:
                    hip.check(L.sisr_sumsq_partial(self.flat_g.data_ptr() + 4 * o, n, self._norm_ws.data_ptr() + 8 * parts, st),
                              "sisr_sumsq_partial")
                    parts += L.sisr_sumsq_workspace_bytes(n) // 8
                hip.check(L.sisr_clip_coef(self._norm_ws.data_ptr(), parts, float(self.max_norm), self._norm64.data_ptr(),
                                           self._norm32.data_ptr(), self._norm32.data_ptr() + 4, st), "sisr_clip_coef")
                coef = self._norm32.data_ptr() + 4
            else:  # no gradient anywhere: clip_grad_norm_ reports a zero norm
                self._norm64.zero_()
                self._norm32.copy_(torch.tensor([0.0, 1.0]))
        decay = 1.0 - lr * wd
        e = self.flat_e.data_ptr() if self.flat_e is not None else None
        omd = 1.0 - self.ema_decay if self.flat_e is not None else 0.0
        for o, n, missed in segs:
            t = self._t - missed
            bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
            hip.check(L.sisr_update_flat(self.flat_p.data_ptr() + 4 * o, self.flat_g.data_ptr() + 4 * o,
                                         self.flat_m.data_ptr() + 4 * o, self.flat_v.data_ptr() + 4 * o,
                                         None if e is None else e + 4 * o, n, b2, 1 - b1, 1 - b2, eps, lr / bc1,
                                         math.sqrt(bc2), 1.0, coef, decay, omd, st), "sisr_update_flat")
        if e is not None:
            for o, n in self._skipped_ranges(skipped):
                hip.check(L.sisr_ema_flat(self.flat_p.data_ptr() + 4 * o, e + 4 * o, n, omd, st), "sisr_ema_flat")

    # -- torch-compatible (de)serialisation
    def state_dict(self):
        for p, st in self.state.items():
            if len(st):
                st['step'] = torch.tensor(float(self._t - self._missed.get(p, 0)), dtype=torch.float32)
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)  # torch casts / copies the loaded tensors next to the parameters
        steps = []
        for p in self.param_groups[0]['params']:
            st = self.state.get(p)
            if not st:
                continue
            for key, flat in (('exp_avg', self.flat_m), ('exp_avg_sq', self.flat_v)):
                view = self._view(flat, p)
                view.copy_(st[key])
                st[key] = view
            steps.append((p, int(float(st['step']))))
        self._t = max([s for _, s in steps], default=0)
        self._missed = {p: self._t - s for p, s in steps}
        self._plan = None
        if self.flat_e is not None:  # the average is no optimiser state in torch's schema: it restarts from the parameters
            self.load_ema(None)      # as they are; a caller that has one stored hands it to load_ema afterwards
