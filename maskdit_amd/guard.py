"""Device-side guard of the fused optimizer step: skip a step whose gradient holds an inf / NaN -- what the
reference's GradScaler did for `optimizer.step()` (train.py:39-50,226) -- and clip by global norm
(`torch.nn.utils.clip_grad_norm_`), without a host sync, without atomics, bit-reproducible.

`GuardState` owns the 64-byte device record `mdt_guard_state` (include/maskdit_hip.h) and the fp64 partial-sum workspace,
and wraps the three library entries.  It is only imported by an optimizer that was built with a guard switched on.
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import call

# byte offsets of mdt_guard_state
_SUMSQ, _NORM, _COEF, _SKIP, _APPLIED, _SKIPPED = 0, 16, 20, 24, 32, 40


class GuardState:
    def __init__(self, device, max_grad_norm: float = 0.0, skip_nonfinite: bool = False):
        self.max_norm = float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.buf = torch.zeros(64, device=device, dtype=torch.uint8)
        self.sum_flag = self.buf[_SUMSQ:_SUMSQ + 16].view(torch.float64)  # (sumsq, nonfinite): what a sharded step all-reduces
        self.norm = self.buf[_NORM:_NORM + 4].view(torch.float32)[0]      # 0-dim views: reading them is the caller's sync
        self.coef = self.buf[_COEF:_COEF + 4].view(torch.float32)[0]
        self.skip = self.buf[_SKIP:_SKIP + 4].view(torch.int32)[0]
        self.counters = self.buf[_APPLIED:_APPLIED + 16].view(torch.int64)  # (applied, skipped)
        self.ws = None
        self._started = False  # a sumsq of this step has been issued (the next one accumulates)

    @property
    def ptr(self) -> int:
        return self.buf.data_ptr()

    def begin(self):
        self._started = False

    def sumsq(self, g_ptr: int, n: int, grad_scale: float, stream):
        need = int(_lib.lib().mdt_grad_sumsq_ws_floats(n))
        if self.ws is None or self.ws.numel() < need:
            self.ws = torch.empty(need, device=self.buf.device, dtype=torch.float32)
        call('mdt_grad_sumsq', g_ptr, n, float(grad_scale), self.ws.data_ptr(), self.ws.numel(), self.ptr, int(self._started), stream)
        self._started = True

    def decide(self, beta1: float, beta2: float, stream):
        call('mdt_guard_decide', self.ptr, self.max_norm, int(self.skip_nonfinite), float(beta1), float(beta2), stream)

    def step(self, p, g, m, v, ema, w16, n, hyp, decay, grad_scale, stream):
        lr, b1, b2, eps, wd, bc1, bc2 = hyp
        call('mdt_adamw_ema_step_guarded', p, g, m, v, ema, w16, n, lr, b1, b2, eps, wd, bc1, bc2, decay, float(grad_scale),
             self.ptr, int(self.skip_nonfinite), stream)

    # ---- host reads (each one synchronises) / checkpoint upload ----------------------------------
    def applied_steps(self) -> int:
        return int(self.counters[0].item())

    def skipped_steps(self) -> int:
        return int(self.counters[1].item())

    def set_applied(self, step: int):
        self.counters[0:1].fill_(int(step))
