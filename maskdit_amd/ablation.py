"""Drop-in for `sample.ablation_sampler` (sample.py:73-188): the generalized EDM sampler -- Euler or Heun steps, VP / VE /
iDDPM / EDM time discretization, VP / VE / linear noise schedule sigma(t), VP or no signal scaling s(t), the `alpha` blend
of the second evaluation point and stochastic churn -- plus the routing of the reference's sampling entry points
(sample.py:240-245) between it and `edm_sampler`.

With `round_sigma` the identity (EDMPrecond.round_sigma, models/maskdit.py:775) every quantity of a step that is not a
tensor of the batch depends on the step index only.  `step_table` computes all of them once, in fp64, with the
reference's own scalar operations in the reference's order, into one row per step (columns MDT_ABL_* of
include/maskdit_hip.h).  Three fused kernels apply a row to the fp64 state:

    mdt_ablation_prep    x_hat = A x_cur + C noise, and the network input c_in(sigma) (float(x_hat) / s)
    mdt_ablation_slope1  D -> d_cur = P x_hat - Q D -> x_prime (second evaluation follows) or x_next
    mdt_ablation_slope2  D' -> d' = P2 x_prime - Q2 D' -> x_next = x_hat + H (W1 d_cur + W2 d')

They find their row through the device step counter (mdt_sampler_advance), so one captured graph replays every step of
every discretization / schedule / scaling / alpha / churn setting; only `cfg_scale` is a captured value.  The churn noise
is an input buffer of the graph: the caller's `randn_like` runs once per step outside the graph (as sample.py:168 calls
it), its draw is copied into the buffer, and the graph applies it with the row's C (zero when there is no churn).
"""
from __future__ import annotations

import ctypes as C
import weakref
from typing import Dict, Tuple

import numpy as np
import torch

from . import _lib
from . import sampler as _sampler
from ._lib import call
from .engine import check_precision, plan_key, reads_f32_arena
from .loss import unwrap_model
from .precond import EDMPrecond

SOLVERS = ('euler', 'heun')
DISCRETIZATIONS = ('vp', 've', 'iddpm', 'edm')
SCHEDULES = ('vp', 've', 'linear')
SCALINGS = ('vp', 'none')
ABLATION_KEYS = ('solver', 'discretization', 'schedule', 'scaling')

# the MDT_ABL_* columns of include/maskdit_hip.h, in order; the row is padded to NCOL
COLS = ('a', 'c', 'sig', 's', 'p', 'q', 'sig2', 's2', 'p2', 'q2', 'h', 'ah', 'w1', 'w2', 'second')
NCOL = 16
MAX_STEPS = 1024  # rows of the persistent table a captured graph reads


def check_choices(solver, discretization, schedule, scaling):
    """sample.py:80-83, as ValueError."""
    for name, value, allowed in (('solver', solver, SOLVERS), ('discretization', discretization, DISCRETIZATIONS),
                                 ('schedule', schedule, SCHEDULES), ('scaling', scaling, SCALINGS)):
        if value not in allowed:
            raise ValueError(f'{name} must be one of {allowed}, got {value!r}')


def step_table(num_steps, device, net_sigma_min=0, net_sigma_max=float('inf'), sigma_min=None, sigma_max=None, rho=7,
               solver='heun', discretization='edm', schedule='linear', scaling='none', epsilon_s=1e-3, C_1=0.001,
               C_2=0.008, M=1000, alpha=1, S_churn=0, S_min=0, S_max=float('inf'), S_noise=1):
    """The per-step coefficients of sample.py:85-186 in fp64 on `device`, computed with the reference's operations in its
    order.  Returns (table [num_steps, NCOL] fp64, sigma(t_0) s(t_0) -- the latents' factor, sample.py:160 -- and the
    per-step list of whether the step takes the second evaluation)."""
    check_choices(solver, discretization, schedule, scaling)
    round_sigma = torch.as_tensor  # EDMPrecond.round_sigma (models/maskdit.py:775)

    # sample.py:86-92
    vp_sigma = lambda beta_d, beta_min: lambda t: (np.e ** (0.5 * beta_d * (t ** 2) + beta_min * t) - 1) ** 0.5  # noqa: E731
    vp_sigma_deriv = lambda beta_d, beta_min: lambda t: 0.5 * (beta_min + beta_d * t) * (sigma(t) + 1 / sigma(t))  # noqa: E731
    vp_sigma_inv = lambda beta_d, beta_min: lambda sigma: ((beta_min ** 2 + 2 * beta_d * (  # noqa: E731
        sigma ** 2 + 1).log()).sqrt() - beta_min) / beta_d
    ve_sigma = lambda t: t.sqrt()  # noqa: E731
    ve_sigma_deriv = lambda t: 0.5 / t.sqrt()  # noqa: E731
    ve_sigma_inv = lambda sigma: sigma ** 2  # noqa: E731

    # sample.py:95-108
    if sigma_min is None:
        vp_def = vp_sigma(beta_d=19.1, beta_min=0.1)(t=epsilon_s)
        sigma_min = {'vp': vp_def, 've': 0.02, 'iddpm': 0.002, 'edm': 0.002}[discretization]
    if sigma_max is None:
        vp_def = vp_sigma(beta_d=19.1, beta_min=0.1)(t=1)
        sigma_max = {'vp': vp_def, 've': 100, 'iddpm': 81, 'edm': 80}[discretization]
    sigma_min = max(sigma_min, net_sigma_min)
    sigma_max = min(sigma_max, net_sigma_max)
    vp_beta_d = 2 * (np.log(sigma_min ** 2 + 1) / epsilon_s - np.log(sigma_max ** 2 + 1)) / (epsilon_s - 1)
    vp_beta_min = np.log(sigma_max ** 2 + 1) - 0.5 * vp_beta_d

    # sample.py:111-128
    step_indices = torch.arange(num_steps, dtype=torch.float64, device=device)
    if discretization == 'vp':
        orig_t_steps = 1 + step_indices / (num_steps - 1) * (epsilon_s - 1)
        sigma_steps = vp_sigma(vp_beta_d, vp_beta_min)(orig_t_steps)
    elif discretization == 've':
        orig_t_steps = (sigma_max ** 2) * ((sigma_min ** 2 / sigma_max ** 2) ** (step_indices / (num_steps - 1)))
        sigma_steps = ve_sigma(orig_t_steps)
    elif discretization == 'iddpm':
        u = torch.zeros(M + 1, dtype=torch.float64, device=device)
        alpha_bar = lambda j: (0.5 * np.pi * j / M / (C_2 + 1)).sin() ** 2  # noqa: E731
        for j in torch.arange(M, 0, -1, device=device):  # M, ..., 1
            u[j - 1] = ((u[j] ** 2 + 1) / (alpha_bar(j - 1) / alpha_bar(j)).clip(min=C_1) - 1).sqrt()
        u_filtered = u[torch.logical_and(u >= sigma_min, u <= sigma_max)]
        sigma_steps = u_filtered[((len(u_filtered) - 1) / (num_steps - 1) * step_indices).round().to(torch.int64)]
    else:
        sigma_steps = (sigma_max ** (1 / rho) + step_indices / (num_steps - 1) * (
            sigma_min ** (1 / rho) - sigma_max ** (1 / rho))) ** rho

    # sample.py:131-152
    if schedule == 'vp':
        sigma = vp_sigma(vp_beta_d, vp_beta_min)
        sigma_deriv = vp_sigma_deriv(vp_beta_d, vp_beta_min)
        sigma_inv = vp_sigma_inv(vp_beta_d, vp_beta_min)
    elif schedule == 've':
        sigma, sigma_deriv, sigma_inv = ve_sigma, ve_sigma_deriv, ve_sigma_inv
    else:
        sigma = lambda t: t  # noqa: E731
        sigma_deriv = lambda t: 1  # noqa: E731
        sigma_inv = lambda sigma: sigma  # noqa: E731
    if scaling == 'vp':
        s = lambda t: 1 / (1 + sigma(t) ** 2).sqrt()  # noqa: E731
        s_deriv = lambda t: -sigma(t) * sigma_deriv(t) * (s(t) ** 3)  # noqa: E731
    else:
        s = lambda t: 1  # noqa: E731
        s_deriv = lambda t: 0  # noqa: E731

    # sample.py:155-160
    t_steps = sigma_inv(round_sigma(sigma_steps))
    t_steps = torch.cat([t_steps, torch.zeros_like(t_steps[:1])])  # t_N = 0
    scale0 = sigma(t_steps[0]) * s(t_steps[0])

    # sample.py:161-186, the scalar half of every step
    rows, second = [], []
    for i, (t_cur, t_next) in enumerate(zip(t_steps[:-1], t_steps[1:])):
        gamma = min(S_churn / num_steps, np.sqrt(2) - 1) if S_min <= sigma(t_cur) <= S_max else 0
        t_hat = sigma_inv(round_sigma(sigma(t_cur) + gamma * sigma(t_cur)))
        a = s(t_hat) / s(t_cur)
        c = (sigma(t_hat) ** 2 - sigma(t_cur) ** 2).clip(min=0).sqrt() * s(t_hat) * S_noise
        h = t_next - t_hat
        p = sigma_deriv(t_hat) / sigma(t_hat) + s_deriv(t_hat) / s(t_hat)
        q = sigma_deriv(t_hat) * s(t_hat) / sigma(t_hat)
        t_prime = t_hat + alpha * h
        p2 = sigma_deriv(t_prime) / sigma(t_prime) + s_deriv(t_prime) / s(t_prime)
        q2 = sigma_deriv(t_prime) * s(t_prime) / sigma(t_prime)
        two = not (solver == 'euler' or i == num_steps - 1)
        second.append(two)
        rows.append([a, c, sigma(t_hat), s(t_hat), p, q, sigma(t_prime), s(t_prime), p2, q2, h, alpha * h,
                     1 - 1 / (2 * alpha), 1 / (2 * alpha), float(two)])
    f64 = dict(dtype=torch.float64, device=device)
    pad = torch.zeros(NCOL - len(COLS), **f64)
    table = torch.stack([torch.cat([torch.stack([torch.as_tensor(v, **f64).reshape(()) for v in r]), pad]) for r in rows])
    return table, scale0, second


class _GraphedAblation:
    """Captured graphs + persistent buffers (table, noise, state) for one (net, batch, cfg?, precision)."""

    def __init__(self, net: EDMPrecond, B: int, use_cfg: bool, precision: str = 'bf16'):
        # as _sampler._GraphedHeun: the cache owns neither the network nor its engine
        self.B, self.use_cfg = B, use_cfg
        self.sigma_data = float(net.sigma_data)
        sp = net.spec
        dev = next(net.parameters()).device
        self.chw = sp.C * sp.R * sp.R
        self.dup = 2 if use_cfg else 1
        self._eng_ref = weakref.ref(net.engine())
        self.precision = precision
        self.pl = self.eng.plan(B * self.dup, False, False, None, precision)
        f64 = dict(device=dev, dtype=torch.float64)
        self.x = torch.zeros(B, self.chw, **f64)       # x_cur at a step's start, x_prime between the evaluations, x_next
        self.x_hat = torch.zeros(B, self.chw, **f64)
        self.d_cur = torch.zeros(B, self.chw, **f64)
        self.noise = torch.zeros(B, self.chw, **f64)
        self.table = torch.zeros(MAX_STEPS, NCOL, **f64)
        self.step_idx = torch.zeros(1, device=dev, dtype=torch.int32)
        self.sig = torch.zeros(B * self.dup, device=dev, dtype=torch.float32)
        self.stream = torch.cuda.Stream(device=dev)
        self.graph_full = self.graph_short = None
        self.captured_cfg = None

    @property
    def eng(self):
        return self._eng_ref()

    def _eval(self, st, which):
        """network evaluation at row column SIG (which = 0, from x_cur: writes x_hat) or SIG2 (which = 1, at x_prime)"""
        pl = self.pl
        call('mdt_ablation_prep', self.x.data_ptr(), self.noise.data_ptr(), self.table.data_ptr(), self.step_idx.data_ptr(),
             which, self.x_hat.data_ptr(), pl.buf['xin'].data_ptr(), self.sig.data_ptr(), self.B, self.chw, self.dup,
             self.sigma_data, st)
        call('mdt_precond_coef', self.sig.data_ptr(), pl.buf['coef'].data_ptr(), self.B * self.dup, self.sigma_data, st)
        pl.fwd.run(st)

    def _record(self, st, cfg_scale, second):
        Fp = self.pl.buf['F'].data_ptr()
        tp, ip = self.table.data_ptr(), self.step_idx.data_ptr()
        self._eval(st, 0)
        call('mdt_ablation_slope1', self.x_hat.data_ptr(), Fp, tp, ip, cfg_scale, int(self.use_cfg), self.d_cur.data_ptr(),
             self.x.data_ptr(), self.B, self.chw, self.sigma_data, st)
        if second:
            self._eval(st, 1)
            call('mdt_ablation_slope2', self.x_hat.data_ptr(), self.x.data_ptr(), Fp, self.d_cur.data_ptr(), tp, ip,
                 cfg_scale, int(self.use_cfg), self.B, self.chw, self.sigma_data, st)
        call('mdt_sampler_advance', ip, st)

    def capture(self, cfg_scale: float):
        L = _lib.lib()
        self.destroy()
        if self.eng.shadows_dirty and not reads_f32_arena(self.precision):
            self.eng.refresh_shadows()
        torch.cuda.synchronize()
        graphs = []
        with torch.cuda.stream(self.stream):
            st = self.stream.cuda_stream
            for second in (True, False):
                _lib.check(L.mdt_graph_begin(st), 'mdt_graph_begin')
                try:
                    self._record(st, cfg_scale, second)
                finally:
                    g = C.c_void_p()
                    rc = L.mdt_graph_end(st, C.byref(g))
                _lib.check(rc, 'mdt_graph_end')
                graphs.append(g)
        self.graph_full, self.graph_short = graphs
        self.captured_cfg = cfg_scale

    def destroy(self):
        L = _lib.lib()
        for g in (self.graph_full, self.graph_short):
            if g is not None:
                L.mdt_graph_destroy(g)
        self.graph_full = self.graph_short = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


_CACHE: Dict[Tuple[int, int, bool, str], _GraphedAblation] = {}
_sampler._CACHES.append(_CACHE)  # sampler.release_graphs() releases these graphs too


def release_graphs():
    """Destroy every cached ablation-sampler graph."""
    while _CACHE:
        _CACHE.popitem()[1].destroy()


def _graphed(net: EDMPrecond, B: int, use_cfg: bool, precision: str = 'bf16') -> _GraphedAblation:
    """The rules of sampler._graphed: dead-engine cleanup, at most 4 entries, dropped when the plan cache evicts its plan."""
    for k in [k for k, v in _CACHE.items() if v.eng is None]:
        _CACHE.pop(k).destroy()
    key = (id(net.engine()), B, use_cfg, precision)
    g = _CACHE.get(key)
    if g is None or g.eng is not net.engine() or g.pl is not net.engine()._plans.get(plan_key(B * g.dup, False, False, None, precision)):
        if len(_CACHE) >= 4:
            _CACHE.pop(next(iter(_CACHE))).destroy()
        g = _GraphedAblation(net, B, use_cfg, precision)
        _CACHE[key] = g

        def dropped(key=key, ref=weakref.ref(g)):
            if _CACHE.get(key) is ref() and ref() is not None:
                _CACHE.pop(key).destroy()
        g.pl.evict_hooks.append(dropped)
    return g


@torch.no_grad()
def ablation_sampler(net, latents, class_labels=None, cfg_scale=None, feat=None, randn_like=torch.randn_like, num_steps=18,
                     sigma_min=None, sigma_max=None, rho=7, solver='heun', discretization='edm', schedule='linear',
                     scaling='none', epsilon_s=1e-3, C_1=0.001, C_2=0.008, M=1000, alpha=1, S_churn=0, S_min=0,
                     S_max=float('inf'), S_noise=1, use_graph=True, precision=None):
    """Same signature and result (fp64 [N, C, H, W]) as sample.py:73-188, plus `use_graph` and `precision` as on
    `edm_sampler` ('bf16', 'fp32' or 'bf16x3'; None = the network's `eval_precision`).  `randn_like` is called once per
    step, as the reference calls it, so the caller's generators end in the reference's state.  `use_graph=False` issues
    the same launches without capture: same kernels, same bits."""
    check_choices(solver, discretization, schedule, scaling)
    raw = unwrap_model(net)
    if not isinstance(raw, EDMPrecond):
        raise TypeError(f'maskdit_amd.ablation_sampler expects a maskdit_amd EDMPrecond, got {type(raw).__name__}')
    if feat is not None:
        raise NotImplementedError('feat conditioning is outside the shipped configurations')
    if not latents.is_cuda:
        raise _lib.MaskDiTLibError('maskdit_amd: latents are not on a HIP device; there is no CPU path')
    if raw.training:
        raise RuntimeError('ablation_sampler needs net.eval() (generate.py:41)')
    if num_steps > MAX_STEPS:
        raise ValueError(f'num_steps exceeds the captured table capacity ({MAX_STEPS})')
    precision = raw.eval_precision if precision is None else precision
    check_precision(precision)
    table, scale0, second = step_table(num_steps, latents.device, raw.sigma_min, raw.sigma_max, sigma_min, sigma_max, rho,
                                       solver, discretization, schedule, scaling, epsilon_s, C_1, C_2, M, alpha, S_churn,
                                       S_min, S_max, S_noise)
    B = latents.shape[0]
    labels = raw._labels(class_labels, B, latents.device)
    x_next = latents.to(torch.float64) * scale0  # sample.py:160

    use_cfg = cfg_scale is not None
    g = _graphed(raw, B, use_cfg, precision)
    s = float(cfg_scale) if use_cfg else 0.0
    stale = raw.engine().shadows_dirty and not reads_f32_arena(precision)
    if use_graph and (g.graph_full is None or g.captured_cfg != s or stale):
        g.capture(s)
    if not use_graph and stale:
        raw.engine().refresh_shadows()
    L = _lib.lib()
    cur = torch.cuda.current_stream()
    g.table[:num_steps].copy_(table)
    g.step_idx.zero_()
    g.x.copy_(x_next.reshape(B, -1))
    lab = g.pl.buf['labels']
    lab[:B].copy_(labels)
    if use_cfg:
        lab[B:].zero_()  # models/maskdit.py:566-567: y_null
    g.stream.wait_stream(cur)
    with torch.cuda.stream(g.stream):
        st = g.stream.cuda_stream
        x_cur = g.x.view_as(latents)
        for i in range(num_steps):
            g.noise.copy_(randn_like(x_cur).reshape(B, -1))  # sample.py:168, one draw per step
            if use_graph:
                _lib.check(L.mdt_graph_launch(g.graph_full if second[i] else g.graph_short, st), 'mdt_graph_launch')
            else:
                g._record(st, s, second[i])
        out = g.x.clone().view_as(x_next)
    cur.wait_stream(g.stream)
    return out


def add_sampler_args(ap):
    """The five sampler flags of the reference's entry points (sample.py:357-363, train.py:322-326)."""
    ap.add_argument('--S_churn', type=int, default=0, help='Stochasticity strength')
    ap.add_argument('--solver', type=str, default=None, choices=list(SOLVERS), help='Ablate ODE solver')
    ap.add_argument('--discretization', type=str, default=None, choices=list(DISCRETIZATIONS), help='Ablate ODE solver')
    ap.add_argument('--schedule', type=str, default=None, choices=list(SCHEDULES), help='Ablate noise schedule sigma(t)')
    ap.add_argument('--scaling', type=str, default=None, choices=list(SCALINGS), help='Ablate signal scaling s(t)')


def select_sampler(num_steps, S_churn=0, solver=None, discretization=None, schedule=None, scaling=None):
    """sample.py:240-245: any of solver / discretization / schedule / scaling given -> ablation_sampler with the given
    keywords, else edm_sampler.  Returns (sampler function, keywords)."""
    kw = dict(num_steps=num_steps, S_churn=S_churn, solver=solver, discretization=discretization, schedule=schedule,
              scaling=scaling)
    kw = {k: v for k, v in kw.items() if v is not None}
    return (ablation_sampler if any(k in kw for k in ABLATION_KEYS) else _sampler.edm_sampler), kw
