"""Generate tests/golden/ablation_sampler.npz by RUNNING THE REFERENCE'S OWN `sample.ablation_sampler`.

Runs only in the build container (needs the reference tree, as make_golden.py does).  DiT-S/2 at R = 32 with weights from
`oracle.maskdit_oracle.init_params(cfg, seed=SEED, dezero=True)`, per-seed StackedRandomGenerator latents / labels /
churn noise, 6 steps, over the combinations of COMBOS.  For every run it records:

  z      the sampler output (stored as float32 to keep the file small: the rounding is 6e-8 of max|z|, 1 % of the
         tightest bound a test applies to it);
  sig    the fp64 noise level of every network call, in call order (a recording wrapper around the net);
  spread max|z(weights +-1 ulp) - z| / max|z|: the reference's own sensitivity to a disturbance of the size of a
         different summation order.  Asserted <= SPREAD_MAX for every combination but the full VP triple (whose tests
         bound it at 2.5x its own stored spread instead).

and, per combination, `toy`: the same sampler on an analytic denoiser D(x, s) = x sd^2 / (s^2 + sd^2) (no network), which
pins the per-step coefficient table on its own.

    python tests/golden/make_golden_ablation.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get('MASKDIT_REFERENCE', '/root/reference')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(HERE, '_refshim'))
sys.path.insert(0, REF)

from oracle import maskdit_oracle as O  # noqa: E402

import models.maskdit as ref_m  # noqa: E402  (reference)
from sample import ablation_sampler as ref_ablation_sampler  # noqa: E402  (reference)
from utils import StackedRandomGenerator  # noqa: E402  (reference)

torch.set_num_threads(8)

SEED = 21                  # weight seed
SEEDS = [300, 302]        # StackedRandomGenerator seeds (batch of 2; at 300-301 edm_vp_vp spreads 2.2e-6)
NUM_STEPS = 6
CFG = 1.5
SPREAD_MAX = 2e-6          # of max|z|: 2.5x under TOL_F32 = 5e-6
TOY_SHAPE = [len(SEEDS), 4, 4, 4]
SIGMA_DATA = 0.5

# name, sampler keywords, also run without CFG
COMBOS = [
    ('edm_heun', dict(solver='heun', discretization='edm', schedule='linear', scaling='none'), True),
    ('edm_euler', dict(solver='euler', discretization='edm', schedule='linear', scaling='none'), False),
    ('vp_vp_vp', dict(solver='heun', discretization='vp', schedule='vp', scaling='vp'), True),
    ('vp_vp_none', dict(solver='heun', discretization='vp', schedule='vp', scaling='none'), False),
    ('edm_vp_vp', dict(solver='heun', discretization='edm', schedule='vp', scaling='vp'), False),
    ('ve_ve_none', dict(solver='heun', discretization='ve', schedule='ve', scaling='none'), False),
    ('iddpm', dict(solver='heun', discretization='iddpm', schedule='linear', scaling='none'), False),
    ('vp_euler_linear', dict(solver='euler', discretization='vp', schedule='linear', scaling='none'), False),
    ('edm_alpha05', dict(solver='heun', discretization='edm', schedule='linear', scaling='none', alpha=0.5), False),
    ('edm_churn', dict(solver='heun', discretization='edm', schedule='linear', scaling='none', S_churn=10, S_min=0.05,
                       S_max=50, S_noise=1.003), False),
]
SPREAD_EXEMPT = ('vp_vp_vp',)


class Recorder:
    """The net as the sampler sees it, recording the fp64 noise level of every call."""

    def __init__(self, net):
        self.net, self.sig = net, []
        self.sigma_min, self.sigma_max, self.round_sigma = net.sigma_min, net.sigma_max, net.round_sigma

    def __call__(self, x, sigma, *a, **k):
        self.sig.append(float(torch.as_tensor(sigma, dtype=torch.float64)))
        return self.net(x, sigma, *a, **k)


class Toy:
    """Analytic denoiser: D(x, s) = x sd^2 / (s^2 + sd^2) in fp64 of the fp32 input the sampler passes."""
    sigma_min, sigma_max = 0, float('inf')

    def round_sigma(self, sigma):
        return torch.as_tensor(sigma)

    def __call__(self, x, sigma, class_labels=None, cfg_scale=None, feat=None):
        s = torch.as_tensor(sigma, dtype=torch.float64)
        return {'x': x.to(torch.float64) * (SIGMA_DATA ** 2 / (s * s + SIGMA_DATA ** 2))}


def build_net(P):
    net = ref_m.Precond_models['edm'](img_resolution=32, img_channels=4, num_classes=1000, model_type='DiT-S/2',
                                      use_decoder=True, mae_loss_coef=0.1, pad_cls_token=False)
    net.load_state_dict(P, strict=True)
    return net.eval()


def run(net, kw, cfg_scale):
    rnd = StackedRandomGenerator('cpu', SEEDS)
    latents = rnd.randn([len(SEEDS), 4, 32, 32])
    labels = torch.eye(1000)[rnd.randint(1000, size=[len(SEEDS)])]
    rec = Recorder(net)
    with torch.no_grad():
        z = ref_ablation_sampler(rec, latents.float(), labels.float(), cfg_scale=cfg_scale, randn_like=rnd.randn_like,
                                 num_steps=NUM_STEPS, **kw)
    return z, np.array(rec.sig)


def main():
    cfg = O.make_cfg('DiT-S/2', img_resolution=32)
    P = O.init_params(cfg, seed=SEED, dezero=True)
    ulp = {d: {k: torch.nextafter(v, torch.full_like(v, d * float('inf'))) if v.is_floating_point() else v
               for k, v in P.items()} for d in (1, -1)}
    nets = {0: build_net(P), 1: build_net(ulp[1]), -1: build_net(ulp[-1])}
    out = dict(seed=np.int64(SEED), seeds=np.array(SEEDS), num_steps=np.int64(NUM_STEPS), cfg_scale=np.float64(CFG),
               toy_shape=np.array(TOY_SHAPE), sigma_data=np.float64(SIGMA_DATA),
               combos=np.array(json.dumps([[name, kw, nocfg] for name, kw, nocfg in COMBOS])))
    bad = []
    for name, kw, nocfg in COMBOS:
        for tag, cs in [('', CFG)] + ([('_nocfg', None)] if nocfg else []):
            z, sig = run(nets[0], kw, cs)
            zmax = z.abs().max().item()
            spread = max((run(nets[d], kw, cs)[0] - z).abs().max().item() / zmax for d in (1, -1))
            out[f'{name}{tag}_z'] = z.numpy().astype(np.float32)
            out[f'{name}{tag}_sig'] = sig
            out[f'{name}{tag}_spread'] = np.float64(spread)
            print(f'{name + tag:>22}: max|z| {zmax:.4f}, +-1 ulp spread {spread:.2e}, {len(sig)} evaluations', flush=True)
            if spread > SPREAD_MAX and name not in SPREAD_EXEMPT:
                bad.append((name + tag, spread))
        rnd = StackedRandomGenerator('cpu', SEEDS)
        toy_lat = rnd.randn(TOY_SHAPE)
        with torch.no_grad():
            out[f'{name}_toy'] = ref_ablation_sampler(Toy(), toy_lat, None, randn_like=rnd.randn_like, num_steps=NUM_STEPS,
                                                      **kw).numpy()
    assert not bad, f'combinations above the {SPREAD_MAX:g} spread condition at these seeds: {bad}'
    np.savez_compressed(os.path.join(HERE, 'ablation_sampler.npz'), **out)
    print('ablation_sampler.npz written')


if __name__ == '__main__':
    main()
