"""Golden fixtures for patch sizes 4 and 8, produced by RUNNING THE REFERENCE ITSELF.

Imports the reference exactly as make_golden.py does (through that module: `_refshim` stand-ins, parameters drawn by
`oracle.maskdit_oracle.init_params`) and records one masked training step of DiT-S/4 on a 32^2 latent and of DiT-S/8 on a
64^2 latent (T = 64 both, B = 4, mask ratio 0.5) in the layout gen_train uses for s2_train.npz: inputs and draws, losses,
D_yn, gradient norms + 64 sampled entries per tensor, one AdamW + EMA step.

    python tests/golden/make_golden_patch.py            # rewrites s4_train.npz and s8_train.npz

make_golden.gen_train itself hard-codes the token count of patch 2 for the mask-noise draw, hence this sibling.
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden import make_golden as MG  # noqa: E402  (imports the reference)

O = MG.O


def gen_train_patch(tag, model_type, R, B, seed):
    cfg = O.make_cfg(model_type, img_resolution=R)
    P = O.init_params(cfg, seed=seed, dezero=True)
    net = MG.build_ref(model_type, R, P)
    net.train()
    wrapped = MG.Wrap(net)
    g = torch.Generator().manual_seed(seed + 100)
    images = 0.5 * torch.randn(B, 4, R, R, generator=g)
    cls = torch.randint(0, 1000, (B,), generator=g)
    keep = (torch.rand(B, 1, generator=g) >= 0.1).float()
    labels = MG.one_hot(cls) * keep
    T = int(net.model.x_embedder.num_patches)
    torch.manual_seed(seed + 200)  # the reference's internal draws in order (loss.py:35,39; maskdit.py:102)
    rnd_normal = torch.randn(B, 1, 1, 1)
    noise = torch.randn(B, 4, R, R)
    mask_noise = torch.rand(B, T)
    torch.manual_seed(seed + 200)
    loss = MG.Losses['edm']()(net=wrapped, images=images, labels=labels, mask_ratio=0.5, mae_loss_coef=0.1)
    out = dict(seed=np.int64(seed), B=np.int64(B), R=np.int64(R), images=images.numpy(), cls=cls.numpy(), keep=keep.numpy(),
               rnd_normal=rnd_normal.numpy(), noise=noise.numpy(), mask_noise=mask_noise.numpy(), loss=loss.detach().numpy())
    with torch.no_grad():
        mdict = {k: torch.from_numpy(v) for k, v in O.get_mask_from_noise(mask_noise.numpy(), 0.5).items()}
        sigma = (rnd_normal * 1.2 - 1.2).exp()
        out['D_yn'] = net(images + noise * sigma, sigma, labels, mask_ratio=0.5, mask_dict=mdict)['x'].numpy()
    names = [k for k in P if k not in O.NON_TRAINABLE]
    out['param_names'] = np.array(names)
    out['param_sums'] = np.stack([MG.checks(P[k])[0] for k in names])
    loss.mean().backward()
    sd = dict(net.named_parameters())
    gc = [MG.checks(sd[k].grad if sd[k].grad is not None else torch.zeros_like(sd[k])) for k in names]
    out['grad_sums'] = np.stack([c[0] for c in gc])
    out['grad_samples'] = np.stack([c[1] for c in gc])
    ema = copy.deepcopy(net)
    opt = torch.optim.AdamW([p for p in net.parameters() if p.requires_grad], lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0)
    opt.step()
    MG.update_ema(ema, net, decay=0.9999)
    sd, se = dict(net.named_parameters()), dict(ema.named_parameters())
    uc, ec = [MG.checks(sd[k]) for k in names], [MG.checks(se[k]) for k in names]
    out['upd_sums'] = np.stack([c[0] for c in uc])
    out['upd_samples'] = np.stack([c[1] for c in uc])
    out['ema_sums'] = np.stack([c[0] for c in ec])
    out['ema_samples'] = np.stack([c[1] for c in ec])
    np.savez_compressed(os.path.join(HERE, f'{tag}.npz'), **out)
    print(f'{tag}.npz written; loss =', loss.detach().numpy())


JOBS = {
    's4_train': lambda: gen_train_patch('s4_train', 'DiT-S/4', 32, 4, seed=11),
    's8_train': lambda: gen_train_patch('s8_train', 'DiT-S/8', 64, 4, seed=12),
}

if __name__ == '__main__':
    for job in (sys.argv[1:] or list(JOBS)):
        JOBS[job]()
