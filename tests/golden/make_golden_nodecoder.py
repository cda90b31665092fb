"""Golden fixtures for the decoder-less models (use_decoder=False), produced by RUNNING THE REFERENCE ITSELF.

Imports the reference exactly as make_golden.py does (through that module: `_refshim` stand-ins, parameters drawn by
`oracle.maskdit_oracle.init_params`) and builds its EDMPrecond with `use_decoder=False` (models/maskdit.py:302-331: no
decoder_layer, decoder_blocks, decoder_pos_embed or mask_token; the final layer reads the encoder's width).  Records, in the
layout of make_golden_patch.gen_train_patch (inputs and draws, losses, D_yn, gradient norms + 64 sampled entries per tensor,
one AdamW + EMA step):

    s2nd_train.npz   DiT-S/2 on a 16^2 latent (T = 64), B = 4, mask ratio 0.64: int(64 * 0.36) = 23 kept tokens
    s4nd_train.npz   DiT-S/4 on a 32^2 latent (T = 64), B = 4, mask ratio 0.5
    nd_sampler.npz   the reference's edm_sampler on the S/2 model: 6 steps, 3 seeds, cfg 1.5 and no cfg (s2_sampler.npz layout)
    param_order_nodecoder.json   named_parameters() of the reference for DiT-S/2 and DiT-XL/2 (name, shape, requires_grad)

    python tests/golden/make_golden_nodecoder.py            # rewrites the four files
"""
import copy
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden import make_golden as MG  # noqa: E402  (imports the reference)

O = MG.O


def build_ref(model_type, R, P, use_decoder=False):
    net = MG.ref_m.Precond_models['edm'](img_resolution=R, img_channels=4, num_classes=1000, model_type=model_type,
                                         use_decoder=use_decoder, mae_loss_coef=0.1, pad_cls_token=False)
    net.load_state_dict(P, strict=True)
    return net


def gen_train_nodecoder(tag, model_type, R, B, seed, mask_ratio):
    cfg = O.make_cfg(model_type, img_resolution=R, use_decoder=False)
    P = O.init_params(cfg, seed=seed, dezero=True)
    net = build_ref(model_type, R, P)
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
    loss = MG.Losses['edm']()(net=wrapped, images=images, labels=labels, mask_ratio=mask_ratio, mae_loss_coef=0.1)
    out = dict(seed=np.int64(seed), B=np.int64(B), R=np.int64(R), mask_ratio=np.float64(mask_ratio), images=images.numpy(),
               cls=cls.numpy(), keep=keep.numpy(), rnd_normal=rnd_normal.numpy(), noise=noise.numpy(),
               mask_noise=mask_noise.numpy(), loss=loss.detach().numpy())
    with torch.no_grad():
        mdict = {k: torch.from_numpy(v) for k, v in O.get_mask_from_noise(mask_noise.numpy(), mask_ratio).items()}
        sigma = (rnd_normal * 1.2 - 1.2).exp()
        out['D_yn'] = net(images + noise * sigma, sigma, labels, mask_ratio=mask_ratio, mask_dict=mdict)['x'].numpy()
    names = [k for k in P if k not in O.NON_TRAINABLE]
    out['param_names'] = np.array(names)
    out['param_sums'] = np.stack([MG.checks(P[k])[0] for k in names])
    loss.mean().backward()
    sd = dict(net.named_parameters())
    assert all(sd[k].grad is not None for k in names), 'a trainable parameter of the reference got no gradient'
    gc = [MG.checks(sd[k].grad) for k in names]
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


def gen_sampler_nodecoder(tag='nd_sampler', model_type='DiT-S/2', R=16, seeds=(300, 301, 302), num_steps=6, cfg_scale=1.5, seed=23):
    cfg = O.make_cfg(model_type, img_resolution=R, use_decoder=False)
    P = O.init_params(cfg, seed=seed, dezero=True)
    net = build_ref(model_type, R, P)
    net.eval()
    seeds = list(seeds)
    rnd = MG.StackedRandomGenerator('cpu', seeds)
    latents = rnd.randn([len(seeds), 4, R, R])
    cls = rnd.randint(1000, size=[len(seeds)])
    labels = torch.eye(1000)[cls]
    with torch.no_grad():
        z = MG.ref_edm_sampler(net, latents.float(), labels.float(), randn_like=rnd.randn_like, cfg_scale=cfg_scale,
                               num_steps=num_steps)
        z_nocfg = MG.ref_edm_sampler(net, latents.float(), labels.float(), randn_like=rnd.randn_like, cfg_scale=None,
                                     num_steps=num_steps)
    np.savez_compressed(os.path.join(HERE, f'{tag}.npz'), seed=np.int64(seed), seeds=np.array(seeds), R=np.int64(R),
                        latents=latents.numpy(), cls=cls.numpy(), num_steps=np.int64(num_steps),
                        cfg_scale=np.float64(cfg_scale), z=z.numpy(), z_nocfg=z_nocfg.numpy())
    print(f'{tag}.npz written; z std', z.std().item())


def gen_param_order_nodecoder():
    out = {}
    for mt in ('DiT-S/2', 'DiT-XL/2'):
        net = MG.ref_m.Precond_models['edm'](img_resolution=32, img_channels=4, num_classes=1000, model_type=mt,
                                             use_decoder=False, mae_loss_coef=0.1, pad_cls_token=False)
        out[mt] = [[n, list(p.shape), bool(p.requires_grad)] for n, p in net.named_parameters()]
    with open(os.path.join(HERE, 'param_order_nodecoder.json'), 'w') as f:
        json.dump(out, f)
    print('param_order_nodecoder.json written')


JOBS = {
    's2nd_train': lambda: gen_train_nodecoder('s2nd_train', 'DiT-S/2', 16, 4, seed=21, mask_ratio=0.64),
    's4nd_train': lambda: gen_train_nodecoder('s4nd_train', 'DiT-S/4', 32, 4, seed=22, mask_ratio=0.5),
    'nd_sampler': gen_sampler_nodecoder,
    'param_order_nodecoder': gen_param_order_nodecoder,
}

if __name__ == '__main__':
    for job in (sys.argv[1:] or list(JOBS)):
        JOBS[job]()
