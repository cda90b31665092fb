"""Warm, graph-replayed EDM sampler throughput per network arithmetic, one process, one box: XL/2 (random init), 50 Heun
steps (99 evaluations of the CFG-doubled batch), cfg 1.5, batch 64 -- 'bf16', 'fp32' and 'bf16x3' -- with each result's
rel-to-max difference from the fp32 plan's.      python tools/sampler_bench.py [steps = 50] [batch = 64]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import maskdit_amd as M  # noqa: E402

GF_PER_EVAL = 251.6  # XL/2 at 256^2 (T = 256): 2 * MACs of one sample's forward, GFLOP


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    sb = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    net = M.Precond_models['edm'](img_resolution=32, img_channels=4, num_classes=1000, model_type='DiT-XL/2', use_decoder=True,
                                  mae_loss_coef=0.1, pad_cls_token=False).to(dev)
    net.eval()
    with torch.no_grad():  # adaLN-zero init would leave the blocks' branches at zero: give every weight some magnitude
        for p in net.parameters():
            if p.dim() >= 2:
                p.normal_(0.0, p.shape[-1] ** -0.5)
    gs = torch.Generator(device=dev).manual_seed(7)
    lat = torch.randn(sb, 4, 32, 32, device=dev, generator=gs)
    lab = torch.eye(1000, device=dev)[torch.randint(0, 1000, (sb,), device=dev, generator=gs)]
    evals = 2 * steps - 1
    res = {}
    for prec in ('bf16', 'fp32', 'bf16x3'):
        M.edm_sampler(net, lat, lab, cfg_scale=1.5, num_steps=2, precision=prec)  # plan + graph capture + warm-up
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        z = M.edm_sampler(net, lat, lab, cfg_scale=1.5, num_steps=steps, precision=prec)
        e1.record()
        torch.cuda.synchronize()
        res[prec] = (e0.elapsed_time(e1) / 1e3, z)
    z32 = res['fp32'][1]
    print(f'XL/2 {steps}-step Heun, cfg 1.5, batch {sb} ({evals} evaluations of batch {2 * sb}), hipGraph, one process')
    print(f'{"precision":>9} {"seconds":>8} {"samples/s":>10} {"TF/s":>7} {"vs fp32":>8} {"rel-to-max vs fp32":>19} {"finite":>6}')
    for prec, (t, z) in res.items():
        d = float((z - z32).abs().max() / z32.abs().max())
        tf = sb * evals * 2 * GF_PER_EVAL / t / 1e3
        print(f'{prec:>9} {t:8.3f} {sb / t:10.3f} {tf:7.1f} {res["fp32"][0] / t:7.2f}x {d:19.3e} {bool(torch.isfinite(z).all())!s:>6}')


if __name__ == '__main__':
    main()
