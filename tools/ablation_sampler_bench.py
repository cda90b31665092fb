"""Warm, graph-replayed ablation_sampler against edm_sampler in one process: XL/2 (random init, as tools/sampler_bench.py),
50 steps, batch 64, cfg 1.5, at 'bf16' and 'fp32'.  ablation_sampler(solver='heun', discretization='edm',
schedule='linear', scaling='none') makes the same 99 evaluations as edm_sampler; the two alternate, REPS runs each, so the
box's run-to-run spread shows next to their ratio.  Euler (50 evaluations) and VP/VP/VP are timed once.

    python tools/ablation_sampler_bench.py [steps = 50] [batch = 64] [out = profiles/ablation_sampler_bench.txt]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import maskdit_amd as M  # noqa: E402
from maskdit_amd import _lib  # noqa: E402

REPS = {'bf16': 5, 'fp32': 2}
HEUN_EDM = dict(solver='heun', discretization='edm', schedule='linear', scaling='none')
OTHERS = {'ablation euler/edm/linear/none': dict(solver='euler', discretization='edm', schedule='linear', scaling='none'),
          'ablation heun/vp/vp/vp': dict(solver='heun', discretization='vp', schedule='vp', scaling='vp')}


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    z = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3, z


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    sb = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, 'profiles', 'ablation_sampler_bench.txt')
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    net = M.Precond_models['edm'](img_resolution=32, img_channels=4, num_classes=1000, model_type='DiT-XL/2', use_decoder=True,
                                  mae_loss_coef=0.1, pad_cls_token=False).to(dev)
    net.eval()
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() >= 2:
                p.normal_(0.0, p.shape[-1] ** -0.5)
    gs = torch.Generator(device=dev).manual_seed(7)
    lat = torch.randn(sb, 4, 32, 32, device=dev, generator=gs)
    lab = torch.eye(1000, device=dev)[torch.randint(0, 1000, (sb,), device=dev, generator=gs)]
    lines = [f'XL/2, {steps} steps, cfg 1.5, batch {sb}, hipGraph replay, one process; kernel sources {_lib.source_hash()}',
             f'{"precision":>9} {"sampler":<32} {"runs samples/s":<48} {"mean":>7}']
    for prec, reps in REPS.items():
        edm = lambda: M.edm_sampler(net, lat, lab, cfg_scale=1.5, num_steps=steps, precision=prec)  # noqa: E731
        abl = lambda: M.ablation_sampler(net, lat, lab, cfg_scale=1.5, num_steps=steps, precision=prec, **HEUN_EDM)  # noqa: E731
        edm(), abl()  # plans, graph captures, warm-up at the measured step count
        res = {'edm_sampler': [], 'ablation heun/edm/linear/none': []}
        for _ in range(reps):
            for name, fn in (('edm_sampler', edm), ('ablation heun/edm/linear/none', abl)):
                t, z = timed(fn)
                res[name].append(sb / t)
                print(f'{prec} {name}: {sb / t:.3f} samples/s', flush=True)
        d = float((z - edm()).abs().max() / z.abs().max())
        for name, kw in OTHERS.items():
            M.ablation_sampler(net, lat, lab, cfg_scale=1.5, num_steps=steps, precision=prec, **kw)
            t, _ = timed(lambda: M.ablation_sampler(net, lat, lab, cfg_scale=1.5, num_steps=steps, precision=prec, **kw))
            res[name] = [sb / t]
        for name, v in res.items():
            lines.append(f'{prec:>9} {name:<32} {" ".join(f"{x:.3f}" for x in v):<48} {sum(v) / len(v):7.3f}')
        e, a = res['edm_sampler'], res['ablation heun/edm/linear/none']
        spread = (max(e) - min(e)) / (sum(e) / len(e))
        lines.append(f'{prec:>9} ablation/edm samples/s {sum(a) / sum(e):.4f} (worst pair {min(x / y for x, y in zip(a, e)):.4f}); '
                     f'edm_sampler same-run spread {100 * spread:.2f} %; rel-to-max difference of the two results {d:.2e}')
        M.sampler.release_graphs()
    text = '\n'.join(lines)
    print(text)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
