"""Decoder-less models (use_decoder=False) on one MI355X: what the missing decoder buys, and what the two kernels of
csrc/final_keep.hip cost.

  kernels  mdt_final_keep_fwd / mdt_final_keep_bwd at the DiT-XL/2 batch-1024 shapes (D 1152, T 256; masked: 128 kept rows
           per sample, unmasked: 256) beside their HBM floor -- x read once plus F (forward) or dx (backward) written once,
           at 5.7 TB/s
  train    DiT-XL/2 on a 32^2 latent, bf16 training step, mask ratio 0.5 and 0: without the decoder beside with it, in
           the same process
  sampler  the 50-step edm_sampler (cfg 1.5, 'bf16') at batch 64, both models

    python tools/nodecoder_bench.py [--out profiles/nodecoder_bench.txt] [--batch 256]

Run without --part, the tool starts one child process per part, each under its own time limit, and stops at the first
part that fails.  Each figure is the best of three groups of back-to-back launches between two events, after three warm-up
launches (kernels: ten launches a group; whole steps: three).
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = 'cuda'
HBM = 5.7e12
PARTS = (('kernels', 120), ('train', 300), ('sampler', 240))  # (name, time limit of the child in seconds)


def timed(fn, reps=10, groups=3):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    best = float('inf')
    for _ in range(groups):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / reps)
    return best * 1e3  # us


def kernels(a, lines):
    import torch
    import maskdit_amd as M
    from maskdit_amd._lib import call
    st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    B, T, D, Cc, p, R = 1024, 256, 1152, 4, 2, 32
    O_ = p * p * Cc
    lines.append(f'-- kernels at the XL/2 batch-{B} shapes (D {D}, T {T}, patch vector {O_}); floor = (x + F | dx) bytes at 5.7 TB/s')
    for name, L in (('masked 0.5', 128), ('unmasked', T)):
        Lp = (L + 63) // 64 * 64
        x = torch.randn(B * Lp, D, device=DEV)
        mod, dmod = torch.randn(B, 2 * D, device=DEV) * 0.1, torch.zeros(B, 2 * D, device=DEV)
        W, b = torch.randn(O_, D, device=DEV) * 0.03, torch.randn(O_, device=DEV)
        Fo, dF = torch.empty(B, Cc, R, R, device=DEV), torch.randn(B, Cc, R, R, device=DEV)
        stats, dx = torch.empty(B * Lp, 2, device=DEV), torch.empty(B * Lp, D, device=DEV)
        dW, db = torch.zeros(O_, D, device=DEV), torch.zeros(O_, device=DEV)
        ids = M.get_mask(B, T, 1 - L / T, DEV)['ids32'].data_ptr() if L < T else None
        fwd = timed(lambda: call('mdt_final_keep_fwd', x.data_ptr(), mod.data_ptr(), mod.data_ptr() + 4 * D, 2 * D, W.data_ptr(),
                                 b.data_ptr(), ids, 2 * T, Fo.data_ptr(), stats.data_ptr(), B, T, L, Lp, D, Cc, p, st()))
        bwd = timed(lambda: call('mdt_final_keep_bwd', dF.data_ptr(), x.data_ptr(), stats.data_ptr(), mod.data_ptr(),
                                 mod.data_ptr() + 4 * D, 2 * D, W.data_ptr(), ids, 2 * T, dx.data_ptr(), dW.data_ptr(), db.data_ptr(),
                                 dmod.data_ptr(), dmod.data_ptr() + 4 * D, 2 * D, B, T, L, Lp, D, Cc, p, st()))
        f_floor = (4 * B * L * D + 4 * B * Cc * R * R) / HBM * 1e6
        b_floor = (4 * B * L * D + 4 * B * Lp * D) / HBM * 1e6
        lines.append(f'   {name:11s} final_keep_fwd {fwd:8.1f} us  floor {f_floor:6.1f} us  ({fwd / f_floor:4.1f}x)')
        lines.append(f'   {name:11s} final_keep_bwd {bwd:8.1f} us  floor {b_floor:6.1f} us  ({bwd / b_floor:4.1f}x)   (two launches: dx, dW)')


def _net(use_decoder):
    import maskdit_amd as M
    return M.Precond_models['edm'](img_resolution=32, img_channels=4, num_classes=1000, model_type='DiT-XL/2',
                                   use_decoder=use_decoder, mae_loss_coef=0.1, pad_cls_token=False).to(DEV)


def train(a, lines):
    import torch
    import maskdit_amd as M
    B = a.batch
    g = torch.Generator(device=DEV).manual_seed(0)
    images = 0.5 * torch.randn(B, 4, 32, 32, device=DEV, generator=g)
    labels = torch.zeros(B, 1000, device=DEV)
    labels[torch.arange(B), torch.randint(0, 1000, (B,), device=DEV, generator=g)] = 1
    loss_fn = M.Losses['edm']()
    lines.append(f'-- DiT-XL/2, 32^2 latent, bf16 training step (forward + backward + FusedAdam) at batch {B}')
    res = {}
    for use_decoder in (False, True):
        net = _net(use_decoder).train()
        opt = M.FusedAdam(net.parameters(), lr=1e-4)
        n_par = sum(q.numel() for q in net.parameters() if q.requires_grad)
        for ratio in (0.5, 0.0):
            def step():
                opt.zero_grad(set_to_none=True)
                loss_fn(net, images, labels, mask_ratio=ratio, mae_loss_coef=0.1).mean().backward()
                opt.step()
            us = timed(step, reps=3, groups=3)
            res[use_decoder, ratio] = us
            lines.append(f'   {"with decoder" if use_decoder else "no decoder":13s} ({n_par / 1e6:6.1f} M parameters)  mask ratio {ratio:3.1f}: '
                         f'{us / 1e3:8.2f} ms = {B / us * 1e6:8.1f} img/s')
        del net, opt
        torch.cuda.empty_cache()
    for ratio in (0.5, 0.0):
        lines.append(f'   mask ratio {ratio:3.1f}: the decoder-less step takes {res[False, ratio] / res[True, ratio]:5.3f} of the step with the decoder')


def sampler(a, lines):
    import torch
    import maskdit_amd as M
    n = 64
    g = torch.Generator(device=DEV).manual_seed(1)
    lat = torch.randn(n, 4, 32, 32, device=DEV, generator=g)
    labels = torch.zeros(n, 1000, device=DEV)
    labels[torch.arange(n), torch.randint(0, 1000, (n,), device=DEV, generator=g)] = 1
    lines.append(f"-- DiT-XL/2, 50-step edm_sampler, cfg 1.5, 'bf16', batch {n}")
    for use_decoder in (False, True):
        net = _net(use_decoder).eval()
        t = timed(lambda: M.edm_sampler(net, lat, labels, cfg_scale=1.5, num_steps=50), reps=1, groups=3)
        lines.append(f'   {"with decoder" if use_decoder else "no decoder":13s} {t / 1e3:8.1f} ms = {n / t * 1e6:7.2f} samples/s')
        del net
        M.sampler.release_graphs()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'nodecoder_bench.txt'))
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--part', choices=[n for n, _ in PARTS])
    a = ap.parse_args()
    if a.part:  # a child: one part, its lines on stdout
        lines = []
        dict(kernels=kernels, train=train, sampler=sampler)[a.part](a, lines)
        print('\n'.join(lines))
        return 0
    text = []
    for name, limit in PARTS:  # the parent never touches the GPU: one fresh process per part, each under its own limit
        r = subprocess.run(['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--part', name,
                            '--batch', str(a.batch)], capture_output=True, text=True)
        if r.returncode != 0:
            print(r.stdout[-2000:], r.stderr[-4000:], sep='\n')
            print(f'nodecoder_bench: part {name!r} ended with status {r.returncode}: stopping here')
            return r.returncode
        text.append(r.stdout.rstrip())
    import torch  # (the device name only)
    text.insert(0, f'nodecoder_bench: {torch.cuda.get_device_name(0)}')
    out = '\n'.join(text)
    print(out)
    with open(a.out, 'w') as f:
        f.write(out + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
