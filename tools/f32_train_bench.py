#!/usr/bin/env python
"""fp32 training of the unmasked stage against the bf16 unmasked step, in ONE process with the two routes alternating, plus
the two GEMMs of the fp32 backward on the shapes of an encoder block:

    python tools/f32_train_bench.py [--batch 64] [--steps 6] [--warmup 2] [--model DiT-XL/2] [--res 32]

Writes profiles/f32_train_bench.txt.  Yardsticks: the 157 TFLOP/s fp32 matrix peak of the device and mdt_gemm_f32's own
0.78 of it in the sampler."""
import argparse
import ctypes as C
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import maskdit_amd as M  # noqa: E402
from maskdit_amd import _lib  # noqa: E402
from maskdit_amd._lib import GemmF32Args, GemmF32TNArgs  # noqa: E402

PEAK = 157.0


def time_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def gemm_rows(Mr, W, out):
    """weight-gradient (mdt_gemm_f32_tn) and data-gradient (mdt_gemm_f32, K-major weight) products of one encoder block"""
    st = torch.cuda.current_stream().cuda_stream
    L = _lib.lib()
    for name, n_out, n_in in [('qkv', 3 * W, W), ('proj', W, W), ('fc1', 4 * W, W), ('fc2', W, 4 * W)]:
        dY, X = torch.randn(Mr, n_out, device='cuda'), torch.randn(Mr, n_in, device='cuda')
        Wt, dW, dX = torch.randn(n_out, n_in, device='cuda'), torch.zeros(n_out, n_in, device='cuda'), torch.empty(Mr, n_in, device='cuda')
        n = int(L.mdt_gemm_f32_tn_ws_floats(Mr, n_out, n_in, 1))
        ws = torch.empty(max(n, 4), device='cuda')
        t = GemmF32TNArgs()
        t.A, t.lda, t.B, t.ldb, t.M, t.N1, t.N2 = dY.data_ptr(), n_out, X.data_ptr(), n_in, Mr, n_out, n_in
        t.C, t.ldc, t.accumulate, t.ws, t.ws_floats = dW.data_ptr(), n_in, 1, ws.data_ptr(), n
        g = GemmF32Args()
        g.A, g.lda, g.B, g.ldb, g.b_kmajor = dY.data_ptr(), n_out, Wt.data_ptr(), n_in, 1
        g.M, g.N, g.K, g.out, g.ldo, g.rows_per_sample = Mr, n_in, n_out, dX.data_ptr(), n_in, 1
        flop = 2.0 * Mr * n_out * n_in
        ms_t = time_ms(lambda: _lib.call('mdt_gemm_f32_tn', C.byref(t), st), 5)
        ms_g = time_ms(lambda: _lib.call('mdt_gemm_f32', C.byref(g), st), 5)
        out.append(f'  {name:5s} M={Mr} {n_out}x{n_in}: wgrad mdt_gemm_f32_tn {ms_t:8.3f} ms {flop / ms_t / 1e9:6.1f} TF/s '
                   f'({flop / ms_t / 1e9 / PEAK:.2f} of peak, {n // (n_out * n_in) if n else 1} chunks) | '
                   f'dgrad mdt_gemm_f32 {ms_g:8.3f} ms {flop / ms_g / 1e9:6.1f} TF/s ({flop / ms_g / 1e9 / PEAK:.2f} of peak)')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--steps', type=int, default=6)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--model', default='DiT-XL/2')
    ap.add_argument('--res', type=int, default=32)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'f32_train_bench.txt'))
    a = ap.parse_args()
    dev = 'cuda'
    torch.manual_seed(0)
    net = M.Precond_models['edm'](img_resolution=a.res, img_channels=4, num_classes=1000, model_type=a.model, use_decoder=True,
                                  mae_loss_coef=0.1, pad_cls_token=False).to(dev).train()
    with torch.no_grad():  # de-zero the adaLN / output layers so that every kernel sees ordinary numbers
        for p in net.parameters():
            if p.requires_grad and float(p.abs().max()) == 0:
                p.normal_(std=0.02)
    opt = M.FusedAdam(net.parameters(), lr=1e-5, adam_w_mode=True, weight_decay=0)
    loss_fn = M.Losses['edm']()
    B = a.batch
    x = torch.randn(B, 4, a.res, a.res, device=dev) * 0.5
    y = torch.zeros(B, 1000, device=dev)
    y[torch.arange(B), torch.randint(0, 1000, (B,), device=dev)] = 1

    def step(prec):
        net.set_train_precision(prec)
        opt.zero_grad(set_to_none=True)
        loss = loss_fn(net, x, y, mask_ratio=0, mae_loss_coef=0.1)
        loss.mean().backward()
        opt.step()
        return loss

    times = {'fp32': [], 'bf16': []}
    for i in range(a.warmup + a.steps):
        for prec in ('fp32', 'bf16'):  # alternating: both routes see the same clocks / temperature
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = step(prec)
            torch.cuda.synchronize()
            if i >= a.warmup:
                times[prec].append(time.perf_counter() - t0)
            assert bool(torch.isfinite(loss).all())
    sp = net.spec
    out = [f'f32_train_bench: {a.model} {a.res}x{a.res} latents (T = {sp.T}), batch {B}, unmasked, {a.steps} timed steps after '
           f'{a.warmup} warm-up, routes alternating in one process; device {torch.cuda.get_device_name(0)}']
    for prec in ('fp32', 'bf16'):
        ts = sorted(times[prec])
        med = ts[len(ts) // 2]
        out.append(f'  {prec} step (forward + backward + FusedAdam): median {med * 1e3:9.2f} ms  min {ts[0] * 1e3:9.2f} ms  '
                   f'{B / med:8.1f} img/s')
    f = sorted(times['fp32'])[len(times['fp32']) // 2] / sorted(times['bf16'])[len(times['bf16']) // 2]
    out.append(f'  fp32 / bf16 step time: {f:.1f}x')
    from maskdit_amd.engine import PassPlan
    fl = PassPlan.f32_train_floats(sp, B)
    out.append('  fp32 plan buffers: ' + ', '.join(f'{k} {4 * v / 2**20:.0f} MiB' for k, v in fl.items())
               + f'; {4 * sum(fl.values()) / B / 2**20:.0f} MiB per sample; allocated by the plan: '
               f'{net.engine().plan(B, False, True, None, "fp32").nbytes / 2**20:.0f} MiB')
    out.append(f'GEMMs of one encoder block backward (M = {B * sp.T} tokens, width {sp.D}); fp32 matrix peak {PEAK:.0f} TF/s, '
               'mdt_gemm_f32 in the sampler 0.78 of it:')
    del opt
    net.engine().release_plans()
    torch.cuda.empty_cache()
    gemm_rows(B * sp.T, sp.D, out)
    text = '\n'.join(out) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main()
