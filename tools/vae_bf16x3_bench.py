"""Throughput of the autoencoder at `precision='bf16x3'` (fp32-accurate) beside the default 'bf16', with synthetic weights,
in ONE process:

  end to end   decode img/s at 256^2 and 512^2 (latent sides 32, 64) and encode img/s at 256^2, batch 16, for three routes:
               'bf16', 'bf16x3' (implicit-GEMM 3x3 convolutions, mdt_conv3x3_bf16x3_nhwc) and 'bf16x3' with every stride-1 3x3
               convolution forced through a materialised fp32 im2col matrix + mdt_gemm_bf16x3 (MDT_VAE_X3_IM2COL=1; the
               encoder's three stride-2 convolutions have no im2col writer and stay implicit).  The routes alternate inside
               each of `--repeats` rounds; a figure is the median round, its spread (max - min) / median.
  per shape    every 3x3 convolution shape of the 256^2 decoder: TFLOP/s (2 M N K, the fp32-equivalent work) of the implicit
               kernel beside mdt_gemm_bf16x3 on a materialised matrix of the same M, N, K (which leaves out the time to
               write that matrix).
  accuracy     decode / encode error of both precisions against the fp64 fixture (tests/golden/vae_f32.npz), as
               tests/test_70_vae_f32_gpu.py measures it.

HIP events around `--iters` calls after `--warmup` calls.  Ends with the verdict the route exists for: the implicit route must
beat the im2col route by more than the im2col route's own spread.

    python tools/vae_bf16x3_bench.py [--batch 16] [--iters 3] [--warmup 1] [--repeats 3] [--out profiles/vae_bf16x3_bench.txt]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from maskdit_amd import autoencoder as AE  # noqa: E402
from maskdit_amd import ops  # noqa: E402
from maskdit_amd._lib import call  # noqa: E402

ROUTES = ('bf16', 'bf16x3', 'bf16x3-im2col')
# (Hi, C, Cout, up) of the 3x3 convolutions of the decoder at a 32 x 32 latent, conv_in (an im2col GEMM on both routes) left out
DEC_SHAPES = [(32, 512, 512, 0), (32, 512, 512, 1), (64, 512, 512, 0), (64, 512, 512, 1), (128, 512, 256, 0), (128, 256, 256, 0),
              (128, 256, 256, 1), (256, 256, 128, 0), (256, 128, 128, 0), (256, 128, 3, 0)]


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / iters


def set_route(vae, route):
    vae.set_precision('bf16' if route == 'bf16' else 'bf16x3')
    AE.X3_FORCE_IM2COL = route == 'bf16x3-im2col'


def end_to_end(vae, say, a):
    dev = 'cuda'
    g = torch.Generator(device=dev).manual_seed(1)
    work = [('decode 256^2', lambda x: vae.decode(x), torch.randn(a.batch, 4, 32, 32, device=dev, generator=g) * 0.5),
            ('decode 512^2', lambda x: vae.decode(x), torch.randn(a.batch, 4, 64, 64, device=dev, generator=g) * 0.5),
            ('encode 256^2', lambda x: vae.encode_moments(x),
             torch.randint(0, 256, (a.batch, 256, 256, 3), device=dev, dtype=torch.uint8, generator=g))]
    verdicts = []
    for name, fn, x in work:
        ips = {r: [] for r in ROUTES}
        for rep in range(a.repeats):
            for r in ROUTES:
                set_route(vae, r)
                ms = timed(lambda: fn(x), a.iters, a.warmup if rep == 0 else 1)
                ips[r].append(a.batch / (ms / 1e3))
        med = {r: statistics.median(v) for r, v in ips.items()}
        spread = {r: (max(v) - min(v)) / med[r] for r, v in ips.items()}
        for r in ROUTES:
            say(f'{name} batch {a.batch} {r:14s}: {med[r]:9.1f} img/s (rounds {" ".join(f"{v:.1f}" for v in ips[r])}; spread {100 * spread[r]:.1f} %)')
        gain = med['bf16x3'] / med['bf16x3-im2col'] - 1
        ok = gain > spread['bf16x3-im2col']
        verdicts.append(ok)
        say(f"{name}: implicit / im2col = {1 + gain:.3f} (im2col spread {100 * spread['bf16x3-im2col']:.1f} %: "
            f"{'implicit route faster beyond the spread' if ok else 'NOT faster beyond the spread'}); bf16 / bf16x3 = {med['bf16'] / med['bf16x3']:.2f}")
        vae.release_workspace()
    set_route(vae, 'bf16')
    return all(verdicts)


def per_shape(say, a):
    dev, st, B = 'cuda', ops.stream_ptr(), a.batch
    g = torch.Generator(device=dev).manual_seed(2)
    for Hi, C, Cout, up in DEC_SHAPES:
        Ho = Hi << up
        M, K, ldo = B * Ho * Ho, 9 * C, (Cout + 3) // 4 * 4
        raw = torch.zeros(32 + B * Hi * Hi * C, device=dev)
        raw[32:].normal_(generator=g)
        w = torch.randn(Cout, K, device=dev, generator=g) * K ** -0.5
        bias = torch.randn(Cout, device=dev, generator=g)
        out = torch.empty(M, ldo, device=dev)
        col = torch.randn(M, K, device=dev, generator=g)
        t_imp = timed(lambda: call('mdt_conv3x3_bf16x3_nhwc', raw[32:].data_ptr(), B, Hi, C, up, 0, w.data_ptr(), bias.data_ptr(), None,
                                   out.data_ptr(), ldo, Cout, st), a.iters, a.warmup)
        t_mat = timed(lambda: ops.gemm_bf16x3(col, w, out, M, Cout, K, ldo=ldo, bias=bias), a.iters, a.warmup)
        tf = 2.0 * M * Cout * K / 1e9
        say(f'conv {Hi:3d}^2{"x2" if up else "  "} C {C:3d} -> {Cout:3d} (M {M}, N {Cout}, K {K}): implicit {t_imp:8.3f} ms {tf / t_imp:6.1f} TF/s | '
            f'gemm_bf16x3 on the materialised matrix {t_mat:8.3f} ms {tf / t_mat:6.1f} TF/s')
        del raw, col, out


def accuracy(say):
    from oracle import vae_oracle as VO
    from tests import vae_encoder_ref as VE
    gdir = os.path.join(ROOT, 'tests', 'golden')
    f, gd, ge = (np.load(os.path.join(gdir, n)) for n in ('vae_f32.npz', 'vae_decode.npz', 'vae_encode.npz'))
    ref0 = torch.from_numpy(f['dec_lv0_crop']).double() / 127.5 - 1
    ref1 = torch.from_numpy(f['dec64_img1_sub'])
    absmax = max(ref0.abs().max().item(), ref1.abs().max().item())
    mom64 = torch.from_numpy(f['mom64_256'])
    dec = AE.get_model(None)
    dec.load_state_dict(VO.init_vae_params(seed=int(gd['seed'])))
    dec = dec.to('cuda')
    enc = AE.get_model(None, encoder=True)
    enc.load_state_dict({**AE.synthetic_state_dict(1, encoder=False), **VE.init_vae_encoder_params(int(ge['seed']))})
    enc = enc.to('cuda')
    say(f"reference fp32 vs fp64 (fixture): decode {float(f['dec_e_ref']):.3e}, encode {float(f['enc_e_ref']):.3e} of max")
    for r in ROUTES:
        set_route(dec, r)
        set_route(enc, r)
        x = dec.decode(torch.from_numpy(gd['z']).cuda()).double().cpu()
        e_dec = max((x[0, :, 64:192, 64:192] - ref0).abs().max().item(), (x[1, :, ::4, ::4] - ref1).abs().max().item()) / absmax
        mom = enc.encode_moments(torch.from_numpy(ge['img256'])[None].cuda()).double().cpu()
        e_enc = ((mom[0] - mom64).abs().max() / mom64.abs().max()).item()
        say(f'{r:14s} vs fp64: decode {e_dec:.3e}, encode {e_enc:.3e} of max')
    set_route(dec, 'bf16')


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vae_bf16x3_bench.txt'))
    a = ap.parse_args(argv)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f'tools/vae_bf16x3_bench.py --batch {a.batch} --iters {a.iters} --warmup {a.warmup} --repeats {a.repeats} on '
        f'{torch.cuda.get_device_name(0)}; synthetic weights')
    accuracy(say)
    vae = AE.get_model(None, encoder=True)
    vae.load_state_dict(AE.synthetic_state_dict(0))
    vae = vae.to('cuda')
    ok = end_to_end(vae, say, a)
    del vae
    torch.cuda.empty_cache()
    per_shape(say, a)
    say(f"verdict: the implicit route {'beats' if ok else 'DOES NOT beat'} the materialised-im2col route beyond its run-to-run spread on every workload")
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
