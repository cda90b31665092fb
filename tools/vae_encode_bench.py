"""Throughput of the VAE encoder (FrozenAutoencoderKL.encode_moments) with synthetic weights: img/s and TFLOP/s at batch
64 for 256^2 and 512^2 images (uint8 input, the extraction tool's form), HIP events around `--iters` calls after
`--warmup` calls.  FLOP count from the layer shapes (2 * M * N * K per convolution / GEMM, attention included).

    python tools/vae_encode_bench.py [--sides 256 512] [--batch 64] [--iters 10] [--warmup 3] [--out FILE.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from maskdit_amd import autoencoder as AE  # noqa: E402


def encoder_flops(R):
    """FLOP of one R x R image through encode_moments (convolutions, 1x1 GEMMs, attention score / value GEMMs)."""
    f = 2 * R * R * 27 * AE.CH  # conv_in
    H, c = R, AE.CH
    for i_level, mult in enumerate(AE.CH_MULT):
        cout = AE.CH * mult
        for _ in range(AE.NUM_RES_BLOCKS):
            f += 2 * H * H * (9 * c * cout + 9 * cout * cout + (c * cout if c != cout else 0))
            c = cout
        if i_level != len(AE.CH_MULT) - 1:
            H //= 2
            f += 2 * H * H * 9 * c * c
    T = H * H
    f += 2 * 2 * T * 9 * c * c * 2                      # mid.block_1, mid.block_2
    f += 2 * T * c * c * 4 + 2 * 2 * T * T * c          # q, k, v, proj_out + QK^T, PV
    f += 2 * T * 9 * c * 2 * AE.Z_CH + 2 * T * 64        # conv_out, quant_conv
    return f


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--sides', type=int, nargs='+', default=[256, 512])
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default='')
    a = ap.parse_args(argv)
    dev = 'cuda'
    vae = AE.get_model(None, encoder=True)
    vae.load_state_dict(AE.synthetic_state_dict(0))
    vae = vae.to(dev)
    res = []
    for R in a.sides:
        g = torch.Generator(device=dev).manual_seed(R)
        x = torch.randint(0, 256, (a.batch, R, R, 3), device=dev, dtype=torch.uint8, generator=g)
        for _ in range(a.warmup):
            vae.encode_moments(x)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.iters):
            mom = vae.encode_moments(x)
        t1.record()
        t1.synchronize()
        ms = t0.elapsed_time(t1) / a.iters
        assert bool(torch.isfinite(mom).all())
        ips = a.batch / (ms / 1e3)
        gf = encoder_flops(R) / 1e9
        r = dict(side=R, batch=a.batch, chunk=vae.encode_chunk(R), ms_per_batch=round(ms, 3), img_per_s=round(ips, 1),
                 gflop_per_img=round(gf, 1), tflops=round(ips * gf / 1e3, 1))
        print(json.dumps(r))
        res.append(r)
        vae.release_workspace()
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
