"""fp32-faithful path (csrc/f32path.hip): mdt_gemm_f32 per XL/2 inference shape + the three-launch attention, TF/s against
the 157.3 TFLOP/s fp32 matrix peak; beside it mdt_gemm_bf16x3 (the 'bf16x3' plan's Linear layers) in fp32-equivalent TF/s
(2 M N K / time) against its 417 TFLOP/s roof (2.5 PF bf16 / 6 products), also on the conditioning-path shapes (M = 128) the
plan routes to it.      python tools/f32_bench.py [rows = 32768]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from maskdit_amd import ops  # noqa: E402

PEAK = 157.3
X3_ROOF = 2500.0 / 6


def timed(fn, iters=5):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / iters


def main():
    M = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
    torch.manual_seed(0)
    print(f'{"shape":>34} {"epilogue":>9} {"us":>9} {"TF/s":>7} {"of peak":>8} | {"bf16x3 us":>9} {"TF/s":>7} {"of roof":>8} {"vs fp32":>8}')
    shapes = [(M, 3456, 1152, 'NONE', 'qkv'), (M, 1152, 1152, 'GATE_RES', 'proj'), (M, 4608, 1152, 'GELU', 'fc1'),
              (M, 1152, 4608, 'GATE_RES', 'fc2'), (M, 1536, 512, 'NONE', 'dec qkv'), (M, 512, 512, 'GATE_RES', 'dec proj'),
              (M, 2048, 512, 'GELU', 'dec fc1'), (M, 512, 2048, 'GATE_RES', 'dec fc2'), (M, 512, 1152, 'NONE', 'decoder_layer'),
              # conditioning path at the sampler's CFG-doubled batch 128: t-embedder, label table (K = num_classes), adaLN
              (128, 1152, 256, 'SILU', 't_emb 0'), (128, 1152, 1152, 'NONE', 't_emb 2'), (128, 1152, 1000, 'GATE_RES', 'y_emb'),
              (128, 221440, 1152, 'NONE', 'adaLN')]
    for M, N, K, epi, name in shapes:
        A = torch.randn(M, K, device='cuda')
        W = torch.randn(N, K, device='cuda') * K ** -0.5
        b = torch.randn(N, device='cuda')
        out = torch.empty(M, N, device='cuda')
        kw = dict(bias=b, epi=getattr(ops, 'F32EPI_' + epi))
        if epi == 'GATE_RES':
            rps = min(M, 256)
            kw.update(res=torch.randn(M, N, device='cuda'), gate=torch.randn(M // rps, N, device='cuda'), gate_ld=N, rows_per_sample=rps)
        us = timed(lambda: ops.gemm_f32(A, W, out, M, N, K, **kw))
        ux = timed(lambda: ops.gemm_bf16x3(A, W, out, M, N, K, **kw))
        tf, tx = 2.0 * M * N * K / us / 1e6, 2.0 * M * N * K / ux / 1e6
        print(f'{name + f" {M}x{N}x{K}":>34} {epi:>9} {us:9.1f} {tf:7.1f} {tf / PEAK:8.3f} | {ux:9.1f} {tx:7.1f} {tx / X3_ROOF:8.3f} {us / ux:7.2f}x')
    M = shapes[0][0]
    for H, hd, name in [(16, 72, 'encoder attention'), (16, 32, 'decoder attention')]:
        B, L = M // 256, 256
        qkv = torch.randn(B * L, 3 * H * hd, device='cuda')
        for three, tag in ((False, 'fused'), (True, '3 launch')):
            us = timed(lambda: ops.attention_f32(qkv, B, L, H, hd, three_launch=three))
            tf = 4.0 * B * H * L * L * hd / us / 1e6
            print(f'{name + f" B{B} L{L} H{H} hd{hd}":>34} {tag:>9} {us:9.1f} {tf:7.1f} {tf / PEAK:8.3f}')
    x = torch.randn(M, 1152, device='cuda')
    mod = torch.randn(M // 256, 3 * 1152, device='cuda')
    us = timed(lambda: ops.ln_modulate_f32(x, mod[:, :1152], mod[:, 2304:], 3456, 256))
    print(f'{"ln_modulate_f32 " + str(M) + "x1152":>34} {"":>9} {us:9.1f} {M * 1152 * 8 / us / 1e6:7.2f} TB/s')


if __name__ == '__main__':
    main()
