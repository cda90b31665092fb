"""Token-boundary kernels of the patch-4 / patch-8 models (csrc/patch.hip) on one MI355X, one process.

For DiT-XL/4 and DiT-XL/8 on a 64^2 latent at batch 256 (and DiT-XL/2 on a 32^2 latent, the same T = 256, for comparison):
  * time and effective bytes/s of the six boundary entries (tokenizer, de-tokenizer, loss; forward and backward);
  * beside each product kernel, the bare product of its plain composition on a PRE-GATHERED operand (mdt_gemm_f32 for
    the forward / data-gradient products, mdt_gemm_f32_tn for the weight gradients): the composition also needs a patch
    gather and, for the de-tokenizer, LayerNorm passes, so this column is a LOWER bound of the composition's time;
  * mdt_ln_modulate_f32 on the same rows as the HBM yardstick;
  * the whole bf16 training step (img/s), the 50-step sampler (samples/s) and the share of the step that the six
    boundary kernels take.

    python tools/patch_edge_bench.py [--out profiles/patch_edge_bench.txt] [--batch 256]

Each figure is the best of three groups of ten back-to-back launches between two events, after three warm-up launches.
"""
import argparse
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import maskdit_amd as M  # noqa: E402
from maskdit_amd import _lib  # noqa: E402
from maskdit_amd._lib import GemmF32Args, GemmF32TNArgs, call  # noqa: E402

DEV = 'cuda'


def st():
    return torch.cuda.current_stream().cuda_stream


def timed(fn, reps=10, groups=3):
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


def gemm_f32(A, Bw, out, Mr, N, K, b_kmajor=0):
    a = GemmF32Args()
    a.A, a.lda, a.B, a.ldb, a.b_kmajor = A.data_ptr(), K, Bw.data_ptr(), (N if b_kmajor else K), b_kmajor
    a.M, a.N, a.K, a.epi, a.out, a.ldo, a.rows_per_sample = Mr, N, K, _lib.F32EPI_NONE, out.data_ptr(), N, 1
    return lambda: call('mdt_gemm_f32', C.byref(a), st())


def gemm_tn(A, Bm, Cout, Mr, N1, N2):
    a = GemmF32TNArgs()
    a.A, a.lda, a.B, a.ldb, a.M, a.N1, a.N2 = A.data_ptr(), N1, Bm.data_ptr(), N2, Mr, N1, N2
    a.C, a.ldc, a.accumulate = Cout.data_ptr(), N2, 1
    n = int(_lib.lib().mdt_gemm_f32_tn_ws_floats(Mr, N1, N2, 1))
    ws = torch.empty(max(n, 4), device=DEV)
    a.ws, a.ws_floats = ws.data_ptr(), n
    return lambda: (ws, call('mdt_gemm_f32_tn', C.byref(a), st()))[1]


def boundary(p, R, B, D, lines):
    Cc, Dd = 4, 512
    T, K = (R // p) ** 2, 4 * p * p
    Mr = B * T
    x, dF = torch.randn(B, Cc, R, R, device=DEV), torch.randn(B, Cc, R, R, device=DEV)
    W, b, pos = torch.randn(D, K, device=DEV) * 0.05, torch.randn(D, device=DEV), torch.randn(T, D, device=DEV)
    tok, dtok = torch.empty(Mr, D, device=DEV), torch.randn(Mr, D, device=DEV)
    dW, db = torch.zeros(D, K, device=DEV), torch.zeros(D, device=DEV)
    xd = torch.randn(Mr, Dd, device=DEV)
    mod, dmod = torch.randn(B, 2 * Dd, device=DEV) * 0.1, torch.zeros(B, 2 * Dd, device=DEV)
    Wf, bf = torch.randn(K, Dd, device=DEV) * 0.05, torch.randn(K, device=DEV)
    Fo, stats = torch.empty(B, Cc, R, R, device=DEV), torch.empty(Mr, 2, device=DEV)
    dx, dWf, dbf = torch.empty(Mr, Dd, device=DEV), torch.zeros(K, Dd, device=DEV), torch.zeros(K, device=DEV)
    yn, y, Dn = torch.randn(B, Cc, R, R, device=DEV), torch.randn(B, Cc, R, R, device=DEV), torch.empty(B, Cc, R, R, device=DEV)
    coef = torch.rand(8, B, device=DEV) + 0.5
    mask = (torch.rand(B, T, device=DEV) < 0.5).float()
    loss, dl = torch.empty(B, device=DEV), torch.ones(B, device=DEV) / B
    pre = torch.randn(Mr, K, device=DEV)  # a pre-gathered [rows, K] operand for the bare products
    xn = torch.empty(Mr, Dd, device=DEV)
    img = 4 * B * Cc * R * R
    rows = {}
    rows['tokenizer fwd'] = (timed(lambda: call('mdt_patch_embed_fwd', x.data_ptr(), None, W.data_ptr(), b.data_ptr(), pos.data_ptr(), None, 0,
                                                tok.data_ptr(), B, Cc, R, p, T, D, st())), img + 4 * Mr * D,
                             timed(gemm_f32(pre, W, tok, Mr, D, K)) if K > 16 else None)
    rows['tokenizer bwd'] = (timed(lambda: call('mdt_patch_embed_bwd', x.data_ptr(), None, dtok.data_ptr(), None, 0, dW.data_ptr(), db.data_ptr(),
                                                B, Cc, R, p, T, D, st())), img + 4 * Mr * D,
                             timed(gemm_tn(dtok, pre, dW, Mr, D, K)) if K > 16 else None)
    rows['de-tokenizer fwd'] = (timed(lambda: call('mdt_final_fwd', xd.data_ptr(), mod.data_ptr(), mod.data_ptr() + 4 * Dd, 2 * Dd, Wf.data_ptr(),
                                                   bf.data_ptr(), Fo.data_ptr(), stats.data_ptr(), B, T, Dd, Cc, p, st())), img + 4 * Mr * Dd,
                                timed(gemm_f32(xd, Wf, pre, Mr, K, Dd)) if K > 16 else None)
    rows['de-tokenizer bwd'] = (timed(lambda: call('mdt_final_bwd', dF.data_ptr(), xd.data_ptr(), stats.data_ptr(), mod.data_ptr(), mod.data_ptr() + 4 * Dd,
                                                   2 * Dd, Wf.data_ptr(), dx.data_ptr(), dWf.data_ptr(), dbf.data_ptr(), dmod.data_ptr(),
                                                   dmod.data_ptr() + 4 * Dd, 2 * Dd, B, T, Dd, Cc, p, st())), img + 4 * Mr * Dd * (4 if K > 16 else 2),
                                (timed(gemm_f32(pre, Wf, dx, Mr, Dd, K, b_kmajor=1)) + timed(gemm_tn(pre, xd, dWf, Mr, K, Dd))) if K > 16 else None)
    rows['loss fwd'] = (timed(lambda: call('mdt_edm_loss_fwd', Fo.data_ptr(), yn.data_ptr(), y.data_ptr(), coef.data_ptr(), mask.data_ptr(), 0.1,
                                           Dn.data_ptr(), loss.data_ptr(), B, Cc, R, p, st())), 4 * img, None)
    rows['loss bwd'] = (timed(lambda: call('mdt_edm_loss_bwd', dl.data_ptr(), Dn.data_ptr(), yn.data_ptr(), y.data_ptr(), coef.data_ptr(),
                                           mask.data_ptr(), 0.1, dF.data_ptr(), B, Cc, R, p, st())), 4 * img, None)
    ln = timed(lambda: call('mdt_ln_modulate_f32', xd.data_ptr(), mod.data_ptr(), mod.data_ptr() + 4 * Dd, 2 * Dd, T, xn.data_ptr(), Mr, Dd, st()))
    lines.append(f'-- boundary kernels, patch {p}, R {R}, B {B}, D {D}: T {T}, patch vector {K}')
    for k, (us, nbytes, comp) in rows.items():
        c = f'   bare product of the composition {comp:9.1f} us  ({"fused not slower" if us <= comp else "FUSED SLOWER"})' if comp else ''
        lines.append(f'   {k:18s} {us:9.1f} us  {nbytes / us / 1e6:7.2f} TB/s effective{c}')
    lines.append(f'   {"ln_modulate_f32":18s} {ln:9.1f} us  {8 * Mr * Dd / ln / 1e6:7.2f} TB/s  (HBM yardstick, [B T, 512] rows)')
    return sum(v[0] for v in rows.values())


def whole(model, R, B, edge_us, lines):
    net = M.Precond_models['edm'](img_resolution=R, img_channels=4, num_classes=1000, model_type=model, use_decoder=True,
                                  mae_loss_coef=0.1, pad_cls_token=False).to(DEV)
    net.train()
    opt = M.FusedAdam(net.parameters(), lr=1e-4)
    g = torch.Generator(device=DEV).manual_seed(0)
    images = 0.5 * torch.randn(B, 4, R, R, device=DEV, generator=g)
    labels = torch.zeros(B, 1000, device=DEV)
    labels[torch.arange(B), torch.randint(0, 1000, (B,), device=DEV, generator=g)] = 1
    loss_fn = M.Losses['edm']()

    def step():
        opt.zero_grad(set_to_none=True)
        loss_fn(net, images, labels, mask_ratio=0.5, mae_loss_coef=0.1).mean().backward()
        opt.step()

    us = timed(step, reps=3, groups=3)
    lines.append(f'-- {model}, R {R}: training step {us / 1e3:8.2f} ms = {B / us * 1e6:8.1f} img/s at B {B}; boundary kernels {edge_us / 1e3:6.2f} ms '
                 f'= {100 * edge_us / us:5.2f} % of the step')
    net.eval()
    lat = torch.randn(16, 4, R, R, device=DEV, generator=g)
    t = timed(lambda: M.edm_sampler(net, lat, labels[:16], cfg_scale=1.5, num_steps=50), reps=1, groups=2)
    lines.append(f'   50-step sampler (cfg 1.5, bf16, 16 samples): {t / 1e3:8.1f} ms = {16 / t * 1e6:7.2f} samples/s')
    del net, opt
    M.sampler.release_graphs()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'patch_edge_bench.txt'))
    ap.add_argument('--batch', type=int, default=256)
    a = ap.parse_args()
    lines = [f'patch_edge_bench: {torch.cuda.get_device_name(0)}, batch {a.batch}']
    for model, p, R in (('DiT-XL/4', 4, 64), ('DiT-XL/8', 8, 64), ('DiT-XL/2', 2, 32)):
        edge = boundary(p, R, a.batch, 1152, lines)
        whole(model, R, a.batch, edge, lines)
    text = '\n'.join(lines)
    print(text)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
