"""Patch sizes 4 and 8 (DiT-*/4, DiT-*/8) on the GPU: the token-boundary kernels of csrc/patch.hip, then the models end to
end through the public surface.

Kernel tests use the criterion of tests/test_80_f32_train_gpu.py: relative L2 error per tensor against torch in fp64,
    e_hip <= 4 e_ref,   e_ref = the same computation by torch (CPU) in fp32,
and every output sits inside a frame of sentinels that must survive the launch.  Accumulating outputs (`+=`) are
pre-filled and compared against pre-fill + result in both precisions.

End-to-end tests use the bounds and helpers of tests/test_10_engine_gpu.py (bf16 training, samplers), TOL_F32 of
tests/test_50_bf16x3_gpu.py ('fp32' / 'bf16x3' inference) and `_check` of test_80 (fp32 training).

Measured figures: none recorded yet -- every test prints its errors before it asserts (run with -s); DESIGN.md section 7.4.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import maskdit_amd as M
    from maskdit_amd import _lib
    from oracle import maskdit_oracle as O
    import tests.test_10_engine_gpu as T10
    import tests.test_80_f32_train_gpu as T80
    from tests.test_50_bf16x3_gpu import TOL_F32

DEV = 'cuda'
SENT = 12345.0


def _st():
    return torch.cuda.current_stream().cuda_stream


def _rel(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return ((a - ref).norm() / (ref.norm() + 1e-300)).item()


def _within(what, got, r32, r64):
    e_hip, e_ref = _rel(got, r64), _rel(r32, r64)
    print(f'[{what}] e_ref {e_ref:.3e}  e_hip {e_hip:.3e}  (ratio {e_hip / max(e_ref, 1e-300):.2f})')
    assert e_hip <= 4 * e_ref, f'{what}: e_hip {e_hip:.3e} > 4 e_ref {e_ref:.3e}'


class Framed:
    """A flat device buffer of `n` floats with `pad` sentinels on either side."""

    def __init__(self, n, pad=256, fill=None):
        self.buf = torch.full((n + 2 * pad,), SENT, device=DEV)
        self.n, self.pad = n, pad
        if fill is not None:
            self.view[:] = fill.to(DEV).flatten()

    @property
    def view(self):
        return self.buf[self.pad:self.pad + self.n]

    def ptr(self):
        return self.view.data_ptr()

    def intact(self):
        return bool((self.buf[:self.pad] == SENT).all()) and bool((self.buf[self.pad + self.n:] == SENT).all())

    def get(self, *shape):
        return self.view.cpu().view(*shape)


# ---------------------------------------------------------------------------------------------------------------------
# tokenizer

def _tokenizer_ref(dt, x, in_scale, W, b, pos, ids, p, dout, W0, b0):
    """tokens [B, L, D] and pre-fill + gradients by torch in `dt`"""
    Wl, bl = W.to(dt).clone().requires_grad_(True), b.to(dt).clone().requires_grad_(True)
    xs = x.to(dt) * (in_scale.to(dt).view(-1, 1, 1, 1) if in_scale is not None else 1)
    tok = F.conv2d(xs, Wl, bl, stride=p).flatten(2).transpose(1, 2) + pos.to(dt)[None]
    if ids is not None:
        tok = torch.gather(tok, 1, ids[:, :, None].expand(-1, -1, tok.shape[2]))
    tok.backward(dout.to(dt))
    return tok.detach(), W0.to(dt) + Wl.grad, b0.to(dt) + bl.grad


@pytest.mark.parametrize('p,R,D,B,gathered', [(4, 32, 384, 3, True), (4, 32, 384, 3, False), (8, 64, 384, 2, True),
                                              (8, 64, 384, 2, False), (8, 64, 1152, 1, False)])
def test_tokenizer_fwd_bwd_vs_fp64(p, R, D, B, gathered):
    C_, T = 4, (R // p) ** 2
    assert T == 64
    L = 24 if gathered else T  # 24: not a multiple of the 64-row token tile, B * L = 72 or 48 rows
    g = torch.Generator().manual_seed(p * 1000 + D + B + gathered)
    x = torch.randn(B, C_, R, R, generator=g)
    W, b = torch.randn(D, C_, p, p, generator=g) / (C_ * p * p) ** 0.5, torch.randn(D, generator=g)
    pos = torch.randn(T, D, generator=g)
    in_scale = None if gathered else torch.rand(B, generator=g) + 0.5
    ids = torch.stack([torch.randperm(T, generator=g)[:L] for _ in range(B)]) if gathered else None
    dout = torch.randn(B, L, D, generator=g)
    W0, b0 = torch.randn(D, C_, p, p, generator=g), torch.randn(D, generator=g)
    r64 = _tokenizer_ref(torch.float64, x, in_scale, W, b, pos, ids, p, dout, W0, b0)
    r32 = _tokenizer_ref(torch.float32, x, in_scale, W, b, pos, ids, p, dout, W0, b0)
    xd, Wd, bd, posd, dd = (t.to(DEV).contiguous() for t in (x, W, b, pos, dout))
    scd = in_scale.to(DEV) if in_scale is not None else None
    ids32 = torch.full((B, 2 * T), -1, dtype=torch.int32, device=DEV)  # (an unused slot of the table would index out of range)
    if gathered:
        ids32[:, :L] = ids.to(DEV)
    idp = ids32.data_ptr() if gathered else None
    out = Framed(B * L * D)
    _lib.call('mdt_patch_embed_fwd', xd.data_ptr(), scd.data_ptr() if scd is not None else None, Wd.data_ptr(), bd.data_ptr(),
              posd.data_ptr(), idp, 2 * T, out.ptr(), B, C_, R, p, L, D, _st())
    dW, db = Framed(D * C_ * p * p, fill=W0), Framed(D, fill=b0)
    _lib.call('mdt_patch_embed_bwd', xd.data_ptr(), scd.data_ptr() if scd is not None else None, dd.data_ptr(), idp, 2 * T,
              dW.ptr(), db.ptr(), B, C_, R, p, L, D, _st())
    torch.cuda.synchronize()
    assert out.intact() and dW.intact() and db.intact(), 'a tokenizer kernel wrote outside its output'
    tag = f'p={p} D={D} B={B} {"gathered" if gathered else "full"}'
    _within(f'tokenizer fwd {tag}', out.get(B, L, D), r32[0], r64[0])
    _within(f'tokenizer dW {tag}', dW.get(D, C_, p, p), r32[1], r64[1])
    _within(f'tokenizer dbias {tag}', db.get(D), r32[2], r64[2])


# ---------------------------------------------------------------------------------------------------------------------
# de-tokenizer

def _final_ref(dt, x, mod, W, b, dF, W0, b0, dmod0, B, T, Dd, p):
    C_, w = 4, int(T ** 0.5)
    xs, ms, Wl, bl = (t.to(dt).clone().requires_grad_(True) for t in (x, mod, W, b))
    sh, sc = ms[:, :Dd], ms[:, Dd:2 * Dd]
    mean = xs.mean(-1, keepdim=True)
    rstd = (xs.var(-1, unbiased=False, keepdim=True) + 1e-6).rsqrt()
    xn = ((xs - mean) * rstd).view(B, T, Dd) * (1 + sc[:, None]) + sh[:, None]
    o = xn @ Wl.t() + bl  # [B, T, p * p * C]
    Fo = torch.einsum('nhwpqc->nchpwq', o.view(B, w, w, p, p, C_)).reshape(B, C_, w * p, w * p)
    Fo.backward(dF.to(dt))
    stats = torch.stack([mean.detach().flatten(), rstd.detach().flatten()], 1)
    return [Fo.detach(), stats, xs.grad, W0.to(dt) + Wl.grad, b0.to(dt) + bl.grad, dmod0.to(dt) + ms.grad]


@pytest.mark.parametrize('p', [4, 8])
def test_detokenizer_fwd_bwd_vs_fp64(p):
    B, T, Dd, C_ = 2, 64, 512, 4
    O_, R = p * p * C_, 8 * p
    ld = 2 * Dd + 8  # modulation rows at a pitch that is not 2 Dd: the tail columns must keep their pre-fill
    g = torch.Generator().manual_seed(90 + p)
    x = torch.randn(B * T, Dd, generator=g) * 1.5 + 0.3
    mod = torch.randn(B, ld, generator=g) * 0.5
    W, b = torch.randn(O_, Dd, generator=g) / Dd ** 0.5, torch.randn(O_, generator=g)
    dF = torch.randn(B, C_, R, R, generator=g)
    W0, b0, dmod0 = torch.randn(O_, Dd, generator=g), torch.randn(O_, generator=g), torch.randn(B, ld, generator=g)
    r64 = _final_ref(torch.float64, x, mod, W, b, dF, W0, b0, dmod0, B, T, Dd, p)
    r32 = _final_ref(torch.float32, x, mod, W, b, dF, W0, b0, dmod0, B, T, Dd, p)
    xd, md, Wd, bd, dFd = (t.to(DEV).contiguous() for t in (x, mod, W, b, dF))
    Fo, stats = Framed(B * C_ * R * R), Framed(2 * B * T)
    _lib.call('mdt_final_fwd', xd.data_ptr(), md.data_ptr(), md.data_ptr() + 4 * Dd, ld, Wd.data_ptr(), bd.data_ptr(), Fo.ptr(),
              stats.ptr(), B, T, Dd, C_, p, _st())
    torch.cuda.synchronize()
    assert Fo.intact() and stats.intact(), 'final_fwd wrote outside its outputs'
    _within(f'de-tokenizer F p={p}', Fo.get(B, C_, R, R), r32[0], r64[0])
    st = stats.get(B * T, 2)
    _within(f'de-tokenizer mean p={p}', st[:, 0], r32[1][:, 0], r64[1][:, 0])
    _within(f'de-tokenizer rstd p={p}', st[:, 1], r32[1][:, 1], r64[1][:, 1])
    dx, dW, db, dmod = Framed(B * T * Dd), Framed(O_ * Dd, fill=W0), Framed(O_, fill=b0), Framed(B * ld, fill=dmod0)
    _lib.call('mdt_final_bwd', dFd.data_ptr(), xd.data_ptr(), stats.ptr(), md.data_ptr(), md.data_ptr() + 4 * Dd, ld, Wd.data_ptr(),
              dx.ptr(), dW.ptr(), db.ptr(), dmod.ptr(), dmod.ptr() + 4 * Dd, ld, B, T, Dd, C_, p, _st())
    torch.cuda.synchronize()
    assert dx.intact() and dW.intact() and db.intact() and dmod.intact(), 'final_bwd wrote outside its outputs'
    dm = dmod.get(B, ld)
    assert torch.equal(dm[:, 2 * Dd:], dmod0[:, 2 * Dd:]), 'final_bwd touched modulation columns that are not its own'
    _within(f'de-tokenizer dx p={p}', dx.get(B * T, Dd), r32[2], r64[2])
    _within(f'de-tokenizer dW p={p}', dW.get(O_, Dd), r32[3], r64[3])
    _within(f'de-tokenizer dbias p={p}', db.get(O_), r32[4], r64[4])
    _within(f'de-tokenizer dshift p={p}', dm[:, :Dd], r32[5][:, :Dd], r64[5][:, :Dd])
    _within(f'de-tokenizer dscale p={p}', dm[:, Dd:2 * Dd], r32[5][:, Dd:2 * Dd], r64[5][:, Dd:2 * Dd])


# ---------------------------------------------------------------------------------------------------------------------
# loss

def _loss_ref(dt, Fx, yn, y, coef, mask, dl, p, mae_coef):
    cfg = dict(patch=p, C=4)
    Fg = Fx.to(dt).clone().requires_grad_(True)
    c_skip, c_out, wgt = (coef[i].to(dt).view(-1, 1, 1, 1) for i in (0, 1, 4))
    D = c_skip * yn.to(dt) + c_out * Fg
    l = wgt * (D - y.to(dt)) ** 2
    if mask is not None:
        l = F.avg_pool2d(l.mean(1), p).flatten(1)
        un = 1 - mask.to(dt)
        l = (l * un).sum(1) / un.sum(1) + mae_coef * O.mae_loss(cfg, yn.to(dt), D, mask.to(dt))
    else:
        l = l.mean(dim=[1, 2, 3])
    l.backward(dl.to(dt))
    return D.detach(), l.detach(), Fg.grad


@pytest.mark.parametrize('p,R', [(4, 32), (8, 64)])
def test_loss_fwd_bwd_vs_fp64(p, R):
    B, C_, T = 3, 4, 64
    g = torch.Generator().manual_seed(7 * p)
    Fx, y, noise = (torch.randn(B, C_, R, R, generator=g) for _ in range(3))
    sigma = torch.tensor([0.2, 1.1, 9.0]).view(B, 1, 1, 1)
    yn = 0.5 * y + noise * sigma
    s = sigma.flatten().double()
    coef = torch.zeros(8, B, dtype=torch.float64)
    coef[0], coef[1], coef[4] = 0.25 / (s ** 2 + 0.25), s * 0.5 / (s ** 2 + 0.25).sqrt(), (s ** 2 + 0.25) / (s * 0.5) ** 2
    coef = coef.float()  # the kernel's inputs ARE these fp32 values: both references start from them
    mask = torch.from_numpy(O.get_mask_from_noise(torch.rand(B, T, generator=g).numpy(), 0.5)['mask']).float()
    assert 0 < mask.sum() < B * T  # both kinds of patch
    dl = torch.randn(B, generator=g)
    Fd, ynd, yd, cd, md, dld = (t.to(DEV).contiguous() for t in (Fx, yn, 0.5 * y, coef, mask, dl))
    n = B * C_ * R * R
    for use_mask in (True, False):
        mk, mc = (mask, 0.1) if use_mask else (None, 0.0)
        r64 = _loss_ref(torch.float64, Fx, yn, 0.5 * y, coef, mk, dl, p, mc)
        r32 = _loss_ref(torch.float32, Fx, yn, 0.5 * y, coef, mk, dl, p, mc)
        D, loss, dF = Framed(n), Framed(B), Framed(n)
        _lib.call('mdt_edm_loss_fwd', Fd.data_ptr(), ynd.data_ptr(), yd.data_ptr(), cd.data_ptr(), md.data_ptr() if use_mask else None,
                  mc, D.ptr(), loss.ptr(), B, C_, R, p, _st())
        _lib.call('mdt_edm_loss_bwd', dld.data_ptr(), D.ptr(), ynd.data_ptr(), yd.data_ptr(), cd.data_ptr(),
                  md.data_ptr() if use_mask else None, mc, dF.ptr(), B, C_, R, p, _st())
        torch.cuda.synchronize()
        assert D.intact() and loss.intact() and dF.intact(), 'a loss kernel wrote outside its outputs'
        tag = f'p={p} {"masked" if use_mask else "unmasked"}'
        _within(f'loss D {tag}', D.get(B, C_, R, R), r32[0], r64[0])
        _within(f'loss {tag}', loss.get(B), r32[1], r64[1])
        _within(f'loss dF {tag}', dF.get(B, C_, R, R), r32[2], r64[2])


# ---------------------------------------------------------------------------------------------------------------------
# end to end

@pytest.mark.parametrize('name,model,R', [('s4_train.npz', 'DiT-S/4', 32), ('s8_train.npz', 'DiT-S/8', 64)])
def test_masked_train_step_vs_oracle_and_fixture(golden_dir, name, model, R):
    """B = 4, mask 0.5: losses and EVERY gradient against the oracle and the reference's fixture, then one FusedAdam step
    (the checks of test_10's test_s2_train_step_vs_oracle_and_fixture)."""
    g = T10._load(golden_dir, name)
    cfg, P, net = T10._build(model, R, int(g['seed']))
    opt = M.FusedAdam(net.parameters(), lr=1e-4, adam_w_mode=True, weight_decay=0)
    assert opt._arena is net.engine()
    opt.zero_grad(set_to_none=True)
    loss, md = T10._run_loss(net, g)
    loss.mean().backward()
    ref_md = O.get_mask_from_noise(g['mask_noise'], 0.5)
    assert np.array_equal(md['ids_keep'].cpu().numpy(), ref_md['ids_keep'])
    D = net.engine().plan(int(g['B']), True, True, md['ids_keep'].shape[1]).buf['D']
    e = T10._relmax(D, torch.from_numpy(g['D_yn']))
    rl = ((loss.detach().cpu() - torch.from_numpy(g['loss'])).abs() / torch.from_numpy(g['loss']).abs()).max().item()
    print(f'[{name}] vs fixture: D_yn {e:.3e}, loss {rl:.3e}')
    assert e <= T10.TOL_D and rl <= T10.TOL_LOSS
    images, labels, rnd, noise, mnoise = T10._inputs(g)
    mdict = {k: torch.from_numpy(v) for k, v in ref_md.items()}
    loss_ref, D_ref, grads_ref = O.loss_and_grads(P, cfg, images, labels, rnd, noise, mdict, 0.1)
    assert torch.allclose(loss_ref, torch.from_numpy(g['loss']), rtol=1e-4, atol=1e-6)  # oracle == reference fixture
    rl = ((loss.detach().cpu() - loss_ref).abs() / loss_ref.abs()).max().item()
    assert rl <= T10.TOL_LOSS
    params = dict(net.named_parameters())
    names = [str(n) for n in g['param_names']]
    worst = ('', 0.0)
    for k, gr in grads_ref.items():
        got = params[k].grad
        assert got is not None, k
        num = (got.detach().cpu().double() - gr.double()).norm().item()
        den = gr.double().norm().item()
        if num / (den + 1e-12) > worst[1]:
            worst = (k, num / (den + 1e-12))
        assert num <= T10.TOL_GRAD * den + 1e-7, f'{k}: grad rel L2 err {num / (den + 1e-12):.3e} (|g| = {den:.3e})'
        # the reference's own gradient norm of the same tensor
        gs = g['grad_sums'][names.index(k)]
        assert abs(got.detach().double().norm().item() - gs[2]) <= T10.TOL_GRAD * gs[2] + 1e-7, k
    print(f'[{name}] worst grad rel L2 err {worst[1]:.3e} at {worst[0]}')
    g_hip = {k: params[k].grad.detach().cpu().clone() for k in grads_ref}
    p_before = {k: params[k].detach().cpu().clone() for k in grads_ref}
    opt.step()
    from tests.golden.make_golden_idx import sample_idx
    bad = 0
    for i, k in enumerate(names):
        p, m, v = p_before[k].clone(), torch.zeros_like(p_before[k]), torch.zeros_like(p_before[k])
        O.adamw_step(p, g_hip[k], m, v, step=1, lr=1e-4)
        assert torch.allclose(params[k].detach().cpu(), p, rtol=1e-5, atol=1e-7), k
        idx = sample_idx(params[k].numel())
        got = params[k].detach().cpu().double().flatten()[idx].numpy()
        bad += int((np.abs(got - g['upd_samples'][i]) > 2.05e-4).sum())  # |step| <= lr = 1e-4 each way
    assert bad == 0


def test_s4_eval_cfg_and_sampler_three_precisions_vs_oracle():
    """DiT-S/4 on a 32^2 latent: eval forward, forward with CFG and a 6-step edm_sampler in 'bf16', 'fp32' and 'bf16x3'
    against the oracle; graph replay equals the direct loop where the existing S/2 tests assert it."""
    cfg, P, net = T10._build('DiT-S/4', 32, seed=5, train=False)
    gcpu = torch.Generator().manual_seed(1)
    x = torch.randn(3, 4, 32, 32, generator=gcpu) * 3
    sigma = torch.tensor([0.3, 2.0, 40.0])
    y = torch.zeros(3, 1000)
    y[torch.arange(3), torch.tensor([1, 500, 999])] = 1
    lat = torch.randn(3, 4, 32, 32, generator=gcpu)
    with torch.no_grad():
        ref = O.precond_forward(P, cfg, x, sigma, y, training=False)
        ref2 = O.precond_forward(P, cfg, x, torch.tensor(2.5), y, cfg_scale=1.5, training=False)
    zref = O.edm_sampler(P, cfg, lat, y, cfg_scale=1.5, num_steps=6)
    for prec in ('bf16', 'fp32', 'bf16x3'):
        net.set_eval_precision(prec)
        with torch.no_grad():
            e1 = T10._relmax(net(x.to(DEV), sigma.to(DEV), y.to(DEV))['x'], ref)
            e2 = T10._relmax(net(x.to(DEV), torch.tensor(2.5, dtype=torch.float64, device=DEV), y.to(DEV), 1.5)['x'], ref2)
        z = M.edm_sampler(net, lat.to(DEV), y.to(DEV), cfg_scale=1.5, num_steps=6, precision=prec)
        z_direct = M.edm_sampler(net, lat.to(DEV), y.to(DEV), cfg_scale=1.5, num_steps=6, precision=prec, use_graph=False)
        e3 = T10._relmax(z, zref)
        print(f'[S/4 {prec}] eval {e1:.2e}, cfg {e2:.2e}, 6-step sampler {e3:.2e}')
        if prec == 'bf16':
            assert e1 <= T10.TOL_D and e2 <= T10.TOL_D
            assert e3 <= 4e-3  # the bound of test_sampler_vs_reference_fixture: 11 bf16 network evaluations compound
            z_again = M.edm_sampler(net, lat.to(DEV), y.to(DEV), cfg_scale=1.5, num_steps=6, precision=prec)
            assert torch.equal(z, z_again)         # graph replay
            assert T10._relmax(z_direct, z) <= 5e-3  # (fp64 state algebra in torch: last bits amplified by bf16 rounding)
        else:
            assert e1 <= TOL_F32 and e2 <= TOL_F32 and e3 <= TOL_F32
            assert torch.equal(z, z_direct)
    net.set_eval_precision('bf16')
    za = M.ablation_sampler(net, lat.to(DEV), y.to(DEV), cfg_scale=1.5, num_steps=6, precision='fp32')
    print(f'[S/4] ablation_sampler (defaults = the EDM sampler) {T10._relmax(za, zref):.2e}')
    assert T10._relmax(za, zref) <= TOL_F32


def test_s4_fp32_unmasked_training_vs_oracle():
    """set_train_precision('fp32'), unmasked, DiT-S/4, R = 32, B = 2: test_80's criterion."""
    R, Bn = 32, 2
    cfg = O.make_cfg('DiT-S/4', img_resolution=R)
    P = O.init_params(cfg, seed=3, dezero=True)
    net = M.Precond_models['edm'](img_resolution=R, img_channels=4, num_classes=1000, model_type='DiT-S/4', use_decoder=True,
                                  mae_loss_coef=0.1, pad_cls_token=False).to(DEV)
    net.load_state_dict(P, strict=True)
    net.train()
    g = torch.Generator().manual_seed(4)
    images = torch.randn(Bn, 4, R, R, generator=g) * 0.5
    labels = torch.zeros(Bn, 1000)
    labels[torch.arange(Bn), torch.randint(0, 1000, (Bn,), generator=g)] = 1
    labels[0] = 0
    inp = (images, labels, torch.randn(Bn, 1, 1, 1, generator=g), torch.randn(Bn, 4, R, R, generator=g))
    loss64, grads64 = T80._oracle(P, cfg, inp, torch.float64)
    loss32, grads32 = T80._oracle(P, cfg, inp, torch.float32)
    net16 = copy.deepcopy(net)
    l16 = T80._hip_loss(net16, inp)
    l16.mean().backward()
    g16 = {k: p.grad.detach().cpu() for k, p in net16.named_parameters() if p.grad is not None}
    del net16
    net.set_train_precision('fp32')
    loss = T80._hip_loss(net, inp)
    loss.mean().backward()
    assert (Bn, False, True, None, 'fp32') in net.engine()._plans
    params = dict(net.named_parameters())
    gh = {k: params[k].grad.detach().cpu().clone() for k in grads64}
    e_hip, k_hip = T80._worst(loss, gh, loss64, grads64)
    e_ref, k_ref = T80._worst(loss32, grads32, loss64, grads64)
    e_bf16, _ = T80._worst(l16, g16, loss64, grads64)
    print(f'worst tensor: hip {k_hip}, oracle fp32 {k_ref}')
    T80._check('S/4 fp32 training, T=64 B=2', e_hip, e_ref, e_bf16)


def test_s4_eval_forward_on_a_128_latent_vs_oracle():
    """DiT-S/4 at R = 128: T = 1024, the first 128^2 latent (a 1024^2 image)."""
    cfg, P, net = T10._build('DiT-S/4', 128, seed=11, train=False)
    gcpu = torch.Generator().manual_seed(3)
    x = torch.randn(1, 4, 128, 128, generator=gcpu) * 2
    sigma = torch.tensor([1.5])
    y = torch.zeros(1, 1000)
    y[0, 321] = 1
    with torch.no_grad():
        ref = O.precond_forward(P, cfg, x, sigma, y, training=False)
        e = T10._relmax(net(x.to(DEV), sigma.to(DEV), y.to(DEV))['x'], ref)
        net.set_eval_precision('fp32')
        e32 = T10._relmax(net(x.to(DEV), sigma.to(DEV), y.to(DEV))['x'], ref)
    print(f'S/4, T = 1024: bf16 {e:.2e}, fp32 {e32:.2e}')
    assert e <= T10.TOL_D and e32 <= TOL_F32
