"""Decoder-less models (use_decoder=False) on the GPU: the two kernels of csrc/final_keep.hip, then the models end to end
through the public surface.

Kernel tests use the criterion of tests/test_90_patch_sizes_gpu.py: relative L2 error per tensor against torch in fp64,
    e_hip <= 4 e_ref,   e_ref = the same computation by torch (CPU) in fp32,
with F and dx pre-filled with a sentinel (every element must be overwritten; removed patches and padding rows must be exactly
0.0), the padding rows of x pre-filled with 1e30 (a kernel that reads one produces inf / garbage), and every output inside a
frame of sentinels.  End-to-end tests use the bounds and helpers of tests/test_10_engine_gpu.py (TOL_D, TOL_LOSS, TOL_GRAD,
TOL_F32, the sampler's 4e-3) and the 2.05e-4 optimizer-step rule of test_90.

Every test prints its figures before it asserts (run with -s); DESIGN.md section 7.5 records them.
"""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import maskdit_amd as M
    from maskdit_amd import _lib
    from oracle import maskdit_oracle as O
    import tests.test_10_engine_gpu as T10
    from tests.test_90_patch_sizes_gpu import Framed, SENT, _within, _st

DEV = 'cuda'
C_ = 4


# ---------------------------------------------------------------------------------------------------------------------
# kernels

def _keep_ref(dt, x, mod, W, b, dF, keep, B, T, L, D, p):
    """x [B, Lp, D] (rows < L real), keep [B, L] = image token of row r (None: identity).  Returns F, stats of the real
    rows, dx of the real rows, and the gradients of W, b, mod (without pre-fill)."""
    w = int(T ** 0.5)
    xs = x[:, :L].to(dt).clone().requires_grad_(True)
    ms, Wl, bl = (t.to(dt).clone().requires_grad_(True) for t in (mod, W, b))
    sh, sc = ms[:, :D], ms[:, D:2 * D]
    mean = xs.mean(-1, keepdim=True)
    rstd = (xs.var(-1, unbiased=False, keepdim=True) + 1e-6).rsqrt()
    xn = (xs - mean) * rstd * (1 + sc[:, None]) + sh[:, None]
    o = xn @ Wl.t() + bl  # [B, L, p * p * C]
    if keep is not None:
        o = torch.zeros(B, T, o.shape[2], dtype=dt).scatter(1, keep[:, :, None].expand(-1, -1, o.shape[2]), o)
    Fo = torch.einsum('nhwpqc->nchpwq', o.view(B, w, w, p, p, C_)).reshape(B, C_, w * p, w * p)
    Fo.backward(dF.to(dt))
    stats = torch.stack([mean.detach().squeeze(-1), rstd.detach().squeeze(-1)], -1)  # [B, L, 2]
    return [Fo.detach(), stats, xs.grad, Wl.grad, bl.grad, ms.grad]


@pytest.mark.parametrize('masked', [True, False], ids=['masked', 'unmasked'])
@pytest.mark.parametrize('p', [2, 4, 8])
@pytest.mark.parametrize('D', [384, 1152, 1280])
def test_final_keep_fwd_bwd_vs_fp64(D, p, masked):
    B, T = 2, 64
    O_, R = p * p * C_, 8 * p
    L, Lp = (23, 64) if masked else (T, T)
    ld = 2 * D + 8  # modulation rows at a pitch that is not 2 D: the tail columns must keep their pre-fill
    g = torch.Generator().manual_seed(95000 + D + p + masked)
    x = torch.randn(B, Lp, D, generator=g) * 1.5 + 0.3
    x[:, L:] = 1e30  # padding rows: never to be read
    mod = torch.randn(B, ld, generator=g) * 0.5
    W, b = torch.randn(O_, D, generator=g) / D ** 0.5, torch.randn(O_, generator=g)
    dF = torch.randn(B, C_, R, R, generator=g)
    W0, b0, dmod0 = torch.randn(O_, D, generator=g), torch.randn(O_, generator=g), torch.randn(B, ld, generator=g)
    keep, ids_p, removed = None, None, torch.zeros(B, T, dtype=torch.bool)
    if masked:
        md = M.get_mask(B, T, 0.64, DEV, noise=torch.rand(B, T, generator=g).to(DEV))
        keep, ids32 = md['ids_keep'].cpu(), md['ids32']
        assert keep.shape[1] == L
        ids_p = ids32.data_ptr()
        removed = md['mask'].cpu() > 0
    r64 = _keep_ref(torch.float64, x, mod, W, b, dF, keep, B, T, L, D, p)
    r32 = _keep_ref(torch.float32, x, mod, W, b, dF, keep, B, T, L, D, p)
    xd, md_, Wd, bd, dFd = (t.to(DEV).contiguous() for t in (x, mod, W, b, dF))
    tag = f'D={D} p={p} {"masked L=23/64" if masked else "unmasked"}'
    # ---- forward
    Fo, stats = Framed(B * C_ * R * R), Framed(2 * B * Lp)
    _lib.call('mdt_final_keep_fwd', xd.data_ptr(), md_.data_ptr(), md_.data_ptr() + 4 * D, ld, Wd.data_ptr(), bd.data_ptr(), ids_p,
              2 * T, Fo.ptr(), stats.ptr(), B, T, L, Lp if masked else 0, D, C_, p, _st())
    torch.cuda.synchronize()
    assert Fo.intact() and stats.intact(), 'final_keep_fwd wrote outside its outputs'
    Fg = Fo.get(B, C_, R, R)
    assert bool(torch.isfinite(Fg).all()) and not bool((Fg == SENT).any()), 'F is not fully defined'
    pix = removed.view(B, 1, 8, 8).repeat_interleave(p, 2).repeat_interleave(p, 3).expand(B, C_, R, R)
    assert bool((Fg[pix] == 0.0).all()), 'a removed patch of F is not exactly zero'
    assert removed.sum().item() == B * (T - L)
    _within(f'keep F {tag}', Fg, r32[0], r64[0])
    st = stats.get(B, Lp, 2)
    _within(f'keep mean {tag}', st[:, :L, 0], r32[1][..., 0], r64[1][..., 0])
    _within(f'keep rstd {tag}', st[:, :L, 1], r32[1][..., 1], r64[1][..., 1])
    assert bool((st[:, L:] == SENT).all()), 'statistics of a padding row were written'
    # ---- backward: pre-filled accumulators
    dx, dW, db, dmod = Framed(B * Lp * D), Framed(O_ * D, fill=W0), Framed(O_, fill=b0), Framed(B * ld, fill=dmod0)

    def bwd(dx_, dW_, db_, dmod_):
        _lib.call('mdt_final_keep_bwd', dFd.data_ptr(), xd.data_ptr(), stats.ptr(), md_.data_ptr(), md_.data_ptr() + 4 * D, ld,
                  Wd.data_ptr(), ids_p, 2 * T, dx_.ptr(), dW_.ptr(), db_.ptr(), dmod_.ptr(), dmod_.ptr() + 4 * D, ld, B, T, L,
                  Lp if masked else 0, D, C_, p, _st())
        torch.cuda.synchronize()
        assert dx_.intact() and dW_.intact() and db_.intact() and dmod_.intact(), 'final_keep_bwd wrote outside its outputs'

    bwd(dx, dW, db, dmod)
    dxg = dx.get(B, Lp, D)
    assert bool(torch.isfinite(dxg).all()) and not bool((dxg == SENT).any()), 'dx is not fully defined'
    assert bool((dxg[:, L:] == 0.0).all()), 'dx of a padding row is not exactly zero'
    dm = dmod.get(B, ld)
    assert torch.equal(dm[:, 2 * D:], dmod0[:, 2 * D:]), 'final_keep_bwd touched modulation columns that are not its own'
    _within(f'keep dx {tag}', dxg[:, :L], r32[2], r64[2])
    _within(f'keep dW {tag}', dW.get(O_, D), W0 + r32[3], W0.double() + r64[3])
    _within(f'keep dbias {tag}', db.get(O_), b0 + r32[4], b0.double() + r64[4])
    _within(f'keep dshift {tag}', dm[:, :D], (dmod0 + r32[5])[:, :D], (dmod0.double() + r64[5])[:, :D])
    _within(f'keep dscale {tag}', dm[:, D:2 * D], (dmod0 + r32[5])[:, D:2 * D], (dmod0.double() + r64[5])[:, D:2 * D])
    # ---- ADD semantics: from zero, a second call doubles the first.  Tolerance: each element is a sum of n <= 128 row terms
    # plus up to 8 atomic partials in any order, rounding error <= n * 2^-24 of the sum of magnitudes; 1e-4 of the tensor's
    # largest magnitude is > 10x that
    z = [Framed(O_ * D, fill=torch.zeros(O_ * D)), Framed(O_, fill=torch.zeros(O_)), Framed(B * ld, fill=torch.zeros(B * ld))]
    dx2 = Framed(B * Lp * D)
    bwd(dx2, *z)
    once = [t.get(t.n).clone() for t in z]
    bwd(dx2, *z)
    for name, a1, fr in zip(('dW', 'dbias', 'dmod'), once, z):
        a2 = fr.get(fr.n)
        err = (a2 - 2 * a1).abs().max().item() / a1.abs().max().item()
        print(f'[keep {name} {tag}] second call vs twice the first: {err:.2e} of the largest magnitude')
        assert err <= 1e-4, f'{name} is not accumulated'
    assert torch.equal(dx2.get(B, Lp, D), dxg), 'dx is stored, not accumulated'


def test_final_keep_refusals():
    """Argument checks only: nothing is launched (the pointers are dummies)."""
    L = _lib.lib()
    a = 4096  # a 16-byte aligned dummy address

    def fwd(D=384, p=2, T=64, Lk=64, Lp=0, ids=None, x=a, ld=None):
        return L.mdt_final_keep_fwd(x, a, a, ld if ld is not None else 2 * D, a, a, ids, 2 * T, a, a, 2, T, Lk, Lp, D, 4, p, None)

    def bwd(D=384, p=2, T=64, Lk=64, Lp=0, ids=None, dx=a):
        return L.mdt_final_keep_bwd(a, a, a, a, a, 2 * D, a, ids, 2 * T, dx, a, a, a, a, 2 * D, 2, T, Lk, Lp, D, 4, p, None)

    for call in (fwd, bwd):
        assert call(D=1284, p=4) != 0 and b'final_keep' in L.mdt_last_error()
        assert call(D=2048) != 0 and b'1280' in L.mdt_last_error()
        assert call(D=400, p=4) != 0 and b'multiple of 32' in L.mdt_last_error()
        assert call(D=386) != 0 and b'multiple of 4' in L.mdt_last_error()
        assert call(p=3) != 0 and b'p*p*C' in L.mdt_last_error()
        assert call(T=60) != 0 and b'square' in L.mdt_last_error()
        assert call(Lk=23) != 0 and b'identity' in L.mdt_last_error()       # ids == NULL needs L == T
        assert call(Lk=65, ids=a) != 0 and call(Lk=0, ids=a) != 0 and call(Lk=40, Lp=32, ids=a) != 0
    assert fwd(x=None) != 0 and b'null pointer' in L.mdt_last_error()
    assert bwd(dx=None) != 0 and b'null pointer' in L.mdt_last_error()
    assert fwd(x=a + 4) != 0 and b'aligned' in L.mdt_last_error()
    assert fwd(ld=770) != 0 and b'aligned' in L.mdt_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# end to end

def _build_nd(model_type, R, seed, train=True):
    cfg = O.make_cfg(model_type, img_resolution=R, use_decoder=False)
    P = O.init_params(cfg, seed=seed, dezero=True)
    net = M.Precond_models['edm'](img_resolution=R, img_channels=4, num_classes=1000, model_type=model_type, use_decoder=False,
                                  mae_loss_coef=0.1, pad_cls_token=False).to(DEV)
    net.load_state_dict(P, strict=True)
    net.train(train)
    return cfg, P, net


def _step_vs_oracle(tag, net, cfg, P, inputs, ratio):
    """One training evaluation + backward against the oracle: loss, D_yn, every gradient.  Returns (loss, md, oracle D)."""
    images, labels, rnd, noise, mnoise = inputs
    B, T = mnoise.shape
    md = M.get_mask(B, T, ratio, DEV, noise=mnoise.to(DEV)) if ratio > 0 else None
    net.zero_grad(set_to_none=True)
    loss = M.Losses['edm']().with_draws(net, images.to(DEV), labels.to(DEV), rnd.to(DEV), noise.to(DEV), md, mae_loss_coef=0.1)
    loss.mean().backward()
    mdict = None
    if ratio > 0:
        ref_md = O.get_mask_from_noise(mnoise.numpy(), ratio)
        assert np.array_equal(md['ids_keep'].cpu().numpy(), ref_md['ids_keep'])
        mdict = {k: torch.from_numpy(v) for k, v in ref_md.items()}
    loss_ref, D_ref, grads_ref = O.loss_and_grads(P, cfg, images, labels, rnd, noise, mdict, 0.1 if ratio > 0 else 0.0)
    Lv = md['ids_keep'].shape[1] if ratio > 0 else None
    pl = net.engine().plan(B, ratio > 0, True, Lv)
    assert pl.Lv == (Lv if ratio > 0 else T)
    e = T10._relmax(pl.buf['D'], D_ref)
    rl = ((loss.detach().cpu() - loss_ref).abs() / loss_ref.abs()).max().item()
    params = dict(net.named_parameters())
    assert set(grads_ref) == {k for k, q in params.items() if q.requires_grad}
    worst = ('', 0.0)
    fails = []
    for k, gr in grads_ref.items():
        got = params[k].grad
        assert got is not None, k
        num, den = (got.detach().cpu().double() - gr.double()).norm().item(), gr.double().norm().item()
        if num / (den + 1e-12) > worst[1]:
            worst = (k, num / (den + 1e-12))
        if num > T10.TOL_GRAD * den + 1e-7:
            fails.append(f'{k}: grad rel L2 err {num / (den + 1e-12):.3e} (|g| = {den:.3e})')
    print(f'[{tag}] vs oracle: D_yn {e:.3e}, loss {rl:.3e}, worst grad rel L2 {worst[1]:.3e} at {worst[0]}')
    assert e <= T10.TOL_D and rl <= T10.TOL_LOSS and not fails, fails
    if ratio > 0:  # the prediction at a removed patch is c_skip * (y + n), bit for bit: F is exactly zero there
        w, p = int(T ** 0.5), cfg['patch']
        pix = (md['mask'] > 0).view(B, 1, w, w).repeat_interleave(p, 2).repeat_interleave(p, 3).expand_as(pl.buf['D'])
        want = pl.buf['coef'][0].view(B, 1, 1, 1) * pl.buf['yn']
        assert bool((pl.buf['F'][pix] == 0).all()) and torch.equal(pl.buf['D'][pix], want[pix])
    return loss, md, D_ref


@pytest.mark.parametrize('name,model,R', [('s2nd_train.npz', 'DiT-S/2', 16), ('s4nd_train.npz', 'DiT-S/4', 32)])
def test_masked_train_step_vs_reference_fixture(golden_dir, name, model, R):
    """The reference's own decoder-less masked step (tests/golden/make_golden_nodecoder.py): D_yn, per-sample losses, every
    gradient tensor, one AdamW + EMA step."""
    g = T10._load(golden_dir, name)
    ratio = float(g['mask_ratio'])
    cfg, P, net = _build_nd(model, R, int(g['seed']))
    import copy
    ema = copy.deepcopy(net)
    opt = M.FusedAdam(net.parameters(), lr=1e-4, adam_w_mode=True, weight_decay=0)
    assert opt._arena is net.engine()
    loss, md, D_ref = _step_vs_oracle(name, net, cfg, P, T10._inputs(g), ratio)
    B = int(g['B'])
    Lv = md['ids_keep'].shape[1]
    assert Lv == int(64 * (1 - ratio)) and (name != 's2nd_train.npz' or Lv == 23)
    D = net.engine().plan(B, True, True, Lv).buf['D']
    e = T10._relmax(D, torch.from_numpy(g['D_yn']))
    rl = ((loss.detach().cpu() - torch.from_numpy(g['loss'])).abs() / torch.from_numpy(g['loss']).abs()).max().item()
    print(f'[{name}] vs fixture: D_yn {e:.3e}, loss {rl:.3e}')
    assert e <= T10.TOL_D and rl <= T10.TOL_LOSS
    params = dict(net.named_parameters())
    names = [str(n) for n in g['param_names']]
    assert set(names) == {k for k, q in params.items() if q.requires_grad}
    from tests.golden.make_golden_idx import sample_idx
    for i, k in enumerate(names):  # the reference's own gradient: its norm and 64 sampled entries
        got = params[k].grad.detach().cpu().double()
        gs = g['grad_sums'][i]
        assert abs(got.norm().item() - gs[2]) <= T10.TOL_GRAD * gs[2] + 1e-7, k
        d = got.flatten()[sample_idx(got.numel())].numpy() - g['grad_samples'][i]
        assert np.linalg.norm(d) <= T10.TOL_GRAD * gs[2] + 1e-7, k
    g_hip = {k: params[k].grad.detach().cpu().clone() for k in names}
    p_before = {k: params[k].detach().cpu().clone() for k in names}
    opt.step()
    M.update_ema(ema, net, decay=0.9999)
    ema_p = dict(ema.named_parameters())
    bad = 0
    for i, k in enumerate(names):
        q, m, v = p_before[k].clone(), torch.zeros_like(p_before[k]), torch.zeros_like(p_before[k])
        O.adamw_step(q, g_hip[k], m, v, step=1, lr=1e-4)
        assert torch.allclose(params[k].detach().cpu(), q, rtol=1e-5, atol=1e-7), k
        idx = sample_idx(params[k].numel())
        got = params[k].detach().cpu().double().flatten()[idx].numpy()
        bad += int((np.abs(got - g['upd_samples'][i]) > 2.05e-4).sum())  # |step| <= lr = 1e-4 each way
        got_e = ema_p[k].detach().cpu().double().flatten()[idx].numpy()
        # ema = 0.9999 p_before + 0.0001 p_after: 1e-4 of the step rule above, plus the fp32 roundings of the blend itself --
        # at most three on either side, half an ulp <= 2^-24 |v| each: 6 * 2^-24 |v| < 2^-21 |v|
        bad += int((np.abs(got_e - g['ema_samples'][i]) > 2.05e-8 + 2.0 ** -21 * np.abs(g['ema_samples'][i]) + 1e-12).sum())
    assert bad == 0


def test_set_valid_on_a_cached_plan(golden_dir):
    """The same S/2 plan (pitch 64) with 23 and then 40 kept tokens: the new launches read the run-time count."""
    g = T10._load(golden_dir, 's2nd_train.npz')
    cfg, P, net = _build_nd('DiT-S/2', 16, int(g['seed']))
    inputs = T10._inputs(g)
    B, T = inputs[4].shape
    plans = []
    for Lv in (23, 40, 23):
        ratio = 1.0 - (Lv + 0.5) / T
        assert int(T * (1 - ratio)) == Lv
        _step_vs_oracle(f'S/2 kept {Lv} of 64', net, cfg, P, inputs, ratio)
        plans.append(net.engine().plan(B, True, True, Lv))
        assert plans[-1].L == 64 and plans[-1].lv_arg.value == Lv
    assert plans[0] is plans[1] is plans[2], 'the 64-row plan was rebuilt instead of re-used'


def test_b2_width_768_train_and_eval_vs_oracle():
    """DiT-B/2 (D = 768 > 512: three float4 slots per lane) on a 16^2 latent, B = 4: masked and unmasked training step and
    an eval forward with cfg, against the oracle."""
    cfg, P, net = _build_nd('DiT-B/2', 16, seed=31)
    B, R, T = 4, 16, 64
    gcpu = torch.Generator().manual_seed(17)
    images = 0.5 * torch.randn(B, 4, R, R, generator=gcpu)
    labels = torch.zeros(B, 1000)
    labels[torch.arange(B), torch.randint(0, 1000, (B,), generator=gcpu)] = 1
    labels[1] = 0
    inputs = (images, labels, torch.randn(B, 1, 1, 1, generator=gcpu), torch.randn(B, 4, R, R, generator=gcpu),
              torch.rand(B, T, generator=gcpu))
    _step_vs_oracle('B/2 masked 0.5', net, cfg, P, inputs, 0.5)
    _step_vs_oracle('B/2 unmasked', net, cfg, P, inputs, 0.0)
    net.eval()
    x = torch.randn(2, 4, R, R, generator=gcpu) * 2
    sigma = torch.tensor([0.4, 9.0])
    with torch.no_grad():
        ref = O.precond_forward(P, cfg, x, sigma, labels[:2], training=False)
        ref2 = O.precond_forward(P, cfg, x, torch.tensor(2.5), labels[:2], cfg_scale=1.5, training=False)
        e1 = T10._relmax(net(x.to(DEV), sigma.to(DEV), labels[:2].to(DEV))['x'], ref)
        e2 = T10._relmax(net(x.to(DEV), torch.tensor(2.5, dtype=torch.float64, device=DEV), labels[:2].to(DEV), 1.5)['x'], ref2)
        net.set_eval_precision('fp32')
        e3 = T10._relmax(net(x.to(DEV), torch.tensor(2.5, dtype=torch.float64, device=DEV), labels[:2].to(DEV), 1.5)['x'], ref2)
    print(f'[B/2 eval] bf16 {e1:.2e}, bf16 cfg {e2:.2e}, fp32 cfg {e3:.2e}')
    assert e1 <= T10.TOL_D and e2 <= T10.TOL_D and e3 <= T10.TOL_F32


def test_sampler_three_precisions_vs_reference_fixture(golden_dir):
    g = T10._load(golden_dir, 'nd_sampler.npz')
    R = int(g['R'])
    cfg, P, net = _build_nd('DiT-S/2', R, int(g['seed']), train=False)
    labels = torch.eye(1000)[torch.from_numpy(g['cls'])].to(DEV)
    lat = torch.from_numpy(g['latents']).to(DEV)
    n, cs = int(g['num_steps']), float(g['cfg_scale'])
    zref, zref0 = torch.from_numpy(g['z']), torch.from_numpy(g['z_nocfg'])
    for prec in ('bf16', 'fp32', 'bf16x3'):
        z = M.edm_sampler(net, lat, labels, cfg_scale=cs, num_steps=n, precision=prec)
        z0 = M.edm_sampler(net, lat, labels, cfg_scale=None, num_steps=n, precision=prec)
        z_direct = M.edm_sampler(net, lat, labels, cfg_scale=cs, num_steps=n, precision=prec, use_graph=False)
        assert z.dtype == torch.float64 and z.shape == lat.shape
        e, e0 = T10._relmax(z, zref), T10._relmax(z0, zref0)
        print(f'[nd_sampler {prec}] cfg {e:.3e}, no cfg {e0:.3e}, direct vs graph {T10._relmax(z_direct, z):.3e}')
        if prec == 'bf16':
            assert e <= 4e-3 and e0 <= 4e-3
            assert torch.equal(z, M.edm_sampler(net, lat, labels, cfg_scale=cs, num_steps=n, precision=prec))  # graph replay
            assert T10._relmax(z_direct, z) <= 5e-3
        else:
            assert e <= T10.TOL_F32 and e0 <= T10.TOL_F32
            assert torch.equal(z, z_direct)
    za = M.ablation_sampler(net, lat, labels, cfg_scale=cs, num_steps=n, precision='fp32')
    print(f'[nd_sampler] ablation_sampler (defaults = the EDM sampler) {T10._relmax(za, zref):.2e}')
    assert T10._relmax(za, zref) <= T10.TOL_F32


def test_a_decoder_model_still_matches_its_fixture_after_a_decoderless_one(golden_dir):
    """The plan cache and the live-engine set are process-wide: a decoder-less engine is built, used and dropped, then the
    S/2 decoder model runs its fixture check."""
    g = T10._load(golden_dir, 's2nd_train.npz')
    cfg, P, net = _build_nd('DiT-S/2', 16, int(g['seed']))
    with torch.no_grad():
        T10._run_loss(net, g, mask_ratio=float(g['mask_ratio']))
    assert len(net.engine()._plans) == 1
    del net
    gc.collect()
    T10.test_forward_loss_vs_reference_fixture(golden_dir, 's2_train.npz', 'DiT-S/2', 32)
