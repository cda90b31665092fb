"""bf16x3 inference arithmetic (csrc/f32path.hip gemm_bf16x3_kernel; Engine.plan(..., precision='bf16x3')): every fp32
operand of a Linear layer split exactly into three bf16 terms, six cross products on the bf16 matrix instruction.

Kernel bounds are stated relative to the largest magnitude of the fp64 result, against mdt_gemm_f32 on the same inputs
(err_x3 <= 2 err_f32 + 1e-7) and against the fp64 product of the bf16-rounded operands (err_x3 <= 0.01 err_bf16: the b1
and b2 planes are used).  Network-level results are held to TOL_F32, the bound the exact-fp32 plan meets."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import maskdit_amd as M
    from maskdit_amd import ops
    from maskdit_amd._lib import call
    from oracle import maskdit_oracle as O

DEV = 'cuda'
TOL_F32 = 5e-6
# tools/f32_bench.py's XL/2 inference shapes (N, K, epilogue) at M = 4096, plus a ragged case
SHAPES = [(4096, 3456, 1152, 'NONE'), (4096, 1152, 1152, 'GATE_RES'), (4096, 4608, 1152, 'GELU'), (4096, 1152, 4608, 'GATE_RES'),
          (4096, 1536, 512, 'NONE'), (4096, 512, 512, 'GATE_RES'), (4096, 2048, 512, 'GELU'), (4096, 512, 2048, 'GATE_RES'),
          (1000, 1000, 1000, 'SILU')]


def _problem(M_, N, K, epi, a_scale=1.0, b_scale=1.0, seed=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    s = a_scale * b_scale
    A = torch.randn(M_, K, device=DEV, generator=g) * a_scale
    W = torch.randn(N, K, device=DEV, generator=g) * (K ** -0.5 * b_scale)
    b = torch.randn(N, device=DEV, generator=g) * s
    kw = dict(bias=b, epi=getattr(ops, 'F32EPI_' + epi))
    extra = {}
    if epi == 'GATE_RES':
        extra['res'] = torch.randn(M_, N, device=DEV, generator=g) * s
        extra['gate'] = torch.randn(M_ // 256, N, device=DEV, generator=g)
        kw.update(res=extra['res'], gate=extra['gate'], gate_ld=N, rows_per_sample=256)
    return A, W, b, kw, extra


def _ref(A, W, b, epi, extra):
    y = A.double() @ W.double().t() + b.double()
    if epi == 'GELU':
        y = F.gelu(y, approximate='tanh')
    elif epi == 'SILU':
        y = F.silu(y)
    elif epi == 'GATE_RES':
        y = extra['res'].double() + extra['gate'].double().repeat_interleave(256, 0) * y
    return y


def _rel(got, ref):
    return ((got.double() - ref).abs().max() / ref.abs().max()).item()


def _poison_lds():
    sink = torch.zeros(4, device=DEV, dtype=torch.int32)
    call('mdt_lds_poison', sink.data_ptr(), torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize('M_,N,K,epi', SHAPES)
def test_gemm_bf16x3_vs_fp64(M_, N, K, epi):
    """Every epilogue (GATE_RES with a gate and rows_per_sample 256), ragged M / N / K, and exponent-range safety: the same
    relative bounds with A scaled by 2^-100 and with B scaled by 2^60."""
    for a_scale, b_scale in ((1.0, 1.0), (2.0 ** -100, 1.0), (1.0, 2.0 ** 60)):
        A, W, b, kw, extra = _problem(M_, N, K, epi, a_scale, b_scale)
        ref = _ref(A, W, b, epi, extra)
        x3 = torch.full((M_, N), float('nan'), device=DEV)
        f32 = torch.full((M_, N), float('nan'), device=DEV)
        ops.gemm_bf16x3(A, W, x3, M_, N, K, **kw)
        ops.gemm_f32(A, W, f32, M_, N, K, **kw)
        ref16 = _ref(A.bfloat16().float(), W.bfloat16().float(), b, epi, extra)
        e3, e32, e16 = _rel(x3, ref), _rel(f32, ref), _rel(ref16, ref)
        print(f'{M_}x{N}x{K} {epi} scale ({a_scale:.0e}, {b_scale:.0e}): bf16x3 {e3:.2e}, fp32 {e32:.2e}, bf16 operands {e16:.2e}')
        assert e3 <= 2 * e32 + 1e-7, f'bf16x3 {e3:.3e} vs fp32 {e32:.3e}'
        assert e3 <= 0.01 * e16, f'bf16x3 {e3:.3e} vs bf16-rounded operands {e16:.3e}'


def test_gemm_bf16x3_inf_operand_row():
    """An inf in A gives inf (not NaN) in every column of its output row; the other rows stay finite."""
    A, W, b, kw, _ = _problem(300, 200, 256, 'NONE')
    A[5, 7] = float('inf')
    out = torch.empty(300, 200, device=DEV)
    ops.gemm_bf16x3(A, W, out, 300, 200, 256, **kw)
    assert bool(torch.isinf(out[5]).all()), 'expected inf in the row of the inf operand'
    assert bool(torch.isfinite(torch.cat([out[:5], out[6:]])).all())


@pytest.mark.parametrize('M_,N,K,epi', [(4096, 1152, 1152, 'GATE_RES'), (1000, 1000, 1000, 'SILU'), (2048, 4608, 1152, 'GELU')])
def test_gemm_bf16x3_poisoned_lds_deterministic(M_, N, K, epi):
    """Each launch behind mdt_lds_poison (a fragment read before its tile was written would surface as NaN / a wrong sum):
    bit-identical to an unpoisoned launch and across three repeats."""
    A, W, b, kw, _ = _problem(M_, N, K, epi)
    clean = torch.empty(M_, N, device=DEV)
    ops.gemm_bf16x3(A, W, clean, M_, N, K, **kw)
    for rep in range(3):
        _poison_lds()
        out = torch.full((M_, N), float('nan'), device=DEV)
        ops.gemm_bf16x3(A, W, out, M_, N, K, **kw)
        assert torch.equal(out.view(torch.int32), clean.view(torch.int32)), f'repeat {rep} differs'


# ---------------------------------------------------------------------------------------------------------- network
def _load(golden_dir, name):
    return np.load(f'{golden_dir}/{name}', allow_pickle=False)


def _build(model_type, R, seed):
    cfg = O.make_cfg(model_type, img_resolution=R)
    P = O.init_params(cfg, seed=seed, dezero=True)
    net = M.Precond_models['edm'](img_resolution=R, img_channels=4, num_classes=1000, model_type=model_type,
                                  use_decoder=True, mae_loss_coef=0.1, pad_cls_token=False).to(DEV)
    net.load_state_dict(P, strict=True)
    net.eval()
    return cfg, P, net


def _relmax(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def test_eval_forward_cfg_and_sampler_bf16x3_vs_oracle(golden_dir):
    """Eval forward, forward_with_cfg, the graph and direct-launch samplers (cfg and none), the churn branch: each
    against the fp32 oracle / the reference's fixtures at TOL_F32."""
    cfg, P, net = _build('DiT-S/2', 32, seed=5)
    net.set_eval_precision('bf16x3')
    gcpu = torch.Generator().manual_seed(1)
    x = torch.randn(3, 4, 32, 32, generator=gcpu) * 3
    sigma = torch.tensor([0.3, 2.0, 40.0])
    y = torch.zeros(3, 1000)
    y[torch.arange(3), torch.tensor([1, 500, 999])] = 1
    with torch.no_grad():
        e1 = _relmax(net(x.to(DEV), sigma.to(DEV), y.to(DEV))['x'], O.precond_forward(P, cfg, x, sigma, y, training=False))
        D2 = net(x.to(DEV), torch.tensor(2.5, dtype=torch.float64, device=DEV), y.to(DEV), 1.5)['x']
        e2 = _relmax(D2, O.precond_forward(P, cfg, x, torch.tensor(2.5), y, cfg_scale=1.5, training=False))
    print(f'bf16x3 eval forward vs oracle: {e1:.2e}; with cfg: {e2:.2e}')
    assert e1 <= TOL_F32 and e2 <= TOL_F32
    g = _load(golden_dir, 's2_sampler.npz')
    cfg, P, net = _build('DiT-S/2', 32, int(g['seed']))
    labels = torch.eye(1000)[torch.from_numpy(g['cls'])].to(DEV)
    lat = torch.from_numpy(g['latents']).to(DEV)
    n = int(g['num_steps'])
    z = M.edm_sampler(net, lat, labels, cfg_scale=float(g['cfg_scale']), num_steps=n, precision='bf16x3')
    z_direct = M.edm_sampler(net, lat, labels, cfg_scale=float(g['cfg_scale']), num_steps=n, precision='bf16x3', use_graph=False)
    z2 = M.edm_sampler(net, lat, labels, cfg_scale=None, num_steps=n, precision='bf16x3')
    e, e2 = _relmax(z, torch.from_numpy(g['z'])), _relmax(z2, torch.from_numpy(g['z_nocfg']))
    print(f'bf16x3 sampler vs reference fixture: cfg {e:.2e}, no cfg {e2:.2e}')
    assert e <= TOL_F32 and e2 <= TOL_F32 and torch.equal(z, z_direct)
    g = _load(golden_dir, 's2_sampler_churn.npz')
    cfg, P, net = _build('DiT-S/2', 32, int(g['seed']))
    rnd = M.StackedRandomGenerator('cpu', [int(s) for s in g['seeds']])
    lat = rnd.randn([len(g['seeds']), 4, 32, 32])
    cls = rnd.randint(1000, size=[len(g['seeds'])])
    z = M.edm_sampler(net, lat.to(DEV), torch.eye(1000)[cls].to(DEV), cfg_scale=float(g['cfg_scale']), num_steps=int(g['num_steps']),
                      randn_like=lambda t: rnd.randn(list(t.shape), dtype=t.dtype).to(t.device), S_churn=float(g['S_churn']),
                      S_min=float(g['S_min']), S_max=float(g['S_max']), S_noise=float(g['S_noise']), precision='bf16x3')
    e3 = _relmax(z, torch.from_numpy(g['z']))
    print(f'bf16x3 sampler with churn vs reference fixture: {e3:.2e}')
    assert e3 <= TOL_F32 and net.eval_precision == 'bf16'


def test_xl2_sampler_50_steps_bf16x3_vs_reference_fixture(golden_dir):
    """XL/2, 50 Heun steps (99 network evaluations), cfg 1.5, graph path, against the reference's own fp32 edm_sampler
    output: the bound the exact-fp32 plan meets."""
    g = _load(golden_dir, 'xl2_sampler.npz')
    cfg, P, net = _build('DiT-XL/2', 32, int(g['seed']))
    labels = torch.eye(1000)[torch.from_numpy(g['cls'])].to(DEV)
    lat = torch.from_numpy(g['latents']).to(DEV)
    z = M.edm_sampler(net, lat, labels, cfg_scale=float(g['cfg_scale']), num_steps=int(g['num_steps']), precision='bf16x3')
    ref = torch.from_numpy(g['z'])
    e = _relmax(z, ref)
    rms = ((z.cpu() - ref).norm() / ref.norm()).item()
    print(f'XL/2 50-step sampler (bf16x3 net) vs reference (fp32 net): rel-to-max err {e:.3e}, rel L2 err {rms:.3e}')
    assert z.dtype == torch.float64 and bool(torch.isfinite(z).all())
    assert e <= TOL_F32 and rms <= TOL_F32


def test_bf16x3_plan_routing():
    """Every Linear layer of the 'bf16x3' forward issues mdt_gemm_bf16x3 and none issues mdt_gemm_f32 (attention keeps its
    own exact-fp32 entry); the fp32 plan of the same network is untouched.  Training / masked plans refuse it."""
    cfg, P, net = _build('DiT-S/2', 32, seed=2)
    eng = net.engine()
    names = [c[2] for c in eng.plan(4, False, False, None, 'bf16x3').fwd.calls]
    sp = net.spec
    linears = 4 + (sp.depth + sp.ddepth) * 4 + 1  # t-embedder x2, label table, adaLN; qkv/proj/fc1/fc2 per block; decoder_layer
    assert names.count('mdt_gemm_bf16x3') == linears and 'mdt_gemm_f32' not in names, names
    assert names.count('mdt_attn_f32') == sp.depth + sp.ddepth
    f32_names = [c[2] for c in eng.plan(4, False, False, None, 'fp32').fwd.calls]
    assert f32_names.count('mdt_gemm_f32') == linears and 'mdt_gemm_bf16x3' not in f32_names
    with pytest.raises(NotImplementedError):
        eng.plan(8, True, True, 128, 'bf16x3')
    with pytest.raises(NotImplementedError):
        eng.plan(8, True, False, 128, 'bf16x3')


def test_bf16x3_isolation_and_master_arena(golden_dir):
    """bf16, fp32 and bf16x3 plans cached side by side: the fp32 sampler's result is bit-identical before and after the
    bf16x3 plan is built and run.  A weight edited in place after the bf16x3 graphs were captured changes the next bf16x3
    sample (the plan reads the fp32 master arena), which then agrees with the fp32 plan of the edited network."""
    g = _load(golden_dir, 's2_sampler.npz')
    cfg, P, net = _build('DiT-S/2', 32, int(g['seed']))
    labels = torch.eye(1000)[torch.from_numpy(g['cls'])].to(DEV)
    lat = torch.from_numpy(g['latents']).to(DEV)
    n, s = int(g['num_steps']), float(g['cfg_scale'])
    M.edm_sampler(net, lat, labels, cfg_scale=s, num_steps=n)
    z32 = M.edm_sampler(net, lat, labels, cfg_scale=s, num_steps=n, precision='fp32')
    zx = M.edm_sampler(net, lat, labels, cfg_scale=s, num_steps=n, precision='bf16x3')
    assert torch.equal(M.edm_sampler(net, lat, labels, cfg_scale=s, num_steps=n, precision='fp32'), z32)
    assert not torch.equal(zx, z32) and _relmax(zx, z32) <= TOL_F32
    with torch.no_grad():
        dict(net.named_parameters())['model.blocks.3.mlp.fc1.weight'].mul_(1.25)
    zx2 = M.edm_sampler(net, lat, labels, cfg_scale=s, num_steps=n, precision='bf16x3')
    z32b = M.edm_sampler(net, lat, labels, cfg_scale=s, num_steps=n, precision='fp32')
    print(f'in-place weight edit: bf16x3 moved {_relmax(zx2, zx):.2e}; vs fp32 of the edited net {_relmax(zx2, z32b):.2e}')
    assert _relmax(zx2, zx) > 1e-4 and _relmax(zx2, z32b) <= TOL_F32


def test_eval_forward_bf16x3_at_1024_tokens_vs_oracle():
    """512^2-latent token counts (T = 1024): attention takes the three-launch exact-fp32 form."""
    cfg, P, net = _build('DiT-S/2', 64, seed=11)
    net.set_eval_precision('bf16x3')
    gcpu = torch.Generator().manual_seed(3)
    x = torch.randn(2, 4, 64, 64, generator=gcpu) * 2
    sigma = torch.tensor([0.5, 7.0])
    y = torch.zeros(2, 1000)
    y[torch.arange(2), torch.tensor([3, 777])] = 1
    with torch.no_grad():
        D = net(x.to(DEV), sigma.to(DEV), y.to(DEV))['x']
        ref = O.precond_forward(P, cfg, x, sigma, y, training=False)
    e = _relmax(D, ref)
    print(f'bf16x3 eval forward, T = 1024: {e:.2e}')
    assert e <= TOL_F32
    assert any(k.startswith('scores_') for k in net.engine().plan(2, False, False, None, 'bf16x3').buf)
