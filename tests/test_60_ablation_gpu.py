"""ablation_sampler on the MI355X: the three kernels against torch fp64 applying the same table row, every combination of
the reference fixture (tests/golden/ablation_sampler.npz, made by the reference's own sample.ablation_sampler) per network
arithmetic, graph replay and capture reuse, isolation from edm_sampler, and the generate.py / train.py routing."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

if torch.cuda.is_available():
    import maskdit_amd as M
    from maskdit_amd import ablation, sampler
    from maskdit_amd._lib import call
    from oracle import maskdit_oracle as O

DEV = 'cuda'
TOL_F32 = 5e-6   # the fp32 path's bound (tests/test_10_engine_gpu.py:214)
TOL_BF16 = 4e-3  # <= 11 bf16 S/2 evaluations (tests/test_10_engine_gpu.py:436,467)
NAMES = ['edm_heun', 'edm_euler', 'vp_vp_vp', 'vp_vp_none', 'edm_vp_vp', 've_ve_none', 'iddpm', 'vp_euler_linear',
         'edm_alpha05', 'edm_churn']
RUNS = [(n, 1.5) for n in NAMES] + [('edm_heun', None), ('vp_vp_vp', None)]


def _col(name):
    return ablation.COLS.index(name)


def _fx(golden_dir):
    g = np.load(os.path.join(golden_dir, 'ablation_sampler.npz'), allow_pickle=False)
    return g, {name: kw for name, kw, _ in json.loads(str(g['combos']))}


def _build(seed):
    cfg = O.make_cfg('DiT-S/2', img_resolution=32)
    P = O.init_params(cfg, seed=seed, dezero=True)
    net = M.Precond_models['edm'](img_resolution=32, img_channels=4, num_classes=1000, model_type='DiT-S/2',
                                  use_decoder=True, mae_loss_coef=0.1, pad_cls_token=False).to(DEV)
    net.load_state_dict(P, strict=True)
    return net.eval()


def _run(net, g, kw, cfg_scale, **extra):
    """The fixture's draws: latents, labels and every churn draw from the seeds' CPU generators."""
    rnd = M.StackedRandomGenerator('cpu', [int(s) for s in g['seeds']])
    lat = rnd.randn([len(g['seeds']), 4, 32, 32])
    labels = torch.eye(1000)[rnd.randint(1000, size=[len(g['seeds'])])]

    def randn_like(x):  # the fixture's generators live on the CPU
        return rnd.randn(list(x.shape), dtype=x.dtype).to(x.device)

    return M.ablation_sampler(net, lat.to(DEV), labels.to(DEV), cfg_scale=cfg_scale, randn_like=randn_like,
                              num_steps=int(g['num_steps']), **kw, **extra)


def _relmax(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def _key(name, cfg_scale):
    return name + ('' if cfg_scale is not None else '_nocfg')


@pytest.mark.parametrize('use_cfg', [True, False])
def test_ablation_kernels(use_cfg):
    """prep / slope1 / slope2 on random fp64 state and fp32 F against torch fp64 applying the same table row."""
    torch.manual_seed(17)
    B, chw, sd, s = 3, 4 * 32 * 32, 0.5, 1.5
    dup = 2 if use_cfg else 1
    table, _, second = ablation.step_table(6, DEV, solver='heun', discretization='vp', schedule='vp', scaling='vp', S_churn=10,
                                           S_min=0.05, S_max=50, alpha=0.7)
    f64 = dict(dtype=torch.float64, device=DEV)
    x0 = torch.randn(B, chw, **f64) * 3
    noise = torch.randn(B, chw, **f64)
    for i in (2, 5):  # a step with the second evaluation, the last step without it
        r = table[i]
        assert second[i] == (i == 2) and (i != 2 or (r[_col('c')] > 0 and r[_col('a')] != 1))
        step = torch.tensor([i], dtype=torch.int32, device=DEV)
        x, x_hat, d_cur = x0.clone(), torch.empty_like(x0), torch.empty_like(x0)
        xin = torch.empty(dup * B, chw, device=DEV)
        sig = torch.empty(dup * B, device=DEV)
        st = torch.cuda.current_stream().cuda_stream

        def net_in(v, c):
            s32, g32 = r[_col('s' + c)].float(), r[_col('sig' + c)].float()
            return (1 / (sd ** 2 + g32 ** 2).sqrt()) * (v.float() / s32), g32

        def denoise(v, Fp, c):
            s32, g32 = r[_col('s' + c)].float(), r[_col('sig' + c)].float()
            Fg = Fp[B:] + s * (Fp[:B] - Fp[B:]) if use_cfg else Fp
            return ((sd ** 2 / (g32 ** 2 + sd ** 2)) * (v.float() / s32) + (g32 * sd / (g32 ** 2 + sd ** 2).sqrt()) * Fg).double()

        call('mdt_ablation_prep', x.data_ptr(), noise.data_ptr(), table.data_ptr(), step.data_ptr(), 0, x_hat.data_ptr(),
             xin.data_ptr(), sig.data_ptr(), B, chw, dup, sd, st)
        xh_ref = r[_col('a')] * x0 + r[_col('c')] * noise
        xin_ref, g32 = net_in(xh_ref, '')
        e = [_relmax(x_hat, xh_ref), _relmax(xin[:B], xin_ref)]
        assert torch.equal(xin[:B], xin[B:]) if use_cfg else True
        assert torch.equal(sig, g32.expand(dup * B))
        F1 = torch.randn(dup * B, chw, device=DEV)
        call('mdt_ablation_slope1', x_hat.data_ptr(), F1.data_ptr(), table.data_ptr(), step.data_ptr(), s, int(use_cfg),
             d_cur.data_ptr(), x.data_ptr(), B, chw, sd, st)
        d_ref = r[_col('p')] * xh_ref - r[_col('q')] * denoise(xh_ref, F1, '')
        e += [_relmax(d_cur, d_ref)]
        if second[i]:
            xp_ref = xh_ref + r[_col('ah')] * d_ref
            e += [_relmax(x, xp_ref)]
            call('mdt_ablation_prep', x.data_ptr(), noise.data_ptr(), table.data_ptr(), step.data_ptr(), 1, x_hat.data_ptr(),
                 xin.data_ptr(), sig.data_ptr(), B, chw, dup, sd, st)
            xin2_ref, g32b = net_in(xp_ref, '2')
            e += [_relmax(xin[:B], xin2_ref), _relmax(x_hat, xh_ref)]
            assert torch.equal(sig, g32b.expand(dup * B))
            F2 = torch.randn(dup * B, chw, device=DEV)
            call('mdt_ablation_slope2', x_hat.data_ptr(), x.data_ptr(), F2.data_ptr(), d_cur.data_ptr(), table.data_ptr(),
                 step.data_ptr(), s, int(use_cfg), B, chw, sd, st)
            dp_ref = r[_col('p2')] * xp_ref - r[_col('q2')] * denoise(xp_ref, F2, '2')
            xn_ref = xh_ref + r[_col('h')] * (r[_col('w1')] * d_ref + r[_col('w2')] * dp_ref)
        else:
            xn_ref = xh_ref + r[_col('h')] * d_ref
        e += [_relmax(x, xn_ref)]
        print(f'step {i} cfg {use_cfg}: ' + ' '.join(f'{v:.1e}' for v in e))
        assert max(e) <= 1e-6


@pytest.mark.parametrize('name,cfg_scale', RUNS)
def test_fp32_vs_reference_fixture(golden_dir, name, cfg_scale):
    """precision='fp32' within TOL_F32 of max|z|; the full VP triple within 2.5x the reference's own +-1-ulp spread."""
    g, combos = _fx(golden_dir)
    net = _build(int(g['seed']))
    k = _key(name, cfg_scale)
    z = _run(net, g, combos[name], cfg_scale, precision='fp32')
    assert z.dtype == torch.float64 and z.shape == (len(g['seeds']), 4, 32, 32)
    e = _relmax(z, torch.from_numpy(g[f'{k}_z']))
    spread = float(g[f'{k}_spread'])
    bound = 2.5 * spread if name == 'vp_vp_vp' else TOL_F32
    print(f'fp32 {k}: rel-to-max {e:.2e} (reference +-1 ulp spread {spread:.2e}, bound {bound:.2e})')
    assert e <= bound


@pytest.mark.parametrize('name,cfg_scale', RUNS)
def test_bf16_vs_reference_fixture(golden_dir, name, cfg_scale):
    g, combos = _fx(golden_dir)
    net = _build(int(g['seed']))
    k = _key(name, cfg_scale)
    z = _run(net, g, combos[name], cfg_scale, precision='bf16')
    e = _relmax(z, torch.from_numpy(g[f'{k}_z']))
    print(f'bf16 {k}: rel-to-max {e:.2e}')
    assert e <= TOL_BF16


@pytest.mark.parametrize('name', ['edm_heun', 'vp_vp_none'])
def test_bf16x3_vs_reference_fixture(golden_dir, name):
    g, combos = _fx(golden_dir)
    net = _build(int(g['seed']))
    z = _run(net, g, combos[name], 1.5, precision='bf16x3')
    e = _relmax(z, torch.from_numpy(g[f'{name}_z']))
    print(f'bf16x3 {name}: rel-to-max {e:.2e}')
    assert e <= TOL_F32


def test_graph_replay_direct_launch_and_capture_reuse(golden_dir):
    g, combos = _fx(golden_dir)
    net = _build(int(g['seed']))
    for name in ('edm_heun', 'edm_churn'):
        z = _run(net, g, combos[name], 1.5)
        z_again = _run(net, g, combos[name], 1.5)
        z_direct = _run(net, g, combos[name], 1.5, use_graph=False)
        assert torch.equal(z, z_again) and torch.equal(z, z_direct), name
    assert len(ablation._CACHE) == 1
    (key, entry), = ablation._CACHE.items()
    graphs = (entry.graph_full, entry.graph_short)
    handles = tuple(h.value for h in graphs)
    for kw in (dict(discretization='vp', schedule='vp', scaling='vp'), dict(discretization='ve', schedule='ve'),
               dict(discretization='iddpm', alpha=0.5), dict(solver='euler', S_churn=3)):
        for n in (3, 7):
            lat = torch.randn(len(g['seeds']), 4, 32, 32, device=DEV)
            z = M.ablation_sampler(net, lat, None, cfg_scale=1.5, num_steps=n, **kw)
            assert bool(torch.isfinite(z).all())
            assert ablation._CACHE.get(key) is entry and (entry.graph_full, entry.graph_short) == graphs
            assert graphs[0] is entry.graph_full and tuple(h.value for h in graphs) == handles
    M.ablation_sampler(net, lat, None, cfg_scale=2.0, num_steps=3)  # a new cfg_scale is a captured value: re-capture
    assert ablation._CACHE.get(key) is entry and entry.graph_full is not graphs[0] and entry.captured_cfg == 2.0
    with pytest.raises(NotImplementedError):
        M.ablation_sampler(net, lat, None, feat=torch.zeros(1))
    with pytest.raises(ValueError):
        M.ablation_sampler(net, lat, None, num_steps=ablation.MAX_STEPS + 1)


def test_edm_sampler_unchanged_by_ablation_runs(golden_dir):
    gs = np.load(os.path.join(golden_dir, 's2_sampler.npz'), allow_pickle=False)
    net = _build(int(gs['seed']))
    labels = torch.eye(1000)[torch.from_numpy(gs['cls'])].to(DEV)
    lat = torch.from_numpy(gs['latents']).to(DEV)
    n = int(gs['num_steps'])
    z0 = M.edm_sampler(net, lat, labels, cfg_scale=float(gs['cfg_scale']), num_steps=n)
    z0_direct = M.edm_sampler(net, lat, labels, cfg_scale=float(gs['cfg_scale']), num_steps=n, use_graph=False)
    g, combos = _fx(golden_dir)
    for name in ('edm_heun', 'vp_vp_vp', 'edm_churn'):
        _run(net, g, combos[name], 1.5)
        _run(net, g, combos[name], None, use_graph=False)
    z1 = M.edm_sampler(net, lat, labels, cfg_scale=float(gs['cfg_scale']), num_steps=n)
    z1_direct = M.edm_sampler(net, lat, labels, cfg_scale=float(gs['cfg_scale']), num_steps=n, use_graph=False)
    assert torch.equal(z0, z1) and torch.equal(z0_direct, z1_direct)
    assert sampler._CACHE and ablation._CACHE
    sampler.release_graphs()
    assert not sampler._CACHE and not ablation._CACHE


CFG = """
model: {precond: edm, model_type: DiT-S/2, in_size: 32, in_channels: 4, num_classes: 1000, use_decoder: true,
        pad_cls_token: false, ext_feature_dim: 0, mask_ratio: 0.5, mask_ratio_fn: constant, mask_ratio_min: 0.25,
        mae_loss_coef: 0.1, class_dropout_prob: 0.1}
train: {batchsize: 16, grad_accum: 2, lr: 1.0e-3, lr_rampup_kimg: 0, max_num_steps: 6}
data: {category: synthetic, resolution: 32, num_channels: 4, root: none}
log: {log_every: 2, ckpt_every: 3}
"""


def test_generate_routes_ablation_flags(tmp_path):
    """generate.py --solver euler --discretization vp == a direct ablation_sampler call with the same seeds; without the
    flags == a direct edm_sampler call."""
    import generate as G
    cfg = os.path.join(str(tmp_path), 'cfg.yaml')
    with open(cfg, 'w') as f:
        f.write(CFG)
    net = _build(21)
    ck = os.path.join(str(tmp_path), 'ck.pt')
    torch.save({'ema': {k: v.detach().cpu() for k, v in net.state_dict().items()}}, ck)
    seeds = [5, 9, 11]
    common = ['--config', cfg, '--ckpt_path', ck, '--seeds', '5,9,11', '--num_steps', '4', '--cfg_scale', '1.5']
    for extra, fn, kw in ((['--solver', 'euler', '--discretization', 'vp'], M.ablation_sampler,
                           dict(S_churn=0, solver='euler', discretization='vp')),
                          ([], M.edm_sampler, {})):
        out = os.path.join(str(tmp_path), 'ab' if extra else 'edm')
        assert G.main(common + extra + ['--outdir', out]) == 3
        rnd = M.StackedRandomGenerator(DEV, seeds)
        lat = rnd.randn([3, 4, 32, 32], device=DEV)
        labels = torch.eye(1000, device=DEV)[rnd.randint(1000, size=[3], device=DEV)]
        z = fn(net, lat, labels, cfg_scale=1.5, randn_like=rnd.randn_like, num_steps=4, precision='bf16', **kw).cpu().numpy()
        got = np.stack([np.load(os.path.join(out, f'{s:06d}.npy')) for s in seeds])
        print(f'generate.py {extra}: max |diff| {np.abs(got - z).max():.2e}')
        assert np.array_equal(got, z), extra


def test_train_in_loop_eval_with_ablation_flag(tmp_path, monkeypatch):
    import train as T
    calls = []
    real = ablation.ablation_sampler

    def counting(*a, **k):
        calls.append(k)
        return real(*a, **k)

    monkeypatch.setattr(ablation, 'ablation_sampler', counting)
    tmp = str(tmp_path)
    cfg = os.path.join(tmp, 'cfg.yaml')
    with open(cfg, 'w') as f:
        f.write(CFG)
    args = T.parse(['--config', cfg, '--results_dir', tmp, '--exp_name', 'r', '--max_num_steps', '3', '--enable_eval',
                    '--eval_seeds', '4', '--num_steps', '3', '--cfg_scale', '1.5', '--max_batch_size', '4', '--solver', 'heun'])
    out = T.train_loop(args)
    ev = out['eval']
    assert ev is not None and ev['n'] == 4 and np.isfinite(ev['mean']) and ev['std'] > 0
    assert 'edm-steps3-ckpt3_cfg1.5' in ev['outdir'] and len(os.listdir(ev['outdir'])) == 4
    assert len(calls) == 1 and calls[0]['solver'] == 'heun' and calls[0]['num_steps'] == 3 and calls[0]['S_churn'] == 0
