"""ablation_sampler (maskdit_amd/ablation.py) without a GPU: the per-step coefficient table against the reference's own
ablation_sampler (tests/golden/ablation_sampler.npz, made by make_golden_ablation.py), the argument checks, the C ABI
entries and the routing of the sampling entry points (sample.py:240-245)."""
import contextlib
import ctypes as C
import io
import json
import os
import re

import numpy as np
import pytest
import torch

import maskdit_amd as M
from maskdit_amd import _lib, ablation
from maskdit_amd.ablation import COLS, select_sampler, step_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['edm_heun', 'edm_euler', 'vp_vp_vp', 'vp_vp_none', 'edm_vp_vp', 've_ve_none', 'iddpm', 'vp_euler_linear',
         'edm_alpha05', 'edm_churn']
K = {c: i for i, c in enumerate(COLS)}


@pytest.fixture(scope='module')
def fx(golden_dir):
    g = np.load(os.path.join(golden_dir, 'ablation_sampler.npz'), allow_pickle=False)
    combos = {name: (kw, nocfg) for name, kw, nocfg in json.loads(str(g['combos']))}
    assert list(combos) == NAMES
    return g, combos


def _net_sigmas(table, second):
    out = []
    for i, two in enumerate(second):
        out.append(table[i, K['sig']].item())
        if two:
            out.append(table[i, K['sig2']].item())
    return np.array(out)


@pytest.mark.parametrize('name', NAMES)
def test_table_network_sigma_matches_reference(fx, name):
    """The noise level of every network call, in call order, equals the reference's to within 1 ulp."""
    g, combos = fx
    kw, nocfg = combos[name]
    table, _, second = step_table(int(g['num_steps']), 'cpu', 0, float('inf'), **kw)
    assert table.dtype == torch.float64 and table.shape == (int(g['num_steps']), ablation.NCOL)
    got = _net_sigmas(table, second)
    for tag in [''] + (['_nocfg'] if nocfg else []):
        ref = g[f'{name}{tag}_sig']
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        ulps = np.abs(got - ref) / np.spacing(np.abs(ref))
        print(f'{name}{tag}: {len(ref)} evaluations, max {ulps.max():.0f} ulp')
        assert (ulps <= 1).all(), (name, ulps)


def _toy(x32, sig, sd):
    s = torch.as_tensor(sig, dtype=torch.float64)
    return x32.to(torch.float64) * (sd ** 2 / (s * s + sd ** 2))


@pytest.mark.parametrize('name', NAMES)
def test_table_applied_as_the_kernels_do_reproduces_reference_toy_run(fx, name):
    """A fp64 loop that applies each table row exactly as mdt_ablation_prep / slope1 / slope2 are specified reproduces the
    reference's ablation_sampler on an analytic denoiser (no network) to 1e-12 of max|z|."""
    g, combos = fx
    kw, _ = combos[name]
    n, sd = int(g['num_steps']), float(g['sigma_data'])
    table, scale0, second = step_table(n, 'cpu', 0, float('inf'), **kw)
    rnd = M.StackedRandomGenerator('cpu', [int(s) for s in g['seeds']])
    x = rnd.randn([int(v) for v in g['toy_shape']]).to(torch.float64) * scale0
    for i in range(n):
        r = table[i]
        noise = rnd.randn_like(x)
        x_hat = r[K['a']] * x + r[K['c']] * noise
        D = _toy(x_hat.float() / r[K['s']].float(), r[K['sig']], sd)
        d = r[K['p']] * x_hat - r[K['q']] * D
        if second[i]:
            xp = x_hat + r[K['ah']] * d
            D2 = _toy(xp.float() / r[K['s2']].float(), r[K['sig2']], sd)
            d2 = r[K['p2']] * xp - r[K['q2']] * D2
            x = x_hat + r[K['h']] * (r[K['w1']] * d + r[K['w2']] * d2)
        else:
            x = x_hat + r[K['h']] * d
    ref = torch.from_numpy(g[f'{name}_toy'])
    e = ((x - ref).abs().max() / ref.abs().max()).item()
    print(f'{name}: toy run rel-to-max {e:.2e}')
    assert e <= 1e-12


def test_second_evaluation_flags_and_churn_coefficient():
    _, _, second = step_table(5, 'cpu', solver='heun')
    assert second == [True, True, True, True, False]
    _, _, second = step_table(5, 'cpu', solver='euler')
    assert second == [False] * 5
    table, _, _ = step_table(6, 'cpu', S_churn=10, S_min=0.05, S_max=50, S_noise=1.003)
    c = table[:, K['c']]
    # sigma(t_0) = 80 is above S_max and sigma(t_5) = 0.002 below S_min: churn on steps 1-4 only
    assert c[0] == 0 and (c[1:5] > 0).all() and c[5] == 0
    assert (table[:, len(COLS):] == 0).all()


@pytest.mark.parametrize('arg,value', [('solver', 'rk4'), ('discretization', 'cosine'), ('schedule', 'exp'),
                                       ('scaling', 've')])
def test_unknown_choices_raise(arg, value):
    with pytest.raises(ValueError):
        step_table(4, 'cpu', **{arg: value})
    with pytest.raises(ValueError):  # before any device work
        M.ablation_sampler(None, torch.zeros(1, 4, 32, 32), **{arg: value})


def test_header_columns_and_entries():
    hdr = open(os.path.join(ROOT, 'include', 'maskdit_hip.h')).read()
    cols = dict((k, int(v)) for k, v in re.findall(r'#define MDT_ABL_(\w+) (\d+)', hdr))
    assert cols.pop('NCOL') == ablation.NCOL
    assert sorted(cols.items(), key=lambda kv: kv[1]) == [(c.upper(), i) for i, c in enumerate(COLS)]
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    for name in ('mdt_ablation_prep', 'mdt_ablation_slope1', 'mdt_ablation_slope2'):
        assert name in _lib.EXPORTED and re.search(rf'\bint {name}\(', hdr)
    # argument checks run before any HIP call
    assert L.mdt_ablation_prep(None, None, None, None, 0, None, None, None, 1, 16, 1, C.c_float(0.5), None) != 0
    assert b'null pointer' in L.mdt_last_error()
    p = C.c_void_p(8)
    assert L.mdt_ablation_prep(p, None, p, p, 0, None, p, p, 1, 16, 1, C.c_float(0.5), None) != 0
    assert b'which = 0 needs noise' in L.mdt_last_error()
    assert L.mdt_ablation_prep(p, p, p, p, 2, p, p, p, 1, 16, 1, C.c_float(0.5), None) != 0
    assert L.mdt_ablation_prep(p, p, p, p, 0, p, p, p, 1, 16, 3, C.c_float(0.5), None) != 0
    assert L.mdt_ablation_slope1(p, p, p, p, C.c_float(1.5), 1, p, p, 0, 16, C.c_float(0.5), None) != 0
    assert L.mdt_ablation_slope2(p, p, p, None, p, p, C.c_float(1.5), 1, 1, 16, C.c_float(0.5), None) != 0


def test_routing_follows_the_reference():
    """sample.py:240-245: any of the four ablation keywords -> ablation_sampler with the non-None keywords."""
    fn, kw = select_sampler(50, 0)
    assert fn is M.edm_sampler and kw == dict(num_steps=50, S_churn=0)
    fn, kw = select_sampler(18, 40)
    assert fn is M.edm_sampler and kw == dict(num_steps=18, S_churn=40)
    for key in ('solver', 'discretization', 'schedule', 'scaling'):
        value = {'solver': 'euler', 'discretization': 'vp', 'schedule': 've', 'scaling': 'none'}[key]
        fn, kw = select_sampler(32, 0, **{key: value})
        assert fn is M.ablation_sampler and kw == {'num_steps': 32, 'S_churn': 0, key: value}
    fn, kw = select_sampler(6, 10, 'heun', 'edm', 'linear', 'vp')
    assert fn is M.ablation_sampler
    assert kw == dict(num_steps=6, S_churn=10, solver='heun', discretization='edm', schedule='linear', scaling='vp')


def test_entry_points_list_the_five_flags():
    import generate
    import train
    for main in (generate.main, train.parse):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf), pytest.raises(SystemExit):
            main(['--help'])
        text = buf.getvalue()
        for flag in ('--S_churn', '--solver {euler,heun}', '--discretization {vp,ve,iddpm,edm}', '--schedule {vp,ve,linear}',
                     '--scaling {vp,none}'):
            assert flag in text, (main.__module__, flag)
    with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
        generate.main(['--config', 'x.yaml', '--solver', 'rk4'])
    a = train.parse(['--config', 'x.yaml'])
    assert (a.S_churn, a.solver, a.discretization, a.schedule, a.scaling) == (0, None, None, None, None)
    assert (a.num_steps, a.cfg_scale, a.enable_eval) == (40, None, False)
    b = train.parse(['--config', 'x.yaml', '--enable_eval', '--solver', 'heun', '--S_churn', '5'])
    assert (b.solver, b.S_churn) == ('heun', 5)
