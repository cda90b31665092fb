"""fp32 training of the unmasked stage (train.py --no_amp): what can be checked without a GPU -- the C ABI of
csrc/f32train.hip (declared, exported, bound; argument validation), the command-line switch and the public setter."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ['mdt_gemm_f32_tn', 'mdt_gemm_f32_tn_ws_floats', 'mdt_colsum_f32', 'mdt_colsum_f32_ws_floats', 'mdt_attn_f32_bwd',
               'mdt_attn_f32_bwd_ws_floats', 'mdt_ln_modulate_bwd_f32', 'mdt_gate_bwd_f32', 'mdt_gate_res_f32', 'mdt_gelu_f32',
               'mdt_gelu_bwd_f32', 'mdt_silu_bwd_f32']


def test_new_entries_declared_exported_and_bound():
    from maskdit_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'maskdit_hip.h')).read()
    L = _lib.lib()
    for name in NEW_ENTRIES:
        assert re.search(r'\b(int|long)\s+%s\s*\(' % name, header), f'{name} is not declared in maskdit_hip.h'
        assert hasattr(L, name), f'{name} is not exported by the built library'
        assert name in _lib._PROTOS or name in _lib._PLAIN, f'{name} is not bound in _lib.py'
    assert 'f32train.hip' in open(os.path.join(ROOT, 'maskdit_amd', 'csrc', 'Makefile')).read()
    assert C.sizeof(_lib.GemmF32TNArgs) == 144  # 3 pointers + ws, 4 + 6 + 1 longs, 6 ints padded to 8-byte slots


def _tn_args(**kw):
    from maskdit_amd._lib import GemmF32TNArgs
    a = GemmF32TNArgs()
    # plausible HOST addresses: validation must refuse before anything is launched
    a.A, a.B, a.C = 4096, 8192, 16384
    a.M, a.N1, a.N2, a.lda, a.ldb, a.ldc = 64, 8, 16, 8, 16, 16
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize('kw,word', [(dict(A=None), 'null'), (dict(C=None), 'null'), (dict(N1=6, lda=6), 'multiples of 4'),
                                     (dict(M=4104, N1=384, N2=1536, lda=384, ldb=1536, ldc=1536), 'workspace'),
                                     (dict(M=4104, N1=384, N2=1536, lda=384, ldb=1536, ldc=1536, ws=65536, ws_floats=1000), 'workspace')])
def test_gemm_f32_tn_argument_validation(kw, word):
    from maskdit_amd import _lib
    L = _lib.lib()
    rc = L.mdt_gemm_f32_tn(C.byref(_tn_args(**kw)), None)
    assert rc < 0
    assert word in L.mdt_last_error().decode()
    assert L.mdt_gemm_f32_tn(None, None) < 0


def test_workspace_queries_and_other_entries_validate():
    from maskdit_amd import _lib
    L = _lib.lib()
    assert L.mdt_gemm_f32_tn_ws_floats(64, 4, 16, 1) == 0               # one chunk: no workspace
    n = L.mdt_gemm_f32_tn_ws_floats(4104, 384, 1536, 1)
    assert n > 384 * 1536 and n % (384 * 1536) == 0                      # several chunks of partial products
    assert L.mdt_gemm_f32_tn_ws_floats(4104, 384, 1536, 1) == n          # a function of the shape alone
    assert L.mdt_colsum_f32_ws_floats(100, 64) == 0 and L.mdt_colsum_f32_ws_floats(4104, 64) > 0
    assert L.mdt_attn_f32_bwd_ws_floats(2, 64, 3, 32) >= 2 * 2 * 3 * 64 * 64
    for name, args in [('mdt_colsum_f32', (None, 64, None, None, 0, 100, 64, 0)),
                       ('mdt_colsum_f32', (4096, 64, 8192, None, 0, 4104, 64, 0)),             # needs a workspace
                       ('mdt_attn_f32_bwd', (None, None, None, 0, None, 2, 64, 3, 32)),
                       ('mdt_attn_f32_bwd', (4096, 8192, 16384, 10, 32768, 2, 64, 3, 32)),     # workspace too small
                       ('mdt_ln_modulate_bwd_f32', (None, None, None, 4, 64, None, 0, None, None, 4, None, 64, 384)),
                       ('mdt_gate_bwd_f32', (None, None, None, 4, 64, None, None, 4, 64, 384)),
                       ('mdt_gate_res_f32', (None, None, None, 4, 64, None, 64, 384)),
                       ('mdt_gelu_f32', (None, None, 10)), ('mdt_gelu_bwd_f32', (None, None, None, 10)),
                       ('mdt_silu_bwd_f32', (None, None, None, 10))]:
        assert getattr(L, name)(*args, None) < 0, name
        assert L.mdt_last_error().decode()


def _run_train(*argv):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), *argv], capture_output=True, text=True, cwd=ROOT, env=env)


def test_no_amp_on_the_masked_config_is_refused_at_start_up():
    r = _run_train('--no_amp', '--config', 'configs/xl2-256-synthetic.yaml')
    assert r.returncode != 0
    assert 'UNMASKED stage' in r.stderr and 'mask_ratio' in r.stderr and '0.5' in r.stderr


def test_no_amp_resolves_to_fp32_on_the_finetune_config():
    import train as T
    from maskdit_amd.schedule import load_config
    cfg = load_config(os.path.join(ROOT, 'configs', 'xl2-256-finetune-synthetic.yaml'))
    ref = load_config(os.path.join(ROOT, 'configs', 'xl2-256-synthetic.yaml'))
    assert cfg.model.mask_ratio == 0 and T.mask_ratio_max(cfg) == 0
    ref.model['mask_ratio'] = cfg.model.mask_ratio
    assert cfg == ref, 'the finetune config is the synthetic config with mask_ratio 0'
    args = T.parse(['--no_amp', '--config', 'configs/xl2-256-finetune-synthetic.yaml'])
    assert args.no_amp and T.resolve_train_precision(args, cfg) == 'fp32'
    assert T.resolve_train_precision(T.parse(['--config', 'x.yaml']), ref) == 'bf16'
    # a schedule that is ever > 0 is refused, a constant 0 and an all-zero schedule are not
    for fn, ratio, rmin, ok in [('constant', 0.5, 0, False), ('linear', 0.0, 0.25, False), ('cosine2', 0.75, 0.0, False),
                                ('exp', 0.0, 0.0, True), ('constant', 0.0, 0.3, True)]:
        cfg.model.update(mask_ratio_fn=fn, mask_ratio=ratio, mask_ratio_min=rmin)
        if ok:
            assert T.resolve_train_precision(args, cfg) == 'fp32'
        else:
            with pytest.raises(SystemExit, match='UNMASKED'):
                T.resolve_train_precision(args, cfg)


def test_set_train_precision_names_and_deepcopy():
    import copy
    import maskdit_amd as M
    net = M.Precond_models['edm'](img_resolution=16, img_channels=4, num_classes=1000, model_type='DiT-S/2')
    assert net.train_precision == 'bf16'
    for bad in ('tf32', 'bf16x3', 'FP32', ''):
        with pytest.raises(ValueError):
            net.set_train_precision(bad)
    assert net.set_train_precision('fp32') is net and net.train_precision == 'fp32'
    assert net._train_plan_precision(False) == 'fp32'
    with pytest.raises(NotImplementedError, match='UNMASKED'):
        net._train_plan_precision(True)
    assert copy.deepcopy(net).train_precision == 'fp32'  # the EMA copy of train.py follows the net
    assert net.set_train_precision('bf16')._train_plan_precision(True) == 'bf16'
    assert M.unwrap_model(net).train_precision == 'bf16'
