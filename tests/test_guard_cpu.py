"""CPU-side checks of the optimizer-step guard: the three library entries refuse bad arguments before any
launch, FusedAdam refuses a bad `max_grad_norm`, train.py reads the config keys and lets the flags override them."""
import os
import sys

import pytest
import torch

from maskdit_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NEW = ['mdt_grad_sumsq', 'mdt_grad_sumsq_chunk', 'mdt_grad_sumsq_ws_floats', 'mdt_guard_decide', 'mdt_adamw_ema_step_guarded']


def test_entries_exported_and_chunk_is_a_function_of_n():
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTED and hasattr(L, name)
    assert L.mdt_grad_sumsq_chunk(1) == L.mdt_grad_sumsq_chunk(16384 * 8192) == 16384
    assert L.mdt_grad_sumsq_chunk(16384 * 8192 + 1) == 32768
    for n in (1, 7, 16384, 16385, 5_000_011, 675_000_000):
        chunk = L.mdt_grad_sumsq_chunk(n)
        chunks = -(-n // chunk)
        assert chunk % 4 == 0 and chunks <= 8192 and L.mdt_grad_sumsq_ws_floats(n) == 2 * chunks
    assert L.mdt_grad_sumsq_ws_floats(0) == 0


def test_sumsq_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    f = L.mdt_grad_sumsq
    assert f(None, 8, 1.0, 64, 2, 64, 0, None) != 0 and b'null pointer' in L.mdt_last_error()
    assert f(64, 8, 1.0, None, 2, 64, 0, None) != 0 and b'null pointer' in L.mdt_last_error()
    assert f(64, 8, 1.0, 64, 2, None, 0, None) != 0 and b'null pointer' in L.mdt_last_error()
    assert f(64, 0, 1.0, 64, 2, 64, 0, None) != 0 and b'n must be positive' in L.mdt_last_error()
    assert f(68, 8, 1.0, 64, 2, 64, 0, None) != 0 and b'16-byte aligned' in L.mdt_last_error()
    assert f(64, 8, 1.0, 72, 2, 64, 0, None) != 0 and b'16-byte aligned' in L.mdt_last_error()
    assert f(64, 8, 1.0, 64, 2, 72, 0, None) != 0 and b'16-byte aligned' in L.mdt_last_error()
    assert f(64, 40000, 1.0, 64, 4, 64, 0, None) != 0 and b'workspace smaller' in L.mdt_last_error()  # 3 chunks need 6


def test_decide_and_guarded_step_refuse_bad_arguments_before_any_launch():
    L = _lib.lib()
    d = L.mdt_guard_decide
    assert d(None, 1.0, 1, 0.9, 0.999, None) != 0 and b'null guard state' in L.mdt_last_error()
    assert d(72, 1.0, 1, 0.9, 0.999, None) != 0 and b'16-byte aligned' in L.mdt_last_error()
    assert d(64, -1.0, 1, 0.9, 0.999, None) != 0 and b'max_norm' in L.mdt_last_error()
    assert d(64, float('nan'), 1, 0.9, 0.999, None) != 0 and b'max_norm' in L.mdt_last_error()
    assert d(64, float('inf'), 1, 0.9, 0.999, None) != 0 and b'max_norm' in L.mdt_last_error()
    assert d(64, 1.0, 1, 1.0, 0.999, None) != 0 and b'betas' in L.mdt_last_error()
    s = L.mdt_adamw_ema_step_guarded
    hyp = (1e-3, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.001, 0.0, 1.0)
    assert s(None, 64, 64, 64, None, None, 8, *hyp, 64, 0, None) != 0 and b'null pointer' in L.mdt_last_error()
    assert s(64, 64, 64, 64, None, None, 8, *hyp, None, 0, None) != 0 and b'null guard state' in L.mdt_last_error()
    assert s(64, 64, 64, 64, None, None, 0, *hyp, 64, 0, None) != 0 and b'bad arguments' in L.mdt_last_error()
    assert s(64, 68, 64, 64, None, None, 8, *hyp, 64, 0, None) != 0 and b'16-byte aligned' in L.mdt_last_error()
    assert s(64, 64, 64, 64, None, None, 8, *hyp, 72, 0, None) != 0 and b'guard state must be 16-byte aligned' in L.mdt_last_error()
    bad_bc = (1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.0, 0.0, 1.0)  # host bias corrections of 0: only the device's may replace them
    assert s(64, 64, 64, 64, None, None, 8, *bad_bc, 64, 0, None) != 0 and b'bad arguments' in L.mdt_last_error()


def test_fused_adam_refuses_a_bad_max_grad_norm():
    from maskdit_amd.optim import FusedAdam
    p = [torch.nn.Parameter(torch.zeros(4))]
    for bad in (-1, -0.5, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='max_grad_norm'):
            FusedAdam(p, max_grad_norm=bad)
    for off in (None, 0, 0.0, False):
        opt = FusedAdam(p, max_grad_norm=off)
        assert opt._guard_cfg is None and opt._guard is None and opt.grad_norm is None and opt.skipped_steps == 0
    assert FusedAdam(p, max_grad_norm=2)._guard_cfg == (2.0, False)
    assert FusedAdam(p, skip_nonfinite=True)._guard_cfg == (0.0, True)
    with pytest.raises(ValueError, match='same betas'):
        FusedAdam([{'params': p}, {'params': [torch.nn.Parameter(torch.zeros(4))], 'betas': (0.5, 0.9)}], skip_nonfinite=True)


CFG = """
model: {precond: edm, model_type: DiT-S/2, in_size: 16, in_channels: 4, num_classes: 1000, use_decoder: true,
        pad_cls_token: false, mask_ratio: 0.5, mae_loss_coef: 0.1, class_dropout_prob: 0.1}
train: {batchsize: 4, lr: 1.0e-3%s}
log: {log_every: 2, ckpt_every: 100}
"""


def test_train_flags_and_config_keys(tmp_path):
    import train as T
    from maskdit_amd.schedule import load_config

    def cfg(extra, name):
        path = os.path.join(str(tmp_path), name)
        with open(path, 'w') as f:
            f.write(CFG % extra)
        return path

    plain = cfg('', 'plain.yaml')
    keyed = cfg(', max_grad_norm: 2.5, skip_nonfinite: true', 'keyed.yaml')
    a = T.parse(['--config', plain])
    assert a.max_grad_norm is None and a.skip_nonfinite is None
    assert T.resolve_guard(a, load_config(plain)) == {}                                   # default: off, no keywords at all
    assert T.resolve_guard(T.parse(['--config', keyed]), load_config(keyed)) == {'max_grad_norm': 2.5, 'skip_nonfinite': True}
    a = T.parse(['--config', plain, '--max_grad_norm', '0.5', '--skip_nonfinite'])
    assert T.resolve_guard(a, load_config(plain)) == {'max_grad_norm': 0.5, 'skip_nonfinite': True}
    a = T.parse(['--config', keyed, '--max_grad_norm', '0', '--skip_nonfinite', 'false'])    # the flags override the keys
    assert T.resolve_guard(a, load_config(keyed)) == {}
    a = T.parse(['--config', keyed, '--max_grad_norm', '1'])
    assert T.resolve_guard(a, load_config(keyed)) == {'max_grad_norm': 1.0, 'skip_nonfinite': True}
