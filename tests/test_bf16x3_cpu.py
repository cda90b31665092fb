"""bf16x3 split-operand GEMM (csrc/f32path.hip, mdt_gemm_bf16x3) without a GPU: the entry is declared, exported and bound,
its argument checks run before any HIP call, and the precision name reaches every public switch."""
import contextlib
import ctypes as C
import io
import os
import re

import pytest

from maskdit_amd import _lib, engine, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def built():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, 'include', 'maskdit_hip.h')).read()
    assert re.search(r'int mdt_gemm_bf16x3\(const mdt_gemm_f32_args\* a, mdt_stream_t stream\);', hdr)
    assert int(re.search(r'#define MDT_ABI_VERSION (\d+)', hdr).group(1)) == 4 == built.mdt_version()
    assert hasattr(built, 'mdt_gemm_bf16x3') and 'mdt_gemm_bf16x3' in _lib.EXPORTED
    assert _lib._PROTOS['mdt_gemm_bf16x3'] == [C.POINTER(_lib.GemmF32Args)]
    assert callable(ops.gemm_bf16x3)


def _args(**kw):
    g = _lib.GemmF32Args()
    g.A, g.B, g.out, g.lda, g.ldb, g.ldo, g.M, g.N, g.K = 16, 16, 16, 8, 8, 8, 4, 4, 8
    for k, v in kw.items():
        setattr(g, k, v)
    return g


@pytest.mark.parametrize('change,msg', [
    (dict(A=None), b'gemm_bf16x3: null pointer'),
    (dict(B=None), b'gemm_bf16x3: null pointer'),
    (dict(out=None), b'gemm_bf16x3: null pointer'),
    (dict(K=6), b'gemm_bf16x3: M, N > 0 and K a positive multiple of 4'),
    (dict(epi=3), b'gemm_bf16x3: GATE_RES needs res and rows_per_sample'),
    (dict(batch=2), b'bf16x3: linear layers only'),
    (dict(batch=4, heads=2), b'bf16x3: linear layers only'),
    (dict(b_kmajor=1), b'bf16x3: linear layers only'),
])
def test_argument_validation_without_gpu(built, change, msg):
    assert built.mdt_gemm_bf16x3(C.byref(_args(**change)), None) != 0
    assert msg in built.mdt_last_error()


def test_precision_names():
    for prec in ('bf16', 'fp32', 'bf16x3'):
        assert engine.check_precision(prec) == prec
    for bad in ('fp16', 'tf32', 'bf16x2'):
        with pytest.raises(ValueError):
            engine.check_precision(bad)
    assert [engine.reads_f32_arena(p) for p in ('bf16', 'fp32', 'bf16x3')] == [False, True, True]
    assert engine.plan_key(4, False, False, None, 'bf16x3') != engine.plan_key(4, False, False, None, 'fp32')


def test_public_switches_accept_bf16x3():
    import maskdit_amd as M
    net = M.Precond_models['edm'](img_resolution=32, img_channels=4, num_classes=1000, model_type='DiT-S/2', pad_cls_token=False)
    assert net.eval_precision == 'bf16'
    assert net.set_eval_precision('bf16x3') is net and net.eval_precision == 'bf16x3'
    with pytest.raises(M.MaskDiTLibError):  # no CPU path for this arithmetic either
        net(__import__('torch').zeros(1, 4, 32, 32), __import__('torch').ones(1))
    import generate
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), pytest.raises(SystemExit):
        generate.main(['--help'])
    assert '{bf16,fp32,bf16x3}' in buf.getvalue()
