"""The fp32-accurate autoencoder arithmetic (`precision='bf16x3'`) without a GPU: the new entries of the C ABI and
their argument checks, the precision switch of FrozenAutoencoderKL and of both command lines, the fp32 / fp64 fixture
(tests/golden/vae_f32.npz, generated from the reference's own modules by make_golden_vae_f32.py) against the CPU oracles,
and the two ISA audits (hand-counted waits; every kernel that existed before compiles to the same instructions)."""
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from maskdit_amd import _lib
from maskdit_amd import autoencoder as AE
from oracle import vae_oracle as VO
from tests import vae_encoder_ref as VE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('mdt_conv3x3_bf16x3_nhwc', 'mdt_gn_im2col_f32', 'mdt_vae_enc_prologue_f32', 'mdt_gn_stats_ordered')


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def f32(golden_dir):
    return np.load(os.path.join(golden_dir, 'vae_f32.npz'))


def test_new_symbols_exported_and_declared():
    hdr = open(os.path.join(ROOT, 'include', 'maskdit_hip.h')).read()
    L = _lib.lib()
    for name in NEW:
        assert re.search(r'\b(?:int|long) ' + name + r'\s*\(', hdr), f'{name} is not declared in maskdit_hip.h'
        assert name in _lib.EXPORTED and hasattr(L, name)
    assert _lib.ABI_VERSION == 4 and L.mdt_version() == 4  # additions only


def test_argument_validation_without_gpu():
    L = _lib.lib()
    conv = L.mdt_conv3x3_bf16x3_nhwc
    assert conv(None, 1, 8, 128, 0, 0, None, None, None, None, 128, 128, None) != 0 and b'null pointer' in L.mdt_last_error()
    assert conv(16, 1, 8, 100, 0, 0, 16, None, None, 16, 128, 128, None) != 0 and b'multiple of 32' in L.mdt_last_error()
    assert conv(16, 1, 8, 128, 1, 1, 16, None, None, 16, 128, 128, None) != 0 and b'not both' in L.mdt_last_error()
    assert conv(16, 1, 9, 128, 0, 1, 16, None, None, 16, 128, 128, None) != 0 and b'even input side' in L.mdt_last_error()
    assert conv(16, 1, 8, 128, 0, 0, 16, None, None, 16, 64, 128, None) != 0 and b'ldo' in L.mdt_last_error()
    assert conv(20, 1, 8, 128, 0, 0, 16, None, None, 16, 128, 128, None) != 0 and b'aligned' in L.mdt_last_error()
    assert conv(16, 40000, 512, 128, 0, 0, 16, None, None, 16, 128, 128, None) != 0 and b'31 bits' in L.mdt_last_error()
    im = L.mdt_gn_im2col_f32
    assert im(None, None, None, None, None, 1, 8, 8, 128, 32, 1, 0, 0, 128, None) != 0 and b'null pointer' in L.mdt_last_error()
    assert im(16, 16, None, None, 16, 1, 8, 8, 128, 32, 1, 0, 0, 128, None) != 0 and b'normalisation' in L.mdt_last_error()
    assert im(16, None, None, None, 16, 1, 8, 8, 128, 32, 2, 0, 0, 512, None) != 0 and b'1x1 / 3x3' in L.mdt_last_error()
    assert im(16, None, None, None, 16, 1, 8, 8, 4, 32, 3, 0, 0, 32, None) != 0 and b'Kp' in L.mdt_last_error()
    st = L.mdt_gn_stats_ordered
    assert st(16, 16, None, 1, 64, 128, 32, None) != 0 and b'null pointer' in L.mdt_last_error()
    assert st(16, 16, 16, 1, 64, 96, 32, None) != 0 and b'divide 1024' in L.mdt_last_error()
    assert L.mdt_gn_stats_ordered_ws_floats(2, 32) == (4096 + 2) * 64
    pro = L.mdt_vae_enc_prologue_f32
    assert pro(None, 1, 0, 16, 1, 128, 28, None) != 0 and b'null pointer' in L.mdt_last_error()
    assert pro(16, 1, 0, 16, 1, 128, 27, None) != 0 and b'multiple of 4' in L.mdt_last_error()
    assert pro(16, 2, 0, 16, 1, 128, 28, None) != 0 and b'0 or 1' in L.mdt_last_error()


def test_precision_switch():
    assert AE.PRECISIONS == ('bf16', 'bf16x3')
    assert AE.get_model(None).precision == 'bf16' and AE.FrozenAutoencoderKL().precision == 'bf16'
    for bad in ('nope', 'fp32', None):
        with pytest.raises(ValueError):
            AE.get_model(None, precision=bad)
        with pytest.raises(ValueError):
            AE.FrozenAutoencoderKL(precision=bad)
    vae = AE.get_model(None, encoder=True, precision='bf16x3')
    assert vae.precision == 'bf16x3'
    with pytest.raises(ValueError):
        vae.set_precision('nope')
    assert vae.precision == 'bf16x3' and vae.set_precision('bf16').precision == 'bf16'
    vae.set_precision('bf16x3')
    # no CPU path at either precision: the library's own error, before anything is packed
    with pytest.raises(_lib.MaskDiTLibError):
        vae.decode(torch.zeros(1, 4, 32, 32))
    with pytest.raises(_lib.MaskDiTLibError):
        vae.encode_moments(torch.zeros(1, 3, 256, 256))
    with pytest.raises(_lib.MaskDiTLibError):
        vae(torch.zeros(1, 128, 128, 3, dtype=torch.uint8), 'encode')
    assert vae._packed_x3 is None and vae._packed is None
    with pytest.raises(NotImplementedError):  # decode-only models refuse to encode at either precision
        AE.get_model(None, precision='bf16x3').encode_moments(torch.zeros(1, 3, 256, 256))


def test_command_lines_parse_vae_precision():
    import extract_latent
    import generate
    g = generate.build_parser()
    a = g.parse_args(['--config', 'c.yaml'])
    assert a.vae_precision == 'bf16' and a.precision == 'bf16'
    a = g.parse_args(['--config', 'c.yaml', '--precision', 'fp32'])
    assert a.vae_precision == 'bf16'  # --precision is the network only
    assert g.parse_args(['--config', 'c.yaml', '--vae_precision', 'bf16x3']).vae_precision == 'bf16x3'
    e = extract_latent.build_parser()
    assert e.parse_args([]).vae_precision == 'bf16'
    assert e.parse_args(['--vae_precision', 'bf16x3']).vae_precision == 'bf16x3'
    for ap in (g, e):
        with pytest.raises(SystemExit):
            ap.parse_args(['--config', 'c.yaml', '--vae_precision', 'fp32'])


def test_fixture_keys_and_shapes(f32):
    want = {'dec_e_ref': ((), np.float64), 'dec_n_u8_ref': ((), np.int64), 'dec_absmax64': ((), np.float64),
            'dec_lv0_crop': ((3, 128, 128), np.float32), 'dec64_img1_sub': ((3, 64, 64), np.float64),
            'mom64_256': ((8, 32, 32), np.float64), 'enc_e_ref': ((), np.float64)}
    assert set(f32.files) == set(want)
    for k, (shp, dt) in want.items():
        assert f32[k].shape == shp and f32[k].dtype == dt, k
    assert 0 < float(f32['dec_e_ref']) < 1e-5 and 0 < float(f32['enc_e_ref']) < 1e-5  # fp32 rounding through ~30 layers
    assert 0 <= int(f32['dec_n_u8_ref']) < 2 * 3 * 256 * 256
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'vae_f32.npz')) < 400 * 1024


def test_oracles_in_fp32_match_the_fp64_fixture(f32, golden_dir):
    """The oracle restatements in fp32 on the stored inputs lie within 2 e_ref of the stored fp64 values: one reference
    rounding error plus one for the oracle's different operation order -- the fixture and the oracles describe the same
    function."""
    torch.set_num_threads(min(8, torch.get_num_threads()))
    gd = np.load(os.path.join(golden_dir, 'vae_decode.npz'))
    ge = np.load(os.path.join(golden_dir, 'vae_encode.npz'))
    with torch.no_grad():
        img = VO.vae_decode(VO.init_vae_params(seed=int(gd['seed'])), torch.from_numpy(gd['z'])).double()
        mom = VE.vae_encode_moments(VE.init_vae_encoder_params(int(ge['seed'])), VE.u8_to_unit(ge['img256'])[None]).double()
    ref0 = torch.from_numpy(f32['dec_lv0_crop']).double() / 127.5 - 1
    ref1 = torch.from_numpy(f32['dec64_img1_sub'])
    absmax = max(ref0.abs().max().item(), ref1.abs().max().item())
    assert absmax <= float(f32['dec_absmax64'])
    e_dec = max((img[0, :, 64:192, 64:192] - ref0).abs().max().item(), (img[1, :, ::4, ::4] - ref1).abs().max().item()) / absmax
    ref = torch.from_numpy(f32['mom64_256'])
    e_enc = ((mom[0] - ref).abs().max() / ref.abs().max()).item()
    print(f'oracle fp32 vs stored fp64: decode {e_dec:.3e} (dec_e_ref {float(f32["dec_e_ref"]):.3e}), '
          f'encode {e_enc:.3e} (enc_e_ref {float(f32["enc_e_ref"]):.3e})')
    assert e_dec <= 2 * float(f32['dec_e_ref'])
    assert e_enc <= 2 * float(f32['enc_e_ref'])


def test_wait_audit_stays_green():
    """tools/check_waits.py as test_host_cpu.py::test_isa_wait_audit runs it: 0 errors with the new kernels in the build
    (conv3x3_bf16x3_kernel hand-counts no wait: hipcc places them, as in gemm_bf16x3_kernel)."""
    assert _tool('check_waits').main([]) == 0
    src = open(os.path.join(ROOT, 'maskdit_amd', 'csrc', 'f32path.hip')).read()
    body = src[src.index('void conv3x3_bf16x3_kernel'):src.index('void softmax_rows_f32_kernel')]
    assert 's_waitcnt' not in body and 'asm' not in body


def _parent_rev():
    """the newest commit that does not declare the new entries (HEAD while this change is uncommitted, HEAD~1 after)"""
    for rev in ('HEAD', 'HEAD~1'):
        r = subprocess.run(['git', '-C', ROOT, 'show', f'{rev}:include/maskdit_hip.h'], capture_output=True, text=True)
        if r.returncode != 0:
            return None
        if NEW[0] not in r.stdout:
            return rev
    return None


def test_existing_kernels_compile_to_the_same_isa(tmp_path):
    """tools/isa_diff.py between the two files this change touches (f32path.hip, vae.hip) as the parent commit has them and
    as they are now, compiled with the Makefile's flags: 0 changed kernels, five new ones.  Needs the git history."""
    rev = _parent_rev() if shutil.which('git') else None
    if rev is None:
        pytest.skip('no git history with the parent commit here: nothing to compare against')
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    flags = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wno-unused-result', '-shared']
    old = tmp_path / 'old'
    old.mkdir()
    ar = subprocess.run(['git', '-C', ROOT, 'archive', rev, 'maskdit_amd/csrc', 'include'], capture_output=True, check=True)
    subprocess.run(['tar', '-x', '-C', str(old)], input=ar.stdout, check=True)
    procs = []
    for tag, root in (('old', str(old)), ('new', ROOT)):
        srcs = [os.path.join(root, 'maskdit_amd', 'csrc', f) for f in ('f32path.hip', 'vae.hip')]
        procs.append(subprocess.Popen([hipcc] + flags + srcs + ['-o', str(tmp_path / f'{tag}.so')], stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    for p in procs:
        out, _ = p.communicate()
        assert p.returncode == 0, out[-3000:]
    diff = _tool('isa_diff')
    a, b = diff.kernels(str(tmp_path / 'old.so')), diff.kernels(str(tmp_path / 'new.so'))
    assert len(a) >= 10 and not set(a) - set(b), 'a kernel of the parent is gone'
    changed = [diff.demangle(k) for k in a if a[k] != b[k]]
    assert not changed, f'existing kernels changed: {changed}'
    new = sorted(diff.demangle(k).split('(')[0] for k in set(b) - set(a))
    assert new == ['f32p::conv3x3_bf16x3_kernel', 'gn_im2col_f32_kernel', 'gn_stats_fold_kernel', 'gn_stats_part_kernel',
                   'vae_enc_prologue_f32_kernel'], new
