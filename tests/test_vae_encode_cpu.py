"""VAE encode side without a GPU: the parameter table and opt-in loading of FrozenAutoencoderKL(encoder=True), the CPU
restatement of the reference's encode_moments against the reference-generated fixture (tests/golden/vae_encode.npz),
the host image pipeline of extract_latent.py (ImageFolder order, ADM center crop), and the argument checks of the three
encoder entries of the C ABI."""
import os

import numpy as np
import pytest
import torch

from maskdit_amd import _lib
from maskdit_amd import autoencoder as AE
from tests import vae_encoder_ref as VE


@pytest.fixture(scope='module')
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, 'vae_encode.npz'))


def test_encoder_param_table_matches_reference(fixture):
    table = AE.encoder_param_table()
    assert [n for n, _ in table] == [str(k) for k in fixture['order']]  # the reference's key order (encoder, quant_conv)
    assert {n: tuple(s) for n, s in table} == VE.vae_encoder_param_shapes()


def test_encoder_opt_in_loading():
    P = VE.init_vae_encoder_params(3)
    full = dict(P)
    full.update(AE.synthetic_state_dict(4, encoder=False))  # decoder + post_quant_conv
    vae = AE.get_model(None, encoder=True)
    missing, unexpected = vae.load_state_dict(full)
    assert not missing and not unexpected
    sd = vae.state_dict()
    assert list(sd)[:len(P)] == list(P)  # encoder.* + quant_conv.* first, in the reference's order
    assert torch.equal(sd['encoder.down.1.downsample.conv.weight'], P['encoder.down.1.downsample.conv.weight'])
    assert torch.equal(sd['quant_conv.bias'], P['quant_conv.bias'])
    for drop in ('encoder.mid.attn_1.k.bias', 'quant_conv.weight'):
        with pytest.raises(RuntimeError):
            vae.load_state_dict({k: v for k, v in full.items() if k != drop})
    with pytest.raises(RuntimeError):  # a shape that is not the reference's
        vae.load_state_dict({**full, 'encoder.conv_in.weight': torch.zeros(128, 4, 3, 3)})
    with pytest.raises(_lib.MaskDiTLibError):
        vae.encode_moments(torch.zeros(1, 3, 256, 256))  # no CPU path


def test_default_model_stays_decode_only():
    vae = AE.get_model(None)
    assert not any(n.startswith(('encoder.', 'quant_conv.')) for n in vae.state_dict())
    full = AE.synthetic_state_dict(5, encoder=True)
    missing, unexpected = vae.load_state_dict(full)  # the encoder keys are accepted and ignored
    assert not missing and not unexpected
    for fn in ('encode', 'encode_moments'):
        with pytest.raises(NotImplementedError):
            vae(torch.zeros(1, 3, 256, 256), fn)
    with pytest.raises(NotImplementedError):
        vae.encode(torch.zeros(1, 3, 256, 256))


def test_helper_restatement_matches_reference_fixture(fixture):
    P = VE.init_vae_encoder_params(int(fixture['seed']))
    for R in (128, 256):
        x = VE.u8_to_unit(fixture[f'img{R}'])[None]
        with torch.no_grad():
            got = VE.vae_encode_moments(P, x)[0]
        ref = torch.from_numpy(fixture[f'mom{R}'])
        assert got.shape == (8, R // 8, R // 8)
        err = ((got - ref).abs().max() / ref.abs().max()).item()
        assert err <= 1e-5, (R, err)


def test_center_crop_matches_reference_fixture(fixture):
    from PIL import Image
    from maskdit_amd.images import center_crop_arr
    for i in range(len(VE.CROP_SIZES)):
        src = VE.crop_source(int(fixture['seed']), i)
        got = center_crop_arr(Image.fromarray(src), 64)
        assert got.dtype == np.uint8 and got.shape == (64, 64, 3)
        assert np.array_equal(got, fixture[f'crop{i}']), i


def test_image_folder_order_and_labels(tmp_path):
    from PIL import Image
    from maskdit_amd.images import image_folder_samples, load_rgb_crop
    layout = {'n02': ['b.png', 'a.JPEG', 'sub/c.png', 'notes.txt'], 'n01': ['z.png', 'y.bmp'], 'n10': []}
    for cls, files in layout.items():
        os.makedirs(tmp_path / cls, exist_ok=True)
        for f in files:
            p = tmp_path / cls / f
            os.makedirs(p.parent, exist_ok=True)
            if f.endswith('.txt'):
                p.write_text('not an image')
            else:
                Image.fromarray(np.full((40, 50, 3), 7, np.uint8)).save(p, format='BMP' if f.endswith('bmp') else
                                                                        'JPEG' if f.endswith('JPEG') else 'PNG')
    (tmp_path / 'stray.png').write_bytes(b'')  # a file at the top level is not a class
    samples, classes = image_folder_samples(str(tmp_path))
    assert classes == ['n01', 'n02', 'n10']
    rel = [(os.path.relpath(p, tmp_path), y) for p, y in samples]
    assert rel == [('n01/y.bmp', 0), ('n01/z.png', 0), ('n02/a.JPEG', 1), ('n02/b.png', 1), ('n02/sub/c.png', 1)]
    img = load_rgb_crop(samples[0][0], 16)
    assert img.shape == (16, 16, 3) and img.dtype == np.uint8 and int(img[8, 8, 0]) == 7


def test_encoder_entry_validation_without_gpu():
    """Argument checks run before any launch (as in test_capi_cpu.py)."""
    L = _lib.lib()
    err = lambda: L.mdt_last_error()
    a = 256  # 16-byte aligned dummy addresses: nothing is dereferenced before the checks
    assert L.mdt_conv3x3_down_nhwc(None, 2, 16, 128, a, a, None, a, 128, 128, None, 0, None) != 0 and b'null operand' in err()
    assert L.mdt_conv3x3_down_nhwc(a, 2, 24, 128, a, a, None, a, 128, 128, None, 0, None) != 0 and b'power of two' in err()
    assert L.mdt_conv3x3_down_nhwc(a, 2, 16, 192, a, a, None, a, 128, 128, None, 0, None) != 0 and b'multiple of 128' in err()
    assert L.mdt_conv3x3_down_nhwc(a, 256, 16, 128, a, a, None, a, 128, 128, None, 0, None) != 0 and b'12 + 12 + 8' in err()
    assert L.mdt_conv3x3_down_nhwc(a, 64, 1024, 128, a, a, None, a, 128, 128, None, 0, None) != 0 and b'4 GB' in err()
    # (2, 16, 128): B * Ho * Ho = 128 rows, not whole 256-row tiles
    assert L.mdt_conv3x3_down_nhwc(a, 2, 16, 128, a, a, None, a, 128, 128, None, 0, None) != 0 and b'multiple of 256' in err()
    assert L.mdt_conv3x3_down_nhwc(a, 4, 16, 128, a, a, None, a, 128, 128, a, 32, None) != 0 and b'Ho * Ho % 128' in err()
    assert L.mdt_conv3x3_down_nhwc(a, 4, 32, 128, a, a, None, a, 128, 128, a, 16, None) != 0 and b'[B, 32, 2]' in err()
    assert L.mdt_conv3x3_down_nhwc(a + 8, 4, 32, 128, a, a, None, a, 128, 128, None, 0, None) != 0 and b'aligned' in err()
    assert L.mdt_vae_enc_prologue(None, 0, 0, a, 1, 256, 64, None) != 0 and b'null pointer' in err()
    assert L.mdt_vae_enc_prologue(a, 2, 0, a, 1, 256, 64, None) != 0 and b'0 or 1' in err()
    assert L.mdt_vae_enc_prologue(a, 1, 0, a, 1, 256, 24, None) != 0 and b'Kp >= 27' in err()
    assert L.mdt_vae_enc_epilogue(a, 128, None, a, a, 1, 64, None) != 0 and b'null pointer' in err()
    assert L.mdt_vae_enc_epilogue(a, 6, a, a, a, 1, 64, None) != 0 and b'ld >= 8' in err()


def test_encode_chunk_stays_in_the_conv_domain():
    for R in AE.ENC_SIDES:
        n = AE.FrozenAutoencoderKL.encode_chunk(R)
        assert n * R * R * AE.CH * 2 + 256 < (1 << 32) and n < 256 and (n * (R // 8) ** 2) % 256 == 0
    assert AE.FrozenAutoencoderKL.encode_chunk(256) == 64 and AE.FrozenAutoencoderKL.encode_chunk(512) == 32
