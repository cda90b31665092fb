"""Generate tests/golden/vae_encode.npz by RUNNING THE REFERENCE ITSELF (like make_golden.py).

Runs only where the reference code base exists (MASKDIT_REFERENCE, default /root/reference; not on the GPU machines).
It imports the reference's `autoencoder.Encoder` (ddconfig of get_model) with an nn.Conv2d(8, 8, 1) as quant_conv
(FrozenAutoencoderKL.encode_moments, autoencoder.py:431-434) and `train_utils.datasets.center_crop_arr` (with the
`_refshim` stand-ins for the uninstalled torchvision / lmdb), loads the weights of
`tests/vae_encoder_ref.init_vae_encoder_params(seed)` and records:

  seed, order            the seed and the reference Encoder's state-dict key order
  img256 / img128        one uint8 [R, R, 3] image per side (smooth random fields, the full 0..255 range)
  mom256 / mom128        the reference's moments of those images, [8, R/8, R/8] fp32 (ToTensor + Normalize(0.5, 0.5))
  crop{i}                center_crop_arr(., 64) of three seeded-random RGB images of awkward sizes (`vae_encoder_ref.crop_source`
                         regenerates the inputs; they are noise, too large to store)

    python tests/golden/make_golden_vae_encode.py      # rewrites tests/golden/vae_encode.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get('MASKDIT_REFERENCE', '/root/reference')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(HERE, '_refshim'))
sys.path.insert(0, REF)

torch.set_num_threads(8)

SEED = 21


def smooth_image(R, seed):
    """uint8 [R, R, 3]: a low-frequency random field (image-like statistics) spread over the full 0..255 range."""
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(1, 3, R // 16, R // 16, generator=g)
    f = torch.nn.functional.interpolate(f, size=(R, R), mode='bicubic', align_corners=False)
    f = f + 0.15 * torch.randn(1, 3, R, R, generator=g)
    f = (f - f.amin()) / (f.amax() - f.amin())
    return (f[0].permute(1, 2, 0) * 255).round().clamp(0, 255).to(torch.uint8).numpy()


def main():
    import autoencoder as ref_ae  # noqa  (reference)
    from train_utils.datasets import center_crop_arr  # noqa  (reference)
    from PIL import Image
    from maskdit_amd import autoencoder as AE
    from tests import vae_encoder_ref as VE

    ddconfig = dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 4, 4],
                    num_res_blocks=2, attn_resolutions=[], dropout=0.0)
    enc = ref_ae.Encoder(**ddconfig)
    qc = torch.nn.Conv2d(8, 8, 1)
    ref_table = [('encoder.' + k, tuple(v.shape)) for k, v in enc.state_dict().items()]
    ref_table += [('quant_conv.' + k, tuple(v.shape)) for k, v in qc.state_dict().items()]
    assert ref_table == list(VE.vae_encoder_param_shapes().items()), 'helper key / shape table differs from the reference'
    assert ref_table == [(n, tuple(s)) for n, s in AE.encoder_param_table()], 'encoder_param_table differs from the reference'
    P = VE.init_vae_encoder_params(SEED)
    enc.load_state_dict({k[len('encoder.'):]: v for k, v in P.items() if k.startswith('encoder.')}, strict=True)
    qc.load_state_dict({k[len('quant_conv.'):]: v for k, v in P.items() if k.startswith('quant_conv.')}, strict=True)
    enc.eval()
    out = dict(seed=np.int64(SEED), order=np.array([k for k, _ in ref_table]))
    for R, s in ((256, 1), (128, 2)):
        img = smooth_image(R, s)
        x = VE.u8_to_unit(img)[None]
        with torch.no_grad():
            mom = qc(enc(x))  # FrozenAutoencoderKL.encode_moments
            mine = VE.vae_encode_moments(P, x)
        err = ((mine - mom).abs().max() / mom.abs().max()).item()
        print(f'{R}^2: moments absmax {mom.abs().max().item():.3f}, mean-half std {mom[:, :4].std().item():.3f}, '
              f'logvar-half std {mom[:, 4:].std().item():.3f}; helper restatement vs reference {err:.2e} of max')
        out[f'img{R}'], out[f'mom{R}'] = img, mom[0].numpy()
    for i in range(len(VE.CROP_SIZES)):
        out[f'crop{i}'] = np.array(center_crop_arr(Image.fromarray(VE.crop_source(SEED, i)), 64))
    path = os.path.join(HERE, 'vae_encode.npz')
    np.savez_compressed(path, **out)
    print(f'{path} written ({os.path.getsize(path)} bytes)')


if __name__ == '__main__':
    main()
