"""Generate tests/golden/vae_f32.npz by RUNNING THE REFERENCE ITSELF in fp32 and in fp64 (like make_golden_vae_encode.py).

Runs only where the reference code base exists (MASKDIT_REFERENCE, default /root/reference; not on the GPU machines).
It imports the reference's `autoencoder.Decoder` / `autoencoder.Encoder` (ddconfig of get_model) with nn.Conv2d stand-ins
for post_quant_conv / quant_conv (FrozenAutoencoderKL.decode / encode_moments, autoencoder.py:431-453), loads the existing
synthetic weights (`oracle.vae_oracle.init_vae_params(11)`, `tests.vae_encoder_ref.init_vae_encoder_params(21)`), and runs
each side twice on the inputs of the EXISTING fixtures (`z` of vae_decode.npz, `img256` of vae_encode.npz; not stored
again): once as it is (fp32, what the reference computes) and once after `.double()`.  The fp64 run is the yardstick of
the 'bf16x3' autoencoder arithmetic; the distance of the reference's own fp32 run from it is the unit of the bounds.

  dec_e_ref        max |fp32 - fp64| / max |fp64| over both decoded images
  dec_n_u8_ref     number of uint8 values in which the fp32 and fp64 images differ after sample.py:287's quantisation
                   (add 1, mul 127.5, clamp 0..255, truncate)
  dec_lv0_crop     fp32 [3, 128, 128]: fp64 decode of image 0, centre crop, as grey levels (x + 1) * 127.5 before clamping
  dec64_img1_sub   fp64 [3, 64, 64]: fp64 decode of image 1 at stride 4
  dec_absmax64     max |fp64| over both decoded images (the denominator of dec_e_ref)
  mom64_256        fp64 [8, 32, 32]: fp64 moments of img256
  enc_e_ref        max |fp32 - fp64| / max |fp64| over the moments

    python tests/golden/make_golden_vae_f32.py      # rewrites tests/golden/vae_f32.npz
"""
import copy
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

DDCONFIG = dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 4, 4],
                num_res_blocks=2, attn_resolutions=[], dropout=0.0)
CROP0, CROP = 64, 128   # centre crop of the 256 x 256 image 0: rows / columns 64 .. 191
STRIDE = 4


def quantise(img):
    """sample.py:287 on a copy: add 1, mul 127.5, clamp to 0..255, truncate to uint8."""
    return img.clone().add_(1).mul(127.5).clamp_(0, 255).to(torch.uint8)


def _load(mod, P, prefix):
    mod.load_state_dict({k[len(prefix):]: v for k, v in P.items() if k.startswith(prefix)}, strict=True)


def main():
    import autoencoder as ref_ae  # noqa  (reference)
    from oracle import vae_oracle as VO
    from tests import vae_encoder_ref as VE

    gd = np.load(os.path.join(HERE, 'vae_decode.npz'))
    ge = np.load(os.path.join(HERE, 'vae_encode.npz'))
    out = {}

    # ---- decode: Decoder(post_quant_conv(z / scale_factor)), autoencoder.py:449-453
    P = VO.init_vae_params(seed=int(gd['seed']))
    dec, pq = ref_ae.Decoder(**DDCONFIG), torch.nn.Conv2d(4, 4, 1)
    _load(dec, P, 'decoder.')
    _load(pq, P, 'post_quant_conv.')
    dec.eval()
    z = torch.from_numpy(gd['z'])
    with torch.no_grad():
        img32 = dec(pq(z / 0.18215))
        dec64, pq64 = copy.deepcopy(dec).double(), copy.deepcopy(pq).double()
        img64 = dec64(pq64(z.double() / 0.18215))
    assert img32.dtype == torch.float32 and img64.dtype == torch.float64
    absmax = img64.abs().max().item()
    out['dec_e_ref'] = np.float64((img32.double() - img64).abs().max().item() / absmax)
    out['dec_absmax64'] = np.float64(absmax)
    q32, q64 = quantise(img32), quantise(img64)
    out['dec_n_u8_ref'] = np.int64((q32 != q64).sum().item())
    lv = (img64[0] + 1) * 127.5
    out['dec_lv0_crop'] = lv[:, CROP0:CROP0 + CROP, CROP0:CROP0 + CROP].to(torch.float32).numpy()
    out['dec64_img1_sub'] = img64[1, :, ::STRIDE, ::STRIDE].contiguous().numpy()
    step = (q32.int() - q64.int()).abs().max().item()
    print(f'decode: fp32 vs fp64 {out["dec_e_ref"]:.3e} of max ({absmax:.3f}); {int(out["dec_n_u8_ref"])} of {q32.numel()} uint8 '
          f'values differ (largest step {step})')

    # ---- encode: quant_conv(Encoder(x)), autoencoder.py:431-434
    Pe = VE.init_vae_encoder_params(int(ge['seed']))
    enc, qc = ref_ae.Encoder(**DDCONFIG), torch.nn.Conv2d(8, 8, 1)
    _load(enc, Pe, 'encoder.')
    _load(qc, Pe, 'quant_conv.')
    enc.eval()
    x = VE.u8_to_unit(ge['img256'])[None]
    with torch.no_grad():
        mom32 = qc(enc(x))
        enc64, qc64 = copy.deepcopy(enc).double(), copy.deepcopy(qc).double()
        mom64 = qc64(enc64(x.double()))
    assert float((mom32 - torch.from_numpy(ge['mom256'])[None]).abs().max()) <= 1e-5 * float(mom32.abs().max()), \
        'the fp32 run does not reproduce mom256 of vae_encode.npz'
    out['mom64_256'] = mom64[0].numpy()
    out['enc_e_ref'] = np.float64((mom32.double() - mom64).abs().max().item() / mom64.abs().max().item())
    print(f'encode: fp32 vs fp64 {out["enc_e_ref"]:.3e} of max ({mom64.abs().max().item():.3f})')

    path = os.path.join(HERE, 'vae_f32.npz')
    np.savez_compressed(path, **out)
    print(f'{path} written ({os.path.getsize(path)} bytes)')
    assert os.path.getsize(path) < 400 * 1024


if __name__ == '__main__':
    main()
