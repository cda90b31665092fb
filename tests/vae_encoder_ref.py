"""CPU reference of the KL-autoencoder ENCODE path (test helper only -- never imported by the product package).

Functional restatement (torch fp32) of the reference's `autoencoder.py` FrozenAutoencoderKL.encode_moments
(:431-434) = Encoder.forward (:270-304) -> quant_conv (1x1, 8 -> 8): conv_in, four down levels of two ResnetBlocks
(+ Downsample = pad (0, 1, 0, 1) + stride-2 3x3 conv on levels 0-2), mid (ResnetBlock, AttnBlock, ResnetBlock),
norm_out + swish + conv_out.  ddconfig = get_model's: ch 128, ch_mult (1, 2, 4, 4), 2 res blocks, no attention
resolutions, double_z (8 output channels).

Pinned by tests/golden/vae_encode.npz: the output of the reference's own Encoder module loaded with
`init_vae_encoder_params(seed)` (tests/golden/make_golden_vae_encode.py)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

CH, CH_MULT, NUM_RES_BLOCKS, Z_CH, IN_CH = 128, (1, 2, 4, 4), 2, 4, 3


def vae_encoder_param_shapes():
    """Encode-side state-dict keys (reference registration order) and shapes: encoder.* then quant_conv.*."""
    shapes = {}

    def conv(name, cin, cout, k):
        shapes[f'{name}.weight'] = (cout, cin, k, k)
        shapes[f'{name}.bias'] = (cout,)

    def norm(name, c):
        shapes[f'{name}.weight'] = (c,)
        shapes[f'{name}.bias'] = (c,)

    def res(name, cin, cout):  # autoencoder.py:78-115
        norm(f'{name}.norm1', cin)
        conv(f'{name}.conv1', cin, cout, 3)
        norm(f'{name}.norm2', cout)
        conv(f'{name}.conv2', cout, cout, 3)
        if cin != cout:
            conv(f'{name}.nin_shortcut', cin, cout, 1)

    conv('encoder.conv_in', IN_CH, CH, 3)
    block_in = CH
    for i_level, mult in enumerate(CH_MULT):
        for j in range(NUM_RES_BLOCKS):
            res(f'encoder.down.{i_level}.block.{j}', block_in, CH * mult)
            block_in = CH * mult
        if i_level != len(CH_MULT) - 1:
            conv(f'encoder.down.{i_level}.downsample.conv', block_in, block_in, 3)
    res('encoder.mid.block_1', block_in, block_in)
    norm('encoder.mid.attn_1.norm', block_in)
    for n in ('q', 'k', 'v', 'proj_out'):
        conv(f'encoder.mid.attn_1.{n}', block_in, block_in, 1)
    res('encoder.mid.block_2', block_in, block_in)
    norm('encoder.norm_out', block_in)
    conv('encoder.conv_out', block_in, 2 * Z_CH, 3)
    conv('quant_conv', 2 * Z_CH, 2 * Z_CH, 1)
    return shapes


def init_vae_encoder_params(seed: int = 0):
    """Deterministic synthetic weights, scaled like oracle/vae_oracle.init_vae_params: convolutions N(0, 1.6 / fan_in)
    so activations keep O(1) scale through the ~27 layers, biases N(0, 0.05), GroupNorm gamma 1 + N(0, 0.1), beta
    N(0, 0.1).  quant_conv is N(0, 1 / fan_in) so the logvar half of the moments stays inside the clamp range."""
    g = torch.Generator().manual_seed(seed)
    P = {}
    for name, shp in vae_encoder_param_shapes().items():
        if name.endswith('.weight') and len(shp) == 4:
            fan_in = shp[1] * shp[2] * shp[3]
            P[name] = torch.randn(shp, generator=g) * ((1.0 if name.startswith('quant_conv') else 1.6) / fan_in) ** 0.5
        elif '.norm' in name and name.endswith('.weight'):
            P[name] = 1.0 + 0.1 * torch.randn(shp, generator=g)
        elif '.norm' in name:
            P[name] = 0.1 * torch.randn(shp, generator=g)
        else:
            P[name] = 0.05 * torch.randn(shp, generator=g)
    return P


def _gn(x, P, name):  # Normalize: GroupNorm(32, eps 1e-6, affine)  (autoencoder.py:35-36)
    return F.group_norm(x, 32, P[name + '.weight'], P[name + '.bias'], eps=1e-6)


def _swish(x):
    return x * torch.sigmoid(x)


def _conv(x, P, name, padding=1, stride=1):
    return F.conv2d(x, P[name + '.weight'], P[name + '.bias'], stride=stride, padding=padding)


def _res(x, P, name):  # ResnetBlock (autoencoder.py:117-140), temb None, dropout 0
    h = _conv(_swish(_gn(x, P, name + '.norm1')), P, name + '.conv1')
    h = _conv(_swish(_gn(h, P, name + '.norm2')), P, name + '.conv2')
    if name + '.nin_shortcut.weight' in P:
        x = _conv(x, P, name + '.nin_shortcut', padding=0)
    return x + h


def _attn(x, P, name):  # AttnBlock (autoencoder.py:165-200)
    h = _gn(x, P, name + '.norm')
    q, k, v = (_conv(h, P, f'{name}.{n}', padding=0) for n in 'qkv')
    b, c, hh, ww = q.shape
    q = q.reshape(b, c, hh * ww).permute(0, 2, 1)
    w_ = torch.softmax(torch.bmm(q, k.reshape(b, c, hh * ww)) * c ** -0.5, dim=2)
    h = torch.bmm(v.reshape(b, c, hh * ww), w_.permute(0, 2, 1)).reshape(b, c, hh, ww)
    return x + _conv(h, P, name + '.proj_out', padding=0)


def vae_encode_moments(P, x):
    """x fp32 [B, 3, R, R] in [-1, 1] -> moments fp32 [B, 8, R/8, R/8]."""
    h = _conv(x, P, 'encoder.conv_in')
    for i_level in range(len(CH_MULT)):
        for j in range(NUM_RES_BLOCKS):
            h = _res(h, P, f'encoder.down.{i_level}.block.{j}')
        if i_level != len(CH_MULT) - 1:  # Downsample (autoencoder.py:56-75)
            h = _conv(F.pad(h, (0, 1, 0, 1)), P, f'encoder.down.{i_level}.downsample.conv', padding=0, stride=2)
    h = _res(h, P, 'encoder.mid.block_1')
    h = _attn(h, P, 'encoder.mid.attn_1')
    h = _res(h, P, 'encoder.mid.block_2')
    h = _conv(_swish(_gn(h, P, 'encoder.norm_out')), P, 'encoder.conv_out')
    return _conv(h, P, 'quant_conv', padding=0)


def u8_to_unit(img_u8):
    """uint8 HWC / BHWC -> fp32 [.., 3, H, W] in [-1, 1]: ToTensor + Normalize(0.5, 0.5) (extract_latent.py:30-33)."""
    t = torch.as_tensor(img_u8)
    t = t.permute(*range(t.dim() - 3), t.dim() - 1, t.dim() - 3, t.dim() - 2).contiguous().float()
    return (t / 255 - 0.5) / 0.5


CROP_SIZES = ((300, 200), (777, 513), (64, 1030))  # (width, height) of the center-crop fixture's inputs


def crop_source(seed, i):
    """uint8 [h, w, 3] noise image number i of CROP_SIZES (the inputs of vae_encode.npz's crop{i}, regenerated)."""
    w, h = CROP_SIZES[i]
    g = torch.Generator().manual_seed(seed + 100 + i)
    return torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).numpy()
