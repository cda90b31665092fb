"""Drop-in for the DECODE side of the reference's `autoencoder.py` (FrozenAutoencoderKL / get_model, autoencoder.py:
412-474): the latent -> image step that follows the sampler (sample.py:248,273-284).

    vae = maskdit_amd.autoencoder.get_model('assets/stable_diffusion/autoencoder_kl.pth')   # reference call, sample.py:248
    images = vae.decode(z)          # z [B, 4, 32, 32] (or 64x64) fp32 on the HIP device -> [B, 3, 8R, 8R] fp32

Parameters carry the reference's state-dict names and shapes (`decoder.mid.block_1.conv1.weight` [512, 512, 3, 3], ...),
so the published `autoencoder_kl.pth` loads with `load_state_dict` (its `encoder.*` / `quant_conv.*` entries are
accepted and ignored unless the model is built with `encoder=True`, see ENCODE side below).

Arithmetic (maskdit_amd/csrc/vae.hip + the bf16 MFMA GEMMs): activations NHWC fp32; `mdt_gn_im2col` applies GroupNorm(32,
eps 1e-6) + swish and writes the bf16 operand; every 3x3 convolution with a multiple of 128 input channels is ONE implicit
GEMM (`mdt_conv3x3_nhwc`, round 3: the MFMA kernel gathers the nine taps, the zero padding and the nearest 2x up-sampling
from the NHWC activation -- rounds 1-2 materialised an im2col matrix of 9x the activation bytes), the 1x1 convolutions and
conv_in (4 channels) are `mdt_gemm_nt` on the activation / a small im2col matrix; the mid-block attention
(1024 tokens, one head of 512 channels) is three GEMMs per image around `mdt_softmax_rows`.  No torch arithmetic, no
CPU fallback.  Supported latent sides: 16, 32, 48, 64 (decode() raises for others).  Determinism: with the fused
convolution epilogue (default) the next GroupNorm's statistics are accumulated with fp32 atomics across waves, so two decodes of
the same latents can differ in the last bits; MDT_VAE_FUSE=0 selects the separate mdt_gn_stats pass, which is run-to-run
bitwise reproducible (use it where that matters, e.g. FID bookkeeping across runs).  ddconfig is the reference's (ch 128, ch_mult (1, 2, 4, 4), 2 res blocks, no attention resolutions,
z_channels 4, 3 output channels).

ENCODE side (opt-in: `get_model(path, encoder=True)`): `encode_moments(x)` / `encode(x)` / `forward(x, fn)` of
autoencoder.py:431-463 -- image [B, 3, R, R] fp32 in [-1, 1] (or uint8 [B, R, R, 3], what extract_latent.py feeds) ->
moments [B, 8, R/8, R/8] fp32, for R = 128, 256, 512.  The Encoder (:212-304) runs on the decoder's building blocks
(GroupNorm + swish writer, implicit-GEMM 3x3 convolutions with the fused epilogue, 1x1 GEMMs, the mid-block attention)
plus three entries of its own: mdt_vae_enc_prologue (image -> conv_in's im2col, optional x mirror),
mdt_conv3x3_down_nhwc (Downsample: pad (0, 1, 0, 1) + stride-2 convolution) and mdt_vae_enc_epilogue (quant_conv ->
NCHW moments).  bf16 operands, fp32 accumulation, like decode.

PRECISION.  Everything above is `precision='bf16'`, the default.  The reference runs its autoencoder in fp32;
`get_model(path, precision='bf16x3')` / `vae.set_precision('bf16x3')` select that accuracy for decode and encode: fp32
weights and fp32 operands (mdt_gn_im2col_f32 / mdt_vae_enc_prologue_f32, exact-form GroupNorm + swish), every 3x3
convolution one implicit GEMM in the three-term split arithmetic of the sampler's 'bf16x3' plan (mdt_conv3x3_bf16x3_nhwc:
any image side, any batch), 1x1 convolutions and the two im2col convolutions on mdt_gemm_bf16x3, attention scores and P V on
the exact-fp32 mdt_gemm_f32 around mdt_softmax_rows_f32, GroupNorm sums from mdt_gn_stats_ordered (fixed summation order:
no atomics anywhere on this path, two runs give identical bits).  MDT_VAE_X3_IM2COL=1
forces the stride-1 3x3 convolutions through a materialised fp32 im2col matrix + mdt_gemm_bf16x3 instead (the comparison
route of tools/vae_bf16x3_bench.py; 9x the activation bytes, small batches only).

LAYOUT.  The topology (ResnetBlock, mid block, up / down ladders, slot ping-pong) is written once, in
FrozenAutoencoderKL._res / _decode / _encode_chunk, against the surface the two arithmetics share: `_Bf16` and `_Bf16x3`
(conv, attn, dec_in, enc_in, packed), chosen by `set_precision`."""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib, ops
from ._lib import call

CH, CH_MULT, NUM_RES_BLOCKS, Z_CH, OUT_CH, GROUPS = 128, (1, 2, 4, 4), 2, 4, 3, 32
IN_CH = 3                     # encoder input channels (RGB)
ENC_SIDES = (128, 256, 512)   # image sides encode_moments accepts
FUSE_EPILOGUE = os.environ.get('MDT_VAE_FUSE', '1') != '0'  # A/B switch (see _Bf16.conv)
# widest convolution (output channels) that takes the fused epilogue: it exists for 128-column tiles only (the 256-wide
# kernel spills with it), so for 256 / 512 channels fusing trades a ~15-20 % slower GEMM against the saved passes
PRECISIONS = ('bf16', 'bf16x3')
X3_FORCE_IM2COL = os.environ.get('MDT_VAE_X3_IM2COL', '0') == '1'  # A/B switch of the 'bf16x3' arithmetic (see _Bf16x3.conv)
X3_ZLINE = 32  # floats of zeros in front of every fp32 workspace buffer: the padding taps of mdt_conv3x3_bf16x3_nhwc read them
FUSE_MAX_COUT = int(os.environ.get('MDT_VAE_FUSE_MAXC', '256'))  # measured at batch 64: 128 -> 62.4 ms, 256 -> 61.7, 512 -> 64.4, off -> 67.4


class _ParamTable(list):
    """(state-dict key, shape) entries, appended in the reference's registration order"""

    def conv(self, name, cin, cout, k):
        self.extend([(f'{name}.weight', (cout, cin, k, k)), (f'{name}.bias', (cout,))])

    def norm(self, name, c):
        self.extend([(f'{name}.weight', (c,)), (f'{name}.bias', (c,))])

    def res(self, name, cin, cout):
        self.norm(f'{name}.norm1', cin)
        self.conv(f'{name}.conv1', cin, cout, 3)
        self.norm(f'{name}.norm2', cout)
        self.conv(f'{name}.conv2', cout, cout, 3)
        if cin != cout:
            self.conv(f'{name}.nin_shortcut', cin, cout, 1)


def decoder_param_table() -> List[Tuple[str, tuple]]:
    """(state-dict key, shape) of post_quant_conv + decoder, in the reference's registration order
    (autoencoder.py:306-372, 419)."""
    t = _ParamTable()
    block_in = CH * CH_MULT[-1]
    t.conv('decoder.conv_in', Z_CH, block_in, 3)
    t.res('decoder.mid.block_1', block_in, block_in)
    t.norm('decoder.mid.attn_1.norm', block_in)
    for n in ('q', 'k', 'v', 'proj_out'):
        t.conv(f'decoder.mid.attn_1.{n}', block_in, block_in, 1)
    t.res('decoder.mid.block_2', block_in, block_in)
    ups: Dict[int, _ParamTable] = {}
    for i_level in reversed(range(len(CH_MULT))):  # built top level first, stored under up.{i_level}
        up = ups[i_level] = _ParamTable()
        block_out = CH * CH_MULT[i_level]
        for j in range(NUM_RES_BLOCKS + 1):
            up.res(f'decoder.up.{i_level}.block.{j}', block_in, block_out)
            block_in = block_out
        if i_level != 0:
            up.conv(f'decoder.up.{i_level}.upsample.conv', block_in, block_in, 3)
    for i_level in range(len(CH_MULT)):  # `self.up.insert(0, up)`: module order is up.0 .. up.3
        t.extend(ups[i_level])
    t.norm('decoder.norm_out', block_in)
    t.conv('decoder.conv_out', block_in, OUT_CH, 3)
    return [('post_quant_conv.weight', (Z_CH, Z_CH, 1, 1)), ('post_quant_conv.bias', (Z_CH,))] + t


def encoder_param_table() -> List[Tuple[str, tuple]]:
    """(state-dict key, shape) of encoder + quant_conv, in the reference's registration order (autoencoder.py:212-284,
    417-418; double_z: conv_out and quant_conv carry 2 * z_channels = 8 channels)."""
    t = _ParamTable()
    t.conv('encoder.conv_in', IN_CH, CH, 3)
    block_in = CH
    for i_level in range(len(CH_MULT)):
        block_out = CH * CH_MULT[i_level]
        for j in range(NUM_RES_BLOCKS):
            t.res(f'encoder.down.{i_level}.block.{j}', block_in, block_out)
            block_in = block_out
        if i_level != len(CH_MULT) - 1:
            t.conv(f'encoder.down.{i_level}.downsample.conv', block_in, block_in, 3)
    t.res('encoder.mid.block_1', block_in, block_in)
    t.norm('encoder.mid.attn_1.norm', block_in)
    for n in ('q', 'k', 'v', 'proj_out'):
        t.conv(f'encoder.mid.attn_1.{n}', block_in, block_in, 1)
    t.res('encoder.mid.block_2', block_in, block_in)
    t.norm('encoder.norm_out', block_in)
    t.conv('encoder.conv_out', block_in, 2 * Z_CH, 3)
    t.conv('quant_conv', 2 * Z_CH, 2 * Z_CH, 1)
    return list(t)


def _rup(x, m):
    return (x + m - 1) // m * m


def _conv_matrices(model):
    """(name, weight [Cout, Cin, k, k] as the matrix [Cout, k * k * Cin] with K ordered (ky, kx, cin) like the im2col rows,
    bias) of every convolution of `model`"""
    W = dict(model.named_weights())
    for name, p in W.items():
        if name.endswith('.weight') and p.dim() == 4:
            base = name[:-len('.weight')]
            yield base, p.detach().permute(0, 2, 3, 1).reshape(p.shape[0], -1), W[base + '.bias'].detach()


def _fold_v_bias(model, pk, dtype):
    """The attention value bias folded into the output projection's (softmax rows sum to 1: P (h Wv^T + 1 bv^T) =
    P h Wv^T + 1 bv^T), computed in `dtype`; pk: name -> (matrix, bias, K, N)."""
    W = dict(model.named_weights())
    for a in ('decoder.mid.attn_1', 'encoder.mid.attn_1') if model.has_encoder else ('decoder.mid.attn_1',):
        wp = W[a + '.proj_out.weight'].detach().reshape(W[a + '.proj_out.weight'].shape[0], -1).to(dtype)
        beff = W[a + '.proj_out.bias'].detach().to(dtype) + wp @ W[a + '.v.bias'].detach().to(dtype)
        m, _, K, N = pk[a + '.proj_out']
        pk[a + '.proj_out'] = (m, beff.to(torch.float32).contiguous(), K, N)


class _Bf16:
    """The default arithmetic (module docstring): bf16 operands, fp32 accumulation.  Workspace keys `out_*`, `sum_*`,
    `sums*`, `col`, `act`, `attn_*`; weight images in `model._packed`."""

    def __init__(self, model):
        self.m = model

    def packed(self):
        """conv weight [Cout, Cin, k, k] -> bf16 [Np, Kp] with K ordered (ky, kx, cin) like the im2col rows, N padded
        to 128 and K to 64; biases fp32 [Np]; the value-bias fold in fp32.  Built on first use, dropped by `_apply`."""
        m = self.m
        if m._packed is None:
            dev = next(m.parameters()).device
            pk = {}
            m._cout = {}
            for base, w, bias in _conv_matrices(m):
                cout, K = w.shape
                Kp, Np = _rup(K, 64), _rup(cout, 128)
                wm = torch.zeros(Np, Kp, device=dev, dtype=torch.float32)
                wm[:cout, :K] = w
                b = torch.zeros(Np, device=dev, dtype=torch.float32)
                b[:cout] = bias
                pk[base] = (wm.to(torch.bfloat16).contiguous(), b, Kp, Np)
                m._cout[base] = cout
            _fold_v_bias(m, pk, torch.float32)
            m._packed = pk
        return m._packed

    def dec_in(self, z, B, R):
        m = self.m
        W = m._weights()
        x = m._buf('x0', (B * R * R, Z_CH), torch.float32)
        call('mdt_vae_prologue', z.data_ptr(), W['post_quant_conv.weight'].data_ptr(), W['post_quant_conv.bias'].data_ptr(),
             x.data_ptr(), B, R * R, float(m.scale_factor), ops.stream_ptr())
        return x

    def enc_in(self, x, u8, flip, B, R):
        m = self.m
        wmat, bias, Kp, Np = m._packed['encoder.conv_in']
        col = m._buf('col', (B * R * R, Kp), torch.bfloat16)
        call('mdt_vae_enc_prologue', x.data_ptr(), int(u8), int(bool(flip)), col.data_ptr(), B, R, Kp, ops.stream_ptr())
        h = m._buf('out_x1', (B * R * R, Np), torch.float32)
        ops.gemm_nt(col, wmat, bias, ops.EPI_F32, outf=h)
        return h

    def conv(self, x, B, H, cin, name, k=3, norm=None, swish=False, up=0, down=0, slot='a', in_stats=None, res=None,
             want_stats=False):
        """x: fp32 [B*H*H, cin] (NHWC) -> (fp32 [B*Ho*Ho, Np], stats).  `down`: the encoder's Downsample (pad (0, 1, 0, 1),
        stride 2, Ho = H / 2; implicit-GEMM form only).  `in_stats`: GroupNorm sums of x that the
        PRODUCER of x already accumulated (round 4: the implicit-GEMM convolution's epilogue), else mdt_gn_stats runs;
        `res`: fp32 [B*Ho*Ho, Np] added to the result inside the epilogue where the implicit-GEMM kernel runs (else by
        mdt_add_f32); `want_stats`: return the sums [B, 32, 2] of the result when the epilogue can produce them."""
        m = self.m
        st = ops.stream_ptr()
        W = m._weights()
        wmat, bias, Kp, Np = m._packed[name]
        sums = gamma = beta = None
        if norm is not None:
            sums = in_stats
            if sums is None:
                sums = m._buf('sums', (B, GROUPS, 2), torch.float32)
                call('mdt_gn_stats', x.data_ptr(), sums.data_ptr(), B, H * H, cin, GROUPS, st)
            gamma, beta = W[norm + '.weight'], W[norm + '.bias']
        Ho = H >> 1 if down else H << up
        M = B * Ho * Ho
        # the implicit-GEMM kernel's shape domain (mdt_conv3x3_nhwc): power-of-two image sides >= 8, whole 256-row tiles,
        # 8-bit batch index, 32-bit source offsets; anything else inside decode()'s domain (R = 48 latents: 48, 96, 192, 384
        # pixel sides; a batch whose pixel rows are not whole 256-row tiles) takes the materialised-im2col GEMM below, which has
        # no shape restriction of its own.  decode() itself accepts R = 16, 32, 48, 64 only (the mid-block attention's T x T
        # GEMMs need R * R % 128 == 0): R = 8 / 24 / 40 raise NotImplementedError there -- the reference decoder is
        # size-agnostic, this one covers the sides the shipped configs (32, 64) and their neighbours use
        implicit_ok = (k == 3 and cin % 128 == 0 and H >= 8 and (H & (H - 1)) == 0 and M % 256 == 0 and B < 256
                       and Ho <= 2048 and B * H * H * cin * 2 + 256 < (1 << 32))
        if down and not implicit_ok:
            raise NotImplementedError(f'maskdit_amd.autoencoder: stride-2 convolution outside the implicit-GEMM domain '
                                      f'(B {B}, H {H}, C {cin}): encode_moments chunks the batch to stay inside it')
        if implicit_ok:
            # implicit GEMM (round 3): the normalised activation is written ONCE as bf16 NHWC (ksize-1 form of
            # mdt_gn_im2col) behind a 256-byte zero line, the MFMA kernel gathers the nine taps (and the 2x up-sampling)
            # itself -- no im2col matrix (9x the activation bytes per convolution in rounds 1-2)
            act = m._buf('act', (B * H * H * cin,), torch.bfloat16, zline=128)
            call('mdt_gn_im2col', x.data_ptr(), sums.data_ptr() if sums is not None else None,
                 gamma.data_ptr() if gamma is not None else None, beta.data_ptr() if beta is not None else None, act.data_ptr(),
                 B, H, H, cin, GROUPS, 1, 0, int(swish), cin, st)
            out = m._buf('out_' + slot, (M, Np), torch.float32)
            # round 4: the skip connection and the NEXT GroupNorm's statistics come out of the epilogue (128-column tiles;
            # MDT_VAE_FUSE=0 = the round-3 form: 256-column tiles where they divide, separate add / statistics passes)
            cout = m._cout[name]
            cpg = cout // GROUPS if cout % GROUPS == 0 else 0
            stats = None
            fuse = FUSE_EPILOGUE and cout <= FUSE_MAX_COUT
            if fuse and want_stats and cout == Np and cpg >= 4 and (cpg & (cpg - 1)) == 0 and (Ho * Ho) % 128 == 0:
                stats = m._buf('sums_' + slot, (B, GROUPS, 2), torch.float32)
                stats.zero_()
            fres = res if fuse else None
            if down:
                call('mdt_conv3x3_down_nhwc', act.data_ptr(), B, H, cin, wmat.data_ptr(), bias.data_ptr(),
                     fres.data_ptr() if fres is not None else None, out.data_ptr(), Np, Np,
                     stats.data_ptr() if stats is not None else None, GROUPS, st)
            else:
                call('mdt_conv3x3_nhwc', act.data_ptr(), B, H, cin, up, wmat.data_ptr(), bias.data_ptr(),
                     fres.data_ptr() if fres is not None else None, out.data_ptr(), Np, Np,
                     stats.data_ptr() if stats is not None else None, GROUPS, st)
            if res is not None and fres is None:
                out = self._add(res, out, slot)
            return out, stats
        col = m._buf('col', (M, Kp), torch.bfloat16)
        call('mdt_gn_im2col', x.data_ptr(), sums.data_ptr() if sums is not None else None,
             gamma.data_ptr() if gamma is not None else None, beta.data_ptr() if beta is not None else None, col.data_ptr(),
             B, H, H, cin, GROUPS, k, up, int(swish), Kp, st)
        out = m._buf('out_' + slot, (M, Np), torch.float32)
        ops.gemm_nt(col, wmat, bias, ops.EPI_F32, outf=out)
        if res is not None:
            out = self._add(res, out, slot)
        return out, None

    def _add(self, a, b, slot):
        c = self.m._buf('sum_' + slot, tuple(a.shape), torch.float32)
        call('mdt_add_f32', a.data_ptr(), b.data_ptr(), c.data_ptr(), a.numel(), ops.stream_ptr())
        return c

    def attn(self, x, B, H, c, name, slot):
        m = self.m
        st = ops.stream_ptr()
        W = m._weights()
        T = H * H
        sums = m._buf('sums', (B, GROUPS, 2), torch.float32)
        call('mdt_gn_stats', x.data_ptr(), sums.data_ptr(), B, T, c, GROUPS, st)
        hn = m._buf('attn_hn', (B * T, c), torch.bfloat16)
        call('mdt_gn_im2col', x.data_ptr(), sums.data_ptr(), W[name + '.norm.weight'].data_ptr(), W[name + '.norm.bias'].data_ptr(),
             hn.data_ptr(), B, H, H, c, GROUPS, 1, 0, 0, c, st)
        q = m._buf('attn_q', (B * T, c), torch.bfloat16)
        k = m._buf('attn_k', (B * T, c), torch.bfloat16)
        ops.gemm_nt(hn, m._packed[name + '.q'][0], m._packed[name + '.q'][1], ops.EPI_BF16, out=q)
        ops.gemm_nt(hn, m._packed[name + '.k'][0], m._packed[name + '.k'][1], ops.EPI_BF16, out=k)
        wv = m._packed[name + '.v'][0]
        o = m._buf('attn_o', (B * T, c), torch.bfloat16)
        vT = m._buf('attn_vT', (c, T), torch.bfloat16)
        S = m._buf('attn_S', (T, T), torch.float32)
        P = m._buf('attn_P', (T, T), torch.bfloat16)
        for b in range(B):
            rows = slice(b * T, (b + 1) * T)
            ops.gemm_nt(wv, hn[rows], None, ops.EPI_BF16, out=vT)               # v^T = Wv h^T  (bias folded into proj_out)
            ops.gemm_nt(q[rows], k[rows], None, ops.EPI_F32, outf=S)             # w_[i, j] = q_i . k_j   (autoencoder.py:186)
            call('mdt_softmax_rows', S.data_ptr(), P.data_ptr(), T, T, float(c) ** -0.5, st)  # :187-188
            ops.gemm_nt(P, vT, None, ops.EPI_BF16, out=o[rows])                  # h_[i, :] = sum_j P[i, j] v_j   (:191-193)
        wp, bp, _, _ = m._packed[name + '.proj_out']
        proj = m._buf('out_a', (B * T, c), torch.float32)
        ops.gemm_nt(o, wp, bp, ops.EPI_F32, outf=proj)
        return self._add(x, proj, slot)


class _Bf16x3:
    """The fp32-accurate arithmetic (module docstring, PRECISION).  Workspace keys `x3_*`, every buffer behind X3_ZLINE zero
    floats so that any activation can be the `act` argument of mdt_conv3x3_bf16x3_nhwc as it is; weight images in
    `model._packed_x3`."""

    def __init__(self, model):
        self.m = model

    def packed(self):
        """conv weight [Cout, Cin, k, k] -> fp32 [Cout, K], K ordered (ky, kx, cin) and zero-padded to a multiple of 4 (the
        encoder's conv_in: 27 -> 28); no padding of Cout; the value-bias fold in fp64, rounded once.  Built when 'bf16x3' is
        first used, dropped by `_apply`."""
        m = self.m
        if m._packed_x3 is None:
            pk = {}
            for base, w, bias in _conv_matrices(m):
                cout, K = w.shape
                wm = torch.zeros(cout, _rup(K, 4), device=w.device, dtype=torch.float32)
                wm[:, :K] = w
                pk[base] = (wm, bias.to(torch.float32).contiguous(), wm.shape[1], cout)
            _fold_v_bias(m, pk, torch.float64)
            m._packed_x3 = pk
        return m._packed_x3

    def _buf(self, key, shape):
        return self.m._buf(key, shape, torch.float32, zline=X3_ZLINE)

    def _sums(self, x, B, HW, c):
        """GroupNorm sums [B, 32, 2] of x in a fixed summation order (mdt_gn_stats_ordered; mdt_gn_stats combines its pixel
        chunks with atomics, which made two decodes differ in the last bits)"""
        sums = self._buf('x3_sums', (B, GROUPS, 2))
        ws = self._buf('x3_sums_ws', (int(_lib.lib().mdt_gn_stats_ordered_ws_floats(B, GROUPS)),))
        call('mdt_gn_stats_ordered', x.data_ptr(), sums.data_ptr(), ws.data_ptr(), B, HW, c, GROUPS, ops.stream_ptr())
        return sums

    def dec_in(self, z, B, R):
        m = self.m
        W = m._weights()
        x = self._buf('x3_x0', (B * R * R, Z_CH))
        call('mdt_vae_prologue', z.data_ptr(), W['post_quant_conv.weight'].data_ptr(), W['post_quant_conv.bias'].data_ptr(),
             x.data_ptr(), B, R * R, float(m.scale_factor), ops.stream_ptr())
        return x

    def enc_in(self, x, u8, flip, B, R):
        wmat, bias, K, cout = self.m._packed_x3['encoder.conv_in']
        col = self._buf('x3_col', (B * R * R, K))
        call('mdt_vae_enc_prologue_f32', x.data_ptr(), int(u8), int(bool(flip)), col.data_ptr(), B, R, K, ops.stream_ptr())
        h = self._buf('x3_out_x1', (B * R * R, cout))
        ops.gemm_bf16x3(col, wmat, h, B * R * R, cout, K, bias=bias)
        return h

    def conv(self, x, B, H, cin, name, k=3, norm=None, swish=False, up=0, down=0, slot='a', in_stats=None, res=None,
             want_stats=False):
        """x: fp32 [B*H*H, cin] (NHWC, from `_buf`) -> (fp32 [B*Ho*Ho, ldo], None), ldo = Cout rounded up to 4; `res` (same
        shape) is added in the epilogue.  `in_stats` / `want_stats` are ignored: the sums always come from mdt_gn_stats_ordered.
        3x3 with cin % 32 == 0: the implicit GEMM, on x itself where there is no GroupNorm / swish in
        front; conv_in (4 / 3 input channels) and, under MDT_VAE_X3_IM2COL=1, every stride-1 3x3: materialised im2col +
        mdt_gemm_bf16x3 (the stride-2 Downsample has no im2col writer and stays implicit); 1x1: mdt_gemm_bf16x3."""
        st = ops.stream_ptr()
        wmat, bias, K, cout = self.m._packed_x3[name]
        Ho = H >> 1 if down else H << up
        M = B * Ho * Ho
        ldo = _rup(cout, 4)
        assert res is None or tuple(res.shape) == (M, ldo)
        out = self._buf('x3_out_' + slot, (M, ldo))
        sums = gamma = beta = None
        if norm is not None:
            sums = self._sums(x, B, H * H, cin)
            W = self.m._weights()
            gamma, beta = W[norm + '.weight'], W[norm + '.bias']

        def write(dst, ksize, upv, Kp):
            call('mdt_gn_im2col_f32', x.data_ptr(), sums.data_ptr() if sums is not None else None,
                 gamma.data_ptr() if gamma is not None else None, beta.data_ptr() if beta is not None else None, dst.data_ptr(),
                 B, H, H, cin, GROUPS, ksize, upv, int(swish), Kp, st)

        pointwise = norm is not None or swish
        if k == 3 and cin % 32 == 0 and (down or not X3_FORCE_IM2COL):
            act = x
            if pointwise:
                act = self._buf('x3_act', (B * H * H, cin))
                write(act, 1, 0, cin)
            call('mdt_conv3x3_bf16x3_nhwc', act.data_ptr(), B, H, cin, up, down, wmat.data_ptr(), bias.data_ptr(),
                 res.data_ptr() if res is not None else None, out.data_ptr(), ldo, cout, st)
            return out, None
        if k == 3:
            a = self._buf('x3_col', (M, K))
            write(a, 3, up, K)
        elif pointwise:
            a = self._buf('x3_act', (M, cin))
            write(a, 1, 0, cin)
        else:
            a = x
        ops.gemm_bf16x3(a, wmat, out, M, cout, K, lda=K, ldb=K, ldo=ldo, bias=bias,
                        epi=ops.F32EPI_GATE_RES if res is not None else ops.F32EPI_NONE, res=res, rows_per_sample=1)
        return out, None

    def attn(self, x, B, H, c, name, slot):
        """AttnBlock (autoencoder.py:165-200): q / k / v / proj_out on mdt_gemm_bf16x3, scores and P V in exact fp32, batched
        over as many images as keep the score buffer within 256 MiB."""
        st = ops.stream_ptr()
        W = self.m._weights()
        pk = self.m._packed_x3
        T = H * H
        sums = self._sums(x, B, T, c)
        hn = self._buf('x3_act', (B * T, c))
        call('mdt_gn_im2col_f32', x.data_ptr(), sums.data_ptr(), W[name + '.norm.weight'].data_ptr(), W[name + '.norm.bias'].data_ptr(),
             hn.data_ptr(), B, H, H, c, GROUPS, 1, 0, 0, c, st)
        qkv = []
        for n in 'qkv':
            wmat, bias, K, cout = pk[f'{name}.{n}']
            t = self._buf('x3_attn_' + n, (B * T, c))
            ops.gemm_bf16x3(hn, wmat, t, B * T, c, c, bias=None if n == 'v' else bias)  # (v bias folded into proj_out's)
            qkv.append(t)
        q, k, v = qkv
        o = self._buf('x3_attn_o', (B * T, c))
        nb = max(1, min(B, (1 << 26) // (T * T)))
        S = self._buf('x3_attn_S', (nb * T, T))
        for b0 in range(0, B, nb):
            n = min(nb, B - b0)
            off = b0 * T * c
            ops.gemm_f32(q, k, S, T, T, c, lda=c, ldb=c, ldo=T, batch=n, heads=1, a_strides=(T * c, 0), b_strides=(T * c, 0),
                         o_strides=(T * T, 0), a_off=off, b_off=off)                       # w_[i, j] = q_i . k_j   (:186)
            call('mdt_softmax_rows_f32', S.data_ptr(), n * T, T, T, float(c) ** -0.5, st)  # :187-188
            ops.gemm_f32(S, v, o, T, c, T, lda=T, ldb=c, ldo=c, b_kmajor=True, batch=n, heads=1, a_strides=(T * T, 0),
                         b_strides=(T * c, 0), o_strides=(T * c, 0), b_off=off, o_off=off)  # h_[i, :] = sum_j P[i, j] v_j
        wp, bp, _, _ = pk[name + '.proj_out']
        out = self._buf('x3_out_' + slot, (B * T, c))
        ops.gemm_bf16x3(o, wp, out, B * T, c, c, bias=bp, epi=ops.F32EPI_GATE_RES, res=x, rows_per_sample=1)
        return out


class FrozenAutoencoderKL(nn.Module):
    """Counterpart of autoencoder.py:412-466: decode-only by default; `encoder=True` adds the encoder + quant_conv
    weights (all of autoencoder_kl.pth, loaded strictly) and the encode side.  The network is written once (`_res`,
    `_decode`, `_encode_chunk`) against the arithmetic `set_precision` chose (`_Bf16` / `_Bf16x3`)."""

    def __init__(self, pretrained_path: Optional[str] = None, scale_factor: float = 0.18215, encoder: bool = False,
                 precision: str = 'bf16'):
        super().__init__()
        self._packed_x3: Optional[dict] = None
        self.set_precision(precision)
        self.scale_factor = scale_factor
        self.embed_dim = Z_CH
        self.has_encoder = bool(encoder)
        self._names: List[str] = []
        for name, shp in (encoder_param_table() if encoder else []) + decoder_param_table():
            p = nn.Parameter(torch.zeros(shp), requires_grad=False)
            self.register_parameter(name.replace('.', '__'), p)  # flat registration, reference names restored below
            self._names.append(name)
        self._packed: Optional[dict] = None
        self._wdict: Optional[dict] = None
        self._ws: Dict[tuple, torch.Tensor] = {}
        if pretrained_path is not None:
            sd = torch.load(pretrained_path, map_location='cpu')
            self.load_state_dict(sd)
        self.eval()

    def set_precision(self, precision: str):
        """'bf16' (default): bf16 operands, fp32 accumulation.  'bf16x3': the reference's fp32 accuracy (module docstring)."""
        if precision not in PRECISIONS:
            raise ValueError(f'maskdit_amd.autoencoder: precision {precision!r} is not one of {PRECISIONS}')
        self.precision = precision
        self._arith = _Bf16x3(self) if precision == 'bf16x3' else _Bf16(self)
        return self

    # ---- state dict under the reference's dotted names ------------------------------------
    def named_weights(self):
        for name in self._names:
            yield name, getattr(self, name.replace('.', '__'))

    def state_dict(self, *a, **k):
        return {name: p.detach() for name, p in self.named_weights()}

    def load_state_dict(self, sd, strict: bool = True):
        """Accepts the full reference checkpoint: without the encoder, `encoder.*` / `quant_conv.*` are not part of the
        decode path and are skipped; every key of the model must be present (strict) with the reference shape."""
        own = dict(self.named_weights())
        missing = [k for k in own if k not in sd]
        skip = () if self.has_encoder else ('encoder.', 'quant_conv.')
        unexpected = [k for k in sd if k not in own and not (skip and k.startswith(skip))]
        if strict and (missing or unexpected):
            raise RuntimeError(f'autoencoder state dict: missing {missing[:4]}... unexpected {unexpected[:4]}...')
        with torch.no_grad():
            for k, p in own.items():
                if k in sd:
                    if tuple(sd[k].shape) != tuple(p.shape):
                        raise RuntimeError(f'{k}: shape {tuple(sd[k].shape)} != {tuple(p.shape)}')
                    p.copy_(sd[k])
        self._packed = None
        self._packed_x3 = None
        return missing, unexpected

    def _apply(self, fn, *a, **k):
        self._packed = None
        self._packed_x3 = None
        self._wdict = None
        self._ws.clear()
        return super()._apply(fn, *a, **k)

    def _weights(self):
        """name -> parameter, built once per device binding (round 2 rebuilt this dict for every convolution)"""
        if self._wdict is None:
            self._wdict = dict(self.named_weights())
        return self._wdict

    def _buf(self, key, shape, dtype, zline=0):
        """View `shape` of workspace buffer `key`, which starts with `zline` zero elements in front of the view: written when
        the buffer is allocated or grows, and no kernel stores in front of its output.  The padding taps of the implicit-GEMM
        convolutions read them."""
        n = 1
        for s in shape:
            n *= s
        t = self._ws.get(key)
        if t is None or t.numel() < zline + n or t.dtype != dtype:
            t = torch.empty(zline + n, device=next(self.parameters()).device, dtype=dtype)
            if zline:
                t[:zline].zero_()
            self._ws[key] = t
        return t[zline:zline + n].view(shape)

    # ---- the network, once for both arithmetics ------------------------------------------------
    def _res(self, x, B, H, cin, cout, name, slot, x_stats=None):
        """ResnetBlock (autoencoder.py:78-140): x + conv2(swish(norm2(conv1(swish(norm1(x)))))) (1x1 shortcut where the widths
        differ) -> (out, GroupNorm sums of out or None).  The add and both statistics ride on the convolutions' epilogues."""
        conv = self._arith.conv
        h, h_stats = conv(x, B, H, cin, name + '.conv1', norm=name + '.norm1', swish=True, slot='h1', in_stats=x_stats,
                          want_stats=True)
        if cin != cout:
            x, _ = conv(x, B, H, cin, name + '.nin_shortcut', k=1, slot='sc')
        return conv(h, B, H, cout, name + '.conv2', norm=name + '.norm2', swish=True, slot=slot, in_stats=h_stats, res=x,
                    want_stats=True)

    def _decode(self, z, B, R):
        a = self._arith
        a.packed()
        x = a.dec_in(z, B, R)
        c = CH * CH_MULT[-1]
        H = R
        x, xs = a.conv(x, B, H, Z_CH, 'decoder.conv_in', slot='x1')
        x, xs = self._res(x, B, H, c, c, 'decoder.mid.block_1', 'p', xs)
        x = a.attn(x, B, H, c, 'decoder.mid.attn_1', 'q')
        x, xs = self._res(x, B, H, c, c, 'decoder.mid.block_2', 'p')
        flip = 1  # block_2 left x in slot 'p': the first block of the ladder writes slot 'q'
        for i_level in reversed(range(len(CH_MULT))):
            cout = CH * CH_MULT[i_level]
            for j in range(NUM_RES_BLOCKS + 1):
                x, xs = self._res(x, B, H, c, cout, f'decoder.up.{i_level}.block.{j}', 'pq'[flip], xs)
                flip ^= 1
                c = cout
            if i_level != 0:
                x, xs = a.conv(x, B, H, c, f'decoder.up.{i_level}.upsample.conv', up=1, slot='u', want_stats=True)
                H *= 2
        y, _ = a.conv(x, B, H, c, 'decoder.conv_out', norm='decoder.norm_out', swish=True, slot='a', in_stats=xs)
        img = torch.empty(B, OUT_CH, H, H, device=z.device, dtype=torch.float32)
        call('mdt_vae_epilogue', y.data_ptr(), y.shape[1], img.data_ptr(), B, H * H, OUT_CH, ops.stream_ptr())
        return img

    def _encode_chunk(self, x, u8, flip, mom):
        a = self._arith
        W = self._weights()
        B = x.shape[0]
        R = x.shape[1] if u8 else x.shape[2]
        h = a.enc_in(x, u8, flip, B, R)
        H, c, xs, sl = R, CH, None, 0
        for i_level in range(len(CH_MULT)):
            cout = CH * CH_MULT[i_level]
            for j in range(NUM_RES_BLOCKS):
                h, xs = self._res(h, B, H, c, cout, f'encoder.down.{i_level}.block.{j}', 'pq'[sl], xs)
                sl ^= 1
                c = cout
            if i_level != len(CH_MULT) - 1:
                h, xs = a.conv(h, B, H, c, f'encoder.down.{i_level}.downsample.conv', down=1, slot='u', want_stats=True)
                H //= 2
        h, _ = self._res(h, B, H, c, c, 'encoder.mid.block_1', 'pq'[sl], xs)
        h = a.attn(h, B, H, c, 'encoder.mid.attn_1', 'pq'[sl ^ 1])
        h, xs = self._res(h, B, H, c, c, 'encoder.mid.block_2', 'pq'[sl])
        y, _ = a.conv(h, B, H, c, 'encoder.conv_out', norm='encoder.norm_out', swish=True, slot='a', in_stats=xs)
        call('mdt_vae_enc_epilogue', y.data_ptr(), y.shape[1], W['quant_conv.weight'].data_ptr(), W['quant_conv.bias'].data_ptr(),
             mom.data_ptr(), B, H * H, ops.stream_ptr())

    # ---- public surface -----------------------------------------------------------------------
    @torch.no_grad()
    def decode(self, z: torch.Tensor) -> torch.Tensor:
        """autoencoder.py:449-453: z / scale_factor -> post_quant_conv -> Decoder -> image [B, 3, 8R, 8R] fp32."""
        if not z.is_cuda:
            raise _lib.MaskDiTLibError('maskdit_amd.autoencoder: z is not on a HIP device; there is no CPU path')
        if next(self.parameters()).device != z.device:
            raise _lib.MaskDiTLibError('maskdit_amd.autoencoder: call .to(z.device) first')
        z = z.to(torch.float32).contiguous()
        B, C, R, R2 = z.shape
        assert C == Z_CH and R == R2 and R % 8 == 0, f'latent shape {tuple(z.shape)}'
        if (R * R) % 128 or R * R > 4096:
            # the mid-block attention runs its T x T score GEMMs through mdt_gemm_nt (N % 128) and mdt_softmax_rows
            # (<= 4096 keys): R = 16, 32, 48, 64 (128 .. 512 px images; the shipped configs use 32 and 64)
            raise NotImplementedError(f'maskdit_amd.autoencoder: latent side {R} unsupported (R * R must be a multiple of 128, <= 4096)')
        return self._decode(z, B, R)

    @staticmethod
    def encode_chunk(R: int) -> int:
        """Images per launch sequence of encode_moments: the largest power of two <= 64 that keeps the widest activation
        (R x R x 128 bf16 per image) inside the implicit-GEMM convolution's 32-bit source offsets (512^2: 32)."""
        n = 64
        while n > 1 and n * R * R * CH * 2 + 256 >= (1 << 32):
            n //= 2
        return n

    @torch.no_grad()
    def encode_moments(self, x: torch.Tensor, flip: bool = False) -> torch.Tensor:
        """autoencoder.py:431-434: Encoder -> quant_conv.  x: fp32 [B, 3, R, R] in [-1, 1] (the reference's argument), or
        uint8 [B, R, R, 3] (an RGB batch as PIL decodes it; ToTensor + Normalize(0.5, 0.5) applied in the prologue).
        flip: mirror the images in x first (extract_latent.py --xflip).  -> moments fp32 [B, 8, R/8, R/8]."""
        if not self.has_encoder:
            raise NotImplementedError('maskdit_amd.autoencoder: this model was built without the encoder '
                                      '(get_model(path, encoder=True) loads it)')
        if not x.is_cuda:
            raise _lib.MaskDiTLibError('maskdit_amd.autoencoder: x is not on a HIP device; there is no CPU path')
        if next(self.parameters()).device != x.device:
            raise _lib.MaskDiTLibError('maskdit_amd.autoencoder: call .to(x.device) first')
        u8 = x.dtype == torch.uint8
        if u8:
            assert x.dim() == 4 and x.shape[3] == IN_CH, f'uint8 images are [B, R, R, 3], got {tuple(x.shape)}'
            B, R, R2 = x.shape[:3]
        else:
            assert x.dim() == 4 and x.shape[1] == IN_CH, f'images are [B, 3, R, R], got {tuple(x.shape)}'
            B, R, R2 = x.shape[0], x.shape[2], x.shape[3]
            x = x.to(torch.float32)
        if R != R2 or R not in ENC_SIDES:
            # the mid-block attention runs on (R/8)^2 tokens (softmax rows <= 4096: R <= 512) and every convolution is an
            # implicit GEMM on power-of-two sides; 384 (and any other side) is outside what this encoder covers
            raise NotImplementedError(f'maskdit_amd.autoencoder: image side {R}x{R2} unsupported (square, one of {ENC_SIDES})')
        x = x.contiguous()
        self._arith.packed()
        mom = torch.empty(B, 2 * Z_CH, R // 8, R // 8, device=x.device, dtype=torch.float32)
        n = self.encode_chunk(R)  # ('bf16x3' has no addressing limit of its own; the same chunks bound its workspace)
        for s in range(0, B, n):
            self._encode_chunk(x[s:s + n], u8, flip, mom[s:s + n])
        return mom

    def sample(self, moments: torch.Tensor) -> torch.Tensor:
        """autoencoder.py:436-442 (== utils.sample): scale_factor * (mean + exp(logvar / 2) * randn), logvar clamped."""
        from . import latents
        return latents.sample(moments, self.scale_factor)

    def encode(self, x, flip: bool = False):
        """autoencoder.py:444-447: sample(encode_moments(x))."""
        if not self.has_encoder:
            raise NotImplementedError('encoding (autoencoder.py:203-304) is outside the sampling path: training consumes '
                                      'pre-computed latent moments (train_utils/datasets.py:240-304); '
                                      'get_model(path, encoder=True) builds the encoder')
        return self.sample(self.encode_moments(x, flip=flip))

    def forward(self, inputs, fn):
        if fn == 'decode':
            return self.decode(inputs)
        if fn == 'encode_moments':
            return self.encode_moments(inputs)
        if fn == 'encode':
            return self.encode(inputs)
        raise NotImplementedError(fn)

    def release_workspace(self):
        self._ws.clear()


def synthetic_state_dict(seed: int = 0, encoder: bool = True) -> Dict[str, torch.Tensor]:
    """Seeded stand-in weights in the checkpoint layout (tools without autoencoder_kl.pth: extract_latent.py --ckpt none,
    tools/vae_encode_bench.py): convolutions N(0, 1.6 / fan_in) (activations stay O(1) through the ~30 layers), biases
    N(0, 0.05), GroupNorm gamma 1 + N(0, 0.1), beta N(0, 0.1)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shp in (encoder_param_table() if encoder else []) + decoder_param_table():
        if name.endswith('.weight') and len(shp) == 4:
            sd[name] = torch.randn(shp, generator=g) * (1.6 / (shp[1] * shp[2] * shp[3])) ** 0.5
        elif '.norm' in name and name.endswith('.weight'):
            sd[name] = 1.0 + 0.1 * torch.randn(shp, generator=g)
        elif '.norm' in name:
            sd[name] = 0.1 * torch.randn(shp, generator=g)
        else:
            sd[name] = 0.05 * torch.randn(shp, generator=g)
    return sd


def get_model(pretrained_path: Optional[str], scale_factor: float = 0.18215, encoder: bool = False,
              precision: str = 'bf16') -> FrozenAutoencoderKL:
    """autoencoder.py:468-474 (`pretrained_path=None`: zero weights, to be filled with load_state_dict; `encoder=True`:
    the encode side as well; `precision`: 'bf16' or the fp32-accurate 'bf16x3')."""
    return FrozenAutoencoderKL(pretrained_path, scale_factor, encoder=encoder, precision=precision)
