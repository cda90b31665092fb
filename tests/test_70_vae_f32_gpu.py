"""The fp32-accurate autoencoder arithmetic (`precision='bf16x3'`: mdt_conv3x3_bf16x3_nhwc, mdt_gn_im2col_f32,
mdt_vae_enc_prologue_f32 + the existing bf16x3 / fp32 GEMMs) on the GPU.

Yardstick: tests/golden/vae_f32.npz (make_golden_vae_f32.py) -- the reference's own Decoder / Encoder modules run in fp64,
and the distance of their fp32 run from it (`dec_e_ref`, `enc_e_ref`).  Every network-level bound is a multiple of those
two numbers, read from the fixture:
  * 3 x e_ref against fp64: the MFMA's block summation order, the three dropped cross products and another order of the
    GroupNorm sums are each allowed one reference rounding error;
  * 4 x e_ref against an fp32 run (the oracle, `mom256`): ours plus the fp32 run's own.
Kernel-level bounds are those of tests/test_50_bf16x3_gpu.py for the linear kernel (same arithmetic at K = 9 C)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'

if torch.cuda.is_available():
    from maskdit_amd import autoencoder as AE
    from maskdit_amd import ops
    from maskdit_amd._lib import call
    from oracle import vae_oracle as VO
    from tests import vae_encoder_ref as VE


def _st():
    return torch.cuda.current_stream().cuda_stream


def _relmax(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-300)).item()


def _bits(t):
    return t.contiguous().view(torch.int32)


def quantise(img):
    """sample.py:287: add 1, mul 127.5, clamp 0..255, truncate to uint8 (on a copy)."""
    return img.detach().clone().add_(1).mul(127.5).clamp_(0, 255).to(torch.uint8)


@pytest.fixture(scope='module')
def fx(golden_dir):
    return {'f32': np.load(os.path.join(golden_dir, 'vae_f32.npz')), 'dec': np.load(os.path.join(golden_dir, 'vae_decode.npz')),
            'enc': np.load(os.path.join(golden_dir, 'vae_encode.npz'))}


@pytest.fixture(scope='module')
def dec(fx):
    """(decode-only model at 'bf16x3', its weights, z, our image, the oracle's fp32 image)"""
    P = VO.init_vae_params(seed=int(fx['dec']['seed']))
    m = AE.get_model(None, precision='bf16x3')
    m.load_state_dict(P)
    m = m.to(DEV)
    z = torch.from_numpy(fx['dec']['z'])
    img = m.decode(z.to(DEV))
    with torch.no_grad():
        ora = VO.vae_decode(P, z)
    return m, P, z, img, ora


@pytest.fixture(scope='module')
def enc(fx):
    P = VE.init_vae_encoder_params(int(fx['enc']['seed']))
    m = AE.get_model(None, encoder=True, precision='bf16x3')
    m.load_state_dict({**AE.synthetic_state_dict(1, encoder=False), **P})
    return m.to(DEV), P


# ------------------------------------------------------------------------------------------------------------ kernels
CONV_SHAPES = [(2, 16, 128, 128, 'plain'), (1, 32, 256, 128, 'up'), (4, 8, 512, 512, 'plain'), (2, 16, 128, 3, 'up'),
               (2, 16, 128, 128, 'down'), (1, 24, 128, 256, 'plain'), (3, 12, 64, 200, 'up'), (1, 10, 32, 8, 'down')]


def _conv_ref(x, w, bias, mode):
    if mode == 'up':
        return F.conv2d(F.interpolate(x, scale_factor=2, mode='nearest'), w, bias, padding=1)
    if mode == 'down':
        return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, bias, stride=2)
    return F.conv2d(x, w, bias, padding=1)


def _im2col(x, mode):
    """the materialised operand of the same convolution, fp32 [M, 9 C] in (ky, kx, c) order: data movement only"""
    B, C = x.shape[:2]
    if mode == 'up':
        cols = F.unfold(F.interpolate(x, scale_factor=2, mode='nearest'), 3, padding=1)
    elif mode == 'down':
        cols = F.unfold(F.pad(x, (0, 1, 0, 1)), 3, stride=2)
    else:
        cols = F.unfold(x, 3, padding=1)
    L = cols.shape[-1]
    return cols.view(B, C, 9, L).permute(0, 3, 2, 1).reshape(B * L, 9 * C).contiguous()


@pytest.mark.parametrize('with_res', [False, True])
@pytest.mark.parametrize('B,Hi,C,Cout,mode', CONV_SHAPES)
def test_conv3x3_bf16x3_vs_fp64(B, Hi, C, Cout, mode, with_res):
    """mdt_conv3x3_bf16x3_nhwc against F.conv2d in fp64 on the CPU on the same fp32 operands, under the bounds
    test_50_bf16x3_gpu.py::test_gemm_bf16x3_vs_fp64 applies to the linear kernel: err <= 2 err(mdt_gemm_f32) + 1e-7 (the
    exact-fp32 GEMM on the materialised im2col matrix of the same operands) and err <= 0.01 err(bf16-rounded operands), all
    relative to the largest fp64 magnitude.  Ragged M and N (Cout 3, 200, 8 without a padded weight), a side that is no power
    of two, two launches bit-identical, NaN poison around the activation and its zero line."""
    torch.manual_seed(31)
    x = torch.randn(B, C, Hi, Hi)
    w = torch.randn(Cout, C, 3, 3) / (3.0 * C ** 0.5)
    bias = torch.randn(Cout)
    Ho = Hi // 2 if mode == 'down' else (Hi * 2 if mode == 'up' else Hi)
    M = B * Ho * Ho
    ldo = (Cout + 3) // 4 * 4
    res = torch.randn(M, ldo) if with_res else None

    def to_rows(t):  # [B, Cout, Ho, Ho] -> [M, Cout]
        return t.permute(0, 2, 3, 1).reshape(M, Cout)

    ref = to_rows(_conv_ref(x.double(), w.double(), bias.double(), mode))
    ref16 = to_rows(_conv_ref(x.bfloat16().double(), w.bfloat16().double(), bias.double(), mode))
    if with_res:
        ref, ref16 = ref + res[:, :Cout].double(), ref16 + res[:, :Cout].double()
    n = B * Hi * Hi * C
    raw = torch.full((64 + n + 64,), float('nan'), device=DEV)
    raw[32:64].zero_()                                                    # the zero line: 32 floats in front of the activation
    raw[64:64 + n].copy_(x.permute(0, 2, 3, 1).reshape(-1))              # NHWC
    act = raw[64:64 + n]
    wm = w.permute(0, 2, 3, 1).reshape(Cout, 9 * C).contiguous().to(DEV)  # K ordered (ky, kx, c)
    db, dres = bias.to(DEV), (res.to(DEV) if with_res else None)
    outs = []
    for _ in range(2):
        out = torch.full((M, ldo), float('nan'), device=DEV)
        call('mdt_conv3x3_bf16x3_nhwc', act.data_ptr(), B, Hi, C, int(mode == 'up'), int(mode == 'down'), wm.data_ptr(), db.data_ptr(),
             dres.data_ptr() if with_res else None, out.data_ptr(), ldo, Cout, _st())
        outs.append(out)
    assert torch.equal(_bits(outs[0][:, :Cout]), _bits(outs[1][:, :Cout])), 'two launches differ'
    if ldo > Cout:
        assert bool(torch.isnan(outs[0][:, Cout:]).all()), 'columns beyond Cout were written'
    f32 = torch.empty(M, ldo, device=DEV)
    ops.gemm_f32(_im2col(x.to(DEV), mode), wm, f32, M, Cout, 9 * C, ldo=ldo, bias=db,
                 epi=ops.F32EPI_GATE_RES if with_res else ops.F32EPI_NONE, res=dres, rows_per_sample=1)
    e3, e32, e16 = _relmax(outs[0][:, :Cout], ref), _relmax(f32[:, :Cout], ref), _relmax(ref16, ref)
    print(f'conv3x3 bf16x3 B{B} H{Hi} C{C}->{Cout} {mode} res {with_res}: bf16x3 {e3:.2e}, fp32 GEMM {e32:.2e}, bf16 operands {e16:.2e}')
    assert e3 <= 2 * e32 + 1e-7, f'bf16x3 {e3:.3e} vs fp32 {e32:.3e}'
    assert e3 <= 0.01 * e16, f'bf16x3 {e3:.3e} vs bf16-rounded operands {e16:.3e}'


@pytest.mark.parametrize('B,H,C,ks,up,norm,swish', [(2, 8, 128, 3, 0, True, True), (3, 4, 512, 3, 1, False, False),
                                                    (2, 8, 256, 1, 0, True, False), (1, 16, 128, 3, 1, True, True),
                                                    (2, 16, 4, 3, 0, False, False), (2, 12, 128, 1, 0, True, True)])
def test_gn_im2col_f32(B, H, C, ks, up, norm, swish):
    """mdt_gn_im2col_f32 against torch fp32 to 1e-5 of max (test_01_vae_gpu.py's tolerance for the fp32 glue kernels); the
    same cases as test_gn_stats_and_im2col plus conv_in's C = 4, K = 36 and a side that is no power of two."""
    torch.manual_seed(1)
    x = (torch.randn(B, H, H, C, device=DEV) * 1.7 + 0.3).contiguous()  # NHWC
    gamma, beta = torch.randn(C, device=DEV) * 0.3 + 1, torch.randn(C, device=DEV) * 0.2
    sums = torch.full((B, 32, 2), 9.0, device=DEV)  # stale contents must be overwritten
    if norm:
        from maskdit_amd import _lib
        ws = torch.empty(int(_lib.lib().mdt_gn_stats_ordered_ws_floats(B, 32)), device=DEV)
        call('mdt_gn_stats_ordered', x.data_ptr(), sums.data_ptr(), ws.data_ptr(), B, H * H, C, 32, _st())
        xg = x.double().view(B, H * H, 32, C // 32)
        assert _relmax(sums, torch.stack([xg.sum((1, 3)), (xg * xg).sum((1, 3))], -1)) < 1e-5
    Kp = ks * ks * C
    Ho = H << up
    col = torch.full((B * Ho * Ho, Kp), float('nan'), device=DEV)
    call('mdt_gn_im2col_f32', x.data_ptr(), sums.data_ptr() if norm else None, gamma.data_ptr() if norm else None,
         beta.data_ptr() if norm else None, col.data_ptr(), B, H, H, C, 32, ks, up, int(swish), Kp, _st())
    t = x.permute(0, 3, 1, 2)
    if norm:
        t = F.group_norm(t, 32, gamma, beta, eps=1e-6)
    if swish:
        t = t * torch.sigmoid(t)
    if up:
        t = F.interpolate(t, scale_factor=2.0, mode='nearest')
    cols = F.unfold(t, ks, padding=ks // 2).view(B, C, ks * ks, Ho * Ho).permute(0, 3, 2, 1).reshape(B * Ho * Ho, Kp)
    e = _relmax(col, cols)
    print(f'gn_im2col_f32 B{B} H{H} C{C} k{ks} up{up} norm{norm} swish{swish}: {e:.2e} of max')
    assert e <= 1e-5
    if not norm and not swish:
        assert torch.equal(_bits(col), _bits(cols)), 'without GroupNorm / swish the writer only moves data'


@pytest.mark.parametrize('B,HW,C', [(2, 256 * 256, 128), (3, 48 * 48, 512), (1, 100, 256)])
def test_gn_stats_ordered(B, HW, C):
    """mdt_gn_stats_ordered against fp64 sums to 1e-5 of max (the fp32 glue tolerance) and bit-identical over three runs at
    sizes that split a sample over many workgroups (mdt_gn_stats adds those with atomics)."""
    from maskdit_amd import _lib
    torch.manual_seed(4)
    x = torch.randn(B, HW, C, device=DEV) * 1.3 + 0.4
    ws = torch.empty(int(_lib.lib().mdt_gn_stats_ordered_ws_floats(B, 32)), device=DEV)
    runs = []
    for _ in range(3):
        sums = torch.full((B, 32, 2), 9.0, device=DEV)
        call('mdt_gn_stats_ordered', x.data_ptr(), sums.data_ptr(), ws.data_ptr(), B, HW, C, 32, _st())
        runs.append(sums)
    xg = x.double().view(B, HW, 32, C // 32)
    assert _relmax(runs[0], torch.stack([xg.sum((1, 3)), (xg * xg).sum((1, 3))], -1)) < 1e-5
    assert torch.equal(_bits(runs[0]), _bits(runs[1])) and torch.equal(_bits(runs[0]), _bits(runs[2]))


@pytest.mark.parametrize('u8', [0, 1])
@pytest.mark.parametrize('flip', [0, 1])
def test_enc_prologue_f32_bit_exact(u8, flip):
    """conv_in's fp32 im2col (K = 27 padded to 28): bit-exact against u8_to_unit (ToTensor + Normalize in fp32 on the CPU),
    flip, unfold."""
    B, R, Kp = 2, 32, 28
    g = torch.Generator().manual_seed(7 + u8 + 2 * flip)
    if u8:
        img = torch.randint(0, 256, (B, R, R, 3), generator=g, dtype=torch.uint8)
        unit = VE.u8_to_unit(img)
    else:
        img = torch.rand(B, 3, R, R, generator=g) * 2 - 1
        unit = img
    if flip:
        unit = unit.flip(dims=[-1])
    want = torch.zeros(B * R * R, Kp)
    want[:, :27] = F.unfold(unit, 3, padding=1).view(B, 3, 9, R * R).permute(0, 3, 2, 1).reshape(B * R * R, 27)
    col = torch.full((B * R * R, Kp), 5.0, device=DEV)
    dimg = img.to(DEV)
    call('mdt_vae_enc_prologue_f32', dimg.data_ptr(), u8, flip, col.data_ptr(), B, R, Kp, _st())
    assert torch.equal(_bits(col.cpu()), _bits(want))


# ------------------------------------------------------------------------------------------------------------ decode
def test_decode_accuracy(dec, fx):
    """err64 = max |x - ref64| / max |ref64| on the stored positions (centre crop of image 0, image 1 at stride 4) must be
    <= 3 dec_e_ref; against the oracle's full fp32 images <= 4 dec_e_ref.  The bf16 path is printed for contrast.
    Measured values: none recorded yet (the test prints them; tools/vae_bf16x3_bench.py writes them to
    profiles/vae_bf16x3_bench.txt)."""
    m, P, z, img, ora = dec
    f = fx['f32']
    e_ref = float(f['dec_e_ref'])
    assert img.shape == (2, 3, 256, 256) and img.dtype == torch.float32 and bool(torch.isfinite(img).all())
    ref0 = torch.from_numpy(f['dec_lv0_crop']).double() / 127.5 - 1     # (the crop is stored as grey levels in fp32: its own
    ref1 = torch.from_numpy(f['dec64_img1_sub'])                        # rounding, 2^-24 of 255, is a tenth of dec_e_ref)
    absmax = max(ref0.abs().max().item(), ref1.abs().max().item())

    def err64(x):
        x = x.detach().double().cpu()
        return max((x[0, :, 64:192, 64:192] - ref0).abs().max().item(), (x[1, :, ::4, ::4] - ref1).abs().max().item()) / absmax

    e64, e32 = err64(img), _relmax(img, ora)
    m.set_precision('bf16')
    try:
        img16 = m.decode(z.to(DEV))
    finally:
        m.set_precision('bf16x3')
    print(f"VAE decode 'bf16x3': {e64:.3e} of max vs fp64 (bound {3 * e_ref:.3e}), {e32:.3e} vs the fp32 oracle (bound {4 * e_ref:.3e}); "
          f"reference fp32 vs fp64 {e_ref:.3e}, oracle fp32 vs fp64 {err64(ora):.3e}; 'bf16' path {err64(img16):.3e} vs fp64")
    assert e64 <= 3 * e_ref
    assert e32 <= 4 * e_ref


def test_decode_pixels(dec, fx):
    """After sample.py:287's quantisation: inside the stored crop every pixel whose fp64 grey level is farther than
    delta = 3 dec_e_ref max|ref64| 127.5 from an integer equals the quantised fp64 value, and over both full images no pixel
    differs from the oracle's fp32 uint8 image by more than one level."""
    m, P, z, img, ora = dec
    f = fx['f32']
    lv = torch.from_numpy(f['dec_lv0_crop']).double()
    delta = 3 * float(f['dec_e_ref']) * float(f['dec_absmax64']) * 127.5
    q = quantise(img.cpu())
    want = lv.clamp(0, 255).to(torch.uint8)
    safe = (lv - lv.round()).abs() > delta
    got = q[0, :, 64:192, 64:192]
    bad = int(((got != want) & safe).sum())
    d = (q.int() - quantise(ora).int()).abs()
    print(f'VAE decode pixels: delta {delta:.2e} levels, {int((~safe).sum())} of {safe.numel()} crop values within delta of a boundary, '
          f'{int((got != want).sum())} crop values differ from fp64 ({bad} of them away from a boundary); '
          f'{int((d != 0).sum())} of {d.numel()} uint8 values differ from the fp32 oracle image (largest step {int(d.max())}; '
          f'the reference fp32 vs fp64: {int(f["dec_n_u8_ref"])})')
    assert bad == 0
    assert int(d.max()) <= 1


def test_decode_reproducible_and_batch_invariant(dec, fx):
    """Two decode calls give identical bits; decode(z[1:2]) agrees with decode(z)[1] to within dec_e_ref (whether it is
    in fact bit-identical is printed; not recorded yet.  The summation order inside a convolution does not depend on the
    batch and the GroupNorm sums are per sample, but the attention GEMMs take another kernel form at batch 1)."""
    m, P, z, img, ora = dec
    again = m.decode(z.to(DEV))
    assert torch.equal(_bits(again), _bits(img)), 'two decodes of the same latents differ'
    one = m.decode(z[1:2].to(DEV))
    e = _relmax(one[0], img[1])
    print(f'decode(z[1:2]) vs decode(z)[1]: {e:.3e} of max; bit-identical: {torch.equal(_bits(one[0]), _bits(img[1]))}')
    assert e <= float(fx['f32']['dec_e_ref'])


def test_decode_domain(dec, fx):
    m, P, z, img, ora = dec
    e_ref = float(fx['f32']['dec_e_ref'])
    big = m.decode(torch.randn(1, 4, 64, 64, device=DEV) * 0.5)
    assert big.shape == (1, 3, 512, 512) and bool(torch.isfinite(big).all())
    z48 = torch.randn(1, 4, 48, 48, generator=torch.Generator().manual_seed(5)) * 0.5
    img48 = m.decode(z48.to(DEV))
    with torch.no_grad():
        ref48 = VO.vae_decode(P, z48)
    e48 = _relmax(img48, ref48)
    print(f"VAE decode 48x48 latent 'bf16x3' vs the fp32 oracle: {e48:.3e} of max (bound {4 * e_ref:.3e})")
    assert img48.shape == (1, 3, 384, 384) and e48 <= 4 * e_ref
    with pytest.raises(NotImplementedError):
        m.decode(torch.zeros(1, 4, 24, 24, device=DEV))
    for prec in AE.PRECISIONS:
        with pytest.raises(NotImplementedError):
            AE.get_model(None, precision=prec).to(DEV).encode_moments(torch.zeros(1, 3, 128, 128, device=DEV))


# ------------------------------------------------------------------------------------------------------------ encode
def test_encode_accuracy(enc, fx):
    """encode_moments on img256 against the fp64 moments, bound 3 enc_e_ref: uint8 input, fp32 NCHW input, and flip=True fed
    with the mirrored image (both input forms); `mom256` of the existing fixture (the reference's fp32 run) at 4 enc_e_ref."""
    m, P = enc
    f = fx['f32']
    e_ref = float(f['enc_e_ref'])
    img = torch.from_numpy(fx['enc']['img256'])
    ref64 = torch.from_numpy(f['mom64_256'])[None]
    ref32 = torch.from_numpy(fx['enc']['mom256'])[None]
    got8 = m.encode_moments(img[None].to(DEV))
    gotf = m.encode_moments(VE.u8_to_unit(img)[None].to(DEV))
    assert got8.shape == (1, 8, 32, 32) and got8.dtype == torch.float32
    e8, ef, e32 = _relmax(got8, ref64), _relmax(gotf, ref64), _relmax(got8, ref32)
    m.set_precision('bf16')
    try:
        e16 = _relmax(m.encode_moments(img[None].to(DEV)), ref64)
    finally:
        m.set_precision('bf16x3')
    print(f"VAE encode 256^2 'bf16x3': uint8 input {e8:.3e} of max vs fp64, fp32 input {ef:.3e} (bound {3 * e_ref:.3e}); "
          f"vs the reference's fp32 moments {e32:.3e} (bound {4 * e_ref:.3e}); reference fp32 vs fp64 {e_ref:.3e}; 'bf16' path {e16:.3e}")
    assert e8 <= 3 * e_ref and ef <= 3 * e_ref
    assert e32 <= 4 * e_ref
    # flip=True on the mirrored image is the encoder on the image itself: the same fp64 yardstick, and the same operand bits
    mirrored = img.flip(dims=[1]).contiguous()  # [R, R, 3]: the x axis
    for name, xin in (('uint8', mirrored[None]), ('fp32', VE.u8_to_unit(mirrored)[None])):
        gflip = m.encode_moments(xin.to(DEV), flip=True)
        eflip = _relmax(gflip, ref64)
        print(f'VAE encode flip=True on the mirrored {name} image: {eflip:.3e} of max vs fp64 (bound {3 * e_ref:.3e})')
        assert eflip <= 3 * e_ref
        assert torch.equal(_bits(gflip), _bits(got8)), 'flip=True of the mirrored image differs from encoding the image'


def test_encode_reproducible(enc, fx):
    m, P = enc
    x = torch.from_numpy(fx['enc']['img256'])[None].to(DEV)
    a, b = m.encode_moments(x), m.encode_moments(x)
    assert torch.equal(_bits(a), _bits(b)), 'two encode_moments calls differ'


# ------------------------------------------------------------------------------------------------------------ default
def test_default_precision_untouched(fx):
    """No `precision` argument: 'bf16', and the fp32 weight images are never packed."""
    P = VO.init_vae_params(seed=int(fx['dec']['seed']))
    m = AE.get_model(None)
    assert m.precision == 'bf16'
    m.load_state_dict(P)
    m = m.to(DEV)
    m.decode(torch.from_numpy(fx['dec']['z']).to(DEV))
    assert m._packed_x3 is None and m._packed is not None
    m.set_precision('bf16x3')
    m.decode(torch.from_numpy(fx['dec']['z'][:1]).to(DEV))
    assert m._packed_x3 is not None
    m.to(DEV)  # `_apply` drops both weight images
    assert m._packed_x3 is None and m._packed is None
    with pytest.raises(ValueError):
        m.set_precision('fp32')
