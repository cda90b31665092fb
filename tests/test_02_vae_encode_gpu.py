"""VAE encode on the GPU (FrozenAutoencoderKL.encode_moments, extract_latent.py): the three encoder kernels against torch,
the whole encoder against the reference-generated fixture (tests/golden/vae_encode.npz) and the CPU restatement
(tests/vae_encoder_ref.py), chunking and batch invariance, the encode / forward surface, and a round trip through the
extraction tool.  Tolerances are stated at each test.  Two encodes of the same images are not bitwise equal: the fused
convolution epilogue accumulates the next GroupNorm's statistics with fp32 atomics (as in decode), and a last-bit change of
a statistic can flip the bf16 rounding of an activation downstream -- REPEAT = the bound for such pairs."""
import os
import pickle
import subprocess
import sys
import tarfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'
REPEAT = 1e-2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if torch.cuda.is_available():
    from maskdit_amd import autoencoder as AE
    from maskdit_amd import latents
    from maskdit_amd._lib import call
    from tests import vae_encoder_ref as VE


def _st():
    return torch.cuda.current_stream().cuda_stream


def _relmax(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def _rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm()).item()


@pytest.fixture(scope='module')
def enc_fixture(golden_dir):
    return np.load(os.path.join(golden_dir, 'vae_encode.npz'))


@pytest.fixture(scope='module')
def vae(enc_fixture):
    P = VE.init_vae_encoder_params(int(enc_fixture['seed']))
    m = AE.get_model(None, encoder=True)
    m.load_state_dict({**AE.synthetic_state_dict(1, encoder=False), **P})
    return m.to(DEV), P


@pytest.mark.parametrize('B,Hi,C', [(4, 16, 128), (1, 64, 256), (3, 32, 512), (2, 256, 128)])
def test_conv3x3_down_vs_conv2d(B, Hi, C):
    """mdt_conv3x3_down_nhwc against F.conv2d(F.pad(x, (0, 1, 0, 1)), stride=2) on the same bf16-rounded operands
    (Downsample, autoencoder.py:56-75).  (2, 16, 128) of the issue is 128 output rows, not whole 256-row tiles: the
    entry rejects it (test_vae_encode_cpu.py), so the smallest case runs with B = 4."""
    torch.manual_seed(41)
    x = torch.randn(B, C, Hi, Hi, device=DEV)
    w = torch.randn(C, C, 3, 3, device=DEV) / (3.0 * C ** 0.5)
    bias = torch.randn(C, device=DEV)
    xb, wb = x.to(torch.bfloat16), w.to(torch.bfloat16)
    ref = F.conv2d(F.pad(xb.float(), (0, 1, 0, 1)), wb.float(), bias, stride=2)      # [B, C, Ho, Ho]
    Ho = Hi // 2
    raw = torch.full((128 + B * Hi * Hi * C,), 7.0, device=DEV, dtype=torch.bfloat16)  # poison: only the zero line may be read outside
    raw[:128].zero_()
    raw[128:].copy_(xb.permute(0, 2, 3, 1).reshape(-1))
    wm = wb.permute(0, 2, 3, 1).reshape(C, -1).contiguous()                           # K ordered (ky, kx, c)
    out = torch.empty(B * Ho * Ho, C, device=DEV)
    call('mdt_conv3x3_down_nhwc', raw[128:].data_ptr(), B, Hi, C, wm.data_ptr(), bias.data_ptr(), None, out.data_ptr(), C, C, None, 0,
         _st())
    got = out.reshape(B, Ho, Ho, C).permute(0, 3, 1, 2)
    err = _relmax(got, ref)
    print(f'conv3x3 stride 2 B{B} H{Hi} C{C}: rel-to-max err {err:.2e}')
    assert err <= 2e-5  # same bf16 operands, fp32 accumulation both ways
    res = torch.randn(B * Ho * Ho, C, device=DEV)
    fused = torch.empty_like(out)
    use_gn = (Ho * Ho) % 128 == 0
    sums = torch.zeros(B, 32, 2, device=DEV) if use_gn else None
    call('mdt_conv3x3_down_nhwc', raw[128:].data_ptr(), B, Hi, C, wm.data_ptr(), bias.data_ptr(), res.data_ptr(), fused.data_ptr(), C, C,
         sums.data_ptr() if use_gn else None, 32, _st())
    assert _relmax(fused, out + res) <= 1e-6, 'fused skip connection differs from conv + add'
    if use_gn:
        v = fused.double().reshape(B, Ho * Ho, 32, C // 32)
        want = torch.stack([v.sum((1, 3)), (v * v).sum((1, 3))], -1)
        e = _relmax(sums, want)
        print(f'  fused GroupNorm sums: rel-to-max err {e:.2e}')
        assert e <= 1e-5


@pytest.mark.parametrize('u8', [0, 1])
@pytest.mark.parametrize('flip', [0, 1])
def test_enc_prologue_bit_exact(u8, flip):
    """conv_in's im2col from the image: bit-exact against torch (ToTensor + Normalize in fp32 on the CPU, flip, unfold)."""
    B, R, Kp = 2, 32, 64
    g = torch.Generator().manual_seed(7 + u8 + 2 * flip)
    if u8:
        img = torch.randint(0, 256, (B, R, R, 3), generator=g, dtype=torch.uint8)
        unit = VE.u8_to_unit(img)
    else:
        img = torch.rand(B, 3, R, R, generator=g) * 2 - 1
        unit = img
    if flip:
        unit = unit.flip(dims=[-1])
    cols = F.unfold(unit, 3, padding=1).view(B, 3, 9, R * R).permute(0, 3, 2, 1).reshape(B * R * R, 27)
    want = torch.zeros(B * R * R, Kp, dtype=torch.bfloat16)
    want[:, :27] = cols.to(torch.bfloat16)
    col = torch.full((B * R * R, Kp), 5.0, device=DEV, dtype=torch.bfloat16)
    dimg = img.to(DEV)
    call('mdt_vae_enc_prologue', dimg.data_ptr(), u8, flip, col.data_ptr(), B, R, Kp, _st())
    assert torch.equal(col.cpu().view(torch.int16), want.view(torch.int16))


def test_enc_epilogue_vs_conv1x1():
    B, HW, ld = 3, 24 * 24, 128
    torch.manual_seed(3)
    h = torch.randn(B * HW, ld, device=DEV)
    qw, qb = torch.randn(8, 8, 1, 1, device=DEV), torch.randn(8, device=DEV)
    mom = torch.empty(B, 8, 24, 24, device=DEV)
    call('mdt_vae_enc_epilogue', h.data_ptr(), ld, qw.data_ptr(), qb.data_ptr(), mom.data_ptr(), B, HW, _st())
    ref = F.conv2d(h[:, :8].reshape(B, 24, 24, 8).permute(0, 3, 1, 2).double(), qw.double(), qb.double())
    assert _relmax(mom, ref) <= 1e-6


def test_encode_moments_vs_reference_fixture(vae, enc_fixture):
    """The whole encoder (~27 bf16-operand convolutions + the attention block, fp32 accumulation) against the reference's
    fp32 modules, through both input forms."""
    m, P = vae
    for R in (256, 128):
        img = torch.from_numpy(enc_fixture[f'img{R}'])
        ref = torch.from_numpy(enc_fixture[f'mom{R}'])[None]
        got8 = m.encode_moments(img[None].to(DEV))
        gotf = m.encode_moments(VE.u8_to_unit(img)[None].to(DEV))
        assert got8.shape == (1, 8, R // 8, R // 8) and got8.dtype == torch.float32
        assert _relmax(got8, gotf) <= REPEAT, 'uint8 and fp32 inputs give the same operand bits (test_enc_prologue_bit_exact)'
        # measured on MI355X (max over 128^2 / 256^2 and two runs): mean 7.8e-3 of max, 7.6e-3 rel L2; logvar 1.01e-2 of max, 7.8e-3
        # rel L2.  Bounds: 3x measured, capped at the decode test's (2.7e-2 of max, 2.2e-2 rel L2)
        for half, sl, bmax in (('mean', slice(0, 4), 2.2e-2), ('logvar', slice(4, 8), 2.7e-2)):
            e, r = _relmax(got8[:, sl], ref[:, sl]), _rel_l2(got8[:, sl], ref[:, sl])
            print(f'VAE encode {R}^2 {half}: {e:.3e} of max, {r:.3e} rel L2')
            assert e <= bmax and r <= 2.2e-2


def test_encode_512_vs_helper_and_chunking(vae):
    m, P = vae
    g = torch.Generator().manual_seed(9)
    x = torch.rand(1, 3, 512, 512, generator=g) * 2 - 1
    got = m.encode_moments(x.to(DEV))
    with torch.no_grad():
        ref = VE.vae_encode_moments(P, x)
    e, r = _relmax(got, ref), _rel_l2(got, ref)
    print(f'VAE encode 512^2 vs CPU restatement: {e:.3e} of max, {r:.3e} rel L2')
    assert e <= 2.2e-2 and r <= 2.1e-2  # measured 7.2-7.8e-3 / 6.8e-3: about 3x
    # a batch of 65 at 512^2 runs as chunks of 32 (the activation limit of the implicit-GEMM convolution)
    xs = (torch.rand(65, 512, 512, 3, generator=g) * 255).to(torch.uint8).to(DEV)
    big = m.encode_moments(xs)
    assert big.shape == (65, 8, 64, 64) and bool(torch.isfinite(big).all())
    one = m.encode_moments(xs[64:65])
    eb = _relmax(one[0], big[64])
    print(f'image 64 of a 65-batch vs alone: {eb:.2e} of max')
    assert eb <= 2e-2  # other tile / chunk composition: bf16 rounding flips through the layers (measured 4.3e-3)
    m.release_workspace()


def test_batch_invariance_encode_and_forward(vae, enc_fixture):
    m, P = vae
    img = torch.from_numpy(enc_fixture['img256'])[None].to(DEV)
    g = torch.Generator().manual_seed(4)
    batch = torch.cat([(torch.rand(2, 256, 256, 3, generator=g) * 255).to(torch.uint8).to(DEV), img], 0)
    alone = m.encode_moments(img)
    inside = m.encode_moments(batch)[2:3]
    e = _relmax(alone, inside)
    print(f'batch invariance (256^2, 1 vs 3): {e:.2e} of max')
    assert e <= 2e-2  # measured 8.3e-3 (the decode test's bound)
    # encode = sample(encode_moments) under the same seed; forward routes like the reference
    x = VE.u8_to_unit(img.cpu()).to(DEV)
    mom = m(x, 'encode_moments')
    torch.manual_seed(123)
    z = m.encode(x)
    torch.manual_seed(123)
    z_ref = latents.sample(mom, 0.18215)
    assert z.shape == (1, 4, 32, 32) and _relmax(z, z_ref) <= REPEAT
    torch.manual_seed(123)
    assert _relmax(m(x, 'encode'), z_ref) <= REPEAT
    torch.manual_seed(123)
    assert torch.equal(m.sample(mom), z_ref)  # the reference's FrozenAutoencoderKL.sample == utils.sample
    assert mom.shape == (1, 8, 32, 32) and _relmax(mom, m.encode_moments(x)) <= REPEAT
    assert m(torch.zeros(1, 4, 32, 32, device=DEV), 'decode').shape == (1, 3, 256, 256)
    with pytest.raises(NotImplementedError):
        m(x, 'reconstruct')
    with pytest.raises(NotImplementedError):
        m.encode_moments(torch.zeros(1, 3, 384, 384, device=DEV))
    # mirrored input == encoding the mirrored image
    assert _relmax(m.encode_moments(img, flip=True), m.encode_moments(img.flip(dims=[2]).contiguous())) <= REPEAT


_FAKE_LMDB = '''
"""In-test stand-in for `lmdb` with writes: a database is a directory holding data.pkl = {key bytes: value bytes}."""
import builtins, os, pickle


class _Txn:
    def __init__(self, env, write):
        self.env, self.write = env, write

    def put(self, k, v):
        assert self.write
        self.env.t[bytes(k)] = bytes(v)

    def get(self, k, default=None):
        return self.env.t.get(bytes(k), default)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        with builtins.open(os.path.join(self.env.path, 'data.pkl'), 'wb') as f:
            pickle.dump(self.env.t, f)


class Environment:
    def __init__(self, path, **kw):
        self.path, self.t = path, {}
        os.makedirs(path, exist_ok=True)

    def begin(self, write=False):
        return _Txn(self, write)

    def close(self):
        pass


def open(path, **kw):
    return Environment(path, **kw)
'''


def test_extract_latent_round_trip(tmp_path, vae):
    """extract_latent.py in a child process on a tiny ImageFolder: WebDataset shards (with --xflip) and LMDB records
    equal direct encode_moments of the cropped images (and of their mirror images), with the right labels and count."""
    from PIL import Image
    from maskdit_amd.data import WdsTarLatents
    from maskdit_amd.images import image_folder_samples, load_rgb_crop
    m, P = vae
    rng = np.random.default_rng(5)
    data = tmp_path / 'data'
    for cls, n in (('b_cls', 3), ('a_cls', 2)):
        os.makedirs(data / 'train' / cls)
        for i in range(n):
            h, w = int(rng.integers(140, 300)), int(rng.integers(140, 300))
            Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(data / 'train' / cls / f'{i}.png')
    ckpt = tmp_path / 'vae.pth'
    torch.save(m.state_dict(), ckpt)
    samples, _ = image_folder_samples(str(data / 'train'))
    N = len(samples)
    crops = torch.from_numpy(np.stack([load_rgb_crop(p, 128) for p, _ in samples])).to(DEV)
    # the tool's batches of 2, encoded directly (same batch composition, so only the REPEAT-level differences remain)
    want = torch.cat([torch.cat([m.encode_moments(crops[s:s + 2], flip=f) for s in range(0, N, 2)]) for f in (False, True)]).cpu()
    labels = [y for _, y in samples] * 2
    base = [sys.executable, os.path.join(ROOT, 'extract_latent.py'), '--data_dir', str(data), '--split', 'train', '--ckpt', str(ckpt),
            '--resolution', '128', '--batch_size', '2', '--xflip', '--outdir', str(tmp_path / 'out'), '--workers', '4']
    env = dict(os.environ)
    r = subprocess.run(base + ['--format', 'wds', '--shard_size', '3'], capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout[-600:], r.stderr[-2000:])  # the last line carries the tool's images/s
    assert r.returncode == 0
    shards = str(tmp_path / 'out' / 'imagenet_128_latent_wds' / 'train')
    got = {}
    for path in sorted(os.listdir(shards)):
        with tarfile.open(os.path.join(shards, path)) as tf:
            for mem in tf:
                key, ext = mem.name.split('.', 1)
                got.setdefault(int(key), {})[ext] = tf.extractfile(mem).read()
    assert sorted(got) == list(range(2 * N))
    for i in range(2 * N):
        z = pickle.loads(got[i]['latent'])
        assert z.shape == (8, 16, 16) and int(got[i]['cls']) == labels[i]
        assert _relmax(torch.from_numpy(z), want[i]) <= REPEAT, i
    n = sum(len(z) for z, _ in WdsTarLatents(shards, batch=1, shuffle_buf=0))
    assert n == 2 * N
    # the LMDB branch, against an lmdb stand-in that supports writes
    fake = tmp_path / 'fake'
    os.makedirs(fake / 'lmdb')
    (fake / 'lmdb' / '__init__.py').write_text(_FAKE_LMDB)
    env['PYTHONPATH'] = str(fake) + os.pathsep + env.get('PYTHONPATH', '')
    r = subprocess.run(base + ['--format', 'lmdb'], capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout[-600:], r.stderr[-2000:])
    assert r.returncode == 0
    with open(tmp_path / 'out' / 'imagenet_128_latent_lmdb' / 'train' / 'data.pkl', 'rb') as f:
        t = pickle.load(f)
    assert int(t[b'length']) == 2 * N and len(t) == 4 * N + 1
    for i in range(2 * N):
        z = torch.from_numpy(np.frombuffer(t[f'z-{i}'.encode()], dtype=np.float32).reshape(8, 16, 16).copy())
        assert _relmax(z, want[i]) <= REPEAT, i
        assert int(t[f'y-{i}'.encode()]) == labels[i]
