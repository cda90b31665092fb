"""fp32 training of the unmasked stage (train.py --no_amp; csrc/f32train.hip) on the GPU.

Every tolerance is MEASURED inside the test against references on the same inputs:
    e_ref  = error of the fp32 reference route (torch CPU fp32 for kernels, the oracle in fp32 end to end) against fp64
    e_hip  = error of the HIP fp32 result against the same fp64 result
    e_bf16 = error of the existing bf16 route on the same inputs
and the criterion is  e_hip <= 4 e_ref  (a tiled / chunked reduction sums in another order than torch)  and
e_hip <= e_bf16 / 100  (bf16 and fp32 round-off differ by 2^15: this only proves that the fp32 route is the one running).
Errors are relative L2 per tensor, the worst tensor on each side.

head_dim 72 occurs only in DiT-XL/2.  The kernel tests (transposed product, attention backward) cover it directly, which
keeps the end-to-end tests at DiT-S/2 size and a few seconds.

Measured on an MI355X: see DESIGN.md section 7.3.
"""
import copy
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import maskdit_amd as M
    from maskdit_amd import _lib
    from maskdit_amd._lib import GemmF32TNArgs, GemmNTArgs, GemmTNArgs
    from oracle import maskdit_oracle as O

DEV = 'cuda'


def _st():
    return torch.cuda.current_stream().cuda_stream


def _rel(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return ((a - ref).norm() / (ref.norm() + 1e-300)).item()


def _check(what, e_hip, e_ref, e_bf16):
    print(f'[{what}] e_ref {e_ref:.3e}  e_hip {e_hip:.3e}  e_bf16 {e_bf16:.3e}  (e_hip / e_ref {e_hip / max(e_ref, 1e-300):.2f}, '
          f'e_bf16 / e_hip {e_bf16 / max(e_hip, 1e-300):.0f})')
    assert e_hip <= 4 * e_ref, f'{what}: e_hip {e_hip:.3e} > 4 e_ref {e_ref:.3e}'
    assert e_hip <= e_bf16 / 100, f'{what}: e_hip {e_hip:.3e} > e_bf16 / 100 ({e_bf16:.3e} / 100)'


def _rup(x, m):
    return (x + m - 1) // m * m


# ---------------------------------------------------------------------------------------------------------------------
# 1. mdt_gemm_f32_tn

def _tn(A, B, Cout, accumulate=0, batch=0, heads=0, a_s=(0, 0), b_s=(0, 0), c_s=(0, 0), M=None, N1=None, N2=None, lda=None,
        ldb=None, ldc=None):
    """C (+)= A^T B through mdt_gemm_f32_tn; A / B / Cout are tensors whose data_ptr is the first problem's base."""
    a = GemmF32TNArgs()
    a.A, a.lda, a.B, a.ldb = A.data_ptr(), lda, B.data_ptr(), ldb
    a.M, a.N1, a.N2 = M, N1, N2
    a.C, a.ldc, a.accumulate = Cout.data_ptr(), ldc, accumulate
    a.batch, a.heads = batch, heads
    a.a_stride_b, a.a_stride_h = a_s
    a.b_stride_b, a.b_stride_h = b_s
    a.c_stride_b, a.c_stride_h = c_s
    n = int(_lib.lib().mdt_gemm_f32_tn_ws_floats(M, N1, N2, max(batch, 1)))
    ws = torch.empty(max(n, 4), device=DEV, dtype=torch.float32)
    a.ws, a.ws_floats = ws.data_ptr(), n
    _lib.call('mdt_gemm_f32_tn', C.byref(a), _st())
    torch.cuda.synchronize()
    return n


def _tn_bf16(A, B):
    """the bf16 weight-gradient kernel (mdt_gemm_tn) on the same operands, zero-padded to its tile rules"""
    Mr, N1 = A.shape
    N2 = B.shape[1]
    Mp, N1p, N2p = _rup(Mr, 64), _rup(N1, 128), _rup(N2, 128)
    A16 = torch.zeros(Mp, N1p, device=DEV, dtype=torch.bfloat16)
    B16 = torch.zeros(Mp, N2p, device=DEV, dtype=torch.bfloat16)
    A16[:Mr, :N1] = A.to(DEV)
    B16[:Mr, :N2] = B.to(DEV)
    out = torch.zeros(N1, N2, device=DEV, dtype=torch.float32)
    a = GemmTNArgs()
    a.A, a.lda, a.B, a.ldb, a.M, a.N1, a.N2 = A16.data_ptr(), N1p, B16.data_ptr(), N2p, Mp, N1p, N2p
    a.C, a.ldc, a.n1_valid, a.n2_valid, a.splits = out.data_ptr(), N2, N1, N2, 0
    _lib.call('mdt_gemm_tn', C.byref(a), _st())
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize('Mr,N1,N2', [(200, 72, 100), (4104, 384, 1536), (64, 4, 16)])
def test_gemm_f32_tn_vs_fp64(Mr, N1, N2):
    g = torch.Generator().manual_seed(Mr + N1)
    A, B = torch.randn(Mr, N1, generator=g), torch.randn(Mr, N2, generator=g)
    C0 = torch.randn(N1, N2, generator=g)
    ref64 = A.double().t() @ B.double()
    e_ref = _rel(A.t() @ B, ref64)
    # the output sits inside a larger buffer of sentinels: two rows above / below, four columns left / right
    SENT = 12345.0
    ldc = N2 + 8
    Ad, Bd = A.to(DEV), B.to(DEV)
    outs = []
    for rep in range(2):
        buf = torch.full((N1 + 4, ldc), SENT, device=DEV)
        n = _tn(Ad, Bd, buf[2:, 4:], M=Mr, N1=N1, N2=N2, lda=N1, ldb=N2, ldc=ldc)
        frame = buf.clone()
        frame[2:N1 + 2, 4:N2 + 4] = SENT
        assert bool((frame == SENT).all()), 'gemm_f32_tn wrote outside its [N1, N2] output'
        outs.append(buf[2:N1 + 2, 4:N2 + 4].cpu())
    if (Mr, N1, N2) == (4104, 384, 1536):
        assert n > N1 * N2, 'this shape must take more than one token chunk (partials in the workspace)'
    assert torch.equal(outs[0], outs[1]), 'two launches differ: the reduction is not deterministic'
    e_hip = _rel(outs[0], ref64)
    _check(f'gemm_f32_tn {Mr}x{N1}x{N2}', e_hip, e_ref, _rel(_tn_bf16(A, B), ref64))
    # accumulate: C0 + A^T B
    acc = C0.to(DEV).contiguous()
    _tn(Ad, Bd, acc, accumulate=1, M=Mr, N1=N1, N2=N2, lda=N1, ldb=N2, ldc=N2)
    ref_acc = C0.double() + ref64
    assert _rel(acc, ref_acc) <= 4 * _rel(C0 + A.t() @ B, ref_acc)
    # the bias gradient: column sums of A
    cs = torch.full((N1,), 1.0, device=DEV)
    nws = int(_lib.lib().mdt_colsum_f32_ws_floats(Mr, N1))
    ws = torch.empty(max(nws, 4), device=DEV)
    _lib.call('mdt_colsum_f32', Ad.data_ptr(), N1, cs.data_ptr(), ws.data_ptr(), nws, Mr, N1, 1, _st())
    cs2 = torch.empty(N1, device=DEV)
    _lib.call('mdt_colsum_f32', Ad.data_ptr(), N1, cs2.data_ptr(), ws.data_ptr(), nws, Mr, N1, 0, _st())
    cs3 = torch.empty(N1, device=DEV)
    _lib.call('mdt_colsum_f32', Ad.data_ptr(), N1, cs3.data_ptr(), ws.data_ptr(), nws, Mr, N1, 0, _st())
    torch.cuda.synchronize()
    assert torch.equal(cs2, cs3)
    ref_cs = A.double().sum(0)
    assert _rel(cs2, ref_cs) <= 4 * max(_rel(A.sum(0), ref_cs), 2.0 ** -24)
    assert _rel(cs, 1 + ref_cs) <= 4 * max(_rel(1 + A.sum(0), 1 + ref_cs), 2.0 ** -24)


@pytest.mark.parametrize('L,hd', [(64, 32), (256, 72)])
def test_gemm_f32_tn_batched_on_packed_qkv(L, hd):
    """dk = dS^T q per (sample, head): A = scores [B, H, L, L], B = the q slot of a packed qkv buffer, C = the k slot of
    dqkv -- strided views, as the attention backward uses the entry."""
    Bn, H = 2, 3
    W = H * hd
    g = torch.Generator().manual_seed(L + hd)
    S = torch.randn(Bn, H, L, L, generator=g)
    qkv = torch.randn(Bn * L, 3 * W, generator=g)
    q = qkv.view(Bn, L, 3, H, hd)[:, :, 0].permute(0, 2, 1, 3)  # [B, H, L, hd]
    ref64 = S.double().transpose(-1, -2) @ q.double()
    e_ref = _rel(S.transpose(-1, -2) @ q, ref64)
    Sd, qd = S.to(DEV).contiguous(), qkv.to(DEV).contiguous()
    outs = []
    for rep in range(2):
        dqkv = torch.full((Bn * L, 3 * W), 7.0, device=DEV)
        _tn(Sd, qd, dqkv[:, W:], batch=Bn * H, heads=H, a_s=(H * L * L, L * L), b_s=(L * 3 * W, hd), c_s=(L * 3 * W, hd),
            M=L, N1=L, N2=hd, lda=L, ldb=3 * W, ldc=3 * W)
        v = dqkv.view(Bn, L, 3, H, hd)
        assert bool((v[:, :, 0] == 7.0).all()) and bool((v[:, :, 2] == 7.0).all()), 'wrote outside the k slot'
        outs.append(v[:, :, 1].permute(0, 2, 1, 3).cpu())
    assert torch.equal(outs[0], outs[1])
    e_bf16 = _rel(torch.stack([_tn_bf16(S[b, h], q[b, h].contiguous()) for b in range(Bn) for h in range(H)]).view(Bn, H, L, hd), ref64)
    _check(f'gemm_f32_tn batched L={L} hd={hd}', _rel(outs[0], ref64), e_ref, e_bf16)


# ---------------------------------------------------------------------------------------------------------------------
# 2. mdt_attn_f32_bwd

def _sdpa_grads(qkv, dout, Bn, L, H, hd, dtype):
    x = qkv.to(dtype).clone().requires_grad_(True)
    q, k, v = x.view(Bn, L, 3, H, hd).permute(2, 0, 3, 1, 4)  # timm Attention layout
    o = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(Bn * L, H * hd)
    o.backward(dout.to(dtype))
    return x.grad.view(Bn, L, 3, H, hd)


@pytest.mark.parametrize('Bn,H,L,hd', [(2, 3, 64, 32), (2, 3, 64, 72), (2, 3, 256, 64), (1, 2, 1024, 32)])
def test_attn_f32_bwd_vs_autograd_fp64(Bn, H, L, hd):
    W = H * hd
    g = torch.Generator().manual_seed(L * hd)
    qkv, dout = torch.randn(Bn * L, 3 * W, generator=g), torch.randn(Bn * L, W, generator=g)
    ref64 = _sdpa_grads(qkv, dout, Bn, L, H, hd, torch.float64)
    ref32 = _sdpa_grads(qkv, dout, Bn, L, H, hd, torch.float32)
    qd, dd = qkv.to(DEV), dout.to(DEV)
    n = int(_lib.lib().mdt_attn_f32_bwd_ws_floats(Bn, L, H, hd))
    ws = torch.empty(n, device=DEV)
    dqkv = torch.full((Bn * L, 3 * W), float('nan'), device=DEV)
    _lib.call('mdt_attn_f32_bwd', qd.data_ptr(), dd.data_ptr(), ws.data_ptr(), n, dqkv.data_ptr(), Bn, L, H, hd, _st())
    # the bf16 route: mdt_attn_fwd + mdt_attn_bwd
    q16, d16 = qd.bfloat16(), dd.bfloat16()
    o16, lse = torch.empty(Bn * L, W, device=DEV, dtype=torch.bfloat16), torch.empty(Bn * H * L, device=DEV)
    delta, dq16 = torch.empty(Bn * H * L, device=DEV), torch.empty(Bn * L, 3 * W, device=DEV, dtype=torch.bfloat16)
    _lib.call('mdt_attn_fwd', q16.data_ptr(), o16.data_ptr(), lse.data_ptr(), Bn, L, H, hd, 0, _st())
    _lib.call('mdt_attn_bwd', q16.data_ptr(), o16.data_ptr(), d16.data_ptr(), lse.data_ptr(), delta.data_ptr(), dq16.data_ptr(),
              Bn, L, H, hd, 0, _st())
    torch.cuda.synchronize()
    got, got16 = dqkv.view(Bn, L, 3, H, hd).cpu(), dq16.float().view(Bn, L, 3, H, hd).cpu()
    worst = lambda x: max(_rel(x[:, :, j], ref64[:, :, j]) for j in range(3))  # noqa: E731
    for j, nm in enumerate(('dq', 'dk', 'dv')):
        print(f'  {nm}: e_ref {_rel(ref32[:, :, j], ref64[:, :, j]):.3e} e_hip {_rel(got[:, :, j], ref64[:, :, j]):.3e}')
    _check(f'attn_f32_bwd B={Bn} H={H} L={L} hd={hd}', worst(got), worst(ref32), worst(got16))


# ---------------------------------------------------------------------------------------------------------------------
# 3. elementwise and reduction kernels

def _ln_mod(x, shift, scale, rows):
    xn = F.layer_norm(x, x.shape[-1:], eps=1e-6)
    return xn * (1 + scale.repeat_interleave(rows, 0)) + shift.repeat_interleave(rows, 0)


@pytest.mark.parametrize('W', [384, 512])
def test_ln_modulate_and_gate_bwd_vs_autograd_fp64(W):
    Bn, rows = 3, 64
    Mr = Bn * rows
    g = torch.Generator().manual_seed(W)
    x, dxn = torch.randn(Mr, W, generator=g) * 1.5 + 0.3, torch.randn(Mr, W, generator=g)
    mod = torch.randn(Bn, 3 * W + 4, generator=g) * 0.5  # shift | scale | gate at a pitch that is not 3 W
    dx0 = torch.randn(Mr, W, generator=g)

    def ln_ref(dt):
        xs, sh, sc = (t.to(dt).clone().requires_grad_(True) for t in (x, mod[:, :W], mod[:, W:2 * W]))
        _ln_mod(xs, sh, sc, rows).backward(dxn.to(dt))
        return [xs.grad + dx0.to(dt), sh.grad, sc.grad]

    r64, r32 = ln_ref(torch.float64), ln_ref(torch.float32)
    xd, dd, md = x.to(DEV), dxn.to(DEV), mod.to(DEV)
    ld = mod.shape[1]
    runs = []
    for rep in range(2):
        dx = dx0.to(DEV).clone()
        dmod = torch.full((Bn, ld), 9.0, device=DEV)
        stats = torch.empty(2 * Mr, device=DEV)
        _lib.call('mdt_ln_modulate_bwd_f32', dd.data_ptr(), xd.data_ptr(), md.data_ptr() + 4 * W, ld, rows, dx.data_ptr(), 1,
                  dmod.data_ptr(), dmod.data_ptr() + 4 * W, ld, stats.data_ptr(), Mr, W, _st())
        torch.cuda.synchronize()
        runs.append([dx.cpu(), dmod[:, :W].cpu(), dmod[:, W:2 * W].cpu()])
        assert bool((dmod[:, 2 * W:] == 9.0).all())
    assert all(torch.equal(a, b) for a, b in zip(*runs)), 'per-sample reductions differ between two runs'
    # bf16 route: mdt_ln_modulate_fwd (statistics) + mdt_ln_modulate_bwd
    xn16, st = torch.empty(Mr, W, device=DEV, dtype=torch.bfloat16), torch.empty(2 * Mr, device=DEV)
    _lib.call('mdt_ln_modulate_fwd', xd.data_ptr(), md.data_ptr(), md.data_ptr() + 4 * W, ld, rows, xn16.data_ptr(), st.data_ptr(), Mr, W, _st())
    dx16, dm16, d16 = dx0.to(DEV).clone(), torch.zeros(Bn, ld, device=DEV), dd.bfloat16()
    _lib.call('mdt_ln_modulate_bwd', d16.data_ptr(), xd.data_ptr(), st.data_ptr(), md.data_ptr() + 4 * W, ld, rows, dx16.data_ptr(), 1,
              dm16.data_ptr(), dm16.data_ptr() + 4 * W, ld, Mr, W, _st())
    torch.cuda.synchronize()
    b16 = [dx16.cpu(), dm16[:, :W].cpu(), dm16[:, W:2 * W].cpu()]
    worst = lambda r: max(_rel(a, b) for a, b in zip(r, r64))  # noqa: E731
    _check(f'ln_modulate_bwd_f32 W={W}', worst(runs[0]), worst(r32), worst(b16))

    # gate backward: y = x + gate * f
    f = torch.randn(Mr, W, generator=g)

    def gate_ref(dt):
        fs, gs = f.to(dt).clone().requires_grad_(True), mod[:, 2 * W:3 * W].to(dt).clone().requires_grad_(True)
        (gs.repeat_interleave(rows, 0) * fs).backward(dxn.to(dt))
        return [fs.grad, gs.grad]

    g64, g32 = gate_ref(torch.float64), gate_ref(torch.float32)
    fd = f.to(DEV)
    runs = []
    for rep in range(2):
        df, dmod = torch.empty(Mr, W, device=DEV), torch.full((Bn, ld), 9.0, device=DEV)
        _lib.call('mdt_gate_bwd_f32', dd.data_ptr(), fd.data_ptr(), md.data_ptr() + 8 * W, ld, rows, df.data_ptr(),
                  dmod.data_ptr() + 8 * W, ld, Mr, W, _st())
        torch.cuda.synchronize()
        runs.append([df.cpu(), dmod[:, 2 * W:3 * W].cpu()])
        assert bool((dmod[:, :2 * W] == 9.0).all()) and bool((dmod[:, 3 * W:] == 9.0).all())
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    dys, dg16, db16 = torch.empty(Mr, W, device=DEV, dtype=torch.bfloat16), torch.zeros(Bn, ld, device=DEV), torch.zeros(W, device=DEV)
    f16 = fd.bfloat16()
    _lib.call('mdt_gate_bwd', dd.data_ptr(), f16.data_ptr(), md.data_ptr() + 8 * W, ld, rows, dys.data_ptr(), dg16.data_ptr() + 8 * W, ld,
              db16.data_ptr(), Mr, W, _st())
    torch.cuda.synchronize()
    worst = lambda r: max(_rel(a, b) for a, b in zip(r, g64))  # noqa: E731
    _check(f'gate_bwd_f32 W={W}', worst(runs[0]), worst(g32), worst([dys.float().cpu(), dg16[:, 2 * W:3 * W].cpu()]))


def test_gelu_and_silu_bwd_vs_autograd_fp64():
    rows = 37
    n = rows * 128  # 18.5 blocks of 256 threads
    g = torch.Generator().manual_seed(5)
    x, dy = torch.randn(n, generator=g) * 2, torch.randn(n, generator=g)

    def ref(fn, dt):
        xs = x.to(dt).clone().requires_grad_(True)
        fn(xs).backward(dy.to(dt))
        return xs.grad

    gelu = lambda t: F.gelu(t, approximate='tanh')  # noqa: E731
    xd, dd = x.to(DEV), dy.to(DEV)
    out = torch.full((n + 64,), 3.0, device=DEV)
    _lib.call('mdt_gelu_bwd_f32', dd.data_ptr(), xd.data_ptr(), out.data_ptr(), n, _st())
    # bf16 route: the DGELU epilogue of mdt_gemm_nt on dy times an identity
    eye = torch.eye(128, device=DEV, dtype=torch.bfloat16)
    d16, x16, o16 = dd.bfloat16().view(rows, 128).contiguous(), xd.bfloat16().view(rows, 128).contiguous(), \
        torch.empty(rows, 128, device=DEV, dtype=torch.bfloat16)
    a = GemmNTArgs()
    a.A, a.lda, a.B, a.ldb, a.M, a.N, a.K = d16.data_ptr(), 128, eye.data_ptr(), 128, rows, 128, 128
    a.epi, a.out, a.ldo, a.aux, a.ldaux, a.rows_per_sample = _lib.EPI_DGELU, o16.data_ptr(), 128, x16.data_ptr(), 128, 1
    _lib.call('mdt_gemm_nt', C.byref(a), _st())
    torch.cuda.synchronize()
    assert bool((out[n:] == 3.0).all())
    r64 = ref(gelu, torch.float64)
    _check('gelu_bwd_f32', _rel(out[:n], r64), _rel(ref(gelu, torch.float32), r64), _rel(o16.float().flatten(), r64))
    # forward GELU and the gate + residual pass of the training forward, against torch fp32 (same criterion, no bf16 sibling)
    go = torch.empty(n, device=DEV)
    _lib.call('mdt_gelu_f32', xd.data_ptr(), go.data_ptr(), n, _st())
    torch.cuda.synchronize()
    assert _rel(go, gelu(x.double())) <= 4 * _rel(gelu(x), gelu(x.double()))
    out = torch.full((n + 64,), 3.0, device=DEV)
    _lib.call('mdt_silu_bwd_f32', dd.data_ptr(), xd.data_ptr(), out.data_ptr(), n, _st())
    s16 = torch.empty(n, device=DEV, dtype=torch.bfloat16)
    _lib.call('mdt_silu_bwd', dd.data_ptr(), xd.data_ptr(), s16.data_ptr(), n, _st())
    torch.cuda.synchronize()
    assert bool((out[n:] == 3.0).all())
    r64 = ref(F.silu, torch.float64)
    _check('silu_bwd_f32', _rel(out[:n], r64), _rel(ref(F.silu, torch.float32), r64), _rel(s16.float(), r64))


# ---------------------------------------------------------------------------------------------------------------------
# 4. - 6. end to end

def _setup(R, Bn, seed=3):
    cfg = O.make_cfg('DiT-S/2', img_resolution=R)
    P = O.init_params(cfg, seed=seed, dezero=True)
    net = M.Precond_models['edm'](img_resolution=R, img_channels=4, num_classes=1000, model_type='DiT-S/2', use_decoder=True,
                                  mae_loss_coef=0.1, pad_cls_token=False).to(DEV)
    net.load_state_dict(P, strict=True)
    net.train()
    g = torch.Generator().manual_seed(seed + 1)
    images = torch.randn(Bn, 4, R, R, generator=g) * 0.5
    labels = torch.zeros(Bn, 1000)
    labels[torch.arange(Bn), torch.randint(0, 1000, (Bn,), generator=g)] = 1
    labels[0] = 0  # a dropped class label
    rnd, noise = torch.randn(Bn, 1, 1, 1, generator=g), torch.randn(Bn, 4, R, R, generator=g)
    return cfg, P, net, (images, labels, rnd, noise)


def _hip_loss(net, inp):
    return M.Losses['edm']().with_draws(net, *(t.to(DEV) for t in inp), None, mae_loss_coef=0.1)


def _temb_in_dtype(t, dim=256, max_period=10000):
    """O.timestep_embedding in the dtype of t: the oracle's own casts its argument to float32, which an fp64 evaluation of
    the rest of the graph cannot consume (F.linear refuses mixed dtypes) -- and an fp64 reference wants it in fp64 anyway."""
    half = dim // 2
    freqs = torch.exp(-math.log(max_period) * torch.arange(half, dtype=t.dtype) / half)
    args = t[:, None] * freqs[None]
    return torch.cat([torch.cos(args), torch.sin(args)], dim=-1)


def _in_dtype(dt, fn, *a, **k):
    """fn(*a) with the oracle's timestep embedding in fp64 when dt is fp64; the fp32 evaluation is the oracle as it stands"""
    if dt != torch.float64:
        return fn(*a, **k)
    keep = O.timestep_embedding
    O.timestep_embedding = _temb_in_dtype
    try:
        return fn(*a, **k)
    finally:
        O.timestep_embedding = keep


def _oracle(P, cfg, inp, dt):
    Pd = {k: v.to(dt) for k, v in P.items()}
    loss, _, grads = _in_dtype(dt, O.loss_and_grads, Pd, cfg, *(t.to(dt) for t in inp), None, 0.1)
    return loss, grads


def _worst(loss, grads, loss64, grads64):
    e = {k: _rel(grads[k], grads64[k]) for k in grads64 if grads64[k].norm() > 0}
    k = max(e, key=e.get)
    print('   worst five: ' + ', '.join(f'{n} {e[n]:.2e}' for n in sorted(e, key=e.get, reverse=True)[:5]))
    return max(e[k], _rel(loss, loss64)), k


@pytest.mark.parametrize('R,Bn', [(16, 4), (32, 2)])
def test_end_to_end_loss_grads_step_vs_oracle(R, Bn):
    """Tests 4 and 5: the four losses and every parameter gradient of an unmasked fp32 step against the oracle in fp64 /
    fp32, autograd semantics of the arena, then FusedAdam.step() + EMA and a following fp32 eval forward (T = 64 with the
    fused L = 64 attention forward; T = 256 for the L = 256 attention inside the plan)."""
    cfg, P, net, inp = _setup(R, Bn)
    loss64, grads64 = _oracle(P, cfg, inp, torch.float64)
    loss32, grads32 = _oracle(P, cfg, inp, torch.float32)
    # the bf16 route on the same inputs (default train precision)
    net16 = copy.deepcopy(net)
    l16 = _hip_loss(net16, inp)
    l16.mean().backward()
    g16 = {k: p.grad.detach().cpu() for k, p in net16.named_parameters() if p.grad is not None}
    del net16
    net.set_train_precision('fp32')
    ema = copy.deepcopy(net)
    assert ema.train_precision == 'fp32'
    for p in ema.parameters():
        p.requires_grad_(False)
    opt = M.FusedAdam(net.parameters(), lr=1e-4, adam_w_mode=True, weight_decay=0)
    opt.zero_grad(set_to_none=True)
    loss = _hip_loss(net, inp)
    loss.mean().backward()
    eng = net.engine()
    assert (Bn, False, True, None, 'fp32') in eng._plans and (Bn, False, True, None) not in eng._plans
    params = dict(net.named_parameters())
    gh = {k: params[k].grad.detach().cpu().clone() for k in grads64}
    mt = params['model.mask_token'].grad
    assert mt is not None and bool((mt == 0).all()), 'mask_token must get a zero gradient, not None'
    e_hip, k_hip = _worst(loss, gh, loss64, grads64)
    e_ref, k_ref = _worst(loss32, grads32, loss64, grads64)
    e_bf16, _ = _worst(l16, g16, loss64, grads64)
    print(f'worst tensor: hip {k_hip}, oracle fp32 {k_ref}; loss e_hip {_rel(loss, loss64):.3e} e_ref {_rel(loss32, loss64):.3e}')
    _check(f'end to end T={(R // 2) ** 2} B={Bn}', e_hip, e_ref, e_bf16)
    # a second backward without zero_grad: gradients double
    loss2 = _hip_loss(net, inp)
    loss2.mean().backward()
    assert torch.equal(loss2, loss)
    for k in grads64:
        assert _rel(params[k].grad, 2 * gh[k].double()) <= 1e-6, k
    # ---- test 5: one optimizer step (on the doubled gradients) + EMA against the oracle's update rules
    g2 = {k: params[k].grad.detach().cpu().clone() for k in grads64}
    p0 = {k: params[k].detach().cpu().clone() for k in grads64}
    opt.fuse_ema(ema, 0.9999)
    opt.step()
    M.update_ema(ema, net, 0.9999)
    ep = dict(ema.named_parameters())
    P1 = dict(P)
    errs = {'p32': 0.0, 'hip': 0.0, 'ema32': 0.0, 'emahip': 0.0}
    for k in grads64:
        ref = {}
        for dt in (torch.float64, torch.float32):
            p, m, v = p0[k].to(dt).clone(), torch.zeros_like(p0[k], dtype=dt), torch.zeros_like(p0[k], dtype=dt)  # (adamw_step is in place)
            e = p.clone()
            O.adamw_step(p, g2[k].to(dt), m, v, step=1, lr=1e-4)
            O.ema_update(e, p, 0.9999)
            ref[dt] = (p, e)
        P1[k] = params[k].detach().cpu().clone()
        # the UPDATE (p1 - p0) is what the step computes (the parameters themselves agree to lr * 2^-24 trivially); a tensor
        # without gradient (mask_token) is not updated at all.  The EMA moves by 1e-4 of that, below one fp32 ulp of the
        # parameter, so it is compared as a value.
        assert torch.equal(P1[k], p0[k]) == (float(g2[k].abs().max()) == 0), k
        if float(g2[k].abs().max()) > 0:
            d64 = ref[torch.float64][0] - p0[k].double()
            errs['p32'] = max(errs['p32'], _rel(ref[torch.float32][0].double() - p0[k].double(), d64))
            errs['hip'] = max(errs['hip'], _rel(P1[k].double() - p0[k].double(), d64))
        errs['ema32'] = max(errs['ema32'], _rel(ref[torch.float32][1], ref[torch.float64][1]))
        errs['emahip'] = max(errs['emahip'], _rel(ep[k], ref[torch.float64][1]))
    print(f'optimizer step: update e_ref {errs["p32"]:.3e} e_hip {errs["hip"]:.3e}; ema e_ref {errs["ema32"]:.3e} e_hip {errs["emahip"]:.3e}')
    assert errs['hip'] <= 4 * errs['p32'] and errs['emahip'] <= 4 * errs['ema32']
    # a following fp32 eval forward reads the updated master weights
    net.eval()
    images, labels, rnd, noise = inp
    sigma = (rnd * 1.2 - 1.2).exp().flatten()
    x = images + noise * sigma.view(-1, 1, 1, 1)
    net.set_eval_precision('fp32')
    with torch.no_grad():
        D = net(x.to(DEV), sigma.to(DEV), labels.to(DEV))['x'].cpu()
    D64 = _in_dtype(torch.float64, O.precond_forward, {k: v.double() for k, v in P1.items()}, cfg, x.double(), sigma.double(),
                    labels.double(), training=False)
    D32 = O.precond_forward(P1, cfg, x, sigma, labels, training=False)
    Dold = _in_dtype(torch.float64, O.precond_forward, {k: v.double() for k, v in P.items()}, cfg, x.double(), sigma.double(),
                     labels.double(), training=False)
    print(f'eval forward after the step: e_ref {_rel(D32, D64):.3e} e_hip {_rel(D, D64):.3e}; stale weights would give {_rel(Dold, D64):.3e}')
    assert _rel(D, D64) <= 4 * _rel(D32, D64)
    assert _rel(D, D64) < _rel(Dold, D64) / 10, 'the eval forward did not read the updated master weights'


def test_refusals_and_default_route_unchanged():
    """Test 6.  The default route: a loss call at mask_ratio 0 with the default train precision IS the bf16 route -- the same
    cached PassPlan object with the same launch lists before and after a detour through 'fp32', and a bit-identical loss.
    The GRADIENTS of the bf16 route are not bit-reproducible against themselves: its weight- and bias-gradient kernels
    (mdt_gemm_tn, mdt_colsum_bf16, ...) accumulate with fp32 atomics, and two direct runs of that route already differ in
    the last bits (measured on an MI355X: model.blocks.0.attn.qkv.bias).  So gradients are compared to the bound of that
    effect: both runs add the same <= 2^10 fp32 partial sums per element in another order, each addition rounding by at
    most 2^-24 of the running sum, which bounds the relative L2 difference of a tensor by 2^10 * 2^-24 = 2^-14 times the
    cancellation of its sums; 1e-5 is asserted (tighter than that bound, 400 times below one bf16 rounding)."""
    cfg, P, net, inp = _setup(16, 4)
    eng = net.engine()
    loss_a = _hip_loss(net, inp)
    loss_a.mean().backward()
    ga = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
    assert list(eng._plans) == [(4, False, True, None)]
    pl = eng._plans[(4, False, True, None)]
    launches = [c[2] for c in pl.fwd.calls + pl.bwd.calls]
    net.set_train_precision('fp32')
    with pytest.raises(NotImplementedError, match='UNMASKED'):
        M.Losses['edm']()(net, inp[0].to(DEV), inp[1].to(DEV), mask_ratio=0.5, mae_loss_coef=0.1)
    md = M.get_mask(4, 64, 0.5, DEV)
    with pytest.raises(NotImplementedError, match='UNMASKED'):
        M.Losses['edm']().with_draws(net, *(t.to(DEV) for t in inp), md, mae_loss_coef=0.1)
    with pytest.raises(NotImplementedError):
        eng.plan(4, True, True, 32, 'fp32')
    with pytest.raises(NotImplementedError):
        eng.plan(4, False, True, None, 'bf16x3')
    with pytest.raises(ValueError):
        net.set_train_precision('tf32')
    net.set_train_precision('bf16')
    for p in net.parameters():
        p.grad = None
    loss_b = _hip_loss(net, inp)
    loss_b.mean().backward()
    assert eng._plans[(4, False, True, None)] is pl and [c[2] for c in pl.fwd.calls + pl.bwd.calls] == launches
    assert not any(len(k) == 5 for k in eng._plans), 'an fp32 plan was built on the default route'
    assert torch.equal(loss_a, loss_b)
    for k, p in net.named_parameters():
        if k in ga:
            assert _rel(p.grad, ga[k]) <= 1e-5, k
