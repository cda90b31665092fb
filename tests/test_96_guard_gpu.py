"""The guard around the fused optimizer step on the GPU: the ordered fp64 sum of squares, the skip of a
step with a non-finite gradient (what the reference's GradScaler did, train.py:39-50,226), clipping by global norm
(torch's clip_grad_norm_ formula), the per-tensor and the ZeRO-1 routes, train.py's flags -- and that the default route
issues exactly the library calls it issued before.

Model: DiT-S/2 at img_resolution 16, batch 4; ONE real backward gives the gradient arena every optimizer twin is fed
(copying it keeps the twins' inputs bit-identical; a second backward would differ by atomics noise).

fp64 references take Adam's betas as the float32 values the C ABI carries (0.9f, 0.999f): 1 - 0.999 differs from
1 - 0.999f by 1.3e-5, which has nothing to do with the guard, while 1 - beta is exact in float32 for a float32 beta."""
import copy
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEV = 'cuda:0'
LR, DECAY = 1e-3, 0.99
B1F, B2F = float(np.float32(0.9)), float(np.float32(0.999))
BAD_KEY = 'model.blocks.5.mlp.fc1.weight'
NEW_ENTRIES = ('mdt_grad_sumsq', 'mdt_guard_decide', 'mdt_adamw_ema_step_guarded')


# ------------------------------------------------------------------------------------------------ 1. sumsq
def _guard_state():
    from maskdit_amd.guard import GuardState
    return GuardState(torch.device(DEV))


def _sumsq(gs, g, accumulate=False):
    from maskdit_amd.optim import _st
    if not accumulate:
        gs.begin()
    gs.sumsq(g.data_ptr(), g.numel(), 1.0, _st())
    return gs.sum_flag.clone()


def _sizes():
    from maskdit_amd import _lib
    chunk = int(_lib.lib().mdt_grad_sumsq_chunk(4096))
    assert chunk == int(_lib.lib().mdt_grad_sumsq_chunk(3 * chunk + 5))  # the chunk length of every size below
    return chunk, [1, 7, 4096, 4099, 1_000_003, 5_000_011, 3 * chunk - 1, 3 * chunk, 3 * chunk + 5]


def test_sumsq_against_fp64():
    gs = _guard_state()
    chunk, sizes = _sizes()
    gen = torch.Generator(device=DEV).manual_seed(3)
    for n in sizes:
        base = torch.randn(n, device=DEV, generator=gen)
        for scale in (1e-3, 1e18):
            g = base * scale
            a = _sumsq(gs, g)
            b = _sumsq(gs, g)
            assert torch.equal(a, b), f'n={n} scale={scale}: two launches differ'
            ref = g.double().norm().item()
            got = math.sqrt(a[0].item())
            rel = abs(got - ref) / ref
            print(f'sumsq n={n} scale={scale:g}: rel err {rel:.2e}, flag {a[1].item()}')
            assert math.isfinite(got) and a[1].item() == 0
            assert rel <= 1e-9, f'n={n} scale={scale}: {rel:.3e}'
            if n >= 4096:  # three 16-byte-aligned sub-ranges form one norm
                c1, c2 = (n // 3) // 4 * 4, (2 * n // 3) // 4 * 4
                _sumsq(gs, g[:c1])
                _sumsq(gs, g[c1:c2], accumulate=True)
                acc = _sumsq(gs, g[c2:], accumulate=True)
                rel = abs(math.sqrt(acc[0].item()) - ref) / ref
                assert rel <= 1e-9 and acc[1].item() == 0, f'n={n} scale={scale}: accumulate {rel:.3e}'


def test_sumsq_nonfinite_flag():
    gs = _guard_state()
    chunk, _ = _sizes()
    gen = torch.Generator(device=DEV).manual_seed(4)
    for n in (7, 4099, 3 * chunk + 5):  # (n % 4 = 3, 3, 1: the last index sits in the scalar tail)
        base = torch.randn(n, device=DEV, generator=gen) * 1e-3
        for bad in (float('inf'), float('-inf'), float('nan')):
            for idx in (0, n // 2, n - 1):
                g = base.clone()
                g[idx] = bad
                a = _sumsq(gs, g)
                assert a[1].item() != 0 and not math.isfinite(a[0].item()), f'n={n} {bad} at {idx}: not flagged'
        a = _sumsq(gs, base)
        assert a[1].item() == 0  # (the flag does not stick)
    big = torch.full((4099,), 3e38, device=DEV)
    a = _sumsq(gs, big)
    assert a[1].item() == 0 and math.isfinite(a[0].item())
    assert abs(math.sqrt(a[0].item()) - big.double().norm().item()) <= 1e-9 * big.double().norm().item()


# ------------------------------------------------------------------------------------------------ model twins
def _build(P0):
    import maskdit_amd as M
    net = M.Precond_models['edm'](img_resolution=16, img_channels=4, num_classes=1000, model_type='DiT-S/2',
                                  use_decoder=True, mae_loss_coef=0.1, pad_cls_token=False).to(DEV)
    net.load_state_dict(P0)
    return net.train()


@pytest.fixture(scope='module')
def base():
    """(P0, G0): initial parameters and the gradient arena of ONE real backward (never modified afterwards)."""
    import maskdit_amd as M
    from oracle import maskdit_oracle as O
    P0 = O.init_params(O.make_cfg('DiT-S/2', img_resolution=16), seed=0, dezero=True)
    net = _build(P0)
    g = torch.Generator().manual_seed(7)
    x = 0.5 * torch.randn(4, 4, 16, 16, generator=g)
    y = torch.zeros(4, 1000)
    y[torch.arange(4), torch.randint(0, 1000, (4,), generator=g)] = 1
    torch.manual_seed(11)
    M.Losses['edm']()(net, x.to(DEV), y.to(DEV), mask_ratio=0.5, mae_loss_coef=0.1).mean().backward()
    G0 = net.engine().G.detach().clone()
    assert bool(torch.isfinite(G0).all()) and G0.abs().max().item() > 0
    return P0, G0


class Twin:
    def __init__(self, base, cls=None, **kw):
        import maskdit_amd as M
        P0, G0 = base
        self.net = _build(P0)
        self.ema = copy.deepcopy(self.net).eval()
        self.ema.engine().P.mul_(0.5)  # (an EMA equal to the model would make d * ema + (1 - d) * p a trivial check)
        self.opt = (cls or M.FusedAdam)(self.net.parameters(), lr=LR, **kw)
        self.opt.fuse_ema(self.ema, DECAY)
        self.feed(G0)

    def feed(self, G):
        self.net._prepare_grad_arena()
        self.net.engine().G.copy_(G)

    def arenas(self):
        eng = self.net.engine()
        return {'p': eng.P.detach(), 'm': self.opt._m, 'v': self.opt._v, 'ema': self.ema.engine().P.detach(), 'w16': eng.W16}

    def snapshot(self):
        return {k: a.clone() for k, a in self.arenas().items()}

    def step(self):
        import maskdit_amd as M
        self.opt.step()
        M.update_ema(self.ema, self.net, DECAY)

    def named(self, flat):
        eng = self.net.engine()
        return {k: eng.view(flat, k) for k, _ in self.net.named_parameters() if k in eng.lay.off}


def _rel_l2_per_tensor(got: dict, ref: dict, bound: float, what: str):
    worst = 0.0
    for k, r in ref.items():
        num = (got[k].double() - r.double()).norm().item()
        den = r.double().norm().item()
        worst = max(worst, num / den if den > 0 else (0.0 if num == 0 else float('inf')))
        assert num <= bound * den, f'{what} {k}: rel L2 {num / (den + 1e-300):.3e} > {bound:g}'
    return worst


def _assert_same_bits(a: dict, b: dict, keys, what):
    for k in keys:
        assert torch.equal(a[k], b[k]), f'{what}: arena {k} differs ({(a[k].float() - b[k].float()).abs().max().item():.3e})'


# ------------------------------------------------------------------------------------------------ 2. skip
@pytest.mark.parametrize('bad', [float('inf'), float('nan')], ids=['inf', 'nan'])
def test_skip_leaves_everything_but_the_ema(base, bad):
    P0, G0 = base
    t = Twin(base, skip_nonfinite=True)
    before = t.snapshot()
    dict(t.net.named_parameters())[BAD_KEY].grad.view(-1)[5] = bad
    t.step()
    after = t.snapshot()
    _assert_same_bits(after, before, ('p', 'm', 'v', 'w16'), 'skipped step')
    ref = DECAY * before['ema'].double() + (1 - DECAY) * before['p'].double()
    r32 = ref.float().abs()
    ulp = torch.nextafter(r32, torch.full_like(r32, float('inf'))) - r32
    err = (after['ema'].double() - ref).abs()
    print('skip: EMA error in ulp, max', (err / ulp.double()).max().item())
    assert bool((err <= 2 * ulp.double()).all())
    assert not torch.equal(after['ema'], before['ema'])
    assert t.opt.skipped_steps == 1
    assert t.opt.state_dict()['param_groups'][0]['step'] == 0
    for k, a in after.items():
        assert bool(torch.isfinite(a.float()).all()), f'arena {k} is not finite after the skipped step'
    # ---- the same gradient with the element restored: the update of a twin that never saw the bad step
    t.feed(G0)
    t.step()
    u = Twin(base)
    u.step()
    p0 = before['p']
    worst = _rel_l2_per_tensor(t.named(t.arenas()['p'] - p0), u.named(u.arenas()['p'] - p0), 1e-6, 'update after a skip')
    print('skip: update vs never-skipped twin, worst per-tensor rel L2', worst)
    assert t.opt.state_dict()['param_groups'][0]['step'] == 1 and u.opt.state_dict()['param_groups'][0]['step'] == 1
    assert t.opt.skipped_steps == 1 and t.opt.param_groups[0]['step'] == 1


# ------------------------------------------------------------------------------------------------ 3. clip
@pytest.fixture(scope='module')
def clipped(base):
    """N measured under a huge max_grad_norm (with that twin's arenas), the clip-only twin after one step with
    max_grad_norm = N / 2, and the fp64 references of its moments."""
    P0, G0 = base
    t = Twin(base, max_grad_norm=1e30)
    t.step()
    N = t.opt.grad_norm.item()
    c = Twin(base, max_grad_norm=N / 2)
    c.step()
    coef = (N / 2) / (N + 1e-6)
    g = G0.double()
    return {'N': N, 'huge': t.snapshot(), 'c': c, 'ref': {'m': (1 - B1F) * coef * g, 'v': (1 - B2F) * coef * coef * g * g}}


def test_clip_norm_and_moments(base, clipped):
    import maskdit_amd as M
    P0, G0 = base
    N, c, ref = clipped['N'], clipped['c'], clipped['ref']
    N64 = G0.double().norm().item()
    print(f'clip: grad_norm {N:.9g} vs fp64 {N64:.9g} (rel {abs(N - N64) / N64:.2e})')
    assert abs(N - N64) <= 1e-6 * N64
    u = Twin(base)
    u.step()
    _assert_same_bits(clipped['huge'], u.snapshot(), ('p', 'm', 'v', 'ema', 'w16'), 'huge max_grad_norm (coef == 1) vs unguarded')
    assert not torch.equal(c.opt._m, u.opt._m), 'max_grad_norm = N / 2 left the first moment unclipped'
    assert abs(c.opt.grad_norm.item() - N64) <= 1e-6 * N64  # (the PRE-clip norm)
    sd = c.opt.state_dict()
    names = [k for k, _ in c.net.named_parameters()]
    got_m = {names[i]: s['exp_avg'].reshape(-1) for i, s in sd['state'].items()}
    got_v = {names[i]: s['exp_avg_sq'].reshape(-1) for i, s in sd['state'].items()}
    wm = _rel_l2_per_tensor(got_m, {k: v.reshape(-1) for k, v in c.named(ref['m']).items()}, 1e-6, 'exp_avg')
    wv = _rel_l2_per_tensor(got_v, {k: v.reshape(-1) for k, v in c.named(ref['v']).items()}, 1e-6, 'exp_avg_sq')
    print(f'clip: worst per-tensor rel L2, exp_avg {wm:.2e}  exp_avg_sq {wv:.2e}')
    assert sd['param_groups'][0]['step'] == 1 and c.opt.skipped_steps == 0
    # for context only: torch's clip_grad_norm_ + the unguarded step against the same fp64 values
    e = Twin(base)
    torch.nn.utils.clip_grad_norm_([p for p in e.net.parameters() if p.grad is not None], N / 2)
    e.step()
    em = ((e.opt._m.double() - ref['m']).norm() / ref['m'].norm()).item()
    ev = ((e.opt._v.double() - ref['v']).norm() / ref['v'].norm()).item()
    print(f'clip: torch clip_grad_norm_ + unguarded step, arena rel L2: exp_avg {em:.2e}  exp_avg_sq {ev:.2e}')


# ------------------------------------------------------------------------------------------------ 4. both / per tensor
def test_both_guards_equal_clip_alone(base, clipped):
    N, c = clipped['N'], clipped['c']
    b = Twin(base, max_grad_norm=N / 2, skip_nonfinite=True)
    b.step()
    _assert_same_bits(b.snapshot(), c.snapshot(), ('p', 'm', 'v', 'ema', 'w16'), 'both guards vs clip alone')
    assert b.opt.skipped_steps == 0 and b.opt.param_groups[0]['step'] == 1
    assert torch.equal(b.opt.grad_norm, c.opt.grad_norm)


def test_per_tensor_path(base):
    import maskdit_amd as M
    P0, G0 = base
    net = _build(P0)
    net._prepare_grad_arena()
    net.engine().G.copy_(G0)
    sub = [(k, p) for k, p in net.named_parameters() if 'blocks.5.' in k or 'final_layer' in k]
    assert 2 < len(sub) < sum(1 for _ in net.parameters())
    opt = M.FusedAdam([p for _, p in sub], lr=LR, max_grad_norm=1e30, skip_nonfinite=True)
    assert opt._arena is None
    opt.step()
    N64 = math.sqrt(sum(p.grad.double().pow(2).sum().item() for _, p in sub))
    N = opt.grad_norm.item()
    print(f'per-tensor: grad_norm {N:.9g} vs fp64 norm of the subset {N64:.9g}')
    assert N64 > 0 and abs(N - N64) <= 1e-6 * N64
    assert opt.skipped_steps == 0 and opt.param_groups[0]['step'] == 1
    assert any(not torch.equal(p.detach().cpu(), P0[k]) for k, p in sub), 'the applied per-tensor step moved nothing'
    before = [(p.detach().clone(), opt.state[p]['exp_avg'].clone(), opt.state[p]['exp_avg_sq'].clone()) for _, p in sub]
    sub[1][1].grad.view(-1)[0] = float('inf')
    opt.step()
    for (k, p), (p0, m0, v0) in zip(sub, before):
        assert torch.equal(p.detach(), p0) and torch.equal(opt.state[p]['exp_avg'], m0) and torch.equal(opt.state[p]['exp_avg_sq'], v0), k
    assert opt.skipped_steps == 1 and opt.param_groups[0]['step'] == 1


# ------------------------------------------------------------------------------------------------ 5. default route
def test_default_route_is_unchanged(base, monkeypatch):
    import maskdit_amd as M
    from maskdit_amd import optim as OPT
    names = []
    real = OPT.call

    def recording(name, *a):
        names.append(name)
        return real(name, *a)

    monkeypatch.setattr(OPT, 'call', recording)
    a = Twin(base)
    a.step()
    z = Twin(base, cls=M.ShardedFusedAdam)
    assert z.opt.world == 1
    z.step()
    assert names.count('mdt_adamw_ema_step') >= 2 and not set(names) & set(NEW_ENTRIES), names
    assert a.opt._guard is None and z.opt._guard is None and a.opt.grad_norm is None and a.opt.skipped_steps == 0
    _assert_same_bits(a.snapshot(), z.snapshot(), ('p', 'm', 'v', 'ema', 'w16'), 'ShardedFusedAdam at world 1')
    monkeypatch.undo()
    P0, G0 = base
    first = Twin(base)                  # built before ...
    import maskdit_amd.guard  # noqa: F401  ... the guard module is (certainly) imported
    second = Twin(base)
    for _ in range(3):
        for t in (first, second):
            t.feed(G0)
            t.step()
    _assert_same_bits(first.snapshot(), second.snapshot(), ('p', 'm', 'v', 'ema', 'w16'), 'three unguarded steps')
    assert first.opt.param_groups[0]['step'] == 3


# ------------------------------------------------------------------------------------------------ 6. ZeRO-1
def _zero_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        import maskdit_amd as M
        from oracle import maskdit_oracle as O
        P0 = O.init_params(O.make_cfg('DiT-S/2', img_resolution=16), seed=0, dezero=True)
        net = _build(P0)
        dp = M.DataParallel(net)
        plain = M.ShardedFusedAdam(net.parameters(), data_parallel=dp, lr=LR)  # (switches the reducer to reduce-scatter)
        g = torch.Generator().manual_seed(7)
        x = 0.5 * torch.randn(4, 4, 16, 16, generator=g)
        y = torch.zeros(4, 1000)
        y[torch.arange(4), torch.randint(0, 1000, (4,), generator=g)] = 1
        half = slice(2 * rank, 2 * rank + 2)
        torch.manual_seed(11 + rank)
        M.Losses['edm']()(dp, x[half].to(DEV), y[half].to(DEV), mask_ratio=0.5, mae_loss_coef=0.1).mean().backward()
        dp.finish_grad_sync()
        eng = net.engine()
        Gfull = eng.G.detach().clone()
        plain._gather(Gfull, eng.lay.slabs)  # the reduced gradient, assembled from its owners
        N64 = Gfull.double().norm().item()
        assert math.isfinite(N64) and N64 > 0
        opt = M.ShardedFusedAdam(net.parameters(), data_parallel=dp, lr=LR, max_grad_norm=N64 / 2, skip_nonfinite=True)
        ref = _build(P0)
        ropt = M.FusedAdam(ref.parameters(), lr=LR, max_grad_norm=N64 / 2, skip_nonfinite=True)
        ref._prepare_grad_arena()
        ref.engine().G.copy_(Gfull)
        P_start = eng.P.detach().clone()
        opt.step()
        ropt.step()
        n_sh, n_ref = opt.grad_norm.item(), ropt.grad_norm.item()
        assert abs(n_sh - n_ref) <= 1e-6 * n_ref and abs(n_ref - N64) <= 1e-6 * N64, (n_sh, n_ref, N64)
        relp = ((eng.P.double() - ref.engine().P.double()).norm() / ref.engine().P.double().norm()).item()
        assert relp <= 1e-6, f'sharded guarded parameters differ from the unsharded ones ({relp:.3e})'
        assert not torch.equal(eng.P.detach(), P_start), 'the applied sharded step moved nothing'
        assert opt.skipped_steps == 0 and ropt.skipped_steps == 0 and opt.param_groups[0]['step'] == 1
        # ---- an inf on rank 1 only, in an element rank 1 owns: BOTH ranks skip
        a, _ = opt._pieces[0]
        if rank == 1:
            eng.G[a] = float('inf')
        P_before = eng.P.detach().clone()
        opt.step()
        assert opt.skipped_steps == 1, f'rank {rank} did not skip'
        assert torch.equal(eng.P.detach(), P_before), f'rank {rank}: parameters changed in a skipped step'
        assert opt.param_groups[0]['step'] == 1
        q.put((rank, 'ok', relp))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, 'FAIL: ' + traceback.format_exc(), 0.0))
    finally:
        dist.destroy_process_group()


def _free_port() -> int:
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


@pytest.mark.timeout(300)
def test_zero1_guard_two_ranks():
    import queue
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_zero_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in procs:
            res.append(q.get(timeout=120))  # each child's own time limit
    except queue.Empty:
        pass
    for p in procs:
        p.join(30)
        if p.is_alive():
            p.kill()
            p.join(10)
    codes = [p.exitcode for p in procs]
    for r in res:
        if r[1] != 'ok':
            print(r[1])
    assert len(res) == 2 and all(r[1] == 'ok' for r in res), [r[1][-800:] for r in res]
    assert codes == [0, 0], codes
    print('ZeRO-1 guard: sharded vs unsharded parameters, rel L2', max(r[2] for r in res))


# ------------------------------------------------------------------------------------------------ 7. train.py
CFG = """
model: {precond: edm, model_type: DiT-S/2, in_size: 32, in_channels: 4, num_classes: 1000, use_decoder: true,
        pad_cls_token: false, ext_feature_dim: 0, mask_ratio: 0.5, mask_ratio_fn: constant, mask_ratio_min: 0.25,
        mae_loss_coef: 0.1, class_dropout_prob: 0.1}
train: {batchsize: 16, grad_accum: 2, lr: 1.0e-3, lr_rampup_kimg: 0, max_num_steps: 6}
data: {category: synthetic, resolution: 32, num_channels: 4, root: none}
log: {log_every: 2, ckpt_every: 100}
"""


def test_train_loop_with_and_without_the_flags(tmp_path):
    import train as T
    tmp = str(tmp_path)
    cfg = os.path.join(tmp, 'cfg.yaml')
    with open(cfg, 'w') as f:
        f.write(CFG)
    out = T.train_loop(T.parse(['--config', cfg, '--results_dir', tmp, '--exp_name', 'g', '--max_num_steps', '4',
                                '--max_grad_norm', '0.5', '--skip_nonfinite']))
    assert out['step'] == 4 and out['skipped'] == 0
    assert np.isfinite(out['loss']) and np.isfinite(out['grad_norm']) and out['grad_norm'] > 0
    assert out['opt'].state_dict()['param_groups'][0]['step'] == 4
    log = open(os.path.join(out['exp_dir'], 'log.txt')).read()
    assert 'Grad Norm: ' in log and 'Skipped: 0' in log
    out = T.train_loop(T.parse(['--config', cfg, '--results_dir', tmp, '--exp_name', 'p', '--max_num_steps', '2']))
    assert set(out) == {'net', 'ema', 'opt', 'step', 'loss', 'exp_dir', 'eval'} and out['step'] == 2
    assert out['opt']._guard is None
    assert 'Grad Norm' not in open(os.path.join(out['exp_dir'], 'log.txt')).read()
