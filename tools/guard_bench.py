"""Cost of the optimizer-step guard on XL/2, one process:  python tools/guard_bench.py [--out FILE]

  * `opt.step()` (kernel(s) + shadow refresh) unguarded, with clipping, with skipping, with both -- the four optimizers
    alternate round by round on the same model and gradient arena;
  * the step kernel alone and the `mdt_grad_sumsq` pass alone, in bytes per second;
  * two ratios against what the bytes predict: the pass reads 4 B per parameter beside the 38 B the step moves, so a
    guarded step should cost about 4 / 38 = 10.5 % more than the unguarded one, and a pure read has no reason to stream
    slower than the step kernel does in the same run.

Writes profiles/guard_bench.txt (first line: the command and the kernel-source hash)."""
import argparse
import copy
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import maskdit_amd as M  # noqa: E402
from maskdit_amd import _lib  # noqa: E402
from maskdit_amd._lib import call  # noqa: E402
from maskdit_amd.guard import GuardState  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'guard_bench.txt'))
ap.add_argument('--model', default='DiT-XL/2')
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--iters', type=int, default=5)
args = ap.parse_args()

dev = torch.device('cuda', 0)
net = M.Precond_models['edm'](img_resolution=32, img_channels=4, num_classes=1000, model_type=args.model).to(dev).train()
ema = copy.deepcopy(net).eval()
eng = net.engine()
n = eng.lay.n
net._prepare_grad_arena()
eng.G.normal_(0.0, 1e-3)
st = torch.cuda.current_stream().cuda_stream


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


opts = {'unguarded': {}, 'clip': dict(max_grad_norm=1.0), 'skip': dict(skip_nonfinite=True),
        'clip + skip': dict(max_grad_norm=1.0, skip_nonfinite=True)}
built = {}
for name, kw in opts.items():
    o = M.FusedAdam(net.parameters(), lr=1e-6, **kw)
    o.fuse_ema(ema, 0.9999)
    built[name] = o
m, v = built['unguarded']._m, built['unguarded']._v
gs = GuardState(dev)


def kernel_alone():
    call('mdt_adamw_ema_step', eng.P.data_ptr(), eng.G.data_ptr(), m.data_ptr(), v.data_ptr(), ema.engine().P.data_ptr(),
         eng.W16.data_ptr(), n, 1e-6, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.001, 0.9999, 1.0, st)


def sumsq_alone():
    gs.begin()
    gs.sumsq(eng.G.data_ptr(), n, 1.0, st)


fns = {k: o.step for k, o in built.items()}
fns['step kernel alone'] = kernel_alone
fns['sumsq pass alone'] = sumsq_alone
times = {k: [] for k in fns}
for k, f in fns.items():  # warm-up (guard state, workspace, shadow tables)
    timed(f, 2)
for _ in range(args.rounds):
    for k, f in fns.items():
        times[k].append(timed(f, args.iters))
med = {k: statistics.median(t) for k, t in times.items()}
spread = {k: (max(t) - min(t)) / statistics.median(t) for k, t in times.items()}

lines = [f'# python tools/guard_bench.py --model {args.model} --rounds {args.rounds} --iters {args.iters}   kernel-source hash {_lib.source_hash()}',
         f'# {torch.cuda.get_device_name(0)}; {sum(p.numel() for p in net.parameters()):,} parameters, arena of {n:,} fp32 elements; '
         f'median of {args.rounds} rounds x {args.iters} calls, the six measurements alternate round by round',
         f'{"":22s} {"ms":>9s} {"spread":>8s} {"vs unguarded":>13s}']
for k in built:
    lines.append(f'opt.step() {k:11s} {med[k]:9.3f} {100 * spread[k]:7.1f}% {med[k] / med["unguarded"]:13.3f}')
bw_step = 38.0 * n / med['step kernel alone'] / 1e9
bw_sum = 4.0 * n / med['sumsq pass alone'] / 1e9
lines += [f'{"step kernel alone":22s} {med["step kernel alone"]:9.3f} {100 * spread["step kernel alone"]:7.1f}%   38 B/param: {bw_step:.2f} TB/s',
          f'{"sumsq pass alone":22s} {med["sumsq pass alone"]:9.3f} {100 * spread["sumsq pass alone"]:7.1f}%    4 B/param: {bw_sum:.2f} TB/s '
          f'({int(_lib.lib().mdt_grad_sumsq_ws_floats(n)) // 2} chunks of {int(_lib.lib().mdt_grad_sumsq_chunk(n))})',
          f'ratio 1: guarded step / unguarded step = {med["clip + skip"] / med["unguarded"]:.3f} (clip + skip), '
          f'{med["clip"] / med["unguarded"]:.3f} (clip), {med["skip"] / med["unguarded"]:.3f} (skip); the bytes predict 1 + 4/38 = 1.105',
          f'ratio 2: sumsq bytes/s / step-kernel bytes/s = {bw_sum / bw_step:.3f} (expected >= 0.8)',
          f'grad norm {built["clip"].grad_norm.item():.6g} (fp64 torch: {eng.G.double().norm().item():.6g}), skipped {built["skip"].skipped_steps}']
text = '\n'.join(lines) + '\n'
print(text, end='')
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, 'w') as f:
    f.write(text)
