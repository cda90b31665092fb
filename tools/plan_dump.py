"""Launch lists of PassPlan as data: every entry of fwd.calls / bwd.calls with its arguments, every address resolved to
[buffer name, byte offset].  Plans are built on an Engine.host_listing engine, so no GPU is needed.

    python tools/plan_dump.py        re-records tests/golden/plan_lists.json.gz (tests/test_plan_lists_cpu.py compares a
                                     freshly built plan with it; re-record only when a launch list changes on purpose)
"""
import ctypes as C
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from maskdit_amd import engine as E  # noqa: E402

FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'plan_lists.json.gz')
ARENAS = ('P', 'G', 'W16', 'WT16', 'Wy16', 'pos', 'dpos')
# (model, latent side, batch, precision, masked, train, kept tokens)
PLAN_SET = [('DiT-S/2', 16, 2, prec, masked, train, 20 if masked else None) for prec, masked, train in
            [('fp32', False, False), ('bf16x3', False, False), ('fp32', False, True), ('bf16', True, True), ('bf16', False, True),
             ('bf16', False, False), ('bf16', True, False)]] + \
           [('DiT-S/4', 32, 1, 'fp32', False, True, None), ('DiT-S/4', 32, 1, 'bf16', True, True, 20)]


def plan_id(model, R, B, prec, masked, train, L):
    return f"{model} R{R} B{B} {prec} {'masked L%d' % L if masked else 'unmasked'} {'train' if train else 'eval'}"


def build_plan(model, R, B, prec, masked, train, L):
    """(listing engine, plan): the caller keeps the engine, a plan holds only a weak reference to it."""
    eng = E.Engine.host_listing(E.make_spec(model, R, 4, 1000))
    return eng, E.PassPlan(eng, B, masked, train, L, prec)


def plan_dump(pl):
    """JSON-able description of one PassPlan: launches, marks and buffers."""
    eng = pl.eng
    spans = [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), name) for name, t in
             list(pl.buf.items()) + [(a, getattr(eng, a)) for a in ARENAS if getattr(eng, a) is not None] if t.numel()]

    def value(v, ctype):
        if isinstance(v, C.c_int):  # (lv_arg / lv_attn: read at launch time)
            v = v.value
        if ctype is not C.c_void_p:
            if isinstance(v, int) and abs(v) > 2 ** 32:
                raise ValueError(f'{v:#x} was passed as a number: an address?')
            return v
        if not v:
            return None
        inside = [(hi - lo, name, v - lo) for lo, hi, name in spans if lo <= v < hi]
        if not inside:
            raise ValueError(f'address {v:#x} belongs to no plan buffer and to no engine arena')
        return list(min(inside)[1:])  # views nest (c_noise is a row of coef): the innermost, i.e. shortest, buffer names it

    def launch(fn, args, name):
        if fn is None:
            seen, hook = [], eng.grad_slab_hook
            eng.grad_slab_hook = lambda *a: seen.append(['slab', *a])
            try:
                args()
            finally:
                eng.grad_slab_hook = hook
            return seen[0] if seen else ['callback']
        out = [name]
        for v, ctype in zip(args, fn.argtypes):
            if hasattr(v, '_obj'):  # C.byref(struct): field by field
                out.append({k: value(getattr(v._obj, k), t) for k, t in v._obj._fields_})
            else:
                out.append(value(v, ctype))
        return out

    return dict(fwd=[launch(*c) for c in pl.fwd.calls], bwd=[launch(*c) for c in pl.bwd.calls], marks=pl.marks,
                buffers={k: [list(t.shape), str(t.dtype)] for k, t in pl.buf.items()})


if __name__ == '__main__':
    doc = {}
    for cfg in PLAN_SET:
        eng, pl = build_plan(*cfg)
        doc[plan_id(*cfg)] = plan_dump(pl)
        print(f'{plan_id(*cfg)}: {len(pl.fwd.calls)} forward, {len(pl.bwd.calls)} backward entries')
    with open(FIXTURE, 'wb') as raw, gzip.GzipFile('', 'wb', fileobj=raw, mtime=0) as fh:  # (no name, no time: same bytes every run)
        fh.write(json.dumps(doc, separators=(',', ':'), sort_keys=True).encode())
    print(f'{FIXTURE}: {os.path.getsize(FIXTURE)} bytes')
