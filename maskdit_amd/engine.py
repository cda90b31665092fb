"""MaskDiT engine: flat parameter arenas + pre-bound launch plans over libmaskdit_hip.so.

Design (MI355X-first):
  * every trainable tensor of the reference state dict is a VIEW into one fp32 arena (same
    names / shapes as the reference checkpoint); gradients, Adam moments
    and the EMA live in arenas of the same layout, so the optimizer + EMA + bf16-shadow refresh
    is ONE streaming kernel and the DP gradient all-reduce works on contiguous slabs;
  * all adaLN modulation Linears (28 + 8 + 2 of them, each fed by the same SiLU(c)) are laid
    out contiguously so the forward needs ONE [B, D] x [N_mod, D]^T GEMM for every
    shift/scale/gate of the network, and the backward one dgrad + one wgrad GEMM;
  * GEMM operands are bf16 shadows of the fp32 master weights (N-major for forward,
    K-major transposed copies for the data-gradient GEMMs), refreshed by the optimizer;
  * a forward / backward pass is a *plan*: a list of (C entry point, pre-marshalled args) built
    once per (batch, mode) over preallocated HBM buffers -- replaying it is a tight loop of
    ctypes calls with no allocation, which also makes it hipGraph-capturable (sampler).

Reference semantics: DiT.forward / forward_encoder (models/maskdit.py:467-557), DiTBlock
(:170-192), DecoderLayer (:195-213), FinalLayer (:216-234), EDMPrecond (:756-773), EDMLoss
(train_utils/loss.py:28-60).  Backward = hand-derived gradients of the same graph.
"""
from __future__ import annotations

import ctypes as C
import os
import weakref
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import (EPI_BF16, EPI_DGELU, EPI_DSILU, EPI_F32, EPI_GATE_RES, EPI_GELU, EPI_SILU, F32EPI_GATE_RES,
                   F32EPI_GELU, F32EPI_NONE, F32EPI_SILU, GemmF32Args, GemmF32TNArgs, GemmNTArgs, GemmTNArgs)

DEC_HIDDEN, DEC_DEPTH, DEC_HEADS = 512, 8, 16  # models/maskdit.py:310-312
MODEL_CONFIGS = {  # models/maskdit.py:649-715  name -> (depth, hidden, patch, heads)
    'DiT-H/2': (32, 1280, 2, 16), 'DiT-H/4': (32, 1280, 4, 16), 'DiT-H/8': (32, 1280, 8, 16),
    'DiT-XL/2': (28, 1152, 2, 16), 'DiT-XL/4': (28, 1152, 4, 16), 'DiT-XL/8': (28, 1152, 8, 16),
    'DiT-L/2': (24, 1024, 2, 16), 'DiT-L/4': (24, 1024, 4, 16), 'DiT-L/8': (24, 1024, 8, 16),
    'DiT-B/2': (12, 768, 2, 12), 'DiT-B/4': (12, 768, 4, 12), 'DiT-B/8': (12, 768, 8, 12),
    'DiT-S/2': (12, 384, 2, 6), 'DiT-S/4': (12, 384, 4, 6), 'DiT-S/8': (12, 384, 8, 6),
}
YPAD = 1024  # label one-hot width padded to a multiple of 128 for the GEMMs
LIVE_ENGINES: 'weakref.WeakSet' = weakref.WeakSet()  # lets the optimizer map a parameter view back to its arena
# mdt_ln_modulate_bwd_gate: LayerNorm backward + the following residual-gate backward in one pass, 18 instead of
# 14 + 8 B/element.  Round 2's column-split kernel (a pair of waves per row, 4 x 12 instead of 4 x 20 running sums per
# lane, second-half loads issued before the row reduction): 631 vs 726 us for the pair on the XL/2 encoder rows at
# micro-batch 1024, 538 vs 606 us on the decoder rows (tools/ln_gate_bench.py); whole step 520.0 -> 518.5 ms on the
# same box.  History: the row-per-wave build (214 VGPRs) lost to the separate kernels (705-762 us), an LDS-atomics
# build was 4x slower (3017 us).  MDT_FUSE_LN_GATE=0 selects the two separate kernels (A/B runs).
FUSE_LN_GATE = os.environ.get('MDT_FUSE_LN_GATE', '1') != '0'
ADA_GROUP = 7  # encoder blocks per adaLN weight-gradient group (XL/2: 4 groups of 7 + the decoder-side group)
FUSE_QKV_COLSUM = os.environ.get('MDT_FUSE_QKV_COLSUM', '1') != '0'  # qkv bias gradient out of the qkv weight-gradient GEMM (A/B switch)
FUSE_COLSUM = os.environ.get('MDT_FUSE_COLSUM', '1') != '0'  # fc1 bias gradient out of the DGELU epilogue (A/B switch)
# Round 6: in TRAINING plans the residual add `x + gate * f(x)` (models/maskdit.py:190-191) is formed by the LayerNorm pass that
# consumes it (mdt_ln_modulate_fwd_res) instead of by the epilogue of the GEMM that produced f(x): the proj / fc2 GEMMs store only
# their bf16 output (plain class) -- 14 instead of 16 B per element, bit-identical x.  MDT_FUSE_RES_LN=0: the MDT_EPI_GATE_RES
# epilogues of rounds 1-5 (A/B runs).  Inference plans keep GATE_RES: they do not store the branch output at all.
FUSE_RES_LN = os.environ.get('MDT_FUSE_RES_LN', '1') != '0'
FUSE_RES_LN_EVAL = os.environ.get('MDT_FUSE_RES_LN_EVAL', '0') != '0'  # the same in inference plans (A/B)


def _rup(x, m):
    return (x + m - 1) // m * m


@dataclass
class Spec:
    model_type: str
    depth: int
    D: int
    heads: int
    patch: int
    R: int
    C: int
    num_classes: int
    mae: bool
    Dd: int = DEC_HIDDEN
    ddepth: int = DEC_DEPTH
    dheads: int = DEC_HEADS
    # use_decoder=False (models/maskdit.py:308-331, 529-553): no DecoderLayer, decoder blocks, decoder_pos_embed or mask
    # token; the final layer reads the encoder's rows at width D.  Such a spec carries ddepth = 0 and Dd = D, so that
    # "the final layer's width" stays sp.Dd for both kinds.
    use_decoder: bool = True

    @property
    def T(self):
        return (self.R // self.patch) ** 2

    @property
    def hd(self):
        return self.D // self.heads

    @property
    def dhd(self):
        return self.Dd // self.dheads

    @property
    def pp(self):
        return self.patch * self.patch * self.C

    @property
    def n_mod(self):
        if not self.use_decoder:
            return self.depth * 6 * self.D + 2 * self.D
        return self.depth * 6 * self.D + self.ddepth * 6 * self.Dd + 2 * self.D + 2 * self.Dd

    def mod_off(self, kind, i=0):
        """Row offset of an adaLN Linear inside the stacked [N_mod, D] weight."""
        if kind == 'enc':
            return i * 6 * self.D
        base = self.depth * 6 * self.D
        if not self.use_decoder:
            if kind != 'fin':
                raise KeyError(f'a decoder-less model has no {kind!r} modulation rows')
            return base
        if kind == 'dec':
            return base + i * 6 * self.Dd
        base += self.ddepth * 6 * self.Dd
        if kind == 'dl':
            return base
        return base + 2 * self.D  # final


def make_spec(model_type, img_resolution, img_channels, num_classes, use_decoder=True, mae_loss_coef=0.1):
    if model_type not in MODEL_CONFIGS:
        raise ValueError(f'unknown model_type {model_type}')
    depth, D, p, heads = MODEL_CONFIGS[model_type]
    sp = Spec(model_type, depth, D, heads, p, img_resolution, img_channels, num_classes, mae_loss_coef > 0)
    if not use_decoder:
        sp = Spec(model_type, depth, D, heads, p, img_resolution, img_channels, num_classes, mae_loss_coef > 0,
                  Dd=D, ddepth=0, dheads=heads, use_decoder=False)
    if sp.hd not in (32, 64, 72, 80):
        raise NotImplementedError(f'head_dim {sp.hd} unsupported')
    # the token-boundary kernels serve patch vectors of 16 elements (embed.hip / loss.hip) and of 64 and 256 (patch.hip)
    if sp.pp not in (16, 64, 256) or sp.num_classes > YPAD or sp.num_classes <= 0:
        raise NotImplementedError(f'patch vector of {sp.pp} elements (supported: 16, 64, 256 = 4 channels at patch 2, 4, 8) '
                                  'or num_classes outside (0, 1024]')
    T = sp.T
    if sp.R % p or T & (T - 1) or T > 1024 or T % 64:
        raise NotImplementedError(f'token count {T} must be a power of two in [64, 1024]: patch {p} serves latent sides '
                                  f'{8 * p}, {16 * p} and {32 * p} (the smallest is {8 * p})')
    return sp


# ------------------------------------------------------------------------------------------
# parameter layout

def param_table(sp: Spec) -> List[Tuple[str, tuple]]:
    """(state-dict key, shape) for every TRAINABLE tensor, in arena order."""
    D, Dd = sp.D, sp.Dd
    ada_w, ada_b, rest = [], [], []

    def ada(prefix, n):
        ada_w.append((f'{prefix}.adaLN_modulation.1.weight', (n, D)))
        ada_b.append((f'{prefix}.adaLN_modulation.1.bias', (n,)))

    def block(prefix, W):
        h = 4 * W
        rest.extend([(f'{prefix}.attn.qkv.weight', (3 * W, W)), (f'{prefix}.attn.qkv.bias', (3 * W,)),
                     (f'{prefix}.attn.proj.weight', (W, W)), (f'{prefix}.attn.proj.bias', (W,)),
                     (f'{prefix}.mlp.fc1.weight', (h, W)), (f'{prefix}.mlp.fc1.bias', (h,)),
                     (f'{prefix}.mlp.fc2.weight', (W, h)), (f'{prefix}.mlp.fc2.bias', (W,))])

    for i in range(sp.depth):
        ada(f'model.blocks.{i}', 6 * D)
        block(f'model.blocks.{i}', D)
    for i in range(sp.ddepth):
        ada(f'model.decoder_blocks.{i}', 6 * Dd)
        block(f'model.decoder_blocks.{i}', Dd)
    if sp.use_decoder:
        ada('model.decoder_layer', 2 * D)
    ada('model.final_layer', 2 * Dd)
    if sp.use_decoder:
        rest.extend([('model.decoder_layer.linear.weight', (Dd, D)), ('model.decoder_layer.linear.bias', (Dd,))])
    rest.extend([('model.final_layer.linear.weight', (sp.pp, Dd)), ('model.final_layer.linear.bias', (sp.pp,)),
                 ('model.x_embedder.proj.weight', (D, sp.C, sp.patch, sp.patch)), ('model.x_embedder.proj.bias', (D,)),
                 ('model.t_embedder.mlp.0.weight', (D, 256)), ('model.t_embedder.mlp.0.bias', (D,)),
                 ('model.t_embedder.mlp.2.weight', (D, D)), ('model.t_embedder.mlp.2.bias', (D,)),
                 ('model.y_embedder.embedding_table.weight', (D, sp.num_classes))])
    if sp.mae and sp.use_decoder:  # (models/maskdit.py:323-324: the mask token belongs to the decoder)
        rest.append(('model.mask_token', (1, 1, Dd)))
    return ada_w + ada_b + rest


class Layout:
    """Offsets (in elements) of every trainable tensor inside the flat arenas."""

    def __init__(self, sp: Spec):
        self.sp = sp
        self.off: Dict[str, int] = {}
        self.shape: Dict[str, tuple] = {}
        o = 0
        for name, shp in param_table(sp):
            n = int(np.prod(shp))
            self.off[name] = o
            self.shape[name] = shp
            o += _rup(n, 8)  # adaLN tensors are multiples of 8 elements, so their stacks stay dense
        self.n = _rup(o, 8)
        self.ada_w = self.off['model.blocks.0.adaLN_modulation.1.weight']
        self.ada_b = self.off['model.blocks.0.adaLN_modulation.1.bias']
        # K-major (transposed) shadows for the data-gradient GEMMs
        self.t_off: Dict[str, int] = {}
        self.t_entries: List[Tuple[int, int, int, int]] = []
        to = 0

        def addT(key, src, rows, cols):
            nonlocal to
            self.t_off[key] = to
            self.t_entries.append((src, to, rows, cols))
            to += _rup(rows * cols, 8)

        addT('ada', self.ada_w, sp.n_mod, sp.D)
        for name, shp in param_table(sp):
            if name.endswith(('attn.qkv.weight', 'attn.proj.weight', 'mlp.fc1.weight', 'mlp.fc2.weight')) \
                    or name in ('model.decoder_layer.linear.weight', 'model.t_embedder.mlp.2.weight'):
                addT(name, self.off[name], shp[0], shp[1])
        self.nt = to
        # block-wise slabs of the arena for gradient all-reduce overlap (name -> (start, end))
        self.slabs: Dict[str, Tuple[int, int]] = {}

        def span(prefix_first, prefix_last_end_name):
            return self.off[prefix_first], self.off[prefix_last_end_name] + _rup(int(np.prod(self.shape[prefix_last_end_name])), 8)

        for i in range(sp.depth):
            self.slabs[f'enc{i}'] = span(f'model.blocks.{i}.attn.qkv.weight', f'model.blocks.{i}.mlp.fc2.bias')
        for i in range(sp.ddepth):
            self.slabs[f'dec{i}'] = span(f'model.decoder_blocks.{i}.attn.qkv.weight', f'model.decoder_blocks.{i}.mlp.fc2.bias')
        # the stacked adaLN weight [N_mod, D] is 35 % of all gradient bytes: its rows are reduced in groups
        # whose modulation gradients become final at different points of the backward pass (decoder side
        # first, then the encoder blocks from the top in groups of ADA_GROUP), not in one piece at the end
        self.ada_groups: List[Tuple[str, int, int]] = []  # (slab name, first row, end row) in backward order
        enc_rows = sp.depth * 6 * sp.D
        self.ada_groups.append(('ada_w_dec', enc_rows, sp.n_mod))
        hi_blk = sp.depth
        while hi_blk > 0:
            lo_blk = max(0, hi_blk - ADA_GROUP)
            self.ada_groups.append((f'ada_w_enc{lo_blk}', lo_blk * 6 * sp.D, hi_blk * 6 * sp.D))
            hi_blk = lo_blk
        for name, r0, r1 in self.ada_groups:
            self.slabs[name] = (self.ada_w + r0 * sp.D, self.ada_w + r1 * sp.D)
        self.slabs['ada_b'] = (self.ada_b, self.off['model.blocks.0.attn.qkv.weight'])
        self.slabs['misc'] = (self.off['model.decoder_layer.linear.weight' if sp.use_decoder else 'model.final_layer.linear.weight'],
                              self.n)


# ------------------------------------------------------------------------------------------
# plans

class Plan:
    """A replayable list of pre-marshalled launches (and optional python callbacks)."""

    def __init__(self, listing: bool = False):
        self.calls: list = []
        self.keep: list = []
        self.listing = listing  # built over HOST buffers (Engine.host_listing): to be read, never launched

    def add(self, name, *args):
        fn = getattr(_lib.lib(), name)
        self.calls.append((fn, args, name))

    def add_callback(self, cb: Callable[[], None]):
        self.calls.append((None, cb, 'callback'))

    def run(self, stream: int):
        if self.listing:
            raise _lib.MaskDiTLibError('this plan lists launches over host memory (Engine.host_listing): it cannot run')
        for fn, args, name in self.calls:
            if fn is None:
                args()
                continue
            rc = fn(*args, stream)
            if rc != 0:
                raise _lib.MaskDiTLibError(f'{name} failed ({rc}): {_lib.lib().mdt_last_error().decode()}')


class Engine:
    """Owns arenas, shadows and launch plans for one EDMPrecond/DiT instance on one GPU."""

    def __init__(self, sp: Spec, device, _listing: bool = False):
        self.sp = sp
        self.device = torch.device(device)
        self.listing = _listing
        if self.device.type != 'cuda' and not _listing:
            raise _lib.MaskDiTLibError('maskdit_amd.Engine needs a CUDA/HIP device: there is no CPU path')
        _lib.lib()
        self.lay = Layout(sp)
        dev = self.device
        self.P = torch.zeros(self.lay.n, device=dev, dtype=torch.float32)
        self.G: Optional[torch.Tensor] = None
        self.W16 = torch.zeros(self.lay.n, device=dev, dtype=torch.bfloat16)
        self.WT16 = torch.zeros(self.lay.nt, device=dev, dtype=torch.bfloat16)
        self.Wy16 = torch.zeros(sp.D, YPAD, device=dev, dtype=torch.bfloat16)
        self.pos = torch.zeros(sp.T, sp.D, device=dev, dtype=torch.float32)
        self.dpos = torch.zeros(sp.T if sp.use_decoder else 0, sp.Dd, device=dev, dtype=torch.float32)  # decoder_pos_embed
        tab, tiles = [], 0
        for src, dst, rows, cols in self.lay.t_entries:
            tab += [src, dst, rows, cols, tiles]
            tiles += ((rows + 63) // 64) * ((cols + 63) // 64)
        self._t_table = torch.tensor(tab, dtype=torch.int64, device=dev)
        self._t_tiles = tiles
        self.shadows_dirty = True
        self._plans: Dict[tuple, 'PassPlan'] = {}   # insertion order = LRU order (plan() re-inserts on every hit)
        self.plan_headroom = 0.05                   # fraction of the device a new plan leaves free (see plan())
        self.grad_slab_hook: Optional[Callable[[str, int, int], None]] = None  # DP overlap (ddp.py)
        self.ema_applied = None
        LIVE_ENGINES.add(self)

    @classmethod
    def host_listing(cls, sp: Spec) -> 'Engine':
        """An engine whose arenas are HOST tensors, for building PassPlan(eng, ...) where there is no GPU and reading its
        launch lists (tools/plan_dump.py, tests/test_plan_lists_cpu.py).  Nothing built from it can launch: plan(),
        refresh_shadows() and Plan.run() raise MaskDiTLibError."""
        return cls(sp, 'cpu', _listing=True)

    def _refuse_listing(self, what: str):
        if self.listing:
            raise _lib.MaskDiTLibError(f'{what} needs the device: this engine only lists plans over host memory')

    # ---- arenas ------------------------------------------------------------------------
    def view(self, arena: torch.Tensor, name: str) -> torch.Tensor:
        o, shp = self.lay.off[name], self.lay.shape[name]
        return arena[o:o + int(np.prod(shp))].view(shp)

    def ensure_grad(self) -> torch.Tensor:
        if self.G is None:
            self.G = torch.zeros(self.lay.n, device=self.device, dtype=torch.float32)
        return self.G

    def refresh_shadows(self, cast: bool = True):
        """bf16 N-major shadow (optional: the optimizer already wrote it), K-major transposes,
        padded label table."""
        self._refuse_listing('Engine.refresh_shadows')
        st = torch.cuda.current_stream().cuda_stream
        sp, lay = self.sp, self.lay
        if cast:
            _lib.call('mdt_cast_f32_bf16', self.P.data_ptr(), lay.n, self.W16.data_ptr(), lay.n, 1, lay.n, 0, st)
        _lib.call('mdt_transpose_bf16_batched', self.W16.data_ptr(), self.WT16.data_ptr(), self._t_table.data_ptr(),
                  len(lay.t_entries), self._t_tiles, st)
        yo = lay.off['model.y_embedder.embedding_table.weight']
        _lib.call('mdt_cast_f32_bf16', self.P.data_ptr() + 4 * yo, sp.num_classes, self.Wy16.data_ptr(), YPAD, sp.D,
                  sp.num_classes, 0, st)
        self.shadows_dirty = False

    # ---- plans -------------------------------------------------------------------------
    def plan(self, B: int, masked: bool, train: bool, L: Optional[int] = None, precision: str = 'bf16') -> 'PassPlan':
        """Plans are keyed on the kept-token count ROUNDED UP to the 64-row tile: a mask-ratio schedule
        (train_utils/helper.py:9-27) changes the exact count nearly every step, but buffers and launch lists only
        depend on the padded count -- the exact one is a run-time argument of the four launches that read it
        (PassPlan.set_valid)."""
        global _PLAN_CLOCK
        self._refuse_listing('Engine.plan')
        check_precision(precision)
        f32_train = precision == 'fp32' and train and not masked  # the unmasked stage (train.py --no_amp): _build_f32_train
        if f32_train and not self.sp.use_decoder:
            raise NotImplementedError(NODECODER_FP32_MESSAGE)
        if reads_f32_arena(precision) and (masked or train) and not f32_train:
            raise NotImplementedError('the fp32-faithful path covers inference (the sampler / eval forward: sample.py:56) and, at '
                                      "precision 'fp32', training of the UNMASKED stage (mask_ratio 0: train.py --no_amp); fp32 "
                                      "TRAINING of the masked stage and a 'bf16x3' training plan are not provided")
        Lv = (L if L is not None else self.sp.T // 2) if masked else None
        key = plan_key(B, masked, train, Lv, precision)
        pl = self._plans.pop(key, None)
        if pl is None:
            # LRU cache under a DEVICE-wide memory budget.  Round 2 dropped every training plan whenever another shape
            # was requested; round 3 budgeted each engine against 0.80 of the device on its own, so with two engines
            # alive (train.py: net + ema; a test process: whatever the previous tests left behind) the second one could
            # neither see nor evict the first one's plans and died with OutOfMemoryError.  Now: what a new
            # plan needs is compared with what the device really has free (torch.cuda.mem_get_info + the caching
            # allocator's idle blocks), and the least-recently-used plan of ANY live engine on this device is dropped
            # until it fits (5 % of the device stays free for the caller's own tensors) or nothing is left to drop.
            while len(self._plans) >= 8:
                _drop_plan(self, next(iter(self._plans)))
            need = PassPlan.estimate_bytes_f32_train(self.sp, B) if f32_train else \
                PassPlan.estimate_bytes(self.sp, B, masked, train, Lv) * (2 if reads_f32_arena(precision) else 1)
            # (a plan something else still refers to -- a pending backward, a captured sampler graph -- gives no memory back
            # when its cache entry goes: after two evictions in a row that freed nothing the loop stops instead of emptying
            # every engine's cache for no gain)
            fruitless = 0
            while need + self.plan_headroom * _device_total(self.device) > _device_available(self.device) and fruitless < 2:
                before = _device_available(self.device)
                if not _evict_lru_plan(self.device):
                    break
                fruitless = fruitless + 1 if _device_available(self.device) <= before else 0
            if f32_train and need > _device_available(self.device):
                # the estimate of this plan is exact to a few per cent (estimate_bytes_f32_train), so a batch that cannot fit
                # is refused here, with the figures, instead of somewhere inside the allocator
                raise RuntimeError(f'maskdit_amd: an fp32 training plan for batch {B} needs {need / 2**30:.1f} GiB of activations and '
                                   f'workspace ({need / B / 2**20:.0f} MiB per sample), the device has '
                                   f'{_device_available(self.device) / 2**30:.1f} GiB available after dropping every cached plan: '
                                   'use a smaller micro-batch (train.batchsize) with train.grad_accum')
            while True:
                try:
                    pl = PassPlan(self, B, masked, train, Lv, precision)
                    break
                except torch.cuda.OutOfMemoryError:
                    if not _evict_lru_plan(self.device):
                        raise
                    torch.cuda.empty_cache()
        elif masked:
            pl.set_valid(Lv)
        _PLAN_CLOCK += 1
        pl.last_use = _PLAN_CLOCK
        self._plans[key] = pl  # most recently used = last
        return pl

    def release_plans(self):
        for key in list(self._plans):
            _drop_plan(self, key)


_PLAN_CLOCK = 0

# Inference arithmetics of Engine.plan: 'bf16' = the training kernels (bf16 shadows of the weights); 'fp32' = exact fp32
# (csrc/f32path.hip); 'bf16x3' = the fp32 plan with its Linear layers on mdt_gemm_bf16x3 (fp32-level accuracy on the bf16
# matrix instruction), attention and everything else as in 'fp32'.
PRECISIONS = ('bf16', 'fp32', 'bf16x3')


NODECODER_FP32_MESSAGE = ("fp32 training (train precision 'fp32', train.py --no_amp) is not provided for a decoder-less model "
                          "(use_decoder=False): it trains with the bf16 kernels (set_train_precision('bf16'), no --no_amp)")


def check_precision(precision: str) -> str:
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {', '.join(map(repr, PRECISIONS))}, got {precision!r}")
    return precision


def reads_f32_arena(precision: str) -> bool:
    """A plan of this precision reads the fp32 master arena itself (no bf16 shadow): the fp32-faithful builder, inference
    only."""
    return precision != 'bf16'


def plan_key(B: int, masked: bool, train: bool, Lv: Optional[int] = None, precision: str = 'bf16') -> tuple:
    """Cache key of Engine.plan(): bf16 keys keep their round-1..5 form; an fp32 plan is another entry."""
    key = (B, masked, train, _rup(Lv, 64) if masked else None)
    return key if precision == 'bf16' else key + (precision,)


def _device_total(device) -> int:
    return torch.cuda.get_device_properties(device).total_memory


def _device_available(device) -> int:
    """Bytes a new allocation can get: free device memory + blocks the caching allocator holds but does not use."""
    free, _ = torch.cuda.mem_get_info(device)
    return free + torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)


def _drop_plan(eng, key):
    """THE way a plan leaves a cache: whoever replays its launch list (the sampler's captured graphs) is told."""
    pl = eng._plans.pop(key)
    for hook in pl.evict_hooks:
        hook()
    pl.evict_hooks = []


def _evict_lru_plan(device) -> bool:
    """Drop the least-recently-used cached plan among ALL live engines on `device`; False when none is cached.  (A plan a
    pending backward still refers to stays alive through that reference -- only the cache entry goes.)"""
    best = None
    for eng in list(LIVE_ENGINES):
        if eng.device != torch.device(device):
            continue
        for key, pl in eng._plans.items():
            if best is None or pl.last_use < best[2].last_use:
                best = (eng, key, pl)
    if best is None:
        return False
    _drop_plan(best[0], best[1])
    return True


def _nt(A, lda, Bw, ldb, M, N, K, bias=0, epi=EPI_BF16, out=0, ldo=0, out2=0, ldo2=0, outf=0, ldof=0, res=0, ldres=0,
        gate=0, gate_ld=0, rps=1, aux=0, ldaux=0, k_splits=0, colsum=0):
    a = GemmNTArgs()
    a.A, a.lda, a.B, a.ldb, a.M, a.N, a.K = A, lda, Bw, ldb, M, N, K
    a.bias, a.epi = bias or None, epi
    a.out, a.ldo, a.out2, a.ldo2 = out or None, ldo, out2 or None, ldo2
    a.outf, a.ldof, a.res, a.ldres = outf or None, ldof, res or None, ldres
    a.gate, a.gate_ld, a.rows_per_sample = gate or None, gate_ld, rps
    a.aux, a.ldaux = aux or None, ldaux
    a.k_splits = k_splits
    a.colsum = colsum or None
    return a


def _tn(A, lda, Bm, ldb, M, N1, N2, Cc, ldc, n1v=0, n2v=0, splits=0, colsum_a=0):
    a = GemmTNArgs()
    a.A, a.lda, a.B, a.ldb, a.M, a.N1, a.N2 = A, lda, Bm, ldb, M, N1, N2
    a.C, a.ldc, a.n1_valid, a.n2_valid, a.splits = Cc, ldc, n1v, n2v, splits
    a.colsum_a = colsum_a or None
    return a


class PassPlan:
    """Buffers + forward/backward launch lists for a fixed (batch, masked?, train?) shape."""

    def __init__(self, eng: Engine, B: int, masked: bool, train: bool, L: Optional[int], precision: str = 'bf16'):
        sp = eng.sp
        self.precision = precision
        # the engine caches its plans, so a plan must not own its engine: Engine <-> PassPlan reference cycles kept
        # 20-240 GB of a dropped model alive until Python's cyclic collector happened to run
        self._eng_ref = weakref.ref(eng)
        self.B, self.masked, self.train = B, masked, train
        self.last_use = 0
        self.evict_hooks: List[Callable[[], None]] = []  # run when the plan cache drops this plan for memory
        self.T = sp.T
        # Lv = kept tokens per sample (models/maskdit.py:99: int(T * (1 - mask_ratio)), any value that a
        # mask-ratio schedule produces); the encoder runs on L = Lv rounded up to the 64-row tile: the
        # padding rows gather (removed) tokens, are masked out as attention KEYS, are skipped by the
        # un-masking gather, and receive exactly zero gradient (mdt_unmask_bwd), so every other kernel
        # simply sees L rows per sample.
        self.Lv = (L if L is not None else sp.T // 2) if masked else sp.T
        if not (1 <= self.Lv <= sp.T):
            raise ValueError(f'kept-token count {self.Lv} outside [1, {sp.T}]')
        self.L = _rup(self.Lv, 64)
        # the exact count as a MUTABLE C int inside the pre-marshalled argument tuples (ctypes reads .value at call
        # time): attention key masking + the un-masking gather / scatter are the only launches that see it
        self.lv_arg = C.c_int(self.Lv)
        self.lv_attn = C.c_int(self.Lv if masked else 0)
        self.Bp = _rup(B, 64)
        self.buf: Dict[str, torch.Tensor] = {}
        self.fwd = Plan(eng.listing)
        self.bwd = Plan(eng.listing)
        self.gen = 0  # forward generation: the saved activations belong to the LAST forward through this plan
        if train:
            eng.ensure_grad()  # before a builder takes the first gradient address (Gf); inference plans need no gradient arena
        if not reads_f32_arena(precision):
            self._build()
        elif train:  # (Engine.plan lets only the unmasked stage at 'fp32' through)
            if not sp.use_decoder:
                raise NotImplementedError(NODECODER_FP32_MESSAGE)
            self._build_f32_train()
        else:
            self._build_f32()

    @property
    def eng(self) -> Engine:
        e = self._eng_ref()
        if e is None:
            raise RuntimeError('maskdit_amd: this plan outlived its Engine (the model was deleted or re-bound)')
        return e

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.buf.values())

    @staticmethod
    def estimate_bytes(sp, B: int, masked: bool, train: bool, Lv: Optional[int]) -> int:
        """Upper estimate of a plan's buffers before it is built (measured: 244 GB in use for XL/2 at B = 1024 incl.
        30 GB of arenas; inference plans keep one block's worth of activations)."""
        L = _rup(Lv, 64) if masked else sp.T
        per_tok_enc = 40 * sp.D if train else 0      # bytes of saved activations per encoder token and block
        per_tok_dec = 40 * sp.Dd if train else 0
        live = 64 * max(sp.D, sp.Dd) * sp.T          # per-sample working set of one block (fwd-only plans)
        io = 6 * 4 * sp.C * sp.R * sp.R              # yn / D / y / noise-sized fp32 images of the loss + precond algebra
        return int(B * (sp.depth * per_tok_enc * L + sp.ddepth * per_tok_dec * sp.T + live + io) * 1.05)

    def set_valid(self, Lv: int):
        if _rup(Lv, 64) != self.L or not (1 <= Lv <= self.T):
            raise ValueError(f'kept-token count {Lv} does not belong to this plan (padded count {self.L})')
        self.Lv = Lv
        self.lv_arg.value = Lv
        self.lv_attn.value = Lv

    # ---- buffers -----------------------------------------------------------------------
    def t(self, name, shape, dtype):
        if name in self.buf:
            return self.buf[name]
        x = torch.zeros(shape, device=self.eng.device, dtype=dtype)
        self.buf[name] = x
        return x

    def f32(self, name, *shape):
        return self.t(name, shape, torch.float32)

    def b16(self, name, *shape):
        return self.t(name, shape, torch.bfloat16)

    # ---- addresses of one parameter (its full state-dict key) in the engine's arenas --------------
    def Pf(self, name):
        """fp32 master"""
        return self.eng.P.data_ptr() + 4 * self.eng.lay.off[name]

    def Gf(self, name):
        """gradient (training plans: __init__ has made sure that the arena exists)"""
        return self.eng.G.data_ptr() + 4 * self.eng.lay.off[name]

    def Wp(self, name):
        """bf16 N-major shadow"""
        return self.eng.W16.data_ptr() + 2 * self.eng.lay.off[name]

    def WT(self, key):
        """bf16 K-major shadow ('ada': the stacked adaLN weight)"""
        return self.eng.WT16.data_ptr() + 2 * self.eng.lay.t_off[key]

    def _io(self):
        """The buffers the callers fill and read, under the same names in every plan, so that the sampler, EDMPrecond.forward
        and EDMLoss drive any of them the same way: 'xin', 'coef' (rows: c_skip, c_out, c_in, c_noise, weight, sigma, -, -;
        'c_noise' is row 3), 'labels', 'ids32' (masked plans), 'F'.  EDMLoss's own buffers (loss.py; 16 KB per sample) are
        allocated here too, so that they are covered by plan()'s out-of-memory handling like everything else: 'yn', 'D', 'y'
        in every plan EDMLoss can be given (all but fp32 / bf16x3 inference), 'dF' in training plans.
        Returns (xin, c_noise, labels, ids32 or None, F)."""
        sp, B = self.eng.sp, self.B
        img = (B, sp.C, sp.R, sp.R)
        xin = self.f32('xin', *img)
        cn = self.buf['c_noise'] = self.f32('coef', 8, B)[3]
        lab = self.f32('labels', B, sp.num_classes)
        ids32 = self.t('ids32', (B, 2 * self.T), torch.int32) if self.masked else None
        Fx = self.f32('F', *img)
        loss = ('yn', 'D', 'y') if self.train or not reads_f32_arena(self.precision) else ()
        for nm in loss + (('dF',) if self.train else ()):
            self.f32(nm, *img)
        return xin, cn, lab, ids32, Fx

    # ---- the bf16 plans (inference and training, masked or not) ------------------------------------
    def _build(self):
        eng, sp, lay = self.eng, self.eng.sp, self.eng.lay
        B, Bp, T, L, D, Dd = self.B, self.Bp, self.T, self.L, sp.D, sp.Dd
        NM = sp.n_mod
        train = self.train
        Pf, Wp, WT = self.Pf, self.Wp, self.WT
        f, g = self.fwd, self.bwd
        xin, cn, lab, ids32, Fx = self._io()
        # ---------------- conditioning path ---------------------------------------------------
        temb = self.b16('temb', Bp, 256)
        h1, a1 = self.b16('h1', Bp, D), self.b16('a1', Bp, D)
        c_t, c_y, c = self.f32('c_t', Bp, D), self.f32('c_y', Bp, D), self.f32('c', Bp, D)
        lab16 = self.b16('lab16', Bp, YPAD)
        sc16 = self.b16('sc16', Bp, D)
        mod = self.f32('mod', Bp, NM)
        f.add('mdt_timestep_embed', cn.data_ptr(), temb.data_ptr(), 256, B, 256)
        self._nt16(f, temb.data_ptr(), 256, Wp('model.t_embedder.mlp.0.weight'), 256, B, D, 256,
                   bias=Pf('model.t_embedder.mlp.0.bias'), epi=EPI_SILU, out=h1.data_ptr(), ldo=D, out2=a1.data_ptr(), ldo2=D)
        self._nt16(f, a1.data_ptr(), D, Wp('model.t_embedder.mlp.2.weight'), D, B, D, D, bias=Pf('model.t_embedder.mlp.2.bias'),
                   epi=EPI_F32, outf=c_t.data_ptr(), ldof=D)
        f.add('mdt_cast_f32_bf16', lab.data_ptr(), sp.num_classes, lab16.data_ptr(), YPAD, B, sp.num_classes, 0)
        self._nt16(f, lab16.data_ptr(), YPAD, eng.Wy16.data_ptr(), YPAD, B, D, YPAD, epi=EPI_F32, outf=c_y.data_ptr(), ldof=D)
        f.add('mdt_add_f32', c_t.data_ptr(), c_y.data_ptr(), c.data_ptr(), B * D)
        f.add('mdt_cast_f32_bf16', c.data_ptr(), D, sc16.data_ptr(), D, B, D, 1)
        self._nt16(f, sc16.data_ptr(), D, eng.W16.data_ptr() + 2 * lay.ada_w, D, B, NM, D, bias=eng.P.data_ptr() + 4 * lay.ada_b,
                   epi=EPI_F32, outf=mod.data_ptr(), ldof=NM)
        # ---------------- encoder --------------------------------------------------------------
        Me = B * L
        x0 = self.f32('x_e0', Me, D)
        f.add('mdt_patch_embed_fwd', xin.data_ptr(), None, Pf('model.x_embedder.proj.weight'),
              Pf('model.x_embedder.proj.bias'), eng.pos.data_ptr(), ids32.data_ptr() if ids32 is not None else None,
              2 * T, x0.data_ptr(), B, sp.C, sp.R, sp.patch, L, D)
        xs_e = [x0]
        fuse = FUSE_RES_LN and (train or FUSE_RES_LN_EVAL)
        pend = None  # (xres, y, gate address): the residual add the NEXT LayerNorm pass has to perform into xs_e[-1]
        for i in range(sp.depth):
            xo, pend = self._block_fwd(f'model.blocks.{i}', 'e', i, xs_e[-1], mod, sp.mod_off('enc', i), D, sp.heads, L, Me,
                                       lvalid=self.lv_attn, pending=pend,
                                       defer_out=fuse and (sp.use_decoder or i + 1 < sp.depth))
            xs_e.append(xo)
        if sp.use_decoder:
            # ---------------- decoder layer + unmask ----------------------------------------------
            self.marks = {'enc_fwd_end': len(f.calls)}  # launch index where the encoder (+ conditioning path) forward ends
            odl = sp.mod_off('dl')
            xnd = self.b16('xn_dl', Me, D)
            st_dl = self.f32('st_dl', Me, 2)
            xdec = self.b16('xdec', Me, Dd)
            if pend is not None:  # the top encoder block's MLP residual is formed here
                f.add('mdt_ln_modulate_fwd_res', pend[0].data_ptr(), pend[1].data_ptr(), pend[2], NM, mod.data_ptr() + 4 * odl,
                      mod.data_ptr() + 4 * (odl + D), NM, L, xs_e[-1].data_ptr(), xnd.data_ptr(), st_dl.data_ptr(), Me, D)
                self.marks['enc_fwd_end'] = len(f.calls)  # (it is encoder work: the mark moves behind it)
            else:
                f.add('mdt_ln_modulate_fwd', xs_e[-1].data_ptr(), mod.data_ptr() + 4 * odl, mod.data_ptr() + 4 * (odl + D), NM, L,
                      xnd.data_ptr(), st_dl.data_ptr(), Me, D)
            self._nt16(f, xnd.data_ptr(), D, Wp('model.decoder_layer.linear.weight'), D, Me, Dd, D,
                       bias=Pf('model.decoder_layer.linear.bias'), epi=EPI_BF16, out=xdec.data_ptr(), ldo=Dd)
            Md = B * T
            xd0 = self.f32('x_d0', Md, Dd)
            use_mt = self.masked and sp.mae
            f.add('mdt_unmask_fwd', xdec.data_ptr(), (ids32.data_ptr() + 4 * T) if self.masked else None, 2 * T,
                  Pf('model.mask_token') if use_mt else None, eng.dpos.data_ptr(), xd0.data_ptr(), B, T, self.lv_arg, Dd, L)
            xs_d = [xd0]
            pend = None
            for i in range(sp.ddepth):  # (the last block forms its own output: mdt_final_fwd reads it)
                xo, pend = self._block_fwd(f'model.decoder_blocks.{i}', 'd', i, xs_d[-1], mod, sp.mod_off('dec', i), Dd, sp.dheads, T, Md,
                                           pending=pend, defer_out=fuse and i + 1 < sp.ddepth)
                xs_d.append(xo)
            ofin = sp.mod_off('fin')
            st_f = self.f32('st_f', Md, 2)
            f.add('mdt_final_fwd', xs_d[-1].data_ptr(), mod.data_ptr() + 4 * ofin, mod.data_ptr() + 4 * (ofin + Dd), NM,
                  Pf('model.final_layer.linear.weight'), Pf('model.final_layer.linear.bias'), Fx.data_ptr(), st_f.data_ptr(),
                  B, T, Dd, sp.C, sp.patch)
        else:
            # ---------------- no decoder (models/maskdit.py:529-553): the final layer reads the encoder's rows; its kernel
            # scatters the kept tokens' patches to their image positions and zeroes the removed ones -----------------------
            self.marks = {'enc_fwd_end': len(f.calls)}
            Md, xs_d = 0, []
            ofin = sp.mod_off('fin')
            st_f = self.f32('st_f', Me, 2)
            ids_p = ids32.data_ptr() if ids32 is not None else None
            f.add('mdt_final_keep_fwd', xs_e[-1].data_ptr(), mod.data_ptr() + 4 * ofin, mod.data_ptr() + 4 * (ofin + D), NM,
                  Pf('model.final_layer.linear.weight'), Pf('model.final_layer.linear.bias'), ids_p, 2 * T, Fx.data_ptr(),
                  st_f.data_ptr(), B, T, self.lv_arg, L, D, sp.C, sp.patch)
        if not train:
            return
        # =================== backward ===========================================================
        Gf, Gp = self.Gf, eng.G.data_ptr()
        dF = self.buf['dF']
        dmod = self.f32('dmod', Bp, NM)
        wmax = max(Me * D, Md * Dd)
        dxe = self.f32('dx_e', Me, D)
        dxd = self.f32('dx_d', Md, Dd) if sp.use_decoder else None
        ws = dict(dys=self.b16('ws_dys', wmax), dh=self.b16('ws_dh', 4 * wmax), dxn=self.b16('ws_dxn', wmax),
                  dao=self.b16('ws_dao', wmax), dqkv=self.b16('ws_dqkv', 3 * wmax),
                  delta=self.f32('ws_delta', max(B * sp.heads * L, B * sp.dheads * T if sp.use_decoder else 0)))
        self._ws = ws
        g.add_callback(lambda: dmod.zero_())
        if not sp.use_decoder:  # dx_e straight from the final layer: real rows stored, the pitch's padding rows zeroed
            g.add('mdt_final_keep_bwd', dF.data_ptr(), xs_e[-1].data_ptr(), st_f.data_ptr(), mod.data_ptr() + 4 * ofin,
                  mod.data_ptr() + 4 * (ofin + D), NM, Pf('model.final_layer.linear.weight'), ids_p, 2 * T, dxe.data_ptr(),
                  Gf('model.final_layer.linear.weight'), Gf('model.final_layer.linear.bias'), dmod.data_ptr() + 4 * ofin,
                  dmod.data_ptr() + 4 * (ofin + D), NM, B, T, self.lv_arg, L, D, sp.C, sp.patch)
        else:
            g.add('mdt_final_bwd', dF.data_ptr(), xs_d[-1].data_ptr(), st_f.data_ptr(), mod.data_ptr() + 4 * ofin,
                  mod.data_ptr() + 4 * (ofin + Dd), NM, Pf('model.final_layer.linear.weight'), dxd.data_ptr(),
                  Gf('model.final_layer.linear.weight'), Gf('model.final_layer.linear.bias'), dmod.data_ptr() + 4 * ofin,
                  dmod.data_ptr() + 4 * (ofin + Dd), NM, B, T, Dd, sp.C, sp.patch)
            for i in reversed(range(sp.ddepth)):
                # the LN1 backward that ends block i also runs the MLP-gate backward that would open block i-1
                nxt = self._gate_info(f'model.decoder_blocks.{i - 1}', 'd', i - 1, mod, dmod, sp.mod_off('dec', i - 1), Dd) \
                    if (i > 0 and FUSE_LN_GATE) else None
                self._block_bwd(f'model.decoder_blocks.{i}', 'd', i, xs_d[i], mod, dmod, sp.mod_off('dec', i), Dd, sp.dheads, T, Md,
                                dxd, fuse_next=nxt, skip_first_gate=(FUSE_LN_GATE and i < sp.ddepth - 1))
                self._slab(f'dec{i}')
            dxdec = self.b16('dxdec', Me, Dd)
            g.add('mdt_unmask_bwd', dxd.data_ptr(), ids32.data_ptr() if self.masked else None, 2 * T, dxdec.data_ptr(),
                  Gf('model.mask_token') if use_mt else None, B, T, self.lv_arg, Dd, L)
            self._tn16(g, dxdec.data_ptr(), Dd, xnd.data_ptr(), D, Me, Dd, D, Gf('model.decoder_layer.linear.weight'), D)
            g.add('mdt_colsum_bf16', dxdec.data_ptr(), Dd, Gf('model.decoder_layer.linear.bias'), Me, Dd)
            self._nt16(g, dxdec.data_ptr(), Dd, WT('model.decoder_layer.linear.weight'), Dd, Me, D, Dd, epi=EPI_BF16,
                       out=ws['dxn'].data_ptr(), ldo=D)
            if FUSE_LN_GATE:
                top = self._gate_info(f'model.blocks.{sp.depth - 1}', 'e', sp.depth - 1, mod, dmod, sp.mod_off('enc', sp.depth - 1), D)
                g.add('mdt_ln_modulate_bwd_gate', ws['dxn'].data_ptr(), xs_e[-1].data_ptr(), st_dl.data_ptr(), mod.data_ptr() + 4 * (odl + D),
                      NM, L, dxe.data_ptr(), 0, dmod.data_ptr() + 4 * odl, dmod.data_ptr() + 4 * (odl + D), NM, Me, D, *top)
            else:
                g.add('mdt_ln_modulate_bwd', ws['dxn'].data_ptr(), xs_e[-1].data_ptr(), st_dl.data_ptr(), mod.data_ptr() + 4 * (odl + D),
                      NM, L, dxe.data_ptr(), 0, dmod.data_ptr() + 4 * odl, dmod.data_ptr() + 4 * (odl + D), NM, Me, D)
        dmod16 = self.b16('dmod16', Bp, NM)

        def ada_group(name, r0, r1):
            """modulation columns [r0, r1) are final: bias grads, weight grads of those adaLN rows, slab hook"""
            n = r1 - r0
            g.add('mdt_cast_f32_bf16', dmod.data_ptr() + 4 * r0, NM, dmod16.data_ptr() + 2 * r0, NM, B, n, 0)
            g.add('mdt_colsum_bf16', dmod16.data_ptr() + 2 * r0, NM, Gp + 4 * (lay.ada_b + r0), B, n)
            self._tn16(g, dmod16.data_ptr() + 2 * r0, NM, sc16.data_ptr(), D, Bp, n, D, Gp + 4 * (lay.ada_w + r0 * D), D)
            self._slab(name)

        groups = {name: (r0, r1) for name, r0, r1 in lay.ada_groups}
        ada_group('ada_w_dec', *groups['ada_w_dec'])  # final layer, decoder blocks, decoder layer: all done above (no decoder: the final layer's rows)
        self.marks['enc_bwd_begin'] = len(g.calls)  # everything from here on is encoder / conditioning-path backward
        for i in reversed(range(sp.depth)):
            nxt = self._gate_info(f'model.blocks.{i - 1}', 'e', i - 1, mod, dmod, sp.mod_off('enc', i - 1), D) \
                if (i > 0 and FUSE_LN_GATE) else None
            self._block_bwd(f'model.blocks.{i}', 'e', i, xs_e[i], mod, dmod, sp.mod_off('enc', i), D, sp.heads, L, Me, dxe,
                            fuse_next=nxt, skip_first_gate=FUSE_LN_GATE and (sp.use_decoder or i + 1 < sp.depth),
                            lvalid=self.lv_attn)
            self._slab(f'enc{i}')
            if f'ada_w_enc{i}' in groups:  # block i is the lowest block of its group
                ada_group(f'ada_w_enc{i}', *groups[f'ada_w_enc{i}'])
        g.add('mdt_patch_embed_bwd', xin.data_ptr(), None, dxe.data_ptr(), ids32.data_ptr() if ids32 is not None else None,
              2 * T, Gf('model.x_embedder.proj.weight'), Gf('model.x_embedder.proj.bias'), B, sp.C, sp.R, sp.patch, L, D)
        # ---- conditioning path backward ------------------------------------------------------
        dsc = self.f32('dsc', Bp, D)
        dc16 = self.b16('dc16', Bp, D)
        dh1 = self.b16('dh1', Bp, D)
        self._slab('ada_b')  # every group has written its part of the stacked adaLN bias gradient
        # M = batch, N = D, K = every modulation output (221 k on XL/2): split the contraction
        self._nt16(g, dmod16.data_ptr(), NM, WT('ada'), NM, B, D, NM, epi=EPI_F32, outf=dsc.data_ptr(), ldof=D,
                   k_splits=max(1, min(64, NM // 2048, 1024 // (((B + 127) // 128) * (D // 128)))))
        g.add('mdt_silu_bwd', dsc.data_ptr(), c.data_ptr(), dc16.data_ptr(), B * D)
        self._tn16(g, dc16.data_ptr(), D, lab16.data_ptr(), YPAD, Bp, D, YPAD, Gf('model.y_embedder.embedding_table.weight'),
                   sp.num_classes, n1v=D, n2v=sp.num_classes)
        self._tn16(g, dc16.data_ptr(), D, a1.data_ptr(), D, Bp, D, D, Gf('model.t_embedder.mlp.2.weight'), D)
        g.add('mdt_colsum_bf16', dc16.data_ptr(), D, Gf('model.t_embedder.mlp.2.bias'), B, D)
        self._nt16(g, dc16.data_ptr(), D, WT('model.t_embedder.mlp.2.weight'), D, B, D, D, epi=EPI_DSILU, out=dh1.data_ptr(), ldo=D,
                   aux=h1.data_ptr(), ldaux=D)
        self._tn16(g, dh1.data_ptr(), D, temb.data_ptr(), 256, Bp, D, 256, Gf('model.t_embedder.mlp.0.weight'), 256)
        g.add('mdt_colsum_bf16', dh1.data_ptr(), D, Gf('model.t_embedder.mlp.0.bias'), B, D)
        self._slab('misc')

    # ---- the fp32-faithful plans (csrc/f32path.hip, csrc/f32train.hip) -----------------------------
    def _build_f32(self):
        """The eval forward in EXACT fp32 -- what the reference's sampler runs (sample.py:56 `net(x_hat.float(), ...)`, no
        autocast in generate.py): fp32 master weights straight from the parameter arena (no bf16 shadow is read), fp32
        activations, fp32-input MFMA GEMMs (mdt_gemm_f32), attention as q k^T -> row softmax -> p v over the packed qkv
        buffer.  Same graph as _build (DiT.forward, models/maskdit.py:511-557, unmasked), same input / output buffers
        (_io), so the sampler and EDMPrecond.forward drive either plan the same way.  Precision 'bf16x3' builds the same
        graph with every Linear layer on mdt_gemm_bf16x3 (see _g32)."""
        self._fwd_f32(save=False)

    def _fwd_f32(self, save: bool):
        """The fp32 forward, emitted once for both fp32 builders.  `save`: keep what a backward needs -- every block gets
        buffers of its own (the inference plan shares one set per stack and ping-pongs the residual stream), and the
        activations (SiLU of the timestep MLP, GELU) and gate + residual adds are passes of their own instead of GEMM
        epilogues, so that the pre-activations h1 / h and the branch outputs survive.  Returns the residual-stream buffers
        (xs_e, xs_d): input of encoder / decoder block i at [i], the stack's output last."""
        eng, sp, lay = self.eng, self.eng.sp, self.eng.lay
        B, T, D, Dd = self.B, self.T, sp.D, sp.Dd
        NM = sp.n_mod
        assert not self.masked
        if sp.num_classes % 4:
            raise NotImplementedError('fp32 path: num_classes must be a multiple of 4 (16-byte label rows)')
        if B * max(sp.heads, sp.dheads) > 65535:
            raise NotImplementedError('fp32 path: batch * heads must not exceed 65535 (one grid row per (sample, head))')
        Pf, Pp = self.Pf, eng.P.data_ptr()
        f = self.fwd
        xin, cn, lab, _, Fx = self._io()
        # ---------------- conditioning path (TimestepEmbedder :34-60, LabelEmbedder :75, SiLU + adaLN Linears :183-186)
        temb, a1 = self.f32('temb', B, 256), self.f32('a1', B, D)
        c_t, c, sc = self.f32('c_t', B, D), self.f32('c', B, D), self.f32('sc', B, D)
        mod = self.f32('mod', B, NM)
        f.add('mdt_timestep_embed_f32', cn.data_ptr(), temb.data_ptr(), 256, B, 256)
        if save:
            h1 = self.f32('h1', B, D)
            self._g32(temb, 256, Pf('model.t_embedder.mlp.0.weight'), 256, B, D, 256, h1, D, bias=Pf('model.t_embedder.mlp.0.bias'))
            f.add('mdt_silu_f32', h1.data_ptr(), a1.data_ptr(), B * D)
        else:
            self._g32(temb, 256, Pf('model.t_embedder.mlp.0.weight'), 256, B, D, 256, a1, D, bias=Pf('model.t_embedder.mlp.0.bias'),
                      epi=F32EPI_SILU)
        self._g32(a1, D, Pf('model.t_embedder.mlp.2.weight'), D, B, D, D, c_t, D, bias=Pf('model.t_embedder.mlp.2.bias'))
        # c = t_emb + y @ table^T (the one-hot / zero / soft label row times the embedding table)
        self._g32(lab, sp.num_classes, Pf('model.y_embedder.embedding_table.weight'), sp.num_classes, B, D, sp.num_classes, c, D,
                  epi=F32EPI_GATE_RES, res=c_t, ldres=D, rps=1)
        f.add('mdt_silu_f32', c.data_ptr(), sc.data_ptr(), B * D)
        self._g32(sc, D, Pp + 4 * lay.ada_w, D, B, NM, D, mod, NM, bias=Pp + 4 * lay.ada_b)
        # ---------------- encoder (all T tokens: masking applies in train mode only, models/maskdit.py:482,539) ---------
        M = B * T
        xs_e = [self.f32('x_e0', M, D)]
        f.add('mdt_patch_embed_fwd', xin.data_ptr(), None, Pf('model.x_embedder.proj.weight'), Pf('model.x_embedder.proj.bias'),
              eng.pos.data_ptr(), None, 2 * T, xs_e[0].data_ptr(), B, sp.C, sp.R, sp.patch, T, D)
        for i in range(sp.depth):
            xs_e.append(self._block_fwd_f32(f'model.blocks.{i}', 'e', i, xs_e[-1], mod, sp.mod_off('enc', i), D, sp.heads, T, M, save))
        self.marks = {'enc_fwd_end': len(f.calls)}
        if not sp.use_decoder:  # (:529-553) the final layer reads the encoder's rows; every token is present
            st_f = self.f32('st_f', M, 2)
            ofin = sp.mod_off('fin')
            f.add('mdt_final_keep_fwd', xs_e[-1].data_ptr(), mod.data_ptr() + 4 * ofin, mod.data_ptr() + 4 * (ofin + D), NM,
                  Pf('model.final_layer.linear.weight'), Pf('model.final_layer.linear.bias'), None, 2 * T, Fx.data_ptr(),
                  st_f.data_ptr(), B, T, T, T, D, sp.C, sp.patch)
            return xs_e, []
        # ---------------- DecoderLayer (:195-213) + decoder_pos_embed (:545) -------------------------------------------
        odl = sp.mod_off('dl')
        xn_e, xdec = self.f32('xn_e', M, D), self.f32('xdec', M, Dd)
        f.add('mdt_ln_modulate_f32', xs_e[-1].data_ptr(), mod.data_ptr() + 4 * odl, mod.data_ptr() + 4 * (odl + D), NM, T,
              xn_e.data_ptr(), M, D)
        self._g32(xn_e, D, Pf('model.decoder_layer.linear.weight'), D, M, Dd, D, xdec, Dd, bias=Pf('model.decoder_layer.linear.bias'))
        xs_d = [self.f32('x_d0', M, Dd)]
        f.add('mdt_add_rows_f32', xdec.data_ptr(), eng.dpos.data_ptr(), xs_d[0].data_ptr(), M, T, Dd)
        for i in range(sp.ddepth):
            xs_d.append(self._block_fwd_f32(f'model.decoder_blocks.{i}', 'd', i, xs_d[-1], mod, sp.mod_off('dec', i), Dd, sp.dheads, T, M,
                                            save))
        ofin = sp.mod_off('fin')
        st_f = self.f32('st_f', M, 2)
        f.add('mdt_final_fwd', xs_d[-1].data_ptr(), mod.data_ptr() + 4 * ofin, mod.data_ptr() + 4 * (ofin + Dd), NM,
              Pf('model.final_layer.linear.weight'), Pf('model.final_layer.linear.bias'), Fx.data_ptr(), st_f.data_ptr(),
              B, T, Dd, sp.C, sp.patch)
        return xs_e, xs_d

    # ---- fp32 training of the unmasked stage (csrc/f32train.hip) -----------------------------------------------------
    @staticmethod
    def _ada_kchunk(NM: int) -> int:
        """Chunk of the stacked adaLN data-gradient contraction: the largest divisor of NM that is a multiple of 4 and <= 1024."""
        return next(c for c in range(1024, 3, -4) if NM % c == 0)

    @staticmethod
    def _f32_train_ws(sp, B: int) -> Tuple[int, int, int]:
        """Floats of the three library workspaces of an fp32 training plan: transposed products, column sums, attention
        backward -- each the largest request among the plan's launches (queried from the library)."""
        L = _lib.lib()
        M, NM, D, Dd = B * sp.T, sp.n_mod, sp.D, sp.Dd
        tn_shapes = [(B, NM, D), (B, D, sp.num_classes), (B, D, D), (B, D, 256), (M, Dd, D)]
        for W in (D, Dd):
            tn_shapes += [(M, W, 4 * W), (M, 4 * W, W), (M, W, W), (M, 3 * W, W)]
        tn = max(int(L.mdt_gemm_f32_tn_ws_floats(m, n1, n2, 1)) for m, n1, n2 in tn_shapes)
        cs = max(int(L.mdt_colsum_f32_ws_floats(M, 4 * max(D, Dd))), int(L.mdt_colsum_f32_ws_floats(B, NM)),
                 int(L.mdt_colsum_f32_ws_floats(NM // PassPlan._ada_kchunk(NM), B * D)))
        at = max(int(L.mdt_attn_f32_bwd_ws_floats(B, sp.T, sp.heads, sp.hd)), int(L.mdt_attn_f32_bwd_ws_floats(B, sp.T, sp.dheads, sp.dhd)))
        return tn, cs, at

    @staticmethod
    def f32_train_floats(sp, B: int) -> Dict[str, int]:
        """fp32 elements of an fp32 training plan's buffers by group: the figures _build_f32_train allocates."""
        M, W = B * sp.T, max(sp.D, sp.Dd)
        tn, cs, at = PassPlan._f32_train_ws(sp, B)
        saved = 12 * M * (sp.depth * sp.D + sp.ddepth * sp.Dd)  # per block: x_out, qkv (3), ao, f_attn, x_mid, h (4), f_mlp
        stream = M * (sp.D + 2 * sp.Dd) + 2 * M + M * (sp.D + sp.Dd)  # x_e0, x_d0, xdec, final-layer stats, dx_e, dx_d
        shared = 5 * M * (sp.D + sp.Dd)                         # xn + act (4) per stack
        work = 10 * M * W + 2 * M                               # df, dh (4), dxn, dao, dqkv (3), LayerNorm statistics
        cond = B * (2 * sp.n_mod + (9 + sp.n_mod // PassPlan._ada_kchunk(sp.n_mod)) * sp.D + 256 + sp.num_classes + 8) + 6 * B * sp.C * sp.R * sp.R
        return dict(saved=saved, stream=stream, shared=shared, work=work, attn=at, wgrad=tn + cs, cond=cond)

    @staticmethod
    def estimate_bytes_f32_train(sp, B: int) -> int:
        return int(4 * sum(PassPlan.f32_train_floats(sp, B).values()) * 1.02)

    def _build_f32_train(self):
        """Forward + backward of the UNMASKED training step in exact fp32: the reference's second stage ("finetune with
        unmasking", README.md:102-119: mask_ratio 0, train.py --no_amp).  The forward is _build_f32's graph, walked with
        `save` (_fwd_f32); the backward is the hand-derived gradient of the same graph, filling the gradient arena the
        bf16 plan fills with the same `+=` semantics.  Weights are read from the fp32 master arena: no bf16 shadow is
        involved.  LayerNorm outputs and GELU outputs are recomputed in the backward instead of being kept (12 instead of
        18 floats per token, block and channel).  (Engine.plan refuses the masked stage and 'bf16x3' before it gets here.)"""
        eng, sp, lay = self.eng, self.eng.sp, self.eng.lay
        B, T, D, Dd = self.B, self.T, sp.D, sp.Dd
        NM = sp.n_mod
        M = B * T
        # ---- workspaces shared by the whole backward: sized for the largest request ------------------------------------
        Wm = max(D, Dd)
        tn_floats, cs_floats, at_floats = self._f32_train_ws(sp, B)
        tnws = self.f32('ws_tn', max(tn_floats, 4))
        csws = self.f32('ws_colsum', max(cs_floats, 4))
        atws = self.f32('ws_attn', at_floats)
        self._f32ws = ws = dict(tn=(tnws.data_ptr(), tn_floats), cs=(csws.data_ptr(), cs_floats), at=(atws.data_ptr(), at_floats),
                                df=self.f32('ws_df', M * Wm), dh=self.f32('ws_dh', 4 * M * Wm), dxn=self.f32('ws_dxn', M * Wm),
                                dao=self.f32('ws_dao', M * Wm), dqkv=self.f32('ws_dqkv', 3 * M * Wm), stats=self.f32('ws_stats', 2 * M))
        xs_e, xs_d = self._fwd_f32(save=True)
        # =================== backward =====================================================================================
        Pf, Gf, Pp, Gp = self.Pf, self.Gf, eng.P.data_ptr(), eng.G.data_ptr()
        g, b = self.bwd, self.buf
        xin, lab, dF, temb, h1, a1, c, sc, mod, xn_e, st_f = (b[k] for k in ('xin', 'labels', 'dF', 'temb', 'h1', 'a1', 'c', 'sc', 'mod',
                                                                              'xn_e', 'st_f'))
        odl, ofin = sp.mod_off('dl'), sp.mod_off('fin')
        dmod = self.f32('dmod', B, NM)
        dxe, dxd = self.f32('dx_e', M, D), self.f32('dx_d', M, Dd)
        g.add_callback(lambda: dmod.zero_())  # (mdt_final_bwd adds its two modulation gradients; every other column is stored)
        g.add('mdt_final_bwd', dF.data_ptr(), xs_d[-1].data_ptr(), st_f.data_ptr(), mod.data_ptr() + 4 * ofin,
              mod.data_ptr() + 4 * (ofin + Dd), NM, Pf('model.final_layer.linear.weight'), dxd.data_ptr(),
              Gf('model.final_layer.linear.weight'), Gf('model.final_layer.linear.bias'), dmod.data_ptr() + 4 * ofin,
              dmod.data_ptr() + 4 * (ofin + Dd), NM, B, T, Dd, sp.C, sp.patch)
        for i in reversed(range(sp.ddepth)):
            self._block_bwd_f32(f'model.decoder_blocks.{i}', 'd', i, xs_d[i], mod, dmod, sp.mod_off('dec', i), Dd, sp.dheads, T, M, dxd)
            self._slab(f'dec{i}')
        # x_d0 = xdec + decoder_pos_embed: d xdec = dx_d.  mask_token takes no part in an unmasked pass: its gradient stays
        # the zero _prepare_grad_arena wrote (train_utils/loss.py:57-58 adds 0 * mask_token.sum() for the same effect)
        f32 = F32EPI_NONE
        g.add('mdt_ln_modulate_f32', xs_e[-1].data_ptr(), mod.data_ptr() + 4 * odl, mod.data_ptr() + 4 * (odl + D), NM, T,
              xn_e.data_ptr(), M, D)
        self._tn32(dxd, Dd, xn_e, D, M, Dd, D, Gf('model.decoder_layer.linear.weight'), D)
        self._cs32(dxd, Dd, Gf('model.decoder_layer.linear.bias'), M, Dd)
        self._g32(dxd, Dd, Pf('model.decoder_layer.linear.weight'), D, M, D, Dd, ws['dxn'], D, epi=f32, b_kmajor=1, to=g)
        g.add('mdt_ln_modulate_bwd_f32', ws['dxn'].data_ptr(), xs_e[-1].data_ptr(), mod.data_ptr() + 4 * (odl + D), NM, T,
              dxe.data_ptr(), 0, dmod.data_ptr() + 4 * odl, dmod.data_ptr() + 4 * (odl + D), NM, ws['stats'].data_ptr(), M, D)
        self.marks['enc_bwd_begin'] = len(g.calls)
        for i in reversed(range(sp.depth)):
            self._block_bwd_f32(f'model.blocks.{i}', 'e', i, xs_e[i], mod, dmod, sp.mod_off('enc', i), D, sp.heads, T, M, dxe)
            self._slab(f'enc{i}')
        g.add('mdt_patch_embed_bwd', xin.data_ptr(), None, dxe.data_ptr(), None, 2 * T, Gf('model.x_embedder.proj.weight'),
              Gf('model.x_embedder.proj.bias'), B, sp.C, sp.R, sp.patch, T, D)
        # ---- every modulation gradient is final: the stacked adaLN Linear (one weight-gradient product), then the
        # conditioning path (SiLU, label table, timestep MLP) ------------------------------------------------------------
        self._tn32(dmod, NM, sc, D, B, NM, D, Gp + 4 * lay.ada_w, D)
        self._cs32(dmod, NM, Gp + 4 * lay.ada_b, B, NM)
        for name, _, _ in lay.ada_groups:
            self._slab(name)
        self._slab('ada_b')
        dsc, dc, da1 = self.f32('dsc', B, D), self.f32('dc', B, D), self.f32('da1', B, D)
        # d silu(c) = dmod W_ada contracts over EVERY modulation output (54 k on S/2, 221 k on XL/2): one fp32 accumulator chain
        # of that length loses ~ sqrt(K) ulp against a blocked sum, so the contraction is cut into equal chunks (one batched
        # launch, one partial [B, D] per chunk) that mdt_colsum_f32 adds in chunk order
        ck = self._ada_kchunk(NM)
        nch = NM // ck
        dsc_part = self.f32('dsc_part', nch, B, D)
        self._g32(dmod, NM, Pp + 4 * lay.ada_w, D, B, D, ck, dsc_part, D, epi=f32, b_kmajor=1, batch=nch, heads=1, a_s=(ck, 0),
                  b_s=(ck * D, 0), o_s=(B * D, 0), to=g)
        g.add('mdt_colsum_f32', dsc_part.data_ptr(), B * D, dsc.data_ptr(), ws['cs'][0], ws['cs'][1], nch, B * D, 0)
        g.add('mdt_silu_bwd_f32', dsc.data_ptr(), c.data_ptr(), dc.data_ptr(), B * D)
        self._tn32(dc, D, lab, sp.num_classes, B, D, sp.num_classes, Gf('model.y_embedder.embedding_table.weight'), sp.num_classes)
        self._tn32(dc, D, a1, D, B, D, D, Gf('model.t_embedder.mlp.2.weight'), D)
        self._cs32(dc, D, Gf('model.t_embedder.mlp.2.bias'), B, D)
        self._g32(dc, D, Pf('model.t_embedder.mlp.2.weight'), D, B, D, D, da1, D, epi=f32, b_kmajor=1, to=g)
        g.add('mdt_silu_bwd_f32', da1.data_ptr(), h1.data_ptr(), da1.data_ptr(), B * D)
        self._tn32(da1, D, temb, 256, B, D, 256, Gf('model.t_embedder.mlp.0.weight'), 256)
        self._cs32(da1, D, Gf('model.t_embedder.mlp.0.bias'), B, D)
        self._slab('misc')

    def _tn32(self, A, lda, Bm, ldb, M, N1, N2, Cp, ldc):
        """One mdt_gemm_f32_tn launch of the backward plan: C += A^T B into the gradient arena (address Cp)."""
        a = GemmF32TNArgs()
        a.A, a.lda, a.B, a.ldb = A.data_ptr(), lda, Bm.data_ptr(), ldb
        a.M, a.N1, a.N2 = M, N1, N2
        a.C, a.ldc, a.accumulate = Cp, ldc, 1
        a.ws, a.ws_floats = self._f32ws['tn']
        self.bwd.add('mdt_gemm_f32_tn', C.byref(self._k(a)))

    def _cs32(self, A, ld, outp, M, N):
        """bias gradient: out += column sums of A"""
        wsp, wsn = self._f32ws['cs']
        self.bwd.add('mdt_colsum_f32', A.data_ptr(), ld, outp, wsp, wsn, M, N, 1)

    def _block_bwd_f32(self, prefix, tag, i, x_in, mod, dmod, moff, W, heads, rows, M, dx):
        """Backward of DiTBlock in fp32: dx (the residual-stream gradient) is updated in place."""
        g, ws = self.bwd, self._f32ws
        NM = self.eng.sp.n_mod
        hd = W // heads
        B = self.B
        s = f'{tag}{i}'
        p, Pf, Gf = prefix + '.', self.Pf, self.Gf
        mp, dp = mod.data_ptr(), dmod.data_ptr()
        sh1, sc1, g1, sh2, sc2, g2 = (mp + 4 * (moff + k * W) for k in range(6))
        dsh1, dsc1, dg1, dsh2, dsc2, dg2 = (dp + 4 * (moff + k * W) for k in range(6))
        b = self.buf
        xn, act = b[f'xn_{tag}'], b[f'act_{tag}']
        qkv, ao, fa, xmid, h, fm = (b[f'{k}_{s}'] for k in ('qkv', 'ao', 'fa', 'xmid', 'h', 'fm'))
        df, dh, dxn, dao, dqkv, stats = (ws[k] for k in ('df', 'dh', 'dxn', 'dao', 'dqkv', 'stats'))
        dxp = dx.data_ptr()
        none = F32EPI_NONE
        # --- MLP branch: x_out = x_mid + g2 * fc2(gelu(fc1(xn2)))
        g.add('mdt_gate_bwd_f32', dxp, fm.data_ptr(), g2, NM, rows, df.data_ptr(), dg2, NM, M, W)
        g.add('mdt_gelu_f32', h.data_ptr(), act.data_ptr(), M * 4 * W)
        self._tn32(df, W, act, 4 * W, M, W, 4 * W, Gf(p + 'mlp.fc2.weight'), 4 * W)
        self._cs32(df, W, Gf(p + 'mlp.fc2.bias'), M, W)
        self._g32(df, W, Pf(p + 'mlp.fc2.weight'), 4 * W, M, 4 * W, W, dh, 4 * W, epi=none, b_kmajor=1, to=g)
        g.add('mdt_gelu_bwd_f32', dh.data_ptr(), h.data_ptr(), dh.data_ptr(), M * 4 * W)
        g.add('mdt_ln_modulate_f32', xmid.data_ptr(), sh2, sc2, NM, rows, xn.data_ptr(), M, W)
        self._tn32(dh, 4 * W, xn, W, M, 4 * W, W, Gf(p + 'mlp.fc1.weight'), W)
        self._cs32(dh, 4 * W, Gf(p + 'mlp.fc1.bias'), M, 4 * W)
        self._g32(dh, 4 * W, Pf(p + 'mlp.fc1.weight'), W, M, W, 4 * W, dxn, W, epi=none, b_kmajor=1, to=g)
        g.add('mdt_ln_modulate_bwd_f32', dxn.data_ptr(), xmid.data_ptr(), sc2, NM, rows, dxp, 1, dsh2, dsc2, NM, stats.data_ptr(), M, W)
        # --- attention branch: x_mid = x_in + g1 * proj(attn(qkv(xn1)))
        g.add('mdt_gate_bwd_f32', dxp, fa.data_ptr(), g1, NM, rows, df.data_ptr(), dg1, NM, M, W)
        self._tn32(df, W, ao, W, M, W, W, Gf(p + 'attn.proj.weight'), W)
        self._cs32(df, W, Gf(p + 'attn.proj.bias'), M, W)
        self._g32(df, W, Pf(p + 'attn.proj.weight'), W, M, W, W, dao, W, epi=none, b_kmajor=1, to=g)
        g.add('mdt_attn_f32_bwd', qkv.data_ptr(), dao.data_ptr(), ws['at'][0], ws['at'][1], dqkv.data_ptr(), B, rows, heads, hd)
        g.add('mdt_ln_modulate_f32', x_in.data_ptr(), sh1, sc1, NM, rows, xn.data_ptr(), M, W)
        self._tn32(dqkv, 3 * W, xn, W, M, 3 * W, W, Gf(p + 'attn.qkv.weight'), W)
        self._cs32(dqkv, 3 * W, Gf(p + 'attn.qkv.bias'), M, 3 * W)
        self._g32(dqkv, 3 * W, Pf(p + 'attn.qkv.weight'), W, M, W, 3 * W, dxn, W, epi=none, b_kmajor=1, to=g)
        g.add('mdt_ln_modulate_bwd_f32', dxn.data_ptr(), x_in.data_ptr(), sc1, NM, rows, dxp, 1, dsh1, dsc1, NM, stats.data_ptr(), M, W)

    def _g32(self, A, lda, Bw, ldb, M, N, K, out, ldo, bias=0, epi=F32EPI_NONE, res=None, ldres=0, gate=0, gate_ld=0, rps=1,
             b_kmajor=0, batch=0, heads=0, a_s=(0, 0), b_s=(0, 0), o_s=(0, 0), to=None):
        """One mdt_gemm_f32 launch -- mdt_gemm_bf16x3 for a Linear layer of a 'bf16x3' plan; A / out / res are tensors or
        raw addresses, Bw / bias / gate raw addresses."""
        ptr = lambda t: t if isinstance(t, int) else t.data_ptr()  # noqa: E731
        a = GemmF32Args()
        a.A, a.lda, a.B, a.ldb, a.b_kmajor = ptr(A), lda, Bw, ldb, b_kmajor
        a.M, a.N, a.K = M, N, K
        a.bias, a.epi = bias or None, epi
        a.out, a.ldo = ptr(out), ldo
        a.res, a.ldres = (ptr(res) if res is not None else None), ldres
        a.gate, a.gate_ld, a.rows_per_sample = gate or None, gate_ld, rps
        a.batch, a.heads = batch, heads
        a.a_stride_b, a.a_stride_h = a_s
        a.b_stride_b, a.b_stride_h = b_s
        a.o_stride_b, a.o_stride_h = o_s
        x3 = self.precision == 'bf16x3' and batch <= 1 and not b_kmajor
        (to or self.fwd).add('mdt_gemm_bf16x3' if x3 else 'mdt_gemm_f32', C.byref(self._k(a)))

    def _block_fwd_f32(self, prefix, tag, i, x_in, mod, moff, W, heads, rows, M, save):
        """DiTBlock.forward (models/maskdit.py:188-192) in fp32.  Inference (`save` False): all blocks of a stack share one
        buffer set, GELU and gate + residual are GEMM epilogues.  `save`: the block keeps qkv, the attention output, both
        branch outputs f, x_mid and the pre-GELU h for its backward."""
        f, Pf, p = self.fwd, self.Pf, prefix + '.'
        NM = self.eng.sp.n_mod
        hd = W // heads
        B = self.B
        s = f'{tag}{i}' if save else tag
        mp = mod.data_ptr()
        sh1, sc1, g1, sh2, sc2, g2 = (mp + 4 * (moff + k * W) for k in range(6))
        xn = self.f32(f'xn_{tag}', M, W)  # (shared by the stack in either plan: the backward recomputes it)
        qkv, ao = self.f32(f'qkv_{s}', M, 3 * W), self.f32(f'ao_{s}', M, W)
        xmid, h = self.f32(f'xmid_{s}', M, W), self.f32(f'h_{s}', M, 4 * W)
        xout = self.f32(f'x_{tag}{i + 1}' if save else f'x_{tag}pp{(i + 1) % 2}', M, W)
        S = None  # attention scores; no workspace where the fused single-launch kernel serves the shape
        ws_floats = int(_lib.lib().mdt_attn_f32_ws_floats(B, rows, heads, hd))
        if ws_floats:  # (the backward's score workspace is at least twice as large)
            S = self._f32ws['at'][0] if save else self.f32(f'scores_{tag}', ws_floats).data_ptr()

        def branch(a, K, wname, res, gate, y, out):
            """out = res + gate * Linear(a): in the GEMM's epilogue, or (save) y = Linear(a) kept and the rest a pass"""
            if save:
                self._g32(a, K, Pf(p + wname + '.weight'), K, M, W, K, self.f32(y, M, W), W, bias=Pf(p + wname + '.bias'))
                f.add('mdt_gate_res_f32', res.data_ptr(), self.buf[y].data_ptr(), gate, NM, rows, out.data_ptr(), M, W)
            else:
                self._g32(a, K, Pf(p + wname + '.weight'), K, M, W, K, out, W, bias=Pf(p + wname + '.bias'), epi=F32EPI_GATE_RES,
                          res=res, ldres=W, gate=gate, gate_ld=NM, rps=rows)

        f.add('mdt_ln_modulate_f32', x_in.data_ptr(), sh1, sc1, NM, rows, xn.data_ptr(), M, W)
        self._g32(xn, W, Pf(p + 'attn.qkv.weight'), W, M, 3 * W, W, qkv, 3 * W, bias=Pf(p + 'attn.qkv.bias'))
        # timm Attention: softmax(q k^T * hd^-0.5) v per (sample, head) on the packed [M, (3, heads, hd)] buffer
        f.add('mdt_attn_f32', qkv.data_ptr(), ao.data_ptr(), S, B, rows, heads, hd)
        branch(ao, W, 'attn.proj', x_in, g1, f'fa_{s}', xmid)
        f.add('mdt_ln_modulate_f32', xmid.data_ptr(), sh2, sc2, NM, rows, xn.data_ptr(), M, W)
        self._g32(xn, W, Pf(p + 'mlp.fc1.weight'), W, M, 4 * W, W, h, 4 * W, bias=Pf(p + 'mlp.fc1.bias'),
                  epi=F32EPI_NONE if save else F32EPI_GELU)
        act = h
        if save:  # (shared by the stack: the backward recomputes it from h)
            act = self.f32(f'act_{tag}', M, 4 * W)
            f.add('mdt_gelu_f32', h.data_ptr(), act.data_ptr(), M * 4 * W)
        branch(act, 4 * W, 'mlp.fc2', xmid, g2, f'fm_{s}', xout)
        return xout

    def _k(self, obj):
        """Every ctypes struct a launch refers to stays alive as long as the plan."""
        self.fwd.keep.append(obj)
        return obj

    def _nt16(self, to: Plan, *a, **kw):
        """One mdt_gemm_nt launch appended to `to` (arguments: _nt)."""
        to.add('mdt_gemm_nt', C.byref(self._k(_nt(*a, **kw))))

    def _tn16(self, to: Plan, *a, **kw):
        """One mdt_gemm_tn launch appended to `to` (arguments: _tn)."""
        to.add('mdt_gemm_tn', C.byref(self._k(_tn(*a, **kw))))

    def _slab(self, name):
        ref = self._eng_ref
        lo, hi = self.eng.lay.slabs[name]

        def cb():
            eng = ref()
            if eng is not None and eng.grad_slab_hook is not None:
                eng.grad_slab_hook(name, lo, hi)

        self.bwd.add_callback(cb)

    def _block_fwd(self, prefix, tag, i, x_in, mod, moff, W, heads, rows, M, lvalid=0, pending=None, defer_out=False):
        """DiTBlock.forward (models/maskdit.py:188-192) as 7 launches.  `pending` = (xres, y, gate) of the previous block's
        MLP branch: this block's first LayerNorm pass then forms x_in = xres + gate * y itself (FUSE_RES_LN); `defer_out`
        hands this block's own MLP residual to whoever normalises its output next.  Returns (x_out buffer, pending)."""
        f = self.fwd
        NM = self.eng.sp.n_mod
        hd = W // heads
        B = self.B
        s = f'{tag}{i}' if self.train else f'{tag}'  # eval: all blocks share one buffer set
        p, Pf, Wp = prefix + '.', self.Pf, self.Wp
        mp = mod.data_ptr()
        sh1, sc1, g1, sh2, sc2, g2 = (mp + 4 * (moff + k * W) for k in range(6))
        xn1, st1 = self.b16(f'xn1_{s}', M, W), self.f32(f'st1_{s}', M, 2)
        qkv = self.b16(f'qkv_{s}', M, 3 * W)
        ao, lse = self.b16(f'ao_{s}', M, W), self.f32(f'lse_{s}', B * heads * rows)
        ya = self.b16(f'ya_{s}', M, W)
        xmid = self.f32(f'xmid_{s}', M, W)
        xn2, st2 = self.b16(f'xn2_{s}', M, W), self.f32(f'st2_{s}', M, 2)
        h, a = self.b16(f'h_{s}', M, 4 * W), self.b16(f'a_{s}', M, 4 * W)
        ym = self.b16(f'ym_{s}', M, W)
        if self.train:
            xout = self.f32(f'x_{tag}{i + 1}', M, W)
        else:  # ping-pong
            xout = self.f32(f'x_{tag}pp{(i + 1) % 2}', M, W)
        tr = self.train
        fuse = FUSE_RES_LN and (tr or FUSE_RES_LN_EVAL)
        if pending is not None:  # x_in = xres + gate * y (the previous block's MLP residual) is formed by this pass
            f.add('mdt_ln_modulate_fwd_res', pending[0].data_ptr(), pending[1].data_ptr(), pending[2], NM, sh1, sc1, NM, rows,
                  x_in.data_ptr(), xn1.data_ptr(), st1.data_ptr(), M, W)
        else:
            f.add('mdt_ln_modulate_fwd', x_in.data_ptr(), sh1, sc1, NM, rows, xn1.data_ptr(), st1.data_ptr(), M, W)
        self._nt16(f, xn1.data_ptr(), W, Wp(p + 'attn.qkv.weight'), W, M, 3 * W, W, bias=Pf(p + 'attn.qkv.bias'), epi=EPI_BF16,
                   out=qkv.data_ptr(), ldo=3 * W)
        f.add('mdt_attn_fwd', qkv.data_ptr(), ao.data_ptr(), lse.data_ptr(), B, rows, heads, hd, lvalid)
        # the bf16 copies of the branch outputs (ya, ym) and the pre-activation h are saved for the
        # backward only: inference plans skip those stores (2 of 10 resp. 2 of 4 epilogue bytes / element)
        if fuse:  # the GEMM stores y only; x_mid = x_in + g1 * y is formed by the LayerNorm pass that consumes it
            self._nt16(f, ao.data_ptr(), W, Wp(p + 'attn.proj.weight'), W, M, W, W, bias=Pf(p + 'attn.proj.bias'), epi=EPI_BF16,
                       out=ya.data_ptr(), ldo=W)
            f.add('mdt_ln_modulate_fwd_res', x_in.data_ptr(), ya.data_ptr(), g1, NM, sh2, sc2, NM, rows, xmid.data_ptr(),
                  xn2.data_ptr(), st2.data_ptr(), M, W)
        else:
            self._nt16(f, ao.data_ptr(), W, Wp(p + 'attn.proj.weight'), W, M, W, W, bias=Pf(p + 'attn.proj.bias'), epi=EPI_GATE_RES,
                       out=ya.data_ptr() if tr else 0, ldo=W, outf=xmid.data_ptr(), ldof=W, res=x_in.data_ptr(), ldres=W,
                       gate=g1, gate_ld=NM, rps=rows)
            f.add('mdt_ln_modulate_fwd', xmid.data_ptr(), sh2, sc2, NM, rows, xn2.data_ptr(), st2.data_ptr(), M, W)
        self._nt16(f, xn2.data_ptr(), W, Wp(p + 'mlp.fc1.weight'), W, M, 4 * W, W, bias=Pf(p + 'mlp.fc1.bias'), epi=EPI_GELU,
                   out=h.data_ptr() if tr else 0, ldo=4 * W, out2=a.data_ptr(), ldo2=4 * W)
        if fuse and defer_out:
            self._nt16(f, a.data_ptr(), 4 * W, Wp(p + 'mlp.fc2.weight'), 4 * W, M, W, 4 * W, bias=Pf(p + 'mlp.fc2.bias'), epi=EPI_BF16,
                       out=ym.data_ptr(), ldo=W)
            return xout, (xmid, ym, g2)
        self._nt16(f, a.data_ptr(), 4 * W, Wp(p + 'mlp.fc2.weight'), 4 * W, M, W, 4 * W, bias=Pf(p + 'mlp.fc2.bias'), epi=EPI_GATE_RES,
                   out=ym.data_ptr() if tr else 0, ldo=W, outf=xout.data_ptr(), ldof=W, res=xmid.data_ptr(), ldres=W,
                   gate=g2, gate_ld=NM, rps=rows)
        return xout, None

    def _gate_info(self, prefix, tag, i, mod, dmod, moff, W):
        """Trailing arguments of mdt_ln_modulate_bwd_gate for the MLP residual gate of block (tag, i):
        (y = fc2 output, gate, gate_ld, dys, dgate, dgate_ld, dbias)."""
        NM = self.eng.sp.n_mod
        ym = self.buf[f'ym_{tag}{i}']
        return (ym.data_ptr(), mod.data_ptr() + 4 * (moff + 5 * W), NM, self._ws['dys'].data_ptr(),
                dmod.data_ptr() + 4 * (moff + 5 * W), NM, self.Gf(f'{prefix}.mlp.fc2.bias'))

    def _block_bwd(self, prefix, tag, i, x_in, mod, dmod, moff, W, heads, rows, M, dx, fuse_next=None, skip_first_gate=False,
                   lvalid=0):
        """Backward of DiTBlock: dx (fp32 residual-stream gradient) is updated in place.  The gate
        backward that opens the block is folded into the LayerNorm backward that precedes it in stream
        order (`skip_first_gate`), and the block's last LayerNorm backward carries the next block's
        (`fuse_next`)."""
        g, ws = self.bwd, self._ws
        NM = self.eng.sp.n_mod
        hd = W // heads
        B = self.B
        s = f'{tag}{i}'
        p, WT, Gf = prefix + '.', self.WT, self.Gf
        mp, dp = mod.data_ptr(), dmod.data_ptr()
        sc1, g1, sc2, g2 = mp + 4 * (moff + W), mp + 4 * (moff + 2 * W), mp + 4 * (moff + 4 * W), mp + 4 * (moff + 5 * W)
        dsh1, dsc1, dg1, dsh2, dsc2, dg2 = (dp + 4 * (moff + k * W) for k in range(6))
        b = self.buf
        xn1, st1, qkv, ao, lse = b[f'xn1_{s}'], b[f'st1_{s}'], b[f'qkv_{s}'], b[f'ao_{s}'], b[f'lse_{s}']
        ya, xmid, xn2, st2, h, a, ym = b[f'ya_{s}'], b[f'xmid_{s}'], b[f'xn2_{s}'], b[f'st2_{s}'], b[f'h_{s}'], b[f'a_{s}'], b[f'ym_{s}']
        dys, dh, dxn, dao, dqkv, delta = (ws[k].data_ptr() for k in ('dys', 'dh', 'dxn', 'dao', 'dqkv', 'delta'))
        dxp = dx.data_ptr()
        # --- MLP branch: x_out = x_mid + g2 * (fc2(gelu(fc1(xn2))))
        if not skip_first_gate:
            g.add('mdt_gate_bwd', dxp, ym.data_ptr(), g2, NM, rows, dys, dg2, NM, Gf(p + 'mlp.fc2.bias'), M, W)
        self._tn16(g, dys, W, a.data_ptr(), 4 * W, M, W, 4 * W, Gf(p + 'mlp.fc2.weight'), 4 * W)
        # dh = (dys W2) * gelu'(h); its column sums (= d fc1.bias) come out of the same epilogue
        self._nt16(g, dys, W, WT(p + 'mlp.fc2.weight'), W, M, 4 * W, W, epi=EPI_DGELU, out=dh, ldo=4 * W, aux=h.data_ptr(),
                   ldaux=4 * W, colsum=Gf(p + 'mlp.fc1.bias') if FUSE_COLSUM else 0)
        self._tn16(g, dh, 4 * W, xn2.data_ptr(), W, M, 4 * W, W, Gf(p + 'mlp.fc1.weight'), W)
        if not FUSE_COLSUM:
            g.add('mdt_colsum_bf16', dh, 4 * W, Gf(p + 'mlp.fc1.bias'), M, 4 * W)
        self._nt16(g, dh, 4 * W, WT(p + 'mlp.fc1.weight'), 4 * W, M, W, 4 * W, epi=EPI_BF16, out=dxn, ldo=W)
        # --- attention branch: x_mid = x_in + g1 * proj(attn(qkv(xn1)))
        if FUSE_LN_GATE:  # the gate backward rides on LN2's backward
            g.add('mdt_ln_modulate_bwd_gate', dxn, xmid.data_ptr(), st2.data_ptr(), sc2, NM, rows, dxp, 1, dsh2, dsc2, NM, M, W,
                  ya.data_ptr(), g1, NM, dys, dg1, NM, Gf(p + 'attn.proj.bias'))
        else:
            g.add('mdt_ln_modulate_bwd', dxn, xmid.data_ptr(), st2.data_ptr(), sc2, NM, rows, dxp, 1, dsh2, dsc2, NM, M, W)
            g.add('mdt_gate_bwd', dxp, ya.data_ptr(), g1, NM, rows, dys, dg1, NM, Gf(p + 'attn.proj.bias'), M, W)
        self._tn16(g, dys, W, ao.data_ptr(), W, M, W, W, Gf(p + 'attn.proj.weight'), W)
        self._nt16(g, dys, W, WT(p + 'attn.proj.weight'), W, M, W, W, epi=EPI_BF16, out=dao, ldo=W)
        g.add('mdt_attn_bwd', qkv.data_ptr(), ao.data_ptr(), dao, lse.data_ptr(), delta, dqkv, B, rows, heads, hd, lvalid)
        # the qkv bias gradient (column sums of dqkv) comes out of the weight-gradient GEMM, which streams dqkv through
        # LDS anyway (mdt_gemm_tn_args.colsum_a): one pass over dqkv less per block
        self._tn16(g, dqkv, 3 * W, xn1.data_ptr(), W, M, 3 * W, W, Gf(p + 'attn.qkv.weight'), W,
                   colsum_a=Gf(p + 'attn.qkv.bias') if FUSE_QKV_COLSUM else 0)
        if not FUSE_QKV_COLSUM:
            g.add('mdt_colsum_bf16', dqkv, 3 * W, Gf(p + 'attn.qkv.bias'), M, 3 * W)
        self._nt16(g, dqkv, 3 * W, WT(p + 'attn.qkv.weight'), 3 * W, M, W, 3 * W, epi=EPI_BF16, out=dxn, ldo=W)
        if fuse_next is not None:
            g.add('mdt_ln_modulate_bwd_gate', dxn, x_in.data_ptr(), st1.data_ptr(), sc1, NM, rows, dxp, 1, dsh1, dsc1, NM, M, W,
                  *fuse_next)
        else:
            g.add('mdt_ln_modulate_bwd', dxn, x_in.data_ptr(), st1.data_ptr(), sc1, NM, rows, dxp, 1, dsh1, dsc1, NM, M, W)

    # ---- execution ---------------------------------------------------------------------------
    def run_forward(self) -> int:
        self.eng._refuse_listing('PassPlan.run_forward')  # (before torch.cuda is asked for a stream)
        if self.eng.shadows_dirty and not reads_f32_arena(self.precision):  # (an fp32 / bf16x3 plan reads the master arena itself)
            self.eng.refresh_shadows()
        self.gen += 1
        self.fwd.run(torch.cuda.current_stream().cuda_stream)
        return self.gen

    def run_backward(self, gen: Optional[int] = None):
        """`gen` = the value run_forward returned for the forward being differentiated.  The activations live in
        this plan's buffers, not in the autograd graph: a later forward of the same shape overwrites them, and a
        backward of the EARLIER forward would silently differentiate the wrong activations -- so it raises."""
        if gen is not None and gen != self.gen:
            raise RuntimeError(
                'maskdit_amd: backward of a forward whose saved activations were overwritten by a later forward of the '
                f'same shape (forward #{gen}, buffers now hold #{self.gen}).  Call backward() before the next forward '
                '(gradient accumulation: one forward/backward per micro-batch), or evaluate under torch.no_grad().')
        self.eng._refuse_listing('PassPlan.run_backward')
        self.bwd.run(torch.cuda.current_stream().cuda_stream)
