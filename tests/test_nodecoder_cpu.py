"""CPU checks of the decoder-less models (use_decoder=False, models/maskdit.py:302-331, 529-553): module surface and
parameter order against the reference's own, arena layout and slabs, the launch lists of every plan kind (built over host
memory, Engine.host_listing), the fp32-training refusal -- and that a model WITH a decoder is laid out and planned exactly
as before."""
import gzip
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from maskdit_amd import engine as E
from oracle import maskdit_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('plan_dump', os.path.join(ROOT, 'tools', 'plan_dump.py'))
PD = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(PD)

MODELS = [('DiT-S/2', 16), ('DiT-S/4', 32), ('DiT-B/2', 16), ('DiT-XL/2', 32), ('DiT-H/8', 64)]


def _net(model='DiT-S/2', R=16, **kw):
    import maskdit_amd as M
    return M.Precond_models['edm'](img_resolution=R, img_channels=4, num_classes=1000, model_type=model, use_decoder=False,
                                   mae_loss_coef=0.1, pad_cls_token=False, **kw)


@pytest.mark.parametrize('model,R', MODELS)
def test_state_dict_is_the_references(model, R):
    net = _net(model, R)
    cfg = O.make_cfg(model, img_resolution=R, use_decoder=False)
    got = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert got == O.param_shapes(cfg)
    assert not any(k.startswith(('model.decoder_', 'model.mask_token')) for k in got)
    if model.startswith('DiT-S'):
        assert len(got) == 132  # 12 blocks x 10 + final layer 4 + embedders 7 + pos_embed
    m = net.model
    assert m.decoder_pos_embed is None and m.decoder_blocks is None and m.decoder_layer is None and m.mask_token is None
    assert m.use_decoder is False and not m.pos_embed.requires_grad
    assert m.final_layer.linear.weight.shape == (m.patch_size ** 2 * 4, net.spec.D)
    # a reference-shaped checkpoint loads strictly and reads back unchanged
    P = O.init_params(cfg, seed=3, dezero=True)
    net.load_state_dict(P, strict=True)
    back = net.state_dict()
    assert all(torch.equal(back[k], P[k]) for k in P)
    assert torch.allclose(m.pos_embed, O.init_params(cfg)['model.pos_embed'])


@pytest.mark.parametrize('model', ['DiT-S/2', 'DiT-XL/2'])
def test_parameter_order_is_the_references(golden_dir, model):
    with open(os.path.join(golden_dir, 'param_order_nodecoder.json')) as f:
        want = json.load(f)[model]
    net = _net(model, 32)
    got = [[n, list(p.shape), bool(p.requires_grad)] for n, p in net.named_parameters()]
    assert got == want


@pytest.mark.parametrize('model,R', MODELS)
def test_layout_has_no_decoder_and_tiles_the_arena(model, R):
    sp = E.make_spec(model, R, 4, 1000, use_decoder=False)
    assert not sp.use_decoder and sp.ddepth == 0 and sp.Dd == sp.D
    assert sp.n_mod == sp.depth * 6 * sp.D + 2 * sp.D and sp.mod_off('fin') == sp.depth * 6 * sp.D
    tab = dict(E.param_table(sp))
    ref = {k: v for k, v in O.param_shapes(O.make_cfg(model, img_resolution=R, use_decoder=False)).items()
           if k not in O.NON_TRAINABLE}
    assert tab == ref
    lay = E.Layout(sp)
    assert not any(name.startswith('dec') for name in lay.slabs)
    assert lay.ada_b - lay.ada_w == sp.n_mod * sp.D
    assert lay.ada_groups[0] == ('ada_w_dec', sp.depth * 6 * sp.D, sp.n_mod)  # the final layer's rows only
    cov = np.zeros(lay.n, dtype=np.int32)
    for lo, hi in lay.slabs.values():
        cov[lo:hi] += 1
    assert (cov == 1).all()
    assert not any('decoder' in k for k in lay.t_off)
    # ZeRO-1 / DDP ownership works from the slabs alone
    from maskdit_amd.zero import owned_pieces
    for world in (1, 3, 8):
        cover = np.zeros(lay.n, dtype=np.int32)
        for r in range(world):
            for a, e in owned_pieces(lay.slabs, world, r):
                cover[a:e] += 1
        assert (cover == 1).all()
    assert E.PassPlan.estimate_bytes(sp, 4, True, True, 23) < E.PassPlan.estimate_bytes(E.make_spec(model, R, 4, 1000), 4, True, True, 23)


PLAN_KINDS = [('bf16', True, True, 23), ('bf16', False, True, None), ('bf16', False, False, None), ('bf16', True, False, 23),
              ('fp32', False, False, None), ('bf16x3', False, False, None)]


@pytest.mark.parametrize('model,R', [('DiT-S/2', 16), ('DiT-S/4', 32), ('DiT-B/2', 16)])
@pytest.mark.parametrize('prec,masked,train,L', PLAN_KINDS)
def test_plans_go_from_the_encoder_to_the_keep_kernels(model, R, prec, masked, train, L):
    sp = E.make_spec(model, R, 4, 1000, use_decoder=False)
    eng = E.Engine.host_listing(sp)
    pl = E.PassPlan(eng, 2, masked, train, L, prec)
    fwd, bwd = [c[2] for c in pl.fwd.calls], [c[2] for c in pl.bwd.calls]
    assert fwd.count('mdt_final_keep_fwd') == 1 and fwd[-1] == 'mdt_final_keep_fwd'
    assert not any(n.startswith('mdt_unmask') or n in ('mdt_final_fwd', 'mdt_final_bwd') for n in fwd + bwd)
    dump = PD.plan_dump(pl)
    keep = dump['fwd'][-1]
    T, D = sp.T, sp.D
    top = f'x_e{sp.depth}' if train else f'x_epp{sp.depth % 2}'
    # x = the top encoder block's own fp32 output; modulation = the final layer's 2 D rows; ids / L / pitch / width
    assert keep[1] == [top, 0] and keep[2] == ['mod', 4 * sp.depth * 6 * D] and keep[3] == ['mod', 4 * (sp.depth * 6 * D + D)]
    assert keep[4] == sp.n_mod and keep[7] == (['ids32', 0] if masked else None) and keep[8] == 2 * T and keep[9] == ['F', 0]
    assert keep[11:] == [2, T, L if masked else T, 64 if masked else T, D, 4, sp.patch]
    if not train:
        assert not bwd
        return
    assert bwd.count('mdt_final_keep_bwd') == 1 and [n for n in bwd if n != 'callback'][0] == 'mdt_final_keep_bwd'
    kb = next(c for c in dump['bwd'] if c[0] == 'mdt_final_keep_bwd')
    assert kb[2] == [top, 0] and kb[10] == ['dx_e', 0] and kb[16:] == keep[11:]
    # the run-time kept count reaches both launches through the plan's one mutable int
    if masked:
        pl.set_valid(40)
        assert PD.plan_dump(pl)['fwd'][-1][13] == 40 and next(c for c in PD.plan_dump(pl)['bwd'] if c[0] == 'mdt_final_keep_bwd')[18] == 40
    # every slab of the layout is announced exactly once, none of a decoder
    slabs = [c[1] for c in dump['bwd'] if c[0] == 'slab']
    assert sorted(slabs) == sorted(eng.lay.slabs)


def test_fp32_training_is_refused_and_names_the_switch():
    import maskdit_amd as M
    net = _net()
    with pytest.raises(NotImplementedError, match='use_decoder=False'):
        net.set_train_precision('fp32')
    assert net.train_precision == 'bf16'
    net.train_precision = 'fp32'  # (set behind the setter's back: the plan-precision choice refuses it as well)
    for masked in (False, True):
        with pytest.raises(NotImplementedError, match='use_decoder'):
            net._train_plan_precision(masked)
    eng = E.Engine.host_listing(net.spec)
    with pytest.raises(NotImplementedError, match='use_decoder'):
        E.PassPlan(eng, 2, False, True, None, 'fp32')
    # the refusals of the flags that stay out of scope are unchanged
    for kw in (dict(pad_cls_token=True), dict(ext_feature_dim=8), dict(use_encoder_feat=True), dict(learn_sigma=True)):
        with pytest.raises(NotImplementedError, match='shipped flag set'):
            M.Precond_models['edm'](img_resolution=16, img_channels=4, num_classes=1000, model_type='DiT-S/2', use_decoder=False, **kw)
    with pytest.raises(NotImplementedError, match='num_classes=0'):
        M.Precond_models['edm'](img_resolution=16, img_channels=4, num_classes=0, model_type='DiT-S/2', use_decoder=False)
    # a decoder model keeps fp32 training of its unmasked stage
    dec = M.Precond_models['edm'](img_resolution=16, img_channels=4, num_classes=1000, model_type='DiT-S/2', use_decoder=True)
    assert dec.set_train_precision('fp32')._train_plan_precision(False) == 'fp32'


def test_a_decoder_model_is_laid_out_and_planned_as_before(golden_dir):
    """Offsets of every tensor and slab of a decoder spec against the addresses the recorded launch lists hold
    (tests/golden/plan_lists.json.gz, read through the loader of tests/test_plan_lists_cpu.py), and the launch names of
    two plans against the recorded ones (test_plan_lists_cpu compares them argument by argument)."""
    with gzip.open(os.path.join(golden_dir, 'plan_lists.json.gz'), 'rt') as fh:
        recorded = json.load(fh)
    sp = E.make_spec('DiT-S/2', 16, 4, 1000)
    assert sp.use_decoder and (sp.Dd, sp.ddepth, sp.dheads) == (512, 8, 16)
    assert sp.n_mod == 12 * 6 * 384 + 8 * 6 * 512 + 2 * 384 + 2 * 512
    lay = E.Layout(sp)
    assert [n for n in lay.slabs if n.startswith('dec')] == [f'dec{i}' for i in range(8)]
    assert lay.slabs['misc'][0] == lay.off['model.decoder_layer.linear.weight']
    assert 'model.mask_token' in lay.off and 'model.decoder_layer.linear.weight' in lay.t_off
    for cfg in (('DiT-S/2', 16, 2, 'bf16', True, True, 20), ('DiT-S/2', 16, 2, 'fp32', False, False, None)):
        want = recorded[PD.plan_id(*cfg)]
        eng, pl = PD.build_plan(*cfg)
        got = json.loads(json.dumps(PD.plan_dump(pl)))
        assert got == want
        # the recorded byte offsets into the parameter / gradient arenas are the layout's
        fin = next(c for c in want['fwd'] if c[0] == 'mdt_final_fwd')
        assert fin[5] == ['P', 4 * lay.off['model.final_layer.linear.weight']] and fin[2] == ['mod', 4 * sp.mod_off('fin')]
        slabs = {c[1]: (c[2], c[3]) for c in want['bwd'] if c[0] == 'slab'}
        assert all(lay.slabs[k] == v for k, v in slabs.items()) and (not slabs or sorted(slabs) == sorted(lay.slabs))


def test_config_and_drivers_name_the_switch():
    from maskdit_amd import schedule  # noqa: F401  (the package imports without a GPU)
    import yaml
    with open(os.path.join(ROOT, 'configs', 'xl2-256-nodecoder-synthetic.yaml')) as f:
        cfg = yaml.safe_load(f)
    with open(os.path.join(ROOT, 'configs', 'xl2-256-synthetic.yaml')) as f:
        base = yaml.safe_load(f)
    assert cfg['model']['use_decoder'] is False and base['model']['use_decoder'] is True
    diff = {k for k in cfg['model'] if cfg['model'][k] != base['model'].get(k)}
    assert diff == {'use_decoder'}
