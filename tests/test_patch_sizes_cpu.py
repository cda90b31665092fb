"""Patch sizes 4 and 8 without a GPU: the oracle against the reference's own fixtures (tests/golden/make_golden_patch.py --
the oracle's patch-generic code had only ever run at patch 2), make_spec's domain, the arena layout and the state-dict
shapes, and the C ABI's refusal of a patch vector the token-boundary kernels do not serve."""
import os

import numpy as np
import pytest
import torch

from oracle import maskdit_oracle as O

torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))


@pytest.mark.parametrize('name,model,R', [('s4_train.npz', 'DiT-S/4', 32), ('s8_train.npz', 'DiT-S/8', 64)])
def test_oracle_train_step_matches_reference_at_patch_4_and_8(golden_dir, name, model, R):
    """The checks and bounds tests/test_oracle_golden.py::test_train_step_matches_reference applies to s2_train.npz."""
    from tests.golden.make_golden_idx import sample_idx
    from tests.test_oracle_golden import _check_param_recipe, _inputs, _sums
    g = np.load(os.path.join(golden_dir, name), allow_pickle=False)
    cfg = O.make_cfg(model, img_resolution=R)
    assert (int(g['B']), int(g['R']), g['mask_noise'].shape[1]) == (4, R, 64)
    P = O.init_params(cfg, seed=int(g['seed']), dezero=True)
    names = _check_param_recipe(P, g)
    images, labels, rnd, noise, md = _inputs(g, cfg)
    loss, D, grads = O.loss_and_grads(P, cfg, images, labels, rnd, noise, md, 0.1)
    np.testing.assert_allclose(loss.numpy(), g['loss'], rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(D.numpy(), g['D_yn'], rtol=1e-4, atol=2e-5)
    for i, k in enumerate(names):
        gs = g['grad_sums'][i]
        got = _sums(grads[k])
        assert abs(got[2] - gs[2]) <= 2e-4 * gs[2] + 1e-9, (k, got, gs)
        idx = sample_idx(grads[k].numel())
        np.testing.assert_allclose(grads[k].double().flatten()[idx].numpy(), g['grad_samples'][i], rtol=2e-3,
                                   atol=2e-4 * gs[2] / max(1.0, grads[k].numel() ** 0.5) + 1e-9, err_msg=k)
    for i, k in enumerate(names):
        p, m, v, e = P[k].clone(), torch.zeros_like(P[k]), torch.zeros_like(P[k]), P[k].clone()
        O.adamw_step(p, grads[k], m, v, step=1, lr=1e-4)
        O.ema_update(e, p, 0.9999)
        idx = sample_idx(p.numel())
        np.testing.assert_allclose(p.double().flatten()[idx].numpy(), g['upd_samples'][i], rtol=1e-6, atol=2e-7, err_msg=k)
        np.testing.assert_allclose(e.double().flatten()[idx].numpy(), g['ema_samples'][i], rtol=1e-6, atol=2e-7, err_msg=k)


def test_make_spec_accepts_all_fifteen_models():
    from maskdit_amd.engine import MODEL_CONFIGS, make_spec
    assert len(MODEL_CONFIGS) == 15
    for name, (depth, D, p, heads) in MODEL_CONFIGS.items():
        for side in (8, 16, 32):  # tokens per side: T = 64, 256, 1024
            sp = make_spec(name, side * p, 4, 1000)
            assert (sp.T, sp.pp, sp.patch, sp.D) == (side * side, 4 * p * p, p, D), name
    with pytest.raises(NotImplementedError, match='smallest is 64'):
        make_spec('DiT-S/8', 32, 4, 1000)    # T = 16
    with pytest.raises(NotImplementedError, match='smallest is 32'):
        make_spec('DiT-XL/4', 16, 4, 1000)   # T = 16
    with pytest.raises(NotImplementedError, match='token count 4096'):
        make_spec('DiT-S/4', 256, 4, 1000)
    with pytest.raises(NotImplementedError, match='token count 4096'):
        make_spec('DiT-S/2', 128, 4, 1000)
    with pytest.raises(NotImplementedError, match='patch vector of 48'):
        make_spec('DiT-S/4', 32, 3, 1000)


@pytest.mark.parametrize('model,R', [('DiT-S/4', 32), ('DiT-S/8', 64), ('DiT-XL/4', 64), ('DiT-XL/8', 64)])
def test_arena_layout_and_state_dict_shapes_follow_the_reference(model, R):
    import maskdit_amd as M
    from maskdit_amd.engine import Layout, make_spec, param_table, MODEL_CONFIGS
    p = MODEL_CONFIGS[model][2]
    sp = make_spec(model, R, 4, 1000)
    cfg = O.make_cfg(model, img_resolution=R)
    shapes = O.param_shapes(cfg)
    tab = dict(param_table(sp))
    assert tab == {k: v for k, v in shapes.items() if k not in O.NON_TRAINABLE}
    assert tab['model.x_embedder.proj.weight'] == (sp.D, 4, p, p) and tab['model.final_layer.linear.weight'] == (p * p * 4, 512)
    lay = Layout(sp)
    spans = sorted((lay.off[k], lay.off[k] + int(np.prod(v))) for k, v in tab.items())
    assert all(a % 8 == 0 for a, _ in spans) and all(spans[i][1] <= spans[i + 1][0] for i in range(len(spans) - 1))
    cov = np.zeros(lay.n, dtype=np.int32)
    for lo, hi in lay.slabs.values():
        cov[lo:hi] += 1
    assert (cov == 1).all()
    if model.startswith('DiT-S'):
        net = M.Precond_models['edm'](img_resolution=R, img_channels=4, num_classes=1000, model_type=model, use_decoder=True,
                                      mae_loss_coef=0.1, pad_cls_token=False)
        assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == shapes
        P = O.init_params(cfg, seed=1)
        net.load_state_dict(P, strict=True)
        assert torch.allclose(net.model.pos_embed, P['model.pos_embed']) and net.model.patch_size == p
        assert not net.model.pos_embed.requires_grad and net.model.x_embedder.proj.weight.shape == (sp.D, 4, p, p)


def test_c_abi_refuses_a_patch_vector_of_36():
    """C = 4, p = 3: none of the six token-boundary entries serves C * p * p = 36; each says so before any launch."""
    from maskdit_amd import _lib
    L = _lib.lib()
    a = 16  # a non-null address that is never dereferenced: the refusal precedes the launch
    B, C_, p, R, T, D, Dd = 2, 4, 3, 24, 64, 384, 512
    calls = {
        'mdt_patch_embed_fwd': (a, None, a, a, a, None, 0, a, B, C_, R, p, T, D, None),
        'mdt_patch_embed_bwd': (a, None, a, None, 0, a, a, B, C_, R, p, T, D, None),
        'mdt_final_fwd': (a, a, a, 2 * Dd, a, a, a, a, B, T, Dd, C_, p, None),
        'mdt_final_bwd': (a, a, a, a, a, 2 * Dd, a, a, a, a, a, a, 2 * Dd, B, T, Dd, C_, p, None),
        'mdt_edm_loss_fwd': (a, a, a, a, None, 0.0, a, a, B, C_, R, p, None),
        'mdt_edm_loss_bwd': (a, a, a, a, a, None, 0.0, a, B, C_, R, p, None),
    }
    for name, args in calls.items():
        assert getattr(L, name)(*args) != 0, name
        msg = L.mdt_last_error()
        assert b'<= 16, 64 or 256' in msg and name[4:].encode() in msg, (name, msg)
    # R not a multiple of p, at a served patch vector
    assert L.mdt_patch_embed_fwd(a, None, a, a, a, None, 0, a, B, C_, 30, 4, T, D, None) != 0
    assert b'multiple of p' in L.mdt_last_error()
    assert L.mdt_edm_loss_fwd(a, a, a, a, None, 0.0, a, a, B, C_, 30, 4, None) != 0
    assert b'multiple of p' in L.mdt_last_error()
