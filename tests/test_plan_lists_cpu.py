"""The launch lists of PassPlan, pinned: tests/golden/plan_lists.json.gz holds, for a set of small plans, every launch with
every argument (addresses as [buffer, byte offset]), the marks and the buffers, as tools/plan_dump.py lists them from plans
built over host memory (Engine.host_listing).  The fixture was recorded from the three separate builders that preceded the
shared fp32 walker, so a plan that still equals it launches exactly what those builders launched.

A pull request that changes a launch list ON PURPOSE re-records the fixture with `python tools/plan_dump.py` and says so;
any other difference is a regression of the builders."""
import gzip
import importlib.util
import json
import os

import pytest

from maskdit_amd import _lib, engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('plan_dump', os.path.join(ROOT, 'tools', 'plan_dump.py'))
PD = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(PD)


@pytest.fixture(scope='module')
def recorded(golden_dir):
    with gzip.open(os.path.join(golden_dir, 'plan_lists.json.gz'), 'rt') as fh:
        return json.load(fh)


def test_fuse_flags_are_at_their_defaults():
    flags = {k: getattr(E, k) for k in ('FUSE_LN_GATE', 'FUSE_QKV_COLSUM', 'FUSE_COLSUM', 'FUSE_RES_LN', 'FUSE_RES_LN_EVAL')}
    assert flags == dict(FUSE_LN_GATE=True, FUSE_QKV_COLSUM=True, FUSE_COLSUM=True, FUSE_RES_LN=True, FUSE_RES_LN_EVAL=False), \
        f'the fixture is recorded with the MDT_FUSE_* switches at their defaults, this process runs with {flags}: unset them'


def test_the_fixture_holds_the_plan_set(recorded):
    assert sorted(recorded) == sorted(PD.plan_id(*cfg) for cfg in PD.PLAN_SET)


@pytest.mark.parametrize('cfg', PD.PLAN_SET, ids=lambda cfg: PD.plan_id(*cfg))
def test_plan_equals_the_recorded_list(recorded, cfg):
    eng, pl = PD.build_plan(*cfg)  # (eng: a plan does not keep its engine alive)
    got = json.loads(json.dumps(PD.plan_dump(pl)))  # (tuples -> lists, as the fixture went through JSON)
    want = recorded[PD.plan_id(*cfg)]
    for side in ('fwd', 'bwd'):
        for k, (a, b) in enumerate(zip(got[side], want[side])):
            assert a == b, f'{side} launch {k} differs:\n  built    {a}\n  recorded {b}'
        assert len(got[side]) == len(want[side]), f'{side}: {len(got[side])} launches built, {len(want[side])} recorded'
    assert got['marks'] == want['marks']
    assert got['buffers'] == want['buffers']
    assert got == want


def test_nothing_built_on_host_memory_can_launch():
    sp = E.make_spec('DiT-S/2', 16, 4, 1000)
    with pytest.raises(_lib.MaskDiTLibError):
        E.Engine(sp, 'cpu')
    eng = E.Engine.host_listing(sp)
    with pytest.raises(_lib.MaskDiTLibError):
        eng.plan(2, False, False)
    with pytest.raises(_lib.MaskDiTLibError):
        eng.refresh_shadows()
    for prec, train in (('bf16', True), ('fp32', True), ('bf16x3', False)):
        pl = E.PassPlan(eng, 2, False, train, None, prec)
        assert pl.fwd.calls and pl.fwd.listing and pl.bwd.listing
        for run in (lambda: pl.fwd.run(0), lambda: pl.bwd.run(0), pl.run_forward, pl.run_backward):
            with pytest.raises(_lib.MaskDiTLibError):
                run()
        assert pl.gen == 0


@pytest.mark.parametrize('model,R,B', [('DiT-S/2', 16, 2), ('DiT-S/2', 32, 1), ('DiT-S/4', 32, 2), ('DiT-B/8', 64, 1), ('DiT-S/2', 16, 5)])
def test_f32_train_memory_model_is_what_the_builder_allocates(model, R, B):
    """PassPlan.f32_train_floats is counted by hand; Engine.plan refuses a batch by it.  It may exceed what the builder
    allocates by a rounding (workspaces of at least 4 floats), never fall short of it, and never by more than 0.1 %."""
    sp = E.make_spec(model, R, 4, 1000)
    eng = E.Engine.host_listing(sp)
    pl = E.PassPlan(eng, B, False, True, None, 'fp32')
    excess = 4 * sum(E.PassPlan.f32_train_floats(sp, B).values()) - pl.nbytes
    print(f'{model} R{R} B{B}: plan {pl.nbytes} bytes, model - plan = {excess} ({excess / pl.nbytes:.2e})')
    assert 0 <= excess <= pl.nbytes / 1000
    assert E.PassPlan.estimate_bytes_f32_train(sp, B) >= pl.nbytes
