"""Which kernel runs a GEMM (host only, no GPU): vitcap_gemm_plan, vitcap_gemm_large_form and vitcap_gemm_tile_plan answer exactly what
tests/golden/gemm_plan.npz records -- the launches vitcap_gemm_ex made over that descriptor lattice before its routing moved into one plan
function (docs/LAB_refactor_gemm_plan.md), and the two older queries' answers of the same day.  A change of a GEMM form shows here as the
descriptors whose launch moved; regenerate with tests/golden/make_golden_gemm_plan.py when the move is meant."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, 'tests', 'golden')


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(REPO, 'vitcap_amd', 'libvitcap_hip.so')):
        g.build()
    from vitcap_amd import _lib
    # the tile heights and persistent grids in the fixture are those of 256 CUs (what the library assumes without a device)
    if torch.cuda.is_available() and torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip('the fixture was recorded for 256 CUs')
    return _lib


@pytest.fixture(scope='module')
def gen():
    spec = importlib.util.spec_from_file_location('make_golden_gemm_plan', os.path.join(GOLDEN, 'make_golden_gemm_plan.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'gemm_plan.npz'))


def _restored(L, env):
    assert L.lib.vitcap_gemm_reserve_cus(0) == 0
    assert os.environ.get('VITCAP_GEMM_4W_DEFER') == env


def test_plan_matches_recorded_launches(L, gen, golden):
    env = os.environ.get('VITCAP_GEMM_4W_DEFER')
    desc = golden['desc']
    assert desc.shape[1] == len(gen.COLS) and golden['plan'].shape == (len(desc), len(gen.PLAN_FIELDS))
    assert (desc == gen.descriptors()).all()                # the generator still spans the lattice of the committed file
    rc, plan = gen.query_plans(L, desc.astype(np.int64))
    _restored(L, env)
    bad = np.flatnonzero((rc != golden['rc']) | (plan != golden['plan']).any(axis=1))
    report = ['%s\n  recorded rc %d %s\n  now      rc %d %s' % (dict(zip(gen.COLS, desc[i].tolist())), golden['rc'][i],
                                                                 dict(zip(gen.PLAN_FIELDS, golden['plan'][i].tolist())), rc[i],
                                                                 dict(zip(gen.PLAN_FIELDS, plan[i].tolist()))) for i in bad[:5]]
    assert len(bad) == 0, '%d of %d descriptors launch another kernel than recorded:\n%s' % (len(bad), len(desc), '\n'.join(report))
    # the lattice reaches every family and every 4-wave variant
    ok = golden['rc'] == 0
    assert set(golden['plan'][ok][:, gen.PLAN_FIELDS.index('family')].tolist()) == set(range(len(L.GemmPlanInfo.FAMILIES)))
    assert set(golden['plan'][ok][:, gen.PLAN_FIELDS.index('variant')].tolist()) == set(range(len(L.GemmPlanInfo.VARIANTS)))


def test_old_queries_match_recorded_answers(L, gen, golden):
    env = os.environ.get('VITCAP_GEMM_4W_DEFER')
    lf, tp = gen.query_large(L)
    _restored(L, env)
    assert (lf == golden['large_form']).all(), np.argwhere(lf != golden['large_form'])[:10]
    assert (tp == golden['tile_plan']).all(), np.argwhere(tp != golden['tile_plan'])[:10]


def test_plan_reports_the_launchers_errors(L):
    """the same code and the same text vitcap_gemm_ex gives: first failed check wins, in the launcher's order"""
    info = L.GemmPlanInfo()
    plan = lambda d, *flags: L.lib.vitcap_gemm_plan(C.byref(d), *(flags + (0,) * (6 - len(flags))), C.byref(info))
    assert L.lib.vitcap_gemm_plan(None, 0, 0, 0, 0, 0, 0, C.byref(info)) == -1 and b'null' in L.lib.vitcap_last_error()
    d = L.GemmDesc(M=8, N=16, K=96, lda=96, ldw=96, ldc=16, tile_hint=7)
    assert plan(d) == -1 and b'multiple of 64' in L.lib.vitcap_last_error()          # before the unknown hint
    d.K = d.lda = d.ldw = 128
    assert plan(d) == -1 and b'unknown tile_hint 7' in L.lib.vitcap_last_error()
    d.tile_hint, d.ldr = 0, 18
    assert plan(d, 1, 1) == -1 and b'residual misaligned' in L.lib.vitcap_last_error()
    assert plan(d, 1, 0) == 0 and L.GemmPlanInfo.FAMILIES[info.family] == 'ring' and (info.wm, info.wn, info.stages) == (1, 1, 4)
    assert (info.grid[0], info.grid[1], info.grid[2], info.block, info.lds_bytes) == (1, 1, 1, 256, 4 * 64 * 128)
    d.abi -= 1
    assert plan(d) == -1 and b'ABI' in L.lib.vitcap_last_error()
