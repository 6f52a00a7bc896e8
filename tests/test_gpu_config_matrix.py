"""The env_config matrix (tests/config_matrix.py) through the HIP library on an MI355X: oracle parity of every row at one wave per SIMD, the
combination rows and the factory defaults in the 256-register builds too (4096 + 256 envs), binding, reset and the plumbing (unroll ring, multi-step
launches, in-kernel re-seeding, odd batch sizes) at observation widths 153 and 117, the second reference golden, and the public factories at their
own defaults.  tests/test_config_matrix_emul.py runs the same checks on the host build.  Run with `pytest -m gpu`."""
import os

import numpy as np
import pytest

import config_matrix as cm
import config_matrix_common as cmc
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

BIG = 4096 + 256          # above one wave per SIMD: the OCC 2 builds (test_gpu_spec_matrix.py's size)


def _cases(rows_of):
    return [pytest.param(engine, name, id='%s-%s' % (engine, name)) for engine in cm.ENGINES for name in rows_of(engine)]


@pytest.mark.parametrize('engine,name', _cases(lambda e: cm.rows_of(e, cm.MOVES_STATE)))
def test_parity_one_wave(engine, name, golden, orc):
    cmc.check_parity(engine, name, None, golden=golden, orc=orc)


@pytest.mark.parametrize('engine,name', _cases(lambda e: [n for n in cm.BIG_ROWS if e in cm.ROWS[n]['engines']]))
def test_parity_256_registers(engine, name, golden, orc, monkeypatch):
    monkeypatch.setenv('LL_SHARE_SIMDS', '1')          # the 256-register builds at every size (SEPMC runs its one-wave build at every size by default)
    cmc.check_parity(engine, name, None, golden=golden, orc=orc, total=BIG // 2 if engine == 'sepmc' else BIG)


@pytest.mark.parametrize('engine', cm.ENGINES)
def test_binding(engine):
    cmc.check_binding(engine, None)


@pytest.mark.parametrize('engine,name', [(e, n) for e in cm.PMC for n in cm.rows_of(e, cm.SAME_STATE) if cm.ROWS[n]['output'] == 'reward'])
def test_reward_rows_against_the_oracle(engine, name, orc):
    cmc.check_reward(engine, name, None, orc)


@pytest.mark.parametrize('name', cm.rows_of('pmc'))
def test_reset(name, golden, orc):
    cmc.check_reset(name, None, golden, orc)


def _device_ring_access():
    import torch
    from lifelike_agility_and_play_amd import gather
    assert torch.cuda.is_available()

    def read_ring(addr, shape):
        return gather.device_tensor(addr, shape).cpu().numpy()

    def write_dev(addr, arr):
        gather.device_tensor(addr, arr.shape).copy_(torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32)))
        torch.cuda.synchronize()
    return read_ring, write_dev


@pytest.mark.parametrize('name', cm.COMBINATION_ROWS)
def test_plumbing(name):
    read_ring, write_dev = _device_ring_access()
    cmc.check_plumbing(name, None, read_ring, write_dev)


@pytest.mark.parametrize('engine,name', [(e, n) for e in cm.ARENA for n in cm.COMBINATION_ROWS])
def test_arena_multi_step_launch(engine, name):
    cmc.check_arena_plumbing(engine, name, None)


@pytest.mark.parametrize('engine', cm.ENGINES)
def test_bad_values_are_refused_at_create_time(engine):
    cmc.check_bad_values(engine, None)


def test_second_reference_golden(model_blob):
    """the HIP library at the factory defaults with a permuted subset prop_type, against the reference's own outputs (tests/golden/pmc_golden_cfg2.npz)"""
    import parity_common as pc
    from lifelike_agility_and_play_amd import mocap
    g = np.load(os.path.join(GOLDEN_DIR, 'pmc_golden_cfg2.npz'), allow_pickle=False)
    cfg = cmc.golden_cfg2_config(g)
    table = mocap.load_mocap('', 1.0 / cfg['control_freq'])
    pc.check_reset_against_goldens(g, model_blob, table, None, cfg=cfg)
    pc.check_scripted_episodes_against_goldens(g, model_blob, table, None, cfg=cfg, min_done=2)


def test_factories_at_their_defaults(orc):
    cmc.check_tracking_factory_defaults(None, orc)
    cmc.check_chase_tag_factory_defaults(None)
