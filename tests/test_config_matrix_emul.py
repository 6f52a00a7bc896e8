"""The env_config matrix (tests/config_matrix.py) on the CPU, through the host build of the kernel source (tests/emul): every field the step
kernels read at run time is held to the oracle away from the training scripts' point, binds where it is meant to act, resets as the oracle does,
and runs through the ring, multi-step launches and in-kernel re-seeding at other observation widths.  tests/test_gpu_config_matrix.py runs the
same matrix through the HIP library."""
import os
import subprocess

import numpy as np
import pytest

import config_matrix as cm
import config_matrix_common as cmc

EMUL_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emul')


@pytest.fixture(scope='module')
def emul_lib():
    subprocess.check_call(['make', '-C', EMUL_DIR, '-s', '-j2'])
    return os.path.join(EMUL_DIR, '_build', 'libllenv_emul.so')


def test_table_is_well_formed():
    for name, row in cm.ROWS.items():
        assert row['kind'] in (cm.MOVES_STATE, cm.SAME_STATE) and set(row['engines']) <= set(cm.ENGINES) and row['engines'], name
        assert set(row.get('cfg_by_engine', {})) <= set(row['engines']), name
        assert (row['kind'] == cm.SAME_STATE) == ('output' in row), name
    assert all(cm.ROWS[n]['engines'] == cm.ENGINES and len(cm.ROWS[n]['cfg']) >= 2 for n in cm.COMBINATION_ROWS)
    # the substep counts and observation widths the rows are there for
    assert [cm.n_sub_of(cm.ROWS[n]['cfg']) for n in ('control_freq_25', 'control_freq_100', 'control_freq_30', 'sim_freq_1000')] == [20, 5, 16, 20]
    assert [3 * cm.prop_dim_of(cm.ROWS[n]['cfg']['prop_type']) + 108 for n in ('prop_e_g', 'prop_e_g_joint_pos', 'prop_vel_only', 'prop_permuted', 'prop_subset_of_four')] == [117, 153, 153, 207, 198]
    assert cm.gather_columns(cm.DEFAULT_PROP, 108) == list(range(207))
    for r in cm.ROWS.values():
        for w in (r['cfg'].get('reward_weights'),):
            assert w is None or set(w) == {'joint_pos', 'joint_vel', 'end_effector', 'root_pose', 'root_vel'}
    assert abs(sum(cm.ROWS['reward_not_unit_sum']['cfg']['reward_weights'].values()) - 1.0) > 0.5
    assert 0.0 in cm.ROWS['reward_one_zero']['cfg']['reward_weights'].values()


def _parity_cases():
    return [pytest.param(engine, name, id='%s-%s' % (engine, name)) for engine in cm.ENGINES for name in cm.rows_of(engine, cm.MOVES_STATE)]


@pytest.mark.parametrize('engine,name', _parity_cases())
def test_parity(engine, name, golden, orc, emul_lib):
    st = cmc.check_parity(engine, name, emul_lib, golden=golden, orc=orc)
    if engine == 'pmc':                   # the host build needs no ill-conditioning allowance at any row: the seeds are chosen so
        assert len(st['ill']) == 0 and st['on_tie'] == 0, (st['ill'], st['on_tie'])


@pytest.mark.parametrize('engine', cm.ENGINES)
def test_binding(engine, emul_lib):
    cmc.check_binding(engine, emul_lib)


@pytest.mark.parametrize('engine,name', [(e, n) for e in cm.PMC for n in cm.rows_of(e, cm.SAME_STATE) if cm.ROWS[n]['output'] == 'reward'])
def test_reward_rows_against_the_oracle(engine, name, orc, emul_lib):
    cmc.check_reward(engine, name, emul_lib, orc)


@pytest.mark.parametrize('name', cm.rows_of('pmc'))
def test_reset(name, golden, orc, emul_lib):
    cmc.check_reset(name, emul_lib, golden, orc)


@pytest.mark.parametrize('name', cm.COMBINATION_ROWS)
def test_plumbing(name, emul_lib):
    read_ring, write_dev = cmc.host_ring_access()
    cmc.check_plumbing(name, emul_lib, read_ring, write_dev)


@pytest.mark.parametrize('engine,name', [(e, n) for e in cm.ARENA for n in cm.COMBINATION_ROWS])
def test_arena_multi_step_launch(engine, name, emul_lib):
    cmc.check_arena_plumbing(engine, name, emul_lib)


@pytest.mark.parametrize('engine', cm.ENGINES)
def test_bad_values_are_refused_at_create_time(engine, emul_lib):
    assert cmc.check_bad_values(engine, emul_lib) == sum(1 for b in cm.BAD_VALUES if engine in b['engines']) >= 5


def test_second_reference_golden(model_blob, emul_lib):
    """the host build at the factory defaults with a permuted subset prop_type, against the reference's own outputs (tests/golden/pmc_golden_cfg2.npz)"""
    import parity_common as pc
    from conftest import GOLDEN_DIR
    from lifelike_agility_and_play_amd import mocap
    g = np.load(os.path.join(GOLDEN_DIR, 'pmc_golden_cfg2.npz'), allow_pickle=False)
    cfg = cmc.golden_cfg2_config(g)
    table = mocap.load_mocap('', 1.0 / cfg['control_freq'])
    pc.check_reset_against_goldens(g, model_blob, table, emul_lib, cfg=cfg)
    pc.check_scripted_episodes_against_goldens(g, model_blob, table, emul_lib, cfg=cfg, min_done=2)


def test_factories_at_their_defaults(orc, emul_lib):
    print('tracking factory: worst state error / bar', cmc.check_tracking_factory_defaults(emul_lib, orc))
    print('chase-tag factory:', cmc.check_chase_tag_factory_defaults(emul_lib))
