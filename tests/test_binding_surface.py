"""The surface of the ctypes bindings: the public names of the three engine classes and the entry points every binding module declares, as recorded
before the classes were given shared bases; and the one rule of handle lifetime they now share (capi.NativeHandle)."""
import os
import subprocess

import pytest

from lifelike_agility_and_play_amd import capi, epmc_capi, pmc_policy_hip, sepmc_capi, xfer
from lifelike_agility_and_play_amd.policies import hl_league, hl_policy_hip, hl_unroll
from sepmc_parity_common import env_config as sepmc_env_config
from test_epmc_oracle_golden import env_config as epmc_env_config

EMUL_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emul')
EMUL_LIB = os.path.join(EMUL_DIR, '_build', 'libllenv_emul.so')

PUBLIC = {
    'Engine': '''
    close counters device_ptrs enable_kernel_timing enable_unrolls episode_histogram episode_info feet fill_random_actions finish_unroll get_spec
    kernel_time_ms kernel_time_stats obs pg_mark_current pg_ptrs probe_pd_torque ref_state reset reward_done sampling_table set_sampling_table
    set_spec set_state set_stream state step step_host step_random step_random_n step_scripted sync table_sync terminal_obs unroll_position'''.split(),
    'EpmcEngine': '''
    close counters device_ptrs enable_kernel_timing episode fill_random_actions get_spec info kernel_time_ms kernel_time_stats obs push_trace rays
    reset reward_done script_reset_rays set_spec set_state set_step_draws state statics step step_host step_random_n step_scripted sync'''.split(),
    'SepmcEngine': '''
    boxes close counters device_ptrs enable_kernel_timing episode fill_random_actions get_spec info kernel_time_ms kernel_time_stats obs push_trace
    rays reset reward_done script_reset set_spec set_state set_step_draws state step step_host step_random_n step_scripted sync vis'''.split(),
}
SIG_KEYS = {
    'capi': '''
    ll_abi_version ll_create ll_destroy ll_device_ptrs ll_enable_kernel_timing ll_enable_unrolls ll_fill_random_actions ll_finish_unroll
    ll_get_counters ll_get_episode_histogram ll_get_episode_info ll_get_feet ll_get_obs ll_get_ref_state ll_get_reward_done ll_get_sampling_table
    ll_get_spec_param ll_get_state ll_get_table_sync ll_get_terminal_obs ll_kernel_time_ms ll_kernel_time_stats ll_last_error ll_load_mocap
    ll_load_mocap_f64 ll_load_obstacles ll_model_blob_len ll_pg_mark_current ll_pg_ptrs ll_probe_pd_torque ll_reset ll_set_actions
    ll_set_sampling_table ll_set_spec_param ll_set_state ll_set_stream ll_step ll_step_random ll_step_random_n ll_step_scripted ll_sync
    ll_unroll_position'''.split(),
    'epmc_capi': '''
    ll_epmc_create ll_epmc_destroy ll_epmc_device_ptrs ll_epmc_enable_kernel_timing ll_epmc_fill_random_actions ll_epmc_get_counters
    ll_epmc_get_episode ll_epmc_get_info ll_epmc_get_obs ll_epmc_get_push_trace ll_epmc_get_rays ll_epmc_get_reward_done ll_epmc_get_spec_param
    ll_epmc_get_state ll_epmc_get_statics ll_epmc_kernel_time_ms ll_epmc_kernel_time_stats ll_epmc_obs_dim ll_epmc_reset ll_epmc_script_reset_rays
    ll_epmc_set_actions ll_epmc_set_spec_param ll_epmc_set_state ll_epmc_set_step_draws ll_epmc_step ll_epmc_step_random_n ll_epmc_step_scripted
    ll_epmc_sync'''.split(),
    'sepmc_capi': '''
    ll_sepmc_create ll_sepmc_destroy ll_sepmc_device_ptrs ll_sepmc_enable_kernel_timing ll_sepmc_fill_random_actions ll_sepmc_get_boxes
    ll_sepmc_get_counters ll_sepmc_get_episode ll_sepmc_get_info ll_sepmc_get_obs ll_sepmc_get_push_trace ll_sepmc_get_rays ll_sepmc_get_reward_done
    ll_sepmc_get_spec_param ll_sepmc_get_state ll_sepmc_get_vis ll_sepmc_kernel_time_ms ll_sepmc_kernel_time_stats ll_sepmc_obs_dim ll_sepmc_reset
    ll_sepmc_script_reset ll_sepmc_set_actions ll_sepmc_set_spec_param ll_sepmc_set_state ll_sepmc_set_step_draws ll_sepmc_step ll_sepmc_step_random_n
    ll_sepmc_step_scripted ll_sepmc_sync'''.split(),
    'pmc_policy_hip': '''
    ll_policy_act ll_policy_act_pg ll_policy_create ll_policy_destroy ll_policy_enable_timing ll_policy_time_ms'''.split(),
    'xfer': '''
    ll_xfer_can_wait_value ll_xfer_close_mem ll_xfer_event_create ll_xfer_event_destroy ll_xfer_event_open ll_xfer_event_record
    ll_xfer_event_synchronize ll_xfer_export_mem ll_xfer_open_mem ll_xfer_pull ll_xfer_set_device ll_xfer_signal_create ll_xfer_signal_destroy
    ll_xfer_stream_create ll_xfer_stream_destroy ll_xfer_stream_synchronize ll_xfer_stream_wait ll_xfer_stream_wait_value ll_xfer_stream_write_value'''.split(),
    'hl_policy_hip': '''
    ll_hl_policy_act ll_hl_policy_act_pg ll_hl_policy_attach_value ll_hl_policy_create ll_hl_policy_destroy ll_hl_policy_enable_timing
    ll_hl_policy_get_state ll_hl_policy_get_value_state ll_hl_policy_reset_state ll_hl_policy_set_state ll_hl_policy_set_value_state
    ll_hl_policy_set_weights ll_hl_policy_state_dim ll_hl_policy_time_ms'''.split(),
    'hl_unroll': '''
    ll_hl_unroll_create_epmc ll_hl_unroll_create_sepmc ll_hl_unroll_destroy ll_hl_unroll_finish ll_hl_unroll_layout ll_hl_unroll_position
    ll_hl_unroll_steps'''.split(),
    'hl_league': '''
    ll_hl_league_create ll_hl_league_destroy ll_hl_league_finish ll_hl_league_get_assignment ll_hl_league_get_outcomes ll_hl_league_get_state
    ll_hl_league_layout ll_hl_league_plan_only ll_hl_league_position ll_hl_league_set_probs ll_hl_league_set_weights ll_hl_league_steps'''.split(),
}


@pytest.fixture(scope='module')
def emul_lib():
    subprocess.check_call(['make', '-C', EMUL_DIR, '-s', '-j2'])
    return EMUL_LIB


@pytest.mark.parametrize('cls', [capi.Engine, epmc_capi.EpmcEngine, sepmc_capi.SepmcEngine])
def test_public_names_of_the_engine_classes(cls):
    assert [n for n in dir(cls) if not n.startswith('_')] == PUBLIC[cls.__name__]


@pytest.mark.parametrize('mod', [capi, epmc_capi, sepmc_capi, pmc_policy_hip, xfer, hl_policy_hip, hl_unroll, hl_league])
def test_declared_entry_points(mod):
    name = mod.__name__.rsplit('.', 1)[1]
    assert sorted(mod._SIGS) == SIG_KEYS[name] == mod.EXPORTED_SYMBOLS


def _ctor_args(cls, model_blob, mocap_table):
    if cls is capi.Engine:
        return (capi.make_config(2, prop_type=['joint_pos']), model_blob, mocap_table)
    if cls is epmc_capi.EpmcEngine:
        return (epmc_capi.make_epmc_config(2, epmc_env_config(1)), model_blob)
    return (sepmc_capi.make_sepmc_config(1, sepmc_env_config((0, 0, 0))), model_blob)


@pytest.mark.parametrize('cls', [capi.Engine, epmc_capi.EpmcEngine, sepmc_capi.SepmcEngine])
def test_close_twice_and_after_a_failed_constructor(cls, emul_lib, model_blob, mocap_table):
    E = cls(*_ctor_args(cls, model_blob, mocap_table), lib_path=emul_lib)
    assert E.h
    E.close()
    assert not E.h                                    # falsy after close(), in every class
    E.close()
    with pytest.raises(capi.LLError) as ei:           # a closed engine answers as a null handle does; nothing is dereferenced
        E.sync()
    assert ei.value.code == capi.LL_EINVAL
    # a constructor that raised in the native create call (a model blob one number short), and one that raised before it had a library
    for blob, lib_path, error in ((model_blob[:-1], emul_lib, capi.LLError), (model_blob, os.path.join(EMUL_DIR, 'no_such_library.so'), ImportError)):
        H = cls.__new__(cls)
        with pytest.raises(error):
            H.__init__(*_ctor_args(cls, blob, mocap_table), lib_path=lib_path)
        assert not getattr(H, 'h', None)
        H.close()
        H.close()


@pytest.mark.parametrize('cls', [capi.Engine, epmc_capi.EpmcEngine, sepmc_capi.SepmcEngine])
def test_step_takes_an_address_or_none(cls, emul_lib, model_blob, mocap_table):
    """step(ptr): an int device address or None, in every class -- the PMC binding used to wrap the address, the other two passed it on as it
    came (the host build's "device" addresses are host addresses)"""
    E = cls(*_ctor_args(cls, model_blob, mocap_table), lib_path=emul_lib)
    try:
        E.reset()
        a = E.device_ptrs().actions
        assert isinstance(a, int)
        E.step(None); E.step(a); E.step()
        steps = E.counters()
        assert steps.pop('arena_steps' if cls is sepmc_capi.SepmcEngine else 'env_steps') == 3 * (1 if cls is sepmc_capi.SepmcEngine else 2)
        assert sorted(steps) == ['episodes', 'nonfinite']
    finally:
        E.close()
