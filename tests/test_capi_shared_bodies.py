"""What the C-ABI entry points that the three engines have in common answer to a bad call: the return code and the ll_last_error() text for a null
handle, for each required pointer left null, for a spec id out of range, for a step ahead of the first reset, and the two get_rays refusals of an engine
too large to keep its ray trace.  The expected values are literals, recorded on the host build of the library (tests/emul) before these entry points
were given one body: whoever touches that body keeps every code and every text."""
import ctypes as C
import os
import subprocess

import pytest

from lifelike_agility_and_play_amd import capi, epmc_capi, sepmc_capi
from sepmc_parity_common import env_config as sepmc_env_config
from test_epmc_oracle_golden import env_config as epmc_env_config

EMUL_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emul')
EMUL_LIB = os.path.join(EMUL_DIR, '_build', 'libllenv_emul.so')
PREFIXES = ('ll_', 'll_epmc_', 'll_sepmc_')


@pytest.fixture(scope='module')
def emul_lib():
    subprocess.check_call(['make', '-C', EMUL_DIR, '-s', '-j2'])
    return EMUL_LIB


_keep = []


def _p():
    b = C.create_string_buffer(1 << 16)
    _keep.append(b)
    return C.cast(b, C.c_void_p)


def _ref(t):
    v = t()
    _keep.append(v)
    return C.byref(v)


# suffix -> (arguments after the handle, the positions among them of the pointers the entry point requires)
CALLS = [
    ('reset', lambda: [None, 1, None, None], ()),
    ('step', lambda: [None], ()),
    ('step_random_n', lambda: [0.1, 1], ()),
    ('kernel_time_stats', lambda: [_ref(C.c_double), _ref(C.c_int), _ref(C.c_int64)], (0, 1, 2)),
    ('set_actions', lambda: [_p()], (0,)),
    ('fill_random_actions', lambda: [0.1], ()),
    ('set_step_draws', lambda: [_p(), 1], (0,)),
    ('set_spec_param', lambda: [0, 0.0], ()),
    ('get_spec_param', lambda: [0, _ref(C.c_double)], (1,)),
    ('sync', lambda: [], ()),
    ('get_obs', lambda: [_p()], (0,)),
    ('get_state', lambda: [_p()], (0,)),
    ('set_state', lambda: [_p()], (0,)),
    ('get_rays', lambda: [_p(), _p(), _p(), _p()], ()),
    ('get_push_trace', lambda: [_p(), _ref(C.c_int32)], (0,)),
    ('get_reward_done', lambda: [_p(), _p(), _p()], ()),
    ('get_counters', lambda: [_ref(C.c_uint64), _ref(C.c_uint64), _ref(C.c_uint64)], ()),
    ('device_ptrs', lambda: [_ref(capi.LLDevicePtrs)], (0,)),
    ('enable_kernel_timing', lambda: [1], ()),
    ('kernel_time_ms', lambda: [_ref(C.c_double), _ref(C.c_int)], (0, 1)),
]
N_SPEC = len(capi.SPEC_IDS)


def _engines(lib_path, model_blob, mocap_table):
    """-> {prefix: (a small engine, its configuration)}"""
    pmc, epmc = capi.make_config(2, prop_type=['joint_pos']), epmc_capi.make_epmc_config(2, epmc_env_config(1))
    sepmc = sepmc_capi.make_sepmc_config(1, sepmc_env_config((0, 0, 0)))
    return {'ll_': (capi.Engine(pmc, model_blob, mocap_table, lib_path=lib_path), pmc),
            'll_epmc_': (epmc_capi.EpmcEngine(epmc, model_blob, lib_path=lib_path), epmc),
            'll_sepmc_': (sepmc_capi.SepmcEngine(sepmc, model_blob, lib_path=lib_path), sepmc)}


def observe(prefix, E, cfg, model_blob):
    """-> {case: (return code, ll_last_error() text, or None where the call returned LL_OK)} of one engine's shared entry points"""
    lib, out = E.lib, {}

    def call(case, name, *args):
        rc = getattr(lib, name)(*args)
        out[case] = (rc, lib.ll_last_error().decode() if rc != 0 else None)

    for suffix, mk, required in CALLS:
        name = prefix + suffix
        if not hasattr(lib, name):
            continue                                            # (the PMC engine has no draws, rays or push trace)
        call(suffix + '(null handle)', name, None, *mk())
        for i in required:
            args = mk()
            args[i] = None
            call('%s(null argument %d)' % (suffix, i), name, E.h, *args)
    call('destroy(null handle)', prefix + 'destroy', None)
    if prefix != 'll_':
        out['obs_dim(null handle)'] = (getattr(lib, prefix + 'obs_dim')(None), None)      # an int, not a status: it leaves no error text
        call('step(before reset)', prefix + 'step', E.h, None)
        call('step_random_n(before reset)', prefix + 'step_random_n', E.h, 0.1, 1)
        call('set_step_draws(negative count)', prefix + 'set_step_draws', E.h, _p(), -1)
    for i in (-1, N_SPEC):
        call('get_spec_param(id %d)' % i, prefix + 'get_spec_param', E.h, i, _ref(C.c_double))
        call('set_spec_param(id %d)' % i, prefix + 'set_spec_param', E.h, i, 0.0)
    # create: the configuration, the model blob, (the start state) and the place for the handle are required
    blob = capi._ptr(model_blob)
    args = [C.byref(cfg), blob, int(model_blob.size)] + ([] if prefix == 'll_' else [_p()]) + [_ref(C.c_void_p)]
    for i in [j for j in range(len(args)) if j != 2]:
        a = list(args)
        a[i] = None
        call('create(null argument %d)' % i, prefix + 'create', *a)
    return out


EXPECTED = {'ll_': {'reset(null handle)': (-1, 'null engine'),
                    'step(null handle)': (-1, 'null engine'),
                    'step_random_n(null handle)': (-1, 'null engine'),
                    'kernel_time_stats(null handle)': (-1, 'null argument'),
                    'kernel_time_stats(null argument 0)': (-1, 'null argument'),
                    'kernel_time_stats(null argument 1)': (-1, 'null argument'),
                    'kernel_time_stats(null argument 2)': (-1, 'null argument'),
                    'set_actions(null handle)': (-1, 'null argument'),
                    'set_actions(null argument 0)': (-1, 'null argument'),
                    'fill_random_actions(null handle)': (-1, 'null engine'),
                    'set_spec_param(null handle)': (-1, 'null engine'),
                    'get_spec_param(null handle)': (-1, 'null argument'),
                    'get_spec_param(null argument 1)': (-1, 'null argument'),
                    'sync(null handle)': (-1, 'null engine'),
                    'get_obs(null handle)': (-1, 'null argument'),
                    'get_obs(null argument 0)': (-1, 'null argument'),
                    'get_state(null handle)': (-1, 'null argument'),
                    'get_state(null argument 0)': (-1, 'null argument'),
                    'set_state(null handle)': (-1, 'null argument'),
                    'set_state(null argument 0)': (-1, 'null argument'),
                    'get_reward_done(null handle)': (-1, 'null engine'),
                    'get_counters(null handle)': (-1, 'null engine'),
                    'device_ptrs(null handle)': (-1, 'null argument'),
                    'device_ptrs(null argument 0)': (-1, 'null argument'),
                    'enable_kernel_timing(null handle)': (-1, 'null engine'),
                    'kernel_time_ms(null handle)': (-1, 'null argument'),
                    'kernel_time_ms(null argument 0)': (-1, 'null argument'),
                    'kernel_time_ms(null argument 1)': (-1, 'null argument'),
                    'destroy(null handle)': (0, None),
                    'get_spec_param(id -1)': (-1, 'unknown spec parameter id'),
                    'set_spec_param(id -1)': (-1, 'unknown spec parameter id'),
                    'get_spec_param(id 27)': (-1, 'unknown spec parameter id'),
                    'set_spec_param(id 27)': (-1, 'unknown spec parameter id'),
                    'create(null argument 0)': (-1, 'null argument'),
                    'create(null argument 1)': (-1, 'null argument'),
                    'create(null argument 3)': (-1, 'null argument')},
            'll_epmc_': {'reset(null handle)': (-1, 'null engine'),
                         'step(null handle)': (-1, 'null engine'),
                         'step_random_n(null handle)': (-1, 'null engine'),
                         'kernel_time_stats(null handle)': (-1, 'null argument'),
                         'kernel_time_stats(null argument 0)': (-1, 'null argument'),
                         'kernel_time_stats(null argument 1)': (-1, 'null argument'),
                         'kernel_time_stats(null argument 2)': (-1, 'null argument'),
                         'set_actions(null handle)': (-1, 'null argument'),
                         'set_actions(null argument 0)': (-1, 'null argument'),
                         'fill_random_actions(null handle)': (-1, 'null engine'),
                         'set_step_draws(null handle)': (-1, 'null argument'),
                         'set_step_draws(null argument 0)': (-1, 'null argument'),
                         'set_spec_param(null handle)': (-1, 'null engine'),
                         'get_spec_param(null handle)': (-1, 'null argument'),
                         'get_spec_param(null argument 1)': (-1, 'null argument'),
                         'sync(null handle)': (-1, 'null engine'),
                         'get_obs(null handle)': (-1, 'null argument'),
                         'get_obs(null argument 0)': (-1, 'null argument'),
                         'get_state(null handle)': (-1, 'null argument'),
                         'get_state(null argument 0)': (-1, 'null argument'),
                         'set_state(null handle)': (-1, 'null argument'),
                         'set_state(null argument 0)': (-1, 'null argument'),
                         'get_reward_done(null handle)': (-1, 'null engine'),
                         'get_counters(null handle)': (-1, 'null engine'),
                         'get_rays(null handle)': (-1, 'null engine'),
                         'get_push_trace(null handle)': (-1, 'null argument'),
                         'get_push_trace(null argument 0)': (-1, 'null argument'),
                         'device_ptrs(null handle)': (-1, 'null argument'),
                         'device_ptrs(null argument 0)': (-1, 'null argument'),
                         'enable_kernel_timing(null handle)': (-1, 'null engine'),
                         'kernel_time_ms(null handle)': (-1, 'null argument'),
                         'kernel_time_ms(null argument 0)': (-1, 'null argument'),
                         'kernel_time_ms(null argument 1)': (-1, 'null argument'),
                         'destroy(null handle)': (0, None),
                         'obs_dim(null handle)': (-1, None),
                         'step(before reset)': (-4, 'll_epmc_reset must be called before ll_epmc_step'),
                         'step_random_n(before reset)': (-4, 'll_epmc_reset must be called before ll_epmc_step_random_n'),
                         'set_step_draws(negative count)': (-1, 'negative draw count'),
                         'get_spec_param(id -1)': (-1, 'unknown spec parameter id'),
                         'set_spec_param(id -1)': (-1, 'unknown spec parameter id'),
                         'get_spec_param(id 27)': (-1, 'unknown spec parameter id'),
                         'set_spec_param(id 27)': (-1, 'unknown spec parameter id'),
                         'create(null argument 0)': (-1, 'null argument'),
                         'create(null argument 1)': (-1, 'null argument'),
                         'create(null argument 3)': (-1, 'null argument'),
                         'create(null argument 4)': (-1, 'null argument')},
            'll_sepmc_': {'reset(null handle)': (-1, 'null engine'),
                          'step(null handle)': (-1, 'null engine'),
                          'step_random_n(null handle)': (-1, 'null engine'),
                          'kernel_time_stats(null handle)': (-1, 'null argument'),
                          'kernel_time_stats(null argument 0)': (-1, 'null argument'),
                          'kernel_time_stats(null argument 1)': (-1, 'null argument'),
                          'kernel_time_stats(null argument 2)': (-1, 'null argument'),
                          'set_actions(null handle)': (-1, 'null argument'),
                          'set_actions(null argument 0)': (-1, 'null argument'),
                          'fill_random_actions(null handle)': (-1, 'null engine'),
                          'set_step_draws(null handle)': (-1, 'null argument'),
                          'set_step_draws(null argument 0)': (-1, 'null argument'),
                          'set_spec_param(null handle)': (-1, 'null engine'),
                          'get_spec_param(null handle)': (-1, 'null argument'),
                          'get_spec_param(null argument 1)': (-1, 'null argument'),
                          'sync(null handle)': (-1, 'null engine'),
                          'get_obs(null handle)': (-1, 'null argument'),
                          'get_obs(null argument 0)': (-1, 'null argument'),
                          'get_state(null handle)': (-1, 'null argument'),
                          'get_state(null argument 0)': (-1, 'null argument'),
                          'set_state(null handle)': (-1, 'null argument'),
                          'set_state(null argument 0)': (-1, 'null argument'),
                          'get_reward_done(null handle)': (-1, 'null engine'),
                          'get_counters(null handle)': (-1, 'null engine'),
                          'get_rays(null handle)': (-1, 'null engine'),
                          'get_push_trace(null handle)': (-1, 'null argument'),
                          'get_push_trace(null argument 0)': (-1, 'null argument'),
                          'device_ptrs(null handle)': (-1, 'null argument'),
                          'device_ptrs(null argument 0)': (-1, 'null argument'),
                          'enable_kernel_timing(null handle)': (-1, 'null engine'),
                          'kernel_time_ms(null handle)': (-1, 'null argument'),
                          'kernel_time_ms(null argument 0)': (-1, 'null argument'),
                          'kernel_time_ms(null argument 1)': (-1, 'null argument'),
                          'destroy(null handle)': (0, None),
                          'obs_dim(null handle)': (-1, None),
                          'step(before reset)': (-4, 'll_sepmc_reset must be called before ll_sepmc_step'),
                          'step_random_n(before reset)': (-4, 'll_sepmc_reset must be called before ll_sepmc_step_random_n'),
                          'set_step_draws(negative count)': (-1, 'negative draw count'),
                          'get_spec_param(id -1)': (-1, 'unknown spec parameter id'),
                          'set_spec_param(id -1)': (-1, 'unknown spec parameter id'),
                          'get_spec_param(id 27)': (-1, 'unknown spec parameter id'),
                          'set_spec_param(id 27)': (-1, 'unknown spec parameter id'),
                          'create(null argument 0)': (-1, 'null argument'),
                          'create(null argument 1)': (-1, 'null argument'),
                          'create(null argument 3)': (-1, 'null argument'),
                          'create(null argument 4)': (-1, 'null argument')}}


@pytest.fixture(scope='module')
def engines(emul_lib, model_blob, mocap_table):
    es = _engines(emul_lib, model_blob, mocap_table)
    yield es
    for e, _ in es.values():
        e.close()


@pytest.mark.parametrize('prefix', PREFIXES)
def test_shared_entry_points_answer_bad_calls_as_recorded(engines, model_blob, prefix):
    got = observe(prefix, *engines[prefix], model_blob)
    assert got == EXPECTED[prefix]


def test_get_rays_refusals_above_512_rows(emul_lib, model_blob):
    e = epmc_capi.EpmcEngine(epmc_capi.make_epmc_config(513, epmc_env_config(1)), model_blob, lib_path=emul_lib)
    s = sepmc_capi.SepmcEngine(sepmc_capi.make_sepmc_config(257, sepmc_env_config((0, 0, 0))), model_blob, lib_path=emul_lib)
    try:
        assert e.lib.ll_epmc_get_rays(e.h, None, None, None, None) == -4
        assert e.lib.ll_last_error().decode() == 'the ray trace is kept for engines of at most 512 envs'
        assert s.lib.ll_sepmc_get_rays(s.h, None, None, None, None) == -4
        assert s.lib.ll_last_error().decode() == 'the ray trace is kept for engines of at most 256 arenas'
    finally:
        e.close(); s.close()
