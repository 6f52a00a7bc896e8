"""The multi-step one-wave-per-SIMD PMC kernels with the trimmed front half of the substep (csrc/pmc_params.hpp PMC_FRONT_TRIM, lanes.hpp WithFrontTrim) on the GPU, from
the contact-rich state of tests/test_front_trim_emul.py (legs overflowing their contact slots, shanks on their limits, legs touching): one launch of three control steps
equals three single launches bit for bit -- the single-step kernels run the candidate loop and the winner scan as they were, so this is the trimmed code against the
untrimmed code on the device -- and both stay where the host build of the kernel source is.  Six envs (a full wave and a partial wave of two) and eight (two full waves)."""
import os
import subprocess

import numpy as np
import pytest

import parity_common as pc
from test_front_trim_emul import STATE_SEED
from test_gpu_substep_plan import SIGMA, against_host_build, everything
from test_substep_plan_emul import contact_rich_state

pytestmark = pytest.mark.gpu

EMUL_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emul')
K = 3


@pytest.fixture(scope='module')
def emul_lib():
    subprocess.check_call(['make', '-C', EMUL_DIR, '-s', '-j2'])
    return os.path.join(EMUL_DIR, '_build', 'libllenv_emul.so')


@pytest.mark.parametrize('n_envs', [6, 8])
def test_one_launch_of_three_steps_equals_three_launches_and_the_host_build(golden, model_blob, mocap_table, emul_lib, n_envs):
    clip, t0 = golden['g2_clip'][:n_envs], golden['g2_t0'][:n_envs]
    kw = dict(auto_reset=1, seed=21)
    M = pc.make_engine(model_blob, mocap_table, n_envs, None, **kw)            # three steps in one launch: the multi-step kernel (trimmed)
    S = pc.make_engine(model_blob, mocap_table, n_envs, None, **kw)            # three single launches: the single-step kernel (as it was)
    H = pc.make_engine(model_blob, mocap_table, n_envs, emul_lib, **kw)        # the host build of the kernel source, one step at a time from S's states
    for E in (M, S, H):
        E.reset(clip=clip, t0=t0)
    s0 = contact_rich_state(S, seed=STATE_SEED)
    for E in (M, S, H):
        E.set_state(s0)
    M.step_random_n(SIGMA, K)
    recent, nobody_easy = [], np.zeros(n_envs, bool)                           # (every env starts hard: none is held to the cap of the envs that start as their clips have them)
    for t in range(K):
        H.set_state(S.state())
        S.step_random(SIGMA)
        H.step_random(SIGMA)
        against_host_build(S, H, '%d envs, single launches, step %d' % (n_envs, t), recent, nobody_easy)
    a, b = everything(M), everything(S)
    for key in a:
        np.testing.assert_array_equal(a[key], b[key], err_msg='%d envs, one launch of %d steps against %d launches: %s' % (n_envs, K, K, key))
    # (M equals S bit for bit, so M is where the host build is)
    assert np.abs(a['state'][:, 25:37]).max() > 0.1
    for E in (M, S, H):
        E.close()
