"""The multi-step PMC kernels with the substep plan and the compare-built turn masks (csrc/pmc_params.hpp SubPlan, lanes.hpp WithSubPlan / WithTurnMasksCmp) on the GPU:
one launch of k control steps equals k single launches (the single-step kernels read their arguments as before) bit for bit, and both stay where the host build of the
kernel source is -- under the default spec and with the planned counts off their defaults, for one full wave plus a partial wave of two and for the 256-register build."""
import os
import subprocess

import numpy as np
import pytest

import parity_common as pc

pytestmark = pytest.mark.gpu

EMUL_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emul')
SIGMA = 0.4


@pytest.fixture(scope='module')
def emul_lib():
    subprocess.check_call(['make', '-C', EMUL_DIR, '-s', '-j2'])
    return os.path.join(EMUL_DIR, '_build', 'libllenv_emul.so')


def everything(E):
    r, d, w = E.reward_done()
    info = E.episode_info()
    return dict(state=E.state(), obs=E.obs(), reward=r, done=d, reason=w, clip=info['clip'], time=info['time'], steps=info['steps'],
                table=np.concatenate([np.ravel(t) for t in E.sampling_table()]))


def against_host_build(G, H, label, recent, easy):
    """the comparison parity_common.check_engine_against_host_build makes after a step both took from the same state and the same actions: same flags and episode
    records; envs whose state agrees to 5e-3 (a contact step is conditioned on the last bit between two float32 builds) agree to 2e-2 in every observation entry and
    5e-3 in the reward; of the envs that started as their clips have them at most one in fifty may be rougher (those dropped onto their bellies are only held to the bars while calm)"""
    a, b = everything(G), everything(H)
    assert np.isfinite(a['obs']).all(), label
    same = (a['done'] == b['done']) & (a['reason'] == b['reason']) & (a['clip'] == b['clip']) & (np.abs(a['time'] - b['time']) < 1e-9) & (a['steps'] == b['steps'])
    sg, sh = a['state'].astype(np.float64), b['state'].astype(np.float64)
    scale = 1.0 + np.maximum(np.abs(sh[:, 7:13]).max(-1, keepdims=True), np.abs(sh[:, 25:37]).max(-1, keepdims=True))
    ds = np.abs(sg - sh); ds[:, 7:13] /= scale; ds[:, 25:37] /= scale
    recent.append(~same | (ds.max(-1) > 5e-3))
    calm = ~np.logical_or.reduce(recent[-3:])      # (the observation carries the two older proprioceptive frames: an env stays set aside while a rough step is among them)
    vel = np.zeros(33, bool); vel[12:30] = True
    obs_vel = np.concatenate([np.zeros(72, bool), np.tile(vel, 3), np.zeros(36, bool)])
    do = np.abs(a['obs'].astype(np.float64) - b['obs'].astype(np.float64)) / np.where(obs_vel, scale, 1.0)
    assert (recent[-1] & easy).sum() <= max(1, int(easy.sum()) // 50), (label, int((recent[-1] & easy).sum()), int(easy.sum()))      # the cap holds for the envs that started as their clips have them
    assert calm.any(), label
    assert do[calm].max() < 2e-2, (label, do[calm].max())
    assert np.abs(a['reward'] - b['reward'])[calm].max() < 5e-3, label
    assert np.abs(a['table'] - b['table']).max() < 1e-6, label


@pytest.mark.parametrize('n_envs,k', [(6, 3), (4100, 2)])
@pytest.mark.parametrize('spec', [dict(), dict(solver_iterations=3, max_contacts_per_leg=2)], ids=['default', 'iters3_contacts2'])
def test_one_launch_of_k_steps_equals_k_launches_and_the_host_build(model_blob, mocap_table, emul_lib, n_envs, k, spec):
    spec = dict(spec)
    kw = dict(auto_reset=1, seed=21, solver_iterations=spec.pop('solver_iterations', 10))
    M = pc.make_engine(model_blob, mocap_table, n_envs, None, **kw)            # k steps in one launch: the multi-step kernel (plan, compare-built masks)
    S = pc.make_engine(model_blob, mocap_table, n_envs, None, **kw)            # k single launches: the single-step kernel
    H = pc.make_engine(model_blob, mocap_table, n_envs, emul_lib, **kw)        # the host build of the kernel source, one step at a time from S's states
    for E in (M, S, H):
        E.set_spec(**spec)
        E.reset()
    s0 = S.state()
    # a hard start for some: dropped onto their bellies with the legs folded (contact slots overflow, legs meet), the rest as the clips have them
    rng = np.random.default_rng(4)
    hard = np.arange(n_envs) % 3 == 0
    s0[hard, 2] = rng.uniform(0.06, 0.12, size=int(hard.sum())).astype(np.float32)
    s0[hard, 13:25] = (np.tile([0.0, -1.4, 2.5], 4) + rng.normal(size=(int(hard.sum()), 12)) * 0.15).astype(np.float32)
    for E in (M, S, H):
        E.set_state(s0)
    M.step_random_n(SIGMA, k)
    recent = []
    for t in range(k):
        H.set_state(S.state())
        S.step_random(SIGMA)
        H.step_random(SIGMA)
        against_host_build(S, H, 'single launches, step %d' % t, recent, ~hard)
    a, b = everything(M), everything(S)
    for key in a:
        np.testing.assert_array_equal(a[key], b[key], err_msg='one launch of %d steps against %d launches: %s' % (k, k, key))
    # (M equals S bit for bit, so M is where the host build is)
    assert np.abs(a['state'][:, 25:37]).max() > 0.1
    for E in (M, S, H):
        E.close()
