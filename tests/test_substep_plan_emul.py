"""The substep plan (csrc/pmc_params.hpp SubPlan, PMC_SUB_PLAN): the step resolves what its substeps branch on -- solver iterations, contact and leg-leg slot counts, the
self-collision, friction-direction, limit-rule and second-ERP switches -- once per control step into two words, and the substeps test bits instead of fetching arguments.
No floating-point operation moves, so the host build of the kernel source with the plan must equal the host build without it (-DPMC_SUB_PLAN=0: every test reads its
argument, as the kernels did before) bit for bit, whatever the switches say and whenever they are set."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import parity_common as pc

EMUL_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emul')
EMUL_LIB = os.path.join(EMUL_DIR, '_build', 'libllenv_emul.so')
NOPLAN_LIB = os.path.join(EMUL_DIR, '_build', 'libllenv_emul_noplan.so')
CSRC = os.path.join(os.path.dirname(EMUL_DIR), os.pardir, 'lifelike_agility_and_play_amd', 'csrc')
N_ENVS, N_STEPS = 6, 3            # one full wave of four envs and a partial wave of two


@pytest.fixture(scope='session')
def emul_lib():
    subprocess.check_call(['make', '-C', EMUL_DIR, '-s', '-j2'])
    return EMUL_LIB


@pytest.fixture(scope='session')
def noplan_lib():
    """the same host build with every new switch off (the flags of tests/emul/Makefile + -DPMC_SUB_PLAN=0); rebuilt when a source is newer"""
    srcs = [os.path.join(EMUL_DIR, f) for f in os.listdir(EMUL_DIR) if f.endswith(('.cpp', '.hpp'))]
    srcs += [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(('.hpp', '.inc'))]
    if not os.path.exists(NOPLAN_LIB) or any(os.path.getmtime(s) > os.path.getmtime(NOPLAN_LIB) for s in srcs):
        os.makedirs(os.path.dirname(NOPLAN_LIB), exist_ok=True)
        subprocess.check_call([os.environ.get('CXX', 'g++'), '-O1', '-g', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-DPMC_SUB_PLAN=0',
                               '-o', NOPLAN_LIB, 'emul.cpp', '-lpthread'], cwd=EMUL_DIR)
    return NOPLAN_LIB


def contact_rich_state(E, seed=3):
    """collapsed, rolled-over robots with folded legs (parity_common.check_contact_rich_parity's): every leg overflows its contact slots, shanks sit on their limits,
    legs reach one another"""
    from scipy.spatial.transform import Rotation as R
    rng = np.random.default_rng(seed)
    st = E.state().astype(np.float64)
    for i in range(st.shape[0]):
        st[i, 2] = rng.uniform(0.05, 0.12)
        st[i, 3:7] = (R.from_quat(st[i, 3:7]) * R.from_euler('xyz', [rng.uniform(-1.4, 1.4) if i % 2 else 0.0, rng.uniform(-0.3, 0.3), 0])).as_quat()
        st[i, 7:13] = rng.normal(size=6) * 0.3
        st[i, 13:25] = np.tile([0.0, -1.4, 2.5], 4) + rng.normal(size=12) * 0.15
        st[i, 25:37] = rng.normal(size=12)
    return st.astype(np.float32)


def outputs(E):
    r, d, w = E.reward_done()
    return dict(state=E.state(), obs=E.obs(), reward=r, done=d, reason=w, table=np.concatenate([np.ravel(t) for t in E.sampling_table()]))


def assert_same(a, b, label):
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg='%s: %s' % (label, k))


@pytest.mark.parametrize('iters', [1, 2, 3, 10])
def test_plan_equals_argument_reads_over_the_switch_matrix(golden, model_blob, mocap_table, emul_lib, noplan_lib, iters):
    clip, t0 = golden['g2_clip'][:N_ENVS], golden['g2_t0'][:N_ENVS]
    A = pc.make_engine(model_blob, mocap_table, N_ENVS, emul_lib, auto_reset=1, seed=5, solver_iterations=iters)
    B = pc.make_engine(model_blob, mocap_table, N_ENVS, noplan_lib, auto_reset=1, seed=5, solver_iterations=iters)
    rng = np.random.default_rng(11)
    acts = (rng.normal(size=(N_STEPS, N_ENVS, 12)) * 0.4).astype(np.float32)
    moved = 0.0
    for mc, sc, ms, fm in itertools.product((1, 2, 4), (0, 1), (1, 2), (0, 2)):
        spec = dict(max_contacts_per_leg=mc, self_collision=sc, max_self=ms, friction_mode=fm)
        for E in (A, B):
            E.set_spec(**spec)
            E.reset(clip=clip, t0=t0)
        st = contact_rich_state(A)
        A.set_state(st); B.set_state(st)
        for t in range(N_STEPS):
            A.step_host(acts[t]); B.step_host(acts[t])
            assert_same(outputs(A), outputs(B), 'solver_iterations=%d %r step %d' % (iters, spec, t))
        assert np.isfinite(A.state()).all()
        moved = max(moved, float(np.abs(A.state()[:, 25:37]).max()))
    assert moved > 0.1                                   # the robots were in motion: the solve had work to do
    A.close(); B.close()


def test_switches_do_change_the_step(golden, model_blob, mocap_table, emul_lib):
    """... and the matrix is not vacuous: from the contact-rich state the planned counts and the friction mode change the result of the step it is set for"""
    clip, t0 = golden['g2_clip'][:N_ENVS], golden['g2_t0'][:N_ENVS]
    act = np.zeros((N_ENVS, 12), np.float32)

    def one_step(iters=10, **spec):
        E = pc.make_engine(model_blob, mocap_table, N_ENVS, emul_lib, auto_reset=0, seed=5, solver_iterations=iters)
        E.set_spec(**spec)
        E.reset(clip=clip, t0=t0)
        E.set_state(contact_rich_state(E))
        E.step_host(act)
        s = E.state()
        E.close()
        return s
    base = one_step()
    assert not np.array_equal(base, one_step(iters=3))
    assert not np.array_equal(base, one_step(max_contacts_per_leg=2))
    assert not np.array_equal(base, one_step(friction_mode=0))


def test_spec_set_between_steps_is_not_stale(golden, model_blob, mocap_table, emul_lib, noplan_lib):
    """step, set_spec(max_contacts_per_leg=2), step, set_spec(self_collision=0), step: the plan is made per control step, so a switch set between two steps acts on the next one
    exactly as it does in the build that reads the arguments"""
    clip, t0 = golden['g2_clip'][:N_ENVS], golden['g2_t0'][:N_ENVS]
    A = pc.make_engine(model_blob, mocap_table, N_ENVS, emul_lib, auto_reset=1, seed=9)
    B = pc.make_engine(model_blob, mocap_table, N_ENVS, noplan_lib, auto_reset=1, seed=9)
    C = pc.make_engine(model_blob, mocap_table, N_ENVS, emul_lib, auto_reset=1, seed=9)             # the plan build with nothing set: the switches must show
    for E in (A, B, C):
        E.reset(clip=clip, t0=t0)
    st = contact_rich_state(A)
    for E in (A, B, C):
        E.set_state(st)
    rng = np.random.default_rng(2)
    acts = (rng.normal(size=(3, N_ENVS, 12)) * 0.4).astype(np.float32)
    differs = []
    for t, spec in enumerate((dict(), dict(max_contacts_per_leg=2), dict(self_collision=0))):
        A.set_spec(**spec); B.set_spec(**spec)
        A.step_host(acts[t]); B.step_host(acts[t]); C.step_host(acts[t])
        assert_same(outputs(A), outputs(B), 'step %d after set_spec(%r)' % (t, spec))
        differs.append(not np.array_equal(A.state(), C.state()))
        C.set_state(A.state())
    assert differs == [False, True, differs[2]] and differs[1], differs
    # the same through one multi-step call per setting (ll_step_random_n re-plans every control step of the launch)
    for E in (A, B):
        E.set_spec(max_contacts_per_leg=4, self_collision=1)
        E.step_random_n(0.3, 2)
        E.set_spec(max_contacts_per_leg=1)
        E.step_random_n(0.3, 3)
    assert_same(outputs(A), outputs(B), 'multi-step calls')
    A.close(); B.close(); C.close()
