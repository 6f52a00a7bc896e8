"""The live random draws of the kernel source compiled for the host (tests/emul) against the NumPy Philox reference (philox_ref.py):
random-policy actions, seeded PMC starts, seeded EPMC / SEPMC resets and step draws.  tests/test_gpu_draws.py repeats them on the HIP library."""
import os
import subprocess

import numpy as np
import pytest

import draws_parity_common as dc
import philox_ref as pr

EMUL_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emul')
EMUL_LIB = os.path.join(EMUL_DIR, '_build', 'libllenv_emul.so')


@pytest.fixture(scope='module')
def emul_lib():
    subprocess.check_call(['make', '-C', EMUL_DIR, '-s', '-j2'])
    return EMUL_LIB


def test_philox_known_answers():
    """Random123's philox4x32_R(10) known-answer vectors, scalar and broadcast"""
    for ctr, key, out in pr.KNOWN_ANSWERS:
        assert tuple(int(w) for w in pr.philox4x32_10(*ctr, *key)) == out
    ctr = np.array([k[0] for k in pr.KNOWN_ANSWERS], dtype=np.uint64)
    key = np.array([k[1] for k in pr.KNOWN_ANSWERS], dtype=np.uint64)
    got = np.stack(pr.philox4x32_10(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], key[:, 0], key[:, 1]), axis=1)
    np.testing.assert_array_equal(got, np.array([k[2] for k in pr.KNOWN_ANSWERS], dtype=np.uint32))


def test_derived_draws():
    """the conversions at their edges: u01_from's 53 bits, the 24-bit EPMC uniform with its block-of-four indexing, Box-Muller's clamp"""
    assert pr.u01_from(0, 0) == 0.0 and pr.u01_from(0xffffffff, 0xffffffff) == 1.0 - 2.0 ** -53
    assert pr.u01_from(0, 0x7ff) == 0.0 and pr.u01_from(0, 0x800) == 2.0 ** -53
    blk = pr.philox4x32_10(3, 2, 1, pr.EPMC_STEP_SALT, 5, 0)
    u = pr.epmc_stream([3], [2], pr.EPMC_STEP_SALT, 5, 8, start=2)[0]
    np.testing.assert_array_equal(u[2:6], [np.float32((int(w) >> 8) / 2.0 ** 24) for w in blk])
    z, m = pr.box_muller4([np.uint32(0xffffffff), np.uint32(0), np.uint32(0), np.uint32(0)])
    assert m[0] == 0.0 and m[2] == np.sqrt(-2.0 * np.log(2.0 ** -32))          # u1 clamps to 1; u3 = 2^-32, never 0
    # SEEDS[1] is chosen for row 0, group 2 at step 0: its first word is 82, where the + 1 of u1 is visible
    r = pr.philox4x32_10(2, 0, 0, pr.RANDOM_POLICY_SALT, *pr.seed_key(dc.SEEDS[1]))
    assert int(r[0]) < 128 and dc.SEEDS[1] >> 32 == 1


def test_pmc_random_policy_actions(model_blob, mocap_table, emul_lib):
    dc.check_pmc_random_actions(model_blob, mocap_table, emul_lib, sizes=(1, 5, 67))


@pytest.mark.parametrize('sepmc', [False, True], ids=['epmc', 'sepmc'])
def test_terrain_random_policy_actions(emul_lib, sepmc):
    dc.check_terrain_random_actions(emul_lib, sizes=(1, 5, 67) if not sepmc else (1, 5, 34), sepmc=sepmc)


def test_pmc_seeded_starts(model_blob, mocap_table, emul_lib):
    dc.check_pmc_starts(model_blob, mocap_table, emul_lib, n=67)


def test_pmc_auto_reset_reseeds(model_blob, mocap_table, emul_lib):
    dc.check_pmc_reseeds(model_blob, mocap_table, emul_lib, n=24)


def test_epmc_seeded_resets(emul_lib):
    dc.check_epmc_seeded_resets(emul_lib, n=3)


def test_epmc_step_draws(emul_lib):
    dc.check_epmc_step_draws(emul_lib, n=3)


def test_sepmc_seeded_resets_and_step_draws(emul_lib):
    dc.check_sepmc_seeded_resets(emul_lib, n=2)


def policy_obs(model_blob, mocap_table, emul_lib, n=64):
    import parity_common as pc
    E = pc.make_engine(model_blob, mocap_table, n, emul_lib, seed=3, auto_reset=1)
    E.reset()
    E.step_random(pc.SIGMA)
    obs = E.obs()
    E.close()
    return obs


def test_policy_tolerances_have_power(model_blob, mocap_table, emul_lib):
    """The tolerances test_gpu_draws.py holds the fused policy kernel to, derived here from a float32 NumPy pass: a float32 policy with the
    clip at +-4, or with one bias dropped, falls outside them; the float32 pass itself stays inside."""
    from conftest import POLICY_WEIGHTS
    from oracle.pmc_policy import PmcPolicy
    w = PmcPolicy(POLICY_WEIGHTS).w
    x = dc.policy_inputs(policy_obs(model_blob, mocap_table, emul_lib), w, 600)
    t = dc.policy_tolerances(w, x)
    ref = t['ref']
    np.testing.assert_allclose(ref['action'], PmcPolicy(POLICY_WEIGHTS).act(x.astype(np.float64)), rtol=0, atol=1e-9)   # the oracle's statement
    np.testing.assert_allclose(ref['value'], PmcPolicy(POLICY_WEIGHTS).value(x.astype(np.float64)), rtol=0, atol=1e-9)
    tie = dc.near_ties(ref['score'], t['delta'])
    assert tie.mean() < 0.05, tie.mean()
    f32 = dc.policy_forward(w, x, np.float32)
    assert (f32['code'][~tie] == ref['code'][~tie]).all()
    for kw in (dict(clip=4.0), dict(drop_bias=22), dict(drop_bias=26), dict(drop_bias=5)):
        bad = dc.policy_forward(w, x, np.float32, code=ref['code'], **kw)
        da, dv = np.abs(bad['action'] - ref['action']).max(), np.abs(bad['value'] - ref['value']).max()
        assert da > t['tol_a'] or dv > t['tol_v'], (kw, da, dv, t)
        if 'clip' in kw or kw['drop_bias'] != 5:
            assert da > t['tol_a'], (kw, da, t)
    print('delta %.3g, action tol %.3g, value tol %.3g, near ties %.2f %%' % (t['delta'], t['tol_a'], t['tol_v'], 100 * tie.mean()))
