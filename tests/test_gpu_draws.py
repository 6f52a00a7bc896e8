"""The HIP library's live random draws against the NumPy Philox reference (draws_parity_common.py, as test_draws_emul.py runs them on the
host build), at the larger-batch build's sizes too; and the fused MFMA policy kernel at its edges against the float64 statement of the policy."""
import numpy as np
import pytest

import draws_parity_common as dc
import philox_ref as pr

pytestmark = pytest.mark.gpu

BIG = 4096 + 104          # past the one-wave-per-SIMD grid: the larger-batch build


def test_pmc_random_policy_actions(model_blob, mocap_table):
    dc.check_pmc_random_actions(model_blob, mocap_table, None, sizes=(1, 5, 67, BIG))


@pytest.mark.parametrize('sepmc', [False, True], ids=['epmc', 'sepmc'])
def test_terrain_random_policy_actions(sepmc):
    dc.check_terrain_random_actions(None, sizes=(1, 5, 67, BIG // 2 if sepmc else BIG), sepmc=sepmc)


def test_pmc_seeded_starts(model_blob, mocap_table):
    dc.check_pmc_starts(model_blob, mocap_table, None, n=BIG)


def test_pmc_auto_reset_reseeds(model_blob, mocap_table):
    dc.check_pmc_reseeds(model_blob, mocap_table, None, n=256)


def test_epmc_seeded_resets_and_step_draws():
    dc.check_epmc_seeded_resets(None, n=67)
    dc.check_epmc_step_draws(None, n=67)


def test_sepmc_seeded_resets_and_step_draws():
    dc.check_sepmc_seeded_resets(None, n=34)


def test_fused_policy_kernel_at_its_edges(model_blob, mocap_table):
    """ll_policy_act / ll_policy_act_pg at n = 1, 15, 16, 17, 33, 1000, 4103 on engine observations, rows far outside the rms range (the +-5
    clip on every column) and rows at the rms mean.  Rows >= n of every output keep their sentinel.  Outside near-ties the code is the float64
    argmax; every env's action is the float64 decoder's at the kernel's code; tolerances from a float32 NumPy pass (policy_tolerances).
    Sampled actions are the kernel's mean + exp(logstd) * eps of the policy-noise stream, and neglogp is that draw's, env by env."""
    import torch
    from conftest import POLICY_WEIGHTS
    import parity_common as pc
    from lifelike_agility_and_play_amd import pmc_policy_hip
    from oracle.pmc_policy import PmcPolicy
    w = PmcPolicy(POLICY_WEIGHTS).w
    E = pc.make_engine(model_blob, mocap_table, 512, None, seed=3, auto_reset=1)
    E.reset()
    for _ in range(20):
        E.step_random(pc.SIGMA)
    real = E.obs()
    E.close()
    pol = pmc_policy_hip.HipPmcPolicy()
    lib = pol.lib
    logstd = w[27].ravel()
    seed, step = 0x1234567890, (1 << 32) + 5                 # both words of the key and of the step counter in use
    dev = torch.device('cuda')
    x_all = dc.policy_inputs(real, w, 4096 + 7)
    t = dc.policy_tolerances(w, x_all)                      # on every row any launch below sees: each launch takes a prefix
    print('delta %.3g, action tol %.3g, value tol %.3g' % (t['delta'], t['tol_a'], t['tol_v']))
    for n in (1, 15, 16, 17, 33, 1000, 4096 + 7):
        x = x_all[:n]
        ref = {k: v[:n] for k, v in t['ref'].items()}
        obs = torch.from_numpy(x).to(dev)
        pad = n + 32

        def outs():
            return (torch.full((pad, 12), float('nan'), device=dev), torch.full((pad,), -7, dtype=torch.int32, device=dev),
                    torch.full((pad,), float('nan'), device=dev), torch.full((pad,), float('nan'), device=dev))

        def run(fn):
            torch.cuda.synchronize()
            pol._chk(fn())
            torch.cuda.synchronize()
        a0, c0, _, _ = outs()
        run(lambda: lib.ll_policy_act(pol.h, obs.data_ptr(), a0.data_ptr(), c0.data_ptr(), n, None))
        a1, c1, nl1, v1 = outs()
        run(lambda: lib.ll_policy_act_pg(pol.h, obs.data_ptr(), a1.data_ptr(), c1.data_ptr(), nl1.data_ptr(), v1.data_ptr(), n, seed, step, 0, None))
        a2, c2, nl2, v2 = outs()
        run(lambda: lib.ll_policy_act_pg(pol.h, obs.data_ptr(), a2.data_ptr(), c2.data_ptr(), nl2.data_ptr(), v2.data_ptr(), n, seed, step, 1, None))
        a0, c0, a1, c1, nl1, v1, a2, c2, nl2, v2 = (z.cpu().numpy() for z in (a0, c0, a1, c1, nl1, v1, a2, c2, nl2, v2))
        what = 'n=%d' % n
        for name, z in (('actions', a0), ('actions (pg)', a1), ('neglogp', nl1), ('value', v1), ('sampled actions', a2), ('sampled neglogp', nl2), ('value (sampled)', v2)):
            assert np.isnan(z[n:]).all(), '%s: %s written past row n' % (what, name)
            assert np.isfinite(z[:n]).all(), '%s: %s not written' % (what, name)
        for name, z in (('code', c0), ('code (pg)', c1), ('code (sampled)', c2)):
            assert (z[n:] == -7).all(), '%s: %s written past row n' % (what, name)
        code = c0[:n]
        assert ((code >= 0) & (code < 256)).all()
        np.testing.assert_array_equal(c1[:n], code); np.testing.assert_array_equal(c2[:n], code)
        tie = dc.near_ties(ref['score'], t['delta'])
        assert tie.mean() <= max(0.01, 1.0 / n), (what, tie.mean())
        wrong = np.flatnonzero(~tie & (code != ref['code']))
        assert not len(wrong), '%s: env %d chose code %d, the float64 argmax is %d (margin %.3g >= delta %.3g)' % (
            what, wrong[0], code[wrong[0]], ref['code'][wrong[0]], np.diff(np.sort(ref['score'][wrong[0]])[-2:])[0], t['delta'])
        if tie.any():                                         # a near-tie: the float64 decoder at the kernel's code, and a close runner-up
            sc = ref['score'][np.flatnonzero(tie), code[tie]]
            assert (ref['score'][tie].max(1) - sc < t['delta']).all()
        at = dc.policy_forward(w, x, code=code)
        for name, z in (('actions', a0[:n]), ('actions (pg, mean)', a1[:n])):
            err = np.abs(z - at['action'])
            assert err.max() <= t['tol_a'], '%s: %s off the float64 policy by %.3g (tolerance %.3g) at env %d' % (what, name, err.max(), t['tol_a'], err.max(1).argmax())
        np.testing.assert_array_equal(a1[:n], a0[:n])
        for name, z in (('value', v1[:n]), ('value (sampled)', v2[:n])):
            err = np.abs(z - at['value'])
            assert err.max() <= t['tol_v'], '%s: %s off the float64 value head by %.3g (tolerance %.3g)' % (what, name, err.max(), t['tol_v'])
        const = 6.0 * np.log(2.0 * np.pi) + logstd.sum()
        np.testing.assert_allclose(nl1[:n], const, rtol=2e-6, atol=2e-5)        # neglogp at the mode
        eps, m = pr.policy_noise(n, step, seed)
        std = np.exp(logstd.astype(np.float32)).astype(np.float64)
        want = a1[:n].astype(np.float64) + std * eps
        err = np.abs(a2[:n] - want)
        tol = 2e-6 * std * m + 2e-7 * np.abs(want) + 1e-7
        bad = np.argwhere(err > tol)
        assert not len(bad), '%s: sampled action (env, col) %s is %r, mean + exp(logstd) * eps_ref = %r' % (what, tuple(bad[0]), a2[tuple(bad[0])], want[tuple(bad[0])])
        nl_ref = 0.5 * (eps ** 2).sum(1) + const
        err = np.abs(nl2[:n] - nl_ref)
        tol = 4e-6 * (eps ** 2).sum(1) + 2e-6 * (0.5 * (eps ** 2).sum(1) + np.abs(logstd).sum() + 6.0 * np.log(2.0 * np.pi))   # float32 sum of 13 terms
        assert (err <= tol).all(), '%s: neglogp off by %.3g at env %d' % (what, err.max(), err.argmax())
    pol.close()
