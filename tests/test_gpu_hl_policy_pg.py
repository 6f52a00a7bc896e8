"""The PPO actor of the on-device EPMC / SEPMC policies (ll_hl_policy_act_pg) on the GPU: single calls at the edges against the float64 reference
fed the same Philox words (tests/hl_policy_pg_ref.py), the device samplers' statistics, the value state through an auto-reset loop, the sampled
actor loop playing the games with the value's explained variance, and ll_hl_policy_act untouched by an attached value branch."""
import numpy as np
import pytest

import hl_policy_pg_ref as G
import hl_policy_ref as R
from test_gpu_hl_policy import SIGMA, SIZES, _epmc_engine, _inputs, _sepmc_engine

pytestmark = pytest.mark.gpu
SEED = 0x1234_5678_9ABC


def _policy(kind, which, max_rows, value=True):
    from lifelike_agility_and_play_amd.policies import hl_policy_hip as H
    if kind == 'epmc':
        path, vpath, cls = R.EPMC_WEIGHTS[which], G.EPMC_VALUE[which], H.HipEpmcPolicy
    else:
        path, vpath, cls = R.SEPMC_WEIGHTS, G.SEPMC_VALUE, H.HipSepmcPolicy
    return cls(path, max_rows, value_npz=vpath if value else None), path, vpath


def _weights(path, vpath):
    w64, w32 = R.load(path), R.load(path, np.float32)
    return w64, w32, G.load_value(vpath, w64), G.load_value(vpath, w32)


def _real_obs(kind, which):
    E = _epmc_engine(which, 256, 1, 3) if kind == 'epmc' else _sepmc_engine(128, 1, 3)
    E.reset()
    E.step_random_n(SIGMA, 20)
    real = E.obs().reshape(-1, E.obs_dim)
    E.close()
    return real


class _Out(object):
    """device outputs of one act_pg call over `pad` rows, filled with sentinels"""

    def __init__(self, kind, pad, nh):
        import torch
        dev = torch.device('cuda')
        self.a = torch.full((pad, 12), float('nan'), device=dev)
        self.c = torch.full((pad,), -7, dtype=torch.int32, device=dev)
        self.hd = torch.full((pad,), float('nan'), device=dev) if kind == 'sepmc' else None
        self.nl = torch.full((pad, nh), float('nan'), device=dev)
        self.v = torch.full((pad,), float('nan'), device=dev)

    def call(self, pol, obs_d, n, reset_d, seed, step, sample, value=True):
        pol.act_pg_ptr(obs_d.data_ptr(), self.a.data_ptr(), n, seed, step, sample, None, reset_d.data_ptr() if reset_d is not None else None,
                       self.c.data_ptr(), self.hd.data_ptr() if self.hd is not None else None, self.nl.data_ptr(), self.v.data_ptr() if value else None)

    def host(self):
        import torch
        torch.cuda.synchronize()
        return dict(action=self.a.cpu().numpy(), code=self.c.cpu().numpy(), heading=self.hd.cpu().numpy() if self.hd is not None else None,
                    neglogp=self.nl.cpu().numpy(), value=self.v.cpu().numpy())


@pytest.mark.parametrize('kind,which', [('epmc', 'hurdle'), ('sepmc', None)])
def test_single_call_at_the_edges(kind, which):
    """act_pg at n = 1 .. 4103 on engine observations, rows far outside the rms range, blank height maps, random policy and value states, every
    7th row reset; rows >= n of every output and of both states keep their sentinels.
    sample=0: the code is ll_hl_policy_act's, actions / heading / policy state equal act's (recorded: bit-identical or not), neglogp and value
    within tolerance of the float64 reference.  sample=1: the code is the reference's wherever the top two perturbed logits are further apart
    than delta (>= 99 % of rows), actions / heading / neglogp / value / value state within tolerance at the kernel's code; the same (seed, step)
    gives bit-identical outputs, and rows 0..16 do not depend on n."""
    import torch
    rng = np.random.default_rng(21)
    real = _real_obs(kind, which)
    N = SIZES[-1]
    pol, path, vpath = _policy(kind, which, N + 32)
    w64, w32, wv64, wv32 = _weights(path, vpath)
    dim, sd = (916, 64) if kind == 'epmc' else (965, 128)
    x_all = _inputs(real, N, dim, rng)
    s_all = rng.normal(0, 0.4, (N + 32, sd)).astype(np.float32)
    v_all = rng.normal(0, 0.4, (N + 32, 64)).astype(np.float32)
    reset_all = np.zeros(N + 32, np.uint8)
    reset_all[::7] = 1
    rs = reset_all[:N].astype(bool)
    obs_d = torch.from_numpy(x_all).cuda()
    reset_d = torch.from_numpy(reset_all).cuda()
    nh = pol.n_heads
    step = 12345
    t = {smp: G.tolerances(kind, w64, w32, x_all, s_all[:N], rs, SEED, step, smp, wv64=wv64, wv32=wv32, vstate=v_all[:N]) for smp in (False, True)}
    for smp in (False, True):
        print('%s sample=%d: delta %.3g, tolerances %s' % (kind, smp, t[smp]['delta'], ' '.join('%s %.3g' % (k[4:], v) for k, v in sorted(t[smp].items())
                                                                                                 if k.startswith('tol_'))))
    head17 = {}
    identical = []
    for smp in (False, True):
        T = t[smp]
        ref = T['ref']
        for n in SIZES:
            what = '%s sample=%d n=%d' % (kind, smp, n)
            pad = n + 32
            o = _Out(kind, pad, nh)
            pol.set_state(s_all)
            pol.set_value_state(v_all)
            o.call(pol, obs_d, n, reset_d, SEED, step, smp)
            out = o.host()
            st, vst = pol.state(), pol.value_state()
            assert np.isnan(out['action'][n:]).all() and (out['code'][n:] == -7).all() and np.isnan(out['neglogp'][n:]).all(), what
            assert np.isnan(out['value'][n:]).all(), what
            np.testing.assert_array_equal(st[n:], s_all[n:], err_msg=what)
            np.testing.assert_array_equal(vst[n:], v_all[n:], err_msg=what)
            if out['heading'] is not None:
                assert np.isnan(out['heading'][n:]).all(), what
            for k in ('action', 'neglogp', 'value'):
                assert np.isfinite(out[k][:n]).all(), (what, k)
            code = out['code'][:n]
            sl = {k: (v[:n] if isinstance(v, np.ndarray) else v) for k, v in ref.items()}
            if not smp:                                                # the modes: exactly what ll_hl_policy_act emits
                a = _Out(kind, pad, nh)
                pol.set_state(s_all)
                pol.act_ptr(obs_d.data_ptr(), a.a.data_ptr(), n, None, reset_d.data_ptr(), a.c.data_ptr(), a.hd.data_ptr() if a.hd is not None else None)
                got = a.host()
                st_act = pol.state()
                np.testing.assert_array_equal(code, got['code'][:n], err_msg=what)
                same = (np.array_equal(out['action'][:n], got['action'][:n]) and np.array_equal(st[:n], st_act[:n])
                        and (out['heading'] is None or np.array_equal(out['heading'][:n], got['heading'][:n])))
                identical.append(same)
                tie = R.near_ties(sl['score'], T['delta'])
            else:
                tie = G.near_ties(sl['pscore'], T['delta'])
                assert tie.mean() <= max(0.01, 1.0 / n), (what, tie.mean())
            wrong = np.flatnonzero(~tie & (code != sl['code']))
            assert not len(wrong), '%s: row %d code %d, reference %d' % (what, wrong[0], code[wrong[0]], sl['code'][wrong[0]])
            at = sl
            if (code != sl['code']).any():
                at = G.forward(kind, w64, x_all[:n], s_all[:n], rs[:n], SEED, step, smp, code=code)
            errs = {'action': np.abs(out['action'][:n] - at['action']).max(), 'neglogp': np.abs(out['neglogp'][:n] - at['neglogp']).max(),
                    'state': np.abs(st[:n] - sl['state']).max(), 'value': np.abs(out['value'][:n] - sl['value']).max(),
                    'vstate': np.abs(vst[:n] - sl['vstate']).max()}
            if out['heading'] is not None:
                errs['heading'] = np.abs(out['heading'][:n] - sl['heading']).max()
            for k, e in errs.items():
                assert e <= T['tol_' + k], '%s: %s off the float64 reference by %.3g (tolerance %.3g)' % (what, k, e, T['tol_' + k])
            if n == N:
                print(what, ' '.join('%s err %.3g' % kv for kv in sorted(errs.items())))
            if smp:
                o2 = _Out(kind, pad, nh)
                pol.set_state(s_all)
                pol.set_value_state(v_all)
                o2.call(pol, obs_d, n, reset_d, SEED, step, smp)
                again = o2.host()
                for k in ('action', 'code', 'neglogp', 'value') + (('heading',) if kind == 'sepmc' else ()):
                    np.testing.assert_array_equal(again[k][:n], out[k][:n], err_msg='%s: %s not reproducible' % (what, k))
                if n >= 17:
                    first = {k: v[:17] for k, v in out.items() if v is not None}
                    if head17:
                        for k, v in first.items():
                            np.testing.assert_array_equal(v, head17[k], err_msg='%s: rows 0..16 of %s depend on n' % (what, k))
                    head17 = head17 or first
    print('%s: sample=0 actions / heading / state bit-identical to ll_hl_policy_act at every n: %s' % (kind, all(identical)))
    pol.close()


@pytest.mark.parametrize('kind', ['epmc', 'sepmc'])
def test_device_sampler_statistics(kind):
    """One observation row copied to 4096 rows, every row reset, 8 steps (32768 draws per head): the sampled codes' histogram passes chi-square
    against the softmax, and the kernel's own exp(-neglogp) of every sampled code is that softmax; the standardised action noise
    (a - mu) / sigma of every dimension, and of the SEPMC heading, has mean 0 and variance 1 within 5 standard errors."""
    import torch
    n, K = 4096, 8
    real = _real_obs(kind, 'hurdle')
    pol, path, _ = _policy(kind, 'hurdle', n, value=False)
    w64 = R.load(path)
    row = real[37:38].astype(np.float32)
    obs_d = torch.from_numpy(np.ascontiguousarray(np.repeat(row, n, axis=0))).cuda()
    reset_d = torch.ones(n, dtype=torch.uint8, device='cuda')
    o = _Out(kind, n, pol.n_heads)
    codes, nls, acts, hds = [], [], [], []
    for k in range(K):
        o.call(pol, obs_d, n, reset_d, 99, 1000 + k, True, value=False)
        out = o.host()
        codes.append(out['code']); nls.append(out['neglogp']); acts.append(out['action'])
        if kind == 'sepmc':
            hds.append(out['heading'])
    m = _Out(kind, n, pol.n_heads)
    m.call(pol, obs_d, 1, reset_d, 99, 0, False, value=False)
    mode = m.host()
    code, nl, act = np.concatenate(codes), np.concatenate(nls), np.concatenate(acts)
    if kind == 'sepmc':      # the heading feeds the mid level, so the codes and means differ per row: the heading's own statistics
        zh = (np.concatenate(hds) - mode['heading'][0]) / np.exp(w64[G.HLC_LOGSTD][0, 0])
        se = 1 / np.sqrt(len(zh))
        print('heading noise: mean %.4f var %.4f (se %.4f)' % (zh.mean(), zh.var(), se))
        assert abs(zh.mean()) < 5 * se and abs(zh.var() - 1) < 5 * np.sqrt(2) * se
    else:
        score = R.forward(kind, w64, row.astype(np.float64), np.zeros((1, 64)))['score'][0]
        p = np.exp(score - score.max())
        p /= p.sum()
        stat, dof, pv = G.chi2_pvalue(np.bincount(code, minlength=256), p)
        print('z codes: %d distinct, chi2 %.1f on %d dof, p %.3g' % (len(np.unique(code)), stat, dof, pv))
        assert pv > 1e-4, (stat, dof, pv)
        np.testing.assert_allclose(np.exp(-nl[:, 0]), p[code], rtol=1e-3)
        uniq, inv = np.unique(code, return_inverse=True)
        mu = G.forward(kind, w64, np.repeat(row, len(uniq), axis=0).astype(np.float64), np.zeros((len(uniq), 64)), sample=False, code=uniq)['action']
        zz = (act - mu[inv]) / np.exp(w64[G.LOGSTD[kind]][0])
        se = 1 / np.sqrt(len(zz))
        print('action noise: |mean| max %.4f, var %.4f .. %.4f (se %.4f)' % (np.abs(zz.mean(0)).max(), zz.var(0).min(), zz.var(0).max(), se))
        assert (np.abs(zz.mean(0)) < 5 * se).all() and (np.abs(zz.var(0) - 1) < 5 * np.sqrt(2) * se).all()
    ls = w64[G.LOGSTD[kind]][0]
    # the llc neglogp is the Gaussian density of the emitted action: 0.5 |eps|^2 + 6 log 2 pi + sum logstd, and its mean is 6 (1 + log 2 pi) + sum logstd
    ent = 6 * (1 + G.LOG_2PI) + ls.sum()
    assert abs(nl[:, -1].mean() - ent) < 5 * np.sqrt(6.0 / len(nl)), (nl[:, -1].mean(), ent)
    pol.close()


@pytest.mark.parametrize('kind', ['epmc', 'sepmc'])
def test_teacher_forced_value_recurrence(kind):
    """64 sampled steps on an auto-reset engine (max_steps 20), act_pg with the done buffer as d_reset: each step the device policy and value
    states are loaded into the float64 reference and the value, value state, actions and neglogp are compared on the re-seeded rows and a sample of
    the others; re-seeded rows' value state comes out of zero."""
    import torch
    from lifelike_agility_and_play_amd import gather
    rng = np.random.default_rng(6)
    E = _epmc_engine('hurdle', 512, 1, 9, max_steps=20) if kind == 'epmc' else _sepmc_engine(256, 1, 9, max_steps=20)
    E.reset()
    pol, path, vpath = _policy(kind, 'hurdle', 512)
    w64, w32, wv64, wv32 = _weights(path, vpath)
    n = E.device_ptrs().n_envs
    T = gather.engine_tensors(E)
    nl = torch.zeros((n, pol.n_heads), device='cuda')
    v = torch.zeros(n, device='cuda')
    code = torch.zeros(n, dtype=torch.int32, device='cuda')
    n_reset, worst = 0, {}
    for step in range(64):
        torch.cuda.synchronize()
        obs = T['obs'].cpu().numpy().astype(np.float64)
        done = T['done'].cpu().numpy().astype(bool) if step else np.zeros(n, bool)
        s0, vs0 = pol.state(), pol.value_state()
        pol.act_pg(E, SEED, step, True, d_neglogp=nl.data_ptr(), d_value=v.data_ptr(), d_code=code.data_ptr())
        torch.cuda.synchronize()
        s1, vs1 = pol.state(), pol.value_state()
        rows = np.union1d(np.flatnonzero(done), rng.choice(n, 32, replace=False))
        n_reset += int(done.sum())
        t = G.tolerances(kind, w64, w32, obs[rows], s0[rows], done[rows], SEED, step, True, rows=rows, wv64=wv64, wv32=wv32, vstate=vs0[rows])
        ref = t['ref']
        kc = code.cpu().numpy()[rows]
        ok = ~G.near_ties(ref['pscore'], t['delta'])
        assert (kc[ok] == ref['code'][ok]).all(), step
        at = ref if (kc == ref['code']).all() else G.forward(kind, w64, obs[rows], s0[rows], done[rows], SEED, step, True, rows=rows, code=kc)
        errs = {'value': np.abs(v.cpu().numpy()[rows] - ref['value']).max(), 'vstate': np.abs(vs1[rows] - ref['vstate']).max(),
                'action': np.abs(T['actions'].cpu().numpy()[rows] - at['action']).max(), 'neglogp': np.abs(nl.cpu().numpy()[rows] - at['neglogp']).max()}
        for k, e in errs.items():
            assert e <= t['tol_' + k], '%s step %d: %s off by %.3g (tolerance %.3g)' % (kind, step, k, e, t['tol_' + k])
            worst[k] = max(worst.get(k, 0.0), e)
        if done.any():
            _, z = G.value(kind, wv64, obs[done], np.zeros((int(done.sum()), 64)))
            assert np.abs(vs1[done] - z).max() <= t['tol_vstate'], step
        E.step()
    torch.cuda.synchronize()
    hs = pol.hs()
    assert hs.shape == (512, 192 if kind == 'epmc' else 256)
    np.testing.assert_array_equal(hs[:, :64], pol.value_state())
    assert not hs[:, 64:128].any()
    print('%s: %d re-seeded rows over 64 steps; worst errors %s' % (kind, n_reset, worst))
    assert n_reset >= n
    pol.close()
    E.close()


def _explained_variance(rew, val, alive, ended, gamma=0.95, tail=100):
    """rew, val, alive [T][n] (alive: the row's episode runs at step t); ended [n]: the episode ended inside the recording.  Returns truncated at
    episode ends; steps of unfinished episodes within `tail` steps of the recording's end are dropped."""
    Tn = rew.shape[0]
    ret = np.zeros_like(rew)
    acc = np.zeros(rew.shape[1])
    for t in range(Tn - 1, -1, -1):
        acc = np.where(alive[t], rew[t] + gamma * acc, 0.0)
        ret[t] = acc
    use = alive.copy()
    use[Tn - tail:, :] &= ended[None, :]
    R_, V_ = ret[use], val[use]
    return 1.0 - np.var(R_ - V_) / np.var(R_), float(np.corrcoef(R_, V_)[0, 1]), int(use.sum()), (R_.mean(), R_.std(), V_.mean(), V_.std())


def _pg_loop(E, pol, steps):
    """act_pg ; step with sampling for `steps` steps, rewards / values / alive masks recorded on the device, one synchronisation at the end"""
    import torch
    from lifelike_agility_and_play_amd import gather
    p = E.device_ptrs()
    n = p.n_envs
    T = gather.engine_tensors(E)
    why = gather.device_tensor(p.done_reason, (n,), torch.uint8)
    gather.use_engine_stream(E)
    try:
        first = torch.zeros(n, dtype=torch.int32, device='cuda')
        alive = torch.ones(n, dtype=torch.bool, device='cuda')
        v = torch.zeros(n, device='cuda')
        nl = torch.zeros((n, pol.n_heads), device='cuda')
        rec_r = torch.zeros((steps, n), device='cuda')
        rec_v = torch.zeros((steps, n), device='cuda')
        rec_a = torch.zeros((steps, n), dtype=torch.bool, device='cuda')
        for t in range(steps):
            pol.act_pg(E, SEED, t, True, d_neglogp=nl.data_ptr(), d_value=v.data_ptr(), reset_from_done=False)
            rec_v[t].copy_(v)
            rec_a[t].copy_(alive)
            E.step()
            rec_r[t].copy_(T['reward'])
            d = T['done'].to(torch.int32) * why.to(torch.int32)
            first.copy_(torch.where(first == 0, d, first))
            alive &= T['done'] == 0
        torch.cuda.current_stream().synchronize()
        return first.cpu().numpy(), rec_r.cpu().numpy().astype(np.float64), rec_v.cpu().numpy().astype(np.float64), rec_a.cpu().numpy(), nl.cpu().numpy()
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream())


# floors from the first measurement on an MI355X (profiles/r08_hl_policy_pg.txt: hurdles reached 0.986, chase tag caught 0.688), with margin.
# The value's explained variance against this engine's returns is recorded, not asserted: it was negative there.
PPO_FLOOR = {'hurdle': 0.9, 'chase': 0.5}


def test_ppo_actor_loop_hurdles():
    """1024 envs on hurdles (max_steps 1000, no auto-reset), act_pg ; step with every head sampled: reach rate >= 0.9, and (recorded) the value's
    explained variance against the realised gamma = 0.95 discounted returns (example_epmc_train.sh)."""
    n = 1024
    E = _epmc_engine('hurdle', n, 0, 0)
    E.reset()
    pol, _, _ = _policy('epmc', 'hurdle', n)
    why, rew, val, alive, nl = _pg_loop(E, pol, 1000)
    E.close()
    pol.close()
    reached, fell = float(((why & 4) != 0).mean()), float(((why & 1) != 0).mean())
    ev, corr, used, mom = _explained_variance(rew, val, alive, why != 0)
    print('EPMC hurdle PPO actor, %d envs: reached %.3f, fell %.3f, unfinished %d; value explained variance %.3f, correlation %.3f over %d steps '
          '(return mean %.3f sd %.3f, value mean %.3f sd %.3f)' % ((n, reached, fell, int((why == 0).sum()), ev, corr, used) + mom))
    assert np.isfinite(nl).all() and np.isfinite(val).all() and val.std() > 0
    assert reached >= PPO_FLOOR['hurdle'], reached


def test_ppo_actor_loop_chase_tag():
    """512 arenas of chase tag (max_steps 700), both robots sampled by act_pg: catch rate >= 0.5, and (recorded) the value's explained variance
    over both robots."""
    import sepmc_parity_common as sc
    n = 512
    E = _sepmc_engine(n, 0, 3)
    E.reset()
    pol, _, _ = _policy('sepmc', None, 2 * n)
    why, rew, val, alive, nl = _pg_loop(E, pol, sc.GAME_MAX_STEPS)
    E.close()
    pol.close()
    caught = float(((why[0::2] & 8) != 0).mean())
    ev, corr, used, mom = _explained_variance(rew, val, alive, why != 0)
    print('SEPMC chase tag PPO actor, %d arenas: caught %.3f, unfinished %d; value explained variance %.3f, correlation %.3f over %d steps '
          '(return mean %.3f sd %.3f, value mean %.3f sd %.3f)' % ((n, caught, int((why == 0).sum()), ev, corr, used) + mom))
    assert np.isfinite(nl).all() and np.isfinite(val).all() and val.std() > 0
    assert caught >= PPO_FLOOR['chase'], caught


@pytest.mark.parametrize('kind', ['epmc', 'sepmc'])
def test_attached_value_leaves_act_bit_identical(kind):
    """ll_hl_policy_act's actions, code, heading and state with and without an attached value branch (and after act_pg calls on it): equal bits."""
    import torch
    rng = np.random.default_rng(2)
    real = _real_obs(kind, 'hurdle')
    n = 1000
    x = torch.from_numpy(_inputs(real, n, 916 if kind == 'epmc' else 965, rng)).cuda()
    res = []
    for value in (False, True):
        pol, _, _ = _policy(kind, 'hurdle', n, value=value)
        if value:
            o = _Out(kind, n, pol.n_heads)
            o.call(pol, x, n, None, 5, 6, True)
            pol.reset_state()
            assert not pol.value_state().any()
        outs = []
        for _ in range(3):
            a = _Out(kind, n, pol.n_heads)
            pol.act_ptr(x.data_ptr(), a.a.data_ptr(), n, None, None, a.c.data_ptr(), a.hd.data_ptr() if a.hd is not None else None)
            h = a.host()
            outs.append((h['action'], h['code'], h['heading'], pol.state()))
        res.append(outs)
        pol.close()
    for (a0, c0, h0, s0), (a1, c1, h1, s1) in zip(*res):
        assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32)) and np.array_equal(c0, c1) and np.array_equal(s0.view(np.uint32), s1.view(np.uint32))
        if h0 is not None:
            assert np.array_equal(h0.view(np.uint32), h1.view(np.uint32))


def test_value_without_branch_is_einval():
    import torch
    from lifelike_agility_and_play_amd import capi
    pol, _, _ = _policy('epmc', 'hurdle', 16, value=False)
    o = _Out('epmc', 16, 2)
    x = torch.zeros((16, 916), device='cuda')
    with pytest.raises(capi.LLError) as ei:
        o.call(pol, x, 16, None, 0, 0, True, value=True)
    assert ei.value.code == -1
    torch.cuda.synchronize()
    assert (o.c.cpu().numpy() == -7).all()                  # nothing was launched
    with pytest.raises(capi.LLError):
        pol.value_state()
    with pytest.raises(capi.LLError) as ei:
        pol.attach_value(weights=np.zeros(100, np.float32))
    assert ei.value.code == -1
    pol.close()
