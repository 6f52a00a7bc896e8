"""The fused EPMC / SEPMC policy kernels (include/hl/llenv_hl_policy.h) on the GPU: one call at the edges against the float64 NumPy policy,
a teacher-forced closed loop on auto-reset engines, and the device actor loop playing the games the NumPy policy is recorded on."""
import os
import sys

import numpy as np
import pytest

import hl_policy_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 15, 16, 17, 33, 1000, 4096 + 7)
SIGMA = float(np.exp(-2.0))


def _epmc_engine(which, n, auto_reset, seed, max_steps=None):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import rollout_epmc_policy as RO
    import epmc_parity_common as ec
    cfg = RO.env_config(RO.ELEMENT[which], n)
    if max_steps:
        cfg['max_steps'] = max_steps
    return ec.make_engine(cfg, n, None, auto_reset=auto_reset, seed=seed)


def _sepmc_engine(n_arenas, auto_reset, seed, max_steps=None):
    import sepmc_parity_common as sc
    cfg = sc._game_cfg()
    if max_steps:
        cfg['max_steps'] = max_steps
    return sc.make_engine(cfg, n_arenas, None, auto_reset=auto_reset, seed=seed)


def _policy(kind, which, max_rows):
    from lifelike_agility_and_play_amd.policies import hl_policy_hip as H
    if kind == 'epmc':
        return H.HipEpmcPolicy(R.EPMC_WEIGHTS[which], max_rows), R.EPMC_WEIGHTS[which]
    return H.HipSepmcPolicy(R.SEPMC_WEIGHTS, max_rows), R.SEPMC_WEIGHTS


def _inputs(real, n, dim, rng):
    """n rows from engine observations: most as they are (jittered), then rows far outside the rms range, rows with a blank height map"""
    x = real[rng.integers(0, len(real), n)].astype(np.float32)
    x[:, :135] += rng.normal(0, 0.01, (n, 135)).astype(np.float32)
    far = rng.random(n) < 0.08
    x[far, :135] *= rng.choice([-60.0, 60.0], (int(far.sum()), 135)).astype(np.float32)
    blank = rng.random(n) < 0.08
    x[blank, 135:460] = 0.0
    x[blank, 588:913] = 3.0
    return np.ascontiguousarray(x[:, :dim])


def compare(kind, what, t, n, act, code, state, heading=None, reset=None, w64=None, obs=None, state0=None):
    """one launch's outputs (rows < n) against the float64 reference `t` (hl_policy_ref.tolerances) -- the code outside near-ties, the actions
    at the kernel's code, the new state, the heading"""
    ref = t['ref']
    tie = R.near_ties(ref['score'], t['delta'])
    assert tie.mean() <= max(0.01, 1.0 / n), (what, tie.mean())
    assert ((code >= 0) & (code < 256)).all(), what
    wrong = np.flatnonzero(~tie & (code != ref['code']))
    assert not len(wrong), '%s: row %d chose code %d, the float64 argmax is %d (margin %.3g >= delta %.3g)' % (
        what, wrong[0], code[wrong[0]], ref['code'][wrong[0]], np.diff(np.sort(ref['score'][wrong[0]])[-2:])[0], t['delta'])
    if tie.any():
        sc = ref['score'][np.flatnonzero(tie), code[tie]]
        assert (ref['score'][tie].max(1) - sc < t['delta']).all(), what
    at = R.forward(kind, w64, obs, state0, reset, code=code) if (code != ref['code']).any() else ref
    errs = {'action': np.abs(act - at['action']).max(), 'state': np.abs(state - ref['state']).max()}
    if heading is not None:
        errs['heading'] = np.abs(heading - ref['heading']).max()
    for k, e in errs.items():
        assert e <= t['tol_' + k], '%s: %s off the float64 policy by %.3g (tolerance %.3g)' % (what, k, e, t['tol_' + k])
    return errs


@pytest.mark.parametrize('kind,which', [('epmc', 'hurdle'), ('epmc', 'hole'), ('sepmc', None)])
def test_single_call_at_the_edges(kind, which):
    """ll_hl_policy_act at n = 1, 15, 16, 17, 33, 1000, 4103 on engine observations (20 random steps in), rows far outside the rms range, rows with
    a blank height map, random non-zero LSTM states (set_state) and every 7th row flagged in d_reset.  Rows >= n of actions, code, heading and
    state keep their sentinels; outside near-ties the code is the float64 argmax; actions are the float64 controller at the kernel's code; state and
    heading within tolerances from a float32 NumPy pass."""
    import torch
    dev = torch.device('cuda')
    rng = np.random.default_rng(11)
    if kind == 'epmc':
        E = _epmc_engine(which, 256, 1, 3)
    else:
        E = _sepmc_engine(128, 1, 3)
    E.reset()
    E.step_random_n(SIGMA, 20)
    real = E.obs().reshape(-1, E.obs_dim)
    E.close()
    N = SIZES[-1]
    pol, path = _policy(kind, which, N + 32)
    dim, sd = (916, 64) if kind == 'epmc' else (965, 128)
    assert pol.state_dim == sd
    x_all = _inputs(real, N, dim, rng)
    s_all = (rng.normal(0, 0.4, (N + 32, sd))).astype(np.float32)
    reset_all = np.zeros(N + 32, np.uint8)
    reset_all[::7] = 1
    w64, w32 = R.load(path), R.load(path, np.float32)
    t_all = R.tolerances(kind, w64, w32, x_all, s_all[:N], reset_all[:N].astype(bool))
    print('%s %s: delta %.3g, tolerances action %.3g state %.3g%s' % (kind, which, t_all['delta'], t_all['tol_action'], t_all['tol_state'],
                                                                      ', heading %.3g' % t_all['tol_heading'] if kind == 'sepmc' else ''))
    obs_d = torch.from_numpy(x_all).to(dev)
    reset_d = torch.from_numpy(reset_all).to(dev)
    for n in SIZES:
        pad = n + 32
        a = torch.full((pad, 12), float('nan'), device=dev)
        c = torch.full((pad,), -7, dtype=torch.int32, device=dev)
        hd = torch.full((pad,), float('nan'), device=dev) if kind == 'sepmc' else None
        pol.set_state(s_all)
        torch.cuda.synchronize()
        pol.act_ptr(obs_d.data_ptr(), a.data_ptr(), n, None, reset_d.data_ptr(), c.data_ptr(), hd.data_ptr() if hd is not None else None)
        torch.cuda.synchronize()
        st = pol.state()
        a, c = a.cpu().numpy(), c.cpu().numpy()
        what = '%s %s n=%d' % (kind, which, n)
        assert np.isnan(a[n:]).all() and (c[n:] == -7).all(), '%s: written past row n' % what
        assert np.isfinite(a[:n]).all(), what
        np.testing.assert_array_equal(st[n:], s_all[n:], err_msg='%s: state written past row n' % what)
        h = None
        if hd is not None:
            h = hd.cpu().numpy()
            assert np.isnan(h[n:]).all() and np.isfinite(h[:n]).all() and (np.abs(h[:n]) <= np.pi + 1e-6).all(), what
            h = h[:n]
        t = dict(t_all, ref={k: v[:n] for k, v in t_all['ref'].items()})
        errs = compare(kind, what, t, n, a[:n], c[:n], st[:n], h, reset_all[:n].astype(bool), w64, x_all[:n], s_all[:n])
        if n == N:
            print(what, ' '.join('%s err %.3g' % kv for kv in sorted(errs.items())), 'reset rows %d' % int(reset_all[:n].sum()))
    pol.close()


@pytest.mark.parametrize('kind', ['epmc', 'sepmc'])
def test_teacher_forced_recurrence(kind):
    """64 closed-loop steps on an auto-reset engine (EPMC 512 envs, SEPMC 256 arenas; max_steps 20 so that episodes end and re-seed), the policy
    acting with the engine's done buffer as d_reset.  Each step the device state is loaded into the float64 reference and one step is compared as in
    the single-call test on the rows that were re-seeded and a sample of the others; re-seeded rows must come out of zero state."""
    import torch
    from lifelike_agility_and_play_amd import gather
    rng = np.random.default_rng(5)
    if kind == 'epmc':
        E = _epmc_engine('hurdle', 512, 1, 9, max_steps=20)
    else:
        E = _sepmc_engine(256, 1, 9, max_steps=20)
    E.reset()
    pol, path = _policy(kind, 'hurdle', 512)
    w64, w32 = R.load(path), R.load(path, np.float32)
    p = E.device_ptrs()
    n = p.n_envs
    T = gather.engine_tensors(E)
    n_reset, worst = 0, {}
    for step in range(64):
        torch.cuda.synchronize()
        obs = T['obs'].cpu().numpy().astype(np.float64)
        done = T['done'].cpu().numpy().astype(bool) if step else np.zeros(n, bool)
        s0 = pol.state()
        code = torch.full((n,), -7, dtype=torch.int32, device='cuda')
        hd = torch.zeros(n, device='cuda') if kind == 'sepmc' else None
        pol.act(E, reset_from_done=True, d_code=code.data_ptr(), d_heading=hd.data_ptr() if hd is not None else None)
        torch.cuda.synchronize()
        s1 = pol.state()
        rows = np.union1d(np.flatnonzero(done), rng.choice(n, 48, replace=False))
        n_reset += int(done.sum())
        t = R.tolerances(kind, w64, w32, obs[rows], s0[rows], done[rows])
        act = T['actions'].cpu().numpy()[rows]
        errs = compare(kind, '%s step %d' % (kind, step), t, len(rows), act, code.cpu().numpy()[rows], s1[rows],
                       hd.cpu().numpy()[rows] if hd is not None else None, done[rows], w64, obs[rows], s0[rows])
        for k, e in errs.items():
            worst[k] = max(worst.get(k, 0.0), e)
        if done.any():                                        # the re-seeded rows: the same step from an explicitly zero state
            z = R.forward(kind, w64, obs[done], np.zeros((int(done.sum()), pol.state_dim)))
            assert np.abs(s1[done] - z['state']).max() <= t['tol_state'], step
        E.step()
    torch.cuda.synchronize()
    print('%s: %d re-seeded rows over 64 steps; worst errors %s' % (kind, n_reset, worst))
    assert n_reset >= n, n_reset                              # every row ended at least one episode (max_steps 20) and was re-seeded
    pol.close()
    E.close()


def _first_end(T, first):
    """first[r] <- the engine's done_reason of row r at its first done (device ops on the engine's stream: no host synchronisation)"""
    import torch
    d = T['done'].to(first.dtype) * T['why'].to(first.dtype)
    first.copy_(torch.where(first == 0, d, first))


def _device_loop(E, pol, steps):
    """act ; step for `steps` steps, first end reason per row recorded on the device, one synchronisation at the end"""
    import torch
    from lifelike_agility_and_play_amd import gather
    p = E.device_ptrs()
    T = gather.engine_tensors(E)
    T['why'] = gather.device_tensor(p.done_reason, (p.n_envs,), torch.uint8)
    gather.use_engine_stream(E)
    try:
        first = torch.zeros(p.n_envs, dtype=torch.int32, device='cuda')
        for _ in range(steps):
            pol.act(E, reset_from_done=False)
            E.step()
            _first_end(T, first)
        torch.cuda.current_stream().synchronize()
        return first.cpu().numpy()
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream())


@pytest.mark.parametrize('which', ['hurdle', 'cube'])
def test_device_actor_loop_plays_playground(which):
    """1024 envs, the protocol of tools/rollout_epmc_policy (reference semantics, max_steps 1000), every episode to its end with act ; step on the device:
    reached >= 0.9, fell <= 0.1 (recorded with the NumPy policy: hurdles 1020 / 1024 reach, stairs 984 / 1024)."""
    n = 1024
    E = _epmc_engine(which, n, 0, 0)
    E.reset()
    pol, _ = _policy('epmc', which, n)
    why = _device_loop(E, pol, 1000)
    E.close()
    pol.close()
    reached, fell = float(((why & 4) != 0).mean()), float(((why & 1) != 0).mean())
    print('EPMC %s, %d envs, device actor loop: reached %.3f, fell %.3f, timed out %.3f, unfinished %d' % (
        which, n, reached, fell, float(((why & 2) != 0).mean()), int((why == 0).sum())))
    assert (why != 0).all()
    assert reached >= 0.9 and fell <= 0.1, (reached, fell)


def test_device_actor_loop_plays_chase_tag():
    """512 arenas, the game configuration of sepmc_parity_common (max_steps 700), both robots driven by the device policy: caught >= 0.6
    (NumPy policy: 79-80 %)."""
    import sepmc_parity_common as sc
    n = 512
    E = _sepmc_engine(n, 0, 3)
    E.reset()
    pol, _ = _policy('sepmc', None, 2 * n)
    why = _device_loop(E, pol, sc.GAME_MAX_STEPS)[0::2]
    E.close()
    pol.close()
    caught = float(((why & 8) != 0).mean())
    print('SEPMC, %d arenas, device actor loop: caught %.3f, robot 0 down %.3f, timed out %.3f, unfinished %d' % (
        n, caught, float(((why & 1) != 0).mean()), float(((why & ~9 & 2) != 0).mean()), int((why == 0).sum())))
    assert (why != 0).all()
    assert caught >= 0.6, caught
