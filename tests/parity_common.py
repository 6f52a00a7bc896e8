"""Parity checks shared by the CPU kernel-logic tests (host emulation of the kernel body) and the GPU tests
(the real HIP library through the C ABI).  Every check compares an Engine (float32) with the float64 oracle or
with reference-generated goldens on identical inputs.

Tolerances (float32 engine vs float64 reference/oracle), as stated in BASELINE.md §5:
  * non-physics math (mocap, obs, reward, flags): 1e-5
  * physics: one control step (10 substeps, contacts included): EVERY sample's state error <= 1e-4 for the configuration
    (base position, quaternion, joint angles) and, for velocities -- joint rates reach 35 rad/s on links that weigh
    170 g, so an absolute 1e-4 is below float32 resolution of the accelerations involved -- <= 1e-3 RELATIVE to
    (1 + largest joint rate of that env), with at most 1 % of the samples above 1e-4.
"""
import numpy as np

from conftest import PMC_PROP_TYPE, PMC_REWARD_WEIGHTS, make_oracle_batch
from lifelike_agility_and_play_amd import capi

NONPHYS_TOL = 1e-5
PHYS_STEP_TOL = 1e-4
SIGMA = float(np.exp(-2.0))          # SURVEY 8d synthetic action scale
TIE_ZONE = 2e-6                      # m: float32 resolution of a contact depth / capsule distance (run_lockstep's selection-tie rule)


def make_engine(model_blob, table, n_envs, lib_path=None, **kw):
    kw.setdefault('control_freq', 50.0)
    kw.setdefault('kd', 0.5)
    kw.setdefault('reward_weights', PMC_REWARD_WEIGHTS)
    kw.setdefault('prop_type', PMC_PROP_TYPE)
    kw.setdefault('prioritized_sample_factor', 3.0)
    cfg = capi.make_config(n_envs, **kw)
    return capi.Engine(cfg, model_blob, table, lib_path=lib_path)


def config_scalars(cfg=None):
    """what the comparators restate of an env_config dict `cfg` (the keys of capi.make_config; None: the training scripts' point, the defaults of
    make_engine / make_oracle_batch): kp, kd, max_tau, the substeps of one control step (PLE:52) and the prop_type list"""
    c = dict(cfg or {})
    n_sub = int((1.0 / float(c.get('control_freq', 50.0))) / (1.0 / float(c.get('sim_freq', 500.0))))
    return dict(kp=float(c.get('kp', 50.0)), kd=float(c.get('kd', 0.5)), max_tau=float(c.get('max_tau', 18.0)), n_sub=n_sub,
                prop_type=list(c.get('prop_type', PMC_PROP_TYPE)))


def prop_layout(prop_type):
    """observation columns by kind for a prop_type list (PLE:101-121: prop = 3 stacked frames of the keys in list order | prop_a 36 | future 72):
    -> (prop_dim, configuration-like columns of the newest frame and every column of prop_a and future, velocity columns of the newest frame)"""
    pd = sum(capi.PROP_SIZES[k] for k in prop_type)
    conf, vel, off = [], [], 2 * pd
    for k in prop_type:
        (conf if k in ('joint_pos', 'e_g') else vel).extend(range(off, off + capi.PROP_SIZES[k]))
        off += capi.PROP_SIZES[k]
    return pd, np.array(conf + list(range(3 * pd, 3 * pd + 108)), dtype=int), np.array(vel, dtype=int)


def quat_align(a, ref):
    """flip the sign of quaternion rows of `a` to match `ref` (q and -q are the same rotation)."""
    a = a.copy()
    s = np.sign(np.sum(a[..., 3:7] * ref[..., 3:7], axis=-1, keepdims=True))
    s[s == 0] = 1
    a[..., 3:7] *= s
    return a


def check_reset_against_goldens(golden, model_blob, table, lib_path, cfg=None):
    """PLE:150-171 / ML:48-57 at explicit (clip, t0): first obs + ghost state vs the imported reference.
    cfg: the env_config the golden file was generated under (None: the training scripts' point); `table` is loaded at its 1 / control_freq."""
    n = len(golden['g2_seed'])
    E = make_engine(model_blob, table, n, lib_path, **(cfg or {}))
    E.reset(clip=golden['g2_clip'], t0=golden['g2_t0'])
    np.testing.assert_allclose(E.obs(), golden['g2_obs'], rtol=NONPHYS_TOL, atol=NONPHYS_TOL)
    kin = quat_align(E.ref_state().astype(np.float64), golden['g2_kin'])
    np.testing.assert_allclose(kin, golden['g2_kin'], rtol=NONPHYS_TOL, atol=2e-5)
    np.testing.assert_array_equal(E.state(), E.ref_state())
    info = E.episode_info()
    np.testing.assert_array_equal(info['clip'], golden['g2_clip'])
    np.testing.assert_array_equal(info['time'], golden['g2_t0'])          # float64, bit exact
    assert (info['steps'] == 0).all()
    # partial reset leaves the other envs untouched
    before = E.obs()
    E.reset(env_ids=[3, 5], clip=[golden['g2_clip'][0]] * 2, t0=[golden['g2_t0'][0]] * 2)
    after = E.obs()
    np.testing.assert_allclose(after[3], golden['g2_obs'][0], rtol=NONPHYS_TOL, atol=NONPHYS_TOL)
    np.testing.assert_array_equal(after[5], after[3])
    mask = np.ones(n, bool); mask[[3, 5]] = False
    np.testing.assert_array_equal(after[mask], before[mask])
    E.close()


def oracle_self_deviation(B1, pre, act, kp=50.0, kd=0.5, max_tau=18.0, n_sub=10):
    """How far the ORACLE's own result of one control step (n_sub substeps -- ten at 50 Hz -- from state `pre` under the PD target of `act`) moves when its state is
    perturbed at float32 resolution: rounded to float32 between substeps, and started from joint angles one float32 ulp up / down.  A step in
    which a contact makes or breaks, or sticks or slips, on the strength of the last bit amplifies such perturbations by orders of magnitude;
    no float32 implementation can then be closer to the float64 oracle than the oracle is to itself.  Returns (configuration, relative velocity)."""
    def ten(s0, r32=False):
        s = np.array(s0, dtype=np.float64)
        tgt = np.clip(s[13:25] + np.asarray(act, np.float64), -3.0, 3.0)
        for _ in range(n_sub):
            tau = np.clip(kp * (tgt - s[13:25]) - kd * s[25:37], -max_tau, max_tau)
            s = B1.substep(s, tau)[0]
            if r32:
                s = s.astype(np.float32).astype(np.float64)
        return s
    base = ten(pre)
    cc = cv = 0.0
    up, dn = np.array(pre, dtype=np.float64), np.array(pre, dtype=np.float64)
    up[13:25] = np.nextafter(up[13:25].astype(np.float32), np.float32(np.inf)).astype(np.float64)
    dn[13:25] = np.nextafter(dn[13:25].astype(np.float32), np.float32(-np.inf)).astype(np.float64)
    for o in (ten(pre, r32=True), ten(up), ten(dn)):
        e = np.abs(quat_align(o, base) - base)
        cc = max(cc, e[0:7].max(), e[13:25].max())
        cv = max(cv, max(e[7:13].max(), e[25:37].max()) / (1.0 + np.abs(base[25:37]).max()))
    return cc, cv, base


def run_lockstep(golden, orc, model_blob, table, lib_path, n_envs, n_steps, seed, resync=True, sigma=SIGMA, policy=None, total_envs=None, spec=None, cfg=None):
    """Step engine and oracle side by side from golden (clip, t0) starts with the same random actions.
    With resync the oracle is re-seeded with the engine's float32 state after every control step, so every step
    is an independent single-control-step comparison.
    total_envs: the engine runs that many envs (the larger-batch kernel builds start above 4096) and the oracle follows n_envs of
    them, spread over the first, middle and last wavefronts of the grid.
    cfg: env_config fields (the keys of capi.make_config) applied to BOTH the engine and the oracle; `table` is then loaded at 1 / control_freq."""
    rng = np.random.default_rng(seed)
    kw = dict(cfg or {})
    N = total_envs or n_envs
    if total_envs:
        third = n_envs // 3
        idx = np.concatenate([np.arange(third), N // 2 - 7 + np.arange(third), N - (n_envs - 2 * third) + np.arange(n_envs - 2 * third)])
    else:
        idx = np.arange(n_envs)
    pick = rng.integers(0, len(golden['g2_clip']), N)
    clip, t0 = golden['g2_clip'][pick], golden['g2_t0'][pick]
    E = make_engine(model_blob, table, N, lib_path, **kw)
    B = make_oracle_batch(orc, model_blob, table, n_envs=n_envs, **kw)
    if spec:                                 # a spec switch that exists in both implementations (include/llenv_model.h LLM_SPEC_*)
        E.set_spec(**spec)
        orc.reset_spec(); orc.set_spec(**spec)
    E.reset(clip=clip, t0=t0)
    es0 = E.state()
    for i in range(n_envs):
        B.reset_env(i, int(clip[idx[i]]), float(t0[idx[i]]))
        B.set_state(i, es0[idx[i]].astype(np.float64))
    B2 = make_oracle_batch(orc, model_blob, table, n_envs=1, **kw)      # scratch env for the selection-tie re-runs below
    stats = dict(config=[], vel=[], obs=[], obs_vel=[], reward=[], feet=[], done_mismatch=0, done=0, on_tie=0, ill=[])
    pd_ = config_scalars(cfg)                                           # (None: make_engine / make_oracle_batch defaults, the PMC config of SURVEY 8)
    pdim, obs_conf, obs_vel = prop_layout(pd_.pop('prop_type'))
    prev_obs = None
    alive = np.ones(n_envs, bool)
    for t in range(n_steps):
        if policy is None:
            act = (rng.normal(size=(N, 12)) * sigma).astype(np.float32)
        else:                                # the trained policy's mean action on the engine's own observation: the tracking-gait regime
            act = policy.act(E.obs().astype(np.float64)).astype(np.float32)
        E.step_host(act)
        eo, (er, ed, ew), es, ek = E.obs(), E.reward_done(), E.state(), E.ref_state()
        efd, efk = E.feet()
        for i in range(n_envs):
            if not alive[i]:
                continue
            e = idx[i]
            pre = B.get_state(i)
            orc.OracleBatch.selection_margin()
            oo, orr, od = B.step_env(i, act[e].astype(np.float64))
            sel = orc.OracleBatch.selection_margin()
            os_ = B.get_state(i)
            err = np.abs(quat_align(es[e].astype(np.float64), os_) - os_)
            vscale = 1.0 + np.abs(os_[25:37]).max()
            if sel < TIE_ZONE and max(err[0:7].max(), err[13:25].max(), err[7:13].max() / vscale, err[25:37].max() / vscale) > PHYS_STEP_TOL:
                # A contact point's depth or a capsule pair's distance came within float32 resolution of (deepest + LLM_SELECT_EPS), where the
                # deepest-K pick changes hands: float32 and float64 may legitimately keep different rows.  The engine must then
                # agree with the oracle for SOME tie tolerance within +-2 TIE_ZONE of the nominal one; such samples are counted and capped.
                stats['on_tie'] += 1
                adopted = False
                for d in (-2.0 * TIE_ZONE, 2.0 * TIE_ZONE):
                    orc.reset_spec(); orc.set_spec(select_eps=capi.LL_SELECT_EPS + d, **(spec or {}))
                    B2.reset_env(0, int(clip[e]), float(t0[e])); B2.set_state(0, pre); B2.step_env(0, act[e].astype(np.float64))
                    orc.reset_spec(); orc.set_spec(**(spec or {}))
                    o2 = B2.get_state(0)
                    e2 = np.abs(quat_align(es[e].astype(np.float64), o2) - o2)
                    if e2[25:37].max() < err[25:37].max():
                        err, os_, vscale, adopted = e2, o2, 1.0 + np.abs(o2[25:37]).max(), True
            else:
                adopted = False
            ce, ve = max(err[0:7].max(), err[13:25].max()), max(err[7:13].max(), err[25:37].max()) / vscale
            if resync and (ce > PHYS_STEP_TOL or ve > 10 * PHYS_STEP_TOL):
                # outside the bars: is the step ill-conditioned in the oracle itself?  (counted, printed, capped by the callers)
                cc, cv, base = oracle_self_deviation(B2, pre, act[e], **pd_)
                assert np.abs(quat_align(base, os_) - os_).max() < 1e-9 or adopted, 'oracle_self_deviation does not restate step_env'
                stats['ill'].append((ce, ve, cc, cv))
            stats['config'].append(max(err[0:7].max(), err[13:25].max()))
            stats['vel'].append(max(err[7:13].max(), err[25:37].max()) / vscale)
            if adopted:                      # the engine's row choice was the other legitimate one: its observation follows its own state
                oo = eo[e].astype(np.float64)
            oe = np.abs(eo[e] - oo)
            # newest prop frame, the keys in prop_type order (PMC_PROP_TYPE: joint_pos 66:78 | joint_vel 78:90 | ang_vel_loc | lin_vel_loc 90:96 | e_g 96:99)
            stats['obs'].append(oe[obs_conf].max())                                                # configuration-like entries, prop_a and future
            stats['obs_vel'].append(oe[obs_vel].max() / vscale if len(obs_vel) else 0.0)           # velocity entries
            if prev_obs is not None:                                                               # deque shift, bit exact
                assert np.array_equal(eo[e][0:2 * pdim], prev_obs[e][pdim:3 * pdim])
                assert np.array_equal(eo[e][3 * pdim:3 * pdim + 24], prev_obs[e][3 * pdim + 12:3 * pdim + 36])
            if not adopted:
                stats['reward'].append(abs(er[e] - orr))
                ofd, ofk = B.get_feet(i)
                stats['feet'].append(max(np.abs(efd[e] - ofd).max(), np.abs(efk[e] - ofk).max()))
            if bool(ed[e]) != od:
                stats['done_mismatch'] += 1
            if od or ed[e]:
                stats['done'] += 1
                alive[i] = False             # reference semantics: a finished env waits for reset()
            elif resync:
                B.set_state(i, es[e].astype(np.float64))
        prev_obs = eo
    E.close()
    if spec:
        orc.reset_spec()
    return {k: (np.array(v) if isinstance(v, list) else v) for k, v in stats.items()}


ILL_FACTOR = 4.0


def bars_with_conditioning(st, label, vel_hi=10 * PHYS_STEP_TOL):
    """EVERY sample: configuration within 1e-4, velocity within 1e-3 of (1 + the env's largest joint rate) -- unless the step is ill-conditioned
    in the ORACLE itself (oracle_self_deviation: contact make / break or stick / slip decided by the last float32 bit; about 1 step in 3000 under
    random actions, both model blobs): such a sample must stay within ILL_FACTOR x the oracle's own deviation.  They are counted, printed and
    capped so that the allowance cannot absorb a regression."""
    c, v = np.asarray(st['config']).reshape(-1), np.asarray(st['vel']).reshape(-1)
    ill = st['ill']
    cap = max(2, len(c) // 1000)
    print('%s: %d samples, %d outside the plain bars and ill-conditioned in the oracle itself (cap %d), %d on a selection tie; worst config %.2e, velocity %.2e'
          % (label, len(c), len(ill), cap, st['on_tie'], c.max(), v.max()))
    assert (c > PHYS_STEP_TOL).sum() + (v > vel_hi).sum() <= 2 * len(ill), 'samples outside the bars that were never examined'
    assert len(ill) <= cap, ill
    for (ce, ve, cc, cv) in ill:
        assert ce <= max(PHYS_STEP_TOL, ILL_FACTOR * cc) and ve <= max(vel_hi, ILL_FACTOR * cv), (label, 'engine error', ce, ve, 'oracle self-deviation', cc, cv)


def check_single_step_parity(golden, orc, model_blob, table, lib_path, n_envs=32, n_steps=12, seed=7, total_envs=None, spec=None, cfg=None):
    st = run_lockstep(golden, orc, model_blob, table, lib_path, n_envs, n_steps, seed, resync=True, total_envs=total_envs, spec=spec, cfg=cfg)
    assert len(st['config']) > n_envs * n_steps * 0.5
    assert st['on_tie'] <= max(2, len(st['config']) // 500), st['on_tie']          # samples on the selection rule's discontinuity: counted, capped (observed: 0 - 1 per run)
    # EVERY sample: configuration within 1e-4, velocities within 1e-3 of (1 + the env's largest joint rate); and at most 1 % of the env-steps
    # above 1e-4 in velocity (float32 rounding through a contact that switches on or off inside the step; 0.4 % measured)
    bars_with_conditioning(st, 'single control step')
    v = np.asarray(st['vel']).reshape(-1)
    assert (v > PHYS_STEP_TOL).sum() <= max(1, len(v) // 100), np.percentile(v, [50, 90, 99, 100])
    ok = np.ones(len(v), bool)                                      # observation, reward and feet follow the state: same samples set aside
    ok[[i for i in range(len(v)) if st['config'][i] > PHYS_STEP_TOL or v[i] > 10 * PHYS_STEP_TOL]] = False
    assert st['obs'][ok].max() < PHYS_STEP_TOL, np.percentile(st['obs'], [50, 90, 99, 100])
    ov = np.asarray(st['obs_vel']).reshape(-1)
    assert (ov > PHYS_STEP_TOL).sum() <= max(1, len(ov) // 100), np.percentile(ov, [50, 90, 99, 100])
    assert st['obs_vel'][ok].max() < 10 * PHYS_STEP_TOL
    assert np.sort(st['reward'])[:len(st['reward']) - len(st['ill'])].max() < PHYS_STEP_TOL
    assert np.sort(st['feet'])[:len(st['feet']) - len(st['ill'])].max() < PHYS_STEP_TOL
    assert st['done_mismatch'] <= max(1, st['done'] // 10)
    return st


def check_policy_driven_parity(golden, orc, model_blob, table, lib_path, n_envs=32, n_steps=40, seed=5):
    """The same single-control-step comparison in the regime the env is built for: actions of the reference's trained policy (walking,
    running, jumping gaits: feet make and break contact, little else touches), 40 steps per env, oracle re-synchronised after every step."""
    from conftest import POLICY_WEIGHTS
    from oracle.pmc_policy import PmcPolicy
    st = run_lockstep(golden, orc, model_blob, table, lib_path, n_envs, n_steps, seed, resync=True, policy=PmcPolicy(POLICY_WEIGHTS))
    assert len(st['config']) > n_envs * n_steps * 0.7                                # the policy keeps most episodes alive
    print('policy-driven parity: %d samples, %d on a selection tie (cap %d)' % (len(st['config']), st['on_tie'], max(2, len(st['config']) // 500)))
    assert st['on_tie'] <= max(2, len(st['config']) // 500), st['on_tie']
    bars_with_conditioning(st, 'policy-driven parity')
    v = np.asarray(st['vel']).reshape(-1)
    # every sample within 1e-3 relative (bars_with_conditioning); a gait's joint rates are a few rad/s, so the same absolute error weighs more
    # against (1 + max rate) than in the flailing runs: up to 5 % of the samples may exceed 1e-4 (measured: 4.0 % on the CPU build, p99 = 1.6e-4)
    assert (v > PHYS_STEP_TOL).sum() <= max(1, 5 * len(v) // 100), np.percentile(v, [50, 90, 99, 100])
    assert np.sort(st['reward'])[:len(st['reward']) - len(st['ill'])].max() < PHYS_STEP_TOL and np.sort(st['feet'])[:len(st['feet']) - len(st['ill'])].max() < PHYS_STEP_TOL
    assert st['done_mismatch'] <= max(1, st['done'] // 10)
    return st


def check_rollout_statistics(golden, orc, model_blob, table, lib_path, n_envs=256, max_steps=160, seed=11, threads=None):
    """Free-running episodes (no resync) of engine and oracle from the same starts with the same action streams.  Contact dynamics are
    chaotic, so trajectories diverge sample-wise within a few steps; what must agree are the DISTRIBUTIONS: episode length
    (two-sample Kolmogorov-Smirnov), mean reward per step, and how episodes end."""
    from scipy import stats as sst
    if threads is None:                                       # the oracle's envs are independent of each other: the thread count changes the wall time only
        import bench
        threads = max(1, min(16, bench.effective_cores()[0]))
    rng = np.random.default_rng(seed)
    clip = rng.integers(0, table.n_clips, n_envs).astype(np.int32)
    dur = table.frame_step * (np.asarray(table.clip_len)[clip] - table.margin - 1)
    t0 = rng.uniform(0.0, 0.6, n_envs) * dur
    E = make_engine(model_blob, table, n_envs, lib_path)
    B = make_oracle_batch(orc, model_blob, table, n_envs=n_envs)
    E.reset(clip=clip, t0=t0)
    for i in range(n_envs):
        B.reset_env(i, int(clip[i]), float(t0[i]))
    out = {}
    alive = {k: np.ones(n_envs, bool) for k in 'eo'}
    length = {k: np.full(n_envs, max_steps) for k in 'eo'}
    rsum = {k: np.zeros(n_envs) for k in 'eo'}
    why = {k: np.zeros(n_envs, int) for k in 'eo'}
    for t in range(max_steps):
        act = (rng.normal(size=(n_envs, 12)) * SIGMA).astype(np.float32)
        E.step_host(act)
        er, ed, ew = E.reward_done()
        _, orr, od = B.step_all_mt(act.astype(np.float64), threads)
        od = np.asarray(od).astype(bool)
        oinfo = None
        for k, r, d in (('e', er, np.asarray(ed).astype(bool)), ('o', orr, od)):
            rsum[k] += np.where(alive[k], r, 0.0)
            new = alive[k] & d
            length[k][new] = t + 1
            if k == 'e':
                why[k][new] = np.asarray(ew)[new]
            else:
                for i in np.where(new)[0]:
                    why[k][i] = B.episode_info(int(i))['done_reason']
            alive[k] &= ~d
        if not alive['e'].any() and not alive['o'].any():
            break
    E.close()
    le, lo = length['e'], length['o']
    ks = sst.ks_2samp(le, lo)
    me, mo = rsum['e'].sum() / le.sum(), rsum['o'].sum() / lo.sum()
    fall = {k: float(((why[k] & capi.DONE_FALL) != 0).mean()) for k in 'eo'}
    out = dict(mean_len=(float(le.mean()), float(lo.mean())), ks_p=float(ks.pvalue), reward=(float(me), float(mo)), fall=fall,
               first_steps_equal=float((le == lo).mean()))
    # bars at what is measured (MI355X, 512 envs: 98 % of the episodes end at the very same step, mean length 58.96 vs 59.09, reward 0.1359 vs
    # 0.1357, falls 7.6 % vs 7.6 %; CPU emulation, 64 envs: 100 %) with room for one in ten episodes to drift -- not at what chaos would allow
    assert out['first_steps_equal'] >= 0.9, out
    assert ks.pvalue > 0.5, out
    assert abs(le.mean() - lo.mean()) < 0.03 * lo.mean(), out
    assert abs(me - mo) < 0.003, out
    assert abs(fall['e'] - fall['o']) < 0.03, out
    return out


def check_contact_rich_parity(golden, orc, model_blob, table, lib_path, n_envs=16, seed=3):
    """Collapsed / rolled-over robots: every lane overflows its contact slots (deepest-K selection), joints sit on their
    limits.  One control step from identical hand-made states, engine vs oracle."""
    from scipy.spatial.transform import Rotation as R
    rng = np.random.default_rng(seed)
    clip, t0 = golden['g2_clip'][:n_envs], golden['g2_t0'][:n_envs]
    E = make_engine(model_blob, table, n_envs, lib_path)
    B = make_oracle_batch(orc, model_blob, table, n_envs=n_envs)
    E.reset(clip=clip, t0=t0)
    st = E.state().astype(np.float64)
    for i in range(n_envs):
        st[i, 2] = rng.uniform(0.05, 0.12)                                        # belly on (or in) the ground
        st[i, 3:7] = (R.from_quat(st[i, 3:7]) * R.from_euler('xyz', [rng.uniform(-1.4, 1.4) if i % 2 else 0.0, rng.uniform(-0.3, 0.3), 0])).as_quat()
        st[i, 7:13] = rng.normal(size=6) * 0.3
        st[i, 13:25] = np.tile([0.0, -1.4, 2.5], 4) + rng.normal(size=12) * 0.15   # folded legs, shanks at their upper limit
        st[i, 25:37] = rng.normal(size=12)
    E.set_state(st)
    st32 = E.state().astype(np.float64)
    out = dict(config=[], vel=[])
    act = (rng.normal(size=(n_envs, 12)) * SIGMA).astype(np.float32)
    for i in range(n_envs):
        B.reset_env(i, int(clip[i]), float(t0[i]))
        B.set_state(i, st32[i])
    E.step_host(act)
    es = E.state().astype(np.float64)
    for i in range(n_envs):
        B.step_env(i, act[i].astype(np.float64))
        os_ = B.get_state(i)
        err = np.abs(quat_align(es[i], os_) - os_)
        out['config'].append(max(err[0:7].max(), err[13:25].max()))
        out['vel'].append(max(err[7:13].max(), err[25:37].max()) / (1.0 + np.abs(os_[25:37]).max()))
    E.close()
    out = {k: np.array(v) for k, v in out.items()}
    assert np.isfinite(es).all()
    # a penetrating start makes a stiff, many-contact solve; every sample still within the bars of free motion (measured: 1e-6 / 1.3e-5)
    assert out['config'].max() < 1e-4, out['config']
    assert out['vel'].max() < 1e-3, out['vel']
    return out


def check_trained_policy_tracks(lib_path, n_envs=16, n_steps=200, seed=7):
    """SURVEY.md 8f-3, the strongest available check on the UNPINNED physics: the reference's PMC policy
    (data/models/primitive_level.model, trained against PyBullet; weights extracted by tools/extract_policy.py into
    lifelike_agility_and_play_amd/assets/pmc_policy.npz) drives our simulator closed-loop.  If our contact/articulated dynamics were not
    Bullet-like the policy would fall within a second; instead it tracks walk / run / jump / idle clips to the end."""
    import os
    import lifelike_agility_and_play_amd as lla
    from conftest import GOLDEN_DIR, POLICY_WEIGHTS
    from oracle.pmc_policy import PmcPolicy
    pol = PmcPolicy(POLICY_WEIGHTS)
    env = lla.create_tracking_game(arena_id='LeggedRobotTracking', data_path='', control_freq=50.0, prop_type=list(PMC_PROP_TYPE),
                                   prioritized_sample_factor=3.0, kp=50.0, kd=0.5, max_tau=18, reward_weights=dict(PMC_REWARD_WEIGHTS),
                                   num_envs=n_envs, seed=seed, auto_reset=False, lib_path=lib_path)
    obs = env.reset()
    alive = np.ones(n_envs, bool)
    steps, rsum, why = np.zeros(n_envs, int), np.zeros(n_envs), np.zeros(n_envs, int)
    for t in range(n_steps):
        obs, r, d, info = env.step(pol.act(obs.astype(np.float64)))
        rsum += np.where(alive, r, 0.0)
        steps += alive
        newly = alive & d
        why[newly] = info['done_reason'][newly]
        alive &= ~d
        if not alive.any():
            break
    env.close()
    ok = alive | (why == capi.DONE_CLIP_END)              # still tracking at the horizon, or reached the end of the clip
    mean_r = rsum.sum() / steps.sum()
    assert ok.mean() >= 0.75, (ok, why)
    assert mean_r > 0.7, mean_r
    return dict(mean_reward=mean_r, tracked=ok.mean(), steps=steps, why=why)


def check_trajectory_ring(model_blob, table, lib_path, read_ring, write_dev=None, cfg=None):
    """ll_enable_unrolls: every step writes its transition into time step (s mod unroll) of block ((s div unroll) mod 2) of the
    env's unroll -- X in the learner's flatten order (future | prop | prop_a), A, neglogp, R, V, r, 1 - done -- and ll_finish_unroll
    fills R with the TD(lambda) returns.  read_ring(address, shape) -> numpy copy (host memory for the emulation library, device
    memory on a GPU); write_dev(address, array) -> stores float32 values at a device address (policy outputs), or None."""
    import os
    from conftest import GOLDEN_DIR
    from lifelike_agility_and_play_amd import gather
    n, unroll = 24, 4
    E = make_engine(model_blob, table, n, lib_path, auto_reset=1, seed=5, **(cfg or {}))
    E.reset()
    ptr, w = E.enable_unrolls(unroll, 2)
    od = E.obs_dim
    assert w == od + 17
    p_nl, p_v = E.pg_ptrs()
    rng = np.random.default_rng(0)
    prev_obs = E.obs()
    hist = []
    for t in range(11):
        act = (rng.normal(size=(n, 12)) * 0.5).astype(np.float32)
        nl, v = rng.uniform(5, 15, n).astype(np.float32), rng.uniform(0, 10, n).astype(np.float32)
        if write_dev is not None:
            E.sync(); write_dev(p_nl, nl); write_dev(p_v, v)
        else:
            nl[:] = 0; v[:] = 0
        E.step_host(act)
        r, d, _ = E.reward_done()
        E.sync()
        ring = read_ring(ptr, (2, n, unroll, w))
        row = ring[(t // unroll) % 2][:, t % unroll]
        f = gather.split_row(row, od)
        np.testing.assert_array_equal(f['X'][:, :72], prev_obs[:, od - 72:])            # future first (dict keys sorted)
        np.testing.assert_array_equal(f['X'][:, 72:], prev_obs[:, :od - 72])            # then prop | prop_a: the observation the action was chosen on
        np.testing.assert_array_equal(f['A'], act)
        np.testing.assert_array_equal(f['neglogp'], nl); np.testing.assert_array_equal(f['V'], v)
        np.testing.assert_array_equal(f['r'], r)
        np.testing.assert_array_equal(f['mask'], 1.0 - d.astype(np.float32))
        hist.append((prev_obs.copy(), act, r.copy(), d.copy(), v.copy()))
        prev_obs = E.obs()
        if t % unroll == unroll - 1:
            # one env's unroll is contiguous and starts, per time step, with the reference's flattened [X_t, A_t] (distill_actor.py:159-162)
            blk = ring[(t // unroll) % 2]
            for e in (0, n - 1):
                steps = hist[-unroll:]
                obs_d = [dict(prop=h[0][e, :od - 108], prop_a=h[0][e, od - 108:od - 72], future=h[0][e, od - 72:]) for h in steps]
                ref = gather.flatten_unroll(obs_d, [h[1][e] for h in steps]).reshape(unroll, od + 12)
                np.testing.assert_array_equal(blk[e][:, :od + 12], ref.astype(np.float32))
            # TD(lambda) returns against a NumPy statement of the recursion
            gamma, lam = 0.95, 0.9
            boot = rng.uniform(0, 10, n).astype(np.float32)
            if write_dev is not None:
                write_dev(p_v, boot)
            else:
                boot[:] = 0
            E.finish_unroll((t // unroll) % 2, gamma, lam)
            E.sync()
            blk = read_ring(ptr, (2, n, unroll, w))[(t // unroll) % 2]
            f = gather.split_row(blk, od)
            adv, vnext, R = np.zeros(n), boot.astype(np.float64), np.zeros((n, unroll))
            for k in range(unroll - 1, -1, -1):
                delta = f['r'][:, k] + gamma * vnext * f['mask'][:, k] - f['V'][:, k]
                adv = delta + gamma * lam * f['mask'][:, k] * adv
                R[:, k] = adv + f['V'][:, k]
                vnext = f['V'][:, k].astype(np.float64)
            np.testing.assert_allclose(f['R'], R, rtol=1e-5, atol=1e-5)
    # the stale-bootstrap guard: once the caller has declared the pg buffers current (ll_pg_mark_current, what act_pg does), a NULL bootstrap
    # is only accepted while that stamp is the current step -- right after a step the value buffer still holds V(obs_{T-1})
    E.pg_mark_current()
    E.finish_unroll(0, 0.95, 0.9)                                            # stamped for this very observation: accepted
    E.step_host(np.zeros((n, 12), np.float32))
    try:
        E.finish_unroll(0, 0.95, 0.9)
        raise AssertionError('a stale value buffer was accepted as the bootstrap')
    except capi.LLError as e:
        assert e.code == capi.LL_ESTATE, e
    E.finish_unroll(0, 0.95, 0.9, d_bootstrap_value=p_v)                     # an explicit bootstrap pointer is always accepted
    E.pg_mark_current()
    E.finish_unroll(0, 0.95, 0.9)
    E.sync()
    E.close()
    # the flatten itself is the reference's: golden generated by running distill_actor._push_data_to_learner
    g = np.load(os.path.join(GOLDEN_DIR, 'unroll_golden.npz'))
    T = int(g['unroll_length'])
    for k in range(len(g['unroll_np'])):
        sl = slice(k * T, (k + 1) * T)
        obs_d = [dict(prop=p, prop_a=a, future=f) for p, a, f in zip(g['obs_prop'][sl], g['obs_prop_a'][sl], g['obs_future'][sl])]
        np.testing.assert_array_equal(gather.flatten_unroll(obs_d, g['action'][sl]), g['unroll_np'][k])
    assert list(g['shapes']) == [72, 99, 36, 12]


def check_multi_step_launch(model_blob, table, lib_path, read_ring, sizes=(24,), k=7, n_launches=5, spec=None, obstacle=False, cfg=None):
    """ll_step_random_n(sigma, k) == k x ll_step_random(sigma), bit for bit -- state, ghost, observation, reward, done reasons, bookkeeping,
    counters, episode histogram, the recorded actions, every row of the unroll buffers and the sampling table -- with uniform sampling and
    auto-reset, with prioritized sampling without auto-reset, and (round 5) WITH BOTH: the table is folded after every control step of a launch
    into a version of its own, and an episode that re-seeds at step s draws from the version steps 0 .. s - 1 left (PLE:235-240 as k launches keep
    it).  The last leg is the one with power: a table that starts at avg_reward 0.9 everywhere, where one finished episode changes what everybody after it draws.
    obstacle: the same with set_obstacle (the jump obstacle's builds)."""
    unroll = 4
    okw = dict(set_obstacle=True, obstacle_height=0.2) if obstacle else {}
    okw.update(cfg or {})                                            # env_config fields of every engine of the check
    for n in sizes:
        for kw in (dict(auto_reset=1, prioritized_sample_factor=0.0), dict(auto_reset=0, prioritized_sample_factor=3.0),
                   dict(auto_reset=1, prioritized_sample_factor=3.0), dict(auto_reset=1, prioritized_sample_factor=3.0 + 1e-9)):
            A = make_engine(model_blob, table, n, lib_path, seed=31, **kw, **okw)
            B = make_engine(model_blob, table, n, lib_path, seed=31, **kw, **okw)
            if spec:                                                 # (a kernel option with its own builds: LLM_SPEC_FRICTION_MODE = 2)
                A.set_spec(**spec); B.set_spec(**spec)
            A.reset(); B.reset()
            sig = SIGMA
            if kw['prioritized_sample_factor'] > 3.0:
                # the leg with power: every clip starts at avg_reward 0.9 (p ~ 1e-3 each), so the first episode that ends makes ITS clip a thousand
                # times likelier than the rest -- whoever re-seeds after it, and from which table, shows at once; wild actions end episodes fast
                A.set_sampling_table(np.full(table.n_clips, 0.9)); B.set_sampling_table(np.full(table.n_clips, 0.9))
                sig = 0.7
            for _ in range(3):                                       # unrolls start wherever they are enabled (not at step 0)
                A.step_random(sig); B.step_random(sig)
            pa, w = A.enable_unrolls(unroll, 2); pb, _ = B.enable_unrolls(unroll, 2)
            assert A.unroll_position() == (0, 0)
            for L in range(n_launches):
                for _ in range(k):
                    A.step_random(sig)
                B.step_random_n(sig, k)
                A.sync(); B.sync()
                assert A.unroll_position() == B.unroll_position() == divmod((L + 1) * k, unroll)
                for x, y in ((A.state(), B.state()), (A.ref_state(), B.ref_state()), (A.obs(), B.obs()), (A.feet()[0], B.feet()[0])):
                    np.testing.assert_array_equal(x, y)
                ra, rb = A.reward_done(), B.reward_done()
                np.testing.assert_array_equal(ra[0], rb[0]); np.testing.assert_array_equal(ra[2], rb[2])
                ia, ib = A.episode_info(), B.episode_info()
                for key in ia:
                    np.testing.assert_array_equal(ia[key], ib[key])
                assert A.counters() == B.counters()
                np.testing.assert_array_equal(A.episode_histogram(), B.episode_histogram())
                np.testing.assert_array_equal(read_ring(pa, (2, n, unroll, w)), read_ring(pb, (2, n, unroll, w)))
                for x, y in zip(A.sampling_table(), B.sampling_table()):
                    np.testing.assert_array_equal(x, y)
            assert A.counters()['episodes'] > 0
            if hasattr(B, 'table_sync'):
                assert B.table_sync() == 0                          # no episode re-seeded from an older version than the exact one
            A.close(); B.close()
        # longer launches, both on: same number of env-steps, everything finite, episodes keep ending and re-seeding
        C = make_engine(model_blob, table, n, lib_path, seed=32, auto_reset=1, prioritized_sample_factor=3.0, **okw)
        if spec:
            C.set_spec(**spec)
        C.reset()
        for _ in range(n_launches):
            C.step_random_n(SIGMA, 4 * k)
        c = C.counters()
        assert c['env_steps'] == n * n_launches * 4 * k and c['episodes'] > 0 and c['nonfinite'] == 0
        p, avg, _ = C.sampling_table()
        assert np.isfinite(C.state()).all() and abs(p.sum() - 1.0) < 1e-9 and (avg != 0).any()
        with np.testing.assert_raises(capi.LLError):
            C.step_random_n(SIGMA, 0)
        C.close()


def check_obstacle_variant(golden, orc, model_blob, table, lib_path, n_envs=24, n_steps=60, seed=2, total_envs=None, spec=None, cap_ill=0, pct=100, cfg=None):
    """set_obstacle=True (PLE:173-193, :262-268, :341-346): engine vs oracle on the jump clips, random policy.  The robot does
    not clear the box, so episodes must end with the COLLISION bit in both, at the same step.
    total_envs: the engine runs that many envs (above 4096: the larger-batch build of the obstacle kernel) and the oracle follows n_envs of them,
    spread over the first, middle and last wavefronts of the grid.
    spec: switches set on BOTH sides for the run (tests/spec_matrix.py).
    cap_ill: samples outside the bars that are ill-conditioned in the oracle itself (oracle_self_deviation, as bars_with_conditioning) allowed.
    pct: 98 for friction_dirs = 1, the rule's documented bars (test_kernel_logic_emul.py::test_sliding_direction_friction_variant)."""
    cnt, tab = table.obstacles()
    clips = np.where(cnt > 0)[0]
    assert len(clips) == 20 and cnt.sum() == 78                          # SURVEY a21 [probe]
    rng = np.random.default_rng(seed)
    clip = rng.choice(clips, n_envs)
    off = np.concatenate([[0], np.cumsum(cnt)])
    # start shortly before a jump peak: the robot inherits the mocap velocity and flies into the box
    t0 = np.array([max(0.0, tab[off[c] + rng.integers(0, cnt[c]), 3] - 0.2) for c in clip])
    t0 = np.minimum(t0, [table.frame_step * (table.clip_len[c] - table.margin - 2) for c in clip])
    kw = dict(set_obstacle=True, obstacle_height=0.2, **(cfg or {}))         # cfg: env_config fields on BOTH sides; `table` loaded at 1 / control_freq
    N = total_envs or n_envs
    third = n_envs // 3
    idx = np.arange(n_envs) if not total_envs else np.concatenate([np.arange(third), N // 2 - 7 + np.arange(third), N - (n_envs - 2 * third) + np.arange(n_envs - 2 * third)])
    reps = (N + n_envs - 1) // n_envs
    clip_all, t0_all = np.tile(clip, reps)[:N], np.tile(t0, reps)[:N]
    clip_all[idx], t0_all[idx] = clip, t0
    E = make_engine(model_blob, table, N, lib_path, **kw)
    B = make_oracle_batch(orc, model_blob, table, n_envs=n_envs, **kw)
    if spec:
        E.set_spec(**spec)
        orc.reset_spec(); orc.set_spec(**spec)
    try:
        return _run_obstacle_variant(E, B, rng, clip, t0, clip_all, t0_all, idx, n_envs, n_steps, orc, model_blob, table, cap_ill, pct, cfg)
    finally:
        if spec:
            orc.reset_spec()


def _run_obstacle_variant(E, B, rng, clip, t0, clip_all, t0_all, idx, n_envs, n_steps, orc, model_blob, table, cap_ill, pct, cfg=None):
    N = E.n_envs
    pd_ = config_scalars(cfg); pd_.pop('prop_type')
    B2 = make_oracle_batch(orc, model_blob, table, n_envs=1, **(cfg or {}))   # the oracle's own deviation (oracle_self_deviation) of a sample outside the bars
    ill = []
    E.reset(clip=clip_all, t0=t0_all)
    es0 = E.state()
    for i in range(n_envs):
        B.reset_env(i, int(clip[i]), float(t0[i]))
        B.set_state(i, es0[idx[i]].astype(np.float64))
    alive = np.ones(n_envs, bool)
    n_coll = mism = 0
    cfg_err, vel_err = [], []
    for t in range(n_steps):
        act_all = (rng.normal(size=(N, 12)) * SIGMA).astype(np.float32)
        E.step_host(act_all)
        r, d, why = (x[idx] for x in E.reward_done())
        es = E.state()[idx]
        act = act_all[idx]
        for i in range(n_envs):
            if not alive[i]:
                continue
            pre = B.get_state(i)
            _, _, od = B.step_env(i, act[i].astype(np.float64))
            oreason = B.episode_info(i)['done_reason']
            # the box is a collision body during the substeps (PLE:182-193): the states after a step that touched it agree too
            os_ = B.get_state(i)
            err = np.abs(quat_align(es[i].astype(np.float64), os_) - os_)
            ce, ve = max(err[0:7].max(), err[13:25].max()), max(err[7:13].max(), err[25:37].max()) / (1.0 + np.abs(os_[25:37]).max())
            if cap_ill and (ce >= 1e-4 or ve >= 1e-3):
                # outside the bars: is the step ill-conditioned in the oracle itself?  Only a step the box took no part in is restated by
                # oracle_self_deviation (the plain batch): one it did take part in stays held to the bars.
                cc, cv, base = oracle_self_deviation(B2, pre, act[i], **pd_)
                if np.abs(quat_align(base, os_) - os_).max() < 1e-9:
                    ill.append((ce, ve, cc, cv))
                    assert ce <= max(1e-4, ILL_FACTOR * cc) and ve <= max(1e-3, ILL_FACTOR * cv), ('engine error', ce, ve, 'oracle self-deviation', cc, cv)
                    ce, ve = 0.0, 0.0
            cfg_err.append(ce)
            vel_err.append(ve)
            if bool(d[i]) != od or (od and (int(why[i]) & 8) != (oreason & 8)):
                mism += 1
            if od or d[i]:
                alive[i] = False
                n_coll += int((oreason & 8) != 0)
            else:
                B.set_state(i, es[i].astype(np.float64))
    E.close()
    assert n_coll >= 3, n_coll
    assert mism <= 1, mism
    assert len(ill) <= cap_ill, ill
    if ill:
        print('obstacle variant: %d sample(s) outside the plain bars, ill-conditioned in the oracle itself: %s' % (len(ill), ill))
    if pct < 100:
        assert np.percentile(cfg_err, pct) < 1e-4 and np.percentile(vel_err, pct) < 1e-3 and max(cfg_err) < 2e-2, (np.percentile(cfg_err, [pct, 100]), np.percentile(vel_err, [pct, 100]))
        return n_coll
    assert max(cfg_err) < 1e-4 and max(vel_err) < 1e-3, (max(cfg_err), max(vel_err))
    return n_coll


def check_reset_onto_a_mocap_discontinuity(orc, model_blob, table, lib_path):
    """The retargeted clips hold IK branch flips between two consecutive frames (clip 27 at 7.07 s, clip 8 at 18.90 s: a hind leg's three joints jump by
    1 - 6 rad): the reference's finite-difference joint velocity (ML:48-63) is 600 - 750 rad/s there, and a uniformly random start lands on such a frame
    once in 2 - 4e7 env-steps.  Every non-finite reset of round 4's soak runs was one of these (tools/diag_nonfinite.py).  With Bullet's velocity clip
    (LLM_MAX_COORD_VEL = btMultiBody::m_maxCoordinateVelocity = 100) engine and oracle come through finite, and agree; without it both blow up
    (the float32 engine to inf -> LL_DONE_NONFINITE, the float64 oracle to 1e30)."""
    cases = [(27, 7.068370648298843), (8, 18.901122098221997), (27, 7.066725201181503)]
    E = make_engine(model_blob, table, len(cases), lib_path)
    B = make_oracle_batch(orc, model_blob, table, n_envs=len(cases))
    clip, t0 = np.array([c for c, _ in cases]), np.array([t for _, t in cases])
    E.reset(clip=clip, t0=t0)
    s0 = E.state()
    assert (np.abs(s0[:, 25:37]).max(1) > 500.0).all(), np.abs(s0[:, 25:37]).max(1)          # the reference's own reset state (G-goldens pin the formula)
    for i, (c, t) in enumerate(cases):
        B.reset_env(i, c, t); B.set_state(i, s0[i].astype(np.float64))
    act = np.zeros((len(cases), 12), np.float32)
    E.step_host(act)
    r, d, why = E.reward_done()
    es = E.state().astype(np.float64)
    assert np.isfinite(es).all() and not (why & capi.LL_DONE_NONFINITE).any(), why
    assert np.abs(es[:, 25:37]).max() <= 100.0 + 1e-3
    worst = 0.0
    for i in range(len(cases)):
        _, _, od = B.step_env(i, act[i].astype(np.float64))
        os_ = B.get_state(i)
        err = np.abs(quat_align(es[i], os_) - os_)
        worst = max(worst, err[0:7].max(), err[13:25].max())
        assert err[0:7].max() < PHYS_STEP_TOL and err[13:25].max() < PHYS_STEP_TOL, (i, err[0:7].max(), err[13:25].max())     # (a violent step -- joint rates at the clip, limit rows deep in penetration -- and still within the standing bars: 1.5e-6)
        assert bool(d[i]) == od, (i, d[i], od)
    E.set_spec(max_coord_vel=1e30)                                   # the switch that turns the clip off: nothing bounds the joint rates any more
    E.reset(clip=clip, t0=t0)
    E.step_host(act)
    # (rounds 1 - 4: the float32 engine then overflowed -> LL_DONE_NONFINITE.  Under round 5's limit rule -- no speculative rows fighting a 700 rad/s joint -- it
    # may come through finite; what the clip is for still shows: rates beyond Bullet's m_maxCoordinateVelocity somewhere in the step's outcome, or the guard)
    # (round 6, advisor: a bare `done.any()` was accepted here too, which a clip end or a fall satisfies.  With auto-reset off the step's outcome stays in the state, so the
    #  rates themselves are looked at; an env the step finished keeps its terminal state as well)
    why2 = E.reward_done()[2]
    assert (why2 & capi.LL_DONE_NONFINITE).any() or np.abs(E.state()[:, 25:37]).max() > 100.0 + 1e-3, (why2, np.abs(E.state()[:, 25:37]).max())
    E.close()
    return worst


def check_deep_penetration_against_oracle(orc, model_blob, table, lib_path, spec, depths=(0.005, 0.03, 0.045, 0.08)):
    """Robots set INTO the ground (feet 5 ... 80 mm below the plane: shallow, around and beyond Bullet's -0.04 threshold) and stepped once, engine against
    oracle under the same penetration-recovery switches (LLM_SPEC_ERP, _ERP_DEEP, _MAX_DEPEN_SPEED): the push-out speed is where those switches act, and
    the deep branch is not met by the random-action parity runs.  Returns the base's upward speeds after the step, per depth."""
    n = len(depths)
    E = make_engine(model_blob, table, n, lib_path, auto_reset=0)
    E.set_spec(**spec)
    orc.reset_spec(); orc.set_spec(**spec)
    try:
        B = make_oracle_batch(orc, model_blob, table, n_envs=n)
        clip, t0 = np.zeros(n, np.int32), np.full(n, 0.3)
        E.reset(clip=clip, t0=t0)
        s0 = E.state().astype(np.float64)
        foot_z = np.array([np.asarray(B.fk_feet(s0[i])).reshape(4, 3)[:, 2].min() for i in range(n)]) - 0.025        # lowest point of the foot spheres (URDF:158)
        for i, d in enumerate(depths):
            s0[i, 2] -= foot_z[i] + d                                   # lowest foot sphere d below the plane
            s0[i, 7:13] = 0.0; s0[i, 25:37] = 0.0                       # at rest: what moves it afterwards is the push-out (and gravity)
        E.set_state(s0.astype(np.float32))
        s0 = E.state().astype(np.float64)
        for i in range(n):
            B.reset_env(i, 0, 0.3); B.set_state(i, s0[i])
        act = np.zeros((n, 12), np.float32)
        E.step_host(act)
        es = E.state().astype(np.float64)
        up = []
        for i in range(n):
            B.step_env(i, act[i].astype(np.float64))
            os_ = B.get_state(i)
            err = np.abs(quat_align(es[i], os_) - os_)
            assert err[0:7].max() < PHYS_STEP_TOL and err[13:25].max() < PHYS_STEP_TOL, (spec, depths[i], err[0:7].max(), err[13:25].max())
            assert err[7:13].max() < 1e-3 * (1 + np.abs(os_[25:37]).max()), (spec, depths[i], err[7:13].max())
            up.append(os_[2] - s0[i, 2])
        return np.array(up)
    finally:
        orc.reset_spec()
        E.close()


def check_scripted_episodes_against_goldens(golden, model_blob, table, lib_path, cfg=None, min_done=6):
    """The engine's whole step() control flow against the REFERENCE's own outputs (golden G5): 12 scripted episodes driven
    exactly as gen_golden.py drove the reference through its fake BulletClient -- physics result and foot positions
    supplied, everything else (time keeping with the Q2 phase lag, mocap lookup, history stacking with raw actions,
    5-term reward, the termination tests, PLE:235-240 table update) computed by the kernel."""
    n_ep = len(golden['g5_seed'])
    E = make_engine(model_blob, table, 1, lib_path, **(cfg or {}))
    n_done = 0
    for e in range(n_ep):
        E.reset(clip=[int(golden['g5_clip'][e])], t0=[float(golden['g5_t0'][e])])
        np.testing.assert_allclose(E.obs()[0], golden['g5_reset_obs'][e], rtol=NONPHYS_TOL, atol=NONPHYS_TOL)
        for t in range(int(golden['g5_n'][e])):
            feet = np.stack([golden['g5_feet_dyn'][e, t], golden['g5_feet_kin'][e, t]])
            E.step_scripted(golden['g5_actions'][e, t][None], golden['g5_dyn'][e, t][None], feet[None])
            obs = E.obs()[0]
            r, d, why = E.reward_done()
            g = golden['g5_obs'][e, t]
            # joint rates in the scripted states reach ~50 rad/s: float32 storage alone is 4e-6 there
            np.testing.assert_allclose(obs, g, rtol=2e-6, atol=NONPHYS_TOL, err_msg='episode %d step %d' % (e, t))
            assert abs(float(r[0]) - golden['g5_reward'][e, t]) < NONPHYS_TOL
            assert bool(d[0]) == bool(golden['g5_done'][e, t]), (e, t, why)
        n_done += bool(d[0])
        prob, avg_r, avg_len = E.sampling_table()
        np.testing.assert_allclose(prob, golden['g5_prob_after'][e], rtol=1e-5, atol=1e-8)       # PLE:239-240
        np.testing.assert_allclose(avg_len, golden['g5_avg_len_after'][e], rtol=1e-6, atol=1e-9)  # PLE:237
    E.close()
    assert n_done >= min_done


def check_auto_reset_equals_manual_reset(model_blob, table, lib_path, n_envs=24, n_steps=40, cfg=None):
    """An env that finishes under auto_reset=1 is re-seeded INSIDE the step kernel (the merged tail of step_env); the same
    episode driven with auto_reset=0 and an explicit ll_reset at the engine-chosen (clip, t0) must give the same
    observation, state, ghost, feet and bookkeeping.  With keep_terminal_obs the finished episode's last observation must be
    the one the non-resetting engine reports."""
    # the host build runs one instruction stream for both engines (exact); on the GPU the in-kernel re-seed and ll_reset are
    # different kernels, whose fused multiply-adds the compiler may contract differently (a few ulp)
    def same(x, y):
        if lib_path is not None:
            np.testing.assert_array_equal(x, y)
        else:
            np.testing.assert_allclose(x, y, rtol=2e-6, atol=2e-6)
    A = make_engine(model_blob, table, n_envs, lib_path, auto_reset=1, seed=21, keep_terminal_obs=True, **(cfg or {}))
    B = make_engine(model_blob, table, n_envs, lib_path, auto_reset=0, seed=21, **(cfg or {}))
    A.reset(); B.reset()
    assert np.array_equal(A.obs(), B.obs())
    rng = np.random.default_rng(5)
    n_reset = 0
    for t in range(n_steps):
        a = (rng.normal(size=(n_envs, 12)) * 0.6).astype(np.float32)      # wild enough to end episodes quickly
        A.step_host(a); B.step_host(a)
        ra, da, wa = A.reward_done()
        rb, db, wb = B.reward_done()
        assert np.array_equal(da, db) and np.array_equal(wa, wb) and np.array_equal(ra, rb)
        if da.any():
            ids = np.where(da)[0]
            same(A.terminal_obs()[ids], B.obs()[ids])        # PLE:227 of the finished episode
            info = A.episode_info()
            B.reset(env_ids=ids, clip=info['clip'][ids], t0=info['time'][ids])        # what A did by itself
            if lib_path is None:
                same(A.state(), B.state())
                B.set_state(A.state())       # keep ulp differences of the two reset kernels from growing through the physics
            n_reset += len(ids)
        same(A.obs(), B.obs())
        same(A.state(), B.state())
        same(A.ref_state(), B.ref_state())
        fa, fb = A.feet(), B.feet()
        same(fa[0], fb[0]); same(fa[1], fb[1])
        ia, ib = A.episode_info(), B.episode_info()
        for k in ('clip', 'time', 'steps', 'reward_sum'):
            same(ia[k], ib[k])
    C = make_engine(model_blob, table, 4, lib_path, auto_reset=1, **(cfg or {}))
    C.reset()
    try:
        C.terminal_obs()
        raise AssertionError('terminal_obs must be refused when keep_terminal_obs is off')
    except capi.LLError:
        pass
    A.close(); B.close(); C.close()
    assert n_reset >= 5
    return n_reset


def check_engine_against_host_build(model_blob, table, emul_lib, n_envs=4096, steps=10, seed=17, gpu_lib=None, report_only=False, sigma=0.4):
    """The net under the PMC step kernels at BASELINE config 2's size: every entry of every observation, reward, done flag and reason, ghost state, feet and episode record the HIP kernel writes, env by env against
    the HOST build of the very same kernel source (tests/emul) -- the envs that finish and RE-SEED inside the step included (actions wild enough to end a few hundred episodes within the run: the rare path on which round 4's chase-tag build lost a
    register to a misplaced copy, HISTORY.md; `profiles/r05_sepmc_seven_ray_root_cause.txt`).  Same config, seed and actions; before every step the host build takes the engine's state, so physics rounding stays one
    step old; bars: 2e-2 on observation entries of envs whose state agrees to 5e-3, 2e-4 on the observations of RE-SEEDED envs (no physics in between).  Envs whose own state differs by more than 5e-3 after the step (a contact step conditioned on the last bit between two float32 builds) are counted, capped at 1 % and left to the physics parity tests;
    envs whose done flag or re-seed draw differs are counted and capped likewise."""
    G = make_engine(model_blob, table, n_envs, gpu_lib, auto_reset=1, seed=seed)
    H = make_engine(model_blob, table, n_envs, emul_lib, auto_reset=1, seed=seed)
    G.reset(); H.reset()
    out = dict(reseeded=0, left_out=0, rough=0, worst_obs=0.0, worst_reseeded_obs=0.0, worst_reward=0.0)
    vel = np.zeros(33, bool); vel[12:30] = True
    obs_vel = np.concatenate([np.zeros(72, bool), np.tile(vel, 3), np.zeros(36, bool)])              # future 72 | prop 3 x 33 (joint rates, base twist: relative) | prop_a 36

    recent = []

    def compare(label, keep, reseeded=None):
        og, oh = G.obs().astype(np.float64), H.obs().astype(np.float64)
        assert np.isfinite(og).all(), label
        sg, sh = G.state().astype(np.float64), H.state().astype(np.float64)
        scale = 1.0 + np.maximum(np.abs(sh[:, 7:13]).max(-1, keepdims=True), np.abs(sh[:, 25:37]).max(-1, keepdims=True))
        ds = np.abs(sg - sh); ds[:, 7:13] /= scale; ds[:, 25:37] /= scale            # (base twist and joint rates relative to the fastest of them)
        rough = ds.max(-1) > 5e-3
        do = np.abs(og - oh) / np.where(obs_vel, scale, 1.0)
        out['rough'] += int((keep & rough).sum())
        recent.append(rough)
        rough = np.logical_or.reduce(recent[-3:])                  # (the observation carries the two older proprioceptive frames: an env stays set aside while a rough step is among them)
        ok = keep & ~rough
        if ok.any():
            out['worst_obs'] = max(out['worst_obs'], float(do[ok].max()))
        bad = ok & (do.max(-1) > 2e-2)              # (orientation-derived entries amplify a state difference of 5e-3 a few times; a wrong register is an O(0.1 .. 1) error)
        res = dict(envs_with_an_observation_entry_off=int(bad.sum()))
        gg, gh = G.ref_state().astype(np.float64), H.ref_state().astype(np.float64)
        res['ghost_off'] = int((ok & (np.abs(gg - gh).max(-1) > 1e-3)).sum())
        if reseeded is not None and (ok & reseeded).any():
            # a re-seeded env starts from its clip's frame: no physics in between, so the two builds must agree far below the contact tolerance
            m = ok & reseeded
            out['worst_reseeded_obs'] = max(out['worst_reseeded_obs'], float(do[m].max()))
            res['reseeded_envs_off'] = int((do[m].max(-1) > 2e-4).sum())
            res['reseeded_state_off'] = int((ds[m].max(-1) > 2e-5).sum())
        out.setdefault('per_step', {})[label] = res
        if not report_only:
            assert sum(res.values()) == 0, (label, res, np.flatnonzero(bad)[:8], do[bad].argmax(-1)[:8] if bad.any() else None)
            assert (keep & rough).mean() < 0.02, (label, (keep & rough).mean())

    compare('reset', np.ones(n_envs, bool), np.ones(n_envs, bool))
    ig, ih = G.episode_info(), H.episode_info()
    assert np.array_equal(ig['clip'], ih['clip']) and np.allclose(ig['time'], ih['time'], atol=1e-9)
    rng = np.random.default_rng(seed)
    for t in range(steps):
        act = (rng.normal(size=(n_envs, 12)) * sigma).astype(np.float32)
        H.set_state(G.state())
        G.step_host(act); H.step_host(act)
        (rg, dg, wg), (rh, dh, wh) = G.reward_done(), H.reward_done()
        ig, ih = G.episode_info(), H.episode_info()
        same = (dg == dh) & (wg == wh) & (ig['clip'] == ih['clip']) & (np.abs(ig['time'] - ih['time']) < 1e-9) & (ig['steps'] == ih['steps'])
        out['left_out'] += int((~same).sum())
        out['reseeded'] += int((dg & same).sum())
        compare('step %d' % t, same, dg & same)
        sg, sh = G.state(), H.state()
        calm = same & (np.abs(sg - sh).max(-1) < 5e-3)
        out['worst_reward'] = max(out['worst_reward'], float(np.abs(rg - rh)[calm].max()))
        if not report_only:
            assert np.abs(rg - rh)[calm].max() < 5e-3, (t, np.abs(rg - rh)[calm].max())
        pg, ph = G.sampling_table()[0], H.sampling_table()[0]
        out['table'] = float(np.abs(pg - ph).max())
        if not report_only:
            assert out['table'] < 1e-6, out
    if not report_only:
        assert out['left_out'] <= max(2, int(0.01 * n_envs * steps)), out
        assert out['reseeded'] >= n_envs // 64, out                               # the in-kernel re-seed was exercised
    G.close(); H.close()
    return out


def check_self_collision_parity(golden, orc, model_blob, table, lib_path, n_envs=16, seed=5, spec=None, cfg=None):
    """Legs driven into one another in mid-air (same-side front/hind pairs, left/right pairs, diagonal): one control step,
    engine vs oracle -- same capsule spec, different formulations -- and the oracle WITHOUT self-collision as the control: the
    legs must have been stopped, not passed through each other (LR:212-217 URDF_USE_SELF_COLLISION).
    `spec`: switches set on BOTH sides for the run (round 6: self_friction = 0.25, Bullet's 0.5 x 0.5 -- the leg-leg contact then carries two tangential rows behind its
    normal row; the returned `moved` is how far the friction moved the oracle's own answer, so that a caller can see the switch had something to act on)."""
    import ctypes as C
    from oracle import oracle as orc_mod
    rng = np.random.default_rng(seed)
    clip, t0 = golden['g2_clip'][:n_envs], golden['g2_t0'][:n_envs]
    kw = dict(cfg or {})                                      # env_config fields on BOTH sides
    E = make_engine(model_blob, table, n_envs, lib_path, **kw)
    if spec:
        E.set_spec(**spec)
    B = make_oracle_batch(orc, model_blob, table, n_envs=n_envs, **kw)
    B0 = make_oracle_batch(orc, model_blob, table, n_envs=n_envs, **kw)
    E.reset(clip=clip, t0=t0)
    st = E.state().astype(np.float64)
    act = np.zeros((n_envs, 12), np.float32)
    for i in range(n_envs):
        st[i, 0:3] = [0, 0, 0.7]; st[i, 3:7] = [0, 0, 0, 1]; st[i, 7:13] = rng.normal(size=6) * 0.2
        q = np.tile([0.0, -0.8, 1.6], 4) + rng.normal(size=12) * 0.05
        qd = rng.normal(size=12) * 0.5
        kind = i % 4
        if kind in (0, 1):                                   # same side: front thigh back, hind thigh forward (right, then left)
            f, h = (0, 2) if kind == 0 else (1, 3)
            q[3 * f + 1], q[3 * f + 2] = -1.0 + rng.uniform(-0.05, 0.1), 0.2
            q[3 * h + 1], q[3 * h + 2] = 1.0 + rng.uniform(-0.1, 0.05), 0.2
            qd[3 * f + 1], qd[3 * h + 1] = -3.0, 3.0
            act[i, 3 * f + 1], act[i, 3 * h + 1] = -0.6, 0.6
        elif kind == 2:                                      # left / right: hips rolled towards each other, legs straight down
            q[0], q[3] = 0.65 + rng.uniform(-0.05, 0.05), -0.6 + rng.uniform(-0.05, 0.05)     # (asymmetric: no tied capsule pairs)
            q[1], q[2], q[4], q[5] = -0.3, 0.6, -0.45, 0.9
            qd[0], qd[3] = 2.0, -2.0
            act[i, 0], act[i, 3] = 0.4, -0.4
        else:                                                # hind pair likewise
            q[6], q[9] = 0.6 + rng.uniform(-0.05, 0.05), -0.65 + rng.uniform(-0.05, 0.05)
            q[7], q[8], q[10], q[11] = -0.45, 0.9, -0.3, 0.6
            qd[6], qd[9] = 2.0, -2.0
            act[i, 6], act[i, 9] = 0.4, -0.4
        st[i, 13:25], st[i, 25:37] = q, qd
    E.set_state(st)
    st32 = E.state().astype(np.float64)
    lib = orc_mod.lib()
    for i in range(n_envs):
        for bb in (B, B0):
            bb.reset_env(i, int(clip[i]), float(t0[i]))
            bb.set_state(i, st32[i])
    E.step_host(act)
    es = E.state().astype(np.float64)
    cfg_err, vel_err, stopped, moved = [], [], 0, 0.0
    orc.reset_spec()
    for i in range(n_envs):
        if spec:
            plain = make_oracle_batch(orc, model_blob, table, n_envs=1, **kw)           # the spec's own answer (without the switches), for `moved`
            plain.reset_env(0, int(clip[i]), float(t0[i])); plain.set_state(0, st32[i])
            plain.step_env(0, act[i].astype(np.float64))
            orc.set_spec(**spec)
        lib.orc_set_self_collision(C.c_int(1))
        B.step_env(i, act[i].astype(np.float64))
        lib.orc_set_self_collision(C.c_int(0))
        B0.step_env(i, act[i].astype(np.float64))
        lib.orc_set_self_collision(C.c_int(1))
        if spec:
            orc.reset_spec()
            moved = max(moved, np.abs(B.get_state(i)[25:37] - plain.get_state(0)[25:37]).max())
        o1, o0 = B.get_state(i), B0.get_state(i)
        err = np.abs(quat_align(es[i], o1) - o1)
        cfg_err.append(max(err[0:7].max(), err[13:25].max()))
        vel_err.append(max(err[7:13].max(), err[25:37].max()) / (1.0 + np.abs(o1[25:37]).max()))
        if np.abs(o1[13:25] - o0[13:25]).max() > 0.02:
            stopped += 1                                      # the legs were held apart by more than a degree
    E.close()
    cfg_err, vel_err = np.array(cfg_err), np.array(vel_err)
    assert stopped >= n_envs // 2, stopped
    assert cfg_err.max() < 1e-4, cfg_err              # every sample (measured: 8e-7 / 2.5e-5 -- since the closest-point routine takes the pair's
    assert vel_err.max() < 1e-3, vel_err              # segments in the spec's order (A first) in both implementations and is regularised for parallel axes)
    return dict(config=cfg_err, vel=vel_err, stopped=stopped, moved=moved)


def check_nonfinite_guard(model_blob, table, lib_path):
    """A NaN / Inf that reaches an env's state ("NaN guard + counter") ends that episode with LL_DONE_NONFINITE, counts once
    per env, zeroes its reward, re-seeds it -- and leaves every other env, including the three that share its wavefront, bit-for-bit
    what they are in a twin engine that was never poisoned."""
    n = 8                                                   # two wavefronts of four envs
    A = make_engine(model_blob, table, n, lib_path, auto_reset=1, seed=9)
    B = make_engine(model_blob, table, n, lib_path, auto_reset=1, seed=9)
    A.reset(); B.reset()
    rng = np.random.default_rng(1)
    for t in range(3):
        a = (rng.normal(size=(n, 12)) * SIGMA).astype(np.float32)
        A.step_host(a); B.step_host(a)
    assert np.array_equal(A.state(), B.state()) and A.counters()['nonfinite'] == 0
    s = A.state()
    s[2, 13 + 4] = np.nan                                   # a joint angle of env 2 (wave 0)
    s[5, 7] = np.inf                                        # a base velocity of env 5 (wave 1): the velocity clip (LLM_MAX_COORD_VEL) must not turn it into a bound
    s[7, 25 + 3] = np.nan                                   # a joint RATE of env 7: the velocity clip must not turn a NaN into a bound
    A.set_state(s)
    a = (rng.normal(size=(n, 12)) * SIGMA).astype(np.float32)
    ep0 = A.counters()['episodes']
    A.step_host(a); B.step_host(a)
    r, d, why = A.reward_done()
    rb, db, whyb = B.reward_done()
    bad, good = np.array([2, 5, 7]), np.array([0, 1, 3, 4, 6])
    assert d[bad].all() and ((why[bad] & capi.LL_DONE_NONFINITE) != 0).all() and (r[bad] == 0.0).all()
    c = A.counters()
    assert c['nonfinite'] == 3 and c['episodes'] - ep0 == 3 + int(db[good].sum())
    sa, oa = A.state(), A.obs()
    assert np.isfinite(sa).all() and np.isfinite(oa).all() and np.isfinite(A.ref_state()).all()      # re-seeded from the clip table
    info = A.episode_info()
    assert (info['steps'][bad] == 0).all() and (info['reward_sum'][bad] == 0.0).all()
    np.testing.assert_array_equal(sa[bad], A.ref_state()[bad])                                        # PLE:162-163
    assert np.array_equal(sa[good], B.state()[good]) and np.array_equal(oa[good], B.obs()[good])      # neighbours untouched
    assert np.array_equal(r[good], rb[good]) and np.array_equal(why[good], whyb[good])
    # the run goes on as if nothing had happened
    for t in range(3):
        A.step_random(SIGMA)
    assert np.isfinite(A.state()).all() and A.counters()['nonfinite'] == 3
    A.close(); B.close()
    # without auto-reset the env is flagged and stays the caller's to reset; the poison does not spread
    E = make_engine(model_blob, table, 4, lib_path, auto_reset=0, seed=2)
    E.reset()
    s = E.state(); s[1, 0] = np.nan; E.set_state(s)
    E.step_host(np.zeros((4, 12), np.float32))
    r, d, why = E.reward_done()
    assert d[1] and (why[1] & capi.LL_DONE_NONFINITE) and r[1] == 0.0 and E.counters()['nonfinite'] == 1
    assert np.isfinite(E.state()[[0, 2, 3]]).all() and np.isfinite(r).all()
    E.reset(env_ids=[1])
    E.step_host(np.zeros((4, 12), np.float32))
    assert np.isfinite(E.state()).all() and E.counters()['nonfinite'] == 1
    E.close()


def check_reset_argument_handling(model_blob, table, lib_path):
    """ll_reset's argument contract: an empty id list is a no-op, repeated ids and start times outside the reference's sampling range
    (ML:50-51) are rejected, start times need their clip."""
    E = make_engine(model_blob, table, 6, lib_path, auto_reset=0, seed=4)
    E.reset()
    before = (E.obs(), E.state(), E.episode_info())
    E.reset(env_ids=np.zeros(0, np.int32))                                   # `reset(env_ids=np.where(done)[0])` when nobody finished
    assert np.array_equal(E.obs(), before[0]) and np.array_equal(E.state(), before[1])
    for bad in (dict(env_ids=[1, 1]), dict(env_ids=[0, 3, 0]), dict(env_ids=[6]), dict(env_ids=[-1])):
        try:
            E.reset(**bad)
            raise AssertionError('accepted %r' % (bad,))
        except capi.LLError as e:
            assert e.code == capi.LL_EINVAL
    c = 7
    tmax = table.frame_step * (int(table.clip_len[c]) - table.margin - 1)     # ML:50
    E.reset(env_ids=[2], clip=[c], t0=[tmax])                                 # the last admissible start: futures stay inside the clip
    assert np.isfinite(E.obs()[2]).all()
    for bad in (dict(env_ids=[2], clip=[c], t0=[tmax + 1e-6]), dict(env_ids=[2], clip=[c], t0=[-1e-9]), dict(env_ids=[2], clip=[c], t0=[float('nan')]),
                dict(env_ids=[2], t0=[0.5]), dict(env_ids=[2], clip=[table.n_clips], t0=[0.0])):
        try:
            E.reset(**bad)
            raise AssertionError('accepted %r' % (bad,))
        except capi.LLError as e:
            assert e.code == capi.LL_EINVAL
    assert np.array_equal(E.state()[[0, 1, 3, 4, 5]], before[1][[0, 1, 3, 4, 5]])
    E.close()


def two_sample_bars(label, fracs, len_e, len_o, ks_p, n, floor_frac=0.03, floor_len=0.03, n_se=3.0, ks_floor=0.01):
    """Bars for outcome statistics of CHAOTIC episodes played by two simulators from the same seeds.  Where most episodes end at the same step on
    both sides the samples are paired and tight bars hold (end-reason fractions within 0.03, mean length within 3 %, KS p > 0.5: the PMC rollout
    test).  Where they decorrelate, engine and oracle are two independent samples of what is claimed to be ONE
    distribution, and the claim is tested as such: a fraction may differ by n_se standard errors of the difference of two binomial fractions
    (or floor_frac, whichever is larger), the mean length by n_se standard errors of the difference of two means (or floor_len of it), and the
    Kolmogorov-Smirnov test must not reject at ks_floor (its p-value is uniform on [0, 1] under the hypothesis: "p > 0.5" would fail every second
    run of a perfect engine).  fracs: {name: (engine, oracle)}."""
    import numpy as np
    for k, (a, b) in fracs.items():
        pbar = 0.5 * (a + b)
        se = np.sqrt(2.0 * pbar * (1.0 - pbar) / n)
        assert abs(a - b) <= max(floor_frac, n_se * se) + 1e-9, (label, k, a, b, 'allowed', max(floor_frac, n_se * se))
    le, lo = np.asarray(len_e, float), np.asarray(len_o, float)
    se = np.sqrt(le.var(ddof=1) / len(le) + lo.var(ddof=1) / len(lo))
    print('%s: mean length %.1f / %.1f, standard error of the difference %.1f (allowed %.1f); KS p %.3f' % (label, le.mean(), lo.mean(), se, max(floor_len * lo.mean(), n_se * se), ks_p))
    assert abs(le.mean() - lo.mean()) <= max(floor_len * lo.mean(), n_se * se), (label, le.mean(), lo.mean(), se)
    assert ks_p > ks_floor, (label, ks_p)
