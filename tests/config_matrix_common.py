"""The checks of the env_config matrix (tests/config_matrix.py), for any build of the engines: the host build of the kernel source
(test_config_matrix_emul.py) and the HIP library (test_gpu_config_matrix.py) run the same functions.  They reuse the standing comparators
(parity_common, epmc_parity_common, sepmc_parity_common) with their standing bars; nothing is restated here."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import config_matrix as cm
import spec_matrix_common as smc
from lifelike_agility_and_play_amd import capi

NONPHYS_TOL = 1e-5


def pmc_inputs(cfg):
    """model blob and the clip table loaded at the row's policy_step (ML:33-46: margin and max_steps follow it)"""
    from lifelike_agility_and_play_amd import mocap, urdf_model
    return urdf_model.default_model_blob(), mocap.load_mocap('', 1.0 / float(cfg.get('control_freq', 50.0)))


@contextlib.contextmanager
def arena_variant(cfg):
    import epmc_parity_common as ec
    with ec.cfg_variant(**cfg):
        yield


def make(engine, lib_path, cfg, n=None, seed=3, **kw):
    """a reset engine of the kind `engine` names under the env_config fields `cfg`: n envs (PMC, EPMC) / arenas (SEPMC)"""
    if engine in cm.PMC:
        import parity_common as pc
        blob, table = pmc_inputs(cfg)
        if engine == 'pmc_obst':
            kw.update(set_obstacle=True, obstacle_height=0.2)
        E = pc.make_engine(blob, table, n or 8, lib_path, seed=seed, **{**kw, **cfg})
    else:
        with arena_variant(cfg):
            if engine == 'epmc':
                import epmc_parity_common as ec
                E = ec.make_engine(ec.env_config(1), n or 4, lib_path, seed=seed, **kw)
            else:
                import sepmc_parity_common as sc
                E = sc.make_engine(sc.env_config((1, 0, 0)), n or 2, lib_path, seed=seed, **kw)
    E.reset()
    return E


# ---- parity ------------------------------------------------------------------------------------------------------------------------------------------

def check_parity(engine, name, lib_path, golden=None, orc=None, total=None, free_run=True):
    """engine vs oracle at row `name`, with the standing comparators and their standing bars.  total: the engine runs that many envs / arenas
    (the larger-batch builds) and the oracle follows the cases spread over its grid; the free-running legs run at their own small sizes only."""
    cfg = cm.cfg_of(name, engine)
    free_run = free_run and 'solver_iterations' not in cfg             # (the oracle envs of oracle/free_run.py take the env_config's keys; the iteration count is not one)
    if engine == 'pmc':
        import parity_common as pc
        blob, table = pmc_inputs(cfg)
        st = pc.check_single_step_parity(golden, orc, blob, table, lib_path, n_envs=16, n_steps=6, cfg=cfg, total_envs=total)
        print('%s %s: worst configuration error %.2e, relative velocity %.2e, reward %.2e, %d outside the plain bars' %
              (engine, name, np.max(st['config']), np.max(st['vel']), np.max(st['reward']), len(st['ill'])))
        return st
    if engine == 'pmc_obst':
        import parity_common as pc
        blob, table = pmc_inputs(cfg)
        # the same 0.8 s of flight into the box at every control_freq (40 steps at 50 Hz)
        n_steps = int(round(40 * float(cfg.get('control_freq', 50.0)) / 50.0))
        return pc.check_obstacle_variant(golden, orc, blob, table, lib_path, n_envs=12, n_steps=n_steps, total_envs=total, cfg=cfg, cap_ill=2)
    import epmc_parity_common as ec
    with arena_variant(cfg):
        if engine == 'epmc':
            out = ec.check_terrain_physics_against_oracle(lib_path, n_envs=16, seed=cm.seed_of(name, engine), total_envs=total)
            if free_run and total is None:
                print('%s %s free run:' % (engine, name), ec.check_free_running_against_oracle_env(lib_path))
            return out
        import sepmc_parity_common as sc
        out = sc.check_pair_physics_against_oracle(lib_path, n_arenas=12, seed=cm.seed_of(name, engine), total_arenas=total, cap_ill=2)
        if free_run and total is None:
            print('%s %s free run:' % (engine, name), sc.check_free_running_against_oracle_env(lib_path))
        return out


# ---- binding -----------------------------------------------------------------------------------------------------------------------------------------

def _frozen(x):
    return tuple(sorted((k, _frozen(v)) for k, v in x.items())) if isinstance(x, dict) else (tuple(x) if isinstance(x, list) else x)


def check_binding(engine, lib_path, n=8, k=25):
    """25 random-policy steps (the engines' own Philox draws, auto-reset on, uniform clip sampling so that no reward feeds back into the starts)
    at every row against the same run at the default point.  MOVES_STATE: the state differs.  SAME_STATE: everything a step moves is
    bit-identical except the row's output -- the observation is the exact column gather of the default run's, the reward differs from the
    default run's (check_reward holds it to the oracle).  A row that does not bind proves nothing and fails."""
    runs = {}
    base = dict(prioritized_sample_factor=0.0) if engine in cm.PMC else {}

    def run(cfg):
        key = _frozen(cfg)
        if key not in runs:
            E = make(engine, lib_path, {**base, **cfg}, n, auto_reset=1)
            smc.step(E, engine, k)
            runs[key] = smc.snapshot(E, engine)
            E.close()
        return runs[key]
    ref = run({})
    assert ref['counters']['episodes'] > 0, (engine, 'no episode ended and re-seeded inside the run')
    unbound, broken = [], []
    for name in cm.rows_of(engine):
        row, cfg = cm.ROWS[name], cm.cfg_of(name, engine)
        got = run(cfg)
        if row['kind'] == cm.MOVES_STATE:
            if np.array_equal(got['state'], ref['state']):
                unbound.append(name)
            if 'prop_type' in cfg:
                assert got['obs'].shape[-1] == ref['obs'].shape[-1] - 3 * (33 - cm.prop_dim_of(cfg['prop_type'])), (name, got['obs'].shape)
            continue
        out = row['output']
        moved = dict(obs=('obs',), reward=('rd0', 'ep_reward_sum'))[out]
        rest_a, rest_b = ({k_: v for k_, v in s.items() if k_ not in moved} for s in (got, ref))
        if not smc.same(rest_a, rest_b):
            broken.append((name, 'moved more than its output', [k_ for k_ in rest_a if not smc.same({k_: rest_a[k_]}, {k_: rest_b[k_]})]))
            continue
        if out == 'obs':
            cols = cm.gather_columns(cfg['prop_type'], ref['obs'].shape[-1] - 99)
            if got['obs'].shape[-1] != len(cols) or not np.array_equal(got['obs'], ref['obs'][..., cols]):
                broken.append((name, 'the observation is not the column gather of the default run\'s', got['obs'].shape))
            if got['obs'].shape == ref['obs'].shape and np.array_equal(got['obs'], ref['obs']):
                unbound.append(name)
        else:
            if np.array_equal(got['rd0'], ref['rd0']):
                unbound.append(name)
    assert not unbound, (engine, 'these rows do not bind in the run: they prove nothing', unbound)
    assert not broken, (engine, broken)


def check_reward(engine, name, lib_path, orc, n=16, k=4):
    """a reward_weights row: the reward of every step against the oracle's formula (PLE:352-425) under the row's weights, given the engine's own
    state, ghost and feet -- so the bar is the one of non-physics math"""
    cfg = cm.cfg_of(name, engine)
    w = [cfg['reward_weights'][key] for key in capi.RW_KEYS]
    E = make(engine, lib_path, cfg, n, auto_reset=0)
    rng = np.random.default_rng(2)
    alive, worst, n_seen = np.ones(n, bool), 0.0, 0
    for _ in range(k):
        E.step_host((rng.normal(size=(n, 12)) * 0.135).astype(np.float32))
        (r, d, why), s, g, (fd, fk) = E.reward_done(), E.state().astype(np.float64), E.ref_state().astype(np.float64), E.feet()
        for i in np.flatnonzero(alive):
            if why[i] & capi.LL_DONE_NONFINITE:
                continue
            worst = max(worst, abs(float(r[i]) - orc.reward(s[i], g[i], fd[i], fk[i], w)))
            n_seen += 1
        alive &= ~d
    E.close()
    print('%s %s: %d rewards against the oracle, worst %.2e' % (engine, name, n_seen, worst))
    assert n_seen >= n and worst < NONPHYS_TOL, (name, n_seen, worst)
    return worst


# ---- reset -------------------------------------------------------------------------------------------------------------------------------------------

def check_reset(name, lib_path, golden, orc, n=16):
    """PMC reset at golden (clip, t0) under the row: first observation and ghost against the oracle's reset_env; the sampling margin (ML:35: what
    bounds an admissible start) and max_steps (ML:45: what the sampling table divides an episode's length by) against the oracle's B.meta()."""
    import parity_common as pc
    from conftest import make_oracle_batch
    cfg = cm.cfg_of(name, 'pmc')
    blob, table = pmc_inputs(cfg)
    B = make_oracle_batch(orc, blob, table, n_envs=n, **cfg)
    margin, frame_rate, max_steps = B.meta()
    assert margin == table.margin == int(np.ceil((1.0 / float(cfg.get('control_freq', 50.0))) / table.frame_step)) + frame_rate + 2
    if float(cfg.get('control_freq', 50.0)) == 25.0:
        assert margin == 127, margin                                      # ML:35 at policy_step 0.04 (125 at 0.02)
    tmax = table.frame_step * (np.asarray(table.clip_len)[golden['g2_clip']] - margin - 1)
    ok = np.flatnonzero(golden['g2_t0'] <= tmax)[:n]
    assert len(ok) == n
    clip, t0 = golden['g2_clip'][ok], golden['g2_t0'][ok]
    E = pc.make_engine(blob, table, n, lib_path, auto_reset=0, **cfg)
    assert E.obs_dim == B.obs_dim == 3 * cm.prop_dim_of(cfg.get('prop_type', cm.DEFAULT_PROP)) + 108
    E.reset(clip=clip, t0=t0)
    obs_o = np.array([B.reset_env(i, int(clip[i]), float(t0[i])) for i in range(n)])
    np.testing.assert_allclose(E.obs(), obs_o, rtol=NONPHYS_TOL, atol=NONPHYS_TOL)
    kin_o = np.array([B.get_ref_state(i) for i in range(n)])
    np.testing.assert_allclose(pc.quat_align(E.ref_state().astype(np.float64), kin_o), kin_o, rtol=NONPHYS_TOL, atol=NONPHYS_TOL)
    np.testing.assert_array_equal(E.state(), E.ref_state())                # PLE:162-163
    # margin: the last admissible start of a clip is frame_step * (clip_len - margin - 1) (ML:50), and nothing beyond it
    for c in (0, 7, table.n_clips - 1):
        last = table.frame_step * (int(table.clip_len[c]) - margin - 1)
        E.reset(env_ids=[1], clip=[c], t0=[last])
        assert np.isfinite(E.obs()[1]).all()
        with pytest.raises(capi.LLError) as ei:
            E.reset(env_ids=[1], clip=[c], t0=[last + 1e-6])
        assert ei.value.code == capi.LL_EINVAL
        if margin > 1:                                                     # a start one frame earlier than the bound of a margin one smaller
            with pytest.raises(capi.LLError):
                E.reset(env_ids=[1], clip=[c], t0=[last + table.frame_step])
    # max_steps: an episode that ends after `steps` steps leaves steps / (max_steps + 1) in its clip's row of the table (PLE:237)
    E.reset(clip=clip, t0=t0)
    rng = np.random.default_rng(4)
    seen = {}
    for t in range(60):
        before = E.episode_info()
        E.step_host((rng.normal(size=(n, 12)) * 0.7).astype(np.float32))
        d = E.reward_done()[1]
        ended = np.flatnonzero(d & (before['steps'] == t))                 # (first end of the env: it was stepped t + 1 times)
        if len(ended):
            _, _, avg_len = E.sampling_table()
            e = ended.max()                                               # the highest env index wins when several finish the same clip in one step
            c = int(clip[e])
            if not any(int(clip[j]) == c for j in ended if j != e):
                seen[c] = (avg_len[c], (t + 1) / (max_steps[c] + 1.0))
        if d.all():
            break
    E.close()
    assert len(seen) >= 2, seen
    for c, (got, want) in seen.items():
        assert abs(got - want) <= 1e-6 * want, (name, c, got, want)
    return margin


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------------------------

def host_ring_access():
    """read_ring / write_dev of the host build: the unroll ring and the pg buffers are host memory"""
    def read_ring(addr, shape):
        n = int(np.prod(shape))
        return np.ctypeslib.as_array((C.c_float * n).from_address(addr)).reshape(shape).copy()

    def write_dev(addr, arr):
        np.ctypeslib.as_array((C.c_float * arr.size).from_address(addr))[:] = arr.ravel()
    return read_ring, write_dev


def check_batch_sizes(cfg, lib_path, read_ring, sizes=(1, 5, 67), k=7):
    """Batches that fill no wavefront and leave odd row bases (obs + env * obs_dim with obs_dim 117 or 153): k steps in one launch equal k
    launches bit for bit -- state, ghost, observation, terminal observation, reward, reasons, bookkeeping and every row of the unroll ring -- and
    an env's results do not depend on how many envs run beside it: the first envs of the largest batch equal the smaller batches."""
    import parity_common as pc
    blob, table = pmc_inputs(cfg)
    unroll, ref = 4, None
    for n in sorted(sizes, reverse=True):
        A = pc.make_engine(blob, table, n, lib_path, seed=31, auto_reset=1, keep_terminal_obs=True, **{'prioritized_sample_factor': 0.0, **cfg})
        B = pc.make_engine(blob, table, n, lib_path, seed=31, auto_reset=1, keep_terminal_obs=True, **{'prioritized_sample_factor': 0.0, **cfg})
        A.reset(); B.reset()
        pa, w = A.enable_unrolls(unroll, 2); pb, _ = B.enable_unrolls(unroll, 2)
        assert w == A.obs_dim + 17
        for _ in range(k):
            A.step_random(0.7)                                             # wild enough to end episodes inside the launch
        B.step_random_n(0.7, k)
        A.sync(); B.sync()
        snap = {}
        for label, E, p in (('a', A, pa), ('b', B, pb)):
            s = dict(state=E.state(), ghost=E.ref_state(), obs=E.obs(), term=E.terminal_obs(), ring=read_ring(p, (2, n, unroll, w)), feet=E.feet()[0])
            s['reward'], _, s['why'] = E.reward_done()
            s.update({'ep_' + k_: v for k_, v in E.episode_info().items()})
            snap[label] = s
        for key in snap['a']:
            np.testing.assert_array_equal(snap['a'][key], snap['b'][key], err_msg='%d envs, %s: one launch of %d steps against %d launches' % (n, key, k, k))
        assert np.isfinite(snap['a']['obs']).all()
        if ref is None:
            ref = snap['a']
            assert A.counters()['episodes'] > 0
        else:
            for key in ('state', 'ghost', 'obs', 'reward', 'why', 'ep_clip', 'ep_time', 'ep_steps'):
                np.testing.assert_array_equal(snap['a'][key], ref[key][:n], err_msg='%s of the first %d envs depends on the batch size' % (key, n))
            np.testing.assert_array_equal(snap['a']['ring'], ref['ring'][:, :n])
        A.close(); B.close()


def check_plumbing(name, lib_path, read_ring, write_dev=None, n_launches=2):
    """a combination row through the PMC engine's plumbing: the unroll ring at the row's obs_dim, multi-step launches against single ones,
    in-kernel re-seeding against ll_reset with keep_terminal_obs, and batches of 1, 5 and 67 envs"""
    import parity_common as pc
    cfg = cm.cfg_of(name, 'pmc')
    blob, table = pmc_inputs(cfg)
    pc.check_trajectory_ring(blob, table, lib_path, read_ring, write_dev, cfg=cfg)
    pc.check_multi_step_launch(blob, table, lib_path, read_ring, sizes=(24,), k=7, n_launches=n_launches, cfg=cfg)
    assert pc.check_auto_reset_equals_manual_reset(blob, table, lib_path, cfg=cfg) >= 5
    check_batch_sizes(cfg, lib_path, read_ring)


def check_arena_plumbing(engine, name, lib_path):
    """EPMC / SEPMC at a combination row: k control steps in one launch == k launches, bit for bit (their own standing checks)"""
    with arena_variant(cm.cfg_of(name, engine)):
        if engine == 'epmc':
            import epmc_parity_common as ec
            ec.check_multi_step_launch(lib_path, sizes=(12,), k=7, n_launches=2)
        else:
            import sepmc_parity_common as sc
            sc.check_multi_step_launch(lib_path, sizes=(6,), k=7, n_launches=2)


# ---- bad values --------------------------------------------------------------------------------------------------------------------------------------

def check_bad_values(engine, lib_path):
    """every BAD_VALUES entry of the engine is refused at create time with LL_EINVAL and a message naming the field; a good config still creates"""
    n_refused = 0
    for bad in cm.BAD_VALUES:
        if engine not in bad['engines']:
            continue
        cfg, poke = dict(bad.get('cfg', {})), bad.get('poke', {})
        with pytest.raises(capi.LLError) as ei:
            _create(engine, lib_path, cfg, poke)
        assert ei.value.code == capi.LL_EINVAL and bad['text'] in str(ei.value), (engine, bad['label'], str(ei.value))
        n_refused += 1
    _create(engine, lib_path, {}, {}).close()
    return n_refused


def _create(engine, lib_path, cfg, poke):
    from lifelike_agility_and_play_amd import urdf_model
    blob = urdf_model.default_model_blob()
    if engine in cm.PMC:
        import parity_common as pc
        from conftest import PMC_PROP_TYPE, PMC_REWARD_WEIGHTS
        _, table = pmc_inputs({})
        kw = dict(control_freq=50.0, kd=0.5, reward_weights=PMC_REWARD_WEIGHTS, prop_type=PMC_PROP_TYPE, set_obstacle=engine == 'pmc_obst', obstacle_height=0.2)
        kw.update(cfg)
        c = capi.make_config(4, **kw)
        for i, v in enumerate(poke.get('prop_order', ())):
            c.prop_order[i] = v
        return capi.Engine(c, blob, table, lib_path=lib_path)
    import epmc_parity_common as ec
    if engine == 'epmc':
        from lifelike_agility_and_play_amd import epmc_capi
        c = epmc_capi.make_epmc_config(4, {**ec.env_config(1), **cfg})
        for i, v in enumerate(poke.get('prop_order', ())):
            c.prop_order[i] = v
        return epmc_capi.EpmcEngine(c, blob, lib_path=lib_path)
    import sepmc_parity_common as sc
    from lifelike_agility_and_play_amd import sepmc_capi
    c = sepmc_capi.make_sepmc_config(2, {**sc.env_config((1, 0, 0)), **cfg})
    for i, v in enumerate(poke.get('prop_order', ())):
        c.prop_order[i] = v
    return sepmc_capi.SepmcEngine(c, blob, lib_path=lib_path)


# ---- the second reference golden and the public factories --------------------------------------------------------------------------------------------

def golden_cfg2_config(g):
    """the env_config tests/golden/pmc_golden_cfg2.npz was generated under (gen_golden.py CFG2: the factory's defaults, a permuted subset prop_type)"""
    return dict(control_freq=float(g['cfg_control_freq']), sim_freq=float(g['cfg_sim_freq']), kp=float(g['cfg_kp']), kd=float(g['cfg_kd']),
                max_tau=float(g['cfg_max_tau']), prioritized_sample_factor=float(g['cfg_prioritized_sample_factor']),
                prop_type=[str(k) for k in g['cfg_prop_type']], reward_weights=None)


def check_tracking_factory_defaults(lib_path, orc, n_steps=4, seeds=(0, 1, 2)):
    """create_tracking_game(arena_id, prop_type) with nothing else set -- 25 Hz, kd 1.0, PLE's reward weights -- against the oracle env made at the
    same defaults: observation shapes as _spaces() promises, then free running (no resync) under the free-run comparators' bars (state within
    1e-5 x 3^t, joints 5 x that; proprioception within 2e-3 + 500 tol, prop_a and future within 2e-3 + 20 tol; done flags equal)."""
    import lifelike_agility_and_play_amd as lla
    from lifelike_agility_and_play_amd import envs
    import parity_common as pc
    prop_type = ['e_g', 'joint_pos']
    env = lla.create_tracking_game(arena_id='LeggedRobotTracking', prop_type=list(prop_type), lib_path=lib_path)
    cfg = env._engine.cfg
    assert (cfg.control_freq, cfg.sim_freq, cfg.kp, cfg.kd, cfg.max_tau, cfg.solver_iterations) == (25.0, 500.0, 50.0, 1.0, 18.0, 10)
    space = envs._spaces(prop_type)[0]
    P = space.spaces['prop'].shape[0]
    assert P == 45 and env.observation_space.spaces[0].spaces['prop'].shape == (45,)
    blob, table = pmc_inputs(dict(control_freq=25.0))
    B = orc.OracleBatch(orc.make_config(n_envs=1, control_freq=25.0, kd=1.0, reward_weights=None, prop_type=prop_type, prioritized_sample_factor=0.0), blob, table)
    rng = np.random.default_rng(1)
    worst = 0.0
    for seed in seeds:
        np.random.seed(seed)
        (o,) = env.reset()
        for k, sp in space.spaces.items():
            assert o[k].shape == sp.shape, (k, o[k].shape, sp.shape)
        oo = B.reset_env(0, env.sampled_data_idx, env.time)
        B.set_state(0, env._engine.state()[0].astype(np.float64))
        np.testing.assert_allclose(np.concatenate(list(o.values())), oo, rtol=NONPHYS_TOL, atol=NONPHYS_TOL)
        for t in range(1, n_steps + 1):
            a = rng.normal(size=12) * 0.135
            (o,), (r,), d, _ = env.step([a])
            oo, orr, od = B.step_env(0, a.astype(np.float32).astype(np.float64))
            tol = 1e-5 * 3.0 ** t
            es, os_ = env._engine.state()[0].astype(np.float64), B.get_state(0)
            err = np.abs(pc.quat_align(es, os_) - os_)
            worst = max(worst, err[:7].max() / tol)
            assert err[:7].max() < tol and err[13:25].max() < 5 * tol, (seed, t, err[:7].max(), err[13:25].max())
            row = np.concatenate(list(o.values()))
            assert row.shape == oo.shape == (P + 108,)
            np.testing.assert_allclose(row[:P], oo[:P], atol=2e-3 + 500 * tol)
            np.testing.assert_allclose(row[P:], oo[P:], atol=2e-3 + 20 * tol)
            assert d == od and abs(r - orr) < 1e-5 + 0.05 * tol, (seed, t, d, od, r, orr)
            if d:
                break
    env.close()
    return worst


def check_chase_tag_factory_defaults(lib_path, n_steps=4):
    """create_chase_tag_game at its own default control_freq (25 Hz: CTG:57; kd 1.0, max_tau 18): observation shapes as _spaces() promises, and the
    engine it builds against the oracle env under the free-run comparator (sepmc_parity_common.check_free_running_against_oracle_env at the
    factory's defaults, a subset prop_type)"""
    import sepmc_parity_common as sc
    from lifelike_agility_and_play_amd import chase_tag
    cfg = sc.env_config((1, 0, 0))
    for k in ('control_freq', 'kp', 'kd', 'max_tau'):
        del cfg[k]
    cfg['prop_type'] = ['e_g', 'joint_pos']
    np.random.seed(3)
    env = chase_tag.create_chase_tag_game(lib_path=lib_path, **cfg)
    space = chase_tag._spaces(cfg['prop_type'])[0]
    obs = env.reset()
    rng = np.random.default_rng(0)
    for t in range(n_steps):
        for o in obs:
            for k, sp in space.spaces.items():
                assert o[k].shape == sp.shape and np.isfinite(o[k]).all(), (k, o[k].shape, sp.shape)
        obs, r, d, info = env.step([{'A_LLC': rng.normal(size=12) * 0.135}, {'A_LLC': rng.normal(size=12) * 0.135}])
        assert len(r) == 2 and np.isfinite(r).all()
    assert env._engine.push_trace().shape[-2] == 20                      # 20 substeps per control step: the factory's 25 Hz reached the kernel
    env.close()
    with arena_variant(dict(control_freq=25.0, kd=1.0, max_tau=18.0)):
        return sc.check_free_running_against_oracle_env(lib_path, n_steps=n_steps, prop_type=cfg['prop_type'], element_sets=((1, 0, 0),))
