"""The engines' live random draws against the NumPy Philox reference (tests/philox_ref.py), shared by the host build of the kernel source
(test_draws_emul.py: lib_path = the emulation library) and the HIP library (test_gpu_draws.py: lib_path = None).

The goldens feed the engines recorded draws (reset(draws=...), reset(clip=, t0=)); these checks close the chain from the live Philox path
to them: every random-policy action per row, group and step; every seeded PMC start, bit for bit; every seeded EPMC / SEPMC reset and
step draw, through a second engine fed the reference's uniforms."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import philox_ref as pr  # noqa: E402
import parity_common as pc  # noqa: E402
import epmc_parity_common as ec  # noqa: E402
import sepmc_parity_common as sc  # noqa: E402
from lifelike_agility_and_play_amd import epmc_capi  # noqa: E402
from test_epmc_oracle_golden import env_config as epmc_env_config  # noqa: E402

SEEDS = (7, 0x10004d34d)     # the second: key word 1 = 1, and the first word of row 0, group 2 at step 0 is 82 -- there u1 = 83 * 2^-32 is not u1 = 82 * 2^-32
EDGE = 1e-12                 # a start whose u1 lies this close to a cdf entry may fall either side of it (the device folds the table by a parallel scan)


def read_floats(lib_path, addr, n):
    """n float32 at an engine address: host memory for the emulation library, device memory for the HIP library."""
    if lib_path is None:
        from lifelike_agility_and_play_amd import gather
        return gather.device_tensor(addr, (n,)).cpu().numpy()
    return np.ctypeslib.as_array((ctypes.c_float * n).from_address(addr)).copy()


def action_buffer(E, lib_path):
    E.sync()
    p = E.device_ptrs()
    return read_floats(lib_path, p.actions, p.n_envs * 12).reshape(p.n_envs, 12)


def assert_actions(a, step, seed, sigma, what):
    ref, sm = pr.random_policy_actions(a.shape[0], step, seed, sigma)
    err = np.abs(a.astype(np.float64) - ref)
    tol = 2e-6 * sm + 1e-7 * sigma                    # a few float32 ulps of sigma * m; a wrong counter is off by O(sigma)
    bad = np.argwhere(err > tol)
    assert not len(bad), '%s: step %d seed %#x: %d of %d actions off the Philox reference, first (row, col) %s: %r vs %r' % (
        what, step, seed, len(bad), a.size, tuple(bad[0]), a[tuple(bad[0])], ref[tuple(bad[0])])


# ---- random-policy actions --------------------------------------------------------------------------------------------------------------

def check_pmc_random_actions(model_blob, table, lib_path, sizes, seeds=SEEDS, sigma=pc.SIGMA, k=5):
    """fill_random_actions, step_random and every step of step_random_n (read from the action columns of the unroll rows) against
    sigma * Box-Muller of counter (row * 3 + g, step lo, step hi, 0xAC710), key (seed lo, seed hi)."""
    for n in sizes:
        for seed in seeds:
            E = pc.make_engine(model_blob, table, n, lib_path, seed=seed, auto_reset=1)
            E.reset()
            E.fill_random_actions(sigma)                         # step count 0
            assert_actions(action_buffer(E, lib_path), 0, seed, sigma, 'PMC fill_random_actions n=%d' % n)
            E.step()
            E.step_random(sigma)                                 # step count 1
            assert_actions(action_buffer(E, lib_path), 1, seed, sigma, 'PMC step_random n=%d' % n)
            addr, w = E.enable_unrolls(k, 1)                     # unroll rows: [obs_dim | A 12 | neglogp | R | V | r | 1 - done]
            E.step_random_n(sigma, k)                            # steps 2 .. k + 1 in one launch
            E.sync()
            ring = read_floats(lib_path, addr, n * k * w).reshape(n, k, w)
            for t in range(k):
                assert_actions(ring[:, t, E.obs_dim:E.obs_dim + 12], 2 + t, seed, sigma, 'PMC step_random_n n=%d, step %d of the launch' % (n, t))
            assert_actions(action_buffer(E, lib_path), 1 + k, seed, sigma, 'PMC step_random_n n=%d (action buffer)' % n)
            E.close()


def check_terrain_random_actions(lib_path, sizes, seeds=SEEDS, sigma=pc.SIGMA, sepmc=False):
    """EPMC / SEPMC: fill_random_actions and k = 1 launches of step_random_n (which record the actions they draw) against the reference;
    SEPMC's rows are its robots (arena * 2 + robot)."""
    for n in sizes:
        for seed in seeds:
            if sepmc:
                E = sc.make_engine(sc.env_config(sc.ALL_ELEMENTS), n, lib_path, auto_reset=1, seed=seed)
            else:
                E = ec.make_engine(epmc_env_config(1), n, lib_path, auto_reset=1, seed=seed)
            what = ('SEPMC' if sepmc else 'EPMC') + ' n=%d' % n
            E.reset()
            E.fill_random_actions(sigma)
            assert_actions(action_buffer(E, lib_path), 0, seed, sigma, what + ' fill_random_actions')
            E.step()
            for s in (1, 2):
                E.step_random_n(sigma, 1)
                assert_actions(action_buffer(E, lib_path), s, seed, sigma, what + ' step_random_n(1)')
            E.close()


# ---- seeded PMC starts ------------------------------------------------------------------------------------------------------------------

def engine_cdf(prob):
    """the inclusive CDF as the engine's host code accumulates it (pmc_engine.hpp:111-114, :337-340): in clip order, the last entry 1"""
    cdf = np.empty(len(prob))
    acc = 0.0
    for c, p in enumerate(prob):
        acc += p
        cdf[c] = acc
    cdf[-1] = 1.0
    return cdf


def assert_starts(E, table, seed, envs, episode, cdf, what):
    """clip equal, time bit-equal (float64) to Pmc::sample_start of (env, episode) for `envs`; envs whose u1 lies within EDGE of a cdf
    entry are skipped (few of them). -> the reference (clip, t0) of `envs`"""
    info = E.episode_info()
    clip, t0, u1 = pr.pmc_start(envs, episode, seed, cdf, table.clip_len, table.frame_step, table.margin)
    edge = np.abs(u1[:, None] - cdf[None, :]).min(1) < EDGE
    assert edge.sum() <= max(1, len(envs) // 100), '%s: %d starts on a cdf edge' % (what, edge.sum())
    ok = ~edge
    bad = np.flatnonzero(ok & (info['clip'][envs] != clip))
    assert not len(bad), '%s: env %d started clip %d, the reference %d' % (what, envs[bad[0]], info['clip'][envs[bad[0]]], clip[bad[0]])
    bad = np.flatnonzero(ok & (info['time'][envs] != t0))
    assert not len(bad), '%s: env %d started at t0 %r, the reference %r' % (what, envs[bad[0]], info['time'][envs[bad[0]]], t0[bad[0]])
    return clip, t0


def check_pmc_starts(model_blob, table, lib_path, n, seeds=SEEDS):
    """Pmc::sample_start through ll_reset and through the auto-reset inside the step: (clip, t0) of counter (env, episode, 0x5eed, 0),
    key (seed lo, seed hi), episode = the env's episode count + 1; the inverse-cdf clip and t0 = u2 * frame_step * (len - margin - 1).
    Then the transitive link: an engine reset with those (clip, t0) starts bit-equal."""
    for seed in seeds:
        E = pc.make_engine(model_blob, table, n, lib_path, seed=seed, auto_reset=1, prioritized_sample_factor=3.0)
        envs = np.arange(n)
        ep = np.zeros(n, dtype=np.int64)
        cdf = engine_cdf(np.full(table.n_clips, 1.0 / table.n_clips))
        E.reset(); ep += 1
        clip, t0 = assert_starts(E, table, seed, envs, ep, cdf, 'reset, uniform table, seed %#x' % seed)
        F = pc.make_engine(model_blob, table, n, lib_path, seed=seed + 1, auto_reset=1, prioritized_sample_factor=3.0)
        F.reset(clip=clip, t0=t0)                                # the recorded-start path the goldens use
        for x, y in ((E.obs(), F.obs()), (E.state(), F.state()), (E.ref_state(), F.ref_state())):
            np.testing.assert_array_equal(x, y)
        F.close()
        # a prioritized table (factor 3): the cdf the engine accumulated from the probabilities it stores
        rng = np.random.default_rng(seed & 0xffff)
        E.set_sampling_table(rng.uniform(0.0, 0.95, table.n_clips))
        cdf = engine_cdf(E.sampling_table()[0])
        E.reset(); ep += 1
        assert_starts(E, table, seed, envs, ep, cdf, 'reset, prioritized table, seed %#x' % seed)
        ids = np.arange(n)[(np.arange(n) % 3) == 1] if n > 1 else np.arange(1)
        E.reset(env_ids=ids); ep[ids] += 1                        # partial reset: only these envs start an episode
        assert_starts(E, table, seed, envs, ep, cdf, 'partial reset, seed %#x' % seed)
        E.close()


def check_pmc_reseeds(model_blob, table, lib_path, n, seed=SEEDS[1], n_steps=40, sigma=0.7):
    """The auto-reset inside step_random re-seeds from episode count + 1 (llenv.hip:385, pmc_step.hpp:2467): uniform table, then a
    prioritized one -- a re-seed in a single-step launch draws from the table the steps before it left (sampling_table() read before)."""
    for factor in (0.0, 3.0):
        E = pc.make_engine(model_blob, table, n, lib_path, seed=seed, auto_reset=1, prioritized_sample_factor=factor)
        E.reset()
        ep = np.ones(n, dtype=np.int64)
        if factor:
            E.set_sampling_table(np.full(table.n_clips, 0.9))       # one finished episode changes what everybody after it draws
        reseeds = 0
        for t in range(n_steps):
            cdf = engine_cdf(E.sampling_table()[0])
            E.step_random(sigma)
            info = E.episode_info()
            new = np.flatnonzero(info['steps'] == 0)               # re-seeded inside this step
            ep[new] += 1
            if len(new):
                assert_starts(E, table, seed, new, ep[new], cdf, 'auto-reset at step %d, factor %g' % (t, factor))
            reseeds += len(new)
        assert reseeds >= max(2, n // 4), reseeds
        E.close()


# ---- seeded EPMC / SEPMC resets and step draws --------------------------------------------------------------------------------------

def _assert_same(what, pairs):
    for name, x, y in pairs:
        assert np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True), '%s: %s differs between the live Philox stream and the reference draws' % (what, name)


def _epmc_views(E):
    rows, n = E.statics()
    f, t, h, fr = E.rays()
    return [('statics', rows), ('n_statics', n), ('state', E.state()), ('obs', E.obs()), ('rays from', f), ('rays to', t), ('ray hit', h),
            ('ray fraction', fr)] + [('episode ' + k, v) for k, v in E.episode().items()]


def _sepmc_views(E):
    rows, n = E.boxes()
    f, t, h, fr = E.rays()
    return [('boxes', rows), ('n_boxes', n), ('state', E.state()), ('obs', E.obs()), ('vis', E.vis()), ('rays from', f), ('rays to', t),
            ('ray hit', h), ('ray fraction', fr)] + [('episode ' + k, v) for k, v in E.episode().items()]


def _compare(what, A, B, views, skip=(), rows=slice(None), close=()):
    """bit-equal views, but those named in `close`: float32 ulps (a draw from the wrong index or stream moves them by O(1))"""
    va, vb = views(A), views(B)
    _assert_same(what, [(k, x[rows], y[rows]) for (k, x), (_, y) in zip(va, vb) if k not in skip and k not in close])
    for (k, x), (_, y) in zip(va, vb):
        if k in close:
            np.testing.assert_allclose(x[rows], y[rows], rtol=1e-6, atol=1e-8, err_msg='%s: %s' % (what, k))


def _step_twice(A, B, sigma):
    """both engines two control steps of the same random actions (episodes of max_steps = 2); -> the rows (envs / arenas) whose episode
    ended at the second step: A re-seeded those inside it, from episode 2 (a row that fell or was caught at the first step re-seeded then)"""
    ended = []
    for t in range(2):
        A.fill_random_actions(sigma); A.step()
        B.fill_random_actions(sigma); B.step()
        ended.append(np.asarray(B.reward_done()[1], dtype=bool))
    rows = ~ended[0] & ended[1]
    assert ended[1].all() and rows.mean() >= 0.5, (ended[0].mean(), ended[1].mean())
    return rows


def _push_cfg(cfg):
    """pushes from the first substeps on: a new force every 6 substeps, held for 2 (PR:56-86 counted in substeps)"""
    cfg = dict(cfg)
    rc = dict(cfg['env_randomize_config'])
    rc['disturb_force_config'] = {'start_time': 0.0, 'interval_time': 0.0125, 'duration_time': 0.0045, 'horizontal_force': [0, 50], 'vertical_force': [0, 10]}
    cfg['env_randomize_config'] = rc
    return cfg


def check_epmc_seeded_resets(lib_path, n, seeds=SEEDS, elements=(0, 1, 2, 3), sigma=pc.SIGMA):
    """Engine A resets (and re-seeds inside its steps) from its own Philox stream; engine B is reset with draws = the reference's u01 stream
    of (seed; env, episode, block, 0x7e44a1): statics, episode, state, obs and ray traces bit-equal.  The draws= path is pinned to the
    reference goldens (check_terrain_and_reset_against_goldens), so this closes the chain from the live path to the reference."""
    L = epmc_capi.LLE_MAX_DRAWS
    for el in elements:
        for seed in seeds:
            cfg = epmc_env_config(el)
            cfg['max_steps'] = 2                                      # episodes time out at the second step and re-seed inside it
            A = ec.make_engine(cfg, n, lib_path, auto_reset=1, seed=seed)
            B = ec.make_engine(cfg, n, lib_path, auto_reset=0, seed=seed)
            envs = np.arange(n)
            A.reset()
            B.reset(draws=pr.epmc_stream(envs, 1, pr.EPMC_RESET_SALT, seed, L))
            what = 'EPMC element %d seed %#x n=%d' % (el, seed, n)
            _compare(what + ', reset', A, B, _epmc_views)
            rows = _step_twice(A, B, sigma)
            B.reset(draws=pr.epmc_stream(envs, 2, pr.EPMC_RESET_SALT, seed, L))     # what A's in-step re-seed (episode 2) drew
            _compare(what + ', in-step re-seed', A, B, _epmc_views, rows=rows)
            A.close(); B.close()


def _forces_drawn(count, n_sub, interval):
    """forces a step draws (epmc_step.hpp:806-816, PR:56-86): the push counter runs once per substep; a positive multiple of the interval
    draws a new force and restarts it. -> (forces drawn, the counter after the step)"""
    k = 0
    for s in range(n_sub):
        count += 1
        if count > 0 and count % interval == 0:
            k += 1
            count = 0
    return k, count


def check_epmc_step_draws(lib_path, n, seed=SEEDS[1], element=0, n_steps=6, sigma=pc.SIGMA):
    """Step draws (joystick target, target speed, pushes) from the step stream (seed; env, episode, index, 0x57e9d3), index continuing at
    EP_STEP_DRAWS: engine B is fed the reference's uniforms through set_step_draws, from the index A's consumption has reached."""
    cfg = _push_cfg(epmc_env_config(element, cmd_range=(2, 4)))
    A = ec.make_engine(cfg, n, lib_path, auto_reset=0, seed=seed)
    B = ec.make_engine(cfg, n, lib_path, auto_reset=0, seed=seed)
    envs = np.arange(n)
    A.reset(); B.reset()
    used = np.zeros(n, dtype=np.int64)                                # EP_STEP_DRAWS: 0 after a reset
    pd = cfg['env_randomize_config']['disturb_force_config']
    count, interval = int(-pd['start_time'] // epmc_capi.TIME_STEP), int(pd['interval_time'] // epmc_capi.TIME_STEP)   # epmc_capi.make_epmc_config
    pushes = cmds = 0
    for t in range(n_steps):
        e = A.episode()
        cmd = (e['counter'].astype(np.int64) % e['cmd_vary_freq'].astype(np.int64)) == 0
        B.set_step_draws(pr.epmc_stream(envs, e['episode'].astype(np.int64), pr.EPMC_STEP_SALT, seed, 64, start=used))
        A.fill_random_actions(sigma); A.step()
        B.fill_random_actions(sigma); B.step()
        what = 'EPMC step draws, step %d' % t
        _compare(what, A, B, _epmc_views)
        _assert_same(what, [('push trace', A.push_trace(), B.push_trace())])
        forces, count = _forces_drawn(count, A.n_sub, interval)
        pushes += forces
        cmds += cmd.sum()
        used += cmd * (1 + (element == 0)) + 3 * forces             # target angle (joystick) + speed on a command step, 3 per force (PR:88-98)
    assert pushes >= n_steps and cmds >= n_steps, (pushes, cmds)   # forces and commands drawn all along
    A.close(); B.close()


def check_sepmc_seeded_resets(lib_path, n, seeds=SEEDS, sigma=pc.SIGMA):
    """SEPMC: as check_epmc_seeded_resets per arena (seed; arena, episode, block, 0x5e9a1d), arenas with every element, and an in-step
    re-seed; then one step with pushes drawn from the step stream (seed; arena, episode, index, 0x57e9d3), index 0 after a reset."""
    L = epmc_capi.LLE_MAX_DRAWS
    arenas = np.arange(n)
    for seed in seeds:
        what = 'SEPMC seed %#x n=%d' % (seed, n)
        cfg = sc.env_config(sc.ALL_ELEMENTS, max_steps=2)
        A = sc.make_engine(cfg, n, lib_path, auto_reset=1, seed=seed)
        B = sc.make_engine(cfg, n, lib_path, auto_reset=0, seed=seed)
        A.reset()
        B.reset(draws=pr.epmc_stream(arenas, 1, pr.SEPMC_RESET_SALT, seed, L))
        _compare(what + ', reset', A, B, _sepmc_views)
        rows = _step_twice(A, B, sigma)
        B.reset(draws=pr.epmc_stream(arenas, 2, pr.SEPMC_RESET_SALT, seed, L))
        # (who0 / who_taker: the contact record of the step that ended the game, sepmc_step.hpp:482; a reset clears it, a re-seed keeps it.
        # The observation's opponent-relative entries (columns 927-929, 942-944 of a robot's row) can round differently in the last ulp between
        # the step kernel's re-seed and the reset kernel on the device, FMA contraction being theirs to choose; the host build is bit-equal.)
        _compare(what + ', in-step re-seed', A, B, _sepmc_views, skip=('episode who0', 'episode who_taker'), rows=rows,
                 close=('obs',) if lib_path is None else ())
        A.close(); B.close()
    seed = seeds[-1]
    cfg = _push_cfg(sc.env_config(sc.ALL_ELEMENTS))
    A = sc.make_engine(cfg, n, lib_path, auto_reset=0, seed=seed)
    B = sc.make_engine(cfg, n, lib_path, auto_reset=0, seed=seed)
    A.reset(); B.reset()
    B.set_step_draws(pr.epmc_stream(arenas, 1, pr.SEPMC_STEP_SALT, seed, 64))
    A.fill_random_actions(sigma); A.step()
    B.fill_random_actions(sigma); B.step()
    _compare('SEPMC step draws', A, B, _sepmc_views)
    tr = A.push_trace()
    _assert_same('SEPMC step draws', [('push trace', tr, B.push_trace())])
    assert (tr[..., 0] > 0.5).any(axis=-1).all(), 'every robot is pushed in the step'
    A.close(); B.close()


# ---- the fused policy kernel (pmc_policy.inc) against the float64 statement (oracle/pmc_policy.py) ---------------------------------------

def policy_inputs(obs_real, w, n, seed=0):
    """n observation rows: the engine's own, every third row pushed to +-(10 .. 1000) sd on every column (the +-5 clip bites column by
    column), every seventh exactly at the rms mean"""
    rng = np.random.default_rng(seed)
    mean, sd = np.concatenate([w[0].ravel(), w[2].ravel()]), np.concatenate([w[1].ravel(), w[3].ravel()])
    x = obs_real[np.arange(n) % len(obs_real)].astype(np.float32).copy()
    far = np.arange(n) % 3 == 1
    s = rng.uniform(10.0, 1000.0, (far.sum(), x.shape[1])) * rng.choice([-1.0, 1.0], (far.sum(), x.shape[1]))
    x[far] = (mean + s * sd).astype(np.float32)
    x[np.arange(n) % 7 == 3] = mean.astype(np.float32)
    return x


def policy_forward(w, obs, dtype=np.float64, code=None, clip=5.0, drop_bias=None):
    """The PMC policy's forward pass in `dtype`, the float32 one in the kernel's order of operations where it matters (the normalisation
    (x - mean) / (sd + 1e-8f), the score ze . code - |code|^2 / 2 with the half-norms rounded from float64, pmc_policy.inc:208-213).
    code: evaluate the decoder at these codes instead of the argmax.  clip / drop_bias: deliberately wrong variants (the tolerances' power).
    -> dict(score [n, 256], code, action [n, 12], value [n])"""
    W = [np.asarray(a, dtype=dtype) for a in w]
    if drop_bias is not None:
        W[drop_bias] = np.zeros_like(W[drop_bias])
    relu = lambda v: np.maximum(v, dtype(0))
    x = np.asarray(obs, dtype=dtype)
    mean, sd = np.concatenate([W[0].ravel(), W[2].ravel()]), np.concatenate([W[1].ravel(), W[3].ravel()])
    ob = np.clip((x - mean) / (sd + dtype(1e-8)), -clip, clip).astype(dtype)
    prop = ob[:, :135]
    h = relu(relu(ob @ W[10] + W[11]) @ W[12] + W[13])
    ze = h @ W[14] + W[15]
    cbh = (-0.5 * (np.asarray(w[16], np.float64) ** 2).sum(0)).astype(dtype)
    score = ze @ W[16] + cbh
    if code is None:
        code = np.argmax(score, 1)
    q = W[16].T[code]
    s = np.concatenate([relu(prop @ W[17] + W[18]), relu(q @ W[19] + W[20])], axis=1)
    a = relu(relu(s @ W[21] + W[22]) @ W[23] + W[24]) @ W[25] + W[26]
    v = (np.tanh(np.tanh(ob @ W[4] + W[5]) @ W[6] + W[7]) @ W[8] + W[9])[:, 0]
    return dict(score=score.astype(np.float64), code=code, action=a.astype(np.float64), value=v.astype(np.float64))


def policy_tolerances(w, obs):
    """From a float32 NumPy pass against the float64 one on the same inputs: delta = 4 x the worst score error (a code choice within delta of
    the runner-up is a near-tie), and 4 x the worst action / value error, never looser than 2e-4."""
    r64 = policy_forward(w, obs)
    r32 = policy_forward(w, obs, np.float32, code=r64['code'])
    delta = 4.0 * np.abs(r32['score'] - r64['score']).max()
    tol_a = min(4.0 * np.abs(r32['action'] - r64['action']).max(), 2e-4)
    tol_v = min(4.0 * np.abs(r32['value'] - r64['value']).max(), 2e-4)
    return dict(delta=delta, tol_a=tol_a, tol_v=tol_v, ref=r64)


def near_ties(score, delta):
    top = np.sort(score, axis=1)[:, -2:]
    return (top[:, 1] - top[:, 0]) < delta
