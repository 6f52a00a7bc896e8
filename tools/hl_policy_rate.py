"""Launch time of the fused EPMC / SEPMC policy kernels (include/hl/llenv_hl_policy.h) and the rate of the closed device actor loop.

    python tools/hl_policy_rate.py [reps] [--pg]

Prints: us per ll_hl_policy_act launch (HIP events, ll_hl_policy_time_ms) at 1024 / 4096 / 16384 rows; env-steps/s of  act ; step  on the device
(EPMC hurdles 4096 envs, SEPMC 2048 arenas = 4096 robot rows, auto-reset, the engine's done buffer as the reset mask); the same loop with the
float64 NumPy policy (oracle/, host round trip every step) at 256 rows, for scale.
--pg: instead, ll_hl_policy_act against the PPO actor ll_hl_policy_act_pg (every head sampled, neglogp and the value branch) at the same row
counts, and env-steps/s of  act_pg ; step  on the device."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np  # noqa: E402


def engine(kind, n, auto_reset=1):
    if kind == 'epmc':
        import rollout_epmc_policy as RO
        import epmc_parity_common as ec
        return ec.make_engine(RO.env_config(RO.ELEMENT['hurdle'], n), n, None, auto_reset=auto_reset, seed=1)
    import sepmc_parity_common as sc
    return sc.make_engine(sc._game_cfg(), n, None, auto_reset=auto_reset, seed=1)


def policy(kind, rows, value=False):
    import hl_policy_ref as R
    import hl_policy_pg_ref as G
    from lifelike_agility_and_play_amd.policies import hl_policy_hip as H
    if kind == 'epmc':
        return H.HipEpmcPolicy(R.EPMC_WEIGHTS['hurdle'], rows, value_npz=G.EPMC_VALUE['hurdle'] if value else None)
    return H.HipSepmcPolicy(R.SEPMC_WEIGHTS, rows, value_npz=G.SEPMC_VALUE if value else None)


def launch_us(kind, rows, reps, pg=False):
    import torch
    pol = policy(kind, rows, value=pg)
    dim = 916 if kind == 'epmc' else 965
    rng = np.random.default_rng(0)
    obs = torch.from_numpy(rng.normal(0, 1, (rows, dim)).astype(np.float32)).cuda()
    act = torch.empty((rows, 12), device='cuda')
    nl = torch.empty((rows, pol.n_heads), device='cuda')
    val = torch.empty(rows, device='cuda')

    def call(i):
        if pg:
            pol.act_pg_ptr(obs.data_ptr(), act.data_ptr(), rows, 7, i, True, d_neglogp=nl.data_ptr(), d_value=val.data_ptr())
        else:
            pol.act_ptr(obs.data_ptr(), act.data_ptr(), rows)
    for i in range(5):
        call(i)
    torch.cuda.synchronize()
    pol.enable_timing(True)
    for i in range(reps):
        call(i)
    ms, n = pol.time_ms()
    pol.close()
    return 1e3 * ms


def device_loop(kind, n, steps, pg=False):
    import torch
    E = engine(kind, n)
    E.reset()
    rows = E.device_ptrs().n_envs
    pol = policy(kind, rows, value=pg)
    nl = torch.empty((rows, pol.n_heads), device='cuda')
    val = torch.empty(rows, device='cuda')

    def act(t):
        if pg:
            pol.act_pg(E, 7, t, True, d_neglogp=nl.data_ptr(), d_value=val.data_ptr())
        else:
            pol.act(E)
    for t in range(10):
        act(t); E.step()
    E.sync()
    t0 = time.perf_counter()
    for t in range(steps):
        act(10 + t)
        E.step()
    E.sync()
    dt = time.perf_counter() - t0
    torch.cuda.synchronize()
    pol.close(); E.close()
    return rows * steps / dt, 1e3 * dt / steps


def host_loop(kind, n, steps):
    from oracle.epmc_policy import EpmcPolicy
    from oracle.sepmc_policy import SepmcPolicy
    import hl_policy_ref as R
    E = engine(kind, n, auto_reset=1)
    E.reset()
    rows = E.device_ptrs().n_envs
    pol = EpmcPolicy(R.EPMC_WEIGHTS['hurdle'], rows) if kind == 'epmc' else SepmcPolicy(R.SEPMC_WEIGHTS, rows)
    t0 = time.perf_counter()
    for _ in range(steps):
        obs = E.obs().reshape(rows, -1)
        _, done = E.reward_done()[:2]
        d = np.asarray(done).reshape(-1)
        if kind == 'sepmc':
            d = np.repeat(d, 2)
        if d.any():
            pol.reset(np.flatnonzero(d))
        E.step_host(pol.act(obs).astype(np.float32))
    E.sync()
    dt = time.perf_counter() - t0
    E.close()
    return rows * steps / dt, 1e3 * dt / steps


def main():
    import torch
    import __graft_entry__ as g
    args = [a for a in sys.argv[1:] if a != '--pg']
    reps = int(args[0]) if args else 200
    print('device: %s; build %s' % (torch.cuda.get_device_name(0), g.build_info().get('code_object_sha256')))
    if '--pg' in sys.argv[1:]:
        for kind in ('epmc', 'sepmc'):
            for r in (1024, 4096, 16384):
                a, b = launch_us(kind, r, reps), launch_us(kind, r, reps, pg=True)
                print('%-5s %5d rows: act %.1f us, act_pg %.1f us (%.2fx)' % (kind.upper(), r, a, b, b / a))
        for kind, n in (('epmc', 4096), ('sepmc', 2048)):
            rate, ms = device_loop(kind, n, 500, pg=True)
            print('%-5s device loop act_pg ; step, %d rows: %.3f ms per step, %.2f M env-steps/s' % (kind.upper(), n if kind == 'epmc' else 2 * n, ms, rate / 1e6))
        return
    for kind in ('epmc', 'sepmc'):
        print('%-5s launch: %s' % (kind.upper(), ', '.join('%d rows %.1f us' % (r, launch_us(kind, r, reps)) for r in (1024, 4096, 16384))))
    for kind, n in (('epmc', 4096), ('sepmc', 2048)):
        rate, ms = device_loop(kind, n, 500)
        print('%-5s device loop act ; step, %d rows: %.3f ms per step, %.2f M env-steps/s' % (kind.upper(), n if kind == 'epmc' else 2 * n, ms, rate / 1e6))
    for kind, n in (('epmc', 256), ('sepmc', 128)):
        rate, ms = host_loop(kind, n, 20)
        print('%-5s NumPy policy on the host, %d rows: %.1f ms per step, %.0f env-steps/s' % (kind.upper(), 256, ms, rate))


if __name__ == '__main__':
    main()
