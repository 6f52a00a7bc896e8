"""The checks of the spec-switch matrix (tests/spec_matrix.py), for any build of the engines: the host build of the kernel source
(test_spec_matrix_emul.py) and the HIP library (test_gpu_spec_matrix.py) run the same functions."""
import numpy as np
import pytest

import spec_matrix as sm
from lifelike_agility_and_play_amd import capi

SIGMA = 1.0


def make(engine, lib_path, n=None, seed=3, **kw):
    """a reset engine of the kind `engine` names (spec_matrix.ENGINES): n envs (PMC) / arenas (SEPMC)"""
    if engine in ('pmc', 'pmc_obst'):
        import parity_common as pc
        from lifelike_agility_and_play_amd import mocap, urdf_model
        if engine == 'pmc_obst':
            kw.update(set_obstacle=True, obstacle_height=0.2)
        E = pc.make_engine(urdf_model.default_model_blob(), mocap.load_mocap('', 1.0 / 50.0), n or 8, lib_path, seed=seed, **kw)
    elif engine == 'epmc':
        import epmc_parity_common as ec
        E = ec.make_engine(ec.env_config(1), n or 4, lib_path, seed=seed, **kw)
    else:
        import sepmc_parity_common as sc
        E = sc.make_engine(sc.env_config((1, 0, 0)), n or 2, lib_path, seed=seed, **kw)
    E.reset()
    return E


def step(E, engine, k=1):
    """k control steps of the random policy (the engines' own Philox draws): one launch per step"""
    for _ in range(k):
        if engine in ('pmc', 'pmc_obst'):
            E.step_random(SIGMA)
        else:
            E.step_random_n(SIGMA, 1)


def snapshot(E, engine):
    """everything a step moves: state, observation, reward / done, counters and the episode bookkeeping"""
    s = dict(state=E.state(), obs=E.obs(), counters=E.counters())
    rd = E.reward_done()
    for i, x in enumerate(rd):
        s['rd%d' % i] = x
    ep = E.episode_info() if engine in ('pmc', 'pmc_obst') else E.episode()
    for k, v in ep.items():
        s['ep_' + k] = v
    return s


def same(a, b):
    return set(a) == set(b) and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a if not isinstance(a[k], dict)) and \
        all(a[k] == b[k] for k in a if isinstance(a[k], dict))


def check_acceptance(engine, lib_path):
    """Every row, both friction modes: set / get round-trips, oracle-only switches and bad values fail at set time with LL_EINVAL and leave the
    value as it was; a REFUSED combination fails at the next step with LL_EINVAL naming the switch, and the engine is left exactly as it was --
    a step after the refusals equals the step of a twin engine that never saw them."""
    E, T = make(engine, lib_path), make(engine, lib_path)
    default = {name: E.get_spec(name) for name in sm.ROWS}
    n_refused = 0
    before = snapshot(E, engine)
    for name, row in sm.ROWS.items():
        for mode in sm.MODES:
            outcome = row['engines'][engine][mode]
            for v in row['values']:
                E.set_spec(friction_mode=mode)
                if outcome == sm.ORACLE:
                    with pytest.raises(capi.LLError) as ei:
                        E.set_spec(**{name: v})
                    assert ei.value.code == capi.LL_EINVAL, (name, ei.value)
                    assert E.get_spec(name) == default[name], name
                    continue
                spec = sm.spec_of(name, v) if name != 'friction_mode' else {name: v}
                E.set_spec(**spec)
                assert E.get_spec(name) == np.float32(v), (name, v, E.get_spec(name))
                if outcome == sm.REFUSED:
                    with pytest.raises(capi.LLError) as ei:
                        step(E, engine)
                    assert ei.value.code == capi.LL_EINVAL and name in str(ei.value), (engine, name, mode, ei.value)
                    assert same(snapshot(E, engine), before), (engine, name, mode, 'a refused step changed the engine')
                    n_refused += 1
                for k in spec:
                    E.set_spec(**{k: default[k]})
        for v in sm.BAD_VALUES.get(name, ()):
            with pytest.raises(capi.LLError) as ei:
                E.set_spec(**{name: v})
            assert ei.value.code == capi.LL_EINVAL, (name, v)
            assert E.get_spec(name) == default[name], (name, v)
    assert {name: E.get_spec(name) for name in sm.ROWS} == default
    step(E, engine); step(T, engine)
    assert same(snapshot(E, engine), snapshot(T, engine)), (engine, 'the refused calls left a trace')
    E.close(); T.close()
    return n_refused


def check_binding(engine, lib_path, n=8, k=25, modes=sm.MODES):
    """A short random-policy run at each PARITY row's value differs from the run at the default (with the row's `base` switches on both
    sides); at an INERT row's value it equals it bit for bit."""
    runs = {}

    def run(spec):
        key = tuple(sorted(spec.items()))
        if key not in runs:
            E = make(engine, lib_path, n)
            E.set_spec(**spec)
            step(E, engine, k)
            runs[key] = snapshot(E, engine)
            E.close()
        return runs[key]
    unbound, moved = [], []
    for name, row in sm.ROWS.items():
        for mode in modes:
            outcome = row['engines'][engine][mode]
            if outcome not in (sm.PARITY, sm.INERT):
                continue
            for v in row['values']:
                spec = {**sm.spec_of(name, v), 'friction_mode': mode} if name != 'friction_mode' else {name: v}
                ref = {k_: x for k_, x in spec.items() if k_ != name}
                if name == 'friction_mode':
                    ref = {name: 2}
                differs = not np.array_equal(run(spec)['state'], run(ref)['state'])
                if outcome == sm.PARITY and not differs and (name, engine) not in sm.BOUND_IN_COMPARATOR:
                    unbound.append((name, v, mode))
                if outcome == sm.INERT and not same(run(spec), run(ref)):
                    moved.append((name, v, mode))
    leg = sm.all_scalars(engine)
    if np.array_equal(run(leg)['state'], run({})['state']):
        unbound.append(('all_scalars', leg, 2))
    assert not unbound, (engine, 'these values do not bind in the run: they prove nothing', unbound)
    assert not moved, (engine, 'these values should have nothing to act on', moved)


def parity_rows(engine, modes=sm.MODES):
    """(name, spec) of every PARITY row of `engine` under the friction modes given"""
    out = []
    for name, row in sm.ROWS.items():
        for mode in modes:
            if row['engines'][engine][mode] == sm.PARITY:
                for v in row['values']:
                    spec = {**sm.spec_of(name, v), 'friction_mode': mode} if name != 'friction_mode' else {name: v}
                    if spec not in [s for _, s in out]:
                        out.append((name, spec))
    return out


def check_parity(engine, name, spec, lib_path, golden=None, orc=None, total=None):
    """engine vs oracle under `spec`, with the existing comparators and their standing bars"""
    if engine == 'pmc':
        import parity_common as pc
        from lifelike_agility_and_play_amd import mocap, urdf_model
        blob, table = urdf_model.default_model_blob(), mocap.load_mocap('', 1.0 / 50.0)
        if name == 'friction_dirs':          # the rule's discontinuity: its documented bars (test_kernel_logic_emul.py::test_sliding_direction_friction_variant)
            st = pc.run_lockstep(golden, orc, blob, table, lib_path, 16, 6, 7, resync=True, spec=spec, total_envs=total)
            c, v = np.asarray(st['config']), np.asarray(st['vel'])
            assert np.percentile(c, 98) < 1e-4 and np.percentile(v, 98) < 1e-3 and c.max() < 2e-2, (np.percentile(c, [98, 100]), np.percentile(v, [98, 100]))
            return st
        return pc.check_single_step_parity(golden, orc, blob, table, lib_path, n_envs=16, n_steps=6, spec=spec, total_envs=total)
    if engine == 'pmc_obst':
        import parity_common as pc
        from lifelike_agility_and_play_amd import mocap, urdf_model
        return pc.check_obstacle_variant(golden, orc, urdf_model.default_model_blob(), mocap.load_mocap('', 1.0 / 50.0), lib_path, n_envs=12, n_steps=40,
                                         total_envs=total, spec=spec, cap_ill=2, pct=98 if name == 'friction_dirs' else 100)
    import epmc_parity_common as ec
    if engine == 'epmc' and name == 'leg_edges':
        with ec.spec_variant(**{k: v for k, v in spec.items() if k != name}):
            kw = dict(n_envs=48, cap_ill=4, cap_tie=2) if lib_path is None else {}          # (the HIP library: the caps of test_gpu_epmc.py::test_legs_on_edges_against_oracle)
            return ec.check_legs_on_edges_against_oracle(lib_path, total_envs=total, **kw)
    with ec.spec_variant(**spec):
        if engine == 'epmc':
            return ec.check_terrain_physics_against_oracle(lib_path, n_envs=16, total_envs=total)
        import sepmc_parity_common as sc
        return sc.check_pair_physics_against_oracle(lib_path, n_arenas=12, total_arenas=total, cap_ill=2)
