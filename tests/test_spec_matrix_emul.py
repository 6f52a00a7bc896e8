"""The spec-switch matrix (tests/spec_matrix.py) on the CPU, through the host build of the kernel source (tests/emul): every run-time physics
switch is accepted or refused as the table says, binds where it is meant to act, and holds the engine to the oracle; and every step-kernel build
the shipped gfx950 code object carries is reached by some row.  tests/test_gpu_spec_matrix.py runs the same matrix through the HIP library."""
import os
import subprocess
import sys

import numpy as np
import pytest

import spec_matrix as sm
import spec_matrix_common as smc
from test_kernel_logic_emul import emul_lib  # noqa: F401  (the session fixture that builds tests/emul)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_table_has_a_row_for_every_switch():
    ids, count = sm.header_spec_ids(os.path.join(ROOT, 'include', 'llenv_model.h'))
    assert sorted(ids.values()) == list(range(count)), ids
    assert {name: row['id'] for name, row in sm.ROWS.items()} == ids
    from lifelike_agility_and_play_amd import capi
    assert capi.SPEC_IDS == ids
    for name, row in sm.ROWS.items():
        assert set(row['engines']) == set(sm.ENGINES) and all(set(m) == set(sm.MODES) for m in row['engines'].values()), name
        assert row['values'], name
        for engine in row.get('xrows', ()):
            assert row['engines'][engine][2] == sm.PARITY, (name, engine)


@pytest.mark.parametrize('engine', sm.ENGINES)
def test_acceptance(engine, emul_lib):  # noqa: F811
    n = smc.check_acceptance(engine, emul_lib)
    expected = sum(1 for row in sm.ROWS.values() for m in sm.MODES if row['engines'][engine][m] == sm.REFUSED)
    assert n == expected >= 1, (n, expected)


@pytest.mark.parametrize('engine', sm.ENGINES)
def test_binding(engine, emul_lib):  # noqa: F811
    smc.check_binding(engine, emul_lib)


def _parity_cases():
    return [pytest.param(engine, name, spec, id='%s-%s-fm%d' % (engine, name, spec.get('friction_mode', 2)))
            for engine in sm.ENGINES for name, spec in smc.parity_rows(engine)]


@pytest.mark.parametrize('engine,name,spec', _parity_cases())
def test_parity(engine, name, spec, golden, orc, emul_lib):  # noqa: F811
    smc.check_parity(engine, name, spec, emul_lib, golden=golden, orc=orc)


def _code_object_builds():
    """the step-kernel builds of the shipped gfx950 code object, unbundled as tools/isa_hazards.check_library does"""
    import tempfile
    import __graft_entry__ as g
    lib = g.build_hip()
    llvm = g._rocm_llvm_bin()
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, 'fat.bin'), os.path.join(d, 'dev.co')
        subprocess.check_call([os.path.join(llvm, 'llvm-objcopy'), '--dump-section', '.hip_fatbin=' + fat, lib, os.path.join(d, 'copy.so')])
        subprocess.check_call([os.path.join(llvm, 'clang-offload-bundler'), '--type=o', '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--input=' + fat,
                               '--output=' + co, '--unbundle'])
        syms = subprocess.run([os.path.join(llvm, 'llvm-objdump'), '--syms', '--demangle', co], check=True, capture_output=True, text=True).stdout
    builds = set()
    for line in syms.splitlines():
        if ' F .text' not in line:                                  # the kernels' code (not their .kd descriptors)
            continue
        b = sm.build_of_symbol(line.split('\t', 1)[1].split(' void ', 1)[-1].strip())
        if b:
            builds.add(b)
    return builds


# ---- csrc/launch_plan.hpp (through tests/emul's emu_step_plan / emu_launch_caps) against the table's restatement and against the rule as written down -----
ENGINE_ID = {'pmc': 0, 'pmc_obst': 0, 'epmc': 1, 'sepmc': 2}        # pmc_tables.hpp LL_ENGINE_*
SIMDS_HW, ONE_WAVE = 1024, 0x7fffffff
CAPS_ENV = ('LL_SHARE_SIMDS', 'LL_SEPMC_ONE_WAVE', 'LL_EPMC_ONE_WAVE', 'LL_DETERMINISTIC', 'LL_SPLIT_RAYS')


def _spec6(engine, spec):
    return [float(engine == 'pmc_obst'), spec.get('friction_mode', 2), spec.get('self_friction', 0), spec.get('pair_friction', 0), spec.get('max_pair', 2), spec.get('leg_edges', 0)]


class Planner:
    """the plan of a step call; every point asked for is kept (`points`) so that the sanitizer build of the header can be walked over the same grid"""

    def __init__(self, lib_path):
        import ctypes as C
        self.C, self.lib, self.points = C, C.CDLL(lib_path), []

    def caps(self, monkeypatch, **env):
        """LaunchCaps as the product reads them from the environment, on a device of SIMDS_HW SIMDs with the shipped LL_SEPMC_ONE_WAVE default"""
        for k in CAPS_ENV:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        out = (self.C.c_int * 7)()
        assert self.lib.emu_launch_caps(SIMDS_HW, 1, out) == 0
        return list(out)

    def plan(self, engine, spec, n_envs, n_steps, caps, scripted=False):
        point = [ENGINE_ID[engine]] + _spec6(engine, spec) + [n_envs, n_steps, int(scripted)] + list(caps)
        out = (self.C.c_int * 8)()
        assert self.lib.emu_step_plan(point[0], (self.C.c_double * 6)(*point[1:7]), n_envs, n_steps, int(scripted), (self.C.c_int * 7)(*caps), out) == 0
        self.points.append((point, list(out)))
        occ, obst, multi, cone, xrows, lds, per, split = out
        return dict(build=(('pmc' if ENGINE_ID[engine] == 0 else engine) + '_step_kernel', occ, bool(obst), bool(multi), bool(cone), bool(xrows)), row_scratch=bool(lds), per=per, split=bool(split))

    def call_builds(self, engine, spec, n_envs, n_steps, caps, scripted=False):
        """the builds of every launch of one step call: the call is cut by its plan, and a PMC launch is planned again with the steps it carries (HipBackend::launch_step)"""
        pl = self.plan(engine, spec, n_envs, n_steps, caps, scripted)
        sizes = {min(n_steps, pl['per'])} | ({n_steps % pl['per']} - {0})
        return {self.plan(engine, spec, n_envs, k, caps, scripted)['build'] for k in sizes} if ENGINE_ID[engine] == 0 else {pl['build']}


@pytest.fixture(scope='module')
def planner(emul_lib):  # noqa: F811
    return Planner(emul_lib)


def _table_grid(planner, monkeypatch):
    """every engine x every PARITY / INERT cell's spec at both friction modes x occupancy 1 / 2 x single / multi-step x the split settings of MULTI_CHECKS:
    (engine, spec, occ, multi, split_rays, builds of the call).  Occupancy 2 both ways it is reached: LL_SHARE_SIMDS at a tiny batch, and a grid beyond the SIMDs"""
    for name, engine, mode, spec in sm.launchable_cells():
        for split in {None} | {s for e, _, _, s in sm.MULTI_CHECKS if e == engine}:
            env = {} if split is None else {'LL_SPLIT_RAYS': int(split)}
            for occ, n_envs, env in ((1, 70, env), (2, 70, dict(env, LL_SHARE_SIMDS=1)), (2, 4 * SIMDS_HW + 2, dict(env, LL_SEPMC_ONE_WAVE=0))):
                caps = planner.caps(monkeypatch, **env)
                for multi in (False, True):
                    yield engine, spec, occ, multi, split, planner.call_builds(engine, spec, n_envs, 3 if multi else 1, caps)


def test_the_plan_yields_the_builds_the_table_expects(planner, monkeypatch):
    n = 0
    for engine, spec, occ, multi, split, builds in _table_grid(planner, monkeypatch):
        assert builds == sm.expected_builds(engine, spec, occ, multi, split_rays=split), (engine, spec, occ, multi, split)
        n += 1
    assert n >= 6 * len(list(sm.launchable_cells()))


def _rule(engine, spec, blocks, n_steps, scripted, caps):
    """the launch rule as it is written down (build, row scratch, steps per launch, ray kernel), from the caps: not from expected_builds, not from the header"""
    simds_hw, simds, epmc_simds, sepmc_simds, det, sr_epmc, sr_sepmc = caps
    cone = spec.get('friction_mode', 2) == 2
    if ENGINE_ID[engine] == 0:
        occ, obst, xrows = (1 if blocks <= simds else 2), engine == 'pmc_obst', spec.get('self_friction', 0) > 0
        single = bool(det) or (xrows and occ == 2) or not (blocks <= simds or blocks <= 2 * simds_hw)
        per = 1 if single else 128
        multi = min(n_steps, per) > 1
        if xrows:
            return dict(build=('pmc_step_kernel', occ, False, multi, True, True), row_scratch=occ == 2, per=per, split=False)
        return dict(build=('pmc_step_kernel', occ, obst, multi, cone, False), row_scratch=obst or (occ == 2 and cone), per=per, split=False)
    xrows = spec.get('self_friction', 0) > 0 or spec.get('leg_edges', 0) != 0
    if engine == 'sepmc':
        xrows = xrows or spec.get('pair_friction', 0) > 0 or spec.get('max_pair', 2) != 2
    occ = 1 if blocks <= (epmc_simds if engine == 'epmc' else sepmc_simds) else 2
    mode = sr_epmc if engine == 'epmc' else (2 if sr_sepmc == 1 and blocks > simds_hw else sr_sepmc)
    split = (not scripted) and (mode >= 1 if n_steps == 1 else mode >= 2)
    one_launch = not xrows and n_steps > 1 and occ == 1 and not split
    return dict(build=(engine + '_step_kernel', occ, False, one_launch, cone or xrows, xrows), row_scratch=True, per=n_steps if one_launch else 1, split=split)


CAPS_TABLE = [      # environment -> (simds, epmc_simds, sepmc_simds, deterministic, split_rays_epmc, split_rays_sepmc) on SIMDS_HW SIMDs
    ({}, (SIMDS_HW, SIMDS_HW, ONE_WAVE, 0, 2, 1)),
    (dict(LL_SHARE_SIMDS=1), (0, 0, 0, 0, 2, 1)),
    (dict(LL_SHARE_SIMDS=1, LL_SEPMC_ONE_WAVE=1, LL_EPMC_ONE_WAVE=1), (0, 0, 0, 0, 2, 1)),
    (dict(LL_DETERMINISTIC=1), (SIMDS_HW, SIMDS_HW, ONE_WAVE, 1, 2, 1)),
    (dict(LL_SEPMC_ONE_WAVE=0), (SIMDS_HW, SIMDS_HW, SIMDS_HW, 0, 2, 1)),
    (dict(LL_SEPMC_ONE_WAVE=1), (SIMDS_HW, SIMDS_HW, ONE_WAVE, 0, 2, 1)),
    (dict(LL_EPMC_ONE_WAVE=1), (SIMDS_HW, ONE_WAVE, ONE_WAVE, 0, 2, 1)),
    (dict(LL_SPLIT_RAYS=0), (SIMDS_HW, SIMDS_HW, ONE_WAVE, 0, 0, 0)),
    (dict(LL_SPLIT_RAYS=1), (SIMDS_HW, SIMDS_HW, ONE_WAVE, 0, 1, 1)),
    (dict(LL_SPLIT_RAYS=2), (SIMDS_HW, SIMDS_HW, ONE_WAVE, 0, 2, 2)),
    (dict(LL_SPLIT_RAYS=1, LL_SEPMC_ONE_WAVE=0), (SIMDS_HW, SIMDS_HW, SIMDS_HW, 0, 1, 1)),
]
CAPS_SPECS = {'pmc': ({}, dict(friction_mode=0), dict(self_friction=0.25)), 'pmc_obst': ({}, dict(friction_mode=0)), 'epmc': ({}, dict(friction_mode=0), dict(leg_edges=1)),
              'sepmc': ({}, dict(friction_mode=0), dict(max_pair=4))}
CAPS_BLOCKS = (SIMDS_HW, SIMDS_HW + 1, 2 * SIMDS_HW, 2 * SIMDS_HW + 1)      # both sides of one and of two waves per SIMD


def _caps_grid(planner, monkeypatch):
    for env, want in CAPS_TABLE:
        caps = planner.caps(monkeypatch, **env)
        assert caps == [SIMDS_HW] + list(want), env
        for engine, specs in CAPS_SPECS.items():
            for spec in specs:
                for blocks in CAPS_BLOCKS:
                    for n_envs in (4 * blocks - 2, 4 * blocks):              # a partial last wave, a full one
                        for n_steps in (1, 3, 129):
                            for scripted in (False, True) if ENGINE_ID[engine] and n_steps == 1 else (False,):
                                yield env, caps, engine, spec, blocks, n_envs, n_steps, scripted


def test_the_plan_under_every_cap(planner, monkeypatch):
    sepmc_mode2 = set()
    for env, caps, engine, spec, blocks, n_envs, n_steps, scripted in _caps_grid(planner, monkeypatch):
        at = (env, engine, spec, n_envs, n_steps, scripted)
        pl = planner.plan(engine, spec, n_envs, n_steps, caps, scripted)
        assert pl == _rule(engine, spec, blocks, n_steps, scripted, caps), at
        _, occ, obst, multi, cone, xrows = pl['build']
        assert not (multi and pl['per'] == 1) and not (pl['split'] and pl['per'] > 1) and not (scripted and pl['split']), at      # scripted rays never split
        if engine == 'pmc' and xrows and occ == 2:
            assert pl['per'] == 1 and not multi, at                                # PMC XROWS at occupancy 2 never plans a multi-step launch
        if ENGINE_ID[engine] == 0 and n_steps == 129 and pl['per'] > 1:           # 128 + 1: the remainder launch of one step runs the loop-free build
            builds = planner.call_builds(engine, spec, n_envs, n_steps, caps)
            assert builds == {pl['build'], pl['build'][:3] + (False,) + pl['build'][4:]} and pl['build'][3], at
        if engine == 'sepmc' and env == dict(LL_SPLIT_RAYS=1) and n_steps == 3:    # mode 1 (single steps split, multi-step calls fused) becomes 2 beyond simds_hw blocks
            sepmc_mode2.add((blocks, pl['split']))
    assert sepmc_mode2 == {(SIMDS_HW, False), (SIMDS_HW + 1, True), (2 * SIMDS_HW, True), (2 * SIMDS_HW + 1, True)}, sepmc_mode2


def _planned_builds(planner, monkeypatch):
    """every build the plan yields anywhere on the two grids above"""
    out = set().union(*(g[-1] for g in _table_grid(planner, monkeypatch)))
    for env, caps, engine, spec, blocks, n_envs, n_steps, scripted in _caps_grid(planner, monkeypatch):
        out |= planner.call_builds(engine, spec, n_envs, n_steps, caps, scripted)
    return out


def test_launch_plan_header_under_asan_ubsan(planner, monkeypatch):
    """csrc/launch_plan.hpp as a program of its own under AddressSanitizer + UndefinedBehaviorSanitizer (tests/emul/launch_plan_walk.cpp): plan_step over
    every point of the two grids, launch_caps_from_env under every environment of CAPS_TABLE: no report, and the answers the tests above hold the plain build to"""
    _planned_builds(planner, monkeypatch)
    emul = os.path.join(ROOT, 'tests', 'emul')
    subprocess.check_call(['make', '-C', emul, '-s', '_build/launch_plan_walk_asan'])
    points = planner.points
    grid = ''.join(' '.join(repr(v) for v in p) + '\n' for p, _ in points)
    for k, (env, want) in enumerate(CAPS_TABLE):
        clean = {name: v for name, v in os.environ.items() if name not in CAPS_ENV}
        out = subprocess.run([os.path.join(emul, '_build', 'launch_plan_walk_asan'), str(SIMDS_HW), '1'], input=grid if k == 0 else '', capture_output=True, text=True,
                             timeout=120, env={**clean, **{name: str(v) for name, v in env.items()}})
        assert out.returncode == 0 and not out.stderr, (env, out.returncode, out.stderr[-3000:])
        lines = [[int(v) for v in line.split()] for line in out.stdout.splitlines()]
        assert lines[0] == [SIMDS_HW] + list(want), env
        if k == 0:
            assert lines[1:] == [plan for _, plan in points] and len(points) > 3000


def test_a_build_the_host_has_no_instantiation_of_is_refused(planner):
    """HostBackend acts on a planned build or raises LL_ESTATE: the five (obst, cone, xrows) the kernel source is instantiated for, and no other"""
    from lifelike_agility_and_play_amd import capi
    have = {(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 1, 1)}
    for obst in (0, 1):
        for cone in (0, 1):
            for xrows in (0, 1):
                assert planner.lib.emu_host_build(obst, cone, xrows) == (0 if (obst, cone, xrows) in have else capi.LL_ESTATE), (obst, cone, xrows)


def test_every_step_kernel_build_is_claimed_by_the_table(planner, monkeypatch):
    shipped = _code_object_builds()
    assert len(shipped) == 35, sorted(shipped)                       # PMC 19, EPMC 8, SEPMC 8
    claimed = sm.claimed_builds()
    unclaimed = sorted(shipped - set(claimed))
    assert not unclaimed, ('step-kernel builds no row of tests/spec_matrix.py reaches', unclaimed)
    assert not sorted(set(claimed) - shipped), ('the table claims builds the code object does not have', sorted(set(claimed) - shipped))
    parity_only = {b for b, who in claimed.items() if any(n == 'multi' or sm.ROWS[n]['engines'][e][m] == sm.PARITY for n, e, m in who)}
    assert parity_only == shipped, sorted(shipped - parity_only)
    planned = _planned_builds(planner, monkeypatch)
    assert planned <= shipped, ('the launch plan yields builds the code object does not have', sorted(planned - shipped))
