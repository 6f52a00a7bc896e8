"""One table of the physics spec's run-time switches (include/llenv_model.h LLM_SPEC_*): for every switch, which engines honour it, under which
friction mode, at which value it binds in a short random-policy run, and which step-kernel builds a run with it reaches.  Both matrix modules
(test_spec_matrix_emul.py on the host build of the kernel source, test_gpu_spec_matrix.py on the HIP library) and the build-coverage check read it.

Outcomes, per engine and friction mode (LLM_SPEC_FRICTION_MODE 0 = the pyramid, 2 = the cone, the default):
  PARITY   the engine accepts the value, a run at it differs from a run at the default, and it matches the oracle under the same switches
  INERT    the engine accepts the value but has nothing it acts on (the robot-robot rows outside SEPMC, the terrain edges on flat ground): a run at it
           equals the run at the default bit for bit, and it reaches the default build
  REFUSED  setting the value succeeds, the next step fails with LL_EINVAL naming the switch, before anything is launched
  ORACLE   the switch exists in the oracle only: the engine refuses every value but the default at set time
"""
import re

PARITY, INERT, REFUSED, ORACLE = 'parity', 'inert', 'refused', 'oracle-only'
ENGINES = ('pmc', 'pmc_obst', 'epmc', 'sepmc')          # pmc_obst: PMC with set_obstacle (the jump clips)
MODES = (0, 2)


def _all(outcome):
    return {e: {m: outcome for m in MODES} for e in ENGINES}


def _cone_only(**per_engine):
    """the switch has rows only in the XROWS builds, which exist with the cone: the pyramid refuses it wherever it would act"""
    out = {}
    for e in ENGINES:
        o = per_engine.get(e, PARITY)
        out[e] = {0: REFUSED if o == PARITY else o, 2: o}
    return out


# name: LLM_SPEC_* id, the non-default values, `base`: switches set on both sides of the binding comparison (a switch that only acts together with
# another one), `xrows`: a PARITY run with it reaches the XROWS build of the engines listed
ROWS = {
    'limit_gate':           dict(id=0, values=(0.5,), base=dict(limit_speculative=1), engines=_all(PARITY)),
    'max_depen_speed':      dict(id=1, values=(0.05,), engines=_all(PARITY)),
    'link_damping':         dict(id=2, values=(0.5,), engines=_all(PARITY)),
    'max_contacts_per_leg': dict(id=3, values=(1,), engines=_all(PARITY)),
    'self_collision':       dict(id=4, values=(0,), engines=_all(PARITY)),
    'self_margin':          dict(id=5, values=(0.05,), engines=_all(PARITY)),
    'max_self':             dict(id=6, values=(0,), base=dict(self_collision=1), engines=_all(PARITY)),
    'erp':                  dict(id=7, values=(0.3,), engines=_all(PARITY)),
    'contact_margin':       dict(id=8, values=(0.05,), engines=dict(_all(PARITY), pmc_obst={0: REFUSED, 2: REFUSED}, sepmc={0: REFUSED, 2: REFUSED})),
    'self_friction':        dict(id=9, values=(0.25,), xrows=('pmc', 'epmc', 'sepmc'), engines=_cone_only(pmc_obst=REFUSED)),
    'warm_start':           dict(id=10, values=(0.5,), engines=_all(ORACLE)),
    'trunk_edges':          dict(id=11, values=(0,), engines=_all(ORACLE)),
    'select_eps':           dict(id=12, values=(1e-3,), engines=_all(ORACLE)),
    'friction_mode':        dict(id=13, values=(0,), engines=_all(PARITY)),
    'row_order':            dict(id=14, values=(1,), engines=_all(ORACLE)),
    'max_coord_vel':        dict(id=15, values=(2.0,), engines=_all(PARITY)),
    'limit_erp':            dict(id=16, values=(0.6,), engines=dict(_all(PARITY), pmc_obst={0: REFUSED, 2: PARITY})),
    'pair_friction':        dict(id=17, values=(0.25,), xrows=('sepmc',), engines=_cone_only(pmc=INERT, pmc_obst=INERT, epmc=INERT)),
    'max_pair':             dict(id=18, values=(4,), xrows=('sepmc',), engines=_cone_only(pmc=INERT, pmc_obst=INERT, epmc=INERT)),
    'friction_dirs':        dict(id=19, values=(1,), engines=_all(PARITY)),
    'limit_speculative':    dict(id=20, values=(1,), engines=_all(PARITY)),
    'gyro':                 dict(id=21, values=(0,), engines=_all(ORACLE)),
    'friction_keep':        dict(id=22, values=(1,), engines=_all(ORACLE)),
    'erp_deep':             dict(id=23, values=(0.02,), base=dict(erp_deep_below=-0.002), engines=_all(PARITY)),
    'erp_deep_below':       dict(id=24, values=(-0.002,), base=dict(erp_deep=0.02), engines=_all(PARITY)),
    'limit_erp_deep':       dict(id=25, values=(0.5,), base=dict(erp_deep_below=-0.002), engines=_all(PARITY)),
    'leg_edges':            dict(id=26, values=(1,), xrows=('epmc', 'sepmc'), engines=_cone_only(pmc=INERT, pmc_obst=REFUSED)),
}
# (row, engine) pairs whose value cannot bind in check_binding's short run from the reset poses -- a leg box must lie across a terrain edge -- so the
# binding evidence is the parity comparator's own: check_legs_on_edges_against_oracle places the robots so and asserts that the rows were felt.
BOUND_IN_COMPARATOR = {('leg_edges', 'epmc')}
# values the engine cannot honour at all: refused at set time on every engine, whatever the friction mode
BAD_VALUES = {
    'max_contacts_per_leg': (0, 5, 2.5), 'max_self': (-1, 3, 0.5), 'max_pair': (-1, 5, 2.5), 'self_friction': (-0.1, 4.5), 'pair_friction': (-0.1, 4.5),
    'friction_mode': (1, 3), 'limit_speculative': (0.5, 2), 'leg_edges': (0.5, 2), 'friction_dirs': (2,), 'max_coord_vel': (0.0, -1.0),
}
# switches left out of the all-scalars leg: the ones that change the build (they have legs of their own), friction_dirs (its own documented bars at
# the rule's discontinuity), and self_collision (max_self = 0 already takes the leg-leg rows out; self_collision = 0 would make max_self moot)
NOT_SCALAR = ('friction_mode', 'self_friction', 'pair_friction', 'max_pair', 'leg_edges', 'friction_dirs', 'self_collision')


def all_scalars(engine, mode=2):
    """every scalar switch that is PARITY on `engine`, moved together to its binding value: the leg that runs them in the 256-register build too"""
    out = {}
    for name, row in ROWS.items():
        if name not in NOT_SCALAR and row['engines'][engine][mode] == PARITY:
            out.update(spec_of(name, row['values'][0]))
    return out


def spec_of(name, value):
    """the switches a run of row `name` at `value` sets (its base first)"""
    row = ROWS[name]
    return {**row.get('base', {}), name: value}


def header_spec_ids(path):
    """LLM_SPEC_* name -> id, and LLM_SPEC_COUNT, parsed from include/llenv_model.h"""
    ids = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r'#define\s+LLM_SPEC_(\w+)\s+(\d+)', open(path).read())}
    return ids, ids.pop('count')


# ---- the step-kernel builds: an independent restatement of csrc/launch_plan.hpp, held to it by test_spec_matrix_emul.py --------------------------------------
# A build is (kernel, OCC, OBST, MULTI, CONE, XROWS); EPMC and SEPMC have no OBST argument (False here).  OCC 1: one wave per SIMD (n <= 4096 envs on the
# MI355X's 1024 SIMDs), OCC 2: the 256-register build of larger batches.

def expected_builds(engine, spec, occ, multi, split_rays=None):
    """the builds one step call reaches: `multi` a multi-step call (ll_*_step_random_n), `spec` the switches that differ from the default;
    `split_rays`: a multi-step call with the rays split off runs as single launches (LL_SPLIT_RAYS; None: the engine's default -- EPMC 2, split;
    SEPMC 1, fused within one wave per SIMD)"""
    if split_rays is None:
        split_rays = engine == 'epmc'
    cone = int(spec.get('friction_mode', 2)) == 2
    if engine in ('pmc', 'pmc_obst'):
        obst = engine == 'pmc_obst'
        if spec.get('self_friction', 0) > 0:                     # (beyond one wave per SIMD a multi-step call runs as single launches)
            return {('pmc_step_kernel', occ, False, multi and occ == 1, True, True)}
        return {('pmc_step_kernel', occ, obst, multi, cone, False)}
    kernel = engine + '_step_kernel'
    xr = spec.get('self_friction', 0) > 0 or spec.get('leg_edges', 0) != 0
    if engine == 'sepmc':
        xr = xr or spec.get('pair_friction', 0) > 0 or spec.get('max_pair', 2) != 2
    if xr:
        return {(kernel, occ, False, False, True, True)}          # every step a launch of its own
    if multi and occ == 1 and not split_rays:
        return {(kernel, 1, False, True, cone, False)}
    return {(kernel, occ, False, False, cone, False)}              # larger multi-step batches, and those with the rays split, run as single launches


# The multi-step legs test_gpu_spec_matrix.py runs (check_multi_step_launch: k steps in one launch == k single launches, bit for bit): engine,
# switches, (occupancies), split_rays.  The EPMC check sets LL_SPLIT_RAYS=0, the setting under which its MULTI builds run; SEPMC's runs its default.
MULTI_CHECKS = [(e, dict(friction_mode=m), (1, 2) if e in ('pmc', 'pmc_obst') else (1,), False if e == 'epmc' else None) for e in ENGINES for m in MODES] + \
               [('pmc', dict(self_friction=0.25), (1, 2), False)]


def launchable_cells():
    """(row, engine, mode, spec) of every PARITY / INERT cell: the runs the table has that launch something"""
    for name, row in ROWS.items():
        for engine, modes in row['engines'].items():
            for mode, outcome in modes.items():
                if outcome in (PARITY, INERT):
                    yield name, engine, mode, ({**spec_of(name, row['values'][0]), 'friction_mode': mode} if name != 'friction_mode' else {'friction_mode': row['values'][0]})


def claimed_builds():
    """every build a check of the table reaches: the single-step builds of each PARITY / INERT cell at either occupancy (the parity comparators
    step one launch at a time), and the builds of the multi-step legs (MULTI_CHECKS).  build -> [(row or 'multi', engine, mode)]"""
    out = {}
    for name, engine, mode, spec in launchable_cells():
        for occ in (1, 2):
            for b in expected_builds(engine, spec, occ, False):
                out.setdefault(b, []).append((name, engine, mode))
    for engine, spec, occs, split in MULTI_CHECKS:
        for occ in occs:
            for b in expected_builds(engine, spec, occ, True, split_rays=split):
                out.setdefault(b, []).append(('multi', engine, int(spec.get('friction_mode', 2))))
    return out


_TEMPLATE_ARGS = re.compile(r'^(pmc_step_kernel|epmc_step_kernel|sepmc_step_kernel)<(.*)>\(')


def build_of_symbol(demangled):
    """'pmc_step_kernel<1, true, false, true, false>(StepParams)' -> ('pmc_step_kernel', 1, True, False, True, False); None for any other kernel"""
    m = _TEMPLATE_ARGS.match(demangled)
    if not m:
        return None
    args = [a.strip() for a in m.group(2).split(',')]
    vals = [int(args[0])] + [a == 'true' for a in args[1:]]
    if m.group(1) == 'pmc_step_kernel':
        occ, obst, multi, cone, xrows = (vals + [False] * 5)[:5]
    else:
        occ, multi, cone, xrows = (vals + [False] * 4)[:4]
        obst = False
    return (m.group(1), occ, obst, multi, cone, xrows)
