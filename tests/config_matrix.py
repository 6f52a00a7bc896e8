"""One table of the env_config fields the step kernels read at run time (csrc/pmc_tables.hpp pmc_fill_params: n_sub, dt, n_iter, kp, kd, max_tau,
mu_foot, rw[5], prop_off[5] / prop_dim / obs_dim, policy_step): for every field the values a run is held to the oracle at, the engines that take it,
and what a run at it must be next to a run at the training scripts' point -- the one point every other engine-vs-oracle comparison of the suite runs
at (control_freq 50, sim_freq 500, kp 50, kd 0.5, max_tau 18 / 16, foot_lateral_friction 0.5, solver_iterations 10, the five-key prop_type, the
training reward weights).  Both matrix modules (test_config_matrix_emul.py on the host build of the kernel source, test_gpu_config_matrix.py on the
HIP library) read it.

Kinds:
  MOVES_STATE  the field acts on the physics or the clock: engine-vs-oracle parity at the value, and a short random-policy run must DIFFER from
               the run at the default point
  SAME_STATE   the field acts on one output only (`output`: 'obs' for a prop_type layout, 'reward' for reward_weights): state, ghost, done and
               bookkeeping are bit-identical to the default run; the observation is the exact column gather of the default run's observation, the
               reward matches the oracle's given the engine's own state and differs from the default run's

Keys of a row's `cfg` are those of capi.make_config for the PMC engines; for EPMC and SEPMC they are the keys of the env_config dict
(`friction_range` goes into its env_randomize_config, `solver_iterations` to make_*_config): epmc_parity_common.cfg_variant.
"""
import spec_matrix as sm

MOVES_STATE, SAME_STATE = 'moves-state', 'same-state'
ENGINES = sm.ENGINES                                   # pmc, pmc_obst (PMC with set_obstacle), epmc, sepmc
PMC, ARENA = ('pmc', 'pmc_obst'), ('epmc', 'sepmc')
PROP_SIZES = {'joint_pos': 12, 'joint_vel': 12, 'root_lin_vel_loc': 3, 'root_ang_vel_loc': 3, 'e_g': 3}   # PLE:102-108
DEFAULT_PROP = ['joint_pos', 'joint_vel', 'root_ang_vel_loc', 'root_lin_vel_loc', 'e_g']                  # the training scripts' list (conftest.PMC_PROP_TYPE)

ROWS = {
    # ---- the clock: substeps per control step (PLE:52), policy_step (mocap lookup, margin, max_steps) ---------------------------------------------
    'control_freq_25':      dict(kind=MOVES_STATE, engines=ENGINES, cfg=dict(control_freq=25.0)),            # 20 substeps
    'control_freq_100':     dict(kind=MOVES_STATE, engines=ENGINES, cfg=dict(control_freq=100.0)),           # 5
    'control_freq_30':      dict(kind=MOVES_STATE, engines=ENGINES, cfg=dict(control_freq=30.0)),            # 16: policy_step is no multiple of dt
    'sim_freq_1000':        dict(kind=MOVES_STATE, engines=PMC, cfg=dict(sim_freq=1000.0)),                  # (EPMC and SEPMC fix 500: PGE:82, CTG:53)
    # ---- the PD law (LR:137-141) ---------------------------------------------------------------------------------------------------------------
    'pd_soft':              dict(kind=MOVES_STATE, engines=ENGINES, cfg=dict(kp=30.0, kd=0.2, max_tau=8.0)),
    'kd_1':                 dict(kind=MOVES_STATE, engines=ENGINES, cfg=dict(kd=1.0)),
    # ---- foot friction (LR:304-308) --------------------------------------------------------------------------------------------------------------
    'foot_friction_1':      dict(kind=MOVES_STATE, engines=PMC, cfg=dict(foot_lateral_friction=1.0)),
    'friction_range_1':     dict(kind=MOVES_STATE, engines=ARENA, cfg=dict(friction_range=[1.0, 1.0])),
    # ---- the solver loop (LR:261) ----------------------------------------------------------------------------------------------------------------
    'solver_iterations_4':  dict(kind=MOVES_STATE, engines=ENGINES, cfg=dict(solver_iterations=4)),
    'solver_iterations_25': dict(kind=MOVES_STATE, engines=ENGINES, cfg=dict(solver_iterations=25)),
    # ---- the factories' own defaults (create_pybullet_envs.py:28-59 for PMC: 25 Hz, kd 1.0, PLE's reward weights, uniform sampling; CTG:57 and
    #      create_pybullet_envs.py:104-140 for chase tag: 25 Hz, kd 1.0, max_tau 18) ----------------------------------------------------------------
    'factory_defaults':     dict(kind=MOVES_STATE, engines=('pmc', 'pmc_obst', 'sepmc'),
                                 cfg=dict(control_freq=25.0, kd=1.0, reward_weights=None, prioritized_sample_factor=0.0),
                                 cfg_by_engine=dict(sepmc=dict(control_freq=25.0, kd=1.0, max_tau=18.0))),
    # ---- prop_type layouts (PLE:101-121): obs_dim 117, 153, 153, 207, 198 -------------------------------------------------------------------------------
    'prop_e_g':             dict(kind=SAME_STATE, output='obs', engines=ENGINES, cfg=dict(prop_type=['e_g'])),
    'prop_e_g_joint_pos':   dict(kind=SAME_STATE, output='obs', engines=ENGINES, cfg=dict(prop_type=['e_g', 'joint_pos'])),
    'prop_vel_only':        dict(kind=SAME_STATE, output='obs', engines=ENGINES, cfg=dict(prop_type=['joint_vel', 'root_lin_vel_loc'])),
    'prop_permuted':        dict(kind=SAME_STATE, output='obs', engines=ENGINES,
                                 cfg=dict(prop_type=['root_lin_vel_loc', 'e_g', 'joint_vel', 'joint_pos', 'root_ang_vel_loc'])),
    'prop_subset_of_four':  dict(kind=SAME_STATE, output='obs', engines=ENGINES,            # (two keys of each size, out of order: 198)
                                 cfg=dict(prop_type=['root_ang_vel_loc', 'joint_vel', 'e_g', 'joint_pos'])),
    # ---- reward weights (PLE:352-370; the PMC reward: EPMC and SEPMC have rewards of their own without weights) ------------------------------------
    'reward_not_unit_sum':  dict(kind=SAME_STATE, output='reward', engines=PMC,
                                 cfg=dict(reward_weights={'joint_pos': 1.0, 'joint_vel': 0.5, 'end_effector': 2.0, 'root_pose': 0.25, 'root_vel': 0.25})),
    'reward_one_zero':      dict(kind=SAME_STATE, output='reward', engines=PMC,
                                 cfg=dict(reward_weights={'joint_pos': 0.4, 'joint_vel': 0.1, 'end_effector': 0.3, 'root_pose': 0.0, 'root_vel': 0.2})),
    # ---- several fields together -------------------------------------------------------------------------------------------------------------------
    'combo_25hz':           dict(kind=MOVES_STATE, engines=ENGINES, cfg=dict(control_freq=25.0, kd=1.0, prop_type=['e_g', 'joint_pos'], solver_iterations=4)),
    'combo_30hz':           dict(kind=MOVES_STATE, engines=ENGINES, cfg=dict(control_freq=30.0, prop_type=['e_g'])),
}
COMBINATION_ROWS = ('combo_25hz', 'combo_30hz')
# the rows that also run in the 256-register builds (the larger-batch kernels: other register budgets, the cone scalars through LDS)
BIG_ROWS = COMBINATION_ROWS + ('factory_defaults',)

# Values refused at create time with LL_EINVAL and a message (pmc_fill_params).  `poke`: written into the config struct behind the Python
# binding's own argument checks, which would raise first.  engines: who takes the field.
BAD_VALUES = [
    dict(label='control_freq 0', engines=ENGINES, cfg=dict(control_freq=0.0), text='control_freq'),
    dict(label='control_freq < 0', engines=ENGINES, cfg=dict(control_freq=-50.0), text='control_freq'),
    dict(label='control_freq NaN', engines=ENGINES, cfg=dict(control_freq=float('nan')), text='control_freq'),
    dict(label='sim_freq < control_freq', engines=PMC, cfg=dict(sim_freq=40.0, control_freq=50.0), text='sim_freq'),
    dict(label='control_freq above the fixed sim_freq', engines=ARENA, cfg=dict(control_freq=600.0), text='sim_freq'),
    dict(label='sim_freq 0', engines=PMC, cfg=dict(sim_freq=0.0), text='sim_freq'),
    dict(label='empty prop_type', engines=ENGINES, cfg=dict(prop_type=[]), text='prop_type'),
    dict(label='duplicate prop_type', engines=ENGINES, poke=dict(prop_order=[4, 0, 4, -1, -1]), text='prop_order'),
    dict(label='prop id out of range', engines=ENGINES, poke=dict(prop_order=[0, 7, -1, -1, -1]), text='prop_order'),
    dict(label='reward weights sum to 0', engines=PMC,
         cfg=dict(reward_weights={'joint_pos': 0.0, 'joint_vel': 0.0, 'end_effector': 0.0, 'root_pose': 0.0, 'root_vel': 0.0}), text='reward_weights'),
    dict(label='reward weights sum below 0', engines=PMC,
         cfg=dict(reward_weights={'joint_pos': 0.3, 'joint_vel': 0.05, 'end_effector': 0.1, 'root_pose': -0.5, 'root_vel': 0.05}), text='reward_weights'),
]

# Case-set seeds of the EPMC / SEPMC one-step comparators (check_terrain_physics_against_oracle, check_pair_physics_against_oracle).  Chosen so that the
# host build needs no ill-conditioning allowance at any row -- never to fit an error:
#  * SEPMC's default set (seed 5) leaves two arenas in robot-robot touch at the last of 20 or 16 substeps, and the comparator's own power
#    assertion asks for three; set 6 has four or five at every row.
#  * EPMC set 11 holds one case at 25 solver iterations in which a contact makes or breaks on the last bit: one float32 ulp on the start joint
#    angles moves the ORACLE's own result by 5e-4, which the comparator's conditioning measure (rounding between substeps only) does not see.
SEEDS = {'epmc': 11, 'sepmc': 6}
SEED_OF_ROW = {('solver_iterations_25', 'epmc'): 12}


def seed_of(name, engine):
    return SEED_OF_ROW.get((name, engine), SEEDS[engine])


def cfg_of(name, engine):
    """the env_config fields a run of row `name` sets on `engine`"""
    row = ROWS[name]
    assert engine in row['engines'], (name, engine)
    return dict(row.get('cfg_by_engine', {}).get(engine, row['cfg']))


def rows_of(engine, kind=None):
    return [name for name, row in ROWS.items() if engine in row['engines'] and (kind is None or row['kind'] == kind)]


def n_sub_of(cfg):
    """substeps of one control step under `cfg` (PLE:52: int(policy_step / dt), in double precision as the engines and the oracle evaluate it)"""
    return int((1.0 / float(cfg.get('control_freq', 50.0))) / (1.0 / float(cfg.get('sim_freq', 500.0))))


def prop_dim_of(prop_type):
    return sum(PROP_SIZES[k] for k in prop_type)


def gather_columns(prop_type, tail):
    """columns of the DEFAULT run's observation (3 stacked frames of DEFAULT_PROP | `tail` further entries that do not depend on prop_type:
    prop_a and future for PMC, prop_a and the perception for EPMC and SEPMC) that make up the observation under `prop_type`, in order"""
    off, o = {}, 0
    for k in DEFAULT_PROP:
        off[k] = o
        o += PROP_SIZES[k]
    cols = [f * o + off[k] + j for f in range(3) for k in prop_type for j in range(PROP_SIZES[k])]
    return cols + list(range(3 * o, 3 * o + tail))
