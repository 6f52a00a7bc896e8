// play_host.hpp -- what the constructors of EpmcEngine and SepmcEngine (the two "play" engines over a PmcEngine) do alike, statement for
// statement.  ll_epmc_config and ll_sepmc_config name the fields read here the same, so each block is a template over the config type.
#pragma once
#include <string.h>

#include "epmc_step.hpp"
#include "pmc_engine.hpp"

// the ll_config of the PmcEngine underneath, n_rows robot rows
template <class CFG>
static ll_config play_base_config(const CFG& c, int n_rows) {
  ll_config b;
  memset(&b, 0, sizeof b);
  b.abi_version = LL_ABI_VERSION;
  b.n_envs = n_rows; b.device = c.device; b.auto_reset = c.auto_reset;
  b.control_freq = c.control_freq; b.sim_freq = 500.0;                   // PGE:82, CTG:53 time_step = 1/500, not configurable
  b.kp = c.kp; b.kd = c.kd; b.max_tau = c.max_tau;
  b.foot_lateral_friction = c.friction_range[0];                         // per-episode value travels in SubstepExtra
  for (int i = 0; i < 5; i++) { b.reward_weights[i] = 1.0; b.prop_order[i] = c.prop_order[i]; }
  b.solver_iterations = c.solver_iterations;
  b.seed = c.seed;
  return b;
}

// the episode length, push schedule and forces, friction and noise ranges of a zeroed EpmcParams
template <class CFG>
static void play_fill_params(EpmcParams& E, const CFG& c) {
  E.max_steps = c.max_steps;
  E.push_enabled = c.push_enabled ? 1 : 0; E.push_count0 = c.push_count0;
  E.push_interval_step = c.push_interval_step; E.push_duration_step = c.push_duration_step;
  E.friction_lo = (float)c.friction_range[0]; E.friction_hi = (float)c.friction_range[1];
  E.hforce_lo = (float)c.horizontal_force[0]; E.hforce_hi = (float)c.horizontal_force[1];
  E.vforce_lo = (float)c.vertical_force[0]; E.vforce_hi = (float)c.vertical_force[1];
  E.push_ratio = (float)c.push_strength_ratio; E.plane_friction = (float)LLM_PLANE_FRICTION;
  E.box_friction = 0.5f; E.terrain_contacts = 1;
  for (int i = 0; i < 4; i++) { E.noise_on[i] = c.noise_enabled[i] ? 1 : 0; E.noise_lo[i] = (float)c.noise_range[i][0]; E.noise_hi[i] = (float)c.noise_range[i][1]; }
}

// the start state as floats: into init[37] for the caller, and onto the device as E.init_state
template <class BK>
static void play_upload_init(PmcEngine<BK>& base, EpmcParams& E, const double* init37, float (&init)[37]) {
  for (int i = 0; i < 37; i++) init[i] = (float)init37[i];
  float* d_init = base.template dalloc<float>(37);
  base.bk.h2d(d_init, init, sizeof init);
  E.init_state = d_init;
}

// ENG::set_step_draws: uniforms for the draws of the next step only, one row of n_draws per env (EPMC) or arena (SEPMC)
template <class ENG>
static void play_set_step_draws(ENG& g, const float* h_draws, int n_draws, size_t draw_rows) {
  if (n_draws < 0) throw PmcError(LL_EINVAL, "negative draw count");
  g.ensure_script_buffers(n_draws);
  g.base.bk.sync();
  if (n_draws > 0) g.base.bk.h2d(g.d_scr_draws, h_draws, draw_rows * n_draws * 4);
  g.pending_step_draws = n_draws > 0 ? n_draws : -1;              // -1: the step must not draw at all
}
