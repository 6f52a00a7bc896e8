// plan_point.hpp -- TEST INFRASTRUCTURE.  csrc/launch_plan.hpp's answer for one step call under explicit caps, without an engine: the handful of StepParams
// fields the plan reads.  spec6 = set_obstacle, friction_mode, self_friction, pair_friction, max_pair, leg_edges; caps7 = the fields of LaunchCaps in their
// order; plan8 = occ, obst, multi, cone, xrows, row_scratch, steps_per_launch, percept.  Shared by emul.cpp (emu_step_plan) and launch_plan_walk.cpp.
#pragma once
#include <string.h>

#include "../../lifelike_agility_and_play_amd/csrc/launch_plan.hpp"

inline void plan_point(int engine, const double* spec6, int n_envs, int n_steps, int scripted_rays, const int* caps7, int* plan8) {
  StepParams P;
  memset(&P, 0, sizeof P);
  P.n_envs = n_envs; P.n_steps = n_steps;
  P.set_obstacle = (int)spec6[0]; P.friction_mode = (int)spec6[1]; P.self_friction = (float)spec6[2];
  P.pair_friction = (float)spec6[3]; P.max_pair = (int)spec6[4]; P.leg_edges = (int)spec6[5];
  const StepPlan p = plan_step(engine, P, scripted_rays != 0, LaunchCaps{caps7[0], caps7[1], caps7[2], caps7[3], caps7[4] != 0, caps7[5], caps7[6]});
  const int out[8] = {p.build.occ, p.build.obst, p.build.multi, p.build.cone, p.build.xrows, p.row_scratch, p.steps_per_launch, p.percept};
  memcpy(plan8, out, sizeof out);
}
