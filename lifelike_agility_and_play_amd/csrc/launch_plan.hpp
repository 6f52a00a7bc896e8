// launch_plan.hpp -- which step-kernel build a step call runs, how the call is cut into launches, how much LDS a launch gets and whether the ray kernel follows it: ONE rule, in plain host C++,
// that every backend acts on (llenv.hip HipBackend, tests/emul HostBackend) and PmcEngine::step cuts its calls by.  tests/spec_matrix.py expected_builds restates it; test_spec_matrix_emul.py holds the two together.
#pragma once
#include <stdlib.h>
#include "lanes.hpp"           // (LL_HD, which pmc_params.hpp is written with)
#include "pmc_tables.hpp"      // StepParams, LL_ENGINE_*, pmc_launch_xrows
struct LaunchCaps {                       // what a backend knows about its device and was told through the environment (launch_caps_from_env)
  int simds_hw, simds, epmc_simds, sepmc_simds;   // SIMDs of the device (four per compute unit); grids of at most so many workgroups run the one-wave-per-SIMD (512-register) builds of PMC / EPMC / SEPMC
  bool deterministic;                     // multi-step PMC calls run as single launches
  int split_rays_epmc, split_rays_sepmc;  // LL_SPLIT_RAYS mode per engine
};
inline bool launch_env_is_1(const char* name, bool unset = false) { const char* v = getenv(name); return v ? v[0] == '1' : unset; }
inline LaunchCaps launch_caps_from_env(int simds_hw, bool sepmc_one_wave_default) {
  LaunchCaps c;
  // LL_SHARE_SIMDS=1: always launch the 256-register builds, also when the grid would fit one 512-register wavefront per SIMD.  A
  // wavefront of the one-wave-per-SIMD builds owns its SIMD's whole register file, so any other kernel that is resident at the same
  // time -- RCCL's gather on the learner rank -- DISPLACES step-kernel waves instead of sharing SIMDs with them, and the step launch
  // ends later by the full residency of that kernel (measured with an RCCL stand-in: profiles/r03_simd_sharing.txt).
  c.simds_hw = simds_hw; c.simds = launch_env_is_1("LL_SHARE_SIMDS") ? 0 : simds_hw;
  // LL_SEPMC_ONE_WAVE (default 1): which chase-tag build runs batches beyond one wave per SIMD.  1: the one-wave-per-SIMD build at EVERY size -- a grid of 16 x the chip's SIMDs runs as
  // waves that follow each other on a SIMD without waiting for a step's slowest wave, and none of them spills (the 256-register chase-tag build carries 868 B of scratch per lane):
  // 32768 arenas 5.18 -> 4.37 ms per step, 8192 arenas 1.45 -> 1.16, 4096 arenas 0.80 -> 0.61 (profiles/r06_sepmc_one_wave_ab.txt).  0: the 256-register build, two waves per SIMD
  // (rounds 2 - 5; still what LL_SHARE_SIMDS=1 selects).  PMC and EPMC keep their 256-register builds for larger batches: those do not spill and win there.
  c.sepmc_simds = (c.simds != 0 && launch_env_is_1("LL_SEPMC_ONE_WAVE", sepmc_one_wave_default)) ? 0x7fffffff : c.simds;
  // LL_EPMC_ONE_WAVE: the same choice for the PlayGround env (default 0: its 256-register build does not spill and wins at larger batches)
  c.epmc_simds = (c.simds != 0 && launch_env_is_1("LL_EPMC_ONE_WAVE")) ? 0x7fffffff : c.simds;
  // LL_DETERMINISTIC=1: multi-step calls run as single launches.  A multi-step launch equals k single launches bit for bit only while every one of its waves is on the chip
  // (ll_get_table_sync == 0); on a device it shares with other kernels -- a collective, other ranks -- a re-seed may have to take the newest table version there is, and which clip it
  // draws then hangs on timing.  Single launches never do.
  c.deterministic = launch_env_is_1("LL_DETERMINISTIC");
  // LL_SPLIT_RAYS (EPMC / SEPMC): 0 = the step kernel casts the 778 rays of a row itself (rounds 1 - 5); 1 = single-step launches leave them to epmc_percept_kernel behind the step
  // kernel; 2 = multi-step calls too run as single steps, each followed by the ray kernel.  Defaults by the A/B on one box (profiles/r06_split_rays_ab.txt): EPMC 2 (hurdles: single steps
  // 0.2983 -> 0.2905 ms, 32-step calls 0.2894 -> 0.2898; cube stairs 0.3163 -> 0.2937), SEPMC 1 (single steps 0.3341 -> 0.3308; 32-step calls would lose 4 %: 0.3153 -> 0.3286)
  const char* sr = getenv("LL_SPLIT_RAYS"); c.split_rays_epmc = sr ? atoi(sr) : 2; c.split_rays_sepmc = sr ? atoi(sr) : 1;
  return c;
}
// One instantiation of a step kernel (llenv.hip pmc_step_kernel: OCC, OBST, MULTI, CONE, XROWS; the EPMC / SEPMC kernels have no OBST).
struct StepBuild {
  int occ; bool obst, multi, cone, xrows;
  int index() const { return (occ - 1) | obst << 1 | multi << 2 | cone << 3 | xrows << 4; }      // into a table of kCount kernels
  static constexpr int kCount = 32;
};
struct StepPlan {
  int blocks;             // workgroups of a launch: one wave of PMC_ENVS_PER_WAVE envs each
  StepBuild build;        // of a launch that carries min(n_steps, steps_per_launch) control steps
  bool row_scratch;       // the launch gets the per-row scratch in LDS on top of the constant tables
  int steps_per_launch;   // control steps one launch of the call carries at most; 1: every step a launch of its own (n_steps = 1, step_count advancing by one each)
  bool percept;           // epmc_percept_kernel follows each launch (EpmcParams::split_rays is set to it); only ever with single steps
};
inline StepPlan plan_step(int engine, const StepParams& P, bool scripted_rays, const LaunchCaps& c) {
  const int blocks = (P.n_envs + PMC_ENVS_PER_WAVE - 1) / PMC_ENVS_PER_WAVE;
  const bool cone = P.friction_mode == 2, xrows = pmc_launch_xrows(P, engine);      // (an XROWS launch under the pyramid has been refused: pmc_launch_refusal)
  StepPlan p = {blocks, {}, true, 1, false};
  if (engine == LL_ENGINE_PMC) {
    const int occ = blocks <= c.simds ? 1 : 2;
    // A multi-step launch needs every workgroup on the chip at once -- its waves wait for each other's finished episodes -- one 512-register wave per SIMD while
    // the grid fits, two 256-register waves otherwise.  The XROWS builds run multi-step calls in one launch only within one wave per SIMD (the 256-register
    // multi-step XROWS build once returned near-3e38 entries for one env of 4352 where single launches were finite; it is not built).
    const bool single = c.deterministic || (xrows && occ == 2) || !(occ == 1 || blocks <= 2LL * c.simds_hw);
    p.steps_per_launch = single ? 1 : LL_MAX_STEPS_PER_LAUNCH;      // (the per-step slots of the sampling table)
    p.build = xrows ? StepBuild{occ, false, false, true, true} : StepBuild{occ, P.set_obstacle != 0, false, cone, false};
    p.row_scratch = xrows ? occ == 2 : (P.set_obstacle || (occ == 2 && cone));      // (occ 2 with the cone: WithConeInLds)
  } else {
    const bool sepmc = engine == LL_ENGINE_SEPMC;
    const int occ = blocks <= (sepmc ? c.sepmc_simds : c.epmc_simds) ? 1 : 2;
    // (SEPMC beyond one wave per SIMD: a multi-step call is better off as single steps with the rays split off: 32768 arenas 4.52 -> 4.37 ms per step, profiles/r06_sepmc_one_wave_ab.txt)
    const int mode = !sepmc ? c.split_rays_epmc : (c.split_rays_sepmc == 1 && blocks > c.simds_hw) ? 2 : c.split_rays_sepmc;
    // the rays of the step's observation by the kernel of their own?  Not when the caller plays rayTestBatch (scripted rays) -- and a multi-step call only under LL_SPLIT_RAYS=2, as single steps
    p.percept = !scripted_rays && (P.n_steps == 1 ? mode >= 1 : mode >= 2);
    // the MULTI builds exist without XROWS at one wave per SIMD only (llenv.hip epmc_step_kernel); every other multi-step call runs its steps as single launches
    p.steps_per_launch = (!xrows && occ == 1 && !p.percept) ? P.n_steps : 1;
    p.build = StepBuild{occ, false, false, cone || xrows, xrows};
  }
  p.build.multi = P.n_steps > 1 && p.steps_per_launch > 1;      // a launch of one step, a call's remainder included, runs the loop-free build
  return p;
}
