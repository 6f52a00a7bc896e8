// launch_plan_walk.cpp -- TEST INFRASTRUCTURE.  csrc/launch_plan.hpp on its own, for the sanitizer build (make asan): reads the grid points
// tests/test_spec_matrix_emul.py walks, one per line in plan_point's argument order, and prints each point's plan8 -- after one line with the caps
// launch_caps_from_env reads from the environment the program was started in (argv: simds_hw, the LL_SEPMC_ONE_WAVE default).
#include <stdio.h>
#include <stdlib.h>

#include "plan_point.hpp"

int main(int argc, char** argv) {
  if (argc != 3) return 3;
  const LaunchCaps e = launch_caps_from_env(atoi(argv[1]), atoi(argv[2]) != 0);
  printf("%d %d %d %d %d %d %d\n", e.simds_hw, e.simds, e.epmc_simds, e.sepmc_simds, e.deterministic, e.split_rays_epmc, e.split_rays_sepmc);
  int engine, n_envs, n_steps, scripted, c[7], p[8];
  double s[6];
  while (scanf("%d %lf %lf %lf %lf %lf %lf %d %d %d %d %d %d %d %d %d %d", &engine, &s[0], &s[1], &s[2], &s[3], &s[4], &s[5], &n_envs, &n_steps, &scripted,
               &c[0], &c[1], &c[2], &c[3], &c[4], &c[5], &c[6]) == 17) {
    plan_point(engine, s, n_envs, n_steps, scripted, c, p);
    printf("%d %d %d %d %d %d %d %d\n", p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]);
  }
  return feof(stdin) ? 0 : 1;
}
