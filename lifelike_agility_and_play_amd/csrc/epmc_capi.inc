// epmc_capi.inc -- the extern "C" entry points of include/llenv_epmc.h over `EPMC_ENGINE` (an EpmcEngine<Backend>).
// Included after pmc_capi.inc (shares its error plumbing) by the translation unit that defines EPMC_ENGINE.
struct ll_epmc_engine {
  EPMC_ENGINE* e;
};
static const EpmcParams& ll_play(ll_epmc_engine* h) { return h->e->E; }

extern "C" {

int ll_epmc_create(const ll_epmc_config* cfg, const double* model_blob, int blob_len, const double* init_state37, ll_epmc_engine** out) { return ll_create_as(out, cfg, model_blob, blob_len, init_state37); }
int ll_epmc_destroy(ll_epmc_engine* h) { return ll_destroy_as(h); }
int ll_epmc_reset(ll_epmc_engine* h, const int32_t* env_ids, int n, const float* h_draws, const float* h_prev_orn) { return ll_reset_as(h, env_ids, n, h_draws, h_prev_orn); }
int ll_epmc_step(ll_epmc_engine* h, const float* d_actions) { return ll_step_as(h, d_actions); }
int ll_epmc_step_random_n(ll_epmc_engine* h, float sigma, int n_steps) { return ll_step_random_n_as(h, sigma, n_steps); }
int ll_epmc_kernel_time_stats(ll_epmc_engine* h, double* avg_launch_ms, int* n_launches, int64_t* n_control_steps) { return ll_kernel_time_stats_as(h, avg_launch_ms, n_launches, n_control_steps); }
int ll_epmc_set_actions(ll_epmc_engine* h, const float* h_actions) { return ll_set_actions_as(h, h_actions); }
int ll_epmc_step_scripted(ll_epmc_engine* h, const float* h_actions, const float* h_state, const uint8_t* h_ray_hit, const float* h_ray_frac,
                          const float* h_draws, int n_draws) {
  LL_TRY
  LL_CHECK(h && h_actions && h_state && h_ray_hit && h_ray_frac, "null argument");
  h->e->step_scripted(h_actions, h_state, h_ray_hit, h_ray_frac, h_draws, n_draws);
  LL_CATCH
}
int ll_epmc_set_step_draws(ll_epmc_engine* h, const float* h_draws, int n_draws) { return ll_set_step_draws_as(h, h_draws, n_draws); }
int ll_epmc_script_reset_rays(ll_epmc_engine* h, const uint8_t* h_ray_hit, const float* h_ray_frac) {
  LL_TRY
  LL_CHECK(h && h_ray_hit && h_ray_frac, "null argument");
  h->e->script_reset_rays(h_ray_hit, h_ray_frac);
  LL_CATCH
}
int ll_epmc_set_spec_param(ll_epmc_engine* h, int id, double value) { return ll_set_spec_param_as(h, id, value); }
int ll_epmc_get_spec_param(ll_epmc_engine* h, int id, double* value) { return ll_get_spec_param_as(h, id, value); }
int ll_epmc_sync(ll_epmc_engine* h) { return ll_sync_as(h); }
int ll_epmc_obs_dim(ll_epmc_engine* h) { return ll_obs_dim_as(h); }

int ll_epmc_get_obs(ll_epmc_engine* h, float* h_obs) { return ll_get_obs_as(h, h_obs); }
int ll_epmc_get_reward_done(ll_epmc_engine* h, float* h_reward, uint8_t* h_done, uint8_t* h_done_reason) { return ll_get_reward_done_as(h, h_reward, h_done, h_done_reason); }
int ll_epmc_get_state(ll_epmc_engine* h, float* h_state37) { return ll_get_state_as(h, h_state37); }
int ll_epmc_set_state(ll_epmc_engine* h, const float* h_state37) { return ll_set_state_as(h, h_state37); }
int ll_epmc_get_episode(ll_epmc_engine* h, float* h_rows19) {
  LL_TRY
  LL_CHECK(h && h_rows19, "null argument");
  const size_t N = h->e->base.P.n_envs;
  std::vector<float> ep(N * EPMC_EP_STRIDE);
  h->e->base.get_vec(h->e->E.ep, ep.data(), ep.size());
  static const int src[19] = {EP_TARGET, EP_TARGET + 1, EP_TARGET + 2, EP_TARGET_SPD, EP_FRICTION, EP_CMD_FREQ, EP_COUNTER, EP_PUSH_FORCE, EP_PUSH_FORCE + 1,
                              EP_PUSH_FORCE + 2, EP_NOISE, EP_NOISE + 1, EP_NOISE + 2, EP_NOISE + 3, EP_LAST_DIFF, EP_INIT_DIFF, EP_TOTAL_SPD, EP_MAX_SPD, EP_EPISODE};
  for (size_t e = 0; e < N; e++)
    for (int i = 0; i < 19; i++) h_rows19[e * 19 + i] = ep[e * EPMC_EP_STRIDE + src[i]];
  LL_CATCH
}
int ll_epmc_get_info(ll_epmc_engine* h, float* h_rows6) {
  LL_TRY
  LL_CHECK(h && h_rows6, "null argument");
  h->e->base.get_vec(h->e->E.info, h_rows6, (size_t)h->e->base.P.n_envs * 6);
  LL_CATCH
}
int ll_epmc_get_statics(ll_epmc_engine* h, float* h_rows, int32_t* h_count) {
  LL_TRY
  LL_CHECK(h && h_rows && h_count, "null argument");
  const size_t N = h->e->base.P.n_envs;
  h->e->base.get_vec(h->e->E.statics, h_rows, N * EPMC_MAX_STATICS * 8);
  std::vector<float> ep(N * EPMC_EP_STRIDE);
  h->e->base.get_vec(h->e->E.ep, ep.data(), ep.size());
  for (size_t e = 0; e < N; e++) h_count[e] = (int32_t)ep[e * EPMC_EP_STRIDE + EP_N_STATICS];
  LL_CATCH
}
int ll_epmc_get_rays(ll_epmc_engine* h, float* h_from, float* h_to, uint8_t* h_hit, float* h_frac) { return ll_get_rays_as(h, h_from, h_to, h_hit, h_frac, "the ray trace is kept for engines of at most 512 envs"); }
int ll_epmc_get_push_trace(ll_epmc_engine* h, float* h_rows, int32_t* n_sub) { return ll_get_push_trace_as(h, h_rows, n_sub); }
int ll_epmc_get_counters(ll_epmc_engine* h, uint64_t* steps, uint64_t* episodes, uint64_t* nonfinite) { return ll_get_counters_as(h, steps, episodes, nonfinite, 1); }
int ll_epmc_device_ptrs(ll_epmc_engine* h, ll_device_ptrs_t* out) { return ll_device_ptrs_as(h, out, false); }
int ll_epmc_enable_kernel_timing(ll_epmc_engine* h, int on) { return ll_enable_kernel_timing_as(h, on); }
int ll_epmc_kernel_time_ms(ll_epmc_engine* h, double* avg_ms, int* n) { return ll_kernel_time_ms_as(h, avg_ms, n); }
int ll_epmc_fill_random_actions(ll_epmc_engine* h, float sigma) { return ll_fill_random_actions_as(h, sigma); }

}  // extern "C"
