// sepmc_capi.inc -- the extern "C" entry points of include/llenv_sepmc.h over `SEPMC_ENGINE` (a SepmcEngine<Backend>).
// Included after pmc_capi.inc (shares its error plumbing) by the translation unit that defines SEPMC_ENGINE.
struct ll_sepmc_engine {
  SEPMC_ENGINE* e;
};
static const EpmcParams& ll_play(ll_sepmc_engine* h) { return h->e->S.e; }

extern "C" {

int ll_sepmc_create(const ll_sepmc_config* cfg, const double* model_blob, int blob_len, const double* init_state37, ll_sepmc_engine** out) { return ll_create_as(out, cfg, model_blob, blob_len, init_state37); }
int ll_sepmc_destroy(ll_sepmc_engine* h) { return ll_destroy_as(h); }
int ll_sepmc_reset(ll_sepmc_engine* h, const int32_t* arena_ids, int n, const float* h_draws, const float* h_prev_orn) { return ll_reset_as(h, arena_ids, n, h_draws, h_prev_orn); }
int ll_sepmc_step(ll_sepmc_engine* h, const float* d_actions) { return ll_step_as(h, d_actions); }
int ll_sepmc_step_random_n(ll_sepmc_engine* h, float sigma, int n_steps) { return ll_step_random_n_as(h, sigma, n_steps); }
int ll_sepmc_kernel_time_stats(ll_sepmc_engine* h, double* avg_launch_ms, int* n_launches, int64_t* n_control_steps) { return ll_kernel_time_stats_as(h, avg_launch_ms, n_launches, n_control_steps); }
int ll_sepmc_set_actions(ll_sepmc_engine* h, const float* h_actions) { return ll_set_actions_as(h, h_actions); }
int ll_sepmc_fill_random_actions(ll_sepmc_engine* h, float sigma) { return ll_fill_random_actions_as(h, sigma); }
int ll_sepmc_step_scripted(ll_sepmc_engine* h, const float* h_actions, const float* h_state, const uint8_t* h_ray_hit, const float* h_ray_frac,
                           const uint8_t* h_vis_blocked, const int32_t* h_contacts, const float* h_draws, int n_draws) {
  LL_TRY
  LL_CHECK(h && h_actions && h_state && h_ray_hit && h_ray_frac && h_vis_blocked && h_contacts, "null argument");
  h->e->step_scripted(h_actions, h_state, h_ray_hit, h_ray_frac, h_vis_blocked, h_contacts, h_draws, n_draws);
  LL_CATCH
}
int ll_sepmc_set_step_draws(ll_sepmc_engine* h, const float* h_draws, int n_draws) { return ll_set_step_draws_as(h, h_draws, n_draws); }
int ll_sepmc_script_reset(ll_sepmc_engine* h, const uint8_t* h_ray_hit, const float* h_ray_frac, const uint8_t* h_vis_blocked) {
  LL_TRY
  LL_CHECK(h && h_ray_hit && h_ray_frac && h_vis_blocked, "null argument");
  h->e->script_reset(h_ray_hit, h_ray_frac, h_vis_blocked);
  LL_CATCH
}
int ll_sepmc_set_spec_param(ll_sepmc_engine* h, int id, double value) { return ll_set_spec_param_as(h, id, value); }
int ll_sepmc_get_spec_param(ll_sepmc_engine* h, int id, double* value) { return ll_get_spec_param_as(h, id, value); }
int ll_sepmc_sync(ll_sepmc_engine* h) { return ll_sync_as(h); }
int ll_sepmc_obs_dim(ll_sepmc_engine* h) { return ll_obs_dim_as(h); }

int ll_sepmc_get_obs(ll_sepmc_engine* h, float* h_obs) { return ll_get_obs_as(h, h_obs); }
int ll_sepmc_get_reward_done(ll_sepmc_engine* h, float* h_reward, uint8_t* h_done, uint8_t* h_done_reason) {
  LL_TRY
  LL_CHECK(h, "null engine");
  const size_t N = h->e->base.P.n_envs;
  if (h_reward) h->e->base.get_vec(h->e->base.P.reward, h_reward, N);
  if (h_done || h_done_reason) {
    std::vector<uint8_t> d(N), r(N);
    h->e->base.get_vec(h->e->base.P.done, d.data(), N);
    h->e->base.get_vec(h->e->base.P.done_reason, r.data(), N);
    for (size_t a = 0; a < N / 2; a++) {
      if (h_done) h_done[a] = d[2 * a];
      if (h_done_reason) h_done_reason[a] = r[2 * a];
    }
  }
  LL_CATCH
}
int ll_sepmc_get_state(ll_sepmc_engine* h, float* h_state37) { return ll_get_state_as(h, h_state37); }
int ll_sepmc_set_state(ll_sepmc_engine* h, const float* h_state37) { return ll_set_state_as(h, h_state37); }
int ll_sepmc_get_episode(ll_sepmc_engine* h, float* h_rows21) {
  LL_TRY
  LL_CHECK(h && h_rows21, "null argument");
  const size_t N = h->e->base.P.n_envs;
  std::vector<float> sp(N * SEPMC_SP_STRIDE);
  h->e->base.get_vec(h->e->S.sp, sp.data(), sp.size());
  static const int src[16] = {SP_FLAG, SP_FLAG + 1, SP_FLAG + 2, SP_WITH_FLAG0, SP_FRICTION, SP_FIX_SPD, SP_COUNTER, SP_PUSH_FORCE, SP_PUSH_FORCE + 1, SP_PUSH_FORCE + 2,
                              SP_NOISE, SP_NOISE + 1, SP_NOISE + 2, SP_NOISE + 3, SP_LAST_TWO, SP_LAST_ESC};
  for (size_t a = 0; a < N / 2; a++) {
    const float* r0 = &sp[(2 * a) * SEPMC_SP_STRIDE];
    const float* r1 = &sp[(2 * a + 1) * SEPMC_SP_STRIDE];
    float* o = h_rows21 + a * 21;
    for (int i = 0; i < 16; i++) o[i] = r0[src[i]];
    o[16] = r0[SP_SWITCH]; o[17] = r0[SP_VISIBLE]; o[18] = r1[SP_VISIBLE];
    o[19] = r0[SP_WHO0]; o[20] = r0[SP_WHO_T];
  }
  LL_CATCH
}
int ll_sepmc_get_info(ll_sepmc_engine* h, float* h_rows4) {
  LL_TRY
  LL_CHECK(h && h_rows4, "null argument");
  const size_t N = h->e->base.P.n_envs;
  std::vector<float> inf(N * 4);
  h->e->base.get_vec(h->e->S.info, inf.data(), inf.size());
  for (size_t a = 0; a < N / 2; a++)
    for (int i = 0; i < 4; i++) h_rows4[a * 4 + i] = inf[(2 * a) * 4 + i];
  LL_CATCH
}
int ll_sepmc_get_boxes(ll_sepmc_engine* h, float* h_rows, int32_t* h_count) {
  LL_TRY
  LL_CHECK(h && h_rows && h_count, "null argument");
  const size_t N = h->e->base.P.n_envs;
  std::vector<float> bx(N * EPMC_MAX_BOXES * EPMC_BOX_WORDS), sp(N * SEPMC_SP_STRIDE);
  h->e->base.get_vec(h->e->S.e.boxes, bx.data(), bx.size());
  h->e->base.get_vec(h->e->S.sp, sp.data(), sp.size());
  for (size_t a = 0; a < N / 2; a++) {
    const int n = (int)sp[(2 * a) * SEPMC_SP_STRIDE + SP_N_BOXES];
    h_count[a] = n < LLS_MAX_BOXES ? n : LLS_MAX_BOXES;
    for (int b = 0; b < LLS_MAX_BOXES; b++) {
      const float* r = &bx[((2 * a) * EPMC_MAX_BOXES + b) * EPMC_BOX_WORDS];
      float* o = h_rows + (a * LLS_MAX_BOXES + b) * 6;
      for (int k = 0; k < 3; k++) { o[k] = b < n ? 0.5f * (r[2 * k] + r[2 * k + 1]) : 0.0f; o[3 + k] = b < n ? 0.5f * (r[2 * k + 1] - r[2 * k]) : 0.0f; }
    }
  }
  LL_CATCH
}
int ll_sepmc_get_rays(ll_sepmc_engine* h, float* h_from, float* h_to, uint8_t* h_hit, float* h_frac) { return ll_get_rays_as(h, h_from, h_to, h_hit, h_frac, "the ray trace is kept for engines of at most 256 arenas"); }
int ll_sepmc_get_vis(ll_sepmc_engine* h, float* h_rows) {
  LL_TRY
  LL_CHECK(h && h_rows, "null argument");
  if (!h->e->S.vis_trace) throw PmcError(LL_ESTATE, "the visibility trace is kept for engines of at most 256 arenas");
  const size_t N = h->e->base.P.n_envs;
  std::vector<float> tr(N * 16 * 8);
  h->e->base.get_vec(h->e->S.vis_trace, tr.data(), tr.size());
  for (size_t a = 0; a < N / 2; a++) {
    float* o = h_rows + a * SEPMC_N_VIS * 8;
    for (int i = 0; i < SEPMC_N_VIS * 8; i++) o[i] = 0.0f;
    for (int me = 0; me < 2; me++)
      for (int k = 0; k < 16; k++) {
        const int g = k >> 2, s = k & 3;
        if (!(s < 2 || (s == 2 && (g == 0 || g == 2)) || (s == 3 && g == 0 && me == 0))) continue;
        const int slot = s == 3 ? 0 : 1 + 10 * me + (s == 0 ? g : (s == 1 ? 4 + g : 8 + (g >> 1)));
        for (int i = 0; i < 8; i++) o[slot * 8 + i] = tr[((2 * a + me) * 16 + k) * 8 + i];
      }
  }
  LL_CATCH
}
int ll_sepmc_get_push_trace(ll_sepmc_engine* h, float* h_rows, int32_t* n_sub) { return ll_get_push_trace_as(h, h_rows, n_sub); }
int ll_sepmc_get_counters(ll_sepmc_engine* h, uint64_t* steps, uint64_t* episodes, uint64_t* nonfinite) { return ll_get_counters_as(h, steps, episodes, nonfinite, 2); }
int ll_sepmc_device_ptrs(ll_sepmc_engine* h, ll_device_ptrs_t* out) { return ll_device_ptrs_as(h, out, false); }
int ll_sepmc_enable_kernel_timing(ll_sepmc_engine* h, int on) { return ll_enable_kernel_timing_as(h, on); }
int ll_sepmc_kernel_time_ms(ll_sepmc_engine* h, double* avg_ms, int* n) { return ll_kernel_time_ms_as(h, avg_ms, n); }

}  // extern "C"
