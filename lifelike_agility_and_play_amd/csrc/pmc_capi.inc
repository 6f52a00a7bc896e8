// pmc_capi.inc -- the extern "C" entry points of include/llenv.h over `ENGINE` (a PmcEngine<Backend>).
// Included once by the translation unit that defines ENGINE.
#include <stdio.h>

#include "../../include/llenv.h"

struct ll_engine {
  ENGINE* e;
};

static thread_local std::string g_ll_err;

#define LL_TRY try {
#define LL_CATCH                                     \
  }                                                  \
  catch (const PmcError& ex) {                       \
    g_ll_err = ex.what();                            \
    return ex.code;                                  \
  }                                                  \
  catch (const std::bad_alloc&) {                    \
    g_ll_err = "out of host memory";                 \
    return LL_ENOMEM;                                \
  }                                                  \
  catch (const std::exception& ex) {                 \
    g_ll_err = ex.what();                            \
    return LL_EINVAL;                                \
  }                                                  \
  return LL_OK;
#define LL_CHECK(c, msg) \
  if (!(c)) throw PmcError(LL_EINVAL, msg)

#include "capi_shared.inc"

extern "C" {

const char* ll_last_error(void) { return g_ll_err.c_str(); }
int ll_abi_version(void) { return LL_ABI_VERSION; }
int ll_model_blob_len(void) { return LLM_BLOB_LEN; }

int ll_create(const ll_config* cfg, const double* model_blob, int blob_len, ll_engine** out) { return ll_create_as(out, cfg, model_blob, blob_len); }

int ll_destroy(ll_engine* h) { return ll_destroy_as(h); }

int ll_load_mocap(ll_engine* h, const float* h_frames, const int32_t* h_clip_len, int n_clips, double frame_step) {
  LL_TRY
  LL_CHECK(h && h_frames && h_clip_len, "null argument");
  size_t total = 0;
  for (int c = 0; c < n_clips; c++) total += h_clip_len[c];
  std::vector<double> f(total * 19);
  for (size_t i = 0; i < f.size(); i++) f[i] = (double)h_frames[i];
  h->e->load_mocap(f.data(), h_clip_len, n_clips, frame_step);
  LL_CATCH
}

// float64 rows (what the reference parses from JSON); preferred -- see DESIGN.md "mocap table precision"
int ll_load_mocap_f64(ll_engine* h, const double* h_frames, const int32_t* h_clip_len, int n_clips, double frame_step) {
  LL_TRY
  LL_CHECK(h && h_frames && h_clip_len, "null argument");
  h->e->load_mocap(h_frames, h_clip_len, n_clips, frame_step);
  LL_CATCH
}

int ll_load_obstacles(ll_engine* h, const int32_t* h_count, const double* h_table, int n_clips) {
  LL_TRY
  LL_CHECK(h && h_count, "null argument");
  h->e->load_obstacles(h_count, h_table, n_clips);
  LL_CATCH
}

int ll_reset(ll_engine* h, const int32_t* h_env_ids, int n, const int32_t* h_clip_idx, const double* h_t0) { return ll_reset_as(h, h_env_ids, n, h_clip_idx, h_t0); }

int ll_step(ll_engine* h, const float* d_actions) { return ll_step_as(h, d_actions); }

int ll_step_scripted(ll_engine* h, const float* d_actions, const float* h_state, const float* h_feet) {
  LL_TRY
  LL_CHECK(h && h_state, "null argument");
  h->e->step_scripted(d_actions, h_state, h_feet);
  LL_CATCH
}

int ll_probe_pd_torque(ll_engine* h, const float* h_rows, int n, int mode, float* h_tau) {
  LL_TRY
  LL_CHECK(h && h_rows && h_tau, "null argument");
  LL_CHECK(mode == 0 || mode == 1, "mode must be 0 (target) or 1 (action)");
  h->e->probe_pd_torque(h_rows, n, mode, h_tau);
  LL_CATCH
}

int ll_set_spec_param(ll_engine* h, int id, double value) { return ll_set_spec_param_as(h, id, value); }
int ll_get_spec_param(ll_engine* h, int id, double* value) { return ll_get_spec_param_as(h, id, value); }

int ll_fill_random_actions(ll_engine* h, float sigma) {
  LL_TRY
  LL_CHECK(h, "null engine");
  h->e->fill_random_actions(sigma);
  LL_CATCH
}

int ll_step_random(ll_engine* h, float sigma) {
  LL_TRY
  LL_CHECK(h, "null engine");
  h->e->step_random(sigma);
  LL_CATCH
}

int ll_step_random_n(ll_engine* h, float sigma, int n_steps) { return ll_step_random_n_as(h, sigma, n_steps); }

int ll_sync(ll_engine* h) { return ll_sync_as(h); }

int ll_set_stream(ll_engine* h, void* hip_stream) {
  LL_TRY
  LL_CHECK(h, "null engine");
  h->e->bk.sync();
  h->e->bk.set_stream(hip_stream);
  LL_CATCH
}

int ll_enable_unrolls(ll_engine* h, int unroll_length, int n_buffers, float** d_base, int* row_floats) {
  LL_TRY
  LL_CHECK(h && d_base && row_floats, "null argument");
  h->e->enable_unrolls(unroll_length, n_buffers);
  *d_base = h->e->d_traj;
  *row_floats = h->e->P.obs_dim + LL_UNROLL_EXTRA;
  LL_CATCH
}
int ll_pg_ptrs(ll_engine* h, float** d_neglogp, float** d_value) {
  LL_TRY
  LL_CHECK(h, "null engine");
  if (d_neglogp) *d_neglogp = h->e->d_neglogp;
  if (d_value) *d_value = h->e->d_value;
  LL_CATCH
}
int ll_unroll_position(ll_engine* h, int64_t* unroll_index, int* time_step) {
  LL_TRY
  LL_CHECK(h && unroll_index && time_step, "null argument");
  h->e->unroll_position(unroll_index, time_step);
  LL_CATCH
}
int ll_pg_mark_current(ll_engine* h) {
  LL_TRY
  LL_CHECK(h, "null engine");
  h->e->value_step = h->e->P.step_count;
  LL_CATCH
}
int ll_finish_unroll(ll_engine* h, int buffer, float gamma, float lam, const float* d_bootstrap_value) {
  LL_TRY
  LL_CHECK(h, "null engine");
  h->e->finish_unroll(buffer, gamma, lam, d_bootstrap_value);
  LL_CATCH
}

int ll_device_ptrs(ll_engine* h, ll_device_ptrs_t* out) { return ll_device_ptrs_as(h, out, true); }

int ll_get_obs(ll_engine* h, float* h_obs) { return ll_get_obs_as(h, h_obs); }
int ll_get_terminal_obs(ll_engine* h, float* h_obs) {
  LL_TRY
  LL_CHECK(h && h_obs, "null argument");
  if (!h->e->P.keep_term_obs) throw PmcError(LL_ESTATE, "terminal observations are off: set ll_config.keep_terminal_obs (auto_reset=1)");
  h->e->get_vec(h->e->P.term_obs, h_obs, (size_t)h->e->P.n_envs * h->e->P.obs_dim);
  LL_CATCH
}

int ll_get_reward_done(ll_engine* h, float* h_reward, uint8_t* h_done, uint8_t* h_done_reason) { return ll_get_reward_done_as(h, h_reward, h_done, h_done_reason); }

int ll_set_actions(ll_engine* h, const float* h_actions) { return ll_set_actions_as(h, h_actions); }

int ll_get_state(ll_engine* h, float* h_state) { return ll_get_state_as(h, h_state); }
int ll_set_state(ll_engine* h, const float* h_state) { return ll_set_state_as(h, h_state); }
int ll_get_ref_state(ll_engine* h, float* h_state) {
  LL_TRY
  LL_CHECK(h && h_state, "null argument");
  h->e->get_soa(h->e->P.kin, 37, h_state);
  LL_CATCH
}

int ll_get_episode_info(ll_engine* h, int32_t* h_clip, double* h_time, int32_t* h_steps, float* h_reward_sum) {
  LL_TRY
  LL_CHECK(h, "null engine");
  const size_t N = h->e->P.n_envs;
  if (h_clip) h->e->get_vec(h->e->P.clip, h_clip, N);
  if (h_time) h->e->get_vec(h->e->P.time, h_time, N);
  if (h_steps) h->e->get_vec(h->e->P.ep_steps, h_steps, N);
  if (h_reward_sum) h->e->get_vec(h->e->P.reward_sum, h_reward_sum, N);
  LL_CATCH
}

int ll_get_sampling_table(ll_engine* h, double* h_prob, double* h_avg_reward_sum, double* h_avg_episode_len) {
  LL_TRY
  LL_CHECK(h, "null engine");
  h->e->need(true, false);
  const size_t C = h->e->P.n_clips;
  // (every step kernel folds the episodes it finished into the table before it ends)
  if (h_prob) h->e->get_vec(h->e->d_prob, h_prob, C);
  if (h_avg_reward_sum) h->e->get_vec(h->e->d_avg_reward, h_avg_reward_sum, C);
  if (h_avg_episode_len) h->e->get_vec(h->e->d_avg_len, h_avg_episode_len, C);
  LL_CATCH
}
int ll_set_sampling_table(ll_engine* h, const double* h_avg_reward_sum) {
  LL_TRY
  LL_CHECK(h && h_avg_reward_sum, "null argument");
  h->e->set_sampling_table(h_avg_reward_sum);
  LL_CATCH
}

int ll_get_feet(ll_engine* h, float* h_feet_dyn, float* h_feet_ref) {
  LL_TRY
  LL_CHECK(h, "null engine");
  const size_t N = h->e->P.n_envs;
  std::vector<float> rows(N * 24);
  h->e->get_soa(h->e->P.feet, 24, rows.data());
  for (size_t e = 0; e < N; e++)
    for (int l = 0; l < 4; l++)
      for (int c = 0; c < 3; c++) {     // device fields: [c*... ] = component c of leg l at field c + 3*l  (dyn), 12 + c + 3*l (ghost)
        if (h_feet_dyn) h_feet_dyn[e * 12 + 3 * l + c] = rows[e * 24 + c + 3 * l];
        if (h_feet_ref) h_feet_ref[e * 12 + 3 * l + c] = rows[e * 24 + 12 + c + 3 * l];
      }
  LL_CATCH
}

int ll_get_counters(ll_engine* h, uint64_t* steps, uint64_t* episodes, uint64_t* nonfinite) { return ll_get_counters_as(h, steps, episodes, nonfinite, 1); }

int ll_get_table_sync(ll_engine* h, uint64_t* stale_reseeds) {
  LL_TRY
  LL_CHECK(h && stale_reseeds, "null argument");
  unsigned long long c[4];
  h->e->get_vec(h->e->P.counters, c, 4);
  *stale_reseeds = c[3];
  LL_CATCH
}

int ll_get_episode_histogram(ll_engine* h, uint64_t* counts16) {
  LL_TRY
  LL_CHECK(h && counts16, "null argument");
  unsigned long long c[16];
  h->e->get_vec(h->e->P.ep_hist, c, 16);
  for (int i = 0; i < 16; i++) counts16[i] = c[i];
  LL_CATCH
}

#if defined(PMC_ABLATION)
// ablation builds only (tools/ablate.sh): the PMC_TS stamps of the last step, [n_envs][PMC_TS_SLOTS]
int ll_debug_timestamps(ll_engine* h, uint64_t* out) {
  LL_TRY
  LL_CHECK(h && out, "null argument");
  h->e->get_vec(h->e->P.counters + 4, (unsigned long long*)out, (size_t)PMC_TS_SLOTS * h->e->P.n_envs);
  LL_CATCH
}
#endif

int ll_enable_kernel_timing(ll_engine* h, int on) { return ll_enable_kernel_timing_as(h, on); }
int ll_kernel_time_ms(ll_engine* h, double* avg_ms, int* n_launches) { return ll_kernel_time_ms_as(h, avg_ms, n_launches); }
int ll_kernel_time_stats(ll_engine* h, double* avg_launch_ms, int* n_launches, int64_t* n_control_steps) { return ll_kernel_time_stats_as(h, avg_launch_ms, n_launches, n_control_steps); }

}  // extern "C"
