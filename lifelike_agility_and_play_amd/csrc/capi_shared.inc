// capi_shared.inc -- the entry points that ll_*, ll_epmc_* and ll_sepmc_* have in common, each written once as a function template over the
// handle type: its LL_TRY, its LL_CHECK with its message, its body and its LL_CATCH.  The extern "C" entry points of the three *_capi.inc files
// are then `return ll_x(h, ...);`.  Included by pmc_capi.inc after the LL_TRY / LL_CATCH / LL_CHECK macros.
//
// ll_pmc(h) is the PmcEngine behind a handle: the engine itself for ll_engine, the `base` an EpmcEngine / SepmcEngine owns for the other two.
// ll_play(h) (epmc_capi.inc, sepmc_capi.inc) is the EpmcParams of such an engine.
#include <type_traits>

template <class H>
static auto& ll_pmc(H* h) { return h->e->base; }
static ENGINE& ll_pmc(ll_engine* h) { return *h->e; }

// init37...: the start state, of the two engines that take one
template <class H, class CFG, class... INIT>
static int ll_create_as(H** out, const CFG* cfg, const double* model_blob, int blob_len, const INIT*... init37) {
  LL_TRY
  LL_CHECK(cfg && model_blob && (init37 && ... && true) && out, "null argument");
  *out = nullptr;
  H* h = new H;
  try {
    h->e = new typename std::remove_pointer<decltype(h->e)>::type(*cfg, model_blob, blob_len, init37...);
  } catch (...) {
    delete h;
    throw;
  }
  *out = h;
  LL_CATCH
}
template <class H>
static int ll_destroy_as(H* h) {
  LL_TRY
  if (h) {
    delete h->e;
    delete h;
  }
  LL_CATCH
}
// a, b: clip and start time (PMC), or draws and previous orientation (EPMC, SEPMC)
template <class H, class A, class B>
static int ll_reset_as(H* h, const int32_t* ids, int n, const A* a, const B* b) {
  LL_TRY
  LL_CHECK(h, "null engine");
  h->e->reset(ids, n, a, b);
  LL_CATCH
}
template <class H>
static int ll_step_as(H* h, const float* d_actions) {
  LL_TRY
  LL_CHECK(h, "null engine");
  h->e->step(d_actions);
  LL_CATCH
}
template <class H>
static int ll_step_random_n_as(H* h, float sigma, int n_steps) {
  LL_TRY
  LL_CHECK(h, "null engine");
  h->e->step_random_n(sigma, n_steps);
  LL_CATCH
}
template <class H>
static int ll_set_step_draws_as(H* h, const float* h_draws, int n_draws) {
  LL_TRY
  LL_CHECK(h && (h_draws || n_draws == 0), "null argument");
  h->e->set_step_draws(h_draws, n_draws);
  LL_CATCH
}
template <class H>
static int ll_set_actions_as(H* h, const float* h_actions) {
  LL_TRY
  LL_CHECK(h && h_actions, "null argument");
  auto& e = ll_pmc(h);
  e.bk.sync();
  e.bk.h2d(e.d_actions, h_actions, (size_t)e.P.n_envs * 12 * 4);
  LL_CATCH
}
// (the PMC engine's own fill_random_actions asks for the mocap table first: ll_fill_random_actions stays written out)
template <class H>
static int ll_fill_random_actions_as(H* h, float sigma) {
  LL_TRY
  LL_CHECK(h, "null engine");
  auto& e = ll_pmc(h);
  e.bk.launch_actions(e.P, e.d_actions, sigma);
  LL_CATCH
}
template <class H>
static int ll_set_spec_param_as(H* h, int id, double value) {
  LL_TRY
  LL_CHECK(h, "null engine");
  ll_pmc(h).bk.sync();
  std::string e = pmc_set_spec_param(ll_pmc(h).P, id, value);
  if (!e.empty()) throw PmcError(LL_EINVAL, e);
  LL_CATCH
}
template <class H>
static int ll_get_spec_param_as(H* h, int id, double* value) {
  LL_TRY
  LL_CHECK(h && value, "null argument");
  LL_CHECK(id >= 0 && id < LLM_SPEC_COUNT, "unknown spec parameter id");
  *value = pmc_get_spec_param(ll_pmc(h).P, id);
  LL_CATCH
}
template <class H>
static int ll_sync_as(H* h) {
  LL_TRY
  LL_CHECK(h, "null engine");
  ll_pmc(h).bk.sync();
  LL_CATCH
}
template <class H>
static int ll_obs_dim_as(H* h) { return h ? ll_pmc(h).P.obs_dim : LL_EINVAL; }

// terminal_obs: only the PMC engine keeps terminal observations
template <class H>
static int ll_device_ptrs_as(H* h, ll_device_ptrs_t* out, bool terminal_obs) {
  LL_TRY
  LL_CHECK(h && out, "null argument");
  auto& e = ll_pmc(h);
  const StepParams& P = e.P;
  out->obs = P.obs; out->reward = P.reward; out->done = P.done; out->done_reason = P.done_reason;
  out->actions = e.d_actions; out->terminal_obs = terminal_obs ? P.term_obs : nullptr;
  out->obs_dim = P.obs_dim; out->n_envs = P.n_envs; out->stream = e.bk.stream_handle();
  LL_CATCH
}
template <class H>
static int ll_get_obs_as(H* h, float* h_obs) {
  LL_TRY
  LL_CHECK(h && h_obs, "null argument");
  auto& e = ll_pmc(h);
  e.get_vec(e.P.obs, h_obs, (size_t)e.P.n_envs * e.P.obs_dim);
  LL_CATCH
}
// one entry per row (PMC, EPMC; an arena's robots share done and its reason: ll_sepmc_get_reward_done)
template <class H>
static int ll_get_reward_done_as(H* h, float* h_reward, uint8_t* h_done, uint8_t* h_done_reason) {
  LL_TRY
  LL_CHECK(h, "null engine");
  auto& e = ll_pmc(h);
  const size_t N = e.P.n_envs;
  if (h_reward) e.get_vec(e.P.reward, h_reward, N);
  if (h_done) e.get_vec(e.P.done, h_done, N);
  if (h_done_reason) e.get_vec(e.P.done_reason, h_done_reason, N);
  LL_CATCH
}
template <class H>
static int ll_get_state_as(H* h, float* h_state37) {
  LL_TRY
  LL_CHECK(h && h_state37, "null argument");
  ll_pmc(h).get_soa(ll_pmc(h).P.state, 37, h_state37);
  LL_CATCH
}
template <class H>
static int ll_set_state_as(H* h, const float* h_state37) {
  LL_TRY
  LL_CHECK(h && h_state37, "null argument");
  ll_pmc(h).set_soa(ll_pmc(h).P.state, 37, h_state37);
  LL_CATCH
}
// refusal: what an engine too large to keep the trace answers, in its own unit (envs, arenas)
template <class H>
static int ll_get_rays_as(H* h, float* h_from, float* h_to, uint8_t* h_hit, float* h_frac, const char* refusal) {
  LL_TRY
  LL_CHECK(h, "null engine");
  if (!ll_play(h).ray_trace) throw PmcError(LL_ESTATE, refusal);
  const size_t N = ll_pmc(h).P.n_envs, R = EPMC_N_RAYS;
  std::vector<float> tr(N * R * 8);
  ll_pmc(h).get_vec(ll_play(h).ray_trace, tr.data(), tr.size());
  for (size_t i = 0; i < N * R; i++) {
    for (int k = 0; k < 3; k++) {
      if (h_from) h_from[i * 3 + k] = tr[i * 8 + k];
      if (h_to) h_to[i * 3 + k] = tr[i * 8 + 3 + k];
    }
    if (h_hit) h_hit[i] = tr[i * 8 + 6] > 0.5f;
    if (h_frac) h_frac[i] = tr[i * 8 + 7];
  }
  LL_CATCH
}
template <class H>
static int ll_get_push_trace_as(H* h, float* h_rows, int32_t* n_sub) {
  LL_TRY
  LL_CHECK(h && h_rows, "null argument");
  auto& e = ll_pmc(h);
  e.get_vec(ll_play(h).push_trace, h_rows, (size_t)e.P.n_envs * e.P.n_sub * 4);
  if (n_sub) *n_sub = e.P.n_sub;
  LL_CATCH
}
// rows_per_step: the rows that one counted step moves (2 for SEPMC, which counts arena steps)
template <class H>
static int ll_get_counters_as(H* h, uint64_t* steps, uint64_t* episodes, uint64_t* nonfinite, int rows_per_step) {
  LL_TRY
  LL_CHECK(h, "null engine");
  auto& e = ll_pmc(h);
  unsigned long long c[4];
  e.get_vec(e.P.counters, c, 4);
  if (steps) *steps = (uint64_t)e.P.step_count * (uint64_t)(e.P.n_envs / rows_per_step);
  if (episodes) *episodes = c[1];
  if (nonfinite) *nonfinite = c[2];
  LL_CATCH
}
template <class H>
static int ll_enable_kernel_timing_as(H* h, int on) {
  LL_TRY
  LL_CHECK(h, "null engine");
  ll_pmc(h).bk.enable_timing(on != 0);
  LL_CATCH
}
template <class H>
static int ll_kernel_time_ms_as(H* h, double* avg_ms, int* n_launches) {
  LL_TRY
  LL_CHECK(h && avg_ms && n_launches, "null argument");
  ll_pmc(h).bk.collect_timing(avg_ms, n_launches);
  LL_CATCH
}
template <class H>
static int ll_kernel_time_stats_as(H* h, double* avg_launch_ms, int* n_launches, int64_t* n_control_steps) {
  LL_TRY
  LL_CHECK(h && avg_launch_ms && n_launches && n_control_steps, "null argument");
  long long st = 0;
  ll_pmc(h).bk.collect_timing(avg_launch_ms, n_launches, &st);
  *n_control_steps = (int64_t)st;
  LL_CATCH
}
