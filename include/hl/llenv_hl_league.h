/*
 * llenv_hl_league.h -- C ABI of the league actor of the SEPMC engine (chase tag, two robots per arena): the recorded loop of
 * llenv_hl_unroll.h with robot 1 of every arena acting with an OPPONENT's weights, drawn per episode on the device.
 *
 * The reference trains chase tag against a league (train_scripts/example_sepmc_train.sh: PFSPGameMgr).  Its actor
 * (learning/actors/distill_actor.py:57-82, :187-208, :294-308) loads the learner's model into agent 0 and the model the task names
 * (task.model_key2) into agent 1, pushes agent 0's transitions only, pulls fresh weights every update_model_freq (320) steps without
 * touching the recurrent state, and reports every finished episode to the league manager, which draws the next opponent from the win
 * rates.  A league binds ONE ll_sepmc_engine created with auto_reset = 1 and does all of that between the engine's steps without the host.
 *
 * Slots.  Slot 0 is the learner: policy weights and a value branch, packed as ll_hl_policy_create and ll_hl_policy_attach_value take them
 * (LLH_SEPMC_N_FLOATS, LLH_SEPMC_VF_N_FLOATS).  Slots 1 .. K (1 <= K <= LLG_MAX_OPPONENTS) are opponents: policy weights only.  All of
 * them live in one device allocation.  Rows are the engine's, 2 arena + robot; robot 0 of every arena is the learner (the reference's
 * me_id = 0), robot 1 of arena a acts with slot[a].
 *
 * State.  Every row has exactly one acting policy, so the league owns ONE policy-state buffer [2 A][128] (the layout of
 * ll_hl_policy_get_state) and one value-state buffer [A][64] for the learner's rows.  Both start at zero; a row whose done flag is set
 * starts its step from zero state, as in the loop of llenv_hl_policy.h.
 *
 * Opponent draw.  At the start of every step, an arena whose done flag the previous step set -- and every arena at the league's first
 * step -- draws the opponent of the episode that starts: Philox4x32-10, key (seed lo, seed hi), counter (arena, episode lo, episode hi,
 * LEAGUE_SALT = 0x1EA60E), `episode` being the league's own count of the episodes that arena has started before this one (0 for the
 * first).  u = ((w0 >> 8) + 0.5) 2^-24 in float32; slot = 1 + the first k with u < cdf[k]; cdf is the float32 running sum of the
 * probabilities of ll_hl_league_set_probs, set to exactly 1 from the last slot with a non-zero probability on.  (For the one word whose u
 * rounds to 1 no k qualifies: it takes that last slot.)  A slot with probability 0 is never drawn and may stay without weights.  Until the
 * first ll_hl_league_set_probs every opponent has probability 1 / K.
 *
 * Outcome tally.  In the same pass, before the re-draw, the finished episode is counted under the slot it was played against: episodes,
 * and how many of them had LLS_DONE_FALL, LLS_DONE_TIME, LLS_DONE_CATCH, LLS_DONE_NONFINITE set in the arena's done_reason
 * (LLG_N_OUTCOMES = 5 counters per opponent slot, in that order).  What counts as a win stays the league manager's business.
 *
 * One act launch per step.  After the draw the arenas are sorted by slot into groups of at most 16 rows of one slot; one kernel launch
 * runs the learner's groups, every opponent group with its slot's weights, and the learner's value branch.  Philox counters use the
 * row's own number and the league's step count, and a row's results do not depend on the group it sits in: the rows of the learner are,
 * bit for bit, what ll_hl_policy_act_pg gives for them, and so are an opponent's under a policy with that slot's weights.  `sample` applies
 * to both sides (TLeague's opponent agents run the same agent code).  Opponent rows get no value, and their code, heading and neglogp are
 * not written anywhere.
 *
 * Recording.  Only the learner's rows are recorded: n_rows = A.  A row is exactly the SEPMC row of llenv_hl_unroll.h (1244 floats, the
 * same fields at the same offsets, S laid out vf | pi | z | hlc, M by the same rule, a zero pad column), the ring is
 * [n_buffers][A][unroll_length][1244] with the same ring arithmetic, and r is robot 0's reward: a learner that reads the blocks of
 * ll_hl_unroll_create_sepmc reads these unchanged.
 *
 * Same conventions as llenv.h: 0 or a negative LL_E* code, ll_last_error() for the text.  Argument errors are LL_EINVAL and are checked
 * before the device is touched; there is no CPU path: LL_ENODEV without a HIP device.
 */
#ifndef LLENV_HL_LEAGUE_H
#define LLENV_HL_LEAGUE_H

#include <stdint.h>

#include "../llenv_sepmc.h"
#include "llenv_hl_policy.h"
#include "llenv_hl_unroll.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LLG_MAX_OPPONENTS 8
#define LLG_N_OUTCOMES 5          /* episodes | fall | time | catch | nonfinite */

typedef struct ll_hl_league ll_hl_league;

/*
 * LL_EINVAL for n_opponents outside 1 .. LLG_MAX_OPPONENTS, a non-positive unroll_length or n_buffers, an engine without auto_reset or
 * with more than 32768 arenas.  The engine must outlive the league.
 */
int ll_hl_league_create(ll_sepmc_engine* e, int n_opponents, int unroll_length, int n_buffers, ll_hl_league** out);
int ll_hl_league_destroy(ll_hl_league* lg);
/*
 * Replaces the weights of `slot` and touches no recurrent state: the actor's _update_agents_model in the middle of an episode
 * (distill_actor.py:294-308).  h_vf_weights is required for slot 0 and must be NULL for an opponent slot (LL_EINVAL).  The upload is
 * ordered on the engine's stream, from a pinned staging buffer the league owns: the call neither waits for the device nor races a launch
 * in flight; steps queued before it use the old weights, steps queued after it the new ones.  A second call for the same slot waits for
 * that slot's previous upload only.
 */
int ll_hl_league_set_weights(ll_hl_league* lg, int slot, const float* h_weights, int n_floats, const float* h_vf_weights, int n_vf_floats);
/* n = n_opponents probabilities, each >= 0, their sum within 1e-6 of 1 (LL_EINVAL).  Ordered on the engine's stream: draws of later steps use them. */
int ll_hl_league_set_probs(ll_hl_league* lg, const double* h_probs, int n);
/*
 * n_steps x { record X, S, M ; tally, draw, sort ; act ; engine step ; record A, neglogp, V, r, discount } on the engine's stream, no host
 * synchronisation inside.  The guards of the recorder's steps call: the engine must have been reset (LL_ESTATE), n_steps must be positive
 * and at most unroll_length x n_buffers (LL_EINVAL).  LL_ESTATE while slot 0, or a slot with a non-zero probability, has no weights.
 */
int ll_hl_league_steps(ll_hl_league* lg, uint64_t seed, int sample, int n_steps);
/* where the NEXT step writes, as the recorder's position call */
int ll_hl_league_position(ll_hl_league* lg, int64_t* unroll_index, int* time_step);
/* kind LLH_SEPMC, n_rows = the engine's arena count */
int ll_hl_league_layout(ll_hl_league* lg, ll_hl_unroll_layout_t* out);
/* TD(lambda) returns into R of block `buffer`: the recursion, the NULL bootstrap rule and the LL_ESTATE cases of the recorder's finish call */
int ll_hl_league_finish(ll_hl_league* lg, int buffer, float gamma, float lam, const float* d_bootstrap_value);
/* h_slot [A]: the slot robot 1 of every arena acts with (0 before the first step); h_episode [A]: the episodes the arena has started.
 * Either may be NULL.  Synchronises. */
int ll_hl_league_get_assignment(ll_hl_league* lg, int32_t* h_slot, int64_t* h_episode);
/* h_outcomes [n_opponents][LLG_N_OUTCOMES]; clear != 0 zeroes the tally after the copy.  Synchronises. */
int ll_hl_league_get_outcomes(ll_hl_league* lg, uint64_t* h_outcomes, int clear);
/* h_state [2 A][128], h_vstate [A][64]; either may be NULL.  Synchronises. */
int ll_hl_league_get_state(ll_hl_league* lg, float* h_state, float* h_vstate);
/*
 * For measuring: n_launches of the plan kernel against an all-zero done buffer, on the engine's stream.  Nothing is tallied or drawn;
 * the row list and the group table are written again as they stand.  LL_ESTATE before the first step.
 */
int ll_hl_league_plan_only(ll_hl_league* lg, int n_launches);

#ifdef __cplusplus
}
#endif
#endif
