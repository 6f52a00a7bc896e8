"""What the league actor costs the on-device SEPMC actor loop (include/hl/llenv_hl_league.h).

    python tools/hl_league_cost.py [reps]

One process, 2048 arenas (4096 robot rows), unroll length 128, two buffers, auto-reset engines with one seed each, HIP-event time on each engine's
stream of
  (a) HlUnrollRecorder.steps with one policy on all 4096 rows: the loop before the league (both robots one policy, both recorded, both valued),
  (b) HlLeagueActor.steps with one opponent slot holding the learner's weights,
  (c) HlLeagueActor.steps with four opponent slots of other weights, uniform probabilities,
  (d) the plan kernel alone (ll_hl_league_plan_only: the sort without tally or draw) on (c)'s league,
(a), (b), (c) in turns inside this one run, `reps` unrolls each; medians, with every repeat printed (boxes differ by a few per cent: only the
comparison inside a run counts).  The yardstick for (b) and (c) is (a) itself, the margin (a)'s own spread (max - min) over its repeats."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np  # noqa: E402

from hl_policy_rate import engine, policy  # noqa: E402

L, SEED, ARENAS = 128, 7, 2048


def main():
    import torch
    import __graft_entry__ as g
    import hl_policy_pg_ref as G
    import hl_policy_ref as R
    from lifelike_agility_and_play_amd import gather
    from lifelike_agility_and_play_amd.policies import hl_league as LG
    from lifelike_agility_and_play_amd.policies import hl_policy_hip as H
    from lifelike_agility_and_play_amd.policies import hl_unroll as U
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    print('device: %s; build %s' % (torch.cuda.get_device_name(0), g.build_info().get('code_object_sha256')))
    w, v = H.pack_weights(H.LLH_SEPMC, R.SEPMC_WEIGHTS), H.pack_value_weights(H.LLH_SEPMC, G.SEPMC_VALUE)
    rng = np.random.default_rng(1)
    others = [(w * (1.0 + 0.02 * rng.standard_normal(w.size))).astype(np.float32) for _ in range(4)]
    Ea, Eb, Ec = engine('sepmc', ARENAS), engine('sepmc', ARENAS), engine('sepmc', ARENAS)
    for E in (Ea, Eb, Ec):
        E.reset()
    pol = policy('sepmc', 2 * ARENAS, value=True)
    rec = U.HlUnrollRecorder(Ea, pol, L, 2)
    lb = LG.HlLeagueActor(Eb, 1, L, 2)
    lb.set_weights(0, w, value_weights=v)
    lb.set_weights(1, w)
    lc = LG.HlLeagueActor(Ec, 4, L, 2)
    lc.set_weights(0, w, value_weights=v)
    for k in range(4):
        lc.set_weights(1 + k, others[k])
    lc.set_probs([0.25] * 4)

    def timed(E, fn):
        gather.use_engine_stream(E)             # torch events land on that engine's stream
        try:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)
        finally:
            torch.cuda.set_stream(torch.cuda.default_stream())

    legs = (('a', Ea, lambda: rec.steps(SEED, L)), ('b', Eb, lambda: lb.steps(SEED, L)), ('c', Ec, lambda: lc.steps(SEED, L)))
    for _, E, fn in legs:                       # warm-up: one unroll each
        fn()
        E.sync()
    t = {k: [] for k in 'abcd'}
    for _ in range(reps):
        for k, E, fn in legs:
            t[k].append(1e3 * timed(E, fn) / L)
        t['d'].append(1e3 * timed(Ec, lambda: lc.plan_only(L)) / L)
    med = {k: float(np.median(x)) for k, x in t.items()}
    spread = max(t['a']) - min(t['a'])
    print('SEPMC %d arenas, L %d, %d unrolls each, us per control step (median; every repeat in brackets):' % (ARENAS, L, reps))
    names = dict(a='(a) recorder.steps, one policy, 4096 rows', b='(b) league.steps, K = 1, same weights', c='(c) league.steps, K = 4, uniform',
                 d='(d) plan kernel alone')
    for k in 'abcd':
        print('      %-44s %8.1f us   [%s]' % (names[k], med[k], ' '.join('%.1f' % x for x in t[k])))
    print('      (a) spread over its repeats (max - min): %.1f us' % spread)
    for k in 'bc':
        d = med[k] - med['a']
        print('      (%s) - (a) = %+.1f us = %+.1f %% of (a): %s' % (k, d, 100 * d / med['a'], 'within (a) + its spread' if d <= spread else 'ABOVE (a) + its spread'))
    slot, episode = lc.assignment()
    o = lc.outcomes()
    print('      (c) after %d steps: arenas per slot %s, episodes started %d, tally episodes per slot %s' % (
        (reps + 1) * L, np.bincount(slot, minlength=5)[1:].tolist(), int(episode.sum()), o[:, 0].tolist()))
    for x in (rec, lb, lc, pol, Ea, Eb, Ec):
        x.close()


if __name__ == '__main__':
    main()
