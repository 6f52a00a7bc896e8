"""What scoring a recorded unroll block costs (include/hl/llenv_hl_score.h), written to profiles/hl_score.txt.

    python tools/hl_score_cost.py [output file]

Three cases, each in a child process of its own under its own time limit (a case that fails or runs out of time ends the run: nothing more is started
on the device): 4096 EPMC hurdles rows, 4096 SEPMC robot rows (2048 arenas, the recorder), and the league's 2048 learner rows, all at L = 128.
Inside one case, one process, HIP events on the engine's stream:
  record   the actor loop fills the block (HlUnrollRecorder.steps / HlLeagueActor.steps, 128 steps);
  score    ONE scoring launch of that block under the recording policy's weights: a discarded warm-up, then three runs;
  act_pg   128 ll_hl_policy_act_pg launches with value, sample = 0, on the same row count and the engine's current observations: the nearest thing
           the library could do before the scorer (it samples its own heads and advances the policy's own state).
The scorer does the same stages per time step without the draws and without 127 launch gaps, so score <= act_pg x 128 is the expectation; the
ratio to the time the loop needs to RECORD such a block is printed last."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

L, SEED = 128, 7
CASES = (('epmc', 4096, False), ('sepmc', 2048, False), ('sepmc', 2048, True))      # kind, EPMC envs / SEPMC arenas, league
CASE_SECONDS = 240


def case(kind, n, league):
    import numpy as np
    import torch
    import __graft_entry__ as g
    from hl_policy_rate import engine, policy
    from lifelike_agility_and_play_amd import gather
    from lifelike_agility_and_play_amd.policies import hl_policy_hip as H
    from lifelike_agility_and_play_amd.policies import hl_score as SC
    E = engine(kind, n)
    E.reset()
    p = E.device_ptrs()
    if league:
        import hl_policy_pg_ref as G
        import hl_policy_ref as R
        from lifelike_agility_and_play_amd.policies import hl_league as LG
        w, v = H.pack_weights(H.LLH_SEPMC, R.SEPMC_WEIGHTS), H.pack_value_weights(H.LLH_SEPMC, G.SEPMC_VALUE)
        src = LG.HlLeagueActor(E, 1, L, 2)
        src.set_weights(0, w, value_weights=v)
        src.set_weights(1, w)
        pol = policy(kind, src.n_rows, value=True)
    else:
        from lifelike_agility_and_play_amd.policies import hl_unroll as U
        pol = policy(kind, p.n_envs, value=True)
        src = U.HlUnrollRecorder(E, pol, L, 2)
    rows = src.n_rows
    out = torch.empty((rows, L, SC.LLS_OUT_FLOATS), device='cuda')
    act = torch.empty((rows, 12), device='cuda')
    nl = torch.empty((rows, pol.n_heads), device='cuda')
    val = torch.empty(rows, device='cuda')
    torch.cuda.synchronize()
    gather.use_engine_stream(E)                 # torch events land on the engine's stream
    try:
        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        src.steps(SEED, L)                      # warm-up unroll (block 0)
        t_record = timed(lambda: src.steps(SEED, L))       # block 1
        timed(lambda: SC.score(pol, src, 1, out))          # warm-up, discarded
        t_score = [timed(lambda: SC.score(pol, src, 1, out)) for _ in range(3)]

        def act_loop():
            for t in range(L):
                pol.act_pg_ptr(p.obs, act.data_ptr(), rows, SEED, t, False, p.stream, p.done, None, None, nl.data_ptr(), val.data_ptr(), p.obs_dim)
        timed(act_loop)
        t_act = [timed(act_loop) for _ in range(3)]
        f = SC.split_out(out, src.kind)
        recorded = src.split_row(src.block(1))
        same_v = bool((f['V'] == recorded['V']).all())
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream())
    name = '%s %d rows%s' % (kind.upper(), rows, ' (league, learner rows of %d arenas)' % n if league else '')
    print('%s, L %d, block %.2f GB; device %s; build %s' % (name, L, rows * L * src.row_floats * 4 / 1e9, torch.cuda.get_device_name(0),
                                                          g.build_info().get('code_object_sha256')))
    print('      score, one launch                 %9.2f ms   (runs: %s)   V equals the recorded V bit for bit: %s' % (
        float(np.median(t_score)), ' '.join('%.2f' % x for x in t_score), same_v))
    print('      act_pg x %d, value, sample = 0    %9.2f ms   (runs: %s)   score / act_pg loop = %.3f' % (
        L, float(np.median(t_act)), ' '.join('%.2f' % x for x in t_act), float(np.median(t_score)) / float(np.median(t_act))))
    print('      recording the block (steps x %d) %9.2f ms   score / record = %.3f' % (L, t_record, float(np.median(t_score)) / t_record))
    src.close(); pol.close(); E.close()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == '--case':
        case(sys.argv[2], int(sys.argv[3]), sys.argv[4] == '1')
        return
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'hl_score.txt')
    lines = ['Teacher-forced scoring of recorded unroll blocks (include/hl/llenv_hl_score.h) on an MI355X.',
             '== python tools/hl_score_cost.py  (HIP events on the engine\'s stream; every case a process of its own, score and act_pg in that one process) ==']
    ok = True
    for kind, n, league in CASES:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--case', kind, str(n), '1' if league else '0'], capture_output=True, text=True,
                               timeout=CASE_SECONDS, cwd=ROOT)
            status, text, err = r.returncode, r.stdout, r.stderr
        except subprocess.TimeoutExpired as e:
            status, text, err = 124, e.stdout or '', 'time limit of %d s' % CASE_SECONDS
            text = text.decode() if isinstance(text, bytes) else text
        lines += text.rstrip().splitlines()
        print(text, end='')
        if status != 0:
            ok = False
            lines.append('case %s %d league=%d ended with status %d; nothing further was run' % (kind, n, league, status))
            lines += err.rstrip().splitlines()[-12:]
            print(err, file=sys.stderr)
            break
    with open(path, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
