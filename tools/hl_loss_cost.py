"""What the PPO loss of a scored unroll block costs (include/hl/llenv_hl_loss.h), written to profiles/hl_loss.txt.

    python tools/hl_loss_cost.py [output file]

Three blocks, each in a child process of its own under its own time limit (a case that fails or runs out of time ends the run: nothing more is started
on the device): 4096 EPMC hurdles rows, 4096 SEPMC robot rows (2048 arenas, the recorder), and the league's 2048 learner rows, all at L = 128, each in
both modes.  Inside one case, one process, HIP events on the engine's stream, a discarded warm-up and three runs of each:
  loss     ONE ll_hl_loss_unroll / ll_hl_loss_league call (three launches in ppo, four in ppo2) on the finished, scored block;
  torch    the same loss and statistics written with torch ops on views of the same tensors, float64, no gradient: what a caller had to do before
           (ppo2 walks the unroll backwards, a handful of launches per time step);
  score    the scoring launch on that block.
Expectation: loss below torch, and a small fraction of score."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

L, SEED = 128, 7
CASES = (('epmc', 4096, False), ('sepmc', 2048, False), ('sepmc', 2048, True))      # kind, EPMC envs / SEPMC arenas, league
CASE_SECONDS = 300


def torch_loss(torch, f, s, cfg, ppo2):
    """the loss of the header with torch ops in float64 on views f (block) and s (score): default configuration (merged heads, normalised advantages)"""
    d = torch.float64
    n_, e_, v, o = s['neglogp'].to(d), s['entropy'].to(d), s['V'].to(d), f['neglogp'].to(d)
    if ppo2:
        r, dc = f['r'].to(d), f['discount'].to(d)
        Rn, Rs = v[:, -1], []
        for t in range(v.shape[1] - 2, -1, -1):
            boot = Rn if t == v.shape[1] - 2 else (1.0 - cfg.lam) * v[:, t + 1] + cfg.lam * Rn
            Rn = r[:, t] + cfg.gamma * dc[:, t] * boot
            Rs.append(Rn)
        R = torch.stack(Rs[::-1], dim=1)
        n_, e_, v, o = n_[:, :-1], e_[:, :-1], v[:, :-1], o[:, :-1]
        adv = R - v
    else:
        R = f['R'].to(d)
        adv = R - f['V'].to(d)
    adv = (adv - adv.mean()) / torch.sqrt(adv.var(unbiased=False) + cfg.adv_eps)
    rho = torch.exp(o.sum(-1) - n_.sum(-1))
    pg = torch.maximum(-adv * rho, -adv * torch.clamp(rho, 1.0 - cfg.clip_range, 1.0 + cfg.clip_range))
    vl = 0.5 * (v - R) ** 2
    ent = e_.mean(dim=(0, 1))
    kl = 0.5 * ((n_ - o) ** 2).mean(dim=(0, 1))
    clip = ((rho - 1.0).abs() > cfg.clip_range).to(d).mean()
    loss = pg.mean() + cfg.vf_coef * vl.mean() - cfg.ent_coef * ent.sum()
    return torch.stack([loss, pg.mean(), vl.mean(), clip, R.mean(), v.mean(), 1.0 - (R - v).var(unbiased=False) / R.var(unbiased=False)]), ent, kl


def case(kind, n, league):
    import numpy as np
    import torch
    import __graft_entry__ as g
    from hl_policy_rate import engine, policy
    from lifelike_agility_and_play_amd import gather
    from lifelike_agility_and_play_amd.policies import hl_loss as HL
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
    grad = torch.empty((rows, L, SC.LLS_OUT_FLOATS), device='cuda')
    stats = torch.empty(HL.LLL_N_STATS, dtype=torch.float64, device='cuda')
    nbytes = HL.workspace_bytes(rows, L)
    work = torch.empty(nbytes // 8, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    gather.use_engine_stream(E)                 # torch events and torch ops land on the engine's stream
    try:
        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        def three(fn):
            timed(fn)                           # warm-up, discarded
            return [timed(fn) for _ in range(3)]

        src.steps(SEED, L + 1, False)           # unroll 0 and the first step of unroll 1, sample = 0
        src.finish(0)
        t_score = three(lambda: SC.score(pol, src, 0, out))
        name = '%s %d rows%s' % (kind.upper(), rows, ' (league, learner rows of %d arenas)' % n if league else '')
        print('%s, L %d, block %.2f GB; device %s; build %s' % (name, L, rows * L * src.row_floats * 4 / 1e9, torch.cuda.get_device_name(0),
                                                              g.build_info().get('code_object_sha256')))
        print('      score, one launch                        %9.3f ms   (runs: %s)' % (float(np.median(t_score)), ' '.join('%.3f' % x for x in t_score)))
        f, s = src.split_row(src.block(0)), SC.split_out(out, src.kind)
        for mode, label in ((HL.LLL_PPO, 'ppo'), (HL.LLL_PPO2, 'ppo2')):
            cfg = HL.default_config(mode=mode, ent_coef=0.01)
            t_loss = three(lambda: HL.loss_block(src, 0, cfg, out.data_ptr(), None, grad.data_ptr(), stats.data_ptr(), work.data_ptr(), nbytes))
            t_torch = three(lambda: torch_loss(torch, f, s, cfg, mode == HL.LLL_PPO2))
            torch.cuda.synchronize()
            st = HL.named(stats)
            ref = torch_loss(torch, f, s, cfg, mode == HL.LLL_PPO2)[0].tolist()
            ml, mt = float(np.median(t_loss)), float(np.median(t_torch))
            print('      %-4s loss, %d launches                   %9.3f ms   (runs: %s)   loss / score = %.4f' % (
                label, 3 + (mode == HL.LLL_PPO2), ml, ' '.join('%.3f' % x for x in t_loss), ml / float(np.median(t_score))))
            print('      %-4s the same with torch ops, float64    %9.3f ms   (runs: %s)   loss / torch = %.3f   loss %.12g (torch %.12g)' % (
                label, mt, ' '.join('%.3f' % x for x in t_torch), ml / mt, st['loss'], ref[0]))
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream())
    src.close(); pol.close(); E.close()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == '--case':
        case(sys.argv[2], int(sys.argv[3]), sys.argv[4] == '1')
        return
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'hl_loss.txt')
    lines = ['The PPO loss of scored unroll blocks (include/hl/llenv_hl_loss.h) on an MI355X.',
             '== python tools/hl_loss_cost.py  (HIP events on the engine\'s stream; every case a process of its own, loss, torch and score in that one process) ==']
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
