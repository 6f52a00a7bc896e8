"""What recording learner-ready unrolls costs the on-device EPMC / SEPMC actor loop (include/hl/llenv_hl_unroll.h).

    python tools/hl_unroll_cost.py [reps]

One process.  At 4096 EPMC hurdles rows and 2048 SEPMC arenas (4096 robot rows), unroll length 128, two buffers, auto-reset engines, HIP-event time
on the engine's stream of
  (a) the plain loop  act_pg ; step  (every head sampled, neglogp and value into scratch buffers): what the actor could do before the recorder,
  (b) HlUnrollRecorder.steps: the same loop with every row packed into the unroll block,
  (c) HlUnrollRecorder.finish: the TD(lambda) pass over one block,
(a) and (b) in turns inside this one run, `reps` unrolls each, medians reported (boxes differ by a few per cent: only the comparison inside a run
counts).  Next to (b) - (a): the bytes the record kernels move per step divided by the bandwidth of a device triad measured here (a = b + 1.5 c
on 3 x 1 GiB with torch's own kernel -- the measurement bench.py --full reports as roofline.peak_measured_triad)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np  # noqa: E402

from hl_policy_rate import engine, policy  # noqa: E402

L, SEED = 128, 7


def triad_gbs():
    import torch
    nel = 1 << 28
    b = torch.ones(nel, device='cuda'); c = torch.ones(nel, device='cuda'); a = torch.empty_like(b)
    for _ in range(3):
        torch.add(b, c, alpha=1.5, out=a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        torch.add(b, c, alpha=1.5, out=a)
    e1.record(); torch.cuda.synchronize()
    return 10 * 3 * nel * 4 / (e0.elapsed_time(e1) * 1e-3) / 1e9


def measure(kind, n, reps):
    import torch
    from lifelike_agility_and_play_amd import gather
    from lifelike_agility_and_play_amd.policies import hl_unroll as U
    E = engine(kind, n)
    E.reset()
    rows = E.device_ptrs().n_envs
    pol = policy(kind, rows, value=True)
    rec = U.HlUnrollRecorder(E, pol, L, 2)
    nl = torch.empty((rows, pol.n_heads), device='cuda')
    val = torch.empty(rows, device='cuda')
    code = torch.empty(rows, dtype=torch.int32, device='cuda')
    hd = torch.empty(rows, device='cuda')
    torch.cuda.synchronize()
    gather.use_engine_stream(E)                 # torch events land on the engine's stream
    try:
        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        t_plain = [0]

        def plain():
            for _ in range(L):
                pol.act_pg(E, SEED, t_plain[0], True, d_neglogp=nl.data_ptr(), d_value=val.data_ptr(), d_code=code.data_ptr(),
                           d_heading=hd.data_ptr() if kind == 'sepmc' else None)
                E.step()
                t_plain[0] += 1
        plain(); rec.steps(SEED, L)             # warm-up: one unroll each
        E.sync()
        a, b, c = [], [], []
        for _ in range(reps):
            a.append(1e3 * timed(plain) / L)
            b.append(1e3 * timed(lambda: rec.steps(SEED, L)) / L)
            k = rec.position()[0] - 1
            c.append(1e3 * timed(lambda: rec.finish(k % 2, 0.95, 0.95, val.data_ptr())))
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream())
    f = rec.fields
    read_floats = f['X'][1] + (128 if kind == 'epmc' else 192) + f['A'][1] + f['neglogp'][1] + 2       # obs, both states, the policy's outputs, reward
    write_floats = rec.row_floats - 1                                                                  # everything but R
    rf, blk = rec.row_floats, rec.n_bytes // 2
    rec.close(); pol.close(); E.close()
    return dict(kind=kind, rows=rows, a=float(np.median(a)), b=float(np.median(b)), c=float(np.median(c)), a_all=a, b_all=b,
                bytes_per_step=4 * rows * (read_floats + write_floats), row_floats=rf, block_bytes=blk)


def main():
    import torch
    import __graft_entry__ as g
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    print('device: %s; build %s' % (torch.cuda.get_device_name(0), g.build_info().get('code_object_sha256')))
    bw = triad_gbs()
    print('device triad a = b + 1.5 c on 3 x 1 GiB: %.0f GB/s' % bw)
    for kind, n in (('epmc', 4096), ('sepmc', 2048)):
        m = measure(kind, n, reps)
        ideal = m['bytes_per_step'] / (bw * 1e9) * 1e6
        extra = m['b'] - m['a']
        print('%-5s %d rows, L %d, row %d floats, block %.2f GB, %d unrolls each, us per control step (median; all: a %s, b %s):' % (
            m['kind'].upper(), m['rows'], L, m['row_floats'], m['block_bytes'] / 1e9, reps, ' '.join('%.1f' % x for x in m['a_all']),
            ' '.join('%.1f' % x for x in m['b_all'])))
        print('      (a) act_pg ; step            %8.1f us' % m['a'])
        print('      (b) recorder.steps           %8.1f us   (b) - (a) = %.1f us = %.1f %% of (a)' % (m['b'], extra, 100 * extra / m['a']))
        print('      record traffic %.1f MB per step / triad = %.1f us; (b) - (a) is %.2f x that' % (m['bytes_per_step'] / 1e6, ideal, extra / ideal))
        print('      (c) finish, per block        %8.1f us   (%.2f us per control step of the unroll)' % (m['c'], m['c'] / L))


if __name__ == '__main__':
    main()
