"""The league actor (include/hl/llenv_hl_league.h, policies.hl_league) on the GPU: the recorded learner rows, the assignment and the tally against a
hand loop of ordinary policies on the existing act_pg kernel, bit for bit; the weight swaps; the seeds; TD(lambda); guards and canaries; and the tie
to the existing recorder when every slot holds the same weights."""
import numpy as np
import pytest

import hl_league_ref as LR
import hl_policy_pg_ref as G
import hl_policy_ref as R
import hl_unroll_ref as UR
from test_gpu_hl_policy import _epmc_engine, _sepmc_engine

pytestmark = pytest.mark.gpu
L = 16
LL_EINVAL, LL_ESTATE = -1, -4
_SETS = {}


def _weight_set(i, kind='sepmc'):
    """(policy, value) weights number i: 0 the fixtures, i > 0 the fixtures times (1 + 0.02 N(0, 1)) -- multiplicative, so the rms scale stays positive"""
    from lifelike_agility_and_play_amd.policies import hl_policy_hip as H
    if (kind, i) not in _SETS:
        k = H.LLH_SEPMC if kind == 'sepmc' else H.LLH_EPMC
        w = H.pack_weights(k, R.SEPMC_WEIGHTS if kind == 'sepmc' else R.EPMC_WEIGHTS['hurdle'])
        v = H.pack_value_weights(k, G.SEPMC_VALUE if kind == 'sepmc' else G.EPMC_VALUE['hurdle'])
        if i:
            rng = np.random.default_rng(1000 + i)
            w = (w * (1.0 + 0.02 * rng.standard_normal(w.size))).astype(np.float32)
            v = (v * (1.0 + 0.02 * rng.standard_normal(v.size))).astype(np.float32)
        _SETS[(kind, i)] = (w, v)
    return _SETS[(kind, i)]


def _engine(n, seed, max_steps=16):
    E = _sepmc_engine(n, 1, seed, max_steps=max_steps)
    E.reset()
    return E


def _policy(i, rows, value):
    from lifelike_agility_and_play_amd.policies import hl_policy_hip as H
    w, v = _weight_set(i)
    p = H.HipSepmcPolicy(None, rows, weights=w)
    if value:
        p.attach_value(weights=v)
    return p


def _league(E, probs, sets, n_buffers=3, unroll=L):
    """sets: weight set number of slot 0, 1, ..; None leaves the slot without weights"""
    from lifelike_agility_and_play_amd.policies import hl_league as LG
    lg = LG.HlLeagueActor(E, len(probs), unroll, n_buffers)
    for slot, i in enumerate(sets):
        if i is not None:
            w, v = _weight_set(i)
            lg.set_weights(slot, w, value_weights=v if slot == 0 else None)
    lg.set_probs(probs)
    return lg


class HandLoop(object):
    """The loop the league replaces, on the parent's kernels: one ordinary HipSepmcPolicy per slot, each acting on ALL 2 A rows into buffers of its own
    (d_reset = the engine's done buffer, step = t); per row the action of the policy the host mirror of the draw assigns goes into the engine's action
    buffer.  A row's state in a policy it is not assigned to is garbage, but every re-assignment coincides with a d_reset of that row."""

    def __init__(self, E, probs, seed, pols):
        import torch
        from lifelike_agility_and_play_amd import gather
        self.E, self.pols, self.seed = E, pols, seed
        self.p = E.device_ptrs()
        self.n, self.A = self.p.n_envs, self.p.n_envs // 2
        self.T = gather.engine_tensors(E)
        self.why = gather.device_tensor(self.p.done_reason, (self.n,), torch.uint8)
        self.mirror = LR.Mirror(self.A, probs, seed)
        dev = 'cuda'
        self.buf = {s: dict(act=torch.zeros((self.n, 12), device=dev), code=torch.zeros(self.n, dtype=torch.int32, device=dev),
                            hd=torch.zeros(self.n, device=dev), nl=torch.zeros((self.n, 3), device=dev), v=torch.zeros(self.n, device=dev)) for s in pols}
        torch.cuda.synchronize()
        self.t = 0
        self.rec = {k: [] for k in ('obs', 'reset', 'action', 'code', 'heading', 'neglogp', 'value', 'reward', 'done', 'why', 'hs', 'slot', 'first_actions')}

    def run(self, steps):
        import torch
        from lifelike_agility_and_play_amd import gather
        gather.use_engine_stream(self.E)
        try:
            for _ in range(steps):
                t, T, rec = self.t, self.T, self.rec
                torch.cuda.current_stream().synchronize()
                slot = self.mirror.begin_step(rec['done'][-1][::2], rec['why'][-1][::2]) if t else self.mirror.begin_step()
                rec['slot'].append(slot)
                row_slot = np.zeros(self.n, np.int64)
                row_slot[1::2] = slot
                assert set(np.unique(row_slot)) <= set(self.pols), 'an arena drew a slot without a policy'
                rec['hs'].append(self.pols[0].hs()[:self.n])                       # (waits for the device)
                rec['obs'].append(T['obs'].cpu().numpy().reshape(self.n, -1))
                rec['reset'].append(T['done'].cpu().numpy().copy())
                for s, pol in self.pols.items():
                    b = self.buf[s]
                    pol.act_pg_ptr(self.p.obs, b['act'].data_ptr(), self.n, self.seed, t, True, self.p.stream, self.p.done, b['code'].data_ptr(), b['hd'].data_ptr(),
                                   b['nl'].data_ptr(), b['v'].data_ptr() if s == 0 else None, self.p.obs_dim)
                sel = torch.as_tensor(row_slot, device='cuda')
                for s in self.pols:
                    T['actions'].view(self.n, 12)[sel == s] = self.buf[s]['act'][sel == s]
                if t == 0:
                    rec['first_actions'] = {s: self.buf[s]['act'].cpu().numpy() for s in self.pols}
                b0 = self.buf[0]
                rec['action'].append(T['actions'].cpu().numpy().reshape(self.n, 12).copy())
                rec['code'].append(b0['code'].cpu().numpy()); rec['heading'].append(b0['hd'].cpu().numpy())
                rec['neglogp'].append(b0['nl'].cpu().numpy()); rec['value'].append(b0['v'].cpu().numpy())
                self.E.step()
                torch.cuda.current_stream().synchronize()
                rec['reward'].append(T['reward'].cpu().numpy().reshape(self.n).copy())
                rec['done'].append(T['done'].cpu().numpy().reshape(self.n).copy())
                rec['why'].append(self.why.cpu().numpy().copy())
                self.t += 1
        finally:
            torch.cuda.set_stream(torch.cuda.default_stream())

    def unroll(self, u, length=L):
        """block u of the learner's rows as the league must have recorded it"""
        rec, sl = self.rec, slice(u * length, (u + 1) * length)
        ev = lambda k: np.stack(rec[k][sl])[:, ::2]                                  # noqa: E731
        return UR.pack_unroll('sepmc', ev('obs'), ev('code'), ev('action'), ev('neglogp'), ev('value'), ev('reward'), ev('done'), ev('hs'), ev('reset'),
                              heading=ev('heading'), dtype=np.float32)


def _host_block(lg, k):
    import torch
    torch.cuda.synchronize()
    return lg.block(k).cpu().numpy()


def _assert_blocks_equal(lg, hand, n_blocks, msg=''):
    from lifelike_agility_and_play_amd.policies import hl_unroll as U
    for u in range(n_blocks):
        g, w = U.split_row(_host_block(lg, u)), U.split_row(hand.unroll(u, lg.unroll_length))
        for name in U.LLU_FIELDS:
            if name != 'R':                                  # (ll_hl_league_finish's)
                np.testing.assert_array_equal(g[name], w[name], err_msg='%s unroll %d, field %s' % (msg, u, name))


@pytest.mark.parametrize('A,probs,eseed,seed', LR.GPU_CASES)
def test_league_is_the_hand_loop_bit_for_bit(A, probs, eseed, seed):
    """2 L + 1 league steps against the hand loop on a twin engine: every field but R of blocks 0 and 1, the assignment and the tally are equal.  The
    engines end every episode within 16 steps, so every arena draws at least three times."""
    from lifelike_agility_and_play_amd.policies import hl_unroll as U
    K = len(probs)
    live = [0] + [1 + k for k in range(K) if probs[k] > 0]
    EA, EB = _engine(A, eseed), _engine(A, eseed)
    lg = _league(EA, probs, [s if s in live else None for s in range(K + 1)])
    pols = {s: _policy(s, 2 * A, value=(s == 0)) for s in live}
    try:
        assert (lg.n_rows, lg.unroll_length, lg.n_buffers, lg.row_floats) == (A, L, 3, 1244) and lg.fields == U.row_layout(lg.kind)[0]
        assert lg.n_bytes == 3 * A * L * 1244 * 4 and lg.position() == (0, 0)
        lg.steps(seed, 2 * L + 1)
        assert lg.position() == (2, 1)
        hand = HandLoop(EB, probs, seed, pols)
        hand.run(2 * L + 1)
        fa = hand.rec['first_actions']
        for s in live[1:]:
            assert (fa[s] != fa[0]).any(), 'weight set %d acts like the fixtures' % s
        _assert_blocks_equal(lg, hand, 2, '%d arenas, %d opponents' % (A, K))
        slot, episode = lg.assignment()
        np.testing.assert_array_equal(slot, hand.mirror.slot)
        np.testing.assert_array_equal(episode, hand.mirror.episode)
        np.testing.assert_array_equal(lg.outcomes(), hand.mirror.tally)
        # what the seeds promise (test_hl_league_api), from the data
        hist = np.stack(hand.rec['slot'])                                          # [steps][A]
        assert set(np.unique(hist)) == set(live[1:]), 'slots used: %s' % np.unique(hist)
        counts = np.stack([(hist == s).sum(axis=1) for s in live[1:]])
        assert (counts % 16 != 0).any(), 'no partial group occurred'
        assert hand.mirror.tally[:, 0].sum() >= 2 * A and (hand.mirror.episode >= 3).all()
        g0, g1 = U.split_row(_host_block(lg, 0)), U.split_row(_host_block(lg, 1))
        restarts = (np.stack(hand.rec['reset'])[1:, ::2] != 0).sum(axis=0)          # d_reset flags of steps t = 1 .. 2 L
        assert (restarts >= 2).all(), 'every learner row restarts at least twice at t > 0'
        masked = (g0['M'] == 1.0).sum(axis=1) + (g1['M'] == 1.0).sum(axis=1)        # (a restart at an unroll's first frame carries no mask)
        assert (masked <= restarts).all()            # (episodes that run their 16 steps end on an unroll's last step here; test_nothing_else_moved has M = 1)
        np.testing.assert_array_equal(g0['M'][:, 1:], 1.0 - g0['discount'][:, :-1])
        if K > 1:
            changed = (np.diff(hist, axis=0) != 0).any()
            assert changed, 'no arena ever changed its opponent'
        # the state buffer: odd rows under their drawn policy, even rows and the value state under the learner's
        st, vst = lg.state()
        np.testing.assert_array_equal(st[::2], pols[0].state()[:2 * A:2])
        np.testing.assert_array_equal(vst, pols[0].value_state()[:2 * A:2])
        for s in live[1:]:
            rows = 2 * np.nonzero(hand.mirror.slot == s)[0] + 1
            np.testing.assert_array_equal(st[rows], pols[s].state()[rows])
    finally:
        lg.close()
        for p in pols.values():
            p.close()
        EA.close(); EB.close()


@pytest.mark.parametrize('swap_slot', [0, 1])
def test_weight_swap_mid_episode(swap_slot):
    """17 arenas, one opponent: 8 steps, ll_hl_league_set_weights(slot, another model), 8 more.  The hand loop moves state() and value_state() of the
    slot's policy into a fresh one with the other weights.  Equal bits: the swap touched no recurrent state and took effect between steps 7 and 8."""
    A, seed = 17, 0x5A17
    EA, EB = _engine(A, 9), _engine(A, 9)
    lg = _league(EA, (1.0,), [0, 1], n_buffers=2)
    pols = {0: _policy(0, 2 * A, True), 1: _policy(1, 2 * A, False)}
    fresh = _policy(2, 2 * A, value=(swap_slot == 0))
    try:
        lg.steps(seed, 8)
        w, v = _weight_set(2)
        lg.set_weights(swap_slot, w, value_weights=v if swap_slot == 0 else None)       # (no synchronisation: ordered on the engine's stream)
        lg.steps(seed, 8)
        hand = HandLoop(EB, (1.0,), seed, pols)
        hand.run(8)
        old = pols[swap_slot]
        assert np.abs(old.state()).max() > 0                                             # mid-episode: there is state to keep
        fresh.set_state(old.state())
        if swap_slot == 0:
            fresh.set_value_state(old.value_state())
        hand.pols[swap_slot] = fresh
        hand.run(8)
        _assert_blocks_equal(lg, hand, 1, 'swap of slot %d' % swap_slot)
        # ... and the swap mattered: the same run without it records other actions after step 8
        EC = _engine(A, 9)
        lg2 = _league(EC, (1.0,), [0, 1], n_buffers=2)
        try:
            lg2.steps(seed, 16)
            a, b = lg.split_row(_host_block(lg, 0)), lg2.split_row(_host_block(lg2, 0))
            np.testing.assert_array_equal(a['A'][:, :8], b['A'][:, :8])
            assert (a['X'][:, 9:] != b['X'][:, 9:]).any()
        finally:
            lg2.close(); EC.close()
    finally:
        lg.close(); fresh.close()
        for p in pols.values():
            p.close()
        EA.close(); EB.close()


def test_policy_weight_swap_epmc():
    """ll_hl_policy_set_weights on a plain EPMC policy at 63 rows: 8 act_pg steps, the swap on the engine's stream, 8 more -- against a twin that
    continues with a fresh policy of the new weights given the old policy's states.  Equal bits in every output and both states."""
    import torch
    from lifelike_agility_and_play_amd import gather
    from lifelike_agility_and_play_amd.policies import hl_policy_hip as H
    n, seed = 63, 0xE9
    (w1, v1), (w2, v2) = _weight_set(0, 'epmc'), _weight_set(1, 'epmc')

    def run(E, pol, t0, t1, out):
        T = gather.engine_tensors(E)
        nl, v = torch.zeros((n, 2), device='cuda'), torch.zeros(n, device='cuda')
        torch.cuda.synchronize()
        for t in range(t0, t1):
            pol.act_pg(E, seed, t, True, d_neglogp=nl.data_ptr(), d_value=v.data_ptr())
            E.sync()
            out.append((T['actions'].cpu().numpy().copy(), nl.cpu().numpy(), v.cpu().numpy()))
            E.step()

    EA, EB = _epmc_engine('hurdle', n, 1, 5, max_steps=16), _epmc_engine('hurdle', n, 1, 5, max_steps=16)
    pa = H.HipEpmcPolicy(None, n, weights=w1)
    pa.attach_value(weights=v1)
    pb = H.HipEpmcPolicy(None, n, weights=w1)
    pb.attach_value(weights=v1)
    pc = H.HipEpmcPolicy(None, n, weights=w2)
    pc.attach_value(weights=v2)
    try:
        EA.reset(); EB.reset()
        got, want = [], []
        run(EA, pa, 0, 8, got)
        pa.set_weights(weights=w2, value_weights=v2, stream=EA.device_ptrs().stream)
        pa.set_weights(weights=w2, value_weights=v2, stream=EA.device_ptrs().stream)      # a second swap waits for the first upload only
        run(EA, pa, 8, 16, got)
        run(EB, pb, 0, 8, want)
        assert np.abs(pb.state()).max() > 0
        pc.set_state(pb.state()); pc.set_value_state(pb.value_state())
        run(EB, pc, 8, 16, want)
        for t, (g, w) in enumerate(zip(got, want)):
            for a, b in zip(g, w):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), 'step %d' % t
        np.testing.assert_array_equal(pa.state(), pc.state())
        np.testing.assert_array_equal(pa.value_state(), pc.value_state())
        assert not np.array_equal(got[8][0], got[7][0])
        with pytest.raises(Exception) as ei:
            pa.set_weights(weights=w2)                                                    # a branch is attached: the model comes whole
        assert ei.value.code == LL_EINVAL
        with pytest.raises(Exception) as ei:
            pa.set_weights(weights=w2[:-1], value_weights=v2)
        assert ei.value.code == LL_EINVAL
    finally:
        for x in (pa, pb, pc, EA, EB):
            x.close()


def test_seeds():
    """The same (seed, n) reproduces block 0 bit for bit -- in one call or cut in two, step and episode counts carrying over; another seed changes the
    recorded actions and the assignment."""
    from lifelike_agility_and_play_amd.policies import hl_unroll as U
    A, probs = 64, (0.25, 0.25, 0.25, 0.25)
    blocks, slots = [], []
    for seed, cuts in ((77, (L,)), (77, (7, L - 7)), (78, (L,))):
        E = _engine(A, 5)
        lg = _league(E, probs, [0, 1, 2, 1, 2], n_buffers=1)
        try:
            for c in cuts:
                lg.steps(seed, c)
            blocks.append(U.split_row(_host_block(lg, 0)))
            slots.append(lg.assignment()[0])
        finally:
            lg.close(); E.close()
    for name in U.LLU_FIELDS:
        if name != 'R':
            assert np.array_equal(blocks[0][name].view(np.uint32), blocks[1][name].view(np.uint32)), name
    np.testing.assert_array_equal(slots[0], slots[1])
    assert (blocks[0]['A'] != blocks[2]['A']).any() and (slots[0] != slots[2]).any()
    np.testing.assert_array_equal(blocks[0]['X'][:, 0], blocks[2]['X'][:, 0])        # (the engines start alike)


def test_td_lambda_returns():
    """64 arenas, L 16: R of finish(0, 0.95, 0.95) against the float64 recursion on the recorded r, V, discount and the bootstrap.  Tolerance, the
    recorder's rule: 4 x the worst deviation of the same recursion in NumPy float32 from float64.  NULL bootstrap = the next block's first V;
    LL_ESTATE before that step has run."""
    import torch
    A, gamma, lam = 64, 0.95, 0.95
    E = _engine(A, 7)
    lg = _league(E, (0.5, 0.5), [0, 1, 2], n_buffers=2)
    try:
        lg.steps(3, L)
        with pytest.raises(Exception) as ei:
            lg.finish(0, gamma, lam)
        assert ei.value.code == LL_ESTATE and 'next unroll' in str(ei.value)
        lg.steps(3, 1)
        f0, f1 = lg.split_row(lg.block(0)), lg.split_row(lg.block(1))

        def host(x):
            torch.cuda.synchronize()
            return x.cpu().numpy()
        r, V, m, boot = host(f0['r']), host(f0['V']), host(f0['discount']), host(f1['V'][:, 0])
        assert np.isfinite(r).all() and np.isfinite(V).all() and set(np.unique(m)) <= {0.0, 1.0} and (m == 0).any() and np.ptp(V) > 0
        lg.finish(0, gamma, lam)
        R_null = host(f0['R'])
        ref64 = UR.td_lambda(r, V, m, boot, gamma, lam)
        dev32 = float(np.abs(UR.td_lambda(r, V, m, boot, gamma, lam, dtype=np.float32).astype(np.float64) - ref64).max())
        err = float(np.abs(R_null.astype(np.float64) - ref64).max())
        print('%d arenas, L %d: |R - float64| max %.3e; NumPy float32 recursion vs float64 max %.3e, allowed 4 x = %.3e' % (A, L, err, dev32, 4 * dev32))
        assert dev32 > 0 and err <= 4 * dev32, (err, dev32)
        bt = f1['V'][:, 0].clone()
        torch.cuda.synchronize()
        lg.finish(0, gamma, lam, bt.data_ptr())
        assert np.array_equal(host(f0['R']).view(np.uint32), R_null.view(np.uint32))
        with pytest.raises(Exception) as ei:
            lg.finish(1, gamma, lam)                           # block 1 holds no complete unroll
        assert ei.value.code == LL_ESTATE
        for b in (-1, 2):
            with pytest.raises(Exception) as ei:
                lg.finish(b)
            assert ei.value.code == LL_EINVAL
    finally:
        lg.close(); E.close()


def test_guards_and_canaries():
    """Refused calls return the stated code and leave the ring and position() untouched; one recorded unroll writes every column of block 0 except R,
    zeros in the pad, and nothing in block 1; the rows of a slot nobody can draw never get a state."""
    import torch
    from lifelike_agility_and_play_amd import capi
    from lifelike_agility_and_play_amd.policies import hl_league as LG
    PAT = 0x7FC0BEEF
    A, probs = 17, (0.6, 0.0, 0.4)
    E = _engine(A, 11)
    N = _sepmc_engine(4, 0, 11, max_steps=16)                  # no auto_reset
    lg = None
    try:
        for eng, k, code in ((E, 0, LL_EINVAL), (E, 9, LL_EINVAL), (N, 1, LL_EINVAL)):
            with pytest.raises(capi.LLError) as ei:
                LG.HlLeagueActor(eng, k, L, 2)
            assert ei.value.code == code and str(ei.value)
        for bad in ((0, 2), (L, 0)):
            with pytest.raises(capi.LLError) as ei:
                LG.HlLeagueActor(E, 1, *bad)
            assert ei.value.code == LL_EINVAL
        lg = LG.HlLeagueActor(E, 3, L, 2)
        ring = lg.buffers()
        ring.view(torch.int32).fill_(PAT)
        torch.cuda.synchronize()
        (w, v), (w1, _) = _weight_set(0), _weight_set(1)

        def refused(code, fn, *a, **kw):
            with pytest.raises(capi.LLError) as ei:
                fn(*a, **kw)
            assert ei.value.code == code and str(ei.value), (fn.__name__, a)

        refused(LL_ESTATE, lg.steps, 1, 1)                                   # no weights at all
        lg.set_weights(0, w, value_weights=v)
        refused(LL_ESTATE, lg.steps, 1, 1)                                   # every opponent can be drawn (1 / K each) and none has weights
        lg.set_weights(1, w1)
        lg.set_weights(3, w1)
        refused(LL_ESTATE, lg.steps, 1, 1)                                   # slot 2 still can
        refused(LL_EINVAL, lg.set_weights, 1, w1, value_weights=v)           # a vf for an opponent slot
        refused(LL_EINVAL, lg.set_weights, 0, w)                             # the learner without one
        refused(LL_EINVAL, lg.set_weights, 4, w1)
        refused(LL_EINVAL, lg.set_weights, -1, w1)
        refused(LL_EINVAL, lg.set_weights, 1, w1[:-1])
        for bad in ((0.5, 0.5), (0.5, 0.25, 0.2), (0.7, -0.1, 0.4), (0.5, float('nan'), 0.5), (0.5, 0.25, 0.25 + 1e-5)):
            refused(LL_EINVAL, lg.set_probs, bad)
        refused(LL_ESTATE, lg.steps, 1, 1)                                   # (the refused probabilities changed nothing)
        lg.set_probs(probs)
        for n_steps in (2 * L + 1, 0, -3):
            refused(LL_EINVAL, lg.steps, 1, n_steps)
        refused(LL_ESTATE, lg.finish, 0)
        refused(LL_ESTATE, lg.plan_only, 1)
        torch.cuda.synchronize()
        assert lg.position() == (0, 0) and bool((ring.view(torch.int32) == PAT).all()), 'a refused call wrote into the ring'
        assert not lg.assignment()[0].any() and not lg.outcomes().any()
        lg.steps(1, L)
        torch.cuda.synchronize()
        assert lg.position() == (1, 0)
        bits = ring.view(torch.int32)
        assert bool((bits[1] == PAT).all()), 'the other buffer was touched'
        roff = lg.fields['R'][0]
        assert bool((bits[0][..., roff] == PAT).all()), 'R written before finish'
        rest = torch.cat([bits[0][..., :roff], bits[0][..., roff + 1:]], dim=-1)
        assert not bool((rest == PAT).any()), 'a column of the recorded block was left unwritten'
        poff, pdim = lg.fields['pad']
        assert pdim == 1 and poff + pdim == lg.row_floats and not bool(bits[0][..., poff:].any())
        f = lg.split_row(ring[0])
        assert bool(torch.isfinite(f['X']).all()) and bool(torch.isfinite(f['S']).all()) and bool(torch.isfinite(f['A']).all())
        lg.steps(1, 1)                                                       # (its plan tallies the episodes step L - 1 ended: all that were still running)
        slot, episode = lg.assignment()
        assert set(np.unique(slot)) <= {1, 3} and (episode >= 2).all()
        before = lg.outcomes().copy()
        lg.plan_only(3)                                                      # measures, moves nothing
        s2, e2 = lg.assignment()
        np.testing.assert_array_equal(s2, slot); np.testing.assert_array_equal(e2, episode)
        np.testing.assert_array_equal(lg.outcomes(), before)
        got = lg.outcomes(clear=True)
        assert not got[1].any() and got[:, 0].sum() > 0 and not lg.outcomes().any()
        assert (got[:, 1:].sum(axis=1) >= got[:, 0]).all()                   # every finished episode has a reason
        st, vst = lg.state()
        assert np.abs(st).max() > 0 and np.abs(vst).max() > 0 and np.isfinite(st).all()
    finally:
        if lg is not None:
            lg.close()
        E.close(); N.close()


def test_zero_probability_slot_rows_are_untouched():
    """64 arenas, slot 2 of 2 with probability 0 and garbage-free: after 20 steps no arena sits in it, and switching the probabilities over makes
    every later draw take it -- the upload is ordered with the steps."""
    A = 64
    E = _engine(A, 13)
    lg = _league(E, (1.0, 0.0), [0, 1, None], n_buffers=2)
    try:
        lg.steps(5, 20)
        slot20, ep20 = lg.assignment()
        assert (slot20 == 1).all()
        with pytest.raises(Exception) as ei:
            lg.set_probs((0.0, 1.0)); lg.steps(5, 1)
        assert ei.value.code == LL_ESTATE                                    # slot 2 has no weights yet
        lg.set_weights(2, _weight_set(2)[0])
        lg.steps(5, 17)                                                       # queued behind the upload; an episode lasts at most 16 steps, so by step 36 ...
        slot, episode = lg.assignment()
        assert (episode > ep20).all() and (slot == 2).all()                   # ... every arena has drawn again, under the new probabilities
        o = lg.outcomes()
        assert o[0, 0] == episode.sum() - A - o[1, 0]                        # every finished episode sits under the slot it was played against
    finally:
        lg.close(); E.close()


def test_nothing_else_moved():
    """20 league steps with every slot holding the same weights against 20 steps of the existing recorder with that one policy on a twin engine: the
    engine's obs, reward and done, and the learner rows' recorded A, neglogp and V are the same bits."""
    from lifelike_agility_and_play_amd.policies import hl_unroll as U
    A, steps, seed = 64, 20, 0xBEE
    EA, EB = _engine(A, 13), _engine(A, 13)
    lg = _league(EA, (0.3, 0.3, 0.4), [0, 0, 0, 0], n_buffers=2, unroll=32)
    pol = _policy(0, 2 * A, True)
    rec = U.HlUnrollRecorder(EB, pol, 32, 2)
    try:
        lg.steps(seed, steps)
        rec.steps(seed, steps)
        assert np.array_equal(np.asarray(EA.obs()).view(np.uint32), np.asarray(EB.obs()).view(np.uint32))
        for a, b in zip(EA.reward_done(), EB.reward_done()):
            np.testing.assert_array_equal(a, b)
        import torch
        torch.cuda.synchronize()
        g, w = lg.split_row(lg.block(0).cpu().numpy()), rec.split_row(rec.block(0).cpu().numpy())
        for name in ('A', 'neglogp', 'V', 'X', 'S', 'M', 'r', 'discount'):
            np.testing.assert_array_equal(g[name][:, :steps], w[name][::2, :steps], err_msg=name)
        assert (g['M'][:, 1:steps] == 1.0).any(), 'no restart inside the unroll: M = 1 never recorded'
        st, vst = lg.state()
        np.testing.assert_array_equal(st, pol.state()[:2 * A])
        np.testing.assert_array_equal(vst, pol.value_state()[:2 * A:2])
        assert len(np.unique(lg.assignment()[0])) == 3
    finally:
        rec.close(); pol.close(); lg.close(); EA.close(); EB.close()
