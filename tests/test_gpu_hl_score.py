"""The teacher-forced scorer (include/hl/llenv_hl_score.h, policies.hl_score) on the GPU: fabricated blocks under other weights against the float64
reference (tests/hl_score_ref.py), the round trip through the recorder and the league -- a block scored under the weights it was recorded with
gives back its own neglogp and V --, and the guards that need a device."""
import numpy as np
import pytest

import hl_policy_pg_ref as G
import hl_policy_ref as R
import hl_score_ref as SR
import hl_unroll_ref as UR
from test_gpu_hl_policy_pg import _policy, _real_obs
from test_gpu_hl_unroll import _engine, _rows

pytestmark = pytest.mark.gpu
SEED = 0x5C0_4E5_EED
LL_EINVAL, LL_ESTATE = -1, -4
N_FAB, L_FAB = 33, 5
_FAB = {}


def _paths(kind):
    return (R.EPMC_WEIGHTS['hurdle'], G.EPMC_VALUE['hurdle']) if kind == 'epmc' else (R.SEPMC_WEIGHTS, G.SEPMC_VALUE)


def _s_layout(kind, st, vst):
    """device-layout states -> the S of a row: vf | pi (zeros) | z [| hlc]"""
    pi = np.zeros((len(st), 64), st.dtype)
    return np.concatenate([vst, pi, st] if kind == 'epmc' else [vst, pi, st[:, 64:128], st[:, 0:64]], axis=1)


def _fabricated(kind):
    """One block of 33 rows x 5 time steps per kind, made once: engine observations, S_0 ~ N(0, 0.4), M = 1 at a third of the (row, t > 0) cells, the
    heads sampled by the float32 NumPy actor reference under the fixture weights W_a; W_b = W_a with every array but the two normalisation arrays times
    (1 + 0.02 xi); the float64 scoring of the block under W_b and the tolerances (hl_score_ref.tolerances).  Every case below is a corner [:n, :L] of
    this block -- rows are independent and time step t depends on steps <= t only -- so the one reference serves them all."""
    if kind in _FAB:
        return _FAB[kind]
    from lifelike_agility_and_play_amd.policies import hl_unroll as U
    k = SR.KIND[kind]
    rng = np.random.default_rng(31 + k)
    real = _real_obs(kind, 'hurdle')
    path, vpath = _paths(kind)
    wa = R.load(path, np.float32)
    wva = G.load_value(vpath, wa)
    n, L = N_FAB, L_FAB
    obs = real[rng.integers(0, len(real), (L, n))].astype(np.float32)
    S0 = rng.normal(0.0, 0.4, (n, U.S_DIM[k])).astype(np.float32)
    M = rng.random((L, n)) < 1.0 / 3.0
    M[0] = False
    st = S0[:, 128:192] if kind == 'epmc' else np.concatenate([S0[:, 192:256], S0[:, 128:192]], axis=1)
    vst = S0[:, 0:64]
    rec = {key: [] for key in ('code', 'action', 'neglogp', 'value', 'heading', 'hs')}
    for t in range(L):
        rec['hs'].append(_s_layout(kind, st, vst))
        r = G.forward(kind, wa, obs[t], st, M[t], SEED, t, True, wv=wva, vstate=vst)
        st, vst = r['state'].astype(np.float32), r['vstate'].astype(np.float32)
        for key in ('code', 'action', 'neglogp', 'value'):
            rec[key].append(r[key])
        rec['heading'].append(r['heading'] if kind == 'sepmc' else np.zeros(n, np.float32))
    zero = np.zeros((L, n), np.float32)
    block = UR.pack_unroll(kind, obs, np.stack(rec['code']), np.stack(rec['action']), np.stack(rec['neglogp']), np.stack(rec['value']), zero, zero,
                           np.stack(rec['hs']), M, heading=np.stack(rec['heading']), dtype=np.float32)
    f = U.split_row(block, U.row_layout(k)[0])
    f['S'][:, 0] = S0                                    # (the pi part too: never read)
    f['M'][::3, 0] = 1.0                                 # M of the first frame is ignored
    assert (f['M'][:, 1:] == 1.0).mean() > 0.2 and np.isfinite(block).all()
    wb, wvb = SR.perturbed(wa, rng), SR.perturbed(wva, rng)
    wb64, wvb64 = {i: a.astype(np.float64) for i, a in wb.items()}, {i: a.astype(np.float64) for i, a in wvb.items()}
    t = SR.tolerances(kind, wb64, wvb64, wb, wvb, block)
    print('%s fabricated %d x %d: float32 - float64 %s' % (kind, n, L, ' '.join('%s %.3g' % kv for kv in sorted(t['dev'].items()))))
    _FAB[kind] = dict(block=block, wa=SR.pack(kind, wa, wva), wb=SR.pack(kind, wb, wvb), wb64=wb64, t=t)
    return _FAB[kind]


def _carrier(kind, fab, max_rows=16):
    """the weight carrier: made with W_a, given states of its own (scoring must not touch them), then handed W_b by set_weights"""
    from lifelike_agility_and_play_amd.policies import hl_policy_hip as H
    pol = (H.HipEpmcPolicy if kind == 'epmc' else H.HipSepmcPolicy)(None, max_rows, weights=fab['wa'][0])
    pol.attach_value(weights=fab['wa'][1])
    rng = np.random.default_rng(7)
    pol.set_state(rng.normal(0, 0.4, (max_rows, pol.state_dim)).astype(np.float32))
    pol.set_value_state(rng.normal(0, 0.4, (max_rows, 64)).astype(np.float32))
    pol.set_weights(weights=fab['wb'][0], value_weights=fab['wb'][1])
    return pol


def _score_rows(pol, rows, n, L, extra=3):
    """rows [n][L][rf] (host) scored into a NaN-filled buffer of n + extra rows -> the whole buffer on the host"""
    import torch
    from lifelike_agility_and_play_amd.policies import hl_score as SC
    d_rows = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    d_out = torch.full((n + extra, L, SC.LLS_OUT_FLOATS), float('nan'), device='cuda')
    torch.cuda.synchronize()
    SC.score_rows(pol, d_rows.data_ptr(), n, L, d_out.data_ptr())
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


@pytest.mark.parametrize('kind', ['epmc', 'sepmc'])
def test_fabricated_blocks_against_float64(kind):
    """n_rows 1, 16, 17, 33 x unroll_length 1, 5 of the fabricated block, scored under W_b by a carrier of max_rows 16: every output within the tolerances
    of the float64 reference, the Gaussian entropies the constant formulas, pad columns zero, rows >= n_rows of an over-allocated NaN-filled d_out
    untouched, rows 0..16 the same bits at n_rows 17 and 33, and the carrier's own state and value state the same bits before and after."""
    from lifelike_agility_and_play_amd.policies import hl_score as SC
    fab = _fabricated(kind)
    k = SR.KIND[kind]
    t = fab['t']
    pol = _carrier(kind, fab)
    try:
        st0, vst0 = pol.state(), pol.value_state()
        head = {}
        for L in (1, L_FAB):
            for n in (1, 16, 17, N_FAB):
                what = '%s n_rows %d, unroll_length %d' % (kind, n, L)
                out = _score_rows(pol, fab['block'][:n, :L], n, L)
                assert np.isnan(out[n:]).all(), what + ': rows >= n_rows written'
                got = out[:n]
                assert np.isfinite(got).all(), what
                f = SC.split_out(got, k)
                assert not f['pad'].any(), what
                err = SR.errors(kind, got, t['ref'][:n, :L])
                print(what, ' '.join('%s %.3g (tol %.3g)' % (g, e, t['tol'][g]) for g, e in sorted(err.items())))
                for g, e in err.items():
                    assert e <= t['tol'][g], '%s: %s off the float64 reference by %.3g (tolerance %.3g)' % (what, g, e, t['tol'][g])
                for col, val in SR.gaussian_entropy(kind, fab['wb64']).items():
                    assert np.abs(got[..., col] - val).max() <= t['tol']['entropy'], (what, col)
                if n >= 17:
                    head.setdefault(L, []).append(got[:17].copy())
        for L, (a, b) in head.items():
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), 'rows 0..16 depend on n_rows (unroll_length %d)' % L
        assert np.array_equal(pol.state().view(np.uint32), st0.view(np.uint32)) and np.array_equal(pol.value_state().view(np.uint32), vst0.view(np.uint32))
    finally:
        pol.close()


def _host(x):
    import torch
    torch.cuda.synchronize()
    return x.cpu().numpy()


@pytest.mark.parametrize('kind,n,sample', [('epmc', 33, False), ('epmc', 33, True), ('sepmc', 17, False), ('sepmc', 17, True)])
def test_round_trip_through_the_recorder(kind, n, sample):
    """EPMC hurdles at 33 envs / SEPMC at 17 arenas, L 8, 2 buffers, max_steps 4, 17 steps: every episode ends within 4 steps, so M = 1 occurs at t > 0
    and a restart falls on the first frame of unroll 1.  Blocks 0 and 1 are scored with the actor's own policy object.  They are scored after step 16:
    the 17th step is the first of unroll 2 and overwrites the first frame of block 0 (two buffers), after which block 0 is no one unroll any more --
    it is then scored once more and its new first frame checked, which starts from its own S like any first frame.
    sample = 0: every neglogp column and V equal the recorded ones bit for bit.  sample = 1: V and the z neglogp bit for bit, every output within the
    tolerances of the float64 reference on the recorded block, the largest difference of the Gaussian heads from the recorded values printed.
    Scoring leaves the blocks' bytes, the recorder's position and the policy's two states as they were."""
    import torch
    from lifelike_agility_and_play_amd.policies import hl_score as SC
    from lifelike_agility_and_play_amd.policies import hl_unroll as U
    L = 8
    rows = _rows(kind, n)
    k = SR.KIND[kind]
    nh = 2 if kind == 'epmc' else 3
    E = _engine(kind, n, 5, 4)
    pol, path, vpath = _policy(kind, 'hurdle', rows)
    rec = U.HlUnrollRecorder(E, pol, L, 2)
    try:
        rec.steps(SEED, 2 * L, sample)
        ring0 = _host(rec.buffers()).copy()
        st0, vst0 = pol.state(), pol.value_state()
        outs = [SC.score(pol, rec, b) for b in (0, 1)]
        assert rec.position() == (2, 0)
        ring1 = _host(rec.buffers())
        assert np.array_equal(ring0.view(np.uint32), ring1.view(np.uint32)), 'scoring wrote into the blocks'
        assert np.array_equal(pol.state().view(np.uint32), st0.view(np.uint32)) and np.array_equal(pol.value_state().view(np.uint32), vst0.view(np.uint32))
        late_masks = 0
        if sample:
            w64, w32 = R.load(path), R.load(path, np.float32)
            wv64, wv32 = G.load_value(vpath, w64), G.load_value(vpath, w32)
        for b in (0, 1):
            what = '%s %d rows sample=%d block %d' % (kind, rows, sample, b)
            assert tuple(outs[b].shape) == (rows, L, 8) and outs[b].ll_kind == k
            got = _host(outs[b])
            g, f = SC.split_out(got, k), U.split_row(ring0[b])
            assert np.isfinite(got).all() and not g['pad'].any(), what
            late_masks += int((f['M'][:, 1:] == 1.0).sum())
            bit = lambda a, c: np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(c).view(np.uint32))      # noqa: E731
            assert bit(g['V'], f['V']), what + ': V'
            assert bit(g['neglogp'][..., nh - 2], f['neglogp'][..., nh - 2]), what + ': z neglogp'
            if not sample:
                assert bit(g['neglogp'], f['neglogp']), what + ': neglogp'
            else:
                t = SR.tolerances(kind, w64, wv64, w32, wv32, ring0[b])
                err = SR.errors(kind, got, t['ref'])
                print(what, ' '.join('%s %.3g (tol %.3g)' % (gr, e, t['tol'][gr]) for gr, e in sorted(err.items())),
                      '| Gaussian neglogp - recorded: max %.3g' % np.abs(np.delete(g['neglogp'], nh - 2, axis=-1) - np.delete(f['neglogp'], nh - 2, axis=-1)).max())
                for gr, e in err.items():
                    assert e <= t['tol'][gr], '%s: %s off the float64 reference by %.3g (tolerance %.3g)' % (what, gr, e, t['tol'][gr])
        assert late_masks > 0, 'no M = 1 at t > 0'
        f1 = U.split_row(ring0[1])
        assert not f1['M'][:, 0].any() and (np.abs(f1['S'][:, 0]).max(axis=1) == 0).any(), 'no restart on the first frame of unroll 1'
        # the 17th step: block 1 scores to the same bits, the position is the recorder's, and block 0's new first frame gives back its own values
        rec.steps(SEED, 1, sample)
        again = _host(SC.score(pol, rec, 1))
        assert np.array_equal(again.view(np.uint32), _host(outs[1]).view(np.uint32)) and rec.position() == (2, 1)
        g0 = SC.split_out(_host(SC.score(pol, rec, 0)), k)
        f0 = U.split_row(_host(rec.block(0)))
        np.testing.assert_array_equal(g0['V'][:, 0], f0['V'][:, 0])
        np.testing.assert_array_equal(g0['neglogp'][:, 0, nh - 2], f0['neglogp'][:, 0, nh - 2])
    finally:
        torch.cuda.synchronize()
        rec.close(); pol.close(); E.close()


def test_league_blocks():
    """17 arenas, 2 opponents, L 8, max_steps 4, 17 steps: blocks 0 and 1 (scored after step 16, see above) under an ordinary SEPMC policy of max_rows 16
    holding slot 0's weights and value branch: n_rows is the arena count, V and the z neglogp are the recorded bits."""
    from lifelike_agility_and_play_amd.policies import hl_policy_hip as H
    from lifelike_agility_and_play_amd.policies import hl_score as SC
    from test_gpu_hl_league import _league, _weight_set
    from test_gpu_hl_league import _engine as _league_engine
    A, L = 17, 8
    E = _league_engine(A, 9, max_steps=4)
    lg = _league(E, (0.5, 0.5), [0, 1, 2], n_buffers=2, unroll=L)
    w, v = _weight_set(0)
    pol = H.HipSepmcPolicy(None, 16, weights=w)
    pol.attach_value(weights=v)
    try:
        lg.steps(SEED, 2 * L)
        outs = [SC.score(pol, lg, b) for b in (0, 1)]
        for b in (0, 1):
            assert tuple(outs[b].shape) == (A, L, 8)
            g, f = SC.split_out(_host(outs[b]), H.LLH_SEPMC), lg.split_row(_host(lg.block(b)))
            assert np.isfinite(_host(outs[b])).all()
            np.testing.assert_array_equal(g['V'], f['V'], err_msg='block %d V' % b)
            np.testing.assert_array_equal(g['neglogp'][..., 1], f['neglogp'][..., 1], err_msg='block %d z neglogp' % b)
        lg.steps(SEED, 1)
        assert lg.position() == (2, 1)
        assert np.array_equal(_host(SC.score(pol, lg, 1)).view(np.uint32), _host(outs[1]).view(np.uint32))
    finally:
        pol.close(); lg.close(); E.close()


def test_guards():
    """A carrier without a value branch, a kind mismatch, a buffer out of range: LL_EINVAL; a block that holds no complete unroll: LL_ESTATE; NULL and
    non-positive arguments with a real carrier: LL_EINVAL.  None of them writes d_out."""
    import torch
    from lifelike_agility_and_play_amd import capi
    from lifelike_agility_and_play_amd.policies import hl_score as SC
    from lifelike_agility_and_play_amd.policies import hl_unroll as U
    L, n = 8, 16
    E = _engine('epmc', n, 3, 16)
    pol = _policy('epmc', 'hurdle', n)[0]
    novalue = _policy('epmc', 'hurdle', n, value=False)[0]
    other = _policy('sepmc', None, n)[0]
    rec = U.HlUnrollRecorder(E, pol, L, 2)
    try:
        out = torch.full((n, L, 8), float('nan'), device='cuda')
        rows = torch.zeros((n, L, 1128), device='cuda')
        torch.cuda.synchronize()

        def refused(code, fn, *a):
            with pytest.raises(capi.LLError) as ei:
                fn(*a)
            assert ei.value.code == code and str(ei.value), a

        refused(LL_ESTATE, SC.score, pol, rec, 0, out)                       # nothing recorded
        rec.steps(SEED, L - 1)
        refused(LL_ESTATE, SC.score, pol, rec, 0, out)                       # one step short of an unroll
        rec.steps(SEED, 1)
        refused(LL_ESTATE, SC.score, pol, rec, 1, out)                       # block 1 holds no complete unroll
        for b in (-1, 2):
            refused(LL_EINVAL, SC.score, pol, rec, b, out)
        refused(LL_EINVAL, SC.score, other, rec, 0, out)                     # an LLH_SEPMC carrier for EPMC rows
        refused(LL_EINVAL, SC.score, novalue, rec, 0, out)
        refused(LL_EINVAL, SC.score_rows, novalue, rows.data_ptr(), n, L, out.data_ptr())
        for bad in ((0, L), (n, 0), (-1, L), (n, -2)):
            refused(LL_EINVAL, SC.score_rows, pol, rows.data_ptr(), bad[0], bad[1], out.data_ptr())
        refused(LL_EINVAL, SC.score_rows, pol, 0, n, L, out.data_ptr())
        refused(LL_EINVAL, SC.score_rows, pol, rows.data_ptr(), n, L, 0)
        with pytest.raises(ValueError):
            SC.score(pol, rec, 0, out[:, :4])
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()) and rec.position() == (1, 0), 'a refused call wrote d_out or moved the recorder'
        SC.score(pol, rec, 0, out)                                           # ... and the complete block is accepted
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all())
    finally:
        torch.cuda.synchronize()
        rec.close()
        for x in (pol, novalue, other, E):
            x.close()


@pytest.mark.parametrize('kind', ['epmc', 'sepmc'])
def test_code_out_of_range_is_nan_and_nothing_else(kind):
    """A code of 300 and a code of -1 planted in one row of the fabricated block: that row's z and llc columns (neglogp and entropy) of those two time
    steps are NaN, and every other cell of the output is the same bits as without them."""
    from lifelike_agility_and_play_amd.policies import hl_unroll as U
    fab = _fabricated(kind)
    k = SR.KIND[kind]
    nh = 2 if kind == 'epmc' else 3
    pol = _carrier(kind, fab)
    try:
        clean = _score_rows(pol, fab['block'], N_FAB, L_FAB)
        planted = fab['block'].copy()
        f = U.split_row(planted, U.row_layout(k)[0])
        az = nh - 2
        f['A'][20, 1, az], f['A'][20, 3, az] = 300.0, -1.0
        got = _score_rows(pol, planted, N_FAB, L_FAB)
        bad = np.zeros(got.shape, bool)
        for t in (1, 3):
            bad[20, t, [nh - 2, nh - 1, 2 * nh - 2, 2 * nh - 1]] = True
        assert np.isnan(got[bad]).all()
        assert np.array_equal(got[~bad].view(np.uint32), clean[~bad].view(np.uint32))
        assert np.isfinite(clean[:N_FAB]).all()
    finally:
        pol.close()
