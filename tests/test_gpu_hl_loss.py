"""The PPO loss of a scored block (include/hl/llenv_hl_loss.h, policies.hl_loss) on the GPU against the float64 reference (tests/hl_loss_ref.py):
fabricated blocks in every mode, the identity block (made of exact ties), exclusions, reproducibility, and the round trip record -> finish -> score ->
loss through a recorder and a league.

The bars are derived, not measured (hl_loss_ref.bars): a float64 mean over N samples in any summation order, with an exp good to 4 ulp, agrees within
(N + 16) 2^-53 mean|term|; adv_std, loss and explained_variance get that bound propagated; every gradient entry lies within one float32 ulp of the
float32-rounded reference; counts, pad columns and excluded rows are exact."""
import itertools

import numpy as np
import pytest

import hl_loss_ref as LR

pytestmark = pytest.mark.gpu
SEED = 0x1055_5EED
LL_EINVAL, LL_ESTATE = -1, -4
COMBOS = [dict(mode=m, merge_heads=mh, vf_clip=vc) for m, mh, vc in itertools.product((LR.PPO, LR.PPO2), (1, 0), (0.0, 0.1))]
# the sweeps run ceil(cells / HLL_THREADS = 256) workgroups, at most HLL_MAX_GROUPS = 1024, each leaving one row of partials; a fold pass of the one folding
# workgroup takes HLL_THREADS = 256 rows.  257 x 256 cells are 257 workgroups: the last row of partials is folded in a second pass.
BIG = (257, 256)
SHAPES = [(1, 1), (1, 2), (3, 5), (64, 2), (65, 7), (513, 5), BIG]
_FAB = {}


def _cfg(lib, c):
    from lifelike_agility_and_play_amd.policies import hl_loss as HL
    return HL.default_config(lib, **c)


def _fabricated(kind, n, L):
    """block, score, weight of one shape, made once: hl_loss_ref.fabricate, then every sample that lies within 1e-6 of a clip boundary or a tie under any
    of the configurations used here gets its scored neglogp and V moved by 2e-3 (again until none is left), so that device and reference cannot differ
    by which side of a branch a rounding error falls on.  Weights: U(0.25, 2) with two zeros from three rows up, none (NULL) below."""
    key = (kind, n, L)
    if key not in _FAB:
        nh = 2 if kind == 'epmc' else 3
        block, score = LR.fabricate(kind, n, L, 100 * n + L + LR.KIND[kind])
        weight = None
        if n >= 3:
            weight = np.random.default_rng(n + L).uniform(0.25, 2.0, (n, L)).astype(np.float32)
            weight[1, 0] = weight[2, L - 2] = 0.0
        cfgs = [LR.config(ent_coef=0.01, vf_coef=0.5, **c) for c in COMBOS if L >= 2 or c['mode'] == LR.PPO]
        for _ in range(8):
            bad = np.zeros((n, L), bool)
            for cfg in cfgs:
                bad |= LR.near_tie_mask(kind, cfg, block, score, weight)
            if not bad.any():
                break
            score[bad, :nh] += np.float32(2e-3)
            score[bad, 2 * nh] += np.float32(2e-3)
        _FAB[key] = (block, score, weight)
    return _FAB[key]


class _Device(object):
    """block, score and weight of one case on the device, an over-allocated NaN-filled d_grad and d_stats, and the workspace"""

    def __init__(self, kind, block, score, weight, extra=2):
        import torch
        from lifelike_agility_and_play_amd.policies import hl_loss as HL
        self.HL, self.torch = HL, torch
        self.lib = HL.load_library()
        self.kind, (self.n, self.L) = LR.KIND[kind], score.shape[:2]
        self.rows = torch.from_numpy(np.ascontiguousarray(block)).cuda()
        self.score = torch.from_numpy(np.ascontiguousarray(score)).cuda()
        self.weight = torch.from_numpy(np.ascontiguousarray(weight)).cuda() if weight is not None else None
        self.grad = torch.empty((self.n + extra, self.L, 8), device='cuda')
        self.stats = torch.empty(HL.LLL_N_STATS + 4, dtype=torch.float64, device='cuda')
        self.nbytes = HL.workspace_bytes(self.n, self.L, self.lib)
        self.work = torch.empty(self.nbytes // 8, dtype=torch.float64, device='cuda')

    def run(self, cfg, weight='own'):
        """-> (d_stats [24], d_grad [n + extra][L][8]) on the host"""
        torch = self.torch
        self.grad.fill_(float('nan'))
        self.stats.fill_(float('nan'))
        self.work.fill_(float('nan'))                      # (its contents are irrelevant: a call that depended on them would show)
        w = self.weight if isinstance(weight, str) else weight
        torch.cuda.synchronize()
        self.HL.loss_rows(self.kind, cfg, self.rows.data_ptr(), self.n, self.L, self.score.data_ptr(), w.data_ptr() if w is not None else None,
                          self.grad.data_ptr(), self.stats.data_ptr(), self.work.data_ptr(), self.nbytes, lib=self.lib)
        torch.cuda.synchronize()
        return self.stats.cpu().numpy(), self.grad.cpu().numpy()


def _check(what, ref, cfg, stats, grad, n, nh):
    """device statistics and gradient against a reference result, to the bars of the module docstring"""
    assert np.isnan(stats[LR.N_STATS:]).all() and np.isnan(grad[n:]).all(), what + ': written beyond the outputs'
    stats, grad = stats[:LR.N_STATS], grad[:n]
    assert np.isfinite(stats).all() and np.isfinite(grad).all(), what
    bar = LR.bars(ref, cfg)
    err = np.abs(stats - ref['stats'])
    worst = int(np.argmax(np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), 0.0)))
    print('%s: N %d  statistic nearest its bar: %d, off %.3g (bar %.3g)' % (what, ref['n_valid'], worst, err[worst], bar[worst]))
    assert stats[1] == ref['stats'][1] and stats[2] == ref['stats'][2], what + ': counts'
    for i in range(LR.N_STATS):
        assert err[i] <= bar[i], '%s: statistic %d is %r, the reference %r: off by %.3g (bar %.3g)' % (what, i, stats[i], ref['stats'][i], err[i], bar[i])
    want = ref['grad'].astype(np.float32)
    ulp = np.spacing(np.abs(want))
    off = np.abs(grad.astype(np.float64) - want.astype(np.float64))
    assert (off <= ulp).all(), '%s: %d gradient entries beyond one float32 ulp, the worst %.3g ulp' % (what, int((off > ulp).sum()), float((off / ulp).max()))
    assert not grad[..., 2 * nh + 1:].any() and not grad[~ref['valid']].any(), what + ': pad columns / excluded rows'


@pytest.mark.parametrize('kind', ['epmc', 'sepmc'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_fabricated_blocks_against_float64(kind, shape):
    """both modes x merged / per head x vf_clip 0 / 0.1 on one fabricated block per shape ((1, 1) in ppo only): statistics and gradient to the bars, nothing
    written beyond [n_rows][L][8] and LLL_N_STATS doubles of NaN-filled over-allocated outputs, d_rows and d_score the same bits afterwards."""
    n, L = shape
    nh = 2 if kind == 'epmc' else 3
    block, score, weight = _fabricated(kind, n, L)
    dev = _Device(kind, block, score, weight)
    for c in COMBOS:
        if c['mode'] == LR.PPO2 and L < 2:
            continue
        c = dict(c, ent_coef=0.01, vf_coef=0.5)
        cfg = LR.config(**c)
        assert LR.near_ties(kind, cfg, block, score, weight) == 0
        ref = LR.evaluate(kind, cfg, block, score, weight)
        stats, grad = dev.run(_cfg(dev.lib, c))
        _check('%s %dx%d %s' % (kind, n, L, c), ref, cfg, stats, grad, n, nh)
        if n >= 65:
            assert 0 < ref['stats'][14] < 1, 'the case exercises neither branch of the surrogate'
    assert np.array_equal(dev.rows.cpu().numpy().view(np.uint32), block.view(np.uint32)) and np.array_equal(dev.score.cpu().numpy().view(np.uint32), score.view(np.uint32))


@pytest.mark.parametrize('kind', ['epmc', 'sepmc'])
def test_identity_block(kind):
    """The scored neglogp and V are the block's own, bit for bit: rho is exactly 1, approx_kl and clip_frac exactly 0, every neglogp gradient
    float32(a w / W) to the ulp bar, and with vf_clip > 0 the value terms tie and the unclipped branch is the active one: a case made of exact ties, on
    which device and reference agree by the tie rule alone."""
    n, L = 65, 7
    nh = 2 if kind == 'epmc' else 3
    block, score, weight = _fabricated(kind, n, L)
    from lifelike_agility_and_play_amd.policies import hl_unroll as U
    f = U.split_row(block, U.row_layout(LR.KIND[kind])[0])
    score = score.copy()
    score[..., :nh], score[..., 2 * nh] = f['neglogp'], f['V']
    dev = _Device(kind, block, score, weight)
    for c in COMBOS:
        c = dict(c, ent_coef=0.01, vf_coef=0.5)
        cfg = LR.config(**c)
        ref = LR.evaluate(kind, cfg, block, score, weight)
        assert not ref['clipped'].any() and not ref['vclipped'].any() and (ref['rho'] == 1.0).all()
        stats, grad = dev.run(_cfg(dev.lib, c))
        _check('%s identity %s' % (kind, c), ref, cfg, stats, grad, n, nh)
        assert not stats[11:17].any(), 'approx_kl and clip_frac must be exactly 0'
        q = (ref['adv_hat'] * np.where(ref['valid'], ref['w'], 0.0) / ref['stats'][0]).astype(np.float32)
        for h in range(nh):
            assert (np.abs(grad[:n, :, h].astype(np.float64) - q) <= np.spacing(np.abs(q))).all()
        if cfg['mode'] == LR.PPO:
            np.testing.assert_array_equal(grad[:n, :, 2 * nh] == 0, (f['V'] == f['R']) | ~ref['valid'])      # d/dv = v - R, the unclipped branch


def test_exclusions():
    """Weights with zeros, a negative and a NaN; a scorer-style NaN pair (z and llc neglogp and entropy of one time step); in ppo2 a NaN V, which excludes
    its own step and exactly the earlier steps of its row up to a discount = 0 step.  The counts are exact and apart, excluded rows are zero, and what
    remains equals the reference on the block with those samples taken out by weight.  A block with no valid sample: zeros and the right counts."""
    kind, n, L, nh = 'sepmc', 65, 7, 3
    block, score, weight = (a.copy() for a in _fabricated(kind, n, L))
    from lifelike_agility_and_play_amd.policies import hl_unroll as U
    f = U.split_row(block, U.row_layout(LR.KIND[kind])[0])
    weight[5, 1], weight[6, 2], weight[7, 3] = -1.0, np.nan, np.inf
    score[9, 2, [1, 2, 4, 5]] = np.nan
    for mode in (LR.PPO, LR.PPO2):
        sc = score.copy()
        want_nonfinite = 1
        if mode == LR.PPO2:
            f['discount'][11] = 1.0
            f['discount'][11, 1] = 0.0
            sc[11, 4, 2 * nh] = np.nan
            want_nonfinite = 4                            # (9, 2), and row 11 at t = 4 (its own v), 3 and 2 (through R); t = 1 cuts, t = 0 lies beyond
        c = dict(mode=mode, ent_coef=0.01)
        cfg = LR.config(**c)
        dev = _Device(kind, block, sc, weight)
        ref = LR.evaluate(kind, cfg, block, sc, weight)
        assert ref['stats'][1] == 5 and ref['stats'][2] == want_nonfinite          # two zeros of the fabricated weights, a negative, a NaN, an inf; none on the bootstrap step
        if mode == LR.PPO2:
            assert not ref['valid'][11, 2:5].any() and ref['valid'][11, :2].all() and ref['valid'][11, 5]
        stats, grad = dev.run(_cfg(dev.lib, c))
        _check('exclusions mode %d' % mode, ref, cfg, stats, grad, n, nh)
        assert (grad[:n, :, 2 * nh] != 0)[ref['valid']].all(), 'a valid sample without a value gradient'
        # the same block with the excluded samples taken out by weight and the NaNs replaced: the reference of the remaining samples
        w2, sc2 = np.where(ref['valid'], weight, 0.0).astype(np.float32), np.where(np.isfinite(sc), sc, 0.0).astype(np.float32)
        cell = np.ones((n, L), bool)
        cell[:, L - 1] = mode != LR.PPO2
        if mode == LR.PPO:
            ref2 = LR.evaluate(kind, cfg, block, sc2, w2)
            assert np.array_equal(ref2['valid'], ref['valid'])
            stats2 = ref2['stats'].copy()
            stats2[1], stats2[2] = ref['stats'][1], ref['stats'][2]
            _check('exclusions, removed', dict(ref2, stats=stats2), cfg, stats, grad, n, nh)
        none = dev.torch.zeros((n, L), device='cuda')
        stats, grad = dev.run(_cfg(dev.lib, c), weight=none)
        assert stats[1] == cell.sum() and not stats[[0] + list(range(2, LR.N_STATS))].any() and not grad[:n].any() and np.isnan(grad[n:]).all()


def test_reproducible_and_unit_weights_are_null():
    """two calls on the same inputs: the same bits in d_stats and d_grad; d_weight of all ones: the same bits as NULL"""
    kind, (n, L) = 'epmc', BIG
    block, score, weight = _fabricated(kind, n, L)
    dev = _Device(kind, block, score, weight)
    for c in (dict(mode=LR.PPO, vf_clip=0.1), dict(mode=LR.PPO2, merge_heads=0)):
        cfg = _cfg(dev.lib, c)
        a, b = dev.run(cfg), dev.run(cfg)
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint64 if x.dtype == np.float64 else np.uint32), y.view(np.uint64 if y.dtype == np.float64 else np.uint32))
        ones = dev.torch.ones((n, L), device='cuda')
        a, b = dev.run(cfg, weight=ones), dev.run(cfg, weight=None)
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint64 if x.dtype == np.float64 else np.uint32), y.view(np.uint64 if y.dtype == np.float64 else np.uint32))
        assert a[0][0] == n * L - (n if c['mode'] == LR.PPO2 else 0)


def _host(x):
    import torch
    torch.cuda.synchronize()
    return x.cpu().numpy()


def _loss_round_trip(kind, src, pol, k, nh, what):
    """finish, score under the recording weights, loss in both modes: against the reference on the downloaded block and score"""
    from lifelike_agility_and_play_amd.policies import hl_loss as HL
    from lifelike_agility_and_play_amd.policies import hl_score as SC
    src.finish(0)
    out = SC.score(pol, src, 0)
    block, score = _host(src.block(0)).copy(), _host(out).copy()
    assert np.isfinite(score).all() and np.isfinite(src.split_row(block)['R']).all()
    for c in (dict(mode=LR.PPO, ent_coef=0.01), dict(mode=LR.PPO2, ent_coef=0.01, merge_heads=0)):
        stats, grad = HL.ppo_loss(out, src, 0, HL.default_config(**c))
        assert grad.ll_kind == k and tuple(grad.shape) == tuple(out.shape) and stats.dtype.is_floating_point and stats.element_size() == 8
        stats, grad = _host(stats), _host(grad)
        cfg = LR.config(**c)
        ref = LR.evaluate(kind, cfg, block, score)
        pad = np.full(4, np.nan)
        _check('%s %s' % (what, c), ref, cfg, np.concatenate([stats, pad]), np.concatenate([grad, np.full((1,) + grad.shape[1:], np.nan, np.float32)]), grad.shape[0], nh)
        assert not stats[11:17].any(), what + ': approx_kl and clip_frac of a block scored under its own weights must be exactly 0'
        assert HL.named(stats)['W'] == ref['n_valid'] and set(SC.split_out(grad, k)) == {'neglogp', 'entropy', 'V', 'pad'}
    assert np.array_equal(_host(src.block(0)).view(np.uint32), block.view(np.uint32)), 'the loss wrote into the block'


@pytest.mark.parametrize('kind,n', [('epmc', 33), ('sepmc', 17)])
def test_round_trip_through_the_recorder(kind, n):
    """L 8, two buffers, L + 1 steps with sample = 0: finish(0), score under the recording weights, ll_hl_loss_unroll.  approx_kl and clip_frac are exactly 0,
    statistics and gradient match the reference on the downloaded block and score.  Before the unroll is complete: LL_ESTATE; a buffer out of range or a
    NULL pointer: LL_EINVAL; none of them writes."""
    import ctypes as C
    import torch
    from lifelike_agility_and_play_amd import capi
    from lifelike_agility_and_play_amd.policies import hl_loss as HL
    from lifelike_agility_and_play_amd.policies import hl_unroll as U
    from test_gpu_hl_policy_pg import _policy
    from test_gpu_hl_unroll import _engine, _rows
    L = 8
    rows, k, nh = _rows(kind, n), LR.KIND[kind], 2 if kind == 'epmc' else 3
    E = _engine(kind, n, 5, 4)
    pol = _policy(kind, 'hurdle', rows)[0]
    rec = U.HlUnrollRecorder(E, pol, L, 2)
    try:
        out = torch.zeros((rows, L, 8), device='cuda')
        grad = torch.full((rows, L, 8), float('nan'), device='cuda')

        def refused(code, *a, **kw):
            with pytest.raises(capi.LLError) as ei:
                HL.ppo_loss(*a, **kw)
            assert ei.value.code == code and str(ei.value)

        refused(LL_ESTATE, out, rec, 0, grad=grad)                    # nothing recorded
        rec.steps(SEED, L - 1, False)
        refused(LL_ESTATE, out, rec, 0, grad=grad)                    # one step short of an unroll
        rec.steps(SEED, 2, False)
        refused(LL_ESTATE, out, rec, 1, grad=grad)                    # block 1 holds one step
        for b in (-1, 2):
            refused(LL_EINVAL, out, rec, b, grad=grad)
        lib = HL.load_library()
        p = C.c_void_p(out.data_ptr())
        nbytes = HL.workspace_bytes(rows, L)
        cfg = HL.default_config(lib)
        for bad in range(4):                                           # d_score, d_grad, d_stats, d_work
            args = [p, p, p, p]
            args[bad] = None
            assert lib.ll_hl_loss_unroll(rec.h, 0, C.byref(cfg), args[0], None, args[1], args[2], args[3], nbytes) == LL_EINVAL
        assert lib.ll_hl_loss_unroll(rec.h, 0, None, p, None, p, p, p, nbytes) == LL_EINVAL
        assert lib.ll_hl_loss_unroll(rec.h, 0, C.byref(cfg), p, None, p, p, p, nbytes - 8) == LL_EINVAL
        with pytest.raises(ValueError):
            HL.ppo_loss(out[:, :4], rec, 0)
        torch.cuda.synchronize()
        assert bool(torch.isnan(grad).all()) and not bool(out.any()) and rec.position() == (1, 1), 'a refused call wrote or moved the recorder'
        _loss_round_trip(kind, rec, pol, k, nh, '%s %d rows through the recorder' % (kind, rows))
    finally:
        torch.cuda.synchronize()
        rec.close(); pol.close(); E.close()


def test_round_trip_through_the_league():
    """16 arenas, one opponent, L 8: the learner rows of block 0 through ll_hl_loss_league, under an ordinary SEPMC policy holding slot 0's weights"""
    import torch
    from lifelike_agility_and_play_amd import capi
    from lifelike_agility_and_play_amd.policies import hl_loss as HL
    from lifelike_agility_and_play_amd.policies import hl_policy_hip as H
    from test_gpu_hl_league import _league, _weight_set
    from test_gpu_hl_league import _engine as _league_engine
    A, L = 16, 8
    E = _league_engine(A, 9, max_steps=4)
    lg = _league(E, (1.0,), [0, 1], n_buffers=2, unroll=L)
    w, v = _weight_set(0)
    pol = H.HipSepmcPolicy(None, 16, weights=w)
    pol.attach_value(weights=v)
    try:
        out = torch.zeros((A, L, 8), device='cuda')
        with pytest.raises(capi.LLError) as ei:
            HL.ppo_loss(out, lg, 0)
        assert ei.value.code == LL_ESTATE
        lg.steps(SEED, L + 1, False)
        with pytest.raises(capi.LLError) as ei:
            HL.ppo_loss(out, lg, 2)
        assert ei.value.code == LL_EINVAL
        _loss_round_trip('sepmc', lg, pol, H.LLH_SEPMC, 3, 'league, %d learner rows' % A)
    finally:
        torch.cuda.synchronize()
        pol.close(); lg.close(); E.close()
