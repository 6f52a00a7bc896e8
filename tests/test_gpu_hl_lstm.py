"""The LN-LSTM core (include/hl/llenv_hl_lstm.h, policies.hl_lstm) on the GPU against the float64 pass of tests/hl_lstm_ref.py.

Bars (hl_lstm_ref.bars): per output array the larger of 4 x the worst deviation of the float32 NumPy pass of the same statement on the same inputs and
4 2^-24 max|ref|; a bar may not exceed 1e-3 max|ref| (tests/test_hl_lstm_ref.py asserts that for every case here that needs no GPU to build; the chain case
asserts it itself).  Every call gets NaN-filled, over-allocated outputs, tape and workspace; nothing may be written beyond the outputs and the inputs must
be the same bits afterwards.  The shapes come from the kernels' constants, named in hl_lstm_ref."""
import numpy as np
import pytest

import hl_lstm_ref as T

pytestmark = pytest.mark.gpu
EXTRA = 24            # floats past the end of every output, the tape and the workspace


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class _Dev(object):
    """the weights of one case on the device, and raw calls with guarded buffers"""

    def __init__(self, w):
        import torch
        from lifelike_agility_and_play_amd.policies import hl_lstm as HT
        self.HT, self.torch = HT, torch
        self.lib = HT.load_library()
        self.D = int(w[10].shape[0])
        self.w_host = [np.ascontiguousarray(np.asarray(a, np.float32)) for a in w]
        self.w = [torch.from_numpy(a).cuda() for a in self.w_host]
        self.ws = HT.weights_struct([t.data_ptr() for t in self.w], self.D)

    def _nan(self, n):
        return self.torch.full((int(n) + EXTRA,), float('nan'), dtype=self.torch.float32, device='cuda')

    def call(self, E, S0, M, dY, dS=None, s0=None, m=None, dy=None, y_stride=None, keep=None, inference=False):
        """forward and backward on host arrays -> dict(Y, S_end, dE, dS0, wgrad) on the host.  s0 = (address, row stride), m = (address, row stride, step
        stride), dy = (address, stride) take the place of the dense uploads; keep: tensors to hold alive and to compare afterwards as {name: (tensor, host)}."""
        torch, HT = self.torch, self.HT
        n, L = E.shape[:2]
        D = self.D
        ys = y_stride or D
        tape_bytes, work_bytes = HT.workspace_bytes(n, L, D, self.lib)
        ins = {'E': np.ascontiguousarray(E, np.float32)}
        if s0 is None:
            ins['S0'] = np.ascontiguousarray(S0, np.float32)
        if m is None:
            ins['M'] = np.ascontiguousarray(M, np.float32)
        if dy is None and dY is not None:
            ins['dY'] = np.ascontiguousarray(dY, np.float32)
        if dS is not None:
            ins['dS'] = np.ascontiguousarray(dS, np.float32)
        dev = {k: torch.from_numpy(v).cuda() for k, v in ins.items()}
        s0 = s0 or (dev['S0'].data_ptr(), 64)
        m = m or (dev['M'].data_ptr(), L, 1)
        dy = dy or ((dev['dY'].data_ptr(), D) if 'dY' in dev else None)
        Y, S_end, tape = self._nan(n * L * ys), self._nan(n * 64), self._nan(tape_bytes // 4)
        dE, dS0, wg, work = self._nan(n * L * 256), self._nan(n * 64), self._nan(37568 + 33 * D), self._nan((work_bytes + 15) // 16 * 4)
        torch.cuda.synchronize()
        if inference:
            HT.forward(self.ws, dev['E'].data_ptr(), s0[0], s0[1], m[0], m[1], m[2], n, L, Y.data_ptr(), ys, None, None, 0, lib=self.lib)
            torch.cuda.synchronize()
            assert bool(torch.isnan(S_end).all()) and bool(torch.isnan(tape).all())
            return dict(Y=Y[:n * L * ys].cpu().numpy().reshape(n, L, ys)[..., :D])
        HT.forward(self.ws, dev['E'].data_ptr(), s0[0], s0[1], m[0], m[1], m[2], n, L, Y.data_ptr(), ys, S_end.data_ptr(), tape.data_ptr(), tape_bytes, lib=self.lib)
        HT.backward(self.ws, dev['E'].data_ptr(), m[0], m[1], m[2], n, L, tape.data_ptr(), tape_bytes, dy[0], dy[1], dev['dS'].data_ptr() if dS is not None else None,
                    dE.data_ptr(), dS0.data_ptr(), wg.data_ptr(), work.data_ptr(), work_bytes, lib=self.lib)
        torch.cuda.synchronize()
        sizes = dict(Y=n * L * ys, S_end=n * 64, tape=tape_bytes // 4, dE=n * L * 256, dS0=n * 64, wgrad=37568 + 33 * D, work=work_bytes // 4)
        bufs = dict(Y=Y, S_end=S_end, tape=tape, dE=dE, dS0=dS0, wgrad=wg, work=work)
        for k, b in bufs.items():
            assert bool(torch.isnan(b[sizes[k]:]).all()), '%s: written beyond its end' % k
        for k, v in ins.items():
            assert np.array_equal(_bits(dev[k].cpu().numpy()), _bits(v)), '%s changed' % k
        for t, h in zip(self.w, self.w_host):
            assert np.array_equal(_bits(t.cpu().numpy()), _bits(h)), 'a weight array changed'
        for k, (t, h) in (keep or {}).items():
            assert np.array_equal(_bits(t.cpu().numpy()), _bits(h)), '%s changed' % k
        out = {k: bufs[k][:sizes[k]].cpu().numpy() for k in ('Y', 'S_end', 'dE', 'dS0', 'wgrad')}
        Yf = out['Y'].reshape(n, L, ys)
        assert np.isnan(Yf[..., D:]).all(), 'Y: written between the frames'
        out.update(Y=Yf[..., :D], S_end=out['S_end'].reshape(n, 64), dE=out['dE'].reshape(n, L, 256), dS0=out['dS0'].reshape(n, 64))
        return out


def _check(what, got, ref, bar, keys=None):
    for k in keys or ('Y', 'S_end', 'dE', 'dS0', 'wgrad'):
        assert got[k].shape == ref[k].shape and np.isfinite(got[k]).all(), '%s %s: shape or a non-finite value' % (what, k)
        top, err = float(np.abs(ref[k]).max()), float(np.abs(got[k].astype(np.float64) - ref[k]).max())
        print('%s %s: off %.3g, bar %.3g, max|ref| %.3g' % (what, k, err, bar[k], top))
        assert bar[k] <= T.CAP * top, '%s %s: the bar %.3g exceeds 1e-3 max|ref| = %.3g: a badly chosen case' % (what, k, bar[k], T.CAP * top)
        assert err <= bar[k], '%s %s: off by %.3g, bar %.3g (max|ref| %.3g)' % (what, k, err, bar[k], top)


@pytest.mark.parametrize('D', [1, 12, 256])
@pytest.mark.parametrize('shape', T.GPU_SHAPES, ids=lambda s: '%dx%d' % s)
def test_cases_against_float64(shape, D):
    """every output of a forward and a backward call within its bar; guarded buffers; inputs untouched.  Resets on a fifth of the steps, one zero-state row
    from three rows up, a dS_end."""
    w, (E, S0, M, dY, dS) = T.gpu_case(shape, D)
    ref, bar = T.bars(w, E, S0, M, dY, dS)
    got = _Dev(w).call(E, S0, M, dY, dS)
    _check('%dx%d D %d' % (shape + (D,)), got, ref, bar)
    off, dim, _ = T.layout(D)
    g = [got['wgrad'][o:o + d] for o, d in zip(off, dim)]
    assert np.array_equal(_bits(g[2]), _bits(g[3])) and np.array_equal(_bits(g[2]), _bits(g[5])), 'd b, d beta_x and d beta_h are the same numbers'


@pytest.mark.parametrize('D', [1, 12])
def test_special_inputs(D):
    """M all zero, M non-zero at every step, M of 2.0, -1 and NaN; all rows from a zero S0; no dS_end; Y with a stride and without a tape; dY = 0; dS_end
    alone at L = 1"""
    shape = (17, 3)
    w, (E, S0, M, dY, dS) = T.gpu_case(shape, D)
    dev = _Dev(w)
    n, L = shape
    odd = np.zeros_like(M)
    odd[:, 1], odd[::2, 2], odd[1::2, 2] = 2.0, -1.0, np.nan
    odd[0, 1] = 0.0
    for what, Mx, S0x, dSx in (('M = 0', np.zeros_like(M), S0, dS), ('M != 0', np.ones_like(M), S0, dS), ('M 2, -1, NaN', odd, S0, None), ('S0 = 0', M, np.zeros_like(S0), dS)):
        ref, bar = T.bars(w, E, S0x, Mx, dY, dSx)
        _check(what, dev.call(E, S0x, Mx, dY, dSx, y_stride=D + 3), ref, bar)
        _check(what + ', no tape', dev.call(E, S0x, Mx, dY, inference=True), ref, bar, keys=('Y',))
    # the cut by the device's own answer: rows whose every later step resets take nothing from dS_end
    allset = dev.call(E, S0, np.ones_like(M), np.zeros_like(dY), dS)
    assert not allset['dS0'].any() and not allset['dE'][:, :L - 1].any() and allset['dE'][:, L - 1].any()
    zero = dev.call(E, S0, M, np.zeros_like(dY), None)
    for k in ('dE', 'dS0', 'wgrad'):
        assert not zero[k].any(), 'dY = 0 must give an all-zero %s' % k
    ref, bar = T.bars(w, E[:, :1], S0, M[:, :1], np.zeros_like(dY[:, :1]), dS)
    _check('dS_end alone', dev.call(E[:, :1], S0, M[:, :1], np.zeros_like(dY[:, :1]), dS), ref, bar)


def _fabricated_block(kind, n, L, seed):
    """a block in the row layout of llenv_hl_unroll.h with a full observation, a recurrent state in the first frame and resets"""
    import hl_loss_ref as LR
    from lifelike_agility_and_play_amd.policies import hl_unroll as U
    block, score = LR.fabricate(kind, n, L, seed)
    lay, rf = U.row_layout(LR.KIND[kind])
    f = U.split_row(block, lay)
    rng = np.random.default_rng(seed + 1)
    f['X'][:] = rng.normal(0.0, 1.0, f['X'].shape)
    f['S'][:] = rng.uniform(-0.5, 0.5, f['S'].shape)
    f['M'][:] = rng.uniform(0, 1, (n, L)) < 0.25
    f['M'][0] = 0
    return block, score, lay, rf, f


@pytest.mark.parametrize('kind', ['epmc', 'sepmc'])
def test_chain_block_to_loss_to_bptt(kind):
    """record layout -> value of the block under perturbed weights -> ll_hl_loss_rows -> BPTT: S0 and M are read in place out of the block (strides), E is the
    reference embed of the block's observations, the forward's Y is the scored V, and dY is the V column of the loss's d_grad at stride 8, in place."""
    import torch
    import hl_loss_ref as LR
    import hl_policy_pg_ref as G
    import hl_policy_ref as R
    import hl_score_ref as SR
    from lifelike_agility_and_play_amd.policies import hl_loss as HL
    n, L, nh = 5, 4, 2 if kind == 'epmc' else 3
    block, score, lay, rf, f = _fabricated_block(kind, n, L, 77 + nh)
    wp = R.load(R.EPMC_WEIGHTS['hurdle'] if kind == 'epmc' else R.SEPMC_WEIGHTS)
    wv = SR.perturbed(G.load_value(G.EPMC_VALUE['hurdle'] if kind == 'epmc' else G.SEPMC_VALUE, wp), np.random.default_rng(5))
    wv = {k: a.astype(np.float32).astype(np.float64) for k, a in wv.items()}
    w = T.branch_weights(kind, 'value', wv)
    E = np.stack([T.value_embed(kind, wv, f['X'][:, t]) for t in range(L)], axis=1).astype(np.float32)
    S0, M = f['S'][:, 0, :64].copy(), f['M'].copy()
    dev = _Dev(w)
    rows = torch.from_numpy(block).cuda()
    s0 = (rows.data_ptr() + 4 * lay['S'][0], L * rf)
    m = (rows.data_ptr() + 4 * lay['M'][0], L * rf, rf)
    # score: the forward's Y is the V column
    Y = dev.call(E, None, None, None, s0=s0, m=m, inference=True)['Y']
    score[..., 2 * nh] = Y[..., 0]
    d_score = torch.from_numpy(score).cuda()
    grad = torch.full((n, L, 8), float('nan'), device='cuda')
    stats = torch.empty(HL.LLL_N_STATS, dtype=torch.float64, device='cuda')
    nbytes = HL.workspace_bytes(n, L)
    work = torch.empty(nbytes // 8, dtype=torch.float64, device='cuda')
    HL.loss_rows(LR.KIND[kind], HL.default_config(), rows.data_ptr(), n, L, d_score.data_ptr(), None, grad.data_ptr(), stats.data_ptr(), work.data_ptr(), nbytes)
    torch.cuda.synchronize()
    g_host = grad.cpu().numpy()
    dY = g_host[..., 2 * nh:2 * nh + 1].copy()
    assert np.isfinite(dY).all() and dY.all(), 'every sample of the block is valid and has a value gradient'
    ref, bar = T.bars(w, E, S0, M, dY, None)
    got = dev.call(E, None, None, None, s0=s0, m=m, dy=(grad.data_ptr() + 4 * 2 * nh, 8), keep=dict(block=(rows, block), grad=(grad, g_host)))
    _check('%s chain' % kind, got, ref, bar)
    assert np.array_equal(_bits(got['Y']), _bits(Y)), 'the forward with a tape and without one'


def test_rows_are_independent_and_calls_reproducible():
    """row r's Y, S_end, dE and dS0 in an n-row call are the bits of a 1-row call; two calls give the same bits in every output"""
    shape, D = (17, 3), 12
    w, (E, S0, M, dY, dS) = T.gpu_case(shape, D)
    dev = _Dev(w)
    a, b = dev.call(E, S0, M, dY, dS), dev.call(E, S0, M, dY, dS)
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    for r in (0, 7, 8, 16):
        one = dev.call(E[r:r + 1], S0[r:r + 1], M[r:r + 1], dY[r:r + 1], dS[r:r + 1])
        for k in ('Y', 'S_end', 'dE', 'dS0'):
            assert np.array_equal(_bits(one[k][0]), _bits(a[k][r])), (r, k)
    shape = T.SECOND_FOLD_PASS
    w, (E, S0, M, dY, dS) = T.gpu_case(shape, 1)
    dev = _Dev(w)
    a, b = dev.call(E, S0, M, dY, dS), dev.call(E, S0, M, dY, dS)
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


def test_autograd_function():
    """ln_lstm's .grads are the bits of the raw calls; a second backward through a fresh forward agrees; bad tensors raise"""
    import torch
    from lifelike_agility_and_play_amd.policies import hl_lstm as HT
    shape, D = (17, 3), 12
    w, (E, S0, M, dY, dS) = T.gpu_case(shape, D)
    dev = _Dev(w)
    raw = dev.call(E, S0, M, dY, dS)
    off, dim, _ = T.layout(D)

    def run():
        Et, St = torch.from_numpy(E).cuda().requires_grad_(), torch.from_numpy(S0).cuda().requires_grad_()
        ws = [t.clone().requires_grad_() for t in dev.w]
        Y, S_end = HT.ln_lstm(Et, St, torch.from_numpy(M).cuda(), ws, D)
        ((Y * torch.from_numpy(dY).cuda()).sum() + (S_end * torch.from_numpy(dS).cuda()).sum()).backward()
        torch.cuda.synchronize()
        return dict(Y=Y.detach().cpu().numpy(), S_end=S_end.detach().cpu().numpy(), dE=Et.grad.cpu().numpy(), dS0=St.grad.cpu().numpy(),
                    wgrad=np.concatenate([t.grad.cpu().numpy().ravel() for t in ws])), [tuple(t.grad.shape) for t in ws]
    first, shp = run()
    second, _ = run()
    assert shp == HT.shapes(D)
    for k in raw:
        assert np.array_equal(_bits(first[k]), _bits(raw[k])), k
        assert np.array_equal(_bits(second[k]), _bits(raw[k])), k
    # Y alone: S_end's gradient is absent
    Et = torch.from_numpy(E).cuda().requires_grad_()
    Y, _ = HT.ln_lstm(Et, torch.from_numpy(S0).cuda(), torch.from_numpy(M).cuda(), dev.w, D)
    (Y * torch.from_numpy(dY).cuda()).sum().backward()
    torch.cuda.synchronize()
    only = dev.call(E, S0, M, dY, None)
    assert np.array_equal(_bits(Et.grad.cpu().numpy()), _bits(only['dE']))
    good = dict(E=torch.from_numpy(E).cuda(), S0=torch.from_numpy(S0).cuda(), M=torch.from_numpy(M).cuda())
    for name, bad in (('E', good['E'].double()), ('E', good['E'][:, :, :255]), ('E', good['E'].transpose(0, 1)), ('E', good['E'].cpu()), ('S0', good['S0'][:, :63]),
                      ('S0', good['S0'][:4]), ('M', good['M'][:, :2]), ('M', good['M'].half())):
        with pytest.raises(ValueError):
            HT.ln_lstm(*[(bad if k == name else good[k]) for k in ('E', 'S0', 'M')], dev.w, D)
    with pytest.raises(ValueError):
        HT.ln_lstm(good['E'], good['S0'], good['M'], dev.w[:10], D)
    with pytest.raises(ValueError):
        HT.ln_lstm(good['E'], good['S0'], good['M'], dev.w, D + 1)
    with pytest.raises(ValueError):
        HT.ln_lstm(good['E'], good['S0'], good['M'], dev.w[:9] + [dev.w[9].t().contiguous().t(), dev.w[10]], D)
