"""The statement of the LN-LSTM core (tests/hl_lstm_ref.py) held to what already stands, without a GPU: its backward against torch autograd in float64 and
against central differences, its forward against hl_policy_ref.lstm step by step, embed + core against hl_policy_pg_ref.value bit for bit, the identities the
header names (d b == d beta_x == d beta_h, the M cut, M[0] ignored), and the condition on the bars of every GPU case."""
import numpy as np
import pytest

import hl_lstm_ref as T
import hl_policy_pg_ref as G
import hl_policy_ref as R


def _random_weights(D, seed):
    rng = np.random.default_rng(seed)
    w = [rng.normal(0, 1 / np.sqrt(s[0]) if len(s) == 2 else 0.3, s) for s in T.shapes(D)]
    for i in (4, 6, 8):
        w[i] = 1.0 + w[i]                         # the gammas around one
    return w


def _torch_cell(w, E, S0, M, dY, dS_end):
    """the same cell in torch ops, float64 on the CPU, differentiated by autograd -> dict like hl_lstm_ref.evaluate"""
    import torch
    tt = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=True)
    wt = [tt(a) for a in w]
    wx, wh, b, bx, gx, bh, gh, bc, gc, wo, bo = wt
    Et, St = tt(E), tt(S0)
    cut = torch.tensor(T.resets(M))

    def ln(x, beta, gamma):
        m = x.mean(dim=1, keepdim=True)
        var = ((x - m) ** 2).mean(dim=1, keepdim=True)
        return (x - m) / torch.sqrt(var + 1e-12) * gamma + beta
    c, h = St[:, :32], St[:, 32:]
    ys = []
    for t in range(E.shape[1]):
        keep = (~cut[:, t])[:, None].to(torch.float64)
        c, h = c * keep, h * keep
        z = ln(Et[:, t] @ wx, bx, gx) + ln(h @ wh, bh, gh) + b
        i, f, o, g = torch.split(z, 32, dim=1)
        c = torch.sigmoid(f + 1) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(ln(c, bc, gc))
        ys.append(h @ wo + bo)
    Y, S_end = torch.stack(ys, dim=1), torch.cat([c, h], dim=1)
    loss = (Y * torch.tensor(np.asarray(dY, np.float64))).sum()
    if dS_end is not None:
        loss = loss + (S_end * torch.tensor(np.asarray(dS_end, np.float64))).sum()
    loss.backward()
    return dict(Y=Y.detach().numpy(), S_end=S_end.detach().numpy(), dE=Et.grad.numpy(), dS0=St.grad.numpy(), wgrad=T.pack([a.grad.numpy() for a in wt]))


@pytest.mark.parametrize('D', [1, 12, 256])
def test_backward_is_torch_autograd_in_float64(D):
    """resets, two zero-state rows and a dS_end: every array within 1e-10 of its largest entry"""
    w = _random_weights(D, 10 + D)
    E, S0, M, dY, dS = T.case(6, 7, D, 20 + D, zero_rows=(1, 4))
    assert T.resets(M)[:, 1:].any() and not S0[1].any()
    got, want = T.evaluate(w, E, S0, M, dY, dS), _torch_cell(w, E, S0, M, dY, dS)
    for k in want:
        top = np.abs(want[k]).max()
        assert top > 0 and np.abs(got[k] - want[k]).max() <= 1e-10 * top, (k, np.abs(got[k] - want[k]).max(), top)
    got, want = T.evaluate(w, E, S0, M, dY, None), _torch_cell(w, E, S0, M, dY, None)
    for k in want:
        assert np.abs(got[k] - want[k]).max() <= 1e-10 * np.abs(want[k]).max(), k


def test_backward_against_central_differences():
    """a dozen entries of E, S0 and the weights (none in the h of a zero-state step, where LN(v) is not smooth at the step of a difference)"""
    D = 12
    w = _random_weights(D, 3)
    E, S0, M, dY, dS = T.case(3, 4, D, 5)
    M[:] = 0
    M[1, 2] = 1.0
    E, S0 = E.astype(np.float64), S0.astype(np.float64)
    r = T.evaluate(w, E, S0, M, dY, dS)
    off, _, _ = T.layout(D)

    def loss(w_, E_, S_):
        Y, S_end = T.forward(w_, E_, S_, M)
        return float((Y * dY).sum() + (S_end * dS).sum())
    eps = 1e-6
    picks = [('E', (0, 0, 3)), ('E', (1, 1, 200)), ('E', (2, 3, 77)), ('S0', (0, 5)), ('S0', (2, 40)), ('S0', (1, 33))]
    picks += [(i, idx) for i, idx in ((0, (17, 5)), (0, (255, 127)), (1, (3, 64)), (2, (40,)), (4, (100,)), (6, (9,)), (7, (2,)), (8, (31,)), (9, (4, 7)), (10, (11,)))]
    for what, idx in picks:
        args = [[a.copy() for a in w], E.copy(), S0.copy()]
        tgt = args[1] if what == 'E' else args[2] if what == 'S0' else args[0][what]
        base = tgt[idx]
        tgt[idx] = base + eps
        up = loss(*args)
        tgt[idx] = base - eps
        dn = loss(*args)
        num = (up - dn) / (2 * eps)
        ana = r['dE'][idx] if what == 'E' else r['dS0'][idx] if what == 'S0' else r['wgrad'][off[what] + int(np.ravel_multi_index(idx, T.shapes(D)[what]))]
        assert abs(num - ana) <= 1e-6 * max(1.0, abs(ana)), (what, idx, num, ana)


@pytest.mark.parametrize('kind,branch', sorted(T.BRANCHES))
def test_forward_is_hl_policy_ref_lstm_step_by_step(kind, branch):
    """the shipped arrays of every branch: (c, h) after each step are hl_policy_ref.lstm's bits, and Y is h wo + bo"""
    w = R.load(R.EPMC_WEIGHTS['hurdle'] if kind == 'epmc' else R.SEPMC_WEIGHTS)
    if branch == 'value':
        w = G.load_value(G.EPMC_VALUE['hurdle'] if kind == 'epmc' else G.SEPMC_VALUE, w)
    k0, head, D = T.BRANCHES[(kind, branch)]
    ws = T.branch_weights(kind, branch, w)
    E, S0, M, _, _ = T.case(4, 5, D, 9)
    Y, S_end, steps = T.forward(ws, E, S0, M, tape=True)
    c, h = S0[:, :32].astype(np.float64), S0[:, 32:].astype(np.float64)
    for t in range(5):
        if t > 0:
            c, h = c.copy(), h.copy()
            c[M[:, t] != 0] = 0
            h[M[:, t] != 0] = 0
        c, h = R.lstm(w, E[:, t].astype(np.float64), c, h, k0)
        assert np.array_equal(steps[t]['h2'], h)
        assert np.array_equal(Y[:, t], h @ w[head[0]] + w[head[1]].reshape(-1))
    assert np.array_equal(S_end, np.concatenate([c, h], axis=1))


@pytest.mark.parametrize('kind', ['epmc', 'sepmc'])
def test_embed_and_core_are_the_value_branch_bit_for_bit(kind):
    w = R.load(R.EPMC_WEIGHTS['hurdle'] if kind == 'epmc' else R.SEPMC_WEIGHTS)
    wv = G.load_value(G.EPMC_VALUE['hurdle'] if kind == 'epmc' else G.SEPMC_VALUE, w)
    rng = np.random.default_rng(4)
    n, L = 3, 4
    obs = rng.normal(0, 1, (n, L, 916 if kind == 'epmc' else 965))
    st = rng.uniform(-0.5, 0.5, (n, 64))
    reset = rng.uniform(0, 1, (n, L)) < 0.3
    E = np.stack([T.value_embed(kind, wv, obs[:, t]) for t in range(L)], axis=1)
    Y, S_end = T.forward(T.branch_weights(kind, 'value', wv), E, st, reset.astype(np.float32))
    vst = st
    for t in range(L):
        v, vst = G.value(kind, wv, obs[:, t], vst, reset[:, t] if t > 0 else None)
        assert np.array_equal(v, Y[:, t, 0]), (kind, t)
    assert np.array_equal(vst, S_end)


def test_bias_and_betas_share_one_gradient_and_the_mask_cuts():
    D = 12
    w = _random_weights(D, 8)
    E, S0, M, dY, dS = T.case(4, 6, D, 12)
    M[:] = 0
    M[2, 3] = 2.0
    M[3, 2] = np.nan
    r = T.evaluate(w, E, S0, M, dY, dS)
    off, dim, total = T.layout(D)
    g = [r['wgrad'][o:o + d] for o, d in zip(off, dim)]
    assert np.array_equal(g[2], g[3]) and np.array_equal(g[2], g[5]) and g[2].any()
    assert total == 37568 + 33 * D and off[9] == 37568 and len(r['wgrad']) == total
    # nothing flows across a reset: S0 and the frames before it get no gradient from later ones, and do not reach later outputs
    late = dY.copy()
    late[2, :3] = 0
    late[3, :2] = 0
    rl = T.evaluate(w, E, S0, M, late, dS)
    assert not rl['dS0'][2].any() and not rl['dS0'][3].any() and rl['dS0'][0].all() and not rl['dE'][2, :3].any() and rl['dE'][2, 3:].any()
    E2, S2 = E.copy(), S0.copy()
    E2[2, :3] += 1.0
    S2[2] += 1.0
    Y2, Se2 = T.forward(w, E2, S2, M)
    Y1, Se1 = T.forward(w, E, S0, M)
    assert np.array_equal(Y2[2, 3:], Y1[2, 3:]) and np.array_equal(Se2[2], Se1[2]) and not np.array_equal(Y2[2, :3], Y1[2, :3])
    dY2 = dY.copy()
    dY2[2, 3:] = 0
    r2 = T.evaluate(w, E, S0, M, dY2, None)
    r1 = T.evaluate(w, E, S0, M, dY, None)
    assert np.array_equal(r2['dE'][2, :3], r1['dE'][2, :3])
    # M[:, 0] is not read
    M0 = M.copy()
    M0[:, 0] = [1.0, np.nan, -3.0, 7.0]
    r0 = T.evaluate(w, E, S0, M0, dY, dS)
    for k in r:
        assert np.array_equal(r0[k], r[k]), k
    # a zero-state row: v = 0, r = 1e6; its dS0 h half is large, and d wh gets nothing from that step
    S3 = S0.copy()
    S3[1] = 0
    one = T.evaluate(w, E[1:2, :1], S3[1:2], M[1:2, :1], dY[1:2, :1], None)
    assert np.abs(one['dS0'][0, 32:]).max() > 1e3 * np.abs(one['dS0'][0, :32]).max() and not one['wgrad'][off[1]:off[1] + dim[1]].any()


@pytest.mark.parametrize('D', [1, 12, 256])
def test_every_gpu_case_keeps_its_bars_under_the_cap(D):
    """a bar may not exceed 1e-3 max|ref| of its array"""
    for shape in T.GPU_SHAPES:
        w, (E, S0, M, dY, dS) = T.gpu_case(shape, D)
        ref, bar = T.bars(w, E, S0, M, dY, dS)
        for k in ref:
            top = float(np.abs(ref[k]).max())
            print('%s D %d %s: bar %.3g, max|ref| %.3g' % (shape, D, k, bar[k], top))
            assert top > 0 and bar[k] <= T.CAP * top, (shape, D, k)
        assert T.bars_within_cap(ref, bar)
