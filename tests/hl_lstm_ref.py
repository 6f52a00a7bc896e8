"""The normative statement of the layer-normalised LSTM core of the EPMC / SEPMC networks and its linear head (include/hl/llenv_hl_lstm.h): the forward
over an unroll with resets, and the exact backward through time, in NumPy with the arithmetic type as a parameter -- so that a float32 pass against the
float64 one gives the bars of the GPU tests (the hl_policy_pg_ref.tolerances recipe).

Weights are eleven arrays, in this order: wx [256][128], wh [32][128], b [128], beta_x, gamma_x, beta_h, gamma_h [128], beta_c, gamma_c [32], wo [32][D],
bo [D].  The first nine are arrays k0 .. k0 + 8 of a branch (hl_policy_ref.lstm), the last two its head.

Also here: the value branches' embed (the lines of hl_policy_pg_ref.value up to `emb`), so that embed -> this core can be held to hl_policy_pg_ref.value."""
import numpy as np

import hl_policy_ref as R

NAMES = ('wx', 'wh', 'b', 'beta_x', 'gamma_x', 'beta_h', 'gamma_h', 'beta_c', 'gamma_c', 'wo', 'bo')
N_IN, N_GATES, N_UNITS = 256, 128, 32
EPS = 1e-12
# (kind, branch) -> (k0, head arrays, D)
BRANCHES = {('epmc', 'z'): (79, (88, 89), 256), ('epmc', 'value'): (36, (45, 46), 1), ('sepmc', 'hlc'): (85, (94, 95), 1),
            ('sepmc', 'z'): (129, (138, 139), 256), ('sepmc', 'value'): (40, (49, 50), 1)}


def shapes(n_out):
    return [(N_IN, N_GATES), (N_UNITS, N_GATES), (N_GATES,), (N_GATES,), (N_GATES,), (N_GATES,), (N_GATES,), (N_UNITS,), (N_UNITS,), (N_UNITS, n_out), (n_out,)]


def layout(n_out):
    """-> (offsets [11], sizes [11], total) of the packed weight gradient"""
    dim = [int(np.prod(s)) for s in shapes(n_out)]
    off = [int(x) for x in np.concatenate([[0], np.cumsum(dim)[:-1]])]
    return off, dim, int(sum(dim))


def branch_weights(kind, branch, arrays, dt=np.float64):
    """the eleven arrays of a branch out of a {number: array} dict; the vectors flattened (the files hold some of them as (1, n))"""
    k0, head, D = BRANCHES[(kind, branch)]
    ws = [np.asarray(arrays[k0 + i], dt) for i in range(9)] + [np.asarray(arrays[head[0]], dt), np.asarray(arrays[head[1]], dt)]
    return [w.reshape(s) for w, s in zip(ws, shapes(D))]


def pack(grads):
    return np.concatenate([np.asarray(g).ravel() for g in grads])


def _sig(x):
    return 1 / (1 + np.exp(-x))


def _ln_fwd(x, beta, gamma):
    m = x.mean(axis=1, keepdims=True)
    var = ((x - m) ** 2).mean(axis=1, keepdims=True)
    sd = np.sqrt(var + x.dtype.type(EPS))
    xh = (x - m) / sd                       # (the forms of hl_policy_ref._ln, so that the forward is its bits)
    return xh * gamma + beta, xh, 1 / sd


def _ln_bwd(dy, xh, r, gamma):
    dxh = dy * gamma
    return r * (dxh - dxh.mean(axis=1, keepdims=True) - xh * (dxh * xh).mean(axis=1, keepdims=True))


def resets(M):
    """[n][L] bool: where the state is zeroed before the step; M[:, 0] is not read.  Any non-zero value counts, and so does NaN."""
    M = np.asarray(M)
    z = ~(M == 0)
    z[:, 0] = False
    return z


def forward(w, E, S0, M, dt=np.float64, tape=False):
    """E [n][L][256], S0 [n][64] c | h, M [n][L] -> (Y [n][L][D], S_end [n][64]) in dt; with tape=True also the per-step intermediates"""
    w = [np.asarray(a, dt) for a in w]
    wx, wh, b, bx, gx, bh, gh, bc, gc, wo, bo = w
    E, S0 = np.asarray(E, dt), np.asarray(S0, dt)
    n, L = E.shape[:2]
    cut = resets(M)
    c, h = S0[:, :32].copy(), S0[:, 32:].copy()
    Y = np.zeros((n, L, wo.shape[1]), dt)
    steps = []
    for t in range(L):
        keep = (~cut[:, t])[:, None].astype(dt)
        c, h = c * keep, h * keep
        u, v = E[:, t] @ wx, h @ wh
        lx, xx, rx = _ln_fwd(u, bx, gx)
        lh, xh, rh = _ln_fwd(v, bh, gh)
        z = lx + lh + b
        i, f, o, g = np.split(z, 4, axis=1)
        si, sf, so, tg = _sig(i), _sig(f + 1), _sig(o), np.tanh(g)
        c2 = sf * c + si * tg
        nn, ch, rc = _ln_fwd(c2, bc, gc)
        tn = np.tanh(nn)
        h2 = so * tn
        Y[:, t] = h2 @ wo + bo
        if tape:
            steps.append(dict(c=c, h=h, xx=xx, rx=rx, xh=xh, rh=rh, si=si, sf=sf, so=so, tg=tg, ch=ch, rc=rc, tn=tn, h2=h2))
        c, h = c2, h2
    out = (Y, np.concatenate([c, h], axis=1))
    return out + (steps,) if tape else out


def backward(w, E, S0, M, dY, dS_end=None, dt=np.float64):
    """the exact derivative of sum(Y dY) + sum(S_end dS_end) -> (dE [n][L][256], dS0 [n][64], [11 weight gradients])"""
    w = [np.asarray(a, dt) for a in w]
    wx, wh, b, bx, gx, bh, gh, bc, gc, wo, bo = w
    E, dY = np.asarray(E, dt), np.asarray(dY, dt)
    n, L = E.shape[:2]
    cut = resets(M)
    steps = forward(w, E, S0, M, dt, tape=True)[2]
    dS = np.zeros((n, 64), dt) if dS_end is None else np.asarray(dS_end, dt)
    dc, dh = dS[:, :32].copy(), dS[:, 32:].copy()
    g = [np.zeros_like(a) for a in w]
    dE = np.zeros_like(E)
    for t in range(L - 1, -1, -1):
        s = steps[t]
        g[9] += s['h2'].T @ dY[:, t]
        g[10] += dY[:, t].sum(axis=0)
        dh = dh + dY[:, t] @ wo.T
        do = dh * s['tn'] * s['so'] * (1 - s['so'])
        dn = dh * s['so'] * (1 - s['tn'] ** 2)
        g[7] += dn.sum(axis=0)
        g[8] += (dn * s['ch']).sum(axis=0)
        dc = dc + _ln_bwd(dn, s['ch'], s['rc'], gc)
        di = dc * s['tg'] * s['si'] * (1 - s['si'])
        df = dc * s['c'] * s['sf'] * (1 - s['sf'])
        dg = dc * s['si'] * (1 - s['tg'] ** 2)
        dz = np.concatenate([di, df, do, dg], axis=1)
        g[2] += dz.sum(axis=0)
        g[3] += dz.sum(axis=0)
        g[4] += (dz * s['xx']).sum(axis=0)
        g[5] += dz.sum(axis=0)
        g[6] += (dz * s['xh']).sum(axis=0)
        du = _ln_bwd(dz, s['xx'], s['rx'], gx)
        dv = _ln_bwd(dz, s['xh'], s['rh'], gh)
        g[0] += E[:, t].T @ du
        g[1] += s['h'].T @ dv
        dE[:, t] = du @ wx.T
        keep = (~cut[:, t])[:, None].astype(dt)
        dc, dh = dc * s['sf'] * keep, (dv @ wh.T) * keep
    return dE, np.concatenate([dc, dh], axis=1), g


def evaluate(w, E, S0, M, dY, dS_end=None, dt=np.float64):
    """every output of a forward and a backward call: dict(Y, S_end, dE, dS0, wgrad (packed))"""
    Y, S_end = forward(w, E, S0, M, dt)
    dE, dS0, g = backward(w, E, S0, M, dY, dS_end, dt)
    return dict(Y=Y, S_end=S_end, dE=dE, dS0=dS0, wgrad=pack(g))


CAP = 1e-3      # a bar may not exceed CAP max|ref| of its array: a case that breaks this is badly chosen


def bars(w, E, S0, M, dY, dS_end=None):
    """float64 reference, and per output array the larger of 4 x the worst deviation of the float32 pass and 4 2^-24 max|ref| -> (ref, {name: bar})"""
    f32 = lambda a: None if a is None else np.asarray(a, np.float32)
    ref = evaluate(w, E, S0, M, dY, dS_end)
    low = evaluate([f32(a) for a in w], f32(E), f32(S0), M, f32(dY), f32(dS_end), np.float32)
    bar = {}
    for k in ref:
        top = float(np.abs(ref[k]).max())
        bar[k] = max(4.0 * float(np.abs(low[k].astype(np.float64) - ref[k]).max()), 4.0 * 2.0 ** -24 * top)
    return ref, bar


def bars_within_cap(ref, bar):
    return all(bar[k] <= CAP * float(np.abs(ref[k]).max()) for k in ref)


def value_embed(kind, wv, obs):
    """the value branch's feed-forward front: hl_policy_pg_ref.value up to `emb` [n][256]"""
    dt = wv[0].dtype
    obs = np.asarray(obs, dt)
    relu = lambda v: np.maximum(v, 0)
    x = np.clip((obs[:, :135] - wv[0]) / (wv[1] + dt.type(1e-8)), -5, 5)
    f1 = np.tanh(x @ wv[2] + wv[3])
    e2d, e1d, efr = R.percepts(wv, obs, 4)
    if kind == 'epmc':
        vec = relu(obs[:, 913:916] @ wv[28] + wv[29])
        usr = relu(np.concatenate([vec, e2d, e1d, efr], axis=1) @ wv[30] + wv[31])
        f2 = np.tanh(usr @ wv[32] + wv[33])
        return np.tanh(np.concatenate([f1, f2], axis=1) @ wv[34] + wv[35])
    usr = relu(np.concatenate([e2d, e1d, efr], axis=1) @ wv[28] + wv[29])
    f2 = np.tanh(usr @ wv[30] + wv[31])
    hv = np.concatenate([obs[:, 913:918], obs[:, 933:948], obs[:, 955:962], obs[:, 962:964]], axis=1)
    hu = relu(relu(hv @ wv[32] + wv[33]) @ wv[34] + wv[35])
    f3 = np.tanh(hu @ wv[36] + wv[37])
    return np.tanh(np.concatenate([f1, f2, f3], axis=1) @ wv[38] + wv[39])


def case(n, L, D, seed, zero_rows=(), reset_p=0.2, dS=True):
    """uniform inputs of one shape: E in (-1, 1), S0 in (-0.5, 0.5) (rows of zero_rows zero), M with a share reset_p of ones, dY in (-1, 1) / (n L),
    dS_end in (-1, 1) / n or None"""
    rng = np.random.default_rng(seed)
    E = rng.uniform(-1, 1, (n, L, N_IN)).astype(np.float32)
    S0 = rng.uniform(-0.5, 0.5, (n, 64)).astype(np.float32)
    S0[list(zero_rows)] = 0
    M = (rng.uniform(0, 1, (n, L)) < reset_p).astype(np.float32)
    dY = (rng.uniform(-1, 1, (n, L, D)) / (n * L)).astype(np.float32)
    dS_end = (rng.uniform(-1, 1, (n, 64)) / n).astype(np.float32) if dS else None
    return E, S0, M, dY, dS_end


def shipped_weights(kind, branch, seed, n_out=None):
    """The eleven arrays of a shipped branch (tests/golden), perturbed with hl_score_ref.perturbed and rounded to float32 -- what the device is given --
    as float64.  n_out: keep the first n_out outputs of the head."""
    import hl_policy_pg_ref as G
    import hl_score_ref as SR
    w = R.load(R.EPMC_WEIGHTS['hurdle'] if kind == 'epmc' else R.SEPMC_WEIGHTS)
    if branch == 'value':
        w = G.load_value(G.EPMC_VALUE['hurdle'] if kind == 'epmc' else G.SEPMC_VALUE, w)
    ws = branch_weights(kind, branch, SR.perturbed(w, np.random.default_rng(seed)))
    if n_out is not None:
        ws[9], ws[10] = ws[9][:, :n_out], ws[10][:n_out]
    return [np.ascontiguousarray(a.astype(np.float32)).astype(np.float64) for a in ws]


# The shapes of the GPU tests (tests/test_gpu_hl_lstm.py), named from the kernels' constants (csrc/hl_lstm.inc): the forward takes HLS_FROWS = 16 rows per workgroup (one
# matrix-core tile), the sequential backward HLS_ROWS = 8, a dE workgroup HLS_DE_FRAMES = 16 frames, a weight-gradient workgroup sums HLS_CHUNK = 64 frames, and a fold
# pass adds HLS_FOLD_PASS = 8 rows of partials.  (17, 3) and (33, 2) are one row past one and two forward tiles.
HLS_ROWS, HLS_DE_FRAMES, HLS_CHUNK, HLS_FOLD_PASS = 8, 16, 64, 8
PAST_ONE_GROUP = (13, 5)        # 65 frames: one past what a single weight-gradient workgroup sums (and 13 rows: past one sequential workgroup, 65 frames: past four dE ones)
SECOND_FOLD_PASS = (65, 8)      # 520 frames = 9 chunks and 9 row groups: both kinds of partials take a second fold pass
GPU_SHAPES = [(1, 1), (1, 2), (3, 5), (17, 3), (33, 2), PAST_ONE_GROUP, SECOND_FOLD_PASS]
GPU_BRANCH = {1: [('epmc', 'value'), ('sepmc', 'hlc'), ('sepmc', 'value')], 12: [('sepmc', 'z')], 256: [('epmc', 'z'), ('sepmc', 'z')]}
assert PAST_ONE_GROUP[0] * PAST_ONE_GROUP[1] == HLS_CHUNK + 1 and SECOND_FOLD_PASS[0] == HLS_ROWS * HLS_FOLD_PASS + 1
assert -(-SECOND_FOLD_PASS[0] * SECOND_FOLD_PASS[1] // HLS_CHUNK) == HLS_FOLD_PASS + 1


def gpu_case(shape, D):
    """weights and inputs of the GPU case (shape, D): the branch rotates with the shape, a fifth of the steps reset, the middle row starts from zero"""
    n, L = shape
    i = GPU_SHAPES.index(tuple(shape))
    kind, branch = GPU_BRANCH[D][i % len(GPU_BRANCH[D])]
    w = shipped_weights(kind, branch, 1000 + 10 * i + D, n_out=D)
    return w, case(n, L, D, 7000 + 100 * i + D, zero_rows=(n // 2,) if n >= 3 else ())
