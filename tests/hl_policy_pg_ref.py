"""Row-wise reference of the PPO actor of the on-device EPMC / SEPMC policies (ll_hl_policy_act_pg, include/hl/llenv_hl_policy.h): the value
branches (epmc_net.py:226-244, sepmc_net.py:271-292) and the three samplers (SEPMC heading, z code, low-level action), with the arithmetic type
as a parameter like tests/hl_policy_ref.py, whose building blocks (percept stacks, layer-normalised LSTM, mid level) it uses.  The Philox words
are those of tests/philox_ref.py under the kernel's counter layouts and salts (hl_policy.inc), so a float64 pass fed the same words is what the
kernel computes up to float32 rounding, and a float32 pass against it gives the tolerances."""
import numpy as np

import hl_policy_ref as R
import philox_ref as P

GOLDEN = R.GOLDEN
EPMC_VALUE = {k: '%s/epmc_value_%s.npz' % (GOLDEN, k) for k in ('hurdle', 'hole', 'cube')}
SEPMC_VALUE = '%s/sepmc_value.npz' % GOLDEN

# hl_policy.inc: counter (row * G + g, step lo, step hi, salt), key (seed lo, seed hi)
HEADING_SALT = 0x4EAD1C      # G 1: the first Box-Muller normal of the block
Z_SALT = 0x2C0DE5            # G 64: word j of block g perturbs code 4 g + j
LLC_SALT = 0x11C5A7          # G 3: four normals per block, as philox_ref.policy_noise
N_HEADS = {'epmc': 2, 'sepmc': 3}
LOGSTD = {'epmc': 101, 'sepmc': 151}     # llc logstd (1, 12)
HLC_LOGSTD = 96                          # SEPMC hlc 'logvar' (1, 1), used as the DiagGaussian's logstd half (sepmc_net.py:143-150)
LOG_2PI = np.log(2 * np.pi)


def _counter(rows, step, G, salt, seed):
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 1)
    ctr = rows * np.uint64(G) + np.arange(G, dtype=np.uint64)[None, :]
    k0, k1 = P.seed_key(seed)
    step = int(step)
    return P.philox4x32_10(ctr, step & P.MASK32, (step >> 32) & P.MASK32, salt, k0, k1)


def gumbel(words):
    """-log(-log u), u = ((w >> 8) + 0.5) 2^-24, in float64 (-log u through log1p above 1/2, as the kernel)"""
    k = (np.asarray(words, dtype=np.uint32) >> np.uint32(8)).astype(np.float64)
    lo = k < 2 ** 23
    t = np.where(lo, -np.log(np.where(lo, (k + 0.5) * 2.0 ** -24, 0.5)), -np.log1p(-np.where(lo, 0.25, (2 ** 24 - 1 - k + 0.5) * 2.0 ** -24)))
    return -np.log(t)


def z_noise(rows, step, seed):
    """[len(rows), 256] Gumbel perturbations of the z logits"""
    w = np.stack(_counter(rows, step, 64, Z_SALT, seed), axis=-1)          # [n, 64 blocks, 4 words]: code 4 g + j
    return gumbel(w.reshape(len(np.atleast_1d(rows)), 256))


def llc_noise(rows, step, seed):
    """[len(rows), 12] standard normals of the low-level action"""
    z, _ = P.box_muller4(_counter(rows, step, 3, LLC_SALT, seed))
    return z.reshape(len(np.atleast_1d(rows)), 12)


def heading_noise(rows, step, seed):
    """[len(rows)] standard normal of the SEPMC heading"""
    z, _ = P.box_muller4(_counter(rows, step, 1, HEADING_SALT, seed))
    return z[:, 0, 0]


def load_value(path, w_policy):
    """the value arrays of `path` in w_policy's dtype, with the rms statistics (arrays 0, 1) of the policy's weights"""
    dt = w_policy[0].dtype
    w = R.load(path, dt)
    w[0], w[1] = w_policy[0], w_policy[1]
    return w


def value(kind, wv, obs, vstate, reset=None):
    """the value branch on obs rows; vstate [n][64] c | h (rows with reset start from zero) -> (value [n], new vstate [n][64])"""
    dt = wv[0].dtype
    obs = np.asarray(obs, dt)
    st = np.array(vstate, dt)
    if reset is not None:
        st[np.asarray(reset, bool)] = 0
    relu = lambda v: np.maximum(v, 0)
    x = np.clip((obs[:, :135] - wv[0]) / (wv[1] + dt.type(1e-8)), -5, 5)
    f1 = np.tanh(x @ wv[2] + wv[3])
    e2d, e1d, efr = R.percepts(wv, obs, 4)
    if kind == 'epmc':
        vec = relu(obs[:, 913:916] @ wv[28] + wv[29])
        usr = relu(np.concatenate([vec, e2d, e1d, efr], axis=1) @ wv[30] + wv[31])
        f2 = np.tanh(usr @ wv[32] + wv[33])
        emb = np.tanh(np.concatenate([f1, f2], axis=1) @ wv[34] + wv[35])
        k0 = 36
    else:
        usr = relu(np.concatenate([e2d, e1d, efr], axis=1) @ wv[28] + wv[29])
        f2 = np.tanh(usr @ wv[30] + wv[31])
        hv = np.concatenate([obs[:, 913:918], obs[:, 933:948], obs[:, 955:962], obs[:, 962:964]], axis=1)   # percept_vec, *_cheat, with_flag
        hu = relu(relu(hv @ wv[32] + wv[33]) @ wv[34] + wv[35])
        f3 = np.tanh(hu @ wv[36] + wv[37])
        emb = np.tanh(np.concatenate([f1, f2, f3], axis=1) @ wv[38] + wv[39])
        k0 = 40
    c, h = R.lstm(wv, emb, st[:, :32], st[:, 32:], k0)
    return (h @ wv[k0 + 9] + wv[k0 + 10])[:, 0], np.concatenate([c, h], axis=1)


def logsumexp(s):
    m = s.max(axis=1, keepdims=True)
    return (m + np.log(np.exp(s - m).sum(axis=1, keepdims=True)))[:, 0]


def forward(kind, w, obs, state, reset=None, seed=0, step=0, sample=True, rows=None, code=None, wv=None, vstate=None):
    """one ll_hl_policy_act_pg step of rows `rows` (default 0 .. n-1: the Philox row index) -> dict(action, code, score, pscore (the perturbed
    logits), state, heading (SEPMC), neglogp [n][n_heads], value / vstate (with wv)).  `code` imposes the z code (the controller and the z
    neglogp are evaluated there); with sample=False every noise is zero and the heads are the modes."""
    dt = w[0].dtype
    obs = np.asarray(obs, dt)
    n = obs.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    st = np.array(state, dt)
    if reset is not None:
        st[np.asarray(reset, bool)] = 0
    x = np.clip((obs[:, :135] - w[0]) / (w[1] + dt.type(1e-8)), -5, 5)
    out = {}
    nl = []
    if kind == 'epmc':
        target, cz, hz, off = obs[:, 913:916], st[:, 0:32], st[:, 32:64], 0
    else:
        relu = lambda v: np.maximum(v, 0)
        e2d, e1d, efr = R.percepts(w, obs, 53)
        mlc_embed = relu(np.concatenate([e2d, e1d, efr], axis=1) @ w[77] + w[78])
        vec = np.concatenate([obs[:, 913:918], obs[:, 918:933], obs[:, 948:955], obs[:, 962:964]], axis=1)
        hu = relu(relu(vec @ w[79] + w[80]) @ w[81] + w[82])
        embed = relu(np.concatenate([relu(x @ w[51] + w[52]), mlc_embed, hu], axis=1) @ w[83] + w[84])
        hc, hh = R.lstm(w, embed, st[:, 0:32], st[:, 32:64], 85)
        mu = np.clip(hh @ w[94] + w[95], -np.pi, np.pi)[:, 0]
        eps = heading_noise(rows, step, seed).astype(dt) if sample else np.zeros(n, dt)
        ls = w[HLC_LOGSTD][0, 0]
        heading = mu + np.exp(ls) * eps                 # not clipped
        nl.append(dt.type(0.5) * eps * eps + dt.type(0.5 * LOG_2PI) + ls)
        target = np.stack([np.cos(heading), np.sin(heading), obs[:, 964]], axis=1)
        cz, hz, off = st[:, 64:96], st[:, 96:128], 50
        out['heading'] = heading
    r = R.mid(w, x, obs, target, cz, hz, off)
    score = r['score']
    pscore = score + z_noise(rows, step, seed).astype(dt) if sample else score
    use = np.argmax(pscore, axis=1) if code is None else np.asarray(code)
    redo = np.flatnonzero(use != r['code'])
    action = r['action'].copy()
    if len(redo):
        action[redo] = R.mid(w, x[redo], obs[redo], target[redo], cz[redo], hz[redo], off, code=use[redo])['action']
    nl.append(logsumexp(score) - score[np.arange(n), use])
    ls = w[LOGSTD[kind]][0]
    e = llc_noise(rows, step, seed).astype(dt) if sample else np.zeros((n, 12), dt)
    action = action + np.exp(ls) * e
    nl.append(dt.type(0.5) * (e * e).sum(axis=1) + dt.type(6 * LOG_2PI) + ls.sum())
    zst = np.concatenate([r['c'], r['h']], axis=1)
    out.update(action=action, code=use, score=score, pscore=pscore, neglogp=np.stack(nl, axis=1),
               state=zst if kind == 'epmc' else np.concatenate([hc, hh, zst], axis=1))
    if wv is not None:
        out['value'], out['vstate'] = value(kind, wv, obs, vstate, reset)
    return out


def tolerances(kind, w64, w32, obs, state, reset=None, seed=0, step=0, sample=True, rows=None, wv64=None, wv32=None, vstate=None):
    """float32 pass against the float64 one fed the same draws (hl_policy_ref.tolerances): delta = 4 x the worst perturbed-logit error, every
    other output's tolerance 4 x its worst error, the float32 pass evaluated at the float64 codes."""
    kw = dict(reset=reset, seed=seed, step=step, sample=sample, rows=rows, vstate=vstate)
    r64 = forward(kind, w64, obs, state, wv=wv64, **kw)
    r32 = forward(kind, w32, obs, state, code=r64['code'], wv=wv32, **kw)
    t = dict(ref=r64, delta=4.0 * np.abs(r32['pscore'] - r64['pscore']).max())
    keys = ('action', 'state', 'neglogp') + (('heading',) if kind == 'sepmc' else ()) + (('value', 'vstate') if wv64 is not None else ())
    for k in keys:
        t['tol_' + k] = max(4.0 * np.abs(r32[k].astype(np.float64) - r64[k]).max(), 1e-6)
    return t


def near_ties(pscore, delta):
    top = np.sort(pscore, axis=1)[:, -2:]
    return (top[:, 1] - top[:, 0]) < delta


def chi2_pvalue(counts, probs, min_expected=5.0):
    """Pearson chi-square of a histogram against probabilities (bins of expected count < min_expected pooled) -> (statistic, dof, p-value by
    the Wilson-Hilferty normal approximation)"""
    from math import erfc, sqrt
    counts = np.asarray(counts, np.float64)
    exp = np.asarray(probs, np.float64) * counts.sum()
    big = exp >= min_expected
    o = np.append(counts[big], counts[~big].sum())
    e = np.append(exp[big], exp[~big].sum())
    keep = e > 0
    o, e = o[keep], e[keep]
    stat = float(((o - e) ** 2 / e).sum())
    k = len(o) - 1
    zz = ((stat / k) ** (1.0 / 3) - (1 - 2.0 / (9 * k))) / sqrt(2.0 / (9 * k))
    return stat, k, 0.5 * erfc(zz / sqrt(2))
