"""Row-wise references for the on-device EPMC / SEPMC policies (include/hl/llenv_hl_policy.h): the forward pass of oracle.epmc_policy.EpmcPolicy.act /
oracle.sepmc_policy.SepmcPolicy.act, restated here with the arithmetic type as a parameter, an explicit recurrent state in the device layout, and the
z code optionally imposed -- so that a float32 pass against the float64 one gives the tolerances (the draws_parity_common.policy_tolerances recipe)
and the controller can be evaluated at the kernel's code.  test_hl_policy_api checks that the float64 pass IS the oracle's."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import epmc_policy as EP  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
EPMC_WEIGHTS = {k: os.path.join(GOLDEN, 'epmc_policy_%s.npz' % k) for k in ('hurdle', 'hole', 'cube')}
SEPMC_WEIGHTS = os.path.join(GOLDEN, 'sepmc_policy.npz')


def load(npz_path, dt=np.float64):
    z = np.load(npz_path)
    return {int(k[1:]): z[k].astype(dt) for k in z.files}


def _conv2d(x, w, b, stride=1):
    kh, kw, ci, co = w.shape
    oh, pt, pb = EP._same_pad(x.shape[1], kh, stride)
    ow, pl, pr = EP._same_pad(x.shape[2], kw, stride)
    xp = np.pad(x, ((0, 0), (pt, pb), (pl, pr), (0, 0)))
    out = np.zeros((x.shape[0], oh, ow, co), x.dtype)
    for di in range(kh):
        for dj in range(kw):
            out += xp[:, di:di + (oh - 1) * stride + 1:stride, dj:dj + (ow - 1) * stride + 1:stride, :] @ w[di, dj]
    return np.maximum(out + b, 0)


def _conv1d(x, w, b, stride=1):
    return _conv2d(x[:, None], w[None], b, stride)[:, 0]


def _ln(x, beta, gamma):
    m = x.mean(axis=1, keepdims=True)
    v = ((x - m) ** 2).mean(axis=1, keepdims=True)
    return (x - m) / np.sqrt(v + x.dtype.type(1e-12)) * gamma + beta


def _sig(x):
    return 1 / (1 + np.exp(-x))


def percepts(w, obs, k):
    """the three conv stacks, weights k .. k + 23 -> (e2d 28, e1d 32, efr 28)"""
    n = obs.shape[0]

    def enc2d(img, kk):
        e = _conv2d(img, w[kk], w[kk + 1])
        e = _conv2d(e, w[kk + 2], w[kk + 3], 2)
        e = _conv2d(e, w[kk + 4], w[kk + 5], 2)
        return _conv2d(e, w[kk + 6], w[kk + 7]).reshape(n, -1)
    p1d = obs[:, 460:588]
    pad = np.concatenate([p1d[:, -4:], p1d, p1d[:, :4]], axis=1)[:, :, None]
    e = _conv1d(pad, w[k + 8], w[k + 9])[:, 4:-4, :]
    e = _conv1d(e, w[k + 10], w[k + 11], 2)
    e = _conv1d(e, w[k + 12], w[k + 13], 2)
    e1d = _conv1d(e, w[k + 14], w[k + 15]).reshape(n, -1)
    return enc2d(obs[:, 135:460].reshape(n, 25, 13, 1), k), e1d, enc2d(obs[:, 588:913].reshape(n, 25, 13, 1), k + 16)


def lstm(w, x, c, h, k0):
    zz = _ln(x @ w[k0], w[k0 + 3], w[k0 + 4]) + _ln(h @ w[k0 + 1], w[k0 + 5], w[k0 + 6]) + w[k0 + 2]
    i, f, o, u = np.split(zz, 4, axis=1)
    c = _sig(f + 1) * c + _sig(i) * np.tanh(u)
    return c, _sig(o) * np.tanh(_ln(c, w[k0 + 7], w[k0 + 8]))


def mid(w, x, obs, target, c, h, off, code=None):
    """EPMC's policy / SEPMC's mlc_encoder + llc; EPMC array numbers, SEPMC's are `off` = 50 further on"""
    relu = lambda v: np.maximum(v, 0)
    e2d, e1d, efr = percepts(w, obs, off + 49)
    usr = relu(np.concatenate([relu(target @ w[off + 73] + w[off + 74]), e2d, e1d, efr], axis=1) @ w[off + 75] + w[off + 76])
    embed = relu(np.concatenate([relu(x @ w[off + 47] + w[off + 48]), usr], axis=1) @ w[off + 77] + w[off + 78])
    c, h = lstm(w, embed, c, h, off + 79)
    score = h @ w[off + 88] + w[off + 89]
    best = np.argmax(score, axis=1)
    use = best if code is None else np.asarray(code)
    zq = w[off + 90].T[use]
    s = np.concatenate([relu(x @ w[off + 91] + w[off + 92]), relu(zq @ w[off + 93] + w[off + 94])], axis=1)
    hdn = relu(relu(s @ w[off + 95] + w[off + 96]) @ w[off + 97] + w[off + 98])
    return dict(action=hdn @ w[off + 99] + w[off + 100], code=best, score=score, c=c, h=h)


def forward(kind, w, obs, state, reset=None, code=None):
    """kind 'epmc' | 'sepmc'; w from load(.., dt); obs [n][916 | 965]; state [n][64 | 128] in the device layout (rows with reset[r] start from zero).
    -> dict(action, code, score, state [n][state_dim], heading (SEPMC))"""
    dt = w[0].dtype
    obs = np.asarray(obs, dt)
    st = np.array(state, dt)
    if reset is not None:
        st[np.asarray(reset, bool)] = 0
    x = np.clip((obs[:, :135] - w[0]) / (w[1] + dt.type(1e-8)), -5, 5)
    if kind == 'epmc':
        r = mid(w, x, obs, obs[:, 913:916], st[:, 0:32], st[:, 32:64], 0, code)
        r['state'] = np.concatenate([r['c'], r['h']], axis=1)
        return r
    relu = lambda v: np.maximum(v, 0)
    e2d, e1d, efr = percepts(w, obs, 53)
    mlc_embed = relu(np.concatenate([e2d, e1d, efr], axis=1) @ w[77] + w[78])
    vec = np.concatenate([obs[:, 913:918], obs[:, 918:933], obs[:, 948:955], obs[:, 962:964]], axis=1)
    hu = relu(relu(vec @ w[79] + w[80]) @ w[81] + w[82])
    embed = relu(np.concatenate([relu(x @ w[51] + w[52]), mlc_embed, hu], axis=1) @ w[83] + w[84])
    hc, hh = lstm(w, embed, st[:, 0:32], st[:, 32:64], 85)
    heading = np.clip(hh @ w[94] + w[95], -np.pi, np.pi)
    target = np.concatenate([np.cos(heading), np.sin(heading), obs[:, 964:965]], axis=1)
    r = mid(w, x, obs, target, st[:, 64:96], st[:, 96:128], 50, code)
    r['heading'] = heading[:, 0]
    r['state'] = np.concatenate([hc, hh, r['c'], r['h']], axis=1)
    return r


def tolerances(kind, w64, w32, obs, state, reset=None):
    """float32 pass against the float64 one on the same inputs (draws_parity_common.policy_tolerances): delta = 4 x the worst logit error (a code
    within delta of the runner-up is a near-tie); action / state / heading tolerances 4 x the worst error, evaluated at the float64 codes."""
    r64 = forward(kind, w64, obs, state, reset)
    r32 = forward(kind, w32, obs, state, reset, code=r64['code'])
    t = dict(ref=r64, delta=4.0 * np.abs(r32['score'] - r64['score']).max())
    for k in ('action', 'state') + (('heading',) if kind == 'sepmc' else ()):
        t['tol_' + k] = max(4.0 * np.abs(r32[k].astype(np.float64) - r64[k]).max(), 1e-6)
    return t


def near_ties(score, delta):
    top = np.sort(score, axis=1)[:, -2:]
    return (top[:, 1] - top[:, 0]) < delta
