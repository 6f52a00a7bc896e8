"""NumPy restatement of what the unroll recorder (include/hl/llenv_hl_unroll.h) leaves in a block: the packing of one robot's time steps into rows
X | A | neglogp | R | V | r | discount | S | M | pad, the M / S rule of the reference's actor (learning/actors/distill_actor.py:121-140), and the
TD(lambda) recursion of ll_hl_unroll_finish -- plus its closed form, which the recursion is tested against."""
import numpy as np

from lifelike_agility_and_play_amd.policies import hl_unroll as U
from lifelike_agility_and_play_amd.policies.hl_policy_hip import LLH_EPMC, LLH_SEPMC

KIND = {'epmc': LLH_EPMC, 'sepmc': LLH_SEPMC}


def mask_and_state(hs, reset):
    """hs [T][n][S]: the recurrent state (policies.hl_policy_hip hs() layout) found BEFORE the act of every time step of ONE unroll; reset [T][n]: the
    d_reset flag that act was given.  Returns (S, M) as recorded: a restarted row starts from zero state; M_t is the flag for t > 0 and 0 for the
    first frame of the unroll, which carries the state itself (distill_actor.py: `mask = False` at the top of an unroll, `mask = done` after a frame)."""
    reset = np.asarray(reset) != 0
    S = np.where(reset[..., None], 0.0, np.asarray(hs))
    M = reset.astype(np.float64)
    M[0] = 0.0
    return S, M


def pack_unroll(kind, obs, code, action, neglogp, value, reward, done, hs, reset, heading=None, dtype=np.float64):
    """One unroll [T] of n rows -> block [n][T][row_floats], R left at zero (ll_hl_unroll_finish writes it).
    obs [T][n][obs_dim], code [T][n], action [T][n][12], neglogp [T][n][heads], value / reward / done [T][n] of the step, hs / reset as mask_and_state,
    heading [T][n] (SEPMC)."""
    k = KIND[kind]
    lay, rf = U.row_layout(k)
    T, n = np.asarray(code).shape
    S, M = mask_and_state(hs, reset)
    rows = np.zeros((T, n, rf), dtype)
    f = U.split_row(rows, lay)
    f['X'][:] = obs
    a = [np.asarray(code, dtype)[..., None], np.asarray(action, dtype)]
    if k == LLH_SEPMC:
        a.insert(0, np.asarray(heading, dtype)[..., None])
    f['A'][:] = np.concatenate(a, axis=-1)
    f['neglogp'][:] = neglogp
    f['V'][:] = value
    f['r'][:] = reward
    f['discount'][:] = 1.0 - (np.asarray(done) != 0)
    f['S'][:] = S
    f['M'][:] = M
    return np.ascontiguousarray(rows.transpose(1, 0, 2))


def td_lambda(r, V, discount, bootstrap, gamma, lam, dtype=np.float64):
    """The recursion of ll_hl_unroll_finish / ll_finish_unroll over [n][T] arrays, every operation rounded to `dtype`:
    delta_t = r_t + gamma V_{t+1} m_t - V_t, A_t = delta_t + gamma lam m_t A_{t+1}, R_t = A_t + V_t, V_T = bootstrap [n]."""
    r, V, m = (np.asarray(x, dtype) for x in (r, V, discount))
    g, l = dtype(gamma), dtype(lam)
    n, T = r.shape
    R = np.zeros((n, T), dtype)
    adv, vnext = np.zeros(n, dtype), np.asarray(bootstrap, dtype)
    for t in range(T - 1, -1, -1):
        delta = r[:, t] + g * vnext * m[:, t] - V[:, t]
        adv = delta + g * l * m[:, t] * adv
        R[:, t] = adv + V[:, t]
        vnext = V[:, t]
    return R


def td_lambda_closed_form(r, V, discount, bootstrap, gamma, lam):
    """R_t = V_t + sum_k (gamma lam)^k (prod_{j<k} m_{t+j}) delta_{t+k}, float64, term by term"""
    r, V, m = (np.asarray(x, np.float64) for x in (r, V, discount))
    n, T = r.shape
    Vn = np.concatenate([V[:, 1:], np.asarray(bootstrap, np.float64)[:, None]], axis=1)
    delta = r + gamma * Vn * m - V
    R = np.zeros((n, T))
    for t in range(T):
        acc, w = np.zeros(n), np.ones(n)
        for k in range(T - t):
            acc += w * delta[:, t + k]
            w = w * gamma * lam * m[:, t + k]
        R[:, t] = V[:, t] + acc
    return R
