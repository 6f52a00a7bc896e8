"""NumPy restatement of the league actor's bookkeeping (include/hl/llenv_hl_league.h, csrc/hl_league.inc): the opponent draw from Philox, the
counting sort of the arenas into 16-row groups of one slot, and a host mirror of the draw / tally the plan kernel performs between two steps.
Also fixes the cases and seeds the GPU tests run (GPU_CASES), so that what they rely on can be asserted from Philox alone without a GPU."""
import numpy as np

import philox_ref as P

LEAGUE_SALT = 0x1EA60E       # hl_league.inc HL_LEAGUE_SALT: counter (arena, episode lo, episode hi, salt), key (seed lo, seed hi), word 0
GROUP = 16                   # rows of one act workgroup
OUTCOME_BITS = (1, 2, 8, 16)  # LLS_DONE_FALL, _TIME, _CATCH, _NONFINITE: columns 1..4 of the tally (column 0: episodes)

# (arenas, probabilities of slots 1..K, engine seed, draw seed): test_gpu_hl_league's bit-for-bit cases.  The last has a slot nobody may draw.
GPU_CASES = [
    (1, (1.0,), 5, 0x1EA6_0001),
    (17, (0.5, 0.25, 0.25), 5, 0x1EA6_0002),
    (33, (1.0,), 5, 0x1EA6_0003),
    (64, (0.4, 0.0, 0.35, 0.25), 5, 0x1EA6_0004),
]


def cdf_of(probs):
    """float32 running sum of the probabilities, exactly 1 from the last slot with a non-zero probability on (what ll_hl_league_set_probs uploads)"""
    p = np.asarray(probs, np.float64)
    assert (p >= 0).all() and abs(p.sum() - 1.0) <= 1e-6
    last = int(np.nonzero(p > 0)[0][-1])
    cdf, run = np.zeros(len(p), np.float32), np.float32(0.0)
    for k in range(len(p)):
        run = np.float32(run + np.float32(p[k]))
        cdf[k] = np.float32(1.0) if k >= last else run
    return cdf


def u_of_word(w):
    """((w >> 8) + 0.5) 2^-24, every operation in float32 (the topmost word rounds to 1.0)"""
    k = (np.asarray(w, np.uint32) >> np.uint32(8)).astype(np.float32)
    return (k + np.float32(0.5)) * np.float32(2.0 ** -24)


def slot_of_u(u, cdf):
    """1 + the first k with u < cdf[k]; no such k (u = 1): the first k with cdf[k] = 1, the last slot that can be drawn"""
    u = np.asarray(u, np.float32)
    cdf = np.asarray(cdf, np.float32)
    below = u[..., None] < cdf
    first = np.argmax(below, axis=-1)
    fallback = int(np.argmax(cdf >= np.float32(1.0)))
    return 1 + np.where(below.any(axis=-1), first, fallback)


def draw_word(arena, episode, seed):
    k0, k1 = P.seed_key(seed)
    ep = np.asarray(episode, np.uint64)
    return P.philox4x32_10(arena, ep & np.uint64(P.MASK32), ep >> np.uint64(32), LEAGUE_SALT, k0, k1)[0]


def draw_slot(arena, episode, seed, cdf):
    """the slot robot 1 of `arena` acts with in the arena's episode number `episode` (0: the first); arguments broadcast"""
    return slot_of_u(u_of_word(draw_word(arena, episode, seed)), cdf)


def plan(slots, K):
    """slots [A] in 1..K -> (rows [A]: the rows 2 a + 1 sorted by slot, arenas ascending inside a slot; groups [(slot, first, count)]: at most
    16 consecutive entries of rows, all of one slot, slots ascending, only a slot's last group partial, no group for an empty slot)"""
    slots = np.asarray(slots)
    order = np.argsort(slots, kind='stable')
    rows = (2 * order + 1).astype(np.int32)
    groups, first = [], 0
    for k in range(1, K + 1):
        n = int((slots == k).sum())
        for i in range(0, n, GROUP):
            groups.append((k, first + i, min(GROUP, n - i)))
        first += n
    return rows, groups


class Mirror(object):
    """What hl_league_plan_kernel keeps: slot and episode count of every arena, the tally [K][5]."""

    def __init__(self, n_arenas, probs, seed):
        self.A, self.K, self.seed = n_arenas, len(probs), seed
        self.cdf = cdf_of(probs)
        self.slot = np.zeros(n_arenas, np.int32)
        self.episode = np.zeros(n_arenas, np.int64)
        self.tally = np.zeros((self.K, 5), np.uint64)
        self.started = False

    def begin_step(self, done=None, done_reason=None):
        """done / done_reason [A]: what the previous step left for robot 0 of every arena (ignored at the first step).  -> slot [A] of this step"""
        if not self.started:
            who = np.ones(self.A, bool)
            self.started = True
        else:
            who = np.asarray(done) != 0
            for a in np.nonzero(who)[0]:
                t = self.tally[self.slot[a] - 1]
                t[0] += 1
                for c, bit in enumerate(OUTCOME_BITS):
                    if int(done_reason[a]) & bit:
                        t[1 + c] += 1
        idx = np.nonzero(who)[0]
        if len(idx):
            self.slot[idx] = draw_slot(idx, self.episode[idx], self.seed, self.cdf)
            self.episode[idx] += 1
        return self.slot.copy()
