"""TEST INFRASTRUCTURE: a NumPy statement of the counter-based generator the kernels draw from, and of the ways its words become numbers.

Philox4x32-10 is restated from the published definition (Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as easy as 1, 2, 3",
SC 2011; the Random123 library's philox4x32_R with R = 10), not from csrc/pmc_math.hpp, and is pinned to Random123's known answers
(test_draws_emul.py).  The derived draws below each point at the kernel code they mirror; the counter and key layouts and the salts are
named constants read from that code, so a test that disagrees with the engine names the stream that moved."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # Philox4x32 round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # Weyl key increments (golden ratio, sqrt(3) - 1)
MASK32 = 0xFFFFFFFF

# Stream layouts: counter (c0, c1, c2, c3), key (seed lo, seed hi) everywhere
RANDOM_POLICY_SALT = 0xAC710      # llenv.hip:190          counter (row * 3 + g, step lo, step hi, salt)
PMC_START_WORD = 0x5eed           # pmc_step.hpp:2255      counter (env, episode, 0x5eed, 0)
EPMC_RESET_SALT = 0x7e44a1        # epmc_step.hpp:724, :900    counter (env, episode, block, salt)
EPMC_STEP_SALT = 0x57e9d3         # epmc_step.hpp:767-768
SEPMC_RESET_SALT = 0x5e9a1d       # sepmc_step.hpp:320, :516   counter (arena, episode, block, salt)
SEPMC_STEP_SALT = 0x57e9d3        # sepmc_step.hpp:369-370
POLICY_NOISE_SALT = 0x9011C7      # pmc_policy.inc:78      counter (env * 3 + g, step lo, step hi, salt)

# Random123 philox4x32_R(10) known answers (kat_vectors): (counter, key, out)
KNOWN_ANSWERS = (
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def _u64(x):
    return np.asarray(x, dtype=np.uint64) & np.uint64(MASK32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of counters (c0, c1, c2, c3) under keys (k0, k1); arguments broadcast, words are returned as four uint32 arrays.
    One round: (hi, lo) of M0 * c0 and M1 * c2 (64-bit products), then
    c' = (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)); the key gains (W0, W1) between rounds."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(_u64(x) for x in (c0, c1, c2, c3, k0, k1)))
    c0, c1, c2, c3, k0, k1 = (x.copy() for x in (c0, c1, c2, c3, k0, k1))
    m, sh = np.uint64(MASK32), np.uint64(32)
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(W0)) & m
            k1 = (k1 + np.uint64(W1)) & m
        p0 = np.uint64(M0) * c0           # < 2^64: exact in uint64
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & m, (p0 >> sh) ^ c3 ^ k1, p0 & m
    return tuple(x.astype(np.uint32) for x in (c0, c1, c2, c3))


def seed_key(seed):
    seed = int(seed)
    return seed & MASK32, (seed >> 32) & MASK32


# ---- derived draws ---------------------------------------------------------------------------------------------------------------------

def box_muller4(r):
    """Four standard normals from one Philox block, as llenv.hip:191-196 (random_action_group) and pmc_policy.inc:79-83 (policy_noise)
    form them: u1, u3 = min(((float)r + 1.0f) * 2^-32, 1) and u2, u4 = (float)r * 2^-32, in float32; the transcendentals here in float64.
    -> (normals [..., 4] float64, Box-Muller radii m [..., 4] float64: the radius each normal was scaled by)."""
    k = np.float32(2.0 ** -32)
    f = [np.asarray(x).astype(np.float32) for x in r]          # (float)r: round to nearest float32
    u1 = np.minimum((f[0] + np.float32(1.0)) * k, np.float32(1.0)).astype(np.float64)
    u2 = (f[1] * k).astype(np.float64)
    u3 = np.minimum((f[2] + np.float32(1.0)) * k, np.float32(1.0)).astype(np.float64)
    u4 = (f[3] * k).astype(np.float64)
    m1, m2 = np.sqrt(-2.0 * np.log(u1)), np.sqrt(-2.0 * np.log(u3))
    a2, a4 = 2.0 * np.pi * u2, 2.0 * np.pi * u4
    z = np.stack([m1 * np.cos(a2), m1 * np.sin(a2), m2 * np.cos(a4), m2 * np.sin(a4)], axis=-1)
    return z, np.stack([m1, m1, m2, m2], axis=-1)


def _grouped_normals(n_rows, step, seed, salt):
    """[n_rows, 12] normals of counter (row * 3 + g, step lo, step hi, salt), key (seed lo, seed hi), g = 0..2, and their radii."""
    gid = np.arange(3 * n_rows, dtype=np.uint64)
    step = int(step)
    k0, k1 = seed_key(seed)
    z, m = box_muller4(philox4x32_10(gid, step & MASK32, (step >> 32) & MASK32, salt, k0, k1))
    return z.reshape(n_rows, 12), m.reshape(n_rows, 12)


def random_policy_actions(n_rows, step, seed, sigma):
    """llenv.hip:187-197 (random_action_group, pmc_actions_kernel; the step kernels' own draw): a = sigma * N(0, 1) of row `row` at
    control step `step` (the engine's step count, + the step's index inside a multi-step launch). -> (actions, sigma * radius)"""
    z, m = _grouped_normals(n_rows, step, seed, RANDOM_POLICY_SALT)
    return sigma * z, sigma * m


def policy_noise(n_envs, step, seed):
    """pmc_policy.inc:75-84: the twelve standard normals of env e at policy step `step` -> (eps [n, 12], radii [n, 12])"""
    return _grouped_normals(n_envs, step, seed, POLICY_NOISE_SALT)


def u01_from(hi, lo):
    """pmc_math.hpp:321-323: the top 53 bits of (hi << 32 | lo) times 2^-53 -- a double in [0, 1)."""
    v = (_u64(hi) << np.uint64(32)) | _u64(lo)
    return (v >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def pmc_start_uniforms(env, episode, seed):
    """pmc_step.hpp:2255-2256 (Pmc::sample_start): (u1, u2) of counter (env, episode, 0x5eed, 0)."""
    k0, k1 = seed_key(seed)
    r = philox4x32_10(env, episode, PMC_START_WORD, 0, k0, k1)
    return u01_from(r[0], r[1]), u01_from(r[2], r[3])


def pmc_start(env, episode, seed, cdf, clip_len, frame_step, margin):
    """Pmc::sample_start (pmc_step.hpp:2252-2263): clip = the first i with u1 < cdf[i] (capped at n_clips - 1), and
    t0 = u2 * (frame_step * (clip_len[clip] - margin - 1)) in float64. -> (clip, t0, u1)"""
    u1, u2 = pmc_start_uniforms(env, episode, seed)
    cdf = np.asarray(cdf, dtype=np.float64)
    clip = np.minimum(np.searchsorted(cdf, u1, side='right'), len(cdf) - 1)       # number of entries <= u1 = first i with u1 < cdf[i]
    t0 = u2 * (frame_step * (np.asarray(clip_len, dtype=np.float64)[clip] - margin - 1))
    return clip, t0, u1


def epmc_uniforms(index, key_id, episode, salt, seed):
    """EpmcDraws::u01 (epmc_step.hpp:97-108): draw i of stream (key_id = env or arena, episode, salt) is word i & 3 of block i >> 2,
    the block being Philox of counter (key_id, episode, i >> 2, salt); the word's top 24 bits times 2^-24 (a float32).
    index, key_id and episode broadcast."""
    index = np.asarray(index, dtype=np.int64)
    k0, k1 = seed_key(seed)
    r = np.stack(philox4x32_10(key_id, episode, index >> 2, salt, k0, k1), axis=-1)
    w = np.take_along_axis(r, np.broadcast_to(index & 3, r.shape[:-1])[..., None], axis=-1)[..., 0]
    return ((w >> np.uint32(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def epmc_stream(key_id, episode, salt, seed, n, start=0):
    """[len(key_id), n] uniforms start .. start + n - 1 of each stream (the layout reset(draws=) / set_step_draws take)."""
    key_id = np.asarray(key_id, dtype=np.int64).reshape(-1, 1)
    episode = np.asarray(episode, dtype=np.int64).reshape(-1, 1)
    start = np.asarray(start, dtype=np.int64).reshape(-1, 1)
    idx = start + np.arange(n, dtype=np.int64)[None, :]
    return epmc_uniforms(idx, key_id, episode, salt, seed)
