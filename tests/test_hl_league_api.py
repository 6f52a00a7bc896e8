"""The league actor (include/hl/llenv_hl_league.h, policies.hl_league) without a GPU: header, binding and library agree; the draw's salt is a stream
of its own; argument checks; and the NumPy reference of the draw and of the plan (tests/hl_league_ref.py) the GPU tests compare against -- with the
properties of the GPU cases' seeds those tests rely on asserted here from Philox alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from lifelike_agility_and_play_amd import capi
from lifelike_agility_and_play_amd.policies import hl_league as LG
from lifelike_agility_and_play_amd.policies import hl_policy_hip as H
import hl_league_ref as LR
import hl_policy_pg_ref as G
import philox_ref as P

HEADER = os.path.join(ROOT, 'include', 'hl', 'llenv_hl_league.h')
SOURCE = os.path.join(ROOT, 'lifelike_agility_and_play_amd', 'csrc', 'hl_league.inc')


def _lib():
    import __graft_entry__ as g
    g.build_hip()
    return LG.load_library()


def test_header_binding_and_library_agree():
    text = open(HEADER).read()
    declared = sorted(set(re.findall(r'\b(ll_hl_league_[a-z0-9_]+)\s*\(', text)))
    assert declared == LG.EXPORTED_SYMBOLS
    for name in ('create', 'destroy', 'set_weights', 'set_probs', 'steps', 'position', 'layout', 'finish', 'get_assignment', 'get_outcomes', 'get_state'):
        assert 'll_hl_league_' + name in declared, name
    lib = _lib()
    for name in declared:
        assert hasattr(lib, name), name
    for cite in ('distill_actor.py:57-82', ':187-208', ':294-308', 'example_sepmc_train.sh'):
        assert cite in text, cite
    assert re.search(r'#define LLG_MAX_OPPONENTS\s+%d\b' % LG.MAX_OPPONENTS, text) and re.search(r'#define LLG_N_OUTCOMES\s+%d\b' % len(LG.OUTCOMES), text)
    from lifelike_agility_and_play_amd import policies
    assert policies.HlLeagueActor is LG.HlLeagueActor
    # the plain policy's weight swap is declared, bound and exported too
    assert 'll_hl_policy_set_weights' in H.EXPORTED_SYMBOLS and hasattr(lib, 'll_hl_policy_set_weights')


def test_league_salt_is_a_new_stream():
    src = open(SOURCE).read()
    assert re.search(r'#define HL_LEAGUE_SALT 0x%xu\b' % LR.LEAGUE_SALT, src, re.I)
    assert ('0x%X' % LR.LEAGUE_SALT) in open(HEADER).read()
    old = {P.RANDOM_POLICY_SALT, P.PMC_START_WORD, P.EPMC_RESET_SALT, P.EPMC_STEP_SALT, P.SEPMC_RESET_SALT, P.SEPMC_STEP_SALT, P.POLICY_NOISE_SALT,
           G.HEADING_SALT, G.Z_SALT, G.LLC_SALT}
    assert LR.LEAGUE_SALT not in old


def test_null_handles_are_einval():
    lib = _lib()
    w = np.zeros(8, np.float32)
    out = C.c_void_p()
    assert lib.ll_hl_league_create(None, 1, 16, 2, C.byref(out)) == -1 and not out.value
    assert lib.ll_hl_league_create(None, 1, 16, 2, None) == -1
    assert lib.ll_hl_league_set_weights(None, 0, w.ctypes.data_as(C.c_void_p), 8, None, 0) == -1
    p = (C.c_double * 1)(1.0)
    assert lib.ll_hl_league_set_probs(None, p, 1) == -1
    assert lib.ll_hl_league_steps(None, 0, 1, 1) == -1
    k, t = C.c_int64(0), C.c_int(0)
    assert lib.ll_hl_league_position(None, C.byref(k), C.byref(t)) == -1
    assert lib.ll_hl_league_layout(None, None) == -1
    assert lib.ll_hl_league_finish(None, 0, 0.95, 0.95, None) == -1
    assert lib.ll_hl_league_get_assignment(None, None, None) == -1
    assert lib.ll_hl_league_get_outcomes(None, None, 0) == -1
    assert lib.ll_hl_league_get_state(None, None, None) == -1
    assert lib.ll_hl_league_plan_only(None, 1) == -1
    assert lib.ll_last_error().decode()
    assert lib.ll_hl_league_destroy(None) == 0
    assert lib.ll_hl_policy_set_weights(None, w.ctypes.data_as(C.c_void_p), 8, None, 0, None) == -1


def test_no_gpu_means_loud_failure():
    """A league is made of a SEPMC engine only, and without a HIP device that cannot exist: LL_ENODEV, no CPU path, and the binding raises
    instead of crashing.  (With a device present the second half has nothing to show.)"""
    import torch
    with pytest.raises(TypeError):
        LG.HlLeagueActor(object(), 1, 16, 2)
    if not torch.cuda.is_available():
        from test_gpu_hl_policy import _sepmc_engine
        with pytest.raises(capi.LLError) as ei:
            E = _sepmc_engine(4, 1, 5, max_steps=16)
            LG.HlLeagueActor(E, 1, 16, 2)
        assert ei.value.code == -5                # LL_ENODEV


def test_cdf_and_edges():
    """cdf: float32 running sum, 1 from the last live slot on; u below an edge takes the slot the edge closes, u at the edge the next live one; a slot
    with probability 0 has an empty interval; the one word whose u rounds to 1 takes the last live slot."""
    cdf = LR.cdf_of((0.25, 0.0, 0.5, 0.25, 0.0))
    np.testing.assert_array_equal(cdf, np.array([0.25, 0.25, 0.75, 1.0, 1.0], np.float32))
    below = np.nextafter(np.float32(0.25), np.float32(0))
    assert LR.slot_of_u(below, cdf) == 1
    assert LR.slot_of_u(np.float32(0.25), cdf) == 3          # (slot 2 is empty)
    assert LR.slot_of_u(np.nextafter(np.float32(0.75), np.float32(0)), cdf) == 3 and LR.slot_of_u(np.float32(0.75), cdf) == 4
    assert LR.slot_of_u(np.float32(1.0), cdf) == 4
    u = LR.u_of_word(np.array([0, 255, 256, 0x80000000, 0xFFFFFEFF, 0xFFFFFFFF], np.uint32))
    assert u.dtype == np.float32 and u[0] == u[1] == np.float32(2.0 ** -25) and u[2] == np.float32(1.5 * 2.0 ** -24) and u[3] == np.float32(0.5 + 2.0 ** -25)
    assert u[4] < 1.0 and u[5] == 1.0                       # 2^24 - 0.5 is no float32: the topmost word rounds up
    # rounding of the running sum cannot open an interval for a dead last slot
    cdf = LR.cdf_of((0.1,) * 3 + (0.7 - 1e-7, 0.0))
    assert cdf[3] == 1.0 and cdf[4] == 1.0 and (LR.slot_of_u(LR.u_of_word(np.arange(0xFFFF0000, 0x100000000, 251, dtype=np.uint64).astype(np.uint32)), cdf) <= 4).all()


def test_draw_follows_the_probabilities():
    """20 000 (arena, episode) pairs: the histogram passes chi-square against the probabilities, the zero slot is never drawn (fixed seed: deterministic)"""
    probs = np.array([0.4, 0.0, 0.35, 0.05, 0.2])
    arena, episode = np.meshgrid(np.arange(200), np.arange(100), indexing='ij')
    s = LR.draw_slot(arena.ravel(), episode.ravel(), 0xC0FFEE, LR.cdf_of(probs))
    counts = np.bincount(s, minlength=6)[1:]
    assert counts.sum() == 20000 and counts[1] == 0
    stat, dof, pv = G.chi2_pvalue(counts, probs)
    print('chi2 %.2f on %d dof, p %.3f, counts %s' % (stat, dof, pv, counts))
    assert dof == 3 and pv > 1e-3
    # the draw depends on the arena, the episode and the seed, each on its own
    base = LR.draw_word(3, 7, 11)
    assert base != LR.draw_word(4, 7, 11) and base != LR.draw_word(3, 8, 11) and base != LR.draw_word(3, 7, 12) and base != LR.draw_word(3, 7 + (1 << 32), 11)


@pytest.mark.parametrize('A,K', [(1, 1), (17, 3), (33, 1), (64, 4), (1000, 8)])
def test_plan_is_a_counting_sort_into_groups_of_one_slot(A, K):
    rng = np.random.default_rng(A * 10 + K)
    slots = rng.integers(1, K + 1, A)
    if K == 4:
        slots[slots == 2] = 3                               # an empty slot
    rows, groups = LR.plan(slots, K)
    assert sorted(rows.tolist()) == [2 * a + 1 for a in range(A)]            # every arena once
    seen = 0
    for slot, first, count in groups:
        assert first == seen and 1 <= count <= LR.GROUP
        members = (rows[first:first + count] - 1) // 2
        assert (slots[members] == slot).all()                                # a group never mixes slots
        assert (np.diff(members) > 0).all()
        seen += count
    assert seen == A
    assert [g[0] for g in groups] == sorted(g[0] for g in groups)
    for k in range(1, K + 1):
        n, mine = int((slots == k).sum()), [g for g in groups if g[0] == k]
        assert len(mine) == (n + LR.GROUP - 1) // LR.GROUP                   # none for an empty slot
        assert all(g[2] == LR.GROUP for g in mine[:-1])                      # only the last may be partial
    assert len(groups) <= (A + LR.GROUP - 1) // LR.GROUP + K                 # the act launch's upper bound


@pytest.mark.parametrize('A,probs,eseed,seed', LR.GPU_CASES)
def test_gpu_cases_exercise_every_slot_and_a_partial_group(A, probs, eseed, seed):
    """What test_gpu_hl_league relies on, from Philox alone: over the first four episodes of every arena each slot with a non-zero probability is
    drawn and the dead one never; and at the first step, where every arena draws episode 0 at once, some slot's row count is no multiple of 16."""
    cdf = LR.cdf_of(probs)
    arena, episode = np.meshgrid(np.arange(A), np.arange(4), indexing='ij')
    s = LR.draw_slot(arena, episode, seed, cdf)
    live = {1 + k for k, p in enumerate(probs) if p > 0}
    assert set(np.unique(s)) == live
    first = np.bincount(s[:, 0], minlength=len(probs) + 1)[1:]
    assert (first % LR.GROUP != 0).any()
    m = LR.Mirror(A, probs, seed)
    np.testing.assert_array_equal(m.begin_step(), s[:, 0])
    done = np.arange(A) % 2 == 0
    np.testing.assert_array_equal(m.begin_step(done, np.full(A, 2 | 8)), np.where(done, s[:, 1], s[:, 0]))
    assert m.tally[:, 0].sum() == done.sum() and (m.tally[:, 2] == m.tally[:, 0]).all() and (m.tally[:, 3] == m.tally[:, 0]).all() and not m.tally[:, 1].any()
