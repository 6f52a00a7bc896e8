"""The unroll recorder of the on-device EPMC / SEPMC actors without a GPU: include/hl/llenv_hl_unroll.h == policies.hl_unroll == what libllenv.so
exports, the row layout, argument checks before the device is touched, loud failure without a device, and the NumPy reference the GPU tests compare
against (tests/hl_unroll_ref.py): TD(lambda) against its closed form, the M / S rule on a hand-written case."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from lifelike_agility_and_play_amd import capi
from lifelike_agility_and_play_amd.policies import hl_policy_hip as H
from lifelike_agility_and_play_amd.policies import hl_unroll as U
import hl_unroll_ref as UR


def _lib():
    import __graft_entry__ as g
    g.build_hip()
    return U.load_library()


def test_header_binding_and_library_agree():
    text = open(os.path.join(ROOT, 'include', 'hl', 'llenv_hl_unroll.h')).read()
    declared = sorted(set(re.findall(r'\b(ll_hl_unroll_[a-z0-9_]+)\s*\(', text)))
    assert declared == U.EXPORTED_SYMBOLS and len(declared) == 7
    lib = _lib()
    for name in declared:
        assert hasattr(lib, name), name
    fields = re.findall(r'#define LLU_([A-Z]+) (\d+)\n', text)
    assert [(n, int(v)) for n, v in fields[:10]] == list(zip(('X', 'A', 'NEGLOGP', 'R', 'V', 'REWARD', 'DISCOUNT', 'S', 'M', 'PAD'), range(10)))
    assert len(U.LLU_FIELDS) == 10 and re.search(r'#define LLU_N_FIELDS 10\b', text)
    for name, kind in (('LLU_EPMC_ROW_FLOATS', H.LLH_EPMC), ('LLU_SEPMC_ROW_FLOATS', H.LLH_SEPMC)):
        assert re.search(r'#define %s\s+%d\b' % (name, U.ROW_FLOATS[kind]), text), name
    # struct ll_hl_unroll_layout_t: six int32, two int32[10], a pointer, a uint64
    assert C.sizeof(U.LLHlUnrollLayout) == 6 * 4 + 2 * 10 * 4 + 8 + 8 and U.LLHlUnrollLayout.d_base.offset == 104


def test_row_layout():
    """the table of the header: widths, offsets, row_floats a multiple of 4"""
    lay, rf = U.row_layout(H.LLH_EPMC)
    assert rf == 1128 and [lay[k] for k in U.LLU_FIELDS] == [(0, 916), (916, 13), (929, 2), (931, 1), (932, 1), (933, 1), (934, 1), (935, 192), (1127, 1), (1128, 0)]
    lay, rf = U.row_layout(H.LLH_SEPMC)
    assert rf == 1244 and [lay[k] for k in U.LLU_FIELDS] == [(0, 965), (965, 14), (979, 3), (982, 1), (983, 1), (984, 1), (985, 1), (986, 256), (1242, 1), (1243, 1)]
    rows = np.arange(2 * 3 * 1244, dtype=np.float32).reshape(2, 3, 1244)
    f = U.split_row(rows)
    assert f['X'].shape == (2, 3, 965) and f['A'].shape == (2, 3, 14) and f['S'].shape == (2, 3, 256) and f['R'].shape == (2, 3) and f['pad'].shape == (2, 3, 1)
    assert f['M'][1, 2] == rows[1, 2, 1242] and f['V'][0, 1] == rows[0, 1, 983]
    f['R'][:] = -1.0                                     # views, not copies
    assert (rows[..., 982] == -1.0).all()
    with pytest.raises(ValueError):
        U.split_row(np.zeros((4, 224), np.float32))


def test_bad_arguments_are_einval_before_the_device():
    lib = _lib()
    h = C.c_void_p()
    for create in (lib.ll_hl_unroll_create_epmc, lib.ll_hl_unroll_create_sepmc):
        assert create(None, None, 32, 2, C.byref(h)) == -1 and not h.value
        assert lib.ll_last_error().decode()
        assert create(None, None, 32, 2, None) == -1
    assert lib.ll_hl_unroll_steps(None, 1, 1, 1) == -1
    assert lib.ll_hl_unroll_finish(None, 0, 0.95, 0.95, None) == -1
    assert lib.ll_hl_unroll_layout(None, None) == -1
    k, t = C.c_int64(0), C.c_int(0)
    assert lib.ll_hl_unroll_position(None, C.byref(k), C.byref(t)) == -1
    assert lib.ll_hl_unroll_destroy(None) == 0


def test_no_gpu_means_loud_failure():
    """A recorder cannot be made of anything but an engine and a policy, and without a HIP device neither can exist: the policy refuses with
    LL_ENODEV (no CPU fallback) and the binding raises instead of crashing.  (With a device present the second half has nothing to show.)"""
    import torch
    with pytest.raises(TypeError):
        U.HlUnrollRecorder(object(), None, 32, 2)
    if not torch.cuda.is_available():
        import hl_policy_pg_ref as G
        import hl_policy_ref as R
        with pytest.raises(capi.LLError) as ei:
            pol = H.HipEpmcPolicy(R.EPMC_WEIGHTS['hurdle'], 64, value_npz=G.EPMC_VALUE['hurdle'])
            U.HlUnrollRecorder(None, pol, 32, 2)
        assert ei.value.code == -5                # LL_ENODEV


def test_td_lambda_is_its_closed_form():
    rng = np.random.default_rng(3)
    n, T = 37, 24
    r, V, boot = rng.normal(size=(n, T)), rng.normal(size=(n, T)), rng.normal(size=n)
    done = rng.random((n, T)) < 0.15
    done[0] = False
    done[1, -1] = True
    m = 1.0 - done
    for gamma, lam in ((0.95, 0.95), (0.99, 0.8), (1.0, 1.0), (0.9, 0.0)):
        R = UR.td_lambda(r, V, m, boot, gamma, lam)
        np.testing.assert_allclose(R, UR.td_lambda_closed_form(r, V, m, boot, gamma, lam), rtol=1e-12, atol=1e-12)
        # a row that ends at its last step does not see the bootstrap
        assert np.array_equal(R[1], UR.td_lambda(r, V, m, boot + 5.0, gamma, lam)[1])
        assert (R[0] != UR.td_lambda(r, V, m, boot + 5.0, gamma, lam)[0]).all() or gamma * lam == 0.0
    # lam = 0: the one-step TD target; gamma = lam = 1 without ends: the sum of rewards plus the bootstrap
    np.testing.assert_allclose(UR.td_lambda(r, V, m, boot, 0.9, 0.0)[:, :-1], r[:, :-1] + 0.9 * V[:, 1:] * m[:, :-1], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(UR.td_lambda(r[:1], V[:1], m[:1], boot[:1], 1.0, 1.0)[0, 0], r[0].sum() + boot[0], rtol=1e-12)
    # the float32 pass is the float64 one up to rounding
    R32 = UR.td_lambda(r, V, m, boot, 0.95, 0.95, dtype=np.float32)
    assert R32.dtype == np.float32 and 0 < np.abs(R32 - UR.td_lambda(r, V, m, boot, 0.95, 0.95)).max() < 1e-4


def test_mask_and_state_rule_three_steps():
    """distill_actor.py:121-140 by hand, one robot, two unrolls of 3 frames, the episode ending at global steps 1 and 2 (so the act of steps 2 and 3
    restarts from zero): `mask = False` at the top of every unroll, `mask = done` after a frame.
    unroll 0: frames 0, 1, 2 -> M 0, 0, 1; unroll 1: frame 3 is a first frame -> M 0 although it restarted, then 0, 0.  S of a restarted frame is zero."""
    hs = np.arange(1, 7, dtype=np.float64)[:, None, None] * np.ones((6, 1, 192))
    done = np.array([0, 1, 1, 0, 0, 0])[:, None]
    reset = np.concatenate([[[0]], done[:-1]])             # the d_reset of step t is the done of step t - 1
    want_M = [[0, 0, 1], [0, 0, 0]]
    want_S = [[1, 2, 0], [0, 5, 6]]
    for u in range(2):
        S, M = UR.mask_and_state(hs[3 * u:3 * u + 3], reset[3 * u:3 * u + 3])
        assert M[:, 0].tolist() == want_M[u] and S[:, 0, 0].tolist() == want_S[u] and S[:, 0, 191].tolist() == want_S[u]
    # and through the packing: EPMC rows, every field where the header says
    T, n = 3, 1
    rng = np.random.default_rng(0)
    obs, act, nl = rng.normal(size=(T, n, 916)), rng.normal(size=(T, n, 12)), rng.normal(size=(T, n, 2))
    code, val, rew = np.array([[7], [255], [0]]), rng.normal(size=(T, n)), rng.normal(size=(T, n))
    blk = UR.pack_unroll('epmc', obs, code, act, nl, val, rew, done[:3], hs[:3], reset[:3])
    assert blk.shape == (1, 3, 1128)
    row = blk[0, 2]
    assert np.array_equal(row[:916], obs[2, 0]) and row[916] == 0.0 and np.array_equal(row[917:929], act[2, 0]) and np.array_equal(row[929:931], nl[2, 0])
    assert row[931] == 0.0 and row[932] == val[2, 0] and row[933] == rew[2, 0] and row[934] == 0.0 and not row[935:1127].any() and row[1127] == 1.0
    assert blk[0, 1, 916] == 255.0 and blk[0, 1, 934] == 0.0 and blk[0, 0, 934] == 1.0 and (blk[0, 1, 935:1127] == 2.0).all() and blk[0, 1, 1127] == 0.0
    blk = UR.pack_unroll('sepmc', rng.normal(size=(T, n, 965)), code, act, rng.normal(size=(T, n, 3)), val, rew, done[:3], np.ones((T, n, 256)), reset[:3],
                         heading=np.array([[0.5], [-0.25], [3.0]]))
    assert blk.shape == (1, 3, 1244) and blk[0, 1, 965] == -0.25 and blk[0, 1, 966] == 255.0 and np.array_equal(blk[0, 1, 967:979], act[1, 0])
    assert blk[0, 2, 1242] == 1.0 and not blk[..., 1243].any()
