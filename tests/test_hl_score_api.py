"""The teacher-forced scorer of recorded unrolls without a GPU: include/hl/llenv_hl_score.h == policies.hl_score == what libllenv.so exports, the
layout of an output row, argument checks before the device is touched, and the NumPy reference the GPU tests compare against
(tests/hl_score_ref.py) on a hand-written two-step case."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from lifelike_agility_and_play_amd import capi
from lifelike_agility_and_play_amd.policies import hl_policy_hip as H
from lifelike_agility_and_play_amd.policies import hl_score as SC
from lifelike_agility_and_play_amd.policies import hl_unroll as U
import hl_policy_pg_ref as G
import hl_policy_ref as R
import hl_score_ref as SR


def _lib():
    import __graft_entry__ as g
    g.build_hip()
    return SC.load_library()


def test_header_binding_and_library_agree():
    text = open(os.path.join(ROOT, 'include', 'hl', 'llenv_hl_score.h')).read()
    declared = sorted(set(re.findall(r'\b(ll_hl_score_[a-z0-9_]+)\s*\(', text)))
    assert declared == SC.EXPORTED_SYMBOLS == sorted(SC._SIGS) and len(declared) == 4
    lib = _lib()
    for name in declared:
        assert hasattr(lib, name), name
    assert re.search(r'#define LLS_OUT_FLOATS %d\b' % SC.LLS_OUT_FLOATS, text) and SC.LLS_OUT_FLOATS == 8
    fields = re.findall(r'#define LLS_([A-Z]+) (\d+)\n', text)
    assert [(n, int(v)) for n, v in fields] == list(zip(('NEGLOGP', 'ENTROPY', 'V', 'PAD'), range(4)))
    assert len(SC.LLS_FIELDS) == 4 and re.search(r'#define LLS_N_FIELDS 4\b', text)
    # struct ll_hl_score_layout_t: four int32, two int32[4]
    assert C.sizeof(SC.LLHlScoreLayout) == 4 * 4 + 2 * 4 * 4 and SC.LLHlScoreLayout.off.offset == 16
    # additive entry points: the ABI version of llenv.h stays
    assert lib.ll_abi_version() == capi.LL_ABI_VERSION


@pytest.mark.parametrize('kind,nh,want', [(H.LLH_EPMC, 2, [(0, 2), (2, 2), (4, 1), (5, 3)]), (H.LLH_SEPMC, 3, [(0, 3), (3, 3), (6, 1), (7, 1)])])
def test_layout_table(kind, nh, want):
    """the table of the header from the library, and the binding's restatement of it"""
    lib = _lib()
    lay = SC.LLHlScoreLayout()
    assert lib.ll_hl_score_layout(kind, C.byref(lay)) == 0
    assert (lay.kind, lay.n_heads, lay.out_floats, lay.reserved) == (kind, nh, 8, 0)
    assert [(lay.off[i], lay.dim[i]) for i in range(4)] == want
    assert [SC.out_layout(kind)[k] for k in SC.LLS_FIELDS] == want
    assert sum(d for _, d in want) == SC.LLS_OUT_FLOATS
    rows = np.arange(2 * 3 * 8, dtype=np.float32).reshape(2, 3, 8)
    f = SC.split_out(rows, kind)
    assert f['neglogp'].shape == (2, 3, nh) and f['entropy'].shape == (2, 3, nh) and f['V'].shape == (2, 3) and f['pad'].shape == (2, 3, 7 - 2 * nh)
    assert f['V'][1, 2] == rows[1, 2, 2 * nh] and f['entropy'][0, 1, 0] == rows[0, 1, nh]
    f['V'][:] = -1.0                                     # views, not copies
    assert (rows[..., 2 * nh] == -1.0).all()
    with pytest.raises(ValueError):
        SC.split_out(np.zeros((4, 7), np.float32), kind)
    with pytest.raises(ValueError):
        SC.split_out(rows)                               # a bare array does not say its kind


def test_bad_arguments_are_einval_before_the_device():
    lib = _lib()
    lay = SC.LLHlScoreLayout()
    for kind in (0, 3, -1):
        assert lib.ll_hl_score_layout(kind, C.byref(lay)) == -1 and lib.ll_last_error().decode()
    assert lib.ll_hl_score_layout(H.LLH_EPMC, None) == -1
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    assert lib.ll_hl_score_rows(None, p, 1, 1, p, None) == -1 and lib.ll_last_error().decode()
    assert lib.ll_hl_score_rows(None, None, 1, 1, None, None) == -1
    for n, L in ((0, 1), (1, 0), (-4, 8), (8, -1)):
        assert lib.ll_hl_score_rows(None, p, n, L, p, None) == -1
    for fn in (lib.ll_hl_score_unroll, lib.ll_hl_score_league):
        assert fn(None, None, 0, p) == -1 and lib.ll_last_error().decode()
        assert fn(None, None, -1, None) == -1


def test_no_gpu_means_loud_failure():
    """score() takes a recorder or a league and nothing else; without a HIP device neither a carrier nor a block can exist (LL_ENODEV, no CPU path)."""
    import torch
    with pytest.raises(TypeError):
        SC.score(None, object(), 0)
    if not torch.cuda.is_available():
        with pytest.raises(capi.LLError) as ei:
            H.HipEpmcPolicy(R.EPMC_WEIGHTS['hurdle'], 16, value_npz=G.EPMC_VALUE['hurdle'])
        assert ei.value.code == -5                # LL_ENODEV


def _two_step_block(kind, w, wv, rng, n=3):
    """n rows, two time steps, by the float64 actor reference (sample = 0: the modes), the second step from whatever the first left; S_0 random"""
    k = SR.KIND[kind]
    od = H.OBS_DIM[k]
    obs = rng.normal(0.0, 0.5, (2, n, od))
    obs[..., 135:913] = rng.uniform(0.0, 1.0, (2, n, 778))
    S0 = rng.normal(0.0, 0.4, (n, U.S_DIM[k]))
    st = S0[:, 128:192] if kind == 'epmc' else np.concatenate([S0[:, 192:256], S0[:, 128:192]], axis=1)
    vst = S0[:, 0:64]
    steps = []
    for t in range(2):
        r = G.forward(kind, w, obs[t], st, sample=False, wv=wv, vstate=vst)
        steps.append(r)
        st, vst = r['state'], r['vstate']
    lay, rf = U.row_layout(k)
    blk = np.zeros((n, 2, rf))
    f = U.split_row(blk, lay)
    for t, r in enumerate(steps):
        f['X'][:, t] = obs[t]
        a = [r['code'][:, None].astype(np.float64), r['action']]
        if kind == 'sepmc':
            a.insert(0, r['heading'][:, None])
        f['A'][:, t] = np.concatenate(a, axis=1)
        f['neglogp'][:, t] = r['neglogp']
        f['V'][:, t] = r['value']
    f['S'][:, 0] = S0
    return blk, steps


@pytest.mark.parametrize('kind', ['epmc', 'sepmc'])
def test_reference_two_steps_by_hand(kind):
    """The reference on two hand-made steps.  Scored under the weights that made them, the modes give back the actor reference's neglogp and V, the
    state carried from step 0 to step 1.  With M_1 = 1, step 1 is a fresh step 0 from zero state (and S_1, M_0 are never read).  With the action put
    k sigma off the mean, the Gaussian neglogp is the closed form 0.5 * 12 k^2 + 6 log 2 pi + sum logstd; the entropies are the constants."""
    rng = np.random.default_rng(5)
    path, vpath = (R.EPMC_WEIGHTS['hurdle'], G.EPMC_VALUE['hurdle']) if kind == 'epmc' else (R.SEPMC_WEIGHTS, G.SEPMC_VALUE)
    w = R.load(path)
    wv = G.load_value(vpath, w)
    k = SR.KIND[kind]
    nh = H.N_HEADS[k]
    blk, steps = _two_step_block(kind, w, wv, rng)
    f = U.split_row(blk, U.row_layout(k)[0])
    out = SR.score(kind, w, wv, blk)
    o = SC.split_out(out, k)
    assert out.shape == (3, 2, 8) and not o['pad'].any()
    for t in range(2):
        np.testing.assert_allclose(o['neglogp'][:, t], steps[t]['neglogp'], rtol=0, atol=1e-9)
        np.testing.assert_allclose(o['V'][:, t], steps[t]['value'], rtol=0, atol=1e-12)
    for col, val in SR.gaussian_entropy(kind, w).items():
        np.testing.assert_allclose(out[..., col], val, rtol=0, atol=1e-12)
    sc = steps[0]['score']
    p = np.exp(sc - G.logsumexp(sc)[:, None])
    np.testing.assert_allclose(o['entropy'][:, 0, nh - 2], -(p * np.log(p)).sum(axis=1), rtol=0, atol=1e-9)
    # M_1 = 1 on row 1: its step 1 is a fresh step 0 from zero state; rows 0 and 2 keep their carried state; S_1 and M_0 are not read
    b2 = blk.copy()
    f2 = U.split_row(b2, U.row_layout(k)[0])
    f2['M'][1, 1] = 1.0
    f2['M'][:, 0] = 1.0
    f2['S'][:, 1] = 123.0
    out2 = SR.score(kind, w, wv, b2)
    fresh = np.zeros_like(b2[:, :1])
    ff = U.split_row(fresh, U.row_layout(k)[0])
    ff['X'][:, 0], ff['A'][:, 0] = f['X'][:, 1], f['A'][:, 1]
    out_fresh = SR.score(kind, w, wv, fresh)
    np.testing.assert_array_equal(out2[1, 1], out_fresh[1, 0])
    np.testing.assert_array_equal(out2[[0, 2]], out[[0, 2]])
    np.testing.assert_array_equal(out2[:, 0], out[:, 0])
    assert (out2[1, 1, :nh] != out[1, 1, :nh]).any() and out2[1, 1, 2 * nh] != out[1, 1, 2 * nh]
    # sigma-scaled actions (and heading): the closed form
    b3 = blk.copy()
    f3 = U.split_row(b3, U.row_layout(k)[0])
    ls = w[G.LOGSTD[kind]][0]
    for kk, row in ((0.0, 0), (1.0, 1), (-2.5, 2)):
        f3['A'][row, :, -12:] += kk * np.exp(ls)
        if kind == 'sepmc':
            f3['A'][row, 0, 0] += kk * np.exp(w[G.HLC_LOGSTD][0, 0])
    out3 = SR.score(kind, w, wv, b3)
    for kk, row in ((0.0, 0), (1.0, 1), (-2.5, 2)):
        np.testing.assert_allclose(out3[row, :, nh - 1], 0.5 * 12 * kk * kk + 6 * G.LOG_2PI + ls.sum(), rtol=0, atol=1e-7)
        if kind == 'sepmc':
            np.testing.assert_allclose(out3[row, 0, 0], 0.5 * kk * kk + 0.5 * G.LOG_2PI + w[G.HLC_LOGSTD][0, 0], rtol=0, atol=1e-7)
    if kind == 'epmc':                                   # (the z head does not see the action; SEPMC's sees the heading through the target)
        np.testing.assert_array_equal(out3[..., nh - 2], out[..., nh - 2])
    # a code outside 0 .. 255: NaN in that time step's z and llc columns, everything else as it was
    b4 = blk.copy()
    f4 = U.split_row(b4, U.row_layout(k)[0])
    az = 1 if kind == 'sepmc' else 0
    f4['A'][0, 1, az], f4['A'][2, 0, az] = 300.0, -1.0
    out4 = SR.score(kind, w, wv, b4)
    bad = np.zeros(out.shape, bool)
    for row, t in ((0, 1), (2, 0)):
        bad[row, t, [nh - 2, nh - 1, 2 * nh - 2, 2 * nh - 1]] = True
    assert np.isnan(out4[bad]).all()
    np.testing.assert_array_equal(out4[~bad], out[~bad])
    # float32 against float64: the tolerance rule gives something sane on this block
    w32 = R.load(path, np.float32)
    t = SR.tolerances(kind, w, wv, w32, G.load_value(vpath, w32), blk)
    assert set(t['tol']) == set(SR.GROUPS[kind]) and all(1e-6 <= v < 1e-2 for v in t['tol'].values()), t['tol']
    assert all(e <= t['tol'][g] for g, e in SR.errors(kind, SR.score(kind, w32, G.load_value(vpath, w32), blk), t['ref']).items())


def test_pack_and_perturbed():
    w = R.load(R.EPMC_WEIGHTS['hurdle'], np.float32)
    wv = G.load_value(G.EPMC_VALUE['hurdle'], w)
    pw, pv = SR.pack('epmc', w, wv)
    np.testing.assert_array_equal(pw, H.pack_weights(H.LLH_EPMC, R.EPMC_WEIGHTS['hurdle']))
    np.testing.assert_array_equal(pv, H.pack_value_weights(H.LLH_EPMC, G.EPMC_VALUE['hurdle']))
    b = SR.perturbed(w, np.random.default_rng(1))
    assert b[0] is w[0] and b[1] is w[1] and all(b[i].dtype == np.float32 and b[i].shape == w[i].shape for i in w)
    rel = np.abs(b[97] / w[97] - 1.0)
    assert 0.01 < rel.mean() < 0.03
