"""The PPO actor of the on-device EPMC / SEPMC policies without a GPU: the new declarations of include/hl/llenv_hl_policy.h against the binding and
libllenv.so, the value-branch fixtures against the checkpoint's array map, argument checks, LL_ENODEV without a device, and the row-wise reference
the GPU tests compare against (tests/hl_policy_pg_ref.py): modes equal to hl_policy_ref's, normalised categorical neglogp, a Gumbel sampler
whose histogram is the softmax, a finite value on recorded observations."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from lifelike_agility_and_play_amd import capi
from lifelike_agility_and_play_amd.policies import hl_policy_hip as H
import hl_policy_pg_ref as G
import hl_policy_ref as R
import philox_ref as P

HEADER = os.path.join(ROOT, 'include', 'hl', 'llenv_hl_policy.h')
NEW = ['ll_hl_policy_act_pg', 'll_hl_policy_attach_value', 'll_hl_policy_get_value_state', 'll_hl_policy_set_value_state']


def _lib():
    import __graft_entry__ as g
    g.build_hip()
    return H.load_library()


def test_new_declarations_binding_and_library_agree():
    text = open(HEADER).read()
    declared = sorted(set(re.findall(r'\b(ll_hl_policy_[a-z0-9_]+)\s*\(', text)))
    assert declared == H.EXPORTED_SYMBOLS
    assert set(NEW) <= set(declared)
    lib = _lib()
    for name in NEW:
        assert hasattr(lib, name), name
    for name, v in (('LLH_EPMC_VF_N_FLOATS', 137872), ('LLH_SEPMC_VF_N_FLOATS', 182864), ('LLH_EPMC_N_HEADS', 2), ('LLH_SEPMC_N_HEADS', 3)):
        assert re.search(r'#define %s\s+%d\b' % (name, v), text), name
    assert H.VF_N_FLOATS == {H.LLH_EPMC: 137872, H.LLH_SEPMC: 182864} and H.N_HEADS == {H.LLH_EPMC: 2, H.LLH_SEPMC: 3}
    assert G.N_HEADS == {'epmc': 2, 'sepmc': 3}
    src = open(os.path.join(ROOT, 'lifelike_agility_and_play_amd', 'csrc', 'hl_policy.inc')).read()
    for name, v in (('HL_HEADING_SALT', G.HEADING_SALT), ('HL_Z_SALT', G.Z_SALT), ('HL_LLC_SALT', G.LLC_SALT)):
        assert re.search(r'#define %s 0x%xu\b' % (name, v), src, re.I), name


def test_salts_are_new_streams():
    old = {P.RANDOM_POLICY_SALT, P.PMC_START_WORD, P.EPMC_RESET_SALT, P.EPMC_STEP_SALT, P.SEPMC_RESET_SALT, P.SEPMC_STEP_SALT, P.POLICY_NOISE_SALT}
    new = {G.HEADING_SALT, G.Z_SALT, G.LLC_SALT}
    assert len(new) == 3 and not (new & old)


# (shape of every value array) -- epmc_net.py:226-244 / sepmc_net.py:271-289
_PERCEPTS = [(1, 1, 1, 4), (4,), (4, 4, 4, 4), (4,), (2, 2, 4, 4), (4,), (2, 2, 4, 1), (1,),
             (4, 1, 4), (4,), (4, 4, 4), (4,), (4, 4, 4), (4,), (4, 4, 1), (1,),
             (1, 1, 1, 4), (4,), (4, 4, 4, 4), (4,), (2, 2, 4, 4), (4,), (2, 2, 4, 1), (1,)]
_LSTM = [(256, 128), (32, 128)] + [(128,)] * 5 + [(32,)] * 2
VALUE_SHAPES = {
    'epmc': [(135, 128), (128,)] + _PERCEPTS + [(3, 32), (32,), (120, 64), (64,), (64, 128), (128,), (256, 256), (256,)] + _LSTM + [(32, 1), (1,)],
    'sepmc': [(135, 128), (128,)] + _PERCEPTS + [(88, 64), (64,), (64, 128), (128,), (29, 64), (64,), (64, 64), (64,), (64, 128), (128,),
                                                 (384, 256), (256,)] + _LSTM + [(32, 1), (1,)],
}


@pytest.mark.parametrize('path,kind', [(G.EPMC_VALUE[k], 'epmc') for k in ('hurdle', 'hole', 'cube')] + [(G.SEPMC_VALUE, 'sepmc')])
def test_value_fixtures_follow_the_array_map(path, kind):
    z = np.load(path)
    first = 2
    want = {'w%d' % (first + i): s for i, s in enumerate(VALUE_SHAPES[kind])}
    assert sorted(z.files) == sorted(want)
    for k, s in want.items():
        assert z[k].shape == s and z[k].dtype == np.float32, (k, z[k].shape, s)
    assert os.path.getsize(path) < 1 << 20
    # the LSTM's three bias-like vectors (b, beta_x, beta_h) receive identical gradients: equal up to float32 rounding of the updates
    k0 = 36 if kind == 'epmc' else 40
    b = z['w%d' % (k0 + 2)]
    np.testing.assert_allclose(z['w%d' % (k0 + 3)], b, rtol=0, atol=1e-5)
    np.testing.assert_allclose(z['w%d' % (k0 + 5)], b, rtol=0, atol=1e-5)


def test_pack_value_weights_sizes():
    for which, path in sorted(G.EPMC_VALUE.items()):
        w = H.pack_value_weights(H.LLH_EPMC, path)
        assert w.dtype == np.float32 and w.size == 137872, which
        np.testing.assert_array_equal(w[:135 * 128], np.load(path)['w2'].ravel())
    w = H.pack_value_weights(H.LLH_SEPMC, G.SEPMC_VALUE)
    assert w.dtype == np.float32 and w.size == 182864
    np.testing.assert_array_equal(w[-1:], np.load(G.SEPMC_VALUE)['w50'].ravel())


def test_null_policy_is_einval():
    lib = _lib()
    w = np.zeros(137872, np.float32)
    s = np.zeros(64, np.float32)
    assert lib.ll_hl_policy_attach_value(None, w.ctypes.data_as(C.c_void_p), 137872) == -1
    assert lib.ll_hl_policy_act_pg(None, None, 916, None, None, None, None, None, None, 0, 0, 1, 1, None) == -1
    assert lib.ll_hl_policy_get_value_state(None, s.ctypes.data_as(C.c_void_p)) == -1
    assert lib.ll_hl_policy_set_value_state(None, s.ctypes.data_as(C.c_void_p)) == -1
    assert lib.ll_last_error().decode()


def test_no_gpu_means_loud_failure():
    """The right policy and value weights without a HIP device: LL_ENODEV, no CPU fallback."""
    import torch
    if torch.cuda.is_available():
        pytest.skip('a GPU is present')
    for cls, path, vpath in ((H.HipEpmcPolicy, R.EPMC_WEIGHTS['hurdle'], G.EPMC_VALUE['hurdle']), (H.HipSepmcPolicy, R.SEPMC_WEIGHTS, G.SEPMC_VALUE)):
        with pytest.raises(capi.LLError) as ei:
            cls(path, 64, value_npz=vpath)
        assert ei.value.code == -5                # LL_ENODEV


def _obs(kind, n, rng):
    z = np.load(os.path.join(R.GOLDEN, 'epmc_golden.npz' if kind == 'epmc' else 'sepmc_golden.npz'))
    real = z['e_obs_full'].reshape(-1, 916 if kind == 'epmc' else 965).astype(np.float64)
    x = real[rng.integers(0, len(real), n)]
    x[:, :135] += rng.normal(0, 0.05, (n, 135))
    return x


@pytest.mark.parametrize('kind', ['epmc', 'sepmc'])
def test_modes_are_the_oracle_policy(kind):
    """sample=False: the reference's actions, code, heading and policy state == hl_policy_ref.forward's (== the oracle's,
    test_hl_policy_api.test_reference_is_the_oracle_policy), the Gaussian neglogp is its normalising constant."""
    rng = np.random.default_rng(3)
    n = 20
    path = R.EPMC_WEIGHTS['hurdle'] if kind == 'epmc' else R.SEPMC_WEIGHTS
    w = R.load(path)
    obs = _obs(kind, n, rng)
    st = rng.normal(0, 0.3, (n, 64 if kind == 'epmc' else 128))
    reset = np.arange(n) % 4 == 0
    a = R.forward(kind, w, obs, st, reset)
    b = G.forward(kind, w, obs, st, reset, seed=5, step=9, sample=False)
    np.testing.assert_array_equal(b['code'], a['code'])
    for k in ('action', 'state') + (('heading',) if kind == 'sepmc' else ()):
        np.testing.assert_allclose(b[k], a[k], rtol=0, atol=1e-12, err_msg=k)
    ls = w[G.LOGSTD[kind]][0]
    np.testing.assert_allclose(b['neglogp'][:, -1], 6 * G.LOG_2PI + ls.sum(), rtol=1e-12)
    if kind == 'sepmc':
        np.testing.assert_allclose(b['neglogp'][:, 0], 0.5 * G.LOG_2PI + w[G.HLC_LOGSTD][0, 0], rtol=1e-12)


@pytest.mark.parametrize('kind', ['epmc', 'sepmc'])
def test_sampled_heads_are_consistent(kind):
    """sample=True: the code is the argmax of the perturbed logits, the llc neglogp is the Gaussian density of the emitted action around the
    controller's mean at that code, and exp(-neglogp) of the z head over all 256 codes sums to one."""
    rng = np.random.default_rng(4)
    n = 12
    path = R.EPMC_WEIGHTS['hole'] if kind == 'epmc' else R.SEPMC_WEIGHTS
    w = R.load(path)
    obs = _obs(kind, n, rng)
    st = np.zeros((n, 64 if kind == 'epmc' else 128))
    r = G.forward(kind, w, obs, st, seed=77, step=3, sample=True)
    np.testing.assert_array_equal(r['code'], np.argmax(r['score'] + G.z_noise(np.arange(n), 3, 77), axis=1))
    zc = 1 if kind == 'sepmc' else 0                                  # the z column of neglogp
    tot = np.zeros(n)
    for c in range(256):
        tot += np.exp(-G.forward(kind, w, obs, st, seed=77, step=3, sample=True, code=np.full(n, c))['neglogp'][:, zc])
    np.testing.assert_allclose(tot, 1.0, rtol=1e-10)
    mean = G.forward(kind, w, obs, st, seed=77, step=3, sample=False, code=r['code'])['action'] if kind == 'epmc' else None
    if mean is not None:
        ls = w[G.LOGSTD[kind]][0]
        want = 0.5 * (((r['action'] - mean) / np.exp(ls)) ** 2).sum(axis=1) + 6 * G.LOG_2PI + ls.sum()
        np.testing.assert_allclose(r['neglogp'][:, 1], want, rtol=1e-10)
    r2 = G.forward(kind, w, obs, st, seed=77, step=4, sample=True)
    assert (r2['action'] != r['action']).any()                      # another step, other draws


def test_gumbel_words_at_the_ends_are_finite():
    g = G.gumbel(np.array([0, 255, 1 << 31, (1 << 31) - 1, 0xFFFFFF00, 0xFFFFFFFF], np.uint32))
    assert np.isfinite(g).all()
    assert g[0] < -2.8 and g[-1] > 17.0                              # u = 2^-25 and u = 1 - 2^-25


def test_gumbel_sampler_follows_the_softmax():
    """Over 24 000 (seed, step) draws of one row, the Gumbel-max code's histogram passes chi-square against the softmax of the logits (fixed
    seeds: deterministic)."""
    rng = np.random.default_rng(8)
    w = R.load(R.EPMC_WEIGHTS['cube'])
    obs = _obs('epmc', 1, rng)
    score = R.forward('epmc', w, obs, np.zeros((1, 64)))['score'][0] * 0.25      # flattened: many codes with mass
    p = np.exp(score - score.max())
    p /= p.sum()
    counts = np.zeros(256)
    for seed in (1, 2, 3):
        for s0 in range(0, 8000, 500):
            steps = np.arange(s0, s0 + 500)
            nz = np.stack([G.z_noise([17], s, seed)[0] for s in steps])
            counts += np.bincount(np.argmax(score[None, :] + nz, axis=1), minlength=256)
    stat, dof, pv = G.chi2_pvalue(counts, p)
    print('chi2 %.1f on %d dof, p %.3f' % (stat, dof, pv))
    assert dof > 20 and pv > 1e-3, (stat, dof, pv)


@pytest.mark.parametrize('kind,which', [('epmc', 'hurdle'), ('epmc', 'hole'), ('epmc', 'cube'), ('sepmc', None)])
def test_value_on_recorded_observations_is_finite(kind, which):
    z = np.load(os.path.join(R.GOLDEN, 'epmc_golden.npz' if kind == 'epmc' else 'sepmc_golden.npz'))
    obs = z['e_obs_full'].reshape(-1, 916 if kind == 'epmc' else 965).astype(np.float64)
    path, vpath = (R.EPMC_WEIGHTS[which], G.EPMC_VALUE[which]) if kind == 'epmc' else (R.SEPMC_WEIGHTS, G.SEPMC_VALUE)
    w, w32 = R.load(path), R.load(path, np.float32)
    wv = G.load_value(vpath, w)
    vs = np.zeros((len(obs), 64))
    for _ in range(3):
        v, vs = G.value(kind, wv, obs, vs)
        assert np.isfinite(v).all() and np.isfinite(vs).all()
    print(kind, which, 'value range %.3f .. %.3f' % (v.min(), v.max()))
    assert np.ptp(v) > 0
    t = G.tolerances(kind, w, w32, obs[:8], np.zeros((8, 64 if kind == 'epmc' else 128)), seed=1, step=2, wv64=wv, wv32=G.load_value(vpath, w32),
                     vstate=np.zeros((8, 64)))
    assert t['tol_value'] < 1e-3 and t['tol_neglogp'] < 1e-2, t
