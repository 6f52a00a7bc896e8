"""The host twin of the step kernels' math, rotation and geometry helpers (tests/lanes/math_helpers_host.cpp: pmc_math.hpp and the self-contained static members of
Pmc<L> compiled for the host lanes with correctly rounded IEEE operations and glibc's float functions) one helper at a time against the float64 statement of that
helper (tests/math_helpers_ref.py), on the exact, random and edge inputs of tests/math_helpers_common.py and under its class table.  No GPU: the same driver is compiled
for the GPU lanes and held to this twin's error and to the same statements in tests/test_gpu_math_helpers.py."""
import os
import re

import numpy as np
import pytest

import math_helpers_common as mh
import math_helpers_ref as ref


@pytest.fixture(scope='module')
def host():
    h = mh.HostRunner()          # builds tests/lanes/_build/libmath_helpers_host.so when its sources are newer
    h.cases = {}
    return h


def cases_of(host, name):
    if name not in host.cases:
        host.cases[name] = mh.cases(name, host.dims)
    return host.cases[name]


@pytest.mark.parametrize('name', list(mh.HELPERS))
def test_host_twin_against_statement(host, name):
    for case in cases_of(host, name):
        got = host.run(0, name, case)
        r = mh.check(name, case, got, host.dims, 'twin')
        print('%-22s %-52s worst |twin - statement| %.3e, worst error / bound %.3f' % (name, case.klass, r['err'].max(), r['ratio']))
        mh.partial_exec_check(host, 0, name, case, host.dims, got, 'twin')


@pytest.mark.parametrize('name', list(mh.HELPERS))
def test_input_classes(host, name):
    """every helper has its exact class (but Philox, whose every input is exact) and at least 4096 random inputs with fixed seeds; a second build of the cases is the same"""
    cs = cases_of(host, name)
    assert name == 'philox' or cs[0].klass == 'exact'
    assert name == 'mocap' or sum(c.n for c in cs if c.klass.startswith('random')) >= 4096
    again = mh.cases(name, host.dims)
    assert all(a.X.tobytes() == b.X.tobytes() and a.auxd.tobytes() == b.auxd.tobytes() for a, b in zip(cs, again))


@pytest.mark.parametrize('name', [n for n in mh.HELPERS if n in ref.STATEMENTS])
def test_bound_model_states_what_the_statement_states(host, name):
    """the bound models follow the helpers' operation sequences; their VALUES must be the independent statements' (so a bound is a bound on the right thing)"""
    for case in cases_of(host, name):
        w = mh.want(name, case, host.dims)
        v, m = w['v'], w['model_v'][:, :w['v'].shape[1]]
        ok = ~np.isnan(v) & ~np.isnan(m)
        if not ok.any():
            continue          # (a class held to the helper's own properties only)
        # 1e-9: the series of the small-angle branches and of sincos_joint's polynomials against the exact functions
        assert np.abs(v - m)[ok].max() <= 1e-9 + 1e-12 * np.abs(v[ok]).max(), (name, case.klass, np.abs(v - m)[ok].max())


def test_statements_against_scipy():
    from scipy.spatial.transform import Rotation as R
    r = np.random.default_rng(5)
    q = r.normal(size=(2000, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    np.testing.assert_allclose(ref.s_rotvec_of(q, None), R.from_quat(q).as_rotvec(), atol=1e-12)
    rv = r.normal(size=(2000, 3)) * r.uniform(0, 1.5, (2000, 1))
    got, sp = ref.s_quat_of_rotvec(rv, None), R.from_rotvec(rv).as_quat()
    np.testing.assert_allclose(got, sp * np.sign(np.einsum('ni,ni->n', got, sp))[:, None], atol=1e-14)


def test_seg_seg_branches_and_shares(host):
    """each of the lt / gt / interior branches is met, and the share of samples whose (s, t) hang on a comparison is below 5 % in every random class"""
    for case in cases_of(host, 'seg_seg_st'):
        X = case.X[:case.n].astype(np.float64)
        _, _, _, _, t0, _ = ref.seg_seg_f64(X)
        if case.klass.startswith('random'):
            assert (t0 < 0).sum() > 100 and (t0 > 1).sum() > 100 and ((t0 > 0) & (t0 < 1)).sum() > 100
            assert ref.seg_seg_fragile(X).mean() <= 0.05
            print('seg_seg_st %s: %.2f %% of the samples left out of the (s, t) comparison' % (case.klass, 100 * ref.seg_seg_fragile(X).mean()))


def test_sincos_joint_reduction_is_fused_in_the_twin(host):
    """pmc_step.hpp sincos_joint: the two Cody-Waite steps are one rounding each (lm::nfma_) in EVERY build -- the twin is built with -ffp-contract=off, and with separate
    products its error at |x| <= 1e3 was 3e-5"""
    case = [c for c in cases_of(host, 'sincos_joint') if c.klass == 'random |x| <= 1000'][0]
    got = host.run(0, 'sincos_joint', case)[:, :2].astype(np.float64)
    x = case.X[:, 0].astype(np.float64)
    err = np.abs(got - np.stack([np.sin(x), np.cos(x)], axis=1)).max()
    print('sincos_joint |x| <= 1e3: worst absolute error of the twin %.3e' % err)
    assert err <= 9e-8


def test_chol6_reciprocal_diagonal_within_2u(host):
    """d[i] * L_ii within 2 u of 1 (u = 2^-24): d[i] is the reciprocal of the stored L_ii = sqrt(s), one rounding of a reciprocal and one of the product.
    (chol6 used to take ONE reciprocal square root r of the pivot s and set d[i] = r, L_ii = s r: s r^2 carries the rounding of r twice and of s r once, and was
    2.38e-7 = 4 u from 1 here, 193 of 24576 entries above 2 u, and 3 u on an MI355X.)"""
    case = [c for c in cases_of(host, 'chol_solve') if c.klass.startswith('random')][0]
    dl = host.run(0, 'chol_solve', case)[:case.n, 6:12].astype(np.float64)
    print('chol6: worst |d[i] L_ii - 1| = %.3e = %.2f u, %d of %d above 2 u' % (np.abs(dl - 1).max(), np.abs(dl - 1).max() / ref.U, (np.abs(dl - 1) > 2 * ref.U).sum(), dl.size))
    assert np.abs(dl - 1).max() <= 2 * ref.U


def test_argument_check_refuses_what_would_index_outside(host):
    d = host.dims
    w, out, auxd, consts = np.zeros((4, d.n_in, 16), np.float32), np.zeros((4, d.n_out, 16), np.float32), np.zeros(d.n_auxd), mh.model_consts(d)
    assert host.launch(0, 0, 0, 1, 15, w, out, auxd, consts) == 0
    assert host.launch(0, 0, 0, 2, 15, w, out, auxd, consts) == -2                     # more blocks than the buffers hold
    assert host.launch(0, 0, 0, 0, 15, w, out, auxd, consts) == -2 and host.launch(0, 0, 0, d.max_blocks + 1, 15, w, out, auxd, consts) == -2
    assert host.launch(0, 20, 0, 1, 15, w, out, auxd, consts) == -2 and host.launch(0, -1, 0, 1, 15, w, out, auxd, consts) == -2     # no such helper
    assert host.launch(0, mh.HELPERS['link_inertia']['id'], 3, 1, 15, w, out, auxd, consts) == -2                                  # no such link
    assert host.launch(0, 0, 0, 1, 15, w, out, auxd[:-1].copy(), consts) == -2 and host.launch(0, 0, 0, 1, 15, w, out, auxd, consts[:-1].copy()) == -2
    assert host.launch(0, 0, 0, 1, 15, w, out[:, :-1].copy(), auxd, consts) == -2
    assert host.launch(3, 0, 0, 1, 15, w, out, auxd, consts) == -1


def test_a_wrong_helper_is_reported_by_name(host):
    """the comparison is fed the twin's own answer with the damage a wrong sign, a swapped operand or a wrong branch would do: it must fail, and name the helper"""
    def answer(name, klass):
        c = [c for c in cases_of(host, name) if c.klass.startswith(klass)][0]
        return c, host.run(0, name, c)
    c, got = answer('qmul', 'exact')
    got[:, 3] = -got[:, 3]
    with pytest.raises(AssertionError, match=r'^qmul \[exact'):
        mh.check('qmul', c, got, host.dims, 'twin')
    c, got = answer('rotvec_of', 'edges: angle 0.5e-3')
    got[:, :3] *= np.float32(1 + 3e-7)           # the series cut one term short is 4e-8 relative at 1e-3; 3e-7 is two and a half ulp
    with pytest.raises(AssertionError, match=r'^rotvec_of \[edges'):
        mh.check('rotvec_of', c, got, host.dims, 'twin')
    c, got = answer('sincos_joint', 'random |x| <= 6.3')
    x = c.X[:, 0].astype(np.float64)
    got[:, 0] = np.sin(x + 2.6e-7 * np.sign(x) * (np.abs(x) > 4.7)).astype(np.float32)       # the unfused reduction's error from k = 3 on
    with pytest.raises(AssertionError, match=r'^sincos_joint \[random'):
        mh.check('sincos_joint', c, got, host.dims, 'twin')
    c, got = answer('leg_fk', 'random')
    got[:, 18:27] = got[:, 9:18]                 # R3 built from the thigh angle alone
    with pytest.raises(AssertionError, match=r'^leg_fk \[random'):
        mh.check('leg_fk', c, got, host.dims, 'twin')
    c, got = answer('terrain_sdf', 'random yaw 0.3')
    got[:, 1], got[:, 2] = got[:, 2].copy(), got[:, 1].copy()      # the normal left in the record's frame with its axes exchanged
    with pytest.raises(AssertionError, match=r'^terrain_sdf \[random'):
        mh.check('terrain_sdf', c, got, host.dims, 'twin')


def test_every_helper_is_in_the_table():
    """A plain text scan (as test_lane_prims_emul.py's): every LL_HD function defined in pmc_math.hpp and every listed member of Pmc<L> is named by an entry of
    math_helpers_common.HELPERS or by EXEMPT with its reason -- a helper added later cannot go untested silently."""
    csrc = os.path.join(mh.ROOT, 'lifelike_agility_and_play_amd', 'csrc')
    known = {n for h in mh.HELPERS.values() for n in h['names']} | set(mh.EXEMPT)
    text = open(os.path.join(csrc, 'pmc_math.hpp')).read()
    defined = set(re.findall(r'LL_HD\s+[^;{()]*?\b(operator\s*[-+]|[A-Za-z_][A-Za-z_0-9]*)\s*\(', text))
    defined = {re.sub(r'\s', '', d) for d in defined}
    assert len(defined) >= 30, sorted(defined)
    assert not defined - known, 'functions of pmc_math.hpp that no entry of math_helpers_common.HELPERS (or EXEMPT, with its reason) names: %s' % sorted(defined - known)
    step = open(os.path.join(csrc, 'pmc_step.hpp')).read()
    for m in mh.PMC_MEMBERS:
        assert re.search(r'static LL_HD [^;{]*\b%s\s*\(' % m, step), 'pmc_step.hpp no longer defines %s' % m
        assert m in known, m
    body = open(os.path.join(mh.LANES_DIR, 'math_helpers_body.hpp')).read()
    for n in known - set(mh.EXEMPT):
        assert re.search(r'(\b|operator)%s\s*(<[^<>();]*>)?\s*\(' % re.escape(n), body) or n in ('operator+', 'operator-', 'shape_sdf_rec'), 'the driver never calls %s' % n
    assert all(mh.EXEMPT.values())
