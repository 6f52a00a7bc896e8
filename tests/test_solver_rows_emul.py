"""The host twin of the step kernels' row builders and sweeps (tests/lanes/solver_rows_host.cpp: permute4, finish_row, cross_gram, gs_round, gs_cone_round, contact_row and
contact_rows_cone_piped of Pmc<L>, and their composition from the contact geometry to the velocity change, compiled for the host lanes with correctly rounded IEEE operations and -ffp-contract=off) one entry at a time against the float64
statement of that entry (tests/solver_rows_ref.py), on the exact, random and edge inputs of tests/solver_rows_common.py and under its class table.  No GPU: the same driver
is compiled for the GPU lanes and held to this twin's error and to the same statements in tests/test_gpu_solver_rows.py.

The statements are also shown to bite: each takes switches that make it wrong the way a kernel could be, and the wrong answer must sit at least ten bars away."""
import os
import re

import numpy as np
import pytest

import lane_prims_ref
import solver_rows_common as sc
import solver_rows_ref as ref


@pytest.fixture(scope='module')
def host():
    h = sc.HostRunner()          # builds tests/lanes/_build/libsolver_rows_host.so when its sources are newer
    h.cases = {}
    return h


def cases_of(host, name):
    if name not in host.cases:
        host.cases[name] = sc.cases(name, host.dims)
    return host.cases[name]


@pytest.mark.parametrize('name', list(sc.ENTRIES))
def test_host_twin_against_statement(host, name):
    for case in cases_of(host, name):
        for policy in sc.ENTRIES[name]['host']:
            who = sc.HOST_POLICIES[policy]
            got = host.run(policy, name, case)
            r = sc.check(name, case, got, who)
            print('%-20s %-18s %-8s %-18s targ %d worst |twin - statement| %.3e, worst error / bound %.3f' % (name, who, case.klass, case.note or '', case.targ, r['err'].max(), r['ratio']))
            sc.partial_exec_check(host, policy, name, case, got, who)
            if name == 'pair_row':
                sc.arena_rows_agree(case, got, who)
            if name in ('self_row', 'pair_row'):
                sc.cleared_row_changes_nothing(name, case, got, who)


def test_piped_contact_rows_are_the_plain_ones(host):
    """contact_rows_cone_piped against contact_row x 3 + cross_gram x 2 on the same inputs: coefficients, c and inv bit for bit"""
    for plain, piped in zip(cases_of(host, 'contact_rows'), cases_of(host, 'contact_rows_piped')):
        assert plain.X.tobytes() == piped.X.tobytes()
        sc.piped_against_plain(piped, host.run(2, 'contact_rows_piped', piped), host.run(2, 'contact_rows', plain), sc.HOST_POLICIES[2])


@pytest.mark.parametrize('name', list(sc.ENTRIES))
def test_input_classes(host, name):
    """every entry has its exact class and at least 1024 random rows with fixed seeds; a second build of the cases is the same; the four rows of a wave differ; on the exact
    and edge classes every intermediate of the statement is a float32 with room to spare (so no association or contraction can matter); the random rows mix live and dead
    lanes as the issue of this layer asks"""
    cs = cases_of(host, name)
    for targ in sc.ENTRIES[name]['targs']:
        mine = [c for c in cs if c.targ == targ]
        assert mine[0].klass == 'exact' and sum(c.n for c in mine if c.klass == 'random') >= 1024
    again = sc.cases(name, host.dims)
    assert len(again) == len(cs) and all(a.X.tobytes() == b.X.tobytes() for a, b in zip(cs, again))
    for c in cs:
        assert c.X.shape[1] <= host.dims.n_in and c.n % 4 == 0
        assert all(c.X[i].tobytes() != c.X[j].tobytes() for i in range(4) for j in range(i)), (name, c.klass)
        w = sc.want(name, c)
        if c.klass != 'random':
            for t in w['trace'] + [np.nan_to_num(w['v'])]:
                assert (t == t.astype(np.float32)).all() and np.abs(t).max() < 2.0 ** 16 and (t * 2.0 ** 6 == np.round(t * 2.0 ** 6)).all(), (name, c.klass, c.note)
        elif sc.ENTRIES[name]['stmt'] in ('gs_round', 'gs_cone_round'):
            inv = c.X[:, sc.ROW_INV]
            dead = inv == 0
            assert 0.15 <= dead.mean() <= 0.40, dead.mean()
            assert dead.all(axis=1).any() and (dead.reshape(-1, 4, 4).all(axis=2).sum(axis=1) == 1).any()
        if c.klass == 'random':
            assert (np.abs(c.X[np.isfinite(c.X) & (c.X != 0)]) > 2.0 ** -40).all()          # nothing near the denormals goes in


@pytest.mark.parametrize('name', list(sc.ENTRIES))
def test_model_states_what_the_statement_states(host, name):
    """the bound models follow the kernel's form (pending increments moved by Gram scalars); their VALUES must be the dense statements' (so a bound is a bound on the right thing)"""
    for case in cases_of(host, name):
        w = sc.want(name, case)
        v, m = w['v'], w['model_v']
        assert (np.isnan(v) == np.isnan(m)).all()
        ok = ~np.isnan(v)
        assert np.abs(v - m)[ok].max() <= 1e-12 * max(1.0, np.abs(v[ok]).max()), (name, case.klass, np.abs(v - m)[ok].max())
        assert (w['twin'][ok] >= w['madd'][ok]).all() and (w['madd'][ok] >= 0).all()


def test_turn_order_is_the_one_of_turns8():
    """solver_rows_ref.turn_order against lane_prims_ref's statement of turns8 (H_ = 0, then H_ = 1): with every coupling 1 and wide bounds each turn commits more than
    the one before, so the committed increments sort the lanes by their turn"""
    class C:
        pass
    order = []
    for h in (0, 1):
        c = C()
        c.targ = h
        c.w = np.zeros((4, 80, 16))
        c.w[:, 0], c.w[:, 2], c.w[:, 3], c.w[:, 4:20] = 1.0, -1e30, 1e30, 1.0
        c.aux = np.zeros((4, 1))
        r = lane_prims_ref.Res(c)
        lane_prims_ref.turns8(c, r)
        dl = r.out[1][0]
        took = np.flatnonzero(dl > 0)
        order += list(took[np.argsort(dl[took])])
    assert order == ref.turn_order() and order[:12] == ref.turn_order(limit=True)
    assert ref.turn_order(limit=True, limit_takes_sub3=True) == ref.turn_order() and ref.turn_order(leg_major=True) == list(range(16))


WRONG = [('finish_row', 0, 'no_joint_part'), ('finish_row', 0, 'plus_inv'), ('finish_row', 1, 'no_joint_part'), ('cross_gram', 0, 'no_joint_part'), ('cross_gram', 0, 'plus_inv'),
         ('contact_rows', 0, 'no_joint_part'), ('contact_rows', 0, 'plus_inv'),
         ('gs_round', 0, 'leg_major'), ('gs_round', 1, 'leg_major'), ('gs_round', 2, 'leg_major'), ('gs_round', 0, 'limit_takes_sub3'),
         ('gs_round', 0, 'lower_bound_at_minus_hi'), ('gs_round', 1, 'lower_bound_at_minus_hi'), ('gs_cone_round', 0, 'leg_major'), ('gs_cone_round', 0, 'stale_velocity'),
         ('self_row', 0, 'no_apply_factors'), ('self_row', 1, 'no_apply_factors'), ('pair_row', 0, 'no_apply_factors'), ('pair_row', 1, 'no_apply_factors'), ('self_pieces', 2, 'no_apply_factors')]
# 'pair shares added in me order' has no wrong form to state: the shares are two, and a + b == b + a in IEEE arithmetic, bit for bit.  What the fixed order protects -- both
# rows of an arena holding the same bits of c, inv and lam -- is asserted directly instead (solver_rows_common.arena_rows_agree), and shown to bite below.


@pytest.mark.parametrize('name,targ,switch', WRONG)
def test_a_wrong_statement_is_ten_bars_away(host, name, targ, switch):
    """on the random class the statement made wrong by `switch` differs from the right one by at least 10 x the bar of that word, in every word the switch can reach"""
    case = [c for c in cases_of(host, name) if c.klass == 'random' and c.targ == targ][0]
    w = sc.want(name, case)
    bad, _ = sc.statement(name, case, **{switch: True})
    if switch == 'lower_bound_at_minus_hi':          # the unilateral rounds are handed hi = 3e38: a lower bound there is no bound at all -- the natural wrong form of this switch
        assert (case.X[:, 29] == np.float32(ref.BIG)).all()
    ok = ~np.isnan(w['v'])
    with np.errstate(invalid='ignore', divide='ignore'):
        away = np.where(ok & (bad != w['v']), np.abs(bad - w['v']) / w['twin'], 0.0).max(axis=(0, 2))
    base_words = [4, 5] if name == 'self_pieces' else [8, 9]          # self_row_apply's 4 x / 8 x factors act on VA and VB
    reach = {'no_apply_factors': lambda k: k in base_words, 'no_joint_part': lambda k: k % sc.RW >= sc.ROW_NK if name != 'cross_gram' and k < 3 * sc.RW else True, 'plus_inv': lambda k: k % sc.RW >= sc.ROW_NK if name != 'cross_gram' and k < 3 * sc.RW else True}
    words = [k for k in range(sc.ENTRIES[name]['words']) if ok[:, k].any() and reach.get(switch, lambda k: True)(k)]
    assert words
    print('%s targ %d, %s: the wrong statement is %s bars away (least over the words it reaches)' % (name, targ, switch, '%.3g' % min(away[k] for k in words)))
    for k in words:
        assert away[k] >= 10.0, (name, switch, k, away[k])


def test_argument_check_refuses_what_would_index_outside(host):
    d = host.dims
    w, out, consts = np.zeros((4, d.n_in, 16), np.float32), np.zeros((4, d.n_out, 16), np.float32), d.consts
    assert host.launch(0, 0, 0, 1, 15, w, out, consts) == 0
    assert host.launch(0, 0, 0, 2, 15, w, out, consts) == -2                     # more blocks than the buffers hold
    assert host.launch(0, 0, 0, 0, 15, w, out, consts) == -2 and host.launch(0, 0, 0, d.max_blocks + 1, 15, w, out, consts) == -2
    assert host.launch(0, d.n_entries, 0, 1, 15, w, out, consts) == -2 and host.launch(0, -1, 0, 1, 15, w, out, consts) == -2       # no such entry
    assert host.launch(0, sc.ENTRIES['gs_round']['id'], 3, 1, 15, w, out, consts) == -2 and host.launch(0, sc.ENTRIES['permute4']['id'], 1, 1, 15, w, out, consts) == -2
    assert host.launch(0, sc.ENTRIES['contact_rows_piped']['id'], 1, 1, 15, w, out, consts) == -2 and host.launch(2, sc.ENTRIES['contact_rows_piped']['id'], 1, 1, 15, w, out, consts) == 0
    assert host.launch(0, 0, 0, 1, 15, w, out, consts[:-1].copy()) == -2 and host.launch(0, 0, 0, 1, 15, w[:, :-1].copy(), out, consts) == -2
    assert host.launch(0, 0, 0, 1, 15, w, out[:, :-1].copy(), consts) == -2
    assert host.launch(3, 0, 0, 1, 15, w, out, consts) == -1 and host.launch(-1, 0, 0, 1, 15, w, out, consts) == -1


def test_a_wrong_entry_is_reported_by_name(host):
    """the comparison is fed the twin's own answer with the damage a wrong sign, a wrong leg, a wrong turn or a wrong bound would do: it must fail, and name the entry"""
    def answer(name, klass, targ=0):
        c = [c for c in cases_of(host, name) if c.klass == klass and c.targ == targ][0]
        return c, host.run(0 if name != 'contact_rows_piped' else 2, name, c)
    c, got = answer('finish_row', 'exact')
    got[:, sc.ROW_NK:] = -got[:, sc.ROW_NK:]                                   # + inv
    with pytest.raises(AssertionError, match=r'^finish_row \[exact'):
        sc.check('finish_row', c, got, 'twin')
    c, got = answer('finish_row', 'random', 1)
    got[:, 0], got[:, 1] = got[:, 1].copy(), got[:, 0].copy()                    # ca[0] and ca[1] exchanged
    with pytest.raises(AssertionError, match=r'^finish_row \[random.*a move'):
        sc.check('finish_row', c, got, 'twin')
    c, got = answer('finish_row', 'random', 1)
    got[:, sc.ROW_NK + 3] = 0.0                                                  # LIMIT forming the scalar of lane 3
    with pytest.raises(AssertionError, match=r'^finish_row \[random.*does not form'):
        sc.check('finish_row', c, got, 'twin')
    c, got = answer('cross_gram', 'random')
    got[:, 4:8] = got[:, 0:4]                                                    # the joint part added for the wrong leg
    with pytest.raises(AssertionError, match=r'^cross_gram \[random'):
        sc.check('cross_gram', c, got, 'twin')
    c, got = answer('gs_round', 'random', 1)
    got[:, 0] = np.where(np.arange(16) == 5, got[:, 0] * np.float32(1 + 1e-4), got[:, 0])      # one lane's multiplier a ten-thousandth off
    with pytest.raises(AssertionError, match=r'^gs_round \[random, targ 1'):
        sc.check('gs_round', c, got, 'twin')
    c, got = answer('gs_round', 'edges', 0)
    got[:, 0, 3] = 0.25                                                          # sub-lane 3 of a limit round committing something
    with pytest.raises(AssertionError, match=r'^gs_round \[edges: all dead, targ 0'):
        sc.check('gs_round', c, got, 'twin')
    c, got = answer('gs_cone_round', 'random')
    got[:, 0], got[:, 1] = got[:, 1].copy(), got[:, 0].copy()                    # the two rows of a pair exchanged
    with pytest.raises(AssertionError, match=r'^gs_cone_round \[random'):
        sc.check('gs_cone_round', c, got, 'twin')
    c, got = answer('contact_rows_piped', 'random', 1)
    got[:, 87:103], got[:, 103:119] = got[:, 103:119].copy(), got[:, 87:103].copy()      # n12 and n21 exchanged
    with pytest.raises(AssertionError, match=r'^contact_rows_piped \[random'):
        sc.check('contact_rows_piped', c, got, 'twin')
    c, got = answer('compose', 'random', 1)
    got[:, 9] = got[:, 9] * np.float32(1.01)                                    # the hip joint's velocity change one per cent off (a forward bound carried through two
                                                                                # coupled rounds is wide: this entry catches what is consistently wrong, the entries above what is slightly wrong)
    with pytest.raises(AssertionError, match=r'^compose \[random, targ 1'):
        sc.check('compose', c, got, 'twin')
    c, got = answer('clip_velocities', 'edges')
    got[:, :9] = np.where(np.isnan(got[:, :9]), c.X[:, 9:10], got[:, :9])          # an infinity or a NaN coming out as the bound
    with pytest.raises(AssertionError, match=r'^clip_velocities \[edges.*did not come out NaN'):
        sc.check('clip_velocities', c, got, 'twin')
    c, got = answer('pd', 'edges')
    got[1::2, 3:6] = np.clip(got[1::2, 3:6], -c.X[1::2, 11:12], c.X[1::2, 11:12])       # the max_tau argument ignored
    assert (c.X[1::2, 12] > 0).all() and (c.X[0::2, 12] == 0).all()
    with pytest.raises(AssertionError, match=r'^pd \[edges'):
        sc.check('pd', c, got, 'twin')
    c, got = answer('pick_rank', 'random', 2)
    got[:, 0] = c.X[:, 2][:, (np.arange(16) & ~3) | 2]                                  # taken whatever the rank says
    with pytest.raises(AssertionError, match=r'^pick_rank \[random, targ 2'):
        sc.check('pick_rank', c, got, 'twin')
    c, got = answer('pair_row', 'random', 0)
    got[1::2, 3] = np.nextafter(got[1::2, 3], np.float32(np.inf))                        # robot 1 summing its own share first, one ulp away
    with pytest.raises(AssertionError, match=r'^pair_row \[random.*c differs between the two rows of arena'):
        sc.arena_rows_agree(c, got, 'twin')
    c, got = answer('self_row', 'edges', 0)
    got[:, 8] = got[:, 8] + np.float32(0.25)                                            # a turn on a cleared row moving the velocity
    with pytest.raises(AssertionError, match=r'^self_row \[edges.*cleared row changed'):
        sc.cleared_row_changes_nothing('self_row', c, got, 'twin')
    c, got = answer('self_row', 'random', 0)
    got[:, 8] = c.X[:, 73] + (got[:, 8] - c.X[:, 73]) * np.float32(0.25)                 # self_row_apply without its 4 x
    with pytest.raises(AssertionError, match=r'^self_row \[random'):
        sc.check('self_row', c, got, 'twin')
    c, got = answer('cand_eval_point', 'random')
    got[:, 2] = got[:, 2] - got[:, 3]                                                    # a sphere tested at its lowest point instead of its centre
    with pytest.raises(AssertionError, match=r'^cand_eval_point \[random'):
        sc.check('cand_eval_point', c, got, 'twin')
    c, got = answer('gs_round', 'exact', 2)
    got[1] = np.nan                                                              # a row that did not answer
    with pytest.raises(AssertionError, match=r'^gs_round \[exact'):
        sc.check('gs_round', c, got, 'twin')


def test_every_member_is_in_the_table():
    """A plain text scan (function names only, as test_math_helpers_emul.py's): every member of Pmc<L> this layer is asked to hold is still defined in pmc_step.hpp, named
    by an entry of solver_rows_common.ENTRIES and called by the driver body; what is left for a later layer is listed with its reason, and is still there to be left."""
    step = open(os.path.join(sc.ROOT, 'lifelike_agility_and_play_amd', 'csrc', 'pmc_step.hpp')).read()
    body = open(os.path.join(sc.LANES_DIR, 'solver_rows_body.hpp')).read()
    named = {n for h in sc.ENTRIES.values() for n in h['names']}
    called_through = {'row_coeffs', 'neg_scaled', 'joint_part', 'gram_finish', 'row_perm_a', 'row_perm_b'}        # the pieces of contact_rows_cone_piped, which calls each
    for m in sc.PMC_MEMBERS:
        assert re.search(r'static LL_HD [^;{]*\b%s\s*\(' % m, step), 'pmc_step.hpp no longer defines %s' % m
        assert m in named, 'no entry names %s' % m
        if m in called_through:
            piped = step[step.index('static LL_HD void contact_rows_cone_piped'):]
            assert re.search(r'\b%s\s*\(' % m, piped[:piped.index('static LL_HD void pd_torque')]), 'contact_rows_cone_piped no longer calls %s' % m
        else:
            assert re.search(r'K::(template )?%s\s*(<[^<>();]*>)?\s*\(' % m, body), 'the driver never calls %s' % m
    assert named <= set(sc.PMC_MEMBERS)
    for m, why in sc.LATER.items():
        assert why and m not in named
        assert re.search(r'\b%s\s*\(' % m, step), 'pmc_step.hpp no longer has %s: take it off the list' % m
    for inst in ('gs_round<true, true>', 'gs_round<false, true>', 'gs_round<false, false>', 'finish_row<true>', 'finish_row<false>'):
        assert inst in body and inst in step, inst
