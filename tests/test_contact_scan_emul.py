"""The host twin of the step kernels' contact selections (tests/lanes/contact_scan_host.cpp: self_pick of Pmc<L>, one slot of the leg-leg pick, and the terrain-edge detectors
reverse_edge and leg_edge, compiled for the host lanes with correctly rounded IEEE operations and -ffp-contract=off) against the statement of the entry (tests/contact_scan_ref.py), bit for bit, on the input classes of
tests/contact_scan_common.py.  No GPU: the same driver is compiled for the GPU lanes and held to this twin and to the same statement in tests/test_gpu_contact_scan.py.

The statement is also shown to bite: it takes switches that make it wrong the way a kernel could be, and the wrong answer must differ from the twin's on the test's
own inputs."""
import os
import re

import numpy as np
import pytest

import contact_scan_common as sc
import contact_scan_ref as ref


@pytest.fixture(scope='module')
def host():
    h = sc.HostRunner()          # builds tests/lanes/_build/libcontact_scan_host.so when its sources are newer
    h.cases = {}
    return h


def cases_of(host, name):
    if name not in host.cases:
        host.cases[name] = sc.cases(name)
    return host.cases[name]


@pytest.mark.parametrize('name', list(sc.PICK_ENTRIES))
def test_host_twin_against_statement(host, name):
    n = 0
    for case in cases_of(host, name):
        for policy in sc.ENTRIES[name]['host']:
            who = sc.HOST_POLICIES[policy]
            got = host.run(policy, name, case)
            n += sc.check(name, case, got, who)
            sc.partial_exec_check(host, policy, name, case, got, who)
            if case.klass == 'permuted' and case.note == 'separated':
                sc.kept_set_does_not_move(name, case, got, who)
    print('%s: %d words held to the statement bit for bit over %d cases' % (name, n, len(cases_of(host, name))))


@pytest.mark.parametrize('name', list(sc.PICK_ENTRIES))
def test_input_classes(host, name):
    """every targ has every class, at least 1024 random rows with fixed seeds; a second build of the cases is the same; the four rows of a wave differ; the classes hold
    what their names promise (on the inputs alone)"""
    cs = cases_of(host, name)
    again = sc.cases(name)
    assert len(cs) == len(again) and all(a.X.tobytes() == b.X.tobytes() for a, b in zip(cs, again))
    for targ in sc.ENTRIES[name]['targs']:
        mine = [c for c in cs if c.targ == targ]
        assert sorted({c.klass for c in mine}) == sorted(sc.CLASSES) and sum(c.n for c in mine if c.klass == 'random') >= 1024
    for c in cs:
        assert c.X.shape[1] <= host.dims.n_in and c.n % 4 == 0
        assert all(c.X[i].tobytes() != c.X[j].tobytes() for i in range(4) for j in range(i)), (name, c.klass)
        K = c.targ + 1
        D = c.X[:, 0:2]
        live = D < sc.FAR
        assert ((D == sc.FAR) | (D < 1.0)).all() and (np.abs(D[live & (D != 0)]) > 2.0 ** -40).all()          # a pair or exactly 1e30; nothing near the denormals
        per = live.reshape(c.n, -1).sum(axis=1)          # pairs per row
        assert (c.X[:, 2:4] == ref.pair_codes()[None]).all()
        if c.klass == 'random':
            assert 0.4 <= live.mean() <= 0.6 and 0.05 <= (per == 0).mean() <= 0.2          # about half of the slots, and rows with have == false
        elif c.klass == 'few':
            assert (per < K).all() if c.note == 'fewer' else not live.any()
            assert c.note == 'none' or all((per == k).any() for k in range(K))
        elif c.klass == 'signs':
            assert ((D == 0) & np.signbit(D)).any() and ((D == 0) & ~np.signbit(D)).any() and (D[live] < 0).any()
            thr0 = (D.reshape(c.n, -1).min(axis=1) + sc.SELECT_EPS).astype(np.float32) == 0
            assert thr0.any() and ((D.reshape(c.n, -1) == 0).any(axis=1) & thr0).any()          # rows whose threshold is exactly 0, with zeros on it
        elif c.klass == 'threshold':
            assert (per == int(c.note.split()[1]) + 4).all()
        elif c.klass == 'ties':
            d = np.sort(D.reshape(c.n, -1), axis=1)
            assert (d[:, 0] == d[:, 1]).mean() > 0.5          # the closest depth held by more than one pair


def test_threshold_class_sits_on_the_threshold(host):
    """per slot r: in slot r of the rule's own run the pairs left hold one exactly at float32(closest + eps), its float32 neighbour above and the one below; the pair at
    the threshold has the lowest pair index among those within it in a good share of the rows, and not in another"""
    for name in sc.PICK_ENTRIES:
        for c in cases_of(host, name):
            if c.klass != 'threshold':
                continue
            r = int(c.note.split()[1])
            flat = c.X[:, 0:2].reshape(c.n, 32)
            d = np.sort(flat, axis=1)
            # the r closer ones go first (each alone within its own tolerance: they are 1e-3 apart), then the closest of slot r is d[:, r]
            assert (np.diff(d[:, :r + 1], axis=1) > 5e-4).all()
            t = (d[:, r] + sc.SELECT_EPS).astype(np.float32)
            assert (d[:, r + 1] == np.nextafter(t, np.float32(-np.inf))).all() and (d[:, r + 2] == t).all() and (d[:, r + 3] == np.nextafter(t, np.float32(np.inf))).all()
            assert (d[:, r + 4:] == sc.FAR).all()
            code = ref.pair_codes().reshape(32)
            within = (flat >= d[:, r:r + 1]) & (flat <= t[:, None])
            at_thr_wins = np.where(within, code, 99).min(axis=1) == np.where(flat == t[:, None], code, 99).min(axis=1)
            assert 0.15 <= at_thr_wins.mean() <= 0.6, at_thr_wins.mean()


WRONG = [('self_pick', 'highest_index'), ('self_pick', 'strict')]


@pytest.mark.parametrize('name,switch', WRONG)
def test_a_wrong_statement_differs_from_the_twin(host, name, switch):
    """a bit-exact entry: the statement made wrong by `switch` must differ from the twin's answer -- for every targ, in the class built for it (the threshold class for `<`,
    the tie classes for the index rule) and, for the index rule, in the random class too"""
    for targ in sc.ENTRIES[name]['targs']:
        K = targ + 1
        for klass in {'strict': ['threshold'], 'highest_index': ['ties', 'threshold', 'random']}[switch]:
            hit = 0
            for case in [c for c in cases_of(host, name) if c.targ == targ and c.klass == klass]:
                if klass == 'threshold' and int(case.note.split()[1]) >= K:
                    continue                # that slot is not run
                got = host.run(0, name, case)[:, :sc.words_of(name, case)]
                bad = sc.statement(name, case, **{switch: True})[:, :sc.words_of(name, case)]
                differs = ~sc.bits_equal(got, np.nan_to_num(bad).astype(np.float32)) & ~np.isnan(bad)
                assert differs.any(), (name, switch, targ, klass, case.note)
                hit += int(differs.any(axis=(1, 2)).sum())
            assert hit
            print('%s targ %d, %s: the wrong statement differs from the twin in %d rows of the %s class' % (name, targ, switch, hit, klass))


def test_argument_check_refuses_what_would_index_outside(host):
    d = host.dims
    w, out, consts = np.zeros((4, d.n_in, 16), np.float32), np.zeros((4, d.n_out, 16), np.float32), d.consts
    assert host.launch(0, 0, 0, 1, 15, w, out, consts) == 0
    assert host.launch(0, 0, 0, 2, 15, w, out, consts) == -2                     # more blocks than the buffers hold
    assert host.launch(0, 0, 0, 0, 15, w, out, consts) == -2 and host.launch(0, 0, 0, d.max_blocks + 1, 15, w, out, consts) == -2
    assert host.launch(0, d.n_entries, 0, 1, 15, w, out, consts) == -2 and host.launch(0, -1, 0, 1, 15, w, out, consts) == -2       # no such entry
    assert host.launch(0, sc.ENTRIES['self_pick']['id'], 2, 1, 15, w, out, consts) == -2 and host.launch(0, 0, -1, 1, 15, w, out, consts) == -2
    assert host.launch(0, 0, 0, 1, 15, w, out, consts[:-1].copy()) == -2 and host.launch(0, 0, 0, 1, 15, w[:, :-1].copy(), out, consts) == -2
    assert host.launch(0, 0, 0, 1, 15, w, out[:, :-1].copy(), consts) == -2
    assert host.launch(1, 0, 0, 1, 15, w, out, consts) == -1 and host.launch(-1, 0, 0, 1, 15, w, out, consts) == -1


def test_a_wrong_entry_is_reported_by_name(host):
    """the comparison is fed the twin's own answer with the damage a wrong tie rule, a pair left uncleared or a leak between rows would do: it must fail, and name the entry"""
    def answer(name, klass, targ, note=None):
        c = [c for c in cases_of(host, name) if c.klass == klass and c.targ == targ and (note is None or c.note == note)][0]
        return c, host.run(0, name, c)
    c, got = answer('self_pick', 'random', 1)
    got[:, sc.PICK_WORDS + 2] = got[:, 2]                                        # the second slot reporting the first's depth
    with pytest.raises(AssertionError, match=r'^self_pick \[random, targ 1'):
        sc.check('self_pick', c, got, 'twin')
    c, got = answer('self_pick', 'ties', 0)
    got[:, 9:11] = c.X[:, 0:2]                                                   # the winner not cleared
    with pytest.raises(AssertionError, match=r'^self_pick \[ties, targ 0'):
        sc.check('self_pick', c, got, 'twin')
    c, got = answer('self_pick', 'signs', 0)
    got[:, 2] = np.where(got[:, 2] == 0, -got[:, 2], got[:, 2])                    # a zero depth with the other sign
    with pytest.raises(AssertionError, match=r'^self_pick \[signs, targ 0'):
        sc.check('self_pick', c, got, 'twin')
    c, got = answer('self_pick', 'random', 0)
    got[1] = got[0]                                                              # a row answering with its neighbour's data
    with pytest.raises(AssertionError, match=r'^self_pick \[random, targ 0'):
        sc.check('self_pick', c, got, 'twin')
    c, got = answer('self_pick', 'few', 0, 'none')
    got[:, 0] = 1.0                                                              # have without a pair
    with pytest.raises(AssertionError, match=r'^self_pick \[few: none, targ 0'):
        sc.check('self_pick', c, got, 'twin')
    c, got = answer('self_pick', 'permuted', 1, 'separated')
    got[3, 2] = got[3, sc.PICK_WORDS + 2]                                        # one arrangement picking another pair
    with pytest.raises(AssertionError, match=r'^self_pick \[permuted: separated.*kept set moved'):
        sc.kept_set_does_not_move('self_pick', c, got, 'twin')
    c, got = answer('self_pick', 'ties', 0)
    got[2] = np.nan                                                              # a row that did not answer
    with pytest.raises(AssertionError, match=r'^self_pick \[ties'):
        sc.check('self_pick', c, got, 'twin')


def test_pair_codes_are_the_kernels():
    """the pair indices the self_pick inputs carry are the ones substep_impl forms (a plain text scan for the expressions), and all 32 of a row differ"""
    step = open(os.path.join(sc.ROOT, 'lifelike_agility_and_play_amd', 'csrc', 'pmc_step.hpp')).read()
    assert 'lm::sel(legf < 0.5f, ln.lane_f(3.0f), legf - one) : legf + ln.lane_f(4.0f)' in step and 'lm::sel(own_s, one, zero) + lm::sel(oth_s, ln.lane_f(2.0f), zero)' in step
    assert 'cpair[pass] = lp * 4.0f + sp;' in step
    codes = ref.pair_codes()
    assert sorted(codes.reshape(-1).tolist()) == list(range(32))
    assert codes[0].tolist() == [12, 13, 14, 15, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11] and codes[1][:8].tolist() == [16, 18, 17, 19, 20, 22, 21, 23]


def test_every_member_is_in_the_table():
    """A plain text scan (function names only, as test_solver_rows_emul.py's): every member of Pmc<L> this layer is asked to hold is defined in pmc_step.hpp, named by an
    entry of contact_scan_common.ENTRIES and called by the driver body -- and by substep_impl, which must not carry a second copy of the text; what is left for a later
    layer is listed with its reason, and is still there to be left."""
    import solver_rows_common as sr
    step = open(os.path.join(sc.ROOT, 'lifelike_agility_and_play_amd', 'csrc', 'pmc_step.hpp')).read()
    body = open(os.path.join(sc.LANES_DIR, 'contact_scan_body.hpp')).read()
    named = {n for h in sc.ENTRIES.values() for n in h['names']}
    sub = step[step.index('void substep_impl('):]
    for m in sc.PMC_MEMBERS:
        assert re.search(r'static LL_HD [^;{]*\b%s\s*\(' % m, step), 'pmc_step.hpp no longer defines %s' % m
        assert m in named, 'no entry names %s' % m
        assert re.search(r'K::(template )?%s\s*(<[^<>();]*>)?\s*\(' % m, body), 'the driver never calls %s' % m
        assert re.search(r'\b%s\s*(<[^<>();]*>)?\s*\(ln,' % m, sub), 'substep_impl no longer calls %s' % m
    for m in sc.CALLED_THROUGH:
        assert re.search(r'K::(template )?%s\s*\(' % m, body), 'the driver never calls %s' % m
    assert named <= set(sc.PMC_MEMBERS) | sc.CALLED_THROUGH
    assert 'L::rmin(code)' not in sub and 'L::rmin(code)' in step          # the pick's text lives in the member alone
    for m, why in sc.LATER.items():
        assert why and m not in named
    assert not set(sc.LATER) & set(sc.PMC_MEMBERS) and not (set(sc.PMC_MEMBERS) & set(sr.LATER)) and not ({'leg_edge', 'reverse_edge'} & set(sr.LATER))


# ---- the terrain-edge detectors -----------------------------------------------------------------------------------------------------------------------------
def edge_cases_of(host, name):
    key = 'edge:' + name
    if key not in host.cases:
        host.cases[key] = sc.edge_cases(name)
    return host.cases[key]


@pytest.mark.parametrize('name', list(sc.EDGE_ENTRIES))
def test_edge_twin_against_statement(host, name):
    """reverse_edge and leg_edge on the host lanes against the float64 statement: the exact class, the random class and every edge case (contact_scan_common.check_edge says
    what is held bit for bit and what within the twin's own forward bound); every case also under a partial EXEC"""
    for case in edge_cases_of(host, name):
        got = host.run(0, name, case)
        r = sc.check_edge(name, case, got, 'HostLanes', host.dims)
        print('%-13s %-7s %-26s worst |twin - statement| %.3e, worst error / bound %.3f, not sure %.4f' % (name, case.klass, case.note or '', r['err'].max(), r['ratio'], r['unsure']))
        sc.partial_exec_check(host, 0, name, case, got, 'HostLanes')


@pytest.mark.parametrize('name', list(sc.EDGE_ENTRIES))
def test_edge_input_classes(host, name):
    """on the statement alone: at most 5 % of the random samples are left out of the decision comparison and at least 30 % lie within the contact margin; the cases are
    reproducible, every row of a wave differs, and the edge cases are what their names say"""
    cs, again = edge_cases_of(host, name), sc.edge_cases(name)
    assert [c.klass for c in cs] == ['exact', 'random'] + ['edges'] * len(sc.EDGE_NOTES) and all(a.X.tobytes() == b.X.tobytes() for a, b in zip(cs, again))
    for c in cs:
        v, e, sure, hit = sc.edge_want(name, c, host.dims)
        assert c.X.shape[1] <= host.dims.n_in and c.n % 4 == 0
        assert all(c.X[i].tobytes() != c.X[j].tobytes() for i in range(4) for j in range(i)) or c.note in ('n_shapes = 0',), (name, c.klass, c.note)
        found = v[:, 0] < 1.0
        if c.klass == 'random':
            assert c.n >= 1024 and 1 - sure.mean() <= sc.MAX_UNSURE and (hit & sure).mean() >= sc.MIN_HIT, (name, 1 - sure.mean(), hit.mean())
            assert (c.X[:, 12, 0] == 0).any() and (c.X[:, 28:72:8, 0] > 0.05).any()          # rows without a box, floating boxes among them
        elif c.klass == 'exact':
            grid = 4 if name == 'reverse_edge' else 16          # quarters; sixteenths where the edges have to run across the leg boxes
            assert (c.X[:, 0:3] * 4 == np.round(c.X[:, 0:3] * 4)).all() and (c.X[:, 24:72] * grid == np.round(c.X[:, 24:72] * grid)).all() and np.isin(c.X[:, 3:12], [0, 1, -1]).all()
            assert 0.1 < found.mean() < 0.8 and found.any(axis=1).mean() > 0.4
        elif c.note in ('wholly outside', 'n_shapes = 0', 'a box nobody is near'):
            assert not found.any() and (v[:, 4:7] == np.array([0, 0, 1])[None, :, None]).all()
        else:                               # every other case finds something, in every row that is meant to -- for leg_edge as for reverse_edge
            per_row = found.any(axis=1)
            assert per_row.all() if c.note != 'a box only near' else (per_row[0::4].all() and not per_row[1::4].any() and not per_row[2::4].any() and not per_row[3::4].any()), (name, c.note)
            assert hit.any(), (name, c.note)
            if name == 'leg_edge':
                assert (v[:, 7][found] >= 2).all() and (v[:, 8][found] == 0).all()          # a leg link and the listed box
            if c.note == 'parallel to a box axis':          # quarter turns: the edge does not move along two of the box's axes (the 1e-9 guard on both)
                assert np.isin(c.X[:, 3:12], [0, 1, -1]).all() and (c.X[:, 18:21] == 0).all()
            if c.note == 'a floating box':
                assert (c.X[:, 28, 0] > 0.05).all()
                top = sc.edge_want(name, c, host.dims, top_edge_of_floating=True)[0]
                assert not (top[:, 0] < sc.ref.MARGIN).any()          # its top edges reach nothing: what is found is found on the bottom edges
            if c.note == 'a yawed arena':
                assert (c.X[:, 13, 0] == 1).all() and (c.X[:, 17, 0] != 0).any()
                plain = c.X.copy()
                plain[:, 13] = 0
                assert (ref.terrain_edge(name, plain, host.dims.legc, host.dims.basec)[0][:, :4] != v[:, :4]).any()          # the turn matters
            if c.note == 'the two ends at equal depth' and name == 'leg_edge':          # (reverse_edge takes the end it is told) the choice between them matters (another point), and it is the first
                swapped = sc.edge_want(name, c, host.dims, ends_swapped=True)[0]
                assert (np.abs(swapped[:, 0][found] - v[:, 0][found]) <= ref.TIE).all() and (swapped[:, 1:4] != v[:, 1:4]).any(axis=1)[found].mean() > 0.5
            if c.note == 'two boxes at equal depth':
                first, second = c.X.copy(), c.X.copy()
                first[:, 12], second[:, 12], second[:, 24:32] = 1, 1, c.X[:, 32:40]
                v1, v2 = (ref.terrain_edge(name, x, host.dims.legc, host.dims.basec)[0] for x in (first, second))
                tie = (v1[:, 0] < 1.0) & (v2[:, 0] == v1[:, 0])          # reverse_edge: the two boxes continue one another along the x edges, the same depth, another piece
                assert tie.any() and (name == 'leg_edge' or (v1[:, 1:4] != v2[:, 1:4]).any(axis=1)[tie].any())
                assert (v[:, :7] == v1[:, :7]).transpose(0, 2, 1)[tie].all()          # the first listed wins (leg_edge: shape 0, asserted above)


WRONG_EDGE = [('reverse_edge', 'top_edge_of_floating'), ('leg_edge', 'top_edge_of_floating'), ('leg_edge', 'parallel_axis_allowed'), ('reverse_edge', 'ends_swapped'),
              ('leg_edge', 'ends_swapped')]


@pytest.mark.parametrize('name,switch', WRONG_EDGE)
def test_a_wrong_edge_statement_is_ten_bars_away(host, name, switch):
    """on the random class the statement made wrong by `switch` sits at least ten bars from the twin in depth or point, on sure samples within the margin"""
    case = [c for c in edge_cases_of(host, name) if c.klass == 'random'][0]
    v, e, sure, hit = sc.edge_want(name, case, host.dims)
    bad = sc.edge_want(name, case, host.dims, **{switch: True})[0]
    got = host.run(0, name, case)[:, :4].astype(np.float64)
    ok = np.broadcast_to((sure & hit)[:, None, :], got.shape)
    with np.errstate(invalid='ignore', divide='ignore'):
        away = np.where(ok, np.abs(bad[:, :4] - got) / e[:, :4], 0.0)
    n = int((away.max(axis=1) >= 10.0).sum())
    print('%s, %s: the wrong statement is ten bars or more from the twin on %d samples (worst %.3g bars)' % (name, switch, n, away.max()))
    assert n >= 16, (name, switch, n)
