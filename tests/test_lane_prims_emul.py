"""The host twin of the GPU lanes (tests/emul/lanes_host.hpp HostLanes) one primitive at a time against the float64 statement of that primitive
(tests/lane_prims_ref.py), on the exact, random and edge inputs of tests/lane_prims_common.py and under its class table.  No GPU: the same driver
(tests/lanes/lane_prims_body.hpp) is compiled for the GPU lanes and held to this twin and to the same statement in tests/test_gpu_lane_prims.py."""
import os
import re

import numpy as np
import pytest

import lane_prims_common as lp
import lane_prims_ref as ref


@pytest.fixture(scope='module')
def host():
    return lp.HostRunner()          # builds tests/lanes/_build/liblane_prims_host.so when its sources are newer


@pytest.mark.parametrize('name', list(lp.PRIMS))
def test_host_twin_against_statement(host, name):
    for policy in lp.host_policies(name):
        worst, _ = lp.hold_to_statement(host, policy, name, lp.HOST_POLICIES[policy], host_statement=True)
        print('%-20s %-30s worst error / bound on random inputs: %.3f' % (name, lp.HOST_POLICIES[policy], worst))


@pytest.mark.parametrize('name', list(lp.PRIMS))
def test_exact_inputs_are_exact_in_the_statement(host, name):
    """What the exact and edge classes rest on: every float64 intermediate of the statement is a float32 (so no association, fused or not, can round)."""
    for klass in ('exact', 'edges'):
        for c in lp.cases(name, klass, host.dims):
            for x in ref.run(lp.PRIMS[name]['ref'], c).trace:
                with np.errstate(invalid='ignore', over='ignore'):
                    back = x.astype(np.float32).astype(np.float64)
                assert ((back == x) | (np.isnan(back) & np.isnan(x))).all(), '%s [%s, targ %d]: an intermediate of the statement is no float32' % (name, klass, c.targ)
                assert (np.abs(x[np.isfinite(x)]) < 2.0 ** 24).all()


def test_rows_of_a_wave_get_different_data(host):
    for name in lp.PRIMS:
        for klass, c in lp.all_cases(name, host.dims):
            if c.w.any():
                assert len({c.w[r].tobytes() for r in range(4)}) == 4, (name, klass)
            r = ref.run(lp.PRIMS[name]['ref'], c)
            assert r.out or not lp._same_bits(r.aux, c.aux).all(), 'a case of %s [%s] that asks for nothing' % (name, klass)


def test_every_lane_method_the_step_kernels_call_is_in_the_table():
    """A plain text scan of the kernel bodies for the methods they call on the lane policy (L::name( or ln.name( / lanes.name(): a primitive added later cannot go untested silently."""
    csrc = os.path.join(lp.ROOT, 'lifelike_agility_and_play_amd', 'csrc')
    known = {n for p in lp.PRIMS.values() for n in p['names']} | set(lp.NOT_DRIVEN)
    called = set()
    for f in ('pmc_step.hpp', 'epmc_step.hpp', 'sepmc_step.hpp'):
        text = open(os.path.join(csrc, f)).read()
        called |= set(re.findall(r'\b(?:L::|ln\.|lanes\.)(?:template\s+)?([a-z_][a-z_0-9]*)\s*(?:<[^<>();]*>)?\s*\(', text))
    assert len(called) > 60, sorted(called)
    assert not called - known, 'lane-policy methods no entry of lane_prims_common.PRIMS (or NOT_DRIVEN, with its reason) names: %s' % sorted(called - known)


def test_a_broken_lane_or_operand_is_reported_by_name(host):
    """The comparison is fed the twin's own answer with the damage one wrong DPP control or one wrong asm operand would do: it must fail, and name the primitive."""
    def answer(name, klass='random', pick=0):
        c = [c for k, c in lp.all_cases(name, host.dims) if k == klass][pick]
        out, aux = host.run(0, lp.PRIMS[name]['id'], c, 0b1111)
        lp.check_against_reference(name, klass, c, out, aux, 0b1111, 'twin')
        return c, out, aux
    # a row_ror one lane off in one of sixteen turns: lane 4 t + S reads its neighbour's pending increment
    c, out, aux = answer('turns16')
    out[2, 1, 9] = out[2, 1, 10]
    with pytest.raises(AssertionError, match=r'^turns16 \[random'):
        lp.check_against_reference('turns16', 'random', c, out, aux, 0b1111, 'twin')
    # quad_perm [3,3,3,3] where [2,2,2,2] was meant, on exact inputs
    c, out, aux = answer('subbcast', 'exact', 2)
    out[:, 0] = c.w[:, 0][:, np.arange(16) | 3]
    with pytest.raises(AssertionError, match=r'^subbcast \[exact, targ 2'):
        lp.check_against_reference('subbcast', 'exact', c, out, aux, 0b1111, 'twin')
    # two coupling operands of the 30-operand block exchanged: k12 of the second turn used for k21
    c, out, aux = answer('cone_turns4', 'exact', 1)
    c2 = lp.Case(host.dims, c.targ); c2.w[:] = c.w
    L = 4 + c.targ
    c2.w[:, 24 + L], c2.w[:, 40 + L] = c.w[:, 40 + L].copy(), c.w[:, 24 + L].copy()
    out2, aux2 = host.run(0, lp.PRIMS['cone_turns4']['id'], c2, 0b1111)
    with pytest.raises(AssertionError, match=r'^cone_turns4 \[exact, targ 1'):
        lp.check_against_reference('cone_turns4', 'exact', c, out2, aux2, 0b1111, 'twin')
    # a store one word past the row
    c, out, aux = answer('st16', 'edges', 2)
    aux[1, c.ia[1]] = 0.0
    with pytest.raises(AssertionError, match=r'^st16 .*global memory'):
        lp.check_against_reference('st16', 'edges', c, out, aux, 0b1111, 'twin')
    # a row outside EXEC that wrote
    c, out, aux = answer('qsum', 'exact')
    out2, aux2 = host.run(0, lp.PRIMS['qsum']['id'], c, 0b0011)
    out2[2, 0, 0] = 1.0
    with pytest.raises(AssertionError, match=r'^qsum .*outside EXEC'):
        lp.check_against_reference('qsum', 'exact', c, out2, aux2, 0b0011, 'twin')
