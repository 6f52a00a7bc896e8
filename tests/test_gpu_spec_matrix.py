"""The spec-switch matrix (tests/spec_matrix.py) through the HIP library on an MI355X: acceptance, binding and oracle parity of every row in the
one-wave build, the rows that change the build -- and every scalar switch moved together -- in the 256-register build (4096 + 256 envs), the
multi-step XROWS launches against single launches, and kernel timing across a refused step.  Run with `pytest -m gpu`."""
import math

import numpy as np
import pytest

import spec_matrix as sm
import spec_matrix_common as smc
from lifelike_agility_and_play_amd import capi

pytestmark = pytest.mark.gpu

BIG = 4096 + 256          # above one wave per SIMD: the OCC 2 builds (the existing tests' size)
BUILD_ROWS = ('friction_mode', 'self_friction', 'pair_friction', 'max_pair', 'leg_edges')


@pytest.mark.parametrize('engine', sm.ENGINES)
def test_acceptance(engine):
    smc.check_acceptance(engine, None)


@pytest.mark.parametrize('engine', sm.ENGINES)
def test_binding(engine):
    smc.check_binding(engine, None)


def _parity_cases(big):
    out = []
    for engine in sm.ENGINES:
        for name, spec in smc.parity_rows(engine):
            if not big or name in BUILD_ROWS:
                out.append(pytest.param(engine, name, spec, id='%s-%s' % (engine, name)))
        if big:
            out.append(pytest.param(engine, 'all_scalars', sm.all_scalars(engine), id='%s-all_scalars' % engine))
    return out


@pytest.mark.parametrize('engine,name,spec', _parity_cases(False))
def test_parity_one_wave(engine, name, spec, golden, orc):
    smc.check_parity(engine, name, spec, None, golden=golden, orc=orc)


@pytest.mark.parametrize('engine,name,spec', _parity_cases(True))
def test_parity_256_registers(engine, name, spec, golden, orc, monkeypatch):
    monkeypatch.setenv('LL_SHARE_SIMDS', '1')          # the 256-register builds at every size (SEPMC runs its one-wave build at every size by default)
    smc.check_parity(engine, name, spec, None, golden=golden, orc=orc, total=BIG // 2 if engine == 'sepmc' else BIG)


@pytest.mark.parametrize('engine,spec,occs,split', sm.MULTI_CHECKS, ids=lambda x: str(x))
def test_multi_step_launch(engine, spec, occs, split, model_blob, mocap_table):
    """every MULTI build (tests/spec_matrix.py MULTI_CHECKS): k control steps in one launch == k launches, bit for bit.  PMC at both occupancies
    (the XROWS builds: multi-step within one wave per SIMD, single launches beyond), EPMC and SEPMC in their one-wave builds with the rays fused."""
    import torch
    import epmc_parity_common as ec
    import parity_common as pc
    import sepmc_parity_common as sc
    from lifelike_agility_and_play_amd import gather
    assert torch.cuda.is_available()

    def read_ring(addr, shape):
        return gather.device_tensor(addr, shape).cpu().numpy()
    if engine in ('pmc', 'pmc_obst'):
        sizes = (70, 4096, BIG) if 'self_friction' in spec else (70, BIG)
        pc.check_multi_step_launch(model_blob, mocap_table, None, read_ring, sizes=sizes, k=5, n_launches=2, spec=spec, obstacle=engine == 'pmc_obst')
    else:
        with ec.spec_variant(**spec):        # (check_multi_step_launch sets LL_SPLIT_RAYS=0 itself; the sizes of test_gpu_epmc.py / test_gpu_sepmc.py)
            if engine == 'epmc':
                ec.check_multi_step_launch(None, sizes=(70,), k=7, n_launches=3)
            else:
                sc.check_multi_step_launch(None, sizes=(35,), k=7, n_launches=3)


REFUSE = dict(pmc=dict(self_friction=0.25, friction_mode=0), pmc_obst=dict(leg_edges=1), epmc=dict(leg_edges=1, friction_mode=0),
              sepmc=dict(max_pair=3, friction_mode=0))


@pytest.mark.parametrize('engine', sm.ENGINES)
def test_kernel_timing_across_a_refused_step(engine):
    """With kernel timing on: good step, refused step, good step.  The timing reports exactly the two launches that ran, and the engine equals a
    twin that never made the refused call."""
    E, T = smc.make(engine, None), smc.make(engine, None)
    E.enable_kernel_timing(True)
    smc.step(E, engine); smc.step(T, engine)
    default = {k: E.get_spec(k) for k in REFUSE[engine]}
    E.set_spec(**REFUSE[engine])
    with pytest.raises(capi.LLError) as ei:
        smc.step(E, engine)
    assert ei.value.code == capi.LL_EINVAL
    E.set_spec(**default)
    smc.step(E, engine); smc.step(T, engine)
    ms, n, steps = E.kernel_time_stats()
    assert n == 2 and steps == 2 and math.isfinite(ms) and ms > 0, (ms, n, steps)
    assert smc.same(smc.snapshot(E, engine), smc.snapshot(T, engine))
    E.close(); T.close()
