"""The loss of a scored block without a GPU: include/hl/llenv_hl_loss.h == policies.hl_loss == what libllenv.so exports, the config struct against a C
program compiled on the spot, every LLL_* index against hl_loss.STATS, and every LL_EINVAL guard that fires before the device is touched."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from lifelike_agility_and_play_amd import capi
from lifelike_agility_and_play_amd.policies import hl_loss as HL
from lifelike_agility_and_play_amd.policies import hl_policy_hip as H
import hl_loss_ref as LR

HEADER = os.path.join(ROOT, 'include', 'hl', 'llenv_hl_loss.h')


def _lib():
    import __graft_entry__ as g
    g.build_hip()
    return HL.load_library()


def test_header_binding_and_library_agree():
    text = open(HEADER).read()
    declared = sorted(set(re.findall(r'\b(ll_hl_loss_[a-z0-9_]+)\s*\(', text)))
    assert declared == HL.EXPORTED_SYMBOLS == sorted(HL._SIGS) and len(declared) == 5
    lib = _lib()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.ll_abi_version() == capi.LL_ABI_VERSION            # additive entry points
    assert re.search(r'#define LLL_PPO 0\b', text) and re.search(r'#define LLL_PPO2 1\b', text) and (HL.LLL_PPO, HL.LLL_PPO2) == (0, 1)


def test_stat_indices():
    """every #define LLL_<NAME> <index> of the statistics against hl_loss.STATS and the reference's table; the slots tile 0 .. LLL_N_STATS - 1"""
    text = open(HEADER).read()
    defs = {n: int(v) for n, v in re.findall(r'#define LLL_([A-Z_0-9]+) (\d+)\b', text)}
    n_stats = defs.pop('N_STATS')
    defs.pop('PPO'), defs.pop('PPO2')
    assert {k.lower(): v for k, v in defs.items()} == {k.lower(): i for k, (i, _) in HL.STATS.items()}
    assert n_stats == HL.LLL_N_STATS == LR.N_STATS == 20 and HL.STATS == LR.STATS
    cover = sorted(j for i, d in HL.STATS.values() for j in range(i, i + d))
    assert cover == list(range(n_stats))
    assert HL.named(list(range(20)))['clip_frac'] == [14.0, 15.0, 16.0] and HL.named(list(range(20)))['loss'] == 7.0
    with pytest.raises(ValueError):
        HL.named([0.0] * 19)


def test_config_struct_against_c(tmp_path):
    """sizeof and the offset of every field from a C program that includes the header, and the defaults of ll_hl_loss_default_config"""
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang')
    assert cc, 'no C compiler'
    names = [n for n, _ in HL.LossConfig._fields_]
    src = tmp_path / 'cfg.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hl/llenv_hl_loss.h"\nint main(void) {\n  printf("%zu", sizeof(ll_hl_loss_config_t));\n' +
                   ''.join('  printf(" %%zu", offsetof(ll_hl_loss_config_t, %s));\n' % n for n in names) + '  return 0;\n}\n')
    exe = tmp_path / 'cfg'
    subprocess.check_call([cc, '-std=c99', '-I', os.path.join(ROOT, 'include'), '-o', str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(HL.LossConfig) == 48
    assert got[1:] == [getattr(HL.LossConfig, n).offset for n in names] == [4 * i for i in range(12)]
    lib = _lib()
    cfg = HL.default_config(lib)
    want = LR.config()
    for n in names:
        if n != 'reserved':
            assert getattr(cfg, n) == want[n], n
    assert cfg.reserved == 0 and cfg.mode == HL.LLL_PPO and cfg.clip_range == C.c_float(0.2).value and cfg.adv_eps == C.c_float(1e-8).value
    assert HL.default_config(lib, mode=HL.LLL_PPO2, lam=0.5).lam == 0.5
    with pytest.raises(AttributeError):
        HL.default_config(lib, clip=0.1)
    assert lib.ll_hl_loss_default_config(None) == -1


def test_workspace_bytes():
    lib = _lib()
    small, big = HL.workspace_bytes(1, 1, lib), HL.workspace_bytes(4096, 128, lib)
    assert small > 0 and small % 8 == 0 and big - small == 8 * (4096 * 128 - 1)      # the ppo2 returns, one float64 per cell, on top of the partials
    out = C.c_uint64(0)
    for n, L in ((0, 1), (1, 0), (-1, 4)):
        assert lib.ll_hl_loss_workspace_bytes(n, L, C.byref(out)) == -1
    assert lib.ll_hl_loss_workspace_bytes(1, 1, None) == -1


def test_bad_arguments_are_einval_before_the_device():
    """Every guard of the header with host memory standing in for the device pointers: nothing is dereferenced before the checks are through.  The last
    call is good in every argument and reaches the device question: LL_ENODEV on a machine without one."""
    import torch
    lib = _lib()
    n, L = 2, 3
    nbytes = HL.workspace_bytes(n, L, lib)
    buf = (C.c_double * (nbytes // 8 + 64))()
    base = C.addressof(buf)
    base += (-base) % 16
    p = C.c_void_p(base)
    good = dict(kind=H.LLH_EPMC, cfg=HL.default_config(lib), rows=p, n=n, L=L, score=p, weight=None, grad=p, stats=p, work=p, wb=nbytes)

    def call(**kw):
        a = dict(good, **kw)
        return lib.ll_hl_loss_rows(a['kind'], C.byref(a['cfg']) if a['cfg'] is not None else None, a['rows'], a['n'], a['L'], a['score'], a['weight'], a['grad'],
                                   a['stats'], a['work'], a['wb'], None)

    for name in ('cfg', 'rows', 'score', 'grad', 'stats', 'work'):
        assert call(**{name: None}) == -1 and lib.ll_last_error().decode(), name
    for kw in (dict(n=0), dict(n=-3), dict(L=0), dict(L=-1), dict(kind=0), dict(kind=3), dict(wb=nbytes - 1), dict(wb=0)):
        assert call(**kw) == -1, kw
    for field, bad in (('mode', 2), ('mode', -1), ('clip_range', -0.1), ('clip_range', float('nan')), ('clip_range', float('inf')), ('vf_coef', -1.0),
                       ('vf_coef', float('nan')), ('adv_eps', -1e-8), ('adv_eps', float('inf')), ('gamma', 1.5), ('gamma', -0.1), ('gamma', float('nan')),
                       ('lam', 1.01), ('lam', -0.5), ('lam', float('nan')), ('clip_range_lower', float('nan')), ('vf_clip', float('inf')), ('ent_coef', float('nan'))):
        assert call(cfg=HL.default_config(lib, **{field: bad})) == -1, (field, bad)
        assert lib.ll_last_error().decode()
    assert call(cfg=HL.default_config(lib, mode=HL.LLL_PPO2), L=1) == -1                    # ppo2 needs a bootstrap step
    assert call(L=(1 << 31) // 1128 + 1, wb=1 << 62) == -1                                  # 2^31 floats per row or more
    assert call(kind=H.LLH_SEPMC, L=(1 << 31) // 1244 + 1, wb=1 << 62) == -1
    for name in ('score', 'grad'):
        assert call(**{name: C.c_void_p(base + 8)}) == -1, name                            # 16-byte accesses
    for name in ('stats', 'work'):
        assert call(**{name: C.c_void_p(base + 4)}) == -1, name
    for fn in (lib.ll_hl_loss_unroll, lib.ll_hl_loss_league):
        assert fn(None, 0, C.byref(good['cfg']), p, None, p, p, p, nbytes) == -1 and lib.ll_last_error().decode()
    with pytest.raises(TypeError):
        HL.ppo_loss(None, object(), 0)
    if not torch.cuda.is_available():
        assert call() == -5 and 'no HIP device' in lib.ll_last_error().decode()           # LL_ENODEV: no CPU path
        with pytest.raises(capi.LLError) as ei:
            HL.loss_rows(H.LLH_EPMC, good['cfg'], base, n, L, base, None, base, base, base, nbytes, lib=lib)
        assert ei.value.code == -5
