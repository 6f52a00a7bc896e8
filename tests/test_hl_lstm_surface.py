"""The LN-LSTM core without a GPU: include/hl/llenv_hl_lstm.h == policies.hl_lstm == what libllenv.so exports, ll_hl_lstm_weights_t against a C program
compiled on the spot, the packed layout, the workspace sizes, and every LL_EINVAL guard that fires before the device is touched."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from lifelike_agility_and_play_amd import capi
from lifelike_agility_and_play_amd.policies import hl_lstm as HT
import hl_lstm_ref as T

HEADER = os.path.join(ROOT, 'include', 'hl', 'llenv_hl_lstm.h')


def _lib():
    import __graft_entry__ as g
    g.build_hip()
    return HT.load_library()


def test_header_binding_and_library_agree():
    text = open(HEADER).read()
    declared = sorted(set(re.findall(r'\b(ll_hl_lstm_[a-z0-9_]+)\s*\(', text)))
    assert declared == HT.EXPORTED_SYMBOLS == sorted(HT._SIGS) and len(declared) == 4
    lib = _lib()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.ll_abi_version() == capi.LL_ABI_VERSION            # additive entry points
    defs = {n: int(v) for n, v in re.findall(r'#define LLT_([A-Z_0-9]+) (\d+)\b', text)}
    assert defs == dict(N_IN=HT.N_IN, N_GATES=HT.N_GATES, N_UNITS=HT.N_UNITS, STATE_FLOATS=HT.STATE_FLOATS, MAX_OUT=HT.MAX_OUT, N_WEIGHTS=HT.N_WEIGHTS,
                        TAPE_FLOATS=HT.TAPE_FLOATS)
    assert HT.TAPE_FLOATS <= 512 and HT.BRANCHES == T.BRANCHES and HT.WEIGHT_NAMES == T.NAMES
    for (kind, branch), (k0, head, D) in HT.BRANCHES.items():     # the table of the header's text
        assert re.search(r'%s %s\s+%d\s+%d, %d\s+%d\b' % (kind.upper(), branch, k0, head[0], head[1], D), text), (kind, branch)


def test_weights_struct_against_c(tmp_path):
    """sizeof and the offset of every field from a C program that includes the header"""
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang')
    assert cc, 'no C compiler'
    names = [n for n, _ in HT.LstmWeights._fields_]
    src = tmp_path / 'w.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hl/llenv_hl_lstm.h"\nint main(void) {\n  printf("%zu", sizeof(ll_hl_lstm_weights_t));\n' +
                   ''.join('  printf(" %%zu", offsetof(ll_hl_lstm_weights_t, %s));\n' % n for n in names) + '  return 0;\n}\n')
    exe = tmp_path / 'w'
    subprocess.check_call([cc, '-std=c99', '-I', os.path.join(ROOT, 'include'), '-o', str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(HT.LstmWeights) == 96
    assert got[1:] == [getattr(HT.LstmWeights, n).offset for n in names] == [8 * i for i in range(11)] + [88, 92]
    assert names[:11] == list(HT.WEIGHT_NAMES)
    w = HT.weights_struct(list(range(16, 16 * 12, 16)), 7)
    assert (w.wx, w.bo, w.n_out, w.reserved) == (16, 176, 7, 0)
    with pytest.raises(ValueError):
        HT.weights_struct([16] * 10, 1)


@pytest.mark.parametrize('D', [1, 12, 256])
def test_layout_tiles_the_packed_gradient(D):
    lib = _lib()
    off, dim, total = HT.weight_layout(D, lib)
    assert total == 37568 + 33 * D and off[0] == 0
    assert all(off[i] + dim[i] == off[i + 1] for i in range(10)) and off[10] + dim[10] == total
    assert (off, dim, total) == T.layout(D) and dim == [int(np.prod(s)) for s in HT.shapes(D)] and HT.shapes(D) == T.shapes(D)
    assert lib.ll_hl_lstm_weight_layout(D, None, None, None) == 0
    for bad in (0, -1, 257):
        assert lib.ll_hl_lstm_weight_layout(bad, None, None, None) == -1 and lib.ll_last_error().decode()


def test_workspace_bytes():
    lib = _lib()
    tape, work = HT.workspace_bytes(1, 1, 1, lib)
    assert tape == 4 * HT.TAPE_FLOATS and work > 0 and work % 4 == 0
    tape2, work2 = HT.workspace_bytes(4096, 128, 256, lib)
    assert tape2 == 4 * HT.TAPE_FLOATS * 4096 * 128 and work2 % 4 == 0
    # per frame: the gradients at u and at v; per 8 rows: 448 float64; at most HLS_MAX_GROUPS = 80 rows of float64 partials
    assert work2 == 2 * 512 * 4096 * 128 + 512 * 448 * 8 + 80 * (36864 + 33 * 256) * 8
    out = C.c_uint64(0)
    for n, L, D in ((0, 1, 1), (1, 0, 1), (-1, 4, 1), (1, 1, 0), (1, 1, 257), (1 << 16, 1 << 15, 1), (1 << 30, 2, 1)):
        assert lib.ll_hl_lstm_workspace_bytes(n, L, D, C.byref(out), None) == -1, (n, L, D)
    assert lib.ll_hl_lstm_workspace_bytes((1 << 30) - 1, 2, 1, C.byref(out), None) == 0
    assert lib.ll_hl_lstm_workspace_bytes(1, 1, 1, None, None) == 0


def test_bad_arguments_are_einval_before_the_device():
    """Every guard of the header with host memory standing in for the device pointers: nothing is dereferenced before the checks are through.  The last
    calls are good in every argument and reach the device question: LL_ENODEV on a machine without one."""
    import torch
    lib = _lib()
    n, L, D = 2, 3, 5
    tape_bytes, work_bytes = HT.workspace_bytes(n, L, D, lib)
    buf = (C.c_double * ((tape_bytes + work_bytes) // 8 + 64))()
    base = C.addressof(buf)
    base += (-base) % 16
    p = C.c_void_p(base)
    W = HT.weights_struct([base] * 11, D)
    fwd = dict(w=W, e=p, s0=p, s0_rs=64, m=p, m_rs=L, m_ss=1, n=n, L=L, y=p, y_stride=D, s_end=p, tape=p, tape_bytes=tape_bytes)
    bwd = dict(w=W, e=p, m=p, m_rs=L, m_ss=1, n=n, L=L, tape=p, tape_bytes=tape_bytes, dy=p, dy_stride=D, ds_end=p, de=p, ds0=p, wgrad=p, work=p, work_bytes=work_bytes)

    def forward(**kw):
        a = dict(fwd, **kw)
        return lib.ll_hl_lstm_forward(C.byref(a['w']) if a['w'] is not None else None, a['e'], a['s0'], a['s0_rs'], a['m'], a['m_rs'], a['m_ss'], a['n'], a['L'],
                                      a['y'], a['y_stride'], a['s_end'], a['tape'], a['tape_bytes'], None)

    def backward(**kw):
        a = dict(bwd, **kw)
        return lib.ll_hl_lstm_backward(C.byref(a['w']) if a['w'] is not None else None, a['e'], a['m'], a['m_rs'], a['m_ss'], a['n'], a['L'], a['tape'],
                                       a['tape_bytes'], a['dy'], a['dy_stride'], a['ds_end'], a['de'], a['ds0'], a['wgrad'], a['work'], a['work_bytes'], None)

    def changed(**kw):
        w = HT.weights_struct([base] * 11, D)
        for k, v in kw.items():
            setattr(w, k, v)
        return w

    odd = C.c_void_p(base + 8)
    both = [dict(w=None), dict(e=None), dict(m=None), dict(n=0), dict(n=-2), dict(L=0), dict(L=-1), dict(m_rs=0), dict(m_ss=0), dict(m_ss=-1),
            dict(n=1 << 16, L=1 << 15, tape_bytes=1 << 62, work_bytes=1 << 62), dict(tape_bytes=tape_bytes - 1), dict(e=odd), dict(tape=odd),
            dict(w=changed(reserved=1)), dict(w=changed(n_out=0)), dict(w=changed(n_out=257)), dict(w=changed(n_out=-1))]
    both += [dict(w=changed(**{name: None})) for name in HT.WEIGHT_NAMES]
    for kw in both:
        f = {k: v for k, v in kw.items() if k != 'work_bytes'}
        assert forward(**f) == -1 and lib.ll_last_error().decode(), kw
        assert backward(**kw) == -1 and lib.ll_last_error().decode(), kw
    for kw in (dict(s0=None), dict(y=None), dict(s0_rs=63), dict(y_stride=D - 1), dict(tape_bytes=0)):
        assert forward(**kw) == -1 and lib.ll_last_error().decode(), kw
    for kw in (dict(tape=None), dict(dy=None), dict(de=None), dict(wgrad=None), dict(work=None), dict(dy_stride=D - 1), dict(work_bytes=work_bytes - 1), dict(work_bytes=0),
               dict(de=odd), dict(work=odd)):
        assert backward(**kw) == -1 and lib.ll_last_error().decode(), kw
    with pytest.raises(ValueError):
        HT.ln_lstm(np.zeros((1, 1, 256), np.float32), None, None, [None] * 11, 1)
    with pytest.raises(ValueError):
        HT.ln_lstm(torch.zeros((1, 1, 256)), torch.zeros((1, 64)), torch.zeros((1, 1)), [torch.zeros(s) for s in HT.shapes(1)], 1)     # not on the device
    with pytest.raises(KeyError):
        HT.branch_weights('epmc', 'hlc', {})
    picked = HT.branch_weights('sepmc', 'value', {i: np.zeros((1, 128)) if i == 42 else np.full(s, i) for i, s in
                                                   zip(list(range(40, 49)) + [49, 50], HT.shapes(1))})
    assert [a.shape for a in picked] == HT.shapes(1) and picked[9][0, 0] == 49 and picked[0][0, 0] == 40
    if not torch.cuda.is_available():
        # the nullable ones left out, and a good call in full: LL_ENODEV, there is no CPU path
        assert forward(s_end=None, tape=None, tape_bytes=0) == -5 and 'no HIP device' in lib.ll_last_error().decode()
        assert forward() == -5 and backward() == -5 and backward(ds_end=None, ds0=None) == -5
        with pytest.raises(capi.LLError) as ei:
            HT.forward(W, base, base, 64, base, L, 1, n, L, base, D, None, None, 0, lib=lib)
        assert ei.value.code == -5
