"""Shared by tests/test_lane_prims_emul.py and tests/test_gpu_lane_prims.py: the class table of the lane primitives, their inputs (fixed seeds; the four rows of a
wave get DIFFERENT data, so a leak between rows shows), the runners of the host twin and the GPU copies of tests/lanes/, and the comparison.

Input classes
  exact   small integers times 2^-2, couplings whole numbers |k| <= 2, bounds |lo|, |hi| <= 4: every product and every partial sum in ANY association is a float32
          (partial sums far below 2^24), so fused or unfused, tree or sequence cannot differ -- a mismatch is a routing or selection error.  cone_turns4: only rows
          exact by construction (lim == 0; S1 = S2 = 0 under lim > 0; pairs far inside the cone, lim >= 2^10 |S| throughout, where sc clamps to exactly 1).
  random  normal floats of order 1, sum |k| over a lane's incoming couplings <= 1/2 (the diagonally dominant situation of the whitened solver), pairs outside the
          cone; no denormal inputs or products (the GPU build flushes them, the host does not).
  edges   exact too: +-0 and +-inf as u of turns*, lo == hi, NEG_LO with lo = 0, an all-equal row for rmin / submin, n no multiple of 16 and split at 0, 1,
          n - 1, n for ld16 / st16 / st16_rot / copy16 between NaN canaries, count_le16 with ties and n = 0, 1, 16, 17, every candc word (both sides of every
          PIN_CANDS / LKB boundary of GpuLanesPinned among them).
"""
import ctypes as C
import os
import subprocess

import numpy as np

import lane_prims_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES_DIR = os.path.join(ROOT, 'tests', 'lanes')
BUILD_DIR = os.path.join(LANES_DIR, '_build')
HOST_LIB = os.path.join(BUILD_DIR, 'liblane_prims_host.so')
VARIANTS = ['shipped', 'cone_pipe0', 'mfma_gram1', 'peer_mode1', 'peer_mode2']          # the GPU copies (__graft_entry__.LANE_PRIM_VARIANTS)
GPU_POLICIES = ['GpuLanes', 'GpuLanes1', 'GpuLanesPmc1Plain', 'WithTurnMasksCmp<GpuLanes>', 'WithTurnMasksCmp<GpuLanesPmc1Plain>', 'WithConeInLds<GpuLanes1>',
                'WithGramPipe<GpuLanesPmc1Plain>']
HOST_POLICIES = ['HostLanes', 'WithConeInLdsHost<HostLanes>', 'WithGramPipeHost<HostLanes>']
ACTIVE_ROWS = [0b1111, 0b0011, 0b0100]       # the whole wave, rows {0, 1}, row {2}: the primitive runs under a partial EXEC as in the tail wave of an odd batch

MOVES, SUMS, FUSED = 'MOVES', 'SUMS', 'FUSED'
# ---- THE CLASS TABLE: which primitives agree bit for bit between GpuLanes, HostLanes and the float64 statement, and which only to rounding ----------------------------
#   MOVES   no arithmetic: GPU == host twin == reference, bit for bit, on all three input classes
#   SUMS    additions only: GPU == host twin bit for bit on all classes (the twin follows the tree's association; an add rounds once on both sides);
#           both within n u sum |t| of the reference
#   FUSED   a multiply-add: bit for bit on exact and edges; on random each of GPU and twin within the derived bound of the reference (v_fmac / v_fma round once,
#           the twin's product and sum twice; vel_commit's twin sums in lane order, the GPU in a quad-exchange tree followed by row_ror)
#   'bits_on_random': output words of a FUSED primitive that are bit-equal between GPU and twin on random inputs as well (a lone add rounds once on both sides) -- asserted;
#           no other word of a FUSED primitive qualified on the MI355X (profiles/lane_prims_bounds.txt lists what was observed): everywhere else v_fmac / v_fma meet the
#           twin's two roundings
# id: LanePrim of tests/lanes/lane_prims_body.hpp; targs: the template arguments the driver is instantiated for; names: the lane-policy methods the entry covers
PRIMS = {
    'from_prev_leg': dict(id=0, cls=MOVES), 'from_leg2': dict(id=1, cls=MOVES), 'from_next_leg': dict(id=2, cls=MOVES),
    'rbcast': dict(id=3, cls=MOVES, targs=range(16)), 'subbcast': dict(id=4, cls=MOVES, targs=range(4)), 'bcast': dict(id=5, cls=MOVES, targs=range(4)),
    'subbcast6': dict(id=6, cls=MOVES, targs=range(4)), 'subbcast6_after': dict(id=7, cls=MOVES, targs=range(4)),
    'gather_tri3': dict(id=8, cls=MOVES), 'spread3': dict(id=9, cls=MOVES), 'rmin': dict(id=10, cls=MOVES), 'submin': dict(id=11, cls=MOVES),
    'vel_dx': dict(id=12, cls=MOVES, targs=range(6)), 'vel_dq': dict(id=13, cls=MOVES, targs=range(4)),
    'peer': dict(id=14, cls=MOVES, names=['peer', 'peer_u']),
    'row_ballot': dict(id=15, cls=MOVES, host_shape='a row of one lane'),      # (the twin's per-env code is ONE lane: it answers pred ? 1 : 0 by design, held to that)
    'ld16': dict(id=16, cls=MOVES), 'st16': dict(id=17, cls=MOVES), 'st16_rot': dict(id=18, cls=MOVES), 'copy16': dict(id=19, cls=MOVES),
    'count_le16': dict(id=20, cls=MOVES), 'park_row': dict(id=21, cls=MOVES, names=['park_row', 'unpark_row']),
    'cone_lds': dict(id=22, cls=MOVES, targs=range(4), names=['cone_store', 'cone_load', 'row_sync', 'row_scratch']),
    'stage_row': dict(id=23, cls=MOVES), 'legc': dict(id=24, cls=MOVES), 'candc': dict(id=25, cls=MOVES), 'basec': dict(id=26, cls=MOVES), 'candc_of': dict(id=27, cls=MOVES),
    'settle': dict(id=28, cls=MOVES),
    'lane_ids': dict(id=29, cls=MOVES, targs=[0, 5, 10, 15], names=['leg', 'sub', 'legf', 'is_leg', 'is_sub', 'is_lane', 'lane_f', 'i2f']),
    'pick': dict(id=30, cls=MOVES, names=['pick3', 'pick4i', 'pick4d', 'd2f', 'f2i']),
    'ldl_stl': dict(id=31, cls=MOVES, names=['ldl', 'stl']), 'ldl2': dict(id=32, cls=MOVES, targs=range(8), names=['stl_if', 'lddl', 'ldd_idx']),
    'qsum': dict(id=40, cls=SUMS), 'subsum': dict(id=41, cls=SUMS), 'rsum6': dict(id=42, cls=SUMS), 'qsum6': dict(id=43, cls=SUMS), 'subsum3': dict(id=44, cls=SUMS),
    'sufsum4': dict(id=45, cls=SUMS), 'sufsum6': dict(id=46, cls=SUMS),
    'fmac_rbcast': dict(id=50, cls=FUSED, targs=range(16)), 'fmac_rbcast_settled': dict(id=51, cls=FUSED, targs=range(16), ref='fmac_rbcast'),
    'gram4': dict(id=52, cls=FUSED, targs=range(4)), 'gram16': dict(id=53, cls=FUSED), 'gram_pipe': dict(id=54, cls=FUSED, ref='gram16', names=['gram_mfma', 'gram_collect']),
    'turns4': dict(id=55, cls=FUSED, targs=[0, 1, 2, 3, 16, 17, 18, 19], names=['turns4', 'prepare_turn_masks']),
    'turns8': dict(id=56, cls=FUSED, targs=[0, 1, 16, 17]), 'cone_turns4': dict(id=57, cls=FUSED, targs=range(4)),
    'vel_dot': dict(id=58, cls=FUSED), 'vel_commit': dict(id=59, cls=FUSED, bits_on_random=[3]),        # (word 3: lam += dl, one add)
    'vel_commit2': dict(id=60, cls=FUSED, bits_on_random=[3, 4], names=['vel_commit2', 'pair']),
    'turns16': dict(id=61, cls=FUSED, names=['turns4']),
}
# Lane-policy methods the step kernels call that NO primitive case drives, each with the reason (tests/test_lane_prims_emul.py: a method in neither table fails the scan)
NOT_DRIVEN = {
    'any': 'wave-level __any on the GPU, row-level on the host: the two differ by design (it only guards wave-uniform branches)',
    'lane0': 'lane-local compare; the host row is one lane', 'ray_first': 'work split: 16 ways on the GPU, one lane on the host', 'ray_stride': 'as ray_first',
    'params': 'hands the kernel argument block back', 'refresh_consts': 'a compiler barrier, no value',
}
for _k, _v in PRIMS.items():
    _v.setdefault('targs', [0]); _v.setdefault('ref', _k); _v.setdefault('names', [_k])
# what a variant build changes in lanes.hpp: the shipped build runs every primitive, a variant build those its switch touches
BUILD_PRIMS = {'shipped': list(PRIMS), 'cone_pipe0': ['cone_turns4'], 'mfma_gram1': ['gram4', 'gram16', 'gram_pipe'], 'peer_mode1': ['peer'], 'peer_mode2': ['peer']}


class Case:
    def __init__(self, dims, targ=0, ia=(0, 0, 0, 0)):
        self.targ, self.ia = targ, np.array(ia, dtype=np.int32)
        self.w = np.zeros((4, dims.n_in, 16), dtype=np.float32)
        self.aux = np.full((4, dims.n_aux), np.nan, dtype=np.float32)       # NaN canaries: nothing outside what a primitive owns may be written
        self.auxd = np.zeros(dims.n_auxd, dtype=np.float64)
        self.legc, self.candc, self.basec = dims.legc, dims.candc, dims.basec


class Dims:
    def __init__(self, lib):
        d = (C.c_int * 16)()
        lib.ll_lane_prims_dims(d)
        self.n_in, self.n_out, self.n_aux, self.n_auxd, self.lc, self.cw, self.bc, self.n_consts, self.lk_base, self.row_scratch, self.cone_pipe, self.mfma_gram, self.peer_mode, self.n_policies = list(d)[:14]
        # the constant tables: every word its own value (its index in the buffer, + 1), so that a read of the wrong word, leg or lane shows
        self.consts = np.arange(1, self.n_consts + 1, dtype=np.float32)
        self.consts[-1] = 1.0
        self.legc = self.consts[:self.lc * 4].reshape(self.lc, 4)
        self.candc = self.consts[self.lc * 4:self.lc * 4 + self.cw * 16].reshape(self.cw, 16)
        self.basec = self.consts[self.lc * 4 + self.cw * 16:-1]


def _bind(path):
    lib = C.CDLL(path)
    lib.ll_lane_prims_dims.argtypes = [C.POINTER(C.c_int)]
    lib.ll_lane_prims_run.restype = C.c_int
    lib.ll_lane_prims_run.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def build_host():
    subprocess.check_call(['make', '-C', LANES_DIR, '-s'])
    return HOST_LIB


class HostRunner:
    def __init__(self):
        self.lib = _bind(build_host())
        self.dims = Dims(self.lib)
        self.n_policies = self.dims.n_policies

    def run(self, policy, prim_id, case, active):
        out = np.full((4, self.dims.n_out, 16), np.nan, dtype=np.float32)
        aux = case.aux.copy()
        w, auxd, consts, ia = np.ascontiguousarray(case.w), case.auxd.copy(), self.dims.consts, case.ia.copy()
        rc = self.lib.ll_lane_prims_run(policy, prim_id, case.targ, w.ctypes.data, out.ctypes.data, active, aux.ctypes.data, auxd.ctypes.data, consts.ctypes.data, ia.ctypes.data)
        assert rc == 0, rc
        return out, aux


class GpuRunner:
    """One launch of one wave per run() on the default stream, synchronised; torch only holds the device buffers."""
    def __init__(self, path, host_dims):
        import torch
        self.torch = torch
        self.lib = _bind(path)
        self.dims = Dims(self.lib)
        assert (self.dims.n_in, self.dims.n_out, self.dims.n_aux, self.dims.n_auxd, self.dims.n_consts) == (host_dims.n_in, host_dims.n_out, host_dims.n_aux, host_dims.n_auxd, host_dims.n_consts)
        dev = 'cuda:0'
        self.w = torch.empty((4, self.dims.n_in, 16), dtype=torch.float32, device=dev)
        self.out = torch.empty((4, self.dims.n_out, 16), dtype=torch.float32, device=dev)
        self.aux = torch.empty((4, self.dims.n_aux), dtype=torch.float32, device=dev)
        self.auxd = torch.empty(self.dims.n_auxd, dtype=torch.float64, device=dev)
        self.consts = torch.from_numpy(self.dims.consts.copy()).to(dev)
        self.nan_out = torch.full_like(self.out, float('nan'))

    def run(self, policy, prim_id, case, active):
        t = self.torch
        self.w.copy_(t.from_numpy(case.w)); self.aux.copy_(t.from_numpy(case.aux)); self.auxd.copy_(t.from_numpy(case.auxd)); self.out.copy_(self.nan_out)
        ia = case.ia.copy()
        t.cuda.synchronize()
        rc = self.lib.ll_lane_prims_run(policy, prim_id, case.targ, self.w.data_ptr(), self.out.data_ptr(), active, self.aux.data_ptr(), self.auxd.data_ptr(), self.consts.data_ptr(), ia.ctypes.data)
        try:
            assert rc == 0, 'll_lane_prims_run: %d' % rc
            t.cuda.synchronize()
            return self.out.cpu().numpy(), self.aux.cpu().numpy()
        except (AssertionError, RuntimeError) as e:        # a launch that failed or faulted: nothing more is started on this device
            import pytest
            pytest.exit('the lane primitive launch (policy %d, primitive %d, targ %d) failed: %s' % (policy, prim_id, case.targ, e), returncode=3)


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------------------
def _ex(rng, shape, lim=8, scale=0.25):
    return (rng.integers(-lim, lim + 1, size=shape) * scale).astype(np.float32)


def _rnd(rng, shape):
    x = rng.standard_normal(shape).astype(np.float32)
    return np.where(np.abs(x) < 2.0 ** -10, np.float32(0.5), x)       # nothing whose product with another operand could go denormal


def _leg_uniform(x):
    return np.repeat(x[..., ::4], 4, axis=-1)


def _couplings(rng, klass, shape, groups):
    """couplings [rows, groups, 16]: exact: whole numbers |k| <= 2; random: the sum of |k| over a lane's `groups` incoming couplings is at most 1/2"""
    if klass != 'random':
        return rng.integers(-2, 3, size=shape).astype(np.float32)
    k = rng.standard_normal(shape)
    k *= rng.uniform(0.1, 0.5, size=(shape[0], 1, 16)) / np.abs(k).sum(axis=1, keepdims=True)
    return (k * (1 - 2.0 ** -20)).astype(np.float32)


def cases(name, klass, dims):
    """the Cases of primitive `name` in input class `klass` (fixed seed per (name, class))"""
    rng = np.random.default_rng([PRIMS[name]['id'], ['exact', 'random', 'edges'].index(klass)])
    val = (lambda shape: _rnd(rng, shape)) if klass == 'random' else (lambda shape: _ex(rng, shape))
    out = []

    def new(targ=0, ia=(0, 0, 0, 0), words=0):
        c = Case(dims, targ, ia)
        if words:
            c.w[:, :words] = val((4, words, 16))
        out.append(c)
        return c

    P = PRIMS[name]
    nwords = {'from_prev_leg': 1, 'from_leg2': 1, 'from_next_leg': 1, 'rbcast': 1, 'subbcast': 1, 'bcast': 1, 'subbcast6': 6, 'subbcast6_after': 6, 'gather_tri3': 3,
              'spread3': 1, 'rmin': 1, 'submin': 1, 'vel_dx': 2, 'vel_dq': 1, 'peer': 1, 'row_ballot': 1, 'park_row': 4, 'cone_lds': 32, 'settle': 1, 'lane_ids': 0, 'pick': 1,
              'subsum': 1, 'rsum6': 6, 'subsum3': 3, 'fmac_rbcast': 3, 'fmac_rbcast_settled': 3, 'gram4': 28, 'gram16': 12, 'gram_pipe': 12, 'vel_dot': 14, 'vel_commit': 15,
              'vel_commit2': 27}
    if name in nwords:
        if klass == 'edges' and name not in ('rmin', 'submin', 'park_row', 'row_ballot'):
            return out
        for targ in P['targs']:
            c = new(targ, words=nwords[name])
            if klass == 'edges' and name in ('rmin', 'submin'):
                c.w[:, 0] = (np.arange(4, dtype=np.float32)[:, None] - 1.5) * (0.5 + targ)      # a row whose values are all equal
                c.w[3, 0, 5] -= 1.0                    # ... and one with a single smaller lane
            if name == 'park_row':
                c.ia[0] = {'exact': 0, 'random': 301, 'edges': dims.row_scratch - 4}[klass]
            if name == 'row_ballot' and klass == 'edges':
                c.w[0, 0] = 1.0; c.w[1, 0] = -1.0; c.w[2, 0] = np.where(np.arange(16) == 15, 1.0, -1.0); c.w[3, 0] = np.where(np.arange(16) == 0, 1.0, -1.0)
    elif name in ('qsum', 'qsum6'):                    # leg-uniform input
        if klass != 'edges':
            new(words=6).w[:, :6] = _leg_uniform(val((4, 6, 16)))
    elif name in ('sufsum4', 'sufsum6'):               # sub-lane 3 holds zero
        if klass != 'edges':
            new(words=6).w[:, :6, 3::4] = 0.0
    elif name in ('ld16', 'st16', 'copy16', 'stage_row', 'st16_rot'):
        if klass != 'edges' and name != 'stage_row':
            shapes = [(0, 16, 0)]
        elif name == 'stage_row':
            shapes = [(0, n, 0) for n in {'exact': [16], 'random': [64], 'edges': [4, 20, 36]}[klass]]
        else:
            shapes = [(0, 1), (0, 5), (0, 17), (16, 17), (16, 31), (0, 32)] + ([(32, 33), (48, 63)] if name != 'copy16' else [])
            shapes = [(i0, n, s) for i0, n in shapes for s in ([0, 1, n - 1, n] if name == 'st16_rot' else [0])]
        for i0, n, split in shapes:
            c = new(ia=(n, 0, 0, 0) if name == 'stage_row' else (i0, n, split, 0), words=1)
            if name in ('ld16', 'copy16', 'stage_row'):
                c.aux[:, :n] = val((4, n))
    elif name == 'count_le16':
        for n in {'exact': [7], 'random': [23], 'edges': [0, 1, 16, 17]}[klass]:
            tbl = np.sort(rng.integers(0, 6, size=n)).astype(np.float64) / 4.0       # non-decreasing, with ties
            for u in ([-1.0, 9.0] + ([tbl[0], tbl[n // 2], tbl[-1]] if n else [])):
                c = new(ia=(n, 0, 0, 0))
                c.auxd[:n] = tbl; c.auxd[n:-1] = -5.0; c.auxd[-1] = u                # (beyond n: values that WOULD count)
    elif name in ('legc', 'candc', 'basec'):
        n = {'legc': dims.lc, 'candc': dims.cw, 'basec': dims.bc}[name]
        for i in (range(n) if klass == 'edges' else [int(rng.integers(0, n))]):     # edges: every word -- both sides of every PIN_CANDS / LKB boundary among them
            new(ia=(i, 0, 0, 0))
    elif name == 'candc_of':
        for word in ([0, 11, 12, dims.lk_base - 1, dims.lk_base, dims.cw - 1] if klass == 'edges' else [int(rng.integers(0, dims.cw))]):
            for sub2 in range(4):
                new(ia=(sub2, word, 0, 0))
    elif name == 'ldl_stl':
        for base, stride in {'exact': [(0, 1)], 'random': [(3, 5)], 'edges': [(7, 8), (0, 0)]}[klass]:
            c = new(ia=(base, stride, 0, 0), words=1)
            c.aux[:, :dims.n_aux // 2] = val((4, dims.n_aux // 2))
    elif name == 'ldl2':
        for targ in P['targs']:
            for ia in {'exact': [(0, 1, 0, 1)], 'random': [(3, 5, 2, 3)], 'edges': [(7, 8, 5, 6), (0, 4, 0, 0)]}[klass]:
                c = new(targ, ia=ia, words=1)
                c.w[:, 1] = rng.integers(0, dims.n_auxd, size=(4, 16))              # the per-lane index of ldd_idx: inside the table
                assert (c.w[:, 1] >= 0).all() and (c.w[:, 1] < dims.n_auxd).all()
                c.auxd[:] = rng.permutation(dims.n_auxd) / 4.0 - 2.0                # every word its own value
    elif name in ('turns4', 'turns8', 'turns16'):
        for targ in P['targs']:
            variants = ['plain'] if klass != 'edges' else ['zeros_infs', 'lo_eq_hi'] + (['neg_lo_zero'] if targ & 16 else [])
            for v in variants:
                c = new(targ)
                c.w[:, 0] = val((4, 16)); c.w[:, 1] = val((4, 16))
                a, b = (np.abs(_rnd(rng, (4, 16))), np.abs(_rnd(rng, (4, 16)))) if klass == 'random' else (_ex(rng, (4, 16), 16, 0.25), _ex(rng, (4, 16), 16, 0.25))
                lo, hi = -np.abs(a), np.abs(b)                                      # lo <= 0 <= hi, |lo|, |hi| <= 4
                if targ & 16:
                    lo = np.abs(np.where(lo == 0, np.float32(1.0), lo))             # NEG_LO: the row passes -lo (a zero bound is the edge case's: +0 against -0 has no one answer)
                c.w[:, 2], c.w[:, 3] = lo, hi
                c.w[:, 4:20] = _couplings(rng, klass, (4, 16, 16), 16)
                if v == 'zeros_infs':                                               # (u = +-0 only between bounds of opposite sign: a zero AT a zero bound has no one answer)
                    c.w[:, 0, 0::4] = [0.0, -0.0, np.inf, -np.inf]
                    c.w[:, 2] = np.where(c.w[:, 2] == 0, 1.0 if targ & 16 else -1.0, c.w[:, 2]); c.w[:, 3] = np.where(c.w[:, 3] == 0, 1.0, c.w[:, 3])
                if v == 'lo_eq_hi':
                    c.w[:, 3] = np.abs(c.w[:, 3]); c.w[:, 2] = -c.w[:, 3] if targ & 16 else c.w[:, 3]
                if v == 'neg_lo_zero':
                    # lo = 0 taken negative is -0.  u in odd eighths, even couplings, bounds in quarters: u moves by quarters and never IS zero (med3(+0, -0, hi) has no one answer)
                    c.w[:, 2] = 0.0; c.w[:, 3] = np.abs(c.w[:, 3]) + 1.0
                    c.w[:, 0] = (2 * rng.integers(-12, 12, size=(4, 16)) + 1) / 8.0
                    c.w[:, 4:20] = 2.0 * rng.integers(-1, 2, size=(4, 16, 16))
    elif name == 'cone_turns4':
        if klass == 'edges':
            return out
        for targ in P['targs']:
            c = new(targ)
            c.w[:, 0:6] = val((4, 6, 16))
            k = _couplings(rng, klass, (4, 64, 16), 64).reshape(4, 4, 16, 16)           # [row, (k11 k12 k21 k22), L, lane]
            if klass == 'random':                                                   # what reaches a lane's S1 (k11, k12) or S2 (k21, k22) in the block's four turns sums to <= 1/2
                k = rng.standard_normal((4, 2, 2, 16, 16))
                k *= rng.uniform(0.1, 0.5, size=(4, 2, 1, 1, 16)) / np.abs(k[:, :, :, targ::4]).sum(axis=(2, 3), keepdims=True)
                k = (k * (1 - 2.0 ** -20)).astype(np.float32)
                c.w[:, 6] = rng.uniform(0.2, 2.0, size=(4, 16)).astype(np.float32)  # pairs inside and outside the cone
                c.w[0, 6, 0::5] = 0.0
            else:
                c.w[0, 6] = 0.0                                                     # row 0: no normal force anywhere: e = -lambda
                c.w[1, 0:2] = 0.0; c.w[1, 6] = 2.0 ** 20                            # row 1: S1 = S2 = 0 under a positive bound
                c.w[2, 6] = 2.0 ** 20                                               # row 2: far inside the cone
                c.w[3, 6] = np.where(np.arange(16) % 3 == 0, 0.0, 2.0 ** 20); c.w[3, 0:2, 1::4] = 0.0       # row 3: all three kinds side by side
            c.w[:, 8:72] = k.reshape(4, 64, 16)
    else:
        raise KeyError(name)
    return out


# ---- comparison ----------------------------------------------------------------------------------------------------------------------------------------
def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


def check_against_reference(name, klass, case, got_out, got_aux, active, who, host_statement=False, r=None):
    """`who`'s answer (out [4, words, 16], aux [4, n_aux]) against the float64 statement.  Returns the worst error / bound (0 where the comparison is bit for bit).
    Rows outside `active` keep their NaN sentinel; words the driver does not store keep it too; aux words nobody owns keep their canary."""
    r = r or ref.run(PRIMS[name]['ref'], case, host_statement)
    rows = [i for i in range(4) if (active >> i) & 1]
    idle = [i for i in range(4) if not (active >> i) & 1]
    tag = '%s [%s, targ %d, ia %s, rows %s] %s' % (name, klass, case.targ, [int(v) for v in case.ia], rows, who)
    assert np.isnan(got_out[idle]).all(), tag + ': a row outside EXEC wrote its output'
    assert _same_bits(got_aux[idle], case.aux[idle]).all(), tag + ': a row outside EXEC wrote global memory'
    assert np.isnan(np.delete(got_out, list(r.out), axis=1)[rows]).all(), tag + ': wrote an output word the primitive does not have'
    assert _same_bits(got_aux[rows], r.aux[rows]).all(), tag + ': global memory differs from the statement (canaries included) at %s' % (np.argwhere(~_same_bits(got_aux[rows], r.aux[rows]))[:4].tolist(),)
    worst = 0.0
    exact = PRIMS[name]['cls'] == MOVES or klass != 'random'
    for word, want in r.out.items():
        got = got_out[rows, word]
        if exact:
            ok = _same_bits(got, want[rows])
            assert ok.all(), tag + ': word %d differs from the statement at (row, lane) %s: got %s, statement %s' % (
                word, np.argwhere(~ok)[:4].tolist(), got[~ok][:4], want[rows][~ok][:4])
        else:
            err = np.abs(got.astype(np.float64) - want[rows])
            b = r.bound[word][rows]
            bad = ~(err <= b)
            assert not bad.any(), tag + ': word %d off the statement by more than its bound at (row, lane) %s: error %s, bound %s' % (
                word, np.argwhere(bad)[:4].tolist(), err[bad][:4], b[bad][:4])
            with np.errstate(invalid='ignore', divide='ignore'):
                worst = max(worst, float(np.nanmax(np.where(b > 0, err / b, 0.0))))
    return worst


def check_bit_equal(name, klass, case, a_out, a_aux, b_out, b_aux, who):
    ok = _same_bits(a_out, b_out)
    assert ok.all(), '%s [%s, targ %d, ia %s] %s: outputs differ at (row, word, lane) %s: %s against %s' % (
        name, klass, case.targ, list(case.ia), who, np.argwhere(~ok)[:4].tolist(), a_out[~ok][:4], b_out[~ok][:4])
    assert _same_bits(a_aux, b_aux).all(), '%s [%s] %s: global memory differs' % (name, klass, who)


def bits_required(name, klass):
    """must two implementations agree bit for bit, in every word, on this class of inputs? (the class table)"""
    return PRIMS[name]['cls'] in (MOVES, SUMS) or klass != 'random'


def words_bit_equal(a_out, b_out):
    """the output words in which two answers are the same bits"""
    return {w for w in range(a_out.shape[1]) if _same_bits(a_out[:, w], b_out[:, w]).all()}


def actives(name):
    return [0b1111, 0b0011, 0b1100] if name == 'peer' else ACTIVE_ROWS       # peer runs only with complete pairs


def host_policies(name):
    return [0] + ([1] if name == 'cone_lds' else []) + ([2] if name == 'gram_pipe' else [])


_CASES, _REFS = {}, {}


def all_cases(name, dims):
    """[(class, Case)] of a primitive: generated once, shared by every test that needs them, never changed"""
    if name not in _CASES:
        _CASES[name] = [(klass, c) for klass in ('exact', 'random', 'edges') for c in cases(name, klass, dims)]
    return _CASES[name]


def hold_to_statement(runner, policy, name, who, host_statement=False):
    """every case of `name` under every active_rows against the float64 statement; returns (worst error / bound on the random class, {(case index, active): (out, aux)})"""
    worst, got = 0.0, {}
    for i, (klass, c) in enumerate(all_cases(name, runner.dims)):
        if (name, i, host_statement) not in _REFS:
            _REFS[name, i, host_statement] = ref.run(PRIMS[name]['ref'], c, host_statement)
        for active in actives(name):
            out, aux = runner.run(policy, PRIMS[name]['id'], c, active)
            got[i, active] = (out, aux)
            worst = max(worst, check_against_reference(name, klass, c, out, aux, active, who, host_statement, _REFS[name, i, host_statement]))
    return worst, got


def with_targ(case, targ):
    import copy
    c = copy.copy(case)
    c.targ = targ
    return c
