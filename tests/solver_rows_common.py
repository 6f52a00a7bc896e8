"""Shared by tests/test_solver_rows_emul.py and tests/test_gpu_solver_rows.py: the entry table of the step kernels' row builders and sweeps (the members of Pmc<L> in
lifelike_agility_and_play_amd/csrc/pmc_step.hpp that turn whitened coefficients into constraint rows and sweep them), their inputs (fixed seeds; every row of a wave gets
different data, so a leak between rows shows), the runners of the host twin and the GPU copies of tests/lanes/solver_rows_body.hpp, and the comparison.
One sample per environment ROW of 16 lanes: [row][word][16 lanes], up to 64 one-wave workgroups (256 rows) a launch.

Classes (those of tests/math_helpers_common.py)
  MOVES   no arithmetic: GPU == host twin == statement, bit for bit
  MADD    multiplies and adds only: equal to the statement's float32 on exact and edge inputs; on random inputs each of GPU and twin within the derived forward bound
          (solver_rows_ref: u (|value| + carried error) per operation, n u sum |t| for a sum whose association the builds choose; a clamp and the cone's scale-back carry it)
  APPROX  a reciprocal or reciprocal square root (1 / nn of contact_row, the cone's scale): the twin within its own bound with each such operation counted as one rounding;
          the GPU within max(4 x dev_host, the multiply-add bound), dev_host = the twin's worst |answer - statement| over the same input class and output word (the rule
          and the reason of math_helpers_common.py)
Input classes
  exact   small integers times 2^-2, one-hot coefficients (so every Gram scalar is a whole number |k| <= 2), inv in {0, 1}, bounds in quarters: every product and every
          partial sum in any association is a float32 (the statements' traces are checked for it).  The cone round only with rows exact by construction: lim = 0, or pairs
          far inside the cone (lim = 2^20: the scale clamps to exactly 1); the contact rows with cvalid false (1 / nn is no float32) -- coefficients, c and zero scalars -- and, among
          the edges, with live contacts built so that |gt|^2 + |jt|^2 = 2: Gram and cross scalars in exact halves.
  random  order-1 normals, 1024 rows, rows built from real gt, jt with inv = 1 / (|gt|^2 + |jt|^2): the system is a Gram matrix, as the kernel meets it.  About a quarter
          of the lanes dead (inv = 0), all four lanes of one leg and a whole row among them.  No float32 intermediate is denormal.
  edges   exact too: a row of all dead lanes; lam = 0 with u < 0 under UNILATERAL (commits exactly zero); hi = 0 with lam != 0 (returns to zero); lim = 0 and a huge lim
          in the cone; cvalid false; the max_tau argument of pd_torque 0 and greater than 0; +-inf and NaN into clip_velocities (they must come out NaN, not a bound).
The sign of a zero: the lane-varying forms negate by `zero - x` and sum products of zeros (a dead row: 0 - inv, gt * 0), which gives +0 where the float64 statement gives -0.
The entries of ZERO_SIGN_FREE are held to the statement's VALUE on exact and edge inputs (+0 == -0); their move words, and every other entry, to its bits.

UNILATERAL and `hi`: gs_round passes `hi` to the turns as the bound of the INCREMENT as it stands (its comment: "a huge constant ... no bound arithmetic"), so a
unilateral round is [0, hi] only for the hi the kernel passes, 3e38.  The unilateral cases pass that; finite bounds are the friction rounds' (<false, false>).
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

import solver_rows_ref as ref
from solver_rows_ref import LANE, LEG, SUB, U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LANES_DIR = os.path.join(ROOT, 'tests', 'lanes')
HOST_LIB = os.path.join(LANES_DIR, '_build', 'libsolver_rows_host.so')
GPU_POLICIES = ['GpuLanes', 'GpuLanes1', 'GpuLanesPmc1Plain', 'WithTurnMasksCmp<GpuLanes>', 'WithTurnMasksCmp<GpuLanesPmc1Plain>', 'WithConeInLds<GpuLanes1>',
                'WithGramPipe<GpuLanesPmc1Plain>']          # = lane_prims_common.GPU_POLICIES
HOST_POLICIES = ['HostLanes', 'WithConeInLdsHost<HostLanes>', 'WithGramPipeHost<HostLanes>']
VARIANTS = ['shipped', 'cone_pipe0', 'mfma_gram1', 'peer_mode1', 'peer_mode2']           # the GPU copies (__graft_entry__.SOLVER_ROWS_VARIANTS)
ACTIVE_ROWS = [0b1111, 0b0011, 0b0100]                       # the whole wave, rows {0, 1}, row {2}: the entry runs under a partial EXEC as in the tail wave of an odd batch
MOVES, MADD, APPROX = 'MOVES', 'MADD', 'APPROX'
ALL7, PIPE = list(range(7)), [6]
RW, ROW_C, ROW_INV, ROW_LAM, ROW_NK = 29, 10, 11, 12, 13     # a Row as it travels: ca[4] cb[2] cj[4] | c | inv | lam | nk[16]  (solver_rows_body.hpp)

# id: SolverRowsEntry of tests/lanes/solver_rows_body.hpp; targs: the template arguments the driver is instantiated for; policies / host: the GPU / host lane policies whose
# code the entry's differs under (kGram16, kGramPipe, kConeInLds, the turn masks), GpuLanes / HostLanes alone otherwise; variants: the builds whose switch reaches the entry
# (LL_MFMA_GRAM: gram4 / gram16; LL_CONE_PIPE: cone_turns4; LL_PEER_MODE reaches none: not built); names: the members of Pmc<L> the entry covers (the coverage scan)
ENTRIES = {
    'permute4': dict(id=0, cls=MOVES, words=4, policies=[0], host=[0], variants=['shipped']),
    'finish_row': dict(id=1, cls=MADD, words=RW, targs=[0, 1], policies=ALL7, host=[0, 2], variants=['shipped', 'mfma_gram1'], moves=list(range(10)) + [ROW_LAM], names=['finish_row', 'permute4']),
    'cross_gram': dict(id=2, cls=MADD, words=16, policies=ALL7, host=[0, 2], variants=['shipped', 'mfma_gram1']),
    'gs_round': dict(id=3, cls=MADD, words=4, targs=[0, 1, 2], policies=ALL7, host=[0, 1, 2], variants=['shipped']),
    'gs_cone_round': dict(id=4, cls=APPROX, words=5, policies=ALL7, host=[0, 1, 2], variants=['shipped', 'cone_pipe0']),
    'contact_rows': dict(id=5, cls=APPROX, words=3 * RW + 32, policies=ALL7, host=[0, 1, 2], variants=['shipped', 'mfma_gram1'], names=['contact_row', 'cross_gram', 'finish_row']),
    'contact_rows_piped': dict(id=5, cls=APPROX, words=3 * RW + 32, targs=[1], policies=PIPE, host=[2], variants=['shipped'], stmt='contact_rows',
                               names=['contact_rows_cone_piped', 'row_coeffs', 'neg_scaled', 'joint_part', 'gram_finish', 'row_perm_a', 'row_perm_b']),
    'compose': dict(id=6, cls=APPROX, words=12, targs=[0, 1], policies=ALL7, host=[0, 1, 2], variants=['shipped', 'cone_pipe0', 'mfma_gram1'],
                    names=['contact_row', 'cross_gram', 'contact_rows_cone_piped', 'gs_round', 'gs_cone_round']),
    'pd': dict(id=7, cls=MADD, words=6, policies=[0], host=[0], variants=['shipped'], names=['pd_target', 'pd_torque']),
    'clip_velocities': dict(id=8, cls=MOVES, words=9, policies=[0], host=[0], variants=['shipped']),
    'pick_rank': dict(id=9, cls=MOVES, words=3, targs=[0, 1, 2, 3], policies=[0], host=[0], variants=['shipped']),
    'self_row': dict(id=10, cls=APPROX, words=11, targs=[0, 1], policies=[0], host=[0], variants=['shipped'],
                     names=['self_row_build', 'self_row_pack', 'self_row_clear', 'self_row_velocity', 'self_row_apply', 'self_turn', 'self_fric_turn']),
    'self_pieces': dict(id=10, cls=MADD, words=13, targs=[2], policies=[0], host=[0], variants=['shipped'], names=['self_row_pack', 'self_row_velocity', 'self_row_apply', 'self_row_clear'],
                        moves=[0, 1, 2, 7, 8, 9, 10, 11, 12]),
    'pair_row': dict(id=11, cls=APPROX, words=11, targs=[0, 1], policies=[0], host=[0], variants=['shipped', 'peer_mode1', 'peer_mode2'], actives=[0b1111, 0b0011, 0b1100],
                     names=['pair_row_build', 'pair_turn', 'pair_fric_turn']),
    'cand_eval_point': dict(id=12, cls=APPROX, words=4, policies=[0], host=[0], variants=['shipped']),
}
for _k, _v in ENTRIES.items():
    _v.setdefault('targs', [0]); _v.setdefault('names', [_k]); _v.setdefault('moves', []); _v.setdefault('stmt', _k); _v.setdefault('actives', ACTIVE_ROWS)
ZERO_SIGN_FREE = {'finish_row', 'cross_gram', 'gs_round', 'gs_cone_round', 'contact_rows', 'contact_rows_piped', 'compose', 'self_row', 'self_pieces', 'pair_row', 'cand_eval_point'}
GS_TARGS = {0: (True, True), 1: (False, True), 2: (False, False)}      # gs_round<LIMIT, UNILATERAL>: the three the kernel instantiates
# The members of Pmc<L> this layer is asked to hold (the coverage scan of test_solver_rows_emul.py: each is defined in pmc_step.hpp, named by an entry, called by the driver) ...
PMC_MEMBERS = ['permute4', 'finish_row', 'cross_gram', 'contact_row', 'row_coeffs', 'neg_scaled', 'joint_part', 'gram_finish', 'row_perm_a', 'row_perm_b',
               'contact_rows_cone_piped', 'gs_round', 'gs_cone_round', 'pd_target', 'pd_torque', 'clip_velocities', 'pick_rank', 'self_row_clear', 'self_row_pack',
               'self_row_velocity', 'self_row_apply', 'self_turn', 'self_fric_turn', 'self_row_build', 'pair_row_build', 'pair_turn', 'pair_fric_turn', 'cand_eval_point']
# ... and what stays for a later layer, each with the reason
# (the terrain-edge detectors leg_edge / reverse_edge and one slot of the leg-leg pick, self_pick, are held in contact_scan_common.py, which also lists what is still open
#  there: the deepest-K selection of the ground contacts)
LATER = {
    'substep_impl': 'the candidate scan, contact selection and the composition of the rounds: held end to end by the step parity tests',
}


class Dims:
    def __init__(self, lib):
        d = (C.c_int * 16)()
        lib.ll_solver_rows_dims(d)
        self.n_in, self.n_out, self.max_blocks, self.n_consts, self.n_policies, self.cone_pipe, self.mfma_gram, self.n_entries, self.peer_mode = list(d)[:9]
        self.consts = np.zeros(self.n_consts, dtype=np.float32)          # no entry reads the tables
        self.consts[-1] = 1.0


class Case:
    def __init__(self, klass, X, targ=0, note=None):
        self.klass, self.targ, self.note = klass, targ, note
        self.X = np.ascontiguousarray(X, dtype=np.float32)                # [rows, words, 16]; rows a multiple of 4
        assert self.X.shape[0] % 4 == 0 and self.X.shape[2] == 16
        self.n = self.X.shape[0]


def _bind(path):
    lib = C.CDLL(path)
    lib.ll_solver_rows_dims.argtypes = [C.POINTER(C.c_int)]
    lib.ll_solver_rows_run.restype = C.c_int
    lib.ll_solver_rows_run.argtypes = [C.c_int] * 5 + [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_long]
    return lib


class HostRunner:
    def __init__(self):
        subprocess.check_call(['make', '-C', LANES_DIR, '-s'])
        self.lib = _bind(HOST_LIB)
        self.dims = Dims(self.lib)

    def launch(self, policy, eid, targ, n_blocks, active, w, out, consts):
        return self.lib.ll_solver_rows_run(policy, eid, targ, n_blocks, active, w.ctypes.data, w.size, out.ctypes.data, out.size, consts.ctypes.data, consts.size)

    def run(self, policy, name, case, active=0b1111, limit=None):
        """-> [rows, n_out, 16] float32; rows outside `active` (and every word never written) stay NaN"""
        d = self.dims
        X = case.X if limit is None else case.X[:limit]
        res = []
        for i in range(0, len(X), 4 * d.max_blocks):
            w = np.zeros((min(4 * d.max_blocks, len(X) - i), d.n_in, 16), dtype=np.float32)
            w[:, :X.shape[1]] = X[i:i + 4 * d.max_blocks]
            out = np.full((len(w), d.n_out, 16), np.nan, dtype=np.float32)
            rc = self.launch(policy, ENTRIES[name]['id'], case.targ, len(w) // 4, active, w, out, d.consts)
            assert rc == 0, (name, rc)
            res.append(out)
        return np.concatenate(res)


class GpuRunner(HostRunner):
    """One launch per run() chunk on the default stream, synchronised; torch only holds the device buffers."""
    def __init__(self, path, host_dims):
        import torch
        self.torch = torch
        self.lib = _bind(path)
        self.dims = Dims(self.lib)
        assert (self.dims.n_in, self.dims.n_out, self.dims.n_consts, self.dims.max_blocks, self.dims.n_entries) == (host_dims.n_in, host_dims.n_out, host_dims.n_consts, host_dims.max_blocks, host_dims.n_entries)

    def launch(self, policy, eid, targ, n_blocks, active, w, out, consts):
        t = self.torch
        dw, dout, dc = (t.from_numpy(x).to('cuda:0') for x in (w, out, consts))
        t.cuda.synchronize()
        rc = self.lib.ll_solver_rows_run(policy, eid, targ, n_blocks, active, dw.data_ptr(), dw.numel(), dout.data_ptr(), dout.numel(), dc.data_ptr(), dc.numel())
        try:
            t.cuda.synchronize()
            out[:] = dout.cpu().numpy()
        except RuntimeError as e:          # a launch that faulted: nothing more is started on this device
            import pytest
            pytest.exit('the solver rows launch (policy %d, entry %d, targ %d) failed: %s' % (policy, eid, targ, e), returncode=3)
        return rc


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------------------
N_RANDOM, N_EXACT = 1024, 64


def _rng(name, klass, targ): return np.random.default_rng([ENTRIES[name]['id'], ['exact', 'random', 'edges'].index(klass), targ])


def _rnd(r, shape):
    x = r.standard_normal(shape).astype(np.float32)
    return np.where(np.abs(x) < 2.0 ** -10, np.float32(0.5), x)          # nothing whose product with another operand could go denormal


def _quarters(r, shape, lim=8): return (r.integers(-lim, lim + 1, size=shape) * 0.25).astype(np.float32)


def _one_hot(r, shape, n, p_zero=0.0):
    """one +-1 among the last n coefficients (or none)"""
    x = np.zeros(shape + (n,), dtype=np.float32)
    idx = r.integers(0, n, size=shape)
    np.put_along_axis(x, idx[..., None], r.choice([-1.0, 1.0], size=shape + (1,)).astype(np.float32), axis=-1)
    return x * (r.random(shape + (1,)) >= p_zero)


def _dead_mask(r, R):
    """about a quarter of the lanes: scattered ones, all four lanes of one leg in every eighth row, a whole row in every sixteenth"""
    dead = r.random((R, 16)) < 0.18
    rows = np.arange(R)
    dead[(rows % 8 == 1)[:, None] & (LEG[None, :] == (rows[:, None] // 8) % 4)] = True
    dead[rows % 16 == 2] = True
    return dead


def row_set(r, klass, R, all_dead=False):
    """gt [R, 16, 6], jt [R, 16, 3], inv [R, 16] as float32"""
    if klass == 'random':
        gt, jt = _rnd(r, (R, 16, 6)), _rnd(r, (R, 16, 3))
        inv = (1.0 / ((gt.astype(np.float64) ** 2).sum(-1) + (jt.astype(np.float64) ** 2).sum(-1))).astype(np.float32)
        dead = _dead_mask(r, R)
    else:
        gt, jt = _one_hot(r, (R, 16), 6), _one_hot(r, (R, 16), 3, p_zero=0.5)
        inv = np.ones((R, 16), dtype=np.float32)
        dead = r.random((R, 16)) < 0.25
        dead[np.arange(R) % 8 == 3] = True
    if all_dead:
        dead[:] = True
    return gt, jt, np.where(dead, np.float32(0.0), inv)


def velocity(r, klass, R):
    dx = _rnd(r, (R, 6)) if klass == 'random' else _quarters(r, (R, 6), 4)
    dq = _rnd(r, (R, 4, 4)) if klass == 'random' else _quarters(r, (R, 4, 4), 4)
    return dx, dq


def row_words(gt, jt, c, inv, lam, nk, limit=False):
    """a finished Row as the driver reads it: [R, RW, 16]; nk [R, 16 (m), 16 (L)] float64, rounded to float32 here.  LIMIT: the scalars of lanes 3, 7, 11, 15 are not
    formed -- NaN in their place, which nothing may read"""
    W = np.zeros((len(gt), RW, 16), dtype=np.float32)
    W[:, :10] = ref.permuted(gt, jt)
    W[:, ROW_C], W[:, ROW_INV], W[:, ROW_LAM] = c, inv, lam
    W[:, ROW_NK:] = nk.transpose(0, 2, 1).astype(np.float32)
    if limit:
        W[:, ROW_NK + 3::4] = np.nan
    return W


def f64(*xs): return [np.asarray(x, dtype=np.float64) for x in xs]


def unit_frames(r, R):
    """orthonormal (un, ut1, ut2) per lane, rounded to float32"""
    a, b = r.standard_normal((R, 16, 3)), r.standard_normal((R, 16, 3))
    un = a / np.linalg.norm(a, axis=-1, keepdims=True)
    t1 = np.cross(un, b); t1 /= np.linalg.norm(t1, axis=-1, keepdims=True)
    return un, t1, np.cross(un, t1)


def draw_factors(r, R):
    """a random symmetric positive definite mass matrix with the kernel's block structure (base 6 x 6, four legs 3 x 3, base-leg couplings, no leg-leg block), factored in
    float64 into LegFactor, Sb, Sd and rounded to float32  -> lf [R, 4, 27], Sb [R, 21], Sd [R, 6] float32 (M itself is then what these reconstruct: ref.mass_matrix)"""
    lf0, Sb0 = np.zeros((R, 4, 27)), 0.2 * r.standard_normal((R, 21))
    lf0[:, :, [1, 2, 4]] = 0.3 * r.standard_normal((R, 4, 3))
    lf0[:, :, 6:9] = 1.0 / r.uniform(0.7, 1.4, size=(R, 4, 3))
    lf0[:, :, 9:27] = 0.2 * r.standard_normal((R, 4, 18))
    M = ref.mass_matrix(lf0, Sb0, 1.0 / r.uniform(0.7, 1.4, size=(R, 6)))
    assert (np.linalg.eigvalsh(M) > 1e-3).all()
    lf, S = np.zeros((R, 4, 27)), M[:, :6, :6].copy()
    for leg in range(4):
        s = slice(6 + 3 * leg, 9 + 3 * leg)
        Lm = np.linalg.cholesky(M[:, s, s])
        Y = np.linalg.solve(Lm, M[:, s, :6]).transpose(0, 2, 1)          # M_bl Lm^-T
        S -= Y @ Y.transpose(0, 2, 1)
        lf[:, leg, 0:6] = np.stack([Lm[:, 0, 0], Lm[:, 1, 0], Lm[:, 2, 0], Lm[:, 1, 1], Lm[:, 2, 1], Lm[:, 2, 2]], axis=1)
        lf[:, leg, 6:9] = 1.0 / np.stack([Lm[:, 0, 0], Lm[:, 1, 1], Lm[:, 2, 2]], axis=1)
        lf[:, leg, 9:27] = Y.transpose(0, 2, 1).reshape(R, 18)
    Lb = np.linalg.cholesky(S)
    Sb = np.stack([Lb[:, i, k] for i in range(6) for k in range(i + 1)], axis=1)
    return lf.astype(np.float32), Sb.astype(np.float32), (1.0 / Lb[:, range(6), range(6)]).astype(np.float32)


def cases(name, dims):
    """[Case] of an entry: exact, random, edges for each of its targs (fixed seed per (entry, class, targ))"""
    out = []
    stmt = ENTRIES[name]['stmt']
    for targ in ENTRIES[name]['targs']:
        for klass in ('exact', 'random', 'edges'):
            r = _rng(stmt, klass, 0 if stmt == 'contact_rows' else targ)          # (the piped form gets the inputs of the plain one: the two are compared)
            R = N_RANDOM if klass == 'random' else N_EXACT
            val = (lambda shape: _rnd(r, shape)) if klass == 'random' else (lambda shape: _quarters(r, shape))
            if stmt == 'permute4':
                if klass != 'edges':
                    out.append(Case(klass, val((R, 4, 16)), targ))
            elif stmt == 'finish_row':
                if klass == 'edges':
                    gt, jt, inv = row_set(r, 'exact', R, all_dead=True)
                else:
                    gt, jt, inv = row_set(r, klass, R)
                X = np.concatenate([gt.transpose(0, 2, 1), jt.transpose(0, 2, 1), inv[:, None]], axis=1)
                out.append(Case(klass, X, targ))
            elif stmt == 'cross_gram':
                gm, jm, inv = row_set(r, 'exact' if klass == 'edges' else klass, R, all_dead=klass == 'edges')
                go, jo, _ = row_set(r, 'exact' if klass == 'edges' else klass, R)
                X = np.concatenate([gm.transpose(0, 2, 1), jm.transpose(0, 2, 1), inv[:, None], go.transpose(0, 2, 1), jo.transpose(0, 2, 1)], axis=1)
                out.append(Case(klass, X, targ))
            elif stmt == 'gs_round':
                limit, uni = GS_TARGS[targ]
                for note in {'exact': ['plain'], 'random': ['plain'], 'edges': ['all dead', 'lam = 0, u < 0', 'hi = 0, lam != 0'][:3 if not uni else 2]}[klass]:
                    gt, jt, inv = row_set(r, 'exact' if klass == 'edges' else klass, R, all_dead=note == 'all dead')
                    c, (dx, dq) = val((R, 16)), velocity(r, klass, R)
                    if uni:
                        hi, lam = np.full((R, 16), ref.BIG, dtype=np.float32), np.abs(val((R, 16)))
                    else:
                        hi = (np.abs(val((R, 16))) + np.float32(0.25)).astype(np.float32)
                        lam = np.clip(val((R, 16)), -hi, hi)
                    if limit and klass == 'edges':
                        inv[:, 3::4] = 0.0                   # sub-lane 3 holds no row (the random class leaves rows there: nothing may take their turns)
                    if note == 'lam = 0, u < 0':            # a free velocity that pushes every row apart, nothing to give back: every turn commits exactly zero
                        lam[:] = 0.0
                        dx[:], dq[:] = 0.0, 0.0
                        c = np.abs(c) + np.float32(0.25)
                        if not uni:
                            hi[:] = 0.0
                    if note == 'hi = 0, lam != 0':
                        hi[:] = 0.0
                        lam = np.where(lam == 0, np.float32(0.5), val((R, 16)))
                    nk = ref.gram(*f64(gt, jt, inv, gt, jt))
                    VA, VB, VJ = ref.scatter_velocity(dx, dq)
                    X = np.concatenate([row_words(gt, jt, c, inv, lam, nk, limit), hi[:, None], VA[:, None], VB[:, None], VJ[:, None]], axis=1)
                    out.append(Case(klass, X, targ, note))
            elif stmt == 'gs_cone_round':
                for note in {'exact': ['plain'], 'random': ['plain'], 'edges': ['all dead', 'lim = 0', 'huge lim']}[klass]:
                    sub = 'exact' if klass == 'edges' else klass
                    g1, j1, inv1 = row_set(r, sub, R, all_dead=note == 'all dead')
                    g2, j2, inv2 = row_set(r, sub, R)
                    live2 = np.ones((R, 16)) if sub == 'exact' else 1.0 / ((g2.astype(np.float64) ** 2).sum(-1) + (j2.astype(np.float64) ** 2).sum(-1))
                    inv2 = np.where(inv1 == 0, 0.0, live2).astype(np.float32)          # a contact without cvalid has none of its three rows
                    c1, c2, (dx, dq) = val((R, 16)), val((R, 16)), velocity(r, klass, R)
                    rows = np.arange(R)[:, None]
                    if klass == 'random':
                        lim = r.uniform(0.2, 2.0, size=(R, 16)).astype(np.float32)          # pairs inside and outside the cone
                        lim[r.random((R, 16)) < 0.1] = 0.0
                        l1, l2 = _rnd(r, (R, 16)), _rnd(r, (R, 16))
                        s = np.minimum(1.0, lim * r.uniform(0.0, 1.0, size=(R, 16)) / np.hypot(l1, l2))
                        lam1, lam2 = (l1 * s).astype(np.float32), (l2 * s).astype(np.float32)
                    else:                                    # rows exact by construction: lim = 0 | far inside the cone | both side by side
                        lim = np.where(rows % 3 == 0, 0.0, np.where(rows % 3 == 1, 2.0 ** 20, np.where(LANE[None, :] % 3 == 0, 0.0, 2.0 ** 20))).astype(np.float32)
                        lam1, lam2 = val((R, 16)), val((R, 16))
                        if note == 'lim = 0':
                            lim[:] = 0.0
                        if note == 'huge lim':
                            lim[:] = 2.0 ** 100
                    k11, k12 = ref.gram(*f64(g1, j1, inv1, g1, j1)), ref.gram(*f64(g1, j1, inv1, g2, j2))
                    k21, k22 = ref.gram(*f64(g2, j2, inv2, g1, j1)), ref.gram(*f64(g2, j2, inv2, g2, j2))
                    VA, VB, VJ = ref.scatter_velocity(dx, dq)
                    X = np.concatenate([row_words(g1, j1, c1, inv1, lam1, k11), row_words(g2, j2, c2, inv2, lam2, k22), k12.transpose(0, 2, 1).astype(np.float32),
                                        k21.transpose(0, 2, 1).astype(np.float32), lim[:, None], VA[:, None], VB[:, None], VJ[:, None]], axis=1)
                    out.append(Case(klass, X, targ, note))
            elif stmt in ('contact_rows', 'compose'):
                X = np.zeros((R, 87 if stmt == 'compose' else 86, 16), dtype=np.float32)
                uni = lambda x: np.repeat(x[:, :, None], 16, axis=2)      # env-uniform words: every lane its copy
                if klass == 'random':
                    X[:, 0:3], X[:, 3:6], X[:, 6:9] = (u.transpose(0, 2, 1) for u in unit_frames(r, R))
                    X[:, 9:21] = 0.3 * _rnd(r, (R, 12, 16))                                   # Pb, d1, d2, d3: lever arms of a leg
                    ldiag = r.uniform(0.5, 1.5, size=(R, 3, 16)).astype(np.float32)
                    X[:, [21, 24, 26]] = ldiag
                    X[:, [22, 23, 25]] = 0.2 * _rnd(r, (R, 3, 16))
                    X[:, 27:30] = (1.0 / ldiag.astype(np.float64)).astype(np.float32)
                    X[:, 30:48] = 0.2 * _rnd(r, (R, 18, 16))
                    X[:, 48:52] = _rnd(r, (R, 4, 16))                                         # qs, bias
                    X[:, 52] = r.random((R, 16)) < 0.75
                    X[:, 53:74] = uni(0.2 * _rnd(r, (R, 21)))
                    X[:, 74:80] = uni((1.0 / r.uniform(0.5, 1.5, size=(R, 6))).astype(np.float32))
                    X[:, 80:86] = uni(_rnd(r, (R, 6)))
                else:                                        # whole numbers, unit diagonals; cvalid false: 1 / nn is no float32 (edges: the same with a zero direction too)
                    X[:, 0:9] = r.integers(-1, 2, size=(R, 9, 16))
                    X[:, 9:21] = r.integers(-2, 3, size=(R, 12, 16))
                    X[:, [21, 24, 26]] = 1.0
                    X[:, [22, 23, 25]] = r.integers(-1, 2, size=(R, 3, 16))
                    X[:, 27:30] = 1.0
                    X[:, 30:48] = r.integers(-1, 2, size=(R, 18, 16))
                    X[:, 48:52] = _quarters(r, (R, 4, 16), 4)
                    X[:, 52] = 0.0
                    X[:, 53:74] = uni(r.integers(-1, 2, size=(R, 21)).astype(np.float32))
                    X[:, 74:80] = 1.0
                    X[:, 80:86] = uni(_quarters(r, (R, 6), 4))
                    if klass == 'edges':
                        X[::2, 3:6] = 0.0
                        if stmt == 'contact_rows':       # odd rows: LIVE contacts whose Gram scalars are exact -- axis directions at the origin, unit factors, no coupling,
                            o = X[1::2]                  # lever arms along axes: gt = [0; u], jt one-hot, |gt|^2 + |jt|^2 = 2, inv = 1 / 2, every scalar a multiple of 1 / 2
                            n, ax3 = len(o), np.eye(3, dtype=np.float32)
                            turn, turn_d = r.integers(0, 3, size=(n, 16)), r.integers(0, 3, size=(n, 16))
                            for k in range(3):
                                o[:, 3 * k:3 * k + 3] = (ax3[(turn + k) % 3] * r.choice([-1.0, 1.0], size=(n, 16, 1))).transpose(0, 2, 1)
                                o[:, 12 + 3 * k:15 + 3 * k] = (ax3[(turn_d + k) % 3] * r.choice([-1.0, 1.0], size=(n, 16, 1))).transpose(0, 2, 1)
                            o[:, 9:12], o[:, 22:24], o[:, 25], o[:, 30:48], o[:, 53:74] = 0.0, 0.0, 0.0, 0.0, 0.0
                            o[:, 52] = r.random((n, 16)) < 0.8
                            X[1::2] = o
                if stmt == 'compose':
                    X[:, 86] = 0.5
                    if klass == 'random':                # leg-uniform factors of ONE mass matrix per row, leg-uniform joint rates, a friction coefficient per lane
                        lf, Sb, Sd = draw_factors(r, R)
                        X[:, 21:48] = np.repeat(lf, 4, axis=1).transpose(0, 2, 1)
                        X[:, 53:74], X[:, 74:80] = uni(Sb), uni(Sd)
                        X[:, 48:51] = np.repeat(_rnd(r, (R, 4, 3)), 4, axis=1).transpose(0, 2, 1)
                        X[:, 86] = r.uniform(0.3, 1.0, size=(R, 16))
                        # a few contacts a row, as the kernel meets them (sixteen live contacts are 48 rows on 18 degrees of freedom: the sweep is as right as ever, but
                        # a forward bound carried through 32 strongly coupled turns says nothing any more)
                        X[:, 52] = r.random((R, 16)) < 0.25
                        X[np.arange(R) % 16 == 5, 52] = 0.0
                        X[:, 86][r.random((R, 16)) < 0.1] = 0.0
                    elif klass == 'edges':
                        X[:, 86] = 0.0
                out.append(Case(klass, X, targ))
            elif stmt == 'pd':
                X = np.zeros((R, 13, 16), dtype=np.float32)
                uni = lambda x: np.repeat(x[:, None], 16, axis=1)
                if klass == 'random':
                    X[:, 0:9] = _rnd(r, (R, 9, 16)) * np.array([1.5] * 6 + [6.0] * 3, dtype=np.float32)[None, :, None]      # q + act on both sides of +-3
                    X[:, 9], X[:, 10], X[:, 11] = uni(r.uniform(20, 60, R)), uni(r.uniform(0.5, 2.0, R)), uni(r.uniform(10, 30, R))
                    X[:, 12] = uni(np.where(np.arange(R) % 2 == 0, 0.0, r.uniform(10, 30, R)))
                else:
                    X[:, 0:9] = _quarters(r, (R, 9, 16), 10)
                    X[:, 9], X[:, 10], X[:, 11] = uni(r.integers(1, 5, R) * 1.0), uni(r.integers(0, 3, R) * 0.5), uni(r.integers(1, 9, R) * 1.0)
                    X[:, 12] = uni(np.where(np.arange(R) % 2 == 0, 0.0, r.integers(1, 9, R) * 0.5)) if klass == 'edges' else 0.0
                out.append(Case(klass, X, targ))
            elif stmt == 'clip_velocities':
                X = np.zeros((R, 10, 16), dtype=np.float32)
                X[:, 0:3] = 3 * val((R, 3, 16))
                X[:, 3:9] = np.repeat(3 * val((R, 6))[:, :, None], 16, axis=2)
                X[:, 9] = np.repeat((np.abs(val((R,))) + np.float32(0.5))[:, None], 16, axis=1)
                if klass == 'edges':
                    bad = np.array([np.inf, -np.inf, np.nan], dtype=np.float32)
                    X[:, 0:3][r.random((R, 3, 16)) < 0.3] = bad[r.integers(0, 3)]
                    X[:, 0, 0::5], X[:, 1, 1::5], X[:, 2, 2::5] = bad[0], bad[1], bad[2]
                    X[0::3, 3 + (np.arange(len(X[0::3])) % 6)] = bad[np.arange(len(X[0::3])) % 3][:, None]
                out.append(Case(klass, X, targ))
            elif stmt == 'pick_rank':
                if klass != 'edges':
                    X = np.zeros((R, 8, 16), dtype=np.float32)
                    X[:, 0] = np.argsort(r.random((R, 4, 4)), axis=2).reshape(R, 16)          # a ranking of the leg's four candidates
                    X[:, 1] = SUB[None, :]                                                     # ... of which sub-lane s takes the one of rank s
                    X[:, 2:8] = val((R, 6, 16))
                    out.append(Case(klass, X, targ))
            elif stmt in ('self_row', 'pair_row'):
                pair = stmt == 'pair_row'
                X = np.zeros((R, 92 if pair else 77, 16), dtype=np.float32)
                leg = lambda x: np.repeat(x, 4, axis=1).transpose(0, 2, 1) if x.ndim == 3 else np.repeat(x, 4, axis=1)      # [R, 4, w] -> [R, w, 16]: every sub-lane its leg's copy
                uni = lambda x: np.repeat(x[..., None], 16, axis=-1)
                arena = lambda x: np.repeat(x[0::2], 2, axis=0) if pair else x                                        # the same in both rows of an arena
                o = dict(ub=0, e=7, lf=16, qs=43, Sb=46, Sd=67, V=88, have=85, hi=86, lam0=91) if pair else dict(ub=0, e=4, lf=13, qs=40, Sb=43, Sd=64, V=73, have=71, hi=72, lam0=76)
                rnd = klass == 'random'
                if rnd:
                    ub = r.standard_normal((R, 3)); ub /= np.linalg.norm(ub, axis=1, keepdims=True)
                    lf, Sb, Sd = draw_factors(r, R)
                    e, qs = 0.3 * _rnd(r, (R, 4, 9)), _rnd(r, (R, 4, 3))
                else:
                    ub = r.integers(-1, 2, size=(R, 3)).astype(np.float32)
                    lf = np.zeros((R, 4, 27), dtype=np.float32)
                    lf[:, :, [0, 3, 5, 6, 7, 8]] = 1.0
                    lf[:, :, [1, 2, 4]] = r.integers(-1, 2, size=(R, 4, 3))
                    lf[:, :, 9:27] = r.integers(-1, 2, size=(R, 4, 18))
                    Sb, Sd = r.integers(-1, 2, size=(R, 21)).astype(np.float32), np.ones((R, 6), dtype=np.float32)
                    e, qs = r.integers(-2, 3, size=(R, 4, 9)).astype(np.float32), _quarters(r, (R, 4, 3), 4)
                X[:, o['ub']:o['ub'] + 3] = uni(ub)
                X[:, o['e']:o['e'] + 9], X[:, o['lf']:o['lf'] + 27], X[:, o['qs']:o['qs'] + 3] = leg(e), leg(lf), leg(qs)
                X[:, o['Sb']:o['Sb'] + 21], X[:, o['Sd']:o['Sd'] + 6] = uni(Sb), uni(Sd)
                own = r.integers(0, 4, size=R)
                if pair:
                    X[:, 3:6] = uni(0.3 * _rnd(r, (R, 3)) if rnd else r.integers(-2, 3, size=(R, 3)).astype(np.float32))
                    X[:, 6] = LEG[None, :] == own[:, None]
                    X[:, 73:79] = uni(_rnd(r, (R, 6)) if rnd else _quarters(r, (R, 6), 4))
                    X[:, 79], X[:, 80], X[:, 81], X[:, 82] = 0.25, 0.75, -0.03125, 4.0                                   # erp, erp_deep, erp_deep_below, max_depen
                    X[:, 83] = uni(arena((0.05 * r.standard_normal(R)).astype(np.float32) if rnd else _quarters(r, (R,), 2) / 4))
                    X[:, 84] = 512.0 if rnd else 2.0
                    X[:, 87] = (np.arange(R) % 2)[:, None]
                else:
                    other = (own + r.integers(1, 4, size=R)) % 4
                    X[:, 3] = (LEG[None, :] == own[:, None]) * 1.0 - (LEG[None, :] == other[:, None]) * 1.0
                    X[:, 70] = uni(_rnd(r, (R,)) if rnd else _quarters(r, (R,), 4))
                have = arena(r.random(R) < 0.85) if rnd else np.zeros(R, dtype=bool)      # exact and edges: have == false -- a cleared row, and a turn on it that changes nothing
                X[:, o['have']] = have[:, None]
                hi = arena(np.abs(_rnd(r, (R,))) if rnd else np.abs(_quarters(r, (R,), 4)))
                if rnd:
                    hi[np.arange(R) % 16 < 2] = 0.0
                lam0 = arena(_rnd(r, (R,)) if rnd else _quarters(r, (R,), 4))
                lam0 = np.clip(lam0, -hi, hi) if targ == 1 else np.abs(lam0)
                if klass == 'edges':
                    lam0[:] = 0.0
                X[:, o['hi']], X[:, o['lam0']] = uni(hi.astype(np.float32)), uni(lam0.astype(np.float32))
                dx, dq = velocity(r, klass, R)
                X[:, o['V']], X[:, o['V'] + 1], X[:, o['V'] + 2] = ref.scatter_velocity(dx, dq)
                out.append(Case(klass, X, targ))
            elif stmt == 'self_pieces':
                if klass != 'edges':
                    X = np.zeros((R, 13, 16), dtype=np.float32)
                    X[:, 0:3] = np.repeat(val((R, 4, 3)), 4, axis=1).transpose(0, 2, 1)
                    X[:, 3:10] = np.repeat(val((R, 7))[:, :, None], 16, axis=2)
                    dx, dq = velocity(r, klass, R)
                    X[:, 10], X[:, 11], X[:, 12] = ref.scatter_velocity(dx, dq)
                    out.append(Case(klass, X, targ))
            elif stmt == 'cand_eval_point':
                X = np.zeros((R, 36, 16), dtype=np.float32)
                uni = lambda x: np.repeat(x[..., None], 16, axis=-1)
                capsule = r.random((R, 16)) < 0.5
                if klass == 'random':                    # spheres (no axis: ax = 0, len far below the switch) and capsules (unit axis; len at least 1e-4, or at most 1e-8)
                    rot = lambda shape: np.linalg.qr(r.standard_normal(shape + (3, 3)))[0]
                    X[:, 0:3], X[:, 3:12] = uni(_rnd(r, (R, 3))), uni(rot((R,)).reshape(R, 9))
                    X[:, 12:21] = rot((R, 16)).reshape(R, 16, 9).transpose(0, 2, 1)
                    X[:, 21:24], X[:, 27:30] = 0.3 * _rnd(r, (R, 3, 16)), 0.1 * _rnd(r, (R, 3, 16))
                    ax, ez = (x / np.linalg.norm(x, axis=-1, keepdims=True) for x in (r.standard_normal((R, 16, 3)), r.standard_normal((R, 16, 3))))
                    ax, ez = ax.astype(np.float32).astype(np.float64), ez.astype(np.float32).astype(np.float64)
                    az = (ax * ez).sum(-1).astype(np.float32).astype(np.float64)
                    ln_ = np.linalg.norm(ez - az[..., None] * ax, axis=-1)
                    short = (r.random((R, 16)) < 0.2) | (ln_ < 1e-2)
                    ln_ = np.where(short | ~capsule, 1e-8 * r.uniform(0.01, 1.0, size=(R, 16)), ln_)
                    X[:, 24:27], X[:, 30:33] = ez.transpose(0, 2, 1), (ax * capsule[..., None]).transpose(0, 2, 1)
                    X[:, 33], X[:, 34], X[:, 35] = r.uniform(0.01, 0.05, size=(R, 16)), az * capsule, ln_
                else:                                    # whole numbers and quarters, signed permutations as rotations, len 1 (1 / len exact) or 2^-30 (below the switch)
                    perm = lambda shape: np.eye(3)[np.argsort(r.random(shape + (3,)), axis=-1)] * r.choice([-1.0, 1.0], size=shape + (3, 1))
                    X[:, 0:3], X[:, 3:12] = uni(_quarters(r, (R, 3))), uni(perm((R,)).reshape(R, 9))
                    X[:, 12:21] = perm((R, 16)).reshape(R, 16, 9).transpose(0, 2, 1)
                    X[:, 21:24], X[:, 24:27], X[:, 27:30] = _quarters(r, (R, 3, 16)), r.integers(-1, 2, size=(R, 3, 16)), _quarters(r, (R, 3, 16))
                    X[:, 30] = capsule
                    X[:, 33], X[:, 34] = np.abs(_quarters(r, (R, 16))) + 0.25, r.integers(-1, 2, size=(R, 16))
                    X[:, 35] = np.where(r.random((R, 16)) < 0.5, 1.0, 2.0 ** -30)
                out.append(Case(klass, X, targ))
            else:
                raise KeyError(name)
    return out


# ---- what the statement says of a case -----------------------------------------------------------------------------------------------------------------------
_WANT = {}


def decode_row(X, w0):
    """a Row's words back into gt [R, 16, 6], jt [R, 16, 3], c, inv, lam (the permutation undone: ca[0] = gt[sub], ...)"""
    R = len(X)
    gt, jt = np.zeros((R, 16, 6)), np.zeros((R, 16, 3))
    for k in range(4):
        gt[:, LANE, SUB ^ k] = X[:, w0 + k]
    for k in range(2):
        gt[:, LANE, 4 + ((SUB ^ k) & 1)] = X[:, w0 + 4 + k]
    for k in range(4):
        keep = (SUB ^ k) < 3
        jt[:, LANE[keep], (SUB ^ k)[keep]] = X[:, w0 + 6 + k][:, keep]
    return gt, jt, X[:, w0 + ROW_C], X[:, w0 + ROW_INV], X[:, w0 + ROW_LAM]


def rare_inputs(X, pair):
    o = dict(ub=0, e=7, lf=16, qs=43, Sb=46, Sd=67, V=88, have=85, hi=86, lam0=91) if pair else dict(ub=0, e=4, lf=13, qs=40, Sb=43, Sd=64, V=73, have=71, hi=72, lam0=76)
    L = lambda a, n: X[:, a:a + n, 0::4].transpose(0, 2, 1)          # a leg-uniform word group -> [R, 4, n]
    I = dict(ub=X[:, 0:3, 0], e=L(o['e'], 9).reshape(len(X), 4, 3, 3), lf=L(o['lf'], 27), qs=L(o['qs'], 3), Sb=X[:, o['Sb']:o['Sb'] + 21, 0], Sd=X[:, o['Sd']:o['Sd'] + 6, 0],
             V=(X[:, o['V']], X[:, o['V'] + 1], X[:, o['V'] + 2]), have=X[:, o['have'], 0] > 0.5, hi=X[:, o['hi'], 0], lam0=X[:, o['lam0'], 0])
    if pair:
        I.update(pb=X[:, 3:6, 0], jsel=(X[:, 6, 0::4] > 0.5) * 1.0, xi=X[:, 73:79, 0])
    else:
        I['jsel'] = X[:, 3, 0::4]
    return I


def contact_inputs(X):
    T = lambda a, b: X[:, a:b].transpose(0, 2, 1)
    d = np.stack([T(12, 15), T(15, 18), T(18, 21)], axis=2)
    return dict(us=[T(0, 3), T(3, 6), T(6, 9)], Pb=T(9, 12), d=d, lf=T(21, 48), qs=T(48, 51), bias=X[:, 51], cvalid=X[:, 52] > 0.5, Sb=X[:, 53:74, 0], Sd=X[:, 74:80, 0], xi=X[:, 80:86, 0])


def _put(v, e, word, x):
    v[:, word], e[:, word] = x.v, x.e


def statement(name, case, **wrong):
    """-> v [rows, words, 16] float64: what the entry's stored words should hold (NaN: a word the driver does not store); `wrong`: the statement's switches"""
    h = ENTRIES[name]
    stmt = h['stmt']
    X = case.X.astype(np.float64)
    R = len(X)
    v = np.full((R, h['words'], 16), np.nan)
    trace = []
    if stmt == 'permute4':
        for k in range(4):
            v[:, k] = X[:, :4][:, SUB ^ k, LANE]
    elif stmt == 'finish_row':
        gt, jt, inv = X[:, 0:6].transpose(0, 2, 1), X[:, 6:9].transpose(0, 2, 1), X[:, 9]
        v[:, :10] = ref.permuted(gt, jt)
        v[:, ROW_LAM] = 0.0
        v[:, ROW_NK:] = ref.gram(gt, jt, inv, gt, jt, **wrong).transpose(0, 2, 1)
        if case.targ:
            v[:, ROW_NK + 3::4] = np.nan
    elif stmt == 'cross_gram':
        T = lambda a, b: X[:, a:b].transpose(0, 2, 1)
        v[:] = ref.gram(T(0, 6), T(6, 9), X[:, 9], T(10, 16), T(16, 19), **wrong).transpose(0, 2, 1)
    elif stmt == 'gs_round':
        limit, uni = GS_TARGS[case.targ]
        gt, jt, c, inv, lam = decode_row(X, 0)
        dx, dq = ref.gather_velocity(X[:, 30], X[:, 31], X[:, 32])
        lam2, dx2, dq2 = ref.gs_round(gt, jt, c, inv, lam, X[:, 29], dx, dq, limit, uni, trace=trace, **wrong)
        v[:, 0] = lam2
        v[:, 1], v[:, 2], v[:, 3] = ref.scatter_velocity(dx2, dq2)
    elif stmt == 'gs_cone_round':
        g1, j1, c1, inv1, lam1 = decode_row(X, 0)
        g2, j2, c2, inv2, lam2 = decode_row(X, RW)
        dx, dq = ref.gather_velocity(X[:, 91], X[:, 92], X[:, 93])
        a, b, dx2, dq2 = ref.gs_cone_round(g1, j1, c1, inv1, lam1, g2, j2, c2, inv2, lam2, X[:, 90], dx, dq, trace=trace, **wrong)
        v[:, 0], v[:, 1] = a, b
        v[:, 2], v[:, 3], v[:, 4] = ref.scatter_velocity(dx2, dq2)
    elif stmt == 'contact_rows':
        I = contact_inputs(X)
        rows = []
        for k, uu in enumerate(I['us']):
            gt, jt, c, inv = ref.contact_row(uu, I['Pb'], I['d'], I['lf'], I['Sb'], I['Sd'], I['xi'], I['qs'], I['bias'] if k == 0 else 0.0, I['cvalid'])
            rows.append((gt, jt, inv))
            v[:, k * RW:k * RW + 10] = ref.permuted(gt, jt)
            v[:, k * RW + ROW_C], v[:, k * RW + ROW_INV], v[:, k * RW + ROW_LAM] = c, inv, 0.0
            v[:, k * RW + ROW_NK:(k + 1) * RW] = ref.gram(gt, jt, inv, gt, jt, **wrong).transpose(0, 2, 1)
        (g1, j1, i1), (g2, j2, i2) = rows[1], rows[2]
        v[:, 87:103] = ref.gram(g1, j1, i1, g2, j2, **wrong).transpose(0, 2, 1)
        v[:, 103:119] = ref.gram(g2, j2, i2, g1, j1, **wrong).transpose(0, 2, 1)
    elif stmt == 'pd':
        tgt = np.clip(X[:, 0:3] + X[:, 3:6], -3.0, 3.0)
        mt = np.where(X[:, 12] > 0, X[:, 12], X[:, 11])[:, None]
        v[:, 0:3] = tgt
        v[:, 3:6] = np.clip((tgt - X[:, 0:3]) * X[:, 9:10] - X[:, 6:9] * X[:, 10:11], -mt, mt)
    elif stmt == 'clip_velocities':
        with np.errstate(invalid='ignore'):
            v[:] = np.where(np.isfinite(X[:, :9]), np.clip(X[:, :9], -X[:, 9:10], X[:, 9:10]), np.inf)      # (inf: the mark of "must come out NaN", see want())
    elif stmt == 'pick_rank':
        k = (LANE & ~3) | case.targ
        take = np.abs(X[:, 0][:, k] - X[:, 1]) < 0.5
        for w in range(3):
            v[:, w] = np.where(take, X[:, 2 + w][:, k], X[:, 5 + w])
    elif stmt in ('self_row', 'pair_row'):
        pair, I = stmt == 'pair_row', rare_inputs(X, stmt == 'pair_row')
        jt, gt, vrow, nn = ref.rare_half(I['ub'], I.get('pb'), I['jsel'], I['e'], I['lf'], I['Sb'], I['Sd'], I['qs'], I.get('xi'))
        dx, dq = ref.gather_velocity(*I['V'])
        share = ref.rare_share(gt, jt, dx, dq) * I['have']
        o = np.arange(R) ^ 1
        if pair:                               # the two rows of an arena are ONE row of the system: free velocity, diagonal and row velocity are the sums of the two shares
            vrow, nn, w_v = vrow + vrow[o], nn + nn[o], share + share[o]
            bias = ref.row_bias(X[:, 79, 0], X[:, 80, 0], X[:, 81, 0], X[:, 82, 0], X[:, 83, 0], X[:, 84, 0]) if case.targ == 0 else 0.0
        else:
            w_v, bias = share, X[:, 70, 0]
        have = I['have']
        with np.errstate(divide='ignore'):
            c, inv, lam = (vrow + bias) * have, np.where(have, 1.0 / nn, 0.0), I['lam0'] * have
        fric = case.targ == 1
        nl, dx2, dq2 = ref.rare_turn(gt * have[:, None], jt * have[:, None, None], c, inv, lam, w_v, -I['hi'] if fric else 0.0, I['hi'] if fric else np.inf, dx, dq, **wrong)
        sa, sb, sj = ref.packed(gt * have[:, None], jt * have[:, None, None])
        v[:, 0], v[:, 1], v[:, 2] = sa, sb, sj
        for w, x in ((3, c), (4, inv), (5, 0.0 * c), (6, share), (7, nl)):
            v[:, w] = x[:, None]
        v[:, 8], v[:, 9], v[:, 10] = ref.scatter_velocity(dx2, dq2)
    elif stmt == 'self_pieces':
        jt, gt, d = X[:, 0:3, 0::4].transpose(0, 2, 1), X[:, 3:9, 0], X[:, 9, 0]
        dx, dq = ref.gather_velocity(X[:, 10], X[:, 11], X[:, 12])
        v[:, 0], v[:, 1], v[:, 2] = ref.packed(gt, jt)
        v[:, 3] = ref.rare_share(gt, jt, dx, dq)[:, None]
        _, dx2, dq2 = ref.rare_turn(gt, jt, 0.0, 1.0, np.zeros(R), -d, -np.inf, np.inf, dx, dq, **wrong)      # (an increment of exactly d)
        v[:, 4], v[:, 5], v[:, 6] = ref.scatter_velocity(dx2, dq2)
        v[:, 7:13] = 0.0
    elif stmt == 'cand_eval_point':
        T = lambda a, b: X[:, a:b].transpose(0, 2, 1)
        ln_, r_, az, ax = X[:, 35], X[:, 33], X[:, 34], T(30, 33)
        il = np.where(ln_ < 1e-6, 0.0, 1.0 / np.maximum(ln_, 1e-12))
        x = T(27, 30) - (T(24, 27) - az[..., None] * ax) * (il * r_)[..., None]
        Pb = T(21, 24) + np.einsum('rlij,rlj->rli', T(12, 21).reshape(R, 16, 3, 3), x)
        Pw = np.einsum('rij,rlj->rli', X[:, 3:12, 0].reshape(R, 3, 3), Pb) + X[:, 0:3, 0][:, None, :]
        rs = np.where((ax ** 2).sum(-1) < 0.5, r_, 0.0)
        v[:, 0:3] = Pw.transpose(0, 2, 1)
        v[:, 2] += rs
        v[:, 3] = rs
    elif stmt == 'compose':
        I = contact_inputs(X)
        if not I['cvalid'].any():          # no contact anywhere: nothing moves (and the whole-number factors of this class need not be a mass matrix)
            v[:] = 0.0
        else:
            lam, dxi, dqd = ref.compose(I['us'], I['Pb'], I['d'], I['lf'], I['Sb'], I['Sd'], I['xi'], I['qs'], I['bias'], I['cvalid'], X[:, 86], case.targ == 0)
            v[:, 0:3] = lam
            v[:, 3:9] = dxi[:, :, None]
            v[:, 9:12] = dqd[:, LEG].transpose(0, 2, 1)
    else:
        raise KeyError(name)
    return v, trace


def model(name, case, mode):
    """-> (v, e) [rows, words, 16]: the entry in the kernel's form, its value and its forward bound under `mode` ('twin' / 'madd', math_helpers_ref)"""
    h = ENTRIES[name]
    stmt = h['stmt']
    X = case.X.astype(np.float64)
    R = len(X)
    v, e = np.full((R, h['words'], 16), np.nan), np.full((R, h['words'], 16), np.nan)

    def gram_words(w0, G, limit=False):
        v[:, w0:w0 + 16], e[:, w0:w0 + 16] = G.v.transpose(0, 2, 1), G.e.transpose(0, 2, 1)
        if limit:
            v[:, w0 + 3:w0 + 16:4] = np.nan

    def run():
        if stmt in ('permute4', 'clip_velocities', 'pick_rank'):
            v[:], e[:] = statement(name, case)[0], 0.0
        elif stmt == 'pd':
            from math_helpers_ref import E
            q, act, qd = ([E(X[:, 3 * k + j]) for j in range(3)] for k in range(3))
            mt = np.where(X[:, 12] > 0, X[:, 12], X[:, 11])
            for j in range(3):
                tgt = ref.eclamp(q[j] + act[j], -3.0, 3.0)
                _put(v, e, j, tgt)
                _put(v, e, 3 + j, ref.eclamp((tgt - q[j]) * E(X[:, 9]) + (E(0.0) - qd[j]) * E(X[:, 10]), E(-mt), E(mt)))
        elif stmt == 'finish_row':
            gt, jt, inv = X[:, 0:6].transpose(0, 2, 1), X[:, 6:9].transpose(0, 2, 1), X[:, 9]
            v[:, :10], e[:, :10] = ref.permuted(gt, jt), 0.0
            v[:, ROW_LAM], e[:, ROW_LAM] = 0.0, 0.0
            gram_words(ROW_NK, ref.m_gram(gt, jt, inv, gt, jt), case.targ)
        elif stmt == 'cross_gram':
            T = lambda a, b: X[:, a:b].transpose(0, 2, 1)
            gram_words(0, ref.m_gram(T(0, 6), T(6, 9), X[:, 9], T(10, 16), T(16, 19)))
        elif stmt == 'gs_round':
            limit, uni = GS_TARGS[case.targ]
            gt, jt, c, inv, lam = decode_row(X, 0)
            dx, dq = ref.gather_velocity(X[:, 30], X[:, 31], X[:, 32])
            for w, x in enumerate(ref.m_gs_round(gt, jt, c, inv, lam, X[:, 29], dx, dq, limit, uni)):
                _put(v, e, w, x)
        elif stmt == 'gs_cone_round':
            g1, j1, c1, inv1, lam1 = decode_row(X, 0)
            g2, j2, c2, inv2, lam2 = decode_row(X, RW)
            dx, dq = ref.gather_velocity(X[:, 91], X[:, 92], X[:, 93])
            for w, x in enumerate(ref.m_gs_cone_round(g1, j1, c1, inv1, lam1, g2, j2, c2, inv2, lam2, X[:, 90], dx, dq)):
                _put(v, e, w, x)
        elif stmt == 'contact_rows':
            I = contact_inputs(X)
            rows = []
            for k, uu in enumerate(I['us']):
                gt, jt, c, inv = ref.m_contact_row(uu, I['Pb'], I['d'], I['lf'], I['Sb'], I['Sd'], I['xi'], I['qs'], I['bias'] if k == 0 else np.zeros_like(I['bias']), I['cvalid'])
                G, J = ref.stack_e(gt), ref.stack_e(jt)
                rows.append((G, J, inv))
                v[:, k * RW:k * RW + 10], e[:, k * RW:k * RW + 10] = ref.permuted(G.v, J.v), ref.permuted(G.e, J.e)
                _put(v, e, k * RW + ROW_C, c); _put(v, e, k * RW + ROW_INV, inv)
                v[:, k * RW + ROW_LAM], e[:, k * RW + ROW_LAM] = 0.0, 0.0
                gram_words(k * RW + ROW_NK, ref.m_gram(G, J, inv, G, J))
            (g1, j1, i1), (g2, j2, i2) = rows[1], rows[2]
            gram_words(87, ref.m_gram(g1, j1, i1, g2, j2))
            gram_words(103, ref.m_gram(g2, j2, i2, g1, j1))
        elif stmt in ('self_row', 'pair_row'):
            from math_helpers_ref import E
            pair, I = stmt == 'pair_row', rare_inputs(X, stmt == 'pair_row')
            sj, gt, vrow, nn = ref.e_rare_half(I['ub'], I.get('pb'), I['jsel'], I['e'], I['lf'], I['Sb'], I['Sd'], I['qs'], I.get('xi'), pair)
            have, o = I['have'], np.arange(R) ^ 1
            gate = lambda x: E(np.where(have if x.v.ndim == 1 else have[:, None], x.v, 0.0), np.where(have if x.v.ndim == 1 else have[:, None], x.e, 0.0))
            sa, sb, sjl = (gate(x) for x in ref.e_packed(gt, sj))
            share = ref.e_rare_share(sa, sb, sjl, *I['V'])
            flip = lambda x: E(x.v[o], x.e[o])
            first = (np.arange(R) % 2 == 0)
            both = lambda x: ref.esel_(first, x, flip(x)) + ref.esel_(first, flip(x), x)          # robot 0's share first, in both rows
            if pair:
                vrow, nn, w_v = both(vrow), both(nn), both(share)
                c = vrow + ref.e_row_bias(X[:, 79, 0], X[:, 80, 0], X[:, 81, 0], X[:, 82, 0], X[:, 83, 0], X[:, 84, 0]) if case.targ == 0 else vrow + E(0.0)
            else:
                w_v, c = share, vrow + E(X[:, 70, 0])
            c, inv, lam = gate(c), gate(1.0 / nn), E(I['lam0'] * have)
            x = lam - (c + w_v) * inv
            fric = case.targ == 1
            nl = ref.eclamp(x, E(-I['hi']) if fric else E(0.0), E(I['hi']) if fric else E(np.inf))
            VA, VB, VJ = ref.e_rare_apply(sa, sb, sjl, nl - lam, *I['V'])
            for w, q in ((0, sa), (1, sb), (2, sjl), (8, VA), (9, VB), (10, VJ)):
                _put(v, e, w, q)
            for w, q in ((3, c), (4, inv), (5, E(np.zeros(R))), (6, share), (7, nl)):
                v[:, w], e[:, w] = q.v[:, None], q.e[:, None]
        elif stmt == 'self_pieces':
            from math_helpers_ref import E
            jt, gt, d = X[:, 0:3, 0::4].transpose(0, 2, 1), X[:, 3:9, 0], X[:, 9, 0]
            sa, sb, sj = (E(q) for q in ref.packed(gt, jt))
            V = (X[:, 10], X[:, 11], X[:, 12])
            for w, q in ((0, sa), (1, sb), (2, sj)) + tuple(zip((4, 5, 6), ref.e_rare_apply(sa, sb, sj, E(d), *V))):
                _put(v, e, w, q)
            q = ref.e_rare_share(sa, sb, sj, *V)
            v[:, 3], e[:, 3] = q.v[:, None], q.e[:, None]
            v[:, 7:13], e[:, 7:13] = 0.0, 0.0
        elif stmt == 'cand_eval_point':
            from math_helpers_ref import E
            import math_helpers_ref as mr
            c3 = lambda a: [E(X[:, a + i]) for i in range(3)]
            ln_, r_, az, ax, ez, A, lp = X[:, 35], E(X[:, 33]), E(X[:, 34]), c3(30), c3(24), c3(27), c3(21)
            inv = 1.0 / E(np.maximum(ln_, 1e-12))
            il = E(np.where(ln_ < 1e-6, 0.0, inv.v), np.where(ln_ < 1e-6, 0.0, inv.e))
            xx = [A[i] - ((ez[i] - az * ax[i]) * il) * r_ for i in range(3)]
            Pb = mr.add3(lp, mr.mulMV([E(X[:, 12 + i]) for i in range(9)], xx))
            Pw = mr.mulMV([E(X[:, 3 + i]) for i in range(9)], Pb)
            rs = np.where(sum(a.v ** 2 for a in ax) < 0.5, r_.v, 0.0)
            for i in range(3):
                _put(v, e, i, (Pw[i] + E(X[:, i])) + E(rs) if i == 2 else Pw[i] + E(X[:, i]))
            v[:, 3], e[:, 3] = rs, 0.0
        elif stmt == 'compose':
            I = contact_inputs(X)
            lam_n, lam_1, lam_2, dxi, du = ref.m_compose(I['us'], I['Pb'], I['d'], I['lf'], I['Sb'], I['Sd'], I['xi'], I['qs'], I['bias'], I['cvalid'], X[:, 86], case.targ == 0)
            for w, x in enumerate([lam_n, lam_1, lam_2] + dxi + du):
                v[:, w], e[:, w] = np.broadcast_to(x.v, (R, 16)), np.broadcast_to(x.e, (R, 16))
        else:
            raise KeyError(name)
    ref.in_mode(mode, run)
    return v, e


def want(name, case):
    """-> dict(v statement, model_v, twin, madd bounds [rows, words, 16], trace); cached per case object"""
    key = (name, id(case))
    if key not in _WANT:
        sv, trace = statement(name, case)
        mv, mt = model(name, case, 'twin')
        _, mm = (mv, mt) if ENTRIES[name]['cls'] != APPROX else model(name, case, 'madd')
        must_nan = np.isinf(sv)            # clip_velocities: a NaN or an infinity must come out NaN and not a bound, as clip1 promises
        sv, mv = np.where(must_nan, 0.0, sv), np.where(must_nan, 0.0, mv)
        _WANT[key] = dict(v=sv, model_v=mv, twin=mt, madd=mm, trace=trace, must_nan=must_nan)
    return _WANT[key]


# ---- comparison ----------------------------------------------------------------------------------------------------------------------------------------
def _bits(x): return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def bits_equal(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


def rows_on(n, active): return ((active >> (np.arange(n) % 4)) & 1).astype(bool)


def head(name, case, who): return '%s [%s%s, targ %d] %s' % (name, case.klass, '' if case.note in (None, 'plain') else ': ' + case.note, case.targ, who)


def check(name, case, got, who, bar='twin', dev_host=None, active=0b1111):
    """Holds the answer `got` [rows, n_out, 16] of `who` to the statement; -> dict(err [words] worst |answer - statement| over the case, ratio worst error / bar, word, bar).
    bar: 'twin' (the twin's own forward bound) or 'gpu' (max(4 dev_host, multiply-add bound) for APPROX, the multiply-add bound for MADD).  No sample is left out."""
    h, w = ENTRIES[name], want(name, case)
    words, v = h['words'], w['v'][:len(got)]
    on = rows_on(len(got), active)
    hd = head(name, case, who)
    assert np.isnan(got[~on]).all(), hd + ': a row outside EXEC wrote'
    assert np.isnan(got[:, words:]).all(), hd + ': a word past the entry\'s outputs was written'
    g = got[:, :words].copy()
    must_nan = w['must_nan'][:len(got)] & on[:, None, None]
    assert np.isnan(g[must_nan]).all(), hd + ': a NaN or an infinity did not come out NaN'
    g[must_nan] = 0.0
    stored = ~np.isnan(v)
    assert np.isnan(g[~stored]).all(), hd + ': a word the entry does not form was written (word %d)' % np.argwhere(~np.isnan(g) & ~stored)[0][1] if (~np.isnan(g) & ~stored).any() else ''
    cmp_ = stored & on[:, None, None]
    assert (np.isfinite(g) | ~cmp_).all(), hd + ': a non-finite answer (or a word left unwritten) at (row, word, lane) %s' % (np.argwhere(~np.isfinite(g) & cmp_)[0].tolist(),)
    want32 = np.where(stored, v, 0.0).astype(np.float32)
    for word in h['moves'] if h['cls'] != MOVES else range(words):
        same = bits_equal(g[:, word], want32[:, word]) | ~cmp_[:, word]
        assert same.all(), hd + ': word %d (a move) differs from the statement in bits at (row, lane) %s' % (word, np.argwhere(~same)[0].tolist())
    err = np.where(cmp_, np.abs(g.astype(np.float64) - np.where(stored, v, 0.0)), 0.0)
    if h['cls'] == MOVES:
        return dict(err=np.zeros(words), err_at=0.0, ratio=0.0, word=0, bar=0.0)
    if case.klass != 'random':           # every intermediate of the statement is a float32 here: its value is THE answer
        same = (g == want32) & ((np.signbit(g) == np.signbit(want32)) | (name in ZERO_SIGN_FREE)) | ~cmp_
        assert same.all(), hd + ': exact inputs, but the answer is not the statement\'s float32 at (row, word, lane) %s (%r, %r)' % (
            np.argwhere(~same)[0].tolist(), g[tuple(np.argwhere(~same)[0])], want32[tuple(np.argwhere(~same)[0])])
    if bar == 'twin' or h['cls'] == MADD:
        b = w['twin' if (bar == 'twin' and h['cls'] != MADD) else 'madd'][:len(got)]
    else:
        b = np.maximum(4.0 * dev_host[None, :, None], w['madd'][:len(got)])
    b = np.where(cmp_, b, np.inf)
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where(err > 0, err / b, 0.0)
    bad = np.argwhere(ratio > 1.0)
    assert not len(bad), hd + ': |answer - statement| = %.3e above the bar %.3e at (row, word, lane) %s (%d such)' % (err[tuple(bad[0])], b[tuple(bad[0])], bad[0].tolist(), len(bad))
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return dict(err=err.max(axis=(0, 2)), err_at=float(err[at]), ratio=float(ratio.max()), word=int(at[1]), bar=float(b[at]) if (np.isfinite(b[at]) and case.klass == 'random') else 0.0)


def partial_exec_check(runner, policy, name, case, full, who):
    """rows {0, 1} and row {2} alone of ONE wave: the active rows answer what they answered in the whole wave, the others write nothing (NaN canaries, bit for bit)"""
    for active in ENTRIES[name]['actives'][1:]:
        got = runner.run(policy, name, case, active, limit=4)
        on = rows_on(4, active)
        assert np.isnan(got[~on]).all(), '%s: a row outside EXEC %s wrote' % (head(name, case, who), bin(active))
        assert bits_equal(got[on], full[:4][on]).all(), '%s: rows %s answer differently alone' % (head(name, case, who), bin(active))


def piped_against_plain(case, piped, plain, who):
    """contact_rows_cone_piped gives the rows of contact_row x 3 + cross_gram x 2: bit for bit for the coefficients, c and inv (and lam); the Gram and cross scalars are
    held to the statement's bound by check() -- the sum order of two additions differs"""
    for k in range(3):
        for word in list(range(k * RW, k * RW + ROW_NK)):
            same = bits_equal(piped[:, word], plain[:, word])
            assert same.all(), '%s: word %d of row %d differs from contact_row\'s in bits at (row, lane) %s' % (head('contact_rows_piped', case, who), word - k * RW, k, np.argwhere(~same)[0].tolist())


def arena_rows_agree(case, got, who):
    """c and inv of a pair row sum robot 0's share first in both rows: the two rows of an arena hold the same BITS of c, inv and, after the turn, lam (me = 0 and me = 1)"""
    assert (case.X[0::2, 87] == 0).all() and (case.X[1::2, 87] == 1).all()
    for word, what in ((3, 'c'), (4, 'inv'), (7, 'lam')):
        same = bits_equal(got[0::2, word], got[1::2, word])
        assert same.all(), '%s: %s differs between the two rows of arena %d' % (head('pair_row', case, who), what, np.argwhere(~same)[0][0])


def cleared_row_changes_nothing(name, case, got, who):
    """have == false leaves a cleared row (coefficients, c, inv, lam all zero), and the turn on it changes nothing: the velocity comes back bit for bit"""
    pair = name == 'pair_row'
    off = case.X[:, 85 if pair else 71, 0] < 0.5
    assert off.any()
    V = 88 if pair else 73
    assert (got[off, 0:8] == 0).all(), '%s: a row built with have == false is not cleared' % head(name, case, who)
    assert bits_equal(got[off, 8:11], case.X[off, V:V + 3]).all(), '%s: a turn on a cleared row changed the velocity' % head(name, case, who)
