"""Shared by tests/test_math_helpers_emul.py and tests/test_gpu_math_helpers.py: the class table of the step kernels' math, rotation and geometry helpers
(lifelike_agility_and_play_amd/csrc/pmc_math.hpp; the self-contained static members of Pmc<L> in pmc_step.hpp), their inputs (fixed seeds), the runners of the host twin
and the GPU copy of tests/lanes/math_helpers_body.hpp, and the comparison.  One sample per lane: [row][word][16 lanes], up to 64 one-wave workgroups a launch.

Classes
  MOVES   no arithmetic: GPU == host twin == statement, bit for bit
  MADD    multiplies and adds only: bit for bit with the statement on exact inputs (small integers and powers of two: every intermediate is a float32); on random
          inputs each of GPU and twin within the derived forward bound (math_helpers_ref: u (|value| + carried error) per operation, valid under any contraction)
  APPROX  a reciprocal, square root, division, library function or hand-written series: the twin (correctly rounded operations, glibc's float functions) within its
          own forward bound with every library call counted as 1 ulp; the GPU within max(4 x dev_host, arithmetic forward bound of the helper's multiply-adds), dev_host =
          the twin's worst |answer - statement| over the same input class and output word.  Why 4: a 1-ulp rcp / sqrt / rsq at most doubles the rounding term of its
          operation against a correctly rounded one, and the device library's functions are specified to a few ulp where glibc's are under one; it is also the margin
          tests/hl_score_ref.tolerances uses for float32 against float64.
All inputs are finite; no float32 intermediate is denormal unless the class says so (the GPU build flushes them, the twin does not).
Zero-length segments are not a case the kernels produce (a capsule axis has its link's length): seg_seg_st is not run on them.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

import math_helpers_ref as ref
from math_helpers_ref import U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LANES_DIR = os.path.join(ROOT, 'tests', 'lanes')
HOST_LIB = os.path.join(LANES_DIR, '_build', 'libmath_helpers_host.so')
GPU_POLICIES = ['GpuLanes', 'GpuLanes1', 'GpuLanesPmc1Plain']
ACTIVE_ROWS = [0b1111, 0b0011, 0b0100]       # the whole wave, rows {0, 1}, row {2}
MOVES, MADD, APPROX = 'MOVES', 'MADD', 'APPROX'
TABLES = [0, 1, 2]                           # helpers that read the leg / link constant tables run under every policy (LDS in some builds, registers in others)

# id: MathHelper of tests/lanes/math_helpers_body.hpp; words: the output words; names: the functions the entry covers (the coverage scan of test_math_helpers_emul.py)
HELPERS = {
    'v3ops': dict(id=0, cls=MADD, words=13, names=['operator+', 'operator-', 'scale', 'dot', 'cross']),
    'm3ops': dict(id=1, cls=MADD, words=24, names=['mul', 'mulT', 'rot_sym']),
    'svops': dict(id=2, cls=MADD, words=41, names=['crm', 'crf', 'apply', 'add']),
    'moves': dict(id=3, cls=MOVES, words=21, names=['mk3', 'cvt3', 'cvt6', 'qconj', 'load_box', 'store_box']),
    'philox': dict(id=4, cls=MOVES, words=6, names=['philox4x32', 'u01_from']),
    'qmul': dict(id=5, cls=MADD, words=4), 'qnormalize': dict(id=6, cls=APPROX, words=4), 'qmat': dict(id=7, cls=MADD, words=9),
    'rotvec_of': dict(id=8, cls=APPROX, words=3), 'quat_of_rotvec': dict(id=9, cls=APPROX, words=4), 'quat_of_small_rotvec': dict(id=10, cls=APPROX, words=4),
    'axis_angle_scaled': dict(id=11, cls=APPROX, words=4),
    'chol_solve': dict(id=12, cls=APPROX, words=33, names=['chol6', 'fwd6', 'bwd6']), 'fwd_bwd6': dict(id=13, cls=MADD, words=12, names=['fwd6', 'bwd6']),
    'plane_space': dict(id=14, cls=APPROX, words=6), 'row_bias': dict(id=15, cls=MADD, words=1), 'clip1': dict(id=16, cls=MADD, words=1),
    'damping_force': dict(id=17, cls=APPROX, words=6),
    'qmul_t': dict(id=32, cls=MADD, words=4), 'qconj_t': dict(id=33, cls=MOVES, words=4), 'qnormalize_t': dict(id=34, cls=APPROX, words=4),
    'rotvec_of_t': dict(id=35, cls=APPROX, words=3), 'quat_of_rotvec_t': dict(id=36, cls=APPROX, words=4), 'axis_angle_scaled_t': dict(id=37, cls=APPROX, words=4),
    'sincos_joint': dict(id=38, cls=APPROX, words=2), 'leg_fk': dict(id=39, cls=APPROX, words=48, policies=TABLES), 'foot_world': dict(id=40, cls=APPROX, words=3, policies=TABLES),
    'own_link_inertia': dict(id=41, cls=MADD, words=38, policies=TABLES, names=['own_link_inertia', 'own_link', 'own_link_held']),
    'link_inertia': dict(id=42, cls=MADD, words=19, policies=TABLES, targs=[0, 1, 2]),
    'lm_fwd_bwd': dict(id=43, cls=MADD, words=12, names=['lm_fwd', 'lm_bwd', 'sv_to6']), 'seg_seg_st': dict(id=44, cls=APPROX, words=8),
    'damping_force_t': dict(id=45, cls=APPROX, words=6, names=['damping_force']),
    'terrain_sdf': dict(id=46, cls=APPROX, words=5, names=['terrain_sdf_rec', 'shape_sdf_rec']),
    'mocap': dict(id=47, cls=APPROX, words=19, names=['mocap_gather', 'mocap_finish']),
}
# The sign of a zero: the lane-varying forms negate by `zero - x` (there is no lane-varying unary minus), which gives +0 where the scalar forms' `-x` and the
# statement give -0 -- rotvec_of_t / axis_angle_scaled_t after the w < 0 flip, the rotation matrices of leg_fk at q = 0.  On exact inputs those helpers are held to the
# statement's VALUE (+0 == -0); every other helper to its bits.
ZERO_SIGN_FREE = {'rotvec_of_t', 'axis_angle_scaled_t', 'leg_fk', 'foot_world'}
for _k, _v in HELPERS.items():
    _v.setdefault('policies', [0]); _v.setdefault('targs', [0]); _v.setdefault('names', [_k])
# LL_HD functions of pmc_math.hpp / listed members of Pmc<L> that no entry drives, each with the reason (test_math_helpers_emul.py: a function in neither table fails the scan)
EXEMPT = {}
# the members of Pmc<L> the scan asks for (the solver rows, finish_row, gs_round, the cone round and the contact builders are held one by one in solver_rows_common.py,
# the terrain-edge detectors leg_edge / reverse_edge and one slot of the leg-leg pick, self_pick, in contact_scan_common.py; still open, listed there as LATER: the
# deepest-K selection of the ground contacts, the candidate depth loop and the geometry of the leg-leg and robot-robot scans inside substep_impl)
PMC_MEMBERS = ['sincos_joint', 'leg_fk', 'foot_world', 'own_link_inertia', 'link_inertia', 'damping_force', 'chol6', 'fwd6', 'bwd6', 'lm_fwd', 'lm_bwd', 'shape_sdf_rec',
               'terrain_sdf_rec', 'seg_seg_st', 'plane_space', 'row_bias', 'clip1', 'mocap_gather', 'mocap_finish']


class Dims:
    def __init__(self, lib):
        d = (C.c_int * 16)()
        lib.ll_math_helpers_dims(d)
        self.n_in, self.n_out, self.n_auxd, self.max_blocks, self.lc, self.cw, self.bc, self.n_consts, self.lk_base, self.n_policies = list(d)[:10]


class Ctx:
    """what a statement needs beside the inputs: the constant tables of the case and where a sample sits in its row"""
    def __init__(self, dims, consts, targ=0):
        self.legc = consts[:dims.lc * 4].reshape(dims.lc, 4)
        self.candc = consts[dims.lc * 4:dims.lc * 4 + dims.cw * 16].reshape(dims.cw, 16)
        self.lk_base, self.targ = dims.lk_base, targ

    @staticmethod
    def lane(n): return np.arange(n) % 16
    @staticmethod
    def leg(n): return (np.arange(n) % 16) // 4


def model_blob():
    from lifelike_agility_and_play_amd import urdf_model
    return urdf_model.default_model_blob()


def model_consts(dims):
    """the tables of the default model as csrc/pmc_tables.hpp fills the fields these helpers read (joint origins, link masses, COMs, inertias, foot origin; the
    own-link words of the candidate table); everything else zero"""
    from lifelike_agility_and_play_amd import urdf_model as um
    b = model_blob()
    consts = np.zeros(dims.n_consts, dtype=np.float32)
    consts[-1] = 1.0
    c = Ctx(dims, consts)
    for l in range(4):
        for k in range(3):
            i = 3 * l + k
            c.legc[3 * k:3 * k + 3, l] = b[um.OFF_JOINT_ORIGIN + 3 * i:um.OFF_JOINT_ORIGIN + 3 * i + 3]
            c.legc[12 + 3 * k:15 + 3 * k, l] = b[um.OFF_LINK_COM + 3 * i:um.OFF_LINK_COM + 3 * i + 3]
            c.legc[9 + k, l] = b[um.OFF_LINK_MASS + i]
            I = b[um.OFF_LINK_INERTIA + 9 * i:um.OFF_LINK_INERTIA + 9 * i + 9]
            c.legc[21 + 6 * k:27 + 6 * k, l] = I[[0, 1, 2, 4, 5, 8]]
            c.candc[dims.lk_base:dims.lk_base + 10, 4 * l + k] = np.concatenate([[b[um.OFF_LINK_MASS + i]], b[um.OFF_LINK_COM + 3 * i:um.OFF_LINK_COM + 3 * i + 3], I[[0, 1, 2, 4, 5, 8]]])
        c.legc[48:51, l] = b[um.OFF_FOOT_POS + 3 * l:um.OFF_FOOT_POS + 3 * l + 3]
    return consts


def integer_consts(dims):
    """tables of small whole numbers, every word different: the exact class of the helpers that read them"""
    consts = np.zeros(dims.n_consts, dtype=np.float32)
    consts[-1] = 1.0
    c = Ctx(dims, consts)
    c.legc[:] = ((np.arange(dims.lc * 4).reshape(dims.lc, 4) * 7) % 11 - 5)
    c.candc[:] = ((np.arange(dims.cw * 16).reshape(dims.cw, 16) * 5) % 9 - 4)
    c.candc[dims.lk_base] = np.abs(c.candc[dims.lk_base]) + 1
    c.legc[9:12] = np.abs(c.legc[9:12]) + 1
    return consts


class Case:
    def __init__(self, klass, X, consts, targ=0, auxd=None, n=None, note=None):
        X = np.asarray(X, dtype=np.float32)
        self.klass, self.n, self.targ, self.consts, self.note = klass, len(X) if n is None else n, targ, consts, note
        pad = (-len(X)) % 64
        self.X = np.concatenate([X, np.repeat(X[:1], pad, axis=0)]) if pad else X          # whole waves; the padding repeats the first sample and is not compared
        self.auxd = np.zeros(38) if auxd is None else np.asarray(auxd, dtype=np.float64)


def _bind(path):
    lib = C.CDLL(path)
    lib.ll_math_helpers_dims.argtypes = [C.POINTER(C.c_int)]
    lib.ll_math_helpers_run.restype = C.c_int
    lib.ll_math_helpers_run.argtypes = [C.c_int] * 5 + [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_long]
    return lib


def to_rows(X, n_words):
    """[n, words] -> [rows][n_words][16], words beyond the case's zero"""
    n, w = X.shape
    out = np.zeros((n // 16, n_words, 16), dtype=np.float32)
    out[:, :w] = X.reshape(n // 16, 16, w).transpose(0, 2, 1)
    return out


def from_rows(R, words): return R[:, :words].transpose(0, 2, 1).reshape(-1, words)


class HostRunner:
    def __init__(self):
        subprocess.check_call(['make', '-C', LANES_DIR, '-s'])
        self.lib = _bind(HOST_LIB)
        self.dims = Dims(self.lib)

    def launch(self, policy, hid, targ, n_blocks, active, w, out, auxd, consts):
        return self.lib.ll_math_helpers_run(policy, hid, targ, n_blocks, active, w.ctypes.data, w.size, out.ctypes.data, out.size, auxd.ctypes.data, auxd.size, consts.ctypes.data, consts.size)

    def run(self, policy, name, case, active=0b1111, limit=None):
        """-> [n, words] float32; rows outside `active` (and everything never written) stay NaN"""
        h, d = HELPERS[name], self.dims
        X = case.X if limit is None else case.X[:limit]
        res = []
        for i in range(0, len(X), 64 * d.max_blocks):
            w = to_rows(X[i:i + 64 * d.max_blocks], d.n_in)
            out = np.full((len(w), d.n_out, 16), np.nan, dtype=np.float32)
            rc = self.launch(policy, h['id'], case.targ, len(w) // 4, active, w, out, case.auxd, case.consts)
            assert rc == 0, (name, rc)
            res.append(from_rows(out, d.n_out))
        return np.concatenate(res)


class GpuRunner(HostRunner):
    """One launch per run() chunk on the default stream, synchronised; torch only holds the device buffers."""
    def __init__(self, path, host_dims):
        import torch
        self.torch = torch
        self.lib = _bind(path)
        self.dims = Dims(self.lib)
        assert (self.dims.n_in, self.dims.n_out, self.dims.n_auxd, self.dims.n_consts, self.dims.max_blocks) == (host_dims.n_in, host_dims.n_out, host_dims.n_auxd, host_dims.n_consts, host_dims.max_blocks)

    def launch(self, policy, hid, targ, n_blocks, active, w, out, auxd, consts):
        t = self.torch
        dw, dout, da, dc = (t.from_numpy(x).to('cuda:0') for x in (w, out, auxd, consts))
        t.cuda.synchronize()
        rc = self.lib.ll_math_helpers_run(policy, hid, targ, n_blocks, active, dw.data_ptr(), dw.numel(), dout.data_ptr(), dout.numel(), da.data_ptr(), da.numel(), dc.data_ptr(), dc.numel())
        t.cuda.synchronize()
        out[:] = dout.cpu().numpy()
        return rc


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------------------
N = 4096


def _rng(name, k=0): return np.random.default_rng([sum(name.encode()) * 7919 + len(name), k])
def _ints(r, n, w, lo=-4, hi=4): return r.integers(lo, hi + 1, size=(n, w)).astype(np.float32)
def _unit(r, n, k=3): v = r.normal(size=(n, k)); return v / np.linalg.norm(v, axis=1, keepdims=True)


def _quat_of(axis, angle):
    return np.concatenate([axis * np.sin(0.5 * angle)[:, None], np.cos(0.5 * angle)[:, None]], axis=1)


def _rotmats(r, n):
    from scipy.spatial.transform import Rotation as R
    return R.from_quat(_unit(r, n, 4)).as_matrix().reshape(n, 9)


def _perm_mats(r, n):
    """signed permutation matrices: rotations and reflections with entries 0, +-1 (exact)"""
    out = np.zeros((n, 3, 3))
    for i in range(n):
        out[i, np.arange(3), r.permutation(3)] = r.choice([-1.0, 1.0], 3)
    return out.reshape(n, 9)


ANGLE_EDGES = [('angle 1e-7', lambda r, n: np.full(n, 1e-7)), ('angle 0.5e-3 .. 2e-3', lambda r, n: r.uniform(0.5e-3, 2e-3, n)), ('angle 0.1', lambda r, n: np.full(n, 0.1)),
               ('angle pi - 1e-6', lambda r, n: np.full(n, np.pi - 1e-6)), ('angle pi - 1e-3', lambda r, n: np.full(n, np.pi - 1e-3))]


def _rotvec_cases(name, consts, as_quat):
    """the classes of rotvec_of (v, w) -- as_quat: the same quaternions for axis_angle_scaled"""
    r = _rng(name)
    out = [Case('exact', [[0, 0, 0, 1], [0, 0, 0, 2], [0, 0, 0, 0.5], [0, 0, 0, -1]], consts)]
    q = _quat_of(_unit(r, N), r.uniform(0, np.pi, N)) * r.choice([-1.0, 1.0], N)[:, None]
    out.append(Case('random unit, both signs of w', q, consts))
    for tag, f in ANGLE_EDGES:
        q = _quat_of(_unit(r, 512), f(r, 512)) * r.choice([-1.0, 1.0], 512)[:, None]
        out.append(Case('edges: ' + tag, q, consts))
    z = np.zeros((8, 4)); z[:, 3] = [1, -1, 0.5, -0.0, 0.0, 2, -0.25, 1e-3]
    out.append(Case('edges: v = 0', z, consts))
    if not as_quat:
        v = _unit(r, N) * r.uniform(0, 1, N)[:, None]
        out.append(Case('random non-unit, |v| <= 1, w in [-1, 2]', np.concatenate([v, r.uniform(-1, 2, (N, 1))], axis=1), consts))
        v = _unit(r, 64); v[:, :] *= r.uniform(0.1, 1, (64, 1))
        out.append(Case('edges: w = -0', np.concatenate([v, np.full((64, 1), -0.0)], axis=1), consts))
    else:
        out.append(Case('edges: angle 1e-9 1e-8 1e-7', _quat_of(_unit(r, 192), np.repeat([1e-9, 1e-8, 1e-7], 64)), consts))
    return out


def _quat_of_rotvec_cases(name, consts):
    r = _rng(name)
    out = [Case('exact', [[0, 0, 0]], consts), Case('random angle < 2 pi', _unit(r, N) * r.uniform(0, 2 * np.pi, (N, 1)), consts)]
    for tag, a in [('angle 1e-7', 1e-7), ('angle 1', 1.0), ('angle pi', np.pi), ('angle 2 pi - 1e-3', 2 * np.pi - 1e-3)]:
        out.append(Case('edges: ' + tag, _unit(r, 256) * a, consts))
    out.append(Case('edges: angle 0.5e-3 .. 2e-3', _unit(r, 512) * r.uniform(0.5e-3, 2e-3, (512, 1)), consts))
    return out


def _spd6(r, n):
    """the base block: mass 5 - 15 on the linear diagonal, inertia 0.02 - 1 on the angular, coupling from a COM offset <= 0.2 m; angular part first"""
    from scipy.spatial.transform import Rotation as R
    m, c = r.uniform(5, 15, n), _unit(r, n) * r.uniform(0, 0.2, (n, 1))
    Rm = R.from_quat(_unit(r, n, 4)).as_matrix()
    Ic = np.einsum('nij,nj,nkj->nik', Rm, r.uniform(0.02, 1, (n, 3)), Rm)
    cx = np.zeros((n, 3, 3))
    cx[:, 0, 1], cx[:, 0, 2], cx[:, 1, 0], cx[:, 1, 2], cx[:, 2, 0], cx[:, 2, 1] = -c[:, 2], c[:, 1], c[:, 2], -c[:, 0], -c[:, 1], c[:, 0]
    A = np.zeros((n, 6, 6))
    A[:, :3, :3] = Ic + m[:, None, None] * (np.einsum('ni,ni->n', c, c)[:, None, None] * np.eye(3) - np.einsum('ni,nj->nij', c, c))
    A[:, :3, 3:] = m[:, None, None] * cx
    A[:, 3:, :3] = np.transpose(A[:, :3, 3:], (0, 2, 1))
    A[:, 3:, 3:] = m[:, None, None] * np.eye(3)
    return A


IL = np.tril_indices(6)


def _int_factor(r, n):
    """lower-triangular factors with small whole numbers below a power-of-two diagonal: A = L L^T, its factor and every intermediate are whole numbers"""
    L = np.tril(r.integers(-2, 3, size=(n, 6, 6)).astype(np.float64), -1)
    L[:, np.arange(6), np.arange(6)] = 2.0 ** r.integers(0, 3, size=(n, 6))
    return L


def seg_cases(consts):
    r = _rng('seg_seg_st')
    def seg(n, lo=0.1, hi=0.4):
        p = r.uniform(-0.3, 0.3, (n, 3)); return p, p + _unit(r, n) * r.uniform(lo, hi, (n, 1))
    out = [Case('exact', [[0, 0, 0, 4, 0, 0, 8, 2, 1, 8, 4, 1], [0, 0, 0, 0, 2, 0, 1, -4, 0, 1, -8, 2], [1, 1, 1, 1, 1, 3, -2, -2, -4, -2, -2, -8], [0, 0, 0, 1, 0, 0, 4, 1, 0, 8, 2, 0]], consts,
                note='the closest points are end points: s and t clamp to 0 or 1')]
    p1, q1 = seg(N); p2, q2 = seg(N)
    out.append(Case('random general position', np.concatenate([p1, q1, p2, q2], axis=1), consts))
    for ang in (0.0, 1e-6, 1e-3):
        p1, q1 = seg(512)
        d1 = q1 - p1
        perp = np.cross(d1, _unit(r, 512)); perp /= np.linalg.norm(perp, axis=1, keepdims=True)
        d2 = (d1 / np.linalg.norm(d1, axis=1, keepdims=True) * np.cos(ang) + perp * np.sin(ang)) * r.uniform(0.1, 0.4, (512, 1))
        p2 = p1 + np.cross(d1, perp) / np.linalg.norm(d1, axis=1, keepdims=True) * r.uniform(0.02, 0.1, (512, 1)) + d1 * r.uniform(-0.5, 0.5, (512, 1))
        out.append(Case('edges: parallel within %g rad' % ang, np.concatenate([p1, q1, p2, p2 + d2], axis=1), consts))
    p1, q1 = seg(512); x = p1 + (q1 - p1) * r.uniform(0.1, 0.9, (512, 1)); d2 = _unit(r, 512) * r.uniform(0.1, 0.4, (512, 1)); tt = r.uniform(0.1, 0.9, (512, 1))
    out.append(Case('edges: intersecting', np.concatenate([p1, q1, x - d2 * tt, x + d2 * (1 - tt)], axis=1), consts))
    p1, q1 = seg(512); p2, q2 = seg(512)
    sh = np.concatenate([p1, q1, q1, q1 + (q2 - p2)], axis=1); sh[256:, 6:9], sh[256:, 9:12] = (p1 + (q2 - p2))[256:], p1[256:]
    out.append(Case('edges: shared end points', sh, consts))
    return out


BOXES = [(0.6, 0.02, 0.15), (0.6, 0.02, 0.3), (1.2, 0.3, 0.075), (1.2, 0.3, 0.15)]       # hurdle bars and stair treads: x, y, z sizes (m)


def sdf_cases(consts):
    """one record and one frame per row (16 lanes share them), one point per lane.  Point classes per lane: inside, on a face, outside a face, an edge, a corner,
    on and near the rod axis, just outside (e2 flushes on the device)"""
    r = _rng('terrain_sdf')
    out = []
    def rows(n_rows, yaws, rods, flush=False, kinds=(0, 2, 3, 4, 7)):
        X = np.zeros((n_rows * 16, 16))
        for i in range(n_rows):
            sx, sy, sz = BOXES[i % len(BOXES)]
            c = r.uniform(-1, 1, 3) * [2, 2, 0] + [0, 0, 0.5 * sz + (0.3 if rods[i % len(rods)] < 0 else 0.0)]
            rec = np.array([c[0] - sx / 2, c[0] + sx / 2, c[1] - sy / 2, c[1] + sy / 2, c[2] - sz / 2, c[2] + sz / 2, rods[i % len(rods)], 0.01])
            lo, hi = rec[[0, 2, 4]], rec[[1, 3, 5]]
            yaw = yaws[i % len(yaws)]
            frame = [0.0 if yaw is None else 1.0, 1.5, -0.75, 1.0 if yaw is None else np.cos(yaw), 0.0 if yaw is None else np.sin(yaw)]
            for l in range(16):
                kind = kinds[l % len(kinds)]
                u = r.uniform(0.1, 0.9, 3)
                P = lo + (hi - lo) * u                                            # 0: inside
                ax, side = r.integers(3), r.integers(2)
                if flush:      # below the bottom face z0 = 0 of a box that stands on the ground, by 1e-30 .. 1e-19: the square of the distance is below 1.2e-38
                    P[2] = -10.0 ** r.uniform(-30, -19.05)
                elif kind == 1: P[ax] = np.float32(hi[ax] if side else lo[ax])     # on a face
                elif kind == 2: P[ax] = (hi[ax] + r.uniform(0.001, 0.1)) if side else (lo[ax] - r.uniform(0.001, 0.1))      # outside a face
                elif kind == 3:                                                   # outside an edge
                    for a in {ax, (ax + 1) % 3}: P[a] = hi[a] + r.uniform(0.001, 0.1) if r.integers(2) else lo[a] - r.uniform(0.001, 0.1)
                elif kind == 4:                                                   # outside a corner
                    for a in range(3): P[a] = hi[a] + r.uniform(0.001, 0.1) if r.integers(2) else lo[a] - r.uniform(0.001, 0.1)
                elif kind in (5, 6):                                              # on the rod axis / inside the rod radius (within the record's y range)
                    ze = hi[2] if rec[6] >= 0 else lo[2]
                    P = np.array([rec[r.integers(2)], lo[1] + (hi[1] - lo[1]) * u[1], ze])
                    if kind == 6: P += np.array([np.cos(u[0] * 6.28), 0, np.sin(u[0] * 6.28)]) * r.uniform(0.002, 0.009)
                elif kind == 7:                                                   # above / beside the rods, outside their radius
                    ze = hi[2] if rec[6] >= 0 else lo[2]
                    P = np.array([rec[r.integers(2)] + r.uniform(-0.03, 0.03), lo[1] + (hi[1] - lo[1]) * u[1], ze + r.uniform(-0.03, 0.03)])
                if yaw is not None:                                               # the point is built in the record's frame and handed over in world coordinates
                    cs, sn = frame[3], frame[4]
                    P = np.array([frame[1] + P[0] * cs - P[1] * sn, frame[2] + P[0] * sn + P[1] * cs, P[2]])
                X[i * 16 + l] = np.concatenate([rec, P, frame])
        return X
    pow2 = np.zeros((64, 16)); pow2[:, :8] = [-2, 2, -1, 1, 0, 0.5, 0, 0]; pow2[:, 11:] = [0, 0, 0, 1, 0]
    pts = [[0, 0, 0.25], [1.5, 0.5, 0.25], [0, 0, 1], [0, 3, 0.25], [-4, 0, 0.125], [1, 0.5, 0.375], [0.5, -0.75, 0.25], [0, 0, -1]]
    pow2[:, 8:11] = np.array(pts * 8)
    out.append(Case('exact', pow2, consts, note='inside and outside a face of a box with power-of-two faces'))
    for yaw, tag in ((None, 'not yawed'), (0.0, 'yaw 0'), (0.3, 'yaw 0.3'), (np.pi / 2, 'yaw pi/2')):
        out.append(Case('random %s' % tag, rows(256, [yaw], [0.0, 1.0, -1.0]), consts))
        out.append(Case('edges: on a face, on the rod axis, inside the rod radius, %s' % tag, rows(48, [yaw], [0.0, 1.0, -1.0], kinds=(1, 5, 6)), consts))
    out.append(Case('edges: outside by less than 1.1e-19', rows(16, [None], [0.0], flush=True), consts, note='flush'))
    return out


def mocap_cases(consts):
    """one frame pair a launch (the double table); rows: frac {0, 2^-24, 0.5, 1 - 2^-24} x frame step {1/30, 1/120} x want_vel {1, 0}.  -> cases with .frames"""
    from scipy.spatial.transform import Rotation as R
    r = _rng('mocap')
    combos = np.array([[f, fs, wv] for f in (0.0, 2.0 ** -24, 0.5, 1 - 2.0 ** -24) for fs in (np.float32(1 / 30), np.float32(1 / 120)) for wv in (1.0, 0.0)], dtype=np.float64)
    X = np.repeat(combos, 16, axis=0)
    out = []
    def pair(tag, fc, fn, klass='edges'):
        c = Case('%s: %s' % (klass, tag) if klass == 'edges' else klass, X, consts, auxd=np.concatenate([fc, fn]))
        c.frames = (fc, fn)
        out.append(c)
    def frame(q): return np.concatenate([r.uniform(-1, 1, 3), q, r.uniform(-1, 1, 12)])
    fc = np.concatenate([[1, -2, 0.5], [0, 0, 0, 1], np.arange(12) - 6.0]); fn = fc.copy(); fn[:3] += [0.5, 1, -2]; fn[7:] += 0.5
    pair('exact', fc, fn, klass='exact')
    for ang, tag in [(0.0, 'identity'), (1e-6, '1e-6 rad'), (0.7e-3, '0.7e-3 rad'), (1.4e-3, '1.4e-3 rad'), (0.05, '0.05 rad'), (3.0, '3.0 rad')]:
        qc = R.from_quat(_unit(r, 1, 4)[0])
        qn = R.from_rotvec(_unit(r, 1)[0] * ang) * qc
        pair('rotation ' + tag, frame(qc.as_quat()), frame(qn.as_quat() if ang else qc.as_quat()))
    qc = R.from_quat(_unit(r, 1, 4)[0])
    pair('antipodal sign', frame(qc.as_quat()), frame(-(R.from_rotvec(_unit(r, 1)[0] * 0.01) * qc).as_quat()))
    z = np.load(os.path.join(ROOT, 'lifelike_agility_and_play_amd', 'assets', 'mocap_f64.npz'))
    fr, ends = z['frames'], np.cumsum(z['clip_len'])
    ok = np.ones(len(fr) - 1, dtype=bool); ok[ends[:-1] - 1] = False                  # consecutive frames of ONE clip
    ang = (R.from_quat(fr[1:, 3:7]) * R.from_quat(fr[:-1, 3:7]).inv()).magnitude()
    for i in np.argsort(np.where(ok, ang, -1))[-10:]:
        pair('file frames %d, %d (%.3f rad)' % (i, i + 1, ang[i]), fr[i], fr[i + 1])
    return out


def cases(name, dims):
    """[Case]: the exact class first, then the random ones, then the edges"""
    r, mc, ic = _rng(name), model_consts(dims), integer_consts(dims)
    h = HELPERS[name]
    if name in ('v3ops', 'm3ops', 'svops', 'qmul', 'qmul_t', 'qmat', 'lm_fwd_bwd'):
        w = dict(v3ops=7, m3ops=27, svops=33, qmul=8, qmul_t=8, qmat=4, lm_fwd_bwd=18)[name]
        ex, rn = _ints(r, 256, w), r.normal(size=(N, w))
        if name == 'lm_fwd_bwd':
            ex[:, 6:9] = 2.0 ** r.integers(-2, 1, (256, 3)); rn[:, 6:9] = r.uniform(0.5, 2, (N, 3))
        return [Case('exact', ex, mc), Case('random', rn, mc)]
    if name == 'moves':
        ed = np.zeros((64, 21), dtype=np.float32); ed[:, :] = np.array([0.0, -0.0, 2e-38, -3e38, 2.0 ** -126, 1.0, -1.0] * 3)[None, :]
        return [Case('exact', _ints(r, 64, 21), mc), Case('random', r.normal(size=(N, 21)), mc), Case('edges: +-0, extremes', ed, mc)]
    if name == 'qconj_t':
        return [Case('exact', _ints(r, 64, 4), mc), Case('random', r.normal(size=(N, 4)), mc)]
    if name == 'philox':
        bits = r.integers(0, 2 ** 32, size=(N, 6), dtype=np.uint64).astype(np.uint32)
        bits[:4] = [[0] * 6, [0xffffffff] * 6, [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0xA4093822, 0x299F31D0]]
        return [Case('random', bits.view(np.float32), mc)]
    if name in ('qnormalize', 'qnormalize_t'):
        q = _unit(r, N, 4)
        near = _unit(r, 1024, 4).astype(np.float32).astype(np.float64) * (1 + r.uniform(-1e-6, 1e-6, (1024, 1)))
        return [Case('exact', [[0, 0, 0, 2], [0, 4, 0, 0], [-0.5, 0, 0, 0], [0, 0, 1, 0], [2, 2, 2, 2], [1, -1, 1, -1]], mc), Case('random |q| in [0.5, 2]', q * r.uniform(0.5, 2, (N, 1)), mc),
                Case('edges: |q| within 1e-6 of 1', near, mc)]
    if name in ('rotvec_of', 'rotvec_of_t'): return _rotvec_cases(name, mc, False)
    if name in ('axis_angle_scaled', 'axis_angle_scaled_t'): return _rotvec_cases(name, mc, True)
    if name in ('quat_of_rotvec', 'quat_of_rotvec_t'): return _quat_of_rotvec_cases(name, mc)
    if name == 'quat_of_small_rotvec':
        below = _unit(r, 256) * np.sqrt(1 - r.uniform(1e-5, 1e-3, (256, 1)))
        return [Case('exact', [[0, 0, 0]], mc), Case('random a2 < 1', _unit(r, N) * np.sqrt(r.uniform(0, 1 - 1e-5, (N, 1))), mc), Case('edges: a2 just below 1', below, mc),
                Case('edges: a2 = 1 (the fallback)', [[1, 0, 0], [0, -1, 0], [0, 0, 1], [-1, 0, 0]], mc)]
    if name == 'sincos_joint':
        out = [Case('exact', [[0.0], [-0.0]], mc)]
        for lim in (0.78, 3.2, 6.3, 1e3):
            out.append(Case('random |x| <= %g' % lim, r.uniform(-lim, lim, (N, 1)), mc))
        k = np.arange(-8, 9)
        xs = []
        for kk in k:
            x0 = np.float32(kk * np.pi / 2)
            xs += [x0, np.nextafter(x0, np.float32(np.inf)), np.nextafter(x0, np.float32(-np.inf)), np.float32(kk * np.pi / 2 + 1e-4), np.float32(kk * np.pi / 2 - 1e-4)]
        out.append(Case('edges: k pi/2 +- {0, 1 ulp, 1e-4}, k = -8 .. 8', np.array(xs)[:, None], mc))
        return out
    if name in ('leg_fk', 'foot_world'):
        from lifelike_agility_and_play_amd import urdf_model as um
        b = model_blob()
        lo, hi = b[um.OFF_Q_LO:um.OFF_Q_LO + 12].reshape(4, 3), b[um.OFF_Q_HI:um.OFF_Q_HI + 12].reshape(4, 3)
        leg = Ctx.leg(N)
        q = np.repeat(r.uniform(0, 1, (N // 4, 3)), 4, axis=0) * (hi[leg] - lo[leg] + 1.0) + lo[leg] - 0.5        # one pose per leg: its four sub-lanes hold the same angles
        if name == 'leg_fk':
            return [Case('exact', np.zeros((64, 3)), ic, note='q = 0 with whole-number tables'), Case('random, limits widened by 0.5 rad', q, mc)]
        pose = np.repeat(np.concatenate([r.uniform(-2, 2, (N // 16, 3)), _rotmats(r, N // 16)], axis=1), 16, axis=0)
        exp = np.repeat(np.concatenate([_ints(r, 4, 3), _perm_mats(r, 4)], axis=1), 16, axis=0)
        return [Case('exact', np.concatenate([np.zeros((64, 3)), exp], axis=1), ic), Case('random, limits widened by 0.5 rad', np.concatenate([q, pose], axis=1), mc)] + golden_feet_cases(mc)
    if name in ('own_link_inertia', 'link_inertia'):
        return [Case('exact', np.concatenate([_perm_mats(r, 64), _ints(r, 64, 3)], axis=1), ic, targ=t) for t in h['targs']] + \
               [Case('random', np.concatenate([_rotmats(r, N), r.normal(size=(N, 3)) * 0.3], axis=1), mc, targ=t) for t in h['targs']]
    if name in ('damping_force', 'damping_force_t'):
        def mk(n, vel):
            A = r.normal(size=(n, 3, 3)) * 0.1
            S = np.einsum('nij,nkj->nik', A, A)
            kd = np.full((n, 1), 0.04) if name == 'damping_force' else np.repeat(r.uniform(0.01, 0.1, (n // 16, 1)), 16, axis=0)
            return np.concatenate([vel, r.normal(size=(n, 3)) * 0.1, S[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]], r.uniform(0.1, 2, (n, 1)), kd], axis=1)
        ex = np.concatenate([_ints(r, 64, 6, -1, 1) * 0, _ints(r, 64, 9), np.ones((64, 1)), np.full((64, 1), 0.5)], axis=1)
        ex[:, 0], ex[:, 5] = 0, 0; ex[:, 2], ex[:, 3] = 3, 4          # w = (0, 0, 3), v = (4, 0, 0): |w| = 3 and, with com = 0, |vc| = 4
        ex[:, 6:9] = 0
        return [Case('exact', ex, mc), Case('random', mk(N, r.normal(size=(N, 6))), mc), Case('edges: v = 0', mk(64, np.zeros((64, 6))), mc)]
    if name == 'chol_solve':
        L = _int_factor(r, 64)
        A = np.einsum('nij,nkj->nik', L, L)
        return [Case('exact', np.concatenate([A[:, IL[0], IL[1]], np.einsum('nij,nj->ni', A, _ints(r, 64, 6, -2, 2).astype(np.float64))], axis=1), mc, note='whole-number factor'),
                Case('random base-block inertia', np.concatenate([_spd6(r, N)[:, IL[0], IL[1]], r.normal(size=(N, 6))], axis=1), mc)]
    if name == 'fwd_bwd6':
        Li = _int_factor(r, 64)
        Lr = np.linalg.cholesky(_spd6(r, N))
        f = lambda L, x: np.concatenate([L[:, IL[0], IL[1]], 1.0 / L[:, np.arange(6), np.arange(6)], x], axis=1)
        return [Case('exact', f(Li, _ints(r, 64, 6)), mc), Case('random', f(Lr, r.normal(size=(N, 6))), mc)]
    if name == 'plane_space':
        n = _unit(r, N)
        z = (0.70710678 + r.uniform(1e-6, 1e-3, 512) * r.choice([-1, 1], 512)) * r.choice([-1, 1], 512)
        ph = r.uniform(0, 2 * np.pi, 512)
        nz = np.stack([np.sqrt(1 - z * z) * np.cos(ph), np.sqrt(1 - z * z) * np.sin(ph), z], axis=1)
        axes = np.concatenate([np.eye(3), -np.eye(3)])
        return [Case('exact', axes, mc), Case('random unit normals', n, mc), Case('edges: |n.z| within 1e-3 of 0.70710678', nz, mc, note='threshold')]
    if name == 'row_bias':
        par = [0.2, 0.8, -0.02, 0.04]      # erp, erp_deep, erp_deep_below, max_depen
        d = np.concatenate([r.uniform(1e-4, 0.05, N // 4), -r.uniform(1e-4, 0.019, N // 4), -r.uniform(0.021, 0.1, N // 2)])
        X = np.concatenate([d[:, None], np.full((N, 1), 500.0), np.tile(par, (N, 1))], axis=1)
        ex = np.array([[0.0, 512, 0.25, 0.5, -0.125, 64], [-0.0, 512, 0.25, 0.5, -0.125, 64], [0.5, 512, 0.25, 0.5, -0.125, 64], [-0.0625, 512, 0.25, 0.5, -0.125, 64], [-0.25, 512, 0.25, 0.5, -0.125, 64],
                       [-0.25, 512, 0.25, 0.5, -0.125, 2], [-0.125, 512, 0.25, 0.5, -0.125, 64]])
        return [Case('exact', ex, mc, note='d = +-0, both sides of 0 and of erp_deep_below, the cap'), Case('random, d on both sides of 0 and of erp_deep_below', X, mc)]
    if name == 'clip1':
        x = r.normal(size=(N, 1)) * 3
        ed = np.array([[2, 2], [-2, 2], [2.5, 2], [-2.5, 2], [1e30, 2], [-1e30, 2], [np.nan, 2], [0, 2], [-0.0, 2], [1, 2]])
        return [Case('exact', ed, mc, note='x at +-vmax, beyond, NaN'), Case('random', np.concatenate([x, np.full((N, 1), 2.0)], axis=1), mc)]
    if name == 'seg_seg_st': return seg_cases(mc)
    if name == 'terrain_sdf': return sdf_cases(mc)
    if name == 'mocap': return mocap_cases(mc)
    raise KeyError(name)


def golden_feet_cases(mc):
    """foot_world at the poses of the PMC golden (g3_state: base pose and joint angles the reference visited), against the chain product scipy forms from the model blob
    -- the statement tests/test_oracle_physics.py pins the oracle's feet to at 1e-12.  (The feet the golden itself stores, g4_feet_* / g5_feet_*, are scripted inputs of
    the reward, not the forward kinematics of the states next to them.)"""
    from scipy.spatial.transform import Rotation as R
    from lifelike_agility_and_play_amd import urdf_model as um
    g, b = np.load(os.path.join(ROOT, 'tests', 'golden', 'pmc_golden.npz')), model_blob()
    jo, ax = b[um.OFF_JOINT_ORIGIN:um.OFF_JOINT_ORIGIN + 36].reshape(12, 3), b[um.OFF_JOINT_AXIS:um.OFF_JOINT_AXIS + 36].reshape(12, 3)
    fp = b[um.OFF_FOOT_POS:um.OFF_FOOT_POS + 12].reshape(4, 3)
    X, want = [], []
    for s in g['g3_state'][:16]:
        Rb = R.from_quat(s[3:7])
        Rm = Rb.as_matrix().astype(np.float32)
        p32 = s[0:3].astype(np.float32)
        for lane in range(16):
            l = lane // 4
            q32 = s[13 + 3 * l:16 + 3 * l].astype(np.float32)
            pos, rot = p32.astype(np.float64), R.from_matrix(Rm.astype(np.float64))     # (the chain starts from the float32 pose the helper is handed)
            for j in range(3):
                pos = pos + rot.apply(jo[3 * l + j].astype(np.float32).astype(np.float64))
                rot = rot * R.from_rotvec(ax[3 * l + j] * np.float64(q32[j]))
            X.append(np.concatenate([q32, p32, Rm.reshape(9)])); want.append(pos + rot.apply(fp[l].astype(np.float32).astype(np.float64)))
    c = Case('edges: the poses of the PMC golden', np.array(X), mc)
    c.golden = np.array(want)
    return [c]


# ---- what is asked of an answer ------------------------------------------------------------------------------------------------------------------------
_WANT = {}


def want(name, case, dims):
    """-> dict(v [n, words] statement, twin [n, words] the twin's bound, madd [n, words] the multiply-add bound, extra ...); cached per case object"""
    key = id(case)
    if key in _WANT:
        return _WANT[key]
    h = HELPERS[name]
    with np.errstate(invalid='ignore'):
        X = case.X.astype(np.float64)
    ctx = Ctx(dims, case.consts, case.targ)
    w = {}
    if name in ('moves', 'qconj_t', 'philox'):
        if name == 'philox':
            import philox_ref
            b = case.X.view(np.uint32).astype(np.uint64)
            o = philox_ref.philox4x32_10(*[b[:, i] for i in range(6)])
            u = philox_ref.u01_from(o[0], o[1]).view(np.uint64)
            w['bits'] = np.stack(list(o) + [(u & np.uint64(0xffffffff)).astype(np.uint32), (u >> np.uint64(32)).astype(np.uint32)], axis=1).astype(np.uint32)
        else:
            v = case.X.copy()
            v[:, 0 if name == 'qconj_t' else 9:(3 if name == 'qconj_t' else 12)] *= -1.0
            with np.errstate(invalid='ignore'):
                if name == 'qconj_t':
                    v[:, :3] = np.float32(0.0) - case.X[:, :3]       # the lane-varying form subtracts from zero: +0 stays +0
            w['bits'] = np.ascontiguousarray(v).view(np.uint32)
    elif name == 'terrain_sdf':
        d, n, isb, margin = ref.terrain_sdf(X, ctx)
        b = ref.terrain_sdf_bound(X, d)
        w['v'] = np.concatenate([d[:, None], n, isb[:, None]], axis=1)
        sure = margin > 1e-5
        w['sure'] = sure
        dist = np.where(isb > 0.5, np.where(d > 0, d, np.inf), d + X[:, 7])         # what n was divided by: the distance outside a box, the distance to the rod's axis
        bn = np.where(np.isinf(dist), 4 * U, np.minimum(2.0, b / np.maximum(dist, 1e-30) + 4 * U))
        bb = np.concatenate([b[:, None], np.repeat(bn[:, None], 3, axis=1), np.zeros((len(X), 1))], axis=1)
        w['v'][~sure, 1:] = np.nan
        if case.note == 'flush':       # the device flushes e2 and answers the face's normal, the twin divides by the root of a denormal: only d, and a unit normal, are asked
            w['v'][:, 1:] = np.nan
            e2 = X[:, 10] ** 2
            w['unit_tol'] = np.where(e2 >= 2.0 ** -150, 2.0 ** -149 / np.maximum(e2, 2.0 ** -150), 0.0)     # the spacing of a denormal e2 relative to it
        w['twin'] = w['madd'] = bb
    elif name == 'mocap':
        fc, fn = case.frames
        n = len(X)
        leg = Ctx.leg(n)
        v = np.zeros((n, 19))
        for i in range(0, n, 16):
            p, q, vv, ww, jp, jv = ref.mocap(fc, fn, X[i, 0], X[i, 1], X[i, 2] > 0.5)
            v[i:i + 16, :13] = np.concatenate([p, q, vv, ww])
            for j in range(3):
                v[i:i + 16, 13 + j], v[i:i + 16, 16 + j] = jp[3 * leg[:16] + j], jv[3 * leg[:16] + j]
        FC, FN = np.tile(fc, (n, 1)), np.tile(fn, (n, 1))
        mv, mt = ref.mocap_model(FC, FN, X[:, 0], X[:, 1], X[:, 2] > 0.5, 'twin')
        _, mm = ref.mocap_model(FC, FN, X[:, 0], X[:, 1], X[:, 2] > 0.5, 'madd')
        sign = np.where(np.einsum('ni,ni->n', mv[:, 3:7], v[:, 3:7]) < 0, -1.0, 1.0)      # scipy's Slerp answers a rotation: the quaternion's sign follows the helper's
        v[:, 3:7] *= sign[:, None]
        w['model_v'] = mv
        jb = U * np.abs(v[:, 13:]) * 1.001 + 1e-300
        w['v'], w['twin'], w['madd'] = v, np.concatenate([mt, jb], axis=1), np.concatenate([mm, jb], axis=1)
    else:
        mv, mt = ref.model(name, X, ctx, 'twin', h['words'])
        _, mm = ref.model(name, X, ctx, 'madd', h['words'])
        w['model_v'], w['twin'], w['madd'] = mv, mt, mm
        w['v'] = mv
        if name in ref.STATEMENTS:
            sv = ref.STATEMENTS[name](X, ctx)
            w['v'] = mv.copy()
            w['v'][:, :sv.shape[1]] = np.where(np.isnan(sv), mv[:, :sv.shape[1]], sv)
        if name == 'quat_of_small_rotvec':          # held to its own comment: the series is within 1e-9 of the true quaternion for h <= 0.5, plus rounding
            w['v'] = ref.s_quat_of_rotvec(X, ctx)
            w['twin'], w['madd'] = mt + 1e-9, mm + 1e-9
        if name == 'seg_seg_st':
            fr = ref.seg_seg_fragile(X)
            w['fragile'] = fr
            w['gap'] = np.linalg.norm(w['v'][:, 0:3] - w['v'][:, 3:6], axis=1)
            w['gap_bound'] = {k: np.linalg.norm(w[k][:, :6], axis=1) * 2 for k in ('twin', 'madd')}
            w['v'][fr] = np.nan
        if name == 'plane_space' and case.note == 'threshold':
            w['v'][:] = np.nan                      # (near the threshold only the frame's own properties are held: orthonormal below)
    _WANT[key] = w
    return w


def _bits_equal(a, b):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) == np.ascontiguousarray(b, dtype=np.float32).view(np.uint32)


def check(name, case, got, dims, who, bar='twin', dev_host=None, active=0b1111, limit=None):
    """Holds the answer `got` [n, n_out] of `who` to the statement; -> dict(err [words] worst |answer - statement| over the class, ratio worst error / bar).
    bar: 'twin' (the twin's own forward bound) or 'gpu' (max(4 dev_host, multiply-add bound) for APPROX, the multiply-add bound for MADD)."""
    h, w = HELPERS[name], want(name, case, dims)
    n = case.n if limit is None else min(case.n, limit)
    words = h['words']
    rows_on = ((active >> ((np.arange(len(got)) // 16) % 4)) & 1).astype(bool)
    on = rows_on.copy(); on[n:] = False
    head = '%s [%s, targ %d] %s' % (name, case.klass, case.targ, who)
    assert np.isnan(got[~rows_on]).all(), head + ': a row outside EXEC wrote'
    assert np.isnan(got[:, words:]).all(), head + ': a word past the helper\'s outputs was written'
    g = got[:, :words]
    if 'bits' in w:
        same = g.view(np.uint32) == w['bits']
        assert same[on].all(), head + ': differs from the statement in bits at sample %d' % np.argwhere(~same & on[:, None])[0][0]
        return dict(err=np.zeros(words), ratio=0.0, word=0, bar=0.0)
    v = w['v']
    cmp_ = ~np.isnan(v) & on[:, None]
    with np.errstate(invalid='ignore'):
        finite_ok = np.isfinite(g) | ~cmp_ | np.isnan(v)
        if name == 'clip1':
            nan_in = np.isnan(case.X[:, 0])
            assert np.isnan(g[nan_in & on, 0]).all(), head + ': a NaN did not stay a NaN'
            cmp_[nan_in] = False
            finite_ok[nan_in] = True
        assert finite_ok.all(), head + ': a non-finite answer at sample %d' % np.argwhere(~finite_ok)[0][0]
        err = np.where(cmp_, np.abs(g.astype(np.float64) - v), 0.0)
    if case.klass == 'exact':          # (every intermediate of the model is a float32 here, so its value is THE answer: np.linalg's own rounding does not enter)
        want32 = np.where(np.isnan(v), np.nan, w.get('model_v', v)[:, :words] if name != 'mocap' else v).astype(np.float32)
        same = (g == want32) & ((np.signbit(g) == np.signbit(want32)) | (name in ZERO_SIGN_FREE)) | ~cmp_
        assert same.all(), head + ': exact inputs, but the answer is not the statement\'s float32 at sample %d word %d (%r, %r)' % (
            *np.argwhere(~same)[0], g[tuple(np.argwhere(~same)[0])], want32[tuple(np.argwhere(~same)[0])])
    if bar == 'twin' or h['cls'] == MADD:
        b = w['twin' if (bar == 'twin' and h['cls'] != MADD) else 'madd']
    else:
        b = np.maximum(4.0 * dev_host[None, :], w['madd'])
    b = np.where(cmp_, b, np.inf)
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where(err > 0, err / b, 0.0)
    bad = np.argwhere(ratio > 1.0)
    assert not len(bad), head + ': |answer - statement| = %.3e above the bar %.3e at sample %d word %d (%d such)' % (err[tuple(bad[0])], b[tuple(bad[0])], *bad[0], len(bad))
    worst = float(ratio.max()) if ratio.size else 0.0
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)          # where error / bar is worst: the table's line
    at_word, at_bar = int(at[1]), float(b[at]) if np.isfinite(b[at]) else 0.0
    # ---- what single helpers are held to beside the statement --------------------------------------------------------------------------------------
    gd = g.astype(np.float64)
    kb = 'twin' if bar == 'twin' else 'madd'
    if name in ('qnormalize', 'qnormalize_t'):
        dn = np.abs(np.linalg.norm(gd[on], axis=1) - 1.0)
        assert (dn <= 4 * U).all(), head + ': the norm of the result is %.2e from 1 (4 u = %.2e)' % (dn.max(), 4 * U)
    if name == 'sincos_joint':
        assert (err[np.abs(case.X[:, 0]) <= 1e3] <= 9e-8).all(), head + ': %.3e from sin / cos, above 1.5 ulp (9e-8)' % err.max()
    if name == 'plane_space':
        nrm, p, q = case.X[on, :3].astype(np.float64), gd[on, 0:3], gd[on, 3:6]
        dots = np.abs(np.stack([np.einsum('ni,ni->n', p, p) - 1, np.einsum('ni,ni->n', q, q) - 1, np.einsum('ni,ni->n', p, q), np.einsum('ni,ni->n', p, nrm), np.einsum('ni,ni->n', q, nrm)]))
        tol = 16 * U + np.abs(np.einsum('ni,ni->n', nrm, nrm) - 1)           # a handful of roundings of unit quantities; the normal's own distance from unit length
        assert (dots <= tol[None, :]).all(), head + ': the tangent frame is not orthonormal (%.2e)' % dots.max()
    if name == 'seg_seg_st':
        fr = w['fragile'] & on
        gap = np.linalg.norm(gd[:, 0:3] - gd[:, 3:6], axis=1)
        ge = np.abs(gap - w['gap'])[fr]
        gb = (w['gap_bound'][kb] if (bar == 'twin' or dev_host is None) else np.maximum(w['gap_bound'][kb], 4 * dev_host[:6].max()))[fr]
        assert (ge <= gb).all(), head + ': |c1 - c2| off by %.2e on a sample left out of the (s, t) comparison' % ge.max()
        if case.klass.startswith('random'):
            assert fr.sum() <= 0.05 * on.sum(), head + ': %d of %d samples left out of the (s, t) comparison' % (fr.sum(), on.sum())
    if name == 'terrain_sdf':
        share = 1.0 - w['sure'][on].mean()
        if case.klass.startswith('random'):
            assert share <= 0.05, head + ': %.1f %% of the samples left out of the n / is_box comparison' % (100 * share)
        nn = np.linalg.norm(gd[on, 1:4], axis=1)
        assert np.isfinite(got[on, :5]).all() and (np.abs(nn - 1) <= 8 * U + w.get('unit_tol', np.zeros(len(on)))[on]).all(), head + ': a normal that is not finite and of unit length'
    if name == 'foot_world' and hasattr(case, 'golden'):
        eg = np.abs(gd[on] - case.golden[:on.sum()])
        assert (eg <= np.where(cmp_, b, 0)[on] + 1e-9).all(), head + ': %.2e from the feet of the PMC golden' % eg.max()
    return dict(err=err.max(axis=0), ratio=worst, word=at_word, bar=at_bar)


def partial_exec_check(runner, policy, name, case, dims, full, who):
    """rows {0, 1} and row {2} alone of ONE wave: the active rows answer what they answered in the whole wave, the others write nothing"""
    for active in ACTIVE_ROWS[1:]:
        got = runner.run(policy, name, case, active, limit=64)
        rows_on = ((active >> (np.arange(64) // 16)) & 1).astype(bool)
        assert np.isnan(got[~rows_on]).all(), '%s [%s] %s: a row outside EXEC %s wrote' % (name, case.klass, who, bin(active))
        assert _bits_equal(got[rows_on], full[:64][rows_on]).all() or (np.isnan(got[rows_on]) == np.isnan(full[:64][rows_on])).all() and \
            (_bits_equal(got[rows_on], full[:64][rows_on]) | np.isnan(got[rows_on])).all(), '%s [%s] %s: rows %s answer differently alone' % (name, case.klass, who, bin(active))
