"""Shared by tests/test_contact_scan_emul.py and tests/test_gpu_contact_scan.py: the entry table of the step kernels' contact selections (the members of Pmc<L> in
lifelike_agility_and_play_amd/csrc/pmc_step.hpp that choose among contact candidates -- so far self_pick, one slot of the leg-leg pick), their inputs (fixed seeds; every
row of a wave gets different data, so a leak between rows shows), the runners of the host twin and the GPU copies of tests/lanes/contact_scan_body.hpp, and the comparison.
One sample per environment ROW of 16 lanes: [row][word][16 lanes], up to 64 one-wave workgroups (256 rows) a launch.

The entry is of the class MOVES of tests/math_helpers_common.py in what it must give: comparisons of float32 values, selects, minima, sums in which one lane contributes
and ONE float32 addition (the threshold), so GPU == host twin == statement, bit for bit, on every input class; no sample is left out.
Input classes (a row's 32 slots: 16 lanes x 2 pairs; 1e30 = no pair)
  random      depths of a few centimetres, about half of the slots 1e30; every other block of sixteen rows on a grid of 2^-18 m, so that several pairs sit within the
              tolerance; a tenth of the rows without any pair (have == false)
  ties        exact ties across lanes and the two pairs of a lane (depths from a set of four values)
  threshold   per slot r: r well separated closer pairs, then the closest of slot r and three more exactly AT float32(closest + eps), one float32 above it and one
              below it, all at random places (so the one at the threshold has the lower pair index in about half of the rows)
  few         fewer pairs than slots, and none at all
  signs       negative depths, +0 and -0, and the closest at float32(-1e-5), where the threshold is exactly 0 and both zeros sit on it
  permuted    one set of pairs in eight arrangements across the row: well separated depths, whose picks must not move, and depths within the tolerance, whose picks
              the rule names
Every class runs with one slot and with two (the second slot on what the first left).

The terrain-edge detectors reverse_edge and leg_edge (class APPROX: divisions and square roots enter) are held to the float64 statement contact_scan_ref.terrain_edge with
the pinned tables of the default model (legc, basec as the engines build them), the default contact margin and a list of 0 to 6 box records per row; check_edge says what
is held exactly and what within which bar.  Their classes:
  exact     quarter turns about z, positions and box coordinates in quarters
  random    1024 seeded poses about a quarter turn with boxes about the robot's footprint, a floating box and a yawed arena in one of seven, rows without a box; the CPU test holds the
            share left out of the decision comparison (at most 5 %) and the share within the contact margin (at least 30 %) on the statement alone
  edges     an edge parallel to a box axis (the 1e-9 guard); the two ends of the piece at equal depth; an edge wholly outside; n_shapes = 0; a floating box; a yawed arena; two boxes at equal depth; one row of the
            wave near a box and the others not (the wave-uniform skip), and a box nobody is near
leg_edge's exact and edge cases stand on sixteenths: the straight legs are 0.195 / 0.153 m from the base origin, and a box edge at 0.1875 runs across their boxes.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

import contact_scan_ref as ref
from contact_scan_ref import FAR, SELECT_EPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LANES_DIR = os.path.join(ROOT, 'tests', 'lanes')
HOST_LIB = os.path.join(LANES_DIR, '_build', 'libcontact_scan_host.so')
GPU_POLICIES = ['GpuLanes', 'GpuLanesPmc1Plain']             # the plain lanes and the pinned lanes of the one-wave-per-SIMD kernels (llenv.hip)
HOST_POLICIES = ['HostLanes']
VARIANTS = ['shipped', 'front_trim0']                        # the GPU copies (__graft_entry__.CONTACT_SCAN_VARIANTS): PMC_FRONT_TRIM 1 / 0, the two forms of rmin in lanes.hpp
ACTIVE_ROWS = [0b1111, 0b0011, 0b0100]                       # the whole wave, rows {0, 1}, row {2}: the entry runs under a partial EXEC as in the tail wave of an odd batch
MOVES, APPROX = 'MOVES', 'APPROX'
LC_COUNT, BC_COUNT = 151, 31                                 # csrc/pmc_params.hpp (the dims call checks the sum)
PICK_WORDS = 11                                              # one slot of self_pick: have | cmin | dsel | u6[6] | cd[0] | cd[1]

# id: ContactScanEntry of tests/lanes/contact_scan_body.hpp; targs: the arguments the driver takes (self_pick: slots - 1); policies / host: the GPU / host lane policies the
# entry runs under; variants: the builds whose switch reaches the entry (PMC_FRONT_TRIM: rmin of lanes.hpp); names: the members of Pmc<L> the entry covers (the coverage scan)
ENTRIES = {
    'self_pick': dict(id=0, cls=MOVES, words=2 * PICK_WORDS, targs=[0, 1], policies=[0, 1], host=[0], variants=VARIANTS, names=['self_pick']),
    'reverse_edge': dict(id=1, cls=APPROX, words=7, targs=[0], policies=[0, 1], host=[0], variants=['shipped'], names=['reverse_edge']),
    'leg_edge': dict(id=2, cls=APPROX, words=9, targs=[0], policies=[0, 1], host=[0], variants=['shipped'], names=['leg_edge', 'leg_fk']),
}
EDGE_ENTRIES = ('reverse_edge', 'leg_edge')
PICK_ENTRIES = ('self_pick',)
MAX_UNSURE, MIN_HIT = 0.05, 0.30                             # shares of the random class: left out of the decision comparison at most, within the margin at least
# The members of Pmc<L> this layer is asked to hold (the coverage scan of test_contact_scan_emul.py: each is defined in pmc_step.hpp, named by an entry, called by the driver) ...
PMC_MEMBERS = ['self_pick', 'reverse_edge', 'leg_edge']
CALLED_THROUGH = {'leg_fk'}                                  # (held alone by the math helpers; here it makes the LegKin leg_edge takes)
# ... and what stays for a later layer, each with the reason
LATER = {
    'keep_deepest': 'the deepest-K selection of the ground contacts (four rounds of quad minimum and claim, the rank and pick_rank reorder) is still text of substep_impl: '
                    'moved into a member it changed the code object of the step kernels and cost 0.34 % of the contract kernel (profiles/contact_scan_seam_ab.txt), '
                    'which the gate of this layer does not allow.  No member of that name exists yet',
    'seg_seg': 'the capsule-pair geometry of the leg-leg scan around it (end points, depth, pair index) is text of substep_impl; seg_seg_st itself is held by the math helpers',
    'substep_impl': 'the candidate depth loop, the deepest-K selection, the capsule-pair geometry of the leg-leg scan, the robot-robot scan with its two-best insertion: no '
                    'seam yet, held end to end by the step parity tests',
}


class Dims:
    def __init__(self, lib):
        d = (C.c_int * 16)()
        lib.ll_contact_scan_dims(d)
        self.n_in, self.n_out, self.max_blocks, self.n_consts, self.n_policies, self.front_trim, self.n_entries, self.pick_words = list(d)[:8]
        self.consts = np.zeros(self.n_consts, dtype=np.float32)
        self.consts[-1] = 1.0
        if hasattr(lib, 'll_contact_scan_tables'):          # (the host twin: the pinned tables of the default model, as the engines build them)
            from lifelike_agility_and_play_amd import urdf_model
            blob = np.ascontiguousarray(urdf_model.default_model_blob(), dtype=np.float64)
            lib.ll_contact_scan_tables.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_long]
            assert lib.ll_contact_scan_tables(blob.ctypes.data, len(blob), self.consts.ctypes.data, self.consts.size) == 0
        self.legc, self.basec = self.consts[:LC_COUNT * 4].reshape(LC_COUNT, 4), self.consts[-1 - BC_COUNT:-1]


class Case:
    def __init__(self, klass, X, targ=0, note=None):
        self.klass, self.targ, self.note = klass, targ, note
        self.X = np.ascontiguousarray(X, dtype=np.float32)                # [rows, words, 16]; rows a multiple of 4
        assert self.X.shape[0] % 4 == 0 and self.X.shape[2] == 16
        self.n = self.X.shape[0]


def _bind(path):
    lib = C.CDLL(path)
    lib.ll_contact_scan_dims.argtypes = [C.POINTER(C.c_int)]
    lib.ll_contact_scan_run.restype = C.c_int
    lib.ll_contact_scan_run.argtypes = [C.c_int] * 5 + [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_long]
    return lib


class HostRunner:
    def __init__(self):
        subprocess.check_call(['make', '-C', LANES_DIR, '-s'])
        self.lib = _bind(HOST_LIB)
        self.dims = Dims(self.lib)
        assert self.dims.pick_words == PICK_WORDS

    def launch(self, policy, eid, targ, n_blocks, active, w, out, consts):
        return self.lib.ll_contact_scan_run(policy, eid, targ, n_blocks, active, w.ctypes.data, w.size, out.ctypes.data, out.size, consts.ctypes.data, consts.size)

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
        self.dims.consts, self.dims.legc, self.dims.basec = host_dims.consts, host_dims.legc, host_dims.basec          # the tables the twin ran with
        assert (self.dims.n_in, self.dims.n_out, self.dims.n_consts, self.dims.max_blocks, self.dims.n_entries, self.dims.pick_words) == (
            host_dims.n_in, host_dims.n_out, host_dims.n_consts, host_dims.max_blocks, host_dims.n_entries, host_dims.pick_words)

    def launch(self, policy, eid, targ, n_blocks, active, w, out, consts):
        t = self.torch
        dw, dout, dc = (t.from_numpy(x).to('cuda:0') for x in (w, out, consts))
        t.cuda.synchronize()
        rc = self.lib.ll_contact_scan_run(policy, eid, targ, n_blocks, active, dw.data_ptr(), dw.numel(), dout.data_ptr(), dout.numel(), dc.data_ptr(), dc.numel())
        try:
            t.cuda.synchronize()
            out[:] = dout.cpu().numpy()
        except RuntimeError as e:          # a launch that faulted: nothing more is started on this device
            import pytest
            pytest.exit('the contact scan launch (policy %d, entry %d, targ %d) failed: %s' % (policy, eid, targ, e), returncode=3)
        return rc


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------------------
N_RANDOM, N_EDGE = 1024, 64
CLASSES = ['random', 'ties', 'threshold', 'few', 'signs', 'permuted']


def _rng(name, klass, targ): return np.random.default_rng([ENTRIES[name]['id'], CLASSES.index(klass), targ])


def _up(x): return np.nextafter(np.asarray(x, dtype=np.float32), np.float32(np.inf))
def _down(x): return np.nextafter(np.asarray(x, dtype=np.float32), np.float32(-np.inf))
def _thr(x): return (np.asarray(x, dtype=np.float32) + SELECT_EPS).astype(np.float32)


def _depths(r, shape):
    """a few centimetres either side of the ground, nothing near the denormals"""
    x = r.uniform(-0.03, 0.02, size=shape).astype(np.float32)
    return np.where(np.abs(x) < 2.0 ** -20, np.float32(0.004), x)


def slot_sets(r, klass, G, n, rounds, note):
    """G groups of n candidate slots (a row's 32) -> [G, n] float32 depths, 1e30 where there is no candidate"""
    D = np.full((G, n), FAR, dtype=np.float32)
    g = np.arange(G)
    place = lambda vals: np.put_along_axis(D, np.argsort(r.random((G, n)), axis=1)[:, :vals.shape[1]], vals.astype(np.float32), axis=1)
    if klass == 'random':
        D = _depths(r, (G, n))
        D[(g // 16) % 2 == 1] = (np.round(D[(g // 16) % 2 == 1] * 2.0 ** 18) * 2.0 ** -18).astype(np.float32)
        D[r.random((G, n)) < 0.5] = FAR
    elif klass == 'ties':
        vals = np.array([-0.0125, 0.0, 0.00390625, 0.0078125], dtype=np.float32)
        D = vals[r.integers(0, 4, size=(G, n))]
        D[r.random((G, n)) < 0.4] = FAR
    elif klass == 'threshold':
        k = note                            # the round the threshold is probed in
        b = np.sort(_depths(r, (G, 1)) + np.float32(1e-3) * np.arange(k + 1, dtype=np.float32)[None, :], axis=1).astype(np.float32)
        t = _thr(b[:, k])
        place(np.concatenate([b, np.stack([t, _up(t), _down(t)], axis=1)], axis=1))
    elif klass == 'few':
        cnt = g % rounds if note == 'fewer' else np.zeros(G, dtype=int)
        vals = _depths(r, (G, rounds))
        place(np.where(np.arange(rounds)[None, :] < cnt[:, None], vals, FAR))
    elif klass == 'signs':
        pool = np.array([-1e-5, 0.0, -0.0, 0.0, -0.0, -0.02, -1e-3, 1e-5, 2e-5], dtype=np.float32)
        D = pool[r.integers(0, len(pool), size=(G, n))]
        D[g % 2 == 0] = np.where(D[g % 2 == 0] < np.float32(-1e-5), np.float32(0.0), D[g % 2 == 0])      # every other group: the deepest is float32(-1e-5), the threshold exactly 0
        D[r.random((G, n)) < 0.4] = FAR
    else:
        raise KeyError(klass)
    return D


NOTES = {'random': [None], 'ties': [None], 'threshold': [0, 1], 'few': ['fewer', 'none'], 'signs': [None], 'permuted': ['separated', 'within the tolerance']}


def cases(name, dims=None, targs=None):
    """[Case] of an entry (fixed seed per (entry, class, targ))"""
    out = []
    for targ in (ENTRIES[name]['targs'] if targs is None else targs):
        for klass in CLASSES:
            r = _rng(name, klass, targ)
            R = N_RANDOM if klass == 'random' else N_EDGE
            for note in NOTES[klass]:
                tag = None if note is None else ('round %d' % note if klass == 'threshold' else note)
                if klass == 'permuted':
                    cnt = 5
                    v = (_depths(r, (R // 8, 1)) + np.float32(1e-3 if note == 'separated' else 3e-6) * np.arange(cnt, dtype=np.float32)).astype(np.float32)
                    flat = np.full((R // 8, 32), FAR, dtype=np.float32)
                    flat[:, :cnt] = v
                    cd = np.stack([np.repeat(flat, 8, axis=0)[i][r.permutation(32)] for i in range(R)]).reshape(R, 2, 16)
                else:
                    cd = slot_sets(r, klass, R, 32, targ + 1, note).reshape(R, 2, 16)
                    if klass == 'random':
                        cd[r.random(R) < 0.1] = FAR                          # have == false among them
                X = np.zeros((R, 16, 16), dtype=np.float32)
                X[:, 0:2], X[:, 2:4] = cd, ref.pair_codes()[None]
                pn = (r.integers(-64, 65, size=(R, 12, 16)) * 2.0 ** -6).astype(np.float32)   # every lane's point and normal different, some of them -0
                X[:, 4:16] = np.where((pn == 0) & (r.random(pn.shape) < 0.5), np.float32(-0.0), pn)
                out.append(Case(klass, X, targ, tag))
    return out


# ---- statements ------------------------------------------------------------------------------------------------------------------------------------------
_WANT = {}


def statement(name, case, **wrong):
    """-> [rows, words, 16] float64 holding float32 values; NaN: a word the statement does not name (held to the twin's bits only)"""
    X, R = case.X, case.n
    v = np.full((R, ENTRIES[name]['words'], 16), np.nan)
    if name == 'self_pick':
        slots = case.targ + 1
        cP, cN = X[:, 4:10].reshape(R, 2, 3, 16), X[:, 10:16].reshape(R, 2, 3, 16)
        uni, after = ref.self_pick(X[:, 0:2], X[:, 2:4], cP, cN, slots, **wrong)
        for s in range(slots):
            v[:, s * PICK_WORDS:s * PICK_WORDS + 9] = uni[:, s, :, None]
            v[:, s * PICK_WORDS + 9:s * PICK_WORDS + 11] = after[:, s]
    else:
        raise KeyError(name)
    return v


def want(name, case):
    key = (name, id(case))
    if key not in _WANT:
        _WANT[key] = statement(name, case)
    return _WANT[key]


# ---- comparison ----------------------------------------------------------------------------------------------------------------------------------------
def _bits(x): return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def bits_equal(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


def rows_on(n, active): return ((active >> (np.arange(n) % 4)) & 1).astype(bool)


def words_of(name, case): return (case.targ + 1) * PICK_WORDS


def head(name, case, who): return '%s [%s%s, targ %d] %s' % (name, case.klass, '' if case.note is None else ': ' + case.note, case.targ, who)


def check(name, case, got, who, active=0b1111):
    """Holds the answer `got` [rows, n_out, 16] of `who` to the statement, bit for bit; no sample is left out.  -> the number of words compared"""
    v = want(name, case)[:len(got)]
    words = words_of(name, case)
    on = rows_on(len(got), active)
    hd = head(name, case, who)
    assert np.isnan(got[~on]).all(), hd + ': a row outside EXEC wrote'
    assert np.isnan(got[:, words:]).all(), hd + ': a word past the entry\'s outputs was written'
    g = got[:, :words]
    assert not np.isnan(g[on]).any(), hd + ': a word left unwritten (or a NaN) at (row, word, lane) %s' % (np.argwhere(np.isnan(g) & on[:, None, None])[:1].tolist(),)
    stated = ~np.isnan(v[:, :words]) & on[:, None, None]
    v32 = np.nan_to_num(v[:, :words]).astype(np.float32)
    same = bits_equal(g, v32) | ~stated
    bad = np.argwhere(~same)
    assert not len(bad), hd + ': word %d differs from the statement in bits at (row, lane) (%d, %d): %r, stated %r (%d such)' % (
        bad[0][1], bad[0][0], bad[0][2], g[tuple(bad[0])], np.float32(v[tuple(bad[0])]), len(bad))
    return int(stated.sum())


def partial_exec_check(runner, policy, name, case, full, who):
    """rows {0, 1} and row {2} alone of ONE wave: the active rows answer what they answered in the whole wave, the others write nothing (NaN canaries, bit for bit)"""
    for active in ACTIVE_ROWS[1:]:
        got = runner.run(policy, name, case, active, limit=4)
        on = rows_on(4, active)
        assert np.isnan(got[~on]).all(), '%s: a row outside EXEC %s wrote' % (head(name, case, who), bin(active))
        assert bits_equal(got[on], full[:4][on]).all(), '%s: rows %s answer differently alone' % (head(name, case, who), bin(active))


def kept_set_does_not_move(name, case, got, who):
    """the 'separated' arrangements of one set of pairs: dsel of each slot is the same in all eight rows of a group"""
    assert case.klass == 'permuted' and case.note == 'separated'
    kept = np.stack([got[:, s * PICK_WORDS + 2, 0] for s in range(case.targ + 1)], axis=1).reshape(case.n // 8, 8, -1)
    assert bits_equal(kept, kept[:, :1]).all(), '%s: the kept set moved with the arrangement of the candidates' % head(name, case, who)


# ---- the terrain-edge entries: inputs -----------------------------------------------------------------------------------------------------------------------
# words: base position (3) | R (9) | n_shapes | yawed ycx ycy ycs ysn | q1 q2 q3 (per leg) | endf / edgef = the sub-lane, as the kernel passes it | - - | 6 records of 8 words
EDGE_WORDS = 72
TRUNK_BOTTOM = 0.0645          # the flat under the trunk below the base origin: half extent 0.055 less the box centre's -0.0095 (basec)
LEG_XY = (0.195, 0.153)        # where the straight legs stand in the base frame


def rot_zyx(yaw, pitch=0.0, roll=0.0):
    """[n, 9] row-major Rz(yaw) Ry(pitch) Rx(roll), rounded to float32 (quarter turns give exact 0 and +-1)"""
    yaw, pitch, roll = np.broadcast_arrays(np.asarray(yaw, dtype=np.float64), pitch, roll)
    cz, sz, cy, sy, cx, sx = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    m = np.stack([cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx, sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx, -sy, cy * sx, cy * cx], axis=-1)
    return np.where(np.abs(m) < 1e-12, 0.0, np.where(np.abs(np.abs(m) - 1) < 1e-12, np.sign(m), m)).astype(np.float32)


def edge_words(p, Rm, boxes, n, q=None, yaw=None):
    R = len(p)
    X = np.zeros((R, EDGE_WORDS, 16), dtype=np.float32)
    X[:, 0:3], X[:, 3:12], X[:, 12] = np.asarray(p)[:, :, None], np.asarray(Rm)[:, :, None], np.asarray(n, dtype=np.float32)[:, None]
    X[:, 13:18] = np.array([0, 0, 0, 1, 0], dtype=np.float32)[None, :, None] if yaw is None else np.asarray(yaw)[:, :, None]
    if q is not None:
        X[:, 18:21] = np.repeat(np.asarray(q).transpose(0, 2, 1), 4, axis=2)          # q [R, 4 legs, 3]
    X[:, 21] = (np.arange(16) % 4)[None, :]
    X[:, 24:72] = np.asarray(boxes, dtype=np.float32).reshape(R, 48)[:, :, None]
    return X


def box(x0, x1, y0, y1, z0, z1): return np.stack(np.broadcast_arrays(x0, x1, y0, y1, z0, z1, 0.0, 0.0), axis=-1)


FAR_BOX = [40.0, 41.0, 40.0, 41.0, 0.0, 0.25]


def random_edges(name, r, R):
    """seeded poses within reach of the boxes: the robot near a quarter turn (so that edges run along the trunk and across the legs), boxes about its footprint"""
    quarter = r.integers(0, 4, size=R)
    arena = np.where(r.random(R) < 0.15, r.uniform(-np.pi, np.pi, size=R), 0.0)          # a yawed arena in one row of seven: the records stand in a frame turned about the robot's place
    yaw = quarter * (np.pi / 2) + r.uniform(-0.12, 0.12, size=R) + arena
    p = np.stack([r.uniform(-0.2, 0.2, R), r.uniform(-0.2, 0.2, R), r.uniform(0.30, 0.40, R)], axis=1).astype(np.float32)
    Rm = rot_zyx(yaw, r.uniform(-0.05, 0.05, R), r.uniform(-0.05, 0.05, R))
    q = np.stack([r.uniform(-0.1, 0.1, (R, 4)), r.uniform(-0.25, 0.25, (R, 4)), r.uniform(-0.3, 0.3, (R, 4))], axis=2).astype(np.float32)
    boxes = np.tile(np.array(FAR_BOX + [0, 0], dtype=np.float64), (R, 6, 1))
    n = r.integers(1, 7, size=R)
    n[r.random(R) < 0.06] = 0
    turned = (quarter % 2 == 1)[:, None]
    for si in range(6):
        c = p[:, :2].astype(np.float64) + r.uniform(-0.02, 0.02, (R, 2))
        if name == 'reverse_edge':
            half = np.stack([r.uniform(0.02, 0.13, R), r.uniform(0.02, 0.09, R)], axis=1)
            z1 = p[:, 2] - TRUNK_BOTTOM + r.uniform(-0.03, 0.025, R)
        else:
            half = np.stack([LEG_XY[0] + r.uniform(-0.025, 0.025, R), LEG_XY[1] + r.uniform(-0.02, 0.02, R)], axis=1)
            z1 = p[:, 2] - r.uniform(0.06, 0.36, R)
        half = np.where(turned, half[:, ::-1], half)
        floating = r.random(R) < 0.15          # a hanging bar: its bottom edges count
        z0 = np.where(floating, z1, 0.0)
        z1 = np.where(floating, z1 + 0.05, z1)
        b = box(c[:, 0] - half[:, 0], c[:, 0] + half[:, 0], c[:, 1] - half[:, 1], c[:, 1] + half[:, 1], z0, z1)
        stray = r.random(R) < 0.2              # some boxes elsewhere: out of reach, or only near
        b[stray, :4] += r.choice([-1.0, 1.0], size=(int(stray.sum()), 1)) * r.uniform(0.2, 3.0, size=(int(stray.sum()), 1))
        boxes[:, si] = b
    yawed = np.stack([arena != 0, p[:, 0], p[:, 1], np.cos(arena), np.sin(arena)], axis=1).astype(np.float32)
    boxes[arena != 0, :, 0:2] -= p[arena != 0, None, 0:1]          # (a yawed record is given about the arena's centre: world = centre + turn . record)
    boxes[arena != 0, :, 2:4] -= p[arena != 0, None, 1:2]
    return edge_words(p, Rm, boxes, n, q, yawed)


def leg_box(p, turned, z1, near=0.1875, z0=0.0):
    """a box about the base origin whose x edges (its y edges when turned) run `near` from it, across the boxes of the straight legs; the other pair half a metre away"""
    hx, hy = np.where(turned, 0.5, near), np.where(turned, near, 0.5)
    return box(p[:, 0] - hx, p[:, 0] + hx, p[:, 1] - hy, p[:, 1] + hy, z0, z1)


def exact_edges(name, r, R):
    """quarter turns about z, positions and box coordinates in quarters: every decision is one between float32 facts"""
    p = np.stack([r.integers(-1, 2, R) * 1.0 + (np.arange(R) % 4) * 0.25, r.integers(-2, 3, R) * 0.25, r.choice([0.25, 0.5], R)], axis=1).astype(np.float32)
    Rm = rot_zyx(r.integers(0, 4, R) * (np.pi / 2))
    boxes = np.tile(np.array(FAR_BOX + [0, 0], dtype=np.float64), (R, 6, 1))
    if name == 'leg_edge':                  # sixteenths: the straight legs stand 0.195 / 0.153 m from the base origin, edges at 0.1875 run across their boxes
        p[:, 2] = 0.25
        for si in range(6):
            boxes[:, si] = leg_box(p, r.integers(0, 2, R) == 1, r.choice([0.125, 0.0625], R), r.choice([0.1875, 0.25], R))
        return edge_words(p, Rm, boxes, r.integers(1, 7, R), np.zeros((R, 4, 3), dtype=np.float32))
    for si in range(6):
        x0, y0 = p[:, 0] + r.choice([-0.25, 0.0], R), p[:, 1] + r.choice([-0.25, 0.0], R)
        x1, y1 = x0 + r.choice([0.25, 0.5], R), y0 + r.choice([0.25, 0.5], R)
        boxes[:, si] = box(x0, x1, y0, y1, 0.0, r.choice([0.25, 0.5], R))
    return edge_words(p, Rm, boxes, r.integers(1, 7, R), np.zeros((R, 4, 3), dtype=np.float32))


def edge_edges(name, r, note, R=N_EDGE):
    """the edge cases, every one on quarter turns and quarter coordinates.  -> X"""
    p = np.stack([(np.arange(R) % 4) * 0.25 - 0.25, r.integers(-1, 2, R) * 0.25, np.full(R, 0.25)], axis=1).astype(np.float32)          # every row of a wave another place
    quarter = r.integers(0, 4, R)
    Rm = rot_zyx(quarter * (np.pi / 2))
    q = np.zeros((R, 4, 3), dtype=np.float32)
    boxes = np.tile(np.array(FAR_BOX + [0, 0], dtype=np.float64), (R, 6, 1))
    n, yaw = np.full(R, 2), None
    under = lambda dz=0.0: box(p[:, 0], p[:, 0] + 0.25, p[:, 1], p[:, 1] + 0.25, 0.0, 0.25 + dz)          # a corner of it under the base origin
    if name == 'leg_edge':                  # the same cases on boxes whose edges run across the leg boxes (sixteenths; leg_box)
        turned = quarter % 2 == 1           # the near pair of edges along the robot's own y, where its legs stand
        z1 = r.choice([0.125, 0.0625], R)
        under = lambda dz=0.0: leg_box(p, turned, z1)
    if note == 'parallel to a box axis':          # quarter turns: every edge is parallel to one axis of the trunk box, d = 0 on the two others (the 1e-9 guard)
        boxes[:, 0] = under()
    elif note == 'the two ends at equal depth':  # quarter turns: the edge runs parallel to the face it lies on, both ends of the piece are equally deep, the first is taken
        boxes[:, 0] = under()
    elif note == 'wholly outside':
        n[:] = 3                                   # listed, near or far, none within the margin: depth 1e30, Pb from the zero point, nw = +z
        boxes[:, 0] = box(p[:, 0] + 0.5, p[:, 0] + 0.75, p[:, 1] + 0.5, p[:, 1] + 0.75, 0.0, 0.25)
    elif note == 'n_shapes = 0':
        n[:] = 0
        boxes[:, 0] = under()
    elif note == 'a floating box':                 # z0 above LLM_FLOATING_MIN_Z: the BOTTOM edges, which reach the trunk from below; its top edges are far above
        boxes[:, 0] = box(p[:, 0], p[:, 0] + 0.25, p[:, 1], p[:, 1] + 0.25, 0.25, 1.0) if name == 'reverse_edge' else leg_box(p, turned, 1.0, z0=z1)
    elif note == 'a yawed arena':                  # the record given in a frame a quarter turn about (ycx, ycy) away
        k = r.integers(1, 4, R)
        boxes[:, 0] = under() if name == 'reverse_edge' else leg_box(p, turned ^ (k % 2 == 1), z1)
        yaw = np.stack([np.ones(R), p[:, 0], p[:, 1], np.round(np.cos(k * np.pi / 2)), np.round(np.sin(k * np.pi / 2))], axis=1).astype(np.float32)
        boxes[:, 0, 0:2] -= p[:, 0:1]              # (given about the arena's centre: world = centre + turn . record)
        boxes[:, 0, 2:4] -= p[:, 1:2]
    elif note == 'two boxes at equal depth':       # the same top, side by side along the edge: the first listed wins
        boxes[:, 0], boxes[:, 1] = under(), under()
        if name == 'reverse_edge':
            boxes[:, 1, 0:4] = boxes[:, 0, 0:4] + np.array([0.0, 0.0, -0.25, -0.25])[None]          # (leg_edge: the same box twice -- shape says which was taken)
    elif note == 'a box only near':                # the wave-uniform skip: row 0 of every wave has a box within the margin, the others have it only near or far away
        boxes[:, 0] = under()
        off = np.where(np.arange(R) % 4 == 0, 0.0, np.where(np.arange(R) % 4 == 1, 0.25, 8.0))
        if name == 'leg_edge':              # a sixteenth wider on every side: near every leg box, within the margin of none
            boxes[:, 0, 0:4] += np.where(np.arange(R) % 4 == 1, 0.0625, 0.0)[:, None] * np.array([-1.0, 1.0, -1.0, 1.0])[None]
            off = np.where(np.arange(R) % 4 < 2, 0.0, 8.0)
        boxes[:, 0, 0:2] += off[:, None]
    elif note == 'a box nobody is near':
        boxes[:, 0] = under()
        boxes[:, 0, 0:4] += 16.0
    else:
        raise KeyError(note)
    return edge_words(p, Rm, boxes, n, q, yaw)


EDGE_NOTES = ['parallel to a box axis', 'the two ends at equal depth', 'wholly outside', 'n_shapes = 0', 'a floating box', 'a yawed arena', 'two boxes at equal depth', 'a box only near', 'a box nobody is near']


def edge_cases(name):
    out = []
    eid = ENTRIES[name]['id']
    out.append(Case('exact', exact_edges(name, np.random.default_rng([eid, 0]), N_EDGE), 0))
    out.append(Case('random', random_edges(name, np.random.default_rng([eid, 1]), N_RANDOM), 0))
    for k, note in enumerate(EDGE_NOTES):
        out.append(Case('edges', edge_edges(name, np.random.default_rng([eid, 2, k]), note), 0, note))
    return out


_EDGE_WANT = {}


def edge_want(name, case, dims, **wrong):
    key = (name, id(case))
    if wrong:
        return ref.terrain_edge(name, case.X, dims.legc, dims.basec, **wrong)
    if key not in _EDGE_WANT:
        _EDGE_WANT[key] = ref.terrain_edge(name, case.X, dims.legc, dims.basec)
    return _EDGE_WANT[key]


def check_edge(name, case, got, who, dims, bar='twin', dev_host=None, active=0b1111):
    """Holds `got` to the float64 statement.
    random: a sample is sure when the margin of every decision of the statement (the 1e-9 guard, cut empty or not, the parallel axis, the face and its side, the piece
            empty or not, which end, which box and link, within the contact margin or not) exceeds its forward bound.  On sure samples: within the margin or not, exactly;
            on those within it link and shape exactly and depth, Pb, nw within the bar -- the twin's own bound, for the GPU max(4 dev_host, that bound).  A candidate at or
            beyond the margin is none to the caller (substep_impl keeps depth < margin_dist only); for leg_edge it is held to being at or beyond it: leg_edge's `near`
            drops the pieces that only clip a corner of the margin-grown box, all of them beyond the margin, which the rule keeps.  reverse_edge has no `near` in its valid
            and is held in full on every candidate the rule finds.  Samples that are not sure are counted and left out.
    exact and edges: no sample is left out; found or not, link, shape and nw bit for bit (quarter turns and quarter coordinates make them float32 facts).  Depth and Pb are
            held to the same bar as in the random class and not to their bits: the centre of the trunk box in the pinned table (0.00458458, -0.00306684, -0.00947989) is no
            quarter, so pa = edge - centre rounds in float32, and with it the depth and the place where the piece is cut; the twin's depth sits one float32 off the
            statement's (-0.045520104 against -0.045520112), its Pb likewise (-0.13691545 against -0.13691542).  Not every word is a float32 on these inputs.
    -> dict(err [words], ratio, unsure)"""
    v, e, sure, hit = edge_want(name, case, dims)
    words = ENTRIES[name]['words']
    v, e, sure, hit = v[:len(got), :words], e[:len(got), :words], sure[:len(got)], hit[:len(got)]
    on = rows_on(len(got), active)
    hd = head(name, case, who)
    assert np.isnan(got[~on]).all(), hd + ': a row outside EXEC wrote'
    assert np.isnan(got[:, words:]).all(), hd + ': a word past the entry\'s outputs was written'
    g = got[:, :words].astype(np.float64)
    assert np.isfinite(g[on]).all(), hd + ': a word left unwritten or not finite'
    b = e if bar == 'twin' else np.maximum(4.0 * dev_host[None, :, None], e)
    if case.klass != 'random':
        use = np.broadcast_to(on[:, None, None], g.shape)
        same = bits_equal(got[:, :words], v.astype(np.float32)) | ((v == 0) & (g == 0)) | ~use
        for word in range(4):          # depth and Pb of a candidate: within the bar
            same[:, word] |= (v[:, 0] < 1.0) & (np.abs(g[:, word] - v[:, word]) <= b[:, word])
        bad = np.argwhere(~same)
        assert not len(bad), hd + ': exact inputs, but word %d is not the statement\'s at (row, lane) (%d, %d): %r, stated %r (%d such)' % (
            (bad[0][1], bad[0][0], bad[0][2], got[tuple(bad[0])], np.float32(v[tuple(bad[0])]), len(bad)) if len(bad) else (0, 0, 0, 0, 0, 0))
        err = np.where(use & (v[:, 0:1] < 1.0), np.abs(g - v), 0.0)
        with np.errstate(invalid='ignore', divide='ignore'):
            ratio = np.where(err > 0, err / b, 0.0)
        return dict(err=err.max(axis=(0, 2)), ratio=float(ratio.max()), unsure=0.0, bar=float(b[np.unravel_index(int(np.argmax(ratio)), ratio.shape)]))
    ok = sure & on[:, None]
    within = g[:, 0] < np.float64(np.float32(ref.MARGIN))
    same = (within == hit) | ~ok
    assert same.all(), hd + ': within the contact margin / not, against the statement on a sure sample at (row, lane) %s' % (np.argwhere(~same)[:1].tolist(),)
    held = hit
    if name == 'reverse_edge':              # no `near` in its valid: every candidate the rule finds is held in full, beyond the margin too
        held = v[:, 0] < 1.0
        same = ((g[:, 0] < 1.0) == held) | ~ok
        assert same.all(), hd + ': a candidate found / not found against the statement on a sure sample at (row, lane) %s' % (np.argwhere(~same)[:1].tolist(),)
    use = np.broadcast_to((ok & held)[:, None, :], g.shape)
    for word in range(7, words):
        same = (g[:, word] == v[:, word]) | ~use[:, word]
        assert same.all(), hd + ': word %d (link / shape) differs from the statement on a sure sample at (row, lane) %s' % (word, np.argwhere(~same)[:1].tolist())
    err = np.where(use, np.abs(g - v), 0.0)
    bad = np.argwhere(err > b)
    assert not len(bad), hd + ': |answer - statement| = %.3e above the bar %.3e at (row, word, lane) %s (%d such)' % (
        (err[tuple(bad[0])], b[tuple(bad[0])], bad[0].tolist(), len(bad)) if len(bad) else (0, 0, [], 0))
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where(err > 0, err / b, 0.0)
    return dict(err=err.max(axis=(0, 2)), ratio=float(ratio.max()), unsure=float(1 - sure.mean()), bar=float(b[np.unravel_index(int(np.argmax(ratio)), ratio.shape)]))
