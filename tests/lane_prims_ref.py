"""What each primitive of the lane policy (lifelike_agility_and_play_amd/csrc/lanes.hpp) is MEANT to compute, in NumPy float64, written from the comments of
lanes.hpp -- not from tests/emul/lanes_host.hpp.  One function per primitive, vectorised over the rows of a wave; GpuLanes and HostLanes both answer to it
(tests/test_lane_prims_emul.py, tests/test_gpu_lane_prims.py).

A function takes a Case (tests/lane_prims_common.py: operand words w[row, word, lane], aux[row, :], auxd[:], ia[:], targ) and returns
    out    {word: [rows, 16] float64}     every word the driver (tests/lanes/lane_prims_body.hpp) stores, in its order
    aux    [rows, AUX_WORDS] float64      the global-memory words after the call (NaN canaries where nothing may be written)
    bound  {word: [rows, 16]} or None     the forward bound n * u * sum |t_i| of that output (u = 2^-24, t_i the terms that enter it, n the roundings on its longest path)
    trace  [arrays]                       every intermediate: on the `exact` inputs each must be a float32 (the premise that association and fusing cannot matter)
A row is one environment: lane = 4 * leg + sub."""
import numpy as np

U = 2.0 ** -24
LANE = np.arange(16)
LEG = LANE // 4
SUB = LANE % 4
QUAD0 = LANE & ~3


class Res:
    def __init__(self, case):
        self.out, self.bound, self.trace = {}, None, []
        self.aux = case.aux.astype(np.float64).copy()

    def t(self, x):
        self.trace.append(np.asarray(x, dtype=np.float64))
        return x

    def put(self, word, x, bound=None):
        x = np.array(x, dtype=np.float64)
        assert x.ndim == 2 and x.shape[1] == 16, x.shape
        self.out[word] = self.t(x)
        if bound is not None:
            self.bound = self.bound or {}
            self.bound[word] = np.broadcast_to(bound, x.shape).copy()


def _uni(x):        # an env-uniform value, as every lane of the row sees it
    return np.repeat(np.asarray(x, dtype=np.float64)[:, None], 16, axis=1)


# ---- moves -----------------------------------------------------------------------------------------------------------------------------------
def from_prev_leg(c, r): r.put(0, c.w[:, 0][:, (LANE - 4) % 16])          # the same sub-lane of leg (leg + 3) % 4
def from_leg2(c, r): r.put(0, c.w[:, 0][:, (LANE + 8) % 16])
def from_next_leg(c, r): r.put(0, c.w[:, 0][:, (LANE + 4) % 16])          # ... of leg (leg + 1) % 4
def rbcast(c, r): r.put(0, _uni(c.w[:, 0, c.targ]))                       # lane L of the row
def subbcast(c, r): r.put(0, c.w[:, 0][:, QUAD0 | c.targ])                # sub-lane K of the own leg
def bcast(c, r): r.put(0, _uni(c.w[:, 0, 4 * c.targ]))                    # leg l, from its sub-lane 0
def settle(c, r): from_prev_leg(c, r)


def subbcast6(c, r):
    for i in range(6):
        r.put(i, c.w[:, i][:, QUAD0 | c.targ])


def subbcast6_after(c, r):
    for i in range(6):
        r.put(i, c.w[:, i][:, QUAD0 | c.targ])
        r.put(6 + i, c.w[:, i][:, QUAD0])


def gather_tri3(c, r):       # column k of a 3 x 3 matrix in sub-lane k as d[0..2]: m11 m12 m22 m13 m23 m33 to every sub-lane
    for m, (row, col) in enumerate([(0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2)]):
        r.put(m, c.w[:, row][:, QUAD0 | col])


def spread3(c, r):
    for k in range(3):
        r.put(k, c.w[:, 0][:, QUAD0 | k])


def rmin(c, r): r.put(0, _uni(c.w[:, 0].min(axis=1)))
def submin(c, r): r.put(0, np.repeat(c.w[:, 0].reshape(-1, 4, 4).min(axis=2), 4, axis=1))


def vel_dx(c, r):            # VA: lane (leg, s) holds dx[s];  VB: dx[4 + (s & 1)]
    i = c.targ
    r.put(0, _uni(c.w[:, 0, i] if i < 4 else c.w[:, 1, i & 1]))


def vel_dq(c, r): r.put(0, c.w[:, 0][:, QUAD0 | c.targ])                   # VJ: dq_leg[s]
def peer(c, r): r.put(0, c.w[[1, 0, 3, 2], 0])                             # the same lane of row ^ 1


def row_ballot(c, r):        # bit j = lane j of the row
    r.put(0, _uni(((c.w[:, 0] > 0) * (1 << LANE)).sum(axis=1)))


def row_ballot_host(c, r):   # the host's per-env code is a row of ONE lane (lanes_host.hpp): lane 0 speaks
    r.put(0, _uni((c.w[:, 0, 0] > 0) * 1.0))


def ld16(c, r):
    i0, n = c.ia[0], c.ia[1]
    i = i0 + LANE
    r.put(0, np.where(i < n, c.aux[:, np.minimum(i, n - 1)], 0.0))


def st16(c, r):
    i0, n = c.ia[0], c.ia[1]
    for l in range(16):
        if i0 + l < n:
            r.aux[:, i0 + l] = c.w[:, 0, l]


def st16_rot(c, r):          # element i goes to i + (n - split) if i < split, else to i - split
    i0, n, split = c.ia[0], c.ia[1], c.ia[2]
    for l in range(16):
        i = i0 + l
        if i < n:
            r.aux[:, i + (n - split) if i < split else i - split] = c.w[:, 0, l]


def copy16(c, r):
    i0, n = c.ia[0], c.ia[1]
    h = c.aux.shape[1] // 2
    for l in range(16):
        if i0 + l < n:
            r.aux[:, h + i0 + l] = c.aux[:, i0 + l]


def count_le16(c, r):
    n, u = c.ia[0], c.auxd[-1]
    r.put(0, np.full((c.w.shape[0], 16), float((c.auxd[:n] <= u).sum())))


def park_row(c, r):
    for i in range(4):
        r.put(i, _uni(c.w[:, i, 0]))


def cone_lds(c, r):
    for k in range(2):
        for t in range(4):
            r.put(k * 4 + t, c.w[:, (k * 4 + c.targ) * 4 + t])


def stage_row(c, r):
    n = c.ia[0]
    for ch in range((n + 15) // 16):
        i = ch * 16 + LANE
        r.put(ch, np.where(i < n, c.aux[:, np.minimum(i, n - 1)], 0.0))


def legc(c, r): r.put(0, np.repeat(c.legc[c.ia[0]][None, LEG], c.w.shape[0], axis=0))          # legc [field][leg]
def candc(c, r): r.put(0, np.repeat(c.candc[c.ia[0]][None, :], c.w.shape[0], axis=0))          # candc [word][lane]: the own column
def basec(c, r): r.put(0, np.full((c.w.shape[0], 16), c.basec[c.ia[0]]))
def candc_of(c, r): r.put(0, np.repeat(c.candc[c.ia[1]][None, QUAD0 + c.ia[0]], c.w.shape[0], axis=0))   # the column of sub-lane sub2 of the own leg


def lane_ids(c, r):
    R = c.w.shape[0]
    for word, v in enumerate([LEG, SUB, LEG, LEG == (c.targ & 3), SUB == (c.targ & 3), LANE == c.targ]):
        r.put(word, np.repeat(np.asarray(v, dtype=np.float64)[None], R, axis=0))


def pick(c, r):
    R = c.w.shape[0]
    r.put(0, np.repeat(np.array([1.0, 2.0, 3.0, 3.0])[None, LEG], R, axis=0))      # leg 0 -> x, 1 -> y, 2, 3 -> z
    r.put(1, np.repeat(np.array([4.0, 5.0, 6.0, 7.0])[None, LEG], R, axis=0))
    r.put(2, np.repeat(np.array([8.0, 9.0, 10.0, 11.0])[None, LEG], R, axis=0))
    r.put(3, np.trunc(c.w[:, 0]) + 0.0)                                          # through an int: no negative zero


def ldl_stl(c, r):           # element base + stride * leg; stores from sub-lane 0 only
    base, stride = c.ia[0], c.ia[1]
    h = c.aux.shape[1] // 2
    r.put(0, c.aux[:, base + stride * LEG])
    for leg in range(4):
        r.aux[:, h + base + stride * leg] = c.w[:, 0, 4 * leg]


def ldl2(c, r):              # stl under a lane predicate (still sub-lane 0 only), ldl for doubles, a double load by a per-lane index
    base, stride, dbase, dstride = (int(v) for v in c.ia)
    m = (LEG == (c.targ & 3)) if c.targ < 4 else (SUB == (c.targ & 3))
    for leg in range(4):
        if m[4 * leg]:
            r.aux[:, base + stride * leg] = c.w[:, 0, 4 * leg]
    r.put(0, np.repeat(c.auxd[None, dbase + dstride * LEG], c.w.shape[0], axis=0))
    r.put(1, c.auxd[c.w[:, 1].astype(np.int64)])


# ---- sums ------------------------------------------------------------------------------------------------------------------------------------
def _sum_terms(r, terms, n):           # the sum of `terms` ([k, rows, 16]) and its forward bound with n roundings
    s = terms[0].copy()
    for t in terms[1:]:
        s = r.t(s + t)
    return s, n * U * np.abs(terms).sum(axis=0)


def _quad_sum(x):
    return np.repeat(x.reshape(x.shape[0], 4, 4).sum(axis=2), 4, axis=1)


def qsum(c, r, word=0, out=0):         # over the four LEGS of a leg-uniform value
    x = c.w[:, word]
    s, b = _sum_terms(r, np.stack([x[:, (LANE + 4 * k) % 16] for k in range(4)]), 2)
    r.put(out, s, b)


def subsum(c, r, word=0, out=0):       # over the four SUB-lanes of a leg
    x = c.w[:, word]
    s, b = _sum_terms(r, np.stack([x[:, QUAD0 | ((SUB + k) & 3)] for k in range(4)]), 2)
    r.put(out, s, b)


def rsum6(c, r):                       # six row sums (all 16 lanes)
    for i in range(6):
        x = c.w[:, i]
        s, b = _sum_terms(r, np.stack([x[:, (LANE + k) % 16] for k in range(16)]), 4)
        r.put(i, s, b)


def qsum6(c, r):
    for i in range(6):
        qsum(c, r, i, i)


def subsum3(c, r):
    for i in range(3):
        subsum(c, r, i, i)


def _sufsum(c, r, n):                  # x[k] <- x[k] + x[k+1] + x[k+2] over the sub-lanes (sub-lane 3 holds zero)
    for i in range(n):
        x = c.w[:, i]
        terms = np.stack([np.where(SUB + k <= 3, x[:, np.minimum(LANE + k, QUAD0 + 3)], 0.0) for k in range(3)])
        s, b = _sum_terms(r, terms, 2)
        r.put(i, s, b)


def sufsum4(c, r): _sufsum(c, r, 4)
def sufsum6(c, r): _sufsum(c, r, 6)


# ---- multiply-adds ---------------------------------------------------------------------------------------------------------------------------
def fmac_rbcast(c, r):                 # acc += (x of lane L) * k
    acc, x, k = c.w[:, 0], c.w[:, 1], c.w[:, 2]
    p = r.t(x[:, [c.targ]] * k)
    r.put(0, acc + p, 2 * U * (np.abs(acc) + np.abs(p)))


def _gram_rows(c, r, rows, g0):        # g[L] = g0[L] + sum_i y[i] * (x[i] of lane L), L in rows
    x, y = c.w[:, 0:6], c.w[:, 6:12]
    for L in range(16):
        g = g0[:, L].copy()
        mag = np.abs(g)
        if L in rows:
            for i in range(6):
                p = r.t(y[:, i] * x[:, i, [L]])
                g = r.t(g + p)
                mag = mag + np.abs(p)
        r.put(L, g, 12 * U * mag)      # six products and six sums (unfused), or six fused steps


def gram4(c, r):                       # the chain of blocks 0 .. targ: rows 4 t + S, S <= targ
    _gram_rows(c, r, [4 * t + s for t in range(4) for s in range(c.targ + 1)], c.w[:, 12:28])


def gram16(c, r):
    _gram_rows(c, r, range(16), np.zeros_like(c.w[:, 12:28]))


def _turns(c, r, order, neg_lo, kword):
    """Gauss-Seidel turns of the lanes in `order`: the pending increment clamped, the lane whose turn it is keeps it, every lane's moves by k * d.
    Bound: the plain forward bound n u sum |t_i| per output.  A lane's u is u0 + sum_t d_t k_t: the terms are u0 and the T products, their magnitudes those of
    the float64 run, and n = 2 T, the roundings on the longest path (the unfused twin rounds product and sum of every turn; the GPU's v_fmac half of that).  The
    increment lane L keeps is its clamped u when its turn comes: the terms that had entered by then, same n.  A lane without a turn keeps its dl: bound 0."""
    u, dl, lo, hi = c.w[:, 0].copy(), c.w[:, 1].copy(), c.w[:, 2], c.w[:, 3]
    if neg_lo:
        lo = -lo
    mag = np.abs(u)
    n = 2 * len(order)
    bdl = np.zeros_like(u)
    for t, L in enumerate(order):
        d = np.minimum(np.maximum(u, lo), hi)
        dl[:, L] = d[:, L]
        bdl[:, L] = n * U * mag[:, L]
        with np.errstate(invalid='ignore'):
            p = r.t(d[:, [L]] * c.w[:, kword(t, L)])
            u = r.t(u + p)
        mag = mag + np.abs(p)
    r.put(0, u, n * U * mag)
    r.put(1, dl, bdl)


def turns4(c, r):
    s = c.targ & 3
    _turns(c, r, [s, 4 + s, 8 + s, 12 + s], bool(c.targ & 16), lambda t, L: 4 + t)


def turns8(c, r):
    h = c.targ & 1
    _turns(c, r, [[0, 4, 8, 12, 1, 5, 9, 13], [2, 6, 10, 14, 3, 7, 11, 15]][h], bool(c.targ & 16), lambda t, L: 4 + L)


def turns16(c, r):
    _turns(c, r, [4 * t + s for s in range(4) for t in range(4)], False, lambda t, L: 4 + L)


def cone_turns4(c, r):
    """sc = clamp(lim * rsq(S1^2 + S2^2), 0, 1) with 0 * inf = 0 (a row without normal force lands on 0 whatever the length) and a pair of length zero
    under a positive bound on sc = 1; the lane whose turn it is keeps e = S * sc - lambda for both rows; every lane's S moves by the 2 x 2 coupling.
    Bound: 32 * u * M, M the largest magnitude among the row's inputs and its intermediate S (each turn about 8 u M: six roundings and v_rsq's 1 ulp;
    the coupling gain 1/2 makes four turns sum to under 16 u M; a factor 2 of margin)."""
    S1, S2, d1, d2 = (c.w[:, i].copy() for i in range(4))
    lam1, lam2, lim = c.w[:, 4], c.w[:, 5], c.w[:, 6]
    M = np.abs(c.w[:, :72]).max(axis=(1, 2))
    for t in range(4):
        L = 4 * t + c.targ
        len2 = r.t(r.t(S2 * S2) + r.t(S1 * S1))
        with np.errstate(divide='ignore', invalid='ignore'):
            sc = np.where(lim == 0.0, 0.0, np.clip(lim / np.sqrt(len2), 0.0, 1.0))
        e1 = r.t(r.t(S1 * sc) - lam1)
        e2 = r.t(r.t(S2 * sc) - lam2)
        d1[:, L] = e1[:, L]
        d2[:, L] = e2[:, L]
        S1 = r.t(r.t(S1 + r.t(e1[:, [L]] * c.w[:, 8 + L])) + r.t(e2[:, [L]] * c.w[:, 24 + L]))
        S2 = r.t(r.t(S2 + r.t(e1[:, [L]] * c.w[:, 40 + L])) + r.t(e2[:, [L]] * c.w[:, 56 + L]))
        M = np.maximum(M, np.maximum(np.abs(S1).max(axis=1), np.abs(S2).max(axis=1)))
    b = np.repeat((32 * U * M)[:, None], 16, axis=1)
    for word, v in enumerate([S1, S2, d1, d2]):
        r.put(word, v, b)


def _vel_coeffs(c, base):
    return c.w[:, base:base + 4], c.w[:, base + 4:base + 6], c.w[:, base + 6:base + 10]        # ca[k], cb[k], cj[k]


def vel_dot(c, r):                     # c + sum_k ca[k] VA[s ^ k] + sum_k cb[k] VB[s ^ k] + sum_k cj[k] VJ[s ^ k]
    ca, cb, cj = _vel_coeffs(c, 1)
    VA, VB, VJ = c.w[:, 11], c.w[:, 12], c.w[:, 13]
    acc = c.w[:, 0].copy()
    mag = np.abs(acc)
    for co, V, n in ((ca, VA, 4), (cb, VB, 2), (cj, VJ, 4)):
        for k in range(n):
            p = r.t(co[:, k] * V[:, LANE ^ k])
            acc = r.t(acc + p)
            mag = mag + np.abs(p)
    r.put(0, acc, 20 * U * mag)


def _vel_commit_sums(c, r, rows):
    """dx += sum over the 16 lanes of gt * dl, dq += sum over the leg's 4 lanes of jt * dl, with lane m's coefficients stored as ca[k] = gt[s ^ k],
    cb[k] = gt[4 + ((s ^ k) & 1)], cj[k] = jt[s ^ k], and the result laid out as VA (lane (leg, s): dx[s]), VB (dx[4 + (s & 1)]), VJ (dq_leg[s])."""
    R = c.w.shape[0]
    tA, tB, tJ = np.zeros((R, 4)), np.zeros((R, 2)), np.zeros((R, 4, 4))
    mA, mB, mJ = np.zeros((R, 4)), np.zeros((R, 2)), np.zeros((R, 4, 4))
    for dlw, base in rows:
        ca, cb, cj = _vel_coeffs(c, base)
        dl = c.w[:, dlw]
        for m in range(16):
            s = m & 3
            for k in range(4):
                p = r.t(ca[:, k, m] * dl[:, m]); tA[:, s ^ k] = r.t(tA[:, s ^ k] + p); mA[:, s ^ k] += np.abs(p)
                p = r.t(cj[:, k, m] * dl[:, m]); tJ[:, m >> 2, s ^ k] = r.t(tJ[:, m >> 2, s ^ k] + p); mJ[:, m >> 2, s ^ k] += np.abs(p)
            for k in range(2):
                p = r.t(cb[:, k, m] * dl[:, m]); tB[:, (s ^ k) & 1] = r.t(tB[:, (s ^ k) & 1] + p); mB[:, (s ^ k) & 1] += np.abs(p)
    VA, VB, VJ = c.w[:, 11], c.w[:, 12], c.w[:, 13]
    n = 18     # the longest path of either side: the twin's product, sixteen sums in lane order and the add into the state (the GPU's tree: 6 or 7 roundings)
    r.put(0, VA + tA[:, SUB], n * U * (np.abs(VA) + mA[:, SUB]))
    r.put(1, VB + tB[:, SUB & 1], n * U * (np.abs(VB) + mB[:, SUB & 1]))
    r.put(2, VJ + tJ[:, LEG, SUB], n * U * (np.abs(VJ) + mJ[:, LEG, SUB]))


def vel_commit(c, r):
    _vel_commit_sums(c, r, [(0, 1)])
    r.put(3, c.w[:, 14] + c.w[:, 0], U * (np.abs(c.w[:, 14]) + np.abs(c.w[:, 0])))


def vel_commit2(c, r):
    _vel_commit_sums(c, r, [(0, 1), (16, 17)])
    r.put(3, c.w[:, 14] + c.w[:, 0], U * (np.abs(c.w[:, 14]) + np.abs(c.w[:, 0])))
    r.put(4, c.w[:, 15] + c.w[:, 16], U * (np.abs(c.w[:, 15]) + np.abs(c.w[:, 16])))


class _Case64:
    def __init__(self, case):
        self.__dict__.update(case.__dict__)
        self.w, self.aux = case.w.astype(np.float64), case.aux.astype(np.float64)


def run(name, case, host_statement=False):
    case = _Case64(case)
    r = Res(case)
    fn = globals()[name]
    if host_statement and name == 'row_ballot':
        fn = row_ballot_host
    fn(case, r)
    return r
