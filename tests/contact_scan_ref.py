"""Statements of the step kernels' leg-leg pick (the member self_pick of Pmc<L>, lifelike_agility_and_play_amd/csrc/pmc_step.hpp) and of its terrain-edge detectors
(reverse_edge, leg_edge: terrain_edge() at the end of this file, in float64 with a forward-error model), written from the RULE and not from the kernel text, in NumPy.

self_pick      the oracle's rule for equally deep candidates (oracle/pmc_oracle.c: "candidates within LLM_SELECT_EPS of the deepest are equally deep: the lowest index
               wins") over the up to 32 capsule pairs of a row (16 lanes x 2), evaluated on the float32 depths: the closest pair dmin; pairs with
               depth <= float32(dmin + float32(LLM_SELECT_EPS)) are equally close and the lowest PAIR INDEX wins (the pair indices of a row are all different).  The slot
               gets that pair's own depth, and its point and normal as sums over the row in which the other lanes add +0 (x + 0 in float32: a -0 arrives as +0), and the
               pair is cleared (1e30).  Without any pair (dmin >= 1e29) have is false, dsel is 0 and nothing is cleared; cmin and u6 then say nothing (NaN here: held to
               the twin's bits only).
               Every comparison is one of float32 values and the only arithmetic is the one float32 addition of the threshold, so the rule is a function of the input
               BITS: GPU, host twin and statement agree bit for bit on every input, a tie at the threshold included.

The statement takes switches that make it wrong the way a kernel could be (tests/test_contact_scan_emul.py shows that the tests' own inputs tell them apart):
  highest_index   the highest pair index among the pairs within the threshold instead of the lowest
  strict          `<` at the threshold instead of `<=`
"""
import numpy as np

FAR = np.float32(1.0e30)
SELECT_EPS = np.float32(1e-5)          # (float)LLM_SELECT_EPS, include/llenv_model.h
SUB = np.arange(16) % 4
LEG = np.arange(16) // 4


def _plus_zero(x): return (np.asarray(x, dtype=np.float32) + np.float32(0.0)).astype(np.float32)


def self_pick(cd, cpair, cP, cN, slots, highest_index=False, strict=False):
    """cd, cpair [R, 2, 16]; cP, cN [R, 2, 3, 16] float32 -> [R, slots, 11] per slot: have | cmin | dsel | u6[0..5] (row-uniform) and cd_after [R, slots, 2, 16]"""
    cd = np.asarray(cd, dtype=np.float32).copy()
    R = len(cd)
    code = np.asarray(cpair, dtype=np.float32).reshape(R, 32)          # index = 16 * pass + lane
    pn = np.concatenate([np.asarray(cP, dtype=np.float32).transpose(0, 2, 1, 3).reshape(R, 3, 32), np.asarray(cN, dtype=np.float32).transpose(0, 2, 1, 3).reshape(R, 3, 32)], axis=1)
    assert all(len(set(row.tolist())) == 32 for row in code), 'the pair indices of a row are all different'
    out, after = np.full((R, slots, 9), np.nan), np.zeros((R, slots, 2, 16), dtype=np.float32)
    rows = np.arange(R)
    for s in range(slots):
        d = cd.reshape(R, 32)
        dmin = d.min(axis=1)
        have = dmin < np.float32(1.0e29)
        thr = (dmin + SELECT_EPS).astype(np.float32)
        within = (d < thr[:, None]) if strict else (d <= thr[:, None])
        if strict:
            within |= d == dmin[:, None]
        key = np.where(within, code, -1.0 if highest_index else 1.0e9)
        cmin = key.max(axis=1) if highest_index else key.min(axis=1)
        w = np.argmax(within & (code == cmin[:, None]), axis=1)
        out[:, s, 0] = have
        out[:, s, 1] = np.where(have, cmin, np.nan)
        out[:, s, 2] = np.where(have, d[rows, w], 0.0)
        out[:, s, 3:9] = np.where(have[:, None], _plus_zero(pn[rows, :, w]), np.nan)
        d[rows[have], w[have]] = FAR
        after[:, s] = cd
    return out, after


def pair_codes():
    """the oracle's pair index of the two pairs a lane tests, as substep_impl forms it: pass 0 the previous leg's capsule against the own, pass 1 (legs 0 and 1 only) the
    own against the leg two away; capsule bits: bit 0 = A's, bit 1 = B's  -> [2, 16]"""
    lp0 = np.where(LEG == 0, 3, LEG - 1)
    sp1 = (SUB >> 1) + 2 * (SUB & 1)
    return np.stack([lp0 * 4 + SUB, (LEG + 4) * 4 + sp1]).astype(np.float32)


# ---- terrain edges against the body box (reverse_edge) and the leg boxes (leg_edge) ---------------------------------------------------------------------------------
# Written from the rule as the comments above the two members (and the oracle's edge_vs_box) give it, in float64 on the float32 inputs, with the forward-error arithmetic
# of tests/math_helpers_ref.py (E: a float64 value and a bound on |float32 evaluation - value|) so that one pass gives the statement, its bound and the margin of every
# decision.  oracle/ keeps its reverse_edge and leg_reverse_edge static (not exposed to Python), so there is no cross-check against it here; the whole-step parity tests
# are that check.
#   1. the edge (edge e of the box record: 0 x = x0, 1 x = x1, 2 y = y0, 3 y = y1; at the top z1, at the bottom z0 of a box that floats, z0 > LLM_FLOATING_MIN_Z; turned
#      about (ycx, ycy) in a yawed arena) is cut to the robot box grown by the margin: nothing left, no candidate;
#   2. the middle of the rest names the face: the axis of largest |p_i| - h_i (leg boxes: the axis the edge is most parallel to is no candidate);
#   3. the edge is cut to the exact extents of the other two axes; reverse_edge takes end `endf` of the piece, leg_edge the deeper end (the first on a tie);
#      depth = signed distance to the face's plane, point = the point of the terrain edge (returned in the base frame), normal = the face's inward normal (world);
#   4. the deepest over the boxes (the first on a tie), for leg_edge over the thigh box and then the shank box too.  None: depth 1e30, the zero point, normal +z.
# Switches that make it wrong: top_edge_of_floating (a floating box offers its top edges), parallel_axis_allowed (leg_edge: no axis excluded), ends_swapped.
TIE = 1e-12               # depths closer than this are a tie (the first wins): the leg tables carry entries of 1e-18 (the URDF's cos(pi / 2)) that move a float64 depth by
                          # 1e-19, which no float32 evaluation sees; anything a float32 can tell apart is five orders above it
MARGIN, FLOATING_MIN_Z = 0.02, np.float32(0.05)          # LLM_CONTACT_MARGIN, LLM_FLOATING_MIN_Z (include/llenv_model.h)
BC_BOX, LC_THBOX, LC_SHBOX = 19, 69, 114                  # csrc/pmc_params.hpp


def _eabs(a):
    from math_helpers_ref import E
    return E(np.abs(a.v), a.e)


def _margin(a, b, alive=True):
    """how far the comparison of a and b is from flipping in float32: |a - b| less both bounds; operands without any error compare as they are (inf)"""
    from math_helpers_ref import E
    a, b = E.of(a), E.of(b)
    with np.errstate(invalid='ignore'):
        m = np.where((a.e + b.e) == 0, np.inf, np.abs(a.v - b.v) - (a.e + b.e))
    return np.where(alive, m, np.inf)


def _edge_vs_box(rec, n_shapes, yaw, e_idx, cw, W, h, end, across, st, link_id, wrong):
    """steps 1 - 4 for one robot box against every listed record; st: the running best (dict of E), updated in place"""
    from math_helpers_ref import E, esel, emax, emin
    N = len(e_idx)
    yawed, ycx, ycy, ycs, ysn = yaw
    for si in range(rec.shape[1]):
        r = rec[:, si].astype(np.float64)
        listed = si < n_shapes
        floats = rec[:, si, 4] > FLOATING_MIN_Z
        ze = np.where(floats & (not wrong.get('top_edge_of_floating')), r[:, 4], r[:, 5])
        al = [np.where(e_idx == 1, r[:, 1], r[:, 0]), np.where(e_idx == 3, r[:, 3], r[:, 2])]
        bl = [np.where(e_idx == 0, r[:, 0], r[:, 1]), np.where(e_idx == 2, r[:, 2], r[:, 3])]
        aw = [esel(yawed, E(ycx) + E(al[0]) * E(ycs) - E(al[1]) * E(ysn), E(al[0])), esel(yawed, E(ycy) + E(al[0]) * E(ysn) + E(al[1]) * E(ycs), E(al[1])), E(ze)]
        bw = [esel(yawed, E(ycx) + E(bl[0]) * E(ycs) - E(bl[1]) * E(ysn), E(bl[0])), esel(yawed, E(ycy) + E(bl[0]) * E(ysn) + E(bl[1]) * E(ycs), E(bl[1])), E(ze)]
        ra, dw = [aw[k] - cw[k] for k in range(3)], [bw[k] - aw[k] for k in range(3)]
        pa = [ra[0] * W[3 * i] + ra[1] * W[3 * i + 1] + ra[2] * W[3 * i + 2] for i in range(3)]
        d = [dw[0] * W[3 * i] + dw[1] * W[3 * i + 1] + dw[2] * W[3 * i + 2] for i in range(3)]
        margins = []
        # the parameter interval of the edge inside a slab |p_i| <= half: it enters at the smaller and leaves at the larger of the two crossings (a component that does
        # not move, below 1e-9, counts as moving by 1e-9: the crossings go to +-infinity-like values on the right sides)
        def slab(i, half):
            step = esel(np.abs(d[i].v) < 1e-9, E(np.float64(np.float32(1e-9))), d[i])
            per = 1.0 / step
            c0, c1 = ((-half) - pa[i]) * per, (half - pa[i]) * per
            return emin(c0, c1), emax(c0, c1)
        take = lambda xs, k: E(np.choose(k, [x.v for x in xs]), np.choose(k, [np.broadcast_to(x.e, (N,)) for x in xs]))
        for i in range(3):
            margins.append(_margin(_eabs(d[i]), 1e-9, listed))
        grown = [slab(i, h[i] + E.of(MARGIN)) for i in range(3)]
        exact = [slab(i, h[i]) for i in range(3)]
        t_in, t_out = E(np.zeros(N)), E(np.ones(N))
        for enter, leave in grown:                 # 1. cut to the box grown by the margin
            t_in, t_out = emax(t_in, enter), emin(t_out, leave)
        valid = listed & (t_in.v <= t_out.v)
        margins.append(_margin(t_in, t_out, listed))
        mid = (t_in + t_out) * 0.5
        pm = [pa[i] + mid * d[i] for i in range(3)]
        out_by = [_eabs(pm[i]) - h[i] for i in range(3)]          # how far the middle lies outside each pair of faces
        allowed = np.ones((3, N), dtype=bool)
        if across and not wrong.get('parallel_axis_allowed'):     # the axis the edge is most parallel to (the first of equals) is no candidate
            ad = [_eabs(x) for x in d]
            par = np.argmax(np.stack([x.v for x in ad]), axis=0)
            allowed[par, np.arange(N)] = False
            for i in range(3):
                margins.append(_margin(take(ad, par), ad[i], valid & (par != i)))
        face = np.argmax(np.where(allowed, np.stack([x.v for x in out_by]), -np.inf), axis=0)          # 2. the face: the largest of them (the first of equals)
        for i in range(3):
            margins.append(_margin(take(out_by, face), out_by[i], valid & (face != i) & allowed[i]))
        side = take(pm, face)
        sg = np.where(side.v >= 0, 1.0, -1.0)
        margins.append(_margin(side, 0.0, valid))
        u0, u1 = E(np.zeros(N)), E(np.ones(N))
        for i, (enter, leave) in enumerate(exact):                # 3. cut to the exact extents of the two other axes
            u0 = esel(face == i, u0, emax(u0, enter))
            u1 = esel(face == i, u1, emin(u1, leave))
        margins.append(_margin(u0, u1, valid))
        valid = valid & (u0.v <= u1.v)
        pick = lambda xs: take(xs, face)
        pax, dax, hax = pick(pa), pick(d), pick(h)
        dep0, dep1 = E(sg) * (pax + u0 * dax) - hax, E(sg) * (pax + u1 * dax) - hax
        if end is None:                     # leg_edge: the deeper end, the first on a tie
            second = dep1.v < dep0.v - TIE
            margins.append(_margin(dep1, dep0, valid))
        else:
            second = end > 0.5
        if wrong.get('ends_swapped'):
            second = ~second
        dep, u = esel(second, dep1, dep0), esel(second, u1, u0)
        better = valid & (dep.v < st['depth'].v - TIE)
        margins.append(_margin(dep, st['depth'], valid))
        st['hit_margin'] = np.minimum(st['hit_margin'], np.where(valid, np.abs(dep.v - MARGIN) - dep.e - MARGIN * 2.0 ** -24, np.inf))
        st['depth'] = esel(better, dep, st['depth'])
        st['Pw'] = [esel(better, aw[k] + u * dw[k], st['Pw'][k]) for k in range(3)]
        st['nw'] = [esel(better, E(-sg) * pick([W[k], W[3 + k], W[6 + k]]), st['nw'][k]) for k in range(3)]
        st['shape'] = np.where(better, float(si), st['shape'])
        st['link'] = np.where(better, link_id, st['link'])
        st['margin'] = np.minimum(st['margin'], np.min(margins, axis=0))


def terrain_edge(name, X, legc, basec, **wrong):
    """X [R, words, 16] float32 (the driver's input words) -> v, e [R, 9, 16] (depth | Pb | nw | link | shape; reverse_edge leaves the last two NaN), sure [R, 16], hit [R, 16]"""
    import math_helpers_ref as mr
    from math_helpers_ref import E, esel
    R_ = len(X)
    N = R_ * 16
    lane = np.tile(np.arange(16), R_)
    leg = lane // 4
    uni = lambda w: np.repeat(X[:, w, 0].astype(np.float64), 16)
    per = lambda w: X[:, w].reshape(N).astype(np.float64)
    p, Rm = [E(uni(k)) for k in range(3)], [E(uni(3 + k)) for k in range(9)]
    n_shapes = np.clip(np.rint(uni(12)), 0, 6)
    yaw = (uni(13) > 0.5, uni(14), uni(15), uni(16), uni(17))
    rec = np.repeat(X[:, 24:72, 0].reshape(R_, 6, 8), 16, axis=0)
    end = per(21)
    st = dict(depth=E(np.full(N, np.float64(FAR))), Pw=[E(np.zeros(N))] * 3, nw=[E(np.zeros(N)), E(np.zeros(N)), E(np.ones(N))], shape=np.full(N, -1.0), link=np.full(N, 3.0),
              margin=np.full(N, np.inf), hit_margin=np.full(N, np.inf))
    if name == 'reverse_edge':
        bc = basec.astype(np.float64)[BC_BOX:BC_BOX + 12]
        h, W = [], []
        for a in range(3):
            u = [E(np.full(N, bc[3 + 3 * a + k])) for k in range(3)]
            ha = mr.dot3(u, u).sqrt()
            h.append(ha)
            W += [x * (1.0 / ha) for x in mr.mulMV(Rm, u)]
        cw = mr.add3(p, mr.mulMV(Rm, [E(np.full(N, bc[k])) for k in range(3)]))
        _edge_vs_box(rec, n_shapes, yaw, leg, cw, W, h, end, False, st, 3.0, wrong)
    else:
        class Ctx:
            pass
        ctx = Ctx()
        ctx.legc = legc
        fk = mr._leg_fk(ctx, leg, [E(per(18)), E(per(19)), E(per(20))])
        e_idx = np.rint(end).astype(int)
        for lb, (Rk, pk, f0) in enumerate(((fk[1], fk[4], LC_THBOX), (fk[2], fk[5], LC_SHBOX))):
            L3 = lambda f: [E(legc[f + k, leg].astype(np.float64)) for k in range(3)]
            cw = mr.add3(mr.mulMV(Rm, mr.add3(pk, mr.mulMV(Rk, L3(f0)))), p)
            h, W = [], []
            for a in range(3):
                u = L3(f0 + 3 + 3 * a)
                ha = mr.dot3(u, u).sqrt()
                h.append(ha)
                W += [x * (1.0 / ha) for x in mr.mulMV(Rm, mr.mulMV(Rk, u))]
            _edge_vs_box(rec, n_shapes, yaw, e_idx, cw, W, h, None, True, st, 2.0 + lb, wrong)
    Pb = mr.mulTMV(Rm, [st['Pw'][k] - p[k] for k in range(3)])
    outs = [st['depth']] + Pb + st['nw']
    v, e = np.full((N, 9), np.nan), np.full((N, 9), np.nan)
    for w, x in enumerate(outs):
        v[:, w], e[:, w] = x.v, x.e
    if name == 'leg_edge':
        v[:, 7], v[:, 8], e[:, 7:] = st['link'], st['shape'], 0.0
    sh = lambda a: a.reshape(R_, 16, -1).transpose(0, 2, 1)
    sure = (np.minimum(st['margin'], st['hit_margin']) > 0).reshape(R_, 16)
    return sh(v), sh(e), sure, (st['depth'].v < MARGIN).reshape(R_, 16)
