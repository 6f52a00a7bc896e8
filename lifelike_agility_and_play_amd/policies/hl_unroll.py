"""ctypes binding of include/hl/llenv_hl_unroll.h: the actor loop  act_pg ; step  of an EPMC / SEPMC engine and an on-device policy with a value
branch, recorded on the device as learner-ready unroll blocks [n_buffers][n_rows][unroll_length][row_floats] (one float32 row per robot and
control step: X, A, neglogp, R, V, r, discount, S, M -- the input tuple of the reference's epmc_net).

    pol = HipEpmcPolicy('epmc_policy_hurdle.npz', max_rows=4096, value_npz='epmc_value_hurdle.npz')
    rec = HlUnrollRecorder(engine, pol, unroll_length=128, n_buffers=2)
    rec.steps(seed, 129)                 # unroll 0 and the first step of unroll 1, asynchronous on the engine's stream
    rec.finish(0, gamma=0.95, lam=0.95)  # TD(lambda) returns of block 0, bootstrapped from V of unroll 1's first row
    f = split_row(rec.block(0))          # named torch views: f['X'] [n_rows][128][916], f['R'] [n_rows][128], ...
"""
import ctypes as C

from .. import capi
from . import hl_policy_hip as H

LLU_FIELDS = ('X', 'A', 'neglogp', 'R', 'V', 'r', 'discount', 'S', 'M', 'pad')      # LLU_X .. LLU_PAD
A_DIM = {H.LLH_EPMC: 13, H.LLH_SEPMC: 14}            # [heading (SEPMC)] | z code | action[12]
S_DIM = {H.LLH_EPMC: 192, H.LLH_SEPMC: 256}          # vf | pi | z [| hlc], each c[32] | h[32]
ROW_FLOATS = {H.LLH_EPMC: 1128, H.LLH_SEPMC: 1244}


class LLHlUnrollLayout(C.Structure):   # struct ll_hl_unroll_layout_t
    _fields_ = [('kind', C.c_int32), ('row_floats', C.c_int32), ('n_rows', C.c_int32), ('unroll_length', C.c_int32), ('n_buffers', C.c_int32),
                ('reserved', C.c_int32), ('off', C.c_int32 * len(LLU_FIELDS)), ('dim', C.c_int32 * len(LLU_FIELDS)), ('d_base', C.c_void_p),
                ('n_bytes', C.c_uint64)]


_SIGS = {
    'll_hl_unroll_create_epmc': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    'll_hl_unroll_create_sepmc': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    'll_hl_unroll_destroy': (C.c_int, [C.c_void_p]),
    'll_hl_unroll_layout': (C.c_int, [C.c_void_p, C.POINTER(LLHlUnrollLayout)]),
    'll_hl_unroll_steps': (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_int]),
    'll_hl_unroll_position': (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    'll_hl_unroll_finish': (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p]),
}
EXPORTED_SYMBOLS = sorted(_SIGS)


def load_library(path=None):
    return capi.bind(H.load_library(path), _SIGS)


def row_layout(kind):
    """{field: (first column, width)} of one row and row_floats, restated from the header (ll_hl_unroll_layout reports the same)."""
    dims = (H.OBS_DIM[kind], A_DIM[kind], H.N_HEADS[kind], 1, 1, 1, 1, S_DIM[kind], 1)
    out, off = {}, 0
    for name, d in zip(LLU_FIELDS, dims):
        out[name] = (off, d)
        off += d
    rf = (off + 3) // 4 * 4
    out['pad'] = (off, rf - off)
    assert rf == ROW_FLOATS[kind]
    return out, rf


def split_row(block, layout=None):
    """Named views of an unroll block [..., row_floats] (NumPy array or torch tensor): X, A, neglogp, S and pad keep their last axis, R, V, r,
    discount and M lose it.  layout: {field: (offset, width)} (HlUnrollRecorder.fields); by default chosen by the row size (1128 EPMC, 1244 SEPMC)."""
    if layout is None:
        kinds = [k for k, rf in ROW_FLOATS.items() if rf == block.shape[-1]]
        if not kinds:
            raise ValueError('rows of %d floats are neither EPMC (1128) nor SEPMC (1244) unroll rows' % block.shape[-1])
        layout = row_layout(kinds[0])[0]
    out = {}
    for name, (off, d) in layout.items():
        out[name] = block[..., off] if name in ('R', 'V', 'r', 'discount', 'M') else block[..., off:off + d]
    return out


class HlUnrollRecorder(capi.NativeHandle):
    """ll_hl_unroll over `engine` (an EpmcEngine / SepmcEngine, or a game holding one as .engine) and `policy` (HipEpmcPolicy / HipSepmcPolicy with
    a value branch).  Both must stay open while the recorder lives."""
    _destroy = 'll_hl_unroll_destroy'

    def __init__(self, engine, policy, unroll_length, n_buffers=2, lib_path=None):
        from ..epmc_capi import EpmcEngine
        from ..sepmc_capi import SepmcEngine
        self._open(load_library(lib_path))
        eng = getattr(engine, 'engine', engine)
        self.engine, self.policy = eng, policy
        if isinstance(eng, EpmcEngine):
            create = self.lib.ll_hl_unroll_create_epmc
        elif isinstance(eng, SepmcEngine):
            create = self.lib.ll_hl_unroll_create_sepmc
        else:
            raise TypeError('HlUnrollRecorder records an EpmcEngine or a SepmcEngine, not %r' % type(eng).__name__)
        self._chk(create(eng.h, policy.h, int(unroll_length), int(n_buffers), C.byref(self.h)))
        lay = LLHlUnrollLayout()
        self._chk(self.lib.ll_hl_unroll_layout(self.h, C.byref(lay)))
        self.layout = lay
        self.kind, self.row_floats, self.n_rows = int(lay.kind), int(lay.row_floats), int(lay.n_rows)
        self.unroll_length, self.n_buffers = int(lay.unroll_length), int(lay.n_buffers)
        self.d_base, self.n_bytes = int(lay.d_base), int(lay.n_bytes)
        self.fields = {name: (int(lay.off[i]), int(lay.dim[i])) for i, name in enumerate(LLU_FIELDS)}

    def steps(self, seed, n_steps, sample=True):
        """n_steps x { act_pg ; step } recorded, queued on the engine's stream; the Philox step index is the recorder's own step count."""
        self._chk(self.lib.ll_hl_unroll_steps(self.h, int(seed) & 0xFFFFFFFFFFFFFFFF, 1 if sample else 0, int(n_steps)))

    def position(self):
        """(unroll index, time step) the NEXT step writes; unroll k lives in block k % n_buffers"""
        k, t = C.c_int64(0), C.c_int(0)
        self._chk(self.lib.ll_hl_unroll_position(self.h, C.byref(k), C.byref(t)))
        return k.value, t.value

    def finish(self, buffer, gamma=0.95, lam=0.95, d_bootstrap=None):
        """TD(lambda) returns into R of block `buffer`; d_bootstrap: device address of [n_rows] float32 values, None: V of the next unroll's first
        row (LLError LL_ESTATE while that step has not run)."""
        self._chk(self.lib.ll_hl_unroll_finish(self.h, int(buffer), float(gamma), float(lam), C.c_void_p(int(d_bootstrap)) if d_bootstrap else None))

    def buffers(self):
        """the whole ring as a torch tensor [n_buffers][n_rows][unroll_length][row_floats] (no copy)"""
        from .. import gather
        return gather.device_tensor(self.d_base, (self.n_buffers, self.n_rows, self.unroll_length, self.row_floats))

    def block(self, k):
        """torch view of the block unroll k lives in, [n_rows][unroll_length][row_floats]"""
        return self.buffers()[k % self.n_buffers]

    def split_row(self, block):
        return split_row(block, self.fields)
