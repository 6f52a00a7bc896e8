"""ctypes binding of include/hl/llenv_hl_league.h: the league actor of the SEPMC engine.  Robot 0 of every arena is the learner (slot 0: policy
and value branch), robot 1 acts with one of n_opponents opponent slots, drawn per episode on the device from host-supplied probabilities; only the
learner's rows are recorded, as the SEPMC rows of policies.hl_unroll, and every finished episode is tallied under the slot it was played against.

    lg = HlLeagueActor(engine, n_opponents=4, unroll_length=128, n_buffers=2)
    lg.set_weights(0, 'sepmc_policy.npz', value_npz='sepmc_value.npz')     # the learner
    for k, path in enumerate(opponent_models):
        lg.set_weights(1 + k, path)
    lg.set_probs(pfsp_probabilities)        # from the league manager's win rates
    lg.steps(seed, 129)                     # asynchronous on the engine's stream
    lg.finish(0)
    f = lg.split_row(lg.block(0))           # [n_arenas][128][...] torch views, as HlUnrollRecorder's
    lg.outcomes(clear=True)                 # [n_opponents][5]: episodes | fall | time | catch | nonfinite
"""
import ctypes as C
import os

import numpy as np

from .. import capi
from . import hl_policy_hip as H
from . import hl_unroll as U

MAX_OPPONENTS = 8
OUTCOMES = ('episodes', 'fall', 'time', 'catch', 'nonfinite')       # LLG_N_OUTCOMES columns

_SIGS = {
    'll_hl_league_create': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    'll_hl_league_destroy': (C.c_int, [C.c_void_p]),
    'll_hl_league_set_weights': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    'll_hl_league_set_probs': (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int]),
    'll_hl_league_steps': (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_int]),
    'll_hl_league_position': (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    'll_hl_league_layout': (C.c_int, [C.c_void_p, C.POINTER(U.LLHlUnrollLayout)]),
    'll_hl_league_finish': (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p]),
    'll_hl_league_get_assignment': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'll_hl_league_get_outcomes': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    'll_hl_league_get_state': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'll_hl_league_plan_only': (C.c_int, [C.c_void_p, C.c_int]),
}
EXPORTED_SYMBOLS = sorted(_SIGS)


def load_library(path=None):
    return capi.bind(U.load_library(path), _SIGS)


row_layout = U.row_layout
split_row = U.split_row


class HlLeagueActor(capi.NativeHandle):
    """ll_hl_league over `engine` (a SepmcEngine created with auto_reset, or a game holding one as .engine), which must stay open while the
    league lives."""
    _destroy = 'll_hl_league_destroy'

    def __init__(self, engine, n_opponents, unroll_length, n_buffers=2, lib_path=None):
        from ..sepmc_capi import SepmcEngine
        self._open(load_library(lib_path))
        eng = getattr(engine, 'engine', engine)
        if not isinstance(eng, SepmcEngine):
            raise TypeError('HlLeagueActor drives a SepmcEngine, not %r' % type(eng).__name__)
        self.engine = eng
        self._chk(self.lib.ll_hl_league_create(eng.h, int(n_opponents), int(unroll_length), int(n_buffers), C.byref(self.h)))
        lay = U.LLHlUnrollLayout()
        self._chk(self.lib.ll_hl_league_layout(self.h, C.byref(lay)))
        self.layout = lay
        self.n_opponents = int(n_opponents)
        self.kind, self.row_floats, self.n_rows = int(lay.kind), int(lay.row_floats), int(lay.n_rows)
        self.n_arenas = self.n_rows
        self.unroll_length, self.n_buffers = int(lay.unroll_length), int(lay.n_buffers)
        self.d_base, self.n_bytes = int(lay.d_base), int(lay.n_bytes)
        self.fields = {name: (int(lay.off[i]), int(lay.dim[i])) for i, name in enumerate(U.LLU_FIELDS)}

    def set_weights(self, slot, weights, value_npz=None, value_weights=None):
        """A new model for `slot` (0: the learner, with its value branch; 1 .. n_opponents: an opponent, policy only), uploaded in the order of
        the engine's stream; no recurrent state is touched.  weights: an .npz path (tests/golden/sepmc_policy.npz layout) or the packed
        float32 array; the value branch likewise through value_npz or value_weights."""
        w = H.pack_weights(H.LLH_SEPMC, weights) if isinstance(weights, (str, bytes, os.PathLike)) else np.ascontiguousarray(weights, dtype=np.float32)
        v = None
        if value_npz is not None:
            v = H.pack_value_weights(H.LLH_SEPMC, value_npz)
        elif value_weights is not None:
            v = np.ascontiguousarray(value_weights, dtype=np.float32)
        self._chk(self.lib.ll_hl_league_set_weights(self.h, int(slot), w.ctypes.data_as(C.c_void_p), int(w.size),
                                                    v.ctypes.data_as(C.c_void_p) if v is not None else None, int(v.size) if v is not None else 0))

    def set_probs(self, probs):
        """The probability of every opponent slot for the draws of later steps (non-negative, sum 1): PFSP's weighting of the win rates."""
        p = np.ascontiguousarray(probs, dtype=np.float64).ravel()
        self._chk(self.lib.ll_hl_league_set_probs(self.h, p.ctypes.data_as(C.POINTER(C.c_double)), int(p.size)))

    def steps(self, seed, n_steps, sample=True):
        """n_steps x { draw ; act ; step } recorded, queued on the engine's stream; the Philox step index is the league's own step count."""
        self._chk(self.lib.ll_hl_league_steps(self.h, int(seed) & 0xFFFFFFFFFFFFFFFF, 1 if sample else 0, int(n_steps)))

    def position(self):
        """(unroll index, time step) the NEXT step writes; unroll k lives in block k % n_buffers"""
        k, t = C.c_int64(0), C.c_int(0)
        self._chk(self.lib.ll_hl_league_position(self.h, C.byref(k), C.byref(t)))
        return k.value, t.value

    def finish(self, buffer, gamma=0.95, lam=0.95, d_bootstrap=None):
        """TD(lambda) returns into R of block `buffer`, as HlUnrollRecorder.finish"""
        self._chk(self.lib.ll_hl_league_finish(self.h, int(buffer), float(gamma), float(lam), C.c_void_p(int(d_bootstrap)) if d_bootstrap else None))

    def buffers(self):
        """the whole ring as a torch tensor [n_buffers][n_arenas][unroll_length][row_floats] (no copy)"""
        from .. import gather
        return gather.device_tensor(self.d_base, (self.n_buffers, self.n_rows, self.unroll_length, self.row_floats))

    def block(self, k):
        """torch view of the block unroll k lives in, [n_arenas][unroll_length][row_floats]: the learner's rows"""
        return self.buffers()[k % self.n_buffers]

    def split_row(self, block):
        return U.split_row(block, self.fields)

    def assignment(self):
        """(slot [n_arenas] int32: the slot robot 1 of every arena acts with, 0 before the first step; episodes [n_arenas] int64: the episodes
        the arena has started).  Waits for the device."""
        s, e = np.zeros(self.n_arenas, np.int32), np.zeros(self.n_arenas, np.int64)
        self._chk(self.lib.ll_hl_league_get_assignment(self.h, s.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p)))
        return s, e

    def outcomes(self, clear=False):
        """[n_opponents][5] uint64, columns OUTCOMES: the finished episodes under the slot they were played against.  Waits for the device."""
        o = np.zeros((self.n_opponents, len(OUTCOMES)), np.uint64)
        self._chk(self.lib.ll_hl_league_get_outcomes(self.h, o.ctypes.data_as(C.c_void_p), 1 if clear else 0))
        return o

    def state(self):
        """(policy state [2 n_arenas][128] of every row under its acting policy, value state [n_arenas][64] of the learner).  Waits for the device."""
        s, v = np.zeros((2 * self.n_arenas, 128), np.float32), np.zeros((self.n_arenas, H.VALUE_STATE_DIM), np.float32)
        self._chk(self.lib.ll_hl_league_get_state(self.h, s.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p)))
        return s, v

    def plan_only(self, n_launches):
        """n launches of the plan kernel that tally and draw nothing (for measuring)"""
        self._chk(self.lib.ll_hl_league_plan_only(self.h, int(n_launches)))
