"""ctypes binding of include/hl/llenv_hl_policy.h: the trained EPMC / SEPMC policies as ONE fused kernel each inside libllenv.so,
evaluated straight on an engine's device buffers, with each row's LSTM state kept on the device.  `oracle/epmc_policy.py` and
`oracle/sepmc_policy.py` (NumPy, float64) state the same forward pass.

    pol = HipEpmcPolicy('epmc_policy_hurdle.npz', max_rows=4096)
    for t in range(T):
        pol.act(engine)          # obs -> actions on the engine's stream; rows whose done flag is set start from zero state
        engine.step()

The PPO actor (ll_hl_policy_act_pg): every head sampled, its neglogp and the value of a second network with its own LSTM state:

    pol = HipEpmcPolicy('epmc_policy_hurdle.npz', max_rows=4096, value_npz='epmc_value_hurdle.npz')
    for t in range(T):
        pol.act_pg(engine, seed, t, d_neglogp=neglogp.data_ptr(), d_value=value.data_ptr())
        engine.step()
"""
import ctypes as C

import numpy as np

from .. import capi

LLH_EPMC, LLH_SEPMC = 1, 2
N_FLOATS = {LLH_EPMC: 208437, LLH_SEPMC: 316806}
OBS_DIM = {LLH_EPMC: 916, LLH_SEPMC: 965}
ARRAYS = {LLH_EPMC: [0, 1] + list(range(47, 102)), LLH_SEPMC: [0, 1] + list(range(51, 152))}    # checkpoint array numbers, packing order
VF_N_FLOATS = {LLH_EPMC: 137872, LLH_SEPMC: 182864}
VF_ARRAYS = {LLH_EPMC: list(range(2, 47)), LLH_SEPMC: list(range(2, 51))}                         # the value branch
N_HEADS = {LLH_EPMC: 2, LLH_SEPMC: 3}           # neglogp columns: EPMC z, llc; SEPMC hlc, z, llc
VALUE_STATE_DIM = 64                            # c | h of the value LSTM

_SIGS = {
    'll_hl_policy_create': (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    'll_hl_policy_destroy': (C.c_int, [C.c_void_p]),
    'll_hl_policy_state_dim': (C.c_int, [C.c_void_p]),
    'll_hl_policy_act': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    'll_hl_policy_reset_state': (C.c_int, [C.c_void_p, C.c_void_p]),
    'll_hl_policy_get_state': (C.c_int, [C.c_void_p, C.c_void_p]),
    'll_hl_policy_set_state': (C.c_int, [C.c_void_p, C.c_void_p]),
    'll_hl_policy_attach_value': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    'll_hl_policy_act_pg': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_void_p]),
    'll_hl_policy_get_value_state': (C.c_int, [C.c_void_p, C.c_void_p]),
    'll_hl_policy_set_value_state': (C.c_int, [C.c_void_p, C.c_void_p]),
    'll_hl_policy_set_weights': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    'll_hl_policy_enable_timing': (C.c_int, [C.c_void_p, C.c_int]),
    'll_hl_policy_time_ms': (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
}
EXPORTED_SYMBOLS = sorted(_SIGS)


def load_library(path=None):
    return capi.bind(capi.load_library(path), _SIGS)


def pack_weights(kind, npz_path):
    """The arrays of `kind` from an .npz with keys 'w<k>' (what tools/extract_epmc_policy.py writes), float32, flattened in checkpoint order."""
    z = np.load(npz_path)
    flat = np.concatenate([z['w%d' % k].astype(np.float32).ravel() for k in ARRAYS[kind]])
    assert flat.size == N_FLOATS[kind], (flat.size, N_FLOATS[kind])
    return np.ascontiguousarray(flat)


def pack_value_weights(kind, npz_path):
    """The value branch of `kind` (arrays 2..46 EPMC, 2..50 SEPMC) from an .npz with keys 'w<k>' (tools/extract_epmc_policy.py --value),
    float32, flattened in checkpoint order."""
    z = np.load(npz_path)
    flat = np.concatenate([z['w%d' % k].astype(np.float32).ravel() for k in VF_ARRAYS[kind]])
    assert flat.size == VF_N_FLOATS[kind], (flat.size, VF_N_FLOATS[kind])
    return np.ascontiguousarray(flat)


def _vp(x):
    return C.c_void_p(int(x)) if x else None


class _HipHlPolicy(capi.NativeHandle):
    KIND, _destroy = None, 'll_hl_policy_destroy'

    def __init__(self, npz_path, max_rows, device=0, lib_path=None, weights=None, value_npz=None):
        self._open(load_library(lib_path))
        w = pack_weights(self.KIND, npz_path) if weights is None else np.ascontiguousarray(weights, dtype=np.float32)
        self.max_rows = int(max_rows)
        self._chk(self.lib.ll_hl_policy_create(self.KIND, w.ctypes.data_as(C.c_void_p), int(w.size), self.max_rows, int(device), C.byref(self.h)))
        self.state_dim = int(self.lib.ll_hl_policy_state_dim(self.h))
        self.n_heads = N_HEADS[self.KIND]
        self.has_value = False
        if value_npz is not None:
            self.attach_value(value_npz)

    def attach_value(self, npz_path=None, weights=None):
        """ll_hl_policy_attach_value: the value branch from an .npz (tests/golden/epmc_value_*.npz, sepmc_value.npz) or packed `weights`;
        every row's value state starts at zero."""
        w = pack_value_weights(self.KIND, npz_path) if weights is None else np.ascontiguousarray(weights, dtype=np.float32)
        self._chk(self.lib.ll_hl_policy_attach_value(self.h, w.ctypes.data_as(C.c_void_p), int(w.size)))
        self.has_value = True

    def set_weights(self, npz_path=None, value_npz=None, weights=None, value_weights=None, stream=None):
        """ll_hl_policy_set_weights: a new model (and, with a value branch attached, a new branch) for a policy in use, uploaded in the order
        of `stream` (None: the default stream); no recurrent state is touched."""
        w = pack_weights(self.KIND, npz_path) if weights is None else np.ascontiguousarray(weights, dtype=np.float32)
        v = None
        if value_npz is not None or value_weights is not None:
            v = pack_value_weights(self.KIND, value_npz) if value_weights is None else np.ascontiguousarray(value_weights, dtype=np.float32)
        self._chk(self.lib.ll_hl_policy_set_weights(self.h, w.ctypes.data_as(C.c_void_p), int(w.size), v.ctypes.data_as(C.c_void_p) if v is not None else None,
                                                    int(v.size) if v is not None else 0, _vp(stream)))

    def act_ptr(self, d_obs, d_actions, n_rows, stream=None, d_reset=None, d_code=None, d_heading=None, obs_stride=None):
        """ll_hl_policy_act on raw device addresses; asynchronous on `stream` (None: the default stream)."""
        self._chk(self.lib.ll_hl_policy_act(self.h, _vp(d_obs), int(OBS_DIM[self.KIND] if obs_stride is None else obs_stride), _vp(d_reset), _vp(d_actions),
                                            _vp(d_code), _vp(d_heading), int(n_rows), _vp(stream)))

    def act(self, engine, reset_from_done=True, d_code=None, d_heading=None):
        """obs buffer of `engine` (an EpmcEngine / SepmcEngine, or a game holding one as .engine) -> its action buffer, queued on the engine's
        stream.  reset_from_done: rows whose done flag is set (an auto-reset engine re-seeded them in the last step) start from zero state."""
        eng = getattr(engine, 'engine', engine)
        p = eng.device_ptrs()
        self.act_ptr(p.obs, p.actions, p.n_envs, p.stream, p.done if reset_from_done else None, d_code, d_heading, p.obs_dim)

    def act_pg_ptr(self, d_obs, d_actions, n_rows, seed, step, sample=True, stream=None, d_reset=None, d_code=None, d_heading=None, d_neglogp=None,
                   d_value=None, obs_stride=None):
        """ll_hl_policy_act_pg on raw device addresses; asynchronous on `stream` (None: the default stream).  d_neglogp [n_rows][n_heads],
        d_value [n_rows] (needs attach_value)."""
        self._chk(self.lib.ll_hl_policy_act_pg(self.h, _vp(d_obs), int(OBS_DIM[self.KIND] if obs_stride is None else obs_stride), _vp(d_reset),
                                               _vp(d_actions), _vp(d_code), _vp(d_heading), _vp(d_neglogp), _vp(d_value), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                               int(step) & 0xFFFFFFFFFFFFFFFF, 1 if sample else 0, int(n_rows), _vp(stream)))

    def act_pg(self, engine, seed, step, sample=True, d_neglogp=None, d_value=None, reset_from_done=True, d_code=None, d_heading=None):
        """The PPO actor's step on `engine`'s buffers, queued on its stream: sampled (or, sample=False, modal) heads into the engine's action
        buffer, neglogp / value into the given device buffers; reset_from_done as in act (the value state of those rows starts from zero too)."""
        eng = getattr(engine, 'engine', engine)
        p = eng.device_ptrs()
        self.act_pg_ptr(p.obs, p.actions, p.n_envs, seed, step, sample, p.stream, p.done if reset_from_done else None, d_code, d_heading, d_neglogp,
                        d_value, p.obs_dim)

    def value_state(self):
        """[max_rows][64] float32: c | h of the value LSTM"""
        s = np.empty((self.max_rows, VALUE_STATE_DIM), np.float32)
        self._chk(self.lib.ll_hl_policy_get_value_state(self.h, s.ctypes.data_as(C.c_void_p)))
        return s

    def set_value_state(self, s):
        s = np.ascontiguousarray(s, dtype=np.float32).reshape(self.max_rows, VALUE_STATE_DIM)
        self._chk(self.lib.ll_hl_policy_set_value_state(self.h, s.ctypes.data_as(C.c_void_p)))

    def hs(self):
        """The recurrent state in the reference network's S layout, [max_rows][192] (EPMC: vf c|h, pi, z c|h) or [max_rows][256] (SEPMC: vf, pi,
        z, hlc), each LSTM's 64 values c | h; pi is zeros (llc_light has no LSTM), vf zeros without a value branch."""
        st = self.state()
        vf = self.value_state() if self.has_value else np.zeros((self.max_rows, VALUE_STATE_DIM), np.float32)
        pi = np.zeros((self.max_rows, VALUE_STATE_DIM), np.float32)
        if self.KIND == LLH_EPMC:
            return np.concatenate([vf, pi, st], axis=1)
        return np.concatenate([vf, pi, st[:, 64:128], st[:, 0:64]], axis=1)

    def reset_state(self, stream=None):
        self._chk(self.lib.ll_hl_policy_reset_state(self.h, _vp(stream)))

    def state(self):
        """[max_rows][state_dim] float32 (EPMC: c | h; SEPMC: hlc c | hlc h | z c | z h)"""
        s = np.empty((self.max_rows, self.state_dim), np.float32)
        self._chk(self.lib.ll_hl_policy_get_state(self.h, s.ctypes.data_as(C.c_void_p)))
        return s

    def set_state(self, s):
        s = np.ascontiguousarray(s, dtype=np.float32).reshape(self.max_rows, self.state_dim)
        self._chk(self.lib.ll_hl_policy_set_state(self.h, s.ctypes.data_as(C.c_void_p)))

    def enable_timing(self, on=True):
        self._chk(self.lib.ll_hl_policy_enable_timing(self.h, 1 if on else 0))

    def time_ms(self):
        """(average ms per ll_hl_policy_act / ll_hl_policy_act_pg launch since the last call, number of launches)"""
        ms, n = C.c_double(0), C.c_int(0)
        self._chk(self.lib.ll_hl_policy_time_ms(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value


class HipEpmcPolicy(_HipHlPolicy):
    """A trained environmental-level policy (tests/golden/epmc_policy_{hurdle,hole,cube}.npz layout); rows = the EPMC engine's envs."""
    KIND = LLH_EPMC


class HipSepmcPolicy(_HipHlPolicy):
    """The trained strategic-level policy (tests/golden/sepmc_policy.npz layout); rows = 2 arena + robot, the SEPMC engine's row order.
    d_heading (act / act_ptr) receives the high level's heading angle of every row."""
    KIND = LLH_SEPMC
