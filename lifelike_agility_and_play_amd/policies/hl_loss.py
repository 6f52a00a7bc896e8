"""ctypes binding of include/hl/llenv_hl_loss.h: the PPO loss of a scored unroll block (policies.hl_score rows of a policies.hl_unroll block), its
statistics and its gradient with respect to the scorer's eight output columns, on the device, in float64, in three launches (ppo) or four (ppo2).

    rec.steps(seed, 129) ; rec.finish(0)
    out = score(learner, rec, 0)
    stats, grad = ppo_loss(out, rec, 0)          # stats: float64 device tensor [LLL_N_STATS]; grad [n_rows][128][8] float32, dloss / d out
    torch.cuda.synchronize()
    named(stats)['pg_loss'], split_out(grad)['neglogp']
"""
import ctypes as C

from .. import capi
from . import hl_league as G
from . import hl_score as SC
from . import hl_unroll as U

LLL_PPO, LLL_PPO2 = 0, 1
# name -> (first index, width) into d_stats: LLL_W .. LLL_EXPLAINED_VARIANCE
STATS = {'W': (0, 1), 'n_excluded_weight': (1, 1), 'n_excluded_nonfinite': (2, 1), 'adv_mean': (3, 1), 'adv_std': (4, 1), 'pg_loss': (5, 1),
         'value_loss': (6, 1), 'loss': (7, 1), 'entropy': (8, 3), 'approx_kl': (11, 3), 'clip_frac': (14, 3), 'return_mean': (17, 1), 'value_mean': (18, 1),
         'explained_variance': (19, 1)}
LLL_N_STATS = 20


class LossConfig(C.Structure):   # struct ll_hl_loss_config_t
    _fields_ = [('mode', C.c_int32), ('merge_heads', C.c_int32), ('adv_normalize', C.c_int32), ('reserved', C.c_int32), ('clip_range', C.c_float),
                ('clip_range_lower', C.c_float), ('vf_clip', C.c_float), ('vf_coef', C.c_float), ('ent_coef', C.c_float), ('gamma', C.c_float),
                ('lam', C.c_float), ('adv_eps', C.c_float)]


_P = C.c_void_p
_SIGS = {
    'll_hl_loss_default_config': (C.c_int, [C.POINTER(LossConfig)]),
    'll_hl_loss_workspace_bytes': (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_uint64)]),
    'll_hl_loss_rows': (C.c_int, [C.c_int, C.POINTER(LossConfig), _P, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.c_uint64, _P]),
    'll_hl_loss_unroll': (C.c_int, [_P, C.c_int, C.POINTER(LossConfig), _P, _P, _P, _P, _P, C.c_uint64]),
    'll_hl_loss_league': (C.c_int, [_P, C.c_int, C.POINTER(LossConfig), _P, _P, _P, _P, _P, C.c_uint64]),
}
EXPORTED_SYMBOLS = sorted(_SIGS)


def load_library(path=None):
    return capi.bind(SC.load_library(path), _SIGS)


def _chk(lib, rc):
    if rc != 0:
        raise capi.LLError(rc, lib.ll_last_error().decode())


def default_config(lib=None, **changes):
    """ll_hl_loss_default_config (ppo, merged heads, normalised advantages, clip 0.2, vf_coef 1, ent_coef 0, gamma = lam = 0.95), with `changes` set."""
    lib = lib or load_library()
    cfg = LossConfig()
    _chk(lib, lib.ll_hl_loss_default_config(C.byref(cfg)))
    for k, v in changes.items():
        if k not in dict(LossConfig._fields_):
            raise AttributeError('ll_hl_loss_config_t has no field %r' % k)
        setattr(cfg, k, v)
    return cfg


def workspace_bytes(n_rows, L, lib=None):
    lib = lib or load_library()
    out = C.c_uint64(0)
    _chk(lib, lib.ll_hl_loss_workspace_bytes(int(n_rows), int(L), C.byref(out)))
    return out.value


def named(stats):
    """{name: float, or a list of three for the per-head entries} of a stats tensor or array; call after synchronising with the stream of the call."""
    v = [float(x) for x in (stats.tolist() if hasattr(stats, 'tolist') else stats)]
    if len(v) != LLL_N_STATS:
        raise ValueError('%d values are not the %d statistics of a loss call' % (len(v), LLL_N_STATS))
    return {name: (v[i] if d == 1 else v[i:i + d]) for name, (i, d) in STATS.items()}


def _ptr(x):
    return C.c_void_p(int(x)) if x else None


def loss_rows(kind, cfg, d_rows, n_rows, L, d_score, d_weight, d_grad, d_stats, d_work, work_bytes, stream=None, lib=None):
    """ll_hl_loss_rows on raw device addresses (d_weight: 0 / None for all ones); asynchronous on `stream` (None: the default stream)."""
    lib = lib or load_library()
    _chk(lib, lib.ll_hl_loss_rows(int(kind), C.byref(cfg) if cfg is not None else None, _ptr(d_rows), int(n_rows), int(L), _ptr(d_score), _ptr(d_weight),
                                  _ptr(d_grad), _ptr(d_stats), _ptr(d_work), int(work_bytes), _ptr(stream)))


def _source(src):
    if isinstance(src, U.HlUnrollRecorder):
        return 'll_hl_loss_unroll'
    if isinstance(src, G.HlLeagueActor):
        return 'll_hl_loss_league'
    raise TypeError('the loss takes an HlUnrollRecorder or an HlLeagueActor, not %r' % type(src).__name__)


def loss_block(recorder_or_league, buffer, cfg, d_score, d_weight, d_grad, d_stats, d_work, work_bytes):
    """ll_hl_loss_unroll / ll_hl_loss_league on raw device addresses (d_weight: 0 / None for all ones), queued on the engine's stream; nothing is allocated."""
    src = recorder_or_league
    name = _source(src)
    lib = capi.bind(src.lib, _SIGS)
    _chk(lib, getattr(lib, name)(src.h, int(buffer), C.byref(cfg) if cfg is not None else None, _ptr(d_score), _ptr(d_weight), _ptr(d_grad), _ptr(d_stats),
                                 _ptr(d_work), int(work_bytes)))


def ppo_loss(score_out, recorder_or_league, buffer, cfg=None, weight=None, grad=None):
    """The loss of block `buffer` of an HlUnrollRecorder or an HlLeagueActor under its scored rows `score_out` (hl_score.score), queued on the engine's
    stream.  weight: float32 device tensor [n_rows][unroll_length] or None.  Returns (stats, grad): stats a float64 device tensor [LLL_N_STATS] (named()
    after synchronising), grad [n_rows][unroll_length][8] float32 (the one passed, or a new one) carrying ll_kind, so hl_score.split_out(grad) names its
    columns.  In ppo mode R is read as it stands: finish() the block first.  LLError LL_ESTATE while the block holds no complete unroll."""
    import torch
    src = recorder_or_league
    _source(src)
    lib = capi.bind(src.lib, _SIGS)
    shape = (src.n_rows, src.unroll_length, SC.LLS_OUT_FLOATS)

    def want(t, what, shp, dtype=torch.float32):
        if tuple(t.shape) != shp or t.dtype != dtype or not t.is_contiguous() or not t.is_cuda:
            raise ValueError('%s must be a contiguous %s device tensor of shape %s' % (what, str(dtype).split('.')[-1], shp))
    want(score_out, 'score_out', shape)
    if weight is not None:
        want(weight, 'weight', shape[:2])
    if grad is not None:
        want(grad, 'grad', shape)
    if cfg is None:
        cfg = default_config(lib)
    nbytes = workspace_bytes(src.n_rows, src.unroll_length, lib)
    if grad is None:
        grad = torch.empty(shape, dtype=torch.float32, device='cuda')
    stats = torch.empty(LLL_N_STATS, dtype=torch.float64, device='cuda')
    work = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device='cuda')
    torch.cuda.current_stream().synchronize()                # (the allocations are torch's; the launches run on the engine's stream)
    loss_block(src, buffer, cfg, score_out.data_ptr(), weight.data_ptr() if weight is not None else None, grad.data_ptr(), stats.data_ptr(), work.data_ptr(), nbytes)
    grad.ll_kind = src.kind
    stats.ll_work = work                                     # the workspace lives as long as the result: the launches are still reading it
    return stats, grad
