"""ctypes binding of include/hl/llenv_hl_score.h: recorded EPMC / SEPMC unroll blocks (policies.hl_unroll rows) scored under any weights on the
device -- the neglogp of the RECORDED action of every head, every head's entropy and the value prediction of every time step, the LSTMs starting
from the S of the unroll's first frame and re-zeroed where M says so.  One kernel launch per block.  The weights are those of an ordinary
HipEpmcPolicy / HipSepmcPolicy with a value branch (renew them with set_weights); its own recurrent state and max_rows play no part.

    rec.steps(seed, 129) ; rec.finish(0)
    learner = HipEpmcPolicy('new_model.npz', max_rows=1, value_npz='new_value.npz')      # the weight carrier
    f = split_out(score(learner, rec, 0))       # torch views [n_rows][128][..]: f['neglogp'], f['entropy'], f['V']
"""
import ctypes as C

from .. import capi
from . import hl_league as G
from . import hl_policy_hip as H
from . import hl_unroll as U

LLS_OUT_FLOATS = 8
LLS_FIELDS = ('neglogp', 'entropy', 'V', 'pad')      # LLS_NEGLOGP .. LLS_PAD


class LLHlScoreLayout(C.Structure):   # struct ll_hl_score_layout_t
    _fields_ = [('kind', C.c_int32), ('n_heads', C.c_int32), ('out_floats', C.c_int32), ('reserved', C.c_int32),
                ('off', C.c_int32 * len(LLS_FIELDS)), ('dim', C.c_int32 * len(LLS_FIELDS))]


_SIGS = {
    'll_hl_score_layout': (C.c_int, [C.c_int, C.POINTER(LLHlScoreLayout)]),
    'll_hl_score_rows': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'll_hl_score_unroll': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    'll_hl_score_league': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
}
EXPORTED_SYMBOLS = sorted(_SIGS)


def load_library(path=None):
    return capi.bind(G.load_library(path), _SIGS)


def out_layout(kind):
    """{field: (first column, width)} of an output row, restated from the header (ll_hl_score_layout reports the same): neglogp and entropy of
    every head in action-space order (EPMC z, llc; SEPMC hlc, z, llc), V, zero pad up to LLS_OUT_FLOATS."""
    nh = H.N_HEADS[kind]
    return {'neglogp': (0, nh), 'entropy': (nh, nh), 'V': (2 * nh, 1), 'pad': (2 * nh + 1, LLS_OUT_FLOATS - 2 * nh - 1)}


def split_out(array, kind=None):
    """Named views of scored rows [..., 8] (NumPy array or torch tensor): neglogp, entropy and pad keep their last axis, V loses it.  kind:
    LLH_EPMC / LLH_SEPMC; None takes the kind a tensor returned by score() carries."""
    if kind is None:
        kind = getattr(array, 'll_kind', None)
        if kind is None:
            raise ValueError('split_out needs the kind of the rows (LLH_EPMC or LLH_SEPMC)')
    if array.shape[-1] != LLS_OUT_FLOATS:
        raise ValueError('rows of %d columns are not scored rows (%d columns)' % (array.shape[-1], LLS_OUT_FLOATS))
    return {name: (array[..., off] if name == 'V' else array[..., off:off + d]) for name, (off, d) in out_layout(kind).items()}


def _chk(lib, rc):
    if rc != 0:
        raise capi.LLError(rc, lib.ll_last_error().decode())


def score_rows(policy, d_rows, n_rows, L, d_out, stream=None):
    """ll_hl_score_rows on raw device addresses: d_rows [n_rows][L][row_floats of the policy's kind] -> d_out [n_rows][L][8]; asynchronous on
    `stream` (None: the default stream)."""
    lib = capi.bind(policy.lib, _SIGS)
    _chk(lib, lib.ll_hl_score_rows(policy.h, C.c_void_p(int(d_rows)) if d_rows else None, int(n_rows), int(L), C.c_void_p(int(d_out)) if d_out else None,
                                   C.c_void_p(int(stream)) if stream else None))


def score(policy, recorder_or_league, buffer, d_out=None):
    """Block `buffer` of an HlUnrollRecorder or an HlLeagueActor scored under `policy`'s weights, queued on the engine's stream behind the steps
    that filled it.  Returns the torch tensor [n_rows][unroll_length][8] (d_out, or a new one): synchronise with the engine's stream before
    reading it.  LLError LL_ESTATE while the block holds no complete unroll."""
    import torch
    src = recorder_or_league
    if isinstance(src, U.HlUnrollRecorder):
        name = 'll_hl_score_unroll'
    elif isinstance(src, G.HlLeagueActor):
        name = 'll_hl_score_league'
    else:
        raise TypeError('score() takes an HlUnrollRecorder or an HlLeagueActor, not %r' % type(src).__name__)
    shape = (src.n_rows, src.unroll_length, LLS_OUT_FLOATS)
    if d_out is None:
        d_out = torch.empty(shape, dtype=torch.float32, device='cuda')
        torch.cuda.current_stream().synchronize()            # (the allocation is torch's; the launch runs on the engine's stream)
    elif tuple(d_out.shape) != shape or d_out.dtype != torch.float32 or not d_out.is_contiguous() or not d_out.is_cuda:
        raise ValueError('d_out must be a contiguous float32 device tensor of shape %s' % (shape,))
    lib = capi.bind(policy.lib, _SIGS)
    _chk(lib, getattr(lib, name)(policy.h, src.h, int(buffer), C.c_void_p(d_out.data_ptr())))
    d_out.ll_kind = src.kind
    return d_out
