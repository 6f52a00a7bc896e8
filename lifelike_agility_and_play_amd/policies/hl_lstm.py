"""ctypes binding of include/hl/llenv_hl_lstm.h: the layer-normalised LSTM core that the five recurrent networks of the EPMC / SEPMC policies share, with
its linear head -- forward over an unroll and backward through time on the device -- and, on top of it, a torch.autograd.Function.

    w = branch_weights('epmc', 'value', arrays)              # the eleven tensors of a branch out of {number: tensor}
    Y, S_end = ln_lstm(E, S0, M, w, 1)                       # E [n][L][256], S0 [n][64], M [n][L] -> Y [n][L][1], S_end [n][64]
    (Y * dY).sum().backward()                                # E.grad, S0.grad and the eleven weights' .grad

Everything runs on the current torch stream; nothing is synchronised."""
import ctypes as C

from .. import capi
from . import hl_loss as HL

N_IN, N_GATES, N_UNITS, STATE_FLOATS, MAX_OUT, N_WEIGHTS, TAPE_FLOATS = 256, 128, 32, 64, 256, 11, 356
WEIGHT_NAMES = ('wx', 'wh', 'b', 'beta_x', 'gamma_x', 'beta_h', 'gamma_h', 'beta_c', 'gamma_c', 'wo', 'bo')
# (kind, branch) -> (k0: arrays k0 .. k0 + 8 are the cell's, the head's two arrays, D)
BRANCHES = {('epmc', 'z'): (79, (88, 89), 256), ('epmc', 'value'): (36, (45, 46), 1), ('sepmc', 'hlc'): (85, (94, 95), 1),
            ('sepmc', 'z'): (129, (138, 139), 256), ('sepmc', 'value'): (40, (49, 50), 1)}


class LstmWeights(C.Structure):   # struct ll_hl_lstm_weights_t
    _fields_ = [(n, C.c_void_p) for n in WEIGHT_NAMES] + [('n_out', C.c_int32), ('reserved', C.c_int32)]


_P, _U64P = C.c_void_p, C.POINTER(C.c_uint64)
_SIGS = {
    'll_hl_lstm_weight_layout': (C.c_int, [C.c_int, _U64P, _U64P, _U64P]),
    'll_hl_lstm_workspace_bytes': (C.c_int, [C.c_int, C.c_int, C.c_int, _U64P, _U64P]),
    'll_hl_lstm_forward': (C.c_int, [C.POINTER(LstmWeights), _P, _P, C.c_int64, _P, C.c_int64, C.c_int64, C.c_int, C.c_int, _P, C.c_int64, _P, _P, C.c_uint64, _P]),
    'll_hl_lstm_backward': (C.c_int, [C.POINTER(LstmWeights), _P, _P, C.c_int64, C.c_int64, C.c_int, C.c_int, _P, C.c_uint64, _P, C.c_int64, _P, _P, _P, _P, _P,
                                      C.c_uint64, _P]),
}
EXPORTED_SYMBOLS = sorted(_SIGS)


def load_library(path=None):
    return capi.bind(HL.load_library(path), _SIGS)


def _chk(lib, rc):
    if rc != 0:
        raise capi.LLError(rc, lib.ll_last_error().decode())


def _ptr(x):
    return C.c_void_p(int(x)) if x else None


def shapes(n_out):
    """the shapes of the eleven weight arrays, in order"""
    return [(N_IN, N_GATES), (N_UNITS, N_GATES)] + [(N_GATES,)] * 5 + [(N_UNITS,)] * 2 + [(N_UNITS, int(n_out)), (int(n_out),)]


def weight_layout(n_out, lib=None):
    """ll_hl_lstm_weight_layout -> (offsets [11], sizes [11], total) of the packed weight gradient, in floats"""
    lib = lib or load_library()
    off, dim, total = (C.c_uint64 * N_WEIGHTS)(), (C.c_uint64 * N_WEIGHTS)(), C.c_uint64(0)
    _chk(lib, lib.ll_hl_lstm_weight_layout(int(n_out), off, dim, C.byref(total)))
    return list(off), list(dim), total.value


def workspace_bytes(n_rows, L, n_out, lib=None):
    """ll_hl_lstm_workspace_bytes -> (tape_bytes, work_bytes)"""
    lib = lib or load_library()
    tape, work = C.c_uint64(0), C.c_uint64(0)
    _chk(lib, lib.ll_hl_lstm_workspace_bytes(int(n_rows), int(L), int(n_out), C.byref(tape), C.byref(work)))
    return tape.value, work.value


def weights_struct(addresses, n_out):
    """ll_hl_lstm_weights_t of eleven raw device addresses"""
    if len(addresses) != N_WEIGHTS:
        raise ValueError('the core has %d weight arrays, not %d' % (N_WEIGHTS, len(addresses)))
    w = LstmWeights()
    for name, a in zip(WEIGHT_NAMES, addresses):
        setattr(w, name, int(a) if a else None)
    w.n_out, w.reserved = int(n_out), 0
    return w


def forward(w, d_e, d_s0, s0_row_stride, d_m, m_row_stride, m_step_stride, n_rows, L, d_y, y_stride, d_s_end, d_tape, tape_bytes, stream=None, lib=None):
    """ll_hl_lstm_forward on raw device addresses (d_s_end, d_tape: 0 / None to leave out); asynchronous on `stream` (None: the default stream)."""
    lib = lib or load_library()
    _chk(lib, lib.ll_hl_lstm_forward(C.byref(w) if w is not None else None, _ptr(d_e), _ptr(d_s0), int(s0_row_stride), _ptr(d_m), int(m_row_stride),
                                     int(m_step_stride), int(n_rows), int(L), _ptr(d_y), int(y_stride), _ptr(d_s_end), _ptr(d_tape), int(tape_bytes), _ptr(stream)))


def backward(w, d_e, d_m, m_row_stride, m_step_stride, n_rows, L, d_tape, tape_bytes, d_dy, dy_stride, d_ds_end, d_de, d_ds0, d_wgrad, d_work, work_bytes,
             stream=None, lib=None):
    """ll_hl_lstm_backward on raw device addresses (d_ds_end, d_ds0: 0 / None to leave out); asynchronous on `stream`."""
    lib = lib or load_library()
    _chk(lib, lib.ll_hl_lstm_backward(C.byref(w) if w is not None else None, _ptr(d_e), _ptr(d_m), int(m_row_stride), int(m_step_stride), int(n_rows), int(L),
                                      _ptr(d_tape), int(tape_bytes), _ptr(d_dy), int(dy_stride), _ptr(d_ds_end), _ptr(d_de), _ptr(d_ds0), _ptr(d_wgrad),
                                      _ptr(d_work), int(work_bytes), _ptr(stream)))


def branch_weights(kind, branch, arrays):
    """The eleven arrays of a branch -- BRANCHES[(kind, branch)] -- out of a {number: tensor or array} dict, in the order of the struct, each reshaped to
    its shape in shapes(D) (the files hold some vectors as (1, n))."""
    if (kind, branch) not in BRANCHES:
        raise KeyError('no branch %r of kind %r: %s' % (branch, kind, sorted(BRANCHES)))
    k0, head, D = BRANCHES[(kind, branch)]
    picked = [arrays[k0 + i] for i in range(9)] + [arrays[head[0]], arrays[head[1]]]
    return [a.reshape(s) for a, s in zip(picked, shapes(D))]


def _want(t, what, shape):
    import torch
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
        raise ValueError('%s must be a contiguous float32 CUDA tensor of shape %s' % (what, tuple(shape)))


def _function():
    import torch

    class LnLstm(torch.autograd.Function):
        @staticmethod
        def forward(ctx, E, S0, M, n_out, *weights):
            lib = load_library()
            ctx.set_materialize_grads(False)
            n, L = E.shape[:2]
            tape_bytes, work_bytes = workspace_bytes(n, L, n_out, lib)
            Y = torch.empty((n, L, n_out), dtype=torch.float32, device=E.device)
            S_end = torch.empty((n, STATE_FLOATS), dtype=torch.float32, device=E.device)
            tape = torch.empty(tape_bytes // 4, dtype=torch.float32, device=E.device)
            w = weights_struct([t.data_ptr() for t in weights], n_out)
            forward(w, E.data_ptr(), S0.data_ptr(), STATE_FLOATS, M.data_ptr(), L, 1, n, L, Y.data_ptr(), n_out, S_end.data_ptr(), tape.data_ptr(), tape_bytes,
                    torch.cuda.current_stream().cuda_stream, lib)
            ctx.save_for_backward(E, M, tape, *weights)
            ctx.ll = (n, L, n_out, tape_bytes, work_bytes)
            return Y, S_end

        @staticmethod
        def backward(ctx, dY, dS_end):
            lib = load_library()
            n, L, n_out, tape_bytes, work_bytes = ctx.ll
            E, M, tape = ctx.saved_tensors[:3]
            weights = ctx.saved_tensors[3:]
            dY = dY.contiguous().float() if dY is not None else torch.zeros((n, L, n_out), dtype=torch.float32, device=E.device)
            dS_end = dS_end.contiguous().float() if dS_end is not None else None
            off, dim, total = weight_layout(n_out, lib)
            dE = torch.empty_like(E)
            dS0 = torch.empty((n, STATE_FLOATS), dtype=torch.float32, device=E.device)
            wgrad = torch.empty(total, dtype=torch.float32, device=E.device)
            work = torch.empty((work_bytes + 15) // 16 * 4, dtype=torch.float32, device=E.device)
            w = weights_struct([t.data_ptr() for t in weights], n_out)
            backward(w, E.data_ptr(), M.data_ptr(), L, 1, n, L, tape.data_ptr(), tape_bytes, dY.data_ptr(), n_out, dS_end.data_ptr() if dS_end is not None else None,
                     dE.data_ptr(), dS0.data_ptr(), wgrad.data_ptr(), work.data_ptr(), work_bytes, torch.cuda.current_stream().cuda_stream, lib)
            grads = [wgrad[o:o + d].view(s) for o, d, s in zip(off, dim, shapes(n_out))]       # views of the one packed buffer
            return (dE, dS0, None, None) + tuple(grads)

    return LnLstm


_FN = []


def ln_lstm(E, S0, M, weights, n_out):
    """The core over an unroll: E [n][L][256], S0 [n][64] (c | h), M [n][L] (the state is zeroed before step t > 0 where M[:, t] != 0; M[:, 0] is not read),
    weights: the eleven tensors in the order of WEIGHT_NAMES with the shapes of shapes(n_out) -> (Y [n][L][n_out], S_end [n][64]).  Differentiable in E, S0
    and the weights; the weights' gradients are views of one packed buffer.  Runs on the current torch stream without synchronising.  ValueError for a
    tensor that is not a contiguous float32 CUDA tensor of the right shape."""
    n_out = int(n_out)
    if not 1 <= n_out <= MAX_OUT:
        raise ValueError('n_out must lie in 1 .. %d' % MAX_OUT)
    if getattr(E, 'ndim', 0) != 3 or E.shape[0] < 1 or E.shape[1] < 1:
        raise ValueError('E must be a contiguous float32 CUDA tensor of shape (n, L, %d)' % N_IN)
    n, L = E.shape[:2]
    _want(E, 'E', (n, L, N_IN))
    _want(S0, 'S0', (n, STATE_FLOATS))
    _want(M, 'M', (n, L))
    weights = list(weights)
    if len(weights) != N_WEIGHTS:
        raise ValueError('the core has %d weight tensors, not %d' % (N_WEIGHTS, len(weights)))
    for name, t, s in zip(WEIGHT_NAMES, weights, shapes(n_out)):
        _want(t, name, s)
    if not _FN:
        _FN.append(_function())
    return _FN[0].apply(E, S0, M, n_out, *weights)
