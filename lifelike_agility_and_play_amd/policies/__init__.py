"""On-device policies of the environmental (EPMC) and strategic (SEPMC) levels: hl_policy_hip binds include/hl/llenv_hl_policy.h,
hl_unroll binds include/hl/llenv_hl_unroll.h (the actor loop recorded as learner-ready unrolls)."""
from .hl_policy_hip import HipEpmcPolicy, HipSepmcPolicy, pack_value_weights, pack_weights  # noqa: F401
from .hl_unroll import HlUnrollRecorder, split_row  # noqa: F401

__all__ = ['HipEpmcPolicy', 'HipSepmcPolicy', 'HlUnrollRecorder', 'pack_value_weights', 'pack_weights', 'split_row']
