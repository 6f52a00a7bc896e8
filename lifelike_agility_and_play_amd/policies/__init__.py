"""On-device policies of the environmental (EPMC) and strategic (SEPMC) levels: hl_policy_hip binds include/hl/llenv_hl_policy.h,
hl_unroll binds include/hl/llenv_hl_unroll.h (the actor loop recorded as learner-ready unrolls), hl_league binds include/hl/llenv_hl_league.h
(the SEPMC actor loop against drawn opponents)."""
from .hl_policy_hip import HipEpmcPolicy, HipSepmcPolicy, pack_value_weights, pack_weights  # noqa: F401
from .hl_league import HlLeagueActor  # noqa: F401
from .hl_unroll import HlUnrollRecorder, split_row  # noqa: F401

__all__ = ['HipEpmcPolicy', 'HipSepmcPolicy', 'HlLeagueActor', 'HlUnrollRecorder', 'pack_value_weights', 'pack_weights', 'split_row']
