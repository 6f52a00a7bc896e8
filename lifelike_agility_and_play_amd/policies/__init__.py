"""On-device policies of the environmental (EPMC) and strategic (SEPMC) levels: hl_policy_hip binds include/hl/llenv_hl_policy.h."""
from .hl_policy_hip import HipEpmcPolicy, HipSepmcPolicy, pack_value_weights, pack_weights  # noqa: F401

__all__ = ['HipEpmcPolicy', 'HipSepmcPolicy', 'pack_value_weights', 'pack_weights']
