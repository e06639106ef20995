from .engine import EngineStats, SweepEngine  # noqa: F401
from .fastpath import (  # noqa: F401
    HOLD_IDLE,
    HOLD_INVALID,
    HOLD_NOT_HELD,
    HOLD_OK,
    HOLD_OVERLOADED,
    HOLD_SLO_VIOLATED,
    HOLD_STATUS_NAMES,
    ROLLOUT_MAX_STEPS,
    FastSweep,
    HoldResult,
    PlanResult,
    RolloutResult,
    SloPlanResult,
    TokenPlanResult,
    WinnerRecord,
    feed_back,
)
from .snapshot import CellSnapshot, build_cell_snapshot, compute_batch_size  # noqa: F401
