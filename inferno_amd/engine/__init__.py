from .engine import EngineStats, SweepEngine  # noqa: F401
from .fastpath import (  # noqa: F401
    ROLLOUT_MAX_STEPS,
    FastSweep,
    PlanResult,
    RolloutResult,
    SloPlanResult,
    TokenPlanResult,
    WinnerRecord,
    feed_back,
)
from .snapshot import CellSnapshot, build_cell_snapshot, compute_batch_size  # noqa: F401
