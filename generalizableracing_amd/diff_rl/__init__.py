"""The diff_rl workflow: BPTT through the analytic step (the reference's standalone/diff_rl)."""
from .bptt import BPTT  # noqa: F401
from .config import QuadcopterDiffRLRunnerCfg  # noqa: F401
from .model import BaseModel  # noqa: F401
from .runner import AlgoRunner  # noqa: F401
