"""kubernetesclustercapacity_amd — MI355X-native engine for the hot path of
AshutoshNirkhe/KubernetesClusterCapacity (per-node request sums + nodes x specs fit).

The compute lives in libkcc.so (hand-written gfx950 HIP kernels behind the C-ABI of
include/kcc.h).  Importing this package does not touch the GPU; constructing a
CapacityEngine loads libkcc.so and fails loudly if it is missing.
"""
from ._lib import KCC_EXT_MAX  # noqa: F401  (extra resources of CapacityEngine.fit_ext)
from ._lib import KCC_DEPLOY_PACK, KCC_DEPLOY_SPREAD  # noqa: F401  (CapacityEngine.deploy)
from ._lib import KCC_DRAIN_MAX_SHAPES  # noqa: F401  (CapacityEngine.drain)
from ._lib import (KCC_CAND_BADROW, KCC_CAND_OK, KCC_CAND_TOOMANY,  # noqa: F401
                   KCC_CONS_MAX_PODS)  # (CapacityEngine.consolidate)
from ._lib import (KCC_WHY_CAP, KCC_WHY_CPU, KCC_WHY_EXT0, KCC_WHY_MEM,  # noqa: F401
                   KCC_WHY_PODS, KCC_WHY_SLOTS)  # (CapacityEngine.fit_explain)
from .engine import (CapacityEngine, ConsolidateResult, DeployResult, DrainResult,  # noqa: F401
                     ExplainResult, KccError, RequestSums, explain_groups, select_groups, verdict)
from .shard import node_range, shard_bounds  # noqa: F401

__all__ = ["CapacityEngine", "KccError", "RequestSums", "DeployResult", "DrainResult",
           "ConsolidateResult", "ExplainResult", "verdict", "select_groups", "explain_groups", "node_range",
           "shard_bounds", "KCC_EXT_MAX", "KCC_DEPLOY_PACK", "KCC_DEPLOY_SPREAD",
           "KCC_DRAIN_MAX_SHAPES", "KCC_CONS_MAX_PODS", "KCC_CAND_OK", "KCC_CAND_BADROW",
           "KCC_CAND_TOOMANY", "KCC_WHY_SLOTS", "KCC_WHY_CPU", "KCC_WHY_MEM", "KCC_WHY_EXT0",
           "KCC_WHY_PODS", "KCC_WHY_CAP"]
