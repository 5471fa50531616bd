"""Server-side aggregation reductions (reference fl4health/strategies/aggregate_utils.py:8-55
and utils/functions.py:63-108 pseudo-sorted determinism).

Torch-native: payloads are lists of flat fp32 tensors; the weighted reduce is
one fused kernel over a stacked [K, n] buffer per tensor slot (K clients) —
deterministic fixed-order summation (pseudo-sort analogue) instead of the
reference's per-layer NumPy loop.
"""
from __future__ import annotations

import logging
import math

import torch

from fl4health_amd.common import FitRes, Parameters
from fl4health_amd.ops import functional as F

log = logging.getLogger(__name__)


def pseudo_sort_key(cid: str, num_examples: int, parameters: Parameters) -> tuple:
    """Deterministic ordering key (reference utils/functions.py:63-82): sample
    count + a content signature (sum of zeroeth elements of the floating
    tensors) so that two clients with equal num_examples and unstable cids
    still land in a pinned fp-summation order. The cid is kept as the final
    tiebreak for the (measure-zero) case of identical signatures."""
    sig = 0.0
    for t in parameters.tensors:
        if t.is_floating_point() and t.numel() > 0:
            sig += float(t.reshape(-1)[0])
    return (num_examples + sig, cid)


def decode_and_pseudo_sort_results(
    results: list[tuple[object, FitRes]],
) -> list[tuple[object, Parameters, int]]:
    sortable = [(proxy, res.parameters, res.num_examples) for proxy, res in results]
    return sorted(
        sortable, key=lambda t: pseudo_sort_key(str(getattr(t[0], "cid", "")), t[2], t[1])
    )


def aggregate_results(results: list[tuple[Parameters, int]], weighted: bool = True) -> Parameters:
    """Weighted (sum n_i w_i / sum n_i) or unweighted (mean) average, per tensor slot."""
    assert results, "no results to aggregate"
    n_slots = len(results[0][0].tensors)
    total_examples = sum(n for _, n in results)
    k = len(results)
    if weighted:
        ws = torch.tensor([n / total_examples for _, n in results], dtype=torch.float32)
    else:
        ws = torch.full((k,), 1.0 / k, dtype=torch.float32)
    out_tensors = []
    for slot in range(n_slots):
        stack = torch.stack([p.tensors[slot] for p, _ in results])  # [K, ...]
        w = ws.to(stack.device)
        flat = stack.reshape(k, -1)
        out = F.weighted_sum_rows(flat.contiguous(), w).view(stack.shape[1:])
        out_tensors.append(out)
    meta = dict(results[0][0].meta)
    return Parameters(out_tensors, meta)


def aggregate_losses(results: list[tuple[int, float]], weighted: bool = True) -> float:
    """Aggregate client losses (reference aggregate_utils.py:35-55)."""
    if weighted:
        total = sum(n for n, _ in results)
        return sum(n * loss for n, loss in results) / total
    return sum(loss for _, loss in results) / len(results)


# ---- Byzantine-robust reductions -------------------------------------------
# A weighted mean lets one client that sends 1e6 or a NaN own the result. The
# reductions below bound a minority's influence: coordinate-wise order
# statistics (median, trimmed mean) and distance-based selection ((Multi-)Krum,
# Blanchard et al. 2017). They take the same [(Parameters, num_examples)] lists
# as aggregate_results and work per tensor slot.


def robust_sort_key(cid: str, num_examples: int, parameters: Parameters) -> tuple:
    """pseudo_sort_key for payloads that may hold NaN/Inf: a non-finite
    signature would make Python's sort inconsistent, so it maps to +inf and
    the cid decides among such clients."""
    key = pseudo_sort_key(cid, num_examples, parameters)[0]
    return (key if math.isfinite(key) else math.inf, cid)


def decode_and_robust_sort_results(
    results: list[tuple[object, FitRes]],
) -> list[tuple[object, Parameters, int]]:
    sortable = [(proxy, res.parameters, res.num_examples) for proxy, res in results]
    return sorted(
        sortable, key=lambda t: robust_sort_key(str(getattr(t[0], "cid", "")), t[2], t[1])
    )


def _rank_mean_per_slot(results: list[tuple[Parameters, int]], lo: int, hi: int) -> Parameters:
    out_tensors = []
    for slot in range(len(results[0][0].tensors)):
        first = results[0][0].tensors[slot]
        rows = [p.tensors[slot].reshape(-1).float() for p, _ in results]
        out = F.rank_mean_rows(rows, lo, hi)
        out_tensors.append(out.view(first.shape).to(first.dtype))
    return Parameters(out_tensors, dict(results[0][0].meta))


def aggregate_median(results: list[tuple[Parameters, int]]) -> Parameters:
    """Coordinate-wise median; for even K the mean of the two middle values."""
    assert results, "no results to aggregate"
    k = len(results)
    if k == 1:
        return Parameters([t.clone() for t in results[0][0].tensors], dict(results[0][0].meta))
    lo = k // 2 if k % 2 == 1 else k // 2 - 1
    return _rank_mean_per_slot(results, lo, k // 2 + 1)


def aggregate_trimmed_mean(results: list[tuple[Parameters, int]], beta: float) -> Parameters:
    """Coordinate-wise mean after dropping the b = int(beta*K) smallest and
    the b largest values (NaN counts as largest)."""
    assert results, "no results to aggregate"
    k = len(results)
    if not (0.0 <= beta < 0.5):
        raise ValueError(f"beta must be in [0, 0.5), got {beta}")
    b = int(beta * k)
    if k - 2 * b < 1:
        raise ValueError(f"trimming {b} from each side of {k} clients leaves nothing")
    if k == 1:
        return Parameters([t.clone() for t in results[0][0].tensors], dict(results[0][0].meta))
    return _rank_mean_per_slot(results, b, k - b)


def krum_scores(results: list[tuple[Parameters, int]], num_malicious: int) -> torch.Tensor:
    """score(i) = sum of the K-f-2 smallest squared distances from client i to
    the OTHER clients, distances summed over all tensor slots. A NaN distance
    counts as +inf. Returns an fp64 [K] tensor on the payload's device."""
    assert results, "no results to aggregate"
    k = len(results)
    n_near = k - num_malicious - 2
    if num_malicious < 0 or n_near < 1:
        raise ValueError(f"Krum needs K - f - 2 >= 1, got K={k} f={num_malicious}")
    if k < 2 * num_malicious + 3:
        log.warning("Krum: K=%d < 2f+3=%d, the robustness guarantee does not hold", k, 2 * num_malicious + 3)
    dist = None
    for slot in range(len(results[0][0].tensors)):
        rows = [p.tensors[slot].reshape(-1).float() for p, _ in results]
        d = F.pairwise_sqdist_rows(rows)
        dist = d if dist is None else dist + d
    inf = torch.full_like(dist, math.inf)
    dist = torch.where(torch.isnan(dist), inf, dist)
    dist = torch.where(torch.eye(k, dtype=torch.bool, device=dist.device), inf, dist)
    return torch.sort(dist, dim=1).values[:, :n_near].sum(dim=1)


def krum_select(results: list[tuple[Parameters, int]], num_malicious: int, num_to_keep: int) -> list[int]:
    """Indices of the max(num_to_keep, 1) lowest Krum scores, selected in one
    shot (Multi-Krum as in flwr, not the iterative variant); ties go to the
    lower index."""
    scores = krum_scores(results, num_malicious).tolist()  # the one host sync
    m = min(max(num_to_keep, 1), len(scores))
    return sorted(range(len(scores)), key=lambda i: (scores[i], i))[:m]
