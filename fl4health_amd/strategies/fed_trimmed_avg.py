"""FedTrimmedAvg: coordinate-wise beta-trimmed mean (Yin et al. 2018; flwr's
FedTrimmedAvg). Per coordinate the b = int(beta*K) smallest and b largest
client values are dropped (NaN counts as largest) and the rest averaged, so up
to b arbitrary clients cannot move a coordinate outside the honest range.

Plain parameter payloads only; no collective fast path (see fed_median.py).
"""
from __future__ import annotations

from fl4health_amd.client_managers.base import ClientProxy
from fl4health_amd.common import FitRes, Parameters, Scalar
from fl4health_amd.strategies.aggregate_utils import aggregate_trimmed_mean, decode_and_robust_sort_results
from fl4health_amd.strategies.basic_fedavg import BasicFedAvg


class FedTrimmedAvg(BasicFedAvg):
    def __init__(self, *, beta: float = 0.2, **fedavg_kwargs) -> None:
        if not (0.0 <= beta < 0.5):
            raise ValueError(f"beta must be in [0, 0.5), got {beta}")
        super().__init__(**fedavg_kwargs)
        self.beta = beta

    def aggregate_fit(
        self,
        server_round: int,
        results: list[tuple[ClientProxy, FitRes]],
        failures: list[tuple[ClientProxy, FitRes] | BaseException],
    ) -> tuple[Parameters | None, dict[str, Scalar]]:
        if not results:
            return None, {}
        if not self.accept_failures and failures:
            return None, {}
        sorted_results = decode_and_robust_sort_results(results)
        params = aggregate_trimmed_mean([(p, n) for _, p, n in sorted_results], self.beta)
        metrics = self.fit_metrics_aggregation_fn([(res.num_examples, res.metrics) for _, res in results])
        return params, metrics

    def supports_collective_aggregation(self) -> bool:
        return False
