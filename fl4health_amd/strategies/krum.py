"""Krum / Multi-Krum (Blanchard et al. 2017; flwr's Krum).

Each client is scored by the sum of its K-f-2 smallest squared distances to
the other clients. num_clients_to_keep = 0 is classic Krum: the lowest-scoring
client's parameters are returned bitwise. m > 0 is Multi-Krum: the m lowest
scores (one shot) are averaged through aggregate_results, unweighted by
default because a hostile client can lie about num_examples.

Plain parameter payloads only; no collective fast path (see fed_median.py).
"""
from __future__ import annotations

from fl4health_amd.client_managers.base import ClientProxy
from fl4health_amd.common import FitRes, Parameters, Scalar
from fl4health_amd.strategies.aggregate_utils import (
    aggregate_results,
    decode_and_robust_sort_results,
    krum_select,
)
from fl4health_amd.strategies.basic_fedavg import BasicFedAvg


class Krum(BasicFedAvg):
    def __init__(
        self,
        *,
        num_malicious_clients: int,
        num_clients_to_keep: int = 0,
        weighted_aggregation: bool = False,
        **fedavg_kwargs,
    ) -> None:
        if num_malicious_clients < 0 or num_clients_to_keep < 0:
            raise ValueError("num_malicious_clients and num_clients_to_keep must be >= 0")
        super().__init__(weighted_aggregation=weighted_aggregation, **fedavg_kwargs)
        self.num_malicious_clients = num_malicious_clients
        self.num_clients_to_keep = num_clients_to_keep

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
        payloads = [(p, n) for _, p, n in sorted_results]
        selected = krum_select(payloads, self.num_malicious_clients, self.num_clients_to_keep)
        if self.num_clients_to_keep == 0:
            winner = payloads[selected[0]][0]
            params = Parameters([t.clone() for t in winner.tensors], dict(winner.meta))
        else:
            # averaged in the pinned result order, not in score order
            params = aggregate_results([payloads[i] for i in sorted(selected)], self.weighted_aggregation)
        metrics = self.fit_metrics_aggregation_fn([(res.num_examples, res.metrics) for _, res in results])
        metrics = dict(metrics)
        metrics["krum_selected"] = ",".join(str(getattr(sorted_results[i][0], "cid", "")) for i in selected)
        return params, metrics

    def supports_collective_aggregation(self) -> bool:
        return False
