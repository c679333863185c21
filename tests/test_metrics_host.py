"""torecsys_amd.metrics against a brute-force loop over hand-sized rank tensors: -1 entries, a sample without any held-out
target, k larger than every rank."""
import math

import pytest
import torch

RANKS = [[[0]], [[3], [-1], [0]], [[2, 0, 5], [7, -1, 1], [-1, -1, -1], [40, 9, 10]], [[0, 1, 2, 3]], [[6, 6], [1, -1]]]


def brute(ranks, k):
    hr, ndcg, mrr, ap = [], [], [], []
    for row in ranks:
        live = sorted(r for r in row if r >= 0)
        if not live:
            continue
        hits = [r for r in live if r < k]
        hr.append(1.0 if hits else 0.0)
        ndcg.append(sum(1 / math.log2(r + 2) for r in hits) / sum(1 / math.log2(i + 2) for i in range(min(len(live), k))))
        mrr.append(1 / (live[0] + 1))
        ap.append(sum(sum(1 for o in live if o <= r) / (r + 1) for r in hits) / min(len(live), k))
    return [sum(v) / len(v) for v in (hr, ndcg, mrr, ap)]


@pytest.mark.parametrize("k", [1, 3, 10, 100])
@pytest.mark.parametrize("ranks", RANKS)
def test_metrics_against_loop(ranks, k):
    from torecsys_amd import metrics
    r = torch.tensor(ranks)
    got = [metrics.hit_rate_at_k(r, k), metrics.ndcg_at_k(r, k), metrics.mean_reciprocal_rank(r),
           metrics.mean_average_precision_at_k(r, k)]
    assert [float(g) for g in got] == pytest.approx(brute(ranks, k), abs=1e-12)
