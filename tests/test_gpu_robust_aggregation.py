"""GPU: the robust-aggregation HIP kernels (robust_ops.hip) against the CPU
path / an fp64 oracle, and the three strategies on CUDA tensors."""
import pytest
import torch

from fl4health_amd.ops import functional as F
from fl4health_amd.strategies import BasicFedAvg, FedMedian, FedTrimmedAvg, Krum

from tests.test_robust_aggregation import (
    ATTACKS,
    EPS,
    attacked_rows,
    fit_results,
    krum_rows,
    within_honest_range,
)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

NAN, INF = float("nan"), float("inf")


def same_bits(a, b):
    """Equal values, with NaN equal to NaN (and -0.0 equal to +0.0)."""
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(
        torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


def special_rows(k, n, seed):
    """Random rows; columns cycle through: plain, ties (integers in [-3, 3]),
    a NaN, a +inf, a -inf, two NaNs. Which row holds the special value moves."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(k, n, generator=g)
    q = torch.randint(-3, 4, (k, n), generator=g).float()
    col = torch.arange(n)
    kind = col % 6
    x[:, kind == 1] = q[:, kind == 1]
    r1, r2 = col % k, (col // 7 + 1) % k
    for code, val in ((2, NAN), (3, INF), (4, -INF), (5, NAN)):
        m = kind == code
        x[r1[m], col[m]] = val
    m = kind == 5
    x[r2[m], col[m]] = NAN
    return [x[i].clone() for i in range(k)]


def rank_ranges(k):
    med = (k // 2, k // 2 + 1) if k % 2 else (k // 2 - 1, k // 2 + 1)
    out = {med, (0, k)}
    for beta in (0.2, 0.4):
        b = int(beta * k)
        if k - 2 * b >= 1:
            out.add((b, k - b))
    return sorted(out)


def check_rank_mean(cpu_rows, gpu_rows, lo, hi):
    k = len(cpu_rows)
    want = F.rank_mean_rows(cpu_rows, lo, hi)
    got = F.rank_mean_rows(gpu_rows, lo, hi)
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == want.shape
    got = got.cpu()
    if hi - lo <= 2:  # median: a pick, or (a+b)/2 -> exact
        assert same_bits(got, want), (k, lo, hi)
        return
    finite = torch.isfinite(want)
    assert same_bits(got[~finite], want[~finite]), (k, lo, hi)
    bound = k * EPS * torch.nan_to_num(torch.stack(cpu_rows).abs(), nan=0.0).max(dim=0).values
    err = (got[finite].double() - want[finite].double()).abs()
    assert (err <= bound[finite].double()).all(), (k, lo, hi, float(err.max()))


# ---- 7. rank_mean_rows -----------------------------------------------------
@requires_gpu
def test_extension_loaded():
    assert F.HAS_EXT


@requires_gpu
@pytest.mark.parametrize("k", [2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64])
def test_rank_mean_rows_matches_cpu(k):
    for n in (1, 3, 255, 1025, 4099):
        cpu_rows = special_rows(k, n, seed=1000 * k + n)
        gpu_rows = [r.cuda() for r in cpu_rows]
        for lo, hi in rank_ranges(k):
            check_rank_mean(cpu_rows, gpu_rows, lo, hi)


@requires_gpu
@pytest.mark.parametrize("k", [3, 9, 17, 33])
def test_rank_mean_rows_misaligned_views(k):
    """Rows that are buf[1:] views are only 4-byte aligned: scalar path."""
    for n in (1, 255, 4099):
        cpu_rows = special_rows(k, n, seed=77 * k + n)
        bufs = [torch.cat([torch.zeros(1), r]).cuda() for r in cpu_rows]
        gpu_rows = [b[1:] for b in bufs]
        assert all(r.data_ptr() % 16 == 4 for r in gpu_rows)
        for lo, hi in rank_ranges(k):
            check_rank_mean(cpu_rows, gpu_rows, lo, hi)


@requires_gpu
@pytest.mark.parametrize("misaligned", [False, True])
def test_rank_mean_rows_second_grid_stride_trip(misaligned):
    """n = 2^21 + 5 exceeds 8192 blocks x 256 threads on the scalar path (one
    column per thread); the aligned path covers it with four columns per
    thread plus the n % 4 tail."""
    n, k = (1 << 21) + 5, 3
    g = torch.Generator().manual_seed(21)
    cpu_rows = [torch.randn(n, generator=g) for _ in range(k)]
    cpu_rows[1][n - 1] = NAN
    cpu_rows[2][1 << 21] = INF
    if misaligned:
        gpu_rows = [torch.cat([torch.zeros(1), r]).cuda()[1:] for r in cpu_rows]
    else:
        gpu_rows = [r.cuda() for r in cpu_rows]
    check_rank_mean(cpu_rows, gpu_rows, 1, 2)
    check_rank_mean(cpu_rows, gpu_rows, 0, 3)


@requires_gpu
def test_rank_mean_rows_two_runs_bitwise_equal():
    rows = [r.cuda() for r in special_rows(33, 4099, seed=5)]
    a, b = F.rank_mean_rows(rows, 6, 27), F.rank_mean_rows(rows, 6, 27)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 8. pairwise_sqdist_rows -----------------------------------------------
def sqdist_oracle(gpu_rows):
    x = torch.stack(gpu_rows).double()
    return torch.stack([((x - x[i]) ** 2).sum(dim=1) for i in range(x.shape[0])])


def check_sqdist(gpu_rows, rtol=1e-5):
    k = len(gpu_rows)
    d = F.pairwise_sqdist_rows(gpu_rows)
    assert d.is_cuda and d.dtype == torch.float64 and d.shape == (k, k)
    want = sqdist_oracle(gpu_rows)
    assert torch.equal(d, d.t()), "not exactly symmetric"
    assert (d.diagonal() == 0).all(), "diagonal not exactly zero"
    err = (d - want).abs()
    assert (err <= rtol * want).all(), float((err / want.clamp_min(1e-300)).max())
    return d


@requires_gpu
@pytest.mark.parametrize("k", [2, 3, 15, 16, 17, 33, 64])
def test_pairwise_sqdist_matches_fp64_oracle(k):
    g = torch.Generator().manual_seed(k)
    for n in (1, 63, 1000, 300001):
        rows = [torch.randn(n, generator=g).cuda() for _ in range(k)]
        check_sqdist(rows)


@requires_gpu
def test_pairwise_sqdist_uses_every_partial_slot():
    n = (1 << 21) + 5
    g = torch.Generator().manual_seed(4)
    rows = [torch.randn(n, generator=g).cuda() for _ in range(4)]
    d1 = check_sqdist(rows)
    d2 = F.pairwise_sqdist_rows(rows)
    assert torch.equal(d1.view(torch.int64), d2.view(torch.int64))


@requires_gpu
@pytest.mark.parametrize("k", [8, 33])
def test_pairwise_sqdist_small_updates_on_large_weights(k):
    """base ~ 1.0 plus 1e-3 updates: ||a||^2 + ||b||^2 - 2ab cancels here."""
    n = 300001
    g = torch.Generator().manual_seed(9)
    base = 1.0 + 0.1 * torch.randn(n, generator=g)
    rows = [(base + 1e-3 * torch.randn(n, generator=g)).cuda() for _ in range(k)]
    check_sqdist(rows)


@requires_gpu
@pytest.mark.parametrize("bad", [NAN, INF])
def test_pairwise_sqdist_non_finite_row_stays_in_its_row_and_column(bad):
    k, n = 5, 1000
    g = torch.Generator().manual_seed(13)
    rows = [torch.randn(n, generator=g) for _ in range(k)]
    rows[2][417] = bad
    rows = [r.cuda() for r in rows]
    d = F.pairwise_sqdist_rows(rows)
    want = sqdist_oracle(rows)
    assert torch.equal(torch.nan_to_num(d, nan=-1.0), torch.nan_to_num(d.t(), nan=-1.0))
    others = [0, 1, 3, 4]
    sub, sub_want = d[others][:, others], want[others][:, others]
    assert torch.isfinite(sub).all()
    assert ((sub - sub_want).abs() <= 1e-5 * sub_want).all()
    if bad != bad:
        assert torch.isnan(d[2]).all() and torch.isnan(d[:, 2]).all()
    else:
        assert (d[2, others] == INF).all() and (d[others, 2] == INF).all()
        assert torch.isnan(d[2, 2])  # inf - inf, as in the oracle
        assert torch.isnan(want[2, 2])


@requires_gpu
def test_pairwise_sqdist_misaligned_views_and_two_runs():
    g = torch.Generator().manual_seed(17)
    bufs = [torch.randn(1001, generator=g).cuda() for _ in range(17)]
    rows = [b[1:] for b in bufs]
    assert all(r.data_ptr() % 16 == 4 for r in rows)
    d1 = check_sqdist(rows)
    d2 = F.pairwise_sqdist_rows(rows)
    assert torch.equal(d1.view(torch.int64), d2.view(torch.int64))
    # same values from aligned copies
    d3 = F.pairwise_sqdist_rows([r.clone() for r in rows])
    assert torch.equal(d1, d3)


# ---- 9. strategies on CUDA tensors -----------------------------------------
def to_cuda(res):
    out = []
    for proxy, r in res:
        p = type(r.parameters)([t.cuda() for t in r.parameters.tensors], dict(r.parameters.meta))
        out.append((proxy, type(r)(p, r.num_examples, dict(r.metrics))))
    return out


@requires_gpu
@pytest.mark.parametrize("attack", list(ATTACKS))
@pytest.mark.parametrize("f", [1, 2])
def test_median_and_trimmed_on_device_match_cpu(f, attack):
    assert F.HAS_EXT
    honest, rows = attacked_rows(f, attack)
    res = fit_results(rows)
    gres = to_cuda(res)
    med_cpu, _ = FedMedian().aggregate_fit(1, res, [])
    med_gpu, _ = FedMedian().aggregate_fit(1, gres, [])
    assert med_gpu.tensors[0].is_cuda
    assert torch.equal(med_gpu.tensors[0].cpu(), med_cpu.tensors[0])
    assert within_honest_range(med_gpu.tensors[0].cpu(), honest).all()
    beta = 0.2 if f == 1 else 0.4
    tr_cpu, _ = FedTrimmedAvg(beta=beta).aggregate_fit(1, res, [])
    tr_gpu, _ = FedTrimmedAvg(beta=beta).aggregate_fit(1, gres, [])
    got = tr_gpu.tensors[0].cpu()
    assert within_honest_range(got, honest).all()
    bound = 5 * EPS * torch.stack(honest).abs().max(dim=0).values
    assert ((got - tr_cpu.tensors[0]).abs() <= bound).all()
    avg, _ = BasicFedAvg().aggregate_fit(1, gres, [])
    assert not within_honest_range(avg.tensors[0].cpu(), honest).all()


@requires_gpu
def test_krum_on_device_matches_cpu():
    assert F.HAS_EXT
    honest, rows = krum_rows()
    res = fit_results(rows)
    gres = to_cuda(res)
    cpu, cpu_metrics = Krum(num_malicious_clients=2).aggregate_fit(1, res, [])
    gpu, gpu_metrics = Krum(num_malicious_clients=2).aggregate_fit(1, gres, [])
    assert gpu.tensors[0].is_cuda
    assert torch.equal(gpu.tensors[0].cpu(), cpu.tensors[0])
    assert gpu_metrics["krum_selected"] == cpu_metrics["krum_selected"]
    assert sum(torch.equal(gpu.tensors[0].cpu(), h) for h in honest) == 1
    _, cpu_metrics = Krum(num_malicious_clients=2, num_clients_to_keep=3).aggregate_fit(1, res, [])
    multi, gpu_metrics = Krum(num_malicious_clients=2, num_clients_to_keep=3).aggregate_fit(1, gres, [])
    chosen = [int(c) for c in gpu_metrics["krum_selected"].split(",")]
    assert gpu_metrics["krum_selected"] == cpu_metrics["krum_selected"]
    assert len(chosen) == 3 and all(c < 5 for c in chosen)
    mean = torch.stack([rows[c] for c in chosen]).double().mean(dim=0)
    assert ((multi.tensors[0].cpu().double() - mean).abs() <= 4 * EPS * mean.abs().clamp_min(1.0)).all()
