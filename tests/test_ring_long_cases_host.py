"""tests/ring_long_cases.py's planted conditions, from the references alone (CPU):
the pair counts, the tiles' block counts {3, 4, 5, 9, 32, 33, 66}, P1
(heterogeneous bounds in one tile) and P2 (ties at an exchanged bound) on the
i8_cases / mx4_cases / mx6_cases restatements and on the metric workload's
float64 distances, the tags, and the metric references' share of lists that
test_gpu_metric._check's strict-id rule exempts."""
import numpy as np
import pytest

import ring_long_cases as L
from test_gpu_metric import _err


def test_shape_pair_counts_and_block_counts():
    f = L.fixture()
    L.check_shape(f["classes"])
    assert f["classes"].shape == (L.NQ, L.R) and L.N == 7861
    assert L.tile_blocks() == [3, 4, 5, 9, 32, 33, 66, 66, 33]
    # one-row tails on buckets 0 and 5, a 16-row tail on bucket 6's last chunk
    assert L.SIZES[0] % 32 == 1 and L.SIZES[5] % 32 == 1 and (L.SIZES[6] - 2 * L.CHUNK) % 32 == 16
    # P1's rows lie before block 31 of chunk 0, most of P2's copies past block 31 of their chunks
    assert ((f["plant"] - L.B6) < 992).all() and np.unique(f["plant"]).size == 16 * L.GROUPS
    assert not np.isin(f["plant"], L.TIE_POS).any()
    assert sorted({c for c, _ in L.TIE_AT}) == [0, 1, 2]
    assert f["even"].size == 128 and f["odd"].size == 128 and L.QTIE % 2 == 0


@pytest.mark.parametrize("storage", ["i8", "mx4", "mx6"])
def test_planted_conditions_on_the_restatement(storage):
    dist = L.restated(storage)
    assert dist.shape == (L.NQ, L.N) and dist.dtype == (np.float32 if storage == "i8" else np.float64)
    gaps = L.check_planted(dist, 100 * L.TOL)
    print(storage, "odd k-th best minus even k-th best:", gaps)


def test_tags():
    L.check_tags()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_metric_workload_conditions_and_strict_id_share(metric):
    from li.index import refine_eps
    assert refine_eps(768, True) > 0
    f = L.fixture()
    D, rd, rp = L.metric_reference(metric)
    qn = np.linalg.norm(f["qm"].astype(np.float64), axis=1)
    yn = np.linalg.norm(f["xm"].astype(np.float64), axis=1)
    assert 0.45 * 27.7 < yn.min() and yn.max() < 4.0 * 1.1 * 27.7 and qn.max() < 2.0 * 2.0 * 1.1 * 27.7
    bound = 2.0 * _err(768, metric, True, qn, yn.max())          # _check's bound of a list
    L.check_planted(D, 100 * bound.max(), ks=(1, 10))
    for k in (1, 10):
        share = L.strict_id_share(metric, k, bound)
        print(metric, k, f"lists with a gap inside the bound: {share:.1%}")
        assert share <= 0.10 and abs(share - L.METRIC_SHARES[metric, k]) < 0.002
    # the metric's lists are not the cosine's
    _, _, cp = L.metric_reference("cosine")
    full = rp[..., 9] >= 0
    differ = np.any(np.sort(rp[..., :10], -1) != np.sort(cp[..., :10], -1), axis=-1)
    assert full.sum() == 342 and differ[full].mean() >= 0.90
