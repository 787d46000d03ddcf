"""The few-query scan (bucket_topk(few=True), scan_few_kernel) against the
oracle on float64 copies of the inputs, by test_gpu_scan_widths.py's rules:
O.bucket_lists k + 1 deep, O.compare_lists with the float32 defaults, and the
strict-id rule with bound 2 * refine_eps(d_pad, True), whose exempt share
(<= 10 %) is asserted from the oracle alone before a GPU list is read.

Each axis at its extremes against the centre (d 740, nq 11, k 10, few_rows 96):
d 8 (d_pad 32: one short segment), 96 and 800 (a short last segment), 992 (the
widest query image); nq 1 (one live column), 85 (255 pairs: several groups a
bucket); k 1 and 16 (both list lengths); few_rows 32 (many slices), 96 (slice
and bucket tails), None (the call's choice).  Query 0 probes nothing (-1) in
round 1 and an empty bucket (C) in round 2.  SEEDS: test_gpu_scan_widths.py's,
but 740 -> 1641 (1640 exempts 15.2 % of the rows at nq 11, k 16; 1641 9.1 %)."""
import functools

import numpy as np
import pytest
import torch

import lmi_oracle as O
import workloads
from li.index import DeviceIndex, DeviceRouter, Searcher, bucket_topk, refine_eps, scan_family

pytestmark = pytest.mark.gpu

N, C, R = 3000, 8, 3
SEEDS = {8: 908, 96: 1996, 740: 1641, 800: 7700, 992: 3892}
CENTRE = (740, 11, 10, 96)
CASES = [CENTRE] + [(d, 11, 10, 96) for d in (8, 96, 800, 992)] + [(740, nq, 10, 96) for nq in (1, 85)] + \
        [(740, 11, k, 96) for k in (1, 16)] + [(740, 11, 10, fr) for fr in (32, None)] + \
        [(992, 85, 16, 32), (8, 1, 1, None), (96, 85, 16, None)]
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731


@functools.lru_cache(maxsize=None)
def _workload(d, nq):
    w = workloads.clustered(n=N, d=d, nq=nq, C=C, seed=SEEDS[d], label_mode="skewed")
    classes = np.ascontiguousarray(O.rank_classes(O.mlp_forward(w["qn"], w["layers"]))[:, :R])
    classes[0, 1], classes[0, 2] = -1, C  # no probe; the empty bucket of the C + 1
    ref = O.bucket_lists(w["labels"], w["x"].astype(np.float64), w["q"].astype(np.float64), classes, R, 17, C + 1)
    return w, classes, ref


@functools.lru_cache(maxsize=None)
def _index(d, nq):
    w = _workload(d, nq)[0]
    return DeviceIndex(w["x"], w["labels"], C + 1, storage="f16", chunk_rows=256, device="cuda")


def exempt_share(d, nq, k):
    """The rows the strict-id rule exempts (an oracle gap <= 2 eps) and the clear ones."""
    ref_d = _workload(d, nq)[2][0][..., :k + 1]
    with np.errstate(invalid="ignore"):
        gaps = np.diff(ref_d.reshape(-1, k + 1), axis=-1)
    gaps[np.isnan(gaps)] = np.inf
    clear = np.all(gaps > 2 * refine_eps((d + 31) // 32 * 32, True), axis=-1)
    return 1.0 - clear.mean(), clear


@pytest.mark.parametrize("d,nq,k,few_rows", CASES)
def test_few_lists_match_oracle(d, nq, k, few_rows):
    w, classes, (ref_d, ref_p) = _workload(d, nq)
    exempt, clear = exempt_share(d, nq, k)
    assert exempt <= 0.10, f"the strict-id rule exempts {exempt:.1%} of the rows"
    ix = _index(d, nq)
    assert scan_family(ix, k, few=True) == "few"
    got_d, got_p, st = bucket_topk(ix, T(w["q"]), T(classes.astype(np.int32)), k, few=True, few_rows=few_rows)
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    got_d, got_p = got_d.cpu().numpy(), got_p.cpu().numpy()
    assert got_d.dtype == np.float32 and got_d.shape == (nq, R, k)
    assert np.all(np.isinf(got_d[0, 1:])) and np.all(got_p[0, 1:] == -1)
    stats = {}
    bad = O.compare_lists(ref_d[..., :k], ref_p[..., :k], got_d, got_p, stats=stats)
    print(f"[few] d{d} nq{nq} k{k} rows{few_rows}: exempt {exempt:.2%}, tie rows {stats['tie_rows']}, mismatched {bad}")
    assert bad == 0
    same = np.all(got_p.reshape(-1, k) == ref_p.reshape(-1, 17)[:, :k], axis=-1)
    assert np.all(same[clear]), f"ids differ in {int((~same & clear).sum())} clear rows"


@pytest.mark.parametrize("d", [96, 740])
def test_search_few_matches_oracle(d):
    w = workloads.clustered(n=N, d=d, nq=5, C=C, seed=SEEDS[d], label_mode="skewed")
    s = Searcher(DeviceIndex(w["x"], w["labels"], C, chunk_rows=256, device="cuda"),
                 DeviceRouter(w["layers"], device="cuda"))
    dists, anns = s.search(T(w["qn"]), T(w["q"]), R, k=10, few=True, semantics="exact")
    classes = O.rank_classes(O.mlp_forward(w["qn"], w["layers"]))
    ref_d, ref_a = O.search_exact(w["labels"], np.arange(1, N + 1), w["x"], w["q"], classes, C, R, k=10)
    assert O.compare_lists(ref_d, ref_a, dists, anns) == 0
