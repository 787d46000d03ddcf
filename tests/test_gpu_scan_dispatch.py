"""The branches of the scan's launch choice (csrc/lmi_scan.hip, pick_launch) that
no other GPU test reaches, each against the oracle: the 8-wave ring's plain
15-entry lists (11 <= k <= 15 through lmi_bucket_topk), the three general-
kernel variants of the lower-bound passes (k > 16 off the fp16 rings: fp32
storage, fp32 queries on an fp16 corpus, and an fp16 corpus with fp16 queries
under LMI_SCAN_V1), and the general kernel's plain fp16-arithmetic and
fp16 x fp32 16-entry variants."""
import functools
import os

import numpy as np
import pytest
import torch

import lmi_oracle as O
import workloads
from li import _lib
from li.index import DeviceIndex, bucket_topk

pytestmark = pytest.mark.gpu

R = 4


@functools.lru_cache(maxsize=None)
def _workload():
    w = workloads.clustered(n=6000, nq=257, C=16)
    classes = O.rank_classes(O.mlp_forward(w["qn"], w["layers"]))[:, :R]
    return w, classes


@functools.lru_cache(maxsize=None)
def _reference(k):
    w, classes = _workload()
    return O.bucket_lists(w["labels"], w["x"], w["q"], classes, R, k, w["C"])


@pytest.mark.parametrize("storage,k,qmode,env", [
    ("f16", 12, _lib.LMI_Q_F16, None),            # 8-wave ring, 15-entry lists, plain
    ("f32", 40, _lib.LMI_Q_F32, None),            # lower bounds, general kernel, fp32 corpus
    ("f16", 40, _lib.LMI_Q_F32, None),            # lower bounds, general kernel, fp16 corpus x fp32 queries
    ("f16", 40, _lib.LMI_Q_F16, "LMI_SCAN_V1"),   # lower bounds, general kernel, fp16 arithmetic
    ("f16", 10, _lib.LMI_Q_F16, "LMI_SCAN_V1"),   # general kernel, fp16 arithmetic, 10-entry lists
    ("f16", 16, _lib.LMI_Q_F16, "LMI_SCAN_V1"),   #   and 16-entry lists
    ("f16", 16, _lib.LMI_Q_F32, None),            # general kernel, fp16 corpus x fp32 queries, 16 entries
], ids=["ring8-kl15", "lo-f32", "lo-f16-qf32", "lo-f16-v1", "general-f16-kl10", "general-f16-kl16",
        "general-f16-qf32-kl16"])
def test_launch_branch_matches_oracle(storage, k, qmode, env):
    w, classes = _workload()
    ix = DeviceIndex(w["x"], w["labels"], w["C"], storage=storage, chunk_rows=512)
    q = torch.from_numpy(w["q"]).cuda()
    ct = torch.from_numpy(classes.astype(np.int32)).cuda()
    if env:
        os.environ[env] = "1"
    _lib.load().lmi_config_reload()
    try:
        d, pos, st = bucket_topk(ix, q, ct, k, qmode=qmode)
        torch.cuda.synchronize()
    finally:
        if env:
            os.environ.pop(env, None)
        _lib.load().lmi_config_reload()
    assert int(st.item()) == 0
    ref_d, ref_p = _reference(k)
    assert O.compare_lists(ref_d, ref_p, d.cpu().numpy(), pos.cpu().numpy()) == 0
